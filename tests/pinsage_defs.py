"""The executable definition of the PinSAGE neighbourhoods (ops.walk_visit_topk / host_walk_visit_topk, include/pgl_amd.h:
pglamd_walk_visit_topk) in numpy, from WALKS somebody else produced, and the graphs the host and GPU tests share.

visit_topk(paths, lengths, seeds, R, T): rows s * R .. s * R + R - 1 of (paths, lengths) are the R walks of seed s (what
ops.random_walk returns for starts = repeat(seeds, R)).  The visits of seed s are positions 1 .. len - 1 of those rows without
the entries equal to seeds[s]; they are counted per distinct node, ordered by (count descending, node id ascending) and cut at
T.  -> nbr int64 [S, T] (padding -1), cnt int32 [S, T] (padding 0), num int32 [S] = min(T, distinct)."""
import numpy as np


def visit_topk(paths, lengths, seeds, R, T, full=False):
    """full=True adds (distinct [S] = distinct visited nodes before the cut, cut_tie [S] = the entries at positions T - 1 and T of
    the full order have equal counts: the id tie-break decides who is kept)."""
    paths, lengths, seeds = np.asarray(paths), np.asarray(lengths), np.asarray(seeds, np.int64).reshape(-1)
    S = len(seeds)
    assert paths.shape[0] == S * R and lengths.shape == (S * R,)
    nbr = np.full((S, T), -1, np.int64)
    cnt = np.zeros((S, T), np.int32)
    num = np.zeros(S, np.int32)
    distinct = np.zeros(S, np.int64)
    cut_tie = np.zeros(S, bool)
    for s in range(S):
        rows = range(s * R, (s + 1) * R)
        visits = np.concatenate([paths[w, 1:lengths[w]] for w in rows]) if R else np.zeros(0, np.int64)
        visits = visits[visits != seeds[s]]
        assert (visits >= 0).all()
        ids, c = np.unique(visits, return_counts=True)
        order = np.lexsort((ids, -c))                    # count descending, then id ascending
        ids, c = ids[order], c[order]
        n = min(T, len(ids))
        nbr[s, :n], cnt[s, :n], num[s] = ids[:n], c[:n], n
        distinct[s] = len(ids)
        cut_tie[s] = len(ids) > T and c[T - 1] == c[T]
    return (nbr, cnt, num, distinct, cut_tie) if full else (nbr, cnt, num)


# ---- hand-worked graphs ------------------------------------------------------------------------------------------------------
def csr_of(edges, n):
    """(indptr int64 [n + 1], col int32 [E]) of the successor index, rows ascending by dst."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    order = np.lexsort((e[:, 1], e[:, 0]))
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=n), out=indptr[1:])
    return indptr, e[order, 1].astype(np.int32)


# ---- the shared RMAT graph ---------------------------------------------------------------------------------------------------
N = 1024
EMPTY = 5            # a node without successors
ZERO_ROW = 9         # a node whose out-edges all have weight zero: a dead end of the weighted walks only
LOOP = 7             # a node with a self-loop: its own visits are dropped
NUM_SEEDS = 2048


def rmat_graph():
    """-> (edges int64 [E, 2], weight float32 [E], hub): RMAT scale 10 with the out-edges of a few nodes removed, a self-loop at
    LOOP, weights with about a fifth zeros and the all-zero row ZERO_ROW; hub = the node with the most successors."""
    from pgl_amd.utils.rmat import rmat_edges
    e = rmat_edges(10, 12000, seed=11).numpy()
    gone = np.isin(e[:, 0], [EMPTY, 33, 34, 35, 500, 501])
    e = np.concatenate([e[~gone], [[LOOP, LOOP], [LOOP, 3], [ZERO_ROW, 1], [ZERO_ROW, 2]]]).astype(np.int64)
    rng = np.random.default_rng(12)
    w = rng.random(len(e)).astype(np.float32) + np.float32(0.01)
    w[rng.random(len(e)) < 0.2] = 0.0
    w[e[:, 0] == ZERO_ROW] = 0.0
    hub = int(np.argmax(np.bincount(e[:, 0], minlength=N)))
    assert hub not in (EMPTY, ZERO_ROW, LOOP)
    return e, w, hub


def rmat_seeds(hub):
    """NUM_SEEDS seeds: the special ones first (so every prefix of 63 or more holds them), repeats included."""
    head = [hub, EMPTY, hub, ZERO_ROW, LOOP, EMPTY, 33, hub]
    rest = np.random.default_rng(13).integers(0, N, NUM_SEEDS - len(head))
    return np.concatenate([head, rest]).astype(np.int64)
