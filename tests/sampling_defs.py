"""Shared by tests/test_sampling_defs.py and tests/test_sampling_gpu.py: the neighbour sampler and the relabel of
pgl_amd/csrc/sampling.hip restated in numpy from their documented definition (no project imports), and the exact law a
sampler without replacement has to obey -- every k-subset of a row equally likely -- as a chi-square check.

The draw: for a seed node v of in-degree deg > k >= 0, Floyd's algorithm over the row's POSITIONS 0 .. deg - 1; draw number
c = 0 .. k - 1 has j = deg - k + c, r = mix64(seed ^ mix64(v * 0x100000001B3 + c)) (all in uint64), t = r % (j + 1); a t
that an earlier draw of this node already produced is replaced by j; the outputs are the row's entries at the chosen
positions IN DRAW ORDER.  k < 0 or deg <= k copies the row.
The relabel: every position of `nodes` keeps its own id (repeats included), new neighbour ids follow in order of first
appearance, a neighbour that equals a seed maps to that seed's FIRST position."""
from itertools import combinations

import numpy as np

U64 = np.uint64
KEY_MUL = 0x100000001B3


def mix64(z):
    """splitmix64's finaliser on a uint64 array (or scalar), wrapping modulo 2^64 as the device does."""
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def sample_restated(indptr, col, eid, nodes, k, seed):
    """ops.sample_neighbors over the CSR (indptr, col, eid) -> (neighbors int64 [sum count], count int64 [len(nodes)],
    eids int64 [sum count]).  eid=None: the edge id of a position is the position itself.  Vectorised over the nodes; the
    only Python loop is over the k draws."""
    indptr = np.asarray(indptr, np.int64)
    nodes = np.asarray(nodes, np.int64)
    k, n = int(k), len(nodes)
    b = indptr[nodes]
    deg = indptr[nodes + 1] - b
    floyd = np.zeros(n, bool) if k < 0 else deg > k
    count = np.where(floyd, k, deg).astype(np.int64)
    offsets = np.cumsum(count) - count
    total = int(count.sum())
    # copy-all first (positions b .. b + deg - 1 in row order); the Floyd rows are overwritten below
    pos = np.repeat(b - offsets, count) + np.arange(total, dtype=np.int64)
    f = np.flatnonzero(floyd)
    if len(f) and k > 0:
        v, d = nodes[f].astype(U64), deg[f]
        chosen = np.empty((len(f), k), np.int64)
        with np.errstate(over="ignore"):
            base = v * U64(KEY_MUL)
        for c in range(k):
            j = d - k + c
            with np.errstate(over="ignore"):
                r = mix64(U64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ mix64(base + U64(c)))
            t = (r % (j + 1).astype(U64)).astype(np.int64)
            dup = (chosen[:, :c] == t[:, None]).any(1)
            chosen[:, c] = np.where(dup, j, t)
        pos[(offsets[f][:, None] + np.arange(k, dtype=np.int64)[None, :]).ravel()] = (b[f][:, None] + chosen).ravel()
    neighbors = np.asarray(col)[pos].astype(np.int64)
    eids = pos if eid is None else np.asarray(eid)[pos].astype(np.int64)
    return neighbors, count, eids


def reindex_restated(nodes, neighbors, count):
    """ops.reindex_graph -> (src int64 [m], dst int64 [m], out_nodes): out_nodes = nodes as given (repeats kept), then the
    neighbour ids that are no seed in order of first appearance; src[e] = index in out_nodes of neighbors[e], the FIRST
    position for an id that `nodes` repeats; dst = repeat(arange(n), count)."""
    nodes, neighbors = np.asarray(nodes, np.int64), np.asarray(neighbors, np.int64)
    n = len(nodes)
    keys = np.concatenate([nodes, neighbors])
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)      # first: lowest position of each id
    new = np.sort(first[first >= n])                                                 # new ids by first appearance
    ident = np.where(first < n, first, n + np.searchsorted(new, first))
    src = ident[np.ravel(inverse)[n:]].astype(np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), np.asarray(count, np.int64))
    return src, dst, np.concatenate([nodes, keys[new]])


def subset_law_chi2(picks, deg, k):
    """Pearson chi-square of the rows of `picks` (int [W, k]: the k positions in [0, deg) one node drew) against the uniform
    law over all C(deg, k) subsets -> (statistic, degrees of freedom).  A row that is no k-subset of range(deg) (a position
    out of range or drawn twice) has probability zero: AssertionError at once.  No cell is pooled or left out."""
    picks = np.asarray(picks, np.int64)
    assert picks.ndim == 2 and picks.shape[1] == k and 0 < k <= deg < 31, (picks.shape, deg, k)
    bad = np.flatnonzero(((picks < 0) | (picks >= deg)).any(1))
    assert not len(bad), "positions outside [0, %d): rows %s = %s" % (deg, bad[:5], picks[bad[:5]].tolist())
    masks = np.bitwise_or.reduce(np.int64(1) << picks, axis=1)
    cells = np.array([sum(1 << p for p in s) for s in combinations(range(deg), k)], np.int64)
    seen = np.bincount(masks, minlength=1 << deg)
    obs = seen[cells].astype(np.float64)
    if obs.sum() != len(picks):                                                      # a mask with fewer than k bits
        bad = np.flatnonzero(~np.isin(masks, cells))
        raise AssertionError("rows that are no %d-subset (a position drawn twice): rows %s = %s" % (k, bad[:5], picks[bad[:5]].tolist()))
    exp = len(picks) / float(len(cells))
    return float(((obs - exp) ** 2 / exp).sum()), len(cells) - 1


# (deg, k, nodes): every cell's expected count is >= 5 700
SUBSET_CASES = [(5, 2, 200000), (6, 3, 200000), (7, 6, 200000), (9, 1, 200000), (8, 4, 400000)]
FIRST_NODE = 1000            # the law graphs' sampled nodes are FIRST_NODE .. FIRST_NODE + W - 1 (nodes below have no in-edges)


def assert_subset_law(picks, deg, k, what):
    """The project's acceptance line for a law (walk_defs.assert_law): p > 1e-4."""
    from scipy.stats import chi2
    stat, dof = subset_law_chi2(picks, deg, k)
    pv = float(chi2.sf(stat, dof))
    print("subset law %s: deg %d k %d cells %d chi2 %.2f p %.4f" % (what, deg, k, dof + 1, stat, pv))
    assert pv > 1e-4, (what, deg, k, stat, dof, pv)


def law_graph(deg, W, rng=None):
    """Edges of a graph whose nodes FIRST_NODE .. FIRST_NODE + W - 1 each have in-degree `deg` from `deg` distinct sources,
    (shuffled when rng is given) -> (edges int64 [W * deg, 2], num_nodes, pos_of_edge int64 [W * deg]: the position of every
    edge inside its destination's row of the dst-sorted stable CSR)."""
    dst = np.repeat(np.arange(FIRST_NODE, FIRST_NODE + W, dtype=np.int64), deg)
    src = (np.tile(np.arange(deg, dtype=np.int64), W) * 7 + np.repeat(np.arange(W, dtype=np.int64), deg)) % (FIRST_NODE + W)
    if rng is not None:
        p = rng.permutation(len(dst))
        dst, src = dst[p], src[p]
    order = np.argsort(dst, kind="stable")
    pos = np.empty(len(dst), np.int64)
    pos[order] = np.arange(len(dst), dtype=np.int64) % deg
    return np.stack([src, dst], 1), FIRST_NODE + W, pos


def csr_by_dst(edges, num_nodes):
    """The dst-sorted stable index ops.CSR holds: (indptr int64 [N + 1], col = src by position, eid = edge id by position)."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    order = np.argsort(edges[:, 1], kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(edges[:, 1], minlength=num_nodes))]).astype(np.int64)
    return indptr, edges[order, 0], order.astype(np.int64)
