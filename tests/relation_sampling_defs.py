"""Shared by tests/test_relation_sampling_host.py and tests/test_relation_sampling_gpu.py: the relation-wise neighbour sampler and
its relabel restated in numpy from their documented definition (no project imports; the single-relation sampler and relabel come from
tests/sampling_defs.py), and the fixture both files sample.

The sampler: relation r of R samples every seed with fan-out f[r] and seed relation_seed(seed, r) = mix64(uint64(seed) ^
mix64(uint64(r))) exactly as the single-relation sampler does (f[r] == 0: nothing); the output is relation-major, then seed position,
then draw order; dst holds the seed POSITION of every slot; eids are relation-local.
The relabel: reindex_graph's contract over the concatenation of the relations' neighbours."""
import numpy as np

import sampling_defs as S

U64 = np.uint64


def relation_seed(seed, r):
    """-> Python int in [0, 2^64)."""
    return int(S.mix64(U64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ S.mix64(U64(int(r)))))


def sample_relations_restated(csrs, nodes, fanouts, seed):
    """csrs: [(indptr, col, eid)] per relation (sampling_defs.csr_by_dst) -> (neighbors, dst, count [R, n], edge_split tuple of
    R + 1 ints, eids)."""
    nodes = np.asarray(nodes, np.int64).reshape(-1)
    n, pos = len(nodes), np.arange(len(nodes), dtype=np.int64)
    nbr, dst, eids, count, split = [], [], [], [], [0]
    for r, ((indptr, col, eid), f) in enumerate(zip(csrs, fanouts)):
        if int(f) == 0:
            a, c, e = np.zeros(0, np.int64), np.zeros(n, np.int64), np.zeros(0, np.int64)
        else:
            a, c, e = S.sample_restated(indptr, col, eid, nodes, int(f), relation_seed(seed, r))
        nbr.append(a); eids.append(e); count.append(c); dst.append(np.repeat(pos, c))
        split.append(split[-1] + len(a))
    cat = lambda xs: np.concatenate(xs).astype(np.int64)
    return cat(nbr), cat(dst), np.stack(count).astype(np.int64).reshape(len(csrs), n), tuple(split), cat(eids)


def reindex_heter_restated(nodes, neighbors, count):
    """neighbors / count: per-relation lists -> (src, dst, out_nodes): sampling_defs.reindex_restated over the concatenation, the
    destinations relation by relation."""
    nodes = np.asarray(nodes, np.int64).reshape(-1)
    flat = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in neighbors])
    src, _, out_nodes = S.reindex_restated(nodes, flat, np.zeros(len(nodes), np.int64))
    pos = np.arange(len(nodes), dtype=np.int64)
    dst = np.concatenate([np.repeat(pos, np.asarray(c, np.int64).reshape(-1)) for c in count])
    return src, dst, out_nodes


# ---- the fixture: R = 4 relations over N = 600 nodes ---------------------------------------------------------------------------
N = 600
EDGE_TYPES = ["cites", "writes", "empty", "topic"]
FANOUTS = [5, -1, 0, 64]
HUB = 77                     # in-degree 300 under every relation that has edges


def _relation_edges(rng, degrees):
    """Edges whose node v has in-degree degrees[v], the sources drawn anew per edge (multi-edges and self-loops may occur), shuffled."""
    dst = np.repeat(np.arange(N, dtype=np.int64), degrees)
    src = rng.integers(0, N, len(dst)).astype(np.int64)
    p = rng.permutation(len(dst))
    return np.stack([src[p], dst[p]], 1)


def fixture_edges():
    """{edge type: int64 [E, 2]}: rows of degree 0, k, k + 1 for every fan-out k in use (5 and 64), 64, 65 and one row of 300 per
    non-empty relation; "empty" has no edges.  The in-neighbours of node 3 under "cites" and of node 6 under "writes" include the
    node itself and node 5, both seeds of fixture_seeds."""
    rng = np.random.default_rng(20221019)
    out = {}
    for t, et in enumerate(EDGE_TYPES):
        if et == "empty":
            out[et] = np.zeros((0, 2), np.int64)
            continue
        deg = rng.choice(np.array([0, 1, 4, 5, 6, 7, 20, 63, 64, 65, 66]), N).astype(np.int64)
        deg[:12] = [0, 5, 6, 64, 65, 4, 66, 1, 63, 0, 7, 20]
        deg[HUB] = 300
        e = _relation_edges(rng, np.roll(deg, 3 * t))
        out[et] = e
    for et, v in (("cites", 3), ("writes", 6)):              # (rows of 64 in-edges; "writes" is copied whole, so 6 and 5 ARE sampled)
        rows = np.flatnonzero(out[et][:, 1] == v)
        out[et][rows[0], 0], out[et][rows[1], 0] = v, 5
    return out


def fixture_seeds(n=2500):
    """Seeds with repeats, a seed that is also a neighbour (3 and 5 under "cites"), the hub and the small-degree rows; unsorted."""
    rng = np.random.default_rng(7)
    head = np.array([3, 5, HUB, 3, 0, 1, 2, 4, 6, 7, 8, 9, 10, 11, HUB, 599, 0], np.int64)
    return np.concatenate([head, rng.integers(0, N, max(n - len(head), 0)).astype(np.int64)])[:max(n, 0)]


def fixture_csrs(edges=None):
    edges = fixture_edges() if edges is None else edges
    return [S.csr_by_dst(edges[et], N) for et in EDGE_TYPES]
