"""Shared by tests/test_weighted_host.py and tests/test_weighted_gpu.py (definitions only, no tests, no project imports): the
integer weight table, the weighted walk step, weighted neighbour sampling without replacement and draws from a single-row
table, restated in numpy from their documented definitions (include/pgl_amd.h), the exact laws they have to obey, and the graph
the table tests run on.

Table: row v with positions b .. b+deg-1 and maximum weight m: q[j] = 0 if w[j] == 0 or m == 0, else
max(1, floor(float64(w[j]) / float64(m) * 2^32)); cum[j] = q[b] + .. + q[j] (int64, within the row); npos[v] = #{q > 0}.
Walk step at cur (row b .. b+deg-1 of the sorted successor index, T = cum[b+deg-1]): dead end when deg == 0 or T == 0; else
r = scale64(draw(key, t+1, 0), T), next = col[smallest j with cum[j] > r].
Sampler: count = npos when k < 0 or npos <= k (the positive positions in row order), else k draws of successive sampling:
R_c = T - q of the chosen, r = scale64(mix64(seed ^ mix64(v * 0x100000001B3 + c)), R_c), pick = the smallest not-yet-chosen j
whose running sum of q over the not-yet-chosen positions <= j exceeds r; output in draw order.
sample_from_table: draw i = smallest j with cum[j] > scale64(mix64(seed ^ mix64(i)), cum[-1])."""
import numpy as np

from sampling_defs import KEY_MUL, U64, mix64

M64 = (1 << 64) - 1


def mix64_int(z):
    """splitmix64's finaliser on a Python int (walk_defs.skip_gram_restated's)."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def scale64_int(r, n):
    """floor(r * n / 2^64) on Python ints."""
    return (r * n) >> 64


def scale64(r, n):
    """floor(r * n / 2^64) on uint64 arrays: the high word of the 128-bit product, from 32-bit halves (walk_core.hpp scale64)."""
    r, n = np.asarray(r, U64), np.asarray(n, U64)
    lo, s = U64(0xFFFFFFFF), U64(32)
    r0, r1, n0, n1 = r & lo, r >> s, n & lo, n >> s
    with np.errstate(over="ignore"):
        t = r1 * n0 + ((r0 * n0) >> s)
        u = (t & lo) + r0 * n1
        return r1 * n1 + (t >> s) + (u >> s)


# ---- the table ---------------------------------------------------------------------------------------------------------------
def quantise(indptr, weight, eid=None):
    """q int64 [E] of every position (weight read through eid when given)."""
    indptr = np.asarray(indptr, np.int64)
    n = len(indptr) - 1
    w = np.asarray(weight)
    w = (w if eid is None else w[np.asarray(eid, np.int64)]).astype(np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    m = np.zeros(n, np.float64)
    np.maximum.at(m, rows, w)
    mr = m[rows]
    zero = (w == 0) | (mr == 0)
    with np.errstate(under="ignore"):
        q = np.floor(w / np.where(zero, 1.0, mr) * 2.0 ** 32)
    return np.where(zero, 0, np.maximum(1, q)).astype(np.int64), rows


def table_restated(indptr, weight, eid=None):
    """-> (cum int64 [E], npos int64 [N])."""
    indptr = np.asarray(indptr, np.int64)
    n = len(indptr) - 1
    q, rows = quantise(indptr, weight, eid)
    cs = np.cumsum(q, dtype=np.int64)
    excl = cs - q
    cum = cs - excl[indptr[rows]] if len(q) else cs
    return cum, np.bincount(rows[q > 0], minlength=n).astype(np.int64)


def q_of(indptr, cum):
    """q back from a table: the first difference of cum inside every row."""
    indptr, cum = np.asarray(indptr, np.int64), np.asarray(cum, np.int64)
    q = np.diff(cum, prepend=0)
    starts = indptr[:-1][np.diff(indptr) > 0]
    q[starts] = cum[starts]
    return q


def table_graph(seed=0):
    """The graph of the table tests -> (indptr int64 [N+1], weight float64 [E], every value exactly representable in fp32).
    Rows 0 .. 6: empty; one edge; all zeros; zeros between positives; 1e-30 .. 1e30; fp32 subnormals; the maximum several times.
    Then ~1500 short random rows (about 10 k edges, so the hub starts in the middle of a 2048-entry scan piece), one hub row of
    70 000 edges (10 % zeros) and a tail of short rows."""
    rng = np.random.default_rng(seed)
    f4 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rows = [f4([]), f4([3.5]), f4([0, 0, 0, 0, 0]), f4([0, 2, 0, 0, 5, 1, 0]), f4([1e-30, 1.0, 1e30, 1e-10, 1e10, 1e-30]),
            f4([1e-45, 3e-45, 1e-40, 5e-39, 1e-45, 0]), f4([7, 7, 1, 7, 0.5, 7])]
    for _ in range(1500):
        d = int(rng.integers(0, 14))
        w = rng.exponential(size=d)
        w[rng.random(d) < 0.1] = 0
        rows.append(f4(w))
    hub = rng.exponential(size=70000)
    hub[rng.random(70000) < 0.1] = 0
    rows.append(f4(hub))
    for _ in range(40):
        rows.append(f4(rng.exponential(size=int(rng.integers(0, 9)))))
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    weight = np.concatenate(rows)
    assert indptr[1507] % 2048 not in (0, 2047) and indptr[1508] - indptr[1507] == 70000
    return indptr, weight


TABLE_GRAPH = table_graph()
HUB_ROW = 1507


def table_graph_edges(seed=1):
    """TABLE_GRAPH as a shuffled edge list: position j of row v becomes an edge (random src) -> v, then the edges are
    permuted -> (edges int64 [E, 2], num_nodes, weight float64 [E] in the edges' order)."""
    indptr, weight = TABLE_GRAPH
    n = len(indptr) - 1
    rng = np.random.default_rng(seed)
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    src = rng.integers(0, n, len(dst))
    p = rng.permutation(len(dst))
    return np.stack([src[p], dst[p]], 1), n, weight[p]


def succ_index(edges, num_nodes):
    """The sorted successor index Graph._csr_succ_sorted() holds: (indptr, col = dst by position, eid = ORIGINAL edge id by
    position): key src, rows ascending by dst, ties in edge-id order."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    order = np.lexsort((e[:, 1], e[:, 0]))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=num_nodes))]).astype(np.int64)
    return indptr, e[order, 1], order.astype(np.int64)


# ---- weighted walks ----------------------------------------------------------------------------------------------------------
def walk_restated(indptr, col, cum, starts, steps, seed):
    """ops.random_walk(..., weights=table) -> (paths int64 [W, steps + 1], lengths int64 [W])."""
    indptr, col, cum = np.asarray(indptr).tolist(), np.asarray(col).tolist(), np.asarray(cum).tolist()
    seed = int(seed) & M64
    paths = np.full((len(starts), steps + 1), -1, np.int64)
    lengths = np.ones(len(starts), np.int64)
    for w, s in enumerate(np.asarray(starts).tolist()):
        key = mix64_int(seed ^ mix64_int(w))
        cur = s
        paths[w, 0] = s
        for t in range(steps):
            b, e = indptr[cur], indptr[cur + 1]
            if e == b or cum[e - 1] == 0:
                break
            r = scale64_int(mix64_int(key ^ mix64_int((t + 1) << 20)), cum[e - 1])
            j = b
            while cum[j] <= r:
                j += 1
            cur = col[j]
            paths[w, t + 1] = cur
            lengths[w] = t + 2
    return paths, lengths


def weighted_successors(edges, q, n):
    """succ[v] = [(dst, q)] for every edge of positive q, in edge order."""
    succ = [[] for _ in range(n)]
    for (s, d), x in zip(np.asarray(edges).tolist(), np.asarray(q).tolist()):
        if x > 0:
            succ[s].append((d, x))
    return succ


def weighted_path_law(wsucc, start, steps):
    """walk_defs.path_law with a weighted step: {path tuple padded with -1 to steps + 1 nodes: probability}; the step from cur
    goes to x with probability (sum of q over the edges cur -> x) / (sum of q over cur's edges)."""
    out = {}

    def rec(walk, pr):
        cand = wsucc[walk[-1]] if len(walk) <= steps else []
        if not cand:
            out[tuple(walk) + (-1,) * (steps + 1 - len(walk))] = pr
            return
        tot = float(sum(x for _, x in cand))
        law = {}
        for d, x in cand:
            law[d] = law.get(d, 0.0) + x / tot
        for d, px in law.items():
            rec(walk + [d], pr * px)

    rec([start], 1.0)
    return out


# The weights of walk_defs.EDGES for the walk tests (edge order): the duplicated edge 0 -> 2 with two different weights, the
# duplicated edge 2 -> 5 with a zero on one copy, a zero-weight edge (3 -> 1), and weights over several orders of magnitude.
WALK_WEIGHTS = np.array([1.0, 2.0, 0.5, 4.0, 3.0, 1.0, 0.25, 1.5, 2.5, 0.0, 6.0, 1.0, 0.0, 2.0, 10.0, 0.125, 1.0, 1.0], np.float32)
LAW_STEPS, LAW_STARTS, LAW_WALKS = 3, (0, 2), 200000


# ---- weighted neighbour sampling ---------------------------------------------------------------------------------------------
def sample_weighted_restated(indptr, col, eid, cum, nodes, k, seed):
    """ops.sample_neighbors(..., weights=table) over the CSR (indptr, col, eid) -> (neighbors, count, eids, positions): positions =
    the chosen position inside its row, for the law checks.  Rows that draw are grouped by degree and handled as matrices; the
    only Python loops are over the distinct degrees and the k draws."""
    indptr, col = np.asarray(indptr, np.int64), np.asarray(col)
    nodes = np.asarray(nodes, np.int64)
    k, n = int(k), len(nodes)
    q = q_of(indptr, cum)
    b, deg = indptr[nodes], indptr[nodes + 1] - indptr[nodes]
    csq = np.concatenate([[0], np.cumsum(q > 0)])
    npos = csq[indptr[nodes + 1]] - csq[indptr[nodes]]
    draws = np.zeros(n, bool) if k < 0 else npos > k
    count = np.where(draws, k, npos).astype(np.int64)
    offsets = np.cumsum(count) - count
    pos = np.empty(int(count.sum()), np.int64)
    # the whole positive set, in row order
    allpos = np.flatnonzero(q > 0)
    for i in np.flatnonzero(~draws & (count > 0)):
        pos[offsets[i]:offsets[i] + count[i]] = allpos[csq[b[i]]:csq[b[i] + deg[i]]]
    sd = U64(int(seed) & M64)
    for d in np.unique(deg[draws]):
        sel = np.flatnonzero(draws & (deg == d))
        Q = q[b[sel][:, None] + np.arange(d, dtype=np.int64)[None, :]]
        avail = np.ones(Q.shape, bool)
        with np.errstate(over="ignore"):
            base = nodes[sel].astype(U64) * U64(KEY_MUL)
        for c in range(k):
            cs = np.cumsum(np.where(avail, Q, 0), axis=1).astype(U64)
            with np.errstate(over="ignore"):
                r = scale64(mix64(sd ^ mix64(base + U64(c))), cs[:, -1])
            j = (cs <= r[:, None]).sum(1)
            assert avail[np.arange(len(sel)), j].all() and (Q[np.arange(len(sel)), j] > 0).all()
            avail[np.arange(len(sel)), j] = False
            pos[offsets[sel] + c] = b[sel] + j
    rowstart = np.repeat(b, count)
    eids = pos if eid is None else np.asarray(eid)[pos].astype(np.int64)
    return col[pos].astype(np.int64), count, eids, pos - rowstart


def successive_law(q, k):
    """{ordered k-tuple of positions: probability} of successive sampling from the integer weights q, by enumeration."""
    q = [int(x) for x in q]
    out = {}

    def rec(chosen, pr, rest):
        if len(chosen) == k:
            out[tuple(chosen)] = pr
            return
        for j, x in enumerate(q):
            if x > 0 and j not in chosen:
                rec(chosen + [j], pr * x / rest, rest - x)

    rec([], 1.0, sum(q))
    return out


# (weights of every sampled row, k, nodes): the law cases of the sampler
SAMPLER_LAW_CASES = [([1, 2, 3, 4, 0], 2, 200000), ([5, 1, 1, 1, 1, 1], 3, 200000)]


def law_rows(weights, nodes, first_node=1000):
    """A dst-sorted CSR whose nodes first_node .. first_node + nodes - 1 each have len(weights) in-edges carrying `weights`
    (col = the position inside the row, eid = the position) -> (indptr, col int64, weight float32 [E], num_nodes)."""
    d = len(weights)
    indptr = np.concatenate([np.zeros(first_node, np.int64), np.arange(nodes + 1, dtype=np.int64) * d])
    return indptr, np.tile(np.arange(d, dtype=np.int64), nodes), np.tile(np.asarray(weights, np.float32), nodes), first_node + nodes


# ---- draws from a single-row table -------------------------------------------------------------------------------------------
def sample_from_table_restated(cum_row, count, seed):
    cum_row = np.asarray(cum_row, np.int64)
    with np.errstate(over="ignore"):
        r = scale64(mix64(U64(int(seed) & M64) ^ mix64(np.arange(count, dtype=U64))), U64(int(cum_row[-1])))
    return np.searchsorted(cum_row.astype(U64), r, side="right").astype(np.int64)
