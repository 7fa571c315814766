"""Shared by tests/test_subgraph_defs.py, test_subgraph_host.py and test_subgraph_gpu.py: the induced subgraph of
pgl_amd/csrc/subgraph.hip restated in numpy from its documented definition (no project imports).

Over the stable dst-sorted index (indptr, col, eid) that ops.CSR holds (sampling_defs.csr_by_dst) and a list `nodes` of
DISTINCT ids inside [0, num_nodes):

    local = full(num_nodes, -1); local[nodes] = arange(len(nodes))
    for i, v in enumerate(nodes):                    # rows in the order given
        for j in range(indptr[v], indptr[v + 1]):    # positions in CSR order
            if local[col[j]] >= 0: emit (local[col[j]], i, eid[j])

The result is grouped by dst_local in non-decreasing order; multi-edges keep their multiplicity, self-loops are kept; the
eids are what the reference's graph_kernel.extract_edges_from_nodes returns, in the same order.  A repeated or out-of-range
id is a ValueError (stricter than the reference on purpose)."""
import numpy as np


def _checked(nodes, num_nodes):
    nodes = np.asarray(nodes, np.int64).reshape(-1)
    if len(nodes) and (nodes.min() < 0 or nodes.max() >= num_nodes):
        raise ValueError("node id outside [0, %d)" % num_nodes)
    if len(np.unique(nodes)) != len(nodes):
        raise ValueError("repeated node id")
    return nodes


def induced_loop(indptr, col, eid, nodes, num_nodes):
    """The definition as written above, edge by edge (small graphs only)."""
    nodes = _checked(nodes, num_nodes)
    local = np.full(num_nodes, -1, np.int64)
    local[nodes] = np.arange(len(nodes), dtype=np.int64)
    out = []
    for i, v in enumerate(nodes):
        for j in range(int(indptr[v]), int(indptr[v + 1])):
            if local[col[j]] >= 0:
                out.append((local[col[j]], i, eid[j]))
    out = np.asarray(out, np.int64).reshape(-1, 3)
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()


def induced_restated(indptr, col, eid, nodes, num_nodes):
    """-> (src_local, dst_local, eids), all int64: the same loops, vectorised (the candidate positions of all selected rows in
    the order given, then the mask)."""
    indptr, col, eid = np.asarray(indptr, np.int64), np.asarray(col, np.int64), np.asarray(eid, np.int64)
    nodes = _checked(nodes, num_nodes)
    local = np.full(num_nodes, -1, np.int64)
    local[nodes] = np.arange(len(nodes), dtype=np.int64)
    b = indptr[nodes]
    deg = indptr[nodes + 1] - b
    start = np.cumsum(deg) - deg
    row = np.repeat(np.arange(len(nodes), dtype=np.int64), deg)
    pos = np.repeat(b - start, deg) + np.arange(int(deg.sum()), dtype=np.int64)      # CSR position of every candidate
    src = local[col[pos]]
    keep = src >= 0
    return src[keep], row[keep], eid[pos][keep]


def induced_brute_force(edges, nodes, num_nodes):
    """Independent of the index: the edges with both endpoints selected (an `isin` mask over the edge LIST), ordered by
    (position of the destination in `nodes`, position in the stable dst-sorted stream) -> (src_local, dst_local, eids)."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    nodes = _checked(nodes, num_nodes)
    keep = np.flatnonzero(np.isin(edges[:, 0], nodes) & np.isin(edges[:, 1], nodes))
    where = {int(v): i for i, v in enumerate(nodes)}
    s = np.asarray([where[int(u)] for u in edges[keep, 0]], np.int64)
    d = np.asarray([where[int(v)] for v in edges[keep, 1]], np.int64)
    # inside one destination row the stable dst-sorted stream lists edges by ascending edge id
    order = np.lexsort((keep, d))
    return s[order], d[order], keep[order]


def graph_with_hub(num_nodes=5000, num_edges=60000, hub_edges=3000, seed=0):
    """The graph of the comparison with the reference's extract_edges_from_nodes: uniform random edges, `hub_edges` of them
    redirected into one destination; multi-edges and self-loops occur."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, num_nodes, (num_edges, 2)).astype(np.int64)
    e[rng.choice(num_edges, hub_edges, replace=False), 1] = num_nodes // 3
    return e


def small_multigraph(n=40, m=300, seed=0):
    """n nodes, m edges with guaranteed multi-edges and self-loops, a few nodes without in-edges."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n - 5, (m, 2)).astype(np.int64)                                # the last five nodes: no edges at all
    e[:20] = e[20:40]                                                                  # twenty repeated pairs
    e[40:50, 1] = e[40:50, 0]                                                          # ten self-loops
    e[50:52] = e[40]                                                                   # a self-loop three times
    return e[rng.permutation(m)], n
