"""pgl.graph_kernel (pgl/graph_kernel.pyx): the reference's native module, by name.  The functions on the hot path are
answered by libpglamd's host-side entry points (numpy in, numpy out); sampling helpers live in pgl_amd.sampling."""
import numpy as np

from . import ops

__all__ = ["build_index", "map_nodes", "map_edges", "metis_partition", "skip_gram_gen_pair", "extract_edges_from_nodes",
           "alias_sample_build_table"]


def build_index(u, v, num_nodes):
    """pgl/graph_kernel.pyx:59-88 -> (degree, sorted_v, sorted_u, sorted_eid, indptr), int64."""
    return ops.host_build_index(u, v, num_nodes)


def map_nodes(nodes, reindex):
    """pgl/graph_kernel.pyx:123-138."""
    return ops.host_map_ids(np.asarray(nodes, dtype=np.int64), reindex)


def map_edges(eids, edges, reindex):
    """pgl/graph_kernel.pyx:104-121: relabel both endpoints of edges[eids] through `reindex` -> int64 [len(eids), 2]."""
    e = np.asarray(edges, dtype=np.int64)[np.asarray(eids, dtype=np.int64)]
    return ops.host_map_ids(e.reshape(-1), reindex).reshape(-1, 2)


def extract_edges_from_nodes(adj_indptr, sorted_v, sorted_eid, sampled_nodes):
    """pgl/graph_kernel.pyx:394-432: the ids of the edges between `sampled_nodes`, row by row in the order the nodes are given,
    every row in the order of the index passed (either of a graph's two indices).  -> int64 array.  Stricter than the
    reference on purpose: a repeated or out-of-range node id is a ValueError (the reference emits a repeated row twice and
    reads outside its table).  (On the device, with the relabelled endpoints: pgl_amd.ops.induced_subgraph.)"""
    return ops.host_induced_subgraph(adj_indptr, sorted_v, sorted_eid, sampled_nodes)[2]


def metis_partition(num_nodes, adj_indptr, sorted_v, nparts, node_weights=None, edge_weights=None, recursive=False):
    """pgl/graph_kernel.pyx:434-472 (K-way; the reference's wrapper never takes the recursive branch: pgl/partition.py:80-89).
    Like pgl_amd.partition.metis_partition: the reference's NAME, answered by the engine's own k-way partitioner
    (pglamd_partition_kway); no METIS code is reachable from the product."""
    if recursive:
        raise NotImplementedError("recursive METIS is not exposed (pgl/partition.py:80: 'recursive metis always core dump')")
    part, _ = ops.host_partition_kway(num_nodes, adj_indptr, sorted_v, nparts, node_weights, edge_weights, 0)
    return part


def skip_gram_gen_pair(walk, win_size=5):
    """pgl/graph_kernel.pyx:341-364: the (center, context) pairs of one walk -> (src, dst) lists.  Position i pairs walk[i] with
    every walk[j], j in [max(0, i - r[i]), min(l - 1, i + r[i])] ascending, skipping equal ids; r comes from the SAME single
    np.random.randint call as the reference's, so under one np.random.seed the pairs are identical.  (On the device, over many
    walks at once: pgl_amd.ops.skip_gram_pairs.)"""
    w = np.asarray(walk, dtype=np.int64).reshape(-1)
    l = int(w.shape[0])
    rnd = np.random.randint(1, win_size + 1, dtype=np.int64, size=l)
    if l == 0:
        return [], []
    i = np.arange(l, dtype=np.int64)
    lo, hi = np.maximum(i - rnd, 0), np.minimum(i + rnd, l - 1)
    cnt = hi - lo + 1
    ii = np.repeat(i, cnt)
    jj = lo[ii] + np.arange(ii.shape[0], dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    keep = w[ii] != w[jj]
    return w[ii][keep].tolist(), w[jj][keep].tolist()


def alias_sample_build_table(probs):
    """pgl/graph_kernel.pyx:366-392 by name and return convention: the alias table of a discrete distribution (Walker / Vose)
    -> (accept float64 [n], alias int64 [n]).  A draw takes a uniform column i and a uniform u in [0, 1): the outcome is i when
    u < accept[i], else alias[i]; so P(k) = (accept[k] + sum over i with alias[i] == k of (1 - accept[i])) / n.  Written from
    that definition: every column i starts with mass n * probs[i]; a column below 1 is topped up by a column above 1, which
    becomes its alias and gives up what it lent.  (The engine's own weighted draws use integer prefix sums instead --
    ops.edge_weight_table / ops.sample_from_table; this is the reference's host helper, kept for its callers.)"""
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    n = int(p.shape[0])
    accept = p * n
    alias = np.arange(n, dtype=np.int64)
    small = [i for i in range(n) if accept[i] < 1.0]
    large = [i for i in range(n) if accept[i] > 1.0]
    while small and large:
        lo, hi = small.pop(), large[-1]
        alias[lo] = hi                                   # column lo: itself with probability accept[lo], else hi
        accept[hi] -= 1.0 - accept[lo]                   # hi lent 1 - accept[lo] of its mass
        if accept[hi] <= 1.0:
            large.pop()
            if accept[hi] < 1.0:
                small.append(hi)
    np.minimum(accept, 1.0, out=accept)                  # what rounding left above (or a hair below) 1 is a full column
    for i in small:
        accept[i] = 1.0
    return accept, alias
