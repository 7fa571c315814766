"""pgl_amd.sampling -- GPU neighbour sampling ("next" row f3).  Mirrors pgl.sampling.NeighborSampler
(pgl/sampling/sage.py:130-155): per layer, sample up to `size` in-neighbours of the current frontier,
relabel the sampled block to local ids, return one small Graph per layer plus the final node set.
The blocks feed GraphSageConv exactly as in examples/graphsage (feature = (x_src, x_dst)).

RelationNeighborSampler does the same over every edge type of a HeterGraph at once (the loop the reference's MAG240M example writes
by hand; pgl.sampling.HeteroNeighborSampler stays the reference's unimplemented stub): one block HeterGraph per layer for RGCNConv.

Also the walk generators of pgl/sampling/walk.py (random_walk, node2vec_walk, node2vec_walk_plus): one kernel launch
for every step of every walker on a tensor graph, its bit-identical host twin on a numpy graph.  The metapath walks of the
reference's metapath2vec example (examples/metapath2vec/datasets/sampling.py:285-398: metapath_randomwalk and
metapath_randomwalk_with_walktimes) run the same way over a HeterGraph, device walks by metapath_walks.

And the batches of Cluster-GCN / GraphSAINT style training: induced_subgraph (graph_kernel.extract_edges_from_nodes,
pgl/graph_kernel.pyx:394-432, with the relabel of pgl/sampling/custom.py:23-83) on the device for a tensor graph, ClusterBatches over
a partition and random_walk_subgraph over walks.

And the sampler pgl.nn.PinSageConv is defined for (the reference has none): pinsage_neighbors and PinSageSampler -- per node the
top-k nodes most often visited by short random walks, weighted by the normalised visit counts (ops.walk_visit_topk: one launch)."""
import numpy as np
import torch

from . import ops
from .bigraph import HeterGraph
from .graph import Graph
from .utils.edge_index import EdgeIndex


class NeighborSampler(object):
    def __init__(self, graph, samples, uva=False, seed=0, weights=None):
        # (uva: the reference's third argument -- sample from a graph kept in pinned host memory, pgl/sampling/sage.py:133-137; accepted,
        #  the index this sampler walks is in HBM)
        if not graph.is_tensor():
            raise ValueError("NeighborSampler needs a tensor-mode graph; call Graph.tensor() first")
        self.graph, self.samples = graph, list(samples)
        self.csr = graph.adj_dst_index.csr
        self._seed = int(seed)
        # weights (engine extension): an edge_feat name, an [E] tensor in original edge order or an ops.WeightTable over the dst
        # index -- every layer then samples in-edges by weight without replacement (ops.sample_neighbors weights=)
        self.weights = None if weights is None else _weight_table(graph, weights, "dst")

    def sample_neighbors(self, nodes):
        """-> (graph_list, nodes): graph_list[i] = (block Graph, number of dst nodes of that block), outermost
        layer first -- the same return convention as the reference (sage.py:139-155).  `nodes` may be unsorted and repeat ids:
        every block's first n_dst rows are its frontier as given, so row i of the last layer's output belongs to nodes[i].
        ValueError for an id outside [0, num_nodes)."""
        nodes = torch.as_tensor(nodes).to(self.graph.edges.device).to(torch.int64)
        graph_list = []
        for layer, size in enumerate(self.samples):
            self._seed += 1
            # the caller's batch is range-checked; later frontiers come out of reindex_graph, the neighbours out of the index
            neighbors, count = ops.sample_neighbors(self.csr, nodes, size, self._seed, check_range=(layer == 0), weights=self.weights)
            edge_src, edge_dst, sample_index = ops.reindex_graph(nodes, neighbors, count, check_range=False)
            # reindex_graph returns the destinations as repeat_interleave(arange, count): the block IS dst-sorted, so its dst
            # index needs no sort (round 2 re-sorted every block of every step through the full radix sort)
            n_blk = int(sample_index.shape[0])
            block = Graph(num_nodes=n_blk, edges=torch.stack([edge_src, edge_dst], 1),
                          adj_dst_index=EdgeIndex.from_sorted(edge_dst, edge_src, n_blk))
            block._ids_in_range = True        # ids come from reindex_graph: the src index (backward) is built without the range read-back
            graph_list.append((block, int(nodes.shape[0])))
            nodes = sample_index
        return graph_list[::-1], nodes


class HeteroNeighborSampler(object):
    """pgl/sampling/sage.py:158-162: declared by the reference, not implemented there either."""

    def __init__(self, graph_list, sample_list, uva=False):
        raise NotImplementedError


class RelationNeighborSampler(object):
    """Layer-wise neighbour sampling over every edge type of a HeterGraph at once -- the mini-batch step of RGCN / R-UniMP, which
    the reference's MAG240M example writes as a loop of one sample_neighbors call per edge type per layer plus reindex_heter_graph
    (examples/NeurIPS2022-OGB-Challenge/MAG240M/dataset/new_dataset_p2p.py:163-193).  (HeteroNeighborSampler above stays the
    reference's unimplemented stub.)  Per layer: ops.sample_neighbors_relations over the graph's stacked predecessor index (one
    count launch, one scan, one fill launch for all edge types, one host read), ONE relabel over all sampled sources, and a block
    HeterGraph whose relations share the relabelled node set.
    samples[layer]: an int (that fan-out for every edge type), a sequence in the order of hg.edge_types, or a dict by edge type
    (a missing type means 0: nothing sampled from it); -1 = all in-neighbours; at most ops.MAX_SAMPLE.
    A tensor HeterGraph runs on the device; a numpy HeterGraph runs the bit-identical host twin and returns numpy blocks with equal
    values.  Edge-weighted relational sampling is not provided (no weights= here)."""

    def __init__(self, hg, samples, seed=0, with_eids=False):
        self.graph, self.edge_types = hg, list(hg.edge_types)
        self.samples = [self._fanouts(s) for s in samples]
        self._seed, self.with_eids = int(seed), bool(with_eids)
        hg._stacked_pred()                                  # (ValueError for a graph without edge types; built once, cached on the graph)

    def _fanouts(self, s):
        types = self.edge_types
        if isinstance(s, dict):
            unknown = [et for et in s if et not in types]
            if unknown:
                raise ValueError("RelationNeighborSampler: unknown edge type %r in samples (the graph has %s)" % (unknown[0], types))
            fan = [int(s.get(et, 0)) for et in types]
        elif isinstance(s, (list, tuple, np.ndarray)):
            fan = [int(f) for f in s]
            if len(fan) != len(types):
                raise ValueError("RelationNeighborSampler: %d fan-outs for %d edge types %s" % (len(fan), len(types), types))
        else:
            fan = [int(s)] * len(types)
        if fan and max(fan) > ops.MAX_SAMPLE:
            raise ValueError("RelationNeighborSampler: fan-out %d exceeds ops.MAX_SAMPLE = %d (pass -1 for all neighbours)"
                             % (max(fan), ops.MAX_SAMPLE))
        return fan

    def sample_neighbors(self, nodes):
        """-> (graph_list, nodes): graph_list[i] = (block HeterGraph, number of dst nodes of that block), outermost layer first, as
        NeighborSampler returns them.  Every relation of a block is a Graph over the block's shared node set whose first n_dst rows
        are the frontier as given (unsorted, repeated ids kept), so `conv(block, h)[:n_dst]` is the next layer's input; a relation
        with no sampled edge is a Graph without edges.  with_eids: block[et].edge_feat["eid"] holds the relation-local ids of the
        sampled edges in the block's edge order.  ValueError for an id outside [0, num_nodes)."""
        hg = self.graph
        stacked = hg._stacked_pred()[0]
        if hg.is_tensor():
            nodes = torch.as_tensor(nodes).to(stacked.indptr.device).to(torch.int64).reshape(-1)
        else:
            nodes = np.asarray(nodes.detach().cpu().numpy() if isinstance(nodes, torch.Tensor) else nodes, dtype=np.int64).reshape(-1)
        graph_list = []
        for layer, fan in enumerate(self.samples):
            self._seed += 1
            n = int(nodes.shape[0])
            if hg.is_tensor():
                # the caller's batch is range-checked; later frontiers come out of the relabel, the neighbours out of the index
                s, offsets, bounds = ops._sample_relations(stacked, nodes, fan, self._seed, self.with_eids, layer == 0)
                src, out_nodes = ops._relabel(nodes.contiguous(), s.neighbors)
                block = self._device_blocks(s, offsets, bounds, src, n, int(out_nodes.shape[0]), fan)
            else:
                s = ops.host_sample_neighbors_relations(stacked, nodes, fan, self._seed, self.with_eids)
                src, out_nodes = ops._host_relabel(nodes, s.neighbors)
                block = HeterGraph(edges=None, multi_graph=self._host_blocks(s, src, int(out_nodes.shape[0])))
            graph_list.append((block, n))
            nodes = out_nodes
        return graph_list[::-1], nodes

    def _edge_feat(self, s, a, b):
        return {"eid": s.eids[a:b]} if self.with_eids else None

    def _host_blocks(self, s, src, n_blk):
        graphs = {}
        for r, et in enumerate(self.edge_types):
            a, b = s.edge_split[r], s.edge_split[r + 1]
            graphs[et] = Graph(num_nodes=n_blk, edges=np.stack([src[a:b], s.dst[a:b]], 1), edge_feat=self._edge_feat(s, a, b))
            graphs[et]._ids_in_range = True   # (what a later tensor() of the block builds its indices with)
        return graphs

    def _device_blocks(self, s, offsets, bounds, src, n, n_blk, fan):
        """The block HeterGraph of one layer with its relations' dst indices, at a number of launches that does not depend on the
        number of relations: the flat arrays are narrowed and stacked ONCE and every relation takes views of them; the fill kernel
        wrote the destinations relation by relation in seed order, so relation r's slice is dst-sorted and its indptr is the scan of
        its counts -- row r of one [R, n_blk + 1] table (rows n .. n_blk - 1, the sampled sources, have no in-edges).
        The same flat arrays ARE the block's stacked predecessor index (the table rebased by the relations' first positions, all
        sources, relation-local positions as edge ids): they seed the block's _stacked_pred cache, with max_segment = the largest
        fan-out when no fan-out is -1, so the first send_recv_relations over the block builds nothing and reads nothing back;
        _block_edges is what its backward builds the successor side from (HeterGraph._stacked_src)."""
        R = len(self.edge_types)
        src32, dst32 = ops.narrow_i64(src), ops.narrow_i64(s.dst)
        edges = torch.stack([src, s.dst], 1)
        indptr = torch.zeros((R, n_blk + 1), dtype=torch.int64, device=src.device)
        if n:
            indptr[:, :n] = offsets.view(R, n) - bounds[:R, None]
            indptr[:, n:] = (bounds[1:] - bounds[:-1])[:, None]
        degree = indptr[:, 1:] - indptr[:, :-1]
        graphs = {}
        for r, et in enumerate(self.edge_types):
            a, b = s.edge_split[r], s.edge_split[r + 1]
            block = Graph(num_nodes=n_blk, edges=edges[a:b], edge_feat=self._edge_feat(s, a, b),
                          adj_dst_index=EdgeIndex.from_sorted(dst32[a:b], src32[a:b], n_blk, indptr=indptr[r], degree=degree[r]))
            block._ids_in_range = True        # ids come from the relabel: the src index (backward) is built without the range read-back
            graphs[et] = block
        hg = HeterGraph(edges=None, multi_graph=graphs)
        if n:
            position = torch.arange(s.edge_split[-1], dtype=torch.int64, device=src.device)
            rel = torch.bucketize(position, bounds[1:], right=True)          # the relation that owns every edge position
            stacked = ops.StackedIndex(indptr + bounds[:R, None], src32, (position - bounds[rel]).to(torch.int32), n_blk, tuple(s.edge_split))
            if min(fan) >= 0:
                stacked.max_segment = max(fan)
            hg._stacked_p = (True, stacked, {et: r for r, et in enumerate(self.edge_types)})
            hg._block_edges = (src, s.dst, rel, s.edge_split, n_blk)
        return hg


def traverse(item):
    """pgl/sampling/sage.py:34-41: every scalar of a nested list / ndarray, depth first."""
    if isinstance(item, (list, np.ndarray)):
        for sub in item:
            yield from traverse(sub)
    else:
        yield item


def flat_node_and_edge(nodes, eids, weights=None):
    """pgl/sampling/sage.py:44-50: distinct node ids, all edge ids (and weights) of nested per-node lists."""
    return list(set(traverse(nodes))), list(traverse(eids)), (None if weights is None else list(traverse(weights)))


def edge_hash(src, dst):
    """pgl/sampling/sage.py:53-56: the key graphsage_sample filters ignore_edges by."""
    return src * 100000007 + dst


def subgraph(graph, nodes, eid=None, edges=None, with_node_feat=True, with_edge_feat=True):
    """pgl/sampling/custom.py:23-83: induced relabelled subgraph of a numpy graph (relabel through the
    native pglamd_map_ids, as the reference goes through graph_kernel.map_edges).  A tensor graph stays on the device
    (_subgraph_tensor): the same edges and features, a tensor Graph."""
    if graph.is_tensor():
        return _subgraph_tensor(graph, nodes, eid, edges, with_node_feat, with_edge_feat)
    if eid is None and edges is None:
        raise ValueError("Eid and edges can't be None at the same time.")
    nodes = np.asarray(nodes, dtype="int64")
    reindex = {int(n): i for i, n in enumerate(nodes)}
    edges = graph.edges[eid] if edges is None else np.asarray(edges, dtype="int64").reshape(-1, 2)
    sub_edge_feat = {}
    if with_edge_feat and graph.edge_feat:
        if eid is None:
            raise ValueError("Eid can not be None with edge features.")
        sub_edge_feat = {k: v[eid] for k, v in graph.edge_feat.items()}
    sub_edges = ops.host_map_ids(np.ascontiguousarray(edges).reshape(-1), reindex).reshape(-1, 2)
    sub_node_feat = {k: v[nodes] for k, v in graph.node_feat.items()} if with_node_feat else {}
    return Graph(edges=sub_edges, num_nodes=len(nodes), node_feat=sub_node_feat, edge_feat=sub_edge_feat)


def _device_ids(graph, ids, hi, what):
    """`ids` as a flat int64 tensor on the graph's device; ValueError for an id outside [0, hi) (one host read: the gathers
    below would read outside their tables)."""
    t = torch.as_tensor(ids).to(device=graph.edges.device, dtype=torch.int64).reshape(-1).contiguous()
    if int(t.shape[0]) and ops._ids_out_of_range(t, hi):
        raise ValueError("pgl_amd.sampling.subgraph: %s outside [0, %d)" % (what, hi))
    return t


def _gather_feats(feats, index):
    return {k: ops.gather_rows(v, index) for k, v in feats.items()}


def _subgraph_tensor(graph, nodes, eid, edges, with_node_feat, with_edge_feat):
    """subgraph() on a tensor graph: the relabel table is a dense int64 [num_nodes] array written by pglamd_scatter_rows and
    read by pglamd_gather_rows; an endpoint that is not in `nodes` maps to 0, as pglamd_map_ids answers on the host."""
    if eid is None and edges is None:
        raise ValueError("Eid and edges can't be None at the same time.")
    n_all, dev = graph.num_nodes, graph.edges.device
    nodes = _device_ids(graph, nodes, n_all, "node ids")
    if eid is not None:
        eid = _device_ids(graph, eid, graph.num_edges, "edge ids")
    if edges is None:
        flat = ops.gather_rows(graph.edges, eid).reshape(-1)
    else:
        flat = _device_ids(graph, edges, n_all, "edge endpoints")
        if int(flat.shape[0]) % 2:
            raise ValueError("edges must have shape (num_edges, 2)")
    sub_edge_feat = {}
    if with_edge_feat and graph.edge_feat:
        if eid is None:
            raise ValueError("Eid can not be None with edge features.")
        sub_edge_feat = _gather_feats(graph.edge_feat, eid)
    table = torch.zeros(max(n_all, 1), dtype=torch.int64, device=dev)
    ops.scatter_rows(table, nodes, torch.arange(int(nodes.shape[0]), dtype=torch.int64, device=dev))
    sub_edges = ops.gather_rows(table, flat).reshape(-1, 2)
    sub_node_feat = _gather_feats(graph.node_feat, nodes) if with_node_feat else {}
    return Graph(edges=sub_edges, num_nodes=int(nodes.shape[0]), node_feat=sub_node_feat, edge_feat=sub_edge_feat)


def induced_subgraph(graph, nodes, with_node_feat=True, with_edge_feat=True):
    """The subgraph induced by `nodes` (distinct ids inside [0, num_nodes), any order; ValueError otherwise): node i of the
    result is nodes[i], its edges are ALL edges of `graph` between two selected nodes -- multi-edges and self-loops kept --
    listed destination by destination in the order of `nodes`, every destination's in-edges in the order of adj_dst_index
    (the edge ids graph_kernel.extract_edges_from_nodes returns, pgl/graph_kernel.pyx:394-432).  node_feat["index"] holds the
    parent ids (the key graphsage_sample's callers use); the other features are the parent's rows / edge rows.
    Tensor graph: pgl_amd.ops.induced_subgraph on the device, a tensor Graph whose dst index is built without a sort (the
    edges come grouped by destination); numpy graph: the host twin, a numpy Graph with the same edges."""
    if graph.is_tensor():
        nodes = torch.as_tensor(nodes).to(device=graph.edges.device, dtype=torch.int64).reshape(-1).contiguous()
        n = int(nodes.shape[0])
        src, dst, eids = ops.induced_subgraph(graph.adj_dst_index.csr, nodes)
        node_feat = _gather_feats(graph.node_feat, nodes) if with_node_feat else {}
        node_feat["index"] = nodes
        edge_feat = _gather_feats(graph.edge_feat, eids) if with_edge_feat else {}
        sub = Graph(num_nodes=n, edges=torch.stack([src, dst], 1), node_feat=node_feat, edge_feat=edge_feat,
                    adj_dst_index=EdgeIndex.from_sorted(dst, src, n))
        sub._ids_in_range = True              # local ids: the src index (backward) is built without the range read-back
        return sub
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    ix = graph.adj_dst_index
    src, dst, eids = ops.host_induced_subgraph(ix._indptr, ix._sorted_v, ix._sorted_eid, nodes, graph.num_nodes)
    node_feat = {k: v[nodes] for k, v in graph.node_feat.items()} if with_node_feat else {}
    node_feat["index"] = nodes
    edge_feat = {k: v[eids] for k, v in graph.edge_feat.items()} if with_edge_feat else {}
    return Graph(edges=np.stack([src, dst], 1), num_nodes=len(nodes), node_feat=node_feat, edge_feat=edge_feat)


class ClusterBatches(object):
    """Cluster-GCN batches: an iterable of (subgraph, node_ids) over the clusters `part` (int [num_nodes]: the part of every
    node -- pgl.partition.metis_partition / random_partition, or the clustering behind Graph.reorder).  Nodes are grouped by
    part once (stable: ascending id inside a part); every pass over the object is one epoch, which draws the order of the
    non-empty clusters from a generator seeded by (seed, epoch number) and joins `clusters_per_batch` consecutive clusters of
    that order into one batch: node_ids = their node ranges concatenated, subgraph = induced_subgraph(graph, node_ids).  Every
    node is in exactly one batch of an epoch.  Tensor graph: node_ids and the subgraph stay on the device."""

    def __init__(self, graph, part, clusters_per_batch=1, shuffle=True, seed=0):
        part = part.detach().cpu().numpy() if isinstance(part, torch.Tensor) else np.asarray(part)
        part = part.astype(np.int64).reshape(-1)
        if part.shape[0] != graph.num_nodes:
            raise ValueError("ClusterBatches: part has %d entries for a graph of %d nodes" % (part.shape[0], graph.num_nodes))
        if part.shape[0] and part.min() < 0:
            raise ValueError("ClusterBatches: negative part id")
        if int(clusters_per_batch) < 1:
            raise ValueError("ClusterBatches: clusters_per_batch must be >= 1")
        self.graph, self.clusters_per_batch, self.shuffle, self.seed = graph, int(clusters_per_batch), bool(shuffle), int(seed)
        order = np.argsort(part, kind="stable").astype(np.int64)
        size = np.bincount(part) if part.shape[0] else np.zeros(0, np.int64)
        ends = np.cumsum(size)
        self._clusters = [(int(e - c), int(e)) for c, e in zip(size, ends) if c > 0]      # node ranges inside `order`
        self._order = torch.from_numpy(order).to(graph.edges.device) if graph.is_tensor() else order
        self._epoch = 0

    def __len__(self):
        return -(-len(self._clusters) // self.clusters_per_batch)

    def __iter__(self):
        k = len(self._clusters)
        rng = np.random.default_rng([self.seed, self._epoch])
        self._epoch += 1
        pick = rng.permutation(k) if self.shuffle else np.arange(k)
        cat = torch.cat if isinstance(self._order, torch.Tensor) else np.concatenate
        for b in range(0, k, self.clusters_per_batch):
            node_ids = cat([self._order[slice(*self._clusters[c])] for c in pick[b:b + self.clusters_per_batch]])
            yield induced_subgraph(self.graph, node_ids), node_ids


def random_walk_subgraph(graph, roots, walk_length, seed=None, weights=None):
    """GraphSAINT's random-walk sampler (the reference's graph_saint_random_walk_sample): one uniform walk of `walk_length` steps
    from every root, node set = the distinct nodes the walks visited (ascending), -> induced_subgraph(graph, node set).  A pure
    function of (graph, roots, walk_length, seed); seed=None draws it from numpy's global generator as the walks do.
    weights: the walks step by edge weight (see walks)."""
    if graph.is_tensor():
        paths, _ = walks(graph, roots, walk_length, seed=seed, weights=weights)
        nodes = torch.unique(paths[paths >= 0])
    else:
        roots = np.asarray(roots, dtype=np.int64).reshape(-1)
        indptr, col = graph._csr_succ_sorted()
        paths, _ = ops.host_random_walk(indptr, col, roots, int(walk_length), 1.0, 1.0, False, _walk_seed(seed), None,
                                        weights=None if weights is None else _weight_table(graph, weights, "succ"))
        nodes = np.unique(paths[paths >= 0])
    return induced_subgraph(graph, nodes)


def graphsage_sample(graph, nodes, samples, ignore_edges=[]):
    """pgl/sampling/sage.py:59-127 (host path, numpy graph): layer-wise predecessor sampling, returns a
    list of (subgraph, sample_index, node_index), one per layer, all over the same relabelled node set."""
    assert not graph.is_tensor(), "You must call Graph.numpy() first."
    node_index = np.asarray(nodes, dtype="int64")
    start_nodes = list(node_index.tolist())
    all_nodes, node_set = list(start_nodes), set(start_nodes)
    eids, edges, eid_set = [], [], set()
    ignore = {(int(s), int(d)) for s, d in ignore_edges}
    layer_eids, layer_edges = [], []
    for layer_idx in reversed(range(len(samples))):
        if len(start_nodes) == 0:
            layer_eids.insert(0, list(eids)); layer_edges.insert(0, list(edges))
            continue
        preds, pred_eids = graph.sample_predecessor(start_nodes, samples[layer_idx], return_eids=True)
        last = set(node_set)
        for srcs, dst, es in zip(preds, start_nodes, pred_eids):
            for src, eid in zip(srcs.tolist(), es.tolist()):
                if (src, dst) in ignore:
                    continue
                if eid not in eid_set:
                    eid_set.add(eid); eids.append(eid); edges.append([src, dst])
                if src not in node_set:
                    node_set.add(src); all_nodes.append(src)
        layer_eids.insert(0, list(eids)); layer_edges.insert(0, list(edges))
        start_nodes = list(node_set - last)
    reindex = {x: i for i, x in enumerate(all_nodes)}
    sample_index = np.array(all_nodes, dtype="int64")
    node_index = ops.host_map_ids(node_index, reindex)
    return [(subgraph(graph, nodes=all_nodes, eid=np.asarray(layer_eids[i], dtype="int64"),
                      edges=np.asarray(layer_edges[i], dtype="int64").reshape(-1, 2)), sample_index, node_index)
            for i in range(len(samples))]


# ------------------------------------------------------------------------------------------------
# random walks (pgl/sampling/walk.py:23-185)
# ------------------------------------------------------------------------------------------------
def _walk_seed(seed):
    """seed=None draws the walk seed from numpy's global generator, so np.random.seed(...) reproduces a run as it does with the
    reference (which samples from np.random / rand())."""
    return int(np.random.randint(0, np.iinfo(np.int64).max, dtype=np.int64)) if seed is None else int(seed)


def _weight_table(graph, weights, index):
    """weights= of the sampling-level functions: an ops.WeightTable over `index` as it is, else the name of an edge_feat entry
    or an [E] tensor / array in original edge order -> Graph.edge_weight_table(weights, index)."""
    return weights if isinstance(weights, ops.WeightTable) else graph.edge_weight_table(weights, index)


def _no_weighted_node2vec(p, q, weights):
    if weights is not None and not (p == 1.0 and q == 1.0):
        ops._weighted_walk_mode(ops.WALK_NODE2VEC, "node2vec_walk")


def walks(graph, nodes, num_steps, p=1.0, q=1.0, plus=False, seed=None, max_trials=None, weights=None):
    """Walks of num_steps steps from every node of `nodes` over a tensor graph's successors, left on the device:
    -> (paths int64 [len(nodes), num_steps + 1], -1 after a dead end; lengths int64 [len(nodes)]).  p == q == 1: uniform steps;
    otherwise node2vec (plus=True: node2vec-plus).  What a GPU training loop feeds to ops.skip_gram_pairs.
    weights (engine extension; p == q == 1 only): an edge_feat name, an [E] tensor in original edge order or an ops.WeightTable
    over the successor index -- every step follows an edge with probability proportional to its weight; a zero-weight edge is
    never followed."""
    if not graph.is_tensor():
        raise ValueError("walks() needs a tensor-mode graph; call Graph.tensor() first (or use random_walk on a numpy graph)")
    csr = graph._csr_succ_sorted()
    starts = torch.as_tensor(nodes).to(device=csr.indptr.device, dtype=torch.int64).reshape(-1)
    _no_weighted_node2vec(p, q, weights)
    return ops.random_walk(csr, starts, num_steps, p=p, q=q, plus=plus, seed=_walk_seed(seed), max_trials=max_trials,
                           weights=None if weights is None else _weight_table(graph, weights, "succ"))


def _walk_lists(graph, nodes, num_steps, p, q, plus, seed, max_trials, weights=None):
    if isinstance(nodes, torch.Tensor):
        nodes = nodes.detach().cpu().numpy()
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    _no_weighted_node2vec(p, q, weights)
    if nodes.shape[0] == 0:
        return []
    if graph.is_tensor():
        paths, lengths = walks(graph, nodes, num_steps, p, q, plus, seed, max_trials, weights)
        paths, lengths = paths.cpu().numpy(), lengths.cpu().numpy()
    else:
        indptr, col = graph._csr_succ_sorted()
        paths, lengths = ops.host_random_walk(indptr, col, nodes, num_steps, p, q, plus, _walk_seed(seed), max_trials,
                                              weights=None if weights is None else _weight_table(graph, weights, "succ"))
    return [row[:n].tolist() for row, n in zip(paths, lengths)]


def random_walk(graph, nodes, max_depth, *, seed=None, max_trials=None, weights=None):
    """pgl/sampling/walk.py:23-64: one walk per start, up to max_depth nodes (max_depth - 1 uniform steps over the successors,
    multi-edges counted with their multiplicity), ending early at a node without successors.  -> list of lists.
    weights (engine extension): steps by edge weight instead of uniformly (see walks)."""
    return _walk_lists(graph, nodes, max(int(max_depth) - 1, 0), 1.0, 1.0, False, seed, max_trials, weights)


def node2vec_walk(graph, nodes, max_depth, p=1.0, q=1.0, *, seed=None, max_trials=None, weights=None):
    """pgl/sampling/walk.py:67-122: random_walk when p == q == 1; otherwise up to max_depth steps (max_depth + 1 nodes), the
    first uniform, each later one weighted 1/p back to prev, 1 to a successor of prev, 1/q elsewhere
    (graph_kernel.node2vec_sample, pyx:140-177).  Exact: rejection sampling with an exact weighted scan after max_trials.
    weights: accepted only with p == q == 1 (ValueError otherwise: weighted node2vec is not provided)."""
    if p == 1.0 and q == 1.0:
        return random_walk(graph, nodes, max_depth, seed=seed, max_trials=max_trials, weights=weights)
    return _walk_lists(graph, nodes, max(int(max_depth), 0), p, q, False, seed, max_trials, weights)


def node2vec_walk_plus(graph, nodes, max_depth, p=1.0, q=1.0, *, seed=None, max_trials=None, weights=None):
    """pgl/sampling/walk.py:125-185: node2vec_walk whose weight-1 set is the union of the successors of every node the walk
    visited before the current one (graph_kernel.node2vec_plus_sample, pyx:180-224).  weights: only with p == q == 1."""
    if p == 1.0 and q == 1.0:
        return random_walk(graph, nodes, max_depth, seed=seed, max_trials=max_trials, weights=weights)
    return _walk_lists(graph, nodes, max(int(max_depth), 0), p, q, True, seed, max_trials, weights)


# ------------------------------------------------------------------------------------------------
# metapath walks over a HeterGraph (examples/metapath2vec/datasets/sampling.py:285-398; the same file under apps/Graph4Rec)
# ------------------------------------------------------------------------------------------------
def _metapath_relations(hg, metapath):
    """`metapath` ("c2p-p2a-a2p-p2c" or a list of edge-type names) -> (the names, their relation numbers in hg's stacked index)."""
    names = metapath.split("-") if isinstance(metapath, str) else list(metapath)
    if not names or (isinstance(metapath, str) and not metapath.strip()):
        raise ValueError("metapath walk: empty metapath %r" % (metapath,))
    number = hg._stacked_succ()[1]
    for et in names:
        if et not in number:
            raise ValueError("metapath walk: unknown edge type %r in metapath %r (the graph has %s)" % (et, metapath, list(number)))
    return names, [number[et] for et in names]


def _metapath_weights(hg, names, weights):
    """weights= of the metapath walks -> the WeightTable over hg's stacked index (None without weights): every edge type of the
    metapath needs an entry (ValueError otherwise); an edge type the metapath never follows gets a table of zeros, which no step
    reads.  Cached on the graph per set of relation tables (Graph.edge_weight_table caches those per tensor version)."""
    if weights is None:
        return None
    if not isinstance(weights, dict):
        raise ValueError("metapath walk: weights must be a dict {edge_type: edge_feat name | [E] weights | ops.WeightTable}, got %s"
                         % type(weights).__name__)
    missing = [et for et in names if et not in weights]
    if missing:
        raise ValueError("metapath walk: weights has no entry for edge type %r of the metapath" % missing[0])
    tables = {et: _weight_table(hg[et], weights[et], "succ") for et in hg.edge_types if et in weights}
    key = (hg.is_tensor(),) + tuple((et, id(t.cum)) for et, t in tables.items())
    hit = getattr(hg, "_stacked_tables", None)
    if hit is not None and hit[0] == key:
        return hit[2]
    stacked = hg._stacked_succ()[0]
    parts = []
    for r, et in enumerate(hg.edge_types):
        if et in tables:
            parts.append(tables[et])
            continue
        E = stacked.edge_base[r + 1] - stacked.edge_base[r]
        if hg.is_tensor():
            z = dict(dtype=torch.int64, device=stacked.col.device)
            parts.append(ops.WeightTable(torch.zeros(E, **z), torch.zeros(stacked.num_nodes, **z)))
        else:
            parts.append(ops.WeightTable(np.zeros(E, np.int64), np.zeros(stacked.num_nodes, np.int64)))
    table = ops.stack_weight_tables(parts)
    hg._stacked_tables = (key, tables, table)              # (holds the relation tables: their ids cannot be reused while it lives)
    return table


def metapath_walks(hg, nodes, metapath, num_steps, *, phase=0, seed=None, weights=None):
    """Metapath walks of num_steps steps from every node of `nodes` over a tensor-mode HeterGraph, left on the device:
    -> (paths int64 [len(nodes), num_steps + 1], -1 after a dead end; lengths int64 [len(nodes)]) -- what ops.skip_gram_pairs
    consumes.  The step from position t follows a uniformly drawn successor under edge type metapath[(phase + t) % len(metapath)];
    a node without successors under that edge type ends the walk.  metapath: the reference's string form "c2p-p2a-a2p-p2c" or a
    list of edge-type names (ValueError for an unknown edge type or an empty metapath).  One kernel launch for all steps of all
    walkers (ops.metapath_walk).  seed=None draws the seed from numpy's global generator, as the other walks do.
    weights (engine extension): a dict {edge_type: edge_feat name | [E] tensor in original edge order | ops.WeightTable over that
    relation's successor index} covering every edge type of the metapath (ValueError otherwise): every step follows an edge with
    probability proportional to its weight; a zero-weight edge is never followed."""
    if not hg.is_tensor():
        raise ValueError("metapath_walks() needs a tensor-mode HeterGraph; call HeterGraph.tensor() first (or use metapath_randomwalk "
                         "on a numpy graph)")
    names, rel = _metapath_relations(hg, metapath)
    stacked = hg._stacked_succ()[0]
    starts = torch.as_tensor(nodes).to(device=stacked.indptr.device, dtype=torch.int64).reshape(-1)
    return ops.metapath_walk(stacked, starts, rel, num_steps, phase=phase, seed=_walk_seed(seed), weights=_metapath_weights(hg, names, weights))


def _metapath_host_ids(nodes):
    if isinstance(nodes, torch.Tensor):
        nodes = nodes.detach().cpu().numpy()
    return np.asarray(nodes, dtype=np.int64).reshape(-1)


def _metapath_arrays(hg, starts, names, rel, num_steps, phase, seed, weights):
    """(paths, lengths) as numpy arrays: the device kernel on a tensor graph, the host twin on a numpy graph -- the same arrays."""
    stacked, table = hg._stacked_succ()[0], _metapath_weights(hg, names, weights)
    if hg.is_tensor():
        paths, lengths = ops.metapath_walk(stacked, torch.from_numpy(starts).to(stacked.indptr.device), rel, num_steps, phase=phase,
                                           seed=seed, weights=table)
        return paths.cpu().numpy(), lengths.cpu().numpy()
    return ops.host_metapath_walk(stacked, starts, rel, num_steps, phase=phase, seed=seed, weights=table)


def metapath_randomwalk(graph, start_nodes, metapath, walk_length, alias_name=None, events_name=None, *, seed=None, weights=None):
    """examples/metapath2vec/datasets/sampling.py:350-398: one walk per start of up to walk_length nodes (walk_length - 1 steps), step i
    following a uniformly drawn successor under edge type metapath[i % len(metapath)], ending early at a node without successors
    under the step's edge type -> list of lists.  alias_name / events_name: the reference's unused parameters, accepted and ignored.
    Tensor HeterGraph: ops.metapath_walk, one launch; numpy HeterGraph: its host twin -- for the same seed the two return equal
    lists.  seed=None draws the seed from numpy's global generator (np.random.seed reproduces a run).  weights: see metapath_walks."""
    names, rel = _metapath_relations(graph, metapath)
    starts = _metapath_host_ids(start_nodes)
    _metapath_weights(graph, names, weights)               # (its argument errors come before the empty-input return; cached)
    if starts.shape[0] == 0:
        return []
    paths, lengths = _metapath_arrays(graph, starts, names, rel, max(int(walk_length) - 1, 0), 0, _walk_seed(seed), weights)
    return [row[:n].tolist() for row, n in zip(paths, lengths)]


def metapath_randomwalk_with_walktimes(graph, start_nodes, metapath, walk_length, walk_times=10, alias_name=None, events_name=None, *,
                                       seed=None):
    """examples/metapath2vec/datasets/sampling.py:285-347: per start up to walk_times of its metapath[0] successors WITHOUT replacement
    (all of them when it has at most walk_times), each the second node of a walk [start, neighbour, ...] that goes on with
    metapath[i % len(metapath)] at step i up to walk_length nodes -> list of lists, start by start.  A start without
    metapath[0] successors contributes no walk.
    Tensor HeterGraph: ops.sample_neighbors over the first relation's successor index (walk_times <= ops.MAX_SAMPLE; a pure
    function of (seed, node id), so a repeated start repeats its neighbours), then ops.metapath_walk from the neighbours with
    phase 1; numpy HeterGraph: the first step through graph.sample_successor as the reference takes it (numpy's global
    generator), the rest by the host twin.  The two follow the same law but are NOT equal for equal seeds: their first-step
    samplers differ."""
    names, rel = _metapath_relations(graph, metapath)
    starts = _metapath_host_ids(start_nodes)
    seed = _walk_seed(seed)
    if starts.shape[0] == 0:
        return []
    n = int(graph.num_nodes)
    if int(starts.min()) < 0 or int(starts.max()) >= n:
        raise ValueError("metapath_randomwalk_with_walktimes: start nodes outside [0, num_nodes=%d)" % n)
    if graph.is_tensor():
        csr = graph[names[0]]._csr_succ_sorted()
        nbr, count = ops.sample_neighbors(csr, torch.from_numpy(starts).to(csr.indptr.device), int(walk_times), seed=seed)
        second, count = nbr.cpu().numpy(), count.cpu().numpy()
    else:
        picked = graph.sample_successor(names[0], starts, max_degree=int(walk_times))
        count = np.asarray([len(p) for p in picked], dtype=np.int64)
        second = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in picked]) if len(picked) else np.zeros(0, np.int64)
    if second.shape[0] == 0:
        return []
    first = np.repeat(starts, count)
    paths, lengths = _metapath_arrays(graph, np.ascontiguousarray(second, dtype=np.int64), names, rel, max(int(walk_length) - 2, 0),
                                      1 % len(rel), seed, None)
    return [[int(s)] + row[:n].tolist() for s, row, n in zip(first, paths, lengths)]


# ------------------------------------------------------------------------------------------------
# PinSAGE neighbourhoods (engine extension: the reference has pgl.nn.PinSageConv and no sampler for it)
# ------------------------------------------------------------------------------------------------
def _visit_weights(cnt, xp):
    """cnt int32 [S, T] -> float32 [S, T]: every row divided by its sum (a row of zeros stays zero)."""
    c = cnt.to(torch.float32) if xp is torch else cnt.astype(np.float32)
    total = c.sum(1, keepdim=True) if xp is torch else c.sum(1, keepdims=True)
    return c / (total.clamp(min=1.0) if xp is torch else np.maximum(total, np.float32(1.0)))


def pinsage_neighbors(graph, nodes, num_walks, walk_length, top_k, seed=None, weights=None):
    """The PinSAGE neighbourhood of every node of `nodes`: the top_k nodes most often visited by num_walks random walks of
    walk_length steps from it (the node itself excluded), with the normalised visit counts as importance weights
    -> (nbr int64 [S, top_k], padding -1; weight float32 [S, top_k] = count / the row's sum of counts, padding 0; num int32 [S]).
    Ties are broken by node id; a node the walks never leave has num 0.  Tensor graph: ops.walk_visit_topk, one launch on the
    device; numpy graph: its bit-identical host twin.  seed=None draws the seed from numpy's global generator, as the walks do.
    weights: an edge_feat name, an [E] tensor / array in original edge order or an ops.WeightTable over the successor index --
    the walks then step by edge weight.  The walks follow SUCCESSORS (src -> dst), like every walk of this library: on a
    directed graph whose messages flow src -> dst the nodes that reach a seed are found on the reversed graph."""
    table = None if weights is None else _weight_table(graph, weights, "succ")
    if graph.is_tensor():
        csr = graph._csr_succ_sorted()
        seeds = torch.as_tensor(nodes).to(device=csr.indptr.device, dtype=torch.int64).reshape(-1)
        nbr, cnt, num = ops.walk_visit_topk(csr, seeds, num_walks, walk_length, top_k, seed=_walk_seed(seed), weights=table)
        return nbr, _visit_weights(cnt, torch), num
    indptr, col = graph._csr_succ_sorted()
    seeds = np.asarray(nodes, dtype=np.int64).reshape(-1)
    nbr, cnt, num = ops.host_walk_visit_topk(indptr, col, seeds, num_walks, walk_length, top_k, seed=_walk_seed(seed), weights=table)
    return nbr, _visit_weights(cnt, np), num


class PinSageSampler(object):
    """Layer-wise PinSAGE blocks for pgl.nn.PinSageConv, with NeighborSampler's return convention: per layer the frontier's
    top_ks[layer] most visited nodes (ops.walk_visit_topk: num_walks walks of walk_length steps per frontier node) become the
    in-neighbours of a relabelled block whose edges run neighbour -> frontier node, and block.edge_feat["weight"] (float32
    [E, 1], the shape the layer's edge operand has in the reference) holds the normalised visit counts in the block's edge
    order, so PinSageConv(block, x, block.edge_feat["weight"]) is the PinSAGE layer.  The walks follow successors, like every walk of this library: a directed graph may want its reverse here.
    weights: as pinsage_neighbors.  Every call of sample_neighbors advances the seed, layer by layer."""

    def __init__(self, graph, num_walks, walk_length, top_ks, seed=0, weights=None):
        if not graph.is_tensor():
            raise ValueError("PinSageSampler needs a tensor-mode graph; call Graph.tensor() first")
        self.graph, self.top_ks = graph, list(top_ks)
        self.num_walks, self.walk_length = int(num_walks), int(walk_length)
        self.csr = graph._csr_succ_sorted()
        self._seed = int(seed)
        self.weights = None if weights is None else _weight_table(graph, weights, "succ")

    def sample_neighbors(self, nodes):
        """-> (graph_list, nodes): graph_list[i] = (block Graph, number of dst nodes of that block), outermost layer first.
        `nodes` may be unsorted and repeat ids: every block's first n_dst rows are its frontier as given.  ValueError for an id
        outside [0, num_nodes)."""
        nodes = torch.as_tensor(nodes).to(self.graph.edges.device).to(torch.int64).reshape(-1)
        graph_list = []
        for layer, top_k in enumerate(self.top_ks):
            self._seed += 1
            # the caller's batch is range-checked; later frontiers come out of reindex_graph
            nbr, cnt, num = ops.walk_visit_topk(self.csr, nodes, self.num_walks, self.walk_length, top_k, seed=self._seed,
                                                weights=self.weights, check_range=(layer == 0))
            filled = nbr >= 0                                  # a prefix of every row: the row-major flattening keeps row order
            edge_src, edge_dst, sample_index = ops.reindex_graph(nodes, nbr[filled], num.to(torch.int64), check_range=False)
            n_blk = int(sample_index.shape[0])
            block = Graph(num_nodes=n_blk, edges=torch.stack([edge_src, edge_dst], 1), edge_feat={"weight": _visit_weights(cnt, torch)[filled].unsqueeze(1)},
                          adj_dst_index=EdgeIndex.from_sorted(edge_dst, edge_src, n_blk))
            block._ids_in_range = True        # ids come from reindex_graph: the src index (backward) is built without the range read-back
            graph_list.append((block, int(nodes.shape[0])))
            nodes = sample_index
        return graph_list[::-1], nodes


# ------------------------------------------------------------------------------------------------
# negatives checked against the graph (ops.sample_negatives): absent edges, corrupted edges, BPR triples
# ------------------------------------------------------------------------------------------------
def _noise_table(graph, noise):
    """noise= of the functions below: None, a single-row ops.WeightTable as it is, or an [N] weight vector (tensor / array) ->
    ops.weight_table on a tensor graph, its host twin on a numpy graph."""
    if noise is None or isinstance(noise, ops.WeightTable):
        return noise
    if graph.is_tensor():
        return ops.weight_table(torch.as_tensor(noise).to(graph.edges.device).reshape(-1))
    w = np.asarray(noise.detach().cpu().numpy() if isinstance(noise, torch.Tensor) else noise).reshape(-1)
    return ops.host_edge_weight_table(np.array([0, w.shape[0]], np.int64), w)


def _negatives(graph, index, src, num_neg, seed, candidates, noise, exclude_self, return_pos=False, **kw):
    """ops.sample_negatives over `index` of a tensor graph, its host twin over the numpy twin of a numpy graph."""
    lo, hi = (0, None) if candidates is None else (int(candidates[0]), int(candidates[1]))
    noise = _noise_table(graph, noise)
    if noise is not None and candidates is not None and (lo, hi) != (0, int(noise.cum.shape[0])):
        raise ValueError("negative sampling: weighted noise over a sub-range of the nodes is not provided; pass candidates=None")
    if graph.is_tensor():
        src = torch.as_tensor(src).to(device=index.indptr.device, dtype=torch.int64).reshape(-1)
        return ops.sample_negatives(index, src, num_neg, seed=_walk_seed(seed), lo=lo, hi=hi, noise=noise, exclude_self=exclude_self,
                                    return_pos=return_pos, **kw)
    if isinstance(src, torch.Tensor):
        src = src.detach().cpu().numpy()
    return ops.host_sample_negatives(index[0], index[1], np.asarray(src, dtype=np.int64).reshape(-1), num_neg, seed=_walk_seed(seed),
                                     lo=lo, hi=hi, noise=noise, exclude_self=exclude_self, return_pos=return_pos, **kw)


def negative_samples(graph, src, num_neg, seed=0, candidates=None, noise=None, exclude_self=True, **kw):
    """For every node of `src` num_neg nodes that are NOT its successors in `graph` -> int64 [len(src), num_neg] (a tensor on a
    tensor graph: one launch of ops.sample_negatives; a numpy array, equal value for value, on a numpy graph: its host twin).
    candidates: None (all nodes) or an (lo, hi) pair of node ids; noise: None (uniform), an [N] weight vector or a single-row
    ops.WeightTable -- the word2vec noise distribution is degree ** 0.75; exclude_self: the node itself is no negative either.
    The draws depend on (seed, position in src, k) alone: a node listed twice gets different negatives.  ValueError for a node
    whose successors cover all candidates unless allow_empty=True (its row is then -1)."""
    return _negatives(graph, graph._csr_succ_sorted(), src, num_neg, seed, candidates, noise, exclude_self, **kw)


def corrupt_edges(graph, edges, num_neg, side="dst", seed=0, candidates=None, noise=None, exclude_self=False, **kw):
    """The corrupted triples of a link-prediction / knowledge-graph loss: for every edge (u, v) of `edges` ([n, 2]) num_neg
    replacements of the chosen end -> int64 [n, num_neg].  side="dst": ids x such that (u, x) is no edge of `graph`;
    side="src": ids x such that (x, v) is none (searched in the predecessor index Graph._csr_pred_sorted).  candidates, noise,
    exclude_self (against the end that is kept) and the tensor / numpy convention as negative_samples."""
    if side not in ("dst", "src"):
        raise ValueError("corrupt_edges: side must be 'dst' or 'src'")
    e = edges if isinstance(edges, torch.Tensor) else np.asarray(edges)
    e = e.reshape(-1, 2)
    index = graph._csr_succ_sorted() if side == "dst" else graph._csr_pred_sorted()
    return _negatives(graph, index, e[:, 0] if side == "dst" else e[:, 1], num_neg, seed, candidates, noise, exclude_self, **kw)


def bpr_triples(graph, users, item_range, seed=0):
    """The (user, positive item, negative item) triples of a BPR step (examples/lightgcn/utils.py UniformSample_original_python,
    examples/ngcf/utils.py: a Python loop per user) over a user -> item graph: per user one uniform successor and one id of
    item_range = (lo, hi) that is not a successor -> (users, pos, neg), each int64 [m]; users without a positive are dropped, as
    the reference's loop skips them.  One library launch on a tensor graph; equal numpy arrays on a numpy graph.  The draws depend
    on (seed, position in users): a user listed twice gets two different triples.  ValueError for a user who has every item."""
    neg, pos = _negatives(graph, graph._csr_succ_sorted(), users, 1, seed, item_range, None, False, return_pos=True)
    if graph.is_tensor():
        users = torch.as_tensor(users).to(device=neg.device, dtype=torch.int64).reshape(-1)
    else:
        users = np.asarray(users.detach().cpu().numpy() if isinstance(users, torch.Tensor) else users, dtype=np.int64).reshape(-1)
    keep = pos >= 0
    return users[keep], pos[keep], neg[keep, 0]


# The reference keeps these functions in three submodules (pgl/sampling/sage.py, custom.py, walk.py) and its programs import from there
# (`from pgl.sampling.custom import subgraph`: 15 places); all three names answer with this module.
import sys as _sys                                                   # noqa: E402
custom = sage = walk = _sys.modules[__name__]
_sys.modules[__name__ + ".custom"] = _sys.modules[__name__ + ".sage"] = _sys.modules[__name__ + ".walk"] = custom
__path__ = []                                                        # (lets `import <alias>.sampling.custom` reach the finders: a module without __path__ is refused as a parent)
