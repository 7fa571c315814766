"""Graph read-out layers over the segment kernels (pgl/nn/pool.py:30-262): a batched graph's nodes are one sorted
segment per member graph (graph_node_id), so every read-out is a segment reduction / segment softmax."""
import warnings

import torch
import torch.nn as nn

from .. import math as gmath
from . import functional as GF

__all__ = ["GraphPool", "GraphNorm", "GlobalAttention", "Set2Set", "SAGPool"]


class GraphPool(nn.Module):
    """pgl/nn/pool.py:30-62."""

    def __init__(self, pool_type=None):
        super(GraphPool, self).__init__()
        self.pool_type = pool_type

    def forward(self, graph, feature, pool_type=None):
        if pool_type is not None:
            warnings.warn("The pool_type argument in forward function will be discarded in the future, "
                          "please initialize it when creating a GraphPool instance.")
        else:
            pool_type = self.pool_type
        return gmath.segment_pool(feature, graph.graph_node_id, pool_type)


class GraphNorm(nn.Module):
    """pgl/nn/pool.py:65-93: every node feature divided by sqrt(number of nodes of its graph)."""

    def forward(self, graph, feature):
        return GF.graph_norm(graph, feature)


def _readout_plan(graph, x, fused):
    """The read-out plan (pgl_amd.readout_ops.readout_plan) when the fused read-out takes (graph, x), else None: `fused` set, x a CUDA
    fp32 [N, d] tensor of a supported width, a tensor graph whose _graph_node_index is a HOST array consistent with N (the test
    SAGPool._host_plan uses: a caller's own device tensor would cost a host read).  Built once per (graph, device) and kept on the
    graph object, so a training loop and a captured step reuse it."""
    import numpy as np
    from .. import readout_ops
    if not (fused and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        return None
    index = getattr(graph, "_graph_node_index", None)
    if index is None or not getattr(graph, "is_tensor", lambda: False)() or not readout_ops.readout_supported(x.shape[1]):
        return None
    if isinstance(index, torch.Tensor) and index.is_cuda:
        return None
    cache = graph.__dict__.setdefault("_readout_plans", {})
    hit = cache.get(x.device)
    if hit is not None and hit[0] is index:
        return hit[1] if hit[1] is not None and hit[1].N == int(x.shape[0]) else None
    seg_ptr = np.asarray(index, dtype=np.int64).reshape(-1)
    ok = seg_ptr.shape[0] == graph.num_graph + 1 and seg_ptr.shape[0] >= 2 and int(seg_ptr[0]) == 0 and not (np.diff(seg_ptr) < 0).any()
    plan = readout_ops.readout_plan(seg_ptr, x.device) if ok else None
    cache[x.device] = (index, plan)
    return plan if plan is not None and plan.N == int(x.shape[0]) else None


class GlobalAttention(nn.Module):
    """pgl/nn/pool.py:148-179: softmax over each graph's nodes of gate(x), weighted sum of nn(x).

    fused=True: the segment softmax of the gate, the product with nn(x) and the segment sum run as ONE streaming kernel
    (pgl_amd.readout_ops.attention_readout, csrc/readout.hip) that reads nn(x) once and writes only [num_graphs, d] and the
    per-graph (max, sum); the backward is one more launch that recomputes the weights.  No host read, no [N, .] temporary, bit
    reproducible.  Taken when `_takes_fused` holds: nn(x) is a CUDA fp32 [N, d <= 512] tensor and the graph is a tensor graph
    whose _graph_node_index is a host array (Graph.disjoint's); every other call runs the unfused code.  Use it for batched
    graph classification, where the chain of small launches and its host read dominate, and for one large graph, where the
    chain moves [N, d] through memory several times.
    Measured (one MI355X, median of 5, batches of 128 x 30 / 4096 x 64 / 64 x 4000 nodes and one graph of 2**20 nodes, d = 64 and
    128; profiles/readout/README.md): forward 1.57-5.21x, forward + backward 1.23-1.63x ahead of fused=False; no row loses, of the layer or of
    the bare op (whose smallest margin, 1.22x, is the gate-mode forward on long graphs)."""

    def __init__(self, gate, nn=None, fused=False):
        super(GlobalAttention, self).__init__()
        self.gate = gate
        self.nn = nn
        self.fused = fused

    def _takes_fused(self, graph, x):
        """x: the features the read-out sums (nn(x) when the layer has an nn)."""
        return _readout_plan(graph, x, self.fused) is not None

    def forward(self, graph, x):
        gate_x = self.gate(x).reshape(-1, 1)
        x = self.nn(x) if self.nn else x
        assert x.dim() == gate_x.dim() and x.shape[0] == gate_x.shape[0]
        plan = _readout_plan(graph, x, self.fused and gate_x.dtype == torch.float32)
        if plan is not None:
            from .. import readout_ops
            return readout_ops.attention_readout(x, plan, score=gate_x.reshape(-1))
        graph_id = graph.graph_node_id
        gate_x = gmath.segment_softmax(gate_x, graph_id)
        return gmath.segment_sum(gate_x * x, graph_id)


class Set2Set(nn.Module):
    """pgl/nn/pool.py:96-145.  n_iters rounds of: LSTM step -> query q per graph, attention of every node to its graph's
    query (segment softmax of <x, q>), read-out r = segment sum of the attended features; output [num_graphs, 2 * dim] =
    (q, r) of the last round.  As the reference computes it, the LSTM *input* stays the initial zero query in every round
    (its loop assigns the new query to a fresh name); only the recurrent state carries over.  Kept for parity.

    fused=True: since the LSTM never sees a read-out, only the LAST round's read-out reaches the output -- the earlier ones are
    computed and thrown away by the reference and by the unfused code.  The fused path runs the LSTM n_iters times as before and
    the read-out ONCE, for the last round's q, as one streaming kernel (pgl_amd.readout_ops.attention_readout in query mode: the
    row dot, the segment softmax, the product and the segment sum in one pass over x; csrc/readout.hip), and takes the number of
    graphs from the plan instead of reading graph_id.max() back.  Taken when `_takes_fused` holds (x a CUDA fp32 [N, d <= 512]
    tensor, a tensor graph whose _graph_node_index is a host array) and n_iters > 0; every other call runs the unfused code.
    The fused output has one row per member graph of the plan (num_graph rows); the unfused code counts graph_id.max() + 1, so with
    EMPTY member graphs at the end of the batch it returns fewer rows -- the fused path returns their rows too, (q, 0).
    Measured (the same shapes, n_iters = 3; profiles/readout/README.md): forward 2.05-3.05x, forward + backward 1.67-4.43x ahead of fused=False on
    the three batches, 1.35 ms against 624 ms forward + backward on the graph of 2**20 nodes; no row loses."""

    def __init__(self, input_dim, n_iters, n_layers=1, fused=False):
        super(Set2Set, self).__init__()
        self.input_dim, self.output_dim = input_dim, 2 * input_dim
        self.n_iters, self.n_layers = n_iters, n_layers
        self.fused = fused
        self.lstm = nn.LSTM(input_size=self.output_dim, hidden_size=input_dim, num_layers=n_layers)     # time-major

    def _takes_fused(self, graph, x):
        return self.n_iters > 0 and _readout_plan(graph, x, self.fused) is not None

    def forward(self, graph, x):
        plan = _readout_plan(graph, x, self.fused) if self.n_iters > 0 else None
        if plan is not None:
            return self._forward_fused(x, plan)
        graph_id = graph.graph_node_id
        batch = int(graph_id.max().item()) + 1
        state = (x.new_zeros((self.n_layers, batch, self.input_dim)), x.new_zeros((self.n_layers, batch, self.input_dim)))
        q_in = x.new_zeros((1, batch, self.output_dim))
        out = x.new_zeros((batch, self.output_dim))
        gid = graph_id.long()
        for _ in range(self.n_iters):
            q, state = self.lstm(q_in, state)
            q = q.reshape(batch, self.input_dim)
            e = (x * q[gid]).sum(dim=-1, keepdim=True)
            a = gmath.segment_softmax(e, graph_id, num_segments=batch)
            r = gmath.segment_sum(a * x, graph_id, num_segments=batch)
            out = torch.cat([q, r], dim=-1)
        return out

    def _forward_fused(self, x, plan):
        from .. import readout_ops
        batch = plan.S
        state = (x.new_zeros((self.n_layers, batch, self.input_dim)), x.new_zeros((self.n_layers, batch, self.input_dim)))
        q_in = x.new_zeros((1, batch, self.output_dim))
        for _ in range(self.n_iters):
            q, state = self.lstm(q_in, state)
        q = q.reshape(batch, self.input_dim)
        return torch.cat([q, readout_ops.attention_readout(x, plan, query=q)], dim=-1)


class SAGPool(nn.Module):
    """pgl/nn/pool.py:182-262.  A one-channel graph convolution scores every node; each member graph keeps its top
    ceil(ratio * n) nodes (or, with min_score, the nodes whose per-graph softmax score exceeds it), features gated by the
    score; edges between dropped nodes are removed.  -> (x', graph_node_id', pooled Graph)."""

    def __init__(self, input_dim, ratio=0.5, gnn=None, min_score=None, nonlinearity=None):
        super(SAGPool, self).__init__()
        from .conv import GCNConv
        self.input_dim, self.ratio, self.min_score = input_dim, ratio, min_score
        self.gnn = (GCNConv if gnn is None else gnn)(input_dim, 1)
        self.nonlinearity = torch.tanh if nonlinearity is None else nonlinearity

    def _host_plan(self, graph, x):
        """(seg_ptr, out_ptr) as host int64 arrays when the pooling kernels take this forward, else None.  Everything comes from
        the batched graph's host-side _graph_node_index: no device read."""
        import numpy as np
        from .. import pool_ops
        index = graph._graph_node_index
        if not (pool_ops._ROUTE and self.min_score is None and x.is_cuda and graph.is_tensor()) or index is None:
            return None
        if isinstance(index, torch.Tensor) and index.is_cuda:         # a caller's own device tensor: reading it would be a host read
            return None
        seg_ptr = np.asarray(index, dtype=np.int64).reshape(-1)
        lens = np.diff(seg_ptr)
        if seg_ptr.shape[0] != graph.num_graph + 1 or int(seg_ptr[-1]) != int(x.shape[0]) or not lens.size or (lens < 0).any():
            return None
        k = pool_ops.topk_counts(lens, self.ratio)
        if not pool_ops.topk_supported(lens.max()) or (k < 0).any() or (k > lens).any() or not k.any():
            return None
        return seg_ptr, np.concatenate([np.zeros(1, np.int64), np.cumsum(k, dtype=np.int64)])

    def forward(self, graph, x):
        from ..graph import Graph
        from ..utils.transform import filter_adj
        batch = graph.graph_node_id
        score = self.gnn(graph, x).reshape(-1)
        if self.min_score is None:
            score = self.nonlinearity(score)
        else:
            score = gmath.segment_softmax(score.reshape(-1, 1), batch).reshape(-1)
        plan = self._host_plan(graph, x)
        if plan is not None:
            return self._forward_device(graph, x, score, batch, plan)
        kept, rank = gmath.segment_topk(x, score, batch, self.ratio, self.min_score, return_index=True)
        x = kept * score[rank].reshape(-1, 1)
        batch = batch[rank]
        edges, _ = filter_adj(graph.edges, rank, num_nodes=score.shape[0])
        n_graph = graph.num_graph
        counts = torch.bincount(batch.long(), minlength=n_graph)
        node_index = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int64).cpu().numpy()     # host-side bookkeeping
        g = Graph(num_nodes=int(x.shape[0]), edges=edges, node_feat={"attr": x}, _graph_node_index=node_index,
                  _num_graph=int(batch.max().item()) + 1)
        return x, batch, g

    def _forward_device(self, graph, x, score, batch, plan):
        """The ratio branch on the pooling kernels (csrc/pool.hip): the same four results, one host read (the kept-edge count)."""
        import numpy as np
        from ..graph import Graph
        from .. import pool_ops
        seg_ptr, out_ptr = plan
        dev = score.device
        rank = pool_ops.topk_perm(score.detach().float(), torch.from_numpy(seg_ptr).to(dev), torch.from_numpy(out_ptr).to(dev),
                                  int(out_ptr[-1]))
        x = x[rank] * score[rank].reshape(-1, 1)
        batch = batch[rank]
        edges = graph.edges
        if edges.dtype != torch.int64:
            edges = edges.long()
        edges, _ = pool_ops.filter_edges(edges, rank, int(score.shape[0]))
        g = Graph(num_nodes=int(x.shape[0]), edges=edges, node_feat={"attr": x}, _graph_node_index=out_ptr,
                  _num_graph=int(np.flatnonzero(np.diff(out_ptr))[-1]) + 1)
        return x, batch, g
