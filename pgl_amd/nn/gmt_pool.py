"""Graph Multiset Transformer read-out (pgl/nn/gmt_pool.py:28-291): attention blocks over the dense [batch, max_nodes, dim]
view of a batched graph; the graph-aware block takes its keys / values from a graph convolution (the message-passing
kernels), everything else is dense attention.  The arithmetic follows the reference line by line where it departs from
the paper (softmax over the QUERY axis, the first LayerNorm applied twice), so that its parameters give its outputs.

fused=True (MAB, PMA, GraphMultisetTransformer; opt-in, the default path is unchanged): the attention of the two POOLING blocks runs as
one streaming kernel per direction (pgl_amd.readout_ops.seed_attention_readout, csrc/seed_readout.hip) over the [N, dim] rows as
they are -- no dense view, no head reshuffle, no bmm, nothing saved but the inputs.

fused_dense (MAB) / fused=True (SAB) / fused_self_att=True (GraphMultisetTransformer; a second opt-in, the default path is unchanged): the
dense attention of `MAB.forward` -- SelfAtt's per-graph queries -- runs as one MFMA kernel per direction
(pgl_amd.readout_ops.set_attention, csrc/set_attention.hip) on the projected [B, n, dim] Q / K / V: no head reshuffle, no bmm, no
[B h, n, n] weights, nothing saved but the inputs.  The two flags are independent: `fused` reaches the pooling blocks only."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils.transform import to_dense_batch

__all__ = ["GraphMultisetTransformer", "MAB", "SAB", "PMA"]


class MAB(nn.Module):
    """pgl/nn/gmt_pool.py:28-112.  Multi-head attention block: Q from a Linear, K / V from Linears or, when a graph is
    given, from two graph convolutions over the node features (then densified).

    fused: used by PMA, whose queries are the same seeds for every graph (`seed_forward`); `forward` itself never reads it.
    fused_dense (an attribute, off by default): `forward` runs its attention core -- the four head reshuffles, the two bmm and the
    softmax -- on pgl_amd.readout_ops.set_attention when the projected Q / K / V are CUDA fp32, autocast is off and
    set_attention_supported holds (sets of <= 128 rows, dim <= 256 with a power-of-two head width >= 4); the dense mask [1, B, n] goes
    in as key_bias [B, n]; `_tail` follows unchanged.  Every other call runs the lines below, bit for bit."""

    def __init__(self, dim_Q, dim_K, dim_V, num_heads, conv=None, layer_norm=False, fused=False):
        super(MAB, self).__init__()
        self.dim_V, self.num_heads, self.layer_norm, self.fused = dim_V, num_heads, layer_norm, fused
        self.fused_dense = False
        self._uniform_plans = {}
        self.proj_q = nn.Linear(dim_K, dim_V)
        make = nn.Linear if conv is None else conv
        self.layer_k = make(dim_K, dim_V)
        self.layer_v = make(dim_K, dim_V)
        if layer_norm:
            self.ln0 = nn.LayerNorm(dim_V)
            self.ln1 = nn.LayerNorm(dim_V)
        self.proj_o = nn.Linear(dim_V, dim_V)

    def forward(self, Q, K, graph=None, mask=None):
        Q = self.proj_q(Q)
        if graph is not None:
            g, x = graph
            K, _ = to_dense_batch(self.layer_k(g, x), g)
            V, _ = to_dense_batch(self.layer_v(g, x), g)
        else:
            K, V = self.layer_k(K), self.layer_v(K)
        h = self.num_heads
        if self.fused_dense and self._takes_dense(Q, K, V):
            from .. import readout_ops
            bias = None if mask is None else mask.reshape(K.shape[0], K.shape[1]).to(torch.float32)
            return self._tail(readout_ops.set_attention(Q, K, V, h, key_bias=bias))
        heads = lambda t: torch.cat(t.chunk(h, dim=2), dim=0)            # [batch*h, n, dim_V / h]
        Qh, Kh, Vh = heads(Q), heads(K), heads(V)
        score = torch.bmm(Qh, Kh.transpose(1, 2)) / math.sqrt(self.dim_V)
        if mask is not None:
            m = torch.cat([mask] * h, dim=0).reshape(Kh.shape[0], Kh.shape[1]).unsqueeze(1)
            score = m + score
        A = F.softmax(score, dim=1)
        out = torch.cat((Qh + torch.bmm(A, Vh)).chunk(h, dim=0), dim=2)
        return self._tail(out)

    def _takes_dense(self, Q, K, V):
        """True when the set-attention kernel takes the projected operands of `forward`."""
        from .. import readout_ops
        return (all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 for t in (Q, K, V)) and not torch.is_autocast_enabled()
                and K.shape == V.shape and Q.shape[0] == K.shape[0] and Q.shape[0] >= 1
                and readout_ops.set_attention_supported(Q.shape[1], K.shape[1], self.dim_V, self.num_heads))

    def _tail(self, out):
        if self.layer_norm:
            out = self.ln0(out)
        out = out + F.relu(self.proj_o(out))
        if self.layer_norm:
            out = self.ln0(out)
        return out

    def _seed_plan(self, seeds, x, graph):
        """The read-out plan when the seed-attention kernel takes this call, else None.  Graph-aware block: graph = (g, node features
        [N, dim]) and the plan is the batched graph's (pgl_amd.nn.pool._readout_plan: a tensor graph whose _graph_node_index is a host
        array).  Plain block: x [B, n, dim] and a uniform plan, seg_ptr = arange(B + 1) * n, kept on the module by (B, n, device)."""
        from .. import readout_ops
        from .pool import _readout_plan
        feat = graph[1] if graph is not None else x
        if not (self.fused and isinstance(feat, torch.Tensor) and feat.is_cuda and feat.dtype == torch.float32 and seeds.is_cuda
                and seeds.dtype == torch.float32 and not torch.is_autocast_enabled()
                and readout_ops.seed_readout_supported(seeds.shape[0], self.dim_V, self.num_heads)):
            return None
        if graph is not None:
            return _readout_plan(graph[0], feat, True)
        if feat.dim() != 3 or feat.shape[1] < 1:
            return None
        key = (int(feat.shape[0]), int(feat.shape[1]), feat.device)
        if key not in self._uniform_plans:
            import numpy as np
            self._uniform_plans[key] = readout_ops.readout_plan(np.arange(key[0] + 1, dtype=np.int64) * key[1], feat.device)
        return self._uniform_plans[key]

    def seed_forward(self, seeds, x, graph=None, key_bias=None):
        """forward(seeds expanded over the batch, x, graph) on the seed-attention kernel -> [B, num_seeds, dim_V], or None when
        `_seed_plan` does not take the call (the caller then runs `forward`).  seeds [num_seeds, dim_Q]; key_bias [N]: the per-node
        form of `mask`."""
        plan = self._seed_plan(seeds, x, graph)
        if plan is None:
            return None
        from .. import readout_ops
        Q = self.proj_q(seeds)
        if graph is not None:
            g, nodes = graph
            K, V = self.layer_k(g, nodes), self.layer_v(g, nodes)
        else:
            K, V = self.layer_k(x).reshape(-1, self.dim_V), self.layer_v(x).reshape(-1, self.dim_V)
        return self._tail(readout_ops.seed_attention_readout(K, V, Q, plan, self.num_heads, key_bias=key_bias))


class SAB(nn.Module):
    """pgl/nn/gmt_pool.py:118-157: self-attention of the (pooled) node set.

    fused=True (also settable afterwards): sets `fused_dense` on the block's MAB, whose attention then runs on the set-attention
    kernel (pgl_amd.readout_ops.set_attention) for CUDA fp32 input of <= 128 rows without autocast; every other call runs the unfused
    code.  Measured (one MI355X, median of 5, dim = 128 with 4 heads and dim = 256 with 8, sets x rows = 4096 x 8, 4096 x 32, 1024 x 75,
    512 x 128 and 8 x 128; profiles/set_attention/README.md): forward 1.47-3.53x and forward + backward 1.12-2.46x ahead of fused=False,
    most on many small sets (4096 x 8: 3.3-3.5x / 1.9-2.5x), least at 128 rows (512 x 128: 1.5x / 1.12x).  No row loses.  When to use
    it: whenever the input is CUDA fp32 with sets of <= 128 rows; longer sets and 16-bit input run the unfused code anyway."""

    def __init__(self, input_dim, output_dim, num_heads, conv=None, layer_norm=False, fused=False):
        super(SAB, self).__init__()
        self.mab = MAB(input_dim, input_dim, output_dim, num_heads, conv=conv, layer_norm=layer_norm)
        self.mab.fused_dense = fused

    @property
    def fused(self):
        return self.mab.fused_dense

    @fused.setter
    def fused(self, value):
        self.mab.fused_dense = value

    def forward(self, x, graph, mask):
        return self.mab(x, x, graph, mask)


class PMA(nn.Module):
    """pgl/nn/gmt_pool.py:160-199: pooling by attention from `num_seeds` learned seed vectors.

    fused=True: the seeds are the same for every graph and the softmax runs over the seed axis, so a node's weights depend on that node
    alone and the block's attention is one streaming kernel (pgl_amd.readout_ops.seed_attention_readout) over K, V [N, dim]: with a
    graph (GMPool_G) the two convolutions' outputs as they are, never densified; without one and with `mask is None` (GMPool_I) the
    [B, n, dim] input viewed as B segments of n rows.  The layer norms and the proj_o tail follow unchanged.  Taken when `_takes_fused`
    holds: CUDA fp32 features, no autocast, num_seeds <= 32, dim <= 256 with a power-of-two head width >= 4, and for GMPool_G a tensor
    graph whose _graph_node_index is a host array (Graph.disjoint's); every other call runs the unfused code.  `key_bias` [N] is the
    per-node form of `mask` for GMPool_G (a mask cannot be given with it).  x may be None when the graph-aware block is taken.
    The unfused fall-back (more than 32 seeds, or a mask) is `MAB.forward`: it takes the set-attention kernel only when `fused_dense`
    is set on this block's MAB by hand; neither `fused` nor GraphMultisetTransformer's `fused_self_att` sets it here."""

    def __init__(self, dim, num_heads, num_seeds, conv=None, layer_norm=False, fused=False):
        super(PMA, self).__init__()
        self.Q_S = nn.Parameter(torch.empty(1, num_seeds, dim))
        nn.init.kaiming_uniform_(self.Q_S)
        self.dim, self.num_seeds = dim, num_seeds
        self.mab = MAB(dim, dim, dim, num_heads, conv=conv, layer_norm=layer_norm, fused=fused)

    @property
    def fused(self):
        return self.mab.fused

    @fused.setter
    def fused(self, value):
        self.mab.fused = value

    def _takes_fused(self, x, graph=None, mask=None):
        return mask is None and self.mab._seed_plan(self.Q_S[0], x, graph) is not None

    def forward(self, x, graph, mask, key_bias=None):
        if mask is None:
            out = self.mab.seed_forward(self.Q_S[0], x, graph, key_bias)
            if out is not None:
                return out
        assert key_bias is None, "key_bias belongs to the fused path; the unfused block takes `mask`"
        return self.mab(self.Q_S.expand(x.shape[0], self.num_seeds, self.dim), x, graph, mask)


class GraphMultisetTransformer(nn.Module):
    """pgl/nn/gmt_pool.py:202-291.  lin1 -> [GMPool_G (graph-aware pooling), SelfAtt, GMPool_I (pooling to one vector)] -> lin2.

    fused=True (also settable afterwards: `.fused` reaches every pooling block): GMPool_G and GMPool_I take the seed-attention kernel
    (see PMA); SelfAtt has its own flag, below.  When the first block is a GMPool_G that takes it, the forward never calls to_dense_batch: the
    `-1e9` mask of the nodes whose lin1 output sums to exactly 0 becomes a per-node key_bias (added in fp32 it swallows the score and
    makes that node's weights 1 / num_seeds, as the dense mask does; padding slots do not exist here and contribute V = 0 there), and
    the batch size is the plan's.  The output has one row per member graph of the plan: TRAILING EMPTY member graphs, which the
    dense view may not count, get their rows too (the seeds' own read-out).  Every call `_takes_fused` refuses (CPU or non-fp32
    input, autocast, more than 32 seeds, an unsupported width, a graph whose _graph_node_index is not a host array) runs the unfused
    code, bit for bit what fused=False runs.
    Measured (one MI355X, median of 5, dim = 128, 4 heads, k = 1 / 8 / 32 seeds in GMPool_G, batches of 128 x 30 / 4096 x 64 / 64 x 4000
    nodes, one graph of 2**20 nodes and an uneven batch of 4 x 10 000 among 252 x 30 nodes; profiles/seed_readout/README.md): forward
    1.26-8.28x ahead of fused=False on every row; forward + backward 1.19-3.65x ahead at k = 1 and 8 everywhere and at k = 32 on the
    three batches with short graphs (the uneven batch: 3.0-3.7x, forward 4.6-8.3x).  LOSING ROWS: forward + backward at k = 32 on long
    graphs, 0.97x at 64 x 4000 and 0.90x on the graph of 2**20 nodes -- the top seed tier's backward runs one wave per SIMD on a
    fixed 1024 waves; keep fused=False for training with more than 16 seeds on graphs of thousands of nodes.

    fused_self_att=True (after the reference's arguments, off by default, settable afterwards): every SelfAtt block runs its attention
    on the set-attention kernel (see SAB).  It reaches the SAB blocks only, as `fused` reaches the PMA blocks only; the pooling
    blocks' unfused fall-back is not switched by it."""

    def __init__(self, input_dim, hidden_dim, output_dim, conv=None, num_nodes=30, pooling_ratio=0.25, pool_sequences=None,
                 num_heads=4, layer_norm=False, fused=False, fused_self_att=False):
        super(GraphMultisetTransformer, self).__init__()
        from .conv import GCNConv
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.conv = conv or GCNConv
        self.num_nodes, self.pooling_ratio = num_nodes, pooling_ratio
        self.pool_sequences = ["GMPool_G", "SelfAtt", "GMPool_I"] if pool_sequences is None else pool_sequences
        self.num_heads, self.layer_norm = num_heads, layer_norm
        self.pools = nn.ModuleList()
        self.lin1 = nn.Linear(input_dim, hidden_dim)
        self.lin2 = nn.Linear(hidden_dim, output_dim)
        n_out = math.ceil(num_nodes * pooling_ratio)
        for i, kind in enumerate(self.pool_sequences):
            if kind not in ("GMPool_G", "GMPool_I", "SelfAtt"):
                raise ValueError("Elements in 'pool_sequences' should be one of 'GMPool_G', 'GMPool_I', or 'SelfAtt'")
            if i == len(self.pool_sequences) - 1:
                n_out = 1
            if kind == "SelfAtt":
                self.pools.append(SAB(hidden_dim, hidden_dim, num_heads, conv=None, layer_norm=layer_norm, fused=fused_self_att))
            else:
                self.pools.append(PMA(hidden_dim, num_heads, n_out, conv=self.conv if kind == "GMPool_G" else None,
                                      layer_norm=layer_norm, fused=fused))
                n_out = math.ceil(n_out * pooling_ratio)

    @property
    def fused(self):
        return any(p.fused for p in self.pools if isinstance(p, PMA))

    @fused.setter
    def fused(self, value):
        for p in self.pools:
            if isinstance(p, PMA):
                p.fused = value

    @property
    def fused_self_att(self):
        return any(p.fused for p in self.pools if isinstance(p, SAB))

    @fused_self_att.setter
    def fused_self_att(self, value):
        for p in self.pools:
            if isinstance(p, SAB):
                p.fused = value

    def _takes_fused(self, graph, x):
        """x: the lin1 output.  True when the FIRST block is a GMPool_G on the kernel, i.e. when no dense view is built."""
        return self.pool_sequences[0] == "GMPool_G" and self.pools[0]._takes_fused(None, (graph, x))

    def forward(self, graph, x):
        x = self.lin1(x)
        if self._takes_fused(graph, x):
            key_bias = (x.sum(-1) == 0).to(x.dtype) * -1e9                   # the mask below, per node
            dense, mask = self.pools[0](None, (graph, x), None, key_bias=key_bias), None
            rest = zip(self.pool_sequences[1:], self.pools[1:])
        else:
            dense, _ = to_dense_batch(x, graph)
            mask = (dense.sum(-1) == 0).to(torch.int64).unsqueeze(0) * -1e9  # padding slots (all-zero rows) pushed to -inf
            rest = zip(self.pool_sequences, self.pools)
        for kind, pool in rest:
            dense = pool(dense, (graph, x) if kind == "GMPool_G" else None, mask)
            mask = None
        return self.lin2(dense.squeeze(1))
