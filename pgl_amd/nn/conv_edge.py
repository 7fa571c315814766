"""The reference's molecular layers with a bond embedding in the message (engine extension; both are new names):
GINEConv (ogb_examples/lsc/PCQM4M/conv.py:27-65) and GENConv (examples/kddcup2021/PCQM4M/models/layers.py:23-113, without its
`concat` branch), over Graph.send_edge_message (csrc/edge_message.hip)."""
import torch
import torch.nn as nn

from .. import message_ops
from .conv import _act, _linear


class _EdgeMessageLayer(nn.Module):
    """The bond tables (edge_vocab given: one [V_f, d] table per categorical edge feature, their rows summed per edge as the
    reference's BondEncoder does, mol_encoder.py:42-58) and the route of the message.  fused=True (the default): Graph.send_edge_message,
    one kernel each way where message_ops.edge_message_supported holds and its own composition elsewhere; fused=False: always the
    composition (message_ops.edge_message_composed), the same definition from torch ops."""

    def _init_edges(self, d, edge_vocab, fused):
        self.fused = bool(fused)
        self.edge_vocab = None if edge_vocab is None else tuple(int(v) for v in edge_vocab)
        self.bond_tables = None
        if self.edge_vocab is not None:
            self.bond_tables = nn.ParameterList([nn.Parameter(nn.init.xavier_uniform_(torch.empty(v, d))) for v in self.edge_vocab])

    def _message(self, graph, x, edge_feat, act, reduce_op, eps, t):
        coded = self.bond_tables is not None
        tables = list(self.bond_tables) if coded else None
        if self.fused:
            return graph.send_edge_message(x, None if coded else edge_feat, edge_feat if coded else None, tables, act, reduce_op, eps, t)
        table, offsets, _ = message_ops.stack_tables(tables) if coded else (None, None, None)
        edges = torch.as_tensor(graph.edges, device=x.device).long()
        return message_ops.edge_message_composed(x, edges[:, 0], edges[:, 1], graph.num_nodes, None if coded else edge_feat,
                                                 edge_feat if coded else None, table, offsets, act, reduce_op, eps, t)


class GINEConv(_EdgeMessageLayer):
    """out = MLP((1 + eps) x + sum_{k = (u -> v)} relu(x[u] + e_k)), MLP = Linear, BatchNorm1d, ReLU, Linear (lsc/PCQM4M/conv.py:35-65).
    edge_vocab=(5, 6, 2): the layer owns the bond tables and forward's edge_feat holds the int codes [E, 3]; edge_vocab=None: edge_feat is
    a dense fp32 [E, input_size].  Timings: profiles/edge_message/README.md."""

    def __init__(self, input_size, output_size, edge_vocab=None, activation=None, init_eps=0.0, train_eps=False, fused=True):
        super(GINEConv, self).__init__()
        self._init_edges(input_size, edge_vocab, fused)
        self.linear1 = _linear(input_size, output_size)
        self.norm = nn.BatchNorm1d(output_size)
        self.linear2 = _linear(output_size, output_size)
        self.epsilon = nn.Parameter(torch.full((1, 1), float(init_eps))) if train_eps else float(init_eps)
        self.activation = _act(activation)

    def forward(self, graph, feature, edge_feat):
        neigh = self._message(graph, feature, edge_feat, "relu", "sum", 0.0, 1.0)
        out = self.linear2(torch.relu(self.norm(self.linear1(neigh + feature * (self.epsilon + 1.0)))))
        return out if self.activation is None else self.activation(out)


class GENConv(_EdgeMessageLayer):
    """out = MLP(x + sum_k softmax_k(t m_k) m_k), m_k = act(x[u] + e_k) + eps, the softmax per channel over the in-edges
    (kddcup2021/PCQM4M/models/layers.py:73-113); MLP: hidden -> 2 hidden -> ... -> hidden over mlp_layers linears, BatchNorm1d and ReLU
    between them.  learn_t: the temperature is a parameter (its value is read on the host once per fused forward).  edge_vocab as in
    GINEConv."""

    def __init__(self, hidden_size, edge_vocab=None, act="swish", eps=1e-7, init_t=1.0, learn_t=False, mlp_layers=2, fused=True):
        super(GENConv, self).__init__()
        self._init_edges(hidden_size, edge_vocab, fused)
        self.act, self.eps = act, float(eps)
        self.t = nn.Parameter(torch.full((1,), float(init_t))) if learn_t else float(init_t)
        widths = [hidden_size] + [2 * hidden_size] * (mlp_layers - 1) + [hidden_size]
        mods = []
        for i in range(len(widths) - 1):
            mods.append(_linear(widths[i], widths[i + 1]))
            if i + 2 < len(widths):
                mods += [nn.BatchNorm1d(widths[i + 1]), nn.ReLU()]
        self.mlp = nn.Sequential(*mods)

    def forward(self, graph, feature, edge_feat):
        return self.mlp(feature + self._message(graph, feature, edge_feat, self.act, "softmax", self.eps, self.t))
