"""Front end of the fused edge-feature messages (csrc/edge_message.hip; pglamd_edge_message / _backward, include/pgl_amd.h): per edge
k = (u -> v)
    pre_k = x[u] + e_k        m_k = act(pre_k) + eps        act = "relu" | "swish" (z * sigmoid(z))
    reduce "sum":      out[v, c] = sum_k m_k[c]                              (GINE: ogbg_molpcba/model.py:266-273, lsc/PCQM4M/conv.py:46-50)
    reduce "softmax":  out[v, c] = sum_k softmax_k(t * m_k[c]) * m_k[c]      (GENConv: kddcup2021/PCQM4M/models/layers.py:73-90)
with the softmax over the in-edges of v, every channel on its own.  e_k is row k of a dense ef [E, d] (original edge order) or, coded,
sum_f table[offsets[f] + codes[k, f]] over f = 0 .. F - 1 in that order (the BondEncoder of mol_encoder.py:42-58, its vocabularies
stacked into one table).  A module of its own beside pgl_amd.ops, whose launch helpers it uses."""
import ctypes

import torch

from . import ops
from .ops import _aligned, _launch, _need_cuda, _ptr, _scratch, _ws_hot

ACT = {"relu": 0, "swish": 1}
REDUCE = {"sum": 0, "softmax": 1}
MAX_D = 1024
MAX_FEATS = 4
LDS_FLOATS = 4080           # table_rows * tile columns the backward's four per-wave gradient copies leave room for in 64 KB of LDS


def _tile_cols(d):
    return min(d, 64 * (4 if d % 4 == 0 else 2 if d % 2 == 0 else 1))


def edge_message_supported(d, table_rows=0):
    """True when the kernels take rows of d floats (1 <= d <= 1024) and, coded, a stacked table of table_rows rows: the forward's LDS copy
    of a column tile and the backward's four gradient copies of it fit 64 KB -- table_rows * min(d, 256) <= 4080 when 4 divides d (15
    rows at d >= 256, 40 at d = 100)."""
    d, table_rows = int(d), int(table_rows)
    return 1 <= d <= MAX_D and table_rows >= 0 and table_rows * _tile_cols(d) <= LDS_FLOATS


def stack_tables(edge_tables):
    """A list of F tensors [V_f, d] -> (stacked table [sum V_f, d], offsets, vocabulary sizes)."""
    sizes = [int(t.shape[0]) for t in edge_tables]
    offsets = [sum(sizes[:f]) for f in range(len(sizes))]
    return (edge_tables[0] if len(edge_tables) == 1 else torch.cat(list(edge_tables), 0)), offsets, sizes


def _operands(what, x, ef, codes, table, offsets, sizes, act, reduce, eps, t, indices, check_range, extra=()):
    """Checks before any launch -> (n, d, x, ef, codes, table, offsets array or None)."""
    if act not in ACT or reduce not in REDUCE:
        raise ValueError("%s: act must be one of %s and reduce one of %s, got %r / %r" % (what, sorted(ACT), sorted(REDUCE), act, reduce))
    if not float(eps) >= 0.0 or (reduce == "softmax" and not float(t) > 0.0):
        raise ValueError("%s: eps must be >= 0 and the temperature > 0, got %r / %r" % (what, eps, t))
    if (ef is None) == (codes is None):
        raise ValueError("%s: exactly one of ef and codes must be given" % what)
    floats = [("x", x)] + ([("ef", ef)] if ef is not None else [("table", table)]) + list(extra)
    for name, v in floats:
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() != 2:
            raise TypeError("%s: %s must be a float32 [rows, d] tensor, got %s" % (what, name, getattr(v, "dtype", type(v))))
    _need_cuda(*(v for _, v in floats), codes)
    n, d = int(x.shape[0]), int(x.shape[1])
    if not 1 <= d <= MAX_D:
        raise ValueError("%s: d = %d must be in 1 .. %d" % (what, d, MAX_D))
    if any(int(v.shape[1]) != d for _, v in floats):
        raise ValueError("%s: every float operand must have d = %d columns" % (what, d))
    for csr in indices:
        if csr.y_rows != 0:
            raise ValueError("%s: an index over a subset of a graph's edges (y_rows = %d) is not supported" % (what, csr.y_rows))
        if csr.num_nodes != n:
            raise ValueError("%s: x holds %d rows, the index %d nodes (bipartite operands are not supported)" % (what, n, csr.num_nodes))
    E = indices[0].num_edges
    off = None
    if ef is not None:
        if int(ef.shape[0]) != E:
            raise ValueError("%s: ef holds %d rows, the index %d edges" % (what, int(ef.shape[0]), E))
    else:
        if not isinstance(codes, torch.Tensor) or codes.dtype not in (torch.int32, torch.int64) or codes.dim() != 2 or int(codes.shape[0]) != E:
            raise TypeError("%s: codes must be an int32 [num_edges, F] = [%d, F] tensor" % (what, E))
        F, T = int(codes.shape[1]), int(table.shape[0])
        if not 1 <= F <= MAX_FEATS or len(offsets) != F or len(sizes) != F:
            raise ValueError("%s: 1 <= F <= %d features with one offset and one vocabulary each, got F = %d" % (what, MAX_FEATS, F))
        if any(o < 0 or s < 1 or o + s > T for o, s in zip(offsets, sizes)):
            raise ValueError("%s: a vocabulary (offset %s, size %s) leaves the table of %d rows" % (what, list(offsets), list(sizes), T))
        if not edge_message_supported(d, T):
            raise ValueError("%s: a table of %d rows at d = %d does not fit the LDS budget (edge_message_supported)" % (what, T, d))
        if check_range and E:
            hi = torch.as_tensor(sizes, device=codes.device)
            if bool(((codes < 0) | (codes >= hi)).any()):
                raise ValueError("%s: a code outside its vocabulary (sizes %s)" % (what, list(sizes)))
        codes = codes.to(torch.int32).contiguous()
        off = (ctypes.c_int32 * F)(*[int(o) for o in offsets])
    return n, d, _aligned(x), _aligned(ef), codes, _aligned(table), off


def edge_message_aggregate(x, csr, ef=None, codes=None, table=None, offsets=None, sizes=None, act="relu", reduce="sum", eps=0.0, t=1.0,
                           return_stats=False, check_range=True):
    """out [N, d] of the module text in one walk of the dst-sorted `csr` (pglamd_edge_message).  x fp32 [N, d]; ef fp32 [E, d] in original
    edge order, or codes int32 [E, F] with the stacked table [T, d], offsets and vocabulary sizes (stack_tables).  return_stats: (out,
    lse) with lse [N, d] = max + log(sum) of t * m_k for the softmax (None for the sum).  ValueError / TypeError before any launch for
    other dtypes or shapes, F > 4, d > 1024, a table beyond edge_message_supported and (check_range: one host read) a code outside its
    vocabulary."""
    n, d, x, ef, codes, table, off = _operands("edge_message_aggregate", x, ef, codes, table, offsets, sizes, act, reduce, eps, t, (csr,), check_range)
    out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    lse = torch.empty((n, d), dtype=torch.float32, device=x.device) if reduce == "softmax" else None
    if n:
        ws = _scratch(_ws_hot, "edge_message", x, csr.num_edges, d, REDUCE[reduce])
        _launch("edge_message", x, _ptr(x), _ptr(ef), _ptr(codes), _ptr(table), off, 0 if codes is None else int(codes.shape[1]),
                0 if table is None else int(table.shape[0]), d, ACT[act], REDUCE[reduce], float(eps), float(t), _ptr(csr.row32), _ptr(csr.col32),
                _ptr(csr.eid32), _ptr(csr.indptr), csr.num_edges, n, _ptr(out), _ptr(lse), _ptr(ws), ws.numel())
    return (out, lse) if return_stats else out


def edge_message_backward(grad_out, x, csr_src, out=None, lse=None, ef=None, codes=None, table=None, offsets=None, sizes=None, act="relu",
                          reduce="sum", eps=0.0, t=1.0, need=(True, True, True)):
    """Backward of edge_message_aggregate in one walk of the src-sorted index -> (dx [N, d], d ef [E, d] or d table [T, d], dt [1]), each
    None where `need` (x, ef / table, t) says not wanted or the call has no such operand (pglamd_edge_message_backward).  out and lse: the
    forward's, for the softmax.  The codes were range-checked by the forward."""
    extra = [("grad_out", grad_out)] + ([("out", out), ("lse", lse)] if reduce == "softmax" else [])
    n, d, x, ef, codes, table, off = _operands("edge_message_backward", x, ef, codes, table, offsets, sizes, act, reduce, eps, t, (csr_src,), False, extra)
    if any(tuple(v.shape) != (n, d) for _, v in extra):
        raise ValueError("edge_message_backward: grad_out, out and lse must be [N, d] = [%d, %d]" % (n, d))
    want_x, want_e, want_t = (bool(v) for v in need)
    want_t = want_t and reduce == "softmax"
    if not (want_x or want_e or want_t):
        return None, None, None
    grad_out = _aligned(grad_out); out = _aligned(out) if reduce == "softmax" else None; lse = _aligned(lse) if reduce == "softmax" else None
    E = csr_src.num_edges
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    dx = new(n, d) if want_x else None
    de = new(E, d) if (want_e and ef is not None) else None
    dtab = new(int(table.shape[0]), d) if (want_e and codes is not None) else None
    dt = new(1) if want_t else None
    T = 0 if table is None else int(table.shape[0])
    ws = _scratch(_ws_hot, "edge_message_backward", x, E, d, T)
    _launch("edge_message_backward", x, _ptr(grad_out), _ptr(x), _ptr(ef), _ptr(codes), _ptr(table), off, 0 if codes is None else int(codes.shape[1]),
            T, d, ACT[act], REDUCE[reduce], float(eps), float(t), _ptr(out), _ptr(lse), _ptr(csr_src.row32), _ptr(csr_src.col32), _ptr(csr_src.eid32),
            _ptr(csr_src.indptr), E, n, _ptr(dx), _ptr(de), _ptr(dtab), _ptr(dt), _ptr(ws), ws.numel())
    return dx, (de if ef is not None else dtab), dt


def edge_message_composed(x, src, dst, n, ef=None, codes=None, table=None, offsets=None, act="relu", reduce="sum", eps=0.0, t=1.0):
    """The same definition from torch ops on any device and dtype (an embedding sum, gathers, index_add): what Graph.send_edge_message
    answers with where the kernels do not take the call, and the `fused=False` side of the layers."""
    if ef is None:
        ef = table[codes[:, 0].long() + offsets[0]]
        for f in range(1, codes.shape[1]):
            ef = ef + table[codes[:, f].long() + offsets[f]]
    pre = x[src] + ef
    m = (torch.relu(pre) if act == "relu" else pre * torch.sigmoid(pre)) + eps
    zeros = lambda: torch.zeros((n, x.shape[1]), dtype=m.dtype, device=m.device)
    if reduce == "sum" or m.shape[0] == 0:
        return zeros().index_add_(0, dst, m)
    idx = dst[:, None].expand_as(m)
    l = t * m
    mx = torch.full_like(zeros(), float("-inf")).scatter_reduce_(0, idx, l.detach(), "amax", include_self=True)
    w = torch.exp(l - mx[dst])
    den = zeros().index_add_(0, dst, w)
    return zeros().index_add_(0, dst, w * m) / den.clamp_min(torch.finfo(m.dtype).tiny)
