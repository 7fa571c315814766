"""Front end of the fused GATv2 attention (csrc/gatv2_attention.hip; pglamd_gatv2_attention / _backward, include/pgl_amd.h) and of
the fused dot-product attention with edge features (csrc/dot_attention.hip; pglamd_dot_attention_edge / _backward).
A module of its own beside pgl_amd.ops, whose launch helpers it uses.  No function here reads a device value back on the host."""
import torch

from . import ops
from .ops import _aligned, _gat_lane_bytes, _launch, _need_cuda, _ptr, _scratch, _seed32, _ws_hot


def gatv2_attention_supported(H, D):
    """True when the fused GATv2 kernels take heads x head_dim: dot_attention's geometry -- one 64-lane tile of 1, 2 or 4 floats
    per lane, every head on a power-of-two span of lanes."""
    return ops.sddmm_supported(int(H), int(D))


def _operands(what, attn, *ts):
    x = ts[0]
    _need_cuda(attn, *ts)
    if x.dim() != 3 or any(t.dtype != torch.float32 or tuple(t.shape) != tuple(x.shape) for t in ts):
        raise TypeError("%s: float32 [N, heads, head_dim] operands of one shape" % what)
    n, H, D = (int(s) for s in x.shape)
    if attn.dtype != torch.float32 or attn.numel() != H * D or tuple(attn.shape[-2:]) != (H, D):
        raise TypeError("%s: attn must be float32 [heads, head_dim] = [%d, %d]" % (what, H, D))
    return n, H, D


def gatv2_attention(x_src, x_dst, attn, csr, negative_slope=0.2, drop_p=0.0, seed=0, return_stats=False):
    """out[i, h] = sum_{e = (u -> i)} keep_e,h softmax_i(sum_d attn[h, d] leaky_relu(x_src[u, h, d] + x_dst[i, h, d])) x_src[u, h] in
    one pass over the edges of the dst-sorted `csr` (pglamd_gatv2_attention).  x_src, x_dst: fp32 [N, H, D]; attn [H, D] (or
    [1, H, D]) -> [N, H, D], or with return_stats (out, row_max [N, H], row_sum [N, H]).  drop_p: attention dropout from
    (seed, original edge id, head), GAT's mask."""
    n, H, D = _operands("gatv2_attention", attn, x_src, x_dst)
    if n != csr.num_nodes:
        raise ValueError("gatv2_attention: x_src, x_dst hold %d rows, the index %d nodes (bipartite operands are not supported)" % (n, csr.num_nodes))
    lane = _gat_lane_bytes(H, D, pow2=True)
    shared = x_src is x_dst
    x_src = _aligned(x_src, lane)
    x_dst = x_src if shared else _aligned(x_dst, lane)
    attn = _aligned(attn, lane)
    out = torch.empty((n, H, D), dtype=torch.float32, device=x_src.device)
    mx = sm = None
    if return_stats:
        mx = torch.empty((n, H), dtype=torch.float32, device=x_src.device)
        sm = torch.empty((n, H), dtype=torch.float32, device=x_src.device)
    if n:
        ws = _scratch(_ws_hot, "gatv2_attention", x_src, csr.num_edges, H, D)
        _launch("gatv2_attention", x_src, _ptr(x_src), _ptr(x_dst), _ptr(attn), H, D, float(negative_slope), float(drop_p), _seed32(seed),
                _ptr(csr.row32), _ptr(csr.col32), _ptr(csr.eid32), _ptr(csr.indptr), csr.num_edges, n, _ptr(out), _ptr(mx), _ptr(sm),
                _ptr(ws), ws.numel())
    return (out, mx, sm) if return_stats else out


def gatv2_attention_backward(grad_out, x_src, x_dst, attn, out, row_max, row_sum, csr_dst, csr_src, negative_slope=0.2, drop_p=0.0, seed=0):
    """Backward of gatv2_attention -> (dx_src [N, H, D], dx_dst [N, H, D], dattn in attn's shape): alpha recomputed per edge from
    (row_max, row_sum), one walk of the dst-sorted and one of the src-sorted index, dattn from per-chunk partials summed in a fixed
    order (pglamd_gatv2_attention_backward)."""
    n, H, D = _operands("gatv2_attention_backward", attn, x_src, x_dst, grad_out, out)
    if n != csr_dst.num_nodes or n != csr_src.num_nodes:
        raise ValueError("gatv2_attention_backward: the operands hold %d rows, the indices %d / %d nodes" % (n, csr_dst.num_nodes, csr_src.num_nodes))
    lane = _gat_lane_bytes(H, D, pow2=True)
    shared = x_src is x_dst
    x_src = _aligned(x_src, lane)
    x_dst = x_src if shared else _aligned(x_dst, lane)
    a = _aligned(attn, lane)
    # (grad_out and out also feed the pack kernel's 16-byte loads)
    grad_out = _aligned(grad_out, 16); out = _aligned(out, 16)
    row_max = row_max.contiguous(); row_sum = row_sum.contiguous()
    dxs, dxd = (torch.empty((n, H, D), dtype=torch.float32, device=x_src.device) for _ in range(2))
    if not n:
        return dxs, dxd, torch.zeros_like(attn)
    da = torch.empty(tuple(attn.shape), dtype=torch.float32, device=x_src.device)
    ws = _scratch(_ws_hot, "gatv2_attention_backward", x_src, csr_dst.num_edges, n, H, D)
    _launch("gatv2_attention_backward", x_src, _ptr(grad_out), _ptr(x_src), _ptr(x_dst), _ptr(a), _ptr(out), _ptr(row_max), _ptr(row_sum),
            H, D, float(negative_slope), float(drop_p), _seed32(seed), _ptr(csr_dst.row32), _ptr(csr_dst.col32), _ptr(csr_dst.eid32),
            _ptr(csr_dst.indptr), _ptr(csr_src.row32), _ptr(csr_src.col32), _ptr(csr_src.eid32), _ptr(csr_src.indptr),
            csr_dst.num_edges, n, _ptr(dxs), _ptr(dxd), _ptr(da), _ptr(ws), ws.numel())
    return dxs, dxd, da


# ------------------------------------------------------------------------------------------------
# dot-product attention with a per-edge feature on the key and the value (csrc/dot_attention.hip, EDGE)
# ------------------------------------------------------------------------------------------------
def dot_attention_edge_supported(H, D):
    """True when the fused dot-product attention kernels take heads x head_dim with an edge feature: ops.dot_attention_supported's
    geometry (the edge feature is walked in the lanes of q, k and v)."""
    return ops.dot_attention_supported(int(H), int(D))


def _edge_operand(what, ef, H, D, *indices):
    """ef as the kernels read it: fp32 [num_edges, H, D], one row per edge of every index, addressed by the index's own edge ids."""
    _need_cuda(ef)
    if ef.dtype != torch.float32 or ef.dim() != 3 or tuple(ef.shape[1:]) != (H, D):
        raise TypeError("%s: ef must be float32 [num_edges, heads, head_dim] = [*, %d, %d]" % (what, H, D))
    for csr in indices:
        if csr.y_rows != 0:
            raise ValueError("%s: an index over a subset of a graph's edges (y_rows = %d) is not supported" % (what, csr.y_rows))
        if int(ef.shape[0]) != csr.num_edges:
            raise ValueError("%s: ef holds %d rows, the index %d edges" % (what, int(ef.shape[0]), csr.num_edges))


def dot_attention_edge(q, k, v, ef, csr, scale=1.0, drop_p=0.0, seed=0, return_stats=False):
    """out[i, h] = sum_{e = (u -> i)} keep_e,h softmax_i(scale * <q[i, h], k[u, h] + ef[e, h]>) (v[u, h] + ef[e, h]) in one pass over
    the edges of the dst-sorted `csr` (pglamd_dot_attention_edge, include/pgl_amd.h).  q, k, v: fp32 [N, H, D]; ef: fp32
    [csr.num_edges, H, D], row csr.eid32[p] for position p (original edge order for a graph's index; eid32 None: the position)
    -> [N, H, D], or with return_stats (out, row_max [N, H], row_sum [N, H]).  drop_p: attention dropout from (seed, original edge
    id, head), GAT's mask."""
    n, H, D = ops._dot_operands("dot_attention_edge", q, k, v)
    if n != csr.num_nodes:
        raise ValueError("dot_attention_edge: q, k, v hold %d rows, the index %d nodes (bipartite operands are not supported)" % (n, csr.num_nodes))
    _edge_operand("dot_attention_edge", ef, H, D, csr)
    lane = _gat_lane_bytes(H, D, pow2=True)
    q = _aligned(q, lane); k = _aligned(k, lane); v = _aligned(v, lane); ef = _aligned(ef, lane)
    out = torch.empty((n, H, D), dtype=torch.float32, device=q.device)
    mx = sm = None
    if return_stats:
        mx = torch.empty((n, H), dtype=torch.float32, device=q.device)
        sm = torch.empty((n, H), dtype=torch.float32, device=q.device)
    if n:
        ws = _scratch(_ws_hot, "dot_attention_edge", q, csr.num_edges, H, D)
        _launch("dot_attention_edge", q, _ptr(q), _ptr(k), _ptr(v), _ptr(ef), H, D, float(scale), float(drop_p), _seed32(seed),
                _ptr(csr.row32), _ptr(csr.col32), _ptr(csr.eid32), _ptr(csr.indptr), csr.num_edges, n, _ptr(out), _ptr(mx), _ptr(sm),
                _ptr(ws), ws.numel())
    return (out, mx, sm) if return_stats else out


def dot_attention_edge_backward(grad_out, q, k, v, ef, out, row_max, row_sum, csr_dst, csr_src, scale=1.0, drop_p=0.0, seed=0, want_ef=True):
    """Backward of dot_attention_edge -> (dq, dk, dv, def or None): alpha recomputed per edge from (row_max, row_sum), one walk of the
    dst-sorted and one of the src-sorted index, both gathering ef through their own eid32; def [num_edges, H, D] (rows as ef's) is
    stored edge by edge from the src-sorted walk, and not at all with want_ef=False (pglamd_dot_attention_edge_backward)."""
    n, H, D = ops._dot_operands("dot_attention_edge_backward", q, k, v, grad_out, out)
    if n != csr_dst.num_nodes or n != csr_src.num_nodes:
        raise ValueError("dot_attention_edge_backward: the operands hold %d rows, the indices %d / %d nodes" % (n, csr_dst.num_nodes, csr_src.num_nodes))
    _edge_operand("dot_attention_edge_backward", ef, H, D, csr_dst, csr_src)
    lane = _gat_lane_bytes(H, D, pow2=True)
    q = _aligned(q, lane); k = _aligned(k, lane); v = _aligned(v, lane); ef = _aligned(ef, lane)
    # (grad_out and out also feed the pack kernel's 16-byte loads)
    grad_out = _aligned(grad_out, 16); out = _aligned(out, 16)
    row_max = row_max.contiguous(); row_sum = row_sum.contiguous()
    dq, dk, dv = (torch.empty((n, H, D), dtype=torch.float32, device=q.device) for _ in range(3))
    de = torch.empty((csr_dst.num_edges, H, D), dtype=torch.float32, device=q.device) if want_ef else None
    if n:
        ws = _scratch(_ws_hot, "dot_attention_edge_backward", q, csr_dst.num_edges, n, H, D)
        _launch("dot_attention_edge_backward", q, _ptr(grad_out), _ptr(q), _ptr(k), _ptr(v), _ptr(ef), _ptr(out), _ptr(row_max), _ptr(row_sum),
                H, D, float(scale), float(drop_p), _seed32(seed), _ptr(csr_dst.row32), _ptr(csr_dst.col32), _ptr(csr_dst.eid32),
                _ptr(csr_dst.indptr), _ptr(csr_src.row32), _ptr(csr_src.col32), _ptr(csr_src.eid32), _ptr(csr_src.indptr),
                csr_dst.num_edges, n, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(de), _ptr(ws), ws.numel())
    return dq, dk, dv, de
