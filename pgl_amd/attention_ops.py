"""Front end of the fused GATv2 attention (csrc/gatv2_attention.hip; pglamd_gatv2_attention / _backward, include/pgl_amd.h) and of
the fused dot-product attention with edge features (csrc/dot_attention.hip; pglamd_dot_attention_edge / _backward), and of the
fused GAT attention on 16-bit rows (csrc/gat_fused_16.hip; pglamd_gat_aggregate_16 / pglamd_gat_backward_16), and of the fused
frequency-adaptive attention of FAGCN (csrc/fa_attention.hip; pglamd_fa_aggregate / pglamd_fa_backward).
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
# FAGCN's frequency-adaptive attention (csrc/fa_attention.hip): a signed tanh gate, no softmax
# ------------------------------------------------------------------------------------------------
def fa_supported(H, D):
    """True when the fused frequency-adaptive attention kernels take heads x head_dim: sddmm's geometry -- one 64-lane tile of 1, 2 or
    4 floats per lane, every head on a power-of-two span of lanes (the backward's per-head sums)."""
    return ops.sddmm_supported(int(H), int(D))


def _fa_operands(what, x, p_src, p_dst, s_src, s_dst, *like_x):
    """-> (n, H, D, p_src, p_dst, s_src, s_dst) with the gate halves as contiguous [n, H] and the scales as contiguous [n] (or None)."""
    _need_cuda(x, p_src, p_dst, s_src, s_dst, *like_x)
    if x.dim() != 3 or any(t.dtype != torch.float32 or tuple(t.shape) != tuple(x.shape) for t in (x,) + like_x):
        raise TypeError("%s: float32 [N, heads, head_dim] operands of one shape" % what)
    n, H, D = (int(s) for s in x.shape)
    for name, t in (("p_src", p_src), ("p_dst", p_dst)):
        if t.dtype != torch.float32 or tuple(t.shape) != (n, H):
            raise TypeError("%s: %s must be float32 [N, heads] = [%d, %d]" % (what, name, n, H))
    for name, t in (("s_src", s_src), ("s_dst", s_dst)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != n):
            raise TypeError("%s: %s must be float32 with one value per node (%d), or None" % (what, name, n))
    flat = lambda t: None if t is None else t.detach().reshape(n).contiguous()
    return n, H, D, p_src.contiguous(), p_dst.contiguous(), flat(s_src), flat(s_dst)


def fa_aggregate(x, p_src, p_dst, s_src, s_dst, csr, drop_p=0.0, seed=0):
    """out[i, h] = sum_{e = (u -> i)} keep_e,h tanh(p_src[u, h] + p_dst[i, h]) s_src[u] s_dst[i] x[u, h] in one pass over the edges of
    the dst-sorted `csr` (pglamd_fa_aggregate, include/pgl_amd.h).  x: fp32 [N, H, D]; p_src, p_dst: fp32 [N, H]; s_src, s_dst: fp32
    [N] constants or None (= 1) -> [N, H, D].  drop_p: attention dropout from (seed, original edge id, head), GAT's mask."""
    n, H, D, p_src, p_dst, s_src, s_dst = _fa_operands("fa_aggregate", x, p_src, p_dst, s_src, s_dst)
    if n != csr.num_nodes:
        raise ValueError("fa_aggregate: x holds %d rows, the index %d nodes (bipartite operands are not supported)" % (n, csr.num_nodes))
    x = _aligned(x, _gat_lane_bytes(H, D, pow2=True))
    out = torch.empty((n, H, D), dtype=torch.float32, device=x.device)
    if n:
        ws = _scratch(_ws_hot, "fa_aggregate", x, csr.num_edges, H, D)
        _launch("fa_aggregate", x, _ptr(x), _ptr(p_src), _ptr(p_dst), _ptr(s_src), _ptr(s_dst), H, D, float(drop_p), _seed32(seed),
                _ptr(csr.row32), _ptr(csr.col32), _ptr(csr.eid32), _ptr(csr.indptr), csr.num_edges, n, _ptr(out), _ptr(ws), ws.numel())
    return out


def fa_backward(grad_out, x, p_src, p_dst, s_src, s_dst, csr_dst, csr_src, drop_p=0.0, seed=0, need=(True, True, True)):
    """Backward of fa_aggregate -> (dx [N, H, D], dp_src [N, H], dp_dst [N, H]), None where `need` (x, p_src, p_dst) says not wanted:
    one walk of the src-sorted index gives dx and dp_src and stores r_e [E, H] in its own edge order (pglamd_fa_backward); dp_dst is
    the sum of those rows by destination -- ops.aggregate over an edge_rows view of the dst-sorted index, as ops.gat_backward sums
    its edge buffer.  The walk skips what is not needed (the dx store; the per-head sums and the edge buffer) without changing the
    bits of the rest.  Deterministic."""
    n, H, D, p_src, p_dst, s_src, s_dst = _fa_operands("fa_backward", x, p_src, p_dst, s_src, s_dst, grad_out)
    if n != csr_dst.num_nodes or n != csr_src.num_nodes:
        raise ValueError("fa_backward: the operands hold %d rows, the indices %d / %d nodes" % (n, csr_dst.num_nodes, csr_src.num_nodes))
    want_x, want_ps, want_pd = (bool(v) for v in need)
    if not (want_x or want_ps or want_pd):
        return None, None, None
    lane = _gat_lane_bytes(H, D, pow2=True)
    x = _aligned(x, lane); grad_out = _aligned(grad_out, lane)
    dev, E = x.device, csr_src.num_edges
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    dx = new(n, H, D) if want_x else None
    dps = new(n, H) if (want_ps or want_pd) else None             # (the walk forms r_e only together with its sum by source)
    r_edge = new(E, H) if want_pd else None
    if n:
        ws = _scratch(_ws_hot, "fa_backward", x, E, H, D)
        _launch("fa_backward", x, _ptr(grad_out), _ptr(x), _ptr(p_src), _ptr(p_dst), _ptr(s_src), _ptr(s_dst), H, D, float(drop_p),
                _seed32(seed), _ptr(csr_src.row32), _ptr(csr_src.col32), _ptr(csr_src.eid32), _ptr(csr_src.indptr), E, n, _ptr(dx),
                _ptr(dps), _ptr(r_edge), _ptr(ws), ws.numel())
    dpd = None
    if want_pd:                 # rows of the src-sorted edge buffer gathered in dst-sorted order
        if n == 0 or E == 0:
            dpd = torch.zeros((n, H), dtype=torch.float32, device=dev)
        else:
            pos = ops._src_pos_in_dst_order(csr_dst, csr_src)
            dpd = ops.aggregate(r_edge, csr_dst.view(col32=pos, eid32=pos, edge_rows=True), "sum", n)
    return dx, (dps if want_ps else None), dpd


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


# ------------------------------------------------------------------------------------------------
# GAT attention on fp16 / bf16 rows (csrc/gat_fused_16.hip): 16-bit storage, fp32 accumulation
# ------------------------------------------------------------------------------------------------
_DTYPE16 = (torch.float16, torch.bfloat16)


def gat16_supported(H, D, backward=False):
    """True when pglamd_gat_aggregate_16 (backward: pglamd_gat_backward_16) takes heads x head_dim: the fp32 kernels' geometry -- one
    64-lane tile of 1, 2 or 4 elements of one head per lane; the backward wants every head on a power-of-two span of lanes."""
    H, D = int(H), int(D)
    if H < 1 or D < 1 or H > 64:
        return False
    for v in (1, 2, 4):
        lph = D // v
        if D % v == 0 and H * D <= 64 * v and not (backward and lph & (lph - 1)):
            return True
    return False


def _lane_bytes16(H, D, pow2=False):
    """_gat_lane_bytes in bytes of a 16-bit element: the same lane of 1, 2 or 4 elements, half as many bytes."""
    return _gat_lane_bytes(H, D, pow2) // 2


def _scores(what, n, H, attn_src, attn_dst):
    attn_src = attn_src.to(torch.float32).contiguous(); attn_dst = attn_dst.to(torch.float32).contiguous()
    if tuple(attn_src.shape) != (n, H) or attn_dst.dim() != 2 or attn_dst.shape[1] != H:
        raise ValueError("%s: attn_src/attn_dst must be [N, heads]" % what)
    return attn_src, attn_dst


def gat_aggregate16(feature, attn_src, attn_dst, csr, negative_slope=0.2, out_size=None, return_stats=False, drop_p=0.0, seed=0):
    """ops.gat_aggregate on 16-bit rows: feature [N, H, D] fp16 or bf16, attn_* [N, H] (taken to fp32) -> out [M, H, D] in feature's
    dtype, or with return_stats (out, row_max, row_sum, out_pos, sum_pos): out_pos in feature's dtype, the statistics fp32.  The sums
    run in fp32 in the fp32 kernel's order and are rounded once: the result is ops.gat_aggregate(feature.float(), ...) rounded to
    feature's dtype, bit for bit, and the statistics are that call's bits (pglamd_gat_aggregate_16, include/pgl_amd.h)."""
    _need_cuda(feature, attn_src, attn_dst)
    if feature.dtype not in _DTYPE16 or feature.dim() != 3:
        raise TypeError("gat_aggregate16: feature must be float16 or bfloat16 [N, heads, head_dim]")
    n, H, D = (int(v) for v in feature.shape)
    feature = _aligned(feature, _lane_bytes16(H, D))
    attn_src, attn_dst = _scores("gat_aggregate16", n, H, attn_src, attn_dst)
    M = ops._rows_out(out_size, n)
    dev = feature.device
    out = torch.empty((M, H, D), dtype=feature.dtype, device=dev)
    mx = sm = out_pos = s_pos = None
    if return_stats:
        mx = torch.empty((M, H), dtype=torch.float32, device=dev)
        sm = torch.empty((M, H), dtype=torch.float32, device=dev)
        if ops._GAT_POS_STATS:
            out_pos = torch.empty((M, H, D), dtype=feature.dtype, device=dev)
            s_pos = torch.empty((M, H), dtype=torch.float32, device=dev)
    if M == 0:
        return (out, mx, sm, out_pos, s_pos) if return_stats else out
    ws = _scratch(_ws_hot, "gat_aggregate", feature, csr.num_edges, H, D)
    _launch("gat_aggregate_16", feature, ops._code(feature.dtype), _ptr(feature), _ptr(attn_src), _ptr(attn_dst), H, D,
            float(negative_slope), float(drop_p), _seed32(seed), _ptr(csr.row32), _ptr(csr.col32), _ptr(csr.eid32), _ptr(csr.indptr),
            csr.num_edges, csr.num_nodes, M, _ptr(out), _ptr(mx), _ptr(sm), _ptr(out_pos), _ptr(s_pos), _ptr(ws), ws.numel())
    return (out, mx, sm, out_pos, s_pos) if return_stats else out


def gat_backward16(grad_out, feature, out, attn_src, attn_dst, row_max, row_sum, csr_dst, csr_src, negative_slope=0.2,
                   drop_p=0.0, seed=0, out_pos=None, sum_pos=None):
    """ops.gat_backward on 16-bit rows -> (grad_feature [N, H, D] in feature's dtype, grad_attn_src [N, H] fp32, grad_attn_dst [N, H]
    fp32).  grad_out, feature, out and out_pos share one 16-bit dtype; the result is ops.gat_backward on their .float() copies, the
    feature gradient rounded once (pglamd_gat_backward_16).  The three routes to d a_dst are ops.gat_backward's."""
    _need_cuda(grad_out, feature, out)
    dt = feature.dtype
    if dt not in _DTYPE16 or feature.dim() != 3 or any(t is not None and t.dtype != dt for t in (grad_out, out, out_pos)):
        raise TypeError("gat_backward16: grad_out, feature, out (and out_pos) must share float16 or bfloat16, feature [N, heads, head_dim]")
    n, H, D = (int(v) for v in feature.shape)
    dev = feature.device
    # (grad_out and out also feed the pack kernel's four-element loads -- 8 bytes -- as out_pos does)
    grad_out = _aligned(grad_out, 8); out = _aligned(out, 8); out_pos = _aligned(out_pos, 8)
    feature = _aligned(feature, _lane_bytes16(H, D, pow2=True))
    attn_src = attn_src.to(torch.float32).contiguous(); attn_dst = attn_dst.to(torch.float32).contiguous()
    row_max = row_max.contiguous(); row_sum = row_sum.contiguous()
    sum_pos = None if sum_pos is None else sum_pos.contiguous()
    gf = torch.empty((n, H, D), dtype=dt, device=dev)
    g_src = torch.empty((n, H), dtype=torch.float32, device=dev)
    use_pre = ops._GAT_BWD_EDGE_BUFFER and out_pos is None
    g_dst = None if use_pre else torch.empty((n, H), dtype=torch.float32, device=dev)
    gpre = torch.empty((csr_dst.num_edges, H), dtype=torch.float32, device=dev) if use_pre else None
    if n == 0:
        return gf, g_src, (g_dst if g_dst is not None else torch.empty((0, H), dtype=torch.float32, device=dev))
    ws = _scratch(_ws_hot, "gat_backward", feature, csr_dst.num_edges, n, H, D)
    _launch("gat_backward_16", feature, ops._code(dt), _ptr(grad_out), _ptr(feature), _ptr(attn_src), _ptr(attn_dst), _ptr(row_max),
            _ptr(row_sum), _ptr(out), H, D, float(negative_slope), float(drop_p), _seed32(seed), _ptr(csr_dst.row32), _ptr(csr_dst.col32),
            _ptr(csr_dst.eid32), _ptr(csr_dst.indptr), _ptr(csr_src.row32), _ptr(csr_src.col32), _ptr(csr_src.eid32),
            _ptr(csr_src.indptr), csr_dst.num_edges, n, _ptr(gf), _ptr(g_src), _ptr(g_dst), _ptr(gpre), _ptr(out_pos), _ptr(sum_pos),
            _ptr(ws), ws.numel())
    if use_pre:                 # rows of the src-sorted edge buffer gathered in dst-sorted order, as ops.gat_backward does
        pos = ops._src_pos_in_dst_order(csr_dst, csr_src)
        g_dst = ops.aggregate(gpre, csr_dst.view(col32=pos, eid32=pos, edge_rows=True), "sum", n)
    return gf, g_src, g_dst
