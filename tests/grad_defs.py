"""Plain torch DEFINITIONS of every differentiable op of pgl_amd, written edge by edge (x[src], index_add, a boolean mask,
torch.where), and the bound a finite-precision gradient of each must meet -- per ELEMENT, from that element's own terms.

Nothing here imports pgl_amd: the formulations share no code with the engine, run on CPU or GPU, in fp64 for "want" and in fp32 for
calibration (what a plain evaluation in the engine's precision uses of the bound).

Conventions
  * A definition is `fn(*inputs, frozen=None)`.  `frozen` (a dict) carries what is decided from the REAL inputs and then held fixed:
    the winner mask of max / min, the slope of a leaky relu, the mask of a relu.  `frozen_fn(*inputs)` computes it.
  * max / min follow PADDLE'S tie rule (graph_send_recv_grad): EVERY message equal to the winner receives the whole gradient -- an
    explicit mask; torch's amax backward splits the gradient evenly among ties and is the wrong reference.
  * abs_terms of a gradient element = the sum of the absolute values of its terms.  For sums of monomials (sum / mean x add / sub / mul /
    div, send_uv, sddmm, gathers, the linear forms, and -- with the masks frozen -- max / min, leaky, relu) that is
    |autograd of fn at (|inputs|) with cotangent |w||: every term of one gradient element is a monomial of fixed sign.  `frozen["abs"]`
    tells a definition it is being evaluated that way (a subtraction then adds).  Softmax-type gradients are differences of such sums
    and get explicit term functions (`*_terms`).
  * `mutant` (a dict, tests only) makes a definition subtly WRONG in one documented way; the sensitivity tests require the bound to
    notice each of them."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _lead(t, nd):
    """[R, *tail] -> [R, 1, ..., 1, *tail] with nd dims (numpy broadcasting of the trailing dims)."""
    return t.reshape((t.shape[0],) + (1,) * (nd - t.dim()) + tuple(t.shape[1:])) if t.dim() < nd else t


def _col(v, like):
    """A per-row vector as a column broadcastable against `like`."""
    return v.reshape((-1,) + (1,) * (like.dim() - 1))


def _rows(n, like):
    return torch.zeros((int(n),) + tuple(like.shape[1:]), dtype=like.dtype, device=like.device)


def degree(index, n):
    return torch.bincount(index, minlength=int(n))[:int(n)]


def _flat(t):
    """[R, *tail] -> [R, prod(tail)] (also for R = 0, where reshape(R, -1) is ambiguous)."""
    return t.reshape(t.shape[0], int(np.prod(t.shape[1:], dtype=np.int64)))


def _is_abs(frozen):
    return bool(frozen) and bool(frozen.get("abs"))


def message(xs, y, mop, frozen=None, mutant=None):
    """x[src] (op) y with numpy broadcasting of the trailing dims; y None: the message is x[src] itself."""
    if y is None:
        return xs
    nd = max(xs.dim(), y.dim())
    xs, y = _lead(xs, nd), _lead(y, nd)
    if mop == "add":
        return xs + y
    if mop == "sub":
        return xs + y if _is_abs(frozen) else xs - y
    if mop == "mul":
        return xs * y
    if mop == "div":
        if mutant and mutant.get("div_dy"):
            # MUTANT: d/dy written as -x / y instead of -x / y^2 (same value, wrong derivative)
            yd, xd = y.detach(), xs.detach()
            return xs / yd + (-xd / yd) * (y - yd)
        return xs / y
    raise ValueError(mop)


def _out_rows(x, out_size):
    return int(out_size) if (out_size is not None and int(out_size) > 0) else int(x.shape[0])


def _extreme(msg, dst, m, rop):
    """max / min of the messages per destination (values only; rows without a message: 0).  Rows are grouped by a stable sort and
    reduced segment by segment: no atomics, so a destination with 30 000 messages costs what any other 30 000 rows cost."""
    flat = _flat(msg.detach())
    cnt = degree(dst, m)
    if flat.shape[0] == 0 or flat.shape[1] == 0:
        return torch.zeros((m,) + tuple(msg.shape[1:]), dtype=msg.dtype, device=msg.device)
    assert int(dst.max()) < m, "a destination beyond the output rows"
    order = torch.argsort(dst, stable=True)
    out = torch.segment_reduce(flat[order], rop, lengths=cnt, axis=0, unsafe=True)
    out = torch.where((cnt > 0)[:, None], out, torch.zeros_like(out))
    return out.reshape((m,) + tuple(msg.shape[1:]))


def _seg_sum(v, ids, m):
    """index_add of the rows of v [R, F] into m rows, for the softmax definitions, whose data has one segment of 30 000 rows: the rows
    are grouped by a stable sort and summed segment by segment (differentiable).  An fp64 index_add of 30 000 rows into ONE row is a
    chain of contended atomics that takes seconds per call on the GPU."""
    if v.shape[0] == 0:
        return _rows(m, v)
    order = torch.argsort(ids, stable=True)
    return torch.segment_reduce(v[order], "sum", lengths=degree(ids, m), axis=0, unsafe=True)


# ------------------------------------------------------------------------------------------------
# send_u_recv / send_ue_recv
# ------------------------------------------------------------------------------------------------
def winner_mask(x, src, dst, rop, out_size=None, y=None, mop="add"):
    """frozen_fn of max / min: which messages equal their destination's winner (from the real inputs)."""
    if rop not in ("max", "min"):
        return {}
    msg = message(x.detach()[src], None if y is None else y.detach(), mop)
    win = _extreme(msg, dst, _out_rows(x, out_size), rop)
    return {"mask": msg == win[dst]}


def send_recv(x, src, dst, rop="sum", out_size=None, y=None, mop="add", frozen=None, mutant=None):
    """send_u_recv (y None) / send_ue_recv: out[v] = REDUCE_{e: dst_e = v} x[src_e] (op) y_e; rows without in-edges are 0; mean
    divides by max(indeg, 1); max / min: Paddle's tie rule."""
    m = _out_rows(x, out_size)
    msg = message(x[src], y, mop, frozen, mutant)
    if mutant and mutant.get("drop_edge") is not None:
        keep = torch.ones(msg.shape[0], dtype=msg.dtype, device=msg.device)
        keep[int(mutant["drop_edge"])] = 0.0                      # MUTANT: one edge's term is lost
        msg = msg * _col(keep, msg)
    if rop in ("sum", "mean"):
        out = _rows(m, msg).index_add(0, dst, msg)
        if rop == "mean":
            deg = degree(dst, m).clamp(min=1).to(msg.dtype)
            if mutant and mutant.get("no_deg_row") is not None:
                deg = deg.clone(); deg[int(mutant["no_deg_row"])] = 1.0      # MUTANT: 1 / deg forgotten on one row
            out = out / _col(deg, out)
        return out
    if rop not in ("max", "min"):
        raise ValueError(rop)
    if frozen and "mask" in frozen:
        mask = frozen["mask"]
    else:
        mask = msg.detach() == _extreme(msg, dst, m, rop)[dst]
    if _is_abs(frozen):
        return _rows(m, msg).index_add(0, dst, msg * mask.to(msg.dtype))       # (terms only: the sum of the winners' magnitudes)
    maskf = mask.to(msg.dtype)
    if mutant and mutant.get("split_ties"):
        cnt = _rows(m, msg).index_add(0, dst, maskf)                           # MUTANT: torch's amax rule, ties share the gradient
        maskf = maskf / cnt.clamp(min=1)[dst]
    # value: the winner itself (msg - msg.detach() is exactly 0); gradient: the WHOLE cotangent to every message equal to it
    return _extreme(msg, dst, m, rop) + _rows(m, msg).index_add(0, dst, maskf * (msg - msg.detach()))


def send_uv(x, y, src, dst, mop="add", frozen=None, mutant=None):
    return message(x[src], y[dst], mop, frozen, mutant)


# ------------------------------------------------------------------------------------------------
# segment ops (ids sorted or not: the definitions do not care)
# ------------------------------------------------------------------------------------------------
def segment_frozen(data, ids, pool, num_segments):
    iota = torch.arange(data.shape[0], device=data.device)
    return winner_mask(data, iota, ids, pool, num_segments)


def segment_pool(data, ids, pool, num_segments, frozen=None, mutant=None):
    iota = torch.arange(data.shape[0], device=data.device)
    out = send_recv(data, iota, ids, pool, num_segments, frozen=frozen, mutant=mutant)
    return out if int(num_segments) > 0 else out[:0]


def segment_softmax(x, ids, num_segments):
    """softmax over the rows of each segment, per column.  edge_softmax(norm_by = dst | src) is this with ids = dst | src."""
    flat = _flat(x)
    mx = _extreme(flat, ids, int(num_segments), "max")
    p = torch.exp(flat - mx[ids])
    s = _seg_sum(p, ids, num_segments)
    return (p / s[ids]).reshape(x.shape)


def segment_softmax_terms(x, ids, num_segments, cot):
    """-> (forward terms, gradient terms, n_terms), all shaped like x.  d x = p (g - sum_seg p g): a difference of two sums, so the
    terms are p |g| + p sum_seg p |g| and the count is the segment's length (+ exp, the division, the product)."""
    x, cot = x.detach().double(), cot.detach().double()
    p = _flat(segment_softmax(x, ids, num_segments))
    g = _flat(cot).abs()
    s = _seg_sum(p * g, ids, num_segments)
    flat = _flat(x)
    mx = _extreme(flat, ids, int(num_segments), "max")
    n = (degree(ids, num_segments)[ids] + 3).double()[:, None].expand_as(p)
    return (p * (1.0 + (flat - mx[ids]).abs())).reshape(x.shape), (p * g + p * s[ids]).reshape(x.shape), n.reshape(x.shape)


# ------------------------------------------------------------------------------------------------
# row moves
# ------------------------------------------------------------------------------------------------
def gather(x, index, frozen=None):
    return x[index]


def scatter_into_zeros(x, index, n_rows, frozen=None):
    """zeros([n_rows, ...]) with rows `index` (unique) overwritten by x."""
    return _rows(n_rows, x).index_add(0, index, x)


# ------------------------------------------------------------------------------------------------
# edge scores
# ------------------------------------------------------------------------------------------------
def sddmm(x, y, src, dst, frozen=None):
    return (x[src] * y[dst]).sum(-1)


def leaky_frozen(pre, slope):
    return torch.where(pre.detach() > 0, torch.ones_like(pre), torch.full_like(pre, slope)).detach()


def add_score_frozen(x, y, w, src, dst, slope=0.2):
    return {"dl": leaky_frozen(x[src] + y[dst], slope), "pre": (x[src] + y[dst]).detach()}


def add_score(x, y, w, src, dst, slope=0.2, frozen=None, mutant=None):
    """s[e, h] = sum_d w[h, d] * leaky(x[src_e, h, d] + y[dst_e, h, d])."""
    pre = x[src] + y[dst]
    dl = frozen["dl"] if frozen and "dl" in frozen else leaky_frozen(pre, slope)
    act = pre * dl
    if mutant and mutant.get("leaky_slope") is not None:
        # MUTANT: leaky' with the wrong slope on negative inputs (same value, wrong derivative)
        bad = torch.where(dl == 1.0, dl, torch.full_like(dl, float(mutant["leaky_slope"])))
        act = act.detach() + (pre - pre.detach()) * bad
    return (act * w).sum(-1)


def attention_keep(seed, eid, n_heads, p):
    """The keep factor of the fused GAT kernels' attention dropout, restated from the text next to pglamd_gat_aggregate in
    include/pgl_amd.h -> [E, H] fp32: 1 / (1 - p) (rounded once in fp32) where edge `eid` keeps head h, else 0.
        h = seed ^ (uint32(eid) * 0x9E3779B1) ^ (uint32(head) * 0x85EBCA77 + 0xC2B2AE3D)
        h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16            (all uint32, wrapping)
        u = float(h >> 8) * 2**-24; kept where u >= p, compared in fp32
    seed: any integer, taken modulo 2**32; eid: ORIGINAL edge ids; head: the index inside the launch."""
    e = (np.asarray(eid).astype(np.int64).reshape(-1, 1) & 0xFFFFFFFF).astype(np.uint32)
    hd = np.arange(int(n_heads), dtype=np.uint32).reshape(1, -1)
    c = lambda v: np.full((1, 1), v, dtype=np.uint32)               # (arrays: numpy wraps uint32 array arithmetic silently)
    h = c(int(seed) % 2 ** 32) ^ (e * c(0x9E3779B1)) ^ (hd * c(0x85EBCA77) + c(0xC2B2AE3D))
    h = h ^ (h >> c(16)); h = h * c(0x7FEB352D); h = h ^ (h >> c(15)); h = h * c(0x846CA68B); h = h ^ (h >> c(16))
    assert h.dtype == np.uint32
    u = (h >> c(8)).astype(np.float32) * np.float32(2.0 ** -24)
    p32 = np.float32(p)
    factor = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(u >= p32, factor, np.float32(0.0)).astype(np.float32)


def _keep_like(keep, like):
    return None if keep is None else torch.as_tensor(keep).to(dtype=like.dtype, device=like.device)


def _dense_gat_fp64(edges, f, a_s, a_d, slope=0.2, keep=None, mutant=None):
    """The formula of pgl/nn/conv.py:331-339 written edge by edge in fp64 torch (autograd-able): an independent
    formulation -- gather, scatter_reduce(amax), index_add -- that shares no code with the engine or the C port.
    keep [E, H] (attention dropout, in the order of `edges`): out[v] = sum_e keep_e alpha_e f[u]; alpha (returned) is the undropped softmax."""
    src, dst = edges[:, 0], edges[:, 1]
    n, H = a_d.shape
    logit = torch.nn.functional.leaky_relu(a_s[src] + a_d[dst], slope)                       # [E, H]
    m = torch.full((n, H), -float("inf"), dtype=logit.dtype, device=logit.device)
    m = m.scatter_reduce(0, dst[:, None].expand(-1, H), logit.detach(), "amax", include_self=True)
    p = torch.exp(logit - m[dst])
    s = torch.zeros((n, H), dtype=logit.dtype, device=logit.device).index_add(0, dst, p)
    alpha = p / s[dst]
    if keep is None:
        out = torch.zeros_like(f).index_add(0, dst, alpha[:, :, None] * f[src])
        return out, alpha
    keep = _keep_like(keep, f)
    if mutant and mutant.get("t_without_mask"):
        # MUTANT: d pre_e = leaky' alpha_e (keep_e t_e - sum alpha_e' t_e'): the row term t[v] forgets the mask (same value, same d f).
        # alpha = p / s: the path through p gives alpha_e keep_e t_e, the path through s gives -alpha_e sum alpha t -- taken unmasked
        fs = f[src]
        through_p = (keep * p / s[dst].detach())[:, :, None] * fs
        through_s = (p.detach() / s[dst])[:, :, None] * fs.detach()
        return torch.zeros_like(f).index_add(0, dst, through_p + through_s - through_s.detach()), alpha
    out = torch.zeros_like(f).index_add(0, dst, (keep * alpha)[:, :, None] * f[src])
    return out, alpha


def gat(f, a_s, a_d, src, dst, slope=0.2, keep=None, mutant=None):
    return _dense_gat_fp64(torch.stack([src, dst], 1), f, a_s, a_d, slope, keep, mutant)[0]


def gat_proj(f, proj, src, dst, slope=0.2, keep=None):
    """gat with the scores computed inside: a_src | a_dst = f.reshape(N, H*D) @ proj (proj [H*D, 2H])."""
    H = f.shape[1]
    att = f.reshape(f.shape[0], -1) @ proj
    return gat(f, att[:, :H], att[:, H:], src, dst, slope, keep)


def gat_pre(a_s, a_d, src, dst):
    return (a_s[src] + a_d[dst]).detach()


def gat_terms(f, a_s, a_d, src, dst, cot, slope=0.2, proj=None, keep=None):
    """Explicit terms of the GAT aggregation.  With alpha the attention, t_e = <g[dst_e], f[src_e]> per head and T_e the same with
    absolute values:  d f[u] = sum_{e: src = u} alpha_e g[dst_e];  d pre_e = leaky'_e alpha_e (t_e - sum_{e' -> dst_e} alpha_e' t_e'),
    d a_src[u] / d a_dst[v] = its sums by source / destination.
    keep [E, H] (attention dropout): out[v] = sum_e keep_e alpha_e f[u] with alpha the undropped softmax -- keep multiplies the out and
    d f terms and T_e = keep_e <|g|, |f|> (so S[v] = sum alpha_e T_e carries it too); one more term in every count for the multiplication.
    -> dict(out=(terms, n), f=..., a_s=..., a_d=...[, proj=...]) of fp64 tensors."""
    f, a_s, a_d, cot = (t.detach().double() for t in (f, a_s, a_d, cot))
    n, H, D = f.shape
    _, alpha = _dense_gat_fp64(torch.stack([src, dst], 1), f, a_s, a_d, slope)
    indeg, outdeg = degree(dst, n).double(), degree(src, n).double()
    g = cot.abs()
    keep = _keep_like(keep, f)
    w = alpha if keep is None else keep * alpha                                              # what weighs a feature row
    out_t = torch.zeros_like(f).index_add(0, dst, w[:, :, None] * f[src].abs())
    f_t = torch.zeros_like(f).index_add(0, src, w[:, :, None] * g[dst])
    T = (g[dst] * f[src].abs()).sum(-1)                                                      # [E, H]
    if keep is not None:
        T = keep * T
    S = torch.zeros((n, H), dtype=f.dtype, device=f.device).index_add(0, dst, alpha * T)
    dl = leaky_frozen(a_s[src] + a_d[dst], slope)
    pre_t = dl * alpha * (T + S[dst])
    as_t = torch.zeros_like(a_s).index_add(0, src, pre_t)
    ad_t = torch.zeros_like(a_d).index_add(0, dst, pre_t)
    seg_of_src = torch.zeros(n, dtype=f.dtype, device=f.device)
    if src.shape[0]:
        seg_of_src = seg_of_src.scatter_reduce(0, src, indeg[dst], "amax", include_self=True)
    base = 4 if keep is None else 5
    n_out = (2 * indeg + base)[:, None, None].expand_as(f)
    n_f = (outdeg + seg_of_src + base)[:, None, None].expand_as(f)
    n_as = (outdeg + seg_of_src + D + base)[:, None].expand_as(a_s)
    n_ad = (2 * indeg + D + base)[:, None].expand_as(a_d)
    res = dict(out=(out_t, n_out), f=(f_t, n_f), a_s=(as_t, n_as), a_d=(ad_t, n_ad))
    if proj is not None:
        pa = proj.detach().double().abs()
        att_t = torch.cat([as_t, ad_t], 1)                                                   # [N, 2H]
        n_att = torch.cat([n_as, n_ad], 1)
        f2 = f.reshape(n, -1).abs()
        # the scores themselves are a GEMM over H*D columns: their rounding reaches every gradient through alpha
        res["f"] = (f_t + (att_t @ pa.t()).reshape(f.shape), n_f + float(2 * H + H * D) + n_att.max(1).values[:, None, None])
        res["proj"] = (f2.t() @ att_t, (n_att.max(0).values + float(n))[None, :].expand(pa.shape[0], -1) + float(H * D))
    return res


# ------------------------------------------------------------------------------------------------
# scaled / fused aggregation forms
# ------------------------------------------------------------------------------------------------
def send_recv_scaled(x, src, dst, src_scale=None, dst_scale=None, frozen=None):
    """out[v] = dst_scale[v] * sum_{u -> v} src_scale[u] * x[u] (the scales carry no gradient)."""
    xs = x if src_scale is None else x * _col(src_scale.to(x.dtype), x)
    out = _rows(x.shape[0], x).index_add(0, dst, xs[src])
    return out if dst_scale is None else out * _col(dst_scale.to(x.dtype), out)


def propagate_step(x, res, src, dst, dst_scale, c=0.0, frozen=None):
    """c * res + dst_scale (.) A x."""
    out = send_recv_scaled(x, src, dst, None, dst_scale)
    return out if res is None else out + res * (abs(c) if _is_abs(frozen) else c)


def row_epilogue(z, bias=None, act=None, normalize=False, eps=1e-12):
    """normalize_L2(act(z + bias)); F.normalize: a / max(||a||, eps)."""
    a = z if bias is None else z + bias
    if act == "relu":
        a = torch.where(a > 0, a, torch.zeros_like(a))
    if normalize:
        a = a / a.norm(dim=1, keepdim=True).clamp(min=eps)
    return a


def row_epilogue_pre(z, bias=None):
    return (z if bias is None else z + bias).detach()


def row_epilogue_terms(z, bias, act, normalize, cot, eps=1e-12):
    """d z = act' (dy - y <y, dy>) / ||a||;  d bias = its column sums.  -> dict(out=(terms, n), z=..., bias=...)."""
    z, cot = z.detach().double(), cot.detach().double()
    b = None if bias is None else bias.detach().double()
    a = z if b is None else z + b
    pre_t = z.abs() if b is None else z.abs() + b.abs()
    on = (a > 0).double() if act == "relu" else torch.ones_like(a)
    a = a * on
    d = float(z.shape[1])
    g = cot.abs()
    if normalize:
        nrm = a.norm(dim=1, keepdim=True).clamp(min=eps)
        y = a / nrm
        out_t = on * pre_t / nrm
        z_t = on * (g + y.abs() * (y.abs() * g).sum(1, keepdim=True)) / nrm
        n_out = torch.full_like(z, d + 3.0)
        n_z = torch.full_like(z, 2.0 * d + 4.0)
    else:
        out_t, z_t = on * pre_t, on * g
        n_out = torch.full_like(z, 2.0)
        n_z = torch.full_like(z, 2.0)
    res = dict(out=(out_t, n_out), z=(z_t, n_z))
    if b is not None:
        res["bias"] = (z_t.sum(0), torch.full_like(b, float(z.shape[0])) + n_z[0])
    return res


def dense_frozen(x, weight, bias, src, dst, act=None, src_scale=None, dst_scale=None, rop="sum"):
    if act != "relu":
        return {}
    z = aggregate_dense(x.detach(), weight.detach(), None if bias is None else bias.detach(), src, dst, None, src_scale, dst_scale, rop)
    return {"relu": (z > 0), "pre": z}


def aggregate_dense(x, weight, bias, src, dst, act=None, src_scale=None, dst_scale=None, rop="sum", frozen=None):
    """act( (dst_scale * REDUCE_{u -> v} src_scale[u] x[u]) @ weight^T + bias ), weight [d_out, d_in]."""
    xs = x if src_scale is None else x * _col(src_scale.to(x.dtype), x)
    agg = send_recv(xs, src, dst, rop)
    if dst_scale is not None:
        agg = agg * _col(dst_scale.to(x.dtype), agg)
    z = agg @ weight.t()
    if bias is not None:
        z = z + bias
    if act == "relu":
        on = frozen["relu"] if frozen and "relu" in frozen else (z.detach() > 0)
        z = torch.where(on, z, torch.zeros_like(z))
    return z


def dual_linear(x, y, wa, wb, frozen=None):
    return x @ wa.t() + y @ wb.t()


def aggregate_dual_linear(x, wa, wb, src, dst, rop="sum", frozen=None):
    return x @ wa.t() + send_recv(x, src, dst, rop) @ wb.t()


# ------------------------------------------------------------------------------------------------
# the harness: fp64 gradients and what bounds a finite-precision evaluation of them
# ------------------------------------------------------------------------------------------------
def evaluate(fn, inputs, cotangent, dtype=torch.float64, frozen_fn=None, **kw):
    """Forward and autograd of `fn` in `dtype` -> (out, [grad per input])."""
    xs = [t.detach().to(dtype).requires_grad_(True) for t in inputs]
    if frozen_fn is not None:
        kw = dict(kw, frozen=frozen_fn(*xs))
    out = fn(*xs, **kw)
    grads = torch.autograd.grad(out, xs, cotangent.detach().to(dtype), allow_unused=True)
    return out.detach(), [torch.zeros_like(x) if g is None else g.detach() for x, g in zip(xs, grads)]


class GradTerms(object):
    """out64 / want64[i]: the fp64 forward and gradients; out_abs / abs_terms64[i]: the sum of |terms| of every element;
    out_n / n_terms[i]: how many terms (+ 1 per extra rounding), broadcast to the element's shape."""
    __slots__ = ("out64", "out_abs", "out_n", "want64", "abs_terms64", "n_terms")


def _expand_n(n, like):
    n = torch.as_tensor(n, dtype=torch.float64, device=like.device)
    if n.dim() == 1 and like.dim() > 1 and n.shape[0] == like.shape[0]:
        n = _col(n, like)
    return n.expand(like.shape) if n.dim() else n.expand(like.shape)


def grad_and_terms(fn, inputs, cotangent, n_out=1.0, n_terms=None, frozen_fn=None, terms=None):
    """fp64 autograd of `fn` and the per-element term magnitudes of the forward and of every gradient.
    n_out / n_terms[i]: term counts (a number, one value per row, or an array broadcastable to the element's shape).
    frozen_fn: see the module docstring.  terms: dict(out=(abs, n), <i>: (abs, n)) of EXPLICIT terms for the ops whose gradients are
    not sums of fixed-sign monomials; what it names replaces the |autograd at |inputs|| evaluation."""
    r = GradTerms()
    r.out64, r.want64 = evaluate(fn, inputs, cotangent, torch.float64, frozen_fn)
    n_terms = [1.0] * len(inputs) if n_terms is None else list(n_terms)
    terms = terms or {}
    if "out" in terms and all(i in terms for i in range(len(inputs))):
        out_abs, abs_g = None, [None] * len(inputs)
    else:
        fr = dict(frozen_fn(*[t.detach().double() for t in inputs]) if frozen_fn is not None else {}, abs=True)
        xs = [t.detach().double().abs().requires_grad_(True) for t in inputs]
        out = fn(*xs, frozen=fr)
        g = torch.autograd.grad(out, xs, cotangent.detach().double().abs(), allow_unused=True)
        out_abs = out.detach().abs()
        abs_g = [torch.zeros_like(x) if gi is None else gi.detach().abs() for x, gi in zip(xs, g)]
    r.out_abs, r.out_n = terms["out"] if "out" in terms else (out_abs, n_out)
    r.out_n = _expand_n(r.out_n, r.out64)
    r.abs_terms64, r.n_terms = [], []
    for i in range(len(inputs)):
        a, n = terms[i] if i in terms else (abs_g[i], n_terms[i])
        r.abs_terms64.append(a)
        r.n_terms.append(_expand_n(n, r.want64[i]))
    return r


EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)


def bound(abs_terms, n_terms, slack=4.0, eps=EPS32, K=1.0):
    """gpu_common.reassociation_bound on torch tensors: K * slack * max(n, 1) * eps * sum|t_i| + tiny."""
    return K * slack * n_terms.clamp(min=1.0) * eps * abs_terms + TINY32


def worst_ratio(got, want64, abs_terms, n_terms, slack=4.0, eps=EPS32):
    """max over the elements of |got - want| / bound (0 for an empty tensor): what an evaluation USES of its bound."""
    if want64.numel() == 0:
        return 0.0
    return float(((got.double() - want64).abs() / bound(abs_terms, n_terms, slack, eps)).max())


def count_out_of_bound(got, want64, abs_terms, n_terms, slack=4.0, eps=EPS32, K=1.0):
    return int(((got.double() - want64).abs() > bound(abs_terms, n_terms, slack, eps, K)).sum())


def aggregate_n_terms(src, dst, x_shape, y_shape=None, rop="sum", out_size=None):
    """Term counts of send_u_recv / send_ue_recv -> (n_out [M], [n_x [N], n_y (a number)]): a destination sums its in-edges, d x[u] sums
    u's out-edges times the columns broadcast onto one x element, d y_e sums the columns broadcast onto one y element; + 1 for the
    message op, + 1 for the 1 / deg of a mean."""
    n = int(x_shape[0])
    m = int(out_size) if (out_size is not None and int(out_size) > 0) else n
    extra = (1.0 if y_shape is not None else 0.0) + (1.0 if rop == "mean" else 0.0)
    xt = tuple(x_shape[1:])
    yt = tuple(y_shape[1:]) if y_shape is not None else xt
    out_tail = tuple(np.broadcast_shapes(xt, yt))
    size = lambda t: float(np.prod(t, dtype=np.int64)) if len(t) else 1.0
    fx, fy = size(out_tail) / max(size(xt), 1.0), size(out_tail) / max(size(yt), 1.0)
    n_out = degree(dst, m).double() + extra
    n_x = degree(src, n).double() * fx + extra + 1.0
    return n_out, [n_x, fy + extra + 1.0]


# ------------------------------------------------------------------------------------------------
# K: composite gradients (softmax, GAT, the additive score, the normalising epilogue, the dense forms) carry the forward's rounding
# too (exp of a difference, a GEMM) and are held to K x the abs-terms bound.  K = max(1, 4 x the worst err / bound of the PLAIN
# DEFINITION evaluated in fp32 torch on the inputs of tests/test_gradients_gpu.py) -- measured by its _measure_definitions(), never
# from the engine; 4: a differently ordered fp32 evaluation may use a few times more of its bound than torch's does.
# ------------------------------------------------------------------------------------------------
FP32_DEFINITION_RATIO = dict(softmax=0.4364, gat=0.063, gat_proj=0.033, add_score=0.092, row_epilogue=0.032, dense=0.023, dual_linear=0.021,
                             gat_drop=0.061, gat_proj_drop=0.027)
K_FAMILY = {k: max(1.0, 4.0 * v) for k, v in FP32_DEFINITION_RATIO.items()}
