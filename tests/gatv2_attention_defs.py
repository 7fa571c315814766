"""The DEFINITION of the fused GATv2 attention (pgl_amd/csrc/gatv2_attention.hip, Graph.gatv2_attention, GATv2Conv(fused=True)) in
plain torch, written edge by edge like dot_attention_defs.dot_attention, the explicit terms that bound a finite-precision evaluation of
it, of its row statistics and of its three gradients, and the inputs the GPU tests run on (tests/test_gatv2_attention_gpu.py) -- kept
here so that the CPU test (tests/test_gatv2_attention_defs.py) can evaluate the fp32 definition on exactly those inputs.

    z_e,h,d    = x_src[u,h,d] + x_dst[v,h,d]                        e = (u -> v)
    s_e,h      = sum_d a[h,d] * L(z_e,h,d)                          L = leaky_relu(.; slope), L'(0) = slope (torch's convention)
    alpha_e,h  = softmax over the in-edges of v of s_e,h
    out[v,h,:] = sum_e keep_e,h alpha_e,h x_src[u,h,:]              (keep: grad_defs.attention_keep, or None)

Nothing here imports pgl_amd.

K (grad_defs.py, the block above FP32_DEFINITION_RATIO): max(1, 4 x the worst err / bound of this definition evaluated in fp32 torch on
the host on the GPU tests' inputs), never measured from the engine.  Measured with measure_definitions():

    family                 worst err / bound of the fp32 definition      K
    gatv2_attention        0.044                                          1
    gatv2_attention_drop   0.044                                          1

(gatv2_attention: the hub and the classes graph over SHAPES with two operands and with one tensor on both sides, their row
statistics, and the exact case -- worst: the output on the classes graph, 4 x 8; gatv2_attention_drop: DROP_CASES -- worst: the
output on the classes graph, 4 x 8, p = 0.3.  d a uses almost nothing of its bound: its count is the number of edges, what a sum of
E terms in ANY order is owed, and every real summation -- torch's, the kernels' chunk partials -- is far from the sequential one.)"""
import numpy as np
import torch

import grad_defs as D

FP32_DEFINITION_RATIO = dict(gatv2_attention=0.044, gatv2_attention_drop=0.044)
K_FAMILY = {k: max(1.0, 4.0 * v) for k, v in FP32_DEFINITION_RATIO.items()}

SHAPES = [(4, 8), (8, 16), (2, 32), (1, 64), (8, 32)]          # 1, 2, 1, 1 and 4 columns per lane
DROP_SEEDS = {0.3: 1234, 0.9: 2 ** 32 - 5}                     # (one of them >= 2**31, passed as a Python int)
DROP_CASES = [("hub", 8, 16, 0.3), ("classes", 8, 16, 0.3), ("classes", 4, 8, 0.3), ("classes", 8, 32, 0.3), ("hub", 8, 16, 0.9),
              ("classes", 8, 16, 0.9)]
EXACT_HD = (8, 16)
EXACT_SLOPE = 0.25                                             # (0.2 * z is not exact in fp32; a quarter of a small integer is)


# ------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------
def leaky(z, slope):
    """leaky_relu with the derivative `slope` at z == 0: torch.where routes the gradient of a zero to its second branch."""
    return torch.where(z > 0, z, slope * z)


def _softmax_by_dst(s, dst, n):
    """s [E, H] -> (p = exp(s - max), max [n, H], sum [n, H]): softmax over each destination's edges is p / sum[dst]."""
    H = s.shape[1]
    m = torch.full((n, H), -float("inf"), dtype=s.dtype, device=s.device)
    m = m.scatter_reduce(0, dst[:, None].expand(-1, H), s.detach(), "amax", include_self=True)
    p = torch.exp(s - m[dst])
    return p, m, torch.zeros((n, H), dtype=s.dtype, device=s.device).index_add(0, dst, p)


def gatv2_attention(x_src, x_dst, a, src, dst, slope=0.2, keep=None, mutant=None, frozen=None, parts=False):
    """x_src, x_dst [N, H, D]; a [H, D]; edge e = (src_e -> dst_e); keep [E, H] in the order of the edge list (None: no dropout).
    A row without in-edges is 0, and so are its statistics.  parts: -> (out, alpha, row_max, row_sum).
    mutant (tests only; each leaves the VALUE as it is):
      "da_identity_negative" -- d s / d a = z instead of L(z): the gradient of a takes L for the identity on the negative side;
      "dxdst_without_lprime" -- d L(z) / d x_dst = 1 instead of L'(z);
      "t_without_mask"       -- the softmax row term of the gradient forgets the mask."""
    n = x_src.shape[0]
    mutant = mutant or {}
    xd = x_dst[dst]
    if mutant.get("dxdst_without_lprime"):
        act = leaky(x_src[src] + xd.detach(), slope) + (xd - xd.detach())          # MUTANT
        z = x_src[src] + xd.detach()
    else:
        z = x_src[src] + xd
        act = leaky(z, slope)
    if mutant.get("da_identity_negative"):
        s = (a.detach() * act).sum(-1) + ((a - a.detach()) * z.detach()).sum(-1)   # MUTANT
    else:
        s = (a * act).sum(-1)                                     # [E, H]
    p, m, sm = _softmax_by_dst(s, dst, n)
    alpha = p / sm[dst]
    v = x_src
    if keep is None:
        out = torch.zeros_like(v).index_add(0, dst, alpha[:, :, None] * v[src])
    else:
        keep = D._keep_like(keep, v)
        if mutant.get("t_without_mask"):
            # MUTANT: d s_e = alpha_e (keep_e T_e - sum alpha_e' T_e'): alpha = p / sm, the path through p gives alpha_e keep_e T_e, the
            # path through sm gives the row term -- taken unmasked here (same value, same direct gradient of x_src)
            vs = v[src]
            through_p = (keep * p / sm[dst].detach())[:, :, None] * vs
            through_z = (p.detach() / sm[dst])[:, :, None] * vs.detach()
            out = torch.zeros_like(v).index_add(0, dst, through_p + through_z - through_z.detach())
        else:
            out = torch.zeros_like(v).index_add(0, dst, (keep * alpha)[:, :, None] * v[src])
    if parts:
        empty = sm == 0
        return out, alpha, torch.where(empty, torch.zeros_like(m), m), sm
    return out


def gatv2_attention_terms(x_src, x_dst, a, src, dst, cot, slope=0.2, keep=None):
    """Explicit terms, as dot_attention_defs.dot_attention_terms.  With alpha the (undropped) attention, g = |cot|,
    T_e = keep_e <g[v], |x_src[u]|> per head, S[v] = sum_{e into v} alpha_e T_e, c_e = alpha_e (T_e + S[v]) >= |ds_e|, L'_e,d in
    {1, slope} and A_e = sum_d |a[d]| |L(z_e,d)| (what a score's rounding is relative to):
        out[v]      sum keep alpha |x_src[u]|                              2 indeg + D + 4 terms
        d x_dst[v]  sum c_e |a| L'_e                                       2 indeg + 2 D + 4
        d x_src[u]  sum keep alpha g[dst_e] + c_e |a| L'_e                 outdeg + (max indeg over u's destinations) + 2 D + 4
        d a         sum over ALL edges of c_e |L(z_e)|                     E + max indeg + 2 D + 4
        row_max[v]  max over the in-edges of A_e                           D + 2
        row_sum[v]  sum p_e (1 + A_e + max A)                              indeg + D + 4
    (+ 1 each with dropout, for the multiplication by keep; the statistics do not see it).
    -> dict(out=(terms, n), xs=..., xd=..., a=..., row_max=..., row_sum=...) of fp64 tensors."""
    x_src, x_dst, a, cot = (t.detach().double() for t in (x_src, x_dst, a, cot))
    a = a.reshape(x_src.shape[1:])
    n, H, Dh = x_src.shape
    E = src.shape[0]
    _, alpha, m, sm = gatv2_attention(x_src, x_dst, a, src, dst, slope, parts=True)
    indeg, outdeg = D.degree(dst, n).double(), D.degree(src, n).double()
    g = cot.abs()
    keep = D._keep_like(keep, x_src)
    w = alpha if keep is None else keep * alpha
    xs_abs = x_src[src].abs()
    out_t = torch.zeros_like(x_src).index_add(0, dst, w[:, :, None] * xs_abs)
    T = (g[dst] * xs_abs).sum(-1)
    if keep is not None:
        T = keep * T
    S = torch.zeros((n, H), dtype=x_src.dtype, device=x_src.device).index_add(0, dst, alpha * T)
    c = alpha * (T + S[dst])
    z = x_src[src] + x_dst[dst]
    dl = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, abs(float(slope))))
    lz = leaky(z, slope).abs()
    through_score = c[:, :, None] * a.abs() * dl
    xd_t = torch.zeros_like(x_src).index_add(0, dst, through_score)
    xs_t = torch.zeros_like(x_src).index_add(0, src, w[:, :, None] * g[dst] + through_score)
    a_t = (c[:, :, None] * lz).sum(0)
    A = (a.abs() * lz).sum(-1)                                    # [E, H]
    A_max = torch.zeros((n, H), dtype=x_src.dtype, device=x_src.device)
    seg_of_src = torch.zeros(n, dtype=x_src.dtype, device=x_src.device)
    if E:
        A_max = A_max.scatter_reduce(0, dst[:, None].expand(-1, H), A, "amax", include_self=True)
        seg_of_src = seg_of_src.scatter_reduce(0, src, indeg[dst], "amax", include_self=True)
    p = alpha * sm[dst]
    sum_t = torch.zeros((n, H), dtype=x_src.dtype, device=x_src.device).index_add(0, dst, p * (1.0 + A + A_max[dst]))
    base = 4.0 if keep is None else 5.0
    ex = lambda cnt: cnt[:, None, None].expand_as(x_src)
    exh = lambda cnt: cnt[:, None].expand(n, H)
    max_in = float(indeg.max()) if n else 0.0
    return dict(out=(out_t, ex(2 * indeg + Dh + base)), xs=(xs_t, ex(outdeg + seg_of_src + 2 * Dh + base)),
                xd=(xd_t, ex(2 * indeg + 2 * Dh + base)), a=(a_t, torch.full_like(a_t, E + max_in + 2 * Dh + base)),
                row_max=(A_max, torch.full_like(A_max, Dh + 2.0)), row_sum=(sum_t, exh(indeg + Dh + 4.0)))


def definition_and_terms(x_src, x_dst, a, cot, src, dst, slope=0.2, keep=None, mutant=None):
    """-> (grad_defs.GradTerms, terms).  x_dst None: ONE tensor on both sides -- inputs (x, a), the terms of d x the sum of both sides'
    (one more term for the addition); else inputs (x_src, x_dst, a).  terms: gatv2_attention_terms' dict (the statistics' bounds)."""
    shared = x_dst is None
    res = gatv2_attention_terms(x_src, x_src if shared else x_dst, a, src, dst, cot, slope, keep)
    a_terms = (res["a"][0].reshape(a.shape), res["a"][1].reshape(a.shape))
    if shared:
        fn = lambda x, w, frozen=None: gatv2_attention(x, x, w.reshape(x.shape[1:]), src, dst, slope, keep=keep, mutant=mutant)
        terms = {"out": res["out"], 0: (res["xs"][0] + res["xd"][0], res["xs"][1] + res["xd"][1] + 1.0), 1: a_terms}
        return D.grad_and_terms(fn, [x_src, a], cot, terms=terms), res
    fn = lambda xs, xd, w, frozen=None: gatv2_attention(xs, xd, w.reshape(xs.shape[1:]), src, dst, slope, keep=keep, mutant=mutant)
    terms = {"out": res["out"], 0: res["xs"], 1: res["xd"], 2: a_terms}
    return D.grad_and_terms(fn, [x_src, x_dst, a], cot, terms=terms), res


# ------------------------------------------------------------------------------------------------
# the GPU tests' inputs (numpy, so that the host measurement and the GPU tests read the same values)
# ------------------------------------------------------------------------------------------------
def _rows(rng, *shape):
    """test_gradients_gpu.rows: standard normal rows, each scaled by 10**U(-4, 0)."""
    import test_gradients_gpu as T
    return T.rows(rng, *shape)


def case_inputs(n, H, Dh, seed=0):
    """-> (x_src, x_dst, a, cot, slope) float32: standard-normal x_src, x_dst and a = N(0, 1) / sqrt(D), so that the scores have a
    spread of about 1 (attention is not uniform) and sum_d |a| |L(z)| stays a small number; the cotangent in per-row scaled rows."""
    rng = np.random.default_rng(211 + 13 * H + Dh + seed)
    f = lambda v: v.astype(np.float32)
    return (f(rng.standard_normal((n, H, Dh))), f(rng.standard_normal((n, H, Dh))), f(rng.standard_normal((H, Dh)) * Dh ** -0.5),
            f(_rows(rng, n, H, Dh)), 0.2)


def exact_inputs(n, seed=0):
    """Large, exact scores: x_src, x_dst integers in [-4, 4], a multiples of 1/8 in [-4, 4], D = 16, slope 1/4 -- every z (an integer
    up to 8), every L(z) (a multiple of 1/4), every product (a multiple of 1/32 up to 32) and every partial sum (up to 512) is exact in
    fp32 in any order; about one z in nine is exactly 0 (the kink), and |s| reaches beyond 100."""
    H, Dh = EXACT_HD
    rng = np.random.default_rng(307 + seed)
    f = lambda v: v.astype(np.float32)
    return (f(rng.integers(-4, 5, (n, H, Dh))), f(rng.integers(-4, 5, (n, H, Dh))), f(rng.integers(-32, 33, (H, Dh)) / 8.0),
            f(_rows(rng, n, H, Dh)), EXACT_SLOPE)


def graph_edges(name):
    """(n, src, dst) of the GPU tests' graphs, from tests/test_gradients_gpu.py."""
    import test_gradients_gpu as T
    return T._hub_edges() if name == "hub" else T._classes_edges()


def cases():
    """(family, what, graph, inputs(n) -> (x_src, x_dst, a, cot, slope), p, shared) of every bound-checked GPU case."""
    out = []
    for shared in (False, True):
        for graph in ("hub", "classes"):
            for H, Dh in SHAPES:
                out.append(("gatv2_attention", "%s %dx%d%s" % (graph, H, Dh, " one tensor" if shared else ""), graph,
                            (lambda n, H=H, Dh=Dh: case_inputs(n, H, Dh)), 0.0, shared))
    out.append(("gatv2_attention", "hub exact scores", "hub", exact_inputs, 0.0, False))
    for graph, H, Dh, p in DROP_CASES:
        out.append(("gatv2_attention_drop", "%s %dx%d p=%g" % (graph, H, Dh, p), graph, (lambda n, H=H, Dh=Dh: case_inputs(n, H, Dh)), p, False))
    return out


def measure_definitions(verbose=True):
    """-> {family: the worst err / bound of the fp32 definition (torch on the host) over the family's cases}: the output, the
    gradients and (without dropout) the row statistics.  No engine involved."""
    worst, edges = {}, {}
    for family, what, graph, make, p, shared in cases():
        if graph not in edges:
            n, src, dst = graph_edges(graph)
            edges[graph] = (n, torch.as_tensor(src.astype(np.int64)), torch.as_tensor(dst.astype(np.int64)))
        n, src, dst = edges[graph]
        xs, xd, a, cot, slope = (torch.as_tensor(v) if isinstance(v, np.ndarray) else v for v in make(n))
        keep = None if p == 0 else torch.as_tensor(D.attention_keep(DROP_SEEDS[p], np.arange(src.shape[0]), xs.shape[1], p))
        r, res = definition_and_terms(xs, None if shared else xd, a, cot, src, dst, slope, keep)
        if shared:
            inputs, fn = [xs, a], (lambda x, w: gatv2_attention(x, x, w, src, dst, slope, keep=keep))
        else:
            inputs, fn = [xs, xd, a], (lambda x, y, w: gatv2_attention(x, y, w, src, dst, slope, keep=keep))
        out32, g32 = D.evaluate(fn, inputs, cot, torch.float32)
        assert bool(torch.isfinite(out32).all()) and all(bool(torch.isfinite(t).all()) for t in g32), what
        parts = [D.worst_ratio(out32, r.out64, r.out_abs, r.out_n)] + \
                [D.worst_ratio(g32[i], r.want64[i], r.abs_terms64[i], r.n_terms[i]) for i in range(len(inputs))]
        if p == 0:
            x2 = xs if shared else xd
            _, _, m32, s32 = gatv2_attention(xs, x2, a, src, dst, slope, parts=True)
            _, _, m64, s64 = gatv2_attention(xs.double(), x2.double(), a.double(), src, dst, slope, parts=True)
            parts += [D.worst_ratio(m32, m64, *res["row_max"]), D.worst_ratio(s32, s64, *res["row_sum"])]
        if verbose:
            print("%s: the fp32 definition uses %s of the bound (out, gradients in input order, a last%s)"
                  % (what, ", ".join("%.3f" % x for x in parts), "; then row_max, row_sum" if p == 0 else ""))
        worst[family] = max(worst.get(family, 0.0), max(parts))
    return worst
