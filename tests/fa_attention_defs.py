"""The DEFINITION of the fused frequency-adaptive attention (pgl_amd/csrc/fa_attention.hip, Graph.fa_aggregate, FAConv(fused=True)) in
plain torch, written edge by edge like gatv2_attention_defs.gatv2_attention, the explicit terms that bound a finite-precision
evaluation of it and of its three gradients, and the inputs the GPU tests run on (tests/test_fa_attention_gpu.py) -- kept here so that
the CPU test (tests/test_fa_attention_defs.py) can evaluate the fp32 definition on exactly those inputs.

    t_e,h      = tanh(p_src[u,h] + p_dst[v,h])                      e = (u -> v)
    w_e,h      = t_e,h * s_src[u] * s_dst[v]                        (s_src, s_dst: constants, no gradient)
    out[v,h,:] = sum_e keep_e,h w_e,h x[u,h,:]                      (keep: grad_defs.attention_keep, or None)

Nothing here imports pgl_amd.

K (grad_defs.py, the block above FP32_DEFINITION_RATIO): max(1, 4 x the worst err / bound of this definition evaluated in fp32 torch on
the host on the GPU tests' inputs), never measured from the engine.  Measured with measure_definitions():

    family            worst err / bound of the fp32 definition      K
    fa_attention      0.070                                          1
    fa_attention_drop 0.063                                          1

(fa_attention: the hub and the classes graph over SHAPES, and the two exact cases -- worst: d x on the classes graph, 1 x 128;
fa_attention_drop: DROP_CASES -- worst: d x on the classes graph, 1 x 128, p = 0.3.  The output and the gate's gradients use a
few per cent at most: their counts carry D, what the dot product <g, x> is owed.)"""
import numpy as np
import torch

import grad_defs as D

FP32_DEFINITION_RATIO = dict(fa_attention=0.070, fa_attention_drop=0.063)
K_FAMILY = {k: max(1.0, 4.0 * v) for k, v in FP32_DEFINITION_RATIO.items()}

SHAPES = [(1, 16), (1, 32), (1, 64), (1, 128), (1, 256), (4, 8), (8, 16)]   # 16 lanes, half a tile, VEC 1, 2, 4, several heads per wave
DROP_SEEDS = {0.3: 1234, 0.9: 2 ** 32 - 5}                     # (one of them >= 2**31, passed as a Python int)
DROP_CASES = [("hub", 1, 64, 0.3), ("classes", 1, 128, 0.3), ("classes", 8, 16, 0.3), ("hub", 1, 256, 0.9), ("classes", 4, 8, 0.9)]
EXACT_HD = (1, 64)
MUTANTS = ("one_minus_t2_as_1", "dpdst_without_mask", "dx_without_sdst")


# ------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------
def _scale(s, like):
    """A per-node constant ([N] or [N, 1]; None: 1) as a detached [N, 1] column in `like`'s dtype."""
    if s is None:
        return torch.ones((like.shape[0], 1), dtype=like.dtype, device=like.device)
    return torch.as_tensor(s).detach().to(dtype=like.dtype, device=like.device).reshape(-1, 1)


def fa_aggregate(x, p_src, p_dst, s_src, s_dst, src, dst, keep=None, mutant=None, frozen=None):
    """x [N, H, D]; p_src, p_dst [N, H]; s_src, s_dst [N] (None: 1); edge e = (src_e -> dst_e); keep [E, H] in the order of the edge
    list (None: no dropout).  A row without in-edges is 0.
    mutant (tests only; each leaves the VALUE as it is):
      "one_minus_t2_as_1"   -- d tanh(z) / d z = 1 instead of 1 - t^2: the gate's gradients forget the saturation;
      "dpdst_without_mask"  -- the gradient of p_dst forgets the dropout mask (needs keep);
      "dx_without_sdst"     -- the gradient of x forgets the destination's scale."""
    mutant = mutant or {}
    ss, sd = _scale(s_src, x), _scale(s_dst, x)
    z = p_src[src] + p_dst[dst]                                   # [E, H]
    if mutant.get("one_minus_t2_as_1"):
        t = torch.tanh(z.detach()) + (z - z.detach())             # MUTANT
    else:
        t = torch.tanh(z)
    w = t * ss[src] * sd[dst]
    if keep is not None:
        keep = D._keep_like(keep, x)
        if mutant.get("dpdst_without_mask"):
            # MUTANT: the path through p_dst is taken unmasked (same value: the added difference is exactly 0)
            via_dst = torch.tanh(p_src.detach()[src] + p_dst[dst]) * ss[src] * sd[dst]
            w = keep * (torch.tanh(p_src[src] + p_dst.detach()[dst]) * ss[src] * sd[dst]) + (via_dst - via_dst.detach())
        else:
            w = keep * w
    elif mutant.get("dpdst_without_mask"):
        raise ValueError("dpdst_without_mask needs a mask")
    xs = x[src]
    if mutant.get("dx_without_sdst"):
        # MUTANT: the gate weighs x[u] as it should, the gradient of x[u] is taken with w / s_dst[v]
        msg = w[:, :, None] * xs.detach() + (w.detach() / sd[dst])[:, :, None] * (xs - xs.detach())
    else:
        msg = w[:, :, None] * xs
    return torch.zeros_like(x).index_add(0, dst, msg)


def fa_closed_form(x, p_src, p_dst, s_src, s_dst, src, dst, cot, keep=None):
    """The gradients written out (the issue's formulas): with g = cot, c_e = keep_e <g[v], x[u]> and r_e = c_e s_src[u] s_dst[v]
    (1 - t_e^2):  d x[u] = sum_{e out of u} keep_e w_e g[v];  d p_src[u] = sum_{e out of u} r_e;  d p_dst[v] = sum_{e into v} r_e."""
    ss, sd = _scale(s_src, x), _scale(s_dst, x)
    t = torch.tanh(p_src[src] + p_dst[dst])
    k = torch.ones_like(t) if keep is None else D._keep_like(keep, x)
    w = k * t * ss[src] * sd[dst]
    c = k * (cot[dst] * x[src]).sum(-1)
    r = c * ss[src] * sd[dst] * (1.0 - t * t)
    dx = torch.zeros_like(x).index_add(0, src, w[:, :, None] * cot[dst])
    return dx, torch.zeros_like(p_src).index_add(0, src, r), torch.zeros_like(p_dst).index_add(0, dst, r)


def fa_reference_order(h, weight, bias, norm, src, dst):
    """FAConv as the reference writes it (pgl/nn/conv.py:1306-1339, dropout off): tanh(Linear([h_u ; h_v])) * d_u * d_v weighs h_u."""
    alpha = torch.tanh(torch.cat([h[src], h[dst]], 1) @ weight.t() + bias) * norm[src] * norm[dst]
    return torch.zeros_like(h).index_add(0, dst, h[src] * alpha)


def fa_terms(x, p_src, p_dst, s_src, s_dst, src, dst, cot, keep=None):
    """Explicit terms.  With z_e = p_src[u] + p_dst[v], t = tanh(z), q_e = s_src[u] s_dst[v], g = |cot| and
    C_e = keep_e <g[v], |x[u]|> >= |c_e|.  The rounded sum z_e moves t by (1 - t^2) |z_e| eps and 1 - t^2 by 2 |t| (1 - t^2) |z_e| eps;
    tanh itself is one rounded operation on |w_e| (inside grad_defs.bound's slack of 4 eps per term); 1 - t^2 cancels, which the 2 t^2
    pays for:
        out[v]      sum keep q (|t| + (1 - t^2) |z|) |x[u]|                          indeg + D + 4 terms
        d x[u]      sum keep q (|t| + (1 - t^2) |z|) g[v]                            outdeg + 4
        d p_src[u]  sum_{e out of u} C_e q (1 - t^2 + 2 t^2 + 2 |t| (1 - t^2) |z|)   outdeg + D + 4
        d p_dst[v]  the same terms summed over the edges into v                      indeg + D + 4
    (+ 1 each with dropout, for the multiplication by keep).
    -> dict(out=(terms, n), x=..., ps=..., pd=...) of fp64 tensors."""
    x, p_src, p_dst, cot = (t.detach().double() for t in (x, p_src, p_dst, cot))
    n, H, Dh = x.shape
    ss, sd = _scale(s_src, x).abs(), _scale(s_dst, x).abs()
    indeg, outdeg = D.degree(dst, n).double(), D.degree(src, n).double()
    z = p_src[src] + p_dst[dst]
    t = torch.tanh(z)
    q = ss[src] * sd[dst]
    one = 1.0 - t * t
    k = torch.ones_like(t) if keep is None else D._keep_like(keep, x)
    wt = k * q * (t.abs() + one * z.abs())
    g = cot.abs()
    xs_abs = x[src].abs()
    out_t = torch.zeros_like(x).index_add(0, dst, wt[:, :, None] * xs_abs)
    x_t = torch.zeros_like(x).index_add(0, src, wt[:, :, None] * g[dst])
    C = k * (g[dst] * xs_abs).sum(-1)
    rt = C * q * (one + 2.0 * t * t + 2.0 * t.abs() * one * z.abs())
    ps_t = torch.zeros_like(p_src).index_add(0, src, rt)
    pd_t = torch.zeros_like(p_dst).index_add(0, dst, rt)
    base = 4.0 if keep is None else 5.0
    ex = lambda cnt: cnt[:, None, None].expand_as(x)
    exh = lambda cnt: cnt[:, None].expand(n, H)
    return dict(out=(out_t, ex(indeg + Dh + base)), x=(x_t, ex(outdeg + base)), ps=(ps_t, exh(outdeg + Dh + base)),
                pd=(pd_t, exh(indeg + Dh + base)))


def definition_and_terms(x, p_src, p_dst, s_src, s_dst, cot, src, dst, keep=None, mutant=None):
    """-> grad_defs.GradTerms over the inputs (x, p_src, p_dst)."""
    res = fa_terms(x, p_src, p_dst, s_src, s_dst, src, dst, cot, keep)
    fn = lambda a, b, c, frozen=None: fa_aggregate(a, b, c, s_src, s_dst, src, dst, keep=keep, mutant=mutant)
    return D.grad_and_terms(fn, [x, p_src, p_dst], cot, terms={"out": res["out"], 0: res["x"], 1: res["ps"], 2: res["pd"]})


# ------------------------------------------------------------------------------------------------
# the GPU tests' inputs (numpy, so that the host measurement and the GPU tests read the same values)
# ------------------------------------------------------------------------------------------------
def _rows(rng, *shape):
    """test_gradients_gpu.rows: standard normal rows, each scaled by 10**U(-4, 0)."""
    import test_gradients_gpu as T
    return T.rows(rng, *shape)


def case_inputs(n, H, Dh, seed=0):
    """-> (x, p_src, p_dst, s_src, s_dst, cot) float32: standard-normal x; p_src, p_dst uniform in [-2, 2], so that |p_src + p_dst|
    spans 0 to about 4 -- the linear and the saturated part of tanh both occur; the scales uniform in [0.05, 1] (degree norms lie in
    (0, 1]); the cotangent in per-row scaled rows."""
    rng = np.random.default_rng(401 + 13 * H + Dh + seed)
    f = lambda v: v.astype(np.float32)
    return (f(rng.standard_normal((n, H, Dh))), f(rng.uniform(-2, 2, (n, H))), f(rng.uniform(-2, 2, (n, H))),
            f(rng.uniform(0.05, 1.0, n)), f(rng.uniform(0.05, 1.0, n)), f(_rows(rng, n, H, Dh)))


def exact_inputs(n, large=False, seed=0):
    """Products that are exact in fp32: x integers in [-4, 4], the scales powers of two in [1/8, 1].  large False: p = 0 on both
    sides, t = 0, out = 0 exactly.  large True: p_src = +-20, p_dst = 0: t = +-1 exactly in fp32 and in fp64 (1 - tanh(20) = 8e-18),
    every product a multiple of 1/64 up to 4 and every partial sum exact in any order: out is an exact signed scaled sum."""
    H, Dh = EXACT_HD
    rng = np.random.default_rng(503 + seed)
    f = lambda v: v.astype(np.float32)
    p_src = rng.choice([-20.0, 20.0], (n, H)) if large else np.zeros((n, H))
    return (f(rng.integers(-4, 5, (n, H, Dh))), f(p_src), f(np.zeros((n, H))), f(2.0 ** -rng.integers(0, 4, n)),
            f(2.0 ** -rng.integers(0, 4, n)), f(_rows(rng, n, H, Dh)))


def graph_edges(name):
    """(n, src, dst) of the GPU tests' graphs, from tests/test_gradients_gpu.py."""
    import test_gradients_gpu as T
    return T._hub_edges() if name == "hub" else T._classes_edges()


def cases():
    """(family, what, graph, inputs(n) -> (x, p_src, p_dst, s_src, s_dst, cot), p) of every bound-checked GPU case."""
    out = []
    for graph in ("hub", "classes"):
        for H, Dh in SHAPES:
            out.append(("fa_attention", "%s %dx%d" % (graph, H, Dh), graph, (lambda n, H=H, Dh=Dh: case_inputs(n, H, Dh)), 0.0))
    out.append(("fa_attention", "hub exact, t = 0", "hub", (lambda n: exact_inputs(n, False)), 0.0))
    out.append(("fa_attention", "classes exact, t = +-1", "classes", (lambda n: exact_inputs(n, True)), 0.0))
    for graph, H, Dh, p in DROP_CASES:
        out.append(("fa_attention_drop", "%s %dx%d p=%g" % (graph, H, Dh, p), graph, (lambda n, H=H, Dh=Dh: case_inputs(n, H, Dh)), p))
    return out


def measure_definitions(verbose=True):
    """-> {family: the worst err / bound of the fp32 definition (torch on the host) over the family's cases}: the output and the three
    gradients.  No engine involved."""
    worst, edges = {}, {}
    for family, what, graph, make, p in cases():
        if graph not in edges:
            n, src, dst = graph_edges(graph)
            edges[graph] = (n, torch.as_tensor(src.astype(np.int64)), torch.as_tensor(dst.astype(np.int64)))
        n, src, dst = edges[graph]
        x, ps, pd, ss, sd, cot = (torch.as_tensor(v) for v in make(n))
        keep = None if p == 0 else torch.as_tensor(D.attention_keep(DROP_SEEDS[p], np.arange(src.shape[0]), x.shape[1], p))
        r = definition_and_terms(x, ps, pd, ss, sd, cot, src, dst, keep)
        fn = lambda a, b, c: fa_aggregate(a, b, c, ss, sd, src, dst, keep=keep)
        out32, g32 = D.evaluate(fn, [x, ps, pd], cot, torch.float32)
        assert bool(torch.isfinite(out32).all()) and all(bool(torch.isfinite(t).all()) for t in g32), what
        parts = [D.worst_ratio(out32, r.out64, r.out_abs, r.out_n)] + \
                [D.worst_ratio(g32[i], r.want64[i], r.abs_terms64[i], r.n_terms[i]) for i in range(3)]
        if verbose:
            print("%s: the fp32 definition uses %s of the bound (out, d x, d p_src, d p_dst)" % (what, ", ".join("%.4f" % v for v in parts)))
        worst[family] = max(worst.get(family, 0.0), max(parts))
    return worst
