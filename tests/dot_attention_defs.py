"""The DEFINITION of the fused dot-product attention (pgl_amd/csrc/dot_attention.hip, Graph.dot_attention, TransformerConv(fused=True))
in plain torch, written edge by edge like grad_defs._dense_gat_fp64, the explicit terms that bound a finite-precision evaluation of it
and of its three gradients, and the inputs the GPU tests run on (tests/test_dot_attention_gpu.py) -- kept here so that the CPU test
(tests/test_dot_attention_defs.py) can evaluate the fp32 definition on exactly those inputs.

    s_e,h      = scale * <q[v,h,:], k[u,h,:]>                       e = (u -> v)
    alpha_e,h  = softmax over the in-edges of v of s_e,h
    out[v,h,:] = sum_e keep_e,h alpha_e,h v[u,h,:]                  (keep: grad_defs.attention_keep, or None)

Nothing here imports pgl_amd.

K (grad_defs.py, the block above FP32_DEFINITION_RATIO): max(1, 4 x the worst err / bound of this definition evaluated in fp32 torch on
the host on the GPU tests' inputs), never measured from the engine.  Measured with measure_definitions():

    family               worst err / bound of the fp32 definition      K
    dot_attention        0.092                                          1
    dot_attention_drop   0.072                                          1

(dot_attention: the hub and the classes graph over SHAPES, and the large exact scores -- worst: d v on the classes graph, 4 x 8;
dot_attention_drop: DROP_CASES -- worst: the output on the classes graph, 4 x 8, p = 0.3.)"""
import numpy as np
import torch

import grad_defs as D

FP32_DEFINITION_RATIO = dict(dot_attention=0.092, dot_attention_drop=0.072)
K_FAMILY = {k: max(1.0, 4.0 * v) for k, v in FP32_DEFINITION_RATIO.items()}

SHAPES = [(4, 8), (8, 16), (2, 32), (1, 64), (8, 32)]          # 1, 2, 1, 1 and 4 columns per lane
DROP_SEEDS = {0.3: 1234, 0.9: 2 ** 32 - 5}                     # (one of them >= 2**31, passed as a Python int)
DROP_CASES = [("hub", 8, 16, 0.3), ("classes", 8, 16, 0.3), ("classes", 4, 8, 0.3), ("classes", 8, 32, 0.3), ("hub", 8, 16, 0.9),
              ("classes", 8, 16, 0.9)]
EXACT_HD = (8, 16)


# ------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------
def _softmax_by_dst(s, dst, n):
    """s [E, H] -> (p = exp(s - max), sum [n, H]): softmax over each destination's edges is p / sum[dst]."""
    H = s.shape[1]
    m = torch.full((n, H), -float("inf"), dtype=s.dtype, device=s.device)
    m = m.scatter_reduce(0, dst[:, None].expand(-1, H), s.detach(), "amax", include_self=True)
    p = torch.exp(s - m[dst])
    return p, torch.zeros((n, H), dtype=s.dtype, device=s.device).index_add(0, dst, p)


def dot_attention(q, k, v, src, dst, scale, keep=None, mutant=None, frozen=None, return_alpha=False):
    """q, k, v [N, H, D]; edge e = (src_e -> dst_e); keep [E, H] in the order of the edge list (None: no dropout).  A row without
    in-edges is 0.  mutant (tests only): "t_without_mask" -- the softmax row term of the gradient forgets the mask;
    "dq_without_scale" -- the gradient of q lacks the factor scale (both leave the value as it is)."""
    n = q.shape[0]
    qs = q
    if mutant and mutant.get("dq_without_scale"):
        qs = q.detach() + (q - q.detach()) / scale                # MUTANT: same value, d s / d q = k instead of scale * k
    s = scale * (qs[dst] * k[src]).sum(-1)                        # [E, H]
    p, z = _softmax_by_dst(s, dst, n)
    alpha = p / z[dst]
    if keep is None:
        out = torch.zeros_like(v).index_add(0, dst, alpha[:, :, None] * v[src])
    else:
        keep = D._keep_like(keep, v)
        if mutant and mutant.get("t_without_mask"):
            # MUTANT: d s_e = alpha_e (keep_e T_e - sum alpha_e' T_e'): alpha = p / z, the path through p gives alpha_e keep_e T_e, the
            # path through z gives the row term -- taken unmasked here (same value, same d v)
            vs = v[src]
            through_p = (keep * p / z[dst].detach())[:, :, None] * vs
            through_z = (p.detach() / z[dst])[:, :, None] * vs.detach()
            out = torch.zeros_like(v).index_add(0, dst, through_p + through_z - through_z.detach())
        else:
            out = torch.zeros_like(v).index_add(0, dst, (keep * alpha)[:, :, None] * v[src])
    return (out, alpha) if return_alpha else out


def dot_attention_terms(q, k, v, src, dst, cot, scale, keep=None):
    """Explicit terms, as grad_defs.gat_terms.  With alpha the (undropped) attention, g = |cot|, T_e = keep_e <g[v], |v[u]|> per head
    and S[v] = sum_{e into v} alpha_e T_e:
        out[v]  sum keep alpha |v[u]|                          2 indeg + D + 4 terms
        dq[v]   scale sum alpha (T_e + S[v]) |k[u]|            2 indeg + 2 D + 4
        dk[u]   scale sum alpha (T_e + S[dst_e]) |q[dst_e]|    outdeg + (max indeg over u's destinations) + 2 D + 4
        dv[u]   sum keep alpha g[dst_e]                        the same with D in place of 2 D
    (+ 1 each with dropout, for the multiplication by keep).  -> dict(out=(terms, n), q=..., k=..., v=...) of fp64 tensors."""
    q, k, v, cot = (t.detach().double() for t in (q, k, v, cot))
    n, H, Dh = q.shape
    _, alpha = dot_attention(q, k, v, src, dst, scale, return_alpha=True)
    indeg, outdeg = D.degree(dst, n).double(), D.degree(src, n).double()
    g, sc = cot.abs(), abs(float(scale))
    keep = D._keep_like(keep, v)
    w = alpha if keep is None else keep * alpha
    out_t = torch.zeros_like(v).index_add(0, dst, w[:, :, None] * v[src].abs())
    v_t = torch.zeros_like(v).index_add(0, src, w[:, :, None] * g[dst])
    T = (g[dst] * v[src].abs()).sum(-1)
    if keep is not None:
        T = keep * T
    S = torch.zeros((n, H), dtype=q.dtype, device=q.device).index_add(0, dst, alpha * T)
    c = alpha * (T + S[dst])
    q_t = sc * torch.zeros_like(q).index_add(0, dst, c[:, :, None] * k[src].abs())
    k_t = sc * torch.zeros_like(k).index_add(0, src, c[:, :, None] * q[dst].abs())
    seg_of_src = torch.zeros(n, dtype=q.dtype, device=q.device)
    if src.shape[0]:
        seg_of_src = seg_of_src.scatter_reduce(0, src, indeg[dst], "amax", include_self=True)
    base = 4.0 if keep is None else 5.0
    ex = lambda cnt: cnt[:, None, None].expand_as(q)
    return dict(out=(out_t, ex(2 * indeg + Dh + base)), q=(q_t, ex(2 * indeg + 2 * Dh + base)),
                k=(k_t, ex(outdeg + seg_of_src + 2 * Dh + base)), v=(v_t, ex(outdeg + seg_of_src + Dh + base)))


def terms_for_inputs(res):
    """dot_attention_terms' result keyed as grad_defs.grad_and_terms(terms=...) wants it for the inputs (q, k, v)."""
    return {"out": res["out"], 0: res["q"], 1: res["k"], 2: res["v"]}


def definition_and_terms(q, k, v, cot, src, dst, scale, keep=None, mutant=None):
    """-> grad_defs.GradTerms of the definition on (q, k, v) with cotangent cot: fp64 values and the explicit terms."""
    fn = lambda a, b, c, frozen=None: dot_attention(a, b, c, src, dst, scale, keep=keep, mutant=mutant)
    return D.grad_and_terms(fn, [q, k, v], cot, terms=terms_for_inputs(dot_attention_terms(q, k, v, src, dst, cot, scale, keep)))


# ------------------------------------------------------------------------------------------------
# the GPU tests' inputs (numpy, so that the host measurement and the GPU tests read the same values)
# ------------------------------------------------------------------------------------------------
def _rows(rng, *shape):
    """test_gradients_gpu.rows: standard normal rows, each scaled by 10**U(-4, 0)."""
    import test_gradients_gpu as T
    return T.rows(rng, *shape)


def case_inputs(n, H, Dh, seed=0):
    """-> (q, k, v, cot, scale) float32: standard-normal q, k with scale = D**-0.5 (attention is not uniform), v and the cotangent
    in per-row scaled rows."""
    rng = np.random.default_rng(97 + 13 * H + Dh + seed)
    f = lambda a: a.astype(np.float32)
    return f(rng.standard_normal((n, H, Dh))), f(rng.standard_normal((n, H, Dh))), f(_rows(rng, n, H, Dh)), f(_rows(rng, n, H, Dh)), float(Dh) ** -0.5


def exact_inputs(n, seed=0):
    """Large, exact scores: q, k integers in [-8, 8], D = 16, scale = 0.25 -- every product, every partial sum (<= 16 * 64) and the scaled
    score are exact in fp32 in any order, and |s| reaches about 160."""
    H, Dh = EXACT_HD
    rng = np.random.default_rng(131 + seed)
    f = lambda a: a.astype(np.float32)
    q, k = rng.integers(-8, 9, (n, H, Dh)), rng.integers(-8, 9, (n, H, Dh))
    return f(q), f(k), f(_rows(rng, n, H, Dh)), f(_rows(rng, n, H, Dh)), 0.25


def graph_edges(name):
    """(n, src, dst) of the GPU tests' graphs, from tests/test_gradients_gpu.py."""
    import test_gradients_gpu as T
    return T._hub_edges() if name == "hub" else T._classes_edges()


def cases():
    """(family, what, graph, inputs(n) -> (q, k, v, cot, scale), p) of every bound-checked GPU case."""
    out = []
    for graph in ("hub", "classes"):
        for H, Dh in SHAPES:
            out.append(("dot_attention", "%s %dx%d" % (graph, H, Dh), graph, (lambda n, H=H, Dh=Dh: case_inputs(n, H, Dh)), 0.0))
    out.append(("dot_attention", "hub exact scores", "hub", exact_inputs, 0.0))
    for graph, H, Dh, p in DROP_CASES:
        out.append(("dot_attention_drop", "%s %dx%d p=%g" % (graph, H, Dh, p), graph, (lambda n, H=H, Dh=Dh: case_inputs(n, H, Dh)), p))
    return out


def measure_definitions(verbose=True):
    """-> {family: the worst err / bound of the fp32 definition (torch on the host) over the family's cases}.  No engine involved."""
    worst, edges = {}, {}
    for family, what, graph, make, p in cases():
        if graph not in edges:
            n, src, dst = graph_edges(graph)
            edges[graph] = (n, torch.as_tensor(src.astype(np.int64)), torch.as_tensor(dst.astype(np.int64)))
        n, src, dst = edges[graph]
        q, k, v, cot, scale = (torch.as_tensor(a) if isinstance(a, np.ndarray) else a for a in make(n))
        keep = None if p == 0 else torch.as_tensor(D.attention_keep(DROP_SEEDS[p], np.arange(src.shape[0]), q.shape[1], p))
        r = definition_and_terms(q, k, v, cot, src, dst, scale, keep)
        fn = lambda a, b, c: dot_attention(a, b, c, src, dst, scale, keep=keep)
        out32, g32 = D.evaluate(fn, [q, k, v], cot, torch.float32)
        assert bool(torch.isfinite(out32).all()) and all(bool(torch.isfinite(t).all()) for t in g32), what
        parts = [D.worst_ratio(out32, r.out64, r.out_abs, r.out_n)] + \
                [D.worst_ratio(g32[i], r.want64[i], r.abs_terms64[i], r.n_terms[i]) for i in range(3)]
        if verbose:
            print("%s: the fp32 definition uses %s of the bound (out, dq, dk, dv)" % (what, ", ".join("%.3f" % x for x in parts)))
        worst[family] = max(worst.get(family, 0.0), max(parts))
    return worst
