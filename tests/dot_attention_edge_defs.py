"""The DEFINITION of the fused dot-product attention WITH EDGE FEATURES (pgl_amd/csrc/dot_attention.hip with EDGE,
Graph.dot_attention(edge_feat=...), TransformerConv(fused=True, fused_edge_feat=True)) in plain torch, written edge by edge like
dot_attention_defs.dot_attention, the explicit terms that bound a finite-precision evaluation of it and of its four gradients, and the
inputs the GPU tests run on (tests/test_dot_attention_edge_gpu.py) -- kept here so that the CPU test
(tests/test_dot_attention_edge_defs.py) can evaluate the fp32 definition on exactly those inputs.

    s_e,h      = scale * <q[v,h,:], k[u,h,:] + ef[e,h,:]>           e = (u -> v)
    alpha_e,h  = softmax over the in-edges of v of s_e,h
    out[v,h,:] = sum_e keep_e,h alpha_e,h (v[u,h,:] + ef[e,h,:])    (keep: grad_defs.attention_keep, or None)

ef [E, H, D] is in the order of the edge list.  Nothing here imports pgl_amd.

K (grad_defs.py, the block above FP32_DEFINITION_RATIO): max(1, 4 x the worst err / bound of this definition evaluated in fp32 torch on
the host on the GPU tests' inputs), never measured from the engine.  Measured with measure_definitions():

    family                    worst err / bound of the fp32 definition      K
    dot_attention_edge        0.083                                           1
    dot_attention_edge_drop   0.095                                           1

(dot_attention_edge: the hub and the classes graph over dot_attention_defs.SHAPES -- worst: the output on the classes graph, 4 x 8;
dot_attention_edge_drop: dot_attention_defs.DROP_CASES -- worst: the output on the classes graph, 4 x 8, p = 0.3.)"""
import numpy as np
import torch

import dot_attention_defs as A
import grad_defs as D

FP32_DEFINITION_RATIO = dict(dot_attention_edge=0.083, dot_attention_edge_drop=0.095)
K_FAMILY = {k: max(1.0, 4.0 * v) for k, v in FP32_DEFINITION_RATIO.items()}

SHAPES, DROP_SEEDS, DROP_CASES = A.SHAPES, A.DROP_SEEDS, A.DROP_CASES


# ------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------
def dot_attention_edge(q, k, v, ef, src, dst, scale, keep=None, mutant=None, frozen=None, return_alpha=False):
    """q, k, v [N, H, D]; ef [E, H, D]; edge e = (src_e -> dst_e); keep [E, H] in the order of the edge list (None: no dropout).  A row
    without in-edges is 0.  mutant (tests only; each leaves the VALUE as it is):
      "def_without_score" -- the gradient of ef forgets the path through the score (scale * ds_e q[v]);
      "def_without_value" -- the gradient of ef forgets the path through the value (w_e g[v]);
      "t_without_ef"      -- T_e = <g[v], v[u]> in place of <g[v], v[u] + ef_e> in every score gradient."""
    n = q.shape[0]
    mutant = mutant or {}
    kx = k[src] + (ef.detach() if mutant.get("def_without_score") else ef)
    vx = v[src] + (ef.detach() if mutant.get("def_without_value") else ef)
    s = scale * (q[dst] * kx).sum(-1)                             # [E, H]
    p, z = A._softmax_by_dst(s, dst, n)
    alpha = p / z[dst]
    w = alpha if keep is None else D._keep_like(keep, v) * alpha
    if mutant.get("t_without_ef"):
        # MUTANT: the weight's gradient reads v[u] alone (T_e without ef); the value's gradient is left as it is
        msg = w.detach()[:, :, None] * vx + (w - w.detach())[:, :, None] * v[src].detach()
    else:
        msg = w[:, :, None] * vx
    out = torch.zeros_like(v).index_add(0, dst, msg)
    return (out, alpha) if return_alpha else out


def dot_attention_edge_terms(q, k, v, ef, src, dst, cot, scale, keep=None):
    """Explicit terms: dot_attention_defs.dot_attention_terms with |k[u]| + |ef_e| in place of |k[u]|, |v[u]| + |ef_e| in place of
    |v[u]| and one more term per count for the addition.  With alpha the (undropped) attention, g = |cot|,
    T_e = keep_e <g[v], |v[u]| + |ef_e|> per head and S[v] = sum_{e into v} alpha_e T_e:
        out[v]  sum keep alpha (|v[u]| + |ef_e|)                       2 indeg + D + 5 terms
        dq[v]   scale sum alpha (T_e + S[v]) (|k[u]| + |ef_e|)         2 indeg + 2 D + 5
        dk[u]   scale sum alpha (T_e + S[dst_e]) |q[dst_e]|            outdeg + (max indeg over u's destinations) + 2 D + 5
        dv[u]   sum keep alpha g[dst_e]                                the same with D in place of 2 D
        def[e]  scale alpha_e (T_e + S[v]) |q[v]| + keep_e alpha_e g[v]     dq's count of its destination v
    (+ 1 each with dropout, for the multiplication by keep).  -> dict(out=(terms, n), q=..., k=..., v=..., ef=...) of fp64 tensors."""
    q, k, v, ef, cot = (t.detach().double() for t in (q, k, v, ef, cot))
    n, H, Dh = q.shape
    _, alpha = dot_attention_edge(q, k, v, ef, src, dst, scale, return_alpha=True)
    indeg, outdeg = D.degree(dst, n).double(), D.degree(src, n).double()
    g, sc = cot.abs(), abs(float(scale))
    keep = D._keep_like(keep, v)
    w = alpha if keep is None else keep * alpha
    ka, va = k[src].abs() + ef.abs(), v[src].abs() + ef.abs()
    out_t = torch.zeros_like(v).index_add(0, dst, w[:, :, None] * va)
    v_t = torch.zeros_like(v).index_add(0, src, w[:, :, None] * g[dst])
    T = (g[dst] * va).sum(-1)
    if keep is not None:
        T = keep * T
    S = torch.zeros((n, H), dtype=q.dtype, device=q.device).index_add(0, dst, alpha * T)
    c = alpha * (T + S[dst])
    q_t = sc * torch.zeros_like(q).index_add(0, dst, c[:, :, None] * ka)
    k_t = sc * torch.zeros_like(k).index_add(0, src, c[:, :, None] * q[dst].abs())
    ef_t = sc * c[:, :, None] * q[dst].abs() + w[:, :, None] * g[dst]
    seg_of_src = torch.zeros(n, dtype=q.dtype, device=q.device)
    if src.shape[0]:
        seg_of_src = seg_of_src.scatter_reduce(0, src, indeg[dst], "amax", include_self=True)
    base = 5.0 if keep is None else 6.0
    ex = lambda cnt, like=q: cnt[:, None, None].expand_as(like)
    n_q = 2 * indeg + 2 * Dh + base
    return dict(out=(out_t, ex(2 * indeg + Dh + base)), q=(q_t, ex(n_q)), k=(k_t, ex(outdeg + seg_of_src + 2 * Dh + base)),
                v=(v_t, ex(outdeg + seg_of_src + Dh + base)), ef=(ef_t, ex(n_q[dst], ef)))


def terms_for_inputs(res):
    """dot_attention_edge_terms' result keyed as grad_defs.grad_and_terms(terms=...) wants it for the inputs (q, k, v, ef)."""
    return {"out": res["out"], 0: res["q"], 1: res["k"], 2: res["v"], 3: res["ef"]}


def definition_and_terms(q, k, v, ef, cot, src, dst, scale, keep=None, mutant=None):
    """-> grad_defs.GradTerms of the definition on (q, k, v, ef) with cotangent cot: fp64 values and the explicit terms."""
    fn = lambda a, b, c, e, frozen=None: dot_attention_edge(a, b, c, e, src, dst, scale, keep=keep, mutant=mutant)
    return D.grad_and_terms(fn, [q, k, v, ef], cot, terms=terms_for_inputs(dot_attention_edge_terms(q, k, v, ef, src, dst, cot, scale, keep)))


# ------------------------------------------------------------------------------------------------
# the GPU tests' inputs (numpy, so that the host measurement and the GPU tests read the same values)
# ------------------------------------------------------------------------------------------------
def case_inputs(n, e, H, Dh, seed=0):
    """-> (q, k, v, ef, cot, scale) float32: dot_attention_defs.case_inputs and ef [e, H, Dh] in per-row scaled rows (a generator of its
    own: q, k, v and the cotangent are the parent module's, value for value)."""
    q, k, v, cot, scale = A.case_inputs(n, H, Dh, seed)
    rng = np.random.default_rng(211 + 13 * H + Dh + seed)
    return q, k, v, A._rows(rng, e, H, Dh).astype(np.float32), cot, scale


def cases():
    """(family, what, graph, H, Dh, p) of every bound-checked GPU case."""
    out = [("dot_attention_edge", "%s %dx%d" % (graph, H, Dh), graph, H, Dh, 0.0) for graph in ("hub", "classes") for H, Dh in SHAPES]
    return out + [("dot_attention_edge_drop", "%s %dx%d p=%g" % (graph, H, Dh, p), graph, H, Dh, p) for graph, H, Dh, p in DROP_CASES]


def measure_definitions(verbose=True):
    """-> {family: the worst err / bound of the fp32 definition (torch on the host) over the family's cases}.  No engine involved."""
    worst, edges = {}, {}
    for family, what, graph, H, Dh, p in cases():
        if graph not in edges:
            n, src, dst = A.graph_edges(graph)
            edges[graph] = (n, torch.as_tensor(src.astype(np.int64)), torch.as_tensor(dst.astype(np.int64)))
        n, src, dst = edges[graph]
        q, k, v, ef, cot, scale = (torch.as_tensor(a) if isinstance(a, np.ndarray) else a for a in case_inputs(n, src.shape[0], H, Dh))
        keep = None if p == 0 else torch.as_tensor(D.attention_keep(DROP_SEEDS[p], np.arange(src.shape[0]), H, p))
        r = definition_and_terms(q, k, v, ef, cot, src, dst, scale, keep)
        fn = lambda a, b, c, e: dot_attention_edge(a, b, c, e, src, dst, scale, keep=keep)
        out32, g32 = D.evaluate(fn, [q, k, v, ef], cot, torch.float32)
        assert bool(torch.isfinite(out32).all()) and all(bool(torch.isfinite(t).all()) for t in g32), what
        parts = [D.worst_ratio(out32, r.out64, r.out_abs, r.out_n)] + \
                [D.worst_ratio(g32[i], r.want64[i], r.abs_terms64[i], r.n_terms[i]) for i in range(4)]
        if verbose:
            print("%s: the fp32 definition uses %s of the bound (out, dq, dk, dv, def)" % (what, ", ".join("%.3f" % x for x in parts)))
        worst[family] = max(worst.get(family, 0.0), max(parts))
    return worst
