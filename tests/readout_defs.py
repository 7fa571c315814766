"""The DEFINITION of the fused attention read-out (pgl_amd/csrc/readout.hip, pgl_amd.readout_ops.attention_readout,
GlobalAttention(fused=True), Set2Set(fused=True)) in plain torch, the explicit terms that bound a finite-precision evaluation of it and
of its gradients, and the inputs the GPU tests run on (tests/test_readout_gpu.py) -- kept here so that the CPU test
(tests/test_readout_defs.py) can evaluate the fp32 definition on exactly those inputs.

    s_i    = score[i]                  (gate mode)          i in segment g = rows seg_ptr[g] .. seg_ptr[g + 1] - 1
    s_i    = <x[i, :], q[g, :]>        (query mode, q [S, d])
    a_i    = exp(s_i - max_g s) / sum_{j in g} exp(s_j - max_g s)
    out[g] = sum_{i in g} a_i x[i, :]                       an empty segment gives 0

Nothing here imports pgl_amd.

The terms.  A weight a_i is exp of a difference over a sum of n_g such values: its relative error is a few eps for the exponential
and the division, n_g eps for the sum, and |s_i - max| eps for the rounding of the difference (grad_defs.segment_softmax_terms: the
factor 1 + |s - max|).  In query mode s_i is itself a rounded dot of d terms: an ABSOLUTE error of up to d eps sigma_i, sigma_i =
<|x[i]|, |q[g]|>, which is a relative error of the weight -- so the factor is e_i = 1 + |s_i - max| + sigma_i there and the count
grows by d.  With g = |cotangent|, T_i = <g[g], |x[i]|> and C_g = sum_{j in g} a_j e_j T_j (ds_i = a_i (t_i - c_g) is a difference of
a dot and of a sum of dots):
    out[g]        sum_i a_i e_i |x[i]|                       n = 2 n_g + 4 (+ d)
    d x[i]        a_i e_i g[g]  (+ a_i e_i (T_i + C_g) |q[g]|)     n = 2 n_g + 4     (query: 2 n_g + 3 d + 5)
    d score[i]    a_i e_i (T_i + C_g)                        n = 2 n_g + 2 d + 4
    d q[g]        sum_i a_i e_i (T_i + C_g) |x[i]|           n = 3 n_g + 3 d + 4
A row whose score is -inf has the weight exactly 0 and e_i = 1 (no rounding happens).

K (grad_defs.py, the block above FP32_DEFINITION_RATIO): max(1, 4 x the worst err / bound of this definition evaluated in fp32 torch on
the host on the GPU tests' inputs), never measured from the engine.  Measured with measure_definitions():

    family           worst err / bound of the fp32 definition      K
    readout_gate     0.052                                          1
    readout_query    0.022                                          1

(worst of both: the output over 70 000 segments of 0 - 3 rows at d = 4.  The counts are worst-case linear ones, as everywhere in
grad_defs: the wide rows use a small part of their bound.)"""
import numpy as np
import torch

import grad_defs as D

FP32_DEFINITION_RATIO = dict(readout_gate=0.052, readout_query=0.022)
K_FAMILY = {k: max(1.0, 4.0 * v) for k, v in FP32_DEFINITION_RATIO.items()}

PIECE = 256                                        # pgl_amd.readout_ops.READOUT_PIECE (tests/test_readout_defs.py compares them)
LENGTHS = [0, 1, 2, 3, 63, 64, 65, PIECE - 1, PIECE, PIECE + 1, 3 * PIECE + 5]
WIDTHS = (1, 6, 64, 100, 512)                      # the scalar path, the fixture width, the vector path, not a power of two, the cap
MANY_SEGMENTS, MANY_D = 70000, 4                   # more pieces than one launch has waves


# ------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------
def seg_ptr_of(lengths):
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(lengths, dtype=np.int64))])


def segment_ids(seg_ptr, device=None):
    seg_ptr = torch.as_tensor(np.asarray(seg_ptr), dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(seg_ptr.shape[0] - 1), seg_ptr[1:] - seg_ptr[:-1]).to(device or "cpu")


def attention_readout(x, seg_ptr, score=None, query=None, frozen=None, return_parts=False):
    """x [N, d]; exactly one of score [N] and query [S, d] -> out [S, d] (return_parts: also the weights a [N] and s - max [N])."""
    assert (score is None) != (query is None)
    S = len(seg_ptr) - 1
    ids = segment_ids(seg_ptr, x.device)
    s = score if query is None else (x * query[ids]).sum(-1)
    m = torch.full((S,), -float("inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, ids, s.detach(), "amax", include_self=True)
    p = torch.exp(s - m[ids])
    z = torch.zeros(S, dtype=s.dtype, device=s.device).index_add(0, ids, p)
    a = p / z[ids]
    out = torch.zeros((S, x.shape[1]), dtype=x.dtype, device=x.device).index_add(0, ids, a[:, None] * x)
    return (out, a, s - m[ids]) if return_parts else out


def readout_terms(x, seg_ptr, cot, score=None, query=None):
    """The explicit terms of the module docstring -> dict(out=(terms, n), x=..., operand=...) of fp64 tensors."""
    x, cot = x.detach().double(), cot.detach().double()
    score = None if score is None else score.detach().double()
    query = None if query is None else query.detach().double()
    S, d = len(seg_ptr) - 1, x.shape[1]
    ids = segment_ids(seg_ptr, x.device)
    n_g = torch.as_tensor(np.diff(np.asarray(seg_ptr)), dtype=torch.float64, device=x.device)
    _, a, diff = attention_readout(x, seg_ptr, score=score, query=query, return_parts=True)
    e = 1.0 + torch.where(torch.isfinite(diff), diff.abs(), torch.zeros_like(diff))
    extra = 0.0
    if query is not None:
        e = e + (x.abs() * query.abs()[ids]).sum(-1)
        extra = float(d)
    ae, g = a * e, cot.abs()
    seg_sum = lambda v: torch.zeros((S,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device).index_add(0, ids, v)
    T = (g[ids] * x.abs()).sum(-1)
    C = seg_sum(ae * T)
    w = ae * (T + C[ids])
    ex = lambda cnt, like: cnt[:, None].expand_as(like)
    out = (seg_sum(ae[:, None] * x.abs()), ex(2 * n_g + 4 + extra, cot))
    if query is None:
        return dict(out=out, x=(ae[:, None] * g[ids], ex(2 * n_g[ids] + 4, x)), operand=(w, 2 * n_g[ids] + 2 * d + 4))
    return dict(out=out, x=(ae[:, None] * g[ids] + w[:, None] * query.abs()[ids], ex(2 * n_g[ids] + 3 * d + 5, x)),
                operand=(seg_sum(w[:, None] * x.abs()), ex(3 * n_g + 3 * d + 4, query)))


def definition_and_terms(x, seg_ptr, cot, score=None, query=None):
    """-> grad_defs.GradTerms of the definition on (x, score | query) with cotangent cot: fp64 values and the explicit terms."""
    t = readout_terms(x, seg_ptr, cot, score=score, query=query)
    terms = {"out": t["out"], 0: t["x"], 1: t["operand"]}
    if query is None:
        fn = lambda a, b, frozen=None: attention_readout(a, seg_ptr, score=b)
        return D.grad_and_terms(fn, [x, score], cot, terms=terms)
    fn = lambda a, b, frozen=None: attention_readout(a, seg_ptr, query=b)
    return D.grad_and_terms(fn, [x, query], cot, terms=terms)


# ------------------------------------------------------------------------------------------------
# the GPU tests' inputs (numpy, so that the host measurement and the GPU tests read the same values)
# ------------------------------------------------------------------------------------------------
def _rows(rng, *shape):
    """Standard normal rows, each scaled by 10**U(-4, 0) (as test_gradients_gpu.rows): small rows are held to small errors."""
    v = rng.standard_normal(shape)
    return v * 10.0 ** rng.uniform(-4.0, 0.0, (shape[0],) + (1,) * (len(shape) - 1))


def case_inputs(mode, lengths, d, seed=0):
    """-> (x [N, d], operand, cot [S, d]) float32.  gate: x in per-row scaled rows, score = 3 x standard normal.  query: x standard
    normal, q = standard normal / sqrt(d), so that the scores stay O(1) and the attention is not uniform."""
    S, N = len(lengths), int(np.sum(lengths))
    rng = np.random.default_rng(211 + 7 * d + 1000 * seed + (0 if mode == "gate" else 5))
    f = lambda a: a.astype(np.float32)
    if mode == "gate":
        return f(_rows(rng, N, d)), f(3.0 * rng.standard_normal(N)), f(_rows(rng, S, d))
    return f(rng.standard_normal((N, d))), f(rng.standard_normal((S, d)) / np.sqrt(d)), f(_rows(rng, S, d))


def many_lengths():
    return np.random.default_rng(5).integers(0, 4, MANY_SEGMENTS)


def exact_scores(n, seed=0):
    """Scores that are multiples of 1 / 4 in [-10, 10]: score + 1e4 and score - 1e4 are exact in fp32 (ulp(1e4) = 2**-10), so the
    shift cancels exactly in s - max."""
    return (np.random.default_rng(17 + seed).integers(-40, 41, n) / 4.0).astype(np.float32)


def cases():
    """(family, what, mode, lengths, d) of every bound-checked GPU case."""
    out = []
    for mode in ("gate", "query"):
        for d in WIDTHS:
            out.append(("readout_" + mode, "%s d=%d" % (mode, d), mode, LENGTHS, d))
        out.append(("readout_" + mode, "%s %d segments d=%d" % (mode, MANY_SEGMENTS, MANY_D), mode, many_lengths(), MANY_D))
    return out


def measure_definitions(verbose=True):
    """-> {family: the worst err / bound of the fp32 definition (torch on the host) over the family's cases}.  No engine involved."""
    worst = {}
    for family, what, mode, lengths, d in cases():
        seg_ptr = seg_ptr_of(lengths)
        x, opnd, cot = (torch.as_tensor(a) for a in case_inputs(mode, lengths, d))
        kw = (lambda b: dict(score=b)) if mode == "gate" else (lambda b: dict(query=b))
        r = definition_and_terms(x, seg_ptr, cot, **kw(opnd))
        fn = lambda a, b: attention_readout(a, seg_ptr, **kw(b))
        out32, g32 = D.evaluate(fn, [x, opnd], cot, torch.float32)
        assert bool(torch.isfinite(out32).all()) and all(bool(torch.isfinite(t).all()) for t in g32), what
        parts = [D.worst_ratio(out32, r.out64, r.out_abs, r.out_n)] + \
                [D.worst_ratio(g32[i], r.want64[i], r.abs_terms64[i], r.n_terms[i]) for i in range(2)]
        if verbose:
            print("%s: the fp32 definition uses %s of the bound (out, d x, d operand)" % (what, ", ".join("%.3f" % v for v in parts)))
        worst[family] = max(worst.get(family, 0.0), max(parts))
    return worst
