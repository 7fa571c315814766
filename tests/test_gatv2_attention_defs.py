"""tests/gatv2_attention_defs.py held to account on the host: the definition against an independent restatement, its autograd
against finite differences, the explicit terms against a per-edge enumeration, mutants refused by a gradient, and the recorded K
table against what the fp32 definition measures on the GPU tests' own inputs.  No GPU, no engine."""
import numpy as np
import pytest
import torch

import gatv2_attention_defs as A
import grad_defs as D


def _small_graph():
    """7 nodes, a few dozen edges: a multi-edge (1 -> 2 three times), self-loops (3 -> 3, 4 -> 4), node 6 isolated, node 0 without in-edges."""
    rng = np.random.default_rng(3)
    src = np.concatenate([[1, 1, 1, 3, 4, 0, 0], rng.integers(0, 6, 30)])
    dst = np.concatenate([[2, 2, 2, 3, 4, 5, 1], rng.integers(1, 6, 30)])
    return 7, torch.as_tensor(src), torch.as_tensor(dst)


def _data(n, H, Dh, seed):
    """-> x_src, x_dst, cot [n, H, Dh] and a [H, Dh] in fp64; no z = x_src[u] + x_dst[v] is anywhere near 0 by accident of a lattice."""
    rng = np.random.default_rng(seed)
    xs, xd, cot = (torch.as_tensor(rng.standard_normal((n, H, Dh))) for _ in range(3))
    return xs, xd, torch.as_tensor(rng.standard_normal((H, Dh))), cot


def _restated(xs, xd, a, src, dst, slope, keep=None):
    """A Python loop per destination with torch.softmax and torch's own leaky_relu: shares no line with the definition."""
    n, H, Dh = xs.shape
    out = torch.zeros_like(xs)
    for i in range(n):
        es = [e for e in range(src.shape[0]) if int(dst[e]) == i]
        if not es:
            continue
        us = torch.as_tensor([int(src[e]) for e in es])
        for h in range(H):
            s = torch.nn.functional.leaky_relu(xs[us, h] + xd[i, h], slope) @ a[h]
            w = torch.softmax(s, 0)
            if keep is not None:
                w = w * torch.as_tensor(np.asarray(keep)[es, h], dtype=w.dtype)
            out[i, h] = w @ xs[us, h]
    return out


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_the_definition_equals_a_loop_over_destinations(p):
    n, src, dst = _small_graph()
    xs, xd, a, _ = _data(n, 3, 4, 1)
    keep = None if p == 0 else D.attention_keep(77, np.arange(src.shape[0]), 3, p)
    got, alpha, m, sm = A.gatv2_attention(xs, xd, a, src, dst, 0.2, keep=keep, parts=True)
    want = _restated(xs, xd, a, src, dst, 0.2, keep)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-14)
    assert torch.allclose(A.gatv2_attention(xs, xs, a, src, dst, 0.3, keep=keep), _restated(xs, xs, a, src, dst, 0.3, keep), rtol=1e-12, atol=1e-14)
    assert bool((got[0] == 0).all()) and bool((got[6] == 0).all())            # rows without in-edges: 0, and so are their statistics
    assert bool((m[0] == 0).all()) and bool((sm[0] == 0).all()) and bool((m[6] == 0).all()) and bool((sm[6] == 0).all())
    s = (a * A.leaky(xs[src] + xd[dst], 0.2)).sum(-1)
    for i in range(1, 6):
        assert torch.equal(m[i], s[dst == i].max(0).values)
        assert torch.allclose(sm[i], torch.exp(s[dst == i] - m[i]).sum(0), rtol=1e-12)
    if keep is not None:
        assert bool((np.asarray(keep) == 0).any()) and not torch.allclose(got, A.gatv2_attention(xs, xd, a, src, dst, 0.2))


def test_the_kink_has_the_slope_as_its_derivative():
    """L'(0) = slope: torch's leaky_relu, and what pglamd_add_score_backward takes (z > 0 ? 1 : slope)."""
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    A.leaky(z, 0.2).sum().backward()
    assert torch.equal(z.grad, torch.full((3,), 0.2, dtype=torch.float64))
    z2 = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.leaky_relu(z2, 0.2).sum().backward()
    assert torch.equal(z2.grad, z.grad)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shared", [False, True])
def test_gradcheck_the_definition(p, shared):
    """fp64 finite differences; the inputs are continuous random numbers, so every |z| is far above eps (asserted)."""
    n, src, dst = _small_graph()
    xs, xd, a, _ = _data(n, 2, 4, 2)
    if shared:
        xd = xs
    assert float((xs[src] + xd[dst]).abs().min()) > 1e-4
    keep = None if p == 0 else D.attention_keep(5, np.arange(src.shape[0]), 2, p)
    if shared:
        ins = [t.clone().requires_grad_(True) for t in (xs, a)]
        fn = lambda x, w: A.gatv2_attention(x, x, w, src, dst, 0.2, keep=keep)
    else:
        ins = [t.clone().requires_grad_(True) for t in (xs, xd, a)]
        fn = lambda x, y, w: A.gatv2_attention(x, y, w, src, dst, 0.2, keep=keep)
    assert torch.autograd.gradcheck(fn, ins, eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_terms_equal_a_per_edge_enumeration_and_dominate(p):
    """Every term sum restated with Python loops over the edges; and each |gradient| (and the output) lies below its term sum."""
    n, src, dst = _small_graph()
    H, Dh, slope = 2, 4, 0.2
    xs, xd, a, cot = _data(n, H, Dh, 4)
    E = src.shape[0]
    keep = None if p == 0 else D.attention_keep(9, np.arange(E), H, p)
    kp = np.ones((E, H)) if keep is None else np.asarray(keep, np.float64)
    res = A.gatv2_attention_terms(xs, xd, a, src, dst, cot, slope, keep)
    _, alpha, m, sm = A.gatv2_attention(xs, xd, a, src, dst, slope, parts=True)
    g = cot.abs()
    T = torch.zeros(E, H, dtype=torch.float64)
    S = torch.zeros(n, H, dtype=torch.float64)
    Ae = torch.zeros(E, H, dtype=torch.float64)
    Amax = torch.zeros(n, H, dtype=torch.float64)
    want = {key: torch.zeros(n, H, Dh, dtype=torch.float64) for key in ("out", "xs", "xd")}
    want["a"] = torch.zeros(H, Dh, dtype=torch.float64)
    want["row_sum"] = torch.zeros(n, H, dtype=torch.float64)
    lk = lambda z: z if z > 0 else slope * z
    for e in range(E):
        u, i = int(src[e]), int(dst[e])
        for h in range(H):
            T[e, h] = kp[e, h] * float((g[i, h] * xs[u, h].abs()).sum())
            S[i, h] += alpha[e, h] * T[e, h]
            Ae[e, h] = sum(abs(float(a[h, d])) * abs(lk(float(xs[u, h, d] + xd[i, h, d]))) for d in range(Dh))
            Amax[i, h] = max(float(Amax[i, h]), float(Ae[e, h]))
    for e in range(E):
        u, i = int(src[e]), int(dst[e])
        for h in range(H):
            al = float(alpha[e, h])
            c = al * (T[e, h] + S[i, h])
            want["out"][i, h] += kp[e, h] * al * xs[u, h].abs()
            want["xs"][u, h] += kp[e, h] * al * g[i, h]
            want["row_sum"][i, h] += al * float(sm[i, h]) * (1.0 + Ae[e, h] + Amax[i, h])
            for d in range(Dh):
                z = float(xs[u, h, d] + xd[i, h, d])
                through = c * abs(float(a[h, d])) * (1.0 if z > 0 else slope)
                want["xs"][u, h, d] += through
                want["xd"][i, h, d] += through
                want["a"][h, d] += c * abs(lk(z))
    want["row_max"] = Amax
    indeg, outdeg = np.bincount(dst.numpy(), minlength=n), np.bincount(src.numpy(), minlength=n)
    reach = np.array([max([indeg[int(dst[e])] for e in range(E) if int(src[e]) == u], default=0) for u in range(n)])
    base = 4 + (p > 0)
    counts = dict(out=2 * indeg + Dh + base, xd=2 * indeg + 2 * Dh + base, xs=outdeg + reach + 2 * Dh + base, row_sum=indeg + Dh + 4)
    for key in want:
        assert torch.allclose(res[key][0], want[key], rtol=1e-12, atol=1e-300), key
    for key in counts:
        assert np.array_equal(res[key][1].reshape(n, -1)[:, 0].numpy(), counts[key].astype(np.float64)), key
    assert bool((res["a"][1] == E + indeg.max() + 2 * Dh + base).all()) and bool((res["row_max"][1] == Dh + 2).all())
    for shared in (False, True):
        r, _ = A.definition_and_terms(xs, None if shared else xd, a, cot, src, dst, slope, keep)
        assert bool((r.out64.abs() <= r.out_abs * (1 + 1e-12)).all())
        for i in range(len(r.want64)):
            assert bool((r.want64[i].abs() <= r.abs_terms64[i] * (1 + 1e-12)).all()), (shared, i)
    assert bool((m.abs() <= Amax * (1 + 1e-12)).all())                # |s| <= A for every edge, so for the maximum too


def _mutant_graph(seed=11, n=400, e=6000):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    return n, torch.as_tensor(src), torch.as_tensor(dst)


def _flagged(mutant, keep_p, H=4, Dh=8):
    """Per input (x_src, x_dst, a): how many elements of the MUTANT's fp64 gradient lie outside the K-fold fp32 bound of the true
    definition."""
    n, src, dst = _mutant_graph()
    xs, xd, a, cot, slope = (torch.as_tensor(v) if isinstance(v, np.ndarray) else v for v in A.case_inputs(n, H, Dh, seed=5))
    keep = None if keep_p == 0 else D.attention_keep(21, np.arange(src.shape[0]), H, keep_p)
    r, _ = A.definition_and_terms(xs, xd, a, cot, src, dst, slope, keep)
    _, bad = D.evaluate(lambda x, y, w: A.gatv2_attention(x, y, w, src, dst, slope, keep=keep, mutant=mutant), [xs, xd, a], cot)
    out_bad = A.gatv2_attention(xs.double(), xd.double(), a.double(), src, dst, slope, keep=keep, mutant=mutant)
    K = max(A.K_FAMILY.values())
    assert D.count_out_of_bound(out_bad, r.out64, r.out_abs, r.out_n, K=K) == 0, "a mutant changes gradients only"
    return [D.count_out_of_bound(bad[i], r.want64[i], r.abs_terms64[i], r.n_terms[i], K=K) for i in range(3)]


def test_a_gradient_of_a_that_takes_the_identity_for_the_negative_side_is_refused():
    dxs, dxd, da = _flagged({"da_identity_negative": True}, 0.0)
    assert da > 0 and dxs == 0 and dxd == 0, (dxs, dxd, da)


def test_a_gradient_of_x_dst_without_the_derivative_of_leaky_relu_is_refused():
    dxs, dxd, da = _flagged({"dxdst_without_lprime": True}, 0.0)
    assert dxd > 0 and dxs == 0 and da == 0, (dxs, dxd, da)


def test_a_row_term_without_the_mask_is_refused_by_every_score_gradient():
    dxs, dxd, da = _flagged({"t_without_mask": True}, 0.5)
    assert dxs > 0 and dxd > 0 and da > 0, (dxs, dxd, da)


def test_the_true_definition_passes_its_own_bound():
    assert _flagged(None, 0.5) == [0, 0, 0] and _flagged(None, 0.0) == [0, 0, 0]


def test_the_exact_case_is_exact_and_sits_on_the_kink():
    """Integers in [-4, 4] and eighths: the fp32 scores equal the fp64 ones bit for bit, many z are exactly 0 and |s| is large."""
    n, src, dst = A.graph_edges("hub")
    src, dst = torch.as_tensor(src.astype(np.int64)), torch.as_tensor(dst.astype(np.int64))
    xs, xd, a, _, slope = (torch.as_tensor(v) if isinstance(v, np.ndarray) else v for v in A.exact_inputs(n))
    z = xs[src] + xd[dst]
    s32 = (a * A.leaky(z, slope)).sum(-1)
    s64 = (a.double() * A.leaky(z.double(), slope)).sum(-1)
    assert torch.equal(s32.double(), s64)
    assert torch.equal((a * A.leaky(z, slope)).flip(-1).sum(-1), s32), "the score depends on the order of its sum"
    assert float((z == 0).double().mean()) > 0.05 and float(s64.abs().max()) >= 100.0


def test_the_k_table_is_what_the_fp32_definition_measures():
    """Re-measures gatv2_attention_defs.FP32_DEFINITION_RATIO on the GPU tests' inputs (fp32 torch on the host): a recorded value
    below what is found fails; and a ratio above 1 would mean the term formulas are wrong, not that K should grow."""
    measured = A.measure_definitions()
    print(measured)
    assert set(measured) == set(A.FP32_DEFINITION_RATIO)
    for family, ratio in measured.items():
        assert ratio <= A.FP32_DEFINITION_RATIO[family], (family, ratio, A.FP32_DEFINITION_RATIO[family])
        assert ratio < 1.0, (family, ratio)
        assert A.K_FAMILY[family] == max(1.0, 4.0 * A.FP32_DEFINITION_RATIO[family])
