"""tests/dot_attention_defs.py held to account on the host: the definition against an independent restatement, its autograd
against finite differences, the explicit terms against a per-edge enumeration, mutants refused by a gradient, and the recorded K
table against what the fp32 definition measures on the GPU tests' own inputs.  No GPU, no engine."""
import numpy as np
import pytest
import torch

import dot_attention_defs as A
import grad_defs as D


def _small_graph():
    """7 nodes, a few dozen edges: a multi-edge (1 -> 2 three times), self-loops (3 -> 3, 4 -> 4), node 6 isolated, node 0 without in-edges."""
    rng = np.random.default_rng(3)
    src = np.concatenate([[1, 1, 1, 3, 4, 0, 0], rng.integers(0, 6, 30)])
    dst = np.concatenate([[2, 2, 2, 3, 4, 5, 1], rng.integers(1, 6, 30)])
    return 7, torch.as_tensor(src), torch.as_tensor(dst)


def _data(n, H, Dh, seed):
    rng = np.random.default_rng(seed)
    return [torch.as_tensor(rng.standard_normal((n, H, Dh))) for _ in range(4)]


def _restated(q, k, v, src, dst, scale, keep=None):
    """A Python loop per destination with torch.softmax: shares no line with the definition."""
    n, H, Dh = q.shape
    out = torch.zeros_like(v)
    for i in range(n):
        es = [e for e in range(src.shape[0]) if int(dst[e]) == i]
        if not es:
            continue
        us = torch.as_tensor([int(src[e]) for e in es])
        for h in range(H):
            a = torch.softmax(scale * (k[us, h] @ q[i, h]), 0)
            if keep is not None:
                a = a * torch.as_tensor(np.asarray(keep)[es, h], dtype=a.dtype)
            out[i, h] = a @ v[us, h]
    return out


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_the_definition_equals_a_loop_over_destinations(p):
    n, src, dst = _small_graph()
    q, k, v, _ = _data(n, 3, 4, 1)
    keep = None if p == 0 else D.attention_keep(77, np.arange(src.shape[0]), 3, p)
    got = A.dot_attention(q, k, v, src, dst, 0.5, keep=keep)
    want = _restated(q, k, v, src, dst, 0.5, keep)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-14)
    assert bool((got[0] == 0).all()) and bool((got[6] == 0).all())            # rows without in-edges
    if keep is not None:
        assert bool((np.asarray(keep) == 0).any()) and not torch.allclose(got, A.dot_attention(q, k, v, src, dst, 0.5))


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_gradcheck_the_definition(p):
    n, src, dst = _small_graph()
    q, k, v, _ = _data(n, 2, 4, 2)
    keep = None if p == 0 else D.attention_keep(5, np.arange(src.shape[0]), 2, p)
    xs = [t.clone().requires_grad_(True) for t in (q, k, v)]
    assert torch.autograd.gradcheck(lambda a, b, c: A.dot_attention(a, b, c, src, dst, 0.7, keep=keep), xs, eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_terms_equal_a_per_edge_enumeration_and_dominate(p):
    """Every term sum restated with Python loops over the edges; and each |gradient| lies below its term sum."""
    n, src, dst = _small_graph()
    H, Dh, scale = 2, 4, 0.6
    q, k, v, cot = _data(n, H, Dh, 4)
    E = src.shape[0]
    keep = None if p == 0 else D.attention_keep(9, np.arange(E), H, p)
    kp = np.ones((E, H)) if keep is None else np.asarray(keep, np.float64)
    res = A.dot_attention_terms(q, k, v, src, dst, cot, scale, keep)
    _, alpha = A.dot_attention(q, k, v, src, dst, scale, return_alpha=True)
    g = cot.abs()
    T = torch.zeros(E, H, dtype=torch.float64)
    S = torch.zeros(n, H, dtype=torch.float64)
    want = {key: torch.zeros(n, H, Dh, dtype=torch.float64) for key in ("out", "q", "k", "v")}
    for e in range(E):
        u, i = int(src[e]), int(dst[e])
        for h in range(H):
            T[e, h] = kp[e, h] * float((g[i, h] * v[u, h].abs()).sum())
            S[i, h] += alpha[e, h] * T[e, h]
    for e in range(E):
        u, i = int(src[e]), int(dst[e])
        for h in range(H):
            a = float(alpha[e, h])
            want["out"][i, h] += kp[e, h] * a * v[u, h].abs()
            want["v"][u, h] += kp[e, h] * a * g[i, h]
            want["q"][i, h] += scale * a * (T[e, h] + S[i, h]) * k[u, h].abs()
            want["k"][u, h] += scale * a * (T[e, h] + S[i, h]) * q[i, h].abs()
    indeg, outdeg = np.bincount(dst.numpy(), minlength=n), np.bincount(src.numpy(), minlength=n)
    reach = np.array([max([indeg[int(dst[e])] for e in range(E) if int(src[e]) == u], default=0) for u in range(n)])
    base = 4 + (p > 0)
    counts = dict(out=2 * indeg + Dh + base, q=2 * indeg + 2 * Dh + base, k=outdeg + reach + 2 * Dh + base, v=outdeg + reach + Dh + base)
    for key in want:
        assert torch.allclose(res[key][0], want[key], rtol=1e-12, atol=1e-300), key
        assert np.array_equal(res[key][1][:, 0, 0].numpy(), counts[key].astype(np.float64)), key
    r = A.definition_and_terms(q, k, v, cot, src, dst, scale, keep)
    assert bool((r.out64.abs() <= r.out_abs * (1 + 1e-12)).all())
    for i in range(3):
        assert bool((r.want64[i].abs() <= r.abs_terms64[i] * (1 + 1e-12)).all()), i


def _mutant_graph(seed=11, n=400, e=6000):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    return n, torch.as_tensor(src), torch.as_tensor(dst)


def _flagged(mutant, keep_p, H=4, Dh=8):
    """Per input: how many elements of the MUTANT's fp64 gradient lie outside the K-fold fp32 bound of the true definition."""
    n, src, dst = _mutant_graph()
    q, k, v, cot, scale = (torch.as_tensor(a) if isinstance(a, np.ndarray) else a for a in A.case_inputs(n, H, Dh, seed=5))
    keep = None if keep_p == 0 else D.attention_keep(21, np.arange(src.shape[0]), H, keep_p)
    r = A.definition_and_terms(q, k, v, cot, src, dst, scale, keep)
    _, bad = D.evaluate(lambda a, b, c: A.dot_attention(a, b, c, src, dst, scale, keep=keep, mutant=mutant), [q, k, v], cot)
    out_bad = A.dot_attention(q.double(), k.double(), v.double(), src, dst, scale, keep=keep, mutant=mutant)
    K = max(A.K_FAMILY.values())
    assert D.count_out_of_bound(out_bad, r.out64, r.out_abs, r.out_n, K=K) == 0, "a mutant changes gradients only"
    return [D.count_out_of_bound(bad[i], r.want64[i], r.abs_terms64[i], r.n_terms[i], K=K) for i in range(3)]


def test_a_row_term_without_the_mask_is_refused_by_the_score_gradients():
    dq, dk, dv = _flagged({"t_without_mask": True}, 0.5)
    assert dq > 0 and dk > 0 and dv == 0, (dq, dk, dv)


def test_a_query_gradient_without_the_scale_is_refused():
    dq, dk, dv = _flagged({"dq_without_scale": True}, 0.0)
    assert dq > 0 and dk == 0 and dv == 0, (dq, dk, dv)


def test_the_true_definition_passes_its_own_bound():
    assert _flagged(None, 0.5) == [0, 0, 0] and _flagged(None, 0.0) == [0, 0, 0]


def test_the_k_table_is_what_the_fp32_definition_measures():
    """Re-measures dot_attention_defs.FP32_DEFINITION_RATIO on the GPU tests' inputs (fp32 torch on the host): a recorded value
    below what is found fails; and a ratio above 1 would mean the term formulas are wrong, not that K should grow."""
    measured = A.measure_definitions()
    print(measured)
    assert set(measured) == set(A.FP32_DEFINITION_RATIO)
    for family, ratio in measured.items():
        assert ratio <= A.FP32_DEFINITION_RATIO[family], (family, ratio, A.FP32_DEFINITION_RATIO[family])
        assert ratio < 1.0, (family, ratio)
        assert A.K_FAMILY[family] == max(1.0, 4.0 * A.FP32_DEFINITION_RATIO[family])
