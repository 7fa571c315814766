"""tests/dot_attention_edge_defs.py held to account on the host: the definition against an independent restatement and against
dot_attention_defs at ef = 0, its autograd against finite differences, the law that ties d ef to d k + d v, the explicit terms above every
gradient, mutants refused by a gradient, the recorded K table against what the fp32 definition measures on the GPU tests' own inputs,
and the front end's source for host reads.  No GPU, no engine."""
import inspect
import re

import numpy as np
import pytest
import torch

import dot_attention_defs as A
import dot_attention_edge_defs as E
import grad_defs as D
from test_dot_attention_defs import _small_graph, _mutant_graph


def _data(n, e, H, Dh, seed):
    rng = np.random.default_rng(seed)
    q, k, v, cot = (torch.as_tensor(rng.standard_normal((n, H, Dh))) for _ in range(4))
    return q, k, v, torch.as_tensor(rng.standard_normal((e, H, Dh))), cot


def _restated(q, k, v, ef, src, dst, scale, keep=None):
    """A Python loop per destination with torch.softmax: shares no line with the definition."""
    n, H, Dh = q.shape
    out = torch.zeros_like(v)
    for i in range(n):
        es = [e for e in range(src.shape[0]) if int(dst[e]) == i]
        if not es:
            continue
        us = torch.as_tensor([int(src[e]) for e in es])
        for h in range(H):
            a = torch.softmax(scale * ((k[us, h] + ef[es, h]) @ q[i, h]), 0)
            if keep is not None:
                a = a * torch.as_tensor(np.asarray(keep)[es, h], dtype=a.dtype)
            out[i, h] = a @ (v[us, h] + ef[es, h])
    return out


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_the_definition_equals_a_loop_over_destinations(p):
    n, src, dst = _small_graph()
    q, k, v, ef, _ = _data(n, src.shape[0], 3, 4, 1)
    keep = None if p == 0 else D.attention_keep(77, np.arange(src.shape[0]), 3, p)
    got = E.dot_attention_edge(q, k, v, ef, src, dst, 0.5, keep=keep)
    assert torch.allclose(got, _restated(q, k, v, ef, src, dst, 0.5, keep), rtol=1e-12, atol=1e-14)
    assert bool((got[0] == 0).all()) and bool((got[6] == 0).all())            # rows without in-edges
    assert not torch.allclose(got, A.dot_attention(q, k, v, src, dst, 0.5, keep=keep))          # ef is read


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_gradcheck_the_definition(p):
    n, src, dst = _small_graph()
    q, k, v, ef, _ = _data(n, src.shape[0], 2, 4, 2)
    keep = None if p == 0 else D.attention_keep(5, np.arange(src.shape[0]), 2, p)
    xs = [t.clone().requires_grad_(True) for t in (q, k, v, ef)]
    assert torch.autograd.gradcheck(lambda a, b, c, e: E.dot_attention_edge(a, b, c, e, src, dst, 0.7, keep=keep), xs, eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_without_edge_features_it_is_the_parent_definition_exactly(p):
    """ef = 0: the fp64 forward and the gradients of q, k, v are dot_attention_defs.dot_attention's, bit for bit (x + 0 is exact)."""
    n, src, dst = _mutant_graph()
    q, k, v, cot, scale = (torch.as_tensor(a) if isinstance(a, np.ndarray) else a for a in A.case_inputs(n, 4, 8, seed=5))
    keep = None if p == 0 else D.attention_keep(21, np.arange(src.shape[0]), 4, p)
    zero = torch.zeros((src.shape[0], 4, 8))
    out_e, g_e = D.evaluate(lambda a, b, c, e: E.dot_attention_edge(a, b, c, e, src, dst, scale, keep=keep), [q, k, v, zero], cot)
    out_a, g_a = D.evaluate(lambda a, b, c: A.dot_attention(a, b, c, src, dst, scale, keep=keep), [q, k, v], cot)
    assert out_e.dtype == torch.float64 and torch.equal(out_e, out_a)
    for i in range(3):
        assert torch.equal(g_e[i], g_a[i]), i


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_the_edge_gradient_summed_by_source_is_dk_plus_dv(p):
    """def[e] is edge e's own contribution to dk[u] + dv[u]: index_add(def, src) == dk + dv, in fp64 to rounding."""
    n, src, dst = _mutant_graph()
    q, k, v, ef, cot, scale = (torch.as_tensor(a) if isinstance(a, np.ndarray) else a for a in E.case_inputs(n, src.shape[0], 4, 8, seed=5))
    keep = None if p == 0 else D.attention_keep(21, np.arange(src.shape[0]), 4, p)
    r = E.definition_and_terms(q, k, v, ef, cot, src, dst, scale, keep)
    dq, dk, dv, de = r.want64
    summed = torch.zeros_like(dk).index_add(0, src, de)
    terms = r.abs_terms64[1] + r.abs_terms64[2]                                # what dk + dv sums, per element
    assert bool(((summed - (dk + dv)).abs() <= 1e-13 * terms).all())
    assert float(de.abs().max()) > 0 and float(summed.abs().max()) > 0


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_terms_dominate_and_reduce_to_the_parents(p):
    """Each |value| lies below its term sum; and at ef = 0 the term sums are dot_attention_defs.dot_attention_terms' with one more
    term per count."""
    n, src, dst = _small_graph()
    H, Dh, scale = 2, 4, 0.6
    q, k, v, ef, cot = _data(n, src.shape[0], H, Dh, 4)
    keep = None if p == 0 else D.attention_keep(9, np.arange(src.shape[0]), H, p)
    r = E.definition_and_terms(q, k, v, ef, cot, src, dst, scale, keep)
    assert bool((r.out64.abs() <= r.out_abs * (1 + 1e-12)).all())
    for i in range(4):
        assert bool((r.want64[i].abs() <= r.abs_terms64[i] * (1 + 1e-12)).all()), i
    assert tuple(r.abs_terms64[3].shape) == tuple(ef.shape) and tuple(r.n_terms[3].shape) == tuple(ef.shape)
    assert torch.equal(r.n_terms[3][:, 0, 0], r.n_terms[0][dst][:, 0, 0])       # def[e] carries dq's count of its destination
    res0 = E.dot_attention_edge_terms(q, k, v, torch.zeros_like(ef), src, dst, cot, scale, keep)
    par = A.dot_attention_terms(q, k, v, src, dst, cot, scale, keep)
    for key in ("out", "q", "k", "v"):
        assert torch.allclose(res0[key][0], par[key][0], rtol=1e-12, atol=1e-300), key
        assert torch.equal(res0[key][1], par[key][1] + 1), key


def _flagged(mutant, keep_p, H=4, Dh=8):
    """Per input: how many elements of the MUTANT's fp64 gradient lie outside the K-fold fp32 bound of the true definition."""
    n, src, dst = _mutant_graph()
    q, k, v, ef, cot, scale = (torch.as_tensor(a) if isinstance(a, np.ndarray) else a for a in E.case_inputs(n, src.shape[0], H, Dh, seed=5))
    keep = None if keep_p == 0 else D.attention_keep(21, np.arange(src.shape[0]), H, keep_p)
    r = E.definition_and_terms(q, k, v, ef, cot, src, dst, scale, keep)
    fn = lambda a, b, c, e: E.dot_attention_edge(a, b, c, e, src, dst, scale, keep=keep, mutant=mutant)
    out_bad, bad = D.evaluate(fn, [q, k, v, ef], cot)
    K = max(E.K_FAMILY.values())
    assert D.count_out_of_bound(out_bad, r.out64, r.out_abs, r.out_n, K=K) == 0, "a mutant changes gradients only"
    return [D.count_out_of_bound(bad[i], r.want64[i], r.abs_terms64[i], r.n_terms[i], K=K) for i in range(4)]


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_an_edge_gradient_without_its_score_term_is_refused(p):
    dq, dk, dv, de = _flagged({"def_without_score": True}, p)
    assert de > 0 and dq == 0 and dk == 0 and dv == 0, (dq, dk, dv, de)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_an_edge_gradient_without_its_value_term_is_refused(p):
    dq, dk, dv, de = _flagged({"def_without_value": True}, p)
    assert de > 0 and dq == 0 and dk == 0 and dv == 0, (dq, dk, dv, de)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_a_row_term_without_the_edge_feature_is_refused_by_the_score_gradients(p):
    dq, dk, dv, de = _flagged({"t_without_ef": True}, p)
    assert dq > 0 and dk > 0 and de > 0 and dv == 0, (dq, dk, dv, de)


def test_the_true_definition_passes_its_own_bound():
    assert _flagged(None, 0.5) == [0, 0, 0, 0] and _flagged(None, 0.0) == [0, 0, 0, 0]


def test_the_k_table_is_what_the_fp32_definition_measures():
    """Re-measures dot_attention_edge_defs.FP32_DEFINITION_RATIO on the GPU tests' inputs (fp32 torch on the host): a recorded value
    below what is found fails, one more than twice it too; and a ratio above 1 would mean the term formulas are wrong, not that K should grow."""
    measured = E.measure_definitions()
    print(measured)
    assert set(measured) == set(E.FP32_DEFINITION_RATIO) == {"dot_attention_edge", "dot_attention_edge_drop"}
    for family, ratio in measured.items():
        assert ratio <= E.FP32_DEFINITION_RATIO[family], (family, ratio, E.FP32_DEFINITION_RATIO[family])
        assert ratio >= 0.5 * E.FP32_DEFINITION_RATIO[family], (family, ratio)    # (nor is the record far above what is found)
        assert ratio < 1.0, (family, ratio)
        assert E.K_FAMILY[family] == max(1.0, 4.0 * E.FP32_DEFINITION_RATIO[family])


def test_the_inputs_are_the_parents_plus_the_edge_feature():
    q, k, v, ef, cot, scale = E.case_inputs(50, 70, 4, 8, seed=2)
    for a, b in zip((q, k, v, cot, scale), A.case_inputs(50, 4, 8, seed=2)):
        assert np.array_equal(a, b)
    assert ef.shape == (70, 4, 8) and ef.dtype == np.float32
    mags = np.abs(ef).reshape(70, -1).max(1)
    assert mags.max() / mags.min() > 100.0                                     # per-row scaled rows
    assert E.SHAPES is A.SHAPES and E.DROP_CASES is A.DROP_CASES and E.DROP_SEEDS is A.DROP_SEEDS


HOST_READS = (".item()", ".tolist()", ".cpu()", ".numpy()", ".nonzero(")


@pytest.mark.parametrize("name", ["dot_attention_edge", "dot_attention_edge_backward"])
def test_the_front_end_reads_nothing_back(name):
    """The bodies of attention_ops.dot_attention_edge / _backward (and of the helper that vets ef) hold no host read of a device value."""
    from pgl_amd import attention_ops
    for fn in (getattr(attention_ops, name), attention_ops._edge_operand):
        src = inspect.getsource(fn)
        body = src.split('"""', 2)[2] if src.count('"""') >= 2 else src        # (the docstring may speak of them)
        body = re.sub(r"#.*", "", body)
        assert len(body.strip()) > 100
        for needle in HOST_READS:
            assert needle not in body, (fn.__name__, needle)
