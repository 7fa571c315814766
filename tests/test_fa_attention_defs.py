"""tests/fa_attention_defs.py held to account on the host: the definition against the reference-order formula of FAConv, its autograd
against the closed-form gradients and finite differences, mutants refused by a gradient, the recorded K table against what the fp32
definition measures on the GPU tests' own inputs -- and what of the feature exists without a GPU: FAConv's new argument and the four
entry points in the ctypes table.  No GPU."""
import numpy as np
import pytest
import torch

import fa_attention_defs as A
import grad_defs as D


def _edges(name):
    n, src, dst = A.graph_edges(name)
    return n, torch.as_tensor(src.astype(np.int64)), torch.as_tensor(dst.astype(np.int64))


def _norm(idx, n):
    """GF.degree_norm: clip(indegree, 1) ** -0.5."""
    return torch.bincount(idx, minlength=n).clamp(min=1).double() ** -0.5


@pytest.mark.parametrize("graph", ["hub", "classes"])
def test_the_definition_equals_the_reference_order_formula(graph):
    """tanh(Linear([h_u ; h_v])) * d_u * d_v, index_add -- with the gate split as the layer splits it: p_src = h . w[:hs] + b,
    p_dst = h . w[hs:].  fp64 on both sides; the two differ by the order of one sum of 2 hs products."""
    n, src, dst = _edges(graph)
    hs = 16
    rng = np.random.default_rng(7)
    h = torch.as_tensor(rng.standard_normal((n, hs)))
    w = torch.as_tensor(rng.standard_normal((1, 2 * hs)) * 0.3)
    b = torch.as_tensor(rng.standard_normal(1))
    norm = _norm(dst, n)
    want = A.fa_reference_order(h, w, b, norm[:, None], src, dst)
    p_src, p_dst = h @ w[:, :hs].t() + b, h @ w[:, hs:].t()
    got = A.fa_aggregate(h[:, None, :], p_src, p_dst, norm, norm, src, dst).reshape(n, hs)
    terms = torch.zeros_like(h).index_add(0, dst, h[src].abs() * (norm[src] * norm[dst])[:, None])
    assert bool(((got - want).abs() <= 1e-12 * terms + 1e-300).all())
    assert bool((got[torch.bincount(dst, minlength=n) == 0] == 0).all())
    assert float(got.abs().max()) > 0.1


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("H,Dh", [(1, 16), (4, 8)])
def test_autograd_of_the_definition_equals_the_closed_form(p, H, Dh):
    n, src, dst = _edges("hub")
    x, ps, pd, ss, sd, cot = (torch.as_tensor(v).double() for v in A.case_inputs(n, H, Dh, seed=2))
    keep = None if p == 0 else D.attention_keep(31, np.arange(src.shape[0]), H, p)
    _, grads = D.evaluate(lambda a, b, c: A.fa_aggregate(a, b, c, ss, sd, src, dst, keep=keep), [x, ps, pd], cot)
    want = A.fa_closed_form(x, ps, pd, ss, sd, src, dst, cot, keep)
    res = A.fa_terms(x, ps, pd, ss, sd, src, dst, cot, keep)
    for g, w, key in zip(grads, want, ("x", "ps", "pd")):
        assert bool(((g - w).abs() <= 1e-12 * res[key][0] + 1e-300).all()), key
        assert bool((w.abs() <= res[key][0] * (1 + 1e-12)).all()), key        # the terms dominate the gradient they bound
    assert not bool(torch.isnan(grads[0]).any()) and float(grads[1].abs().max()) > 0 and float(grads[2].abs().max()) > 0


def test_gradcheck_the_definition_and_constant_scales():
    rng = np.random.default_rng(5)
    n, H, Dh = 7, 2, 3
    src = torch.as_tensor(np.concatenate([[1, 1, 1, 3, 4, 0, 0], rng.integers(0, 6, 20)]))
    dst = torch.as_tensor(np.concatenate([[2, 2, 2, 3, 4, 5, 1], rng.integers(1, 6, 20)]))
    x = torch.as_tensor(rng.standard_normal((n, H, Dh))).requires_grad_(True)
    ps, pd = (torch.as_tensor(rng.uniform(-2, 2, (n, H))).requires_grad_(True) for _ in range(2))
    ss, sd = (torch.as_tensor(rng.uniform(0.1, 1, n)).requires_grad_(True) for _ in range(2))
    keep = D.attention_keep(3, np.arange(src.shape[0]), H, 0.4)
    fn = lambda a, b, c: A.fa_aggregate(a, b, c, ss, sd, src, dst, keep=keep)
    assert torch.autograd.gradcheck(fn, [x, ps, pd], eps=1e-6, atol=1e-7)
    fn(x, ps, pd).sum().backward()
    assert ss.grad is None and sd.grad is None                        # the scales are constants
    out = A.fa_aggregate(x, ps, pd, None, None, src, dst)              # None: 1
    assert torch.equal(out, A.fa_aggregate(x, ps, pd, torch.ones(n), torch.ones(n), src, dst))
    assert bool((out[0] == 0).all()) and bool((out[6] == 0).all())    # rows without in-edges


def _flagged(mutant, keep_p, graph="hub", H=1, Dh=64):
    """Per input (x, p_src, p_dst): how many elements of the MUTANT's fp64 gradient lie outside the K-fold fp32 bound of the true
    definition, on the GPU tests' inputs."""
    n, src, dst = _edges(graph)
    x, ps, pd, ss, sd, cot = (torch.as_tensor(v) for v in A.case_inputs(n, H, Dh))
    keep = None if keep_p == 0 else D.attention_keep(A.DROP_SEEDS[keep_p], np.arange(src.shape[0]), H, keep_p)
    r = A.definition_and_terms(x, ps, pd, ss, sd, cot, src, dst, keep)
    out_bad, bad = D.evaluate(lambda a, b, c: A.fa_aggregate(a, b, c, ss, sd, src, dst, keep=keep, mutant=mutant), [x, ps, pd], cot)
    K = max(A.K_FAMILY.values())
    assert D.count_out_of_bound(out_bad, r.out64, r.out_abs, r.out_n, K=K) == 0, "a mutant changes gradients only"
    return [D.count_out_of_bound(bad[i], r.want64[i], r.abs_terms64[i], r.n_terms[i], K=K) for i in range(3)]


def test_a_gate_gradient_that_takes_one_minus_t_squared_for_one_is_refused():
    dx, dps, dpd = _flagged({"one_minus_t2_as_1": True}, 0.0)
    assert dps > 0 and dpd > 0 and dx == 0, (dx, dps, dpd)


def test_a_gradient_of_p_dst_without_the_mask_is_refused():
    dx, dps, dpd = _flagged({"dpdst_without_mask": True}, 0.3)
    assert dpd > 0 and dx == 0 and dps == 0, (dx, dps, dpd)
    with pytest.raises(ValueError):
        _flagged({"dpdst_without_mask": True}, 0.0)


def test_a_gradient_of_x_without_the_destination_scale_is_refused():
    dx, dps, dpd = _flagged({"dx_without_sdst": True}, 0.0, graph="classes", H=8, Dh=16)
    assert dx > 0 and dps == 0 and dpd == 0, (dx, dps, dpd)


def test_the_true_definition_passes_its_own_bound():
    assert _flagged(None, 0.3) == [0, 0, 0] and _flagged(None, 0.0) == [0, 0, 0]


def test_the_exact_cases_are_exact():
    """p = 0: t = 0 and out = 0 exactly; p_src = +-20: t = +-1 exactly in fp32 and in fp64, every product and partial sum exact -- the
    fp32 definition equals the fp64 one bit for bit, in either order of the sum."""
    n, src, dst = _edges("classes")
    x, ps, pd, ss, sd, _ = (torch.as_tensor(v) for v in A.exact_inputs(n, False))
    assert bool((A.fa_aggregate(x, ps, pd, ss, sd, src, dst) == 0).all())
    x, ps, pd, ss, sd, _ = (torch.as_tensor(v) for v in A.exact_inputs(n, True))
    t = torch.tanh(ps[src] + pd[dst])
    assert bool((t.abs() == 1).all()) and bool((torch.tanh((ps[src] + pd[dst]).double()).abs() == 1).all())
    o32 = A.fa_aggregate(x, ps, pd, ss, sd, src, dst)
    o64 = A.fa_aggregate(x.double(), ps.double(), pd.double(), ss, sd, src, dst)
    flip = torch.arange(src.shape[0] - 1, -1, -1)
    assert torch.equal(o32.double(), o64) and torch.equal(A.fa_aggregate(x, ps, pd, ss, sd, src[flip], dst[flip]), o32)
    assert float(o32.abs().max()) > 1.0


def test_the_k_table_is_what_the_fp32_definition_measures():
    """Re-measures fa_attention_defs.FP32_DEFINITION_RATIO on the GPU tests' inputs (fp32 torch on the host): a recorded value below
    what is found fails; and a ratio above 1 would mean the term formulas are wrong, not that K should grow."""
    measured = A.measure_definitions()
    print(measured)
    assert set(measured) == set(A.FP32_DEFINITION_RATIO)
    for family, ratio in measured.items():
        assert ratio <= A.FP32_DEFINITION_RATIO[family], (family, ratio, A.FP32_DEFINITION_RATIO[family])
        assert ratio < 1.0, (family, ratio)
        assert A.K_FAMILY[family] == max(1.0, 4.0 * A.FP32_DEFINITION_RATIO[family])


# ------------------------------------------------------------------------------------------------
# what of the feature exists without a GPU
# ------------------------------------------------------------------------------------------------
def test_the_four_entry_points_are_in_the_ctypes_table():
    from pgl_amd import _ffi
    for name in ("pglamd_fa_aggregate_workspace_bytes", "pglamd_fa_aggregate", "pglamd_fa_backward_workspace_bytes", "pglamd_fa_backward"):
        assert name in _ffi._SIGNATURES, name


def test_fa_supported_is_the_backward_lane_rule():
    from pgl_amd import attention_ops, ops
    for H, Dh in A.SHAPES:
        assert attention_ops.fa_supported(H, Dh), (H, Dh)
    for H, Dh in [(1, 48), (1, 512), (4, 128), (3, 12)]:
        assert not attention_ops.fa_supported(H, Dh), (H, Dh)
    assert all(attention_ops.fa_supported(1, d) == ops.sddmm_supported(1, d) for d in range(1, 300))


def test_faconv_takes_the_new_argument_last_and_runs_todays_code_on_cpu_input():
    """FAConv(8, fused=True) constructs; a CPU input never takes the fused path, so the layer does what fused=False does -- the same
    result, or the same refusal where the unfused code has no CPU path either."""
    import inspect
    import pgl_amd as pgl
    assert list(inspect.signature(pgl.nn.FAConv.__init__).parameters)[1:] == ["hidden_size", "drop", "fused"]
    torch.manual_seed(3)
    plain = pgl.nn.FAConv(8, drop=0.0)
    fused = pgl.nn.FAConv(8, drop=0.0, fused=True)
    assert fused.fused and not plain.fused and fused.last_attn_seed is None
    fused.load_state_dict(plain.state_dict())
    rng = np.random.default_rng(1)
    edges = np.stack([rng.integers(0, 20, 60), rng.integers(0, 20, 60)], 1).astype(np.int64)
    x = torch.as_tensor(rng.standard_normal((20, 8)).astype(np.float32))
    g = pgl.Graph(edges=edges, num_nodes=20)
    assert not fused._takes_fused(g, x)

    def outcome(layer):
        try:
            with torch.no_grad():
                return layer(g, x)
        except Exception as err:                              # noqa: BLE001  (compared below, type and text)
            return (type(err), str(err))

    want, got = outcome(plain), outcome(fused)
    if isinstance(want, tuple):
        assert got == want, (got, want)
    else:
        assert torch.equal(torch.as_tensor(got), torch.as_tensor(want))
