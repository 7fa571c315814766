"""The fused frequency-adaptive attention (pgl_amd/csrc/fa_attention.hip) and FAConv(fused=True) on the MI355X, held to the DEFINITION
of tests/fa_attention_defs.py: forward and the three gradients per element against fp64 inside the re-association bound of that
element's own terms (grad_defs.grad_and_terms with the explicit terms + gpu_common.check_grad_elements; every element, none left out),
K from the fp32 definition on the host (fa_attention_defs.K_FAMILY; tests/test_fa_attention_defs.py re-measures it).

Graphs: the 3 000-node hub and classes graphs of tests/test_gradients_gpu.py -- the classes graph has rows with 0 / 1 / 16 / 17 / 47
further pieces on BOTH streams, so the unsplit path and both fix-up passes run in the forward and in the src-sorted walk."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import fa_attention_defs as A
import grad_defs as D
from gpu_common import pgl, check_grad_elements, close_rows, host  # noqa: F401  (pgl: the fixture)
from layout_defs import misaligned, assert_same_bits
from test_gradients_gpu import _graphs, _t  # noqa: F401

pytestmark = pytest.mark.gpu

K = A.K_FAMILY
NAMES = ("d x", "d p_src", "d p_dst")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def graphs(pgl):
    return _graphs(pgl)


_REFERENCE = {}


def _reference(key, make):
    """The fp64 definition and its terms, computed once per (graph, inputs) and shared by the tests that need it; never modified."""
    if key not in _REFERENCE:
        _REFERENCE[key] = make()
    return _REFERENCE[key]


def _inputs(G, H, Dh, seed=0):
    """-> x, p_src, p_dst, s_src, s_dst, cot on the device."""
    return tuple(_t(v) for v in A.case_inputs(G.n, H, Dh, seed))


def _run(engine, inputs, cot, need=(True, True, True)):
    xs = [t.detach().requires_grad_(bool(r)) for t, r in zip(inputs, need)]
    out = engine(*xs)
    out.backward(cot)
    return out.detach(), [x.grad for x in xs]


def _check(got, r, family, what):
    out, grads = got
    check_grad_elements(out, r.out64, r.out_abs, r.out_n, K=K[family], what=what + " forward")
    for i, name in enumerate(NAMES):
        check_grad_elements(grads[i], r.want64[i], r.abs_terms64[i], r.n_terms[i], K=K[family], what="%s %s" % (what, name))


def _same(a, b, what):
    assert_same_bits(a[0], b[0], what + ": forward")
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert_same_bits(x, y, "%s: gradient %d" % (what, i))


def _op(G, ss, sd, p=0.0, seed=0):
    return lambda x, ps, pd: G.g.fa_aggregate(x, ps, pd, ss, sd, p, seed)


# ------------------------------------------------------------------------------------------------
# 1. forward and all three gradients against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["hub", "classes"])
@pytest.mark.parametrize("H,Dh", A.SHAPES)
def test_fa_aggregate_against_fp64(pgl, graphs, graph, H, Dh):
    from pgl_amd import attention_ops
    G = graphs[graph]
    assert attention_ops.fa_supported(H, Dh)
    x, ps, pd, ss, sd, cot = _inputs(G, H, Dh)
    r = _reference((graph, H, Dh), lambda: A.definition_and_terms(x, ps, pd, ss, sd, cot, G.src, G.dst))
    what = "fa_aggregate %s %dx%d" % (graph, H, Dh)
    got = _run(_op(G, ss, sd), [x, ps, pd], cot)
    _check(got, r, "fa_attention", what + " Graph.fa_aggregate")
    with torch.no_grad():                                    # without a gradient: the same launch, no autograd node
        plain = G.g.fa_aggregate(x, ps, pd, ss, sd)
    assert_same_bits(plain, got[0], what + ": the forward without gradients")
    if H == 1:                                               # the layer's shapes: feature [N, d], the gate halves [N, 1] and [N]
        flat = _run(lambda a, b, c: G.g.fa_aggregate(a, b, c, ss.reshape(-1, 1), sd.reshape(-1, 1)), [x.reshape(G.n, Dh), ps, pd.reshape(G.n)],
                    cot.reshape(G.n, Dh))
        assert tuple(flat[0].shape) == (G.n, Dh) and tuple(flat[1][0].shape) == (G.n, Dh) and tuple(flat[1][2].shape) == (G.n,)
        _same((flat[0].reshape(G.n, 1, Dh), [flat[1][0].reshape(G.n, 1, Dh), flat[1][1], flat[1][2].reshape(G.n, 1)]), got, what + ": feature [N, d]")


def test_scales_of_none_are_ones(graphs):
    G = graphs["classes"]
    x, ps, pd, _, _, cot = _inputs(G, 1, 64)
    one = torch.ones(G.n, device=x.device)
    r = A.definition_and_terms(x, ps, pd, None, None, cot, G.src, G.dst)
    got = _run(_op(G, None, None), [x, ps, pd], cot)
    _check(got, r, "fa_attention", "fa_aggregate without scales")
    _same(_run(_op(G, one, one), [x, ps, pd], cot), got, "scales of 1 against None")


@pytest.mark.parametrize("name", ["E0", "E1", "N1"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_degenerate_graphs(graphs, name, p):
    G = graphs[name]
    H, Dh = 8, 16
    x, ps, pd, ss, sd, cot = _inputs(G, H, Dh, seed=3)
    keep = None if p == 0 else _t(D.attention_keep(7, np.arange(G.e), H, p))
    family = "fa_attention_drop" if p else "fa_attention"
    r = A.definition_and_terms(x, ps, pd, ss, sd, cot, G.src, G.dst, keep)
    got = _run(_op(G, ss, sd, p, 7), [x, ps, pd], cot)
    assert tuple(got[0].shape) == (G.n, H, Dh) and [tuple(g.shape) for g in got[1]] == [(G.n, H, Dh), (G.n, H), (G.n, H)]
    _check(got, r, family, "fa_aggregate %s p=%g" % (name, p))
    if name == "E0":
        assert all(bool((t == 0).all()) for t in [got[0]] + got[1])


# ------------------------------------------------------------------------------------------------
# 2. dropout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,H,Dh,p", A.DROP_CASES)
def test_fa_aggregate_with_dropout(graphs, graph, H, Dh, p):
    """Against the definition with grad_defs.attention_keep: the forward AND the three gradients, so the backward's mask is the
    forward's."""
    G = graphs[graph]
    seed = A.DROP_SEEDS[p]
    x, ps, pd, ss, sd, cot = _inputs(G, H, Dh)
    keep = _t(D.attention_keep(seed, np.arange(G.e), H, p))
    r = A.definition_and_terms(x, ps, pd, ss, sd, cot, G.src, G.dst, keep)
    eng = lambda s: _run(_op(G, ss, sd, p, s), [x, ps, pd], cot)
    got = eng(seed)
    _check(got, r, "fa_attention_drop", "fa_aggregate %s %dx%d p=%g" % (graph, H, Dh, p))
    _same(eng(seed), got, "the same seed twice")
    assert not torch.equal(eng(seed + 1)[0], got[0]), "another seed gives the same output"


def test_no_dropout_is_the_plain_launch_whatever_the_seed(graphs):
    G = graphs["classes"]
    x, ps, pd, ss, sd, cot = _inputs(G, 1, 128)
    plain = _run(_op(G, ss, sd), [x, ps, pd], cot)
    for seed in (1, 2 ** 32 - 5):
        _same(_run(_op(G, ss, sd, 0.0, seed), [x, ps, pd], cot), plain, "p = 0, seed %d" % seed)


def test_dropout_needs_edge_ids(pgl, graphs):
    """The csr-order view of the dst-keyed index carries no edge ids: dropout over it is refused (PGLAMD_E_ARG), not run with positions."""
    from pgl_amd import attention_ops
    G = graphs["hub"]
    x, ps, pd, ss, sd, _ = _inputs(G, 1, 64)
    vd, _ = G.g._csr_order_views()
    with pytest.raises(ValueError, match=r"dropout needs .* eid.*code -6"):
        attention_ops.fa_aggregate(x, ps, pd, ss, sd, vd, 0.3, 1)


# ------------------------------------------------------------------------------------------------
# 3. empty rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["hub", "classes"])
def test_rows_without_edges_are_exactly_zero(graphs, graph):
    G = graphs[graph]
    x, ps, pd, ss, sd, cot = _inputs(G, 4, 8)
    out, (dx, dps, dpd) = _run(_op(G, ss, sd), [x, ps, pd], cot)
    no_in, no_out = G.indeg == 0, G.outdeg == 0
    assert bool(no_in.any()) and bool(no_out.any())
    assert bool((out[no_in] == 0).all()) and bool((dpd[no_in] == 0).all())
    assert bool((dps[no_out] == 0).all()) and bool((dx[no_out] == 0).all())
    assert bool((out[~no_in] != 0).any()) and bool((dps[~no_out] != 0).any())


# ------------------------------------------------------------------------------------------------
# 4. exact cases
# ------------------------------------------------------------------------------------------------
def test_a_gate_of_zero_gives_exactly_zero(graphs):
    """Integer x, power-of-two scales, p = 0 on both sides: t = 0, out = 0 and d x = 0 exactly; the gate's gradients (1 - t^2 = 1) are
    plain scaled dot products, inside the bound."""
    G = graphs["classes"]
    x, ps, pd, ss, sd, cot = (_t(v) for v in A.exact_inputs(G.n, False))
    r = A.definition_and_terms(x, ps, pd, ss, sd, cot, G.src, G.dst)
    got = _run(_op(G, ss, sd), [x, ps, pd], cot)
    assert bool((got[0] == 0).all()) and bool((got[1][0] == 0).all())
    assert float(got[1][1].abs().max()) > 0
    _check(got, r, "fa_attention", "fa_aggregate, t = 0")


def test_a_saturated_gate_is_the_plain_scaled_sum(pgl, graphs):
    """p_src = +-20: t = +-1 exactly.  (a) integer x and power-of-two scales: every product and partial sum is exact, so out equals
    ops.aggregate of the sign-flipped rows with the same scales BIT FOR BIT in any merge order -- and the fp64 definition.  (b) real x and
    scales, t = +1: the two kernels round s_src[u] * x[u] at different places (aggregate lays the source scale out per edge or
    pre-scales the rows, the fused walk multiplies the gate by it), so the sums are compared inside the bound, not bit for bit."""
    from pgl_amd import ops
    G = graphs["classes"]
    csr = G.g._csr_dst()
    x, ps, pd, ss, sd, cot = (_t(v) for v in A.exact_inputs(G.n, True))
    with torch.no_grad():
        out = G.g.fa_aggregate(x, ps, pd, ss, sd)
        sign = torch.sign(ps).reshape(G.n, 1)
        want = ops.aggregate((x.reshape(G.n, -1) * sign).contiguous(), csr, "sum", G.n, src_scale=ss, dst_scale=sd)
    assert torch.equal(out.reshape(G.n, -1), want), "exact sums differ from ops.aggregate"
    assert torch.equal(out.double(), A.fa_aggregate(x.double(), ps.double(), pd.double(), ss, sd, G.src, G.dst))
    x, _, _, ss, sd, cot = _inputs(G, 1, 128)
    big = torch.full((G.n, 1), 20.0, device=x.device)
    zero = torch.zeros((G.n, 1), device=x.device)
    r = A.definition_and_terms(x, big, zero, ss, sd, cot, G.src, G.dst)
    with torch.no_grad():
        out = G.g.fa_aggregate(x, big, zero, ss, sd)
        want = ops.aggregate(x.reshape(G.n, -1), csr, "sum", G.n, src_scale=ss, dst_scale=sd).reshape(out.shape)
    check_grad_elements(out, r.out64, r.out_abs, r.out_n, K=K["fa_attention"], what="saturated gate against fp64")
    check_grad_elements(want, r.out64, r.out_abs, r.out_n, K=K["fa_attention"], what="ops.aggregate with the same scales against fp64")


# ------------------------------------------------------------------------------------------------
# 5. bit reproducibility, and the gradients that were not asked for
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Dh", [(1, 64), (1, 256), (8, 16)])
def test_two_runs_give_identical_bits_whatever_is_asked_for(graphs, H, Dh):
    G = graphs["classes"]
    x, ps, pd, ss, sd, cot = _inputs(G, H, Dh)
    for p in (0.0, 0.3):
        eng = lambda need=(True, True, True): _run(_op(G, ss, sd, p, 11), [x, ps, pd], cot, need)
        first = eng()
        assert all(g is not None for g in first[1])
        _same(eng(), first, "two runs, p = %g" % p)
        for need in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]:
            got = eng(need)
            assert_same_bits(got[0], first[0], "forward, need %s" % (need,))
            for i in range(3):
                if need[i]:
                    assert_same_bits(got[1][i], first[1][i], "%s with need %s, p = %g" % (NAMES[i], need, p))
                else:
                    assert got[1][i] is None


def test_the_need_flags_skip_work_without_changing_the_rest(pgl, graphs):
    from pgl_amd import attention_ops
    G = graphs["classes"]
    x, ps, pd, ss, sd, cot = _inputs(G, 1, 128)
    cd, cs = G.g._csr_dst(), G.g._csr_src()
    full = attention_ops.fa_backward(cot, x, ps, pd, ss, sd, cd, cs, 0.3, 9)
    assert attention_ops.fa_backward(cot, x, ps, pd, ss, sd, cd, cs, 0.3, 9, need=(False, False, False)) == (None, None, None)
    for need in [(True, False, False), (False, True, False), (False, False, True), (False, True, True)]:
        part = attention_ops.fa_backward(cot, x, ps, pd, ss, sd, cd, cs, 0.3, 9, need=need)
        for i in range(3):
            if need[i]:
                assert_same_bits(part[i], full[i], "%s alone (need %s)" % (NAMES[i], need))
            else:
                assert part[i] is None
    with pytest.raises(ValueError, match="bipartite"):
        attention_ops.fa_aggregate(x[:-1], ps[:-1], pd[:-1], None, None, cd)


# ------------------------------------------------------------------------------------------------
# 6. operand layout
# ------------------------------------------------------------------------------------------------
def _sliced(t):
    """The values of t [..., D] as every second row of a [2 n, ..., D + 3] tensor's first D columns (t [n]: every second element)."""
    if t.dim() == 1:
        view = torch.full((2 * t.shape[0],), float("nan"), dtype=t.dtype, device=t.device)[::2]
        view.copy_(t)
        return view
    big =torch.full((2 * t.shape[0],) + tuple(t.shape[1:-1]) + (t.shape[-1] + 3,), float("nan"), dtype=t.dtype, device=t.device)
    view = big[::2, ..., :t.shape[-1]]
    view.copy_(t)
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


@pytest.mark.parametrize("H,Dh", [(1, 64), (1, 256), (8, 16)])
@pytest.mark.parametrize("layout", ["sliced", "offset-by-one-element"])
def test_operand_layout(graphs, layout, H, Dh):
    """Strided views and contiguous views one element into their storage are copied by the front end (operand layout
    contract), not refused and not read in lanes wider than their address allows: the results equal those on fresh copies bit for bit."""
    G = graphs["classes"]
    x, ps, pd, ss, sd, cot = _inputs(G, H, Dh)
    make = {"sliced": _sliced, "offset-by-one-element": misaligned}[layout]
    want = _run(_op(G, ss, sd, 0.3, 5), [t.clone() for t in (x, ps, pd)], cot.clone())
    got = _run(_op(G, make(ss), make(sd), 0.3, 5), [make(x), make(ps), make(pd)], make(cot))
    _same(got, want, "%s operands %dx%d" % (layout, H, Dh))
    for i, name in enumerate(("x", "p_src", "p_dst")):       # one operand at a time
        ops_ = [x, ps, pd]
        ops_[i] = make(ops_[i])
        _same(_run(_op(G, ss, sd, 0.3, 5), ops_, cot), want, "%s %s alone" % (layout, name))


# ------------------------------------------------------------------------------------------------
# 7. special values
# ------------------------------------------------------------------------------------------------
def test_an_infinite_gate_half_saturates_and_contributes_no_gate_gradient(graphs):
    """p_src[u] = +inf: t = 1 on every edge out of u, 1 - t^2 = 0 -- exactly what p_src[u] = 20 gives (tanhf(20) = 1 in fp32): the same
    bits everywhere, everything finite, and d p_src[u] exactly 0."""
    G = graphs["hub"]
    u = 60                                                     # the hub source
    x, ps, pd, ss, sd, cot = _inputs(G, 1, 64)
    assert int((G.src == u).sum()) > 1000
    a, b = ps.clone(), ps.clone()
    a[u], b[u] = float("inf"), 20.0
    got, ref = _run(_op(G, ss, sd), [x, a, pd], cot), _run(_op(G, ss, sd), [x, b, pd], cot)
    assert all(bool(torch.isfinite(t).all()) for t in [got[0]] + got[1])
    assert bool((got[1][1][u] == 0).all())
    _same(got, ref, "p_src = inf against p_src = 20")


@pytest.mark.parametrize("graph,H,Dh,u", [("hub", 1, 64, 1000), ("classes", 1, 256, 1500), ("classes", 8, 16, 1501)])
def test_a_nan_row_of_x_reaches_exactly_the_rows_it_has_edges_into(graphs, graph, H, Dh, u):
    """(classes, u = 1500 sends to row 4, the hub row in 47 chunks: the containment crosses both fix-up passes.)"""
    G = graphs[graph]
    x, ps, pd, ss, sd, _ = _inputs(G, H, Dh)
    assert int((G.src == u).sum()) > 0
    with torch.no_grad():
        clean = G.g.fa_aggregate(x, ps, pd, ss, sd)
        x2 = x.clone()
        x2[u] = float("nan")
        bad = G.g.fa_aggregate(x2, ps, pd, ss, sd)
    hit = torch.zeros(G.n, dtype=torch.bool, device=x.device)
    hit[G.dst[G.src == u]] = True
    assert bool(hit.any()) and not bool(hit.all())
    assert torch.equal(torch.isnan(bad), hit[:, None, None].expand_as(bad))
    assert torch.equal(bad[~hit].view(torch.int32), clean[~hit].view(torch.int32)), "a row outside the NaN's reach changed"


# ------------------------------------------------------------------------------------------------
# 8. graph replay
# ------------------------------------------------------------------------------------------------
def test_forward_and_backward_replayed_from_a_captured_graph(graphs):
    """Forward plus backward at 1 x 128 on the classes graph captured in torch.cuda.graph on ONE side stream (no parallel branches) after
    a warm-up call there, then replayed on other operand values: the bits of the eager run on those values."""
    G = graphs["classes"]
    x, ps, pd, ss, sd, cot = _inputs(G, 1, 128)
    eager = _run(_op(G, ss, sd, 0.3, 5), [x, ps, pd], cot)
    first = _inputs(G, 1, 128, seed=1)                           # what the capture sees
    xs = [t.clone().requires_grad_(True) for t in first[:3]]
    g = first[5].clone()

    def step():
        out = _op(G, ss, sd, 0.3, 5)(*xs)
        return (out,) + torch.autograd.grad(out, xs, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # warm-up: indices, workspaces
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = step()
    with torch.no_grad():
        for t, new in zip(xs + [g], (x, ps, pd, cot)):
            t.copy_(new)
        for t in res:
            t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _same((res[0], list(res[1:])), eager, "replayed from a captured graph")


# ------------------------------------------------------------------------------------------------
# 9. the layer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Dh", [(1, 48), (1, 512)])
def test_unsupported_shapes_fall_back(pgl, graphs, H, Dh):
    from pgl_amd import attention_ops
    G = graphs["hub"]
    assert not attention_ops.fa_supported(H, Dh)
    x = _t(np.random.default_rng(4).standard_normal((G.n, Dh)))
    with pytest.raises(ValueError, match=r"fa_aggregate.*code -1"):
        G.g.fa_aggregate(x, x[:, 0], x[:, 1])
    torch.manual_seed(2)
    plain = pgl.nn.FAConv(Dh, drop=0.0).cuda()
    fused = pgl.nn.FAConv(Dh, drop=0.0, fused=True).cuda()
    fused.load_state_dict(plain.state_dict())
    assert not fused._takes_fused(G.g, x)
    with torch.no_grad():
        assert_same_bits(fused(G.g, x), plain(G.g, x), "FAConv(%d): fused=True on a shape the kernels do not take" % Dh)


def test_faconv_fused_reproduces_the_reference_fixture(pgl):
    """tests/golden/layers/layer_27_FAConv.npz, generated by the reference's own FAConv: output and gradients at the tolerances
    tests/test_golden_layers.py uses for that file."""
    import json
    import test_golden_layers as TG
    z = np.load(os.path.join(HERE, "golden", "layers", "layer_27_FAConv.npz"))
    assert str(z["cls"]) == "FAConv"
    layer = pgl.nn.FAConv(fused=True, **json.loads(str(z["kwargs"])))
    TG._load_params(layer, TG._params(z))
    layer = layer.cuda().eval()
    g = pgl.Graph(edges=z["edges"], num_nodes=int(z["num_nodes"])).tensor()
    x = torch.as_tensor(z["x"]).cuda().requires_grad_(True)
    assert layer._takes_fused(g, x)
    out = layer(g, x)
    close_rows(host(out), z["out"], rtol=5 * TG.RTOL, atol_row=2 * TG.RTOL)
    TG._check_grads(layer, x, out, z, "FAConv(fused=True)")


def _within(got, want, tol, what):
    err = (got.double() - want.double()).abs()
    ratio = float((err / tol).max())
    print("%s: worst |difference| / bound %.3f" % (what, ratio))
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (what, ratio)


def _layer_run(layer, G, x, w):
    xd = x.detach().clone().requires_grad_(True)
    for prm in layer.parameters():
        prm.grad = None
    out = layer(G.g, xd)
    out.backward(w)
    return dict(out=out.detach(), d_x=xd.grad, d_weight=layer.gate.weight.grad.clone(), d_bias=layer.gate.bias.grad.clone())


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_faconv_fused_against_the_unfused_layer(pgl, graphs, d, training):
    """fused=True against fused=False from one state_dict, drop = 0, inside the bound of the definition.  Both layers form p_src and
    p_dst with the same two products (bit-equal operands), so B = the definition's bound (K x the terms of fa_attention_defs on x,
    p_src, p_dst, the degree norms and the cotangent) holds for each layer's attention output, d x, d p_src and d p_dst against fp64:
    the fused layer is held to B against fp64 directly, the two layers to 2 B against each other.  What lies behind the gate inherits
    B through it, plus the products' own rounding in each layer (n terms each, slack 4, as grad_defs.bound), with w_s | w_d the two
    halves of gate.weight:
        d gate.weight = [d p_src^T x | d p_dst^T x]:  2 (B_p^T |x| + 4 N eps |d p|^T |x|)      d gate.bias = sum_n d p_src: likewise
        d input = d x + d p_src w_s + d p_dst w_d:    2 (B_x + B_ps |w_s| + B_pd |w_d| + 4 * 3 eps (|d x| + |d p_src| |w_s| + |d p_dst| |w_d|))"""
    G = graphs["hub"]
    torch.manual_seed(7)
    plain = pgl.nn.FAConv(d, drop=0.0).cuda()
    fused = pgl.nn.FAConv(d, drop=0.0, fused=True).cuda()
    fused.load_state_dict(plain.state_dict())
    for layer in (plain, fused):
        layer.train(training)
    rng = np.random.default_rng(43)
    x, w = _t(rng.standard_normal((G.n, d))), _t(rng.standard_normal((G.n, d)))
    assert fused._takes_fused(G.g, x) and not plain._takes_fused(G.g, x)
    a, b = _layer_run(plain, G, x, w), _layer_run(fused, G, x, w)
    assert fused.last_attn_seed is None
    with torch.no_grad():
        gw = fused.gate.weight.detach()
        p_src, p_dst = x @ gw[:, :d].t() + fused.gate.bias, x @ gw[:, d:].t()
        norm = pgl.nn.functional.degree_norm(G.g).reshape(-1)
    r = A.definition_and_terms(x.reshape(G.n, 1, d), p_src, p_dst, norm, norm, w.reshape(G.n, 1, d), G.src, G.dst)
    Kf = K["fa_attention"]
    B_out = D.bound(r.out_abs, r.out_n, K=Kf).reshape(G.n, d)
    B_x, B_ps, B_pd = (D.bound(r.abs_terms64[i], r.n_terms[i], K=Kf) for i in range(3))
    B_x = B_x.reshape(G.n, d)
    dx64, dps64, dpd64 = r.want64[0].reshape(G.n, d), r.want64[1], r.want64[2]
    ws, wd = gw[:, :d].double().abs(), gw[:, d:].double().abs()                               # [1, d]
    xa = x.double().abs()
    what = "FAConv(%d) %s" % (d, "train" if training else "eval")
    _within(b["out"], r.out64.reshape(G.n, d), B_out, what + ": fused output against fp64")
    _within(b["out"], a["out"], 2 * B_out, what + ": output, fused against unfused")
    n_eps = 4.0 * G.n * D.EPS32
    tol_w = torch.cat([B_ps.t() @ xa + n_eps * (dps64.abs().t() @ xa), B_pd.t() @ xa + n_eps * (dpd64.abs().t() @ xa)], 1)
    _within(b["d_weight"], a["d_weight"], 2 * tol_w + D.TINY32, what + ": d gate.weight")
    _within(b["d_bias"], a["d_bias"], 2 * (B_ps.sum(0) + n_eps * dps64.abs().sum(0)) + D.TINY32, what + ": d gate.bias")
    tol_x = B_x + B_ps @ ws + B_pd @ wd + 12.0 * D.EPS32 * (dx64.abs() + dps64.abs() @ ws + dpd64.abs() @ wd)
    _within(b["d_x"], a["d_x"], 2 * tol_x + D.TINY32, what + ": d input")
    want_dx = dx64 + dps64 @ gw[:, :d].double() + dpd64 @ gw[:, d:].double()
    _within(b["d_x"], want_dx, tol_x + D.TINY32, what + ": fused d input against fp64")


def test_faconv_fused_in_training_mode_is_the_definition_with_the_seed_it_drew(pgl, graphs):
    """drop = 0.5, .train(): the layer's output against the definition on the layer's own operands with the keep of
    layer.last_attn_seed, per element inside the dropout family's bound.  The seed is the one torch.manual_seed fixes; two forwards draw
    different seeds; an eval forward draws nothing."""
    G = graphs["hub"]
    d = 64
    torch.manual_seed(7)
    fused = pgl.nn.FAConv(d, drop=0.5, fused=True).cuda()
    x = _t(np.random.default_rng(53).standard_normal((G.n, d)))
    fused.train()
    torch.manual_seed(1004)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(1004)
    with torch.no_grad():
        out = fused(G.g, x)
        gw = fused.gate.weight
        p_src, p_dst = x @ gw[:, :d].t() + fused.gate.bias, x @ gw[:, d:].t()
        norm = pgl.nn.functional.degree_norm(G.g).reshape(-1)
    assert fused.last_attn_seed == seed
    cot = torch.zeros((G.n, 1, d), device=x.device)

    def definition(keep, family):
        r = A.definition_and_terms(x.reshape(G.n, 1, d), p_src, p_dst, norm, norm, cot, G.src, G.dst, keep)
        return r.out64.reshape(G.n, d), D.bound(r.out_abs, r.out_n, K=K[family]).reshape(G.n, d)

    want, B = definition(_t(D.attention_keep(seed, np.arange(G.e), 1, 0.5)), "fa_attention_drop")
    _within(out, want, B, "FAConv(fused=True).train(): output")
    other, _ = definition(_t(D.attention_keep(seed + 1, np.arange(G.e), 1, 0.5)), "fa_attention_drop")
    assert float((other - want).abs().max()) > 1e-2 * float(want.abs().max())  # another seed is another mask: the comparison is not vacuous
    with torch.no_grad():
        fused(G.g, x)
    assert fused.last_attn_seed is not None and fused.last_attn_seed != seed, "two forwards drew the same seed"
    fused.eval()
    state = torch.get_rng_state()
    with torch.no_grad():
        got = fused(G.g, x)
    assert torch.equal(torch.get_rng_state(), state), "an eval forward drew from torch's generator"
    assert fused.last_attn_seed is None
    want, B = definition(None, "fa_attention")
    _within(got, want, B, "FAConv(fused=True).eval(): output")


def test_faconv_fused_takes_todays_path_over_a_bigraph(pgl, graphs):
    G = graphs["hub"]
    torch.manual_seed(7)
    plain = pgl.nn.FAConv(64, drop=0.0).cuda()
    fused = pgl.nn.FAConv(64, drop=0.0, fused=True).cuda()
    fused.load_state_dict(plain.state_dict())
    x = _t(np.random.default_rng(59).standard_normal((G.n, 64)))
    bg = pgl.BiGraph(edges=np.stack([G.src_np, G.dst_np], 1), src_num_nodes=G.n, dst_num_nodes=G.n).tensor()
    assert bg.dot_attention_rows() is None and not fused._takes_fused(bg, x)

    def outcome(layer):
        try:
            with torch.no_grad():
                return layer(bg, x)
        except Exception as err:                              # noqa: BLE001  (compared below, type and text)
            return (type(err), str(err))

    want, got = outcome(plain), outcome(fused)
    if isinstance(want, tuple):
        assert got == want, (got, want)
    else:
        assert_same_bits(got, want, "FAConv over a BiGraph")


# ------------------------------------------------------------------------------------------------
# 10. the example
# ------------------------------------------------------------------------------------------------
def test_the_example_trains_the_same_with_and_without_fused(pgl):
    """examples/train_fagcn.py, 4 epochs on a 300-node graph with drop = 0: the --fused loss trajectory against the unfused one.
    Tolerance.  One FAConv layer's fused and unfused outputs lie within 2 B of each other, B <= 4 (indeg + D + 4) eps x the sum of the
    element's |terms| (grad_defs.bound, K = 1); relative to those term sums that is rho = 8 (max indeg + D + 4) eps.  The logits go
    through num_layer such layers (the eps * h_0 skip adds nothing), and the cross entropy is 2-Lipschitz in the logits' largest
    deviation, so the first loss -- same initial parameters -- differs by about 2 num_layer rho times the ratio of term sums to
    values, which is below 8 for these inputs (tanh gates of mixed sign cancel little over a few dozen neighbours).  Every later
    epoch adds the same forward deviation on top of parameters that Adam moved by at most lr per step in either run, whatever the
    gradient's size: epoch k is allowed (k + 1) times the first epoch's budget.  tol_k = (k + 1) * 16 * num_layer * rho."""
    spec = importlib.util.spec_from_file_location("train_fagcn", os.path.join(os.path.dirname(HERE), "examples", "train_fagcn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv = ["--epochs", "4", "--nodes", "300", "--hidden_size", "16", "--feat_size", "8", "--drop", "0", "--num_layer", "2", "--quiet"]
    plain, _ = mod.train(mod.parser().parse_args(argv))
    fused, _ = mod.train(mod.parser().parse_args(argv + ["--fused"]))
    args = mod.parser().parse_args(argv)
    edges, _, _ = mod.planted_graph(args.nodes, args.classes, args.avg_degree, args.hetero, args.feat_size, args.noise, args.seed)
    max_in = int(np.bincount(edges[:, 1], minlength=args.nodes).max())
    rho = 8.0 * (max_in + args.hidden_size + 4) * D.EPS32
    assert len(plain) == len(fused) == 4 and all(np.isfinite(plain)) and plain[-1] < plain[0]
    for k, (a, b) in enumerate(zip(plain, fused)):
        tol = (k + 1) * 16.0 * args.num_layer * rho
        print("epoch %d: loss %.7f unfused, %.7f fused, |difference| %.3g, allowed %.3g" % (k, a, b, abs(a - b), tol))
        assert abs(a - b) <= tol, (k, a, b, tol)
