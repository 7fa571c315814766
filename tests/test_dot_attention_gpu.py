"""The fused dot-product attention (pgl_amd/csrc/dot_attention.hip) and TransformerConv(fused=True) on the MI355X, held to the
DEFINITION of tests/dot_attention_defs.py: forward and the three gradients per element against fp64 inside the re-association bound of
that element's own terms (grad_defs.grad_and_terms with the explicit terms + gpu_common.check_grad_elements; every element, none left
out), K from the fp32 definition on the host (dot_attention_defs.K_FAMILY; tests/test_dot_attention_defs.py re-measures it).

Graphs: the 3 000-node hub and classes graphs of tests/test_gradients_gpu.py -- the classes graph has rows with 0 / 1 / 16 / 17 / 47
further pieces on BOTH streams, so the unsplit path and both fix-up passes run in the forward, the dst-sorted and the src-sorted walk."""
import numpy as np
import pytest
import torch

import dot_attention_defs as A
import grad_defs as D
from gpu_common import pgl, check_grad_elements, close_rows, host, RTOL  # noqa: F401  (pgl: the fixture)
from layout_defs import misaligned, assert_same_bits
from test_gradients_gpu import _graphs, _t, rows  # noqa: F401

pytestmark = pytest.mark.gpu

K = A.K_FAMILY


@pytest.fixture(scope="module")
def graphs(pgl):
    return _graphs(pgl)


def _inputs(G, H, Dh, seed=0):
    q, k, v, cot, scale = A.case_inputs(G.n, H, Dh, seed)
    return _t(q), _t(k), _t(v), _t(cot), scale


def _run(engine, q, k, v, cot):
    xs = [t.detach().requires_grad_(True) for t in (q, k, v)]
    out = engine(*xs)
    out.backward(cot)
    return out.detach(), [x.grad for x in xs]


def _check(got, r, family, what):
    out, grads = got
    check_grad_elements(out, r.out64, r.out_abs, r.out_n, K=K[family], what=what + " forward")
    for i, name in enumerate(("d q", "d k", "d v")):
        check_grad_elements(grads[i], r.want64[i], r.abs_terms64[i], r.n_terms[i], K=K[family], what="%s %s" % (what, name))


def _same(a, b, what):
    assert_same_bits(a[0], b[0], what + ": forward")
    for x, y, name in zip(a[1], b[1], ("d q", "d k", "d v")):
        assert_same_bits(x, y, "%s: %s" % (what, name))


# ------------------------------------------------------------------------------------------------
# 1. forward and all three gradients against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["hub", "classes"])
@pytest.mark.parametrize("H,Dh", A.SHAPES)
def test_dot_attention_against_fp64(pgl, graphs, graph, H, Dh):
    from pgl_amd import autograd as ag
    G = graphs[graph]
    assert pgl.ops.dot_attention_supported(H, Dh)
    q, k, v, cot, scale = _inputs(G, H, Dh)
    r = A.definition_and_terms(q, k, v, cot, G.src, G.dst, scale)
    what = "dot_attention %s %dx%d" % (graph, H, Dh)
    _check(_run(lambda a, b, c: G.g.dot_attention(a, b, c, scale), q, k, v, cot), r, "dot_attention", what + " Graph.dot_attention")
    vd, vs = G.g._csr_order_views()
    _check(_run(lambda a, b, c: ag.dot_attention(a, b, c, vd, lambda: vs, scale), q, k, v, cot), r, "dot_attention", what + " csr-order views")
    with torch.no_grad():                                    # without a gradient: the forward that writes no statistics
        plain = G.g.dot_attention(q, k, v, scale)
    check_grad_elements(plain, r.out64, r.out_abs, r.out_n, K=K["dot_attention"], what=what + " forward without statistics")


# ------------------------------------------------------------------------------------------------
# 2. degenerate graphs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E0", "E1", "N1"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_degenerate_graphs(graphs, name, p):
    G = graphs[name]
    H, Dh = 8, 16
    q, k, v, cot, scale = _inputs(G, H, Dh, seed=3)
    keep = None if p == 0 else _t(D.attention_keep(7, np.arange(G.e), H, p))
    r = A.definition_and_terms(q, k, v, cot, G.src, G.dst, scale, keep)
    got = _run(lambda a, b, c: G.g.dot_attention(a, b, c, scale, p, 7), q, k, v, cot)
    assert tuple(got[0].shape) == (G.n, H, Dh) and all(tuple(g.shape) == (G.n, H, Dh) for g in got[1])
    _check(got, r, "dot_attention_drop" if p else "dot_attention", "dot_attention %s p=%g" % (name, p))
    if name == "E0":
        assert all(bool((t == 0).all()) for t in [got[0]] + got[1])


# ------------------------------------------------------------------------------------------------
# 3. dropout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,H,Dh,p", A.DROP_CASES)
def test_dot_attention_with_dropout(graphs, graph, H, Dh, p):
    G = graphs[graph]
    seed = A.DROP_SEEDS[p]
    q, k, v, cot, scale = _inputs(G, H, Dh)
    keep = _t(D.attention_keep(seed, np.arange(G.e), H, p))
    r = A.definition_and_terms(q, k, v, cot, G.src, G.dst, scale, keep)
    eng = lambda s: _run(lambda a, b, c: G.g.dot_attention(a, b, c, scale, p, s), q, k, v, cot)
    got = eng(seed)
    _check(got, r, "dot_attention_drop", "dot_attention %s %dx%d p=%g" % (graph, H, Dh, p))
    _same(eng(seed), got, "the same seed twice")
    other = eng(seed + 1)
    assert not torch.equal(other[0], got[0]), "another seed gives the same output"


def test_no_dropout_is_the_plain_launch_whatever_the_seed(graphs):
    G = graphs["classes"]
    q, k, v, cot, scale = _inputs(G, 8, 16)
    plain = _run(lambda a, b, c: G.g.dot_attention(a, b, c, scale), q, k, v, cot)
    for seed in (1, 2 ** 32 - 5):
        _same(_run(lambda a, b, c: G.g.dot_attention(a, b, c, scale, 0.0, seed), q, k, v, cot), plain, "p = 0, seed %d" % seed)


def test_dropout_needs_edge_ids(pgl, graphs):
    """The csr-order view of the dst-keyed index carries no edge ids: dropout over it is refused (PGLAMD_E_ARG), not run with positions."""
    G = graphs["hub"]
    q, k, v, _, scale = _inputs(G, 8, 16)
    vd, _ = G.g._csr_order_views()
    with pytest.raises(ValueError, match=r"dropout needs .* eid.*code -6"):
        pgl.ops.dot_attention(q, k, v, vd, scale, 0.3, 1)


# ------------------------------------------------------------------------------------------------
# 4. large, exact scores
# ------------------------------------------------------------------------------------------------
def test_large_exact_scores(graphs):
    """q, k integers in [-8, 8], D = 16, scale = 0.25: every score is exact in fp32 in any summation order and |s| reaches about 160 --
    a kernel that rescales wrongly, or exponentiates before subtracting the maximum, overflows.  Finite, and inside the same bound."""
    G = graphs["hub"]
    q, k, v, cot, scale = (_t(a) if isinstance(a, np.ndarray) else a for a in A.exact_inputs(G.n))
    s = scale * (q[G.dst].double() * k[G.src].double()).sum(-1)
    assert float(s.abs().max()) >= 100.0 and bool((s.float().double() == s).all())
    r = A.definition_and_terms(q, k, v, cot, G.src, G.dst, scale)
    got = _run(lambda a, b, c: G.g.dot_attention(a, b, c, scale), q, k, v, cot)
    assert all(bool(torch.isfinite(t).all()) for t in [got[0]] + got[1])
    _check(got, r, "dot_attention", "dot_attention exact scores")


# ------------------------------------------------------------------------------------------------
# 5. bit reproducibility
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Dh", [(4, 8), (8, 16), (8, 32)])
def test_two_runs_give_identical_bits(graphs, H, Dh):
    G = graphs["classes"]
    q, k, v, cot, scale = _inputs(G, H, Dh)
    for p in (0.0, 0.3):
        eng = lambda: _run(lambda a, b, c: G.g.dot_attention(a, b, c, scale, p, 11), q, k, v, cot)
        _same(eng(), eng(), "two runs, p = %g" % p)


# ------------------------------------------------------------------------------------------------
# 6. operand layout
# ------------------------------------------------------------------------------------------------
def _transposed(t):
    """The values of t [N, H, D] as the non-contiguous view of a [H, N, D] tensor."""
    view = t.transpose(0, 1).contiguous().transpose(0, 1)
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def _sliced(t):
    """The values of t [N, H, D] as every second row of a [2 N, H, D + 3] tensor's first D columns."""
    n, H, Dh = t.shape
    big = torch.full((2 * n, H, Dh + 3), float("nan"), dtype=t.dtype, device=t.device)
    view = big[::2, :, :Dh]
    view.copy_(t)
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


@pytest.mark.parametrize("H,Dh", [(4, 8), (8, 16), (8, 32)])
@pytest.mark.parametrize("layout", ["transposed", "sliced", "offset-by-one-element"])
def test_operand_layout(graphs, layout, H, Dh):
    """Strided views and contiguous views one element into their storage are copied by the front end (operand layout
    contract), not refused and not read in lanes wider than their address allows: the results equal those on fresh copies bit for bit."""
    G = graphs["classes"]
    q, k, v, cot, scale = _inputs(G, H, Dh)
    make = {"transposed": _transposed, "sliced": _sliced, "offset-by-one-element": misaligned}[layout]
    want = _run(lambda a, b, c: G.g.dot_attention(a, b, c, scale, 0.3, 5), *(t.clone() for t in (q, k, v, cot)))
    got = _run(lambda a, b, c: G.g.dot_attention(a, b, c, scale, 0.3, 5), make(q), make(k), make(v), make(cot))
    _same(got, want, "%s operands %dx%d" % (layout, H, Dh))
    for i, name in enumerate("qkv"):                         # one operand at a time
        ops = [q, k, v]
        ops[i] = make(ops[i])
        _same(_run(lambda a, b, c: G.g.dot_attention(a, b, c, scale, 0.3, 5), *ops, cot), want, "%s %s alone" % (layout, name))


# ------------------------------------------------------------------------------------------------
# 7. NaN containment
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,H,Dh", [("hub", 8, 16), ("classes", 4, 8), ("classes", 8, 32)])
def test_a_nan_in_k_stays_in_the_rows_that_read_it(graphs, graph, H, Dh):
    G = graphs[graph]
    q, k, v, _, scale = _inputs(G, H, Dh)
    u, h = (60, 3) if graph == "hub" else (2, 1)                 # a hub source: its edges reach split rows too
    assert int((G.src == u).sum()) > 1000
    with torch.no_grad():
        clean = G.g.dot_attention(q, k, v, scale)
        k2 = k.clone()
        k2[u, h, 0] = float("nan")
        bad = G.g.dot_attention(q, k2, v, scale)
    torch.cuda.synchronize()
    hit = torch.zeros(G.n, dtype=torch.bool, device=q.device)
    hit[G.dst[G.src == u]] = True
    want_nan = torch.zeros((G.n, H, Dh), dtype=torch.bool, device=q.device)
    want_nan[hit, h, :] = True
    assert torch.equal(torch.isnan(bad), want_nan), "the NaN reached %d elements, expected %d" % (int(torch.isnan(bad).sum()), int(want_nan.sum()))
    assert torch.equal(bad[~want_nan].view(torch.int32), clean[~want_nan].view(torch.int32)), "an element outside the NaN's reach changed"


# ------------------------------------------------------------------------------------------------
# 8. unsupported shapes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Dh", [(3, 12), (16, 32)])
def test_unsupported_shapes(pgl, graphs, H, Dh):
    G = graphs["hub"]
    assert not pgl.ops.dot_attention_supported(H, Dh)
    q, k, v, _, scale = _inputs(G, H, Dh)
    with pytest.raises(ValueError, match=r"dot_attention.*code -1"):
        pgl.ops.dot_attention(q, k, v, G.g._csr_dst(), scale)
    torch.manual_seed(2)
    plain = pgl.nn.TransformerConv(24, Dh, num_heads=H, feat_drop=0.0, attn_drop=0.0).cuda()
    fused = pgl.nn.TransformerConv(24, Dh, num_heads=H, feat_drop=0.0, attn_drop=0.0, fused=True).cuda()
    fused.load_state_dict(plain.state_dict())
    x = _t(np.random.default_rng(4).standard_normal((G.n, 24)))
    assert not fused._takes_fused(G.g, x, None)
    with torch.no_grad():
        assert_same_bits(fused(G.g, x), plain(G.g, x), "TransformerConv %dx%d: fused=True on a shape the kernels do not take" % (H, Dh))


# ------------------------------------------------------------------------------------------------
# 9. the layer
# ------------------------------------------------------------------------------------------------
LAYER_CONFIGS = {"default": {}, "gate": dict(gate=True), "head-mean": dict(concat=False),
                 "bare": dict(skip_feat=False, layer_norm=False, activation=None)}


def _layers(pgl, attn_drop=0.0, **kw):
    torch.manual_seed(7)
    plain = pgl.nn.TransformerConv(24, 8, num_heads=4, feat_drop=0.0, attn_drop=attn_drop, **kw).cuda()
    fused = pgl.nn.TransformerConv(24, 8, num_heads=4, feat_drop=0.0, attn_drop=attn_drop, fused=True, **kw).cuda()
    fused.load_state_dict(plain.state_dict())
    return plain, fused


def _rows_ratio(got, want, cancel=None):
    """The worst |got - want| over close_rows' bound at RTOL (printed before the assertion)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    row = np.abs(want).reshape(want.shape[0], -1).max(1).reshape((want.shape[0],) + (1,) * (want.ndim - 1))
    bound = RTOL * np.abs(want) + RTOL * row + (0.0 if cancel is None else RTOL * np.broadcast_to(cancel, want.shape)) + 1e-300
    return float((np.abs(got - want) / bound).max())


@pytest.mark.parametrize("config", list(LAYER_CONFIGS))
def test_transformer_conv_fused_against_the_three_op_layer(pgl, graphs, config):
    """Output, input gradient and every parameter gradient of fused=True against fused=False from one state_dict: close_rows at RTOL,
    nothing added, as test_rgcn_fused_against_fp64_and_the_loop compares its two layers.
    One exception, k.bias: its gradient is analytically ZERO (a constant added to every key shifts all scores of a row alike and the
    softmax does not see it), so both layers return rounding noise there and no relative bound applies.  It is held to RTOL of ITS OWN
    terms through close_rows' `cancel`: d k.bias[c] = sum_u d k[u, c], terms sum_u |d k[u, c]| -- d k read from the three-op layer (the
    gradient of its key projection's output)."""
    G = graphs["hub"]
    kw = LAYER_CONFIGS[config]
    plain, fused = _layers(pgl, **kw)
    rng = np.random.default_rng(43)
    x = rng.standard_normal((G.n, 24)).astype(np.float32)
    w = rng.standard_normal((G.n, 8 if kw.get("concat") is False else 32)).astype(np.float32)
    keys = []

    def keep_key_gradient(mod, args, out):                      # (returns None: the output stays as it is)
        out.retain_grad()
        keys.append(out)

    hook = plain.k.register_forward_hook(keep_key_gradient)
    res = []
    for layer in (plain, fused):
        xd = _t(x).requires_grad_(True)
        assert layer._takes_fused(G.g, xd, None) == (layer is fused)
        out = layer(G.g, xd)
        out.backward(_t(w))
        res.append((out, xd.grad, [p.grad for p in layer.parameters()]))
    hook.remove()
    (o0, gx0, gp0), (o1, gx1, gp1) = res
    assert len(keys) == 1 and keys[0].grad is not None
    own_terms = {"k.bias": host(keys[0].grad.double().abs().sum(0)).reshape(-1, 1)}
    flat = lambda t: host(t).reshape(t.shape[0], -1)
    checks = [("output", host(o1), host(o0), None), ("d x", host(gx1), host(gx0), None)] + \
             [("d " + name, flat(a), flat(b), own_terms.get(name)) for a, b, (name, _) in zip(gp1, gp0, fused.named_parameters())]
    print("fused vs three ops (%s), worst |difference| / bound: %s" % (config, ", ".join("%s %.3f" % (n, _rows_ratio(a, b, c)) for n, a, b, c in checks)))
    for name, a, b, cancel in checks:
        close_rows(a, b, RTOL, what="fused vs three ops (%s): %s" % (config, name), cancel=cancel)


def test_transformer_conv_with_edge_features_takes_todays_path(pgl, graphs):
    G = graphs["hub"]
    plain, fused = _layers(pgl)
    rng = np.random.default_rng(47)
    x, ef = _t(rng.standard_normal((G.n, 24))), _t(rng.standard_normal((G.e, 32)))
    assert not fused._takes_fused(G.g, x, ef)
    with torch.no_grad():
        assert_same_bits(fused(G.g, x, ef), plain(G.g, x, ef), "TransformerConv with edge features")


def test_transformer_conv_fused_in_training_mode_is_the_definition_with_the_seed_it_drew(pgl, graphs):
    """attn_drop = 0.5, .train(): the layer's output against linear -> definition(keep of layer.last_attn_seed) -> skip -> layer norm ->
    relu in fp64, close_rows at 5e-5 (the tolerance tests/test_gat_dropout_gpu.py holds GATConv's training output to; the GEMMs and
    the layer norm are not under test).  The seed is the one torch.manual_seed fixes; an eval forward draws nothing."""
    G = graphs["hub"]
    _, fused = _layers(pgl, attn_drop=0.5)
    x = _t(np.random.default_rng(53).standard_normal((G.n, 24)))
    fused.train()
    torch.manual_seed(1004)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(1004)
    out = fused(G.g, x)
    assert fused.last_attn_seed == seed

    def definition(keep):
        xd = x.double()
        lin = lambda m: xd @ m.weight.detach().double().t() + m.bias.detach().double()
        q, k, v = (lin(m).reshape(G.n, 4, 8) for m in (fused.q, fused.k, fused.v))
        o = A.dot_attention(q, k, v, G.src, G.dst, 8 ** -0.5, keep=keep).reshape(G.n, 32) + lin(fused.skip_feat)
        o = torch.nn.functional.layer_norm(o, (32,), fused.layer_norm.weight.detach().double(), fused.layer_norm.bias.detach().double(),
                                           fused.layer_norm.eps)
        return host(torch.relu(o))

    want = definition(_t(D.attention_keep(seed, np.arange(G.e), 4, 0.5)))
    close_rows(host(out), want, rtol=5e-5, what="TransformerConv(fused=True).train(): output")
    other = definition(_t(D.attention_keep(seed + 1, np.arange(G.e), 4, 0.5)))
    assert np.abs(other - want).max() > 1e-2 * np.abs(want).max()            # another seed is another mask: the comparison is not vacuous
    fused.eval()
    state = torch.get_rng_state()
    with torch.no_grad():
        got = fused(G.g, x)
    assert torch.equal(torch.get_rng_state(), state), "an eval forward drew from torch's generator"
    assert fused.last_attn_seed is None
    close_rows(host(got), definition(None), rtol=5e-5, what="TransformerConv(fused=True).eval(): output")
