"""The fused GATv2 attention (pgl_amd/csrc/gatv2_attention.hip) and GATv2Conv(fused=True) on the MI355X, held to the DEFINITION of
tests/gatv2_attention_defs.py: forward, row statistics and the three gradients per element against fp64 inside the re-association
bound of that element's own terms (grad_defs.grad_and_terms with the explicit terms + gpu_common.check_grad_elements; every element,
none left out), K from the fp32 definition on the host (gatv2_attention_defs.K_FAMILY; tests/test_gatv2_attention_defs.py re-measures
it).

Graphs: the 3 000-node hub and classes graphs of tests/test_gradients_gpu.py -- the classes graph has rows with 0 / 1 / 16 / 17 / 47
further pieces on BOTH streams, so the unsplit path and both fix-up passes run in the forward, the dst-sorted and the src-sorted walk."""
import ctypes

import numpy as np
import pytest
import torch

import gatv2_attention_defs as A
import grad_defs as D
from gpu_common import pgl, check_grad_elements, host  # noqa: F401  (pgl: the fixture)
from layout_defs import misaligned, assert_same_bits
from test_gradients_gpu import _graphs, _t  # noqa: F401

pytestmark = pytest.mark.gpu

K = A.K_FAMILY
NAMES3 = ("d x_src", "d x_dst", "d a")
NAMES2 = ("d x", "d a")


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
    xs, xd, a, cot, slope = A.case_inputs(G.n, H, Dh, seed)
    return _t(xs), _t(xd), _t(a), _t(cot), slope


def _run(engine, inputs, cot):
    xs = [t.detach().requires_grad_(True) for t in inputs]
    out = engine(*xs)
    out.backward(cot)
    return out.detach(), [x.grad for x in xs]


def _check(got, r, family, what):
    out, grads = got
    names = NAMES3 if len(grads) == 3 else NAMES2
    check_grad_elements(out, r.out64, r.out_abs, r.out_n, K=K[family], what=what + " forward")
    for i, name in enumerate(names):
        check_grad_elements(grads[i], r.want64[i], r.abs_terms64[i], r.n_terms[i], K=K[family], what="%s %s" % (what, name))


def _same(a, b, what):
    assert_same_bits(a[0], b[0], what + ": forward")
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert_same_bits(x, y, "%s: gradient %d" % (what, i))


def _two(G, slope, p=0.0, seed=0):
    return lambda x, y, w: G.g.gatv2_attention(x, w, slope, p, seed, x_dst=y)


def _one(G, slope, p=0.0, seed=0):
    return lambda x, w: G.g.gatv2_attention(x, w, slope, p, seed)


# ------------------------------------------------------------------------------------------------
# 1. forward, statistics and all three gradients against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["hub", "classes"])
@pytest.mark.parametrize("H,Dh", A.SHAPES)
def test_gatv2_attention_against_fp64(pgl, graphs, graph, H, Dh):
    from pgl_amd import attention_ops
    G = graphs[graph]
    assert attention_ops.gatv2_attention_supported(H, Dh)
    xs, xd, a, cot, slope = _inputs(G, H, Dh)
    r, res = _reference((graph, H, Dh, "two"), lambda: A.definition_and_terms(xs, xd, a, cot, G.src, G.dst, slope))
    what = "gatv2_attention %s %dx%d" % (graph, H, Dh)
    _check(_run(_two(G, slope), [xs, xd, a], cot), r, "gatv2_attention", what + " Graph.gatv2_attention")
    with torch.no_grad():                                    # without a gradient: the forward that writes no statistics
        plain = G.g.gatv2_attention(xs, a, slope, x_dst=xd)
    check_grad_elements(plain, r.out64, r.out_abs, r.out_n, K=K["gatv2_attention"], what=what + " forward without statistics")
    # the statistics the backward recomputes alpha from
    out, mx, sm = attention_ops.gatv2_attention(xs, xd, a, G.g._csr_dst(), slope, return_stats=True)
    _, _, m64, s64 = A.gatv2_attention(xs.double(), xd.double(), a.double(), G.src, G.dst, slope, parts=True)
    assert_same_bits(out, plain, what + ": the forward with statistics")
    check_grad_elements(mx, m64, *res["row_max"], K=K["gatv2_attention"], what=what + " row_max")
    check_grad_elements(sm, s64, *res["row_sum"], K=K["gatv2_attention"], what=what + " row_sum")
    empty = G.indeg == 0
    assert bool(empty.any()) and bool((mx[empty] == 0).all()) and bool((sm[empty] == 0).all()) and bool((out[empty] == 0).all())


@pytest.mark.parametrize("graph", ["hub", "classes"])
@pytest.mark.parametrize("H,Dh", A.SHAPES)
def test_one_tensor_on_both_sides_through_the_autograd_node(pgl, graphs, graph, H, Dh):
    """x_src is x_dst, as the layer has it: ONE gradient of x, the two walks' results added once by the node."""
    from pgl_amd import autograd as ag
    G = graphs[graph]
    x, _, a, cot, slope = _inputs(G, H, Dh)
    r, _ = _reference((graph, H, Dh, "one"), lambda: A.definition_and_terms(x, None, a, cot, G.src, G.dst, slope))
    what = "gatv2_attention %s %dx%d, one tensor" % (graph, H, Dh)
    got = _run(_one(G, slope), [x, a], cot)
    _check(got, r, "gatv2_attention", what)
    _same(_run(lambda t, w: ag.gatv2_attention(t, t, w, G.g._csr_dst(), G.g._csr_src, slope), [x, a], cot), got, what + ": x passed twice")
    _check(_run(_one(G, slope), [x, a.reshape(1, H, Dh)], cot), _reshaped(r, (1, H, Dh)), "gatv2_attention", what + ", a [1, H, D]")


def _reshaped(r, shape):
    """r (inputs x, a) with a's gradient and terms in `shape`: the layer's parameter is [1, H, D]."""
    q = D.GradTerms()
    for name in D.GradTerms.__slots__:
        setattr(q, name, getattr(r, name))
    q.want64, q.abs_terms64, q.n_terms = ([t[0], t[1].reshape(shape)] for t in (r.want64, r.abs_terms64, r.n_terms))
    return q


# ------------------------------------------------------------------------------------------------
# 2. degenerate graphs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E0", "E1", "N1"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_degenerate_graphs(graphs, name, p):
    G = graphs[name]
    H, Dh = 8, 16
    xs, xd, a, cot, slope = _inputs(G, H, Dh, seed=3)
    keep = None if p == 0 else _t(D.attention_keep(7, np.arange(G.e), H, p))
    family = "gatv2_attention_drop" if p else "gatv2_attention"
    r, _ = A.definition_and_terms(xs, xd, a, cot, G.src, G.dst, slope, keep)
    got = _run(_two(G, slope, p, 7), [xs, xd, a], cot)
    assert tuple(got[0].shape) == (G.n, H, Dh) and [tuple(g.shape) for g in got[1]] == [(G.n, H, Dh), (G.n, H, Dh), (H, Dh)]
    _check(got, r, family, "gatv2_attention %s p=%g" % (name, p))
    r1, _ = A.definition_and_terms(xs, None, a, cot, G.src, G.dst, slope, keep)
    _check(_run(_one(G, slope, p, 7), [xs, a], cot), r1, family, "gatv2_attention %s p=%g, one tensor" % (name, p))
    if name == "E0":
        assert all(bool((t == 0).all()) for t in [got[0]] + got[1])


# ------------------------------------------------------------------------------------------------
# 3. dropout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,H,Dh,p", A.DROP_CASES)
def test_gatv2_attention_with_dropout(graphs, graph, H, Dh, p):
    G = graphs[graph]
    seed = A.DROP_SEEDS[p]
    xs, xd, a, cot, slope = _inputs(G, H, Dh)
    keep = _t(D.attention_keep(seed, np.arange(G.e), H, p))
    r, _ = A.definition_and_terms(xs, xd, a, cot, G.src, G.dst, slope, keep)
    eng = lambda s: _run(_two(G, slope, p, s), [xs, xd, a], cot)
    got = eng(seed)
    _check(got, r, "gatv2_attention_drop", "gatv2_attention %s %dx%d p=%g" % (graph, H, Dh, p))
    _same(eng(seed), got, "the same seed twice")
    other = eng(seed + 1)
    assert not torch.equal(other[0], got[0]), "another seed gives the same output"


def test_no_dropout_is_the_plain_launch_whatever_the_seed(graphs):
    G = graphs["classes"]
    xs, xd, a, cot, slope = _inputs(G, 8, 16)
    plain = _run(_two(G, slope), [xs, xd, a], cot)
    for seed in (1, 2 ** 32 - 5):
        _same(_run(_two(G, slope, 0.0, seed), [xs, xd, a], cot), plain, "p = 0, seed %d" % seed)


def test_dropout_needs_edge_ids(pgl, graphs):
    """The csr-order view of the dst-keyed index carries no edge ids: dropout over it is refused (PGLAMD_E_ARG), not run with positions."""
    from pgl_amd import attention_ops
    G = graphs["hub"]
    xs, xd, a, _, slope = _inputs(G, 8, 16)
    vd, _ = G.g._csr_order_views()
    with pytest.raises(ValueError, match=r"dropout needs .* eid.*code -6"):
        attention_ops.gatv2_attention(xs, xd, a, vd, slope, 0.3, 1)


# ------------------------------------------------------------------------------------------------
# 4. exact scores on the kink
# ------------------------------------------------------------------------------------------------
def test_large_exact_scores_on_the_kink(graphs):
    """x integers in [-4, 4], a multiples of 1/8, D = 16, slope 1/4: every score is exact in fp32 in any summation order, |s| reaches
    beyond 100 and about one z in nine is exactly 0 -- a kernel that rescales wrongly, or exponentiates before subtracting the maximum,
    overflows; one that takes L'(0) for 1 misses d x.  Finite, and inside the same bound."""
    G = graphs["hub"]
    xs, xd, a, cot, slope = (_t(v) if isinstance(v, np.ndarray) else v for v in A.exact_inputs(G.n))
    z = xs[G.src].double() + xd[G.dst].double()
    s = (a.double() * A.leaky(z, slope)).sum(-1)
    assert float(s.abs().max()) >= 100.0 and bool((s.float().double() == s).all()) and float((z == 0).double().mean()) > 0.05
    r, _ = A.definition_and_terms(xs, xd, a, cot, G.src, G.dst, slope)
    got = _run(_two(G, slope), [xs, xd, a], cot)
    assert all(bool(torch.isfinite(t).all()) for t in [got[0]] + got[1])
    _check(got, r, "gatv2_attention", "gatv2_attention exact scores")


# ------------------------------------------------------------------------------------------------
# 5. bit reproducibility
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Dh", [(4, 8), (8, 16), (8, 32)])
def test_two_runs_give_identical_bits(graphs, H, Dh):
    G = graphs["classes"]
    xs, xd, a, cot, slope = _inputs(G, H, Dh)
    for p in (0.0, 0.3):
        eng = lambda: _run(_two(G, slope, p, 11), [xs, xd, a], cot)
        first = eng()
        assert len(first[1]) == 3                             # out, d x_src, d x_dst and d a: all four
        _same(eng(), first, "two runs, p = %g" % p)


# ------------------------------------------------------------------------------------------------
# 6. operand layout
# ------------------------------------------------------------------------------------------------
def _transposed(t):
    """The values of t as the non-contiguous view of a tensor with its first two axes swapped."""
    view = t.transpose(0, 1).contiguous().transpose(0, 1)
    assert torch.equal(view, t) and (min(t.shape[:2]) == 1 or not view.is_contiguous())
    return view


def _sliced(t):
    """The values of t [..., D] as every second row of a [2 n, ..., D + 3] tensor's first D columns."""
    big = torch.full((2 * t.shape[0],) + tuple(t.shape[1:-1]) + (t.shape[-1] + 3,), float("nan"), dtype=t.dtype, device=t.device)
    view = big[::2, ..., :t.shape[-1]]
    view.copy_(t)
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


@pytest.mark.parametrize("H,Dh", [(4, 8), (8, 16), (8, 32)])
@pytest.mark.parametrize("layout", ["transposed", "sliced", "offset-by-one-element"])
def test_operand_layout(graphs, layout, H, Dh):
    """Strided views and contiguous views one element into their storage are copied by the front end (operand layout
    contract), not refused and not read in lanes wider than their address allows: the results equal those on fresh copies bit for bit."""
    G = graphs["classes"]
    xs, xd, a, cot, slope = _inputs(G, H, Dh)
    make = {"transposed": _transposed, "sliced": _sliced, "offset-by-one-element": misaligned}[layout]
    want = _run(_two(G, slope, 0.3, 5), [t.clone() for t in (xs, xd, a)], cot.clone())
    got = _run(_two(G, slope, 0.3, 5), [make(xs), make(xd), make(a)], make(cot))
    _same(got, want, "%s operands %dx%d" % (layout, H, Dh))
    for i, name in enumerate(("x_src", "x_dst", "a")):       # one operand at a time
        ops = [xs, xd, a]
        ops[i] = make(ops[i])
        _same(_run(_two(G, slope, 0.3, 5), ops, cot), want, "%s %s alone" % (layout, name))


# ------------------------------------------------------------------------------------------------
# 7. NaN containment
# ------------------------------------------------------------------------------------------------
def test_a_nan_of_a_hub_source_stays_in_the_rows_that_read_it(graphs):
    """Forward, one tensor on both sides, the NaN in x[u, h, 0] of the hub source: out is NaN in head h of row u (its own in-edges read
    x[u] as the destination) and of the rows u sends to, nowhere else, and every other element has the bits of the clean run."""
    G = graphs["hub"]
    H, Dh, u, h = 8, 16, 60, 3
    x, _, a, _, slope = _inputs(G, H, Dh)
    assert int((G.src == u).sum()) > 1000
    with torch.no_grad():
        clean = G.g.gatv2_attention(x, a, slope)
        x2 = x.clone()
        x2[u, h, 0] = float("nan")
        bad = G.g.gatv2_attention(x2, a, slope)
    hit = torch.zeros(G.n, dtype=torch.bool, device=x.device)
    hit[G.dst[G.src == u]] = True
    hit[u] = bool(G.indeg[u] > 0)
    want_nan = torch.zeros((G.n, H, Dh), dtype=torch.bool, device=x.device)
    want_nan[hit, h, :] = True
    assert torch.equal(torch.isnan(bad), want_nan), "the NaN reached %d elements, expected %d" % (int(torch.isnan(bad).sum()), int(want_nan.sum()))
    assert torch.equal(bad[~want_nan].view(torch.int32), clean[~want_nan].view(torch.int32)), "an element outside the NaN's reach changed"


@pytest.mark.parametrize("graph,H,Dh,u", [("hub", 8, 16, 1000), ("classes", 4, 8, 1500), ("classes", 8, 32, 1501)])
def test_a_nan_in_x_stays_in_what_reads_it_forward_and_backward(graphs, graph, H, Dh, u):
    """One tensor on both sides, x[u, h, 0] = NaN, u an ordinary source.  out: NaN in head h of row u and of the rows u sends to only.
    d x: the softmax of a row that reads the NaN is NaN as a whole, so by the definition every SOURCE of such a row has a NaN
    gradient in head h as well (d x_src[u'] = sum keep alpha g + ...): the NaN elements of d x are exactly those of the fp64
    definition's gradient -- head h of u, of the rows u sends to and of the sources of those rows and of u -- and nothing else.  Every
    element outside is bit-equal to the clean run; d a is NaN at most in head h and has the clean bits in every other head.
    (classes, u = 1500 sends to row 4, the hub row of 3 000 edges in 47 chunks: the containment crosses both fix-up passes.)"""
    G = graphs[graph]
    h = 1
    x, _, a, cot, slope = _inputs(G, H, Dh)
    assert int((G.src == u).sum()) > 0
    clean = _run(_one(G, slope), [x, a], cot)
    x2 = x.clone()
    x2[u, h, 0] = float("nan")
    bad = _run(_one(G, slope), [x2, a], cot)
    fn = lambda t, w: A.gatv2_attention(t, t, w, G.src, G.dst, slope)
    out64, (dx64, da64) = D.evaluate(fn, [x2, a], cot)
    rows = torch.zeros(G.n, dtype=torch.bool, device=x.device)
    rows[G.dst[G.src == u]] = True
    rows[u] = True
    nan_out = torch.isnan(bad[0])
    assert torch.equal(nan_out, torch.isnan(out64)) and bool(nan_out.any())
    assert not bool(nan_out[~rows].any()) and not bool(nan_out[:, [i for i in range(H) if i != h]].any())
    reach = rows.clone()                                       # the sources of the rows whose softmax reads the NaN
    reach[G.src[rows[G.dst]]] = True
    nan_dx = torch.isnan(bad[1][0])
    assert torch.equal(nan_dx, torch.isnan(dx64)) and bool(nan_dx[u, h].all())
    assert not bool(nan_dx[~reach].any()) and not bool(nan_dx[:, [i for i in range(H) if i != h]].any())
    assert bool((~reach).any()), "the NaN's reach is the whole graph: the case shows nothing"
    for got, ref, nan, what in ((bad[0], clean[0], nan_out, "out"), (bad[1][0], clean[1][0], nan_dx, "d x")):
        assert torch.equal(got[~nan].view(torch.int32), ref[~nan].view(torch.int32)), "%s: an element outside the NaN's reach changed" % what
    other = [i for i in range(H) if i != h]
    assert not bool(torch.isnan(bad[1][1][other]).any())
    assert_same_bits(bad[1][1][other], clean[1][1][other], "d a in the heads that do not read the NaN")


# ------------------------------------------------------------------------------------------------
# 8. unsupported shapes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Dh", [(3, 12), (16, 32)])
def test_unsupported_shapes(pgl, graphs, H, Dh):
    from pgl_amd import attention_ops, _ffi, ops
    G = graphs["hub"]
    assert not attention_ops.gatv2_attention_supported(H, Dh)
    xs, xd, a, cot, slope = _inputs(G, H, Dh)
    csr, src_csr = G.g._csr_dst(), G.g._csr_src()
    with pytest.raises(ValueError, match=r"gatv2_attention.*code -1"):
        attention_ops.gatv2_attention(xs, xd, a, csr, slope)
    # the entry points themselves: PGLAMD_E_SHAPE, and not one byte of the outputs written
    lib, p = _ffi.lib(), ops._ptr
    mark = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=xs.device)
    out, mx, sm, dxs, dxd, da = mark(G.n, H, Dh), mark(G.n, H), mark(G.n, H), mark(G.n, H, Dh), mark(G.n, H, Dh), mark(H, Dh)
    ws = torch.zeros(int(lib.pglamd_gatv2_attention_backward_workspace_bytes(G.e, G.n, H, Dh)), dtype=torch.uint8, device=xs.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx = lambda c: (p(c.row32), p(c.col32), p(c.eid32), p(c.indptr))
    rc = lib.pglamd_gatv2_attention(p(xs), p(xd), p(a), H, Dh, slope, 0.0, 0, *idx(csr), G.e, G.n, p(out), p(mx), p(sm), p(ws), ws.numel(), stream)
    assert rc == -1, rc
    rc = lib.pglamd_gatv2_attention_backward(p(cot), p(xs), p(xd), p(a), p(out), p(mx), p(sm), H, Dh, slope, 0.0, 0, *idx(csr), *idx(src_csr),
                                             G.e, G.n, p(dxs), p(dxd), p(da), p(ws), ws.numel(), stream)
    assert rc == -1, rc
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (out, mx, sm, dxs, dxd, da)) and not bool(ws.any())
    # the layer falls back to the code of fused=False
    torch.manual_seed(2)
    plain = pgl.nn.GATv2Conv(24, Dh, num_heads=H, feat_drop=0.0, attn_drop=0.0).cuda()
    fused = pgl.nn.GATv2Conv(24, Dh, num_heads=H, feat_drop=0.0, attn_drop=0.0, fused=True).cuda()
    fused.load_state_dict(plain.state_dict())
    x = _t(np.random.default_rng(4).standard_normal((G.n, 24)))
    assert not fused._takes_fused(G.g, x)
    with torch.no_grad():
        assert_same_bits(fused(G.g, x), plain(G.g, x), "GATv2Conv %dx%d: fused=True on a shape the kernels do not take" % (H, Dh))


# ------------------------------------------------------------------------------------------------
# 9. the layer
# ------------------------------------------------------------------------------------------------
LAYER_H, LAYER_D, LAYER_IN = 4, 8, 24


def _layers(pgl, attn_drop=0.0, concat=True):
    torch.manual_seed(7)
    kw = dict(num_heads=LAYER_H, feat_drop=0.0, attn_drop=attn_drop, concat=concat)
    plain = pgl.nn.GATv2Conv(LAYER_IN, LAYER_D, **kw).cuda()
    fused = pgl.nn.GATv2Conv(LAYER_IN, LAYER_D, fused=True, **kw).cuda()
    fused.load_state_dict(plain.state_dict())
    return plain, fused


def _layer_run(layer, G, x, w):
    """-> dict of the layer's output, the projected feature [N, H, D] (the attention's operand) and every gradient."""
    kept = []
    hook = layer.linear.register_forward_hook(lambda mod, args, out: (out.retain_grad(), kept.append(out))[0])
    xd = x.detach().clone().requires_grad_(True)
    out = layer(G.g, xd)
    out.backward(w)
    hook.remove()
    assert len(kept) == 1
    shape = (G.n, LAYER_H, LAYER_D)
    return dict(out=out.detach(), feature=kept[0].detach().reshape(shape), d_feature=kept[0].grad.reshape(shape), d_x=xd.grad,
                d_attn=layer.attn.grad.reshape(LAYER_H, LAYER_D), d_weight=layer.linear.weight.grad, d_bias=layer.linear.bias.grad)


def _within(got, want, tol, what):
    err = (got.double() - want.double()).abs()
    ratio = float((err / tol).max())
    print("%s: worst |difference| / bound %.3f" % (what, ratio))
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("concat", [True, False], ids=["concat", "head-mean"])
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_gatv2_conv_fused_against_the_three_op_layer(pgl, graphs, concat, training):
    """fused=True against fused=False from one state_dict, attn_drop = 0, inside the bound of the definition.  Both layers project with
    the same GEMM (the features are bit-equal, asserted), so the attention's operand f is shared and B = the definition's bound (K x
    the terms of gatv2_attention_defs on f, attn and the cotangent the layer hands the attention) holds for each layer's attention
    output, d f and d attn against fp64: the fused layer is held to B against fp64 directly, the two layers to 2 B against each other
    (each lies within B of the same fp64 values).  What lies behind the projection inherits B through it, plus the GEMM's own rounding
    in each layer (n terms each, slack 4, as grad_defs.bound):
        d weight = d f^T x:   2 (B^T |x| + 4 N eps |d f|^T |x|)        d bias = sum_n d f:   2 (sum_n B + 4 N eps sum_n |d f|)
        d x = d f W:          2 (B |W| + 4 H D eps |d f| |W|)
    head-mean: the output is the mean over H = 4 heads (a power of two: the cotangent of the attention, w / 4, is exact); its bound is
    the mean of the heads' bounds plus the H + 1 roundings of the mean."""
    G = graphs["hub"]
    plain, fused = _layers(pgl, concat=concat)
    for layer in (plain, fused):
        layer.train(training)
    rng = np.random.default_rng(43)
    x = _t(rng.standard_normal((G.n, LAYER_IN)))
    w = _t(rng.standard_normal((G.n, LAYER_H * LAYER_D if concat else LAYER_D)))
    assert fused._takes_fused(G.g, x) and not plain._takes_fused(G.g, x)
    a, b = _layer_run(plain, G, x, w), _layer_run(fused, G, x, w)
    assert fused.last_attn_seed is None
    assert_same_bits(a["feature"], b["feature"], "the projected features of the two layers")
    f, attn = b["feature"], fused.attn.detach().reshape(LAYER_H, LAYER_D)
    shape = (G.n, LAYER_H, LAYER_D)
    cot = w.reshape(shape) if concat else (w / LAYER_H)[:, None, :].expand(shape).contiguous()
    r, _ = A.definition_and_terms(f, None, attn, cot, G.src, G.dst, 0.2)
    Kf = K["gatv2_attention"]
    B_out, B_f, B_a = D.bound(r.out_abs, r.out_n, K=Kf), D.bound(r.abs_terms64[0], r.n_terms[0], K=Kf), D.bound(r.abs_terms64[1], r.n_terms[1], K=Kf)
    if concat:
        want_out, B_o = r.out64.reshape(G.n, -1), B_out.reshape(G.n, -1)
    else:
        want_out = r.out64.mean(1)
        B_o = B_out.mean(1) + 4.0 * (LAYER_H + 1) * D.EPS32 * r.out64.abs().mean(1)
    what = "GATv2Conv %s %s" % ("concat" if concat else "head-mean", "train" if training else "eval")
    _within(b["out"], want_out, B_o, what + ": fused output against fp64")
    _within(b["d_feature"], r.want64[0], B_f, what + ": fused d feature against fp64")
    _within(b["d_attn"], r.want64[1], B_a, what + ": fused d attn against fp64")
    _within(b["out"], a["out"], 2 * B_o, what + ": output, fused against three ops")
    _within(b["d_feature"], a["d_feature"], 2 * B_f, what + ": d feature, fused against three ops")
    _within(b["d_attn"], a["d_attn"], 2 * B_a, what + ": d attn, fused against three ops")
    gf, Bf2 = r.want64[0].abs().reshape(G.n, -1), B_f.reshape(G.n, -1)
    xa, Wa = x.double().abs(), fused.linear.weight.detach().double().abs()                  # W [H D, in]
    n_eps, hd_eps = 4.0 * G.n * D.EPS32, 4.0 * LAYER_H * LAYER_D * D.EPS32
    _within(b["d_weight"], a["d_weight"], 2 * (Bf2.t() @ xa + n_eps * (gf.t() @ xa)) + D.TINY32, what + ": d linear.weight")
    _within(b["d_bias"], a["d_bias"], 2 * (Bf2.sum(0) + n_eps * gf.sum(0)) + D.TINY32, what + ": d linear.bias")
    _within(b["d_x"], a["d_x"], 2 * (Bf2 @ Wa + hd_eps * (gf @ Wa)) + D.TINY32, what + ": d input")


def test_gatv2_conv_fused_in_training_mode_is_the_definition_with_the_seed_it_drew(pgl, graphs):
    """attn_drop = 0.5, .train(): the layer's output against the definition on the layer's own projected feature with the keep of
    layer.last_attn_seed, per element inside the dropout family's bound (no other op follows the attention in this layer).  The seed is
    the one torch.manual_seed fixes; an eval forward draws nothing."""
    G = graphs["hub"]
    _, fused = _layers(pgl, attn_drop=0.5)
    x = _t(np.random.default_rng(53).standard_normal((G.n, LAYER_IN)))
    fused.train()
    torch.manual_seed(1004)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(1004)
    with torch.no_grad():
        out = fused(G.g, x)
        f = fused.linear(x).reshape(G.n, LAYER_H, LAYER_D)
    assert fused.last_attn_seed == seed
    attn = fused.attn.detach().reshape(LAYER_H, LAYER_D)
    cot = torch.zeros_like(f)

    def definition(keep, family):
        r, _ = A.definition_and_terms(f, None, attn, cot, G.src, G.dst, 0.2, keep)
        return r.out64.reshape(G.n, -1), D.bound(r.out_abs, r.out_n, K=K[family]).reshape(G.n, -1)

    want, B = definition(_t(D.attention_keep(seed, np.arange(G.e), LAYER_H, 0.5)), "gatv2_attention_drop")
    _within(out, want, B, "GATv2Conv(fused=True).train(): output")
    other, _ = definition(_t(D.attention_keep(seed + 1, np.arange(G.e), LAYER_H, 0.5)), "gatv2_attention_drop")
    assert float((other - want).abs().max()) > 1e-2 * float(want.abs().max())  # another seed is another mask: the comparison is not vacuous
    fused.eval()
    state = torch.get_rng_state()
    with torch.no_grad():
        got = fused(G.g, x)
    assert torch.equal(torch.get_rng_state(), state), "an eval forward drew from torch's generator"
    assert fused.last_attn_seed is None
    want, B = definition(None, "gatv2_attention")
    _within(got, want, B, "GATv2Conv(fused=True).eval(): output")


def test_gatv2_conv_fused_takes_todays_path_where_the_kernel_does_not_apply(pgl, graphs):
    """A BiGraph (sources and destinations are different node sets, here of one size so that the layer runs at all) and an fp16 input:
    fused=True runs the code of fused=False -- the same bits, or the same refusal.  (Unsupported shapes: test_unsupported_shapes.)"""
    G = graphs["hub"]
    plain, fused = _layers(pgl)
    x = _t(np.random.default_rng(59).standard_normal((G.n, LAYER_IN)))
    bg = pgl.BiGraph(edges=np.stack([G.src_np, G.dst_np], 1), src_num_nodes=G.n, dst_num_nodes=G.n).tensor()
    assert bg.dot_attention_rows() is None and not fused._takes_fused(bg, x)
    with torch.no_grad():
        assert_same_bits(fused(bg, x), plain(bg, x), "GATv2Conv over a BiGraph")
    half_plain, half_fused = plain.half(), fused.half()
    xh = x.half()
    assert not half_fused._takes_fused(G.g, xh)

    def outcome(layer):
        """The layer's output, or the error it ends in (fused=False has no fp16 send_uv today: the same refusal is the same code)."""
        try:
            with torch.no_grad():
                return layer(G.g, xh)
        except Exception as err:                              # noqa: BLE001  (compared below, type and text)
            return (type(err), str(err))

    want, got = outcome(half_plain), outcome(half_fused)
    if isinstance(want, tuple):
        assert got == want, (got, want)
    else:
        assert_same_bits(got, want, "GATv2Conv on fp16 input")
