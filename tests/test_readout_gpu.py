"""The fused attention read-out (pgl_amd/csrc/readout.hip, pgl_amd.readout_ops.attention_readout) and GlobalAttention(fused=True) /
Set2Set(fused=True) on the MI355X, held to the DEFINITION of tests/readout_defs.py: forward and both gradients per element against
fp64 inside the re-association bound of that element's own terms (gpu_common.check_grad_elements; every element, none left out), K
from the fp32 definition on the host (readout_defs.K_FAMILY; tests/test_readout_defs.py re-measures it).

Segments: readout_defs.LENGTHS = 0, 1, 2, 3, 63, 64, 65 and PIECE - 1, PIECE, PIECE + 1, 3 PIECE + 5 rows -- empty, shorter than a pass
of the wave, a pass more or less, and one, two and four pieces (the merge launch)."""
import os

import numpy as np
import pytest
import torch

import grad_defs as D
import readout_defs as R
from gpu_common import pgl, check_grad_elements  # noqa: F401  (pgl: the fixture)
from layout_defs import assert_same_bits, column_block, misaligned

pytestmark = pytest.mark.gpu

K = R.K_FAMILY
HERE = os.path.dirname(os.path.abspath(__file__))
_REFERENCE = {}
_PLANS = {}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _reference(key, make):
    """The fp64 definition and its terms, computed once per case and shared by the tests that need it; never modified."""
    if key not in _REFERENCE:
        _REFERENCE[key] = make()
    return _REFERENCE[key]


def _plan(lengths):
    from pgl_amd import readout_ops
    key = tuple(int(v) for v in lengths)
    if key not in _PLANS:
        _PLANS[key] = readout_ops.readout_plan(R.seg_ptr_of(lengths), "cuda")
    return _PLANS[key]


def _kw(mode, opnd):
    return {"score": opnd} if mode == "gate" else {"query": opnd}


def _definition(mode, lengths, x, opnd, cot):
    """On the host, from the values the engine sees."""
    x, opnd, cot = (t.detach().cpu() for t in (x, opnd, cot))
    return R.definition_and_terms(x, R.seg_ptr_of(lengths), cot, **_kw(mode, opnd))


def _run(mode, plan, x, opnd, cot, need=(True, True)):
    from pgl_amd import readout_ops
    xs = [x.detach().requires_grad_(bool(need[0])), opnd.detach().requires_grad_(bool(need[1]))]
    out = readout_ops.attention_readout(xs[0], plan, **_kw(mode, xs[1]))
    out.backward(cot)
    return out.detach(), [t.grad for t in xs]


def _check(got, r, family, what):
    out, grads = got
    check_grad_elements(out, r.out64, r.out_abs, r.out_n, K=K[family], what=what + " forward")
    for i, name in enumerate(("d x", "d operand")):
        check_grad_elements(grads[i], r.want64[i], r.abs_terms64[i], r.n_terms[i], K=K[family], what="%s %s" % (what, name))


def _same(a, b, what):
    assert_same_bits(a[0], b[0], what + ": forward")
    for i, (u, v) in enumerate(zip(a[1], b[1])):
        assert_same_bits(u, v, "%s: gradient %d" % (what, i))


def _case(mode, lengths, d, seed=0):
    return tuple(_t(a) for a in R.case_inputs(mode, lengths, d, seed))


# ------------------------------------------------------------------------------------------------
# 1. the definition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gate", "query"])
@pytest.mark.parametrize("d", R.WIDTHS)
def test_attention_readout_against_fp64(pgl, mode, d):
    from pgl_amd import readout_ops
    assert readout_ops.readout_supported(d)
    plan = _plan(R.LENGTHS)
    assert plan.S == len(R.LENGTHS) and plan.N == sum(R.LENGTHS) and plan.num_long == 2 and plan.num_parts == 6 and plan.max_len == 3 * R.PIECE + 5
    x, opnd, cot = _case(mode, R.LENGTHS, d)
    r = _reference((mode, d), lambda: _definition(mode, R.LENGTHS, x, opnd, cot))
    before = dict(readout_ops.LAUNCHES)
    got = _run(mode, plan, x, opnd, cot)
    assert readout_ops.LAUNCHES["attention_readout"] == before.get("attention_readout", 0) + 1
    assert readout_ops.LAUNCHES["attention_readout_backward"] == before.get("attention_readout_backward", 0) + 1
    _check(got, r, "readout_" + mode, "attention_readout %s d=%d" % (mode, d))
    with torch.no_grad():                                    # without a gradient: the same launch, no autograd node
        plain = readout_ops.attention_readout(x, plan, **_kw(mode, opnd))
    assert_same_bits(plain, got[0], "the forward without gradients")
    with pytest.raises(ValueError, match="the plan is for"):
        readout_ops.attention_readout(x[:-1], plan, **_kw(mode, opnd if mode == "query" else opnd[:-1]))


# ------------------------------------------------------------------------------------------------
# 2. empty segments
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gate", "query"])
@pytest.mark.parametrize("lengths", [[0, 5, 0, 0, 300, 0], [0]], ids=["first-and-last-empty", "S1-N0"])
def test_empty_segments_are_exactly_zero(pgl, mode, lengths):
    d = 64
    x, opnd, cot = _case(mode, lengths, d)
    assert tuple(x.shape) == (sum(lengths), d)
    out, (dx, do) = _run(mode, _plan(lengths), x, opnd, cot)
    empty = [g for g, n in enumerate(lengths) if n == 0]
    assert bool((out[empty] == 0).all()) and bool(torch.isfinite(out).all())
    assert tuple(dx.shape) == tuple(x.shape)
    if mode == "query":
        assert bool((do[empty] == 0).all()) and bool(torch.isfinite(do).all())
    if sum(lengths):
        _check((out, [dx, do]), _definition(mode, lengths, x, opnd, cot), "readout_" + mode, "empty segments %s" % mode)


# ------------------------------------------------------------------------------------------------
# 3. bit reproducibility, order independence, need-flags
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gate", "query"])
def test_bits_repeat_and_do_not_depend_on_the_order_of_the_segments(pgl, mode):
    d, lengths = 64, R.LENGTHS
    x, opnd, cot = _case(mode, lengths, d)
    plan = _plan(lengths)
    first = _run(mode, plan, x, opnd, cot)
    _same(_run(mode, plan, x, opnd, cot), first, "a second run")
    # need-flags: a gradient that is skipped leaves the other's bits as they are
    only_x = _run(mode, plan, x, opnd, cot, need=(True, False))
    only_o = _run(mode, plan, x, opnd, cot, need=(False, True))
    assert only_x[1][1] is None and only_o[1][0] is None
    assert_same_bits(only_x[1][0], first[1][0], "d x alone")
    assert_same_bits(only_o[1][1], first[1][1], "d operand alone")
    assert_same_bits(only_x[0], first[0], "forward, d x alone")
    assert_same_bits(only_o[0], first[0], "forward, d operand alone")
    # the segments in another order
    perm = np.random.default_rng(9).permutation(len(lengths))
    assert not np.array_equal(perm, np.arange(len(lengths)))
    ptr = R.seg_ptr_of(lengths)
    rows = torch.as_tensor(np.concatenate([np.arange(ptr[g], ptr[g + 1]) for g in perm])).cuda()
    seg = torch.as_tensor(perm).cuda()
    by_row = lambda t: t[rows].contiguous()
    by_seg = lambda t: t[seg].contiguous()
    p_lengths = [lengths[g] for g in perm]
    p_opnd = by_row(opnd) if mode == "gate" else by_seg(opnd)
    got = _run(mode, _plan(p_lengths), by_row(x), p_opnd, by_seg(cot))
    assert_same_bits(got[0], by_seg(first[0]), "segments permuted: forward")
    assert_same_bits(got[1][0], by_row(first[1][0]), "segments permuted: d x")
    assert_same_bits(got[1][1], by_row(first[1][1]) if mode == "gate" else by_seg(first[1][1]), "segments permuted: d operand")


# ------------------------------------------------------------------------------------------------
# 4. more pieces than a launch has workgroups
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gate", "query"])
def test_more_pieces_than_one_launch_has_waves(pgl, mode):
    lengths = R.many_lengths()
    plan = _plan(lengths)
    assert plan.num_pieces == R.MANY_SEGMENTS > 2048 * 4 and plan.num_long == 0       # (the grid is capped at 2048 workgroups of 4 waves)
    x, opnd, cot = _case(mode, lengths, R.MANY_D)
    got = _run(mode, plan, x, opnd, cot)
    _check(got, _definition(mode, lengths, x, opnd, cot), "readout_" + mode, "%d segments %s" % (R.MANY_SEGMENTS, mode))
    empty = torch.as_tensor(np.flatnonzero(lengths == 0)).cuda()
    assert int(empty.numel()) > 1000 and bool((got[0][empty] == 0).all())


# ------------------------------------------------------------------------------------------------
# 5. non-finite rules
# ------------------------------------------------------------------------------------------------
def _within(got, want64, bound, mask, what):
    got, want64, bound = got.detach().cpu().double(), want64.cpu(), bound.cpu()
    m = mask.expand_as(got) if mask.dim() == got.dim() else mask[:, None].expand_as(got) if got.dim() == 2 else mask
    assert bool(torch.isfinite(got[m]).all()), what + ": not finite"
    ratio = float(((got - want64).abs()[m] / bound[m]).max())
    print("%s: worst |difference| / bound %.3f" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


def test_non_finite_scores_and_rows(pgl):
    """Gate mode, d = 64, five segments: -inf at the first row; a 3-piece segment whose whole first piece is -inf; all -inf; a +inf;
    a NaN row of x.  The non-finite elements of out are those of the fp64 definition (segments 2, 3, 4, whole rows), everything else
    is inside the bound, and so are the gradients of segments 0 and 1, where a -inf row has d score = 0 exactly."""
    d, P = 64, R.PIECE
    lengths = [10, 2 * P + 5, 7, 9, 6]
    ptr = R.seg_ptr_of(lengths)
    x, score, cot = R.case_inputs("gate", lengths, d, seed=3)
    inf = np.float32(np.inf)
    score[ptr[0]] = -inf
    score[ptr[1]:ptr[1] + P] = -inf
    score[ptr[2]:ptr[3]] = -inf
    score[ptr[3] + 4] = inf
    x[ptr[4] + 2] = np.nan
    x, score, cot = _t(x), _t(score), _t(cot)
    r = _definition("gate", lengths, x, score, cot)
    out, (dx, ds) = _run("gate", _plan(lengths), x, score, cot)
    bad64 = ~torch.isfinite(r.out64)
    assert bad64[2:].all() and not bad64[:2].any()           # (what the definition gives: the premise of the comparison)
    assert torch.equal(~torch.isfinite(out).cpu(), bad64), "the non-finite elements of out"
    Kg = K["readout_gate"]
    seg_ok = torch.as_tensor([True, True, False, False, False])
    row_ok = seg_ok[R.segment_ids(ptr)]
    _within(out, r.out64, D.bound(r.out_abs, r.out_n, K=Kg), seg_ok, "non-finite: out of the finite segments")
    _within(dx, r.want64[0], D.bound(r.abs_terms64[0], r.n_terms[0], K=Kg), row_ok, "non-finite: d x of the finite segments")
    _within(ds, r.want64[1], D.bound(r.abs_terms64[1], r.n_terms[1], K=Kg), row_ok, "non-finite: d score of the finite segments")
    minus = torch.isinf(score.cpu()) & row_ok
    assert int(minus.sum()) == P + 1 and bool((ds.cpu()[minus] == 0).all()) and bool((dx.cpu()[minus] == 0).all())


# ------------------------------------------------------------------------------------------------
# 6. large scores
# ------------------------------------------------------------------------------------------------
def test_a_shift_of_the_scores_cancels_exactly(pgl):
    """Scores that are multiples of 1 / 4: score + 1e4 and score - 1e4 are exact in fp32, s - max has the same bits, so the shifted calls
    return the bits of the unshifted one -- which is inside the definition's bound.  Nothing overflows."""
    d, lengths = 64, R.LENGTHS
    x, _, cot = _case("gate", lengths, d)
    score = _t(R.exact_scores(sum(lengths)))
    plan = _plan(lengths)
    base = _run("gate", plan, x, score, cot)
    _check(base, _definition("gate", lengths, x, score, cot), "readout_gate", "exact scores")
    for shift in (1e4, -1e4):
        moved = score + shift
        assert torch.equal(moved - shift, score) and float(moved.abs().min()) > 9.9e3
        _same(_run("gate", plan, x, moved, cot), base, "scores shifted by %g" % shift)


# ------------------------------------------------------------------------------------------------
# 7. operand layout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gate", "query"])
@pytest.mark.parametrize("d", [64, 100])
def test_operand_layout_does_not_change_the_bits(pgl, mode, d):
    lengths = R.LENGTHS
    x, opnd, cot = _case(mode, lengths, d)
    plan = _plan(lengths)
    base = _run(mode, plan, x, opnd, cot)
    assert x.data_ptr() % 16 == 0 and x.is_contiguous()
    strided = column_block(x, 3, 2 * d + 7)
    assert not strided.view.is_contiguous()
    _same(_run(mode, plan, strided.view, opnd, cot), base, "x a row-strided view")
    assert strided.guard.intact()
    _same(_run(mode, plan, misaligned(x), opnd, cot), base, "x one element into its storage")
    _same(_run(mode, plan, x, misaligned(opnd), cot), base, "the operand one element into its storage")
    _same(_run(mode, plan, x, opnd, misaligned(cot)), base, "the cotangent one element into its storage")
    _same(_run(mode, plan, misaligned(x), misaligned(opnd), misaligned(cot)), base, "all three one element into their storage")


# ------------------------------------------------------------------------------------------------
# 8. graph capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gate", "query"])
def test_forward_and_backward_replayed_from_a_captured_graph(pgl, mode):
    """Forward plus backward at d = 128 over LENGTHS captured in torch.cuda.graph on ONE side stream (no parallel branches) after a
    warm-up call there, then replayed on other operand values: the bits of the eager run on those values."""
    from pgl_amd import readout_ops
    d, lengths = 128, R.LENGTHS
    plan = _plan(lengths)
    x, opnd, cot = _case(mode, lengths, d)
    eager = _run(mode, plan, x, opnd, cot)
    first = _case(mode, lengths, d, seed=1)                      # what the capture sees
    xs = [t.clone().requires_grad_(True) for t in first[:2]]
    g = first[2].clone()

    def step():
        out = readout_ops.attention_readout(xs[0], plan, **_kw(mode, xs[1]))
        return (out,) + torch.autograd.grad(out, xs, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # warm-up: workspaces
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = step()
    with torch.no_grad():
        for t, new in zip(xs + [g], (x, opnd, cot)):
            t.copy_(new)
        for t in res:
            t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _same((res[0], list(res[1:])), eager, "replayed from a captured graph")


# ------------------------------------------------------------------------------------------------
# 9. a width the kernels do not take
# ------------------------------------------------------------------------------------------------
def _batch_graph(pgl, lengths, index=None, device="cuda"):
    """A batched tensor graph of len(lengths) member graphs without edges (the read-outs use the node ranges only)."""
    ptr = R.seg_ptr_of(lengths)
    edges = torch.zeros((0, 2), dtype=torch.int64, device=device)
    return pgl.Graph(num_nodes=int(ptr[-1]), edges=edges, _graph_node_index=ptr if index is None else index, _num_graph=len(lengths),
                     _graph_edge_index=np.zeros(len(lengths) + 1, np.int64))


def test_unsupported_width(pgl):
    from pgl_amd import readout_ops, _ffi
    lengths = [3, 70, 1]
    d = 513
    assert not readout_ops.readout_supported(d)
    rng = np.random.default_rng(4)
    x = _t(rng.standard_normal((sum(lengths), d)).astype(np.float32))
    plan = _plan(lengths)
    with pytest.raises(ValueError, match="d = 513"):
        readout_ops.attention_readout(x, plan, score=x[:, 0].contiguous())
    with pytest.raises(ValueError, match="d = 513"):
        readout_ops.attention_readout(x, plan, query=x[:3].contiguous())
    # the entry point itself: PGLAMD_E_ARG, nothing written
    out = torch.full((3, d), 7.0, device="cuda")
    stats = torch.full((3, 2), 7.0, device="cuda")
    p = lambda t: t.data_ptr()
    rc = _ffi.lib().pglamd_attention_readout(p(x), plan.N, d, 0, p(x), p(plan.seg_ptr), plan.S, p(plan.pieces), plan.num_pieces, p(plan.long_segs),
                                             0, 0, p(out), p(stats), None, 0, None)
    torch.cuda.synchronize()
    assert rc == -6 and bool((out == 7.0).all()) and bool((stats == 7.0).all())
    g = _batch_graph(pgl, lengths)
    torch.manual_seed(3)
    before = dict(readout_ops.LAUNCHES)
    ga = pgl.nn.GlobalAttention(torch.nn.Linear(d, 1)).cuda()
    ga_f = pgl.nn.GlobalAttention(ga.gate, fused=True)
    s2s = pgl.nn.Set2Set(d, 2).cuda()
    s2s_f = pgl.nn.Set2Set(d, 2, fused=True).cuda()
    s2s_f.load_state_dict(s2s.state_dict())
    with torch.no_grad():
        for fused, plain in ((ga_f, ga), (s2s_f, s2s)):
            assert not fused._takes_fused(g, x)
            assert_same_bits(fused(g, x), plain(g, x), "%s(%d): fused=True on a width the kernels do not take" % (type(plain).__name__, d))
    assert dict(readout_ops.LAUNCHES) == before


# ------------------------------------------------------------------------------------------------
# 10. the reference's fixtures
# ------------------------------------------------------------------------------------------------
def test_global_attention_fused_matches_reference_python(pgl):
    """tests/test_golden_layers.py::test_batched_graph_matches_reference_python's GlobalAttention, fused, at its tolerances."""
    from test_golden_layers import _load_params, RTOL
    z = np.load(os.path.join(HERE, "golden", "layers", "batched_graph.npz"))
    sizes = z["sizes"].tolist()
    bg = pgl.Graph.disjoint([pgl.Graph(edges=z["edges_%d" % k], num_nodes=m) for k, m in enumerate(sizes)])
    bg.tensor()
    feat = torch.as_tensor(z["feat"]).cuda()
    ga = pgl.nn.GlobalAttention(torch.nn.Linear(6, 1), torch.nn.Linear(6, 4), fused=True)
    _load_params(ga, {k[4:]: z[k] for k in z.files if k.startswith("ga::")})
    ga = ga.cuda()
    assert ga._takes_fused(bg, feat) and ga._takes_fused(bg, ga.nn(feat))
    from pgl_amd import readout_ops
    n0 = readout_ops.LAUNCHES["attention_readout"]
    with torch.no_grad():
        att = ga(bg, feat)
    assert readout_ops.LAUNCHES["attention_readout"] == n0 + 1
    np.testing.assert_allclose(att.cpu().numpy(), z["global_attention"], rtol=5 * RTOL, atol=1e-6)


def test_set2set_fused_matches_reference_python(pgl):
    """tests/test_golden_layers.py::test_set2set_matches_reference_python, fused, at its tolerances: output and input gradient."""
    from test_golden_layers import _readout_case, _sub
    from pgl_amd import readout_ops
    z, bg, feat = _readout_case(pgl)
    s2s = pgl.nn.Set2Set(6, 3, 1, fused=True)
    s2s.load_state_dict({k.replace("lstm.lstm.", "lstm."): torch.as_tensor(v) for k, v in _sub(z, "s2s").items()})
    x = feat.clone().requires_grad_(True)
    s2s = s2s.cuda()
    assert s2s._takes_fused(bg, x)
    n0 = readout_ops.LAUNCHES["attention_readout"]
    out = s2s(bg, x)
    assert readout_ops.LAUNCHES["attention_readout"] == n0 + 1
    np.testing.assert_allclose(out.detach().cpu().numpy(), z["set2set"], rtol=1e-4, atol=1e-5)
    (out * torch.as_tensor(z["set2set_ct"]).cuda()).sum().backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), z["set2set_dx"], rtol=1e-3, atol=1e-5)


# ------------------------------------------------------------------------------------------------
# 11. fused against unfused
# ------------------------------------------------------------------------------------------------
def _close(got, want, tol, what):
    err = (got.detach().double().cpu() - want.detach().double().cpu()).abs()
    ratio = float((err / tol.cpu()).max())
    print("%s: worst |difference| / bound %.3f" % (what, ratio))
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (what, ratio)


def _layer_run(layer, g, x, w):
    xd = x.detach().clone().requires_grad_(True)
    for prm in layer.parameters():
        prm.grad = None
    out = layer(g, xd)
    out.backward(w)
    return out.detach(), xd.grad, {k: p.grad.clone() for k, p in layer.named_parameters()}


def test_global_attention_fused_against_the_unfused_layer(pgl):
    """fused=True against fused=False from one state_dict over LENGTHS at d = 64 (gate: Linear(64, 1), nn: Linear(64, 64)).  Both layers
    form the op's operands h = nn(x) and s = gate(x) with the same products (bit-equal operands), so B = the definition's bound (K x the
    terms of readout_defs on h, s and the cotangent) holds for each layer's output, d h and d s against fp64: the fused layer is held to
    B against fp64 directly, the two layers to 2 B against each other.  What lies behind the operands inherits B through them, plus the
    products' own rounding in each layer (n terms each, slack 4, as grad_defs.bound), with W_n, w_g the weights of nn and gate:
        d nn.weight = d h^T x:        2 (B_h^T |x| + 4 N eps |d h|^T |x|)          d nn.bias = sum_n d h: likewise without x
        d gate.weight = d s^T x:      2 (B_s^T |x| + 4 N eps |d s|^T |x|)          d gate.bias likewise
        d input = d h W_n + d s w_g:  2 (B_h |W_n| + B_s |w_g| + 4 (d + 2) eps (|d h| |W_n| + |d s| |w_g|))"""
    from pgl_amd import readout_ops
    d, lengths = 64, R.LENGTHS
    N = sum(lengths)
    g = _batch_graph(pgl, lengths)
    torch.manual_seed(7)
    plain = pgl.nn.GlobalAttention(torch.nn.Linear(d, 1), torch.nn.Linear(d, d)).cuda()
    fused = pgl.nn.GlobalAttention(torch.nn.Linear(d, 1), torch.nn.Linear(d, d), fused=True).cuda()
    fused.load_state_dict(plain.state_dict())
    rng = np.random.default_rng(43)
    x, w = _t(rng.standard_normal((N, d)).astype(np.float32)), _t(rng.standard_normal((len(lengths), d)).astype(np.float32))
    assert fused._takes_fused(g, x) and not plain._takes_fused(g, x)
    n0 = dict(readout_ops.LAUNCHES)
    a = _layer_run(plain, g, x, w)
    assert dict(readout_ops.LAUNCHES) == n0
    b = _layer_run(fused, g, x, w)
    assert readout_ops.LAUNCHES["attention_readout"] == n0.get("attention_readout", 0) + 1
    assert readout_ops.LAUNCHES["attention_readout_backward"] == n0.get("attention_readout_backward", 0) + 1
    with torch.no_grad():
        h, s = fused.nn(x), fused.gate(x).reshape(-1)
    r = _definition("gate", lengths, h, s, w)
    Kg = K["readout_gate"]
    B_out = D.bound(r.out_abs, r.out_n, K=Kg)
    B_h, B_s = D.bound(r.abs_terms64[0], r.n_terms[0], K=Kg), D.bound(r.abs_terms64[1], r.n_terms[1], K=Kg)[:, None]
    dh64, ds64 = r.want64[0], r.want64[1][:, None]
    xa = x.double().abs().cpu()
    Wn, wg = fused.nn.weight.detach().double().cpu(), fused.gate.weight.detach().double().cpu()         # [d, d], [1, d]
    _close(b[0], r.out64, B_out, "GlobalAttention: fused output against fp64")
    _close(b[0], a[0], 2 * B_out, "GlobalAttention: output, fused against unfused")
    n_eps = 4.0 * N * D.EPS32
    tol = lambda B, g64, rhs: 2 * (B.t() @ rhs + n_eps * (g64.abs().t() @ rhs)) + D.TINY32
    ones = torch.ones((N, 1), dtype=torch.float64)
    _close(b[2]["nn.weight"], a[2]["nn.weight"], tol(B_h, dh64, xa), "GlobalAttention: d nn.weight")
    _close(b[2]["nn.bias"], a[2]["nn.bias"], tol(B_h, dh64, ones).reshape(-1), "GlobalAttention: d nn.bias")
    _close(b[2]["gate.weight"], a[2]["gate.weight"], tol(B_s, ds64, xa), "GlobalAttention: d gate.weight")
    _close(b[2]["gate.bias"], a[2]["gate.bias"], tol(B_s, ds64, ones).reshape(-1), "GlobalAttention: d gate.bias")
    tol_x = B_h @ Wn.abs() + B_s @ wg.abs() + 4.0 * (d + 2) * D.EPS32 * (dh64.abs() @ Wn.abs() + ds64.abs() @ wg.abs())
    _close(b[1], a[1], 2 * tol_x + D.TINY32, "GlobalAttention: d input")
    _close(b[1], dh64 @ Wn + ds64 @ wg, tol_x + D.TINY32, "GlobalAttention: fused d input against fp64")


def _query_jacobian(layer):
    """|d q[k] / d theta| of the layer's LSTM rounds in fp64 on the host, one [d, *theta.shape] tensor per LSTM parameter.  The LSTM's
    input and initial state are zero for every graph, so every graph's q is the same function of the parameters: one row stands
    for all."""
    d = layer.input_dim
    lstm = torch.nn.LSTM(2 * d, d, layer.n_layers).double()
    lstm.load_state_dict({k: v.detach().double().cpu() for k, v in layer.lstm.state_dict().items()})
    state = (torch.zeros((layer.n_layers, 1, d), dtype=torch.float64), torch.zeros((layer.n_layers, 1, d), dtype=torch.float64))
    q_in = torch.zeros((1, 1, 2 * d), dtype=torch.float64)
    for _ in range(layer.n_iters):
        q, state = lstm(q_in, state)
    q = q.reshape(d)
    names, params = zip(*lstm.named_parameters())
    rows = [torch.autograd.grad(q[k], params, retain_graph=True, allow_unused=True) for k in range(d)]
    return {"lstm." + n: torch.stack([torch.zeros_like(p) if r[i] is None else r[i].abs() for r in rows]) for i, (n, p) in enumerate(zip(names, params))}


def test_set2set_fused_against_the_unfused_layer(pgl):
    """fused=True against fused=False from one state_dict over LENGTHS without the empty segment (the unfused layer counts its graphs
    from graph_id.max()) at d = 64, n_iters = 3: exactly ONE read-out launch, for the last round's q.  Both layers run the same LSTM
    on the same zero input, so q -- the first half of the output -- has the same bits in both, and B = the definition's bound on (x, q,
    the read-out half of the cotangent) holds for each layer's read-out, d x and d q against fp64: fused against fp64 within B, fused
    against unfused within 2 B.
    Behind q: both layers hand torch's LSTM backward the sum D = d q + (the cotangent's q half), and differ in it by at most 2 B_q.
    The LSTM sees a zero input and a zero initial state for every graph, so q[s, k] is the same function q0[k] of the parameters for
    every graph s, and d theta = sum_k (d q0[k] / d theta) sum_s D[s, k].  With J = |d q0 / d theta| from fp64 autograd on the host:
        d theta:  sum_k J[k] (2 sum_s B_q[s, k]  +  2 * 4 n eps sum_s |D[s, k]|),   n = 3 (S + 2 d + 8)
    (the second term: the fp32 rounding of each layer's LSTM backward, S graphs and 3 rounds of length-d products; slack 4 as
    grad_defs.bound).  weight_ih has J = 0 (its input is zero): its gradient is exactly 0 in both layers."""
    from pgl_amd import readout_ops
    d, lengths = 64, [n for n in R.LENGTHS if n]
    S, N = len(lengths), sum(lengths)
    g = _batch_graph(pgl, lengths)
    torch.manual_seed(11)
    plain = pgl.nn.Set2Set(d, 3).cuda()
    fused = pgl.nn.Set2Set(d, 3, fused=True).cuda()
    fused.load_state_dict(plain.state_dict())
    rng = np.random.default_rng(47)
    x, w = _t(rng.standard_normal((N, d)).astype(np.float32)), _t(rng.standard_normal((S, 2 * d)).astype(np.float32))
    assert fused._takes_fused(g, x) and not plain._takes_fused(g, x)
    n0 = dict(readout_ops.LAUNCHES)
    a = _layer_run(plain, g, x, w)
    assert dict(readout_ops.LAUNCHES) == n0
    b = _layer_run(fused, g, x, w)
    assert readout_ops.LAUNCHES["attention_readout"] == n0.get("attention_readout", 0) + 1            # n_iters = 3, ONE read-out
    assert readout_ops.LAUNCHES["attention_readout_backward"] == n0.get("attention_readout_backward", 0) + 1
    assert tuple(b[0].shape) == (S, 2 * d)
    assert_same_bits(b[0][:, :d].contiguous(), a[0][:, :d].contiguous(), "Set2Set: the q half of the output")
    q = b[0][:, :d].contiguous()
    assert bool((q == q[0]).all())                           # every graph's q is the same row
    r = _definition("query", lengths, x, q, w[:, d:].contiguous())
    Kq = K["readout_query"]
    B_out, B_x, B_q = D.bound(r.out_abs, r.out_n, K=Kq), D.bound(r.abs_terms64[0], r.n_terms[0], K=Kq), D.bound(r.abs_terms64[1], r.n_terms[1], K=Kq)
    _close(b[0][:, d:], r.out64, B_out, "Set2Set: fused read-out against fp64")
    _close(b[0][:, d:], a[0][:, d:], 2 * B_out, "Set2Set: read-out, fused against unfused")
    _close(b[1], r.want64[0], B_x, "Set2Set: fused d x against fp64")
    _close(b[1], a[1], 2 * B_x, "Set2Set: d x, fused against unfused")
    total = r.want64[1] + w[:, :d].double().cpu()
    per_k = 2.0 * B_q.sum(0) + 2.0 * 4.0 * 3 * (S + 2 * d + 8) * D.EPS32 * total.abs().sum(0)          # [d]
    J = _query_jacobian(fused)
    assert set(J) == set(b[2])
    for name, jac in J.items():
        tol = torch.tensordot(per_k, jac, dims=1) + D.TINY32
        _close(b[2][name], a[2][name], tol, "Set2Set: d %s" % name)
    assert bool((b[2]["lstm.weight_ih_l0"] == 0).all()) and bool((a[2]["lstm.weight_ih_l0"] == 0).all())


# ------------------------------------------------------------------------------------------------
# 12. routing
# ------------------------------------------------------------------------------------------------
def test_routing_leaves_other_graphs_to_the_unfused_code(pgl):
    """A graph whose _graph_node_index is a DEVICE tensor (reading it would be a host read) and a CPU graph: fused=True returns the
    bits of fused=False and no read-out launch is made."""
    from pgl_amd import readout_ops
    lengths, d = [5, 70, 1, 300], 64
    ptr = R.seg_ptr_of(lengths)

    class DeviceIndexGraph(pgl.Graph):                       # graph_node_id from a device index (the base class reads it with numpy)
        @property
        def graph_node_id(self):
            return R.segment_ids(self._graph_node_index.cpu()).to(torch.int32).cuda()

    edges = torch.zeros((0, 2), dtype=torch.int64, device="cuda")
    g_dev = DeviceIndexGraph(num_nodes=int(ptr[-1]), edges=edges, _graph_node_index=torch.as_tensor(ptr).cuda(), _num_graph=len(lengths),
                             _graph_edge_index=np.zeros(len(lengths) + 1, np.int64))
    assert g_dev.is_tensor() and g_dev._graph_node_index.is_cuda
    x = _t(np.random.default_rng(5).standard_normal((sum(lengths), d)).astype(np.float32))
    torch.manual_seed(5)
    ga = pgl.nn.GlobalAttention(torch.nn.Linear(d, 1), torch.nn.Linear(d, d)).cuda()
    ga_f = pgl.nn.GlobalAttention(ga.gate, ga.nn, fused=True)
    s2s = pgl.nn.Set2Set(d, 2).cuda()
    s2s_f = pgl.nn.Set2Set(d, 2, fused=True).cuda()
    s2s_f.load_state_dict(s2s.state_dict())
    before = dict(readout_ops.LAUNCHES)
    with torch.no_grad():
        for fused, plain in ((ga_f, ga), (s2s_f, s2s)):
            assert not fused._takes_fused(g_dev, x)
            assert_same_bits(fused(g_dev, x), plain(g_dev, x), "%s over a device index" % type(plain).__name__)
    # a CPU graph: "fused=True returns the bits of fused=False" has no bits to compare here -- the unfused layer's segment kernels have
    # no host path and raise; what can be held is that fused=True runs that same unfused code (the same error) and launches nothing
    g_cpu = pgl.Graph(num_nodes=int(ptr[-1]), edges=torch.zeros((0, 2), dtype=torch.int64), _graph_node_index=ptr, _num_graph=len(lengths),
                      _graph_edge_index=np.zeros(len(lengths) + 1, np.int64))
    x_cpu = x.cpu()
    for fused, plain in ((ga_f, ga), (s2s_f, s2s)):
        fused_cpu, plain_cpu = fused.cpu(), plain.cpu()
        assert not fused_cpu._takes_fused(g_cpu, x_cpu)
        for layer in (fused_cpu, plain_cpu):
            with torch.no_grad(), pytest.raises(RuntimeError, match="only on an MI355X"):
                layer(g_cpu, x_cpu)
    assert dict(readout_ops.LAUNCHES) == before
    # and the same device features over a host index take the kernel
    g_host = _batch_graph(pgl, lengths)
    ga_f, s2s_f = ga_f.cuda(), s2s_f.cuda()
    assert ga_f._takes_fused(g_host, x) and s2s_f._takes_fused(g_host, x)
    with torch.no_grad():
        ga_f(g_host, x), s2s_f(g_host, x)
    assert readout_ops.LAUNCHES["attention_readout"] == before.get("attention_readout", 0) + 2
    assert g_host._readout_plans[x.device][1] is not None     # the plan is kept on the graph, keyed by device
    plan = g_host._readout_plans[x.device][1]
    with torch.no_grad():
        ga_f(g_host, x)
    assert g_host._readout_plans[x.device][1] is plan
