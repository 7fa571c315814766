"""The fused GAT attention on 16-bit rows (pgl_amd/csrc/gat_fused_16.hip; attention_ops.gat_aggregate16 / gat_backward16,
Graph.gat_aggregate on an fp16 / bf16 feature, GATConv.fused_16bit) on the MI355X.

  a. forward, bit for bit: gat_aggregate16(x16) IS ops.gat_aggregate(x16.float()) rounded to the storage type -- the kernels keep the fp32
     geometry and fp32 sums and round once -- and the fp32 statistics are the fp32 call's bits;
  b. backward, bit for bit, over the three routes to d a_dst;
  c. the forward against the fp64 DEFINITION, independent of the fp32 kernel, inside the gat family's fp32 bound plus one rounding; the
     bound refuses an accumulator rounded to 16 bits after every edge;
  d. GATConv with fused_16bit against the same layer without it;
  e. operand layout, gat16_supported against the ABI, refusals that write nothing.

Graphs, data and helpers: tests/test_gradients_gpu.py (hub: rows without in-edges, multi-edges, self-loops, rows over a chunk boundary,
a source and a destination of ~3 000 edges; classes: every class of split row), tests/gat16_defs.py."""
import numpy as np
import pytest
import torch

import gat16_defs as G16
import grad_defs as D
import test_gradients_gpu as T
from gpu_common import pgl, host  # noqa: F401  (pgl: the fixture)
from layout_defs import misaligned, assert_same_bits
from test_gradients_gpu import _graphs, lattice, rows, _t, GAT_BACKWARD_ROUTES

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DT_ID = {torch.float16: "fp16", torch.bfloat16: "bf16"}
# one element per lane: (2, 8), (1, 64); two: (8, 16); four: (4, 64), (8, 32); a head dimension that is no power of two: (3, 6)
SHAPES = [(2, 8), (1, 64), (8, 16), (4, 64), (8, 32), (3, 6)]
GRAPHS = ["hub", "classes", "E0", "E1", "N1"]
BIG_SEED = 2 ** 31 + 12345


@pytest.fixture(scope="module")
def graphs(pgl):
    return _graphs(pgl)


def _inputs(G, H, D_, dt, seed=0):
    """rows() puts part of the data below fp16's normal range (2**-14 = 6.1e-5) on purpose."""
    rng = np.random.default_rng(211 + H + seed)
    f = _t(rows(rng, G.n, H, D_)).to(dt)
    a_s, a_d = _t(lattice(rng, True, G.n, H)), _t(lattice(rng, False, G.n, H))
    g = _t(rows(rng, G.n, H, D_)).to(dt)
    return f, a_s, a_d, g


def _same(got, want, what):
    if want is None or got is None:
        assert got is None and want is None, what
        return
    assert_same_bits(got, want, what)


def _either(fn32, fn16):
    """-> (result of fn32, result of fn16), or (None, None) when the fp32 call refuses its arguments and the 16-bit call refuses them
    with the same exception."""
    try:
        want = fn32()
    except (ValueError, TypeError, RuntimeError) as exc:
        with pytest.raises(type(exc)):
            fn16()
        return None, None
    return want, fn16()


def _check_forward(pgl, csr, f, a_s, a_d, dt, out_size, stats, p, seed, what):
    att = pgl.attention_ops
    want, got = _either(lambda: pgl.ops.gat_aggregate(f.float(), a_s, a_d, csr, 0.2, out_size, stats, p, seed),
                        lambda: att.gat_aggregate16(f, a_s, a_d, csr, 0.2, out_size, stats, p, seed))
    if want is None:
        return None
    if not stats:
        assert got.dtype == dt
        _same(got, want.to(dt), what + ": out")
        return got
    assert len(got) == len(want) == 5
    for name, a, b in zip(("out", "row_max", "row_sum", "out_pos", "sum_pos"), got, want):
        if name in ("out", "out_pos") and a is not None:
            assert a.dtype == dt, name
            b = b.to(dt)
        elif a is not None:
            assert a.dtype == torch.float32, name
        _same(a, b, "%s: %s" % (what, name))
    return got


# ------------------------------------------------------------------------------------------------
# a. forward, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,D_", SHAPES)
@pytest.mark.parametrize("graph", GRAPHS)
def test_forward_is_the_fp32_kernel_rounded_once(pgl, graphs, graph, H, D_):
    G = graphs[graph]
    csr = G.g._csr_dst()
    for dt in DTYPES:
        f, a_s, a_d, _ = _inputs(G, H, D_, dt)
        if graph == "hub" and dt == torch.float16:
            tiny = (f.float().abs() < 2.0 ** -14) & (f != 0)
            assert 0.01 < float(tiny.float().mean()) < 0.5, "no fp16 subnormals among the data"
        n_checked = 0
        for stats in (False, True):
            for p, seed in ((0.0, 0), (0.4, BIG_SEED)):
                got = _check_forward(pgl, csr, f, a_s, a_d, dt, None, stats, p, seed,
                                     "%s %dx%d %s stats=%s p=%g" % (graph, H, D_, DT_ID[dt], stats, p))
                n_checked += got is not None
        assert n_checked >= 2, "the fp32 call refused every form: nothing was compared"
        if G.e > 1000:
            out = pgl.attention_ops.gat_aggregate16(f, a_s, a_d, csr)
            assert bool((out != 0).any()) and bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_forward_over_many_hub_rows(pgl, dt):
    """200 destinations of ~1 250 edges each (about 20 chunks of 64: every one goes through the block-parallel pass of the fix-up) and 200
    such sources.  An fp32 sum that differs in its last bit shows in one of several thousand 16-bit elements only: the two hub rows of
    the hub graph cannot tell whether the merge loops of the fix-up fuse the same multiply-adds in every instantiation, 200 rows can
    (they did not, before the store pinned the fp32 values as one vector: gat_fused.hpp, store_row)."""
    rng = np.random.default_rng(5)
    n, e = 1000, 250000
    src, dst = rng.integers(0, n, e), rng.integers(0, 200, e)
    G = T._G(pgl, n, np.concatenate([src, dst]), np.concatenate([dst, src]))
    assert int(T.further_pieces(G.dst_np, n)[:200].min()) > 17
    csr = G.g._csr_dst()
    for H, D_ in ((2, 8), (8, 16), (8, 32)):
        f, a_s, a_d, _ = _inputs(G, H, D_, dt)
        for stats in (False, True):
            _check_forward(pgl, csr, f, a_s, a_d, dt, None, stats, 0.0, 0, "hub rows %dx%d %s stats=%s" % (H, D_, DT_ID[dt], stats))
        _check_backward(pgl, G, H, D_, dt, 0.0, "hub rows %dx%d %s" % (H, D_, DT_ID[dt]))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("p", [0.0, 0.4])
def test_forward_out_size_below_and_above_the_rows_of_the_index(pgl, graphs, dt, p):
    """out_size = 3 cuts the classes graph inside its class rows (`r >= out_rows` in store_final and both fix-up passes), n + 37 adds
    rows that no edge reaches (zero_fill_role's `r >= n_csr_rows`)."""
    G = graphs["classes"]
    csr = G.g._csr_dst()
    f, a_s, a_d, _ = _inputs(G, 8, 16, dt)
    full = pgl.attention_ops.gat_aggregate16(f, a_s, a_d, csr, 0.2, None, True, p, BIG_SEED)
    for M in (3, G.n + 37):
        got = _check_forward(pgl, csr, f, a_s, a_d, dt, M, True, p, BIG_SEED, "classes 8x16 %s out_size=%d" % (DT_ID[dt], M))
        _check_forward(pgl, csr, f, a_s, a_d, dt, M, False, p, BIG_SEED, "classes 8x16 %s out_size=%d" % (DT_ID[dt], M))
        for a, b in zip(got, full):
            assert a.shape[0] == M
            _same(a[:min(M, G.n)], b[:min(M, G.n)], "out_size=%d changed the rows of the index" % M)
            assert bool((a[G.n:] == 0).all())


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_forward_same_bits_on_a_second_run_and_on_a_side_stream(pgl, graphs, dt):
    G = graphs["hub"]
    csr = G.g._csr_dst()
    f, a_s, a_d, _ = _inputs(G, 8, 16, dt)
    run = lambda: pgl.attention_ops.gat_aggregate16(f, a_s, a_d, csr, 0.2, None, True, 0.4, BIG_SEED)
    first = run()
    second = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for a, b, c in zip(first, second, third):
        _same(b, a, "second run")
        _same(c, a, "side stream")


# ------------------------------------------------------------------------------------------------
# b. backward, bit for bit
# ------------------------------------------------------------------------------------------------
def _check_backward(pgl, G, H, D_, dt, p, what):
    att = pgl.attention_ops
    cd, cs = G.g._csr_dst(), G.g._csr_src()
    f, a_s, a_d, g = _inputs(G, H, D_, dt)
    seed = BIG_SEED if p > 0 else 0
    out, mx, sm, out_pos, s_pos = att.gat_aggregate16(f, a_s, a_d, cd, 0.2, None, True, p, seed)
    assert (out_pos is not None) == pgl.ops._GAT_POS_STATS
    got = att.gat_backward16(g, f, out, a_s, a_d, mx, sm, cd, cs, 0.2, p, seed, out_pos, s_pos)
    # (the 16-bit out, up-cast, goes in: what the 16-bit backward reads -- not an fp32 forward's out)
    want = pgl.ops.gat_backward(g.float(), f.float(), out.float(), a_s, a_d, mx, sm, cd, cs, 0.2, p, seed,
                                None if out_pos is None else out_pos.float(), s_pos)
    assert got[0].dtype == dt and got[1].dtype == got[2].dtype == torch.float32
    _same(got[0], want[0].to(dt), what + ": d feature")
    _same(got[1], want[1], what + ": d a_src")
    _same(got[2], want[2], what + ": d a_dst")
    assert bool((got[0] != 0).any()) and bool((got[1] != 0).any()) and bool((got[2] != 0).any())


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("graph", ["classes", "hub"])
@pytest.mark.parametrize("route", list(GAT_BACKWARD_ROUTES))
def test_backward_is_the_fp32_kernel_rounded_once_over_every_route(pgl, graphs, route, graph, p, dt):
    keep = (pgl.ops._GAT_POS_STATS, pgl.ops._GAT_BWD_EDGE_BUFFER)
    try:
        pgl.ops._GAT_POS_STATS, pgl.ops._GAT_BWD_EDGE_BUFFER = GAT_BACKWARD_ROUTES[route]
        _check_backward(pgl, graphs[graph], 8, 16, dt, p, "%s 8x16 %s p=%g %s" % (graph, DT_ID[dt], p, route))
    finally:
        pgl.ops._GAT_POS_STATS, pgl.ops._GAT_BWD_EDGE_BUFFER = keep


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("H,D_", [(2, 8), (4, 64)])
def test_backward_is_the_fp32_kernel_rounded_once_at_one_and_four_elements_per_lane(pgl, graphs, H, D_, p, dt):
    for graph in ("classes", "hub"):
        _check_backward(pgl, graphs[graph], H, D_, dt, p, "%s %dx%d %s p=%g" % (graph, H, D_, DT_ID[dt], p))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_autograd_node_takes_and_returns_the_storage_type(pgl, graphs, dt):
    """Graph.gat_aggregate on a 16-bit feature: the output and d feature in the storage type, d attn_* in fp32 -- the bits of the
    front end's own calls; a float32 cotangent is taken as well."""
    G = graphs["hub"]
    f, a_s, a_d, g = _inputs(G, 8, 16, dt)
    xs = [t.detach().requires_grad_(True) for t in (f, a_s, a_d)]
    out = G.g.gat_aggregate(*xs, 0.2)
    assert out.dtype == dt
    out.backward(g)
    assert xs[0].grad.dtype == dt and xs[1].grad.dtype == xs[2].grad.dtype == torch.float32
    att = pgl.attention_ops
    cd, cs = G.g._csr_dst(), G.g._csr_src()
    o, mx, sm, op, sp = att.gat_aggregate16(f, a_s, a_d, cd, 0.2, None, True)
    want = att.gat_backward16(g, f, o, a_s, a_d, mx, sm, cd, cs, 0.2, 0.0, 0, op, sp)
    _same(out.detach(), o, "forward")
    for got, w, name in zip((xs[0].grad, xs[1].grad, xs[2].grad), want, ("d feature", "d a_src", "d a_dst")):
        _same(got, w, name)
    with torch.no_grad():
        _same(G.g.gat_aggregate(f, a_s, a_d, 0.2), o, "the forward without a graph")


# ------------------------------------------------------------------------------------------------
# c. against the definition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("graph,H,D_", [("hub", 8, 16), ("classes", 8, 16), ("hub", 2, 8), ("hub", 4, 64)])
def test_forward_against_the_fp64_definition(pgl, graphs, graph, H, D_, dt):
    """|got - want| <= the gat family's fp32 bound + u16 |want| (+ 2**-25 for fp16), element by element; want: grad_defs.gat in fp64 on
    the up-cast inputs."""
    G = graphs[graph]
    f, a_s, a_d, _ = _inputs(G, H, D_, dt)
    got = pgl.attention_ops.gat_aggregate16(f, a_s, a_d, G.g._csr_dst())
    want, bound = G16.bound16(f, a_s, a_d, G.src, G.dst, dt)
    err = (got.double() - want).abs()
    print("gat16 %s %dx%d %s: the engine uses %.3f of the bound" % (graph, H, D_, DT_ID[dt], float((err / bound).max())))
    bad = ~(err <= bound)
    assert not bool(bad.any()), "%d of %d elements out of bound, worst %.3f of it" % (int(bad.sum()), bad.numel(), float((err / bound).max()))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_the_bound_refuses_an_accumulator_rounded_after_every_edge(graphs, dt):
    """The hub row (destination 70, ~3 000 edges) summed on the host with the running row rounded to 16 bits after every edge leaves the
    bound; the host restatement with ONE rounding stays inside it on every row.
    Data: |rows()|, features of one sign.  A 16-bit accumulator stops growing once a term alpha_e f (about 1 / 3 000 of the row) falls
    below half its spacing (2**-11 resp. 2**-8 of the row): the hub row comes out tens of per cent short, where the bound allows
    4 * 6 004 * 2**-23 + u16 = 0.3 % resp. 0.7 % of sum |t| = |want|.  With rows() as they are -- signed -- the terms cancel, sum |t|
    is ~55 |want| and the fp32 part of a 3 000-edge row's bound alone (0.3 % of sum |t|) is wider than the random walk of 3 000 fp16
    roundings of a small running sum: measured on the host, 0 of the hub row's 128 elements leave the bound in fp16 and 35 in bf16.
    So the signed data is asserted for bf16 and printed for fp16; the one-signed data is asserted for both."""
    G = graphs["hub"]
    hub = 70
    assert int(G.indeg[hub]) >= 2900
    f, a_s, a_d, _ = _inputs(G, 8, 16, dt)
    for name, fx in (("one-signed", f.abs()), ("signed", f)):
        want, bound = (t.cpu() for t in G16.bound16(fx, a_s, a_d, G.src, G.dst, dt))
        once = G16.gat16_host(fx, a_s, a_d, G.src, G.dst, dt)
        assert bool(((once - want).abs() <= bound).all()), "one rounding leaves the bound"
        mutant = G16.gat16_host(fx, a_s, a_d, G.src, G.dst, dt, round_each_edge=True)
        out = (mutant - want).abs() > bound
        print("rounded after every edge, %s, %s rows: %d of %d elements of the hub row out of bound"
              % (DT_ID[dt], name, int(out[hub].sum()), out[hub].numel()))
        if name == "one-signed":
            assert bool(out[hub].all())
        elif dt == torch.bfloat16:
            assert bool(out[hub].any())


# ------------------------------------------------------------------------------------------------
# d. the layer
# ------------------------------------------------------------------------------------------------
TOL = {torch.float16: 4e-3, torch.bfloat16: 3e-2}          # tests/test_a13_f1_layers.py test_layers_with_16bit_feature_storage
LAYERS = {"8x16-concat": (16, 8, True), "4x8-head-mean": (8, 4, False), "1x41-classifier-padded": (41, 1, False), "8x64-in-head-groups": (64, 8, True)}


def _layer_pair(pgl, dim, heads, concat, dt, attn_drop=0.0, din=32):
    torch.manual_seed(3)
    up = pgl.nn.GATConv(din, dim, feat_drop=0.0, attn_drop=attn_drop, num_heads=heads, concat=concat).cuda().to(dt)
    native = pgl.nn.GATConv(din, dim, feat_drop=0.0, attn_drop=attn_drop, num_heads=heads, concat=concat).cuda().to(dt)
    native.load_state_dict(up.state_dict())
    assert up.fused_16bit is False and native.fused_16bit is False, "the switch is off by default"
    native.fused_16bit = True
    return up, native


def _counted(pgl, monkeypatch):
    calls = []
    real = pgl.attention_ops.gat_aggregate16

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(pgl.attention_ops, "gat_aggregate16", counting)
    return calls


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("case", list(LAYERS))
def test_gatconv_on_16_bit_rows_against_its_up_cast_route(pgl, graphs, monkeypatch, case, dt):
    """Output and input gradient of the two routes of one 16-bit layer, relative to the largest value: the tolerances
    test_layers_with_16bit_feature_storage holds a 16-bit GATConv to (output: tol, gradient through the attention: 4 tol)."""
    dim, heads, concat = LAYERS[case]
    G = graphs["hub"]
    up, native = _layer_pair(pgl, dim, heads, concat, dt)
    rng = np.random.default_rng(17)
    x = _t(rng.standard_normal((G.n, 32))).to(dt)
    calls = _counted(pgl, monkeypatch)
    xu, xn = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yu = up(G.g, xu)
    assert not calls, "fused_16bit = False ran the 16-bit kernels"
    yn = native(G.g, xn)
    assert len(calls) == (2 if case == "8x64-in-head-groups" else 1), "fused_16bit = True did not take the 16-bit kernels"
    assert yn.dtype == dt and yn.shape == yu.shape
    cot = torch.linspace(0.5, 1.5, yu.shape[1], device="cuda")
    (yu.float() * cot).sum().backward()
    (yn.float() * cot).sum().backward()
    tol = TOL[dt]
    e_out = float((yn.float() - yu.float()).abs().max()) / float(yu.float().abs().max())
    e_dx = float((xn.grad.float() - xu.grad.float()).abs().max()) / float(xu.grad.float().abs().max())
    print("GATConv %s %s: output %.2e of the largest value (tol %.0e), d x %.2e (tol %.0e)" % (case, DT_ID[dt], e_out, tol, e_dx, 4 * tol))
    assert xn.grad.dtype == dt and float(xu.grad.float().abs().max()) > 0
    assert e_out <= tol and e_dx <= 4 * tol
    with torch.no_grad():                                  # eval forward: the same kernels without the statistics
        assert_same_bits(native(G.g, x), yn.detach(), "forward with and without a graph")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
def test_gatconv_on_16_bit_rows_in_training_mode(pgl, graphs, monkeypatch, dt):
    """attn_drop = 0.6 after torch.manual_seed: the same bits twice, another mask after another seed, and the up-cast route's result
    under the same seed (one protocol: one torch.randint per forward, group h0 runs with seed + h0)."""
    G = graphs["hub"]
    for case in ("8x16-concat", "8x64-in-head-groups"):
        dim, heads, concat = LAYERS[case]
        up, native = _layer_pair(pgl, dim, heads, concat, dt, attn_drop=0.6)
        up.train(); native.train()
        x = _t(np.random.default_rng(19).standard_normal((G.n, 32))).to(dt)

        def run(layer, s):
            torch.manual_seed(s)
            xg = x.clone().requires_grad_(True)
            y = layer(G.g, xg)
            y.float().sum().backward()
            return y.detach(), xg.grad

        calls = _counted(pgl, monkeypatch)
        y1, g1 = run(native, 41)
        assert calls
        y2, g2 = run(native, 41)
        assert_same_bits(y2, y1, case + ": output under one seed")
        assert_same_bits(g2, g1, case + ": d x under one seed")
        y3, _ = run(native, 42)
        assert float((y3.float() - y1.float()).abs().max()) > 1e-2 * float(y1.float().abs().max()), "another seed, the same mask"
        yu, gu = run(up, 41)
        tol = TOL[dt]
        assert float((y1.float() - yu.float()).abs().max()) <= tol * float(yu.float().abs().max())
        assert float((g1.float() - gu.float()).abs().max()) <= 4 * tol * float(gu.float().abs().max())
        monkeypatch.undo()


def test_gatconv_fp32_ignores_the_switch(pgl, graphs, monkeypatch):
    G = graphs["hub"]
    torch.manual_seed(3)
    layer = pgl.nn.GATConv(32, 16, feat_drop=0.0, attn_drop=0.0, num_heads=8).cuda()
    x = _t(np.random.default_rng(23).standard_normal((G.n, 32)))
    calls = _counted(pgl, monkeypatch)
    off = layer(G.g, x)
    layer.fused_16bit = True
    on = layer(G.g, x)
    assert not calls and on.dtype == torch.float32
    assert_same_bits(on, off, "an fp32 layer with the switch on")


# ------------------------------------------------------------------------------------------------
# e. layout, the supported shapes, refusals
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("H,D_", [(2, 8), (8, 16), (8, 32)])
def test_misaligned_and_strided_operands_give_the_aligned_bits(pgl, graphs, H, D_, dt):
    """A contiguous view one element (2 bytes) into its storage and a non-contiguous feature go through ops._aligned."""
    G = graphs["classes"]
    att = pgl.attention_ops
    cd, cs = G.g._csr_dst(), G.g._csr_src()
    f, a_s, a_d, g = _inputs(G, H, D_, dt)
    want = att.gat_aggregate16(f, a_s, a_d, cd, 0.2, None, True)
    want_b = att.gat_backward16(g, f, want[0], a_s, a_d, want[1], want[2], cd, cs, 0.2, 0.0, 0, want[3], want[4])
    wide = torch.zeros((G.n, H, 2 * D_), dtype=dt, device=f.device)
    wide[:, :, ::2] = f
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    for name, fv in (("one element in", misaligned(f)), ("strided", strided)):
        assert fv.data_ptr() % 4 != 0 or not fv.is_contiguous()
        got = att.gat_aggregate16(fv, misaligned(a_s), a_d, cd, 0.2, None, True)
        for a, b in zip(got, want):
            _same(a, b, "forward, feature " + name)
        got_b = att.gat_backward16(misaligned(g), fv, misaligned(want[0]), a_s, a_d, want[1], want[2], cd, cs, 0.2, 0.0, 0,
                                   None if want[3] is None else misaligned(want[3]), want[4])
        for a, b in zip(got_b, want_b):
            _same(a, b, "backward, feature " + name)


CANARY = 0x7B7B


def _abi(pgl, G, H, D_, dt, code=None, ws_short=0, backward=False):
    """One raw call of pglamd_gat_aggregate_16 / pglamd_gat_backward_16 on graph G with canary-filled outputs -> (return code, outputs untouched)."""
    L, P = pgl._ffi.lib(), pgl.ops._ptr
    cd, cs = G.g._csr_dst(), G.g._csr_src()
    n, E = G.n, G.e
    dev_ = cd.row32.device
    code = pgl.ops._code(dt) if code is None else code
    f = torch.zeros((n, H, D_), dtype=dt, device=dev_)
    a = torch.zeros((n, H), dtype=torch.float32, device=dev_)
    ones = torch.ones((n, H), dtype=torch.float32, device=dev_)
    outs = [torch.full((n, H, D_), CANARY, dtype=torch.int16, device=dev_)]
    if not backward:
        need = L.pglamd_gat_aggregate_workspace_bytes(E, H, D_)
        ws = pgl.ops._ws(need, dev_)
        rc = L.pglamd_gat_aggregate_16(code, P(f), P(a), P(a), H, D_, 0.2, 0.0, 0, P(cd.row32), P(cd.col32), P(cd.eid32), P(cd.indptr), E, n, n,
                                       P(outs[0]), None, None, None, None, P(ws), need - ws_short, pgl.ops._stream(f))
    else:
        outs += [torch.full((n, H), CANARY, dtype=torch.int32, device=dev_) for _ in range(2)]
        need = L.pglamd_gat_backward_workspace_bytes(E, n, H, D_)
        ws = pgl.ops._ws(need, dev_)
        rc = L.pglamd_gat_backward_16(code, P(f), P(f), P(a), P(a), P(a), P(ones), P(f), H, D_, 0.2, 0.0, 0, P(cd.row32), P(cd.col32), P(cd.eid32),
                                      P(cd.indptr), P(cs.row32), P(cs.col32), P(cs.eid32), P(cs.indptr), E, n, P(outs[0]), P(outs[1]),
                                      P(outs[2]), None, None, None, P(ws), need - ws_short, pgl.ops._stream(f))
    torch.cuda.synchronize()
    return rc, all(bool((o == CANARY).all()) for o in outs)


def test_gat16_supported_is_what_the_abi_accepts(pgl, graphs):
    """Every (H, D) with H <= 8 and D <= 64, forward and backward: PGLAMD_OK where gat16_supported says yes, PGLAMD_E_SHAPE with nothing
    written where it says no."""
    G = graphs["E1"]
    att = pgl.attention_ops
    yes = {False: 0, True: 0}
    for backward in (False, True):
        for H in range(1, 9):
            for D_ in range(1, 65):
                dt = DTYPES[(H + D_) % 2]
                rc, untouched = _abi(pgl, G, H, D_, dt, backward=backward)
                ok = att.gat16_supported(H, D_, backward=backward)
                yes[backward] += ok
                assert rc == (0 if ok else -1), (H, D_, backward, rc)
                assert untouched == (not ok), (H, D_, backward)
    assert 512 > yes[False] > yes[True] > 0            # both answers occur in both directions; the backward takes fewer shapes
    assert att.gat16_supported(4, 64) and not att.gat16_supported(8, 64) and not att.gat16_supported(3, 6, backward=True)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_the_abi_refuses_without_writing(pgl, graphs, backward):
    G = graphs["classes"]
    assert _abi(pgl, G, 8, 16, torch.float16, backward=backward) == (0, False)
    for code in (1, 2, 3, 7, -1):                                           # PGLAMD_F32, F64, I32, nothing, nothing
        assert _abi(pgl, G, 8, 16, torch.float16, code=code, backward=backward) == (-6, True), code       # PGLAMD_E_ARG
    assert _abi(pgl, G, 8, 16, torch.bfloat16, ws_short=1, backward=backward) == (-4, True)                # PGLAMD_E_WORKSPACE
    assert _abi(pgl, G, 8, 64, torch.bfloat16, backward=backward) == (-1, True)                            # PGLAMD_E_SHAPE: H * D = 512 > 256


def test_other_dtypes_are_still_refused(pgl, graphs):
    G = graphs["hub"]
    f, a_s, a_d, _ = _inputs(G, 8, 16, torch.float16)
    with pytest.raises(TypeError):
        G.g.gat_aggregate(f.double(), a_s.double(), a_d.double(), 0.2)
    with pytest.raises(TypeError):
        pgl.attention_ops.gat_aggregate16(f.float(), a_s, a_d, G.g._csr_dst())
    with pytest.raises(TypeError):
        pgl.ops.gat_aggregate(f, a_s, a_d, G.g._csr_dst())
