"""Rows a7-a9 -- Graph.send_uv (pgl/graph.py:939-966), GF.edge_softmax / pgl.math.segment_softmax (pgl/nn/functional/graph_op.py:101-123, pgl/math.py:181-224), Graph.send_ue_recv (pgl/graph.py:889-937) and their gradients (f1).

Regrouped by SURVEY section 8 row in round 6 (rounds 1-5 kept these tests in files named after the round that added them:
test_gpu_parity.py, test_gpu_round2..5.py); the shared fixtures and the per-element error bounds are in tests/gpu_common.py."""
import ctypes                                   # noqa: F401
import os                                       # noqa: F401
import subprocess                               # noqa: F401
import sys                                      # noqa: F401

import numpy as np                              # noqa: F401
import pytest
import torch                                    # noqa: F401

import golden_vectors as G                      # noqa: F401
import grad_defs as GD                          # noqa: F401
import ref_ops as R                             # noqa: F401
from gpu_common import *                        # noqa: F401,F403

pytestmark = pytest.mark.gpu


def test_g2_send_ue_recv(pgl):
    g = pgl.Graph(edges=G.G1_EDGES, num_nodes=G.G1_N).tensor()
    out = g.send_ue_recv(dev(G.G1_X.astype(np.float32)), dev(G.G2_EFEAT.astype(np.float32)), "add", "sum")
    assert np.array_equal(host(out), G.G2_OUT.astype(np.float32))


def test_g3_segment_softmax(pgl):
    out = pgl.math.segment_softmax(dev(G.G3_DATA), dev(G.G3_IDS))
    np.testing.assert_allclose(host(out), G.G3_OUT, rtol=0, atol=1e-6)
    big = host(pgl.math.segment_softmax(dev(G.G3_DATA_BIG), dev(G.G3_IDS.astype(np.int32))))
    assert np.isfinite(big).all()
    np.testing.assert_allclose(big, G.G3_OUT_BIG, rtol=0, atol=1e-6)


def test_g4_edge_softmax_exact(pgl):
    g = pgl.Graph(edges=G.G4_EDGES, num_nodes=G.G4_N).tensor()
    by_dst = host(pgl.nn.functional.edge_softmax(g, dev(G.G4_LOGITS)))
    by_src = host(pgl.nn.functional.edge_softmax(g, dev(G.G4_LOGITS), norm_by="src"))
    assert np.array_equal(by_dst, G.G4_BY_DST)
    assert np.array_equal(by_src, G.G4_BY_SRC)


# ------------------------------------------------------------------------------------------------
# send_ue_recv / send_uv
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mop", ["add", "sub", "mul", "div"])
@pytest.mark.parametrize("rop", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("shape", [((8, 16), (8, 1)), ((8, 16), (8, 16)), ((32,), (1,)), ((4, 1), (4, 8)), ((6,), (6,))])
def test_send_ue_recv(pgl, mop, rop, shape):
    n, e = 1500, 20000
    xs, ys = shape
    edges, rng = rand_graph(n, e, 31, hub=2100)
    x = rng.standard_normal((n,) + xs).astype(np.float32)
    y = (rng.standard_normal((e,) + ys) + 3.0).astype(np.float32)
    want = R.c_send_ue_recv(x, y, edges[:, 0], edges[:, 1], mop, rop)
    got = host(pgl.Graph(edges=edges, num_nodes=n).tensor().send_ue_recv(dev(x), dev(y), mop, rop))
    assert got.shape == want.shape
    check_aggregate(got, x, edges[:, 0], edges[:, 1], rop, y=y, mop=mop, want=want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_send_ue_recv_operand_layouts_and_widths(pgl, dtype):
    """Edge operand as a full row, one scalar per edge, one weight per head (the GAT layout, heads <= 8 and > 8), across the
    widths where the lane-per-edge / flat / generic kernels take over from each other; hubs and empty rows included."""
    n, e = 2500, 40000
    edges, rng = rand_graph(n, e, 5151, hub=9000)
    edges[edges[:, 1] % 8 == 0, 1] = 5
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    ops_cycle = [("mul", "sum"), ("add", "mean"), ("mul", "max"), ("sub", "sum"), ("div", "mean"), ("add", "min")]
    for i, (xs, ys) in enumerate(UE_SHAPES):
        x = rng.standard_normal((n,) + xs).astype(dtype)
        y = (rng.standard_normal((e,) + ys) + 3.0).astype(dtype)
        for mop, rop in (ops_cycle[i % 6], ops_cycle[(i + 3) % 6]):
            want = R.c_send_ue_recv(x, y, edges[:, 0], edges[:, 1], mop, rop)
            got = host(g.send_ue_recv(dev(x), dev(y), mop, rop))
            assert got.shape == want.shape
            check_aggregate(got, x, edges[:, 0], edges[:, 1], rop, y=y, mop=mop, want=want, what="%s %s %s %s" % (xs, ys, mop, rop))


@pytest.mark.parametrize("mop", ["add", "sub", "mul", "div"])
@pytest.mark.parametrize("shape", [((8,), (8,)), ((8, 16), (8, 1)), ((5,), (5,)), ((1,), (7,))])
def test_send_uv(pgl, mop, shape):
    n, e = 1200, 15000
    edges, rng = rand_graph(n, e, 32)
    x = rng.standard_normal((n,) + shape[0]).astype(np.float32)
    y = (rng.standard_normal((n,) + shape[1]) + 3.0).astype(np.float32)
    want = R.c_send_uv(x, y, edges[:, 0], edges[:, 1], mop)
    got = host(pgl.Graph(edges=edges, num_nodes=n).tensor().send_uv(dev(x), dev(y), mop))
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=0)      # one rounding (div) at most


@pytest.mark.parametrize("d", [1, 8, 16, 100])
def test_segment_softmax_random(pgl, d):
    rng = np.random.default_rng(50 + d)
    ids = np.sort(rng.integers(0, 300, 20000)).astype(np.int64)
    ids[1000:4000] = ids[1000]
    ids = np.sort(ids)
    data = (rng.standard_normal((20000, d)) * 4).astype(np.float32)
    want = R.c_segment_softmax(data, ids)
    got = host(pgl.math.segment_softmax(dev(data), dev(ids)))
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("norm_by", ["dst", "src"])
def test_edge_softmax_random(pgl, norm_by):
    n, e, h = 2000, 40000, 8
    edges, rng = rand_graph(n, e, 60, hub=5000)
    logits = (rng.standard_normal((e, h)) * 3).astype(np.float32)
    want = R.np_edge_softmax(edges, n, logits, norm_by)
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    got = host(pgl.nn.functional.edge_softmax(g, dev(logits), norm_by))
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-7)


def test_full_size_gat_path_properties(pgl, rmat20):
    g, x = rmat20
    h = 8
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    a_s = torch.randn(g.num_nodes, h, generator=gen, device="cuda")
    a_d = torch.randn(g.num_nodes, h, generator=gen, device="cuda")
    alpha = torch.nn.functional.leaky_relu(g.send_uv(a_s, a_d, "add"), 0.2)
    alpha = pgl.nn.functional.edge_softmax(g, alpha)
    # softmax rows sum to one per destination with in-edges (idempotent checksum, any size)
    sums = g.send_ue_recv(torch.ones(g.num_nodes, h, 1, device="cuda"), alpha.reshape(-1, h, 1), "mul", "sum").reshape(-1, h)
    has = g.indegree() > 0
    assert float((sums[has] - 1).abs().max()) < 1e-4 and float(sums[~has].abs().max()) == 0.0
    out = g.send_ue_recv(x.reshape(-1, h, 16), alpha.reshape(-1, h, 1), "mul", "sum")
    # convex combination: every output lies inside the min/max envelope of the inputs
    assert float(out.max()) <= float(x.max()) + 1e-4 and float(out.min()) >= float(x.min()) - 1e-4
    # sampled rows against the numpy oracle
    e = host(g.edges)
    rows = np.unique(e[::400000, 1])[:40]
    sel = np.isin(e[:, 1], rows)
    sub = e[sel]
    w64, a64, nt = fp64_terms(host(x).reshape(-1, h, 16), sub[:, 0], sub[:, 1], "sum", y=host(alpha)[sel].reshape(-1, h, 1), mop="mul")
    assert_within_fp32_reassociation(host(out)[rows], w64[rows], a64[rows], nt[rows])     # per element: the row's own alpha * |f| terms


@pytest.mark.parametrize("H,D", [(8, 16), (4, 4), (1, 32), (3, 8)])
def test_sddmm_and_send_ue_recv_edge_gradient(pgl, H, D):
    n, e = 1500, 20000
    edges, rng = rand_graph(n, e, 900 + H)
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    x = dev(rng.standard_normal((n, H, D)).astype(np.float32))
    y = dev(rng.standard_normal((n, H, D)).astype(np.float32))
    got = host(pgl.ops.sddmm(x, y, g.adj_dst_index.csr))
    want = (host(x)[edges[:, 0]] * host(y)[edges[:, 1]]).sum(-1)
    close_terms(got, want, (np.abs(host(x))[edges[:, 0]] * np.abs(host(y))[edges[:, 1]]).sum(-1), D + 1)      # a dot product of D terms per (edge, head)
    # gradient of send_ue_recv(mul, sum) w.r.t. the edge operand [E,H,1] and the node features
    ef = dev(rng.standard_normal((e, H, 1)).astype(np.float32)).requires_grad_(True)
    xf = x.clone().requires_grad_(True)
    w = dev(rng.standard_normal((n, H, D)).astype(np.float32))
    (g.send_ue_recv(xf, ef, "mul", "sum") * w).sum().backward()
    want_e = (host(x)[edges[:, 0]] * host(w)[edges[:, 1]]).sum(-1, keepdims=True)
    close_terms(host(ef.grad), want_e, (np.abs(host(x))[edges[:, 0]] * np.abs(host(w))[edges[:, 1]]).sum(-1, keepdims=True), D + 1)
    # d/dx[u] = sum over u's out-edges of w[v] * ef[e]: the aggregation over the REVERSED edges with the same edge operand
    check_aggregate(host(xf.grad), host(w), edges[:, 1], edges[:, 0], "sum", y=host(ef.detach()), mop="mul")


@pytest.mark.parametrize("mop", ["add", "sub", "mul", "div"])
@pytest.mark.parametrize("rop", ["sum", "mean"])
@pytest.mark.parametrize("dx,dy", [(1, 1), (8, 8), (8, 1), (3, 3), (5, 1), (16, 16)])
def test_narrow_rows_send_ue_recv(pgl, mop, rop, dx, dy):
    n, e = 3000, 50000
    edges, rng = rand_graph(n, e, 400 + dx + dy, hub=9000)
    x = rng.standard_normal((n, dx)).astype(np.float32)
    y = (rng.standard_normal((e, dy)) + 3.0).astype(np.float32)
    want = R.c_send_ue_recv(x, y, edges[:, 0], edges[:, 1], mop, rop)
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    got = host(g.send_ue_recv(dev(x), dev(y), mop, rop))
    check_aggregate(got, x, edges[:, 0], edges[:, 1], rop, y=y, mop=mop, want=want)


@pytest.mark.parametrize("d", [1, 2, 3, 5, 8, 16])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_narrow_segment_softmax_one_pass(pgl, d, dtype):
    if dtype == np.float64 and d > 8:
        pytest.skip("fp64 d>8 takes the wide path (covered by test_segment_softmax_random)")
    rng = np.random.default_rng(600 + d)
    ids = rng.integers(0, 500, 60000)
    ids[2000:32000] = 250                                       # one segment of 30k elements (~120 chunks)
    ids[40000:40300] = 251
    ids = np.sort(ids).astype(np.int64)
    data = (rng.standard_normal((60000, d)) * 6).astype(dtype)
    data[100] = 80.0                                            # large logits: the running maximum must protect exp
    want = R.c_segment_softmax(data, ids)
    got = host(pgl.math.segment_softmax(dev(data), dev(ids)))
    if dtype == np.float32:
        # the 30k-element segment is summed serially in fp32 by the reference loop (its own rounding noise is ~3e-5
        # there): <=1e-5 against the same loop in fp64, and within that noise of the fp32 loop itself
        exact = R.c_segment_softmax(data.astype(np.float64), ids)
        np.testing.assert_allclose(got, exact, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-7)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    sums = np.zeros((500, d)); np.add.at(sums, ids, got)
    present = np.isin(np.arange(500), ids)
    np.testing.assert_allclose(sums[present], 1.0, rtol=1e-4)


@pytest.mark.parametrize("H,D", [(4, 8), (8, 16), (2, 32), (3, 5)])
def test_graph_sddmm_and_gradients(pgl, H, D):
    n, e = 1500, 20000
    edges, rng = rand_graph(n, e, 777 + H, hub=3000)
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    x = dev(rng.standard_normal((n, H, D)).astype(np.float32)).requires_grad_(True)
    y = dev(rng.standard_normal((n, H, D)).astype(np.float32)).requires_grad_(True)
    ct = dev(rng.standard_normal((e, H)).astype(np.float32))
    out = g.sddmm(x, y)
    src, dst = torch.as_tensor(edges[:, 0]).cuda(), torch.as_tensor(edges[:, 1]).cuda()
    x2, y2 = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    ref = (x2[src] * y2[dst]).sum(-1)
    close_rows(host(out), host(ref))
    (out * ct).sum().backward(); (ref * ct).sum().backward()
    close_rows(host(x.grad), host(x2.grad), rtol=2e-5)
    close_rows(host(y.grad), host(y2.grad), rtol=2e-5)


@pytest.mark.parametrize("H,D", [(4, 8), (8, 16), (1, 64), (3, 4)])
@pytest.mark.parametrize("order", ["edge", "csr"])
def test_additive_score_and_gradients(pgl, H, D, order):
    """GATv2's score sum_d w[h,d] * leaky(x[src] + y[dst]) and all three gradients vs the composed torch formulation;
    hub rows span many chunks (partials + fix-up), in original edge order and in dst-sorted order."""
    from pgl_amd import autograd as ag
    n, e = 1500, 24000
    edges, rng = rand_graph(n, e, 900 + H, hub=4000)
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    mk = lambda *s: dev(rng.standard_normal(s).astype(np.float32)).requires_grad_(True)
    x, y, w = mk(n, H, D), mk(n, H, D), mk(H, D)
    if order == "edge":
        cd, cs = g._csr_dst(), g._csr_src()
        src, dst = torch.as_tensor(edges[:, 0]).cuda(), torch.as_tensor(edges[:, 1]).cuda()
    else:
        cd, cs = g._csr_order_views()
        src, dst = cd.col32.long(), cd.row32.long()
    out = ag.add_score(x, y, w, cd, lambda: cs, 0.2)
    x2, y2, w2 = (t.detach().clone().requires_grad_(True) for t in (x, y, w))
    ref = (torch.nn.functional.leaky_relu(x2[src] + y2[dst], 0.2) * w2).sum(-1)
    close_rows(host(out), host(ref), rtol=2e-5)
    ct = dev(rng.standard_normal((e, H)).astype(np.float32))
    (out * ct).sum().backward(); (ref * ct).sum().backward()
    for a, b, name in ((x, x2, "x"), (y, y2, "y"), (w, w2, "w")):
        close_rows(host(a.grad), host(b.grad), rtol=1e-4)


def test_c3_send_ue_recv_mul_sum_per_element(pgl):
    """send_ue_recv(mul, sum) with [E, H, 1] weights (the GAT path's aggregation, BASELINE configs[2] shapes) element by
    element within the reassociation bound of fp64."""
    from pgl_amd.utils.rmat import rmat_edges
    N, E, H, D = 1 << 20, 20_000_000, 8, 16
    edges = rmat_edges(20, E, seed=42, device=torch.device("cuda"))
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    f = torch.randn(N, H, D, generator=gen, device="cuda")
    w = torch.rand(E, H, 1, generator=gen, device="cuda")
    g = pgl.Graph(edges=edges, num_nodes=N)
    got = g.send_ue_recv(f, w, "mul", "sum").reshape(N, H * D)
    src, dst = edges[:, 0], edges[:, 1]
    s64 = torch.zeros((N, H * D), dtype=torch.float64, device="cuda")
    a64 = torch.zeros((N, H * D), dtype=torch.float64, device="cuda")
    step = 2_000_000                                                           # (the [E, H, D] message is never whole in memory)
    for b in range(0, E, step):
        m = (f[src[b:b + step]].double() * w[b:b + step].double()).reshape(-1, H * D)
        s64.index_add_(0, dst[b:b + step], m)
        a64.index_add_(0, dst[b:b + step], m.abs())
    deg = torch.bincount(dst, minlength=N)
    _assert_bound(got, s64, a64, deg + 2, float(np.finfo(np.float32).eps))


# ------------------------------------------------------------------------------------------------
# gradient kernels that replace the [E, d] gather compositions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 100, 128, 256])
@pytest.mark.parametrize("op", ["max", "min"])
def test_winner_gradient_kernel(pgl, d, op):
    """d x of send_recv(x, max | min): every message equal to the winner gets the row's gradient (ties included: x takes few
    distinct values), hub source and hub destination (split rows in both walks), vs the edge-by-edge formulation."""
    rng = np.random.default_rng(d)
    n, e = 2500, 40000
    edges = np.stack([rng.integers(0, n, e), rng.integers(0, n, e)], 1).astype(np.int64)
    edges[rng.choice(e, 6000, replace=False), 0] = 3
    edges[rng.choice(e, 6000, replace=False), 1] = 8
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    x = dev(rng.integers(-3, 4, (n, d)).astype(np.float32)).requires_grad_(True)
    w = dev(rng.standard_normal((n, d)).astype(np.float32))
    out = g.send_recv(x, op)
    (out * w).sum().backward()
    src, dst = dev(edges[:, 0]), dev(edges[:, 1])
    hit = (x.detach()[src] == out.detach()[dst]).float()
    want = torch.zeros(n, d, device="cuda", dtype=torch.float64).index_add_(0, src, (w[dst] * hit).double())
    # per element, inside the bound of the element's own terms
    n_out, n_terms = GD.aggregate_n_terms(src, dst, x.shape, None, op)
    r = GD.grad_and_terms(lambda a, frozen=None: GD.send_recv(a, src, dst, op, frozen=frozen), [x.detach()], w, n_out, n_terms[:1],
                          lambda a: GD.winner_mask(a, src, dst, op))
    check_grad_elements(x.grad, want, r.abs_terms64[0], r.n_terms[0], what="d x vs the inline formulation")
    check_grad_elements(x.grad, r.want64[0], r.abs_terms64[0], r.n_terms[0], what="d x")
    x2 = x.detach().clone().requires_grad_(True)                    # bit-reproducible
    (g.send_recv(x2, op) * w).sum().backward()
    assert torch.equal(x2.grad, x.grad)


@pytest.mark.parametrize("yshape", ["E", "E1", "Ed", "EHD", "EH1"])
@pytest.mark.parametrize("mop,rop", [("mul", "sum"), ("add", "mean"), ("sub", "sum"), ("div", "mean")])
def test_edge_operand_gradient_kernel(pgl, yshape, mop, rop):
    """d y (and d x) of send_ue_recv for every trailing-dim broadcast shape of the edge operand, vs torch autograd of the
    edge-by-edge formulation in fp64."""
    rng = np.random.default_rng(7)
    n, e, H, D = 1500, 20000, 8, 16
    edges = np.stack([rng.integers(0, n, e), rng.integers(0, n, e)], 1).astype(np.int64)
    edges[rng.choice(e, 3000, replace=False), 1] = 5
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    xs = (n, H, D) if yshape in ("EHD", "EH1") else (n, H * D)
    ys = {"E": (e,), "E1": (e, 1), "Ed": (e, H * D), "EHD": (e, H, D), "EH1": (e, H, 1)}[yshape]
    x = dev(rng.standard_normal(xs).astype(np.float32)).requires_grad_(True)
    y = dev((rng.random(ys) + 0.5).astype(np.float32)).requires_grad_(True)
    w = dev(rng.standard_normal(xs).astype(np.float32))
    out = g.send_ue_recv(x, y, mop, rop)
    (out * w).sum().backward()
    src, dst = dev(edges[:, 0]), dev(edges[:, 1])
    x64, y64 = x.detach().double().requires_grad_(True), y.detach().double().requires_grad_(True)
    yb = y64.reshape((e,) + (1,) * (len(xs) - len(ys)) + tuple(ys[1:])) if len(ys) < len(xs) else y64
    m = {"mul": x64[src] * yb, "add": x64[src] + yb, "sub": x64[src] - yb, "div": x64[src] / yb}[mop]
    ref = torch.zeros(xs, device="cuda", dtype=torch.float64).index_add_(0, dst, m)
    if rop == "mean":
        deg = torch.bincount(dst, minlength=n).clamp(min=1).double()
        ref = ref / deg.reshape((-1,) + (1,) * (len(xs) - 1))
    (ref * w.double()).sum().backward()
    # per element, inside the bound of the element's own terms
    n_out, n_terms = GD.aggregate_n_terms(src, dst, xs, ys, rop)
    r = GD.grad_and_terms(lambda a, b, frozen=None: GD.send_recv(a, src, dst, rop, None, b, mop, frozen=frozen), [x.detach(), y.detach()], w,
                          n_out, n_terms)
    check_grad_elements(out, ref.detach(), r.out_abs, r.out_n, what="forward")
    for i, (got, want, name) in enumerate(((x.grad, x64.grad, "d x"), (y.grad, y64.grad, "d y"))):
        assert tuple(got.shape) == tuple(want.shape), name
        check_grad_elements(got, want, r.abs_terms64[i], r.n_terms[i], what=name)


# ------------------------------------------------------------------------------------------------
# send_uv / segment softmax kernels reworked in round 4 (several element groups in flight per thread, streamed operands
# non-temporal): sizes around the unroll boundaries.  Reference: pgl/graph.py:939-966, pgl/math.py:181-224
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e,d", [(1, 8), (255, 8), (1023, 4), (1025, 8), (4099, 12), (70001, 8), (300000, 6), (65536 * 4 + 3, 16)])
def test_send_uv_and_edge_softmax_at_unroll_boundaries(pgl, e, d):
    rng = np.random.default_rng(e + d)
    n = max(2, e // 7)
    src = rng.integers(0, n, e); dst = rng.integers(0, n, e)
    edges = np.stack([src, dst], 1).astype(np.int64)
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    a = rng.standard_normal((n, d)).astype(np.float32); b = rng.standard_normal((n, d)).astype(np.float32)
    for mop in ("add", "sub", "mul", "div"):
        bb = b if mop != "div" else np.abs(b) + 0.5
        got = host(g.send_uv(dev(a), dev(bb), mop))
        want = R.np_send_uv(a, bb, src, dst, mop)
        np.testing.assert_allclose(got, want, rtol=2e-7, atol=1e-7)
    logits = rng.standard_normal((e, d)).astype(np.float32) * 3
    got = host(pgl.nn.functional.edge_softmax(g, dev(logits)))
    want = R.np_edge_softmax(edges, n, logits)                  # the oracle's restatement of GF.edge_softmax (graph_op.py:117-123)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-7)
    sums = np.zeros((n, d)); np.add.at(sums, dst, got)
    assert np.allclose(sums[np.bincount(dst, minlength=n) > 0], 1.0, atol=1e-5)


@pytest.mark.parametrize("accumulate,out_rows", [(0, None), (1, None), (2, None), (0, 2500)])
def test_abi_edge_operand_e1_mul_reroute_equals_the_general_path(pgl, accumulate, out_rows):
    """low: pglamd_aggregate with y = [E, 1], eid = NULL, MUL, sum, fp32, rows wider than 128 B is answered by the per-position
    scale slot of the flat kernel (documented in include/pgl_amd.h next to the eid == NULL semantics).  Called straight through
    ctypes here and compared with the SAME call carrying an identity eid (the general edge-operand path) and with the oracle,
    including accumulate = 1 / 2 and out_rows < n_csr_rows."""
    from pgl_amd import _ffi
    ops = pgl.ops
    rng = np.random.default_rng(8)
    n, e, d = 4000, 60000, 128
    src = rng.integers(0, n, e).astype(np.int64)
    dst = np.sort(rng.integers(0, (out_rows or n) // 2, e) * 2).astype(np.int64)     # already in destination order: position p == edge p
    x = rng.standard_normal((n, d)).astype(np.float32)
    y = rng.standard_normal((e, 1)).astype(np.float32)
    csr = ops.csr_build(dev(dst), dev(src), n, want_i64=False)
    assert torch.equal(csr.eid32.long(), torch.arange(e, device="cuda"))
    rows = out_rows or n
    before = rng.standard_normal((rows, d)).astype(np.float32)
    ident = torch.arange(e, dtype=torch.int32, device="cuda")

    def call(eid):
        out = dev(before.copy())
        xt, yt = dev(x), dev(y)
        L = _ffi.lib()
        ws_bytes = L.pglamd_aggregate_workspace_bytes(e, d, 1)
        ws = torch.empty(max(int(ws_bytes), 256), dtype=torch.uint8, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        rc = L.pglamd_aggregate(p(xt), 1, n, d, p(yt), 1, p(eid), p(csr.row32), p(csr.col32), p(csr.indptr), e, n, rows, d, 2, 0,
                                None, None, accumulate, p(out), p(ws), ws.numel(), st)
        _ffi.check(rc, "aggregate")
        torch.cuda.synchronize()
        return host(out)

    a, b = call(None), call(ident)
    close_rows(a, b, rtol=2e-6, atol_row=2e-6)
    want = R.c_send_ue_recv(x, y, src, dst, "mul", "sum", out_size=rows)
    has = np.bincount(dst, minlength=rows) > 0
    if accumulate == 1:
        want = want + before                                             # rows without edges: 0 + their old contents
    elif accumulate == 2:
        want = np.where(has[:, None], want, before)
    close_rows(a, want, rtol=1e-5, atol_row=1e-5)
