"""Attention dropout of the fused GAT kernels (pgl_amd/csrc/gat_fused.hip, the DROP = true instantiations) held to its DEFINITION.

The mask is written down next to pglamd_gat_aggregate in include/pgl_amd.h; grad_defs.attention_keep restates it in numpy (and
tests/test_grad_defs.py holds the restatement to values taken from the kernel's own text).  Here:

  a. the kernels' mask IS the documented one, bit by bit: a graph on which every (edge, head) owns an output element;
  b. forward and every gradient against the fp64 definition with the keep factor, element by element (assert_grads), over the hub and
     the classes graph, every lane width, three dropout rates and the three backward routes;
  c. the bound refuses four wrong masks;
  d. GATConv in training mode against the fp64 composition, the seed read from torch's generator as the layer's docstring says;
  e. ops.gat_aggregate(out_size=...) below and above the number of rows of the index.

K for the families gat_drop / gat_proj_drop: measured from the fp32 DEFINITION on the host (test_gradients_gpu._measure_definitions),
see the table in that module's docstring."""
import numpy as np
import pytest
import torch

import grad_defs as D
import test_gradients_gpu as T
from gpu_common import pgl, close_rows, host, rand_graph  # noqa: F401  (pgl: the fixture)
from test_gradients_gpu import assert_grads, _graphs, lattice, rows, _t, GAT_HD, GAT_PROJ_HD, GAT_BACKWARD_ROUTES  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def graphs(pgl):
    return _graphs(pgl)


# ------------------------------------------------------------------------------------------------
# a. the mask, bit by bit
# ------------------------------------------------------------------------------------------------
MASK_E = 70000
# the issue's three shapes (gat_vec takes the smallest lane width that fits 64 lanes: all three run with 1 column per lane) and two
# more for 2 and 4 columns per lane
MASK_SHAPES = [(4, 16), (1, 64), (8, 2), (8, 16), (8, 32)]


def _mask_graph(pgl_, dmax, seed=71):
    """MASK_E edges, edge e from a source of its own (node e) to one of the destinations MASK_E + j, which receive between 1 and dmax
    edges each; the edge list is shuffled, so an edge's original id is not its position in the dst-sorted stream.
    -> (graph, rank [E]: the edge's slot among its destination's edges, deg [n_dst])."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, dmax + 1, MASK_E)
    cut = int(np.searchsorted(np.cumsum(deg), MASK_E))
    deg = deg[:cut + 1].copy()
    deg[-1] -= deg.sum() - MASK_E
    assert deg.sum() == MASK_E and deg.min() >= 1 and deg.max() == dmax and (deg == 1).any()
    start = np.cumsum(deg) - deg
    dst_sorted = np.repeat(np.arange(len(deg)), deg)
    rank_sorted = np.arange(MASK_E) - start[dst_sorted]
    perm = rng.permutation(MASK_E)
    dst, rank = dst_sorted[perm] + MASK_E, rank_sorted[perm]
    G = T._G(pgl_, MASK_E + len(deg), np.arange(MASK_E), dst)
    position = np.empty(MASK_E, np.int64)
    position[np.argsort(dst, kind="stable")] = np.arange(MASK_E)
    assert (position != np.arange(MASK_E)).mean() > 0.99
    return G, rank, deg


def _ulps(got, want):
    """|got - want| in units of want's fp32 spacing (0 where both are 0)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(1e-30))).astype(np.float64)


@pytest.mark.parametrize("H,D_", MASK_SHAPES)
def test_the_kernels_mask_is_the_documented_one(pgl, H, D_):
    """a_src = a_dst = 0: alpha = 1 / deg.  f[e, h, k] = 1 where k is edge e's slot in its destination row: out[v, h, k] is that ONE
    edge's keep factor times 1 / deg -- non-zero exactly where attention_keep keeps (edge, head), and fl32(factor * fl32(1 / deg))
    (the kernel's own two roundings), held to one ulp.  With a cotangent of ones d f[e, h, :] = keep * alpha_e: the same pattern from
    the src-sorted walk, whose edge ids come through src_eid.  Both forms of the forward (with and without the statistics), two
    rates, two seeds (one >= 2**31, a Python int), and the same bits on a second run."""
    G, rank, deg = _mask_graph(pgl, D_)
    E, n = G.e, G.n
    f = np.zeros((n, H, D_), np.float32)
    f[np.arange(E), :, rank] = 1.0
    f = _t(f)
    a = torch.zeros((n, H), dtype=torch.float32, device=f.device)
    inv = (np.float32(1.0) / deg.astype(np.float32))[G.dst_np - E]                       # [E] fl32(1 / deg) of the edge's destination
    csr = G.g._csr_dst()
    exact = True
    for p in (0.4, 0.6):
        for seed in (1234, 2 ** 32 - 7):
            keep = D.attention_keep(seed, np.arange(E), H, p)                           # [E, H], by ORIGINAL edge id
            assert 0.9 * (1 - p) < (keep > 0).mean() < 1.1 * (1 - p)
            val = keep * inv[:, None]                                                   # fp32 x fp32 -> fp32: rounded once
            assert val.dtype == np.float32
            want = np.zeros((n, H, D_), np.float32)
            want[G.dst_np, :, rank] = val
            want_df = np.zeros((n, H, D_), np.float32)
            want_df[:E] = val[:, :, None]
            what = "%dx%d p=%g seed=%d" % (H, D_, p, seed)
            outs = [pgl.ops.gat_aggregate(f, a, a, csr, 0.2, None, False, p, seed),
                    pgl.ops.gat_aggregate(f, a, a, csr, 0.2, None, True, p, seed)[0],
                    pgl.ops.gat_aggregate(f, a, a, csr, 0.2, None, False, p, seed)]
            fg = f.detach().requires_grad_(True)
            out = G.g.gat_aggregate(fg, a, a, 0.2, p, seed)
            out.backward(torch.ones_like(out))
            outs.append(out.detach())
            for o in outs[1:]:
                assert torch.equal(o, outs[0]), what + ": the forms of the forward (or two runs) differ"
            got, got_df = host(outs[0]), host(fg.grad)
            assert np.array_equal(got != 0, want != 0), "%s: %d (edge, head) pairs kept / dropped against the documented mask" % (
                what, int(((got != 0) != (want != 0)).sum()))
            assert np.array_equal(got_df != 0, want_df != 0), what + ": d f carries another mask"
            u_out, u_df = float(_ulps(got, want).max()), float(_ulps(got_df, want_df).max())
            print("%s: out %s (worst %.2f ulp), d f %s (worst %.2f ulp)" % (what, "exact" if u_out == 0 else "not exact", u_out,
                                                                        "exact" if u_df == 0 else "not exact", u_df))
            assert u_out <= 1.0 and u_df <= 1.0, (what, u_out, u_df)
            exact = exact and u_out == 0 and u_df == 0
    print("%dx%d: fl32(factor * fl32(1 / deg)) reproduced %s" % (H, D_, "exactly" if exact else "within one ulp"))


# ------------------------------------------------------------------------------------------------
# b. fp64, element by element, with dropout on
# ------------------------------------------------------------------------------------------------
def _dead_pairs(G, kd):
    """(row, head) pairs with in-edges that lose every one of them."""
    alive = torch.zeros((G.n, kd.shape[1]), dtype=torch.float64, device=kd.device).index_add(0, G.dst, (kd > 0).double())
    return (G.indeg > 0)[:, None] & (alive == 0)


@pytest.mark.parametrize("graph,H,D_", T._both_graphs(GAT_HD))
def test_gat_attention_with_dropout(graphs, graph, H, D_):
    T._gat_drop_case(graphs[graph], graph, H, D_, 0.6)


@pytest.mark.parametrize("graph", ["hub", "classes"])
@pytest.mark.parametrize("p,H,D_", T.GAT_DROP_EXTRA_P)
def test_gat_attention_with_light_and_heavy_dropout(graphs, graph, p, H, D_):
    """p = 0.1 and p = 0.9.  At 0.9 many (row, head) pairs lose every edge: their output is exactly 0, and so is their t[v, h] =
    <g, out> -- seen from outside as d a_dst[v, h] = sum_e alpha_e leaky'_e (keep_e <g, f_u> - t) = 0 exactly."""
    G = graphs[graph]
    f, a_s, a_d, cot, kd, seed = T._gat_drop_case(G, graph, H, D_, p)
    if p < 0.9:
        return
    dead = _dead_pairs(G, kd)
    n_dead = int(dead.sum())
    print("gat %s %dx%d p=%g: %d (row, head) pairs lose every edge" % (graph, H, D_, p, n_dead))
    assert n_dead >= 1000
    xs = [t.detach().requires_grad_(True) for t in (f, a_s, a_d)]
    out = G.g.gat_aggregate(*xs, 0.2, p, seed)
    out.backward(cot)
    assert bool((out.detach()[dead] == 0).all()), "a row without a kept edge is not exactly 0"
    assert bool((xs[2].grad[dead] == 0).all()), "d a_dst of a row without a kept edge is not exactly 0: t[v, h] is not"


@pytest.mark.parametrize("H,D_", [(4, 8), (8, 16), (8, 32)])
@pytest.mark.parametrize("route", list(GAT_BACKWARD_ROUTES))
def test_gat_attention_with_dropout_over_every_backward_route(pgl, graphs, route, H, D_):
    """The three ways to d a_dst with the mask on: the pack kernel's per-node formula (out_pos carries the mask, sum_pos does not), the
    src-sorted walk's d pre_e buffer, and the dst-sorted walk -- on the classes graph, at 1, 2 and 4 columns per lane."""
    keep = (pgl.ops._GAT_POS_STATS, pgl.ops._GAT_BWD_EDGE_BUFFER)
    try:
        pgl.ops._GAT_POS_STATS, pgl.ops._GAT_BWD_EDGE_BUFFER = GAT_BACKWARD_ROUTES[route]
        T._gat_drop_case(graphs["classes"], "classes", H, D_, 0.6, what=" " + route)
    finally:
        pgl.ops._GAT_POS_STATS, pgl.ops._GAT_BWD_EDGE_BUFFER = keep


@pytest.mark.parametrize("H,D_", GAT_PROJ_HD)
def test_gat_attention_with_the_projection_inside_and_dropout(graphs, H, D_):
    T._gat_proj_drop_case(graphs["hub"], H, D_, 0.6)


# ------------------------------------------------------------------------------------------------
# c. the bound refuses a wrong mask
# ------------------------------------------------------------------------------------------------
def _refused(G, graph, forward, check=None, **wrong):
    with pytest.raises(AssertionError, match="out of bound"):
        T._gat_drop_case(G, graph, 8, 16, 0.6, forward=forward, check=check, what=" vs a wrong definition", **wrong)


def _true_keep(G, H=8, p=0.6):
    return D.attention_keep(T.GAT_DROP_SEEDS[p], np.arange(G.e), H, p)


def test_the_bound_refuses_a_mask_keyed_by_sorted_position(graphs):
    """The definition takes edge e's factor from its POSITION in the dst-sorted stream instead of its original id -- what every kernel
    of the engine could do alike without the engine's own tests noticing.  Refused on the classes graph; on the hub graph by the
    gradients alone (the forward is not compared there)."""
    for graph, forward in (("classes", True), ("classes", False), ("hub", False)):
        G = graphs[graph]
        position = np.empty(G.e, np.int64)
        position[np.argsort(G.dst_np, kind="stable")] = np.arange(G.e)
        wrong = D.attention_keep(T.GAT_DROP_SEEDS[0.6], position, 8, 0.6)
        assert ((wrong > 0) != (_true_keep(G) > 0)).mean() > 0.3
        _refused(G, graph, forward, keep=wrong)


def test_the_bound_refuses_one_mask_for_every_head(graphs):
    G = graphs["classes"]
    wrong = np.repeat(_true_keep(G)[:, :1], 8, axis=1)
    _refused(G, "classes", True, keep=wrong)
    _refused(G, "classes", False, keep=wrong)


def test_the_bound_refuses_an_unscaled_mask(graphs):
    """A factor of 1 instead of 1 / (1 - p)."""
    G = graphs["classes"]
    wrong = (_true_keep(G) > 0).astype(np.float32)
    _refused(G, "classes", True, keep=wrong)
    _refused(G, "classes", False, keep=wrong)


def test_the_bound_refuses_a_row_term_without_the_mask(graphs):
    """t[v, h] = sum_e alpha_e <g, f_u> without keep_e: the forward and d f are those of the right definition (and pass); each score
    gradient on its own refuses."""
    G = graphs["classes"]
    mutant = {"t_without_mask": True}
    T._gat_drop_case(G, "classes", 8, 16, 0.6, mutant=mutant, check=[0], what=" vs t without the mask: forward and d f")
    _refused(G, "classes", False, check=[1], mutant=mutant)
    _refused(G, "classes", False, check=[2], mutant=mutant)


# ------------------------------------------------------------------------------------------------
# d. the layer
# ------------------------------------------------------------------------------------------------
def _layer_keep(seed, e, heads, dk, p):
    """The keep factor GATConv's forward runs with (its docstring): heads go through the kernel in groups of `per` = the heads one
    launch of (padded) head width dk takes; group h0 uses seed + h0 and head indices restart at 0."""
    per = max(1, (64 * (4 if dk % 4 == 0 else 2 if dk % 2 == 0 else 1)) // dk)
    if heads <= per:
        return D.attention_keep(seed, np.arange(e), heads, p), 1
    groups = [D.attention_keep(seed + h0, np.arange(e), min(per, heads - h0), p) for h0 in range(0, heads, per)]
    return np.concatenate(groups, axis=1), len(groups)


@pytest.mark.parametrize("heads,dim,dk,concat,launches", [(4, 8, 8, True, 1), (8, 64, 64, True, 2), (3, 5, 8, True, 1), (4, 8, 8, False, 1)],
                         ids=["4x8", "8x64-in-groups-of-4", "3x5-padded-to-8", "4x8-head-mean"])
def test_gatconv_in_training_mode_is_the_definition_with_the_documented_seed(pgl, heads, dim, dk, concat, launches):
    """GATConv(...).train() with attn_drop = 0.6 against linear -> scores -> D.gat(keep=...) -> concat | head mean in fp64.  The seed:
    torch.manual_seed(s), read what the layer will draw, torch.manual_seed(s) again.  Tolerances: close_rows as
    tests/test_a13_f1_layers.py holds GATConv (5e-5 for the output, 2e-4 of the row for a gradient through the layer); the GEMMs are
    not under test here.  In eval mode: the p = 0 definition, and torch's generator is left alone."""
    n, e, din, p = 300, 3000, 32, 0.6
    edges, rng = rand_graph(n, e, 811)
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    src, dst = _t(edges[:, 0], torch.int64), _t(edges[:, 1], torch.int64)
    torch.manual_seed(5)
    layer = pgl.nn.GATConv(din, dim, feat_drop=0.0, attn_drop=p, num_heads=heads, concat=concat).cuda()
    x = _t(rng.standard_normal((n, din)))
    w = _t(rng.standard_normal((n, heads * dim if concat else dim)))

    def definition(keep):
        xd = x.detach().double().requires_grad_(True)
        feat = (xd @ layer.linear.weight.detach().double().t() + layer.linear.bias.detach().double()).reshape(n, heads, dim)
        a_s = (feat * layer.weight_src.detach().double()).sum(-1)
        a_d = (feat * layer.weight_dst.detach().double()).sum(-1)
        out = D.gat(feat, a_s, a_d, src, dst, 0.2, keep=keep)
        out = out.reshape(n, heads * dim) if concat else out.mean(1)
        (out * w.double()).sum().backward()
        return host(out), host(xd.grad)

    layer.train()
    s = 1000 + heads
    torch.manual_seed(s)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    keep, n_groups = _layer_keep(seed, e, heads, dk, p)
    assert n_groups == launches and keep.shape == (e, heads)
    torch.manual_seed(s)
    xg = x.detach().requires_grad_(True)
    out = layer(g, xg)
    (out * w).sum().backward()
    want, want_dx = definition(keep)
    close_rows(host(out), want, rtol=5e-5, what="GATConv %dx%d train: output" % (heads, dim))
    close_rows(host(xg.grad), want_dx, rtol=2e-4, atol_row=2e-4, what="GATConv %dx%d train: d x" % (heads, dim))
    # another seed is another mask (the comparison above is not vacuous)
    other, _ = definition(_layer_keep(seed + 1, e, heads, dk, p)[0])
    assert np.abs(other - want).max() > 1e-2 * np.abs(want).max()
    layer.eval()
    state = torch.get_rng_state()
    with torch.no_grad():
        got = layer(g, x)
    assert torch.equal(torch.get_rng_state(), state), "an eval forward drew from torch's generator"
    close_rows(host(got), definition(None)[0], rtol=5e-5, what="GATConv %dx%d eval: output" % (heads, dim))


# ------------------------------------------------------------------------------------------------
# e. out_size
# ------------------------------------------------------------------------------------------------
def _out_size_inputs(G, H=8, D_=16):
    rng = np.random.default_rng(83)
    a_s, a_d = lattice(rng, True, G.n, H), lattice(rng, False, G.n, H)
    return _t(rows(rng, G.n, H, D_)), _t(a_s), _t(a_d)


@pytest.mark.parametrize("p", [0.0, 0.6])
def test_gat_aggregate_out_size_beyond_the_rows_of_the_index(pgl, graphs, p):
    """out_size = n + 37: the first n rows are those of out_size = None bit for bit; the further rows of all five outputs (out, the
    two softmax statistics, the two positive-part statistics) are exactly 0 -- zero_fill_role's `r >= n_csr_rows`."""
    G = graphs["classes"]
    csr = G.g.adj_dst_index.csr
    f, a_s, a_d = _out_size_inputs(G)
    full = pgl.ops.gat_aggregate(f, a_s, a_d, csr, 0.2, None, True, p, 1234)
    more = pgl.ops.gat_aggregate(f, a_s, a_d, csr, 0.2, G.n + 37, True, p, 1234)
    assert len(full) == len(more) == 5 and all(t is not None for t in more)
    for name, a, b in zip(("out", "row_max", "row_sum", "out_pos", "sum_pos"), full, more):
        assert b.shape[0] == G.n + 37 and a.shape[0] == G.n, name
        assert torch.equal(b[:G.n], a), name + ": the rows of the index changed with out_size"
        assert bool((b[G.n:] == 0).all()), name + ": a row beyond the index is not 0"
    assert bool((full[0] != 0).any())


@pytest.mark.parametrize("p", [0.0, 0.6])
def test_gat_aggregate_out_size_below_the_rows_of_the_index(pgl, graphs, monkeypatch, p):
    """out_size = 3 on the classes graph, whose first five rows are the class rows: inside the cut lie a row the short fix-up pass
    finishes (row 0, 16 further pieces), an unsplit row and one the block-parallel pass finishes (row 2, 17 pieces); beyond it a
    short-pass row (row 3), the hub (row 4, the long pass) and every ordinary row -- `r >= out_rows` in store_final and in both
    passes of gat_fixup_kernel.  The 3 rows equal the first 3 of the full result bit for bit, and nothing is written behind them:
    every output is allocated with 8 more rows filled with NaN (the front end allocates its outputs itself, so torch.empty is
    wrapped for the call) and they are still all NaN afterwards."""
    G = graphs["classes"]
    M = 3
    assert T.further_pieces(G.dst_np, G.n)[:5].tolist() == [16, 0, 17, 1, 47]
    csr = G.g.adj_dst_index.csr
    f, a_s, a_d = _out_size_inputs(G)
    full = pgl.ops.gat_aggregate(f, a_s, a_d, csr, 0.2, None, True, p, 1234)
    torch.cuda.synchronize()
    real_empty, bands = torch.empty, []

    def guarded_empty(*size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        if kw.get("dtype") == torch.float32 and len(shape) >= 2 and shape[0] == M:
            big = real_empty((M + 8,) + shape[1:], **kw)
            big.fill_(float("nan"))
            bands.append(big)
            return big[:M]
        return real_empty(*size, **kw)

    monkeypatch.setattr(torch, "empty", guarded_empty)
    try:
        cut = pgl.ops.gat_aggregate(f, a_s, a_d, csr, 0.2, M, True, p, 1234)
    finally:
        monkeypatch.setattr(torch, "empty", real_empty)
    torch.cuda.synchronize()
    assert len(bands) == 5 and len(cut) == 5
    for name, a, b, band in zip(("out", "row_max", "row_sum", "out_pos", "sum_pos"), full, cut, bands):
        assert b.shape[0] == M and b.data_ptr() == band.data_ptr(), name
        assert torch.equal(b, a[:M]), name + ": the rows inside the cut differ from the full result"
        assert bool(torch.isnan(band[M:]).all()), name + ": written behind row out_size"
    assert bool((cut[0] != 0).all(dim=2).any())
