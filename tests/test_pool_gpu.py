"""The graph-pooling kernels on the MI355X (csrc/pool.hip) held bit for bit to their definitions (tests/pool_defs.py): the per-graph
top-k permutation over every segment length at which the code takes another path (empty, one element, around the wave size, the
wave tier's last length and the block tier's first, the cap), four flavours of scores, more segments than a launch has groups,
determinism and the status bits; the edge filter over every perm shape and every edge count around a tile, more tiles than a
launch has workgroups, a row-strided view and the two flags; and the public routing on top of them -- math.segment_topk,
filter_adj and SAGPool against today's tensor path of the same build, with the path that ran asserted every time."""
import numpy as np
import pytest
import torch

import pool_defs as D
from gpu_common import dev, host, pgl      # noqa: F401  (pgl: the module fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P(pgl):
    from pgl_amd import pool_ops
    return pool_ops


def _topk(P, scores, lens, k, status=None):
    seg_ptr, out_ptr = D.ptr(lens), D.ptr(k)
    before = P.LAUNCHES["topk_perm"]
    perm = P.topk_perm(dev(scores), dev(seg_ptr), dev(out_ptr), int(out_ptr[-1]), status=status)
    assert P.LAUNCHES["topk_perm"] == before + 1
    return host(perm)


def _k_modes(lens):
    return [np.zeros_like(lens), np.minimum(lens, 1), (lens + 1) // 2, lens]


@pytest.mark.parametrize("kind", D.FLAVOURS)
def test_topk_perm_equals_the_definition_at_every_path(P, kind):
    cap = P.TOPK_MAX_SEG
    lens = np.array([0, 1, 2, 63, 64, 65, 255, 256, 257, cap - 1, cap], np.int64)
    rng = np.random.default_rng(10)
    scores = D.score_flavour(kind, int(lens.sum()), rng)
    status = torch.zeros(1, dtype=torch.int64, device="cuda")
    for mode, k in enumerate(_k_modes(lens)):
        want = D.topk_perm_restated(scores, D.ptr(lens), D.ptr(k))
        assert np.array_equal(_topk(P, scores, lens, k, status), want), (kind, mode)
    k = rng.permutation(np.arange(len(lens))) % 4                   # every segment its own mode
    k = np.array([_k_modes(lens)[m][i] for i, m in enumerate(k)], np.int64)
    assert np.array_equal(_topk(P, scores, lens, k, status), D.topk_perm_restated(scores, D.ptr(lens), D.ptr(k)))
    P.topk_check(status)
    got, st = P.host_topk_perm(scores, D.ptr(lens), D.ptr(k))
    assert st == 0 and np.array_equal(got, D.topk_perm_restated(scores, D.ptr(lens), D.ptr(k)))


def test_topk_perm_more_segments_than_a_launch_has_groups(P):
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 4, 70000).astype(np.int64)
    scores = D.score_flavour("ties", int(lens.sum()), rng)
    k = np.minimum(lens, rng.integers(0, 4, len(lens)))
    want = D.topk_perm_restated(scores, D.ptr(lens), D.ptr(k))
    a, b = _topk(P, scores, lens, k), _topk(P, scores, lens, k)
    assert np.array_equal(a, want) and np.array_equal(a, b)


def test_topk_perm_twice_gives_the_same_bits(P):
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 700, 300).astype(np.int64)
    scores = D.score_flavour("special", int(lens.sum()), rng)
    k = (lens + 1) // 2
    a, b = _topk(P, scores, lens, k), _topk(P, scores, lens, k)
    assert np.array_equal(a, b) and np.array_equal(a, D.topk_perm_restated(scores, D.ptr(lens), D.ptr(k)))


def test_topk_perm_flags_a_segment_above_the_cap_and_a_k_above_its_segment(P):
    cap = P.TOPK_MAX_SEG
    rng = np.random.default_rng(13)
    lens = np.array([5, cap + 1, 300], np.int64)
    scores = rng.standard_normal(int(lens.sum())).astype(np.float32)
    status = torch.zeros(1, dtype=torch.int64, device="cuda")
    k = np.array([2, 3, 300], np.int64)
    got = _topk(P, scores, lens, k, status)
    with pytest.raises(ValueError, match="longer than %d" % cap):
        P.topk_check(status)
    assert int(status.item()) == 1
    want = D.topk_perm_restated(scores, D.ptr(lens), D.ptr(np.array([2, 0, 300])))
    assert np.array_equal(got[[0, 1] + list(range(5, 305))], want)  # the other segments are served; the flagged one is not written
    status.zero_()
    _topk(P, scores[:305], np.array([5, 300]), np.array([6, 1]), status)
    with pytest.raises(ValueError, match="k outside"):
        P.topk_check(status)
    assert int(status.item()) == 2
    with pytest.raises(ValueError):
        P.topk_perm(dev(scores).double(), dev(D.ptr(lens)), dev(D.ptr(k)), int(k.sum()))
    with pytest.raises(ValueError):
        P.topk_perm(dev(scores), dev(D.ptr(lens)).int(), dev(D.ptr(k)), int(k.sum()))
    with pytest.raises(ValueError):
        P.topk_perm(dev(scores), torch.as_tensor(D.ptr(lens)), dev(D.ptr(k)), int(k.sum()))


# ---- edge filter
N_NODES, N_EDGES = 3000, 20000


@pytest.fixture(scope="module")
def edges20k():
    rng = np.random.default_rng(20)
    e = rng.integers(0, N_NODES, (N_EDGES, 2)).astype(np.int64)
    e[:300, 1] = e[:300, 0]                                          # self-loops
    e[300:600] = e[600:900]                                          # multi-edges
    return e[rng.permutation(N_EDGES)]


def _perm(kind, rng):
    p = rng.permutation(N_NODES).astype(np.int64)
    return {"empty": p[:0], "one": p[:1], "30%": p[:900], "all": p}[kind]


def _filter(P, edges_t, perm, n):
    before = P.LAUNCHES["filter_edges"]
    out, pos = P.filter_edges(edges_t, dev(perm), n)
    assert P.LAUNCHES["filter_edges"] == before + 1
    return host(out), host(pos)


@pytest.mark.parametrize("kind", ["empty", "one", "30%", "all"])
def test_filter_edges_equals_the_definition(P, edges20k, kind):
    perm = _perm(kind, np.random.default_rng(21))
    full = dev(edges20k)
    for e in (0, 1, 1023, 1024, 1025, N_EDGES):
        got_e, got_p = _filter(P, full[:e], perm, N_NODES)
        want_e, want_p = D.filter_edges_restated(edges20k[:e], perm, N_NODES)
        assert got_e.shape == want_e.shape and np.array_equal(got_e, want_e) and np.array_equal(got_p, want_p), (kind, e)
    h_e, h_p, flags = P.host_filter_edges(edges20k, perm, N_NODES)
    got_e, got_p = _filter(P, full, perm, N_NODES)
    assert flags == 0 and np.array_equal(got_e, h_e) and np.array_equal(got_p, h_p)


def test_filter_edges_more_tiles_than_a_launch_has_workgroups(P, pgl):
    lanes = int(pgl._ffi.lib().pglamd_filter_edges_launch_threads())
    e = lanes * 4 + 1025                                             # tiles of 1024 positions by 256-lane workgroups: one more sweep
    rng = np.random.default_rng(22)
    edges = rng.integers(0, N_NODES, (e, 2)).astype(np.int64)
    perm = rng.permutation(N_NODES)[:900].astype(np.int64)
    got_e, got_p = _filter(P, dev(edges), perm, N_NODES)
    want_e, want_p = D.filter_edges_restated(edges, perm, N_NODES)
    assert np.array_equal(got_e, want_e) and np.array_equal(got_p, want_p)


def test_filter_edges_reads_a_row_strided_view_in_place(P, edges20k):
    wide = np.full((N_EDGES, 5), -7, np.int64)
    wide[:, 1:3] = edges20k
    view = dev(wide)[:, 1:3]
    assert view.stride(0) == 5 and not view.is_contiguous()
    perm = _perm("30%", np.random.default_rng(23))
    got_e, got_p = _filter(P, view, perm, N_NODES)
    want_e, want_p = D.filter_edges_restated(edges20k, perm, N_NODES)
    assert np.array_equal(got_e, want_e) and np.array_equal(got_p, want_p)


def test_filter_edges_names_its_flags(P, edges20k):
    full = dev(edges20k)
    perm = _perm("30%", np.random.default_rng(24))
    bad = perm.copy(); bad[17] = bad[400]
    with pytest.raises(ValueError, match="repeated id") as ei:
        P.filter_edges(full, dev(bad), N_NODES)
    assert ei.value.flags == 2
    for v in (N_NODES, -1, 2 ** 40):
        bad = perm.copy(); bad[17] = v
        with pytest.raises(ValueError, match="outside") as ei:
            P.filter_edges(full, dev(bad), N_NODES)
        assert ei.value.flags == 1
    with pytest.raises(ValueError, match="outside"):                # an edge end beyond the table: refused, not dereferenced
        P.filter_edges(full, dev(perm[perm < 2000]), 2000)
    torch.cuda.synchronize()
    got_e, _ = _filter(P, full, perm, N_NODES)                       # (the device is as it was)
    assert np.array_equal(got_e, D.filter_edges_restated(edges20k, perm, N_NODES)[0])


# ---- the public routing
def _batched(pgl, sizes, rng, feat_dim=6):
    graphs = []
    for m in sizes:
        e = rng.integers(0, m, (int(rng.integers(0, 4 * m + 1)), 2)).astype(np.int64)
        graphs.append(pgl.Graph(edges=e.reshape(-1, 2), num_nodes=int(m)))
    bg = pgl.Graph.disjoint(graphs).tensor()
    x = rng.standard_normal((int(np.sum(sizes)), feat_dim)).astype(np.float32)
    return bg, x


@pytest.mark.parametrize("ratio", [0.5, 0.3, 1.0, 3])
def test_segment_topk_on_the_gpu_equals_the_cpu_copy(pgl, P, ratio):
    rng = np.random.default_rng(30)
    lens = rng.integers(0, 91, 37).astype(np.int64); lens[-1] = 5
    scores = D.score_flavour("ties", int(lens.sum()), rng) + np.float32(0.5) * (rng.random(int(lens.sum())) < 0.3)
    gid = torch.as_tensor(np.repeat(np.arange(len(lens)), lens))
    x = torch.as_tensor(rng.standard_normal((int(lens.sum()), 3)).astype(np.float32))
    s = torch.as_tensor(scores.astype(np.float32))
    want_x, want_p = pgl.math.segment_topk(x, s, gid, ratio, return_index=True)
    assert P.topk_supported(int(lens.max()))
    for kw in ({}, {"num_segments": len(lens)}):
        before = P.LAUNCHES["topk_perm"]
        got_x, got_p = pgl.math.segment_topk(x.cuda(), s.cuda(), gid.cuda(), ratio, return_index=True, **kw)
        assert P.LAUNCHES["topk_perm"] == before + 1                 # the kernel ran
        assert torch.equal(got_p.cpu(), want_p) and torch.equal(got_x.cpu(), want_x)


def test_segment_topk_above_the_cap_keeps_todays_path(pgl, P):
    rng = np.random.default_rng(31)
    lens = np.array([40, P.TOPK_MAX_SEG + 1, 7], np.int64)
    assert not P.topk_supported(int(lens.max()))
    s = torch.as_tensor(rng.standard_normal(int(lens.sum())).astype(np.float32))
    gid = torch.as_tensor(np.repeat(np.arange(3), lens))
    x = s.reshape(-1, 1).clone()
    before = P.LAUNCHES["topk_perm"]
    _, got = pgl.math.segment_topk(x.cuda(), s.cuda(), gid.cuda(), 0.5, return_index=True)
    _, want = pgl.math.segment_topk(x, s, gid, 0.5, return_index=True)
    assert P.LAUNCHES["topk_perm"] == before and torch.equal(got.cpu(), want)
    keep = gid != 1                                                  # the short segments alone: the kernel again
    _, got = pgl.math.segment_topk(x[keep].cuda(), s[keep].cuda(), (gid[keep] // 2).cuda(), 1.0, return_index=True)
    _, want = pgl.math.segment_topk(x[keep], s[keep], gid[keep] // 2, 1.0, return_index=True)
    assert P.LAUNCHES["topk_perm"] == before + 1 and torch.equal(got.cpu(), want)


def test_filter_adj_on_the_gpu_equals_the_cpu_copy(pgl, P, edges20k):
    from pgl_amd.utils.transform import filter_adj
    perm = _perm("30%", np.random.default_rng(32))
    e, p = torch.as_tensor(edges20k), torch.as_tensor(perm)
    attr = torch.arange(N_EDGES, dtype=torch.float32).reshape(-1, 1) * 0.5
    want_e, want_a = filter_adj(e, p, attr, num_nodes=N_NODES)
    before = P.LAUNCHES["filter_edges"]
    got_e, got_a = filter_adj(e.cuda(), p.cuda(), attr.cuda(), num_nodes=N_NODES)
    assert P.LAUNCHES["filter_edges"] == before + 1
    assert torch.equal(got_e.cpu(), want_e) and torch.equal(got_a.cpu(), want_a)
    got_e, got_a = filter_adj(e.cuda(), p.cuda())                    # no node count: today's path
    assert P.LAUNCHES["filter_edges"] == before + 1 and torch.equal(got_e.cpu(), want_e) and got_a is None
    got_e, _ = filter_adj(e.cuda(), p.cuda(), num_nodes=100)         # a node count below the ids: flagged, today's path answers
    assert P.LAUNCHES["filter_edges"] == before + 2 and torch.equal(got_e.cpu(), want_e)


@pytest.mark.parametrize("ratio", [0.5, 3])
def test_sagpool_on_the_kernels_equals_todays_path(pgl, P, ratio, monkeypatch):
    rng = np.random.default_rng(33)
    sizes = rng.integers(1, 91, 37)
    bg, x_np = _batched(pgl, sizes, rng)
    assert P.topk_supported(int(sizes.max()))
    torch.manual_seed(5)
    layer = pgl.nn.SAGPool(6, ratio).cuda()
    cot = torch.as_tensor(rng.standard_normal((int(P.topk_counts(sizes, ratio).sum()), 6)).astype(np.float32)).cuda()
    res = {}
    for device_pool in (False, True):
        monkeypatch.setattr(P, "_ROUTE", device_pool)                # False: today's tensor code in SAGPool, math and filter_adj
        layer.zero_grad()
        x = torch.as_tensor(x_np).cuda().requires_grad_(True)
        before = (P.LAUNCHES["topk_perm"], P.LAUNCHES["filter_edges"])
        px, batch, g = layer(bg, x)
        after = (P.LAUNCHES["topk_perm"], P.LAUNCHES["filter_edges"])
        assert after == (before[0] + device_pool, before[1] + device_pool)
        (px * cot).sum().backward()
        res[device_pool] = (px.detach(), batch, g.edges, np.asarray(g._graph_node_index), g.num_graph, g.num_nodes, x.grad.clone(),
                            [p.grad.clone() for p in layer.parameters()])
    a, b = res[False], res[True]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].dtype == b[1].dtype
    assert torch.equal(a[2], b[2]) and a[2].dtype == b[2].dtype
    assert np.array_equal(a[3], b[3]) and a[3].dtype == b[3].dtype and a[4] == b[4] and a[5] == b[5]
    # gradients: the same autograd nodes run on both paths (the kernels are index work), so bit for bit
    assert torch.equal(a[6], b[6]) and len(a[7]) == len(b[7]) and all(torch.equal(u, v) for u, v in zip(a[7], b[7]))
    assert len(a[7]) >= 1 and all(bool(v.abs().sum() > 0) for v in b[7][:1])
    # and against the definition: the pooled nodes are each graph's top k by the layer's own score
    score = torch.tanh(layer.gnn(bg, torch.as_tensor(x_np).cuda()).reshape(-1)).detach()
    k = P.topk_counts(sizes, ratio)
    rank = D.topk_perm_restated(host(score), D.ptr(sizes), D.ptr(k))
    assert np.array_equal(host(b[1]), np.repeat(np.arange(len(sizes)), k)) and np.array_equal(b[3], D.ptr(k))
    assert np.array_equal(host(b[2]), D.filter_edges_restated(host(bg.edges), rank, int(sizes.sum()))[0])


def test_sagpool_with_a_graph_above_the_cap_keeps_todays_topk(pgl, P):
    """A member graph above the cap: no host plan, the top-k is today's tensor code (the edge filter still has its kernel)."""
    rng = np.random.default_rng(34)
    sizes = np.array([3, P.TOPK_MAX_SEG + 1, 9])
    bg, x_np = _batched(pgl, sizes, rng)
    layer = pgl.nn.SAGPool(6, 0.5).cuda()
    assert layer._host_plan(bg, torch.as_tensor(x_np).cuda()) is None
    before = P.LAUNCHES["topk_perm"]
    px, batch, g = layer(bg, torch.as_tensor(x_np).cuda())
    assert P.LAUNCHES["topk_perm"] == before
    k = P.topk_counts(sizes, 0.5)
    assert np.array_equal(np.asarray(g._graph_node_index), D.ptr(k)) and int(px.shape[0]) == int(k.sum())
    score = torch.tanh(layer.gnn(bg, torch.as_tensor(x_np).cuda()).reshape(-1)).detach()
    assert np.array_equal(np.sort(host(batch)), np.repeat(np.arange(3), k))
    rank = D.topk_perm_restated(host(score), D.ptr(sizes), D.ptr(k))
    assert np.array_equal(host(g.edges), D.filter_edges_restated(host(bg.edges), rank, int(sizes.sum()))[0])


@pytest.mark.parametrize("where", ["numpy", "cpu tensor"])
def test_sagpool_takes_the_node_index_as_the_reference_unit_test_builds_it(pgl, P, where):
    """The reference's own test_sag_pool hands Graph a tensor as _graph_node_index: the host plan reads it like an array."""
    x = torch.randn(8, 4, device="cuda")
    edges = torch.tensor([[0, 1, 2, 3, 4, 5, 5, 6, 6, 7], [1, 0, 3, 4, 2, 6, 7, 7, 5, 6]]).t().contiguous().cuda()
    index = {"numpy": np.array([0, 2, 5, 8]), "cpu tensor": torch.tensor([0, 2, 5, 8])}[where]
    g = pgl.Graph(num_nodes=8, edges=edges, node_feat={"attr": x}, _graph_node_index=index, _num_graph=3).tensor()
    torch.manual_seed(1)
    layer = pgl.nn.SAGPool(4, 0.5, pgl.nn.GCNConv).cuda()
    assert layer._host_plan(g, x) is not None
    out, batch, pg = layer(g, x)
    assert out.shape[0] == 1 + 2 + 2 and pg.num_graph == 3 and pg.edges.shape[1] == 2 and host(batch).tolist() == [0, 1, 1, 2, 2]
    assert np.array_equal(np.asarray(pg._graph_node_index), [0, 1, 3, 5])
