"""The sliced aggregation (ops.slice_plan + pglamd_aggregate_sliced): the hub edges of long rows summed as eight per-XCD virtual rows
in the same launch as the rest of the stream, then added to the row in a fixed order.  Every result is held to the project's fp64
re-association bound (check_aggregate); the thresholds are lowered so that small graphs take the path."""
import numpy as np
import pytest
import torch

from gpu_common import *                        # noqa: F401,F403
import hub_slice_defs as H

pytestmark = pytest.mark.gpu

L = 32


@pytest.fixture()
def sliced(pgl, monkeypatch):
    ops = pgl.ops
    monkeypatch.setattr(ops, "_HUB_TABLE", True)
    monkeypatch.setattr(ops, "_HUB_SLICES", True)
    monkeypatch.setattr(ops, "_SLICE_MIN_EDGES", 0)
    monkeypatch.setattr(ops, "_HUB_MIN_EDGES", 0)
    monkeypatch.setattr(ops, "_SLICE_ROW_MIN", L)
    return ops


@pytest.fixture(scope="module")
def rmat14(pgl):
    from pgl_amd.utils.rmat import rmat_edges
    n = 1 << 14
    edges = rmat_edges(14, 400_000, seed=3, device=torch.device("cuda"))
    g = pgl.Graph(edges=edges, num_nodes=n)
    e = host(edges)
    return g, n, np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])


def _plans(csr):
    return [p for p in (csr._slices or {}).values() if p is not None]


@pytest.mark.parametrize("d,extra", [(96, 0), (128, 0), (256, 0), (128, 100)])
def test_rmat14_sum_within_the_fp64_bound_and_repeatable(sliced, rmat14, d, extra):
    g, n, src, dst = rmat14
    assert int(np.bincount(dst).max()) > 4 * 64                                  # the top row's virtual rows exceed one chunk
    gen = torch.Generator(device="cuda"); gen.manual_seed(d + extra)
    x = torch.randn(n, d, generator=gen, device="cuda")
    csr = g.adj_dst_index.csr
    got = sliced.aggregate(x, csr, "sum", n + extra)
    plans = [p for p in _plans(csr) if p.out_rows == n + extra]
    assert len(plans) == 1 and plans[0].row_min == L and plans[0].n_long >= 64     # the sliced path ran
    assert plans[0].seg_edges[1] < csr.num_edges
    check_aggregate(host(got), host(x), src, dst, "sum", out_size=n + extra, what="sliced d=%d" % d)
    assert torch.equal(got, sliced.aggregate(x, csr, "sum", n + extra))


def test_send_recv_forward_and_backward(sliced, rmat14):
    g, n, src, dst = rmat14
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    x = torch.randn(n, 128, generator=gen, device="cuda").requires_grad_(True)
    w = torch.randn(n, 128, generator=gen, device="cuda")
    out = g.send_recv(x, "sum")
    check_aggregate(host(out), host(x), src, dst, "sum", what="send_recv forward")
    out.backward(w)
    assert _plans(g.adj_dst_index.csr) and _plans(g.adj_src_index.csr)            # both walks were sliced
    check_aggregate(host(x.grad), host(w), dst, src, "sum", what="send_recv backward")   # d x = the transposed aggregation of w
    x2 = x.detach().clone().requires_grad_(True)
    g.send_recv(x2, "sum").backward(w)
    assert torch.equal(x2.grad, x.grad)


def test_hand_built_rows_and_special_values(sliced, pgl):
    n, src, dst = H.hand_graph()
    deg = np.bincount(dst, minlength=n)
    assert deg[2012] == L and deg[2013] == L + 1 and deg[0] == 0
    assert np.bincount(src, minlength=n)[1024:].max() < 24
    g = pgl.Graph(edges=np.stack([src, dst], 1), num_nodes=n).tensor()
    csr = g.adj_dst_index.csr
    rng = np.random.default_rng(6)
    x = rng.standard_normal((n, 128)).astype(np.float32)
    got = sliced.aggregate(dev(x), csr, "sum", n)
    (p,) = _plans(csr)
    hub = next(iter(csr._hub.values()))
    assert np.array_equal(host(hub[0]), np.arange(1024))                          # rank == id
    rows = set(host(p.long_rows).tolist())
    assert 2013 in rows and 2012 not in rows and 2010 in rows and 2011 in rows and p.n_long == 103
    ip, R = host(p.indptr), p.n_long
    i10, i11 = sorted(rows).index(2010), sorted(rows).index(2011)
    assert ip[2011] - ip[2010] == 0                                               # row 2010: nothing left in the rest stream
    assert all(ip[n + s * R + i11 + 1] - ip[n + s * R + i11] == 0 for s in range(8))      # row 2011: eight empty virtual rows
    assert sum(ip[n + s * R + i10 + 1] - ip[n + s * R + i10] for s in range(8)) == 50
    assert p.seg_edges[8] == p.seg_edges[9] and p.seg_edges[7] < p.seg_edges[8]   # slice 7 has no edge at all
    check_aggregate(host(got), x, src, dst, "sum", what="hand-built graph")
    assert torch.equal(got, sliced.aggregate(dev(x), csr, "sum", n))
    assert float(got[deg == 0].abs().max()) == 0.0
    # NaN in one hub row, +inf in one cold row: where they show is what the plain path says
    xs = x.copy(); xs[5] = np.nan; xs[int(src[(src >= 1024) & (dst == 2190)][0])] = np.inf      # (hub 5 feeds rows 2137..2160, not 2190)
    got = sliced.aggregate(dev(xs), csr, "sum", n)
    setattr(sliced, "_HUB_SLICES", False)                                          # (the fixture's monkeypatch restores it)
    plain = sliced.aggregate(dev(xs), csr, "sum", n)
    assert int(torch.isnan(plain).sum()) > 0 and int(torch.isinf(plain).sum()) > 0
    assert torch.equal(torch.isnan(got), torch.isnan(plain)) and torch.equal(torch.isinf(got), torch.isinf(plain))
    assert torch.equal(torch.isnan(got[2010]), torch.isnan(plain[2010]))


def test_plan_declines_without_hubs_and_when_switched_off(sliced, rmat14, pgl):
    n = 1 << 16
    rng = np.random.default_rng(0)
    flat = np.stack([rng.permutation(n).repeat(8)[:400000], rng.integers(0, n, 400000)], 1).astype(np.int64)
    gu = pgl.Graph(edges=flat, num_nodes=n).tensor()
    cu = gu.adj_dst_index.csr
    x = torch.randn(n, 128, device="cuda")
    got = sliced.aggregate(x, cu, "sum", n)
    assert next(iter(cu._hub.values())) is None and not _plans(cu)                # no hub plan: no slices, the plain path
    check_aggregate(host(got), host(x), flat[:, 0], flat[:, 1], "sum", what="hub-less graph")
    # switched off (PGLAMD_HUB_SLICES=0): the hub-table path, no plan is built
    g, n14, src, dst = rmat14
    c = g.adj_dst_index.csr.view()
    x = torch.randn(n14, 128, device="cuda")
    setattr(sliced, "_HUB_SLICES", False)
    off = sliced.aggregate(x, c, "sum", n14)
    assert c._slices is None and next(iter(c._hub.values())) is not None
    setattr(sliced, "_HUB_TABLE", False)
    assert torch.equal(off, sliced.aggregate(x, c.view(), "sum", n14))            # ... which is bit-identical to the plain library


# ------------------------------------------------------------------------------------------------------------------------------------
# Branch by branch.  The chunk is injected through ops._flat_chunk (the plan carries it to the launch; the library latches PGLAMD_CHUNK
# for the life of the process), each case works on a fresh csr.view() (the plan cache key does not hold the chunk), and `launches`
# records which entry points a call reached.  Apart from check_aggregate's fp64 bound every comparison is exact.
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def launches(sliced, monkeypatch):
    names, real = [], sliced._launch

    def recording(name, on, *args, **kw):
        names.append(name)
        return real(name, on, *args, **kw)
    monkeypatch.setattr(sliced, "_launch", recording)
    return names


def _set_chunk(monkeypatch, ops, chunk):
    monkeypatch.setattr(ops, "_flat_chunk", lambda num_edges: chunk)


@pytest.fixture(scope="module")
def built(pgl):
    """name -> (index, n, src, dst): every graph of hub_slice_defs on the device, built once; tests take .view()s of the index."""
    out = {}
    for name, make in H.BUILDERS.items():
        n, src, dst = make()
        g = pgl.Graph(edges=np.stack([src, dst], 1), num_nodes=n).tensor()
        out[name] = (g.adj_dst_index.csr, n, src, dst)
    return out


@pytest.fixture(scope="module")
def graphs(built, pgl):
    n, src, dst = H.rmat14()                           # (the CPU generator's edges: what test_hub_slice_defs.py counted)
    g = pgl.Graph(edges=np.stack([src, dst], 1), num_nodes=n).tensor()
    return dict(built, rmat14=(g.adj_dst_index.csr, n, src, dst))


_REF = {}


def _normal(graphs, name, d):
    """(x on the device, x on the host, fp64 sum, check_aggregate's bound) for standard-normal features of width d on graph `name`:
    computed once per module and shared, never written to."""
    key = (name, d)
    if key not in _REF:
        _, n, src, dst = graphs[name]
        x = np.random.default_rng(1000 + d).standard_normal((n, d)).astype(np.float32)
        want64, absx, n_terms = fp64_terms(x, src, dst, "sum")
        _REF[key] = (dev(x), x, want64, reassociation_bound(absx, n_terms))          # (slack 4.0, fp32 eps: check_aggregate's defaults)
    return _REF[key]


def _check_sum(got, ref, what):
    """check_aggregate(got, x, src, dst, "sum") with the fp64 terms of the shared x computed once: the same reference, the same bound."""
    want64, bound = ref[2], ref[3]
    g = host(got)
    assert g.shape == want64.shape
    _assert_elementwise(np.abs(g.astype(np.float64) - want64), bound, want64, what + " vs fp64")


def _ints(graphs, name, d):
    key = (name, d, "int")
    if key not in _REF:
        _, n, src, dst = graphs[name]
        assert int(np.bincount(dst).max()) * 8 < (1 << 24)                          # every partial sum is an integer below 2^24: exact in fp32
        x = H.small_int_features(n, d, 2000 + d)
        _REF[key] = (dev(x), H.exact_sum(x, src, dst, n))
    return _REF[key]


def _run(ops, launches, x, csr, out_rows, **kw):
    """One aggregate() that must take the sliced entry point -> (result, its plan)."""
    del launches[:]
    got = ops.aggregate(x, csr, "sum", out_rows, **kw)
    assert launches == ["aggregate_sliced"], launches
    (p,) = [p for p in _plans(csr) if p.out_rows == out_rows]
    return got, p


# every d at chunk 8 (both fix-up roles on virtual rows), every chunk at d = 128 / 256, the production threshold with chunk 256
_MATRIX = [(8, d, 32) for d in (96, 98, 100, 126, 128, 132, 252, 256)] + [(c, d, 32) for c in (64, 128, 256) for d in (128, 256)] + \
          [(256, d, 128) for d in (100, 128, 252, 256)] + [(128, 128, 128)]


@pytest.mark.parametrize("chunk,d,row_min", _MATRIX)
def test_rmat14_chunk_width_and_threshold_matrix(sliced, launches, monkeypatch, graphs, chunk, d, row_min):
    csr0, n, src, dst = graphs["rmat14"]
    monkeypatch.setattr(sliced, "_SLICE_ROW_MIN", row_min)
    _set_chunk(monkeypatch, sliced, chunk)
    ref = _normal(graphs, "rmat14", d)
    csr = csr0.view()
    got, p = _run(sliced, launches, ref[0], csr, n)
    assert p.chunk == chunk and p.row_min == row_min and p.n_long >= 64 and 0 < p.seg_edges[1] < csr.num_edges
    assert p.n_long == (470 if row_min == 128 else 1751)
    f = H.plan_facts(p)
    if chunk == 8:                                    # the long AND the short fix-up role run on virtual rows and on remainder rows
        assert f["virtual_long"] > 0 and f["virtual_short"] > 0 and f["rest_long"] > 0 and f["rest_short"] > 0
        assert f["virtual_chunks"] > H.FIX_SHORT + 1
    else:
        assert f["virtual_short"] > 0 and f["rest_short"] > 0
    _check_sum(got, ref, "rmat14 chunk=%d d=%d row_min=%d" % (chunk, d, row_min))
    assert torch.equal(got, _run(sliced, launches, ref[0], csr, n)[0])


@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("chunk", [8, 256])
@pytest.mark.parametrize("name", ["all_hub", "one_slice3", "tiny", "mixed_long", "hand_graph", "rmat14"])
def test_integer_features_sum_exactly(sliced, launches, monkeypatch, graphs, name, chunk, d):
    """No edge dropped, none doubled: with integer-valued fp32 inputs every association gives the fp64 sum bit for bit."""
    csr0, n, src, dst = graphs[name]
    _set_chunk(monkeypatch, sliced, chunk)
    x, want = _ints(graphs, name, d)
    got, p = _run(sliced, launches, x, csr0.view(), n)
    assert p.chunk == chunk
    assert np.array_equal(host(got), want)


@pytest.mark.parametrize("d", [128, 252])
@pytest.mark.parametrize("name", ["mixed_long", "all_hub", "one_slice3"])
def test_every_row_of_a_nan_filled_out_is_written(sliced, launches, monkeypatch, graphs, name, d):
    csr0, n, src, dst = graphs[name]
    _set_chunk(monkeypatch, sliced, 64)
    out_rows = n + 100
    x, _ = _ints(graphs, name, 256)
    x = x[:, :d].contiguous()
    out = torch.full((out_rows, d), float("nan"), device="cuda")
    csr = csr0.view()
    first = _run(sliced, launches, x, csr, out_rows, out=out)[0].clone()
    # again with NaN in every float of the (now existing) workspace as well: what a call leaves in it is nobody's business, and an
    # empty virtual row that is not zero-filled behind the partial rows now shows as NaN in its long row
    assert len(sliced._WS_HOT) >= 1
    for buf in sliced._WS_HOT.values():
        buf.fill_(0xFF)
    out.fill_(float("nan"))
    got, p = _run(sliced, launches, x, csr, out_rows, out=out)
    assert got is out and p.out_rows == out_rows and torch.equal(got, first)
    f = H.plan_facts(p)
    deg = np.bincount(dst, minlength=out_rows)
    if name == "all_hub":
        assert int((deg == 0).sum()) == 8128 + 100 and p.seg_edges[1] == 0
    if name == "one_slice3":
        assert f["empty_virtual"] == 7 * 64
    if name == "mixed_long":
        assert f["empty_virtual"] >= 15 and int((deg[:n] == 0).sum()) > 0
    g = host(got)
    assert not np.isnan(g).any()
    assert not g[deg == 0].any()                                                   # rows without edges, and rows n .. out_rows - 1: exactly 0
    assert np.array_equal(g, H.exact_sum(host(x), src, dst, out_rows))


@pytest.mark.parametrize("name,chunk", [("all_hub", 64), ("all_hub", 256), ("one_slice3", 64), ("one_slice6", 64), ("one_slice6", 256),
                                        ("tiny", 256), ("tiny", 8)])
def test_degenerate_block_tables(sliced, launches, monkeypatch, graphs, name, chunk):
    csr0, n, src, dst = graphs[name]
    _set_chunk(monkeypatch, sliced, chunk)
    ref = _normal(graphs, name, 128)
    got, p = _run(sliced, launches, ref[0], csr0.view(), n)
    count = p.blocks[9:]
    if name == "all_hub":
        assert count[0] == 0 and all(c > 0 for c in count[1:])                     # an empty rest stream
    elif name.startswith("one_slice"):
        assert [c > 0 for c in count[1:]] == [s == int(name[-1]) for s in range(8)]    # one slice with blocks, seven without
    elif chunk == 256:
        assert p.blocks == [0, 0, 1, 1, 1, 2, 2, 2, 2, 0, 1, 0, 0, 1, 0, 0, 0, 1]      # 3 blocks for 8 XCDs, five slices own none
    _check_sum(got, ref, "%s chunk=%d" % (name, chunk))
    xi, want = _ints(graphs, name, 128)
    assert np.array_equal(host(_run(sliced, launches, xi, csr0.view(), n)[0]), want)


def _offset_view(t, elems):
    """A contiguous copy of t that starts `elems` elements into its (512-byte aligned) storage."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (elems * t.element_size()) % 16
    return v


_FALLBACKS = ["d130", "d258", "d260", "x+4", "x+8", "out+4 d128", "out+8 d256", "accumulate1", "accumulate2", "dst_scale", "mean", "max", "min"]


@pytest.mark.parametrize("case", _FALLBACKS)
def test_ineligible_inputs_fall_back_and_do_not_raise(sliced, launches, monkeypatch, graphs, case):
    csr0, n, src, dst = graphs["mixed_long"]
    _set_chunk(monkeypatch, sliced, 64)
    d = int(case[1:]) if case[0] == "d" and case[1:].isdigit() else 256 if case.endswith("d256") else 128
    x = torch.randn(n, d, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    kw, op = {}, "sum"
    if case.startswith("x+"):
        x = _offset_view(x, int(case[2:]) // 4)
    if case in ("mean", "max", "min"):
        op = case
    if case == "dst_scale":
        kw["dst_scale"] = torch.rand(n, device="cuda") + 0.5
    base = torch.randn(n, d, generator=torch.Generator(device="cuda").manual_seed(6), device="cuda")

    def call(csr):
        k = dict(kw)
        if case.startswith("out+"):
            k["out"] = _offset_view(base, int(case[4]) // 4)
        if case.startswith("accumulate"):
            k.update(out=base.clone(), accumulate=int(case[-1]))
        return sliced.aggregate(x, csr, op, n, **k)

    # the same input is eligible apart from the one thing the case changes: a plain call on this graph is sliced
    _run(sliced, launches, torch.randn(n, 128, device="cuda"), csr0.view(), n)
    csr = csr0.view()
    del launches[:]
    got = call(csr)
    assert "aggregate_sliced" not in launches and "aggregate_ext" in launches      # the hub-table path served it
    assert not _plans(csr)                                                         # ... and no slice plan was built for it
    monkeypatch.setattr(sliced, "_HUB_SLICES", False)
    assert torch.equal(got, call(csr0.view()))


def _special_rows(n, src, dst, poisoned):
    """Rows that receive one of the `poisoned` sources."""
    hit = np.zeros(n, bool)
    hit[dst[np.isin(src, poisoned)]] = True
    return hit


@pytest.mark.parametrize("chunk", [8, 64])
@pytest.mark.parametrize("case", ["two slices", "slice and remainder", "nan in the remainder"])
def test_special_values_meet_in_the_combine_step(sliced, launches, monkeypatch, graphs, case, chunk):
    csr0, n, src, dst = graphs["mixed_long"]
    _set_chunk(monkeypatch, sliced, chunk)
    r = dst == 2150
    hub_of = lambda res: int(src[r & (src < H.HUBS) & (src % 8 == res)][0])
    cold = int(src[r & (src >= H.HUBS) & (src != 2150)][0])
    x = _normal(graphs, "mixed_long", 128)[1].copy()
    if case == "two slices":                           # +inf and -inf reach row 2150 through two different slices
        a, b = hub_of(1), hub_of(2)
        x[a], x[b] = np.inf, -np.inf
    elif case == "slice and remainder":                # +inf through a slice, -inf through the row's own remainder
        a, b = hub_of(4), cold
        x[a], x[b] = np.inf, -np.inf
    else:
        a = b = cold
        x[a] = np.nan
    csr = csr0.view()
    got, p = _run(sliced, launches, dev(x), csr, n)
    assert np.array_equal(host(next(iter(csr._hub.values()))[0]), np.arange(H.HUBS))          # rank == id: the residues are the slices
    assert 2150 in host(p.long_rows).tolist()
    monkeypatch.setattr(sliced, "_HUB_SLICES", False)
    plain = sliced.aggregate(dev(x), csr0.view(), "sum", n)
    assert bool(torch.isnan(plain[2150]).all())                                    # inf - inf, or the NaN itself
    assert torch.equal(torch.isnan(got), torch.isnan(plain)) and torch.equal(torch.isinf(got), torch.isinf(plain))
    pos = got == float("inf")
    assert torch.equal(pos, plain == float("inf"))                                 # (the sign of an infinity as well)
    clean = ~_special_rows(n, src, dst, [a, b])
    assert clean.sum() > n // 2 and np.isfinite(host(got)[clean]).all()


def test_workspace_is_reused_across_widths_chunks_and_graphs(sliced, launches, monkeypatch, graphs):
    steps = [("rmat14", 256, 8), ("tiny", 96, 256), ("rmat14", 256, 8), ("all_hub", 128, 64)]
    idx, first = {}, {}
    for name, d, chunk in steps:                       # every configuration first on a fresh workspace
        if (name, d, chunk) in first:
            continue
        _set_chunk(monkeypatch, sliced, chunk)
        idx[name, d, chunk] = graphs[name][0].view()
        sliced.release_workspaces()
        got, p = _run(sliced, launches, _normal(graphs, name, d)[0], idx[name, d, chunk], graphs[name][1])
        assert p.chunk == chunk
        _check_sum(got, _normal(graphs, name, d), "%s d=%d chunk=%d" % (name, d, chunk))
        first[name, d, chunk] = got
    sliced.release_workspaces()
    for name, d, chunk in steps:                       # then one after the other on ONE workspace that only grows
        got, p = _run(sliced, launches, _normal(graphs, name, d)[0], idx[name, d, chunk], graphs[name][1])
        assert p.chunk == chunk and torch.equal(got, first[name, d, chunk]), (name, d, chunk)
    assert len(sliced._WS_HOT) == 1


def _capture(fn):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def test_graph_capture_replays_a_cached_plan(sliced, launches, monkeypatch, graphs):
    csr0, n, src, dst = graphs["rmat14"]
    _set_chunk(monkeypatch, sliced, 64)
    csr = csr0.view()
    x = _normal(graphs, "rmat14", 128)[0].clone()
    x2 = torch.randn(n, 128, generator=torch.Generator(device="cuda").manual_seed(9), device="cuda")
    o = torch.empty(n, 128, device="cuda")
    want2, p = _run(sliced, launches, x2, csr, n)                                  # eager: the plan and the workspace exist
    _run(sliced, launches, x, csr, n, out=o)
    torch.cuda.synchronize()
    del launches[:]
    graph = _capture(lambda: sliced.aggregate(x, csr, "sum", n, out=o))
    assert launches == ["aggregate_sliced"] and len(_plans(csr)) == 1 and _plans(csr)[0] is p
    x.copy_(x2)
    o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, want2)


@pytest.mark.parametrize("hub_plan_cached", [False, True])
def test_graph_capture_without_a_cached_plan_builds_none(sliced, launches, monkeypatch, graphs, hub_plan_cached):
    csr0, n, src, dst = graphs["rmat14"]
    _set_chunk(monkeypatch, sliced, 64)
    ref = _normal(graphs, "rmat14", 128)
    x, o = ref[0], torch.empty(n, 128, device="cuda")
    warm = csr0.view()
    _run(sliced, launches, x, warm, n)                                             # eager first: every route's kernels have run once
    monkeypatch.setattr(sliced, "_HUB_SLICES", False)
    sliced.aggregate(x, csr0.view(), "sum", n)
    monkeypatch.setattr(sliced, "_HUB_TABLE", False)
    sliced.aggregate(x, csr0.view(), "sum", n)
    monkeypatch.setattr(sliced, "_HUB_SLICES", True)
    monkeypatch.setattr(sliced, "_HUB_TABLE", True)
    torch.cuda.synchronize()
    c = csr0.view()
    if hub_plan_cached:                                # the call reaches slice_plan, which must decline: building a plan reads the host
        c._hub = dict(warm._hub)
    del launches[:]
    graph = _capture(lambda: sliced.aggregate(x, c, "sum", n, out=o))
    assert not c._slices and "aggregate_sliced" not in launches
    assert ("aggregate_ext" in launches) == hub_plan_cached                        # hub table where its plan was cached, else the plain entry
    o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _check_sum(o, ref, "captured without a plan")


def _sliced_call(ops, x, sp, out, ws, ws_bytes=None, **change):
    """pglamd_aggregate_sliced through ops._launch as ops._aggregate_sliced calls it, with the named arguments replaced."""
    import ctypes
    a = dict(n_x=int(x.shape[0]), d=int(x.shape[1]), n_hubs=int(sp.hub_ids.shape[0]), E=int(sp.row32.shape[0]), out_rows=sp.out_rows,
             n_long=sp.n_long, blocks=list(sp.blocks), chunk=sp.chunk, ws_bytes=ws.numel() if ws_bytes is None else ws_bytes)
    a.update(change)
    blocks = (ctypes.c_int32 * 18)(*a["blocks"])
    p = ops._ptr
    ops._launch("aggregate_sliced", x, p(x), a["n_x"], a["d"], p(sp.hub_ids), a["n_hubs"], p(sp.row32), p(sp.col32), p(sp.indptr), a["E"],
                a["out_rows"], p(sp.long_rows), a["n_long"], ctypes.cast(blocks, ctypes.c_void_p), p(sp.blocks_dev), a["chunk"], p(out),
                p(ws), a["ws_bytes"])


_REFUSALS = {"chunk 12": ValueError, "d 130": ValueError, "block table": ValueError, "workspace": RuntimeError, "n_long 0": OverflowError,
             "out + 4 bytes": ValueError}


@pytest.mark.parametrize("case", sorted(_REFUSALS))
def test_the_entry_point_refuses_bad_arguments_before_any_launch(sliced, launches, monkeypatch, graphs, pgl, case):
    """Argument checks that return before the first launch: every pointer stays valid and every buffer is as large as the largest
    reading of the arguments needs, so nothing here could reach a kernel with bad data."""
    csr0, n, src, dst = graphs["all_hub"]
    _set_chunk(monkeypatch, sliced, 64)
    d = 130 if case == "d 130" else 128
    _, sp = _run(sliced, launches, torch.zeros(n, 128, device="cuda"), csr0.view(), n)
    x = torch.zeros(n, d, device="cuda")
    out = torch.full((n * d + 16,), float("nan"), device="cuda")
    need = pgl._ffi.lib().pglamd_aggregate_sliced_workspace_bytes(sp.row32.shape[0], d, sp.hub_ids.shape[0], sp.n_long, 8)   # (chunk 8: the largest)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    asked = pgl._ffi.lib().pglamd_aggregate_sliced_workspace_bytes(sp.row32.shape[0], d, sp.hub_ids.shape[0], sp.n_long, sp.chunk)
    o = out[:n * d].view(n, d)
    change = {}
    if case == "chunk 12":
        change = dict(chunk=12)
    elif case == "block table":
        bad = list(sp.blocks)
        bad[9 + 4] += 1
        change = dict(blocks=bad)
    elif case == "workspace":
        change = dict(ws_bytes=asked - 1)
    elif case == "n_long 0":
        change = dict(n_long=0)
    elif case == "out + 4 bytes":
        o = out[1:1 + n * d].view(n, d)
    with pytest.raises(_REFUSALS[case]) as e:
        _sliced_call(sliced, x, sp, o, ws, **change)
    assert "aggregate_sliced" in str(e.value)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                            # refused before anything was launched
    if case == "workspace":                            # ... and exactly what it asked for is enough
        _sliced_call(sliced, x, sp, o, ws, ws_bytes=asked)
        torch.cuda.synchronize()
        assert not bool(o.any()) and bool(torch.isnan(out[n * d:]).all())          # x = 0: every row written, all zeros
