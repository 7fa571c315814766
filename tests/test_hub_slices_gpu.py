"""The sliced aggregation (ops.slice_plan + pglamd_aggregate_sliced): the hub edges of long rows summed as eight per-XCD virtual rows
in the same launch as the rest of the stream, then added to the row in a fixed order.  Every result is held to the project's fp64
re-association bound (check_aggregate); the thresholds are lowered so that small graphs take the path."""
import numpy as np
import pytest
import torch

from gpu_common import *                        # noqa: F401,F403

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


def _hand_graph():
    """8192 nodes; sources 0..1023 all have 24 out-edges (more than any other source), so hub rank == source id.
    rows 2100..2199: ~210 hub edges + 10 cold edges each            row 2010: hub edges only (its rest row is empty)
    row 2011: 50 cold edges (eight empty virtual rows)                row 2012: exactly L edges, row 2013: L + 1
    hubs with id % 8 == 7 send to short rows only (slice 7 has no edge); duplicate edges, self loops and rows without edges."""
    n = 8192
    rng = np.random.default_rng(5)
    slots = np.repeat(np.array([i for i in range(1024) if i % 8 != 7]), 24)      # hub id of every hub -> long-row edge
    dst = np.empty(len(slots), np.int64)
    dst[:16] = 2012; dst[16:33] = 2013; dst[33:83] = 2010                        # (16 / 17 parallel edges from hub 0: duplicates)
    dst[83:] = 2100 + np.arange(len(slots) - 83) % 100
    src, dsts = [slots], [dst]
    h7 = np.repeat(np.array([i for i in range(1024) if i % 8 == 7]), 24)
    src.append(h7); dsts.append(4000 + np.arange(len(h7)) % 3000)
    cold = lambda k: rng.integers(1024, n, k)
    for r, k in [(2011, 50), (2012, 16), (2013, 16)] + [(r, 10) for r in range(2100, 2200)]:
        src.append(cold(k)); dsts.append(np.full(k, r))
    loops = np.array([2150, 3000, 3001, 3002, 3002])                             # self loops: one on a long row, one doubled
    src.append(loops); dsts.append(loops)
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dsts).astype(np.int64)
    perm = rng.permutation(len(src))
    return n, src[perm], dst[perm]


def test_hand_built_rows_and_special_values(sliced, pgl):
    n, src, dst = _hand_graph()
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
