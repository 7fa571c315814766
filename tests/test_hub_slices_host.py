"""ops.slice_plan on CPU tensors: the re-ordered edge stream pglamd_aggregate_sliced walks (a rest stream followed by eight per-XCD
slices of the long rows' hub edges) holds exactly the index's edges, every slice only its own hub ranks, no short row in a slice,
and a block table that tiles the stream's blocks in order.  RMAT-13, 150 k edges, and every graph of tests/hub_slice_defs.py at
chunk 8, 64, 128 and 256 (the chunk is injected through ops._flat_chunk: the plan carries it to the launch)."""
import pytest
import torch

import hub_slice_defs as H

L = 32


@pytest.fixture(scope="module")
def planned():
    from pgl_amd import ops
    from pgl_amd.utils.rmat import rmat_edges
    n, E = 1 << 13, 150000
    e = rmat_edges(13, E, seed=1, device=torch.device("cpu"))
    order = torch.argsort(e[:, 1], stable=True)
    row, col = e[order, 1], e[order, 0]
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    csr = ops.CSR(indptr, row.int(), col.int(), order.int(), n, E)
    hub = ops.hub_plan(csr, n, 512)
    assert hub is not None and len(hub) == 3 and hub[0].shape[0] == 1024          # (_hub entries keep their shape)
    out_rows = n + 100
    plan = ops.slice_plan(csr, hub, n, out_rows, row_min=L)
    assert plan is not None and plan.n_long >= 64 and plan.out_rows == out_rows and plan.row_min == L
    assert ops.slice_plan(csr, hub, n, out_rows, row_min=L) is plan                 # cached on the index
    return ops, csr, hub, plan, n, E


def _check_stream(csr, hub, p, n, E, row_min=L):
    R = p.n_long
    vr, c = p.row32.long(), p.col32.long()
    assert vr.shape[0] == E and bool((vr[1:] >= vr[:-1]).all())                     # one stream, sorted by (virtual) row
    assert int(vr.max()) < p.out_rows + 8 * R
    real = torch.where(vr >= p.out_rows, p.long_rows.long()[(vr - p.out_rows).clamp(min=0) % R], vr)
    src = torch.where(c >= n, hub[0].long()[(c - n).clamp(min=0)], c)
    want = torch.sort(csr.row32.long() * n + csr.col32.long()).values
    assert torch.equal(torch.sort(real * n + src).values, want)
    # indptr describes the stream: out_rows real rows (those past the index's own are empty), then 8 * R virtual rows
    assert p.indptr.shape[0] == p.out_rows + 8 * R + 1 and int(p.indptr[0]) == 0 and int(p.indptr[-1]) == E
    assert torch.equal(p.indptr[1:] - p.indptr[:-1], torch.bincount(vr, minlength=p.out_rows + 8 * R))
    assert int(p.indptr[p.out_rows] - p.indptr[n]) == 0
    # the rest stream keeps the index's order row by row
    rest = vr < p.out_rows
    keep = ~((hub[1].long() >= n) & (csr.indptr[1:] - csr.indptr[:-1] > row_min)[csr.row32.long()])
    assert torch.equal(vr[rest], csr.row32.long()[keep]) and torch.equal(c[rest], hub[1].long()[keep])


def _check_slices(csr, hub, p, n, E, row_min=L, slices_with_edges=range(8)):
    R = p.n_long
    vr, c = p.row32.long(), p.col32.long()
    deg = csr.indptr[1:] - csr.indptr[:-1]
    assert torch.equal(p.long_rows.long(), torch.nonzero(deg > row_min).reshape(-1))
    v = vr >= p.out_rows
    assert int(v.sum()) > 0 and bool((c[v] >= n).all())                             # slices hold hub edges only
    s = (vr[v] - p.out_rows) // R
    assert torch.equal((c[v] - n) % 8, s)
    assert sorted(set(s.tolist())) == list(slices_with_edges)
    rows_in_slices = p.long_rows.long()[(vr[v] - p.out_rows) % R]
    assert bool((deg[rows_in_slices] > row_min).all())                              # no row of <= row_min edges in a slice
    # ... and no hub edge of a long row is left in the rest stream
    rest_long = ~v & (deg[vr.clamp(max=n - 1)] > row_min) & (vr < n)
    assert not bool((c[rest_long] >= n).any())
    assert p.seg_edges[0] == 0 and p.seg_edges[-1] == E and p.seg_edges[1] == int((~v).sum())
    assert all(int(p.indptr[p.out_rows + k * R]) == p.seg_edges[1 + k] for k in range(9))


def _check_blocks(p, E, chunk):
    first, count = p.blocks[:9], p.blocks[9:]
    assert len(p.blocks) == 18 and first[0] == 0 and all(c >= 0 for c in count)
    assert all(first[k] <= first[k + 1] for k in range(8))
    assert all(first[k] + count[k] == (first[k + 1] if k < 8 else p.n_blocks) for k in range(9))
    per = 4 * p.chunk
    assert p.n_blocks == -(-E // per) and p.chunk == chunk
    assert all(abs(first[k] * per - p.seg_edges[k]) < per for k in range(1, 9))     # a segment starts within one block of its table entry
    assert p.blocks_dev.tolist() == p.blocks


def _check_grid_reaches_every_block_once(p):
    """The launch's grid of 8 * slice_blocks_per_xcd blocks, mapped by slice_block as restated in hub_slice_defs, covers
    [0, n_blocks) exactly once, XCD x only through slice x's blocks and its own eighth of the rest.  This guards the TABLES a plan
    emits; it is not a test of the device function, which only a GPU runs."""
    per = H.slice_blocks_per_xcd(p.blocks)
    grid = [H.slice_block(p.blocks, b) for b in range(8 * per)]
    assert sorted(b for b in grid if b >= 0) == list(range(p.n_blocks))
    n_rest = p.blocks[9]
    for b, lb in enumerate(grid):
        x = b % 8
        if lb >= 0:
            in_slice = p.blocks[1 + x] <= lb < p.blocks[1 + x] + p.blocks[10 + x]
            in_rest = n_rest * x // 8 <= lb < n_rest * (x + 1) // 8
            assert in_slice != in_rest, (b, lb)
    assert max(sum(1 for b in range(x, 8 * per, 8) if grid[b] >= 0) for x in range(8)) == per      # the grid is as deep as the busiest XCD needs, no deeper


def test_stream_holds_exactly_the_index_edges(planned):
    ops, csr, hub, p, n, E = planned
    _check_stream(csr, hub, p, n, E)


def test_every_slice_holds_only_its_own_ranks_and_only_long_rows(planned):
    ops, csr, hub, p, n, E = planned
    _check_slices(csr, hub, p, n, E)


def test_block_offsets_are_monotone_and_tile_the_stream(planned):
    ops, csr, hub, p, n, E = planned
    _check_blocks(p, E, ops._flat_chunk(E))
    _check_grid_reaches_every_block_once(p)


def test_plan_declines(planned, monkeypatch):
    ops, csr, hub, p, n, E = planned
    assert ops.slice_plan(csr, None, n, n) is None                                  # no hub plan
    assert ops.slice_plan(csr, hub, n, n, row_min=2000) is None                     # fewer than 64 long rows
    assert ops.slice_plan(csr, hub, n, n - 1, row_min=L) is None                    # out_rows < n: rows of the index would have no output row
    monkeypatch.setattr(ops, "_HUB_SLICES", False)
    assert ops.slice_table(csr, torch.zeros(n, 128), hub, n) is None                # switched off
    monkeypatch.setattr(ops, "_HUB_SLICES", True)
    monkeypatch.setattr(ops, "_SLICE_MIN_EDGES", 0)
    assert ops.slice_table(csr, torch.zeros(n, 130), hub, n) is None                # a width the sliced kernel is not built for
    g63 = H.all_hub(rows=63)
    c63 = H.cpu_csr(ops, *g63)
    assert ops.slice_plan(c63, ops.hub_plan(c63, H.N, 512), H.N, H.N, row_min=L) is None   # 63 long rows: one short of _SLICE_MIN_ROWS
    g64 = H.all_hub(rows=64)
    c64 = H.cpu_csr(ops, *g64)
    assert ops.slice_plan(c64, ops.hub_plan(c64, H.N, 512), H.N, H.N, row_min=L).n_long == 64


_WITH_EDGES = {"all_hub": range(8), "one_slice3": [3], "one_slice6": [6], "tiny": range(8), "mixed_long": range(8), "hand_graph": range(7)}


@pytest.mark.parametrize("chunk", [8, 64, 128, 256])
@pytest.mark.parametrize("name", sorted(H.BUILDERS))
def test_invariants_on_every_builder_and_chunk(name, chunk, monkeypatch):
    from pgl_amd import ops
    n, src, dst = H.BUILDERS[name]()
    E = len(src)
    monkeypatch.setattr(ops, "_flat_chunk", lambda num_edges: chunk)
    base = H.cpu_csr(ops, n, src, dst)
    for out_rows in (n, n + 100):
        csr = base.view()                                                           # (the plan cache key does not contain the chunk)
        hub = ops.hub_plan(csr, n, 512)
        p = ops.slice_plan(csr, hub, n, out_rows, row_min=L)
        assert p is not None and p.out_rows == out_rows and p.row_min == L
        _check_stream(csr, hub, p, n, E)
        _check_slices(csr, hub, p, n, E, slices_with_edges=_WITH_EDGES[name])
        _check_blocks(p, E, chunk)
        _check_grid_reaches_every_block_once(p)


@pytest.mark.parametrize("chunk", [8, 256])
def test_invariants_at_the_production_row_threshold(planned, chunk, monkeypatch):
    ops, csr0, hub0, p0, n, E = planned
    monkeypatch.setattr(ops, "_flat_chunk", lambda num_edges: chunk)
    csr = csr0.view()
    hub = ops.hub_plan(csr, n, 512)
    p = ops.slice_plan(csr, hub, n, n, row_min=128)
    assert p is not None and p.row_min == 128 and 64 <= p.n_long < p0.n_long
    _check_stream(csr, hub, p, n, E, row_min=128)
    _check_slices(csr, hub, p, n, E, row_min=128)
    _check_blocks(p, E, chunk)
    _check_grid_reaches_every_block_once(p)
