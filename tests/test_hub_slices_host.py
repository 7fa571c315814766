"""ops.slice_plan on CPU tensors: the re-ordered edge stream pglamd_aggregate_sliced walks (a rest stream followed by eight per-XCD
slices of the long rows' hub edges) holds exactly the index's edges, every slice only its own hub ranks, no short row in a slice,
and a block table that tiles the stream's blocks in order.  RMAT-13, 150 k edges."""
import pytest
import torch

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


def test_stream_holds_exactly_the_index_edges(planned):
    ops, csr, hub, p, n, E = planned
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
    keep = ~((hub[1].long() >= n) & (csr.indptr[1:] - csr.indptr[:-1] > L)[csr.row32.long()])
    assert torch.equal(vr[rest], csr.row32.long()[keep]) and torch.equal(c[rest], hub[1].long()[keep])


def test_every_slice_holds_only_its_own_ranks_and_only_long_rows(planned):
    ops, csr, hub, p, n, E = planned
    R = p.n_long
    vr, c = p.row32.long(), p.col32.long()
    deg = csr.indptr[1:] - csr.indptr[:-1]
    assert torch.equal(p.long_rows.long(), torch.nonzero(deg > L).reshape(-1))
    v = vr >= p.out_rows
    assert int(v.sum()) > 0 and bool((c[v] >= n).all())                             # slices hold hub edges only
    s = (vr[v] - p.out_rows) // R
    assert torch.equal((c[v] - n) % 8, s)
    assert sorted(set(s.tolist())) == list(range(8))
    rows_in_slices = p.long_rows.long()[(vr[v] - p.out_rows) % R]
    assert bool((deg[rows_in_slices] > L).all())                                    # no row of <= L edges in a slice
    # ... and no hub edge of a long row is left in the rest stream
    rest_long = ~v & (deg[vr.clamp(max=n - 1)] > L) & (vr < n)
    assert not bool((c[rest_long] >= n).any())
    assert p.seg_edges[0] == 0 and p.seg_edges[-1] == E and p.seg_edges[1] == int((~v).sum())
    assert all(int(p.indptr[p.out_rows + k * R]) == p.seg_edges[1 + k] for k in range(9))


def test_block_offsets_are_monotone_and_tile_the_stream(planned):
    ops, csr, hub, p, n, E = planned
    first, count = p.blocks[:9], p.blocks[9:]
    assert len(p.blocks) == 18 and first[0] == 0 and all(c >= 0 for c in count)
    assert all(first[k] <= first[k + 1] for k in range(8))
    assert all(first[k] + count[k] == (first[k + 1] if k < 8 else p.n_blocks) for k in range(9))
    per = 4 * p.chunk
    assert p.n_blocks == -(-E // per) and p.chunk == ops._flat_chunk(E)
    assert all(abs(first[k] * per - p.seg_edges[k]) < per for k in range(1, 9))     # a segment starts within one block of its table entry
    assert p.blocks_dev.tolist() == p.blocks


def test_plan_declines(planned, monkeypatch):
    ops, csr, hub, p, n, E = planned
    assert ops.slice_plan(csr, None, n, n) is None                                  # no hub plan
    assert ops.slice_plan(csr, hub, n, n, row_min=2000) is None                     # fewer than 64 long rows
    monkeypatch.setattr(ops, "_HUB_SLICES", False)
    assert ops.slice_table(csr, torch.zeros(n, 128), hub, n) is None                # switched off
    monkeypatch.setattr(ops, "_HUB_SLICES", True)
    monkeypatch.setattr(ops, "_SLICE_MIN_EDGES", 0)
    assert ops.slice_table(csr, torch.zeros(n, 130), hub, n) is None                # a width the sliced kernel is not built for
