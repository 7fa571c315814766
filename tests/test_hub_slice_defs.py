"""Every property tests/hub_slice_defs.py claims for its graphs, proven with ops.hub_plan / ops.slice_plan on CPU tensors (no GPU):
the hub ranks, the long rows, the three degenerate block tables, the rows that enter each fix-up role, the exactness condition of
the integer features."""
import numpy as np
import pytest

import hub_slice_defs as H

L = 32


@pytest.fixture(scope="module")
def ops():
    from pgl_amd import ops
    return ops


def _plan(ops, monkeypatch, graph, chunk, row_min=L, out_rows=None):
    n, src, dst = graph
    monkeypatch.setattr(ops, "_flat_chunk", lambda num_edges: chunk)
    csr = H.cpu_csr(ops, n, src, dst)
    hub = ops.hub_plan(csr, n, 512)
    assert hub is not None and np.array_equal(hub[0].numpy(), np.arange(H.HUBS))          # rank == id
    return ops.slice_plan(csr, hub, n, n if out_rows is None else out_rows, row_min=row_min), csr


@pytest.mark.parametrize("name", sorted(H.BUILDERS))
def test_builders_shape_and_hub_order(ops, name):
    n, src, dst = H.BUILDERS[name]()
    assert n == H.N == 8192 and src.dtype == np.int64 and dst.dtype == np.int64 and src.shape == dst.shape
    assert src.min() >= 0 and src.max() < n and dst.min() >= 0 and dst.max() < n
    out = np.bincount(src, minlength=n)
    assert (np.diff(out[:H.HUBS]) <= 0).all() and out[H.HUBS:].max() < out[H.HUBS - 1]     # hubs first, ties by id: rank == id
    order = np.lexsort((src, dst))
    assert not np.array_equal(order, np.arange(len(src)))                                  # permuted, not sorted
    n2, s2, d2 = H.BUILDERS[name]()
    assert np.array_equal(src, s2) and np.array_equal(dst, d2)                             # deterministic
    assert int(np.bincount(dst).max()) * 8 < (1 << 24)                                     # small_int_features sums stay exact


def test_all_hub(ops, monkeypatch):
    n, src, dst = H.all_hub()
    assert len(src) == 65536
    deg = np.bincount(dst, minlength=n)
    assert (deg[4096:4160] == 1024).all() and deg.sum() == 65536 and int((deg == 0).sum()) == 8128
    assert (src < H.HUBS).all() and (np.bincount(src, minlength=n)[:H.HUBS] == 64).all()
    p, _ = _plan(ops, monkeypatch, (n, src, dst), 64)
    assert p.n_long == 64 == ops._SLICE_MIN_ROWS == H.MIN_ROWS and p.chunk == 64
    assert p.seg_edges == [0, 0] + [8192 * k for k in range(1, 9)]                         # the rest stream is empty
    assert p.blocks[9] == 0 and p.blocks[10:] == [32] * 8 and p.n_blocks == 256
    f = H.plan_facts(p)
    assert f["empty_virtual"] == 0 and f["rest_chunks"] == 0 and f["virtual_chunks"] == 2 and f["blocks_per_segment"] == [0] + [32] * 8
    p128, _ = _plan(ops, monkeypatch, (n, src, dst), 256, row_min=128)                     # long at the production threshold as well
    assert p128.n_long == 64 and p128.chunk == 256


def test_all_hub_with_63_rows_declines(ops, monkeypatch):
    g = H.all_hub(rows=63)
    assert len(g[1]) == 63 * 1024
    p, _ = _plan(ops, monkeypatch, g, 64)
    assert p is None


@pytest.mark.parametrize("s", [3, 6])
def test_one_slice(ops, monkeypatch, s):
    n, src, dst = H.one_slice(s)
    assert len(src) == 24576 and (np.bincount(src, minlength=n)[:H.HUBS] == 24).all() and (src < H.HUBS).all()
    deg = np.bincount(dst, minlength=n)
    assert (deg[2000:2064] == 48).all() and int((deg > L).sum()) == 64
    assert set((src[(dst >= 2000) & (dst < 2064)] % 8).tolist()) == {s}
    assert not (src[deg[dst] <= L] % 8 == s).any()
    p, _ = _plan(ops, monkeypatch, (n, src, dst), 64)
    want = [84] + [0] * 8
    want[1 + s] = 12
    assert p.n_long == 64 and p.blocks[9:] == want
    if s == 3:
        assert p.blocks[9:] == [84, 0, 0, 0, 12, 0, 0, 0, 0]
    assert p.seg_edges == [0] + [21504] * (1 + s) + [24576] * (8 - s)
    f = H.plan_facts(p)
    assert f["empty_virtual"] == 7 * 64 and f["virtual_chunks"] == 1 and f["blocks_per_segment"] == want


def test_tiny(ops, monkeypatch):
    n, src, dst = H.tiny()
    assert len(src) == 2112
    deg = np.bincount(dst, minlength=n)
    assert (deg[4096:4160] == 33).all() and deg.sum() == 2112 and (src < H.HUBS).all()
    assert (np.bincount(src % 8) == 264).all()
    p, _ = _plan(ops, monkeypatch, (n, src, dst), 256)
    assert p.n_long == 64 and p.n_blocks == 3 and p.chunk == 256
    assert p.seg_edges == [0] + [264 * k for k in range(9)]
    assert p.blocks == [0, 0, 1, 1, 1, 2, 2, 2, 2, 0, 1, 0, 0, 1, 0, 0, 0, 1]
    assert all(e % (4 * 256) != 0 for e in p.seg_edges[2:9])                               # every later boundary lies inside a block
    assert p.n_blocks < 8 and H.slice_blocks_per_xcd(p.blocks) == 1


def test_hand_graph_is_the_graph_the_gpu_test_describes(ops, monkeypatch):
    n, src, dst = H.hand_graph()
    deg = np.bincount(dst, minlength=n)
    assert deg[2012] == L and deg[2013] == L + 1 and deg[0] == 0 and deg[2011] == 50
    assert (np.bincount(src, minlength=n)[:H.HUBS] == 24).all() and np.bincount(src, minlength=n)[H.HUBS:].max() < 24
    p, _ = _plan(ops, monkeypatch, (n, src, dst), 64)
    assert p.n_long == 103 and p.seg_edges[8] == p.seg_edges[9] and p.seg_edges[7] < p.seg_edges[8]


def test_mixed_long(ops, monkeypatch):
    n, src, dst = H.mixed_long()
    hn, hs, hd = H.hand_graph()
    key = lambda s, d: np.sort(s * n + d)
    mine, hand = key(src, dst), key(hs, hd)
    extra = len(src) - len(hs)
    assert extra == 2 * H.HUBS + 3000
    rows_added = (dst == H.MIXED_COLD_ROW) | (dst == H.MIXED_ONE_RESIDUE_ROW) | ((dst >= 7000) & (dst < 8000))
    assert int(rows_added.sum()) == extra and np.array_equal(key(src[~rows_added], dst[~rows_added]), hand)   # hand_graph's edges, untouched
    assert (np.bincount(src, minlength=n)[:H.HUBS] == 26).all() and np.bincount(src, minlength=n)[H.HUBS:].max() < 26
    deg = np.bincount(dst, minlength=n)
    a, b = dst == H.MIXED_COLD_ROW, dst == H.MIXED_ONE_RESIDUE_ROW
    assert int((a & (src >= H.HUBS)).sum()) == 3000 and int((a & (src < H.HUBS)).sum()) == 200
    assert deg[H.MIXED_ONE_RESIDUE_ROW] == 256 > 17 * 8 and set((src[b] % 8).tolist()) == {H.MIXED_RESIDUE} and (src[b] < H.HUBS).all()
    assert deg[7000:8000].max() <= L
    # row 2150 (the special-value cases): long, hub edges of several residues, cold sources and its self loop
    r = dst == 2150
    assert deg[2150] > L and {1, 2, 4} <= set((src[r & (src < H.HUBS)] % 8).tolist()) and int((r & (src >= H.HUBS)).sum()) == 11
    for chunk in (8, 64, 256):
        p, _ = _plan(ops, monkeypatch, (n, src, dst), chunk)
        assert p.n_long == 105
        f = H.plan_facts(p)
        ip = p.indptr.numpy()
        i = p.long_rows.tolist().index(H.MIXED_ONE_RESIDUE_ROW)
        v = [int(ip[n + s * p.n_long + i + 1] - ip[n + s * p.n_long + i]) for s in range(8)]
        assert v == [256 if s == H.MIXED_RESIDUE else 0 for s in range(8)] and ip[H.MIXED_ONE_RESIDUE_ROW + 1] == ip[H.MIXED_ONE_RESIDUE_ROW]
        assert ip[H.MIXED_COLD_ROW + 1] - ip[H.MIXED_COLD_ROW] == 3000
        assert f["rest_chunks"] >= 3000 // chunk                                          # the remainder row is itself split
        if chunk == 8:
            assert f["virtual_long"] == 1 and f["virtual_chunks"] in (32, 33)               # 256 edges: the long role, on a virtual row
            assert f["virtual_short"] >= 600 and f["rest_long"] >= 1 and f["rest_short"] >= 1
        else:
            assert f["virtual_long"] == 0                                                   # (at the default chunk only the short role runs)
        assert f["empty_virtual"] >= 8 + 7                                                  # row 2011's eight, row 2301's seven


def test_rmat14(ops, monkeypatch):
    n, src, dst = H.rmat14()
    assert n == 1 << 14 and len(src) == 400_000 and src.dtype == np.int64
    deg = np.bincount(dst, minlength=n)
    assert int((deg > 128).sum()) == 470 and int((deg > L).sum()) == 1751 and int(deg.max()) == 8650 and int(deg.max()) * 8 < (1 << 24)
    csr = H.cpu_csr(ops, n, src, dst)
    for chunk, row_min, n_long in ((8, L, 1751), (64, L, 1751), (128, L, 1751), (256, L, 1751), (256, 128, 470), (128, 128, 470)):
        monkeypatch.setattr(ops, "_flat_chunk", lambda num_edges: chunk)
        c = csr.view()
        p = ops.slice_plan(c, ops.hub_plan(c, n, 512), n, n, row_min=row_min)
        assert p.n_long == n_long and p.chunk == chunk and 0 < p.seg_edges[1] < 400_000
        f = H.plan_facts(p)
        assert f["virtual_short"] > 0 and f["rest_short"] > 0 and all(b > 0 for b in f["blocks_per_segment"])
        if chunk == 8:                                  # both fix-up roles, on virtual rows and on remainder rows
            assert f["virtual_long"] > 0 and f["rest_long"] > 0 and f["virtual_chunks"] > H.FIX_SHORT + 1
        if chunk == 64:
            assert f["virtual_long"] == 0               # the default chunk alone never runs the long role on a virtual row


def test_plan_facts_on_hand_worked_rows():
    import collections
    import torch
    P = collections.namedtuple("P", ["indptr", "chunk", "out_rows", "n_long", "blocks"])
    # chunk 8, two real rows and eight virtual ones (n_long = 1).  real row 0: edges [0, 8): one chunk, not cut.  real row 1: [8, 30):
    # chunks 1 .. 3.  virtual rows: [30, 30) empty, [30, 38): 8 edges, never cut, [38, 47): 9 edges in chunks 4 and 5,
    # [47, 47 + 136): chunks 5 .. 22 = 18 pieces (long), [183, 183 + 129): chunks 22 .. 38 = 17 pieces (short), then empty rows
    ip = [0, 8, 30, 30, 38, 47, 183, 312, 312, 312, 312]
    f = H.plan_facts(P(torch.tensor(ip), 8, 2, 1, list(range(18))))
    assert f == dict(virtual_chunks=18, rest_chunks=3, virtual_long=1, virtual_short=2, rest_long=0, rest_short=1, empty_virtual=4,
                     blocks_per_segment=list(range(9, 18)))


def test_small_int_features_and_exact_sum():
    x = H.small_int_features(100, 6, 3)
    assert x.dtype == np.float32 and x.shape == (100, 6) and np.array_equal(x, np.round(x)) and x.min() == -8 and x.max() == 8
    assert np.array_equal(x, H.small_int_features(100, 6, 3)) and not np.array_equal(x, H.small_int_features(100, 6, 4))
    src, dst = np.array([0, 1, 1, 99]), np.array([2, 2, 2, 0])
    out = H.exact_sum(x, src, dst, 5)
    assert out.dtype == np.float32 and np.array_equal(out[2], x[0] + 2 * x[1]) and np.array_equal(out[0], x[99]) and not out[[1, 3, 4]].any()


def test_slice_block_emulation_on_a_hand_table():
    # rest: 5 blocks [0, 5); slice 0: 2 blocks [5, 7); slice 7: 1 block [7, 8); the other slices own none
    tab = [0, 5, 7, 7, 7, 7, 7, 7, 7, 5, 2, 0, 0, 0, 0, 0, 0, 1]
    per = H.slice_blocks_per_xcd(tab)
    assert per == 2                                                                        # XCD 0: 0 rest + 2 slice blocks; XCD 7: 1 + 1
    got = [H.slice_block(tab, b) for b in range(8 * per)]
    assert sorted(b for b in got if b >= 0) == list(range(8))
    assert [got[0], got[8]] == [5, 6] and sorted([got[7], got[15]]) == [4, 7]               # XCD x takes slice x's blocks
