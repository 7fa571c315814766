"""The graph-pooling definitions (tests/pool_defs.py) against everything that can be checked without a GPU: today's tensor code of
pgl_amd.math.segment_topk and pgl_amd.utils.transform.filter_adj on CPU tensors, the reference's own outputs
(tests/golden/layers/readouts.npz), the host twins of the kernels (pglamd_segment_topk_host, pglamd_filter_edges_host) bit for
bit, topk_counts against the torch expression it replaces, and the host reads the front end's source is allowed to hold."""
import inspect
import os

import numpy as np
import pytest
import torch

import pool_defs as D

HERE = os.path.dirname(os.path.abspath(__file__))
RATIOS = (0.1, 0.25, 0.3, 1.0 / 3.0, 0.5, 0.7, 0.8, 0.999, 1.0)


def _batch(rng, n_graphs, max_nodes):
    lens = rng.integers(0, max_nodes + 1, n_graphs)
    lens[-1] = max(int(lens[-1]), 1)                                 # (torch's path takes the segment count from the last id)
    return lens.astype(np.int64)


def test_the_two_restatements_of_the_order_agree():
    rng = np.random.default_rng(0)
    for kind in D.FLAVOURS:
        lens = _batch(rng, 9, 40)
        scores = D.score_flavour(kind, int(lens.sum()), rng)
        k = np.minimum(lens, rng.integers(0, 41, len(lens)))
        assert np.array_equal(D.topk_perm_restated(scores, D.ptr(lens), D.ptr(k)), D.topk_perm_by_comparison(scores, D.ptr(lens), D.ptr(k))), kind
    ex = np.array([1, np.nan, -0., 0., np.inf, -1e20, -np.inf, np.nan, 0., -1e20], np.float32)
    assert D.topk_perm_restated(ex, [0, 10], [0, 10]).tolist() == [1, 7, 4, 0, 2, 3, 8, 5, 9, 6]


@pytest.mark.parametrize("ratio", [0.3, 0.5, 1.0, 3, 1])
def test_defs_equal_todays_segment_topk_on_cpu_tensors(ratio):
    import pgl_amd
    from pgl_amd import pool_ops
    rng = np.random.default_rng(1)
    for kind in D.FLAVOURS:
        lens = _batch(rng, 23, 60)
        scores = D.score_flavour(kind, int(lens.sum()), rng)
        scores = np.where(scores < -1e20, np.float32(-7.0), scores).astype(np.float32)      # today's padding value bounds its domain: scores >= -1e20
        scores[scores == -np.inf] = -7.0
        gid = torch.as_tensor(np.repeat(np.arange(len(lens)), lens))
        x = torch.as_tensor(np.arange(len(scores), dtype=np.float32).reshape(-1, 1))
        _, perm = pgl_amd.math.segment_topk(x, torch.as_tensor(scores), gid, ratio, return_index=True)
        k = pool_ops.topk_counts(lens, ratio)
        assert np.array_equal(perm.numpy(), D.topk_perm_restated(scores, D.ptr(lens), D.ptr(k))), (kind, ratio)


def test_defs_equal_todays_filter_adj_on_cpu_tensors():
    from pgl_amd.utils.transform import filter_adj
    rng = np.random.default_rng(2)
    n, e = 300, 2000
    edges = rng.integers(0, n, (e, 2)).astype(np.int64)
    edges[:50, 1] = edges[:50, 0]                                    # self-loops
    edges[50:100] = edges[100:150]                                   # multi-edges
    attr = np.arange(e, dtype=np.float32)
    for m in (0, 1, 90, n):
        perm = rng.permutation(n)[:m].astype(np.int64)
        want_e, want_p = D.filter_edges_restated(edges, perm, n)
        got_e, got_a = filter_adj(torch.as_tensor(edges), torch.as_tensor(perm), torch.as_tensor(attr), num_nodes=n)
        assert np.array_equal(got_e.numpy().reshape(-1, 2), want_e) and np.array_equal(got_a.numpy(), attr[want_p]), m


def test_defs_equal_the_reference_fixtures():
    from pgl_amd import pool_ops
    z = np.load(os.path.join(HERE, "golden", "layers", "readouts.npz"))
    sizes = np.asarray(z["sizes"], np.int64)
    scores = z["feat"][:, 2].astype(np.float32)
    k = pool_ops.topk_counts(sizes, 0.3)
    assert np.array_equal(D.topk_perm_restated(scores, D.ptr(sizes), D.ptr(k)), z["topk_perm"])
    edges = np.concatenate([z["edges_%d" % i] + sizes[:i].sum() for i in range(len(sizes))])
    out, _ = D.filter_edges_restated(edges, z["filter_perm"], int(sizes.sum()))
    assert np.array_equal(out, z["filter_edges"])
    got, pos, flags = pool_ops.host_filter_edges(edges, z["filter_perm"], int(sizes.sum()))
    assert flags == 0 and np.array_equal(got, z["filter_edges"]) and np.array_equal(edges[pos][:, 0], z["filter_perm"][got[:, 0]])
    perm, status = pool_ops.host_topk_perm(scores, D.ptr(sizes), D.ptr(k))
    assert status == 0 and np.array_equal(perm, z["topk_perm"])


def test_topk_counts_equals_the_torch_expression():
    from pgl_amd import pool_ops
    lens = np.arange(0, 5001, dtype=np.int64)
    t = torch.as_tensor(lens)
    for r in RATIOS:
        assert np.array_equal(pool_ops.topk_counts(lens, r), torch.ceil(r * t.float()).long().numpy()), r
    for r in (0, 1, 3, 5000, 10 ** 6):
        assert np.array_equal(pool_ops.topk_counts(lens, r), torch.clamp(t, max=r).numpy()), r
    assert pool_ops.topk_supported(0) and pool_ops.topk_supported(pool_ops.TOPK_MAX_SEG) and not pool_ops.topk_supported(pool_ops.TOPK_MAX_SEG + 1)
    assert pool_ops.TOPK_MAX_SEG >= 4096


@pytest.mark.parametrize("kind", D.FLAVOURS)
def test_host_topk_equals_the_definition_bit_for_bit(kind):
    from pgl_amd import pool_ops
    rng = np.random.default_rng(3)
    cap = pool_ops.TOPK_MAX_SEG
    lens = np.array([0, 1, 2, 63, 64, 65, 255, 256, 257, 0, 1000, cap - 1, cap, 7], np.int64)
    scores = D.score_flavour(kind, int(lens.sum()), rng)             # ("special" holds -inf and values below -1e20)
    for mode in range(4):
        k = [np.zeros_like(lens), np.minimum(lens, 1), (lens + 1) // 2, lens][mode]
        perm, status = pool_ops.host_topk_perm(scores, D.ptr(lens), D.ptr(k))
        assert status == 0 and np.array_equal(perm, D.topk_perm_restated(scores, D.ptr(lens), D.ptr(k))), (kind, mode)


def test_host_topk_flags_and_skips_bad_segments():
    from pgl_amd import pool_ops
    cap = pool_ops.TOPK_MAX_SEG
    rng = np.random.default_rng(4)
    lens = np.array([5, cap + 1, 6], np.int64)
    scores = rng.standard_normal(int(lens.sum())).astype(np.float32)
    k = np.array([2, 3, 6], np.int64)
    perm, status = pool_ops.host_topk_perm(scores, D.ptr(lens), D.ptr(k))
    assert status == 1 and (perm[2:5] == -1).all()
    good = D.topk_perm_restated(scores, D.ptr(lens), D.ptr(np.array([2, 0, 6])))
    assert np.array_equal(perm[[0, 1, 5, 6, 7, 8, 9, 10]], good)
    perm, status = pool_ops.host_topk_perm(scores[:11], D.ptr([5, 6]), D.ptr([6, 1]))          # k > len
    assert status == 2 and (perm[:6] == -1).all() and perm[6] == 5 + int(np.argmax(scores[5:11]))


def test_host_filter_edges_equals_the_definition_bit_for_bit():
    from pgl_amd import pool_ops
    rng = np.random.default_rng(5)
    n = 3000
    edges = rng.integers(0, n, (20000, 2)).astype(np.int64)
    edges[:300, 1] = edges[:300, 0]
    edges[300:600] = edges[600:900]
    for m in (0, 1, 900, n):
        perm = rng.permutation(n)[:m].astype(np.int64)
        for e in (0, 1, 1023, 1024, 1025, 20000):
            got_e, got_p, flags = pool_ops.host_filter_edges(edges[:e], perm, n)
            want_e, want_p = D.filter_edges_restated(edges[:e], perm, n)
            assert flags == 0 and np.array_equal(got_e, want_e) and np.array_equal(got_p, want_p), (m, e)
    assert pool_ops.host_filter_edges(edges, np.array([1, 2, 1]), n)[2] == 2
    assert pool_ops.host_filter_edges(edges, np.array([1, n]), n)[2] == 1
    assert pool_ops.host_filter_edges(np.array([[0, n]]), np.array([0]), n)[2] == 1
    assert pool_ops.host_filter_edges(np.array([[-1, 0]]), np.array([0, 0]), n)[2] == 3


def test_host_reads_in_the_front_end_source():
    from pgl_amd import pool_ops
    reads = (".item(", ".cpu(", ".tolist(", ".numpy(")
    src = inspect.getsource(pool_ops.topk_perm)
    assert not any(r in src for r in reads)
    src = inspect.getsource(pool_ops.filter_edges)
    assert sum(src.count(r) for r in reads) == 1 and "kept, flags = status.tolist()" in src
    assert "flags = int(status.item())" in inspect.getsource(pool_ops.topk_check)
    for quoted in ("`flags = int(status.item())`", "`kept, flags = status.tolist()`"):
        assert quoted in pool_ops.__doc__
    # the routed SAGPool forward adds no read of its own: the plan is host arithmetic on _graph_node_index
    import pgl_amd
    for fn in (pgl_amd.nn.SAGPool._host_plan, pgl_amd.nn.SAGPool._forward_device):
        assert not any(r in inspect.getsource(fn) for r in reads), fn.__name__


def test_front_end_refuses_cpu_and_dtype_mismatches():
    from pgl_amd import pool_ops
    s, p = torch.zeros(4), torch.tensor([0, 4])
    with pytest.raises(ValueError, match="GPU"):
        pool_ops.topk_perm(s, p, p, 4)
    with pytest.raises(ValueError, match="GPU"):
        pool_ops.filter_edges(torch.zeros((3, 2), dtype=torch.int64), torch.tensor([0]), 4)


def test_abi_declares_the_pool_entry_points():
    import pgl_amd
    L = pgl_amd._ffi.lib()
    for name in ("pglamd_segment_topk", "pglamd_segment_topk_host", "pglamd_filter_edges_workspace_bytes", "pglamd_filter_edges_count",
                 "pglamd_filter_edges_fill", "pglamd_filter_edges_host", "pglamd_filter_edges_launch_threads"):
        assert hasattr(L, name) and name in pgl_amd._ffi.exported_symbols()
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "pgl_amd.h")).read()
    assert "#define PGLAMD_TOPK_MAX_SEG %d" % pgl_amd.pool_ops.TOPK_MAX_SEG in hdr
    assert L.pglamd_filter_edges_workspace_bytes(10, 10) > 0
