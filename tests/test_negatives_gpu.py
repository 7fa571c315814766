"""Checked negative sampling on the MI355X (negative.hip) held to its definition, restated in tests/negative_defs.py: device ==
host twin == restatement bit for bit on the hand-built cases (wave and block tails, fallback only, ranges, self, multi-edges,
weighted noise), the flags, one RMAT batch, the sampling layer on tensor graphs, the launch count of bpr_triples, the fixed-seed
uniformity counts, and the example."""
import os
import sys

import numpy as np
import pytest
import torch

import negative_defs as D
from gpu_common import dev, host, pgl      # noqa: F401  (pgl: the module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(pgl):
    edges = D.fixture_edges()
    gt = pgl.Graph(edges=edges, num_nodes=D.N).tensor()
    csr = gt._csr_succ_sorted()
    indptr, col = D.succ_index(edges, D.N)
    assert np.array_equal(host(csr.indptr), indptr) and np.array_equal(host(csr.col32), col)
    table = pgl.ops.weight_table(dev(D.WEIGHTS))
    assert np.array_equal(host(table.cum), D.quantise(D.WEIGHTS))
    host_table = pgl.ops.host_edge_weight_table(np.array([0, D.N], np.int64), D.WEIGHTS)
    return dict(gt=gt, gn=pgl.Graph(edges=edges, num_nodes=D.N), edges=edges, csr=csr, indptr=indptr, col=col, table=table,
                host_table=host_table)


def _device(pgl, fx, src, K, seed, lo, hi, weighted, exclude_self, max_trials, **kw):
    return pgl.ops.sample_negatives(fx["csr"], dev(src), K, seed=seed, lo=lo, hi=None if weighted else hi,
                                    noise=fx["table"] if weighted else None, exclude_self=exclude_self, max_trials=max_trials,
                                    return_pos=True, **kw)


@pytest.mark.parametrize("n,K", D.SHAPES + [(0, 3)])
@pytest.mark.parametrize("lo,hi,weighted,exclude_self,max_trials", D.MODES)
def test_device_is_the_host_twin_is_the_restatement(pgl, fx, n, K, lo, hi, weighted, exclude_self, max_trials):
    src = D.batch(n)
    neg, pos = _device(pgl, fx, src, K, 77, lo, hi, weighted, exclude_self, max_trials)
    assert neg.dtype == pos.dtype == torch.int64 and tuple(neg.shape) == (n, K) and tuple(pos.shape) == (n,)
    want = D.negatives_restated(fx["indptr"], fx["col"], src, K, seed=77, lo=lo, hi=hi, cum=host(fx["table"].cum) if weighted else None,
                                exclude_self=exclude_self, max_trials=max_trials, brute=True)
    assert np.array_equal(host(neg), want[0]) and np.array_equal(host(pos), want[1]) and want[2] == 0
    twin = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src, K, seed=77, lo=lo, hi=None if weighted else hi,
                                         noise=fx["host_table"] if weighted else None, exclude_self=exclude_self, max_trials=max_trials,
                                         return_pos=True)
    assert np.array_equal(host(neg), twin[0]) and np.array_equal(host(pos), twin[1])


@pytest.mark.parametrize("max_trials", [0, 1, 16])
@pytest.mark.parametrize("seed", [0, 5, 2 ** 63 + 9])
def test_a_row_that_leaves_one_id_returns_that_id(pgl, fx, max_trials, seed):
    f = pgl.ops.sample_negatives
    assert bool((f(fx["csr"], dev([D.ALL_BUT_17] * 9), 7, seed=seed, lo=D.LO, hi=D.HI, max_trials=max_trials) == 17).all())
    assert bool((f(fx["csr"], dev([D.ONLY_25] * 9), 7, seed=seed, lo=D.LO, hi=D.HI, exclude_self=True, max_trials=max_trials) == 25).all())
    assert bool((f(fx["csr"], dev([D.W_ONLY_29] * 9), 7, seed=seed, noise=fx["table"], max_trials=max_trials) == 29).all())


@pytest.mark.parametrize("weighted", [False, True])
def test_an_empty_complement_is_minus_one_sets_the_flag_and_raises_unless_allowed(pgl, fx, weighted):
    src = np.array([D.MULTI, D.W_NONE if weighted else D.ALL, D.MULTI], np.int64)
    kw = dict(noise=fx["table"]) if weighted else dict(lo=D.LO, hi=D.HI)
    with pytest.raises(ValueError, match="allow_empty"):
        pgl.ops.sample_negatives(fx["csr"], dev(src), 4, seed=1, **kw)
    for max_trials in (0, 16):
        want = D.negatives_restated(fx["indptr"], fx["col"], src, 4, seed=1, cum=host(fx["table"].cum) if weighted else None,
                                    lo=0 if weighted else D.LO, hi=D.N if weighted else D.HI, max_trials=max_trials)
        for opts in (dict(allow_empty=True), dict(check=False)):
            neg, pos = pgl.ops.sample_negatives(fx["csr"], dev(src), 4, seed=1, return_pos=True, max_trials=max_trials, **kw, **opts)
            assert np.array_equal(host(neg), want[0]) and np.array_equal(host(pos), want[1])
        assert (want[0][1] == -1).all() and want[2] == D.FLAG_EMPTY
    # the flag itself, through the C ABI
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    neg = torch.empty((3, 4), dtype=torch.int64, device="cuda")
    d_src = dev(src)
    P = pgl.ops._ptr
    pgl.ops._launch("sample_negatives", d_src, P(fx["csr"].indptr), P(fx["csr"].col32), D.N, P(fx["table"].cum) if weighted else None,
                    0 if weighted else D.LO, D.N if weighted else D.HI, P(d_src), 3, 4, 0, 16, 1, P(neg), None, P(flags))
    assert int(flags.item()) == D.FLAG_EMPTY


def test_an_out_of_range_source_sets_the_flag_and_is_never_dereferenced(pgl, fx):
    src = np.array([D.MULTI, D.N, -1, 2 ** 62, -2 ** 62, D.SELF_LOOP], np.int64)
    with pytest.raises(ValueError, match="outside"):
        pgl.ops.sample_negatives(fx["csr"], dev(src), 3, seed=2)
    neg, pos = pgl.ops.sample_negatives(fx["csr"], dev(src), 3, seed=2, return_pos=True, check=False)
    want = D.negatives_restated(fx["indptr"], fx["col"], src, 3, seed=2)
    assert np.array_equal(host(neg), want[0]) and np.array_equal(host(pos), want[1]) and want[2] == D.FLAG_RANGE
    assert (host(neg)[1:5] == -1).all() and (host(pos)[1:5] == -1).all() and (host(neg)[[0, 5]] >= 0).all()
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_src, out = dev(src), torch.empty((6, 3), dtype=torch.int64, device="cuda")
    P = pgl.ops._ptr
    pgl.ops._launch("sample_negatives", d_src, P(fx["csr"].indptr), P(fx["csr"].col32), D.N, None, 0, D.N, P(d_src), 6, 3, 0, 16, 2, P(out),
                    None, P(flags))
    assert int(flags.item()) == D.FLAG_RANGE and torch.equal(out, neg)
    with pytest.raises(ValueError, match="out of"):
        pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src, 3, seed=2)


def test_the_key_is_the_position_not_the_node(pgl, fx):
    src = D.batch(40)
    src[7] = src[3]
    neg = host(pgl.ops.sample_negatives(fx["csr"], dev(src), 6, seed=4))
    assert not np.array_equal(neg[3], neg[7])
    perm = np.random.default_rng(0).permutation(40)
    neg_p = host(pgl.ops.sample_negatives(fx["csr"], dev(src[perm]), 6, seed=4))
    assert np.array_equal(neg_p, D.negatives_restated(fx["indptr"], fx["col"], src[perm], 6, seed=4)[0])
    same = np.full(40, D.EMPTY, np.int64)
    assert torch.equal(pgl.ops.sample_negatives(fx["csr"], dev(same), 6, seed=4), pgl.ops.sample_negatives(fx["csr"], dev(same[perm]), 6, seed=4))


def test_empty_row_and_multi_edge_positive(pgl, fx):
    neg, pos = pgl.ops.sample_negatives(fx["csr"], dev(np.full(500, D.EMPTY, np.int64)), 4, seed=8, return_pos=True)
    assert bool((pos == -1).all()) and set(host(neg).ravel().tolist()) == set(range(D.N))
    _, pos = pgl.ops.sample_negatives(fx["csr"], dev(np.full(64, D.MULTI, np.int64)), 2, seed=21, return_pos=True)
    b, end = fx["indptr"][D.MULTI], fx["indptr"][D.MULTI + 1]
    assert host(pos).tolist() == [int(fx["col"][b + D.scale64(D.draw(D.walker_key(21, i), 2, 0), int(end - b))]) for i in range(64)]


def test_argument_errors_come_before_any_launch(pgl, fx, monkeypatch):
    n = [0]
    inner = pgl.ops._launch
    monkeypatch.setattr(pgl.ops, "_launch", lambda *a, **k: (n.__setitem__(0, n[0] + 1), inner(*a, **k))[1])
    src = dev([0, 2])
    for bad in (dict(num_neg=0), dict(max_trials=-1), dict(max_trials=1 << 20), dict(lo=5, hi=5), dict(lo=-1), dict(hi=D.N + 1),
                dict(noise=fx["table"], lo=1), dict(noise=fx["table"], hi=D.N - 1)):
        kw = dict(num_neg=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            pgl.ops.sample_negatives(fx["csr"], src, **kw)
    with pytest.raises(RuntimeError):
        pgl.ops.sample_negatives(fx["csr"], torch.tensor([0, 2]), 2)                     # a CPU tensor: no fallback
    assert n[0] == 0
    # the library's own codes
    L, P = pgl._ffi.lib(), pgl.ops._ptr
    neg = torch.empty((2, 2), dtype=torch.int64, device="cuda")
    rc = lambda num_neg=2, lo=0, hi=D.N, max_trials=16, cum=None: L.pglamd_sample_negatives(
        P(fx["csr"].indptr), P(fx["csr"].col32), D.N, cum, lo, hi, P(src), 2, num_neg, 0, max_trials, 1, P(neg), None, None, None)
    assert rc(num_neg=0) == -6 and rc(max_trials=1 << 20) == -6 and rc(lo=4, hi=4) == -1 and rc(hi=D.N + 1) == -3
    assert rc(cum=P(fx["table"].cum), lo=1) == -3


# ---- one RMAT batch ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat(pgl):
    from pgl_amd.utils.rmat import rmat_edges
    edges = rmat_edges(10, 16000, seed=9).numpy().astype(np.int64)
    gn = pgl.Graph(edges=edges, num_nodes=1 << 10)
    gt = pgl.Graph(edges=edges, num_nodes=1 << 10).tensor()
    indptr, col = gn._csr_succ_sorted()
    src = np.random.default_rng(2).integers(0, 1 << 10, 3000).astype(np.int64)
    w = np.diff(indptr).astype(np.float64) ** 0.75
    table, host_table = pgl.ops.weight_table(dev(w)), pgl.ops.host_edge_weight_table(np.array([0, 1 << 10], np.int64), w)
    assert np.array_equal(host(table.cum), host_table.cum)
    want_u = D.negatives_restated(indptr, col, src, 5, seed=31, exclude_self=True)
    want_w = D.negatives_restated(indptr, col, src, 5, seed=31, cum=host_table.cum)
    return dict(gn=gn, gt=gt, edges=edges, indptr=indptr, col=col, src=src, table=table, host_table=host_table, want_u=want_u, want_w=want_w)


def test_rmat_batch_device_host_restatement(pgl, rmat):
    r = rmat
    csr = r["gt"]._csr_succ_sorted()
    for want, kw, hkw in ((r["want_u"], dict(exclude_self=True), dict(exclude_self=True)),
                          (r["want_w"], dict(noise=r["table"]), dict(noise=r["host_table"]))):
        neg, pos = pgl.ops.sample_negatives(csr, dev(r["src"]), 5, seed=31, return_pos=True, **kw)
        twin = pgl.ops.host_sample_negatives(r["indptr"], r["col"], r["src"], 5, seed=31, return_pos=True, threads=5, **hkw)
        assert np.array_equal(host(neg), want[0]) and np.array_equal(host(pos), want[1]) and want[2] == 0
        assert np.array_equal(twin[0], want[0]) and np.array_equal(twin[1], want[1])
        D.assert_no_successor(r["indptr"], r["col"], r["src"], host(neg))
    got = pgl.sampling.negative_samples(r["gt"], dev(r["src"]), 5, seed=31)
    assert isinstance(got, torch.Tensor) and np.array_equal(host(got), r["want_u"][0])
    assert np.array_equal(pgl.sampling.negative_samples(r["gn"], r["src"], 5, seed=31), host(got))
    got = pgl.sampling.negative_samples(r["gt"], r["src"], 5, seed=31, noise=dev(np.diff(r["indptr"]).astype(np.float64) ** 0.75),
                                        exclude_self=False)
    assert np.array_equal(host(got), r["want_w"][0])


def test_pred_sorted_and_corrupt_edges_on_a_tensor_graph(pgl, rmat):
    r = rmat
    pptr, pcol = D.pred_index(r["edges"], 1 << 10)
    pred = r["gt"]._csr_pred_sorted()
    assert np.array_equal(host(pred.indptr), pptr) and np.array_equal(host(pred.col32), pcol) and r["gt"]._csr_pred_sorted() is pred
    edges = r["edges"][:2000]
    heads = pgl.sampling.corrupt_edges(r["gt"], dev(edges), 3, side="src", seed=2)
    assert np.array_equal(host(heads), D.negatives_restated(pptr, pcol, edges[:, 1], 3, seed=2)[0])
    assert np.array_equal(host(heads), pgl.sampling.corrupt_edges(r["gn"], edges, 3, side="src", seed=2))
    have = set(map(tuple, r["edges"].tolist()))
    assert not any((int(h), int(v)) in have for v, row in zip(edges[:, 1], host(heads)) for h in row)
    tails = pgl.sampling.corrupt_edges(r["gt"], dev(edges), 3, side="dst", seed=2)
    assert np.array_equal(host(tails), D.negatives_restated(r["indptr"], r["col"], edges[:, 0], 3, seed=2)[0])
    D.assert_no_successor(r["indptr"], r["col"], edges[:, 0], host(tails))


def test_bpr_triples_is_one_launch_and_obeys_the_graph(pgl, monkeypatch):
    rng = np.random.default_rng(12)
    e = np.stack([rng.integers(0, 30, 300), rng.integers(30, 70, 300)], 1).astype(np.int64)
    e = e[(e[:, 0] != 3) & (e[:, 0] != 11)]
    gt, gn = pgl.Graph(edges=e, num_nodes=70).tensor(), pgl.Graph(edges=e, num_nodes=70)
    users = np.concatenate([np.arange(30), np.arange(30)]).astype(np.int64)
    gt._csr_succ_sorted()                                                    # (the index is built once per graph)
    n = [0]
    inner = pgl.ops._launch
    monkeypatch.setattr(pgl.ops, "_launch", lambda *a, **k: (n.__setitem__(0, n[0] + 1), inner(*a, **k))[1])
    u, pos, neg = pgl.sampling.bpr_triples(gt, dev(users), (30, 70), seed=5)
    assert n[0] == 1
    u, pos, neg = host(u), host(pos), host(neg)
    assert np.array_equal(u, users[(users != 3) & (users != 11)]) and u.shape == pos.shape == neg.shape
    have = set(map(tuple, e.tolist()))
    assert all((a, b) in have for a, b in zip(u.tolist(), pos.tolist()))
    assert not any((a, b) in have for a, b in zip(u.tolist(), neg.tolist())) and ((neg >= 30) & (neg < 70)).all()
    hu, hpos, hneg = pgl.sampling.bpr_triples(gn, users, (30, 70), seed=5)
    assert np.array_equal(u, hu) and np.array_equal(pos, hpos) and np.array_equal(neg, hneg)


def test_uniformity_counts_equal_the_restatement(pgl, fx):
    """The counts are a pure function of the fixed seed: tests/test_negative_defs.py holds the restatement's counts within five
    binomial standard deviations of their expectation; the device must give exactly those counts."""
    index = (fx["indptr"], fx["col"])
    want = D.uniformity_counts(index)
    got = D.uniformity_counts(index, lambda src, K, c: host(pgl.ops.sample_negatives(
        fx["csr"], dev(src), K, seed=D.UNIFORM_SEED, noise=None if c is None else fx["table"])))
    for (g, probs), (w, _) in zip(got, want):
        print(g.tolist())
        assert D.within_five_sigma(w, probs, D.UNIFORM_DRAWS) and np.array_equal(g, w)


def test_train_lightgcn_bpr_example(pgl):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_lightgcn_bpr
    finally:
        sys.path.pop(0)
    res = train_lightgcn_bpr.main(["--users", "200", "--items", "120", "--steps", "30", "--batch_size", "512"])
    print("train_lightgcn_bpr:", {k: v for k, v in res.items() if k != "losses"})
    assert len(res["losses"]) == 30 and all(np.isfinite(res["losses"])) and res["loss_last"] < res["loss_first"], res
