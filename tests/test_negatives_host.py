"""The host twin of checked negative sampling (pglamd_sample_negatives_host) and the Python layers above it on numpy graphs, held
to the definition restated in tests/negative_defs.py: host twin == restatement == brute force on the hand-built cases, the same
arrays for 1, 3 and 16 threads, the argument errors, Graph._csr_pred_sorted, negative_samples / corrupt_edges / bpr_triples."""
import ctypes

import numpy as np
import pytest

import negative_defs as D


@pytest.fixture(scope="module")
def pgl():
    import pgl_amd
    return pgl_amd


@pytest.fixture(scope="module")
def fx(pgl):
    edges = D.fixture_edges()
    g = pgl.Graph(edges=edges, num_nodes=D.N)
    indptr, col = g._csr_succ_sorted()
    want = D.succ_index(edges, D.N)
    assert np.array_equal(indptr, want[0]) and np.array_equal(col, want[1])
    table = pgl.ops.host_edge_weight_table(np.array([0, D.N], np.int64), D.WEIGHTS)
    assert np.array_equal(table.cum, D.quantise(D.WEIGHTS))
    return dict(g=g, edges=edges, indptr=indptr, col=col, table=table)


def _host(pgl, fx, src, K, seed, lo, hi, weighted, exclude_self, max_trials, **kw):
    return pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src, K, seed=seed, lo=lo, hi=None if weighted else hi,
                                         noise=fx["table"] if weighted else None, exclude_self=exclude_self, max_trials=max_trials,
                                         return_pos=True, **kw)


@pytest.mark.parametrize("n,K", D.SHAPES + [(0, 3)])
@pytest.mark.parametrize("lo,hi,weighted,exclude_self,max_trials", D.MODES)
def test_host_twin_is_the_restatement_and_the_brute_force(pgl, fx, n, K, lo, hi, weighted, exclude_self, max_trials):
    src = D.batch(n)
    neg, pos = _host(pgl, fx, src, K, 77, lo, hi, weighted, exclude_self, max_trials)
    assert neg.dtype == pos.dtype == np.int64 and neg.shape == (n, K) and pos.shape == (n,)
    for brute in (False, True):
        want = D.negatives_restated(fx["indptr"], fx["col"], src, K, seed=77, lo=lo, hi=hi, cum=fx["table"].cum if weighted else None,
                                    exclude_self=exclude_self, max_trials=max_trials, brute=brute)
        assert np.array_equal(neg, want[0]) and np.array_equal(pos, want[1]) and want[2] == 0


@pytest.mark.parametrize("max_trials", [0, 1, 16])
@pytest.mark.parametrize("seed", [0, 5, 2 ** 63 + 9])
def test_a_row_that_leaves_one_id_returns_that_id(pgl, fx, max_trials, seed):
    src = np.array([D.ALL_BUT_17] * 9, np.int64)
    neg = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src, 7, seed=seed, lo=D.LO, hi=D.HI, max_trials=max_trials)
    assert (neg == 17).all()                                  # successors below lo and at or above hi did not shrink the complement
    neg = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], [D.ONLY_25] * 9, 7, seed=seed, lo=D.LO, hi=D.HI, exclude_self=True,
                                        max_trials=max_trials)
    assert (neg == 25).all()
    neg = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], [D.W_ONLY_29] * 9, 7, seed=seed, noise=fx["table"], max_trials=max_trials)
    assert (neg == 29).all()


@pytest.mark.parametrize("weighted", [False, True])
def test_an_empty_complement_is_minus_one_and_raises_unless_allowed(pgl, fx, weighted):
    src = np.array([D.MULTI, D.W_NONE if weighted else D.ALL, D.MULTI], np.int64)
    kw = dict(noise=fx["table"]) if weighted else dict(lo=D.LO, hi=D.HI)
    with pytest.raises(ValueError, match="allow_empty"):
        pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src, 4, seed=1, **kw)
    for max_trials in (0, 16):
        neg, pos = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src, 4, seed=1, allow_empty=True, return_pos=True,
                                                 max_trials=max_trials, **kw)
        assert (neg[1] == -1).all() and (neg[[0, 2]] >= 0).all() and (pos >= 0).all()
        want = D.negatives_restated(fx["indptr"], fx["col"], src, 4, seed=1, cum=fx["table"].cum if weighted else None,
                                    lo=0 if weighted else D.LO, hi=D.N if weighted else D.HI, max_trials=max_trials)
        assert np.array_equal(neg, want[0]) and want[2] == D.FLAG_EMPTY


def test_exclude_self_inside_outside_and_as_a_self_loop(pgl, fx):
    for v, inside in ((D.SELF_IN, True), (D.SELF_IN_LOOP, True), (D.SELF_OUT, False), (D.SELF_LOOP, False)):
        src = np.full(400, v, np.int64)
        for max_trials in (0, 16):
            with_self = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src, 3, seed=3, lo=D.LO, hi=D.HI, exclude_self=True,
                                                      max_trials=max_trials)
            X = D.excluded(fx["indptr"], fx["col"], v, D.LO, D.HI, True)
            assert set(with_self.ravel().tolist()) == set(range(D.LO, D.HI)) - set(X)        # 1200 draws over <= 20 ids: all are met
            assert (v in X) == inside
    plain = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], np.full(400, D.SELF_IN, np.int64), 3, seed=3, lo=D.LO, hi=D.HI)
    assert D.SELF_IN in plain                                 # without exclude_self the source is a legal negative


def test_an_empty_row_has_no_positive_and_unconstrained_negatives(pgl, fx):
    neg, pos = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], np.full(500, D.EMPTY, np.int64), 4, seed=8, return_pos=True)
    assert (pos == -1).all() and set(neg.ravel().tolist()) == set(range(D.N))


def test_the_positive_follows_positions_of_a_multi_edge_row(pgl, fx):
    src = np.full(64, D.MULTI, np.int64)
    _, pos = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src, 2, seed=21, return_pos=True)
    b, end = fx["indptr"][D.MULTI], fx["indptr"][D.MULTI + 1]
    want = [int(fx["col"][b + D.scale64(D.draw(D.walker_key(21, i), 2, 0), int(end - b))]) for i in range(64)]
    assert pos.tolist() == want and end - b == 11 and len(set(want)) <= 6


def test_the_key_is_the_position_not_the_node(pgl, fx):
    src = D.batch(40)
    src[7] = src[3]
    neg = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src, 6, seed=4)
    assert not np.array_equal(neg[3], neg[7])                 # the same source at two positions
    perm = np.random.default_rng(0).permutation(40)
    neg_p = pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], src[perm], 6, seed=4)
    assert np.array_equal(neg_p, D.negatives_restated(fx["indptr"], fx["col"], src[perm], 6, seed=4)[0])
    same = np.full(40, D.EMPTY, np.int64)                     # one unconstrained source everywhere: row i depends on i alone
    assert np.array_equal(pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], same, 6, seed=4),
                          pgl.ops.host_sample_negatives(fx["indptr"], fx["col"], same[perm], 6, seed=4))


@pytest.fixture(scope="module")
def rmat(pgl):
    """RMAT scale 10, 3 000 sources x 5: (numpy graph, indptr, col, sources, noise table, the restated uniform and weighted draws)."""
    from pgl_amd.utils.rmat import rmat_edges
    edges = rmat_edges(10, 16000, seed=9).numpy().astype(np.int64)
    g = pgl.Graph(edges=edges, num_nodes=1 << 10)
    indptr, col = g._csr_succ_sorted()
    src = np.random.default_rng(2).integers(0, 1 << 10, 3000).astype(np.int64)
    table = pgl.ops.host_edge_weight_table(np.array([0, 1 << 10], np.int64), np.diff(indptr).astype(np.float64) ** 0.75)
    want_u = D.negatives_restated(indptr, col, src, 5, seed=31, exclude_self=True)
    want_w = D.negatives_restated(indptr, col, src, 5, seed=31, cum=table.cum)
    return dict(g=g, edges=edges, indptr=indptr, col=col, src=src, table=table, want_u=want_u, want_w=want_w)


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_rmat_batch_is_the_restatement_for_every_thread_count(pgl, rmat, threads):
    r = rmat
    for want, kw in ((r["want_u"], dict(exclude_self=True)), (r["want_w"], dict(noise=r["table"]))):
        neg, pos = pgl.ops.host_sample_negatives(r["indptr"], r["col"], r["src"], 5, seed=31, return_pos=True, threads=threads, **kw)
        assert np.array_equal(neg, want[0]) and np.array_equal(pos, want[1]) and want[2] == 0
        D.assert_no_successor(r["indptr"], r["col"], r["src"], neg)


def test_argument_errors(pgl, fx):
    ip, col = fx["indptr"], fx["col"]
    f = pgl.ops.host_sample_negatives
    for bad in (dict(num_neg=0), dict(max_trials=-1), dict(max_trials=1 << 20), dict(lo=5, hi=5), dict(lo=-1), dict(hi=D.N + 1),
                dict(lo=9, hi=3), dict(noise=fx["table"], lo=1), dict(noise=fx["table"], hi=D.N - 1)):
        kw = dict(num_neg=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            f(ip, col, [0, 1], **kw)
    with pytest.raises(TypeError):
        f(ip, col, [0, 1], 2, noise=fx["table"].cum)
    for bad in ([0, D.N], [-1, 3]):
        with pytest.raises(ValueError, match="out of"):
            f(ip, col, bad, 2)
    # the library's own codes, under the Python checks
    L = pgl._ffi.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    src, neg, flags, cum = np.array([0, 2], np.int64), np.empty((2, 2), np.int64), np.zeros(1, np.int32), fx["table"].cum

    def rc(num_neg=2, lo=0, hi=D.N, max_trials=16, c=None, s=src):
        return L.pglamd_sample_negatives_host(p(ip), p(col), D.N, p(c), lo, hi, p(s), 2, num_neg, 0, max_trials, 1, 1, p(neg), None, p(flags))
    ARG, SHAPE, RANGE = -6, -1, -3
    assert rc() == 0 and rc(c=cum) == 0
    assert rc(num_neg=0) == ARG and rc(max_trials=-1) == ARG and rc(max_trials=1 << 20) == ARG
    assert rc(lo=4, hi=4) == SHAPE and rc(lo=8, hi=4) == SHAPE and rc(lo=-1) == RANGE and rc(hi=D.N + 1) == RANGE
    assert rc(c=cum, lo=1) == RANGE and rc(s=np.array([0, D.N], np.int64)) == RANGE
    assert b"source" in L.pglamd_last_error()


def test_pred_sorted_is_the_mirror(pgl, fx):
    indptr, col = fx["g"]._csr_pred_sorted()
    want = D.pred_index(fx["edges"], D.N)
    assert indptr.dtype == np.int64 and col.dtype == np.int32 and np.array_equal(indptr, want[0]) and np.array_equal(col, want[1])
    assert fx["g"]._csr_pred_sorted()[1] is col               # cached


def test_negative_samples_on_a_numpy_graph(pgl, fx, rmat):
    g, src = fx["g"], D.batch(50)
    got = pgl.sampling.negative_samples(g, src, 4, seed=6, candidates=(D.LO, D.HI))
    assert isinstance(got, np.ndarray) and np.array_equal(got, D.negatives_restated(fx["indptr"], fx["col"], src, 4, seed=6, lo=D.LO, hi=D.HI,
                                                                                   exclude_self=True)[0])
    for noise in (D.WEIGHTS, fx["table"]):
        got = pgl.sampling.negative_samples(g, src, 4, seed=6, noise=noise, exclude_self=False)
        assert np.array_equal(got, D.negatives_restated(fx["indptr"], fx["col"], src, 4, seed=6, cum=fx["table"].cum)[0])
    with pytest.raises(ValueError, match="sub-range"):
        pgl.sampling.negative_samples(g, src, 4, noise=D.WEIGHTS, candidates=(D.LO, D.HI))
    with pytest.raises(ValueError, match="allow_empty"):
        pgl.sampling.negative_samples(g, [D.ALL], 4, candidates=(D.LO, D.HI))
    assert (pgl.sampling.negative_samples(g, [D.ALL], 4, candidates=(D.LO, D.HI), allow_empty=True) == -1).all()
    got = pgl.sampling.negative_samples(rmat["g"], rmat["src"], 5, seed=31)
    assert np.array_equal(got, rmat["want_u"][0])


def test_corrupt_edges_on_a_numpy_graph(pgl, rmat):
    g, edges = rmat["g"], rmat["edges"][:2000]
    tails = pgl.sampling.corrupt_edges(g, edges, 3, side="dst", seed=2)
    assert np.array_equal(tails, D.negatives_restated(rmat["indptr"], rmat["col"], edges[:, 0], 3, seed=2)[0])
    D.assert_no_successor(rmat["indptr"], rmat["col"], edges[:, 0], tails)
    heads = pgl.sampling.corrupt_edges(g, edges, 3, side="src", seed=2)
    pptr, pcol = D.pred_index(rmat["edges"], 1 << 10)
    assert np.array_equal(heads, D.negatives_restated(pptr, pcol, edges[:, 1], 3, seed=2)[0])
    have = set(map(tuple, rmat["edges"].tolist()))
    assert not any((int(h), int(v)) in have for v, row in zip(edges[:, 1], heads) for h in row)     # no head has an edge to the kept tail
    with pytest.raises(ValueError):
        pgl.sampling.corrupt_edges(g, edges, 3, side="both")


def test_bpr_triples_on_a_numpy_graph(pgl):
    """30 users (ids 0 .. 29), 40 items (ids 30 .. 69); users 3 and 11 have no positive."""
    rng = np.random.default_rng(12)
    e = np.stack([rng.integers(0, 30, 300), rng.integers(30, 70, 300)], 1).astype(np.int64)
    e = e[(e[:, 0] != 3) & (e[:, 0] != 11)]
    g = pgl.Graph(edges=e, num_nodes=70)
    users = np.concatenate([np.arange(30), np.arange(30)]).astype(np.int64)
    u, pos, neg = pgl.sampling.bpr_triples(g, users, (30, 70), seed=5)
    assert np.array_equal(u, users[(users != 3) & (users != 11)]) and u.shape == pos.shape == neg.shape
    have = set(map(tuple, e.tolist()))
    assert all((a, b) in have for a, b in zip(u.tolist(), pos.tolist()))
    assert not any((a, b) in have for a, b in zip(u.tolist(), neg.tolist())) and ((neg >= 30) & (neg < 70)).all()
    indptr, col = g._csr_succ_sorted()
    want = D.negatives_restated(indptr, col, users, 1, seed=5, lo=30, hi=70)
    keep = want[1] >= 0
    assert np.array_equal(pos, want[1][keep]) and np.array_equal(neg, want[0][keep, 0])
