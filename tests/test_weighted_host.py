"""Edge-weighted sampling on the host (no GPU): the weight table's host twin against its numpy restatement bit for bit, its
invariants and refusals, weighted walks of the host twin against the restatement and against the exact weighted path law, the
argument checks, graph_kernel.alias_sample_build_table against the reference's table, and the restated weighted neighbour sampler
against the successive-sampling law (which pins the definition the device is held to in tests/test_weighted_gpu.py)."""
import numpy as np
import pytest

import sampling_defs as S
import walk_defs as D
import weighted_defs as W


@pytest.fixture(scope="module")
def pgl():
    import pgl_amd
    return pgl_amd


@pytest.fixture(scope="module")
def walk_graph(pgl):
    g = pgl.Graph(edges=D.EDGES, num_nodes=D.N, edge_feat={"w": W.WALK_WEIGHTS})
    indptr, col = g._csr_succ_sorted()
    table = g.edge_weight_table("w", "succ")
    return g, indptr, col, table


# ---- table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("with_eid", [False, True])
def test_host_table_equals_the_restatement(pgl, dtype, with_eid):
    indptr, weight = W.TABLE_GRAPH
    w = weight.astype(dtype)
    if dtype == np.float64:                                   # values that are NOT fp32 numbers too
        w = w * (1.0 + np.random.default_rng(3).random(len(w)) * 1e-9)
    eid = None
    if with_eid:
        eid = np.random.default_rng(4).permutation(len(w)).astype(np.int32)
        shuffled = np.empty_like(w)
        shuffled[eid] = w
        w = shuffled
    got = pgl.ops.host_edge_weight_table(indptr, w, eid)
    cum, npos = W.table_restated(indptr, w, eid)
    assert got.cum.dtype == np.int64 and got.npos.dtype == np.int64
    assert np.array_equal(got.cum, cum) and np.array_equal(got.npos, npos)


def test_table_invariants_and_edge_rows(pgl):
    indptr, weight = W.TABLE_GRAPH
    t = pgl.ops.host_edge_weight_table(indptr, weight.astype(np.float32))
    q, rows = W.quantise(indptr, weight.astype(np.float32))
    assert np.array_equal(W.q_of(indptr, t.cum), q) and (q >= 0).all() and (q <= 2 ** 32).all()
    inside = np.ones(len(q), bool)
    inside[indptr[:-1][np.diff(indptr) > 0]] = False
    assert (np.diff(t.cum, prepend=0)[inside] >= 0).all()                 # non-decreasing within every row
    last = indptr[1:][np.diff(indptr) > 0] - 1
    assert np.array_equal(t.cum[last], np.array([q[b:e].sum() for b, e in zip(indptr[:-1], indptr[1:]) if e > b]))   # cum[last] = sum of q
    assert np.array_equal(t.npos, np.array([(q[b:e] > 0).sum() for b, e in zip(indptr[:-1], indptr[1:])]))
    row = lambda v: q[indptr[v]:indptr[v + 1]].tolist()
    assert row(0) == [] and t.npos[0] == 0
    assert row(1) == [2 ** 32]
    assert row(2) == [0] * 5 and t.npos[2] == 0 and t.cum[indptr[3] - 1] == 0
    assert row(3) == [0, int(2 / 5 * 2 ** 32), 0, 0, 2 ** 32, int(1 / 5 * 2 ** 32), 0] and t.npos[3] == 3
    assert row(4)[2] == 2 ** 32 and row(4)[0] == 1 and row(4)[5] == 1 and row(4)[1] == 1      # below 2^-32 of the maximum: one quantum
    assert row(5)[5] == 0 and min(row(5)[:5]) >= 1 and row(5)[3] == 2 ** 32                 # fp32 subnormals keep their ratios
    assert row(6) == [2 ** 32, 2 ** 32, int(2 ** 32 / 7), 2 ** 32, int(0.5 / 7 * 2 ** 32), 2 ** 32]
    assert t.npos[W.HUB_ROW] == (q[indptr[W.HUB_ROW]:indptr[W.HUB_ROW + 1]] > 0).sum() > 60000


@pytest.mark.parametrize("bad,word", [(np.nan, "NaN"), (-1.0, "negative"), (np.inf, "infinite"), (-np.inf, "negative")])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_invalid_weights_raise(pgl, bad, word, dtype):
    indptr = np.array([0, 2, 5], np.int64)
    w = np.array([1, 2, 3, 4, 5], dtype)
    w[3] = bad
    with pytest.raises(ValueError, match=word):
        pgl.ops.host_edge_weight_table(indptr, w)
    g = pgl.Graph(edges=np.array([[0, 1], [1, 0], [0, 1], [1, 1], [0, 0]]), num_nodes=2)
    for index in ("dst", "succ"):
        with pytest.raises(ValueError, match=word):
            g.edge_weight_table(w, index)
    with pytest.raises(ValueError):
        pgl.ops.host_edge_weight_table(indptr, w[:4])                         # one weight short
    assert pgl.ops.host_edge_weight_table(indptr, np.array([-0.0, 1, 0, 0, 0], dtype)).npos.tolist() == [1, 0]   # -0.0 is a zero


def test_integer_and_half_weights_are_cast_to_fp32(pgl):
    indptr = np.array([0, 3, 4], np.int64)
    for w in (np.array([1, 2, 4, 9], np.int64), np.array([1, 2, 4, 9], np.float16)):
        t = pgl.ops.host_edge_weight_table(indptr, w)
        assert t.cum.tolist() == [2 ** 30, 2 ** 30 + 2 ** 31, 2 ** 30 + 2 ** 31 + 2 ** 32, 2 ** 32]


def test_graph_tables_compose_the_edge_permutation(pgl):
    edges, n, w = W.table_graph_edges()
    g = pgl.Graph(edges=edges, num_nodes=n, edge_feat={"w": w.astype(np.float32)})
    indptr, _, eid = S.csr_by_dst(edges, n)
    t = g.edge_weight_table("w", "dst")
    cum, npos = W.table_restated(indptr, w.astype(np.float32), eid)
    assert np.array_equal(t.cum, cum) and np.array_equal(t.npos, npos)
    sptr, _, seid = W.succ_index(edges, n)
    t = g.edge_weight_table(w, "succ")                                        # an array in edge order (fp64)
    cum, npos = W.table_restated(sptr, w, seid)
    assert np.array_equal(g._csr_succ_sorted()[0], sptr)
    assert np.array_equal(t.cum, cum) and np.array_equal(t.npos, npos)
    with pytest.raises(ValueError):
        g.edge_weight_table(w[:-1], "dst")
    with pytest.raises(ValueError):
        g.edge_weight_table(w, "src")
    with pytest.raises(KeyError):
        g.edge_weight_table("nope")


# ---- walks -------------------------------------------------------------------------------------------------------------------
def test_host_weighted_walk_equals_the_restatement(pgl, walk_graph):
    g, indptr, col, table = walk_graph
    sptr, scol, seid = W.succ_index(D.EDGES, D.N)
    assert np.array_equal(sptr, indptr) and np.array_equal(scol, col)
    cum, npos = W.table_restated(sptr, W.WALK_WEIGHTS, seid)
    assert np.array_equal(table.cum, cum) and np.array_equal(table.npos, npos)
    starts = np.arange(3000) % D.N
    for seed in (5, 2 ** 40 + 11, 2 ** 64 - 1):
        got = pgl.ops.host_random_walk(indptr, col, starts, 12, seed=seed, weights=table)
        want = W.walk_restated(indptr, col, cum, starts, 12, seed)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[1] < 13).any() and (got[1] == 13).any()
    assert np.array_equal(got[0][starts == 4], np.array([[4] + [-1] * 12] * int((starts == 4).sum())))


def test_threads_do_not_change_the_weighted_walks(pgl, walk_graph):
    _, indptr, col, table = walk_graph
    starts = np.arange(5000) % D.N
    one = pgl.ops.host_random_walk(indptr, col, starts, 12, seed=9, threads=1, weights=table)
    many = pgl.ops.host_random_walk(indptr, col, starts, 12, seed=9, threads=7, weights=table)
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])


def test_a_zero_weight_edge_is_never_followed(pgl, walk_graph):
    g, indptr, col, table = walk_graph
    walks = pgl.sampling.random_walk(g, list(range(D.N)) * 400, 9, seed=2, weights="w")
    steps = {(a, b) for w in walks for a, b in zip(w[:-1], w[1:])}
    positive = {(int(s), int(d)) for (s, d), x in zip(D.EDGES.tolist(), W.WALK_WEIGHTS.tolist()) if x > 0}
    assert (3, 1) not in steps and steps == positive               # 3 -> 1 has weight 0; 2 -> 5 survives through its other copy
    # a node whose out-edges all weigh zero is a dead end
    w0 = W.WALK_WEIGHTS.copy()
    w0[D.EDGES[:, 0] == 6] = 0
    walks = pgl.sampling.random_walk(g, [6, 6, 5], 5, seed=1, weights=w0)
    assert walks[0] == [6] and walks[1] == [6]
    ends = [w[-1] for w in pgl.sampling.random_walk(g, [5] * 200, 30, seed=1, weights=w0) if len(w) < 30]
    assert 6 in ends and set(ends) <= {4, 6}                       # (4 has no successors at all)


def test_constant_weights_give_the_uniform_law(pgl):
    g = pgl.Graph(edges=D.EDGES, num_nodes=D.N)
    indptr, col = g._csr_succ_sorted()
    table = g.edge_weight_table(np.full(len(D.EDGES), 3.0, np.float32), "succ")
    succ = D.successors()
    for start in W.LAW_STARTS:
        starts = np.full(W.LAW_WALKS, start)
        paths, _ = pgl.ops.host_random_walk(indptr, col, starts, W.LAW_STEPS, seed=500 + start, weights=table)
        D.assert_law(paths, D.path_law(succ, start, W.LAW_STEPS, 1.0, 1.0, "uniform"), ("constant weights", start))
        plain, _ = pgl.ops.host_random_walk(indptr, col, starts, W.LAW_STEPS, seed=500 + start)
        # with every q equal to 2^32 the pick floor(r / 2^32) of r = scale64(draw, deg * 2^32) IS scale64(draw, deg): weights
        # that are constant within every row reproduce the unweighted walk sample for sample, not only in law
        assert np.array_equal(plain, paths)
        by_row = g.edge_weight_table(np.where(D.EDGES[:, 0] == 0, 3.0, 5.0).astype(np.float32), "succ")
        assert np.array_equal(pgl.ops.host_random_walk(indptr, col, starts, W.LAW_STEPS, seed=500 + start, weights=by_row)[0], paths)


def test_exact_weighted_walk_law_host(pgl, walk_graph):
    _, indptr, col, table = walk_graph
    q = W.quantise(*_succ_weights())[0]
    sptr, scol, seid = W.succ_index(D.EDGES, D.N)
    qe = np.empty(len(q), np.int64)
    qe[seid] = q                                                   # q by original edge
    wsucc = W.weighted_successors(D.EDGES, qe, D.N)
    for start in W.LAW_STARTS:
        law = W.weighted_path_law(wsucc, start, W.LAW_STEPS)
        assert abs(sum(law.values()) - 1) < 1e-12
        uni = D.path_law(D.successors(), start, W.LAW_STEPS, 1.0, 1.0, "uniform")
        assert max(abs(law.get(k, 0) - uni.get(k, 0)) for k in set(law) | set(uni)) > 0.01      # the weights matter
        paths, _ = pgl.ops.host_random_walk(indptr, col, np.full(W.LAW_WALKS, start), W.LAW_STEPS, seed=700 + start, weights=table)
        D.assert_law(paths, law, ("weighted", start))


def _succ_weights():
    sptr, _, seid = W.succ_index(D.EDGES, D.N)
    return sptr, W.WALK_WEIGHTS, seid


def test_argument_checks(pgl, walk_graph):
    g, indptr, col, table = walk_graph
    with pytest.raises(ValueError, match="node2vec"):
        pgl.ops.host_random_walk(indptr, col, [0], 3, p=2.0, q=1.0, weights=table)
    with pytest.raises(ValueError, match="node2vec"):
        pgl.ops.host_random_walk(indptr, col, [0], 3, p=1.0, q=0.5, plus=True, weights=table)
    for f in (pgl.sampling.node2vec_walk, pgl.sampling.node2vec_walk_plus):
        with pytest.raises(ValueError, match="node2vec"):
            f(g, [0], 4, p=0.5, q=2.0, seed=1, weights="w")
        assert f(g, [0, 1], 4, p=1.0, q=1.0, seed=1, weights="w") == pgl.sampling.random_walk(g, [0, 1], 4, seed=1, weights="w")
    with pytest.raises(ValueError):
        pgl.ops.host_random_walk(indptr, col, [0], 3, weights=pgl.ops.WeightTable(table.cum[:-1], table.npos))
    with pytest.raises(ValueError):
        pgl.ops.host_random_walk(indptr, col, [D.N], 3, weights=table)
    # no weights: what it returned before
    assert pgl.sampling.random_walk(g, [0, 1, 2], 6, seed=3) == pgl.sampling.random_walk(g, [0, 1, 2], 6, seed=3, weights=None)
    sub = pgl.sampling.random_walk_subgraph(g, [0, 2], 4, seed=3, weights="w")
    assert 0 < sub.num_nodes <= D.N


# ---- alias table -------------------------------------------------------------------------------------------------------------
def _alias_distribution(accept, alias):
    accept, alias = np.asarray(accept, np.float64), np.asarray(alias, np.int64)
    n = len(accept)
    acc = np.minimum(accept, 1.0)
    p = acc.copy()
    np.add.at(p, alias, 1.0 - acc)
    return p / n


def test_alias_table_encodes_the_distribution(pgl):
    rng = np.random.default_rng(0)
    assert "alias_sample_build_table" in pgl.graph_kernel.__all__
    for n in (1, 2, 3, 7, 64, 1000):
        for probs in (rng.random(n), rng.exponential(size=n) ** 3, np.ones(n), np.eye(n)[0] * 0.5 + 0.5 / n):
            probs = probs / probs.sum()
            accept, alias = pgl.graph_kernel.alias_sample_build_table(probs)
            assert accept.dtype == np.float64 and alias.dtype == np.int64 and accept.shape == alias.shape == (n,)
            assert (accept >= 0).all() and (accept <= 1).all() and (alias >= 0).all() and (alias < n).all()
            assert np.abs(_alias_distribution(accept, alias) - probs).max() <= 1e-12


def test_alias_table_matches_the_reference_distribution(pgl, ref_native):
    rng = np.random.default_rng(1)
    for n in (1, 5, 33, 500):
        probs = rng.exponential(size=n)
        probs /= probs.sum()
        ours = _alias_distribution(*pgl.graph_kernel.alias_sample_build_table(probs))
        theirs = _alias_distribution(*ref_native.alias_sample_build_table(probs.copy()))
        assert np.abs(ours - probs).max() <= 1e-12 and np.abs(ours - theirs).max() <= 1e-12


# ---- the sampler's definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights,k,nodes", W.SAMPLER_LAW_CASES)
def test_restated_sampler_obeys_the_successive_sampling_law(weights, k, nodes):
    indptr, col, w, n = W.law_rows(weights, nodes, S.FIRST_NODE)
    cum, _ = W.table_restated(indptr, w)
    q = W.q_of(indptr, cum)[:len(weights)]
    law = W.successive_law(q, k)
    assert abs(sum(law.values()) - 1) < 1e-12 and all(q[j] > 0 for t in law for j in t)
    ids = np.arange(S.FIRST_NODE, n)
    nbr, count, eids, pos = W.sample_weighted_restated(indptr, col, None, cum, ids, k, seed=41)
    assert (count == k).all() and np.array_equal(nbr, pos) and np.array_equal(eids, np.repeat(indptr[ids], k) + pos)
    D.assert_law(pos.reshape(nodes, k), law, ("restated sampler", weights, k))


def test_restated_sampler_edge_cases():
    indptr = np.array([0, 0, 4, 9, 12], np.int64)
    w = np.array([0, 2, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0], np.float32)
    col = np.arange(12) + 100
    cum, npos = W.table_restated(indptr, w)
    assert npos.tolist() == [0, 2, 5, 0]
    nodes = np.array([2, 1, 0, 3, 2, 1])
    nbr, count, eids, pos = W.sample_weighted_restated(indptr, col, None, cum, nodes, 3, seed=7)
    assert count.tolist() == [3, 2, 0, 0, 3, 2]
    assert nbr[3:5].tolist() == [101, 103] and nbr[8:].tolist() == [101, 103]          # the positive set in row order
    assert nbr[:3].tolist() == nbr[5:8].tolist() and len(set(nbr[:3].tolist())) == 3     # a repeated node repeats its sample
    nbr, count, _, _ = W.sample_weighted_restated(indptr, col, None, cum, nodes, -1, seed=7)
    assert count.tolist() == [5, 2, 0, 0, 5, 2] and nbr[:5].tolist() == [104, 105, 106, 107, 108]
