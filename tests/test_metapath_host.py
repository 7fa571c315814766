"""Metapath walks on the host twin (pglamd_metapath_walk_host) and on numpy-mode HeterGraphs: the single-relation identity with
the plain walks, edges and dead ends step by step, the exact law (chi-square against the definition restated in
tests/metapath_defs.py), thread independence, argument errors, the public functions and the relation-stacked index."""
import numpy as np
import pytest

import metapath_defs as M
import weighted_defs as W
from walk_defs import assert_law


@pytest.fixture(scope="module")
def pgl():
    import pgl_amd
    return pgl_amd


@pytest.fixture(scope="module")
def case(pgl):
    """(numpy HeterGraph with the weights as edge features, stacked index, stacked weight table, per-relation (indptr, col), the
    integer weight of every edge per relation in edge order)."""
    hg = pgl.HeterGraph(edges={et: M.EDGES[et] for et in M.EDGE_TYPES}, num_nodes=M.N,
                        edge_feat={et: {"w": M.WEIGHTS[et]} for et in M.EDGE_TYPES})
    stacked, number = hg._stacked_succ()
    assert number == {et: r for r, et in enumerate(M.EDGE_TYPES)}
    indices = [hg[et]._csr_succ_sorted() for et in M.EDGE_TYPES]
    tables = [hg[et].edge_weight_table("w", "succ") for et in M.EDGE_TYPES]
    q = []
    for et in M.EDGE_TYPES:
        sptr, _, seid = W.succ_index(M.EDGES[et], M.N)
        qe = np.empty(len(M.EDGES[et]), np.int64)
        qe[seid] = W.quantise(sptr, M.WEIGHTS[et], seid)[0]
        q.append(qe)
    return hg, stacked, pgl.ops.stack_weight_tables(tables), indices, tables, q


def _positive_edge_sets(q):
    return [set(map(tuple, e[qe > 0].tolist())) for e, qe in zip(M.edge_lists(), q)]


# ---- 1. single-relation identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [5, 2 ** 40 + 7])
def test_one_relation_metapath_is_the_plain_walk(pgl, case, seed):
    _, stacked, table, indices, tables, _ = case
    starts = np.arange(3000) % M.N
    for r in (0, 1, 2):
        indptr, col = indices[r]
        want = pgl.ops.host_random_walk(indptr, col, starts, 9, seed=seed)
        got = pgl.ops.host_metapath_walk(stacked, starts, [r], 9, seed=seed)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        want = pgl.ops.host_random_walk(indptr, col, starts, 9, seed=seed, weights=tables[r])
        got = pgl.ops.host_metapath_walk(stacked, starts, [r], 9, seed=seed, weights=table)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[1] == 10).any()                                    # (p2p has cycles: the identity is not one of dead ends alone)


# ---- 2. edges and dead ends --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4, 5])
def test_every_step_is_an_edge_of_its_relation(pgl, case, L):
    _, stacked, table, _, _, q = case
    mp = M.METAPATHS[L]
    starts = np.arange(2400) % M.N
    for phase in (0, L - 1):
        paths, lengths = pgl.ops.host_metapath_walk(stacked, starts, mp, 9, phase=phase, seed=3 + phase)
        assert paths.shape == (2400, 10) and paths.dtype == np.int64 and lengths.dtype == np.int64
        assert np.array_equal(paths[:, 0], starts)
        assert M.follows(paths, lengths, M.edge_sets(), mp, phase)
        paths, lengths = pgl.ops.host_metapath_walk(stacked, starts, mp, 9, phase=phase, seed=3 + phase, weights=table)
        assert M.follows(paths, lengths, _positive_edge_sets(q), mp, phase)
    paths, lengths = pgl.ops.host_metapath_walk(stacked, starts, mp, 9, seed=3)
    assert (lengths < 10).any() and (lengths == 10).any()          # dead ends met, full-length walks too
    assert not M.follows(paths, lengths, M.edge_sets(), mp, 1)     # (the check tells one phase from another)


def test_dead_ends_of_the_relation_and_of_the_node(pgl, case):
    _, stacked, _, _, _, _ = case
    starts = np.array([2] * 4000 + [3, 9, 11], np.int64)
    paths, lengths = pgl.ops.host_metapath_walk(stacked, starts, [0, 1], 6, seed=8)
    at7 = paths[:4000, 1] == 7                                    # 2 -a2p-> 7, and 7 has no p2a successor (but p2p ones)
    assert at7.any() and (lengths[:4000][at7] == 2).all() and (paths[:4000][at7][:, 2:] == -1).all()
    assert (lengths[:4000][~at7] > 2).all()
    assert lengths[4000:].tolist() == [1, 1, 1] and (paths[4000:, 1:] == -1).all()     # no a2p successors: the start alone
    paths, lengths = pgl.ops.host_metapath_walk(stacked, starts, [0, 3], 6, seed=8)     # p2v has no edges
    assert (lengths[:4000] == 2).all() and (paths[:, 2:] == -1).all()


def test_zero_steps_and_no_starts(pgl, case):
    _, stacked, table, _, _, _ = case
    starts = np.array([0, 7, 11, 3], np.int64)
    for weights in (None, table):
        paths, lengths = pgl.ops.host_metapath_walk(stacked, starts, [0, 1], 0, seed=1, weights=weights)
        assert paths.tolist() == [[0], [7], [11], [3]] and lengths.tolist() == [1, 1, 1, 1]
        paths, lengths = pgl.ops.host_metapath_walk(stacked, np.zeros(0, np.int64), [0, 1], 5, seed=1, weights=weights)
        assert paths.shape == (0, 6) and lengths.shape == (0,)


# ---- 3. exact law ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3])
def test_exact_metapath_law(pgl, case, L):
    _, stacked, table, _, _, q = case
    mp = M.METAPATHS[L]
    for start in M.LAW_STARTS:
        starts = np.full(M.LAW_WALKS, start, np.int64)
        paths, _ = pgl.ops.host_metapath_walk(stacked, starts, mp, M.LAW_STEPS, seed=100 * L + start)
        assert_law(paths, M.path_law(M.successors(), start, M.LAW_STEPS, mp), ("host uniform", L, start))
        paths, _ = pgl.ops.host_metapath_walk(stacked, starts, mp, M.LAW_STEPS, seed=150 * L + start, weights=table)
        assert_law(paths, M.path_law(M.successors(q), start, M.LAW_STEPS, mp), ("host weighted", L, start))
        assert not ((paths[:, 0] == 0) & (paths[:, 1] == 5)).any()     # 0 -> 5 carries weight zero: never followed
    # phase L - 1 is the metapath rotated; its first relation is p2a, so the walkers start at a paper
    paths, _ = pgl.ops.host_metapath_walk(stacked, np.full(M.LAW_WALKS, 5, np.int64), mp, M.LAW_STEPS, phase=L - 1, seed=77)
    assert_law(paths, M.path_law(M.successors(), 5, M.LAW_STEPS, mp[L - 1:] + mp[:L - 1]), ("host phase", L))
    assert_law(paths, M.path_law(M.successors(), 5, M.LAW_STEPS, mp, L - 1), ("host phase, by the phase argument", L))


# ---- 4. thread independence --------------------------------------------------------------------------------------------------
def test_host_threads_do_not_change_the_walks(pgl, case):
    _, stacked, table, _, _, _ = case
    starts = np.arange(20000) % M.N
    for weights in (None, table):
        one = pgl.ops.host_metapath_walk(stacked, starts, M.METAPATHS[5], 12, phase=2, seed=9, weights=weights, threads=1)
        for threads in (3, 16):
            many = pgl.ops.host_metapath_walk(stacked, starts, M.METAPATHS[5], 12, phase=2, seed=9, weights=weights, threads=threads)
            assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors(pgl, case):
    _, stacked, table, _, _, _ = case
    starts = np.array([0, 1], np.int64)
    R = stacked.num_relations
    assert R == 4
    for mp, phase, steps in (([], 0, 3), ([0] * 65, 0, 3), ([0, R], 0, 3), ([0, -1], 0, 3), ([0, 1], 2, 3), ([0, 1], -1, 3), ([0, 1], 0, -1),
                             ([0, 1], 0, -2)):
        with pytest.raises(ValueError, match=r"pgl_amd metapath_walk_host: .*\(code -6\)"):        # PGLAMD_E_ARG, the library's message
            pgl.ops.host_metapath_walk(stacked, starts, mp, steps, phase=phase)
    assert pgl.ops.host_metapath_walk(stacked, starts, [0] * 64, 3, phase=63)[0].shape == (2, 4)       # the longest legal metapath
    for bad in (M.N, -1):
        with pytest.raises(ValueError, match="start nodes outside"):
            pgl.ops.host_metapath_walk(stacked, np.array([0, bad], np.int64), [0, 1], 3)
        paths, lengths = pgl.ops.host_metapath_walk(stacked, np.array([0, bad], np.int64), [0, 1], 3, check_range=False)
        assert paths[1].tolist() == [bad, -1, -1, -1] and lengths[1] == 1 and lengths[0] > 1    # the walk of the start alone
    with pytest.raises(ValueError, match="WeightTable"):
        pgl.ops.host_metapath_walk(stacked, starts, [0, 1], 3, weights=case[4][0])                # one relation's table alone
    with pytest.raises(TypeError):
        pgl.ops.host_metapath_walk(stacked, starts, [0, 1], 3, weights=M.WEIGHTS["a2p"])


# ---- 6. public functions on a numpy HeterGraph -------------------------------------------------------------------------------
def test_metapath_randomwalk_on_a_numpy_graph(pgl, case):
    hg, stacked, table, _, _, q = case
    nodes = list(range(M.N)) * 40
    a = pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2p-p2p-p2a", 8, seed=4)
    b = pgl.sampling.metapath_randomwalk(hg, np.asarray(nodes), ["a2p", "p2p", "p2p", "p2a"], 8, None, None, seed=4)
    assert a == b and [w[0] for w in a] == nodes and max(map(len, a)) == 8 and min(map(len, a)) == 1
    paths, lengths = pgl.ops.host_metapath_walk(stacked, nodes, M.METAPATHS[4], 7, seed=4)
    assert a == [row[:n].tolist() for row, n in zip(paths, lengths)]                          # walk_length nodes = walk_length - 1 steps
    assert pgl.sampling.metapath_randomwalk(hg, [], "a2p-p2a", 8) == []
    assert pgl.sampling.metapath_randomwalk(hg, [0, 5], "a2p-p2a", 1, seed=1) == [[0], [5]]
    assert pgl.sampling.metapath_randomwalk(hg, [0, 5], "a2p-p2a", 0, seed=1) == [[0], [5]]
    np.random.seed(11); c = pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2a", 8)
    np.random.seed(11); d = pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2a", 8)
    np.random.seed(12); e = pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2a", 8)
    assert c == d and c != e
    for bad in ("a2p-p2x", ["a2p", "cites"], "", []):
        with pytest.raises(ValueError, match="metapath"):
            pgl.sampling.metapath_randomwalk(hg, nodes, bad, 8, seed=1)
    with pytest.raises(ValueError, match="p2x"):
        pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2x", 8, seed=1)
    with pytest.raises(ValueError):
        pgl.sampling.metapath_randomwalk(hg, [M.N], "a2p-p2a", 8, seed=1)
    with pytest.raises(ValueError, match="tensor-mode"):
        pgl.sampling.metapath_walks(hg, nodes, "a2p-p2a", 8, seed=1)
    # weights: a dict over the metapath's edge types -- names, arrays in edge order and tables all mean the same walk
    with pytest.raises(ValueError, match="p2a"):
        pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2a", 8, seed=1, weights={"a2p": "w"})
    with pytest.raises(ValueError, match="dict"):
        pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2a", 8, seed=1, weights="w")
    w1 = pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2a", 8, seed=6, weights={"a2p": "w", "p2a": "w"})
    w2 = pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2a", 8, seed=6,
                                          weights={"a2p": M.WEIGHTS["a2p"], "p2a": hg["p2a"].edge_weight_table("w", "succ"), "p2p": "w"})
    paths, lengths = pgl.ops.host_metapath_walk(stacked, nodes, [0, 1], 7, seed=6, weights=table)
    assert w1 == w2 == [row[:n].tolist() for row, n in zip(paths, lengths)] and w1 != pgl.sampling.metapath_randomwalk(hg, nodes, "a2p-p2a", 8, seed=6)
    assert M.follows(paths, lengths, _positive_edge_sets(q), [0, 1])


def test_walktimes_on_a_numpy_graph(pgl, case):
    hg = case[0]
    starts = list(range(M.N)) * 6
    for names, length, times in ((["a2p", "p2a"], 7, 2), (["a2p", "p2p", "p2a"], 6, 10), (["p2p"], 5, 1), (["a2p", "p2a"], 2, 3)):
        np.random.seed(5)
        walks = pgl.sampling.metapath_randomwalk_with_walktimes(hg, starts, "-".join(names), length, walk_times=times, seed=2)
        M.walktimes_properties(walks, starts, names, length, times)
        np.random.seed(5)
        assert walks == pgl.sampling.metapath_randomwalk_with_walktimes(hg, starts, names, length, times, None, None, seed=2)
    assert max(map(len, walks)) == 2
    assert pgl.sampling.metapath_randomwalk_with_walktimes(hg, [], "a2p-p2a", 5) == []
    assert pgl.sampling.metapath_randomwalk_with_walktimes(hg, [3, 9, 11], "a2p-p2a", 5) == []      # no a2p successors anywhere
    with pytest.raises(ValueError, match="p2x"):
        pgl.sampling.metapath_randomwalk_with_walktimes(hg, starts, "a2p-p2x", 5)


# ---- 7. the stacked index ----------------------------------------------------------------------------------------------------
def test_stacked_index_round_trips(pgl, case):
    hg, stacked, table, indices, tables, _ = case
    R = len(M.EDGE_TYPES)
    assert stacked.indptr.shape == (R, M.N + 1) and stacked.indptr.dtype == np.int64 and stacked.indptr.flags["C_CONTIGUOUS"]
    assert stacked.col.dtype == np.int32 and stacked.num_nodes == M.N and stacked.num_relations == R
    assert list(stacked.edge_base) == np.concatenate([[0], np.cumsum([len(M.EDGES[et]) for et in M.EDGE_TYPES])]).tolist()
    for r, (indptr, col) in enumerate(indices):
        lo, hi = stacked.edge_base[r], stacked.edge_base[r + 1]
        assert np.array_equal(stacked.indptr[r] - lo, indptr) and np.array_equal(stacked.col[lo:hi], col)
        assert np.array_equal(table.cum[lo:hi], tables[r].cum) and np.array_equal(table.npos[r * M.N:(r + 1) * M.N], tables[r].npos)
        sptr, scol, _ = W.succ_index(M.EDGES[M.EDGE_TYPES[r]], M.N)
        assert np.array_equal(indptr, sptr) and np.array_equal(col, scol)                 # rows ascending by dst
    again = pgl.ops.host_stack_relations(indices)
    assert np.array_equal(again.indptr, stacked.indptr) and np.array_equal(again.col, stacked.col) and again.edge_base == stacked.edge_base
    assert hg._stacked_succ()[0] is stacked                                               # cached
    with pytest.raises(ValueError):
        pgl.ops.host_stack_relations([])
    with pytest.raises(ValueError):
        pgl.ops.host_stack_relations([indices[0], (indices[1][0][:-1], indices[1][1])])
