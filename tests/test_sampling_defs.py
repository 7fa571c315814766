"""tests/sampling_defs.py checked on its own, without a GPU: the Floyd restatement obeys the exact subset law, the relabel
restatement agrees with a dictionary loop (repeated seeds included), and the chi-square check refuses impossible rows."""
from itertools import combinations

import numpy as np
import pytest

import sampling_defs as S


def test_mix64_is_splitmix64():
    # the first outputs of splitmix64 from state 0 are mix64 of 0, of the increment, of twice the increment (the finaliser adds one more)
    g = 0x9E3779B97F4A7C15
    got = [int(S.mix64(np.uint64((i * g) & 0xFFFFFFFFFFFFFFFF))) for i in range(3)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert S.mix64(np.array([0, 1], np.uint64)).dtype == np.uint64


@pytest.mark.parametrize("seed", [0, 2 ** 40 + 3])
@pytest.mark.parametrize("deg,k,W", S.SUBSET_CASES)
def test_restated_floyd_obeys_the_subset_law(deg, k, W, seed):
    edges, n, _ = S.law_graph(deg, W)
    indptr, col, _ = S.csr_by_dst(edges, n)
    nodes = np.arange(S.FIRST_NODE, S.FIRST_NODE + W, dtype=np.int64)
    nbr, count, eids = S.sample_restated(indptr, col, None, nodes, k, seed)
    assert (count == k).all() and np.array_equal(nbr, col[eids])
    picks = (eids - np.repeat(indptr[nodes], count)).reshape(W, k)
    S.assert_subset_law(picks, deg, k, "restated seed %d" % seed)


def test_restated_sampler_structure():
    rng = np.random.default_rng(3)
    n, e = 300, 3000
    edges = np.stack([rng.integers(0, n, e), rng.integers(0, n, e) // 2 * 2], 1)     # odd nodes have no in-edges
    indptr, col, eid = S.csr_by_dst(edges, n)
    nodes = rng.integers(0, n, 500)
    deg = np.bincount(edges[:, 1], minlength=n)[nodes]
    for k in (-1, 0, 1, 3, 10, 64):
        nbr, count, eids = S.sample_restated(indptr, col, eid, nodes, k, 11)
        assert np.array_equal(count, deg if k < 0 else np.minimum(deg, k))
        assert np.array_equal(edges[eids, 0], nbr) and np.array_equal(edges[eids, 1], np.repeat(nodes, count))
        off = np.concatenate([[0], np.cumsum(count)])
        for i in range(len(nodes)):
            row = eids[off[i]:off[i + 1]]
            assert len(set(row.tolist())) == len(row)
            if k < 0 or deg[i] <= k:
                assert np.array_equal(row, eid[indptr[nodes[i]]:indptr[nodes[i] + 1]])          # copied in row order
        # a node's draws depend on (seed, node id, draw number) only: the same rows whatever the node's place in the batch
        nbr1, count1, _ = S.sample_restated(indptr, col, eid, nodes[::-1], k, 11)
        off1 = np.concatenate([[0], np.cumsum(count1)])
        assert all(np.array_equal(nbr1[off1[len(nodes) - 1 - i]:off1[len(nodes) - i]], nbr[off[i]:off[i + 1]]) for i in range(0, 500, 7))
        assert not (0 < k < deg.max()) or not np.array_equal(S.sample_restated(indptr, col, eid, nodes, k, 12)[0], nbr)
    # eid=None: the position itself
    assert np.array_equal(S.sample_restated(indptr, col, None, nodes, 3, 11)[0], S.sample_restated(indptr, col, eid, nodes, 3, 11)[0])


def _reindex_by_dictionary(nodes, neighbors, count):
    ident = {}
    for p, v in enumerate(nodes):
        ident.setdefault(v, p)
    out = list(nodes)
    for v in neighbors:
        if v not in ident:
            ident[v] = len(out); out.append(v)
    return [ident[v] for v in neighbors], [i for i, c in enumerate(count) for _ in range(c)], out


REINDEX_SMALL = [([5, 5, 7], [7, 9, 5, 9, 3], [2, 0, 3]),                # repeated seeds: 5 maps to position 0, 9 and 3 are new
                 ([4, 2, 9], [9, 9, 9, 4], [1, 1, 2]),                    # every neighbour already a seed, one at a later position
                 ([1, 2], [], [0, 0]), ([], [3, 3, 8], []), ([], [], []),
                 ([7, 7, 7, 7], [7, 1 << 40, 7, 1 << 40, 0], [5, 0, 0, 0]),
                 ([3, 1, 3, 1, 2], [8, 2, 8, 1, 3, 6], [1, 1, 1, 1, 2])]


@pytest.mark.parametrize("nodes,neighbors,count", REINDEX_SMALL)
def test_reindex_restated_agrees_with_a_dictionary_loop(nodes, neighbors, count):
    src, dst, out = S.reindex_restated(nodes, neighbors, count)
    w_src, w_dst, w_out = _reindex_by_dictionary(nodes, neighbors, count)
    assert src.tolist() == w_src and dst.tolist() == w_dst and out.tolist() == w_out
    assert src.dtype == dst.dtype == out.dtype == np.int64
    assert out[:len(nodes)].tolist() == list(nodes) and out[src].tolist() == list(neighbors)


def test_reindex_restated_random_against_the_dictionary_loop():
    rng = np.random.default_rng(8)
    for n, m, hi in ((50, 400, 60), (200, 1000, 150), (1, 33, 5), (40, 0, 10)):
        nodes, neighbors = rng.integers(0, hi, n), rng.integers(0, hi * 2, m)
        count = np.bincount(rng.integers(0, n, m), minlength=n)
        src, dst, out = S.reindex_restated(nodes, neighbors, count)
        w = _reindex_by_dictionary(nodes.tolist(), neighbors.tolist(), count.tolist())
        assert (src.tolist(), dst.tolist(), out.tolist()) == w


def test_subset_law_chi2_refuses_impossible_rows_and_sees_a_skewed_law():
    with pytest.raises(AssertionError):
        S.subset_law_chi2(np.array([[0, 1], [2, 2]]), 4, 2)              # a position drawn twice
    with pytest.raises(AssertionError):
        S.subset_law_chi2(np.array([[0, 1], [2, 4]]), 4, 2)              # out of range
    stat, dof = S.subset_law_chi2(np.array(list(combinations(range(5), 2)) * 3), 5, 2)
    assert stat == 0.0 and dof == 9
    # uniform marginals, wrong joint law: only the 5 "cyclic neighbour" pairs {i, i + 1 mod 5} ever occur
    rng = np.random.default_rng(0)
    i = rng.integers(0, 5, 20000)
    picks = np.stack([i, (i + 1) % 5], 1)
    assert np.allclose(np.bincount(picks.ravel(), minlength=5) / 40000.0, 0.2, atol=0.01)
    from scipy.stats import chi2
    stat, dof = S.subset_law_chi2(picks, 5, 2)
    assert chi2.sf(stat, dof) < 1e-100
