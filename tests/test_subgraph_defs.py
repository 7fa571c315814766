"""tests/subgraph_defs.py held to two independent statements of the same thing: a brute-force mask over the edge list (no index
involved) and the reference's own compiled graph_kernel.extract_edges_from_nodes (where the oracle has built it)."""
import numpy as np
import pytest

import sampling_defs as S
import subgraph_defs as D


def _node_sets(n, rng):
    yield "empty", np.zeros(0, np.int64)
    yield "one", np.asarray([int(rng.integers(0, n))], np.int64)
    for frac in (0.1, 0.5, 1.0):
        yield "shuffled %.0f%%" % (100 * frac), rng.permutation(n)[:max(1, int(n * frac))].astype(np.int64)
    yield "arange", np.arange(n, dtype=np.int64)
    yield "descending", np.arange(n, dtype=np.int64)[::-1].copy()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_the_brute_force_mask(seed):
    edges, n = D.small_multigraph(seed=seed)
    assert len(np.unique(edges[:, 0] * n + edges[:, 1])) < len(edges) and (edges[:, 0] == edges[:, 1]).any()
    indptr, col, eid = S.csr_by_dst(edges, n)
    for what, nodes in _node_sets(n, np.random.default_rng(seed)):
        got = D.induced_restated(indptr, col, eid, nodes, n)
        loop = D.induced_loop(indptr, col, eid, nodes, n)
        want = D.induced_brute_force(edges, nodes, n)
        for name, g, l, w in zip(("src", "dst", "eid"), got, loop, want):
            assert g.dtype == np.int64 and np.array_equal(g, w), (what, name, g[:8], w[:8])
            assert np.array_equal(l, w), (what, name, "loop form")
        assert (np.diff(got[1]) >= 0).all(), what                                  # grouped by dst_local, non-decreasing
        assert np.array_equal(nodes[got[0]], edges[got[2], 0]) and np.array_equal(nodes[got[1]], edges[got[2], 1])
        if what in ("arange", "shuffled 100%", "descending"):
            assert len(got[2]) == len(edges) and len(np.unique(got[2])) == len(edges)      # every edge once: multiplicity kept
        if what == "arange":
            assert np.array_equal(got[2], eid) and np.array_equal(got[0], col)


def test_self_loops_and_multi_edges_are_kept():
    edges = np.asarray([[2, 2], [1, 2], [1, 2], [2, 1], [0, 1], [2, 2]], np.int64)
    indptr, col, eid = S.csr_by_dst(edges, 4)
    src, dst, eids = D.induced_restated(indptr, col, eid, [2, 1], 4)
    assert eids.tolist() == [0, 1, 2, 5, 3] and src.tolist() == [0, 1, 1, 0, 0] and dst.tolist() == [0, 0, 0, 0, 1]
    src, dst, eids = D.induced_restated(indptr, col, eid, [3], 4)
    assert len(eids) == 0 and eids.dtype == np.int64


@pytest.mark.parametrize("bad", [[1, 1], [0, 4], [-1], [2, 1 << 40]])
def test_restatement_refuses_repeated_and_out_of_range_ids(bad):
    indptr, col, eid = S.csr_by_dst(np.asarray([[0, 1], [1, 2]], np.int64), 4)
    for fn in (D.induced_restated, D.induced_loop):
        with pytest.raises(ValueError):
            fn(indptr, col, eid, bad, 4)


def test_restatement_equals_the_references_extract_edges_from_nodes(ref_native):
    n = 5000
    edges = D.graph_with_hub(n, 60000, 3000)
    indptr, col, eid = S.csr_by_dst(edges, n)
    assert np.diff(indptr).max() >= 3000
    rng = np.random.default_rng(3)
    for frac in (0.01, 0.3, 1.0):
        nodes = rng.permutation(n)[:int(n * frac)].astype(np.int64)
        want = np.asarray(ref_native.extract_edges_from_nodes(indptr, col, eid, nodes.tolist()), np.int64)
        got = D.induced_restated(indptr, col, eid, nodes, n)[2]
        assert len(want) > 0 and np.array_equal(got, want), (frac, len(got), len(want))
