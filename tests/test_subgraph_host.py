"""The host side of the induced subgraph (pglamd_induced_subgraph_host, graph_kernel.extract_edges_from_nodes,
sampling.induced_subgraph / ClusterBatches / random_walk_subgraph on numpy graphs) held to tests/subgraph_defs.py bit for bit."""
import numpy as np
import pytest

import sampling_defs as S
import subgraph_defs as D


@pytest.fixture(scope="module")
def pgl():
    import pgl_amd
    return pgl_amd


@pytest.fixture(scope="module")
def hub_graph():
    n = 5000
    edges = D.graph_with_hub(n, 60000, 3000)
    return edges, n, S.csr_by_dst(edges, n)


def _sets(n):
    rng = np.random.default_rng(8)
    return [("empty", np.zeros(0, np.int64)), ("1%", rng.permutation(n)[:n // 100]), ("30%", rng.permutation(n)[:n * 3 // 10]),
            ("100%", rng.permutation(n)), ("arange", np.arange(n, dtype=np.int64))]


def test_host_twin_and_extract_edges_equal_the_restatement(pgl, hub_graph):
    edges, n, (indptr, col, eid) = hub_graph
    for what, nodes in _sets(n):
        want = D.induced_restated(indptr, col, eid, nodes, n)
        got = pgl.ops.host_induced_subgraph(indptr, col, eid, nodes, n)
        for name, g, w in zip(("src", "dst", "eid"), got, want):
            assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (what, name)
        e = pgl.graph_kernel.extract_edges_from_nodes(indptr, col, eid, nodes)
        assert e.dtype == np.int64 and np.array_equal(e, want[2]), what
        assert np.array_equal(pgl.graph_kernel.extract_edges_from_nodes(indptr, col, eid, nodes.tolist()), want[2])
        pos = pgl.ops.host_induced_subgraph(indptr, col, None, nodes, n)[2]                # eid None: the position itself
        assert np.array_equal(eid[pos], want[2])
    assert "extract_edges_from_nodes" in pgl.graph_kernel.__all__


def test_extract_edges_accepts_the_src_index_too(pgl, hub_graph):
    """`whichever index the caller passes`: over adj_src_index the rows are out-edges, the definition is the same."""
    edges, n, _ = hub_graph
    g = pgl.Graph(edges=edges, num_nodes=n)
    ix = g.adj_src_index
    nodes = np.random.default_rng(2).permutation(n)[:1500]
    got = pgl.graph_kernel.extract_edges_from_nodes(ix._indptr, ix._sorted_v, ix._sorted_eid, nodes)
    want = D.induced_restated(*S.csr_by_dst(edges[:, ::-1], n), nodes, n)[2]
    assert np.array_equal(got, want)
    assert np.array_equal(np.sort(got), np.sort(D.induced_restated(*S.csr_by_dst(edges, n), nodes, n)[2]))      # the same edge SET


def test_induced_subgraph_on_a_numpy_graph_equals_subgraph_by_those_eids(pgl, hub_graph):
    edges, n, (indptr, col, eid) = hub_graph
    rng = np.random.default_rng(4)
    nf = {"h": rng.standard_normal((n, 7)).astype(np.float32), "y": rng.integers(0, 9, n)}
    ef = {"w": rng.standard_normal((len(edges), 3)).astype(np.float32), "t": np.arange(len(edges), dtype=np.int64)}
    g = pgl.Graph(edges=edges, num_nodes=n, node_feat=nf, edge_feat=ef)
    for what, nodes in _sets(n)[:4]:
        sub = pgl.sampling.induced_subgraph(g, nodes)
        want = D.induced_restated(indptr, col, eid, nodes, n)
        assert not sub.is_tensor() and sub.num_nodes == len(nodes)
        assert sub.edges.dtype == np.int64 and np.array_equal(sub.edges, np.stack([want[0], want[1]], 1)), what
        assert np.array_equal(sub.node_feat["index"], nodes)
        assert np.array_equal(sub.edge_feat["t"], want[2])
        legacy = pgl.sampling.subgraph(g, nodes, eid=want[2])
        assert np.array_equal(legacy.edges, sub.edges) and legacy.num_nodes == sub.num_nodes, what
        for k in nf:
            assert np.array_equal(legacy.node_feat[k], sub.node_feat[k]) and np.array_equal(sub.node_feat[k], nf[k][nodes])
        for k in ef:
            assert np.array_equal(legacy.edge_feat[k], sub.edge_feat[k]) and np.array_equal(sub.edge_feat[k], ef[k][want[2]])
        bare = pgl.sampling.induced_subgraph(g, nodes, with_node_feat=False, with_edge_feat=False)
        assert list(bare.node_feat) == ["index"] and not bare.edge_feat and np.array_equal(bare.edges, sub.edges)


@pytest.mark.parametrize("bad", [[3, 7, 3], [5000], [-1], [0, 1 << 40]])
def test_a_repeated_or_out_of_range_id_is_a_value_error(pgl, hub_graph, bad):
    edges, n, (indptr, col, eid) = hub_graph
    bad = np.asarray(bad, np.int64)
    with pytest.raises(ValueError):
        pgl.ops.host_induced_subgraph(indptr, col, eid, bad, n)
    with pytest.raises(ValueError):
        pgl.graph_kernel.extract_edges_from_nodes(indptr, col, eid, bad)
    with pytest.raises(ValueError):
        pgl.sampling.induced_subgraph(pgl.Graph(edges=edges, num_nodes=n), bad)
    ok = np.asarray([n - 1, 0], np.int64)                                                  # the ends of the range pass, right after
    assert np.array_equal(pgl.graph_kernel.extract_edges_from_nodes(indptr, col, eid, ok), D.induced_restated(indptr, col, eid, ok, n)[2])


def test_cluster_batches_on_a_numpy_graph(pgl, hub_graph):
    edges, n, (indptr, col, eid) = hub_graph
    g = pgl.Graph(edges=edges, num_nodes=n)
    part = np.random.default_rng(6).integers(0, 13, n)
    part[part == 5] = 4                                                                    # an empty cluster
    a, b = (pgl.sampling.ClusterBatches(g, part, clusters_per_batch=3, seed=11) for _ in range(2))
    assert len(a) == 4
    first = list(a)
    assert len(first) == 4
    seen = np.concatenate([ids for _, ids in first])
    assert np.array_equal(np.sort(seen), np.arange(n))                                     # every node in exactly one batch
    for (sub, ids), (sub_b, ids_b) in zip(first, b):
        assert np.array_equal(ids, ids_b) and np.array_equal(sub.edges, sub_b.edges)       # one seed, one order
        want = D.induced_restated(indptr, col, eid, ids, n)
        assert np.array_equal(sub.edges, np.stack([want[0], want[1]], 1)) and np.array_equal(sub.node_feat["index"], ids)
        cuts = np.flatnonzero(np.diff(part[ids]) != 0)
        assert len(cuts) <= 2 and all((np.diff(c) > 0).all() for c in np.split(ids, cuts + 1))      # cluster ranges, ascending inside
    second = list(a)                                                                       # the next epoch draws its own order
    assert np.array_equal(np.sort(np.concatenate([ids for _, ids in second])), np.arange(n))
    assert any(not np.array_equal(x[1], y[1]) for x, y in zip(first, second))
    fixed = [ids for _, ids in pgl.sampling.ClusterBatches(g, part, shuffle=False)]
    assert len(fixed) == 12 and np.array_equal(np.concatenate(fixed), np.argsort(part, kind="stable"))
    with pytest.raises(ValueError):
        pgl.sampling.ClusterBatches(g, part[:-1])


def test_random_walk_subgraph_on_a_numpy_graph(pgl, hub_graph):
    edges, n, (indptr, col, eid) = hub_graph
    g = pgl.Graph(edges=edges, num_nodes=n)
    roots = np.random.default_rng(9).integers(0, n, 200)
    sub = pgl.sampling.random_walk_subgraph(g, roots, 4, seed=5)
    ip, c = g._csr_succ_sorted()
    paths, _ = pgl.ops.host_random_walk(ip, c, roots, 4, seed=5)
    nodes = np.unique(paths[paths >= 0])
    assert len(nodes) > len(np.unique(roots)) and np.array_equal(sub.node_feat["index"], nodes)
    want = D.induced_restated(indptr, col, eid, nodes, n)
    assert np.array_equal(sub.edges, np.stack([want[0], want[1]], 1))
    again = pgl.sampling.random_walk_subgraph(g, roots, 4, seed=5)
    assert np.array_equal(again.edges, sub.edges) and np.array_equal(again.node_feat["index"], nodes)
