"""Relation-wise neighbour sampling on the host twin (pglamd_sample_relations_host) and on numpy-mode HeterGraphs: bit equality
with the definition restated in tests/relation_sampling_defs.py for thread counts 1 and 7, the stacked predecessor index, the shared
relabel, RelationNeighborSampler's blocks edge by edge, the argument errors, and the reference's HeteroNeighborSampler stub."""
import numpy as np
import pytest

import relation_sampling_defs as RS


@pytest.fixture(scope="module")
def pgl():
    import pgl_amd
    return pgl_amd


@pytest.fixture(scope="module")
def case(pgl):
    """(numpy HeterGraph, its stacked predecessor index, the per-relation (indptr, col, eid) restated, the edge lists)."""
    edges = RS.fixture_edges()
    hg = pgl.HeterGraph(edges={et: edges[et] for et in RS.EDGE_TYPES}, num_nodes=RS.N)
    stacked, number = hg._stacked_pred()
    assert number == {et: r for r, et in enumerate(RS.EDGE_TYPES)}
    return hg, stacked, RS.fixture_csrs(edges), edges


def _equal(got, want):
    nbr, dst, count, split, eids = want
    assert got.neighbors.dtype == got.dst.dtype == got.count.dtype == np.int64
    assert np.array_equal(got.neighbors, nbr) and np.array_equal(got.dst, dst) and np.array_equal(got.count, count)
    assert tuple(got.edge_split) == tuple(split) and all(isinstance(s, int) for s in got.edge_split)
    assert got.eids is not None and got.eids.dtype == np.int64 and np.array_equal(got.eids, eids)


# ---- 1. the stacked index ---------------------------------------------------------------------------------------------------------
def test_stacked_index_matches_the_relations(pgl, case):
    hg, stacked, csrs, edges = case
    assert isinstance(stacked, pgl.ops.StackedIndex) and stacked.num_relations == 4 and stacked.num_nodes == RS.N
    assert stacked.indptr.dtype == np.int64 and stacked.indptr.shape == (4, RS.N + 1)
    assert stacked.col.dtype == np.int32 and stacked.eid.dtype == np.int32
    assert tuple(stacked.edge_base) == tuple(np.concatenate([[0], np.cumsum([len(edges[et]) for et in RS.EDGE_TYPES])]).tolist())
    for r, (indptr, col, eid) in enumerate(csrs):
        a, b = stacked.edge_base[r], stacked.edge_base[r + 1]
        assert np.array_equal(stacked.indptr[r], indptr + a)
        assert np.array_equal(stacked.col[a:b], col) and np.array_equal(stacked.eid[a:b], eid)      # relation-LOCAL edge ids
    again = pgl.ops.host_stack_indices([(p, c, e) for p, c, e in csrs])
    assert all(np.array_equal(x, y) for x, y in zip(again[:3], stacked[:3])) and again[3:] == stacked[3:]
    assert hg._stacked_pred()[0] is stacked                                                          # cached
    with pytest.raises(ValueError):
        pgl.ops.host_stack_indices([])
    with pytest.raises(ValueError):
        pgl.ops.host_stack_indices([csrs[0], (csrs[1][0][:-1], csrs[1][1], csrs[1][2])])


def test_relation_seed_is_the_definition(pgl):
    for seed in (0, 1, 12345, 2 ** 63 + 5, -1):
        for r in (0, 1, 3, 63):
            assert pgl.ops.relation_seed(seed, r) == RS.relation_seed(seed, r)
    assert len({pgl.ops.relation_seed(9, r) for r in range(64)}) == 64


# ---- 2. bit equality with the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 7])
@pytest.mark.parametrize("seed", [0, 2 ** 63 + 5])
def test_host_twin_equals_the_restatement(pgl, case, threads, seed):
    _, stacked, csrs, _ = case
    nodes = RS.fixture_seeds()
    assert len(nodes) * 4 > 7 * 1024                                   # (enough slots for the seven threads to share)
    want = RS.sample_relations_restated(csrs, nodes, RS.FANOUTS, seed)
    got = pgl.ops.host_sample_neighbors_relations(stacked, nodes, RS.FANOUTS, seed=seed, return_eids=True, threads=threads)
    _equal(got, want)
    count = want[2]
    assert (count[2] == 0).all() and count[1].max() == 300 and count[3].max() == 64 and count[0].max() == 5     # empty / whole rows / cut rows
    assert want[3][2] == want[3][3]                                    # the fan-out-0 relation owns an empty range
    plain = pgl.ops.host_sample_neighbors_relations(stacked, nodes, RS.FANOUTS, seed=seed, threads=threads)
    assert plain.eids is None and np.array_equal(plain.neighbors, want[0])


@pytest.mark.parametrize("n", [0, 1])
def test_no_seed_and_one_seed(pgl, case, n):
    _, stacked, csrs, _ = case
    nodes = RS.fixture_seeds(n)
    got = pgl.ops.host_sample_neighbors_relations(stacked, nodes, RS.FANOUTS, seed=4, return_eids=True)
    _equal(got, RS.sample_relations_restated(csrs, nodes, RS.FANOUTS, 4))
    assert got.count.shape == (4, n) and len(got.edge_split) == 5


def test_every_relation_is_the_single_relation_sampler(pgl, case):
    """Relation r of the fused sampler == the restated single-relation sampler over relation r alone with relation_seed(seed, r)."""
    import sampling_defs as S
    _, stacked, csrs, _ = case
    nodes = RS.fixture_seeds()
    got = pgl.ops.host_sample_neighbors_relations(stacked, nodes, [5, 5, 5, 5], seed=31, return_eids=True)
    for r, (indptr, col, eid) in enumerate(csrs):
        nbr, count, eids = S.sample_restated(indptr, col, eid, nodes, 5, pgl.ops.relation_seed(31, r))
        a, b = got.edge_split[r], got.edge_split[r + 1]
        assert np.array_equal(got.neighbors[a:b], nbr) and np.array_equal(got.count[r], count) and np.array_equal(got.eids[a:b], eids)


# ---- 3. the shared relabel ------------------------------------------------------------------------------------------------------
def test_reindex_heter_graph_is_the_restatement(pgl, case):
    _, stacked, csrs, _ = case
    nodes = RS.fixture_seeds(400)
    s = pgl.ops.host_sample_neighbors_relations(stacked, nodes, RS.FANOUTS, seed=2)
    parts = [s.neighbors[s.edge_split[r]:s.edge_split[r + 1]] for r in range(4)]
    src, dst, out_nodes = pgl.ops.reindex_heter_graph(nodes, parts, list(s.count))
    want = RS.reindex_heter_restated(nodes, parts, list(s.count))
    assert all(np.array_equal(g, w) and g.dtype == np.int64 for g, w in zip((src, dst, out_nodes), want))
    assert np.array_equal(out_nodes[:400], nodes) and np.array_equal(dst, s.dst)
    assert np.array_equal(out_nodes[src], s.neighbors)
    first = {}
    for p, v in enumerate(out_nodes.tolist()):
        first.setdefault(v, p)
    assert np.array_equal(src, [first[v] for v in s.neighbors.tolist()])          # a neighbour equal to a seed: that seed's FIRST position
    assert (src < 400).any() and (src >= 400).any()
    with pytest.raises(ValueError):
        pgl.ops.reindex_heter_graph(nodes, parts, list(s.count)[:3])
    with pytest.raises(ValueError):
        pgl.ops.reindex_heter_graph(nodes, [np.array([-1], np.int64)], [np.array([1] + [0] * 399, np.int64)])


# ---- 4. the public sampler on a numpy HeterGraph --------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [[[5, -1, 0, 64], [3, 2, 0, 4]], [{"cites": 5, "writes": -1, "topic": 64}, 2]])
def test_sampler_blocks_on_a_numpy_graph(pgl, case, samples):
    hg, _, csrs, edges = case
    batch = RS.fixture_seeds(120)
    sampler = pgl.sampling.RelationNeighborSampler(hg, samples, seed=11, with_eids=True)
    graph_list, nodes = sampler.sample_neighbors(batch)
    assert len(graph_list) == 2 and isinstance(nodes, np.ndarray)
    fan = sampler.samples
    if isinstance(samples[0], dict):
        assert fan == [[5, -1, 0, 64], [2, 2, 2, 2]]                   # a missing edge type means 0; an int serves every edge type
    # graph_list is outermost first.  The outer block's node set is the returned one; its first n_dst entries are its frontier,
    # which is the inner block's whole node set.
    node_sets = [nodes[:graph_list[0][1]], nodes]
    frontiers = [batch, node_sets[0]]
    for layer in (0, 1):
        block, n_dst = graph_list[1 - layer]
        out_nodes, frontier = node_sets[layer], frontiers[layer]
        assert isinstance(block, pgl.HeterGraph) and not block.is_tensor() and block.edge_types == RS.EDGE_TYPES
        assert n_dst == len(frontier) and int(block.num_nodes) == len(out_nodes)
        assert np.array_equal(out_nodes[:n_dst], frontier)             # the first n_dst rows are the frontier as given (repeats kept)
        assert len(np.unique(out_nodes[n_dst:])) == len(out_nodes) - n_dst and not np.isin(out_nodes[n_dst:], frontier).any()
        for r, et in enumerate(RS.EDGE_TYPES):
            g = block[et]
            assert g.num_nodes == len(out_nodes) and g.edges.dtype == np.int64 and g.edges.shape[1] == 2
            indptr = csrs[r][0]
            deg, f = indptr[frontier + 1] - indptr[frontier], fan[layer][r]
            want = np.zeros_like(deg) if f == 0 else (deg if f < 0 else np.minimum(deg, f))
            assert (g.edges[:, 1] < n_dst).all() and (np.diff(g.edges[:, 1]) >= 0).all()          # dst-sorted by construction
            assert np.array_equal(np.bincount(g.edges[:, 1], minlength=n_dst), want)               # counts == min(deg, f)
            assert g.num_edges == int(want.sum()) and (f != 0 or g.num_edges == 0)
            # every block edge, mapped back through the node set, is the edge of THIS relation its id names, entering that frontier node
            orig = edges[et][g.edge_feat["eid"]]
            assert np.array_equal(orig[:, 0], out_nodes[g.edges[:, 0]]) and np.array_equal(orig[:, 1], frontier[g.edges[:, 1]])
            for v in np.unique(g.edges[:, 1]):                         # without replacement: no edge id twice under one frontier row
                e = g.edge_feat["eid"][g.edges[:, 1] == v]
                assert len(np.unique(e)) == len(e)


def test_sampler_is_deterministic_and_advances_its_seed(pgl, case):
    hg = case[0]
    batch = RS.fixture_seeds(64)
    a, b = (pgl.sampling.RelationNeighborSampler(hg, [3, 3], seed=5) for _ in range(2))
    ga, na = a.sample_neighbors(batch)
    gb, nb = b.sample_neighbors(batch)
    assert np.array_equal(na, nb)
    for (x, nx), (y, ny) in zip(ga, gb):
        assert nx == ny and all(np.array_equal(x[et].edges, y[et].edges) for et in RS.EDGE_TYPES)
    assert "eid" not in ga[0][0]["cites"].edge_feat
    ga2, _ = a.sample_neighbors(batch)                                 # the same sampler again: later seeds, other picks
    assert not all(np.array_equal(ga[1][0][et].edges, ga2[1][0][et].edges) for et in RS.EDGE_TYPES)


# ---- 5. argument errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors(pgl, case):
    hg, stacked, _, _ = case
    nodes = RS.fixture_seeds(10)
    f = pgl.ops.host_sample_neighbors_relations
    with pytest.raises(ValueError, match="kMaxSample"):
        f(stacked, nodes, [5, 65, 0, 1])
    with pytest.raises(ValueError, match="fan-outs"):
        f(stacked, nodes, [5, 5, 5])
    for bad in ([0, RS.N], [-1, 3]):
        with pytest.raises(ValueError, match="outside"):
            f(stacked, np.array(bad, np.int64), RS.FANOUTS)
    for samples in ([[5, 65, 0, 1]], [[5, 5]], [{"nope": 3}], [65]):
        with pytest.raises(ValueError):
            pgl.sampling.RelationNeighborSampler(hg, samples)
    with pytest.raises(ValueError, match="outside"):
        pgl.sampling.RelationNeighborSampler(hg, [2]).sample_neighbors(np.array([RS.N], np.int64))
    with pytest.raises(TypeError):
        pgl.sampling.RelationNeighborSampler(hg, [2], weights="w")           # edge-weighted relational sampling is not provided


def test_hetero_neighbor_sampler_stays_the_reference_stub(pgl):
    with pytest.raises(NotImplementedError):
        pgl.sampling.HeteroNeighborSampler([], [])
