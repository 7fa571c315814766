"""Relation-wise neighbour sampling on the MI355X (sampling_rel.hip) held to its definition, restated in numpy in
tests/relation_sampling_defs.py: device == host twin == restatement bit for bit (more slots than one block, whole-row copies longer
than a wave), every relation == ops.sample_neighbors over that relation alone, the shared relabel, the independence of two
relations that hold the same rows, RelationNeighborSampler's blocks under send_recv and RGCNConv (forward and backward, exactly),
the launch count per layer, determinism, and the example."""
import os
import sys

import numpy as np
import pytest
import torch

import relation_sampling_defs as RS
import sampling_defs as S
from gpu_common import dev, host, pgl      # noqa: F401  (pgl: the module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BIG = 1 << 14
BIG_TYPES = RS.EDGE_TYPES + ["rmat_a", "rmat_b", "rmat_c"]
BIG_FANOUTS = RS.FANOUTS + [10, -1, 25]
SEED = 2 ** 40 + 3


def _equal(got, want, what):
    for name, g, w in zip(("neighbors", "dst", "count", "eids"), (got.neighbors, got.dst, got.count, got.eids),
                          (want[0], want[1], want[2], want[4])):
        g = host(g) if isinstance(g, torch.Tensor) else g
        assert g.dtype == np.int64 and g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            e = int(np.flatnonzero(g.ravel() != w.ravel())[0])
            raise AssertionError("%s: %s differ first at entry %d: got %d, want %d" % (what, name, e, g.ravel()[e], w.ravel()[e]))
    assert tuple(got.edge_split) == tuple(want[3]) and all(isinstance(s, int) for s in got.edge_split), what


@pytest.fixture(scope="module")
def big(pgl):
    """The host fixture's four relations plus three RMAT-14 relations of 2^17 edges over 2^14 nodes, 50 001 seeds: (tensor
    HeterGraph, device StackedIndex, host StackedIndex, restated per-relation indices, seeds, the restated sample -- computed once)."""
    from pgl_amd.utils.rmat import rmat_edges
    edges = RS.fixture_edges()
    for i, et in enumerate(BIG_TYPES[4:]):
        edges[et] = rmat_edges(14, 1 << 17, seed=100 + i).numpy().astype(np.int64)
    hg_np = pgl.HeterGraph(edges={et: edges[et] for et in BIG_TYPES}, num_nodes=N_BIG)
    host_stacked = hg_np._stacked_pred()[0]
    hg = pgl.HeterGraph(edges={et: edges[et] for et in BIG_TYPES}, num_nodes=N_BIG).tensor()
    stacked, number = hg._stacked_pred()
    assert number == {et: r for r, et in enumerate(BIG_TYPES)} and isinstance(stacked, pgl.ops.StackedIndex)
    csrs = [S.csr_by_dst(edges[et], N_BIG) for et in BIG_TYPES]
    rng = np.random.default_rng(3)
    nodes = np.concatenate([RS.fixture_seeds(2000), rng.integers(0, N_BIG, 48001)]).astype(np.int64)
    assert len(nodes) == 50001 and len(nodes) % 256 != 0
    want = RS.sample_relations_restated(csrs, nodes, BIG_FANOUTS, SEED)
    assert want[2].max() > 64                                             # whole-row copies longer than a wave
    return hg, stacked, host_stacked, csrs, nodes, want


# ---- 1. bit equality ------------------------------------------------------------------------------------------------------------
def test_stacked_index_on_the_device_is_the_host_one(pgl, big):
    hg, stacked, host_stacked, csrs, _, _ = big
    assert stacked.indptr.dtype == torch.int64 and stacked.col.dtype == torch.int32 and stacked.eid.dtype == torch.int32
    assert tuple(stacked.indptr.shape) == (7, N_BIG + 1) and stacked.edge_base == host_stacked.edge_base
    for a, b in zip(stacked[:3], host_stacked[:3]):
        assert np.array_equal(host(a), b)
    for r, (indptr, col, eid) in enumerate(csrs):
        a, b = stacked.edge_base[r], stacked.edge_base[r + 1]
        assert np.array_equal(host(stacked.indptr[r]), indptr + a) and np.array_equal(host(stacked.col[a:b]), col) and \
            np.array_equal(host(stacked.eid[a:b]), eid)
    assert hg._stacked_pred()[0] is stacked


def test_device_equals_host_twin_equals_restatement(pgl, big):
    _, stacked, host_stacked, _, nodes, want = big
    got = pgl.ops.sample_neighbors_relations(stacked, dev(nodes), BIG_FANOUTS, seed=SEED, return_eids=True)
    assert got.neighbors.dtype == got.dst.dtype == got.count.dtype == got.eids.dtype == torch.int64
    _equal(got, want, "device vs restatement")
    twin = pgl.ops.host_sample_neighbors_relations(host_stacked, nodes, BIG_FANOUTS, seed=SEED, return_eids=True, threads=7)
    _equal(twin, want, "host twin vs restatement")
    plain = pgl.ops.sample_neighbors_relations(stacked, dev(nodes), BIG_FANOUTS, seed=SEED)
    assert plain.eids is None and torch.equal(plain.neighbors, got.neighbors) and torch.equal(plain.dst, got.dst)


def test_every_relation_is_sample_neighbors_over_that_relation(pgl, big):
    hg, stacked, _, _, nodes, _ = big
    d_nodes = dev(nodes)
    got = pgl.ops.sample_neighbors_relations(stacked, d_nodes, BIG_FANOUTS, seed=SEED, return_eids=True)
    for r, et in enumerate(BIG_TYPES):
        a, b = got.edge_split[r], got.edge_split[r + 1]
        if BIG_FANOUTS[r] == 0:
            assert a == b and int(got.count[r].sum()) == 0
            continue
        nbr, cnt, eids = pgl.ops.sample_neighbors(hg[et].adj_dst_index.csr, d_nodes, BIG_FANOUTS[r], seed=pgl.ops.relation_seed(SEED, r),
                                                  return_eids=True)
        assert torch.equal(got.neighbors[a:b], nbr) and torch.equal(got.count[r], cnt) and torch.equal(got.eids[a:b], eids), et
        assert torch.equal(got.dst[a:b], torch.repeat_interleave(torch.arange(len(nodes), device="cuda"), cnt)), et


@pytest.mark.parametrize("n", [0, 1])
def test_no_seed_and_one_seed(pgl, big, n):
    _, stacked, _, csrs, _, _ = big
    nodes = RS.fixture_seeds(n)
    got = pgl.ops.sample_neighbors_relations(stacked, dev(nodes), BIG_FANOUTS, seed=4, return_eids=True)
    _equal(got, RS.sample_relations_restated(csrs, nodes, BIG_FANOUTS, 4), "n = %d" % n)
    assert tuple(got.count.shape) == (7, n)


# ---- 2. the relabel -------------------------------------------------------------------------------------------------------------
def test_reindex_heter_graph_equals_the_restatement(pgl, big):
    _, stacked, _, _, nodes, _ = big
    nodes = nodes[:3000]
    s = pgl.ops.sample_neighbors_relations(stacked, dev(nodes), BIG_FANOUTS, seed=9)
    parts = [s.neighbors[s.edge_split[r]:s.edge_split[r + 1]] for r in range(7)]
    got = pgl.ops.reindex_heter_graph(dev(nodes), parts, list(s.count))
    want = RS.reindex_heter_restated(nodes, [host(p) for p in parts], [host(c) for c in s.count])
    for name, g, w in zip(("src", "dst", "out_nodes"), got, want):
        assert g.dtype == torch.int64 and np.array_equal(host(g), w), name
    assert torch.equal(got[1], s.dst)                                     # what the fill kernel wrote IS reindex_dst
    assert np.array_equal(host(got[2])[:3000], nodes)
    with pytest.raises(ValueError):
        pgl.ops.reindex_heter_graph(dev(nodes), parts, list(s.count)[:3])


# ---- 3. two relations with the same rows pick independently ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 12345])
def test_relations_with_equal_rows_pick_independently(pgl, seed):
    """Both relations hold law_graph(6, 200000)'s rows; with fan-out 3 a node's two pick sets coincide with probability 1 / C(6, 3)
    = 1 / 20, independently over the nodes: same ~ Binomial(200000, 1/20), mean 10000, sigma = sqrt(200000 * 0.05 * 0.95) = 97.5.
    |same - 10000| < 488 is five sigma.  (One shared seed would make every node pick the same positions in both: same = 200000.)"""
    W = 200000
    edges, n, pos_of_edge = S.law_graph(6, W, np.random.default_rng(66))
    hg = pgl.HeterGraph(edges={"a": edges, "b": edges.copy()}, num_nodes=n).tensor()
    nodes = np.arange(S.FIRST_NODE, S.FIRST_NODE + W, dtype=np.int64)
    s = pgl.ops.sample_neighbors_relations(hg._stacked_pred()[0], dev(nodes), [3, 3], seed=seed, return_eids=True)
    assert s.edge_split == (0, 3 * W, 6 * W) and (host(s.count) == 3).all()
    ei = host(s.eids).reshape(2, W, 3)
    assert np.array_equal(edges[ei[0].ravel(), 1], np.repeat(nodes, 3)) and np.array_equal(edges[ei[1].ravel(), 1], np.repeat(nodes, 3))
    picks = pos_of_edge[ei]
    masks = np.bitwise_or.reduce(np.int64(1) << picks, axis=2)
    same = int((masks[0] == masks[1]).sum())
    print("seed %d: nodes whose two pick sets coincide: %d (expected 10000, sigma 97.5)" % (seed, same))
    assert abs(same - 10000) < 488, same
    for r in (0, 1):
        S.assert_subset_law(picks[r], 6, 3, "relation %d seed %d" % (r, seed))


# ---- 4. the sampler's blocks ----------------------------------------------------------------------------------------------------
BLOCK_TYPES = ["r0", "r1", "none", "r2"]
N_BLK_GRAPH = 3000


@pytest.fixture(scope="module")
def block_case(pgl):
    """A HeterGraph whose in-degrees are 0, 1, 2, 4, 9 or 20 under every relation ("none" has no edges), sampled with fan-out 4 in
    two layers: every block row has 0, 1, 2 or 4 in-edges per relation, so a mean divides by a power of two and every sum of small
    integers below is exact in fp32."""
    rng = np.random.default_rng(17)
    edges = {}
    for et in BLOCK_TYPES:
        if et == "none":
            edges[et] = np.zeros((0, 2), np.int64)
            continue
        deg = rng.choice(np.array([0, 1, 2, 4, 9, 20]), N_BLK_GRAPH)
        dst = np.repeat(np.arange(N_BLK_GRAPH, dtype=np.int64), deg)
        e = np.stack([rng.integers(0, N_BLK_GRAPH, len(dst)), dst], 1).astype(np.int64)
        edges[et] = e[rng.permutation(len(e))]
    hg = pgl.HeterGraph(edges=edges, num_nodes=N_BLK_GRAPH).tensor()
    batch = np.concatenate([[5, 9, 5], rng.integers(0, N_BLK_GRAPH, 297)]).astype(np.int64)      # unsorted, with repeats
    sampler = pgl.sampling.RelationNeighborSampler(hg, [4, 4], seed=21, with_eids=True)
    graph_list, nodes = sampler.sample_neighbors(dev(batch))
    return hg, edges, batch, graph_list, nodes


def test_blocks_map_back_to_edges_of_their_relation(pgl, block_case):
    hg, edges, batch, graph_list, nodes = block_case
    nodes = host(nodes)
    node_sets = [nodes[:graph_list[0][1]], nodes]
    frontiers = [batch, node_sets[0]]
    for layer in (0, 1):
        block, n_dst = graph_list[1 - layer]
        out_nodes, frontier = node_sets[layer], frontiers[layer]
        assert isinstance(block, pgl.HeterGraph) and block.is_tensor() and block.edge_types == BLOCK_TYPES
        assert n_dst == len(frontier) and int(block.num_nodes) == len(out_nodes) and np.array_equal(out_nodes[:n_dst], frontier)
        for et in BLOCK_TYPES:
            g = block[et]
            e, eid = host(g.edges), host(g.edge_feat["eid"])
            deg = np.bincount(edges[et][:, 1], minlength=N_BLK_GRAPH)[frontier]
            assert np.array_equal(np.bincount(e[:, 1], minlength=n_dst), np.minimum(deg, 4)) and g._ids_in_range is True
            orig = edges[et][eid]
            assert np.array_equal(orig[:, 0], out_nodes[e[:, 0]]) and np.array_equal(orig[:, 1], frontier[e[:, 1]])
            csr = g.adj_dst_index.csr                                     # the index built without a sort IS the dst-sorted index
            want = S.csr_by_dst(e, len(out_nodes))
            assert np.array_equal(host(csr.indptr), want[0]) and np.array_equal(host(csr.col32), want[1]) and \
                np.array_equal(host(csr.eid32), want[2]) and np.array_equal(host(csr.row32), e[:, 1]) and \
                np.array_equal(host(csr.degree), np.diff(want[0]))


def test_block_send_recv_is_an_exact_scatter_add(pgl, block_case):
    _, _, _, graph_list, _ = block_case
    rng = np.random.default_rng(4)
    for block, n_dst in graph_list:
        n_blk = int(block.num_nodes)
        x = rng.integers(-4, 5, (n_blk, 24)).astype(np.float32)
        for et in BLOCK_TYPES:
            e = host(block[et].edges)
            want = np.zeros_like(x)
            np.add.at(want, e[:, 1], x[e[:, 0]])
            got = host(block[et].send_recv(dev(x), "sum"))
            assert np.array_equal(got, want), et
            if et == "none":
                assert block[et].num_edges == 0 and not got.any()        # the zero-edge relation yields zero rows
            else:
                assert want[:n_dst].any() and not want[n_dst:].any()


def test_rgcn_on_a_block_equals_rgcn_on_the_ordinary_graph_exactly(pgl, block_case):
    _, _, _, graph_list, _ = block_case
    rng = np.random.default_rng(6)
    for block, n_dst in graph_list:
        n_blk = int(block.num_nodes)
        plain = pgl.HeterGraph(edges={et: block[et].edges.clone() for et in BLOCK_TYPES}, num_nodes=n_blk).tensor()
        conv = pgl.nn.RGCNConv(8, 4, BLOCK_TYPES).cuda()
        with torch.no_grad():
            conv.weight.copy_(dev(rng.integers(-2, 3, (4, 8, 4)).astype(np.float32)))
        x0 = rng.integers(-3, 4, (n_blk, 8)).astype(np.float32)
        up = dev(rng.integers(-2, 3, (n_blk, 4)).astype(np.float32))
        res = []
        for g in (block, plain):
            x = dev(x0).requires_grad_(True)
            conv.weight.grad = None
            out = conv(g, x)
            (out * up).sum().backward()
            res.append((host(out), host(x.grad), host(conv.weight.grad)))
        for name, a, b in zip(("forward", "grad x", "grad weight"), res[0], res[1]):
            assert np.array_equal(a, b), name
        assert res[0][0][:n_dst].any() and not res[0][0][n_dst:].any() and res[0][1].any() and res[0][2].any()
        assert np.array_equal(res[0][0] * 4, np.round(res[0][0] * 4))    # (quarters of integers: nothing was rounded)


# ---- 5. launches, determinism, errors ------------------------------------------------------------------------------------------
class _Count(object):
    def __init__(self, ops, monkeypatch):
        self.n, inner = 0, ops._launch

        def counted(*a, **k):
            self.n += 1
            return inner(*a, **k)
        monkeypatch.setattr(ops, "_launch", counted)


def test_launches_per_layer_do_not_depend_on_the_number_of_relations(pgl, block_case, monkeypatch):
    hg, edges, batch, _, _ = block_case
    one = pgl.HeterGraph(edges={"r0": edges["r0"]}, num_nodes=N_BLK_GRAPH).tensor()
    s1 = pgl.sampling.RelationNeighborSampler(one, [4, 4], seed=2)
    s4 = pgl.sampling.RelationNeighborSampler(hg, [4, 4], seed=2)
    c = _Count(pgl.ops, monkeypatch)
    s1.sample_neighbors(dev(batch))
    n1, c.n = c.n, 0
    s4.sample_neighbors(dev(batch))
    n4, c.n = c.n, 0
    print("library launches per 2-layer batch: R = 1: %d, R = 4: %d" % (n1, n4))
    assert n1 == n4 and n1 % 2 == 0 and n1 > 0
    # the fused op itself: count, scan, fill
    pgl.ops.sample_neighbors_relations(hg._stacked_pred()[0], dev(batch), [4, 4, 4, 4], seed=1, check_range=False)
    assert c.n == 3


def test_two_samplers_with_one_seed_give_identical_blocks_and_the_numpy_graph_equal_ones(pgl, block_case):
    hg, edges, batch, graph_list, nodes = block_case
    again = pgl.sampling.RelationNeighborSampler(hg, [4, 4], seed=21, with_eids=True).sample_neighbors(dev(batch))
    hg_np = pgl.HeterGraph(edges=edges, num_nodes=N_BLK_GRAPH)
    on_host = pgl.sampling.RelationNeighborSampler(hg_np, [4, 4], seed=21, with_eids=True).sample_neighbors(batch)
    for other_list, other_nodes in (again, on_host):
        assert np.array_equal(host(nodes), other_nodes if isinstance(other_nodes, np.ndarray) else host(other_nodes))
        for (a, na), (b, nb) in zip(graph_list, other_list):
            assert na == nb and int(a.num_nodes) == int(b.num_nodes)
            for et in BLOCK_TYPES:
                eb, ib = b[et].edges, b[et].edge_feat["eid"]
                assert np.array_equal(host(a[et].edges), eb if isinstance(eb, np.ndarray) else host(eb)), et
                assert np.array_equal(host(a[et].edge_feat["eid"]), ib if isinstance(ib, np.ndarray) else host(ib)), et
    assert isinstance(on_host[1], np.ndarray) and not on_host[0][0][0].is_tensor()


def test_value_errors_come_before_any_launch(pgl, big, monkeypatch):
    _, stacked, _, _, nodes, _ = big
    d_nodes = dev(nodes[:100])
    c = _Count(pgl.ops, monkeypatch)
    with pytest.raises(ValueError, match="kMaxSample"):
        pgl.ops.sample_neighbors_relations(stacked, d_nodes, [5, 5, 5, 65, 5, 5, 5])
    with pytest.raises(ValueError, match="fan-outs"):
        pgl.ops.sample_neighbors_relations(stacked, d_nodes, [5, 5, 5])
    for bad in ([0, N_BIG], [-1, 3]):
        with pytest.raises(ValueError, match="outside"):
            pgl.ops.sample_neighbors_relations(stacked, torch.tensor(bad, device="cuda"), BIG_FANOUTS)
    assert c.n == 0
    with pytest.raises(RuntimeError):
        pgl.ops.sample_neighbors_relations(stacked, torch.tensor([1, 2]), BIG_FANOUTS)          # a CPU tensor: no fallback


def test_train_rgcn_sampled_example(pgl):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_rgcn_sampled
    finally:
        sys.path.pop(0)
    hist = train_rgcn_sampled.main(["--nodes", "2000", "--epochs", "4", "--batch_size", "250", "--hidden_size", "32"])
    loss = [h["train_loss"] for h in hist]
    print("train_rgcn_sampled losses:", loss)
    assert len(loss) == 4 and all(np.isfinite(loss)) and loss[-1] < loss[0], loss
