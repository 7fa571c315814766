"""Neighbour sampling and relabelling on the MI355X (sampling.hip) held to their definition, restated in numpy in
tests/sampling_defs.py: the sampler bit for bit (neighbours, counts and edge ids; more seeds than the launch has threads), the
exact law of the sampled SUBSETS by chi-square in one launch over 200 000 nodes, edge ids on multi-edges, the relabel table bit
for bit at its capacity steps / under contention / with 2^40-scale ids / with repeated seeds, the blocks NeighborSampler
builds from an unsorted batch with repeats, and what the caller sees for a sample size or a node id out of range."""
import numpy as np
import pytest
import torch

import ref_ops as R
import sampling_defs as S
from gpu_common import close_rows, dev, host, pgl, rand_graph      # noqa: F401  (pgl: the module fixture)

pytestmark = pytest.mark.gpu

KS = [-1, 0, 1, 2, 10, 25, 63, 64]
SEEDS = [0, 7, 2 ** 40 + 3, 2 ** 64 - 1]


def _assert_sampler_equals_restatement(pgl, csr, host_csr, nodes, k, seed, what):
    want = S.sample_restated(host_csr[0], host_csr[1], host_csr[2], nodes, k, seed)
    nbr, cnt, eids = pgl.ops.sample_neighbors(csr, dev(np.asarray(nodes, np.int64)), k, seed=seed, return_eids=True)
    assert nbr.dtype == cnt.dtype == eids.dtype == torch.int64
    for name, g, w in (("count", cnt, want[1]), ("neighbors", nbr, want[0]), ("eids", eids, want[2])):
        g = host(g)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            e = int(np.flatnonzero(g != w)[0])
            i = e if name == "count" else int(np.searchsorted(np.cumsum(want[1]), e, side="right"))
            v = int(nodes[i])
            raise AssertionError("%s: %s differ first at entry %d: got %d, want %d (seed position %d, node %d, degree %d, draw %d)"
                                 % (what, name, e, g[e], w[e], i, v, host_csr[0][v + 1] - host_csr[0][v],
                                    e - int(np.cumsum(want[1])[i] - want[1][i]) if name != "count" else -1))
    return want


# ------------------------------------------------------------------------------------------------
# 1. bit equality with the restatement
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat_small(pgl):
    """RMAT-14 with 200 000 edges, a 6 000-edge hub and five rows of 62 .. 66 in-edges (the RMAT draw has none at the last legal
    sample size): multi-edges, nodes without in-edges, degrees around every k."""
    from pgl_amd.utils.rmat import rmat_edges
    n = 1 << 14
    e = rmat_edges(14, 200000, seed=11).numpy()
    rng = np.random.default_rng(1)
    e[rng.choice(len(e), 6000, replace=False), 1] = 4242
    empty = np.flatnonzero(np.bincount(e[:, 1], minlength=n) == 0)[:5]
    e = np.concatenate([e] + [np.stack([rng.integers(0, 40, d), np.full(d, v)], 1) for v, d in zip(empty, (62, 63, 64, 65, 66))])
    e = e[rng.permutation(len(e))]
    g = pgl.Graph(edges=e, num_nodes=n).tensor()
    csr = g.adj_dst_index.csr
    host_csr = S.csr_by_dst(e, n)
    assert np.array_equal(host(csr.indptr), host_csr[0]) and np.array_equal(host(csr.col32), host_csr[1]) and \
        np.array_equal(host(csr.eid32), host_csr[2])                                      # the index the restatement reads IS the device's
    deg = np.diff(host_csr[0])
    assert deg.max() >= 6000 and (deg == 0).sum() > 100
    assert len(np.unique(e[:, 0] * n + e[:, 1])) < len(e)                                  # multi-edges
    for k in (10, 25, 63, 64):
        assert all((deg == d).any() for d in (k - 1, k, k + 1)), k
    return e, n, csr, host_csr, deg


def _seed_list(kind, n, deg):
    rng = np.random.default_rng(5)
    if kind == "shuffled":
        return rng.permutation(n)
    if kind == "repeats":
        out = rng.integers(0, n, 3000)
        out[::10] = 4242                                                                   # the hub, 300 times
        assert len(np.unique(out)) < len(out)
        return out
    if kind == "zero-degree":
        return rng.permutation(np.flatnonzero(deg == 0))
    return np.zeros(0, np.int64)


@pytest.mark.parametrize("kind", ["shuffled", "repeats", "zero-degree", "empty"])
@pytest.mark.parametrize("k", KS)
def test_sampler_equals_the_restatement(pgl, rmat_small, k, kind):
    _, n, csr, host_csr, deg = rmat_small
    nodes = _seed_list(kind, n, deg)
    for seed in SEEDS:
        want = _assert_sampler_equals_restatement(pgl, csr, host_csr, nodes, k, seed, (kind, k, seed))
        if kind in ("zero-degree", "empty") or k == 0:
            assert len(want[0]) == 0                                                       # total = 0: the fill launch is skipped
    if kind == "shuffled" and 0 < k < 64:
        a, b = (S.sample_restated(*host_csr, nodes, k, s)[2] for s in SEEDS[:2])
        assert not np.array_equal(a, b)                                                    # (the cases above do exercise the draw)


@pytest.fixture(scope="module")
def rmat21(pgl):
    from pgl_amd.utils.rmat import rmat_edges
    n = 1 << 21
    g = pgl.Graph(edges=rmat_edges(21, 8_000_000, seed=3, device="cuda"), num_nodes=n)
    csr = g.adj_dst_index.csr
    return n, csr, (host(csr.indptr), host(csr.col32), host(csr.eid32))                    # (csr_build is held bit-exact in test_a1_a3_index.py)


@pytest.mark.parametrize("k", KS)
def test_sampler_equals_the_restatement_with_more_seeds_than_threads(pgl, rmat21, k):
    """Every node of a 2^21-node graph in one call: the grid is capped at 4096 x 256 = 2^20 threads, so the count kernel, the
    fill kernel and the offsets scan all stride."""
    n, csr, host_csr = rmat21
    assert n > 4096 * 256
    nodes = np.arange(n, dtype=np.int64)
    for seed in SEEDS:
        _assert_sampler_equals_restatement(pgl, csr, host_csr, nodes, k, seed, ("rmat21", k, seed))


# ------------------------------------------------------------------------------------------------
# 2. the exact law of the sampled subsets, one launch over all nodes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 2 ** 40 + 3])
@pytest.mark.parametrize("deg,k,W", S.SUBSET_CASES)
def test_exact_subset_law_device(pgl, deg, k, W, seed):
    edges, n, pos_of_edge = S.law_graph(deg, W, np.random.default_rng(deg * 100 + k))
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    nodes = np.arange(S.FIRST_NODE, S.FIRST_NODE + W, dtype=np.int64)
    nbr, cnt, eids = pgl.ops.sample_neighbors(g.adj_dst_index.csr, dev(nodes), k, seed=seed, return_eids=True)
    assert (host(cnt) == k).all()
    ei = host(eids)
    assert np.array_equal(edges[ei, 1], np.repeat(nodes, k)) and np.array_equal(edges[ei, 0], host(nbr))
    S.assert_subset_law(pos_of_edge[ei].reshape(W, k), deg, k, "device seed %d" % seed)


# ------------------------------------------------------------------------------------------------
# 3. structure on multi-edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 10, 64, -1])
def test_edge_ids_distinct_on_multi_edges(pgl, rmat_small, k):
    e, n, csr, host_csr, deg = rmat_small
    nodes = np.random.default_rng(2).permutation(n)
    nbr, cnt, eids = pgl.ops.sample_neighbors(csr, dev(nodes), k, seed=21, return_eids=True)
    nb, ct, ei = host(nbr), host(cnt), host(eids)
    assert np.array_equal(ct, deg[nodes] if k < 0 else np.minimum(deg[nodes], k))
    row = np.repeat(np.arange(n), ct)
    assert np.array_equal(e[ei, 1], nodes[row]) and np.array_equal(e[ei, 0], nb)          # real in-edges of the right node
    assert len(np.unique(ei)) == len(ei)                                                   # distinct seeds: no edge id twice at all
    if k != 1:
        pairs = row * n + nb
        assert len(np.unique(pairs)) < len(pairs)                                          # ... where neighbour ids do repeat inside a row
    nbr2, cnt2 = pgl.ops.sample_neighbors(csr, dev(nodes), k, seed=21)
    assert torch.equal(nbr2, nbr) and torch.equal(cnt2, cnt)


# ------------------------------------------------------------------------------------------------
# 4. reindex_graph against the restatement
# ------------------------------------------------------------------------------------------------
TOTALS = [31, 32, 33, 64, 65, 2048, 2049, 4097, 3_000_001]
REINDEX_CASES = ["total-1-seed", "total-1-neighbour"] + ["total-%d" % t for t in TOTALS] + \
    ["one-new-id", "one-seed-id", "16-ids", "2^40-ids", "all-seeds", "later-seeds", "m=0", "n=0", "n=m=0", "repeats-5-5-7", "repeats-100000"]


def _reindex_case(name):
    rng = np.random.default_rng(REINDEX_CASES.index(name))
    i64 = lambda a: np.asarray(a, np.int64)
    count = None
    if name == "total-1-seed":
        nodes, nbrs = i64([9]), i64([])
    elif name == "total-1-neighbour":
        nodes, nbrs = i64([]), i64([9])
    elif name.startswith("total-"):
        t = int(name[6:])
        n = max(1, t // 3)
        nodes, nbrs = rng.permutation(2 * t)[:n], rng.integers(0, 2 * t, t - n)           # distinct seeds; neighbours: seeds, new ids, repeats
    elif name == "one-new-id":
        nodes, nbrs = rng.permutation(1000)[:100], np.full(100000, 12345)
    elif name == "one-seed-id":
        nodes = rng.permutation(1000)[:100]
        nbrs = np.full(100000, nodes[57])
    elif name == "16-ids":
        nodes, nbrs = i64([3, 900, 5]), rng.integers(0, 16, 200000)
    elif name == "2^40-ids":
        nodes, nbrs = rng.integers(0, 1 << 40, 5000), rng.integers(0, 1 << 40, 50000)
        nbrs[::3] = nodes[rng.integers(0, 5000, len(nbrs[::3]))]
        nbrs[1::3] = nbrs[rng.integers(0, 50000, len(nbrs[1::3]))]
        assert nbrs.max() > 1 << 39
    elif name == "all-seeds":
        nodes = rng.permutation(100000)[:3000]
        nbrs = nodes[rng.integers(0, 3000, 40000)]
    elif name == "later-seeds":                                                            # row i draws from the seeds after position i, and new ids
        nodes = rng.permutation(5000)[:1000]
        count = np.full(1000, 6)
        later = nodes[np.minimum(np.repeat(np.arange(1000), 6) + rng.integers(1, 300, 6000), 999)]
        nbrs = np.where(rng.random(6000) < 0.7, later, rng.integers(5000, 6000, 6000))
    elif name == "m=0":
        nodes, nbrs = rng.permutation(5000)[:1000], i64([])
    elif name == "n=0":
        nodes, nbrs = i64([]), rng.integers(0, 700, 5000)
    elif name == "n=m=0":
        nodes, nbrs = i64([]), i64([])
    elif name == "repeats-5-5-7":
        nodes, nbrs, count = i64([5, 5, 7]), i64([7, 9, 5, 9, 3]), i64([2, 0, 3])
    else:
        nodes, nbrs = rng.integers(0, 20000, 100000), rng.integers(0, 30000, 500000)
        assert len(np.unique(nodes)) < len(nodes)
    if count is None:
        count = np.bincount(rng.integers(0, len(nodes), len(nbrs)), minlength=len(nodes)) if len(nodes) else i64([])
    return i64(nodes), i64(nbrs), i64(count)


@pytest.mark.parametrize("name", REINDEX_CASES)
def test_reindex_graph_equals_the_restatement(pgl, name):
    nodes, nbrs, count = _reindex_case(name)
    if name.startswith("total-"):
        assert len(nodes) + len(nbrs) == int(name.split("-")[1])
    want = S.reindex_restated(nodes, nbrs, count)
    args = (dev(nodes), dev(nbrs), dev(count))
    got = [host(t) for t in pgl.ops.reindex_graph(*args)]
    again = [host(t) for t in pgl.ops.reindex_graph(*args)]
    for what, g, a, w in zip(("src", "dst", "out_nodes"), got, again, want):
        assert g.dtype == np.int64 and g.shape == w.shape, (name, what, g.shape, w.shape, g[:8], w[:8])
        if not np.array_equal(g, w):
            e = int(np.flatnonzero(g != w)[0])
            raise AssertionError("%s: %s differ first at %d: got %s, want %s" % (name, what, e, g[e:e + 4], w[e:e + 4]))
        assert np.array_equal(g, a), (name, what, "two runs differ")


# ------------------------------------------------------------------------------------------------
# 5. the blocks NeighborSampler builds
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampler_graph(pgl):
    n, e, d = 3000, 40000, 24
    edges, rng = rand_graph(n, e, 1200, hub=2000)
    x = rng.standard_normal((n, d)).astype(np.float32)
    batch = rng.integers(0, n, 400).astype(np.int64)
    batch[[7, 50, 399]] = n // 2                                                           # the hub, three times, and random repeats
    assert len(np.unique(batch)) < len(batch) and (np.diff(batch) < 0).any()
    return pgl.Graph(edges=edges, num_nodes=n).tensor(), edges, x, batch


@pytest.mark.parametrize("fanouts", [[5, 5], [25, 10], [-1], [64]])
def test_neighbor_sampler_blocks_are_self_consistent(pgl, sampler_graph, fanouts):
    g, edges, x, batch = sampler_graph
    n = g.num_nodes
    real = np.unique(edges[:, 0] * n + edges[:, 1])
    blocks, nodes = pgl.sampling.NeighborSampler(g, fanouts, seed=40).sample_neighbors(dev(batch))
    assert len(blocks) == len(fanouts)
    frontier, seed, index = dev(batch), 40, None
    for (blk, n_dst), size in zip(blocks[::-1], fanouts):                                  # in sampling order
        seed += 1
        nbr, cnt = pgl.ops.sample_neighbors(g.adj_dst_index.csr, frontier, size, seed=seed)
        src, dst, index = pgl.ops.reindex_graph(frontier, nbr, cnt)
        assert torch.equal(blk.edges, torch.stack([src, dst], 1)) and blk.num_nodes == int(index.shape[0])
        f, idx = host(frontier), host(index)
        assert n_dst == len(f)
        assert np.array_equal(idx[:n_dst], f), "the first n_dst rows of a block are not its frontier"
        assert np.array_equal(idx[host(src)], host(nbr)) and host(dst).max() < n_dst
        assert np.isin(idx[host(src)] * n + idx[host(dst)], real).all(), "a block edge that is no edge of the graph"
        deg = np.bincount(edges[:, 1], minlength=n)[f]
        assert np.array_equal(np.bincount(host(dst), minlength=n_dst), deg if size < 0 else np.minimum(deg, size))
        frontier = index
    assert torch.equal(nodes, index) and np.array_equal(host(nodes)[:len(batch)], batch)
    if fanouts == [-1]:
        blk, n_dst = blocks[0]
        agg = blk.send_recv(dev(x)[nodes], "sum", out_size=n_dst)
        want = R.c_send_u_recv(x, edges[:, 0].copy(), edges[:, 1].copy(), "sum")
        close_rows(host(agg), want[batch])                                                 # the repeated rows included


def test_neighbor_sampler_seeding(pgl, sampler_graph):
    g, _, _, batch = sampler_graph
    a, b = (pgl.sampling.NeighborSampler(g, [5, 5], seed=9) for _ in range(2))
    (ba, na), (bb, nb) = a.sample_neighbors(dev(batch)), b.sample_neighbors(dev(batch))
    assert torch.equal(na, nb) and all(torch.equal(p[0].edges, q[0].edges) and p[1] == q[1] for p, q in zip(ba, bb))
    ba2, na2 = a.sample_neighbors(dev(batch))
    assert not torch.equal(ba2[-1][0].edges, ba[-1][0].edges)                              # the next call draws afresh


# ------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------
def test_sample_size_above_the_limit_is_a_value_error(pgl, sampler_graph):
    g, _, _, batch = sampler_graph
    csr, nodes = g.adj_dst_index.csr, dev(batch)
    assert pgl.ops.MAX_SAMPLE == 64
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match=r"kMaxSample = 64"):
        pgl.ops.sample_neighbors(csr, nodes, 65, seed=1)
    assert torch.cuda.memory_allocated() == before                                         # refused before any output exists
    with pytest.raises(ValueError, match=r"kMaxSample = 64"):
        pgl.sampling.NeighborSampler(g, [10, 65]).sample_neighbors(nodes)
    assert int(pgl.ops.sample_neighbors(csr, nodes, 64, seed=1)[1].max()) == 64            # the limit itself is legal


def test_sampler_range_check(pgl, sampler_graph):
    g, _, _, _ = sampler_graph
    csr = g.adj_dst_index.csr
    for bad in ([g.num_nodes], [-1], [0, 1 << 40]):
        with pytest.raises(ValueError):
            pgl.ops.sample_neighbors(csr, torch.tensor(bad, device="cuda"), 5, seed=1)
        with pytest.raises(ValueError):
            pgl.sampling.NeighborSampler(g, [5, 5]).sample_neighbors(torch.tensor(bad, device="cuda"))
    nbr, cnt = pgl.ops.sample_neighbors(csr, torch.tensor([g.num_nodes - 1, 0], device="cuda"), 5, seed=1)     # the ends of the range pass
    assert int(cnt.sum()) == len(nbr)
    one, zero = torch.tensor([1], device="cuda"), torch.tensor([0], device="cuda")
    for nodes, nbrs in ((torch.tensor([3, -1], device="cuda"), one), (one, torch.tensor([-5], device="cuda"))):
        with pytest.raises(ValueError):                                                    # -1 is the relabel table's empty marker: refused on the host
            pgl.ops.reindex_graph(nodes, nbrs, torch.tensor([1] + [0] * (len(nodes) - 1), device="cuda"))
    assert host(pgl.ops.reindex_graph(zero, zero, one)[2]).tolist() == [0]
