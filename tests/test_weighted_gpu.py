"""Edge-weighted sampling on the MI355X (weighted.hip, the weighted mode of walk.hip): the device weight table against the host
twin bit for bit, weighted walks against the host twin and the exact weighted path law, weighted neighbour sampling against its
numpy restatement and the successive-sampling law, NeighborSampler(weights=), draws from a single-row table, the DeepWalk example
with a degree^0.75 noise distribution, and once that calls without weights still answer what they answered."""
import os
import sys

import numpy as np
import pytest
import torch

import sampling_defs as S
import walk_defs as D
import weighted_defs as W
from gpu_common import dev, host, pgl      # noqa: F401  (pgl: the module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rmat(pgl):
    """RMAT scale 14, 2^18 edges, exponential weights with 10 % zeros: (numpy graph, tensor graph, edges, weights fp32)."""
    from pgl_amd.utils.rmat import rmat_edges
    e = rmat_edges(14, 1 << 18, seed=7).numpy()
    rng = np.random.default_rng(11)
    w = rng.exponential(size=len(e)).astype(np.float32)
    w[rng.random(len(e)) < 0.1] = 0
    gn = pgl.Graph(edges=e, num_nodes=1 << 14, edge_feat={"w": w})
    gt = pgl.Graph(edges=e, num_nodes=1 << 14, edge_feat={"w": w}).tensor()
    return gn, gt, e, w


def _same_table(got, want):
    assert got.cum.dtype == torch.int64 and got.npos.dtype == torch.int64
    assert np.array_equal(host(got.npos), want.npos)
    assert np.array_equal(host(got.cum), want.cum)


# ---- table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("with_eid", [False, True])
def test_device_table_equals_the_host_twin(pgl, dtype, with_eid):
    indptr, weight = W.TABLE_GRAPH
    n, E = len(indptr) - 1, len(weight)
    w = weight.astype(dtype)
    if dtype == np.float64:
        w = w * (1.0 + np.random.default_rng(3).random(E) * 1e-9)
    eid = None
    if with_eid:
        eid = np.random.default_rng(4).permutation(E).astype(np.int32)
        shuffled = np.empty_like(w)
        shuffled[eid] = w
        w = shuffled
    row32 = np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr))
    csr = pgl.ops.CSR(dev(indptr), dev(row32), None, None, n, E)
    got = pgl.ops.edge_weight_table(csr, dev(w), None if eid is None else dev(eid))
    _same_table(got, pgl.ops.host_edge_weight_table(indptr, w, eid))
    cum, npos = W.table_restated(indptr, w, eid)
    assert np.array_equal(host(got.cum), cum) and np.array_equal(host(got.npos), npos)
    hub = slice(indptr[W.HUB_ROW], indptr[W.HUB_ROW + 1])
    assert (np.diff(host(got.cum)[hub]) >= 0).all() and host(got.npos)[W.HUB_ROW] > 60000


def test_graph_tables_on_both_indexes(pgl):
    edges, n, w = W.table_graph_edges()
    gn = pgl.Graph(edges=edges, num_nodes=n, edge_feat={"w": w.astype(np.float32)})
    gt = pgl.Graph(edges=edges, num_nodes=n, edge_feat={"w": w.astype(np.float32)}).tensor()
    for index in ("dst", "succ"):
        t = gt.edge_weight_table("w", index)
        _same_table(t, gn.edge_weight_table("w", index))
        assert gt.edge_weight_table("w", index) is t                       # cached per (index, tensor, version)
        _same_table(gt.edge_weight_table(dev(w), index), gn.edge_weight_table(w, index))     # fp64, a tensor in edge order
    ptr, _, eid = S.csr_by_dst(edges, n)
    cum, npos = W.table_restated(ptr, w.astype(np.float32), eid)
    t = gt.edge_weight_table("w", "dst")
    assert np.array_equal(host(t.cum), cum) and np.array_equal(host(t.npos), npos)
    sptr, _, seid = W.succ_index(edges, n)
    cum, npos = W.table_restated(sptr, w.astype(np.float32), seid)
    t = gt.edge_weight_table("w", "succ")
    assert np.array_equal(host(t.cum), cum) and np.array_equal(host(t.npos), npos)
    gt.edge_feat["w"].mul_(2.0)                                             # an in-place update rebuilds the entry ...
    t2 = gt.edge_weight_table("w", "succ")
    assert t2 is not t and torch.equal(t2.cum, t.cum)                       # ... to the same table: scaling a row changes no q
    half = pgl.ops.edge_weight_table(gt.adj_dst_index.csr, gt.edge_feat["w"].to(torch.bfloat16).float(), gt.adj_dst_index.csr.eid32)
    assert torch.equal(gt.edge_weight_table(gt.edge_feat["w"].to(torch.bfloat16), "dst").cum, half.cum)     # bf16 is cast to fp32


@pytest.mark.parametrize("bad,word", [(np.nan, "NaN"), (-1.0, "negative"), (np.inf, "infinite")])
def test_the_flag_raises(pgl, bad, word):
    indptr, weight = W.TABLE_GRAPH
    n, E = len(indptr) - 1, len(weight)
    csr = pgl.ops.CSR(dev(indptr), dev(np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr))), None, None, n, E)
    for dtype, at in ((np.float32, 17), (np.float64, int(indptr[W.HUB_ROW]) + 40000)):
        w = weight.astype(dtype)
        w[at] = bad
        with pytest.raises(ValueError, match=word):
            pgl.ops.edge_weight_table(csr, dev(w))
    with pytest.raises(ValueError):
        pgl.ops.edge_weight_table(csr, dev(weight[:-1]))
    with pytest.raises(ValueError, match="edge id"):
        pgl.ops.edge_weight_table(csr, dev(weight[:100]), dev(np.arange(E, dtype=np.int32)))


# ---- walks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2 ** 40 + 3])
def test_device_weighted_walks_equal_the_host_twin(pgl, rmat, seed):
    gn, gt, e, w = rmat
    starts = np.random.default_rng(seed % 1000).integers(0, gn.num_nodes, 20000)
    indptr, col = gn._csr_succ_sorted()
    csr = gt._csr_succ_sorted()
    assert np.array_equal(host(csr.indptr), indptr) and np.array_equal(host(csr.col32), col)
    th, td = gn.edge_weight_table("w", "succ"), gt.edge_weight_table("w", "succ")
    _same_table(td, th)
    want = pgl.ops.host_random_walk(indptr, col, starts, 20, seed=seed, weights=th)
    got = pgl.ops.random_walk(csr, dev(starts), 20, seed=seed, weights=td)
    assert np.array_equal(host(got[1]), want[1])
    assert np.array_equal(host(got[0]), want[0])
    assert (want[1] < 21).any() and (want[1] == 21).any()                  # dead ends met, full-length walks too
    # no step follows a zero-weight edge: every (a, b) step has a positive-weight edge a -> b
    ok = set(map(tuple, e[w > 0].tolist()))
    p = want[0]
    steps = np.stack([p[:, :-1].ravel(), p[:, 1:].ravel()], 1)
    steps = np.unique(steps[steps[:, 1] >= 0], axis=0)
    assert all(tuple(s) in ok for s in steps.tolist())
    lists = pgl.sampling.random_walk(gt, starts[:500], 21, seed=seed, weights="w")
    assert lists == pgl.sampling.random_walk(gn, starts[:500], 21, seed=seed, weights="w")
    assert lists == [row[:n].tolist() for row, n in zip(want[0][:500], want[1][:500])]


def test_exact_weighted_walk_law_device(pgl):
    g = pgl.Graph(edges=D.EDGES, num_nodes=D.N, edge_feat={"w": W.WALK_WEIGHTS}).tensor()
    csr, table = g._csr_succ_sorted(), g.edge_weight_table("w", "succ")
    sptr, _, seid = W.succ_index(D.EDGES, D.N)
    qe = np.empty(len(D.EDGES), np.int64)
    qe[seid] = W.quantise(sptr, W.WALK_WEIGHTS, seid)[0]
    wsucc = W.weighted_successors(D.EDGES, qe, D.N)
    const = g.edge_weight_table(torch.full((len(D.EDGES),), 3.0, device="cuda"), "succ")
    for start in W.LAW_STARTS:
        starts = torch.full((W.LAW_WALKS,), start, dtype=torch.int64, device="cuda")
        paths, _ = pgl.ops.random_walk(csr, starts, W.LAW_STEPS, seed=900 + start, weights=table)
        D.assert_law(host(paths), W.weighted_path_law(wsucc, start, W.LAW_STEPS), ("weighted device", start))
        paths, _ = pgl.ops.random_walk(csr, starts, W.LAW_STEPS, seed=950 + start, weights=const)
        D.assert_law(host(paths), D.path_law(D.successors(), start, W.LAW_STEPS, 1.0, 1.0, "uniform"), ("constant weights", start))


def test_weighted_walk_reproducibility_and_argument_checks(pgl, rmat):
    _, gt, _, _ = rmat
    nodes = torch.arange(0, gt.num_nodes, 3, device="cuda")
    a = pgl.sampling.walks(gt, nodes, 30, seed=9, weights="w")
    b = pgl.sampling.walks(gt, nodes, 30, seed=9, weights=gt.edge_feat["w"])
    c = pgl.sampling.walks(gt, nodes, 30, seed=10, weights=gt.edge_weight_table("w", "succ"))
    assert a[0].is_cuda and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    assert not torch.equal(a[0], pgl.sampling.walks(gt, nodes, 30, seed=9)[0])
    with pytest.raises(ValueError, match="node2vec"):
        pgl.sampling.walks(gt, nodes, 5, p=0.5, q=2.0, seed=1, weights="w")
    with pytest.raises(ValueError, match="node2vec"):
        pgl.ops.random_walk(gt._csr_succ_sorted(), nodes, 5, p=1.0, q=2.0, plus=True, weights=gt.edge_weight_table("w", "succ"))
    with pytest.raises(ValueError):
        pgl.sampling.walks(gt, torch.tensor([gt.num_nodes], device="cuda"), 5, seed=1, weights="w")
    with pytest.raises(ValueError):                                        # a table over the other index
        pgl.ops.random_walk(gt._csr_succ_sorted(), nodes, 5, weights=pgl.ops.WeightTable(a[0].reshape(-1), a[1]))
    sub = pgl.sampling.random_walk_subgraph(gt, nodes[:50], 6, seed=3, weights="w")
    assert 0 < sub.num_nodes <= 50 * 7


# ---- sampler -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampler_case(pgl, rmat):
    gn, gt, e, w = rmat
    indptr, col, eid = S.csr_by_dst(e, gn.num_nodes)
    cum, npos = W.table_restated(indptr, w, eid)
    rng = np.random.default_rng(5)
    nodes = rng.integers(0, gn.num_nodes, 4096)
    nodes[:8] = np.argsort(-npos)[:8]                                      # the hubs ...
    nodes[100:108] = nodes[:8]                                             # ... and repeated ids
    nodes[200:210] = nodes[300:310]
    assert npos[nodes[0]] > 64 and (npos[nodes] > 64).sum() > 20 and (npos[nodes] == 0).any()
    return indptr, col, eid, cum, npos, nodes


@pytest.mark.parametrize("k", [1, 5, 64, -1])
def test_weighted_sampler_equals_the_restatement(pgl, rmat, sampler_case, k):
    _, gt, e, w = rmat
    indptr, col, eid, cum, npos, nodes = sampler_case
    csr, table = gt.adj_dst_index.csr, gt.edge_weight_table("w", "dst")
    assert np.array_equal(host(table.cum), cum) and np.array_equal(host(csr.eid32), eid)
    for seed in (3, 2 ** 63 + 5):
        nbr, count, eids = pgl.ops.sample_neighbors(csr, dev(nodes), k, seed=seed, return_eids=True, weights=table)
        wn, wc, we, pos = W.sample_weighted_restated(indptr, col, eid, cum, nodes, k, seed)
        assert np.array_equal(host(count), wc) and np.array_equal(wc, npos[nodes] if k < 0 else np.minimum(k, npos[nodes]))
        assert np.array_equal(host(nbr), wn) and np.array_equal(host(eids), we)
        got_e = host(eids)
        assert (w[got_e] > 0).all()                                        # no zero-weight edge
        assert np.array_equal(e[got_e, 0], host(nbr)) and np.array_equal(e[got_e, 1], np.repeat(nodes, wc))
        owner = np.repeat(np.arange(len(nodes)), wc)
        assert len(np.unique(np.stack([owner, got_e], 1), axis=0)) == len(got_e)      # no position twice within a sample
        nbr2, count2 = pgl.ops.sample_neighbors(csr, dev(nodes), k, seed=seed, weights=table)
        assert torch.equal(nbr2, nbr) and torch.equal(count2, count)
    other = pgl.ops.sample_neighbors(csr, dev(nodes), k, seed=4, weights=table)[0]
    assert (k < 0) == bool(torch.equal(other, nbr2))                       # another seed, another sample (k = -1 draws nothing)


def test_weighted_sampler_argument_checks(pgl, rmat):
    _, gt, _, _ = rmat
    csr, table = gt.adj_dst_index.csr, gt.edge_weight_table("w", "dst")
    nodes = torch.arange(10, device="cuda")
    with pytest.raises(ValueError):
        pgl.ops.sample_neighbors(csr, nodes, 65, weights=table)
    with pytest.raises(ValueError):
        pgl.ops.sample_neighbors(csr, torch.tensor([gt.num_nodes], device="cuda"), 5, weights=table)
    with pytest.raises(TypeError):
        pgl.ops.sample_neighbors(csr, nodes, 5, weights=gt.edge_feat["w"])
    nbr, count = pgl.ops.sample_neighbors(csr, nodes[:0], 5, weights=table)
    assert nbr.numel() == 0 and count.numel() == 0
    nbr, count = pgl.ops.sample_neighbors(csr, nodes, 0, weights=table)
    assert nbr.numel() == 0 and int(count.sum()) == 0


@pytest.mark.parametrize("weights,k,nodes", W.SAMPLER_LAW_CASES)
def test_weighted_sampler_law_device(pgl, weights, k, nodes):
    indptr, col, w, n = W.law_rows(weights, nodes, S.FIRST_NODE)
    E = len(col)
    row32 = np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr))
    csr = pgl.ops.CSR(dev(indptr), dev(row32), dev(col.astype(np.int32)), dev(np.arange(E, dtype=np.int32)), n, E)
    table = pgl.ops.edge_weight_table(csr, dev(w))
    ids = np.arange(S.FIRST_NODE, n)
    nbr, count = pgl.ops.sample_neighbors(csr, dev(ids), k, seed=77, weights=table)
    assert (host(count) == k).all()
    law = W.successive_law(W.q_of(indptr, host(table.cum))[:len(weights)], k)
    D.assert_law(host(nbr).reshape(nodes, k), law, ("device sampler", weights, k))


def test_neighbor_sampler_with_weights(pgl, rmat):
    _, gt, e, w = rmat
    have = set(map(tuple, e[w > 0].tolist()))
    batch = np.random.default_rng(2).integers(0, gt.num_nodes, 512)
    for weights in ("w", gt.edge_feat["w"], gt.edge_weight_table("w", "dst")):
        sampler = pgl.sampling.NeighborSampler(gt, [10, 5], seed=3, weights=weights)
        blocks, nodes = sampler.sample_neighbors(batch)
        ids = host(nodes)
        frontier = batch
        for block, n_dst in blocks[::-1]:                                  # sampling order: the batch's block first
            assert n_dst == len(frontier)
            out = ids[:block.num_nodes]
            assert np.array_equal(out[:n_dst], frontier)                   # the first n_dst rows are the frontier
            be = host(block.edges)
            assert (be[:, 1] < n_dst).all() and np.bincount(be[:, 1], minlength=n_dst).max() <= 10
            assert all((int(a), int(b)) in have for a, b in zip(out[be[:, 0]], out[be[:, 1]]))    # positive-weight edges of the graph
            frontier = out
    plain = pgl.sampling.NeighborSampler(gt, [10, 5], seed=3).sample_neighbors(batch)
    assert not np.array_equal(host(plain[1]), ids)


# ---- draws from a table ------------------------------------------------------------------------------------------------------
def test_sample_from_table(pgl):
    from scipy.stats import chi2
    w = np.random.default_rng(8).exponential(size=100000)
    w[::7] = 0
    t = pgl.ops.weight_table(dev(w))
    want = pgl.ops.host_edge_weight_table(np.array([0, len(w)]), w)
    _same_table(t, want)
    for seed, count in ((0, 200000), (2 ** 63 + 9, 1000), (5, 1)):
        got = host(pgl.ops.sample_from_table(t.cum, count, seed))
        assert np.array_equal(got, W.sample_from_table_restated(want.cum, count, seed))
        assert (w[got] > 0).all()
    assert np.array_equal(host(pgl.ops.sample_from_table(t, 100, 3)), host(pgl.ops.sample_from_table(t.cum, 100, 3)))
    assert pgl.ops.sample_from_table(t, 0).numel() == 0
    six = pgl.ops.weight_table(dev(np.array([1, 2, 0, 4, 0.5, 8], np.float32)))
    draws = host(pgl.ops.sample_from_table(six, 200000, seed=21))
    q = W.q_of(np.array([0, 6]), host(six.cum)).astype(np.float64)
    obs = np.bincount(draws, minlength=6).astype(np.float64)
    assert obs[2] == 0
    exp = 200000 * q / q.sum()
    keep = q > 0
    pv = float(chi2.sf(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum(), keep.sum() - 1))
    assert pv > 1e-4, (obs, exp, pv)
    zero = pgl.ops.weight_table(dev(np.zeros(5, np.float32)))
    assert host(pgl.ops.sample_from_table(zero, 10)).tolist() == [-1] * 10  # nothing to draw
    with pytest.raises(ValueError, match="negative"):
        pgl.ops.weight_table(dev(np.array([1.0, -2.0])))


def test_train_deepwalk_with_degree_noise(pgl):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_deepwalk
    finally:
        sys.path.pop(0)
    r = train_deepwalk.main(["--neg_power", "0.75", "--steps", "20", "--seed", "0"])
    assert np.isfinite(r["loss_first"]) and np.isfinite(r["loss_last"]), r


# ---- what did not change -----------------------------------------------------------------------------------------------------
def test_calls_without_weights_are_unchanged(pgl, rmat):
    gn, gt, e, _ = rmat
    starts = np.random.default_rng(1).integers(0, gn.num_nodes, 5000)
    indptr, col = gn._csr_succ_sorted()
    want = pgl.ops.host_random_walk(indptr, col, starts, 15, seed=6)
    for kw in ({}, {"weights": None}):
        got = pgl.ops.random_walk(gt._csr_succ_sorted(), dev(starts), 15, seed=6, **kw)
        assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1])
    ptr, c, eid = S.csr_by_dst(e, gn.num_nodes)
    nodes = np.random.default_rng(2).integers(0, gn.num_nodes, 2000)
    for k in (5, -1):
        wn, wc, we = S.sample_restated(ptr, c, eid, nodes, k, 9)
        for kw in ({}, {"weights": None}):
            nbr, count, eids = pgl.ops.sample_neighbors(gt.adj_dst_index.csr, dev(nodes), k, seed=9, return_eids=True, **kw)
            assert np.array_equal(host(nbr), wn) and np.array_equal(host(count), wc) and np.array_equal(host(eids), we)
