"""Metapath walks on the MI355X (pglamd_metapath_walk, the relation-stacked mode of walk.hip): the device against the host twin
bit for bit over every flush boundary of the path staging, the single-relation identity with ops.random_walk, the exact law on
the small graph of tests/metapath_defs.py, results and errors, the public functions on tensor HeterGraphs and the
metapath2vec example."""
import os
import sys

import numpy as np
import pytest
import torch

import metapath_defs as M
import weighted_defs as W
from gpu_common import dev, host, pgl      # noqa: F401  (pgl: the module fixture)
from walk_defs import assert_law

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, E = 1 << 14, 1 << 17
TYPES = ["r0", "r1", "r2", "none"]
W_WALKERS = 50001                             # not a multiple of K * kBlock


@pytest.fixture(scope="module")
def rmat(pgl):
    """Three RMAT relations of 2^17 edges over 2^14 nodes and one relation without edges, exponential weights with 10 % zeros:
    (numpy HeterGraph, tensor HeterGraph, starts, host stacked index + table, device stacked index + table)."""
    from pgl_amd.utils.rmat import rmat_edges
    rng = np.random.default_rng(3)
    edges, feat = {}, {}
    for r, et in enumerate(TYPES):
        e = rmat_edges(14, E, seed=20 + r).numpy() if et != "none" else np.zeros((0, 2), np.int64)
        w = rng.exponential(size=len(e)).astype(np.float32)
        w[rng.random(len(e)) < 0.1] = 0
        edges[et], feat[et] = e, {"w": w}
    hn = pgl.HeterGraph(edges=edges, num_nodes=N, edge_feat={et: dict(f) for et, f in feat.items()})
    ht = pgl.HeterGraph(edges=edges, num_nodes=N, edge_feat={et: dict(f) for et, f in feat.items()}).tensor()
    sh, sd = hn._stacked_succ()[0], ht._stacked_succ()[0]
    th = pgl.ops.stack_weight_tables([hn[et].edge_weight_table("w", "succ") for et in TYPES])
    td = pgl.ops.stack_weight_tables([ht[et].edge_weight_table("w", "succ") for et in TYPES])
    assert ht._stacked_succ()[1] == hn._stacked_succ()[1] == {et: r for r, et in enumerate(TYPES)}
    assert np.array_equal(host(sd.indptr), sh.indptr) and np.array_equal(host(sd.col), sh.col) and sd.edge_base == sh.edge_base
    assert sd.indptr.is_contiguous() and sd.indptr.dtype == torch.int64 and sd.col.dtype == torch.int32
    assert np.array_equal(host(td.cum), th.cum) and np.array_equal(host(td.npos), th.npos)
    starts = np.random.default_rng(4).integers(0, N, W_WALKERS)
    return hn, ht, starts, (sh, th), (sd, td)


GPU_METAPATHS = {1: [0], 2: [0, 1], 5: [0, 1, 2, 1, 0]}


# ---- 1. device == host twin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_steps", [0, 1, 7, 8, 9, 40])           # 8 positions are staged per flush: both sides of a flush
def test_device_equals_the_host_twin(pgl, rmat, small, num_steps):
    _, _, starts, (sh, th), (sd, td) = rmat
    dstarts = dev(starts)
    full = set()
    for L, mp in GPU_METAPATHS.items():
        for phase in sorted({0, L - 1}):
            for seed in (1, 2 ** 40 + 3):
                for wh, wd in ((None, None), (th, td)):
                    want = pgl.ops.host_metapath_walk(sh, starts, mp, num_steps, phase=phase, seed=seed, weights=wh)
                    got = pgl.ops.metapath_walk(sd, dstarts, mp, num_steps, phase=phase, seed=seed, weights=wd)
                    what = (L, phase, seed, wh is not None)
                    assert got[0].shape == (W_WALKERS, num_steps + 1), what
                    assert np.array_equal(host(got[1]), want[1]), what
                    assert np.array_equal(host(got[0]), want[0]), what
                    if num_steps:
                        assert (want[1] < num_steps + 1).any(), what                  # dead ends in every case ...
                        full.add((L, bool((want[1] == num_steps + 1).any())))
    # ... and full-length walks: a node reached under one RMAT relation has successors under another with probability about
    # 0.65, so a walk that changes relation survives 9 steps (2 %) but not 40 (0.65^40 < 1e-7); one relation keeps a quarter
    if num_steps:
        assert (1, True) in full and (num_steps > 9 or full == {(1, True), (2, True), (5, True)}), full
    want = pgl.ops.host_metapath_walk(sh, starts, [0, 3], num_steps, seed=5)         # the relation without edges ends every walk
    got = pgl.ops.metapath_walk(sd, dstarts, [0, 3], num_steps, seed=5)
    assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1]) and want[1].max() == min(num_steps, 1) + 1
    # the small graph has cycles across its relations: walks that change relation at every step and are alive at every flush
    hn, ht, _ = small
    few = np.arange(W_WALKERS) % M.N
    for phase in (0, 4):
        want = pgl.ops.host_metapath_walk(hn._stacked_succ()[0], few, M.METAPATHS[5], num_steps, phase=phase, seed=11)
        got = pgl.ops.metapath_walk(ht._stacked_succ()[0], dev(few), M.METAPATHS[5], num_steps, phase=phase, seed=11)
        assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1])
        assert (want[1] == num_steps + 1).any() and (num_steps == 0 or (want[1] < num_steps + 1).any())


# ---- 2. single-relation identity ---------------------------------------------------------------------------------------------
def test_one_relation_metapath_is_random_walk(pgl, rmat):
    _, ht, starts, _, (sd, td) = rmat
    dstarts = dev(starts)
    for r in (0, 2):
        csr = ht[TYPES[r]]._csr_succ_sorted()
        for seed in (7, 2 ** 40 + 9):
            want = pgl.ops.random_walk(csr, dstarts, 20, seed=seed)
            got = pgl.ops.metapath_walk(sd, dstarts, [r], 20, seed=seed)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            want = pgl.ops.random_walk(csr, dstarts, 20, seed=seed, weights=ht[TYPES[r]].edge_weight_table("w", "succ"))
            got = pgl.ops.metapath_walk(sd, dstarts, [r], 20, seed=seed, weights=td)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert int(want[1].max()) == 21 and int(want[1].min()) < 21


# ---- 3. exact law ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(pgl):
    mk = lambda: pgl.HeterGraph(edges={et: M.EDGES[et] for et in M.EDGE_TYPES}, num_nodes=M.N,
                                edge_feat={et: {"w": M.WEIGHTS[et]} for et in M.EDGE_TYPES})
    hn, ht = mk(), mk().tensor()
    q = []
    for et in M.EDGE_TYPES:
        sptr, _, seid = W.succ_index(M.EDGES[et], M.N)
        qe = np.empty(len(M.EDGES[et]), np.int64)
        qe[seid] = W.quantise(sptr, M.WEIGHTS[et], seid)[0]
        q.append(qe)
    return hn, ht, q


@pytest.mark.parametrize("L", [2, 3])
def test_exact_metapath_law_device(pgl, small, L):
    _, ht, q = small
    stacked = ht._stacked_succ()[0]
    table = pgl.ops.stack_weight_tables([ht[et].edge_weight_table("w", "succ") for et in M.EDGE_TYPES])
    mp = M.METAPATHS[L]
    for start in M.LAW_STARTS:
        starts = torch.full((M.LAW_WALKS,), start, dtype=torch.int64, device="cuda")
        paths, _ = pgl.ops.metapath_walk(stacked, starts, mp, M.LAW_STEPS, seed=300 * L + start)
        assert_law(host(paths), M.path_law(M.successors(), start, M.LAW_STEPS, mp), ("device uniform", L, start))
        paths, _ = pgl.ops.metapath_walk(stacked, starts, mp, M.LAW_STEPS, seed=350 * L + start, weights=table)
        paths = host(paths)
        assert_law(paths, M.path_law(M.successors(q), start, M.LAW_STEPS, mp), ("device weighted", L, start))
        assert not ((paths[:, 0] == 0) & (paths[:, 1] == 5)).any()                    # 0 -> 5 carries weight zero
    starts = torch.full((M.LAW_WALKS,), 5, dtype=torch.int64, device="cuda")
    paths, _ = pgl.ops.metapath_walk(stacked, starts, mp, M.LAW_STEPS, phase=L - 1, seed=78)
    assert_law(host(paths), M.path_law(M.successors(), 5, M.LAW_STEPS, mp, L - 1), ("device phase", L))


# ---- 4. results and errors ---------------------------------------------------------------------------------------------------
def test_device_results_and_errors(pgl, rmat):
    _, ht, starts, _, (sd, td) = rmat
    nodes = dev(starts[:5000])
    a = pgl.ops.metapath_walk(sd, nodes, [0, 1, 2], 12, seed=9)
    b = pgl.ops.metapath_walk(sd, nodes, [0, 1, 2], 12, seed=9)
    c = pgl.ops.metapath_walk(sd, nodes, [0, 1, 2], 12, seed=10)
    assert a[0].is_cuda and a[1].is_cuda and a[0].dtype == torch.int64 and a[1].dtype == torch.int64
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    assert not torch.equal(a[0], pgl.ops.metapath_walk(sd, nodes, [0, 1, 2], 12, phase=1, seed=9)[0])
    assert not torch.equal(a[0], pgl.ops.metapath_walk(sd, nodes, [0, 1, 2], 12, seed=9, weights=td)[0])
    empty = pgl.ops.metapath_walk(sd, nodes[:0], [0, 1], 5)
    assert tuple(empty[0].shape) == (0, 6) and tuple(empty[1].shape) == (0,)
    for bad in (N, -1):
        ids = torch.tensor([3, bad], device="cuda")
        with pytest.raises(ValueError, match="start nodes outside"):
            pgl.ops.metapath_walk(sd, ids, [0, 1], 4)
        paths, lengths = pgl.ops.metapath_walk(sd, ids, [0, 1], 4, check_range=False)
        assert host(paths)[1].tolist() == [bad, -1, -1, -1, -1] and int(lengths[1]) == 1
    R = sd.num_relations
    for mp, phase, steps in (([], 0, 3), ([0] * 65, 0, 3), ([0, R], 0, 3), ([0, 1], 2, 3), ([0, 1], 0, -1)):
        with pytest.raises(ValueError, match=r"pgl_amd metapath_walk: .*\(code -6\)"):
            pgl.ops.metapath_walk(sd, nodes, mp, steps, phase=phase)
    with pytest.raises(RuntimeError):
        pgl.ops.metapath_walk(sd, torch.tensor([1, 2]), [0, 1], 4)                   # a CPU tensor: no fallback
    with pytest.raises(ValueError, match="WeightTable"):
        pgl.ops.metapath_walk(sd, nodes, [0, 1], 4, weights=ht["r0"].edge_weight_table("w", "succ"))


# ---- 5. public functions on tensor graphs ------------------------------------------------------------------------------------
def test_public_functions_on_tensor_graphs(pgl, rmat, small):
    hn, ht, starts, _, (sd, td) = rmat
    nodes = starts[:3000]
    for mp, kw in (("r0-r1-r2", {}), (["r2", "r0"], {"weights": {"r0": "w", "r2": "w"}})):
        a = pgl.sampling.metapath_randomwalk(ht, nodes, mp, 8, seed=6, **kw)
        assert a == pgl.sampling.metapath_randomwalk(hn, nodes, mp, 8, seed=6, **kw)
        assert max(map(len, a)) == 8 and min(map(len, a)) < 8
    paths, lengths = pgl.sampling.metapath_walks(ht, dev(nodes), ["r2", "r0"], 7, seed=6, weights={"r0": "w", "r2": ht["r2"].edge_feat["w"]})
    assert paths.is_cuda and a == [row[:n].tolist() for row, n in zip(host(paths), host(lengths))]
    np.random.seed(3); b = pgl.sampling.metapath_walks(ht, nodes, "r0-r1", 9)
    np.random.seed(3); c = pgl.sampling.metapath_walks(ht, nodes, "r0-r1", 9, phase=0)
    assert torch.equal(b[0], c[0]) and not torch.equal(b[0], pgl.sampling.metapath_walks(ht, nodes, "r0-r1", 9, phase=1, seed=1)[0])
    src, dst = pgl.ops.skip_gram_pairs(*b, win_size=3, seed=1)                       # what the walks are for
    assert src.is_cuda and src.shape == dst.shape and src.numel() > 0
    with pytest.raises(ValueError, match="rX"):
        pgl.sampling.metapath_walks(ht, nodes, "r0-rX", 9)
    with pytest.raises(ValueError, match="empty"):
        pgl.sampling.metapath_walks(ht, nodes, "", 9)
    with pytest.raises(ValueError, match="r1"):
        pgl.sampling.metapath_walks(ht, nodes, "r0-r1", 9, weights={"r0": "w"})
    with pytest.raises(ValueError):
        pgl.sampling.metapath_walks(ht, [N], "r0-r1", 9)
    # the cached stacked index follows the graph's mode
    g = pgl.HeterGraph(edges={et: M.EDGES[et] for et in M.EDGE_TYPES}, num_nodes=M.N)
    s0 = g._stacked_succ()[0]
    assert isinstance(s0.indptr, np.ndarray) and g._stacked_succ()[0] is s0
    g.tensor()
    s1 = g._stacked_succ()[0]
    assert s1.indptr.is_cuda and np.array_equal(host(s1.indptr), s0.indptr) and np.array_equal(host(s1.col), s0.col)
    g.numpy()
    assert isinstance(g._stacked_succ()[0].indptr, np.ndarray)
    # with walk times, on the small graph: the properties of the host test, whichever sampler took the first step
    sn, st, _ = small
    nodes = list(range(M.N)) * 6
    for names, length, times in ((["a2p", "p2a"], 7, 2), (["a2p", "p2p", "p2a"], 6, 10), (["p2p"], 5, 1), (["a2p", "p2a"], 2, 3)):
        walks = pgl.sampling.metapath_randomwalk_with_walktimes(st, nodes, "-".join(names), length, walk_times=times, seed=2)
        M.walktimes_properties(walks, nodes, names, length, times)
        assert walks == pgl.sampling.metapath_randomwalk_with_walktimes(st, nodes, names, length, times, None, None, seed=2)
    assert pgl.sampling.metapath_randomwalk_with_walktimes(st, [3, 9, 11], "a2p-p2a", 5, seed=1) == []
    assert pgl.sampling.metapath_randomwalk(st, nodes, "a2p-p2p-p2p-p2a", 8, seed=4) == \
        pgl.sampling.metapath_randomwalk(sn, nodes, "a2p-p2p-p2p-p2a", 8, seed=4)


# ---- 6. the example ----------------------------------------------------------------------------------------------------------
def test_train_metapath2vec_example(pgl):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_metapath2vec
    finally:
        sys.path.pop(0)
    r = train_metapath2vec.main(["--steps", "100", "--seed", "0"])
    # observed on an MI355X, 100 steps: seed 0 loss 3.650 -> 1.195 (x 0.33), cosine 0.537 / 0.235; seed 1 loss 3.635 -> 1.194,
    # cosine 0.542 / 0.235 (200 steps, seed 0: loss -> 1.117, cosine 0.455 / 0.203)
    assert r["loss_last"] < 0.5 * r["loss_first"], r
    assert r["intra_cos"] > r["inter_cos"] + 0.15, r
