"""PinSAGE neighbourhoods on the MI355X (walk_visit.hip): the device against its host twin bit for bit over both tiers, the
shapes around the tier threshold and the cap, uniform and edge-weighted; the device against the definition (tests/pinsage_defs.py)
applied to the device's OWN ops.random_walk paths; reproducibility, the range check, PinSageSampler's blocks with PinSageConv on
them against fp64, and the example.

Walker s * R + r depends on the seed's position alone, so the result of the first S' seeds is the first S' rows of the result of
all of them: the host twin runs once per (shape, mode) on the NUM_SEEDS seeds and every S is compared with a prefix of it."""
import os
import runpy
import sys

import numpy as np
import pytest
import torch

import pinsage_defs as P
from gpu_common import check_aggregate, close_rows, dev, fp64_terms, host, pgl, reassociation_bound      # noqa: F401  (pgl: the module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP = (512, 8, 256)                                  # R * L = PGLAMD_VISIT_MAX, T = PGLAMD_VISIT_MAX_TOPK
SHAPES = [(1, 1, 1), (10, 2, 3), (64, 4, 16), (65, 3, 8),
          (128, 2, 256),                             # R * L = 256: the last wave-tier shape
          (257, 1, 5), (129, 2, 64),                 # the first block-tier shapes
          (200, 10, 50), CAP]
SIZES = [1, 63, 64, 65, P.NUM_SEEDS]
MODES = ["uniform", "weighted"]
DEFS_SHAPES = [(10, 2, 3), (129, 2, 64), (200, 10, 50)]
COVER = 300                                          # seeds the coverage conditions are evaluated on (all inside the S = 2048 runs)
SEED = 1234


@pytest.fixture(scope="module")
def world(pgl):
    edges, w, hub = P.rmat_graph()
    gn = pgl.Graph(edges=edges, num_nodes=P.N, edge_feat={"w": w})
    gt = pgl.Graph(edges=edges, num_nodes=P.N, edge_feat={"w": w}).tensor()
    indptr, col = gn._csr_succ_sorted()
    return dict(gn=gn, gt=gt, indptr=indptr, col=col, csr=gt._csr_succ_sorted(), seeds=P.rmat_seeds(hub), hub=hub,
                table={"uniform": None, "weighted": gn.edge_weight_table("w", "succ")},
                dtable={"uniform": None, "weighted": gt.edge_weight_table("w", "succ")}, want={})


def _want(pgl, world, shape, mode):
    """The host twin on all NUM_SEEDS seeds, computed once per (shape, mode) and left unchanged."""
    key = (shape, mode)
    if key not in world["want"]:
        R, L, T = shape
        world["want"][key] = pgl.ops.host_walk_visit_topk(world["indptr"], world["col"], world["seeds"], R, L, T, seed=SEED,
                                                          weights=world["table"][mode])
    return world["want"][key]


def _same(got, want, S):
    for g, w, name in zip(got, want, ("nbr", "cnt", "num")):
        g = host(g)
        assert g.dtype == w.dtype and g.shape == w[:S].shape, name
        assert np.array_equal(g, w[:S]), "%s: %d of %d entries differ" % (name, int((g != w[:S]).sum()), g.size)


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_equals_the_host_twin(pgl, world, shape, mode, S):
    R, L, T = shape
    got = pgl.ops.walk_visit_topk(world["csr"], dev(world["seeds"][:S]), R, L, T, seed=SEED, weights=world["dtable"][mode])
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
    _same(got, _want(pgl, world, shape, mode), S)


@pytest.mark.parametrize("mode", MODES)
def test_the_compared_rows_cover_every_case(pgl, world, mode):
    """On the expected arrays, so that the comparisons above cannot be vacuous: over the family there is a row with more than T
    distinct visited nodes, one with fewer, one whose counts are equal across the cut at T, and one without any neighbour; the
    seeds hold a repeated id, a node without successors and the hub."""
    seeds = world["seeds"][:COVER]
    more = fewer = tie = none = 0
    for R, L, T in SHAPES:
        paths, lengths = pgl.ops.host_random_walk(world["indptr"], world["col"], np.repeat(seeds, R), L, seed=SEED,
                                                  weights=world["table"][mode])
        nbr, cnt, num, distinct, cut_tie = P.visit_topk(paths, lengths, seeds, R, T, full=True)
        want = _want(pgl, world, (R, L, T), mode)
        assert np.array_equal(nbr, want[0][:COVER]) and np.array_equal(cnt, want[1][:COVER]) and np.array_equal(num, want[2][:COVER])
        more += int((distinct > T).sum()); fewer += int(((distinct < T) & (distinct > 0)).sum())
        tie += int(cut_tie.sum()); none += int((num == 0).sum())
        if (R, L, T) == (200, 10, 50):
            assert (distinct > T).any() and cut_tie.any() and (num == 0).any()       # the block tier has its own
        if (R, L, T) == (10, 2, 3):
            assert (distinct > T).any() and (distinct < T).any() and cut_tie.any() and (num == 0).any()      # and the wave tier
    assert more > 0 and fewer > 0 and tie > 0 and none > 0, (more, fewer, tie, none)
    s = world["seeds"]
    assert s[0] == s[2] == world["hub"] and s[1] == P.EMPTY and world["indptr"][P.EMPTY] == world["indptr"][P.EMPTY + 1]
    if mode == "weighted":
        w = _want(pgl, world, (10, 2, 3), "weighted")
        assert w[2][3] == 0 and _want(pgl, world, (10, 2, 3), "uniform")[2][3] > 0      # the all-zero row: a dead end by weight only


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", DEFS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_equals_the_definition_on_the_devices_own_walks(pgl, world, shape, mode):
    R, L, T = shape
    seeds = dev(world["seeds"][:COVER])
    paths, lengths = pgl.ops.random_walk(world["csr"], seeds.repeat_interleave(R), L, seed=SEED, weights=world["dtable"][mode])
    want = P.visit_topk(host(paths), host(lengths), world["seeds"][:COVER], R, T)
    got = pgl.ops.walk_visit_topk(world["csr"], seeds, R, L, T, seed=SEED, weights=world["dtable"][mode])
    _same(got, want, COVER)
    assert (want[2] > 0).any() and (want[2] == 0).any()


def test_reproducible_and_seeded(pgl, world):
    seeds = dev(world["seeds"][:500])
    for R, L, T in [(10, 2, 3), (200, 10, 50)]:
        a = pgl.ops.walk_visit_topk(world["csr"], seeds, R, L, T, seed=5)
        b = pgl.ops.walk_visit_topk(world["csr"], seeds, R, L, T, seed=5)
        c = pgl.ops.walk_visit_topk(world["csr"], seeds, R, L, T, seed=6)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert not torch.equal(a[0], c[0])
        assert not torch.equal(a[1][0], a[1][2])                # the hub twice: other walkers, other walks


@pytest.mark.parametrize("shape", [(10, 2, 3), (129, 2, 64)], ids=["wave", "block"])
def test_range_check(pgl, world, shape):
    R, L, T = shape
    bad = world["seeds"][:70].copy()
    bad[[4, 66]] = [P.N, -1]
    with pytest.raises(ValueError, match="outside"):
        pgl.ops.walk_visit_topk(world["csr"], dev(bad), R, L, T, seed=SEED)
    got = pgl.ops.walk_visit_topk(world["csr"], dev(bad), R, L, T, seed=SEED, check_range=False)
    want = tuple(a[:70].copy() for a in _want(pgl, world, shape, "uniform"))
    want[0][[4, 66]], want[1][[4, 66]], want[2][[4, 66]] = -1, 0, 0
    _same(got, want, 70)
    _same(got, pgl.ops.host_walk_visit_topk(world["indptr"], world["col"], bad, R, L, T, seed=SEED, check_range=False), 70)


def test_argument_errors_reach_no_launch(pgl, world):
    seeds = dev(world["seeds"][:4])
    for R, L, T in [(4097, 1, 1), (64, 65, 2), (2, 2, 257), (0, 1, 1), (1, 0, 1), (1, 1, 0)]:
        with pytest.raises(ValueError):
            pgl.ops.walk_visit_topk(world["csr"], seeds, R, L, T)
    with pytest.raises(ValueError, match="p != 1 or q != 1"):
        pgl.ops.walk_visit_topk(world["csr"], seeds, 2, 2, 2, p=2.0)
    with pytest.raises(ValueError, match="WeightTable"):
        pgl.ops.walk_visit_topk(world["csr"], seeds, 2, 2, 2, weights=world["gt"].edge_weight_table("w", "dst")._replace(
            npos=torch.zeros(3, dtype=torch.int64, device="cuda")))
    empty = pgl.ops.walk_visit_topk(world["csr"], seeds[:0], 3, 2, 4)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 4) and empty[2].shape == (0,)


def test_pinsage_neighbors_on_a_tensor_graph(pgl, world):
    seeds = world["seeds"][:300]
    nbr, weight, num = pgl.sampling.pinsage_neighbors(world["gt"], seeds, 30, 3, 8, seed=3, weights="w")
    hn, hw, hnum = pgl.sampling.pinsage_neighbors(world["gn"], seeds, 30, 3, 8, seed=3, weights="w")
    assert np.array_equal(host(nbr), hn) and np.array_equal(host(num), hnum)
    assert weight.dtype == torch.float32 and (np.abs(host(weight) - hw) <= np.finfo(np.float32).eps * hw).all()      # one fp32 division each
    assert ((host(weight) > 0) == (hn >= 0)).all()


def test_sampler_blocks_and_the_layer_on_them(pgl, world):
    R, L, top_ks = 20, 3, [5, 3]
    rng = np.random.default_rng(8)
    nodes = np.concatenate([world["seeds"][:8], rng.integers(0, P.N, 248)]).astype(np.int64)
    nodes[100:120] = nodes[:20]                                  # repeats
    sampler = pgl.sampling.PinSageSampler(world["gt"], R, L, top_ks, seed=40)
    blocks, out_nodes = sampler.sample_neighbors(dev(nodes))
    assert len(blocks) == 2 and blocks[1][1] == len(nodes)
    out_nodes = host(out_nodes)
    x_all = rng.standard_normal((P.N, 16)).astype(np.float32)
    torch.manual_seed(0)
    layer = pgl.nn.PinSageConv(16, 12, "sum").cuda()
    layer64 = pgl.nn.PinSageConv(16, 12, "sum").double()
    layer64.load_state_dict({k: v.detach().cpu().double() for k, v in layer.state_dict().items()})
    # innermost block first: layer 0 of the sampler walked from `nodes` with seed 41, layer 1 from that block's nodes with seed 42
    frontiers = [nodes, out_nodes[:blocks[0][1]]]
    for depth, ((block, n_dst), frontier, T) in enumerate(zip(blocks[::-1], frontiers, top_ks)):
        ids = frontiers[1] if depth == 0 else out_nodes          # the global id of every block node
        assert n_dst == len(frontier) and block.num_nodes == len(ids)
        assert np.array_equal(ids[:n_dst], frontier)             # the first n_dst rows are the frontier as given
        nbr, cnt, num = pgl.ops.host_walk_visit_topk(world["indptr"], world["col"], frontier, R, L, T, seed=41 + depth)
        src, dst = host(block.edges[:, 0]), host(block.edges[:, 1])
        filled = nbr >= 0
        assert np.array_equal(dst, np.repeat(np.arange(n_dst), num))
        assert np.array_equal(ids[src], nbr[filled])             # every edge u -> v: u is v's next expected neighbour, in order
        assert all(ids[u] in set(nbr[v, :num[v]].tolist()) for u, v in zip(src[:200], dst[:200]))
        w = host(block.edge_feat["weight"])
        assert w.shape == (len(src), 1) and w.dtype == np.float32
        per_dst = np.bincount(dst, weights=w[:, 0].astype(np.float64), minlength=n_dst)
        assert (np.abs(per_dst[num > 0] - 1.0) <= T * np.finfo(np.float32).eps).all() and (per_dst[num == 0] == 0).all()
        want_w = cnt.astype(np.float32) / np.maximum(cnt.sum(1, keepdims=True), 1).astype(np.float32)
        assert (np.abs(w[:, 0] - want_w[filled]) <= np.finfo(np.float32).eps * want_w[filled]).all()      # one fp32 division each
        # the layer from (nbr, weight) in fp64: neighbours by GLOBAL id, no block involved
        x = x_all[ids]
        neigh64 = np.zeros((len(ids), 16))
        neigh64[:n_dst] = (want_w.astype(np.float64)[:, :, None] * x_all.astype(np.float64)[np.where(filled, nbr, 0)] * filled[:, :, None]).sum(1)
        local = {}
        for i, v in enumerate(ids.tolist()):
            local.setdefault(v, i)
        e_src = np.array([local[v] for v in nbr[filled].tolist()], np.int64)
        e_dst = np.repeat(np.arange(n_dst), num)
        agg = host(block.send_ue_recv(dev(x), block.edge_feat["weight"], "mul", "sum"))
        check_aggregate(agg, x, e_src, e_dst, "sum", y=want_w[filled][:, None], mop="mul", what="block %d aggregation" % depth)
        _, abs_terms, n_terms = fp64_terms(x, e_src, e_dst, "sum", y=want_w[filled][:, None], mop="mul")
        assert (np.abs(agg - neigh64) <= reassociation_bound(abs_terms, n_terms)).all()      # the same bound, against the block-free sum
        with torch.no_grad():
            got = layer(block, dev(x), block.edge_feat["weight"], act="relu")
            x64, n64 = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(neigh64)
            want = torch.nn.functional.normalize(torch.relu(layer64.self_linear(x64) + layer64.neigh_linear(n64)), dim=1)
        close_rows(host(got), want.numpy(), what="PinSageConv on block %d" % depth)


def test_example_trains(capsys, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["train_pinsage.py", "--nodes", "2000", "--epochs", "4", "--batch_size", "250", "--num_walks", "10",
                                      "--walk_length", "2", "--top_ks", "5", "3", "--hidden_size", "32"])
    runpy.run_path(os.path.join(ROOT, "examples", "train_pinsage.py"), run_name="__main__")
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("epoch")]
    assert len(lines) == 4, lines
    loss = [float(l.split("train loss")[1].split()[0]) for l in lines]
    assert all(np.isfinite(loss)) and loss[-1] < loss[0], loss
