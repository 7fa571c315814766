"""PinSAGE neighbourhoods on the host (no GPU): ops.host_walk_visit_topk against the definition (tests/pinsage_defs.py) applied to
the walks of ops.host_random_walk -- the twin the device is then held to bit for bit in tests/test_pinsage_gpu.py -- its argument
checks, the out-of-range seed, sampling.pinsage_neighbors on a numpy graph and the import paths through the `pgl` alias."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pinsage_defs as P


@pytest.fixture(scope="module")
def pgl():
    import pgl_amd
    return pgl_amd


@pytest.fixture(scope="module")
def world(pgl):
    edges, w, hub = P.rmat_graph()
    g = pgl.Graph(edges=edges, num_nodes=P.N, edge_feat={"w": w})
    indptr, col = g._csr_succ_sorted()
    return g, indptr, col, g.edge_weight_table("w", "succ"), P.rmat_seeds(hub)[:200]


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("R,L,T", [(1, 1, 1), (10, 2, 3), (65, 3, 8), (40, 10, 50)])
def test_host_twin_equals_the_definition_on_host_walks(pgl, world, R, L, T, weighted, threads):
    _, indptr, col, table, seeds = world
    weights = table if weighted else None
    paths, lengths = pgl.ops.host_random_walk(indptr, col, np.repeat(seeds, R), L, seed=77, weights=weights)
    want = P.visit_topk(paths, lengths, seeds, R, T)
    got = pgl.ops.host_walk_visit_topk(indptr, col, seeds, R, L, T, seed=77, weights=weights, threads=threads)
    for g_, w_, name in zip(got, want, ("nbr", "cnt", "num")):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        assert np.array_equal(g_, w_), name
    assert (want[2] == 0).any() and (want[2] > 0).any()
    filled = np.arange(T)[None, :] < got[2][:, None]                    # the filled entries are a prefix of every row
    assert ((got[0] >= 0) == filled).all() and ((got[1] > 0) == filled).all()


def test_weighted_walks_never_leave_the_zero_row(pgl, world):
    _, indptr, col, table, _ = world
    seeds = np.array([P.ZERO_ROW, P.EMPTY], np.int64)
    assert indptr[P.ZERO_ROW + 1] > indptr[P.ZERO_ROW]
    _, _, num_u = pgl.ops.host_walk_visit_topk(indptr, col, seeds, 8, 2, 4, seed=1)
    _, _, num_w = pgl.ops.host_walk_visit_topk(indptr, col, seeds, 8, 2, 4, seed=1, weights=table)
    assert num_u.tolist()[1] == 0 and num_u[0] > 0 and num_w.tolist() == [0, 0]


def test_the_result_does_not_depend_on_the_other_seeds(pgl, world):
    _, indptr, col, _, seeds = world
    a = pgl.ops.host_walk_visit_topk(indptr, col, seeds, 10, 3, 5, seed=3)
    b = pgl.ops.host_walk_visit_topk(indptr, col, seeds[:50], 10, 3, 5, seed=3)
    assert all(np.array_equal(x[:50], y) for x, y in zip(a, b))
    assert seeds[0] == seeds[2] and not np.array_equal(a[1][0], a[1][2])      # a repeated seed gets other walkers, other walks
    c = pgl.ops.host_walk_visit_topk(indptr, col, seeds, 10, 3, 5, seed=4)
    assert not np.array_equal(a[0], c[0])


@pytest.mark.parametrize("R,L,T,word", [(4097, 1, 1, "VISIT_MAX"), (64, 65, 1, "VISIT_MAX"), (1, 1, 257, "TOPK"), (0, 1, 1, ">= 1"),
                                        (1, 0, 1, ">= 1"), (1, 1, 0, ">= 1"), (-3, 2, 2, ">= 1")])
def test_argument_errors(pgl, world, R, L, T, word):
    _, indptr, col, _, seeds = world
    with pytest.raises(ValueError, match=word):
        pgl.ops.host_walk_visit_topk(indptr, col, seeds, R, L, T)


def test_the_caps_themselves_are_accepted_and_the_library_refuses_beyond_them(pgl, world):
    _, indptr, col, _, seeds = world
    nbr, cnt, num = pgl.ops.host_walk_visit_topk(indptr, col, seeds[:3], 512, 8, 256)
    assert nbr.shape == (3, 256) and pgl.ops.VISIT_MAX == 4096 and pgl.ops.VISIT_MAX_TOPK == 256
    lib, p = pgl._ffi.lib(), pgl.ops._np_ptr
    out = (np.empty((1, 300), np.int64), np.empty((1, 300), np.int32), np.empty(1, np.int32))
    call = lambda R, L, T: lib.pglamd_walk_visit_topk_host(p(indptr), p(col), None, P.N, p(seeds), 1, R, L, T, 0, 1, p(out[0]), p(out[1]),
                                                           p(out[2]), None)
    assert call(4097, 1, 1) == -3 and b"PGLAMD_VISIT_MAX" in lib.pglamd_last_error()
    assert call(1 << 40, 1 << 40, 1) == -3
    assert call(1, 1, 257) == -3 and b"TOPK" in lib.pglamd_last_error()
    assert call(0, 1, 1) == -6 and call(1, 0, 1) == -6 and call(1, 1, 0) == -6
    assert call(1, 1, 1) == 0


def test_node2vec_parameters_and_foreign_tables_are_refused(pgl, world):
    g, indptr, col, table, seeds = world
    with pytest.raises(ValueError, match="p != 1 or q != 1"):
        pgl.ops.host_walk_visit_topk(indptr, col, seeds, 2, 2, 2, p=0.5)
    with pytest.raises(ValueError, match="weighted node2vec"):
        pgl.ops.host_walk_visit_topk(indptr, col, seeds, 2, 2, 2, weights=table, q=2.0)
    other = pgl.ops.host_edge_weight_table(indptr[:11], np.ones(int(indptr[10]), np.float32))      # a table over another index
    with pytest.raises(ValueError, match="WeightTable over this index"):
        pgl.ops.host_walk_visit_topk(indptr, col, seeds, 2, 2, 2, weights=other)
    with pytest.raises(ValueError, match="WeightTable over this index"):
        pgl.ops.host_walk_visit_topk(indptr, col, seeds, 2, 2, 2, weights=np.ones(len(col), np.float32))


def test_out_of_range_seed(pgl, world):
    _, indptr, col, _, seeds = world
    bad = np.array([seeds[0], P.N, seeds[1], -1, seeds[6]], np.int64)
    with pytest.raises(ValueError, match="outside"):
        pgl.ops.host_walk_visit_topk(indptr, col, bad, 6, 2, 3, seed=9)
    nbr, cnt, num = pgl.ops.host_walk_visit_topk(indptr, col, bad, 6, 2, 3, seed=9, check_range=False)
    assert (nbr[[1, 3]] == -1).all() and (cnt[[1, 3]] == 0).all() and num[[1, 3]].tolist() == [0, 0]
    paths, lengths = pgl.ops.host_random_walk(indptr, col, np.repeat(np.where((bad >= 0) & (bad < P.N), bad, 0), 6), 2, seed=9)
    want = P.visit_topk(paths, lengths, bad, 6, 3)
    for s in (0, 2, 4):                                                    # the rows around a bad seed keep their own walkers
        assert np.array_equal(nbr[s], want[0][s]) and np.array_equal(cnt[s], want[1][s]) and num[s] == want[2][s]
    assert num[0] > 0


@pytest.mark.parametrize("weights", [None, "w"])
def test_pinsage_neighbors_on_a_numpy_graph(pgl, world, weights):
    g, indptr, col, table, seeds = world
    T = 6
    nbr, weight, num = pgl.sampling.pinsage_neighbors(g, seeds, 20, 3, T, seed=21, weights=weights)
    ref = pgl.ops.host_walk_visit_topk(indptr, col, seeds, 20, 3, T, seed=21, weights=None if weights is None else table)
    assert np.array_equal(nbr, ref[0]) and np.array_equal(num, ref[2])
    assert weight.dtype == np.float32 and weight.shape == (len(seeds), T)
    total = weight.astype(np.float64).sum(1)
    assert (np.abs(total[num > 0] - 1.0) <= T * np.finfo(np.float32).eps).all() and (num > 0).any()
    assert (total[num == 0] == 0).all() and (num == 0).any()
    assert ((weight > 0) == (ref[1] > 0)).all()
    assert np.array_equal(weight, (ref[1].astype(np.float32) / np.maximum(ref[1].sum(1, keepdims=True), 1).astype(np.float32)))
    np.random.seed(5)
    a = pgl.sampling.pinsage_neighbors(g, seeds, 20, 3, T)
    np.random.seed(5)
    b = pgl.sampling.pinsage_neighbors(g, seeds, 20, 3, T)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))               # seed=None: numpy's generator, as the walks


def test_sampler_needs_a_tensor_graph_and_the_alias_paths_resolve(pgl, world):
    with pytest.raises(ValueError, match="tensor-mode"):
        pgl.sampling.PinSageSampler(world[0], 4, 2, [3])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import pgl, pgl_amd
from pgl.sampling import PinSageSampler, pinsage_neighbors
import pgl.sampling as s
assert PinSageSampler is pgl_amd.sampling.PinSageSampler is pgl.sampling.PinSageSampler
assert pinsage_neighbors is pgl_amd.sampling.pinsage_neighbors is s.pinsage_neighbors
assert pgl.ops.walk_visit_topk is pgl_amd.ops.walk_visit_topk and pgl.ops.host_walk_visit_topk
print("ok")
""" % (root, os.path.join(root, "pgl_amd", "compat"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
