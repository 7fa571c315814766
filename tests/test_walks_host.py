"""Random walks on the host twin (pglamd_random_walk_host, numpy-mode graphs) and graph_kernel.skip_gram_gen_pair: structure,
the reference's step-count quirks, exact second-order laws (chi-square against the definition, which is itself checked against
the reference's compiled node2vec samplers), and the pgl import paths (pgl/sampling/walk.py, pgl/graph_kernel.pyx)."""
import numpy as np
import pytest

import walk_defs as D


@pytest.fixture(scope="module")
def pgl():
    import pgl_amd
    return pgl_amd


def _graph(pgl):
    return pgl.Graph(edges=D.EDGES, num_nodes=D.N)


def _assert_walks_follow_edges(walks, succ):
    for w in walks:
        for a, b in zip(w[:-1], w[1:]):
            assert b in succ[a], (w, a, b)


def test_walk_structure_and_step_counts(pgl):
    g, succ = _graph(pgl), D.successors()
    nodes = list(range(D.N)) * 50
    rw = pgl.sampling.random_walk(g, nodes, 6, seed=3)
    n2v = pgl.sampling.node2vec_walk(g, nodes, 6, p=0.5, q=2.0, seed=3)
    plus = pgl.sampling.node2vec_walk_plus(g, nodes, 6, p=0.5, q=2.0, seed=3)
    same = pgl.sampling.node2vec_walk(g, nodes, 6, p=1.0, q=1.0, seed=3)
    assert same == rw                                             # p == q == 1 is random_walk, unchanged
    for walks, depth in ((rw, 6), (n2v, 7), (plus, 7)):          # node2vec takes max_depth steps: max_depth + 1 nodes
        assert len(walks) == len(nodes)
        assert [w[0] for w in walks] == nodes
        _assert_walks_follow_edges(walks, succ)
        for w in walks:
            assert 1 <= len(w) <= depth
            assert len(w) == depth or not succ[w[-1]], w         # shorter only when it stopped at a dead end
    assert all(len(w) == 1 for w, s in zip(rw, nodes) if s == 4)  # a dead-end start: the start alone
    assert max(len(w) for w in rw) == 6 and max(len(w) for w in n2v) == 7


def test_walk_edge_cases(pgl):
    g = _graph(pgl)
    assert pgl.sampling.random_walk(g, [], 5) == []
    assert pgl.sampling.node2vec_walk(g, np.array([], np.int64), 5, p=2.0, q=0.5) == []
    assert pgl.sampling.random_walk(g, [0, 4], 0, seed=1) == [[0], [4]]
    assert pgl.sampling.random_walk(g, [0, 4], 1, seed=1) == [[0], [4]]
    assert pgl.sampling.node2vec_walk(g, [0, 4], 0, p=2.0, q=0.5, seed=1) == [[0], [4]]
    w = pgl.sampling.node2vec_walk(g, [0, 4], 1, p=2.0, q=0.5, seed=1)
    assert len(w[0]) == 2 and w[1] == [4]
    for bad in ([D.N], [-1], [0, 99]):
        with pytest.raises(ValueError):
            pgl.sampling.random_walk(g, bad, 4, seed=1)
        with pytest.raises(ValueError):
            pgl.sampling.node2vec_walk_plus(g, bad, 4, p=2.0, q=0.5, seed=1)
    with pytest.raises(ValueError):
        pgl.sampling.node2vec_walk(g, [0], 4, p=0.0, q=1.0)


def test_seed_none_follows_numpy_global_seed(pgl):
    g = _graph(pgl)
    np.random.seed(11); a = pgl.sampling.node2vec_walk(g, list(range(D.N)) * 20, 8, p=0.5, q=2.0)
    np.random.seed(11); b = pgl.sampling.node2vec_walk(g, list(range(D.N)) * 20, 8, p=0.5, q=2.0)
    np.random.seed(12); c = pgl.sampling.node2vec_walk(g, list(range(D.N)) * 20, 8, p=0.5, q=2.0)
    assert a == b and a != c
    assert pgl.sampling.random_walk(g, [0] * 50, 9, seed=5) == pgl.sampling.random_walk(g, [0] * 50, 9, seed=5)


def test_host_threads_do_not_change_the_walks(pgl):
    indptr, col = _graph(pgl)._csr_succ_sorted()
    starts = np.arange(5000) % D.N
    for mode in ((1.0, 1.0, False), (4.0, 0.25, False), (0.25, 4.0, True)):
        one = pgl.ops.host_random_walk(indptr, col, starts, 12, *mode, seed=9, threads=1)
        many = pgl.ops.host_random_walk(indptr, col, starts, 12, *mode, seed=9, threads=7)
        assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])


def test_sorted_successor_index(pgl):
    indptr, col = _graph(pgl)._csr_succ_sorted()
    succ = D.successors()
    for v in range(D.N):
        assert col[indptr[v]:indptr[v + 1]].tolist() == sorted(succ[v])


def test_plus_law_differs_from_node2vec_on_the_test_graph():
    succ = D.successors()
    a, b = D.path_law(succ, 0, 3, 4.0, 0.25, "node2vec"), D.path_law(succ, 0, 3, 4.0, 0.25, "plus")
    assert abs(sum(a.values()) - 1) < 1e-12 and abs(sum(b.values()) - 1) < 1e-12
    assert max(abs(a.get(k, 0) - b.get(k, 0)) for k in set(a) | set(b)) > 0.01


@pytest.mark.parametrize("max_trials", [None, 64, 0])
@pytest.mark.parametrize("mode,p,q,steps", D.LAW_CASES)
def test_exact_walk_laws_host(pgl, mode, p, q, steps, max_trials):
    indptr, col = _graph(pgl)._csr_succ_sorted()
    succ = D.successors()
    W = 60000
    for start in (0, 2):
        paths, lengths = pgl.ops.host_random_walk(indptr, col, np.full(W, start), steps, p, q, mode == "plus", seed=100 + start,
                                                  max_trials=max_trials)
        D.assert_law(paths, D.path_law(succ, start, steps, p, q, mode), (mode, p, q, start, max_trials))


@pytest.mark.parametrize("plus", [False, True])
@pytest.mark.parametrize("p,q", [(0.25, 4.0), (4.0, 0.25), (0.5, 0.5)])
def test_definition_matches_the_reference_samplers(ref_native, plus, p, q):
    """graph_kernel.node2vec_sample / node2vec_plus_sample (pyx:140-224) against draws from step_law's definition, on the same
    (succ, prev_succ, prev): two-sample chi-square, the formula of test_sample_neighbors_matches_the_reference_sampler_distribution."""
    from scipy.stats import chi2
    succ = np.array([3, 5, 5, 7, 8, 9, 11, 12], np.int64)          # 5 twice: a multi-edge
    prev = 7                                                         # the return candidate
    prev_succ = np.array([5, 8, 20], np.int64)                       # 5 and 8 are "in" (weight 1)
    draws = 20000
    cand = sorted(set(succ.tolist()))
    theirs = np.zeros(len(cand), np.int64)
    for _ in range(draws):
        x = ref_native.node2vec_plus_sample(succ, prev_succ, prev, p, q)[0] if plus else \
            ref_native.node2vec_sample(succ, prev_succ, prev, p, q)
        theirs[cand.index(int(x))] += 1
    w = np.array([1.0 / p if x == prev else (1.0 if x in set(prev_succ.tolist()) else 1.0 / q) for x in succ.tolist()])
    law = {}
    for x, wx in zip(succ.tolist(), w / w.sum()):
        law[x] = law.get(x, 0.0) + wx
    ours = np.bincount(np.random.default_rng(7).choice(len(cand), draws, p=[law[c] for c in cand]), minlength=len(cand))
    a, b = ours.astype(np.float64), theirs.astype(np.float64)
    stat2 = float(((a - b) ** 2 / np.maximum(a + b, 1)).sum())
    assert float(chi2.sf(stat2, len(cand) - 1)) > 1e-4, (stat2, a, b)


def test_skip_gram_gen_pair_is_the_references(pgl, ref_native):
    rng = np.random.default_rng(4)
    for n, win in ((0, 5), (1, 5), (2, 1), (17, 3), (80, 5), (200, 10)):
        walk = rng.integers(0, 6, n).tolist()                        # few distinct ids: many repeats
        for seed in (0, 1):
            np.random.seed(seed); ref = ref_native.skip_gram_gen_pair(walk, win)
            np.random.seed(seed); ours = pgl.graph_kernel.skip_gram_gen_pair(walk, win)
            assert list(ours[0]) == list(ref[0]) and list(ours[1]) == list(ref[1]), (n, win, seed)
            after = np.random.randint(1 << 30)                       # ours consumed ONE draw of len(walk) windows, as the reference
            np.random.seed(seed); np.random.randint(1, win + 1, dtype=np.int64, size=n)
            assert after == np.random.randint(1 << 30)
    np.random.seed(3); a = pgl.graph_kernel.skip_gram_gen_pair([1, 2, 3, 4])
    np.random.seed(3); b = ref_native.skip_gram_gen_pair([1, 2, 3, 4])
    assert list(a[0]) == list(b[0]) and list(a[1]) == list(b[1])     # the default win_size


def test_import_paths_through_the_alias():
    """`import pgl` (pgl_amd/compat) in a fresh interpreter: the reference's walk import paths resolve to the engine's functions."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys
sys.path[:0] = [%r, %r]
import pgl
import pgl.sampling.walk as walk_mod
from pgl.sampling import random_walk, node2vec_walk, node2vec_walk_plus
from pgl.sampling.walk import random_walk as rw2
from pgl.graph_kernel import skip_gram_gen_pair
import pgl_amd
assert walk_mod is pgl_amd.sampling and rw2 is random_walk is pgl_amd.sampling.random_walk
assert node2vec_walk is pgl_amd.sampling.node2vec_walk and node2vec_walk_plus is pgl_amd.sampling.node2vec_walk_plus
assert skip_gram_gen_pair is pgl_amd.graph_kernel.skip_gram_gen_pair
print("ok")
""" % (root, os.path.join(root, "pgl_amd", "compat"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout + r.stderr)[-3000:]
