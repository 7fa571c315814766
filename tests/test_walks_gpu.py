"""Random walks and skip-gram pairs on the MI355X (walk.hip): bit-identical to the host twin on an RMAT graph (hubs, dead ends,
multi-edges), reproducible from the seed, exact second-order laws, device skip-gram pairs against a numpy restatement of the
window hash, the reference-named functions on a tensor graph, and examples/train_deepwalk.py end to end."""
import os
import sys

import numpy as np
import pytest
import torch

import walk_defs as D
from gpu_common import dev, host, pgl      # noqa: F401  (pgl: the module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rmat_graph(pgl):
    from pgl_amd.utils.rmat import rmat_edges
    e = rmat_edges(16, 1 << 20, seed=7)
    gn = pgl.Graph(edges=e.numpy(), num_nodes=1 << 16)
    gt = pgl.Graph(edges=e.numpy(), num_nodes=1 << 16).tensor()
    return gn, gt


# (p, q, plus, walkers, steps, max_trials): scan-only runs are smaller (a scan reads every successor of a hub)
BITEXACT = [(1.0, 1.0, False, 100000, 40, 64), (0.25, 4.0, False, 100000, 40, 64), (4.0, 0.25, False, 100000, 40, 64),
            (0.25, 4.0, True, 100000, 40, 64), (4.0, 0.25, False, 20000, 20, 0), (0.25, 4.0, True, 5000, 16, 0)]


@pytest.mark.parametrize("seed", [1, 2 ** 40 + 3])
@pytest.mark.parametrize("p,q,plus,W,steps,max_trials", BITEXACT)
def test_device_walks_equal_the_host_twin(pgl, rmat_graph, p, q, plus, W, steps, max_trials, seed):
    gn, gt = rmat_graph
    starts = np.random.default_rng(seed % 1000).integers(0, gn.num_nodes, W)
    indptr, col = gn._csr_succ_sorted()
    csr = gt._csr_succ_sorted()
    assert np.array_equal(host(csr.indptr), indptr) and np.array_equal(host(csr.col32), col)   # the same sorted index
    want = pgl.ops.host_random_walk(indptr, col, starts, steps, p, q, plus, seed=seed, max_trials=max_trials)
    got = pgl.ops.random_walk(csr, dev(starts), steps, p, q, plus, seed=seed, max_trials=max_trials)
    assert np.array_equal(host(got[1]), want[1])
    assert np.array_equal(host(got[0]), want[0])
    assert (want[1] < steps + 1).any() and (want[1] == steps + 1).any()   # dead ends met, full-length walks too


def test_device_reproducibility(pgl, rmat_graph):
    _, gt = rmat_graph
    nodes = torch.arange(0, gt.num_nodes, 3, device="cuda")
    a = pgl.sampling.walks(gt, nodes, 30, p=0.5, q=2.0, seed=9)
    b = pgl.sampling.walks(gt, nodes, 30, p=0.5, q=2.0, seed=9)
    c = pgl.sampling.walks(gt, nodes, 30, p=0.5, q=2.0, seed=10)
    assert a[0].is_cuda and a[1].is_cuda
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    np.random.seed(4); d = pgl.sampling.walks(gt, nodes, 30, plus=True, p=0.5, q=2.0)
    np.random.seed(4); e = pgl.sampling.walks(gt, nodes, 30, plus=True, p=0.5, q=2.0)
    np.random.seed(5); f = pgl.sampling.walks(gt, nodes, 30, plus=True, p=0.5, q=2.0)
    assert torch.equal(d[0], e[0]) and not torch.equal(d[0], f[0])


def test_device_range_check(pgl, rmat_graph):
    _, gt = rmat_graph
    for bad in ([gt.num_nodes], [-1], [0, 1 << 40]):
        with pytest.raises(ValueError):
            pgl.sampling.walks(gt, torch.tensor(bad, device="cuda"), 5, seed=1)


@pytest.mark.parametrize("max_trials", [None, 64, 0])
@pytest.mark.parametrize("mode,p,q,steps", D.LAW_CASES)
def test_exact_walk_laws_device(pgl, mode, p, q, steps, max_trials):
    g = pgl.Graph(edges=D.EDGES, num_nodes=D.N).tensor()
    csr = g._csr_succ_sorted()
    succ = D.successors()
    W = 200000
    for start in (0, 2):
        paths, _ = pgl.ops.random_walk(csr, torch.full((W,), start, dtype=torch.int64, device="cuda"), steps, p, q,
                                       mode == "plus", seed=300 + start, max_trials=max_trials)
        D.assert_law(host(paths), D.path_law(succ, start, steps, p, q, mode), (mode, p, q, start, max_trials))


def test_skip_gram_pairs_on_device(pgl, rmat_graph):
    _, gt = rmat_graph
    rng = np.random.default_rng(2)
    starts = rng.integers(0, gt.num_nodes, 3000)
    paths, lengths = pgl.ops.random_walk(gt._csr_succ_sorted(), dev(starts), 12, seed=5)
    # hand-made rows too: a length-1 walk, padding, repeated ids (a self-loop walk and an a-b-a-b walk)
    extra = np.full((4, 13), -1, np.int64)
    extra[0, 0] = 7
    extra[1, :13] = 5
    extra[2, :9] = [1, 2, 1, 2, 1, 2, 1, 2, 1]
    extra[3, :4] = [3, 4, 3, 3]
    P = np.concatenate([host(paths), extra])
    L = np.concatenate([host(lengths), [1, 13, 9, 4]])
    assert (L == 1).any() and (L < 13).any()
    for win, seed in ((5, 0), (1, 7), (3, 2 ** 63 + 1)):
        src, dst = pgl.ops.skip_gram_pairs(dev(P), dev(L), win, seed)
        ws, wd = D.skip_gram_restated(P, L, win, seed)
        assert np.array_equal(host(src), ws) and np.array_equal(host(dst), wd), (win, seed)
    e = pgl.ops.skip_gram_pairs(dev(extra[:1]), dev(np.array([1])), 5, 0)
    assert e[0].numel() == 0 and e[1].numel() == 0


def test_reference_named_functions_on_a_tensor_graph(pgl, rmat_graph):
    gn, gt = rmat_graph
    nodes = list(range(0, 4000, 7))
    for f, kw in ((pgl.sampling.random_walk, {}), (pgl.sampling.node2vec_walk, dict(p=0.25, q=4.0)),
                  (pgl.sampling.node2vec_walk_plus, dict(p=4.0, q=0.25)), (pgl.sampling.node2vec_walk, dict(p=1.0, q=1.0))):
        a = f(gt, nodes, 10, seed=17, **kw)
        b = f(gn, nodes, 10, seed=17, **kw)
        assert a == b and len(a) == len(nodes) and [w[0] for w in a] == nodes
        np.random.seed(8); c = f(gt, torch.tensor(nodes, device="cuda"), 10, **kw)
        np.random.seed(8); d = f(gn, np.array(nodes), 10, **kw)
        assert c == d


def test_train_deepwalk_example(pgl):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_deepwalk
    finally:
        sys.path.pop(0)
    r = train_deepwalk.main(["--steps", "300", "--seed", "0"])
    assert r["loss_last"] < 0.8 * r["loss_first"], r
    assert r["intra_cos"] > r["inter_cos"] + 0.15, r
