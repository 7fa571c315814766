"""The fp64 definition of the sparse embedding step (sparse_step_defs.py) against torch.optim, and the front end's refusals."""
import numpy as np
import pytest
import torch

import sparse_step_defs as D
from pgl_amd.embedding_ops import SparseState, sparse_step

N, DIM, LR = 11, 4, 0.05


def _batches():
    gen = np.random.default_rng(5)
    return [(np.array([3, 7, 3, 0, 7, 3, 9]), gen.standard_normal((7, DIM))), (np.array([7, 7, 1, 3, 10]), gen.standard_normal((5, DIM)))]


@pytest.mark.parametrize("kind", D.KINDS)
def test_definition_matches_torch_optim_over_two_steps(kind):
    table = np.random.default_rng(1).standard_normal((N, DIM))
    p = torch.nn.Parameter(torch.tensor(table))
    eps = 1e-8 if kind == "lazy_adam" else 1e-10
    opt = {"sgd": lambda: torch.optim.SGD([p], lr=LR), "adagrad": lambda: torch.optim.Adagrad([p], lr=LR, eps=eps),
           "lazy_adam": lambda: torch.optim.SparseAdam([p], lr=LR, eps=eps), "rowwise_adagrad": lambda: None}[kind]()
    state = {k: np.zeros(N if kind == "rowwise_adagrad" else (N, DIM)) for k in D.STATE_KEYS[kind]}
    drift = np.zeros((N, DIM))                                  # lazy Adam: the steps' eps-placement differences add up in the table
    moment, weight = np.zeros(N), table.copy()                  # shared_embedding.py:335-344, restated
    for t, (ids, rows) in enumerate(_batches(), 1):
        uids, G, _, _ = D.sum_by_id(ids, rows, N)
        before = state
        table, state, _, _, _ = D.step(kind, table, state, ids, rows, lr=LR, eps=eps, t=t)
        if kind == "rowwise_adagrad":
            moment[uids] += (G * G).mean(1)
            weight[uids] += -LR * G / (np.sqrt(moment[uids]) + 1e-10).reshape((-1, 1))
            np.testing.assert_allclose(table, weight, rtol=1e-14, atol=0)
            np.testing.assert_allclose(state["s"], moment, rtol=1e-14, atol=0)
            continue
        dense = np.zeros((N, DIM))
        dense[uids] = G
        p.grad = torch.tensor(dense).to_sparse(1) if kind == "lazy_adam" else torch.tensor(dense)
        opt.step()
        tol = 1e-14 * (1 + np.abs(table))
        if kind == "lazy_adam":
            # SparseAdam adds eps to sqrt(v) before the bias correction, the definition (Paddle's, torch.optim.Adam's) after it: its
            # step is lr mhat / (a + eps / sqrt(c2)) against lr mhat / (a + eps), a = sqrt(v / c2), and
            # |1 / (a + e1) - 1 / (a + e2)| <= |e1 - e2| / a^2 <= (eps / sqrt(c2)) / a^2
            c2 = 1 - 0.999 ** t
            mhat, vhat = state["m"] / (1 - 0.9 ** t), state["v"] / c2
            drift = drift + LR * np.abs(mhat) * (eps / np.sqrt(c2)) / np.maximum(vhat, 1e-300)
            tol = tol + drift
            untouched = np.setdiff1d(np.arange(N), uids)
            assert all(np.array_equal(state[k][untouched], before[k][untouched]) for k in "mv")
        assert (np.abs(p.detach().numpy() - table) <= tol).all()


@pytest.mark.parametrize("case, exc", [("dtype", TypeError), ("ids_dtype", TypeError), ("cpu", ValueError), ("d6", ValueError), ("d1028", ValueError),
                                       ("w_without_col", ValueError), ("shape", ValueError)])
def test_refusals_come_before_any_launch(case, exc):
    d = {"d6": 6, "d1028": 1028}.get(case, 8)
    table, ids, rows, kw = torch.zeros(5, d), torch.tensor([1, 2]), torch.zeros(2, d), {}
    if case == "dtype":
        rows = rows.double()
    elif case == "ids_dtype":
        ids = ids.int()
    elif case == "w_without_col":
        kw = {"w": torch.ones(2)}
    elif case == "shape":
        rows = torch.zeros(3, d)
    with pytest.raises(exc, match="pgl_amd sparse_step"):
        sparse_step(table, ids, rows, SparseState(table, "adagrad", 0.1), **kw)      # (every tensor on the CPU: nothing can launch)
