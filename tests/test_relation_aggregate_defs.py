"""tests/relation_aggregate_defs.py against the oracle's numpy restatement (oracle/ref_ops.py np_send_u_recv, per relation, summed):
the definition the GPU tests hold pgl_amd.ops.aggregate_relations to is the reference's RGCN aggregation loop
(pgl/nn/conv.py:1014-1019), in fp64.  Also: the engine refuses a numpy HeterGraph as Graph.send_recv does."""
import numpy as np
import pytest

import ref_ops as R
import relation_aggregate_defs as D

N = 40


def _edges(seed=0):
    """Three relations over 40 nodes: a random one with duplicates and self-loops, one WITHOUT any edge, one that leaves rows
    10 .. 39 empty; rows 30 .. 39 are empty in every relation."""
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, N, 300), rng.integers(0, 30, 300))
    a[0][:20] = a[1][:20]                                                  # self-loops
    a = (np.concatenate([a[0], a[0][:50]]), np.concatenate([a[1], a[1][:50]]))   # duplicate edges
    b = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    c = (rng.integers(0, N, 60), rng.integers(0, 10, 60))
    return [a, b, c]


@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("stacked_x", [False, True])
@pytest.mark.parametrize("per_relation", [False, True])
@pytest.mark.parametrize("out_size", [None, 17])
def test_definition_is_the_sum_of_the_per_relation_send_recv(op, stacked_x, per_relation, out_size):
    edges = _edges()
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, N, 5)) if stacked_x else rng.standard_normal((N, 5))
    indptr, col = D.stack_edges(edges, N)
    got, abs_terms, n_terms = D.relation_aggregate(x, indptr, col, op, out_size, per_relation)
    # (rows >= M are not computed: the first M rows of the whole result; the oracle itself takes no destination beyond out_size)
    parts = [R.np_send_u_recv(x[r] if stacked_x else x, s, d, op)[:out_size or N] for r, (s, d) in enumerate(edges)]
    want = np.stack(parts, 1) if per_relation else np.sum(parts, 0)
    assert got.shape == want.shape and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)
    M = out_size or N
    assert not got[30:M].any() and not (got[:, 1] if per_relation else np.zeros(1)).any()      # empty rows, the empty relation
    assert (abs_terms >= np.abs(got) - 1e-12).all()
    indeg = sum(np.bincount(d, minlength=N)[:M] for _, d in edges)
    nonempty = sum((np.bincount(d, minlength=N)[:M] > 0).astype(int) for _, d in edges)
    if not per_relation:
        assert np.array_equal(n_terms[:, 0], indeg + nonempty)


@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("stacked_x", [False, True])
@pytest.mark.parametrize("per_relation", [False, True])
def test_gradient_definition_is_the_torch_autograd_of_the_edge_by_edge_form(op, stacked_x, per_relation):
    import torch
    edges = _edges(2)
    rng = np.random.default_rng(3)
    M = 17
    x = torch.tensor(rng.standard_normal((3, N, 4)) if stacked_x else rng.standard_normal((N, 4)), requires_grad=True)
    g = rng.standard_normal((M, 3, 4)) if per_relation else rng.standard_normal((M, 4))
    lists = [(torch.as_tensor(s), torch.as_tensor(d)) for s, d in edges]
    out = D.t_send_recv_relations(x, lists, op, M, per_relation)
    indptr, col = D.stack_edges(edges, N)
    np.testing.assert_allclose(out.detach().numpy(), D.relation_aggregate(x.detach().numpy(), indptr, col, op, M, per_relation)[0],
                               rtol=1e-13, atol=1e-13)
    out.backward(torch.as_tensor(g))
    want, _, _ = D.relation_aggregate_grad(g, indptr, col, tuple(x.shape), op, per_relation)
    np.testing.assert_allclose(x.grad.numpy(), want, rtol=1e-13, atol=1e-13)


def test_col_scale_scales_every_term_by_its_column():
    edges = _edges(4)
    rng = np.random.default_rng(5)
    x, c = rng.standard_normal((N, 3)), rng.standard_normal((3, N))
    indptr, col = D.stack_edges(edges, N)
    got = D.relation_aggregate(x, indptr, col, "sum", None, False, c)[0]
    want = D.relation_aggregate(x[None] * c[:, :, None], indptr, col, "sum")[0]
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)


def test_numpy_hetergraph_refuses_send_recv_relations_like_send_recv():
    import pgl_amd
    s, d = _edges()[0]
    hg = pgl_amd.HeterGraph(edges={"a": np.stack([s, d], 1)}, num_nodes=N)
    x = np.zeros((N, 4), np.float32)
    with pytest.raises(ValueError) as ours:
        hg.send_recv_relations(x)
    with pytest.raises(ValueError) as theirs:
        hg["a"].send_recv(x)
    assert str(ours.value) == str(theirs.value)
    assert pgl_amd.ops.aggregate_relations.__doc__ and pgl_amd.ops.LONG_ROW >= 64
