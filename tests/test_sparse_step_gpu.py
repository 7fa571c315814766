"""csrc/sparse_step.hip through pgl_amd.embedding_ops against its fp64 definition (sparse_step_defs.py), then the fused loss + step functions."""
import numpy as np
import pytest
import torch
from torch.nn.functional import softplus as _softplus

import sparse_step_defs as D
from gpu_common import dev, host, pgl  # noqa: F401
from pgl_amd import embedding_ops as eo

pytestmark = pytest.mark.gpu
N, LR = 97, 0.05


def _ids(pattern):
    """(a) segments of length 1 over a chunk boundary; (b) segments that start, end and straddle at chunk boundaries (short fix-up
    tasks); (c) one id with more than kFixShort = 16 further pieces of 32 (the long fix-up role); (d) = (b) with padding planted."""
    gen = np.random.default_rng(3)
    if pattern == "a":
        ids = gen.permutation(N)[:40]
    elif pattern in "bd":
        ids = np.repeat([5, 9, 20, 21, 60], [1, 31, 33, 64, 65])
        if pattern == "d":
            ids = np.concatenate([ids, [-1, N, -1, N + 5, 2]])
    elif pattern == "c":
        ids = np.concatenate([np.full(700, 44), [3, 96, 0, 44, 45]])
    else:
        ids = np.array([13] * int(pattern))             # "1", "0"
    return gen.permutation(ids).astype(np.int64)


def _problem(kind, form, store, d, pattern):
    gen = np.random.default_rng(7)
    ids = _ids(pattern)
    M = ids.shape[0]
    table = gen.standard_normal((N, d)).astype(np.float32)
    state = {k: np.abs(gen.standard_normal(N if kind == "rowwise_adagrad" else (N, d))).astype(np.float32) for k in D.STATE_KEYS[kind]}
    if store:                                                   # the route taken when the rows are gathered from the table itself
        rows, col, w = table, gen.integers(-1, N + 1, M), gen.standard_normal(M).astype(np.float32)
    elif form == "gathered":
        rows, col, w = gen.standard_normal((61, d)).astype(np.float32), gen.integers(-1, 62, M), gen.standard_normal(M).astype(np.float32)
    else:
        rows, col, w = gen.standard_normal((M, d)).astype(np.float32), None, None
    return ids, table, state, rows, col, w


def _run(kind, ids, table, state, rows, col, w, t0=0, scale=0.5):
    tb = dev(table)
    st = eo.SparseState(tb, kind, LR)
    st.load_state_dict(dict({k: dev(v) for k, v in state.items()}, step=t0))
    rw = tb if rows is table else dev(rows)
    eo.sparse_step(tb, dev(ids), rw, st, col=None if col is None else dev(col), w=None if w is None else dev(w), scale=scale)
    return host(tb), {k: host(v) for k, v in st.tensors.items()}, st.t


def _check(kind, got_t, got_s, ids, table, state, rows, col, w, t, scale=0.5):
    want_t, want_s, uids, bw, bs = D.step(kind, table, state, ids, rows, col, w, scale, lr=LR, eps=1e-8 if kind == "lazy_adam" else 1e-10, t=t)
    rest = np.setdiff1d(np.arange(N), uids)
    assert np.array_equal(got_t[rest], table[rest]), "an untouched row of the table changed"
    assert (np.abs(got_t[uids] - want_t[uids]) <= bw).all(), np.max(np.abs(got_t[uids] - want_t[uids]) / bw)
    for k in state:
        assert np.array_equal(got_s[k][rest], state[k][rest]), "an untouched row of state %s changed" % k
        assert (np.abs(got_s[k][uids] - want_s[k][uids]) <= bs[k]).all(), (k, np.max(np.abs(got_s[k][uids] - want_s[k][uids]) / bs[k]))


@pytest.mark.parametrize("pattern", ["a", "b", "c", "d", "1"])
@pytest.mark.parametrize("d", [4, 36, 128, 260])
@pytest.mark.parametrize("form, store", [("explicit", False), ("gathered", False), ("gathered", True)])
@pytest.mark.parametrize("kind", D.KINDS)
def test_step_against_definition(pgl, kind, form, store, d, pattern):
    prob = _problem(kind, form, store, d, pattern)
    got_t, got_s, t = _run(kind, *prob)
    _check(kind, got_t, got_s, *prob, t=1)
    again_t, again_s, _ = _run(kind, *prob)
    assert np.array_equal(got_t, again_t) and all(np.array_equal(got_s[k], again_s[k]) for k in got_s), "two calls, different bits"


@pytest.mark.parametrize("d", [8, 16, 32, 256, 516, 772])     # the lane groups of 2, 4, 8 and 64 lanes, and 3 and 4 slices per lane
@pytest.mark.parametrize("form, store", [("explicit", False), ("gathered", True)])
def test_other_row_widths(pgl, form, store, d):
    prob = _problem("lazy_adam", form, store, d, "b")
    got_t, got_s, _ = _run("lazy_adam", *prob)
    _check("lazy_adam", got_t, got_s, *prob, t=1)


def test_lazy_adam_carries_its_state(pgl):
    ids, table, state, rows, col, w = _problem("lazy_adam", "explicit", False, 36, "b")
    t1, s1, t = _run("lazy_adam", ids, table, {k: np.zeros_like(v) for k, v in state.items()}, rows, col, w)
    _check("lazy_adam", t1, s1, ids, table, {k: np.zeros_like(v) for k, v in state.items()}, rows, col, w, t=1)
    ids2 = np.concatenate([ids[:50], [1, 2]])
    t2, s2, t = _run("lazy_adam", ids2, t1, s1, rows[:52], None, None, t0=t)
    _check("lazy_adam", t2, s2, ids2, t1, s1, rows[:52], None, None, t=t)


def test_no_entries_launch_nothing(pgl):
    before = eo.LAUNCHES["sparse_step"]
    prob = _problem("adagrad", "explicit", False, 8, "0")
    got_t, got_s, t = _run("adagrad", *prob)
    assert eo.LAUNCHES["sparse_step"] == before and t == 0 and np.array_equal(got_t, prob[1]) and np.array_equal(got_s["s"], prob[2]["s"])


@pytest.mark.parametrize("pattern", ["a", "b", "c", "d", "1"])
@pytest.mark.parametrize("d", [4, 260])
def test_stored_sums(pgl, d, pattern):
    ids, table, _, rows, col, w = _problem("sgd", "gathered", False, d, pattern)
    out_ids, out_rows, count = eo.sparse_sums(dev(ids), dev(rows), N, dev(col), dev(w), 0.5)
    uids, G, A, n = D.sum_by_id(ids, rows, N, col, w, 0.5)
    U = uids.shape[0]
    assert int(count) == U and out_ids.shape[0] == min(ids.shape[0], N)
    assert np.array_equal(host(out_ids)[:U], uids) and (host(out_ids)[U:] == -1).all()
    assert (np.abs(host(out_rows)[:U] - G) <= 4.0 * n[:, None] * D.EPS32 * A + 1e-37).all()


# ---- the fused loss + step functions: P = 96 pairs, K = 3, d = 36, tables of 50 rows ----------------------------------------------------
P, K, DIM, ROWS = 96, 3, 36, 50


def _tables_after(loss_fn, tables, kinds):
    """The fp64 gradient of the existing autograd path's definition fed through the fp64 optimiser definition -> per table
    (want, bound, touched ids): the gradient rows come from torch.autograd in fp64 over the same loss written in torch."""
    leaves = [torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in tables]
    loss_fn(*leaves).backward()
    out = []
    for leaf, table, (kind, touched) in zip(leaves, tables, kinds):
        g = leaf.grad.numpy()[touched]
        zero = {k: np.zeros(table.shape[0] if kind == "rowwise_adagrad" else table.shape) for k in D.STATE_KEYS[kind]}
        want, _, uids, bw, _ = D.step(kind, table, zero, touched, g, lr=LR, eps=1e-8 if kind == "lazy_adam" else 1e-10, t=1)
        out.append((want, bw, uids))
    return out


def _assert_tables(got, tables, wants, amp):
    for g, table, (want, bw, uids) in zip(got, tables, wants):
        rest = np.setdiff1d(np.arange(table.shape[0]), uids)
        assert np.array_equal(g[rest], table[rest]), "an untouched row changed"
        assert (np.abs(g[uids] - want[uids]) <= bw + amp).all(), np.max(np.abs(g[uids] - want[uids]) / (bw + amp))


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("mode, kind", [("skipgram", "lazy_adam"), ("bpr", "rowwise_adagrad"), ("skipgram", "sgd"), ("bpr", "adagrad")])
def test_pair_steps(pgl, mode, kind, shared):
    gen = np.random.default_rng(11)
    emb = (0.5 * gen.standard_normal((ROWS, DIM))).astype(np.float32)
    ctx = emb if shared else (0.5 * gen.standard_normal((ROWS, DIM))).astype(np.float32)
    src, dst, neg = gen.integers(0, 40, P), gen.integers(0, 40, P), gen.integers(0, 40, (P, K))      # rows 40 .. 49 stay untouched
    e = dev(emb)
    c = e if shared else dev(ctx)
    se, sc = eo.SparseState(e, kind, LR), None if shared else eo.SparseState(c, kind, LR)
    if mode == "skipgram":
        want_loss = eo.skip_gram_loss(e, c, dev(src), dev(dst), dev(neg))
        loss = eo.skip_gram_step(e, c, dev(src), dev(dst), dev(neg), se, sc)
    else:
        want_loss = eo.bpr_loss(e, c, dev(src), dev(dst), dev(neg))
        loss = eo.bpr_step(e, c, dev(src), dev(dst), dev(neg), se, sc)
    assert np.array_equal(host(loss), host(want_loss)), "the step's loss is not the loss's bits"
    tgt = torch.tensor(np.concatenate([dst[:, None], neg], 1))

    def loss_fn(E, C=None):
        z = (E[torch.tensor(src)][:, None, :] * (E if C is None else C)[tgt]).sum(-1)
        if mode == "skipgram":
            return (_softplus(-z[:, 0]).sum() + _softplus(z[:, 1:]).sum()) / P
        return _softplus(z[:, 1:] - z[:, :1]).sum() / (P * K)
    t_ids = np.unique(tgt.numpy())
    kinds = [(kind, np.unique(np.concatenate([src, t_ids])))] if shared else [(kind, np.unique(src)), (kind, t_ids)]
    tables = [emb] if shared else [emb, ctx]
    wants = _tables_after(loss_fn, tables, kinds)
    # a coefficient g = w sigma(z), z a DIM-term fp32 dot product: |dz| <= DIM eps sum_k |e_k c_k| <= DIM eps |z| kappa, sigma' <= sigma,
    # so |dg| / |g| <= DIM eps kappa |z| + 4 eps (the softplus chain); here |z| < 4 and the rows of a sum have like magnitudes, so a summed
    # row is off by less than 8 DIM eps of itself.  sgd moves by lr |dG| <= lr 8 DIM eps |G| with |G| < 1; the normalised updates
    # lr G / (|G| + eps), lr G / rms(G) from zero state are homogeneous of degree 0 and move by at most lr times that relative error
    amp = 8 * DIM * D.EPS32 * LR
    _assert_tables([host(e)] if shared else [host(e), host(c)], tables, wants, amp)


@pytest.mark.parametrize("model, kind", [("distmult", "adagrad"), ("transe", "lazy_adam")])
def test_kge_step(pgl, model, kind):
    gen = np.random.default_rng(13)
    ent, rel = (0.5 * gen.standard_normal((ROWS, 40))).astype(np.float32), (0.5 * gen.standard_normal((ROWS, 40))).astype(np.float32)
    h, r, t, neg = gen.integers(0, 40, P), gen.integers(0, 40, P), gen.integers(0, 40, P), gen.integers(0, 40, (4, K))
    E, R = dev(ent), dev(rel)
    want_loss = eo.kge_loss(E, R, dev(h), dev(r), dev(t), dev(neg), model)
    loss = eo.kge_step(E, R, dev(h), dev(r), dev(t), dev(neg), model, eo.SparseState(E, kind, LR), eo.SparseState(R, kind, LR))
    assert np.array_equal(host(loss), host(want_loss))

    h_, r_, t_ = torch.tensor(h), torch.tensor(r), torch.tensor(t)

    def loss_fn(Et, Rt):
        a = Et[h_] + Rt[r_] if model == "transe" else Et[h_] * Rt[r_]
        b = Et[torch.tensor(neg)].repeat_interleave(P // 4, 0)                      # [P, K, d]: chunk c's negatives for its positives
        if model == "transe":
            pos = 12.0 - (a - Et[t_]).pow(2).sum(-1).clamp_min(1e-30).sqrt()
            s = 12.0 - (a[:, None, :] - b).pow(2).sum(-1).clamp_min(1e-30).sqrt()
        else:
            pos, s = (a * Et[t_]).sum(-1), (a[:, None, :] * b).sum(-1)
        return (_softplus(-pos).mean() + _softplus(s).mean(1).mean()) / 2
    kinds = [(kind, np.unique(np.concatenate([h, t, neg.reshape(-1)]))), (kind, np.unique(r))]
    wants = _tables_after(loss_fn, [ent, rel], kinds)
    _assert_tables([host(E), host(R)], [ent, rel], wants, 8 * 40 * D.EPS32 * LR)
