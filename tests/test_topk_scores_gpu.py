"""embedding_ops.topk_scores / sampling.recommend (csrc/topk_scores.hip) against a plain fp64 restatement on the host: scores, the
excluded pairs dropped, lexsort by (-score, id).  Integer-valued inputs make every fp32 chain exact in any order, so ids and scores
must EQUAL the reference; real-valued inputs are held per pair to the re-association bound of the definition's own terms."""
import functools

import numpy as np
import pytest
import torch

import pool_defs
from gpu_common import dev, host, pgl, reassociation_bound  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4, 1), (33, 130, 8, 5), (32, 4097, 64, 20), (70, 1000, 100, 64), (5, 300, 1024, 33)]
EXTRA = 6                                     # graph nodes past the table: they carry exclusion rows, never candidates


@functools.lru_cache(maxsize=None)
def case(Q, N, d, k, sub, real):
    """-> dict of host arrays: the inputs, the exclusion's edges and query ids, the dropped mask [Q, N], fp64 scores and their |terms|.
    Rows 0 .. 5 of the exclusion index: empty, duplicates, all of [lo, hi) but its first id (fewer than k are left), the whole table,
    two random ones."""
    rng = np.random.default_rng(Q * 1000 + N + int(sub))
    draw = (lambda *s: rng.standard_normal(s)) if real else (lambda *s: rng.integers(-2, 3, s))
    query, table, bias = (draw(Q, d).astype(np.float32), draw(N, d).astype(np.float32), draw(N).astype(np.float32))
    lo, hi = (N // 4, N - N // 3) if sub else (0, N)
    rand = lambda: rng.choice(N, min(N, 20), replace=False).tolist()
    rows = [[], [lo, lo, hi - 1, hi - 1, lo], list(range(lo + 1, hi)), list(range(N)), rand(), rand()]
    qids = (np.arange(Q) + 2) % 7                                    # rows 2, 3, 4, 5, then an id outside the index, 0, 1, repeats
    qids[qids == 6] = N + EXTRA + 100
    dropped = np.zeros((Q, N), bool)
    for q, u in enumerate(qids):
        if u < len(rows):
            dropped[q, rows[u]] = True
    edges = np.array([(u, j) for u, r in enumerate(rows) for j in r], np.int64).reshape(-1, 2)
    s64 = query.astype(np.float64) @ table.astype(np.float64).T
    return dict(query=query, table=table, bias=bias, lo=lo, hi=hi, qids=qids.astype(np.int64), dropped=dropped, edges=edges, s64=s64,
                abs64=np.abs(query).astype(np.float64) @ np.abs(table).astype(np.float64).T)


def reference(s32, dropped, lo, hi, k):
    """The definition: per query the candidates of [lo, hi) that are not dropped, NaN first, then score descending (IEEE equality),
    then id ascending; (-1, -inf) behind them."""
    ids, scores = np.full((len(s32), k), -1, np.int64), np.full((len(s32), k), -np.inf, np.float32)
    for q in range(len(s32)):
        cand = np.arange(lo, hi)[~dropped[q, lo:hi]]
        v = s32[q, cand]
        nan = np.isnan(v)
        order = np.lexsort((cand, np.where(nan, 0.0, -v.astype(np.float64)) + 0.0, ~nan))[:k]
        ids[q, :len(order)], scores[q, :len(order)] = cand[order], v[order]
    return ids, scores


def run(pgl, c, k, excl, bias, slices):
    from pgl_amd import embedding_ops as E
    kw = {}
    if excl:
        g = pgl.Graph(edges=c["edges"], num_nodes=c["table"].shape[0] + EXTRA).tensor()
        kw = dict(exclude=g._csr_succ_sorted(), query_ids=dev(c["qids"]))
    ids, scores = E.topk_scores(dev(c["query"]), dev(c["table"]), k, lo=c["lo"], hi=c["hi"], bias=dev(c["bias"]) if bias else None,
                                slices=slices, **kw)
    return host(ids), host(scores)


@pytest.mark.parametrize("slices", [None, 1, 3, 7])
@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("excl", [False, True])
@pytest.mark.parametrize("Q,N,d,k", SHAPES)
def test_exact(pgl, Q, N, d, k, excl, bias, sub, slices):
    c = case(Q, N, d, k, sub, False)
    s32 = (c["s64"] + (c["bias"] if bias else 0.0)).astype(np.float32)              # |s| <= 4 * 1024 + 2: exact in fp32
    want_ids, want_scores = reference(s32, c["dropped"] if excl else np.zeros_like(c["dropped"]), c["lo"], c["hi"], k)
    ids, scores = run(pgl, c, k, excl, bias, slices)
    assert np.array_equal(ids, want_ids) and np.array_equal(scores, want_scores)


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_scores_monotone_in_id(pgl, sign, slices):
    """Scores rise with j: every candidate beats the threshold; they fall: none after the first k does."""
    from pgl_amd import embedding_ops as E
    Q, N, d, k = 33, 1000, 8, 20
    query, table = np.zeros((Q, d), np.float32), np.zeros((N, d), np.float32)
    query[:, 0], table[:, 0] = sign, np.arange(N)
    ids, scores = E.topk_scores(dev(query), dev(table), k, slices=slices)
    want = np.arange(N - 1, N - 1 - k, -1) if sign > 0 else np.arange(k)
    assert np.array_equal(host(ids), np.broadcast_to(want, (Q, k)))
    assert np.array_equal(host(scores), np.broadcast_to((sign * want).astype(np.float32) + 0.0, (Q, k)))


@pytest.mark.parametrize("Q,N,d,k", SHAPES)
def test_real_valued(pgl, Q, N, d, k):
    c = case(Q, N, d, k, False, True)
    s64 = c["s64"] + c["bias"]
    bar = reassociation_bound(c["abs64"] + np.abs(c["bias"]), d + 2)
    (ids, scores), (ids5, scores5) = run(pgl, c, k, True, True, 1), run(pgl, c, k, True, True, 5)
    assert np.array_equal(ids, ids5) and np.array_equal(scores.view(np.uint32), scores5.view(np.uint32))     # slicing: the same bits
    for q in range(Q):
        left = np.flatnonzero(~c["dropped"][q])
        n = min(k, len(left))
        got = ids[q, :n]
        assert (ids[q, n:] == -1).all() and np.isneginf(scores[q, n:]).all()
        assert np.isin(got, left).all() and len(np.unique(got)) == n                # in range, not excluded, distinct
        assert (np.abs(scores[q, :n] - s64[q, got]) <= bar[q, got]).all()           # each score against the fp64 score of its own id
        assert np.array_equal(np.lexsort((got, -scores[q, :n].astype(np.float64))), np.arange(n))   # ordered by the returned (score, id)
        rest = np.setdiff1d(left, got)
        if n:                                                                       # completeness, every candidate not returned
            assert (s64[q, rest] <= s64[q, got[-1]] + bar[q, rest] + bar[q, got[-1]]).all()


def test_recommend(pgl):
    U, I, d, k = 40, 70, 8, 10
    rng = np.random.default_rng(5)
    ui = np.unique(np.stack([rng.integers(0, U, 300), U + rng.integers(0, I, 300)], 1), axis=0)
    g = pgl.Graph(edges=np.concatenate([ui, ui[:, ::-1]]), num_nodes=U + I).tensor()
    emb = rng.integers(-2, 3, (U + I, d)).astype(np.float32)
    nodes = np.array([3, 0, 39, 3, 17], np.int64)
    ids, scores = pgl.sampling.recommend(g, dev(nodes), dev(emb), k, candidates=(U, U + I))
    s = (emb[nodes].astype(np.float64) @ emb.astype(np.float64).T).astype(np.float32)
    dropped = np.zeros((len(nodes), U + I), bool)
    for q, u in enumerate(nodes):
        dropped[q, ui[ui[:, 0] == u, 1]] = True
    assert all(np.array_equal(host(a), b) for a, b in zip((ids, scores), reference(s, dropped, U, U + I, k)))


def test_graph_replay(pgl):
    """One captured call (two launches and a workspace: slices = 3) replays to the eager bits, several times."""
    from pgl_amd import embedding_ops as E
    c = case(33, 130, 8, 5, False, True)
    g = pgl.Graph(edges=c["edges"], num_nodes=130 + EXTRA).tensor()
    index, qids, q, t = g._csr_succ_sorted(), dev(c["qids"]), dev(c["query"]), dev(c["table"])
    call = lambda query: E.topk_scores(query, t, 5, exclude=index, query_ids=qids, slices=3)
    eager = call(q)
    static = torch.zeros_like(q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(static)
    static.copy_(q)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1].view(torch.int32), eager[1].view(torch.int32))


@pytest.mark.parametrize("slices", [1, 2])
def test_special_values(pgl, slices):
    """A NaN, +-inf and a +-0.0 tie in one row, in the order tests/pool_defs.py documents; -0.0 and NaN come back as their representatives."""
    from pgl_amd import embedding_ops as E
    col = np.array([np.nan, np.inf, 5.0, 0.0, -1e-30, 0.0, -3.0], np.float32)
    table, query = np.zeros((7, 4), np.float32), np.zeros((2, 4), np.float32)
    table[:, 0], query[:, 0] = col, (1e-30, -1e-30)                  # 1e-30 * -1e-30 rounds to -0.0; query 1 mirrors the row
    ids, scores = map(host, E.topk_scores(dev(query), dev(table), 7, slices=slices))
    with np.errstate(invalid="ignore", under="ignore"):
        s32 = (query[:, :1].astype(np.float64) * col.astype(np.float64)).astype(np.float32)
    for q in range(2):
        want = pool_defs.topk_perm_by_comparison(s32[q], [0, 7], [0, 7])
        assert np.array_equal(ids[q], want)
        assert np.array_equal(scores[q], s32[q, want], equal_nan=True) and not np.signbit(scores[q][scores[q] == 0]).any()
        assert scores[q].view(np.uint32)[0] == 0x7FC00000
