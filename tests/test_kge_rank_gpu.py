"""The fused filtered link-prediction ranks (pgl_amd/csrc/kge_score.hip, pgl_amd.embedding_ops.kge_ranks / kge_filter / kge_metrics) on
the MI355X, held to the fp64 definition (test_kge_gpu.query / phi) over every (query, candidate) pair.

Exact arithmetic: integer tables in {-2 .. 2} make every sum of the definition exact in fp32 (terms <= 36, sums < 2^24; TransE's
gamma - sqrt(n) keeps the order and the ties of the integers n), so greater and equal must EQUAL the fp64 counts, ties included.
randn tables: per pair the fp32 re-association bar of test_kge_gpu (bilinear 4 (d + 4) eps sum |a_k| |b_k|, distance 4 d eps (gamma +
|gamma - s|)); a pair is undecided when |s64 - ref64| is within the sum of both bars, and the counts are bracketed by the decided
pairs.  Undecided pairs are at most 1 % of Q (hi - lo) per case (checked on the CPU for these shapes and seeds: at most 0.4 %)."""
import functools
import types

import numpy as np
import pytest
import torch

from gpu_common import pgl  # noqa: F401  (the fixture)
from test_kge_gpu import phi, query

pytestmark = pytest.mark.gpu

NR = 3
EPS = float(np.finfo(np.float32).eps)


@functools.lru_cache(maxsize=None)
def case(model, neg_head, Q, Ne, d, lo, hi, integer):
    """-> the inputs, a filter index with every kind of row, and per query the fp64 scores' margin over ref, its bar and the two masks
    (no filter, filter) of the candidates that count."""
    gen = torch.Generator().manual_seed(7 * d + Ne)
    dr = d // 2 if model == "rotate" else d
    if integer:
        ent, rel, gamma = torch.randint(-2, 3, (Ne, d), generator=gen).float(), torch.randint(-2, 3, (NR, dr), generator=gen).float(), 12.0
    else:
        ent, rel = torch.randn(Ne, d, generator=gen), torch.randn(NR, dr, generator=gen)
        gamma = {"transe": (3.0 * d) ** 0.5, "rotate": 1.77 * d / 2}.get(model, 12.0)         # the scores straddle 0
    h, t = (torch.randint(0, Ne, (Q,), generator=gen) for _ in range(2))
    r = torch.randint(0, NR, (Q,), generator=gen)
    kept, other = (t, h) if neg_head else (h, t)
    for i in range(min(Q, Ne // 3) if integer else 0):            # bitwise copies of true rows
        ent[(int(other[i]) + 1 + i) % Ne] = ent[other[i]]
    # rows 0 .. Q - 1: random ids (duplicates, ids outside [lo, hi)) and the query's true entity; row Q: empty; row Q + 1: a whole tile
    rows = [sorted(torch.randint(0, Ne, (Ne // 8 + 2,), generator=gen).tolist() + [int(other[q]), 0, Ne - 1]) for q in range(Q)]
    rows += [[], list(range(min(lo + 32, Ne - 1), min(lo + 64, Ne)))]
    frows = torch.tensor([(q, Q, -1, Q + 1)[q % 4] for q in range(Q)])
    indptr = torch.tensor(np.cumsum([0] + [len(x) for x in rows]))
    col = torch.tensor([j for x in rows for j in x], dtype=torch.int32)
    a = query(ent[kept].double(), rel[r].double(), model, neg_head, gamma)
    s = phi(a[:, None], ent.double()[None], model, gamma)                                     # [Q, Ne]
    if model in ("distmult", "complex"):
        bar = 4.0 * (d + 4) * EPS * (a.abs() @ ent.double().abs().T)
    else:
        bar = 4.0 * d * EPS * (gamma + (gamma - s).abs())
    ref, ref_bar = s.gather(1, other[:, None]), bar.gather(1, other[:, None])
    j = torch.arange(Ne)[None]
    plain = (j >= lo) & (j < hi) & (j != other[:, None])
    listed = torch.zeros(Q, Ne, dtype=torch.bool)
    for q in range(Q):
        if 0 <= int(frows[q]) < len(rows):
            listed[q, rows[int(frows[q])]] = True
    dev = [x.cuda() for x in (ent, rel, h, r, t)]
    index = types.SimpleNamespace(indptr=indptr.cuda(), col32=col.cuda())
    return dev, gamma, index, frows.cuda(), s - ref, bar + ref_bar, (plain, plain & ~listed)


def ranks(E, c, model, neg_head, lo, hi, slices, filtered):
    dev, gamma, index, frows = c[:4]
    kw = dict(filter=index, filter_rows=frows) if filtered else {}
    g, e = E.kge_ranks(*dev, model, gamma=gamma, neg_head=neg_head, lo=lo, hi=hi, slices=slices, **kw)
    assert g.dtype == e.dtype == torch.int64
    return g.cpu(), e.cpu()


@pytest.mark.parametrize("shape", [(1, 1, 8, 0, 1), (33, 129, 8, 0, 129), (70, 300, 40, 17, 290), (32, 257, 1024, 0, 257)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("slices", [None, 1, 3])
@pytest.mark.parametrize("neg_head", [False, True])
@pytest.mark.parametrize("model", ["transe", "distmult", "complex"])
def test_exact_counts(pgl, model, neg_head, slices, shape):
    from pgl_amd import embedding_ops as E
    Q, Ne, d, lo, hi = shape
    c = case(model, neg_head, Q, Ne, d, lo, hi, True)
    margin, masks = c[4], c[6]
    assert int(((margin == 0) & masks[0]).sum()) >= min(Q, Ne // 3) // 2          # the copies do tie
    for filtered in (False, True):
        g, e = ranks(E, c, model, neg_head, lo, hi, slices, filtered)
        print("kge_ranks %s: greater %d, equal %d" % (model, int(g.sum()), int(e.sum())))
        assert torch.equal(g, ((margin > 0) & masks[filtered]).sum(1)) and torch.equal(e, ((margin == 0) & masks[filtered]).sum(1))


@pytest.mark.parametrize("shape", [(1, 9, 8), (37, 300, 40), (33, 1000, 136)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("neg_head", [False, True])
@pytest.mark.parametrize("model", ["transe", "distmult", "complex", "rotate"])
def test_randn_counts_bracketed(pgl, model, neg_head, filtered, shape):
    from pgl_amd import embedding_ops as E
    Q, Ne, d = shape
    c = case(model, neg_head, Q, Ne, d, 0, Ne, False)
    margin, bar, mask = c[4], c[5], c[6][filtered]
    g, e = ranks(E, c, model, neg_head, 0, Ne, None, filtered)
    undecided = ((margin.abs() <= bar) & mask).sum(1)
    lower = ((margin > bar) & mask).sum(1)
    print("kge_ranks %s: undecided %d of %d pairs" % (model, int(undecided.sum()), Q * Ne))
    assert int(undecided.sum()) <= 0.01 * Q * Ne
    assert bool(((lower <= g) & (g <= lower + undecided)).all()), (lower, g, undecided)
    assert bool(((lower <= g + e) & (g + e <= lower + undecided)).all()), (lower, g + e, undecided)


@pytest.mark.parametrize("what", ["fp64", "d = 12", "id >= Ne", "model", "filter alone", "hi <= lo", "slices = 33"])
def test_refusals_before_any_launch(pgl, what, monkeypatch):
    from pgl_amd import embedding_ops as E
    launches = []
    monkeypatch.setattr(E, "_launch", lambda *a, **k: launches.append(a))
    Ne, d = 24, 12 if what == "d = 12" else 16
    ent = torch.randn(Ne, d, device="cuda", dtype=torch.float64 if what == "fp64" else torch.float32)
    rel = torch.randn(NR, d, device="cuda", dtype=ent.dtype)
    h = torch.zeros(6, dtype=torch.int64, device="cuda")
    t = h + Ne if what == "id >= Ne" else h
    kw = {"filter alone": dict(filter=types.SimpleNamespace(indptr=h[:2], col32=h[:0].int())), "hi <= lo": dict(lo=5, hi=5),
          "slices = 33": dict(slices=33)}.get(what, {})
    with pytest.raises(ValueError):
        E.kge_ranks(ent, rel, h, h, t, "quate" if what == "model" else "transe", **kw)
    assert not launches


def test_filter_and_metrics(pgl):
    """kge_filter's rows are the known other ends of each (kept end, relation), ascending; filtered both-directions metrics equal the
    reference's calculate_metrics (apps/Graph4KG/utils.py:116-134) written out in numpy over the fp64 scores of an integer table."""
    from pgl_amd import embedding_ops as E
    gen = torch.Generator().manual_seed(3)
    Ne, d = 12, 8
    known = torch.stack([torch.randint(0, Ne - 1, (40,), generator=gen), torch.randint(0, NR, (40,), generator=gen),
                         torch.randint(0, Ne - 1, (40,), generator=gen)], 1)
    test = torch.cat([known[:10], torch.tensor([[Ne - 1, 0, Ne - 1]])])                        # the last pair is nobody's
    ent, rel = torch.randint(-2, 3, (Ne, d), generator=gen).float(), torch.randint(-2, 3, (NR, d), generator=gen).float()
    counts, want = [], []
    for neg_head in (False, True):
        k, o = (2, 0) if neg_head else (0, 2)
        filt = E.kge_filter(*(known[:, i].cuda().contiguous() for i in range(3)), NR, neg_head=neg_head)
        rows = filt.rows(*(test[:, i].cuda().contiguous() for i in range(3)))
        indptr, col = filt.indptr.cpu(), filt.col32.cpu()
        s = phi(query(ent[test[:, k]].double(), rel[test[:, 1]].double(), "distmult", neg_head, 12.0)[:, None], ent.double()[None], "distmult", 12.0).numpy()
        for q, (row, tr) in enumerate(zip(rows.tolist(), test.tolist())):
            listed = sorted(known[(known[:, k] == tr[k]) & (known[:, 1] == tr[1]), o].tolist())
            assert (row == -1 and not listed) or col[indptr[row]:indptr[row + 1]].tolist() == listed
            keep = np.ones(Ne)
            keep[listed] = 0.0
            want.append(((s[q] > s[q][tr[o]]) * keep).sum() + 1)
        counts.append(E.kge_ranks(ent.cuda(), rel.cuda(), *(test[:, i].cuda().contiguous() for i in range(3)), "distmult", neg_head=neg_head,
                                  filter=filt, filter_rows=rows))
    want = np.array(want)
    got = E.kge_metrics(torch.cat([g for g, _ in counts]))
    ref = {"MRR": (1.0 / want).mean(), "MR": want.mean(), "HITS@1": (want <= 1).mean(), "HITS@3": (want <= 3).mean(), "HITS@10": (want <= 10).mean()}
    assert got.keys() == ref.keys() and all(abs(got[k] - ref[k]) <= 1e-12 for k in ref), (got, ref)
    tied = E.kge_metrics(*(torch.cat(x) for x in zip(*counts)))
    assert abs(tied["MR"] - (want + torch.cat([e for _, e in counts]).cpu().numpy() / 2).mean()) <= 1e-12
