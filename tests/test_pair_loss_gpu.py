"""The fused skip-gram / BPR loss (pgl_amd/csrc/pair_loss.hip, pgl_amd.embedding_ops.pair_loss) and its public wrappers on the MI355X,
held to the definition below: loss, d emb and d ctx within 8 * max(max|def32 - def64|, eps32 * max|def64|) of the fp64 definition, both
terms taken from the host definition and never from the kernel (the 8 covers a summation order that differs from torch's: chunks of
sorted pairs and a fix-up in chunk order against a serial sum).  With O(1) logits a dropped row, pair or negative moves an element by
orders more than the bar.
Largest ratio |got - def64| / (the bar / 8) measured on the MI355X: loss 0.55, d emb 0.54, d ctx 1.44 (BPR, d = 100, K = 5, ids out of
range; profiles/pair_loss/README.md)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import pgl  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
NU, NV = 120, 90


def definition(emb, ctx, src, tgt, mode, w_pos, w_neg):
    """The loss of pgl_amd.embedding_ops.pair_loss in plain torch; an entry with an id outside its table is masked out."""
    ok_t = (tgt >= 0) & (tgt < ctx.shape[0])
    ok = ok_t & ((src >= 0) & (src < emb.shape[0]) & ok_t[:, 0])[:, None]
    z = (emb[src.clamp(0, emb.shape[0] - 1)][:, None, :] * ctx[tgt.clamp(0, ctx.shape[0] - 1)]).sum(-1)
    if mode == "skipgram":
        terms = torch.cat([w_pos * F.softplus(-z[:, :1]), w_neg * F.softplus(z[:, 1:])], 1)
    else:
        terms = torch.cat([torch.zeros_like(z[:, :1]), w_neg * F.softplus(z[:, 1:] - z[:, :1])], 1)
    return (terms * ok).sum()


def evaluate(fn, tables, dtype=None):
    """fn(*tables) and its gradients by autograd: on the host in `dtype`, or (dtype None) on the tables as they are -> [loss, grads...]."""
    xs = [t.detach().requires_grad_(True) if dtype is None else t.detach().cpu().to(dtype).requires_grad_(True) for t in tables]
    loss = fn(*xs)
    loss.backward()
    return [loss.detach()] + [t.grad for t in xs]


def held(what, got, fn, tables):
    """Asserts every entry of got = [loss, grads...] within the bar of fn's fp64 value; prints the ratios |got - def64| / unit."""
    d64, d32 = evaluate(fn, tables, torch.float64), evaluate(fn, tables, torch.float32)
    ratios = []
    for g, w64, w32 in zip(got, d64, d32):
        unit = max(float((w32.double() - w64).abs().max()), EPS32 * float(w64.abs().max()))
        err = float((g.cpu().double() - w64).abs().max())
        ratios.append(err / unit if unit > 0.0 else (0.0 if err == 0.0 else float("inf")))
    print("pair_loss %s: |got - def64| / unit = %s" % (what, ", ".join("%.2f" % r for r in ratios)))
    assert all(r <= 8.0 for r in ratios), ratios


def inputs(d, K, seed=0, out_of_range=False):
    """-> emb [NU, d], ctx [NV, d] (randn / d^(1/4): O(1) logits), src [P], tgt [P, 1 + K], shuffled.  One call holds rows without a pair
    (0 .. 9), runs of one and two pairs, a row of chunk + 5 pairs (it straddles chunks), a row of (kFixShort + 2) chunks of pairs (the
    fix-up's long role) and a pair whose targets are all one row."""
    from pgl_amd.embedding_ops import PAIR_CHUNK
    gen = torch.Generator().manual_seed(1000 * d + 10 * K + seed)
    emb, ctx = (torch.randn(n, d, generator=gen) / d ** 0.25 for n in (NU, NV))
    src = torch.cat([torch.tensor([10, 11, 11]), torch.full((PAIR_CHUNK + 5,), 12), torch.full((18 * PAIR_CHUNK,), 13),
                     torch.randint(14, NU, (200,), generator=gen)])
    tgt = torch.randint(0, NV, (src.shape[0], 1 + K), generator=gen)
    tgt[0] = tgt[0, 0]
    if out_of_range:
        hit = lambda n: torch.rand(n, generator=gen) < 0.1
        tgt[:, 1:][hit(tgt[:, 1:].numel()).reshape(-1, K)] = -1
        tgt[:, 1:][hit(tgt[:, 1:].numel()).reshape(-1, K)] = NV
        tgt[hit(tgt.shape[0]), 0] = NV + 7
        src[hit(src.shape[0])] = -1
        src[hit(src.shape[0])] = NU
    perm = torch.randperm(src.shape[0], generator=gen)
    return emb.cuda(), ctx.cuda(), src[perm].cuda(), tgt[perm].cuda()


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


CASES = [(m, d, K, oor) for oor in (False, True) for m in ("skipgram", "bpr") for d in (4, 64, 100, 256) for K in (0, 1, 5)
         if K > 0 or (m == "skipgram" and not oor)]


@pytest.mark.parametrize("mode,d,K,out_of_range", CASES)
def test_definition(pgl, mode, d, K, out_of_range):
    """In range, and with -1 / N sprinkled into negatives, positives and sources: the definition of the filtered input."""
    from pgl_amd import embedding_ops as E
    emb, ctx, src, tgt = inputs(d, K, out_of_range=out_of_range)
    w_pos, w_neg = 1.0 / src.shape[0], 0.7 / src.shape[0]
    before = dict(E.LAUNCHES)
    got = evaluate(lambda e, c: E.pair_loss(e, c, src, tgt, mode, w_pos, w_neg), (emb, ctx))
    assert E.LAUNCHES["pair_loss"] == before.get("pair_loss", 0) + 1
    held("%s d=%d K=%d oor=%s" % (mode, d, K, out_of_range), got,
         lambda e, c: definition(e, c, src.cpu(), tgt.cpu(), mode, w_pos, w_neg), (emb, ctx))


def test_bits(pgl):
    """The same call twice; the loss without gradients; one launch family a call and no [P, d]-sized allocation."""
    from pgl_amd import embedding_ops as E
    emb, ctx, src, tgt = inputs(64, 5, out_of_range=True)
    run = lambda: evaluate(lambda e, c: E.pair_loss(e, c, src, tgt, "skipgram"), (emb, ctx))
    first, again = run(), run()
    assert all(same_bits(a, b) for a, b in zip(first, again))
    with torch.no_grad():
        assert same_bits(E.pair_loss(emb, ctx, src, tgt, "skipgram"), first[0])
    assert same_bits(E.pair_loss(emb, ctx, src, tgt, "skipgram"), first[0])
    P, d, K = 1 << 14, 256, 1
    gen = torch.Generator().manual_seed(5)
    emb, ctx = torch.randn(NU, d, generator=gen).cuda() / 4, torch.randn(NV, d, generator=gen).cuda() / 4
    src, tgt = torch.randint(0, NU, (P,), generator=gen).cuda(), torch.randint(0, NV, (P, 1 + K), generator=gen).cuda()
    E.pair_loss(emb, ctx, src[:64], tgt[:64], "bpr")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base, before = torch.cuda.memory_allocated(), dict(E.LAUNCHES)
    evaluate(lambda e, c: E.pair_loss(e, c, src, tgt, "bpr"), (emb, ctx))
    torch.cuda.synchronize()
    assert (E.LAUNCHES["pair_loss"], E.LAUNCHES["pair_loss_backward_ctx"]) == (before["pair_loss"] + 1, before.get("pair_loss_backward_ctx", 0) + 1)
    # g is [P, 1 + K] floats; the ids, their two sorted indices and the split-row scratch are a few times that, a [P, d] tensor is 128 times
    bound = 24 * P * (1 + K) * 4 + 4 * (NU + NV) * d * 4
    assert bound < P * d * 4
    assert torch.cuda.max_memory_allocated() - base <= bound, (torch.cuda.max_memory_allocated() - base, bound)


@pytest.mark.parametrize("what", ["cpu", "fp64", "d = 6", "d = 260", "tgt 1-D", "tgt rows", "bpr K = 0"])
def test_refusals(pgl, what):
    from pgl_amd import embedding_ops as E
    d = {"d = 6": 6, "d = 260": 260}.get(what, 8)
    dev, dtype = "cpu" if what == "cpu" else "cuda", torch.float64 if what == "fp64" else torch.float32
    emb, ctx = torch.randn(40, d, device=dev, dtype=dtype), torch.randn(40, d, device=dev, dtype=dtype)
    src = torch.zeros(5, dtype=torch.int64, device=dev)
    tgt = torch.zeros({"tgt 1-D": (5,), "tgt rows": (4, 2), "bpr K = 0": (5, 1)}.get(what, (5, 2)), dtype=torch.int64, device=dev)
    before = dict(E.LAUNCHES)
    with pytest.raises(TypeError if what == "fp64" else ValueError):
        E.pair_loss(emb, ctx, src, tgt, "bpr")
    assert dict(E.LAUNCHES) == before


def test_no_pairs(pgl):
    from pgl_amd import embedding_ops as E
    emb, ctx = torch.randn(40, 8, device="cuda"), torch.randn(50, 8, device="cuda")
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    loss, de, dc = evaluate(lambda e, c: E.pair_loss(e, c, none, none.reshape(0, 3), "bpr"), (emb, ctx))
    assert float(loss) == 0.0 and de.shape == emb.shape and dc.shape == ctx.shape and not bool(de.any()) and not bool(dc.any())


@pytest.mark.parametrize("what", ["pair_mean", "reference", "bpr", "shared"])
def test_public_wrappers(pgl, what):
    """skip_gram_loss / bpr_loss against their op-by-op selves; "shared": one tensor as both tables."""
    import pgl_amd.nn.functional as PF
    emb, ctx, src, tgt = inputs(32, 3, seed=1)
    if what == "shared":
        emb, src = emb[:NV], src % NV
    dst, neg = tgt[:, 0], tgt[:, 1:]
    scores = lambda e, c, s, t: (e[s][:, None, :] * c[t]).sum(-1)
    if what == "pair_mean":         # the expression of examples/train_deepwalk.py: SkipGram.forward
        ref = lambda e, c: -(F.logsigmoid((e[src.cpu()] * c[dst.cpu()]).sum(-1)) +
                             F.logsigmoid(-torch.bmm(c[neg.cpu()], e[src.cpu()].unsqueeze(-1)).squeeze(-1)).sum(-1)).mean()
        fused = lambda e, c: PF.skip_gram_loss(e, c, src, dst, neg)
    elif what == "reference":
        def ref(e, c):
            z = scores(e, c, src.cpu(), tgt.cpu())
            bce = F.binary_cross_entropy_with_logits
            return (bce(z[:, :1], torch.ones_like(z[:, :1])) + bce(z[:, 1:], torch.zeros_like(z[:, 1:]))) / 2
        fused = lambda e, c: PF.skip_gram_loss(e, c, src, dst, neg, reduction="reference")
    else:
        ref = lambda e, c: F.softplus(scores(e, c, src.cpu(), neg[:, :1].cpu()) - scores(e, c, src.cpu(), dst[:, None].cpu())).mean()
        fused = lambda e, c: PF.bpr_loss(e, c, src, dst, neg[:, 0])
    if what == "shared":
        held(what, evaluate(lambda t: fused(*[t * 1.0] * 2), (emb,)), lambda t: ref(t, t), (emb,))      # (t * 1.0: a non-leaf tensor, passed twice)
    else:
        held(what, evaluate(fused, (emb, ctx)), ref, (emb, ctx))
