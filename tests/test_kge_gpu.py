"""The fused KG-embedding scores and loss (pgl_amd/csrc/kge_score.hip, pgl_amd.embedding_ops.kge_scores / kge_loss) on the MI355X, held
to the fp64 restatement below of the definition in the front end's module text, element by element.

Bars (none comes from the kernel): the fp32 re-association bar 4 n eps sum |terms| of the definition's own sums, per element.
  bilinear models   scores: terms |a_k| |b_k| (the definition on |inputs| with every sign +), n = d + 4.
                    loss: its own terms (all positive), n = P + neg.  d ent, d rel: the by-id sum's own terms -- the per-use gradient
                    rows, |c[i,j]| times the definition's derivative on |inputs| -- with n = uses + cs + neg (uses = how often a table
                    row is gathered; cs and neg are the lengths of the sums inside a row gradient).
  distance models   the scores pass through sqrt: the fp32 torch composition of the same definition is evaluated on the same inputs, and
                    the kernel is allowed 4 x its per-element distance from fp64 (another summation order over d and over j) plus the
                    re-association bar of the outer sums: over d for a score (terms gamma + the distance, n = d), P + neg for the loss,
                    uses + cs + neg for a gradient (terms: the per-use gradient rows).
Observed maxima are recorded in profiles/kge/README.md."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import pgl, assert_within_fp32_reassociation, check_grad_elements, reassociation_bound  # noqa: F401  (pgl: the fixture)

pytestmark = pytest.mark.gpu

MODELS = ("transe", "distmult", "complex", "rotate")
SHAPES = [(1, 1, 1, 8), (3, 5, 31, 40), (2, 33, 70, 136), (1, 32, 32, 1024)]
NE, NR, USED_E, USED_R = 24, 5, 20, 4            # the rows USED_E .. NE - 1 / USED_R .. NR - 1 are nobody's


def query(E, R, model, neg_head, gamma, absolute=False):
    if model == "transe":
        return E + R if (absolute or not neg_head) else E - R
    if model == "distmult":
        return E * R
    d = E.shape[-1]
    e_re, e_im = E.chunk(2, -1)
    if model == "rotate":
        th = R / ((gamma + 2.0) / (d // 2) / np.pi)
        r_re, r_im = (torch.ones_like(th), torch.ones_like(th)) if absolute else (torch.cos(th), torch.sin(th))
    else:
        r_re, r_im = R.chunk(2, -1)
    sg = 1.0 if absolute else (-1.0 if neg_head else 1.0)       # head-corrupt: conj(r)
    return torch.cat([e_re * r_re - (-1.0 if absolute else sg) * e_im * r_im, e_im * r_re + sg * e_re * r_im], -1)


def phi(a, b, model, gamma):
    if model == "transe":
        q = (a - b).square().sum(-1)
        assert a.dtype != torch.float64 or float(q.detach().min()) > 1e-30           # the clip is never active
        return gamma - q.clamp(min=1e-30).sqrt()
    if model == "rotate":
        (a_re, a_im), (b_re, b_im) = a.chunk(2, -1), b.chunk(2, -1)
        return gamma - ((a_re - b_re).square() + (a_im - b_im).square() + 1e-12).sqrt().sum(-1)
    return (a * b).sum(-1)


def scores(H, R, T, N, model, neg_head, gamma, absolute=False):
    """Gathered rows H, R, T [P, .] and N [C, neg, d] -> pos [P], s [C, cs, neg]."""
    kept, other = (T, H) if neg_head else (H, T)
    a = query(kept, R, model, neg_head, gamma, absolute)
    C, n, d = N.shape
    return phi(a, other, model, gamma), phi(a.reshape(C, -1, 1, d), N.reshape(C, 1, n, d), model, gamma)


def loss_of(pos, s, tau):
    w = torch.softmax(tau * s, -1).detach() if tau > 0 else 1.0 / s.shape[-1]
    return (F.softplus(-pos).mean() + (w * F.softplus(s)).sum(-1).mean()) / 2


def inputs(C, cs, n, d, model, seed):
    gen = torch.Generator().manual_seed(seed)
    ent, rel = torch.randn(NE, d, generator=gen), torch.randn(NR, d // 2 if model == "rotate" else d, generator=gen)
    h, t = (torch.randint(0, USED_E, (C * cs,), generator=gen) for _ in range(2))
    r, neg = torch.randint(0, USED_R, (C * cs,), generator=gen), torch.randint(0, USED_E, (C, n), generator=gen)
    gamma = {"transe": (3.0 * d) ** 0.5, "rotate": 1.77 * d / 2}.get(model, 12.0)         # the scores straddle 0
    return ent, rel, h, r, t, neg, gamma


def by_id(rows, ids, n):
    return torch.zeros((n,) + rows.shape[1:], dtype=rows.dtype).index_add_(0, ids, rows)


def reference(ent, rel, h, r, t, neg, model, neg_head, gamma, tau, dtype):
    """-> pos, s, loss, the per-use gradient rows (gH, gR, gT, gN) and c = d loss / d (pos, s), all in `dtype` on the host."""
    H, R, T, N = (x.to(dtype).requires_grad_(True) for x in (ent[h], rel[r], ent[t], ent[neg]))
    pos, s = scores(H, R, T, N, model, neg_head, gamma)
    loss = loss_of(pos, s, tau)
    c = torch.autograd.grad(loss, (pos, s), retain_graph=True)
    return pos.detach(), s.detach(), loss.detach(), torch.autograd.grad(loss, (H, R, T, N)), c


def tables(g, h, r, t, neg):
    gH, gR, gT, gN = g
    return by_id(torch.cat([gH, gT, gN.reshape(-1, gN.shape[-1])]), torch.cat([h, t, neg.reshape(-1)]), NE), by_id(gR, r, NR)


def run_case(pgl, model, neg_head, tau, shape):
    from pgl_amd import embedding_ops as E
    C, cs, n, d = shape
    ent, rel, h, r, t, neg, gamma = inputs(C, cs, n, d, model, seed=7 * d + n)
    dev = [x.cuda() for x in (ent, rel, h, r, t, neg)]
    pos, s = E.kge_scores(*dev, model, gamma=gamma, neg_head=neg_head)
    e, l = dev[0].clone().requires_grad_(True), dev[1].clone().requires_grad_(True)
    loss = E.kge_loss(e, l, *dev[2:], model, gamma=gamma, neg_head=neg_head, adv_temp=tau)
    loss.backward()
    return (ent, rel, h, r, t, neg, gamma), [x.detach().cpu() for x in (pos, s.reshape(C, cs, n), loss, e.grad, l.grad)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("tau", [0.0, 1.0])
@pytest.mark.parametrize("neg_head", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_parity(pgl, model, neg_head, tau, shape):
    C, cs, n, d = shape
    (ent, rel, h, r, t, neg, gamma), got = run_case(pgl, model, neg_head, tau, shape)
    p64, s64, l64, g64, c64 = reference(ent, rel, h, r, t, neg, model, neg_head, gamma, tau, torch.float64)
    want = [p64, s64, l64, *tables(g64, h, r, t, neg)]
    uses = [torch.bincount(torch.cat([h, t, neg.reshape(-1)]), minlength=NE)[:, None].double(), torch.bincount(r, minlength=NR)[:, None].double()]
    f = lambda x: x.double().numpy()
    if model in ("distmult", "complex"):
        A = [x.double().abs().requires_grad_(True) for x in (ent[h], rel[r], ent[t], ent[neg])]
        pa, sa = scores(*A, model, neg_head, gamma, absolute=True)
        assert_within_fp32_reassociation(f(got[0]), f(p64), f(pa.detach()), d + 4)
        assert_within_fp32_reassociation(f(got[1]), f(s64), f(sa.detach()), d + 4)
        ga = torch.autograd.grad((c64[0].abs() * pa).sum() + (c64[1].abs() * sa).sum(), A)
        assert_within_fp32_reassociation(f(got[2]), f(l64), f(l64), C * cs + n)
        for gi, wi, ai, ui, what in zip(got[3:], want[3:], tables(ga, h, r, t, neg), uses, ("d ent", "d rel")):
            check_grad_elements(gi, wi, ai, ui + cs + n, what=what)
    else:
        p32, s32, l32, g32, _ = reference(ent, rel, h, r, t, neg, model, neg_head, gamma, tau, torch.float32)
        have = [p32, s32, l32, *tables(g32, h, r, t, neg)]
        outer = [(gamma + (gamma - p64).abs(), d), (gamma + (gamma - s64).abs(), d), (l64, C * cs + n)]
        outer += [(a, u + cs + n) for a, u in zip(tables([x.abs() for x in g64], h, r, t, neg), uses)]
        for gi, wi, hi, (ab, nt), what in zip(got, want, have, outer, ("pos", "s", "loss", "d ent", "d rel")):
            bar = 4.0 * np.abs(f(hi) - f(wi)) + reassociation_bound(f(ab), f(torch.as_tensor(nt)))
            err = np.abs(f(gi) - f(wi))
            print("kge %s %s: max err %.3e, fp32 composition %.3e, max err / bar %.2f" % (model, what, err.max(), np.abs(f(hi) - f(wi)).max(), (err / bar).max()))
            assert (err <= bar).all(), (what, float((err / bar).max()))
    for gi, used in ((got[3], USED_E), (got[4], USED_R)):                       # nobody's rows: exactly +0.0
        assert not bool(gi[used:].view(torch.int32).any())


def test_bits_and_loss_from_scores(pgl):
    """Two calls give the same bits; the loss is the fp64 formula over kge_scores' own output, within the bar of the loss's sums plus the
    scores' own fp32 rounding carried through softplus (|d softplus| <= 1) and the weights (<= 2 tau ds)."""
    shape, tau = (2, 33, 70, 136), 1.0
    for model in MODELS:
        _, first = run_case(pgl, model, True, tau, shape)
        _, again = run_case(pgl, model, True, tau, shape)
        assert all(bool((a.view(torch.int32) == b.view(torch.int32)).all()) for a, b in zip(first, again))
        pos, s, loss = first[0].double(), first[1].double(), first[2].double()
        want = loss_of(pos, s, tau)
        ds = float(np.finfo(np.float32).eps) * float(max(pos.abs().max(), s.abs().max()))
        bar = reassociation_bound(float(want), shape[0] * shape[1] + shape[2]) + (1 + 2 * tau * 2 * float(want)) * ds
        assert abs(float(loss) - float(want)) <= bar, (model, float(loss), float(want), bar)


@pytest.mark.parametrize("what", ["fp64", "d = 12", "P % C", "id >= Ne", "model", "rotate rel width"])
def test_refusals_before_any_launch(pgl, what, monkeypatch):
    from pgl_amd import embedding_ops as E
    launches = []
    monkeypatch.setattr(E, "_launch", lambda *a, **k: launches.append(a))
    d = 12 if what == "d = 12" else 16
    model = {"model": "quate", "rotate rel width": "rotate"}.get(what, "transe")
    ent = torch.randn(NE, d, device="cuda", dtype=torch.float64 if what == "fp64" else torch.float32)
    rel = torch.randn(NR, d, device="cuda", dtype=ent.dtype)
    h = torch.zeros(7 if what == "P % C" else 6, dtype=torch.int64, device="cuda")
    neg = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    if what == "id >= Ne":
        neg[1, 2] = NE
    for fn in (E.kge_scores, E.kge_loss):
        with pytest.raises(ValueError):
            fn(ent, rel, h, h, h, neg, model)
    assert not launches and not E.kge_supported("transe", 12) and not E.kge_supported("quate", 16) and E.kge_supported("rotate", 512)
