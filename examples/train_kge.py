"""Knowledge-graph embedding (apps/Graph4KG) on a synthetic KG with planted structure: entities have hidden coordinates and every relation
type is a fixed translation ("transe", "distmult", "complex") or rotation ("rotate") of them, so held-out MRR is far above chance.
--fused trains through pgl_amd.nn.functional.kge_loss (one fused forward, two backward passes, no [C, cs, neg] tensor); without it
the same definition is composed from torch ops.  Both print the same loss trajectory.  Negatives: one draw of n_neg tails per chunk by
sampling.corrupt_edges, shared by the chunk's cs positives as Graph4KG's chunked sampler shares them.  The draw is checked against the
known tails of the chunk's first head only; the chunk's other positives have other heads, so for them it is Graph4KG's uniform,
unchecked corruption (a head has about 10 of the 2000 entities as tails).  Evaluation: filtered MRR / HITS@10 of the held-out triples in
both directions through kge_filter + kge_ranks (one sweep of the entity table per direction, two integers per query)."""
import argparse
import math

import numpy as np
import torch
import torch.nn.functional as F

import pgl_amd as pgl
import pgl_amd.nn.functional as PF
from pgl_amd import sampling


def planted_kg(n_ent, n_rel, n_triples, rotate, seed):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(n_ent, 2, generator=gen)
    h, r = torch.randint(0, n_ent, (n_triples,), generator=gen), torch.randint(0, n_rel, (n_triples,), generator=gen)
    if rotate:
        ang = 2 * math.pi * (r.double() + 1) / (n_rel + 1)
        target = torch.stack([z[h, 0] * ang.cos() - z[h, 1] * ang.sin(), z[h, 0] * ang.sin() + z[h, 1] * ang.cos()], 1).float()
    else:
        target = z[h] + torch.randn(n_rel, 2, generator=gen)[r]
    t = torch.cdist(target, z).argmin(1)                               # the entity nearest to the moved head
    return torch.stack([h, r, t], 1)


def torch_loss(ent, rel, h, r, t, neg, model, gamma, adv_temp):
    """The definition of pgl_amd.embedding_ops (tail-corrupt) op by op."""
    H, R, T, N = ent[h], rel[r], ent[t], ent[neg]
    C, n, d = N.shape
    if model == "transe":
        a = H + R
    elif model == "distmult":
        a = H * R
    else:
        (h_re, h_im) = H.chunk(2, -1)
        if model == "complex":
            r_re, r_im = R.chunk(2, -1)
        else:
            th = R / ((gamma + 2.0) / (d // 2) / math.pi)
            r_re, r_im = th.cos(), th.sin()
        a = torch.cat([h_re * r_re - h_im * r_im, h_re * r_im + h_im * r_re], -1)

    def phi(a, b):
        if model == "transe":
            return gamma - (a - b).square().sum(-1).clamp(min=1e-30).sqrt()
        if model == "rotate":
            (a_re, a_im), (b_re, b_im) = a.chunk(2, -1), b.chunk(2, -1)
            return gamma - ((a_re - b_re).square() + (a_im - b_im).square() + 1e-12).sqrt().sum(-1)
        return (a * b).sum(-1)
    pos, s = phi(a, T), phi(a.reshape(C, -1, 1, d), N.reshape(C, 1, n, d))
    w = torch.softmax(adv_temp * s, -1).detach() if adv_temp > 0 else 1.0 / n
    return (F.softplus(-pos).mean() + (w * F.softplus(s)).sum(-1).mean()) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="transe", choices=["transe", "distmult", "complex", "rotate"])
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--adv_temp", type=float, default=1.0)
    ap.add_argument("--sparse_step", default=None, choices=["rowwise_adagrad", "adagrad", "lazy_adam", "sgd"],
                    help="with --fused: the fused loss and a sparse optimiser step on the touched rows (kge_step) instead of dense Adam")
    ap.add_argument("--score_block", action="store_true",
                    help="also print the unfiltered tail MRR from kge_scores against one all-entity chunk (a [Q, n_ent] tensor), for comparison")
    args = ap.parse_args()
    if args.sparse_step and not args.fused:
        ap.error("--sparse_step goes with --fused")
    dev = torch.device("cuda:0")
    n_ent, n_rel, C, cs, n_neg, gamma = 2000, 4, 8, 64, 128, 6.0
    triples = planted_kg(n_ent, n_rel, 20000, args.model == "rotate", 0).to(dev)
    train, test = triples[:-1000], triples[-1000:]
    graph = pgl.Graph(edges=train[:, [0, 2]].cpu().numpy(), num_nodes=n_ent).tensor(device=dev)
    torch.manual_seed(0)
    ent = torch.nn.Parameter(torch.empty(n_ent, args.dim, device=dev).uniform_(-0.5, 0.5))
    rel = torch.nn.Parameter(torch.empty(n_rel, args.dim // 2 if args.model == "rotate" else args.dim, device=dev).uniform_(-0.5, 0.5))
    opt = torch.optim.Adam([ent, rel], lr=0.02)
    states = [PF.SparseState(w, args.sparse_step, 0.02) for w in (ent, rel)] if args.sparse_step else None
    gen = torch.Generator().manual_seed(1)
    for step in range(args.steps):
        b = train[torch.randint(0, train.shape[0], (C * cs,), generator=gen).to(dev)]
        neg = sampling.corrupt_edges(graph, b[::cs][:, [0, 2]], n_neg, side="dst", seed=step)
        h, r, t = b[:, 0].contiguous(), b[:, 1].contiguous(), b[:, 2].contiguous()
        if args.sparse_step:
            loss = PF.kge_step(ent, rel, h, r, t, neg, args.model, *states, gamma=gamma, adv_temp=args.adv_temp)
        else:
            if args.fused:
                loss = PF.kge_loss(ent, rel, h, r, t, neg, args.model, gamma=gamma, adv_temp=args.adv_temp)
            else:
                loss = torch_loss(ent, rel, h, r, t, neg, args.model, gamma, args.adv_temp)
            opt.zero_grad()
            loss.backward()
            opt.step()
        if step % 50 == 0 or step == args.steps - 1:
            print("step %4d loss %.4f" % (step, float(loss.detach())))
    chance = float(np.mean(1.0 / np.arange(1, n_ent + 1)))
    with torch.no_grad():
        # filtered ranks of the held-out triples against every entity, tails and heads (apps/Graph4KG/utils.py:205-229): the known
        # true entities of train + test are masked out; no [Q, n_ent] tensor exists
        qh, qr, qt = (test[:, i].contiguous() for i in range(3))
        counts = []
        for neg_head in (False, True):
            filt = PF.kge_filter(triples[:, 0].contiguous(), triples[:, 1].contiguous(), triples[:, 2].contiguous(), n_rel, neg_head=neg_head)
            counts.append(PF.kge_ranks(ent.detach(), rel.detach(), qh, qr, qt, args.model, gamma=gamma, neg_head=neg_head, filter=filt,
                                       filter_rows=filt.rows(qh, qr, qt))[0])
        m = PF.kge_metrics(torch.cat(counts))
        print("held-out filtered MRR %.3f HITS@10 %.3f MR %.1f, both directions (chance MRR %.4f)" % (m["MRR"], m["HITS@10"], m["MR"], chance))
        if args.score_block:                                            # the unfiltered tail MRR through a [Q, n_ent] block of scores
            everyone = torch.arange(n_ent, device=dev)[None]
            _, s = PF.kge_scores(ent.detach(), rel.detach(), qh, qr, qt, everyone, args.model, gamma=gamma)
            s = s[0]
            rank = (s > s.gather(1, test[:, 2:3])).sum(1) + 1
            print("held-out unfiltered tail MRR %.3f (score block)" % float((1.0 / rank).mean()))


if __name__ == "__main__":
    main()
