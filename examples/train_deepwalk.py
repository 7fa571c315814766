#!/usr/bin/env python3
"""DeepWalk on the engine: the flow of the reference's examples/deepwalk (random walks -> skip-gram pairs -> negative
sampling -> a skip-gram loss on two embedding tables), with every stage on the device:

  walks      pgl.sampling.walks           (one kernel launch for all steps of all walkers; the reference: random_walk)
  pairs      pgl.ops.skip_gram_pairs      (count + scan + fill; the reference: graph_kernel.skip_gram_gen_pair per walk)
  negatives  torch.randint                (uniform over the nodes), or with --neg_power a: pgl.ops.sample_from_table over
             outdegree ** a (word2vec's unigram^0.75 noise distribution), one kernel launch per step
  loss       -log s(<u, v>) - sum log s(-<u, n>) on nn.Embedding

The graph is a seeded planted partition (two communities, dense inside, sparse across), so what the embedding learned can be
read off: nodes of one community end up closer (cosine) than nodes of different ones.

    python examples/train_deepwalk.py --steps 300
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402


def planted_graph(n=400, p_in=0.05, p_out=0.002, seed=0):
    """Two communities of n // 2 nodes; each unordered pair is an edge with probability p_in inside a community and p_out
    across; both directions are stored (a walk follows successors)."""
    rng = np.random.default_rng(seed)
    comm = np.arange(n) >= n // 2
    iu, ju = np.triu_indices(n, 1)
    prob = np.where(comm[iu] == comm[ju], p_in, p_out)
    keep = rng.random(iu.shape[0]) < prob
    e = np.stack([iu[keep], ju[keep]], 1)
    edges = np.concatenate([e, e[:, ::-1]]).astype(np.int64)
    return edges, comm


class SkipGram(torch.nn.Module):
    def __init__(self, num_nodes, dim):
        super().__init__()
        self.emb = torch.nn.Embedding(num_nodes, dim)
        self.ctx = torch.nn.Embedding(num_nodes, dim)
        torch.nn.init.uniform_(self.emb.weight, -0.5 / dim, 0.5 / dim)
        torch.nn.init.zeros_(self.ctx.weight)

    def forward(self, src, dst, neg):
        u = self.emb(src)                                    # [P, d]
        pos = (u * self.ctx(dst)).sum(-1)                     # [P]
        negs = torch.bmm(self.ctx(neg), u.unsqueeze(-1)).squeeze(-1)   # [P, K]
        return -(F.logsigmoid(pos) + F.logsigmoid(-negs).sum(-1)).mean()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nodes", type=int, default=400)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--walkers", type=int, default=256, help="walks per training step")
    ap.add_argument("--walk_len", type=int, default=20, help="nodes per walk (the reference's max_depth)")
    ap.add_argument("--win_size", type=int, default=5)
    ap.add_argument("--neg_num", type=int, default=5)
    ap.add_argument("--neg_power", type=float, default=0.0,
                    help="0: uniform negatives (torch.randint); a > 0: negatives drawn proportionally to outdegree ** a")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.025)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    edges, comm = planted_graph(args.nodes, seed=args.seed)
    g = pgl.Graph(edges=edges, num_nodes=args.nodes).tensor()
    dev = g.edges.device
    model = SkipGram(args.nodes, args.dim).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    noise = None
    if args.neg_power > 0:
        noise = pgl.ops.weight_table(g.outdegree().to(torch.float64) ** args.neg_power)
    losses = []
    for step in range(args.steps):
        starts = torch.randint(0, args.nodes, (args.walkers,), device=dev)
        paths, lengths = pgl.sampling.walks(g, starts, args.walk_len - 1, seed=args.seed * 1000003 + step)
        src, dst = pgl.ops.skip_gram_pairs(paths, lengths, args.win_size, seed=args.seed * 1000003 + step)
        if noise is None:
            neg = torch.randint(0, args.nodes, (src.shape[0], args.neg_num), device=dev)
        else:
            neg = pgl.ops.sample_from_table(noise, src.shape[0] * args.neg_num, seed=args.seed * 1000003 + step).reshape(-1, args.neg_num)
        loss = model(src, dst, neg)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if step % 50 == 0 or step == args.steps - 1:
            print("step %d loss %.4f pairs %d" % (step, losses[-1], src.shape[0]), flush=True)

    with torch.no_grad():
        z = F.normalize(model.emb.weight, dim=-1)
        cos = (z @ z.t()).cpu().numpy()
    same = comm[:, None] == comm[None, :]
    off = ~np.eye(args.nodes, dtype=bool)
    res = {"loss_first": float(np.mean(losses[:10])), "loss_last": float(np.mean(losses[-10:])),
           "intra_cos": float(cos[same & off].mean()), "inter_cos": float(cos[~same].mean())}
    print("loss %.4f -> %.4f, mean cosine intra-community %.3f, inter-community %.3f"
          % (res["loss_first"], res["loss_last"], res["intra_cos"], res["inter_cos"]))
    return res


if __name__ == "__main__":
    main()
