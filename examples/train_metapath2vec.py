#!/usr/bin/env python3
"""metapath2vec on the engine: the flow of the reference's examples/metapath2vec (metapath random walks over a heterogeneous
graph -> skip-gram pairs -> negative sampling -> a skip-gram loss on two embedding tables), with every stage on the device:

  walks      pgl.sampling.metapath_walks  (one kernel launch for all steps of all walkers; the reference: metapath_randomwalk,
             one sample_successor call per step in a Python loop)
  pairs      pgl.ops.skip_gram_pairs      (count + scan + fill)
  negatives  pgl.ops.sample_from_table    over degree ** 0.75 (word2vec's noise distribution), one kernel launch per step
  loss       -log s(<u, v>) - sum log s(-<u, n>) on nn.Embedding

The graph is a seeded synthetic author - paper - venue graph with planted communities: every author, paper and venue belongs
to one community, a paper is published at a venue of its community and written by authors of its community, but for a small
share of edges that cross.  Relations a2p / p2a and p2v / v2p; the walks follow "a2p-p2v-v2p-p2a" from the authors.  What the
embedding learned can be read off: authors of one community end up closer (cosine) than authors of different ones.

    python examples/train_metapath2vec.py --steps 300
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402

METAPATH = "a2p-p2v-v2p-p2a"


def planted_heter_graph(authors=1200, papers=2400, venues=24, communities=4, authors_per_paper=3, p_cross=0.05, seed=0):
    """-> (edges {edge type: int64 [E, 2]}, node types, community int64 [N], number of authors).  Node ids: authors first, then
    papers, then venues.  Every paper picks one venue and authors_per_paper authors, each from its own community with probability
    1 - p_cross and from anywhere otherwise."""
    rng = np.random.default_rng(seed)
    comm = np.concatenate([rng.integers(0, communities, authors), rng.integers(0, communities, papers),
                           np.arange(venues) % communities]).astype(np.int64)
    a0, p0, v0 = 0, authors, authors + papers

    def pick(kind0, count, want, k):
        """k members per paper of the node range [kind0, kind0 + count): of the paper's community unless the edge crosses."""
        members = [np.flatnonzero(comm[kind0:kind0 + count] == c) + kind0 for c in range(communities)]
        out = np.empty((len(want), k), np.int64)
        for i, c in enumerate(want):
            for j in range(k):
                pool = members[c] if rng.random() >= p_cross and len(members[c]) else np.arange(kind0, kind0 + count)
                out[i, j] = pool[rng.integers(0, len(pool))]
        return out

    paper_ids = np.arange(p0, v0, dtype=np.int64)
    wrote = pick(a0, authors, comm[p0:v0], authors_per_paper)
    venue = pick(v0, venues, comm[p0:v0], 1)
    a2p = np.stack([wrote.reshape(-1), np.repeat(paper_ids, authors_per_paper)], 1)
    p2v = np.stack([paper_ids, venue.reshape(-1)], 1)
    edges = {"a2p": a2p, "p2a": a2p[:, ::-1].copy(), "p2v": p2v, "v2p": p2v[:, ::-1].copy()}
    return edges, np.array(["a"] * authors + ["p"] * papers + ["v"] * venues), comm, authors


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
    ap.add_argument("--authors", type=int, default=1200)
    ap.add_argument("--papers", type=int, default=2400)
    ap.add_argument("--venues", type=int, default=24)
    ap.add_argument("--communities", type=int, default=4)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--walkers", type=int, default=512, help="walks per training step (they start at authors)")
    ap.add_argument("--walk_len", type=int, default=21, help="nodes per walk (the reference's walk_length)")
    ap.add_argument("--win_size", type=int, default=4)
    ap.add_argument("--neg_num", type=int, default=5)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.025)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    edges, node_types, comm, n_auth = planted_heter_graph(args.authors, args.papers, args.venues, args.communities, seed=args.seed)
    hg = pgl.HeterGraph(edges=edges, num_nodes=len(node_types), node_types=node_types).tensor()
    n = len(node_types)
    dev = hg["a2p"].edges.device
    model = SkipGram(n, args.dim).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    noise = pgl.ops.weight_table(hg.outdegree().to(torch.float64) ** 0.75)
    losses = []
    for step in range(args.steps):
        seed = args.seed * 1000003 + step
        starts = torch.randint(0, n_auth, (args.walkers,), device=dev)
        paths, lengths = pgl.sampling.metapath_walks(hg, starts, METAPATH, args.walk_len - 1, seed=seed)
        src, dst = pgl.ops.skip_gram_pairs(paths, lengths, args.win_size, seed=seed)
        neg = pgl.ops.sample_from_table(noise, src.shape[0] * args.neg_num, seed=seed).reshape(-1, args.neg_num)
        loss = model(src, dst, neg)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if step % 50 == 0 or step == args.steps - 1:
            print("step %d loss %.4f pairs %d" % (step, losses[-1], src.shape[0]), flush=True)

    with torch.no_grad():
        z = F.normalize(model.emb.weight[:n_auth], dim=-1)
        cos = (z @ z.t()).cpu().numpy()
    ca = comm[:n_auth]
    same = ca[:, None] == ca[None, :]
    off = ~np.eye(n_auth, dtype=bool)
    k = min(10, len(losses))
    res = {"loss_first": float(np.mean(losses[:k])), "loss_last": float(np.mean(losses[-k:])),
           "intra_cos": float(cos[same & off].mean()), "inter_cos": float(cos[~same].mean())}
    print("loss %.4f -> %.4f, mean cosine of author pairs: same community %.3f, different communities %.3f"
          % (res["loss_first"], res["loss_last"], res["intra_cos"], res["inter_cos"]))
    return res


if __name__ == "__main__":
    main()
