#!/usr/bin/env python3
"""LightGCN with the BPR loss on the engine: the flow of the reference's examples/lightgcn (an embedding table propagated by
LightGCNConv layers, the layer outputs averaged, the BPR loss of model.py on sampled triples), with the sampling on the device:

  triples    pgl.sampling.bpr_triples     one kernel launch per step: per user a uniform positive and a negative item that is
                                          CHECKED against the user's row (the reference: UniformSample_original_python, a Python
                                          loop per user with `while True: negitem = randint(...)` until the item is no positive)
  propagate  pgl.nn.LightGCNConv          over the symmetric user-item graph
  loss       mean softplus(<u, n> - <u, p>) + decay * ||e0||^2 / 2 per triple

The graph is a seeded synthetic user-item graph with planted taste groups (a user mostly likes the items of its own group), and
one liked item per user is held out, so what was learned can be read off: recall@20 of the held-out items among the items a user
has not interacted with, against the 20 / num_items of a random ranking.

    python examples/train_lightgcn_bpr.py --steps 200
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402


def planted_interactions(users=600, items=400, groups=4, per_user=12, p_own=0.9, seed=0):
    """-> (train [E, 2], held_out [users]) of (user, item) pairs, items numbered 0 .. items-1: every user likes per_user + 1
    distinct items, each from its own group (user % groups == item % groups) with probability p_own; the held-out one is from
    its own group."""
    rng = np.random.default_rng(seed)
    train, held = [], np.empty(users, np.int64)
    for u in range(users):
        own = np.flatnonzero(np.arange(items) % groups == u % groups)
        other = np.flatnonzero(np.arange(items) % groups != u % groups)
        n_own = 1 + int(rng.binomial(per_user, p_own))
        liked = np.concatenate([rng.choice(own, n_own, replace=False), rng.choice(other, per_user + 1 - n_own, replace=False)])
        held[u] = liked[0]
        train += [(u, int(i)) for i in liked[1:]]
    return np.asarray(train, np.int64), held


class LightGCN(torch.nn.Module):
    def __init__(self, num_nodes, dim, layers):
        super().__init__()
        self.emb = torch.nn.Embedding(num_nodes, dim)
        torch.nn.init.normal_(self.emb.weight, std=0.1)
        self.convs = torch.nn.ModuleList([pgl.nn.LightGCNConv() for _ in range(layers)])

    def forward(self, graph):
        h = self.emb.weight
        outs = [h]
        for conv in self.convs:
            h = conv(graph, h)
            outs.append(h)
        return torch.stack(outs, 1).mean(1)

    def bpr_loss(self, graph, users, pos, neg, decay):
        z = self(graph)
        pos_score = (z[users] * z[pos]).sum(-1)
        neg_score = (z[users] * z[neg]).sum(-1)
        e0 = self.emb.weight
        reg = 0.5 * (e0[users].pow(2).sum() + e0[pos].pow(2).sum() + e0[neg].pow(2).sum()) / max(1, users.shape[0])
        return F.softplus(neg_score - pos_score).mean() + decay * reg


def recall_at_k(model, graph, train, held, num_users, num_items, k=20):
    with torch.no_grad():
        z = model(graph)
        score = z[:num_users] @ z[num_users:].t()
        score[torch.as_tensor(train[:, 0], device=score.device), torch.as_tensor(train[:, 1], device=score.device)] = -float("inf")
        top = score.topk(k, dim=1).indices.cpu().numpy()
    return float((top == held[:, None]).any(1).mean())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--users", type=int, default=600)
    ap.add_argument("--items", type=int, default=400)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch_size", type=int, default=2048, help="users drawn per step (with repeats)")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--decay", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    torch.manual_seed(args.seed)
    U, I = args.users, args.items
    train, held = planted_interactions(U, I, args.groups, seed=args.seed)
    ui = train + np.array([0, U])                            # items are nodes U .. U + I - 1
    g = pgl.Graph(edges=np.concatenate([ui, ui[:, ::-1]]), num_nodes=U + I).tensor()
    dev = g.edges.device
    model = LightGCN(U + I, args.dim, args.layers).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    recall_first = recall_at_k(model, g, train, held, U, I)
    losses = []
    for step in range(args.steps):
        batch = torch.randint(0, U, (args.batch_size,), device=dev)
        users, pos, neg = pgl.sampling.bpr_triples(g, batch, (U, U + I), seed=args.seed * 1000003 + step)
        loss = model.bpr_loss(g, users, pos, neg, args.decay)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if step % 50 == 0 or step == args.steps - 1:
            print("step %d loss %.4f triples %d" % (step, losses[-1], users.shape[0]), flush=True)
    m = max(1, min(10, args.steps // 2))
    res = {"loss_first": float(np.mean(losses[:m])), "loss_last": float(np.mean(losses[-m:])), "losses": losses,
           "recall_first": recall_first, "recall_last": recall_at_k(model, g, train, held, U, I), "recall_random": 20.0 / I}
    print("loss %.4f -> %.4f, recall@20 of the held-out items %.3f -> %.3f (a random ranking: %.3f)"
          % (res["loss_first"], res["loss_last"], res["recall_first"], res["recall_last"], res["recall_random"]))
    return res


if __name__ == "__main__":
    main()
