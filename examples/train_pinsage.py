#!/usr/bin/env python3
"""Mini-batch PinSAGE: two `pgl.nn.PinSageConv` layers over the blocks of `pgl.sampling.PinSageSampler`.

The reference ships the layer (pgl/nn/conv.py: PinSageConv) and no sampler for it.  Here a node's neighbourhood is what the
PinSAGE paper defines: the top-k nodes most often visited by short random walks from it, weighted by the normalised visit
counts -- walked, counted and selected in one launch on the device (`pgl_amd.ops.walk_visit_topk`), relabelled into one small
block per layer whose `edge_feat["weight"]` is the layer's edge operand.  Features never leave HBM.

The data is a seeded planted-community graph (no network, nothing to download) at a size that trains in seconds.

    python examples/train_pinsage.py --epochs 5
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402


def planted_communities(n=8000, d=64, classes=16, avg_deg=12, seed=0):
    """Symmetric edges, 80 % of them inside a community; features = a noisy community centre."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, classes, n)
    members = [np.flatnonzero(y == c) for c in range(classes)]
    m = n * avg_deg // 2
    a = rng.integers(0, n, m)
    same = rng.random(m) < 0.8
    pick = rng.random(m)
    b = np.where(same, np.array([members[c][int(p * len(members[c]))] for c, p in zip(y[a], pick)]), rng.integers(0, n, m))
    edges = np.concatenate([np.stack([a, b], 1), np.stack([b, a], 1)]).astype(np.int64)
    centers = rng.standard_normal((classes, d)).astype(np.float32)
    x = centers[y] * 0.3 + rng.standard_normal((n, d)).astype(np.float32)
    perm = rng.permutation(n)
    return edges, x.astype(np.float32), y.astype(np.int64), perm[: n // 2], perm[n // 2: n // 2 + n // 8]


class PinSage(torch.nn.Module):
    def __init__(self, input_size, num_class, num_layers=2, hidden_size=64):
        super().__init__()
        self.convs = torch.nn.ModuleList(
            [pgl.nn.PinSageConv(input_size if i == 0 else hidden_size, hidden_size, "sum") for i in range(num_layers)])
        self.linear = torch.nn.Linear(hidden_size, num_class)

    def forward(self, blocks, feature):
        """blocks: a list of (block, n_dst), outermost first; rows 0 .. n_dst-1 of a block are its destinations."""
        for conv, (g, n_dst) in zip(self.convs, blocks):
            feature = conv(g, feature, g.edge_feat["weight"], act="relu")[:n_dst]
        return self.linear(feature)


def run_epoch(args, model, optim, sampler, feature, labels, index, rng, train):
    model.train(train)
    tot_loss = tot_acc = tot = 0
    order = rng.permutation(index) if train else index
    for i in range(0, len(order), args.batch_size):
        nodes = torch.as_tensor(order[i:i + args.batch_size], device=feature.device)
        blocks, sample_index = sampler.sample_neighbors(nodes)
        pred = model(blocks, feature[sample_index])                    # rows of the last block = the batch, in order
        y = labels[nodes]
        loss = F.cross_entropy(pred, y)
        if train:
            optim.zero_grad(); loss.backward(); optim.step()
        tot_loss += loss.item() * len(nodes); tot_acc += int((pred.argmax(1) == y).sum().item()); tot += len(nodes)
    return tot_loss / tot, tot_acc / tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch_size", type=int, default=512)
    ap.add_argument("--num_walks", type=int, default=50)
    ap.add_argument("--walk_length", type=int, default=3)
    ap.add_argument("--top_ks", type=int, nargs="+", default=[10, 5], help="neighbours per layer, input layer first")
    ap.add_argument("--hidden_size", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=8000)
    ap.add_argument("--lr", type=float, default=0.01)
    args = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    edges, x, y, train_index, val_index = planted_communities(n=args.nodes)
    graph = pgl.Graph(edges=edges, num_nodes=len(x)).tensor()
    # (the sampler walks from the batch outwards: its first layer is the model's last)
    sampler = pgl.sampling.PinSageSampler(graph, args.num_walks, args.walk_length, args.top_ks[::-1], seed=1)
    feature, labels = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)
    model = PinSage(x.shape[1], int(y.max()) + 1, len(args.top_ks), args.hidden_size).to(dev)
    optim = torch.optim.Adam(model.parameters(), lr=args.lr)
    rng = np.random.default_rng(1)
    for epoch in range(args.epochs):
        t0 = time.time()
        tl, ta = run_epoch(args, model, optim, sampler, feature, labels, train_index, rng, True)
        with torch.no_grad():
            vl, va = run_epoch(args, model, optim, sampler, feature, labels, val_index, rng, False)
        torch.cuda.synchronize()
        print("epoch %d  train loss %.4f acc %.3f | val loss %.4f acc %.3f | %.2f s" % (epoch, tl, ta, vl, va, time.time() - t0))


if __name__ == "__main__":
    main()
