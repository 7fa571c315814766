#!/usr/bin/env python3
"""Graph classification with hierarchical self-attention pooling: three blocks of `pgl.nn.GCNConv` + `pgl.nn.SAGPool`, a
mean || max `pgl.nn.GraphPool` read-out after every block, the read-outs summed into an MLP -- the flow of the reference's
examples/sag_pool written against this API.

Every pooling layer keeps each member graph's top ceil(ratio * n) nodes by a learned score and the edges between them.  On a
batched tensor graph that index work runs on the device (csrc/pool.hip: one top-k launch pair, one edge filter with a single
host read); the pooled graph's bookkeeping comes from the batch's host-side node index.

The data is synthetic and seeded (nothing to download): a graph's class is the number of dense communities planted in it
(1, 2 or 3 over the same number of nodes), node features are a constant and the scaled degree.  Small enough to train in
seconds.  With the defaults the held-out accuracy reaches about 0.9 (chance: 0.33); the script exits non-zero below
--min_acc (0.8).

    python examples/train_sagpool.py --epochs 30
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


def planted_graph(rng, label, n_lo=24, n_hi=40, p_in=0.45, p_out=0.03):
    """label + 1 communities of (nearly) equal size; an edge with probability p_in inside a community, p_out across.  Symmetric."""
    n = int(rng.integers(n_lo, n_hi + 1))
    comm = rng.permutation(n) % (label + 1)
    p = np.where(comm[:, None] == comm[None, :], p_in, p_out)
    upper = np.triu(rng.random((n, n)) < p, 1)
    a, b = np.nonzero(upper)
    edges = np.concatenate([np.stack([a, b], 1), np.stack([b, a], 1)]).astype(np.int64).reshape(-1, 2)
    deg = np.bincount(edges[:, 0], minlength=n).astype(np.float32)
    feat = np.stack([np.ones(n, np.float32), deg / 10.0], 1)
    return pgl.Graph(edges=edges, num_nodes=n, node_feat={"x": feat})


def make_dataset(num_graphs, classes, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes, num_graphs)
    return [planted_graph(rng, int(c)) for c in labels], labels.astype(np.int64)


class SAGPoolNet(torch.nn.Module):
    def __init__(self, input_size, hidden_size, num_class, ratio, num_blocks=3):
        super().__init__()
        self.convs = torch.nn.ModuleList(
            [pgl.nn.GCNConv(input_size if i == 0 else hidden_size, hidden_size) for i in range(num_blocks)])
        self.pools = torch.nn.ModuleList([pgl.nn.SAGPool(hidden_size, ratio) for _ in range(num_blocks)])
        self.mean, self.max = pgl.nn.GraphPool("mean"), pgl.nn.GraphPool("max")
        self.mlp = torch.nn.Sequential(torch.nn.Linear(2 * hidden_size, hidden_size), torch.nn.ReLU(),
                                       torch.nn.Linear(hidden_size, num_class))

    def forward(self, graph, x):
        out = 0
        for conv, pool in zip(self.convs, self.pools):
            x = F.relu(conv(graph, x))
            x, _, graph = pool(graph, x)
            out = out + torch.cat([self.mean(graph, x), self.max(graph, x)], dim=1)
        return self.mlp(out)


def batches(graphs, labels, batch_size, dev, order):
    for i in range(0, len(order), batch_size):
        idx = order[i:i + batch_size]
        g = pgl.Graph.disjoint([graphs[j] for j in idx]).tensor(device=dev)
        yield g, g.node_feat["x"], torch.as_tensor(labels[idx], device=dev)


def run_epoch(model, optim, graphs, labels, batch_size, dev, order, train):
    model.train(train)
    tot_loss = tot_acc = 0
    for g, x, y in batches(graphs, labels, batch_size, dev, order):
        pred = model(g, x)
        loss = F.cross_entropy(pred, y)
        if train:
            optim.zero_grad(); loss.backward(); optim.step()
        tot_loss += loss.item() * len(y); tot_acc += int((pred.argmax(1) == y).sum().item())
    return tot_loss / len(order), tot_acc / len(order)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--graphs", type=int, default=600)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--hidden_size", type=int, default=32)
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--min_acc", type=float, default=0.8, help="held-out accuracy the run must reach (chance: 1/3)")
    args = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    classes = 3
    graphs, labels = make_dataset(args.graphs, classes, seed=0)
    split = args.graphs * 4 // 5
    train_idx, val_idx = np.arange(split), np.arange(split, args.graphs)
    model = SAGPoolNet(2, args.hidden_size, classes, args.ratio).to(dev)
    optim = torch.optim.Adam(model.parameters(), lr=args.lr)
    rng = np.random.default_rng(1)
    va = 0.0
    for epoch in range(args.epochs):
        t0 = time.time()
        tl, ta = run_epoch(model, optim, graphs, labels, args.batch_size, dev, rng.permutation(train_idx), True)
        with torch.no_grad():
            vl, va = run_epoch(model, optim, graphs, labels, args.batch_size, dev, val_idx, False)
        torch.cuda.synchronize()
        print("epoch %d  train loss %.4f acc %.3f | val loss %.4f acc %.3f | %.2f s" % (epoch, tl, ta, vl, va, time.time() - t0))
    print("final held-out accuracy %.3f (required: %.2f)" % (va, args.min_acc))
    return 0 if va >= args.min_acc else 1


if __name__ == "__main__":
    sys.exit(main())
