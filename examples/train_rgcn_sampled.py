#!/usr/bin/env python3
"""Mini-batch RGCN: two `pgl.nn.RGCNConv` layers over the blocks of `pgl.sampling.RelationNeighborSampler`.

The reference builds such batches by hand (examples/NeurIPS2022-OGB-Challenge/MAG240M/dataset/new_dataset_p2p.py:163-193: one
`sample_neighbors` call per edge type per layer, `reindex_heter_graph`, an `edge_split` array).  Here every layer samples all edge
types in one count launch, one scan and one fill launch (`pgl_amd.ops.sample_neighbors_relations`), relabels all sampled sources at
once and hands back one block `HeterGraph` per layer whose relations share the node set, so `conv(block, h)[:n_dst]` is the next
layer's input.  Features never leave HBM.

The data is a seeded three-relation graph with planted classes (no network, nothing to download) at a size that trains in seconds.

    python examples/train_rgcn_sampled.py --epochs 5
    python examples/train_rgcn_sampled.py --epochs 5 --fused     # every layer: one aggregation launch over all edge types
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

EDGE_TYPES = ["cites", "coauthor", "venue"]


def planted_relations(n=6000, d=32, classes=8, seed=0):
    """Three edge types over one node set: `cites` 85 % and `coauthor` 70 % inside a class, `venue` uniform noise; features = a
    noisy class centre.  -> ({edge type: int64 [E, 2]}, x, y, train index, validation index)"""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, classes, n)
    members = [np.flatnonzero(y == c) for c in range(classes)]

    def relation(avg_deg, inside):
        m = n * avg_deg
        dst = rng.integers(0, n, m)
        pick = rng.random(m)
        same = np.array([members[c][int(p * len(members[c]))] for c, p in zip(y[dst], pick)])
        src = np.where(rng.random(m) < inside, same, rng.integers(0, n, m))
        return np.stack([src, dst], 1).astype(np.int64)

    edges = {"cites": relation(8, 0.85), "coauthor": relation(4, 0.7), "venue": relation(6, 0.0)}
    centers = rng.standard_normal((classes, d)).astype(np.float32)
    x = centers[y] * 0.4 + rng.standard_normal((n, d)).astype(np.float32)
    perm = rng.permutation(n)
    return edges, x.astype(np.float32), y.astype(np.int64), perm[: n // 2], perm[n // 2: n // 2 + n // 8]


class RGCN(torch.nn.Module):
    def __init__(self, input_size, num_class, num_layers=2, hidden_size=64, fused=False):
        super().__init__()
        self.fused = fused
        self.convs = torch.nn.ModuleList(
            [pgl.nn.RGCNConv(input_size if i == 0 else hidden_size, hidden_size, EDGE_TYPES, fused=fused) for i in range(num_layers)])
        self.linear = torch.nn.Linear(hidden_size, num_class)

    def forward(self, blocks, h):
        """blocks: a list of (block HeterGraph, n_dst), outermost first; rows 0 .. n_dst-1 of a block are its destinations."""
        for conv, (block, n_dst) in zip(self.convs, blocks):
            h = F.relu(conv(block, h, out_size=n_dst) if self.fused else conv(block, h)[:n_dst])
        return self.linear(h)


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch_size", type=int, default=512)
    ap.add_argument("--samples", type=int, nargs="+", default=[10, 5], help="fan-out per edge type and layer, input layer first")
    ap.add_argument("--hidden_size", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=6000)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0, help="seed of the model's initial weights")
    ap.add_argument("--fused", action="store_true", help="RGCNConv(fused=True): one aggregation launch per layer, only the n_dst output rows")
    args = ap.parse_args(argv)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda:0")
    edges, x, y, train_index, val_index = planted_relations(n=args.nodes)
    hg = pgl.HeterGraph(edges=edges, num_nodes=len(x)).tensor(device=dev)
    # (the sampler walks from the batch outwards: its first layer is the model's last)
    sampler = pgl.sampling.RelationNeighborSampler(hg, args.samples[::-1], seed=1)
    feature, labels = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)
    model = RGCN(x.shape[1], int(y.max()) + 1, len(args.samples), args.hidden_size, args.fused).to(dev)
    optim = torch.optim.Adam(model.parameters(), lr=args.lr)
    rng = np.random.default_rng(1)
    history = []
    for epoch in range(args.epochs):
        t0 = time.time()
        tl, ta = run_epoch(args, model, optim, sampler, feature, labels, train_index, rng, True)
        with torch.no_grad():
            vl, va = run_epoch(args, model, optim, sampler, feature, labels, val_index, rng, False)
        torch.cuda.synchronize()
        history.append(dict(train_loss=tl, train_acc=ta, val_loss=vl, val_acc=va))
        print("epoch %d  train loss %.4f acc %.3f | val loss %.4f acc %.3f | %.2f s" % (epoch, tl, ta, vl, va, time.time() - t0))
    return history


if __name__ == "__main__":
    main()
