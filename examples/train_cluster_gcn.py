#!/usr/bin/env python3
"""Cluster-GCN (Chiang et al., KDD 2019) written against the pgl_amd API: the graph is cut into clusters once, every training
step runs a GCN on the subgraph INDUCED by a few clusters drawn at random, and the loss is taken at that batch's training nodes.

  cut     the engine's partitioner (the clustering Graph.reorder computes) or pgl.partition.random_partition (--partition random:
          the baseline the paper compares with -- most edges then leave the batch);
  batch   pgl.sampling.ClusterBatches -> (subgraph, node_ids): extracted and relabelled on the device (pglamd_induced_subgraph_*),
          its dst index comes out grouped and needs no sort; features and labels are gathered by node_ids and never leave HBM;
  eval    full-graph inference with the same weights.

There is no network: the data is a seeded planted-community graph (features = noisy class centres), at a size that trains in
seconds.

    python examples/train_cluster_gcn.py --epochs 5 --clusters 64 --clusters_per_batch 4
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


def planted_communities(n=40000, d=64, classes=16, avg_deg=20, p_in=0.8, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, classes, n)
    members = [np.flatnonzero(y == c) for c in range(classes)]
    m = n * avg_deg // 2
    a = rng.integers(0, n, m)
    inside = np.array([members[c][int(p * len(members[c]))] for c, p in zip(y[a], rng.random(m))])
    b = np.where(rng.random(m) < p_in, inside, rng.integers(0, n, m))
    edges = np.concatenate([np.stack([a, b], 1), np.stack([b, a], 1), np.stack([np.arange(n)] * 2, 1)]).astype(np.int64)      # symmetric + self-loops
    x = rng.standard_normal((classes, d)).astype(np.float32)[y] * 0.4 + rng.standard_normal((n, d)).astype(np.float32)
    perm = rng.permutation(n)
    train = np.zeros(n, bool)
    train[perm[: n // 2]] = True
    return edges, x, y.astype(np.int64), train, perm[n // 2: n // 2 + n // 8]


class GCN(torch.nn.Module):
    def __init__(self, input_size, num_class, num_layers=2, hidden_size=128, drop=0.5):
        super().__init__()
        sizes = [input_size] + [hidden_size] * (num_layers - 1) + [num_class]
        self.convs = torch.nn.ModuleList(
            [pgl.nn.GCNConv(a, b, activation="relu" if i < num_layers - 1 else None) for i, (a, b) in enumerate(zip(sizes, sizes[1:]))])
        self.dropout = torch.nn.Dropout(drop)

    def forward(self, graph, feature):
        for i, conv in enumerate(self.convs):
            feature = conv(graph, self.dropout(feature) if i else feature)
        return feature


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=40000)
    ap.add_argument("--clusters", type=int, default=64)
    ap.add_argument("--clusters_per_batch", type=int, default=4)
    ap.add_argument("--partition", default="engine", choices=["engine", "random"])
    ap.add_argument("--hidden_size", type=int, default=128)
    ap.add_argument("--lr", type=float, default=0.01)
    args = ap.parse_args()
    torch.manual_seed(0)
    np.random.seed(0)
    dev = torch.device("cuda:0")
    edges, x, y, train_mask, val_index = planted_communities(n=args.nodes)
    graph = pgl.Graph(edges=edges, num_nodes=len(x)).tensor(device=dev)
    t0 = time.time()
    if args.partition == "engine":
        part, _ = pgl.ops.host_partition_edges(edges, len(x), args.clusters, None, None, 1.10, 1.10, 0)
    else:
        part = pgl.partition.random_partition(graph, args.clusters)
    loader = pgl.sampling.ClusterBatches(graph, part, clusters_per_batch=args.clusters_per_batch, shuffle=True, seed=1)
    print("%d clusters (%s) in %.2f s, %d batches per epoch" % (args.clusters, args.partition, time.time() - t0, len(loader)))
    feature, labels = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)
    is_train, val_index = torch.as_tensor(train_mask).to(dev), torch.as_tensor(val_index).to(dev)
    model = GCN(x.shape[1], int(y.max()) + 1, 2, args.hidden_size).to(dev)
    optim = torch.optim.Adam(model.parameters(), lr=args.lr)
    for epoch in range(args.epochs):
        model.train()
        t0, tot_loss, tot, kept = time.time(), 0.0, 0, 0
        for sub, node_ids in loader:
            pick = is_train[node_ids]
            pred = model(sub, feature[node_ids])[pick]
            loss = F.cross_entropy(pred, labels[node_ids][pick])
            optim.zero_grad(); loss.backward(); optim.step()
            tot_loss += loss.item() * int(pick.sum()); tot += int(pick.sum()); kept += sub.num_edges
        model.eval()
        with torch.no_grad():
            va = float((model(graph, feature)[val_index].argmax(1) == labels[val_index]).float().mean())
        torch.cuda.synchronize()
        print("epoch %d  train loss %.4f | val acc %.3f | %.0f %% of the edges inside the batches | %.2f s" % (
            epoch, tot_loss / max(tot, 1), va, 100.0 * kept / graph.num_edges, time.time() - t0))


if __name__ == "__main__":
    main()
