#!/usr/bin/env python3
"""Graph pooling on one MI355X: the pooling kernels (csrc/pool.hip, front end pgl_amd/pool_ops.py) next to the tensor code of the
same build (pool_ops._ROUTE = False: the dense argsort of math.segment_topk, the table gather of filter_adj, SAGPool on both), on
the same batched graphs, in the same process.

Shapes (graphs x nodes per graph, --degree random edges per node):  (a) 128 x 30,  (b) 4096 x 64,  (c) 64 x 4000.
Cases per shape:
    topk_perm       pool_ops.topk_perm from host-known pointer arrays          | math.segment_topk's tensor code (ratio 0.5)
    filter_edges    pool_ops.filter_edges (one host read)                      | filter_adj's tensor code
    sagpool fwd     SAGPool(64, 0.5) forward on the kernels                    | the same layer with the switch off
    sagpool f+b     forward and backward of sum(pooled x)                      | the same

Before anything is timed the two results of every case are compared; they must be equal or the run stops.  Device events around
every call, median of --reps after --warmup, minimum and maximum next to it.  A host read inside a call is part of what is timed
(the events bracket the whole call).

    python scripts/bench_pool.py [--reps 5] [--out profiles/pool/bench_pool.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402
from pgl_amd import pool_ops  # noqa: E402
from pgl_amd.utils.transform import filter_adj  # noqa: E402

SHAPES = [("a", 128, 30), ("b", 4096, 64), ("c", 64, 4000)]


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


class Route(object):
    """with Route(False): the tensor code of this build."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old, pool_ops._ROUTE = pool_ops._ROUTE, self.on

    def __exit__(self, *a):
        pool_ops._ROUTE = self.old


def routed(on, fn):
    def run():
        with Route(on):
            return fn()
    return run


def batch(n_graphs, n_nodes, degree, dim, seed):
    rng = np.random.default_rng(seed)
    n = n_graphs * n_nodes
    src = rng.integers(0, n_nodes, n * degree) + np.repeat(np.arange(n_graphs), n_nodes * degree) * n_nodes
    dst = rng.integers(0, n_nodes, n * degree) + np.repeat(np.arange(n_graphs), n_nodes * degree) * n_nodes
    edges = np.stack([src, dst], 1).astype(np.int64)
    index = np.arange(n_graphs + 1, dtype=np.int64) * n_nodes
    eindex = np.arange(n_graphs + 1, dtype=np.int64) * n_nodes * degree
    g = pgl.Graph(edges=edges, num_nodes=n, _num_graph=n_graphs, _graph_node_index=index, _graph_edge_index=eindex).tensor()
    x = torch.as_tensor(rng.standard_normal((n, dim)).astype(np.float32)).cuda()
    return g, x, index


def same(a, b, what):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for u, v in zip(a, b):
        if not torch.equal(u, v):
            raise SystemExit("bench_pool: the two paths differ at %s: nothing is timed" % what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--degree", type=int, default=8)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for tag, G, m in SHAPES:
        g, x, index = batch(G, m, args.degree, args.dim, seed=1)
        n = G * m
        gid = g.graph_node_id
        gen = torch.Generator(device="cuda"); gen.manual_seed(2)
        score = torch.randn(n, generator=gen, device="cuda")
        lens = np.diff(index)
        k = pool_ops.topk_counts(lens, 0.5)
        out_ptr = np.concatenate([np.zeros(1, np.int64), np.cumsum(k)])
        seg_d, out_d = torch.from_numpy(index).cuda(), torch.from_numpy(out_ptr).cuda()
        cases = []
        # top-k
        kern = lambda: pool_ops.topk_perm(score, seg_d, out_d, int(out_ptr[-1]))
        dense = routed(False, lambda: pgl.math.segment_topk(x, score, gid, 0.5, return_index=True)[1])
        perm = kern()
        same(perm, dense(), "topk_perm %s" % tag)
        cases.append(("topk_perm", kern, dense))
        # edge filter
        kern_f = lambda: pool_ops.filter_edges(g.edges, perm, n)[0]
        dense_f = routed(False, lambda: filter_adj(g.edges, perm, num_nodes=n)[0])
        same(kern_f(), dense_f(), "filter_edges %s" % tag)
        cases.append(("filter_edges", kern_f, dense_f))
        # the layer
        torch.manual_seed(0)
        layer = pgl.nn.SAGPool(args.dim, 0.5).cuda()

        def fwd():
            px, b, pg = layer(g, x)
            return px, b, pg.edges

        def fwd_bwd():
            xr = x.detach().requires_grad_(True)
            layer.zero_grad()
            px, _, _ = layer(g, xr)
            px.sum().backward()
            return px.detach(), xr.grad

        for name, fn in (("sagpool fwd", fwd), ("sagpool f+b", fwd_bwd)):
            same(routed(True, fn)(), routed(False, fn)(), "%s %s" % (name, tag))
            cases.append((name, routed(True, fn), routed(False, fn)))
        for name, a, b in cases:
            ta, tb = timed(a, args.warmup, args.reps), timed(b, args.warmup, args.reps)
            rows.append(dict(shape=tag, graphs=G, nodes_per_graph=m, edges=int(g.num_edges), case=name, kernel_ms=ta, torch_ms=tb,
                             ratio=tb[0] / ta[0]))
            print(json.dumps(rows[-1]), flush=True)
    lines = ["shape  graphs x nodes   case           kernels ms (min .. max)        torch ms (min .. max)          torch / kernels"]
    for r in rows:
        lines.append("%-5s  %5d x %-6d   %-13s  %8.3f (%7.3f .. %7.3f)   %8.3f (%7.3f .. %7.3f)   %6.2f" %
                     ((r["shape"], r["graphs"], r["nodes_per_graph"], r["case"]) + r["kernel_ms"] + r["torch_ms"] + (r["ratio"],)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
