#!/usr/bin/env python3
"""GraphMultisetTransformer on one MI355X: fused=True (the pooling blocks' attention on the seed-attention kernels, csrc/seed_readout.hip,
front end pgl_amd/readout_ops.py: seed_attention_readout) next to fused=False of the same build (to_dense_batch, head reshuffles, two
bmm and a softmax per block), the same parameters, the same batched graphs, in the same process.

Shapes (graphs x nodes per graph, a ring of edges in every graph):  (a) 128 x 30,  (b) 4096 x 64,  (c) 64 x 4000,  (d) 1 x 2**20 -- the
shapes of scripts/bench_readout.py -- and (e) an uneven batch, 4 graphs of 10 000 nodes among 252 graphs of 30 (the dense view pads
every graph to 10 000 slots).  dim = 128, 4 heads; pooling_ratio is chosen so that GMPool_G has k = 1, 8 or 32 seeds.  The unfused
layer is not run where its dense [B, max_nodes, dim] view would pass --dense-cap bytes (said so in the table: "not run").

Before anything is timed the two outputs (within 1e-4 of the largest value) and the input gradients (within 1e-2) are compared; they
must agree or the run stops.  The gradient bar is that wide because of the ReLU in each block's tail: a pre-activation within rounding
of 0 switches between two fp32 paths and moves one graph's gradient by one unit in dim (measured at shape c, k = 8: the UNFUSED path
is 3.6e-3 of the largest value away from an fp64 run on one graph of 64, the fused one 8e-6; profiles/seed_readout/README.md).  Device events around every call, median of --reps after --warmup, minimum and maximum next to it.

    python scripts/bench_seed_readout.py [--reps 5] [--out profiles/seed_readout/bench_seed_readout.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402
from pgl_amd import readout_ops  # noqa: E402

SHAPES = [("a", [30] * 128), ("b", [64] * 4096), ("c", [4000] * 64), ("d", [1 << 20]),
          ("e", ([30] * 63 + [10000]) * 4)]
DIM, HEADS, SEEDS = 128, 4, (1, 8, 32)


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


def batch(sizes, dim, seed):
    """A batched tensor graph whose member graphs are rings, with a host _graph_node_index as Graph.disjoint makes it."""
    index = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(index[-1])
    src = np.arange(n, dtype=np.int64)
    gid = np.repeat(np.arange(len(sizes)), sizes)
    dst = index[gid] + (src - index[gid] + 1) % np.asarray(sizes)[gid]
    edges = torch.as_tensor(np.stack([src, dst], 1)).cuda()
    g = pgl.Graph(edges=edges, num_nodes=n, _num_graph=len(sizes), _graph_node_index=index,
                  _graph_edge_index=index.copy())
    x = torch.as_tensor(np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)).cuda()
    return g, x


def close(a, b, what):
    for u, v, tol in zip(a, b, (1e-4, 1e-2)):
        if not bool(((u - v).abs() <= tol * v.abs().max() + 1e-6).all()):
            raise SystemExit("bench_seed_readout: the two paths differ at %s: nothing is timed" % what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dense-cap", type=float, default=8e9, help="largest dense view (bytes) the unfused layer is run on")
    ap.add_argument("--shapes", default="abcde")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for tag, sizes in SHAPES:
        if tag not in args.shapes:
            continue
        g, x = batch(sizes, DIM, seed=1)
        run_unfused = len(sizes) * max(sizes) * DIM * 4 <= args.dense_cap
        for seeds in SEEDS:
            torch.manual_seed(0)
            layer = pgl.nn.GraphMultisetTransformer(DIM, DIM, DIM, num_nodes=seeds, pooling_ratio=1.0, num_heads=HEADS, fused=True).cuda()
            assert layer.pools[0].num_seeds == seeds and layer._takes_fused(g, layer.lin1(x))

            def forward(fused):
                def run():
                    layer.fused = fused
                    with torch.no_grad():
                        return (layer(g, x),)
                return run

            def both(fused):
                def run():
                    layer.fused = fused
                    xx = x.detach().requires_grad_(True)
                    out = layer(g, xx)
                    out.sum().backward()
                    return out.detach(), xx.grad
                return run

            for kind, make in (("fwd", forward), ("f+b", both)):
                before = readout_ops.LAUNCHES["seed_readout"]
                got = make(True)()
                assert readout_ops.LAUNCHES["seed_readout"] == before + 2
                ta = timed(make(True), args.warmup, args.reps)
                tb = None
                if run_unfused:
                    close(got, make(False)(), "%s k=%d %s" % (tag, seeds, kind))
                    tb = timed(make(False), args.warmup, args.reps)
                rows.append(dict(shape=tag, graphs=len(sizes), nodes=int(np.sum(sizes)), max_nodes=int(max(sizes)), k=seeds, case=kind,
                                 fused_ms=ta, unfused_ms=tb, ratio=None if tb is None else tb[0] / ta[0]))
                print(json.dumps(rows[-1]), flush=True)
            del layer
        del g, x
        torch.cuda.empty_cache()
    lines = ["shape  graphs   nodes    max nodes   k  case   fused ms (min .. max)          unfused ms (min .. max)        unfused / fused"]
    for r in rows:
        un = "%8.3f (%7.3f .. %7.3f)   %6.2f" % (r["unfused_ms"] + (r["ratio"],)) if r["unfused_ms"] else "not run (the dense view passes --dense-cap)"
        lines.append("%-5s  %6d  %8d  %8d  %2d  %-5s  %8.3f (%7.3f .. %7.3f)   %s" %
                     ((r["shape"], r["graphs"], r["nodes"], r["max_nodes"], r["k"], r["case"]) + r["fused_ms"] + (un,)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
