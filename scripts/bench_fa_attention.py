#!/usr/bin/env python3
"""FAGCN's frequency-adaptive attention on one MI355X: the fused kernels (Graph.fa_aggregate, FAConv(fused=True)) next to the chain of
edge-wise ops of the same build (two send_uv, a tanh, a product, a dropout, a send_ue_recv: FAConv(fused=False),
pgl_amd/nn/conv_more.py -- code this build did not touch), in one process.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator).

    full graph   "op":    x [N, d], p_src, p_dst [N, 1], the degree norms -> [N, d] for --sizes (32, 64, 128, 256)
                 "layer": FAConv(d) for the same sizes, drop = 0
                 "layer, drop 0.5, train()": FAConv(--drop_size) in training mode with dropout on -- nn.Dropout's mask in the chain,
                 the in-kernel mask in the fused form (the outputs are different draws and are not compared)
    block        the outermost block of one NeighborSampler batch of --seeds seeds at fan-outs --fanouts (512 x 25 x 10): the same op
                 and layer (d = 128) over the block's own nodes

Every row is timed forward and forward + backward (the gradients w.r.t. x and the gate halves resp. the input and the parameters),
with device events around the calls, median of --reps after --warmup, minimum and maximum next to it.  The chain is timed TWICE,
before and after the fused form ("chain" and "chain again"): the distance between its two medians is the margin within which two
times count as equal.  The outputs of the two forms are compared (1e-5 relative plus 1e-5 of the row's largest value, as
tests/gpu_common.close_rows) and the verdict is part of every row ("agree").

    python scripts/bench_fa_attention.py [--reps 20] [--out profiles/fa_attention/bench_fa_attention.txt]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgl_amd as pgl  # noqa: E402
from pgl_amd import attention_ops  # noqa: E402
from pgl_amd.nn import functional as GF  # noqa: E402
from pgl_amd.utils.rmat import rmat_edges  # noqa: E402
from bench_dot_attention import measure  # noqa: E402  (the timing harness: timed(), the agreement check, one JSON row per mode)


def chain(g, x, p_src, p_dst, norm):
    """What FAConv(fused=False) runs after its two projections (drop = 0)."""
    alpha = torch.tanh(g.send_uv(p_src, p_dst, "add")) * g.send_uv(norm, norm, "mul")
    return g.send_ue_recv(x, alpha, "mul", "sum")


def op_rows(rows, what, g, d, args, gen):
    n, dev = g.num_nodes, g.edges.device
    x = torch.randn(n, d, generator=gen, device=dev).requires_grad_(True)
    p_src, p_dst = (torch.randn(n, 1, generator=gen, device=dev).requires_grad_(True) for _ in range(2))
    norm = GF.degree_norm(g)
    measure(rows, what + ": op", n, int(g.num_edges), (1, d), lambda: chain(g, x, p_src, p_dst, norm),
            lambda: g.fa_aggregate(x, p_src, p_dst, norm, norm), args, [x, p_src, p_dst])


def layer_rows(rows, what, g, d, args, gen, drop=0.0):
    n, dev = g.num_nodes, g.edges.device
    torch.manual_seed(0)
    plain = pgl.nn.FAConv(d, drop=drop).to(dev)
    fused = pgl.nn.FAConv(d, drop=drop, fused=True).to(dev)
    fused.load_state_dict(plain.state_dict())
    plain.train(drop > 0); fused.train(drop > 0)
    x = torch.randn(n, d, generator=gen, device=dev).requires_grad_(True)
    assert fused._takes_fused(g, x) and not plain._takes_fused(g, x)
    tag = ": layer FAConv(%d)" % d + (", drop %g, train()" % drop if drop > 0 else "")
    measure(rows, what + tag, n, int(g.num_edges), (1, d), lambda: plain(g, x), lambda: fused(g, x), args,
            [x] + list(plain.parameters()) + list(fused.parameters()))
    if drop > 0:
        for r in rows[-2:]:
            r["outputs_agree"] = None                        # two different masks


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 64, 128, 256], help="hidden sizes: 1, 1, 2 and 4 floats per lane")
    ap.add_argument("--drop_size", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=512)
    ap.add_argument("--fanouts", type=int, nargs="+", default=[25, 10])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    N = 1 << args.scale
    edges = rmat_edges(args.scale, args.edges, seed=42, device=dev)
    g = pgl.Graph(edges=edges, num_nodes=N).tensor(device=dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    for d in args.sizes:
        assert attention_ops.fa_supported(1, d), d
        op_rows(rows, "full graph", g, d, args, gen)
    for d in args.sizes:
        layer_rows(rows, "full graph", g, d, args, gen)
    layer_rows(rows, "full graph", g, args.drop_size, args, gen, drop=0.5)

    nodes = torch.randint(0, N, (args.seeds,), device=dev, generator=torch.Generator(device=dev).manual_seed(args.seeds))
    blocks, _ = pgl.sampling.NeighborSampler(g, args.fanouts, seed=1).sample_neighbors(nodes)
    block = blocks[0][0]                                     # outermost layer first: the largest block of the batch
    what = "block of %d seeds x %s" % (args.seeds, " x ".join(str(f) for f in args.fanouts))
    op_rows(rows, what, block, 128, args, gen)
    layer_rows(rows, what, block, 128, args, gen)

    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": args.edges, "warmup": args.warmup, "reps": args.reps, "rows": rows}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        fmt = lambda t: "%.3f (%.3f .. %.3f)" % (t["ms"], t["ms_min"], t["ms_max"])
        agree = {True: "yes", False: "NO", None: "n/a"}
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges; median ms of %d after %d warm-up calls (min .. max)\n" % (res["graph"], N, args.edges, args.reps, args.warmup))
            f.write("| what | nodes | edges | H x D | mode | chain | chain again | fused | chain / fused | agree |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %d | %d | %s | %s | %s | %s | %s | %.2f | %s |\n"
                        % (r["what"], r["nodes"], r["edges"], r["shape"], r["mode"], fmt(r["three_ops"]), fmt(r["three_ops_again"]), fmt(r["fused"]),
                           r["three_ops_over_fused"], agree[r["outputs_agree"]]))
    return res


if __name__ == "__main__":
    main()
