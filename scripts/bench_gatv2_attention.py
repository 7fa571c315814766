#!/usr/bin/env python3
"""GATv2 attention on one MI355X: the fused kernels (Graph.gatv2_attention, GATv2Conv(fused=True)) next to the three-op composition
of the same build (add_score -> segment softmax -> edge-weighted aggregation: GATv2Conv(fused=False), pgl_amd/nn/conv_more.py), in
one process.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator).

    full graph   "op":    x [N, H, D], attn [H, D] -> [N, H, D] for --shapes (4x8, 8x16, 2x64, 8x32), one tensor on both sides as the layer has it
                 "layer": GATv2Conv(128 -> H x D) for the same shapes, feat_drop = attn_drop = 0
    block        the outermost block of one NeighborSampler batch of --seeds seeds at fan-outs --fanouts (512 x 25 x 10): the same op
                 and layer (8 x 16) over the block's own nodes

Every row is timed forward and forward + backward (the gradients w.r.t. x and attn resp. the input and the parameters), with device
events around the calls, median of --reps after --warmup, minimum and maximum next to it.  The composition is timed TWICE, before
and after the fused form ("three ops" and "three ops again"): the distance between its two medians is the margin within which two
times count as equal.  The outputs of the two forms are compared (1e-5 relative plus 1e-5 of the row's largest value, as
tests/gpu_common.close_rows) and the verdict is part of every row ("agree").  No dropout anywhere.

    python scripts/bench_gatv2_attention.py [--reps 20] [--out profiles/gatv2_attention/bench_gatv2_attention.txt]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgl_amd as pgl  # noqa: E402
from pgl_amd import attention_ops, autograd as ag, ops  # noqa: E402
from pgl_amd.utils.rmat import rmat_edges  # noqa: E402
from bench_dot_attention import measure  # noqa: E402  (the timing harness: timed(), the agreement check, one JSON row per mode)


def three_ops(g, x, attn):
    """What GATv2Conv(fused=False) runs between its projection and its head reshape."""
    H = int(x.shape[1])
    cd, cs = g._csr_order_views()
    alpha = ag.add_score(x, x, attn, cd, lambda: cs, 0.2)
    alpha = ag.segment_softmax(alpha, ops.SegView(cd.indptr, cd.row32, cd.row32, None))
    return ag.aggregate(x.contiguous(), cd, lambda: cs, "sum", None, alpha.reshape(-1, H, 1), "mul")


def op_rows(rows, what, g, H, D, args, gen):
    n, dev = g.num_nodes, g.edges.device
    x = torch.randn(n, H, D, generator=gen, device=dev).requires_grad_(True)
    attn = (torch.randn(H, D, generator=gen, device=dev) * D ** -0.5).requires_grad_(True)
    measure(rows, what + ": op", n, int(g.num_edges), (H, D), lambda: three_ops(g, x, attn), lambda: g.gatv2_attention(x, attn), args, [x, attn])


def layer_rows(rows, what, g, H, D, args, gen):
    n, dev = g.num_nodes, g.edges.device
    torch.manual_seed(0)
    plain = pgl.nn.GATv2Conv(128, D, num_heads=H, feat_drop=0.0, attn_drop=0.0).to(dev)
    fused = pgl.nn.GATv2Conv(128, D, num_heads=H, feat_drop=0.0, attn_drop=0.0, fused=True).to(dev)
    fused.load_state_dict(plain.state_dict())
    x = torch.randn(n, 128, generator=gen, device=dev).requires_grad_(True)
    assert fused._takes_fused(g, x) and not plain._takes_fused(g, x)
    measure(rows, what + ": layer 128 -> %dx%d" % (H, D), n, int(g.num_edges), (H, D), lambda: plain(g, x), lambda: fused(g, x), args,
            [x] + list(plain.parameters()) + list(fused.parameters()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--shapes", type=int, nargs="+", default=[4, 8, 8, 16, 2, 64, 8, 32], help="H D pairs: 1, 2, 2 and 4 floats per lane")
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
    shapes = list(zip(args.shapes[0::2], args.shapes[1::2]))
    for H, D in shapes:
        assert attention_ops.gatv2_attention_supported(H, D), (H, D)
        op_rows(rows, "full graph", g, H, D, args, gen)
    for H, D in shapes:
        layer_rows(rows, "full graph", g, H, D, args, gen)

    nodes = torch.randint(0, N, (args.seeds,), device=dev, generator=torch.Generator(device=dev).manual_seed(args.seeds))
    blocks, _ = pgl.sampling.NeighborSampler(g, args.fanouts, seed=1).sample_neighbors(nodes)
    block = blocks[0][0]                                     # outermost layer first: the largest block of the batch
    what = "block of %d seeds x %s" % (args.seeds, " x ".join(str(f) for f in args.fanouts))
    op_rows(rows, what, block, 8, 16, args, gen)
    layer_rows(rows, what, block, 8, 16, args, gen)

    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": args.edges, "warmup": args.warmup, "reps": args.reps, "rows": rows}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        fmt = lambda t: "%.3f (%.3f .. %.3f)" % (t["ms"], t["ms_min"], t["ms_max"])
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges; median ms of %d after %d warm-up calls (min .. max)\n" % (res["graph"], N, args.edges, args.reps, args.warmup))
            f.write("| what | nodes | edges | H x D | mode | three ops | three ops again | fused | three ops / fused | agree |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %d | %d | %s | %s | %s | %s | %s | %.2f | %s |\n"
                        % (r["what"], r["nodes"], r["edges"], r["shape"], r["mode"], fmt(r["three_ops"]), fmt(r["three_ops_again"]), fmt(r["fused"]),
                           r["three_ops_over_fused"], "yes" if r["outputs_agree"] else "NO"))
    return res


if __name__ == "__main__":
    main()
