#!/usr/bin/env python3
"""GAT attention on 16-bit rows on one MI355X: the native route (attention_ops.gat_aggregate16 through Graph.gat_aggregate,
GATConv.fused_16bit = True) next to the up-cast route of the same build (an fp32 copy of the projected features through the fp32
kernels, the result cast back: GATConv.fused_16bit = False), in one process.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator).

    full graph   "op":    feature [N, H, D] fp16 / bf16, attn_src, attn_dst [N, H] fp32 -> [N, H, D] for --shapes (4x8, 8x16, 2x64, 8x32)
                 "layer": GATConv(128 -> H x D).to(dtype) for the same shapes, feat_drop = attn_drop = 0
    block        the outermost block of one NeighborSampler batch of --seeds seeds at fan-outs --fanouts (512 x 25 x 10): the same op
                 and layer (8 x 16) over the block's own nodes

Every row is timed forward and forward + backward with device events around the calls (scripts/bench_dot_attention.measure): median
of --reps after --warmup, minimum and maximum next to it.  The up-cast route is timed TWICE, before and after the native one: the
distance between its two medians is the margin within which two times count as equal.  "fp32 op": the fp32 fused op of the same shape
on fp32 features, timed after them.  "agree": the two outputs within 1e-5 (the op rows compute the same bits; a layer's native route
projects its scores in the storage type, so its rows differ by the storage type's rounding and say NO).  Peak memory: the highest
torch.cuda.max_memory_allocated above the level before the call, over one forward + backward of the layer, for both routes.
No dropout anywhere.

    python scripts/bench_gat16.py [--reps 20] [--out profiles/gat16/bench_gat16.txt]
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
from pgl_amd.utils.rmat import rmat_edges  # noqa: E402
from bench_dot_attention import measure, timed  # noqa: E402  (the timing harness: timed(), the agreement check, one JSON row per mode)

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _fp32_op(rows, g, H, D, args, gen):
    """The fp32 fused op of the same shape, forward and forward + backward, appended to the two rows measure() just wrote."""
    n, dev = g.num_nodes, g.edges.device
    x = torch.randn(n, H, D, generator=gen, device=dev).requires_grad_(True)
    a_s, a_d = (torch.randn(n, H, generator=gen, device=dev).requires_grad_(True) for _ in range(2))

    def both():
        for t in (x, a_s, a_d):
            t.grad = None
        out = g.gat_aggregate(x, a_s, a_d, 0.2)
        out.backward(torch.ones_like(out))
        return out

    with torch.no_grad():
        rows[-2]["fp32_op"] = timed(lambda: g.gat_aggregate(x, a_s, a_d, 0.2), args.warmup, args.reps)[0]
    rows[-1]["fp32_op"] = timed(both, args.warmup, args.reps)[0]


def op_rows(rows, what, g, H, D, name, args, gen):
    n, dev, dt = g.num_nodes, g.edges.device, DTYPES[name]
    x = torch.randn(n, H, D, generator=gen, device=dev).to(dt).requires_grad_(True)
    a_s, a_d = (torch.randn(n, H, generator=gen, device=dev).requires_grad_(True) for _ in range(2))
    measure(rows, "%s: op %s" % (what, name), n, int(g.num_edges), (H, D), lambda: g.gat_aggregate(x.float(), a_s, a_d, 0.2).to(dt),
            lambda: g.gat_aggregate(x, a_s, a_d, 0.2), args, [x, a_s, a_d])
    _fp32_op(rows, g, H, D, args, gen)


def _peak(fn, inputs):
    for t in inputs:
        t.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    for t in inputs:
        t.grad = None
    return int(peak)


def layer_rows(rows, what, g, H, D, name, args, gen):
    n, dev, dt = g.num_nodes, g.edges.device, DTYPES[name]
    torch.manual_seed(0)
    up = pgl.nn.GATConv(128, D, num_heads=H, feat_drop=0.0, attn_drop=0.0).to(dev).to(dt)
    native = pgl.nn.GATConv(128, D, num_heads=H, feat_drop=0.0, attn_drop=0.0).to(dev).to(dt)
    native.load_state_dict(up.state_dict())
    native.fused_16bit = True
    x = torch.randn(n, 128, generator=gen, device=dev).to(dt).requires_grad_(True)
    inputs = [x] + list(up.parameters()) + list(native.parameters())
    measure(rows, "%s: layer 128 -> %dx%d %s" % (what, H, D, name), n, int(g.num_edges), (H, D), lambda: up(g, x), lambda: native(g, x), args, inputs)
    pgl.ops.release_workspaces()
    rows[-1]["peak_bytes_up_cast"] = _peak(lambda: up(g, x), inputs)
    rows[-1]["peak_bytes_native"] = _peak(lambda: native(g, x), inputs)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--shapes", type=int, nargs="+", default=[4, 8, 8, 16, 2, 64, 8, 32], help="H D pairs: 1, 2, 2 and 4 elements per lane")
    ap.add_argument("--dtypes", nargs="+", default=["fp16", "bf16"], choices=sorted(DTYPES))
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
    for name in args.dtypes:
        for H, D in shapes:
            assert attention_ops.gat16_supported(H, D, backward=True), (H, D)
            op_rows(rows, "full graph", g, H, D, name, args, gen)
        for H, D in shapes:
            layer_rows(rows, "full graph", g, H, D, name, args, gen)

    nodes = torch.randint(0, N, (args.seeds,), device=dev, generator=torch.Generator(device=dev).manual_seed(args.seeds))
    blocks, _ = pgl.sampling.NeighborSampler(g, args.fanouts, seed=1).sample_neighbors(nodes)
    block = blocks[0][0]                                     # outermost layer first: the largest block of the batch
    what = "block of %d seeds x %s" % (args.seeds, " x ".join(str(f) for f in args.fanouts))
    for name in args.dtypes:
        op_rows(rows, what, block, 8, 16, name, args, gen)
        layer_rows(rows, what, block, 8, 16, name, args, gen)

    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": args.edges, "warmup": args.warmup, "reps": args.reps, "rows": rows}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        fmt = lambda t: "%.3f (%.3f .. %.3f)" % (t["ms"], t["ms_min"], t["ms_max"]) if t else "-"
        mib = lambda r, k: "%.0f" % (r[k] / 2 ** 20) if k in r else "-"
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges; median ms of %d after %d warm-up calls (min .. max)\n" % (res["graph"], N, args.edges, args.reps, args.warmup))
            f.write("| what | nodes | edges | H x D | mode | up-cast | up-cast again | margin | native | up-cast / native | verdict | fp32 op | agree | "
                    "peak MiB up-cast | peak MiB native |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                a, b, t = r["three_ops"]["ms"], r["three_ops_again"]["ms"], r["fused"]["ms"]
                margin = abs(a - b)
                verdict = "faster" if t < min(a, b) - margin else "slower" if t > max(a, b) + margin else "tie"
                f.write("| %s | %d | %d | %s | %s | %s | %s | %.3f | %s | %.2f | %s | %s | %s | %s | %s |\n"
                        % (r["what"], r["nodes"], r["edges"], r["shape"], r["mode"], fmt(r["three_ops"]), fmt(r["three_ops_again"]), margin,
                           fmt(r["fused"]), r["three_ops_over_fused"], verdict, fmt(r.get("fp32_op")), "yes" if r["outputs_agree"] else "NO",
                           mib(r, "peak_bytes_up_cast"), mib(r, "peak_bytes_native")))
    return res


if __name__ == "__main__":
    main()
