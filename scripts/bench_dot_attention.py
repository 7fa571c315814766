#!/usr/bin/env python3
"""Dot-product attention on one MI355X: the fused kernels (Graph.dot_attention, TransformerConv(fused=True)) next to the three-op
composition of the same build (sddmm -> segment softmax -> edge-weighted aggregation: pgl_amd/nn/conv_more.py _dot_attention,
TransformerConv(fused=False)).

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator).

    full graph   "op":    q, k, v [N, H, D] -> [N, H, D] for --shapes (8x16, 2x64, 4x8, 8x32); the composition divides q by sqrt(D) first, as the
                          layer does (one pass over [N, H*D], inside the timed call), the fused op takes the raw q and the scale
                 "layer": TransformerConv(128 -> 8 x 16), feat_drop = attn_drop = 0
    block        the outermost block of one NeighborSampler batch of --seeds seeds at fan-outs --fanouts (512 x 25 x 10): the same op
                 (8 x 16) and layer over the block's own nodes

Every row is timed forward and forward + backward (the gradients w.r.t. q, k, v resp. the input and the parameters), with device
events around the calls, median of --reps after --warmup, minimum and maximum next to it.  The composition is timed TWICE, before
and after the fused form ("three ops" and "three ops again"): the distance between its two medians is the margin within which two
times count as equal.  The outputs of the two forms are compared (1e-5 relative plus 1e-5 of the row's largest value, as
tests/gpu_common.close_rows) and the verdict is part of every row ("agree").

    python scripts/bench_dot_attention.py [--reps 20] [--out profiles/dot_attention/bench_dot_attention.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402
from pgl_amd.nn.conv_more import _dot_attention  # noqa: E402
from pgl_amd.utils.rmat import rmat_edges  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(ms=round(float(np.median(ms)), 4), ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4)), out


def same(got, want):
    got, want = got.detach().double(), want.detach().double()
    row = want.abs().reshape(want.shape[0], -1).max(1).values.reshape((-1,) + (1,) * (want.dim() - 1)) if want.numel() else 0.0
    return bool(((got - want).abs() <= 1e-5 * want.abs() + 1e-5 * row + 1e-30).all())


def measure(rows, what, nodes, edges, shape, three_ops, fused, args, inputs):
    """three_ops / fused: callables -> output; timed forward and forward + backward over `inputs` (tensors that require grad)."""
    def with_backward(fn):
        def run():
            for t in inputs:
                t.grad = None
            out = fn()
            out.backward(torch.ones_like(out))
            return out
        return run

    for mode, wrap in (("forward", lambda f: (lambda: f())), ("forward+backward", with_backward)):
        ctx = torch.no_grad() if mode == "forward" else torch.enable_grad()
        with ctx:
            t_ops, want = timed(wrap(three_ops), args.warmup, args.reps)
            t_fused, got = timed(wrap(fused), args.warmup, args.reps)
            t_again, _ = timed(wrap(three_ops), args.warmup, args.reps)
        r = {"what": what, "nodes": nodes, "edges": edges, "shape": "%dx%d" % shape, "mode": mode, "outputs_agree": same(got, want),
             "three_ops": t_ops, "three_ops_again": t_again, "fused": t_fused,
             "three_ops_over_fused": round(min(t_ops["ms"], t_again["ms"]) / t_fused["ms"], 3)}
        rows.append(r)
        print(json.dumps(r), flush=True)


def op_rows(rows, what, g, H, D, args, gen):
    n, dev = g.num_nodes, g.edges.device
    q, k, v = (torch.randn(n, H, D, generator=gen, device=dev).requires_grad_(True) for _ in range(3))
    scale = D ** -0.5
    measure(rows, what + ": op", n, int(g.num_edges), (H, D), lambda: _dot_attention(g, k, q * scale, v),
            lambda: g.dot_attention(q, k, v, scale), args, [q, k, v])


def layer_rows(rows, what, g, args, gen):
    n, dev = g.num_nodes, g.edges.device
    torch.manual_seed(0)
    plain = pgl.nn.TransformerConv(128, 16, num_heads=8, feat_drop=0.0, attn_drop=0.0).to(dev)
    fused = pgl.nn.TransformerConv(128, 16, num_heads=8, feat_drop=0.0, attn_drop=0.0, fused=True).to(dev)
    fused.load_state_dict(plain.state_dict())
    x = torch.randn(n, 128, generator=gen, device=dev).requires_grad_(True)
    assert fused._takes_fused(g, x, None) and not plain._takes_fused(g, x, None)
    measure(rows, what + ": layer 128 -> 8x16", n, int(g.num_edges), (8, 16), lambda: plain(g, x), lambda: fused(g, x), args,
            [x] + list(plain.parameters()) + list(fused.parameters()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--shapes", type=int, nargs="+", default=[8, 16, 2, 64, 4, 8, 8, 32], help="H D pairs: 2, 2, 1 and 4 floats per lane")
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
    for H, D in zip(args.shapes[0::2], args.shapes[1::2]):
        assert pgl.ops.dot_attention_supported(H, D), (H, D)
        op_rows(rows, "full graph", g, H, D, args, gen)
    layer_rows(rows, "full graph", g, args, gen)

    nodes = torch.randint(0, N, (args.seeds,), device=dev, generator=torch.Generator(device=dev).manual_seed(args.seeds))
    blocks, _ = pgl.sampling.NeighborSampler(g, args.fanouts, seed=1).sample_neighbors(nodes)
    block = blocks[0][0]                                     # outermost layer first: the largest block of the batch
    what = "block of %d seeds x %s" % (args.seeds, " x ".join(str(f) for f in args.fanouts))
    op_rows(rows, what, block, 8, 16, args, gen)
    layer_rows(rows, what, block, args, gen)

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
