#!/usr/bin/env python3
"""Dot-product attention WITH EDGE FEATURES on one MI355X: the fused kernels (Graph.dot_attention(edge_feat=...),
TransformerConv(fused=True, fused_edge_feat=True)) next to the user-function path of the same build (Graph.send / Graph.recv with the
layer's message and reduce functions: TransformerConv.send_recv, what fused=False runs when edge_feat is given), and next to the fused op
WITHOUT edge features (Graph.dot_attention), which shows what the third gathered operand costs.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator), the sizes of scripts/bench_dot_attention.py.

    full graph   "op":    q, k, v [N, H, D], ef [E, H, D] -> [N, H, D] for --shapes (4x8, 8x16, 2x64, 8x32)
                 "layer": TransformerConv(128 -> 8 x 16), feat_drop = attn_drop = 0, edge_feat [E, 128]
    block        the outermost block of one NeighborSampler batch of --seeds seeds at fan-outs --fanouts (512 x 25 x 10): the same op
                 (8 x 16) and layer over the block's own nodes

Every row is timed forward and forward + backward, the latter with the gradient of the edge feature ("d ef on") and without it ("d ef
off": edge_feat.requires_grad = False, the kernel stores no per-edge row), with device events around the calls, median of --reps after
--warmup, minimum and maximum next to it.  The user-function path is timed TWICE, before and after the fused form ("send/recv" and
"send/recv again"): the distance between its two medians is the margin within which two times count as equal.  The outputs of the two
forms are compared (1e-5 relative plus 1e-5 of the row's largest value, as tests/gpu_common.close_rows) and the verdict is part of every
row ("agree").  A form that runs out of memory is recorded as such, not skipped silently.

    python scripts/bench_dot_attention_edge.py [--reps 20] [--out profiles/dot_attention_edge/bench_dot_attention_edge.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402
from pgl_amd import attention_ops  # noqa: E402
from pgl_amd.utils.rmat import rmat_edges  # noqa: E402


def timed(fn, warmup, reps):
    try:
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms, out = [], None
        for _ in range(reps):
            out = None
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None, None
    return dict(ms=round(float(np.median(ms)), 4), ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4)), out


def same(got, want):
    if got is None or want is None:
        return None
    got, want = got.detach().double(), want.detach().double()
    row = want.abs().reshape(want.shape[0], -1).max(1).values.reshape((-1,) + (1,) * (want.dim() - 1)) if want.numel() else 0.0
    return bool(((got - want).abs() <= 1e-5 * want.abs() + 1e-5 * row + 1e-30).all())


def measure(rows, what, nodes, edges, shape, send_recv, fused, no_ef, args, inputs, ef):
    """send_recv / fused / no_ef: callables -> output; timed forward and forward + backward over `inputs` (tensors that require grad),
    the backward with and without the gradient of `ef`."""
    def with_backward(fn):
        def run():
            for t in inputs + [ef]:
                t.grad = None
            out = fn()
            out.backward(torch.ones_like(out))
            return out
        return run

    for mode, wrap, ef_grad in (("forward", lambda f: (lambda: f()), False), ("forward+backward, d ef on", with_backward, True),
                                ("forward+backward, d ef off", with_backward, False)):
        ef.requires_grad_(ef_grad)
        ctx = torch.no_grad() if mode == "forward" else torch.enable_grad()
        with ctx:
            t_ref, want = timed(wrap(send_recv), args.warmup, args.reps)
            t_fused, got = timed(wrap(fused), args.warmup, args.reps)
            agree = same(got, want)
            want = got = None
            t_again, _ = timed(wrap(send_recv), args.warmup, args.reps)
            t_no_ef, _ = timed(wrap(no_ef), args.warmup, args.reps)
        best = min(t["ms"] for t in (t_ref, t_again) if t is not None) if (t_ref or t_again) else None
        r = {"what": what, "nodes": nodes, "edges": edges, "shape": "%dx%d" % shape, "mode": mode, "outputs_agree": agree,
             "send_recv": t_ref, "send_recv_again": t_again, "fused": t_fused, "fused_without_edge_feat": t_no_ef,
             "send_recv_over_fused": None if best is None or t_fused is None else round(best / t_fused["ms"], 3),
             "fused_over_fused_without_edge_feat": None if t_fused is None or t_no_ef is None else round(t_fused["ms"] / t_no_ef["ms"], 3)}
        rows.append(r)
        print(json.dumps(r), flush=True)
    ef.requires_grad_(False)


def op_rows(rows, what, g, H, D, args, gen):
    n, e, dev = g.num_nodes, int(g.num_edges), g.edges.device
    assert attention_ops.dot_attention_edge_supported(H, D), (H, D)
    q, k, v = (torch.randn(n, H, D, generator=gen, device=dev).requires_grad_(True) for _ in range(3))
    ef = torch.randn(e, H, D, generator=gen, device=dev)
    layer = pgl.nn.TransformerConv(H * D, D, num_heads=H, feat_drop=0.0, attn_drop=0.0, concat=True)     # (its message / reduce functions only)
    scale = D ** -0.5
    measure(rows, what + ": op", n, e, (H, D), lambda: layer.send_recv(g, q, k, v, ef).reshape(n, H, D),
            lambda: g.dot_attention(q, k, v, scale, edge_feat=ef), lambda: g.dot_attention(q, k, v, scale), args, [q, k, v], ef)


def layer_rows(rows, what, g, args, gen):
    n, e, dev = g.num_nodes, int(g.num_edges), g.edges.device
    torch.manual_seed(0)
    mk = lambda **kw: pgl.nn.TransformerConv(128, 16, num_heads=8, feat_drop=0.0, attn_drop=0.0, **kw).to(dev)
    plain, fused = mk(), mk(fused=True, fused_edge_feat=True)
    fused.load_state_dict(plain.state_dict())
    x = torch.randn(n, 128, generator=gen, device=dev).requires_grad_(True)
    ef = torch.randn(e, 128, generator=gen, device=dev)
    assert fused._takes_fused(g, x, ef) and not plain._takes_fused(g, x, ef)
    measure(rows, what + ": layer 128 -> 8x16", n, e, (8, 16), lambda: plain(g, x, ef), lambda: fused(g, x, ef), lambda: fused(g, x), args,
            [x] + list(plain.parameters()) + list(fused.parameters()), ef)


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
    for H, D in zip(args.shapes[0::2], args.shapes[1::2]):
        op_rows(rows, "full graph", g, H, D, args, gen)
        torch.cuda.empty_cache()
    layer_rows(rows, "full graph", g, args, gen)
    torch.cuda.empty_cache()

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
        fmt = lambda t: "out of memory" if t is None else "%.3f (%.3f .. %.3f)" % (t["ms"], t["ms_min"], t["ms_max"])
        num = lambda x: "-" if x is None else "%.2f" % x
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges; median ms of %d after %d warm-up calls (min .. max)\n" % (res["graph"], N, args.edges, args.reps, args.warmup))
            f.write("| what | nodes | edges | H x D | mode | send/recv | send/recv again | fused | send/recv / fused | fused without edge_feat | "
                    "fused / fused without edge_feat | agree |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %d | %d | %s | %s | %s | %s | %s | %s | %s | %s | %s |\n"
                        % (r["what"], r["nodes"], r["edges"], r["shape"], r["mode"], fmt(r["send_recv"]), fmt(r["send_recv_again"]), fmt(r["fused"]),
                           num(r["send_recv_over_fused"]), fmt(r["fused_without_edge_feat"]), num(r["fused_over_fused_without_edge_feat"]),
                           {True: "yes", False: "NO", None: "-"}[r["outputs_agree"]]))
    return res


if __name__ == "__main__":
    main()
