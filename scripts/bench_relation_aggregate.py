#!/usr/bin/env python3
"""Relational aggregation on one MI355X: the one-launch form (HeterGraph.send_recv_relations, RGCNConv(fused=True)) next to the
per-relation loop of the same build (hg[et].send_recv per edge type plus adds; RGCNConv(fused=False): the reference's loop,
pgl/nn/conv.py:1014-1019).

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator), cut into --relations equal slices
of consecutive edges: every slice is one relation of a HeterGraph over the same 2^20 nodes.  Widths --dims (64 and 128).

    full graph   "aggregate": sum over relations of mean-aggregated x, [N, d] -> [N, d]
                 "layer":     RGCNConv(d, d): order=None (what the byte model picks) and both forced orders
    blocks       one RelationNeighborSampler layer at fan-out --fanout per relation over --seeds seeds (512: a training batch; 524288:
                 a later layer's frontier): RGCNConv(d, d) over the block, conv(block, h, out_size=n_dst) against conv(block, h)[:n_dst]

Every row is timed forward and forward + backward (the gradient w.r.t. the features and the weights), with device events around
the calls, median of --reps after --warmup, minimum and maximum next to it.  The loop is timed TWICE, before and after the fused
form ("loop" and "loop again"): the distance between its two medians is the margin within which two times count as equal.
The outputs of the two forms are compared (1e-5 relative plus 1e-5 of the row's largest value, as tests/gpu_common.close_rows) and
the verdict is part of every row ("agree").

    python scripts/bench_relation_aggregate.py [--reps 20] [--out profiles/relation_aggregate/bench_relation_aggregate.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402
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


def measure(rows, what, size, d, loop, forms, args, inputs):
    """loop / forms[name]: callables -> output; timed forward and forward + backward over `inputs` (tensors that require grad)."""
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
            t_loop, want = timed(wrap(loop), args.warmup, args.reps)
            res, agree = {}, True
            for name, fn in forms.items():
                res[name], got = timed(wrap(fn), args.warmup, args.reps)
                agree = agree and same(got, want)
            t_again, _ = timed(wrap(loop), args.warmup, args.reps)
        r = {"what": what, "size": size, "d": d, "mode": mode, "outputs_agree": agree, "loop": t_loop, "loop_again": t_again}
        for name, t in res.items():
            r[name] = t
            r["loop_over_" + name] = round(min(t_loop["ms"], t_again["ms"]) / t["ms"], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--relations", type=int, default=4)
    ap.add_argument("--fanout", type=int, default=10)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--seeds", type=int, nargs="+", default=[512, 512 * 1024])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    N, R = 1 << args.scale, args.relations
    edges = rmat_edges(args.scale, args.edges, seed=42, device=dev)
    cut = [args.edges * r // R for r in range(R + 1)]
    types = ["r%d" % r for r in range(R)]
    hg = pgl.HeterGraph(edges={et: edges[cut[r]:cut[r + 1]] for r, et in enumerate(types)}, num_nodes=N)
    assert hg.is_tensor()
    stacked = hg._stacked_pred()[0]
    info = {"max_segment": pgl.ops.stacked_max_segment(stacked), "long_row": pgl.ops.LONG_ROW}
    long_rows = pgl.ops.stacked_long_rows(stacked, pgl.ops.LONG_ROW)
    info["long_rows"] = 0 if long_rows is None else int(long_rows.shape[0])
    print(json.dumps(info), flush=True)
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []

    for d in args.dims:
        torch.manual_seed(0)
        x = torch.randn(N, d, generator=gen, device=dev).requires_grad_(True)
        loop_layer = pgl.nn.RGCNConv(d, d, types).to(dev)
        fused_layer = pgl.nn.RGCNConv(d, d, types, fused=True).to(dev)
        fused_layer.load_state_dict(loop_layer.state_dict())
        params = [x] + list(loop_layer.parameters()) + list(fused_layer.parameters())

        def loop_aggregate():
            out = None
            for et in types:
                h = hg[et].send_recv(x, "mean")
                out = h if out is None else out + h
            return out

        measure(rows, "full graph: aggregate", N, d, loop_aggregate, {"fused": lambda: hg.send_recv_relations(x, "mean")}, args, params)
        measure(rows, "full graph: layer", N, d, lambda: loop_layer(hg, x),
                {"fused": lambda: fused_layer(hg, x), "fused_aggregate": lambda: fused_layer(hg, x, order="aggregate"),
                 "fused_project": lambda: fused_layer(hg, x, order="project")}, args, params)
        rows[-1]["order_none"] = rows[-2]["order_none"] = fused_layer.fused_order(args.edges, N, N)

        for n in args.seeds:
            nodes = torch.randint(0, N, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(n))
            sampler = pgl.sampling.RelationNeighborSampler(hg, [args.fanout], seed=1)
            (block, n_dst), = sampler.sample_neighbors(nodes)[0]
            n_blk = int(block.num_nodes)
            h = torch.randn(n_blk, d, generator=gen, device=dev).requires_grad_(True)
            bparams = [h] + params[1:]
            e_blk = sum(int(e) for e in block.num_edges.values())
            measure(rows, "block: layer (%d block rows, %d edges)" % (n_blk, e_blk), n, d, lambda: loop_layer(block, h)[:n_dst],
                    {"fused": lambda: fused_layer(block, h, out_size=n_dst),
                     "fused_aggregate": lambda: fused_layer(block, h, out_size=n_dst, order="aggregate"),
                     "fused_project": lambda: fused_layer(block, h, out_size=n_dst, order="project")}, args, bparams)
            rows[-1]["order_none"] = rows[-2]["order_none"] = fused_layer.fused_order(e_blk, n_dst, n_blk)
        del x

    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": args.edges, "relations": R, "fanout": args.fanout, "warmup": args.warmup,
           "reps": args.reps, "index": info, "rows": rows}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        fmt = lambda t: "%.3f (%.3f .. %.3f)" % (t["ms"], t["ms_min"], t["ms_max"])
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges in %d relations, fan-out %d; median ms of %d after %d warm-up calls (min .. max); "
                    "longest segment %d, %d rows own a segment longer than long_row = %d\n"
                    % (res["graph"], N, args.edges, R, args.fanout, args.reps, args.warmup, info["max_segment"], info["long_rows"], info["long_row"]))
            f.write("| what | size | d | mode | loop | loop again | fused | loop / fused | order=aggregate | order=project | order=None is | agree |\n"
                    "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %d | %d | %s | %s | %s | %s | %.2f | %s | %s | %s | %s |\n"
                        % (r["what"], r["size"], r["d"], r["mode"], fmt(r["loop"]), fmt(r["loop_again"]), fmt(r["fused"]), r["loop_over_fused"],
                           fmt(r["fused_aggregate"]) if "fused_aggregate" in r else "-", fmt(r["fused_project"]) if "fused_project" in r else "-",
                           r.get("order_none", "-"), "yes" if r["outputs_agree"] else "NO"))
    return res


if __name__ == "__main__":
    main()
