#!/usr/bin/env python3
"""Edge-weighted sampling on one MI355X (weighted.hip, the weighted mode of walk.hip) next to the uniform samplers of the same
build.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator), one fp32 weight per edge
(exponential, 10 % zeros, seed 0).

    table    ops.edge_weight_table over the sorted successor index and over the dst index (row maximum, int64 scan, finish).
    walk     1 M walkers x 80 steps: ops.random_walk with weights= next to the uniform walk.  The weighted step adds one
             dependent binary search of the row's prefix sums (about log2(deg) reads of cum) to the uniform step's two reads.
    sample   512 K seed nodes, fan-out 25 and 10: ops.sample_neighbors with weights= next to the uniform (Floyd) sampler.
             Both read their total back between count and fill; the time is of the whole call.

Device events around every call, median of --reps after --warmup; every row also carries the minimum and the maximum.

    python scripts/bench_weighted.py [--reps 7] [--out profiles/weighted/bench_weighted.txt]
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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms)), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--walkers", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--seeds", type=int, default=512 * 1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    N = 1 << args.scale
    g = pgl.Graph(edges=rmat_edges(args.scale, args.edges, seed=42, device=dev), num_nodes=N).tensor()
    rng = np.random.default_rng(0)
    w = rng.exponential(size=g.num_edges).astype(np.float32)
    w[rng.random(g.num_edges) < 0.1] = 0
    w = torch.from_numpy(w).to(dev)
    succ, dst = g._csr_succ_sorted(), g.adj_dst_index.csr
    succ_eid = g._succ_edge_ids()
    rows = []

    def row(name, what, t, base=None):
        r = {"op": name, "case": what, "ms": round(t[0], 3), "ms_min_max": [round(t[1], 3), round(t[2], 3)]}
        if base is not None:
            r["uniform_ms"] = round(base[0], 3)
            r["ratio"] = round(t[0] / base[0], 2)
        rows.append(r)
        print(json.dumps(r), flush=True)

    t = timed(lambda: pgl.ops.edge_weight_table(succ, w, succ_eid), args.warmup, args.reps)
    row("edge_weight_table", "successor index, %d edges" % g.num_edges, t)
    t = timed(lambda: pgl.ops.edge_weight_table(dst, w, dst.eid32), args.warmup, args.reps)
    row("edge_weight_table", "dst index, %d edges" % g.num_edges, t)
    tw, td = g.edge_weight_table(w, "succ"), g.edge_weight_table(w, "dst")

    starts = torch.randint(0, N, (args.walkers,), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    base = timed(lambda: pgl.ops.random_walk(succ, starts, args.steps, seed=1, check_range=False), args.warmup, args.reps)
    t = timed(lambda: pgl.ops.random_walk(succ, starts, args.steps, seed=1, check_range=False, weights=tw), args.warmup, args.reps)
    lw, lu = float(t[3][1].double().mean()), float(base[3][1].double().mean())
    row("random_walk", "%d walkers x %d steps (mean length weighted %.1f, uniform %.1f)" % (args.walkers, args.steps, lw, lu), t, base)

    seeds = torch.randint(0, N, (args.seeds,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for k in (25, 10):
        base = timed(lambda: pgl.ops.sample_neighbors(dst, seeds, k, seed=2, check_range=False), args.warmup, args.reps)
        t = timed(lambda: pgl.ops.sample_neighbors(dst, seeds, k, seed=2, check_range=False, weights=td), args.warmup, args.reps)
        row("sample_neighbors", "%d seeds, fan-out %d (%d / %d neighbours)" % (args.seeds, k, t[3][0].numel(), base[3][0].numel()), t, base)

    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": g.num_edges, "warmup": args.warmup, "reps": args.reps, "rows": rows}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges; median of %d after %d warm-up calls, device events\n" % (res["graph"], N, g.num_edges, args.reps, args.warmup))
            f.write("| op | case | weighted ms (min .. max) | uniform ms | ratio |\n|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %s | %.3f (%.3f .. %.3f) | %s | %s |\n" % (r["op"], r["case"], r["ms"], r["ms_min_max"][0], r["ms_min_max"][1],
                                                                         r.get("uniform_ms", "-"), r.get("ratio", "-")))
    return res


if __name__ == "__main__":
    main()
