#!/usr/bin/env python3
"""Checked negative sampling on one MI355X (negative.hip) next to three yardsticks of the same build.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator).

    negatives  ops.sample_negatives, check=False (one launch, no host read): 1 M sources x 5 negatives (a skip-gram / BPR step)
               and 512 sources x 256 negatives (the knowledge-graph shape), uniform and with outdegree ** 0.75 noise.
    randint    torch.randint of the same shape: these "negatives" are unchecked, so this is the floor.
    host twin  ops.host_sample_negatives on ONE thread (host clock; --host_rows sources of the first shape, scaled to the
               whole shape in the ratio).
    walk       ops.random_walk, 1 M walkers x 80 uniform steps: 80 dependent row reads per lane, the known yardstick.

Device events around every call, median of --reps after --warmup; every row also carries the minimum and the maximum.  Nothing
here has a predecessor to beat: the times are reported, not gated.

    python scripts/bench_negatives.py [--reps 7] [--out profiles/negatives/bench_negatives.txt]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--host_rows", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    N = 1 << args.scale
    g = pgl.Graph(edges=rmat_edges(args.scale, args.edges, seed=42, device=dev), num_nodes=N).tensor()
    succ = g._csr_succ_sorted()
    noise = pgl.ops.weight_table(g.outdegree().to(torch.float64) ** 0.75)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []

    def row(name, what, t, base=None, base_name=None):
        r = {"op": name, "case": what, "ms": round(t[0], 3), "ms_min_max": [round(t[1], 3), round(t[2], 3)]}
        if base is not None:
            r["ratio_to_" + base_name] = round(t[0] / base, 2)
        rows.append(r)
        print(json.dumps(r), flush=True)

    starts = torch.randint(0, N, (args.walkers,), device=dev, generator=gen)
    walk = timed(lambda: pgl.ops.random_walk(succ, starts, args.steps, seed=1, check_range=False), args.warmup, args.reps)
    row("random_walk", "%d walkers x %d uniform steps" % (args.walkers, args.steps), walk)

    for n, K in ((1_000_000, 5), (512, 256)):
        src = torch.randint(0, N, (n,), device=dev, generator=gen)
        floor = timed(lambda: torch.randint(0, N, (n, K), device=dev), args.warmup, args.reps)
        row("torch.randint", "%d x %d, unchecked" % (n, K), floor)
        for what, kw in (("uniform", {}), ("outdegree ** 0.75 noise", {"noise": noise})):
            t = timed(lambda: pgl.ops.sample_negatives(succ, src, K, seed=3, check=False, **kw), args.warmup, args.reps)
            neg = t[3]
            hit = int((neg < 0).sum())
            row("sample_negatives", "%d sources x %d, %s (%d of %d without a negative)" % (n, K, what, hit, neg.numel()), t, floor[0], "randint")
            rows[-1]["ratio_to_walk"] = round(t[0] / walk[0], 4)
        if n >= args.host_rows:
            indptr, col, h_src = succ.indptr.cpu().numpy(), succ.col32.cpu().numpy(), src[:args.host_rows].cpu().numpy()
            t0 = time.perf_counter()
            twin = pgl.ops.host_sample_negatives(indptr, col, h_src, K, seed=3, threads=1)
            ms = (time.perf_counter() - t0) * 1e3
            same = bool(np.array_equal(twin, pgl.ops.sample_negatives(succ, src[:args.host_rows], K, seed=3, check=False).cpu().numpy()))
            r = {"op": "host_sample_negatives", "case": "%d sources x %d, uniform, 1 thread, host clock (equal to the device: %s)" % (args.host_rows, K, same),
                 "ms": round(ms, 3), "ms_for_the_whole_shape": round(ms * n / args.host_rows, 1)}
            rows.append(r)
            print(json.dumps(r), flush=True)

    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": g.num_edges, "warmup": args.warmup, "reps": args.reps, "rows": rows}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges; median of %d after %d warm-up calls, device events\n" % (res["graph"], N, g.num_edges, args.reps, args.warmup))
            f.write("| op | case | ms (min .. max) | x randint | x walk |\n|---|---|---|---|---|\n")
            for r in rows:
                mm = r.get("ms_min_max")
                f.write("| %s | %s | %.3f%s | %s | %s |\n" % (r["op"], r["case"], r["ms"], " (%.3f .. %.3f)" % tuple(mm) if mm else "",
                                                              r.get("ratio_to_randint", "-"), r.get("ratio_to_walk", "-")))
    return res


if __name__ == "__main__":
    main()
