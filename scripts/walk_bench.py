#!/usr/bin/env python3
"""Random-walk and skip-gram throughput on the MI355X (walk.hip).

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator), 1 M walkers:
uniform 80 steps, node2vec (p, q) = (0.25, 4) and (4, 0.25) at 80 steps, node2vec-plus (0.25, 4) at 40 steps, then the
skip-gram pairs (win_size 5) of the uniform walks.  Times are device events over --reps runs after --warmup runs; steps/s
counts the steps actually taken (sum of lengths - walkers).  The host twin's single-thread steps/s is measured on
--host-walkers walkers of the same configuration.  node2vec's mean trials per step is estimated on the host twin by counting
its expected rejection trials along a sample of the host twin's walks (walk_core.hpp's acceptance thresholds).

    python scripts/walk_bench.py [--walkers 1048576] [--reps 5]
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
    return float(np.median(ms)), out


def mean_trials(indptr, col, paths, p, q, plus, max_trials=64):
    """Expected rejection trials per second-order step, exactly, along the given walks: at cur with predecessor prev the
    acceptance probability of one trial is a = mean over succ(cur) of thr[class] / 2^32, and the trials made are min(T, max_trials)
    with T geometric: E = (1 - (1 - a)^max_trials) / a."""
    _, thr = pgl.ops.walk_params(p, q, plus)
    thr = np.asarray(thr, np.float64) / 2.0 ** 32
    out = []
    for row in paths:
        for t in range(1, len(row) - 1):
            cur, prev = row[t], row[t - 1]
            if cur < 0 or indptr[cur + 1] == indptr[cur]:
                break
            cand = col[indptr[cur]:indptr[cur + 1]]
            hist = row[:t] if plus else row[t - 1:t]
            seen = np.concatenate([col[indptr[v]:indptr[v + 1]] for v in hist])
            cls = np.where(cand == prev, 0, np.where(np.isin(cand, seen), 1, 2))
            a = float(thr[cls].mean())
            out.append((1.0 - (1.0 - a) ** max_trials) / a)
    return float(np.mean(out)) if out else 0.0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--walkers", type=int, default=1 << 20)
    ap.add_argument("--host-walkers", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    e = rmat_edges(args.scale, args.edges, seed=42, device=dev)
    g = pgl.Graph(edges=e, num_nodes=1 << args.scale).tensor()
    csr = g._csr_succ_sorted()
    torch.cuda.synchronize()
    indptr, col = csr.indptr.cpu().numpy(), csr.col32.cpu().numpy()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    starts = torch.randint(0, g.num_nodes, (args.walkers,), device=dev, generator=gen)
    hstarts = starts[:args.host_walkers].cpu().numpy()
    res = {"graph": "rmat%d" % args.scale, "nodes": g.num_nodes, "edges": g.num_edges, "walkers": args.walkers, "configs": []}
    uniform = None
    for name, p, q, plus, steps in (("uniform", 1.0, 1.0, False, 80), ("node2vec(0.25,4)", 0.25, 4.0, False, 80),
                                    ("node2vec(4,0.25)", 4.0, 0.25, False, 80), ("plus(0.25,4)", 0.25, 4.0, True, 40)):
        ms, (paths, lengths) = timed(lambda: pgl.ops.random_walk(csr, starts, steps, p, q, plus, seed=7, check_range=False),
                                     args.warmup, args.reps)
        taken = int((lengths - 1).sum())
        t = time.perf_counter()
        hp, hl = pgl.ops.host_random_walk(indptr, col, hstarts, steps, p, q, plus, seed=7, threads=1)
        host_s = time.perf_counter() - t
        row = {"config": name, "steps": steps, "ms": round(ms, 3), "steps_taken": taken,
               "G_steps_per_s": round(taken / ms / 1e6, 3), "mean_length": round(float(lengths.double().mean()), 2),
               "host_1thread_M_steps_per_s": round(float((hl - 1).sum()) / host_s / 1e6, 3)}
        if plus or p != 1.0 or q != 1.0:
            row["mean_trials_per_step"] = round(mean_trials(indptr, col, hp[:500], p, q, plus, pgl.ops.default_max_trials(p, q)), 3)
        res["configs"].append(row)
        print(json.dumps(row), flush=True)
        if name == "uniform":
            uniform = (paths, lengths)
        else:
            del paths, lengths
    ms, (src, dst) = timed(lambda: pgl.ops.skip_gram_pairs(uniform[0], uniform[1], 5, seed=3), args.warmup, args.reps)
    row = {"config": "skip_gram(win=5) of the uniform walks", "ms": round(ms, 3), "pairs": int(src.shape[0]),
           "G_pairs_per_s": round(int(src.shape[0]) / ms / 1e6, 3)}
    res["configs"].append(row)
    print(json.dumps(row), flush=True)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
