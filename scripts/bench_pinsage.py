#!/usr/bin/env python3
"""PinSAGE neighbourhoods on one MI355X: the fused launch (ops.walk_visit_topk, walk_visit.hip) next to the composition a user
had to write before it existed, on the same graph, in the same process.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator), 512 K seeds, the shapes
(num_walks, num_steps, top_k) = (10, 2, 3), (50, 5, 10), (200, 10, 50).

    fused      one launch: walk, count, select; writes S * top_k neighbours and counts.
    composed   ops.random_walk from seeds.repeat_interleave(R) (S * R * (L + 1) int64 positions written to memory), then
               torch: mask the seed and the dead steps, torch.unique(row * (N + 1) + node, return_counts=True) (a sort of
               S * R * L keys), one more sort by (row, count descending, node) and a scatter of every row's first top_k into
               the padded outputs.  It runs over --chunk seeds at a time (the walker number is offset through the seeds'
               position, see composed()): at (200, 10) x 512 K the paths of all seeds at once are 9 GB, the keys as much again.
               No host read inside.

The composed result is compared with the fused one on the first chunk before anything is timed (equal or the run stops).
Device events around every call, median of --reps after --warmup; every row also carries the minimum and the maximum.

    python scripts/bench_pinsage.py [--reps 5] [--out profiles/pinsage/bench_pinsage.txt]
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

SHAPES = [(10, 2, 3), (50, 5, 10), (200, 10, 50)]


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


def composed_chunk(csr, seeds, R, L, T, seed):
    """The visit counts of `seeds` from ops.random_walk + torch, for walkers numbered from 0 (the first chunk of a run)."""
    S, N, dev = int(seeds.shape[0]), csr.num_nodes, seeds.device
    paths, _ = pgl.ops.random_walk(csr, seeds.repeat_interleave(R), L, seed=seed, check_range=False)
    v = paths[:, 1:].reshape(S, R * L)
    v = torch.where(v == seeds[:, None], torch.full_like(v, -1), v)                     # the seed itself and the dead steps
    key = (torch.arange(S, device=dev)[:, None] * (N + 1) + (v + 1)).reshape(-1)
    uniq, count = torch.unique(key, return_counts=True)                                   # sorted by (row, node)
    row, node = uniq // (N + 1), uniq % (N + 1) - 1
    keep = node >= 0
    row, node, count = row[keep], node[keep], count[keep]
    order = torch.argsort((row * (R * L + 1) + (R * L - count)) * (N + 1) + node)       # (row, count descending, node)
    row, node, count = row[order], node[order], count[order]
    first = torch.searchsorted(row, torch.arange(S, device=dev))
    rank = torch.arange(row.shape[0], device=dev) - first[row]
    keep = rank < T
    nbr = torch.full((S, T), -1, dtype=torch.int64, device=dev)
    cnt = torch.zeros((S, T), dtype=torch.int32, device=dev)
    nbr[row[keep], rank[keep]] = node[keep]
    cnt[row[keep], rank[keep]] = count[keep].to(torch.int32)
    return nbr, cnt, (cnt > 0).sum(1).to(torch.int32)


def composed(csr, seeds, R, L, T, seed, chunk):
    """All seeds, `chunk` at a time.  (Walker numbers restart in every chunk, so the walks of later chunks differ from the
    fused call's; the work is the same.  Only the first chunk is compared.)"""
    return [composed_chunk(csr, seeds[i:i + chunk], R, L, T, seed) for i in range(0, int(seeds.shape[0]), chunk)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--seeds", type=int, default=512 * 1024)
    ap.add_argument("--chunk", type=int, default=64 * 1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    N = 1 << args.scale
    g = pgl.Graph(edges=rmat_edges(args.scale, args.edges, seed=42, device=dev), num_nodes=N).tensor()
    succ = g._csr_succ_sorted()
    seeds = torch.randint(0, N, (args.seeds,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    rows = []
    for R, L, T in SHAPES:
        head = seeds[:args.chunk]
        want = pgl.ops.walk_visit_topk(succ, head, R, L, T, seed=3, check_range=False)
        got = composed_chunk(succ, head, R, L, T, 3)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), "the composition and the fused call disagree at %s" % ((R, L, T),)
        del want, got
        f = timed(lambda: pgl.ops.walk_visit_topk(succ, seeds, R, L, T, seed=3, check_range=False), args.warmup, args.reps)
        c = timed(lambda: composed(succ, seeds, R, L, T, 3, args.chunk), args.warmup, args.reps)
        r = {"shape": [R, L, T], "seeds": args.seeds, "steps": args.seeds * R * L, "fused_ms": round(f[0], 3),
             "fused_min_max": [round(f[1], 3), round(f[2], 3)], "composed_ms": round(c[0], 3),
             "composed_min_max": [round(c[1], 3), round(c[2], 3)], "composed_over_fused": round(c[0] / f[0], 2),
             "path_bytes": args.seeds * R * (L + 1) * 8}
        rows.append(r)
        print(json.dumps(r), flush=True)

    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": g.num_edges, "chunk": args.chunk, "warmup": args.warmup,
           "reps": args.reps, "rows": rows}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("%s: %d nodes, %d edges, %d seeds (composition: %d seeds at a time); median of %d after %d warm-up calls, device events\n"
                     % (res["graph"], N, g.num_edges, args.seeds, args.chunk, args.reps, args.warmup))
            fh.write("| (R, L, T) | steps | fused ms (min .. max) | composed ms (min .. max) | composed / fused | paths the composition writes |\n")
            fh.write("|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %s | %.2e | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f | %.2f GB |\n"
                         % (tuple(r["shape"]), r["steps"], r["fused_ms"], r["fused_min_max"][0], r["fused_min_max"][1], r["composed_ms"],
                            r["composed_min_max"][0], r["composed_min_max"][1], r["composed_over_fused"], r["path_bytes"] / 1e9))
    return res


if __name__ == "__main__":
    main()
