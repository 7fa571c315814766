#!/usr/bin/env python3
"""Metapath walks on one MI355X (pglamd_metapath_walk, the relation-stacked mode of walk.hip) next to the uniform walk of the same
build.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator), cut into --relations equal
slices of consecutive edges: every slice is one relation of a HeterGraph over the same 2^20 nodes, the whole list is the union
graph.

    uniform      ops.random_walk over the union graph, 1 M walkers x 80 steps
    metapath R=1 ops.metapath_walk over the union graph stacked as ONE relation, metapath [0]: the same walks bit for bit, so the
                 difference to `uniform` is what the per-position relation look-up costs and nothing else
    metapath R x union  the union graph stacked R times, metapath 0-1-..-(R-1): every relation has the same rows, so these are the
                 same walks again, read through an indptr R times as large (and R copies of col): what the larger footprint costs
    metapath     ops.metapath_walk over the stacked relations with the metapath 0-1-..-(R-1): the same two dependent reads per step
                 over an indptr R times as large.  A walk that changes relation at every step meets dead ends a union walk does
                 not (a node's successors under ONE relation), so the rows also carry the mean walk length and the time per
                 step actually taken

Device events around every call, median of --reps after --warmup; every row also carries the minimum and the maximum.

    python scripts/bench_metapath.py [--reps 7] [--out profiles/metapath/bench_metapath.txt]
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
    ap.add_argument("--relations", type=int, default=4)
    ap.add_argument("--walkers", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    N, R = 1 << args.scale, args.relations
    edges = rmat_edges(args.scale, args.edges, seed=42, device=dev)
    union = pgl.Graph(edges=edges, num_nodes=N).tensor()
    cut = [args.edges * r // R for r in range(R + 1)]
    hg = pgl.HeterGraph(edges={"r%d" % r: edges[cut[r]:cut[r + 1]] for r in range(R)}, num_nodes=N)
    assert hg.is_tensor()
    stacked = hg._stacked_succ()[0]
    succ = union._csr_succ_sorted()
    one = pgl.ops.stack_relations([succ])
    starts = torch.randint(0, N, (args.walkers,), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    rows = []

    def row(name, what, t, base=None):
        mean_len = float(t[3][1].double().mean())
        taken = float((t[3][1] - 1).sum())
        r = {"op": name, "case": what, "ms": round(t[0], 3), "ms_min_max": [round(t[1], 3), round(t[2], 3)], "mean_length": round(mean_len, 2),
             "ns_per_step_taken": round(t[0] * 1e6 / max(taken, 1.0), 3)}
        if base is not None:
            r["uniform_ms"] = round(base[0], 3)
            r["ratio"] = round(t[0] / base[0], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)

    what = "%d walkers x %d steps" % (args.walkers, args.steps)
    base = timed(lambda: pgl.ops.random_walk(succ, starts, args.steps, seed=1, check_range=False), args.warmup, args.reps)
    row("random_walk", "union graph, %s" % what, base)
    t1 = timed(lambda: pgl.ops.metapath_walk(one, starts, [0], args.steps, seed=1, check_range=False), args.warmup, args.reps)
    assert torch.equal(t1[3][0], base[3][0]) and torch.equal(t1[3][1], base[3][1])
    row("metapath_walk", "union graph as one relation, metapath [0], %s (the same walks)" % what, t1, base)
    many = pgl.ops.stack_relations([succ] * R)
    tr = timed(lambda: pgl.ops.metapath_walk(many, starts, list(range(R)), args.steps, seed=1, check_range=False), args.warmup, args.reps)
    assert torch.equal(tr[3][0], base[3][0]) and torch.equal(tr[3][1], base[3][1])
    row("metapath_walk", "union graph stacked %d times, metapath %s, %s (the same walks)" % (R, "-".join(map(str, range(R))), what), tr, base)
    del many
    t = timed(lambda: pgl.ops.metapath_walk(stacked, starts, list(range(R)), args.steps, seed=1, check_range=False), args.warmup, args.reps)
    row("metapath_walk", "%d relations of %d edges, metapath %s, %s" % (R, args.edges // R, "-".join(map(str, range(R))), what), t, base)

    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": args.edges, "relations": R, "warmup": args.warmup, "reps": args.reps, "rows": rows}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges in %d relations; median of %d after %d warm-up calls, device events\n"
                    % (res["graph"], N, args.edges, R, args.reps, args.warmup))
            f.write("| op | case | ms (min .. max) | mean walk length | ns per step taken | uniform ms | ratio |\n|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %s | %.3f (%.3f .. %.3f) | %.2f | %.3f | %s | %s |\n"
                        % (r["op"], r["case"], r["ms"], r["ms_min_max"][0], r["ms_min_max"][1], r["mean_length"], r["ns_per_step_taken"],
                           r.get("uniform_ms", "-"), r.get("ratio", "-")))
    return res


if __name__ == "__main__":
    main()
