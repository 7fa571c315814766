#!/usr/bin/env python3
"""One layer of relation-wise neighbour sampling on one MI355X: the fused path (ops.sample_neighbors_relations over the stacked
predecessor index, then one relabel) next to the composition of the ops this build had before it.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator), cut into --relations equal slices
of consecutive edges: every slice is one relation of a HeterGraph over the same 2^20 nodes.  Fan-out --fanout per relation; seeds
drawn uniformly, --seeds of them per batch (512: a training batch, where launch latency and host reads are the whole cost;
524288: a frontier of a later layer, where the kernels are).

    composed  per relation ops.sample_neighbors(csr_r, nodes, fanout, seed=relation_seed(seed, r)) -- two launches, a scan and a
              host read each -- then torch.cat and ops.reindex_graph over the concatenation.  reindex_graph's own dst (ONE
              repeat_interleave over the summed counts) stands for the R a loop would need, so this side is charged less than
              the hand-written loop costs.
    fused     ops.sample_neighbors_relations (one count launch, one scan, one fill launch that also writes dst, one host read) and
              the same relabel (pglamd_reindex) over its flat output.

Both return the same neighbours and the same relabelled sources (asserted).  Every call ends in a host read, so the device events
around it and a host clock around call + synchronise measure the same thing; both are reported: median of --reps after --warmup,
with the minimum and the maximum.

    python scripts/bench_hetero_sampling.py [--reps 30] [--out profiles/hetero_sampling/bench_hetero_sampling.txt]
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
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(a.elapsed_time(b))
    return dict(ms=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)), wall_ms=float(np.median(wall))), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--relations", type=int, default=4)
    ap.add_argument("--fanout", type=int, default=10)
    ap.add_argument("--seeds", type=int, nargs="+", default=[512, 512 * 1024])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    N, R, ops = 1 << args.scale, args.relations, pgl.ops
    edges = rmat_edges(args.scale, args.edges, seed=42, device=dev)
    cut = [args.edges * r // R for r in range(R + 1)]
    hg = pgl.HeterGraph(edges={"r%d" % r: edges[cut[r]:cut[r + 1]] for r in range(R)}, num_nodes=N)
    assert hg.is_tensor()
    stacked = hg._stacked_pred()[0]
    csrs = [hg[et].adj_dst_index.csr for et in hg.edge_types]
    fan = [args.fanout] * R
    rows = []

    for n in args.seeds:
        nodes = torch.randint(0, N, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(n))

        def composed(relabel):
            parts = [ops.sample_neighbors(c, nodes, args.fanout, seed=ops.relation_seed(1, r), check_range=False) for r, c in enumerate(csrs)]
            nbr = torch.cat([p[0] for p in parts])
            if not relabel:
                return nbr, None
            src, _, out_nodes = ops.reindex_graph(nodes, nbr, torch.stack([p[1] for p in parts]).sum(0), check_range=False)
            return nbr, (src, out_nodes)

        def fused(relabel):
            s = ops.sample_neighbors_relations(stacked, nodes, fan, seed=1, check_range=False)
            return s.neighbors, (ops._relabel(nodes, s.neighbors) if relabel else None)

        for relabel in (False, True):
            tc, oc = timed(lambda: composed(relabel), args.warmup, args.reps)
            tf, of = timed(lambda: fused(relabel), args.warmup, args.reps)
            assert torch.equal(oc[0], of[0])
            if relabel:
                assert torch.equal(oc[1][0], of[1][0]) and torch.equal(oc[1][1], of[1][1])
            r = {"seeds": n, "what": "sample + relabel" if relabel else "sample", "sampled_edges": int(of[0].shape[0]),
                 "composed": {k: round(v, 4) for k, v in tc.items()}, "fused": {k: round(v, 4) for k, v in tf.items()},
                 "ratio_composed_over_fused": round(tc["ms"] / tf["ms"], 3)}
            rows.append(r)
            print(json.dumps(r), flush=True)

    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": args.edges, "relations": R, "fanout": args.fanout, "warmup": args.warmup,
           "reps": args.reps, "rows": rows}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges in %d relations, fan-out %d per relation; median of %d after %d warm-up calls\n"
                    % (res["graph"], N, args.edges, R, args.fanout, args.reps, args.warmup))
            f.write("| seeds | what | sampled edges | composed ms (min .. max; host clock) | fused ms (min .. max; host clock) | composed / fused |\n"
                    "|---|---|---|---|---|---|\n")
            for r in rows:
                c, u = r["composed"], r["fused"]
                f.write("| %d | %s | %d | %.3f (%.3f .. %.3f; %.3f) | %.3f (%.3f .. %.3f; %.3f) | %.2f |\n"
                        % (r["seeds"], r["what"], r["sampled_edges"], c["ms"], c["ms_min"], c["ms_max"], c["wall_ms"], u["ms"], u["ms_min"],
                           u["ms_max"], u["wall_ms"], r["ratio_composed_over_fused"]))
    return res


if __name__ == "__main__":
    main()
