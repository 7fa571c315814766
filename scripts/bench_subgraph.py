#!/usr/bin/env python3
"""Induced-subgraph extraction on one MI355X (subgraph.hip) next to the three other ways to get the same batch.

RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42: the bench workload's generator), cut into 256 clusters
(N / 4096) by pgl.partition.random_partition and by the engine's partitioner (the clustering Graph.reorder computes); batches
of 1, 8 and 64 clusters = 1/256, 1/32 and 1/4 of the nodes, drawn by sampling.ClusterBatches (seed 0, first batch).

    new   ops.induced_subgraph on the device index: mark + scan + count + scan, ONE host read, fill.  Device events around the
          whole call (the host read is inside), median of --reps after --warmup.
    (a)   the host twin (pglamd_induced_subgraph_host), one thread, on the numpy copy of the same index.  Host clock.
    (b)   what a user has without this feature: Graph.numpy() -> the edge ids by a table mask over the edge list ->
          sampling.subgraph -> .tensor() -> adj_dst_index (the radix sort).  Host clock around work that ends in a device
          synchronise; the Graph.numpy() copy of the whole graph is timed once and reported apart (a loop can keep it).
    (c)   torch only, on the device, over ALL E edges: table lookup of both endpoints, mask, nonzero, stable sort by
          destination.  Device events, same reps.  Its result is compared with the kernels' (it must be equal).

Reported per row: the times, sum deg(nodes) (the candidate positions), the kept edges and the bytes the kernels have to move
(min_bytes below: counted from the shapes, not measured).  --out writes the table as text.

    python scripts/bench_subgraph.py [--reps 7] [--out profiles/subgraph/bench_subgraph.txt]
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


def host_timed(fn, reps):
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), out


def min_bytes(N, n, S, kept):
    """Bytes the new path has to move, from the shapes: the table memset (4 N); mark reads the ids and two indptr entries and
    writes a table slot and a degree (8 + 16 + 4 + 8 per node); the row-start scan reads and writes 8 per node; count and fill
    each read a column entry and a table slot per candidate position (2 x 8 S); fill reads an edge id and writes three int64
    per kept edge (4 + 24)."""
    return 4 * N + 36 * n + 16 * n + 16 * S + 28 * kept


def torch_only(table, edges, nodes):
    table.fill_(-1)
    table[nodes] = torch.arange(nodes.shape[0], device=nodes.device)
    s, d = table[edges[:, 0]], table[edges[:, 1]]
    idx = torch.nonzero((s >= 0) & (d >= 0)).reshape(-1)
    dst, order = torch.sort(d[idx], stable=True)
    return s[idx][order], dst, idx[order]


def parent_path(g_np, keep_table, nodes_np):
    e = g_np.edges
    keep_table[:] = False
    keep_table[nodes_np] = True
    eids = np.flatnonzero(keep_table[e[:, 0]] & keep_table[e[:, 1]])
    sub = pgl.sampling.subgraph(g_np, nodes_np, eid=eids).tensor()
    sub.adj_dst_index
    return sub


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--clusters", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    N = 1 << args.scale
    g = pgl.Graph(edges=rmat_edges(args.scale, args.edges, seed=42, device=dev), num_nodes=N).tensor()
    csr = g.adj_dst_index.csr
    torch.cuda.synchronize()
    t = time.perf_counter()
    g_np = g.numpy(inplace=False)
    numpy_copy_ms = (time.perf_counter() - t) * 1e3
    ix = g_np.adj_dst_index
    e_np = g_np.edges
    np.random.seed(0)
    parts = {"random_partition": pgl.partition.random_partition(g_np, args.clusters)}
    parts["engine partitioner"], _ = pgl.ops.host_partition_edges(e_np, N, args.clusters, None, None, 1.10, 1.10, 0)
    table = torch.empty(N, dtype=torch.int64, device=dev)
    keep_table = np.zeros(N, bool)
    res = {"graph": "rmat%d" % args.scale, "nodes": N, "edges": g.num_edges, "clusters": args.clusters,
           "graph_numpy_copy_ms": round(numpy_copy_ms, 1), "rows": []}
    for pname, part in parts.items():
        for per in (1, 8, 64):
            nodes = next(iter(pgl.sampling.ClusterBatches(g, part, clusters_per_batch=per, seed=0)))[1]
            nodes_np = nodes.cpu().numpy()
            ms, lo, hi, (src, dst, eids) = timed(lambda: pgl.ops.induced_subgraph(csr, nodes), args.warmup, args.reps)
            S, kept = int(csr.degree[nodes].sum()), int(eids.shape[0])
            c_ms, _, _, (cs, cd, ce) = timed(lambda: torch_only(table, g.edges, nodes), args.warmup, args.reps)
            same = bool(torch.equal(cs, src) and torch.equal(cd, dst) and torch.equal(ce, eids))
            del cs, cd, ce
            a_ms, ha = host_timed(lambda: pgl.ops.host_induced_subgraph(ix._indptr, ix._sorted_v, ix._sorted_eid, nodes_np, N), 3)
            assert np.array_equal(ha[2], eids.cpu().numpy())
            b_ms, sub = host_timed(lambda: parent_path(g_np, keep_table, nodes_np), 1)
            assert sub.num_edges == kept
            mb = min_bytes(N, len(nodes_np), S, kept)
            row = {"partition": pname, "batch": "1/%d" % (args.clusters // per), "nodes": len(nodes_np), "sum_deg": S, "kept": kept,
                   "new_ms": round(ms, 3), "new_ms_min_max": [round(lo, 3), round(hi, 3)], "min_MB": round(mb / 1e6, 2),
                   "GB_per_s_of_min_bytes": round(mb / ms / 1e6, 1), "host_twin_1thread_ms": round(a_ms, 2),
                   "parent_path_ms": round(b_ms, 1), "torch_only_ms": round(c_ms, 3), "torch_only_equal": same}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("%s: %d nodes, %d edges, %d clusters; Graph.numpy() copy of the whole graph %.0f ms (not in (b))\n"
                    % (res["graph"], N, g.num_edges, args.clusters, numpy_copy_ms))
            f.write("| partition | batch | nodes | sum deg | kept | new ms (min .. max) | min MB | GB/s | (a) host twin ms | (b) parent path ms | (c) torch only ms | (c) == new |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in res["rows"]:
                f.write("| %s | %s | %d | %d | %d | %.3f (%.3f .. %.3f) | %.1f | %.0f | %.2f | %.0f | %.3f | %s |\n"
                        % (r["partition"], r["batch"], r["nodes"], r["sum_deg"], r["kept"], r["new_ms"], r["new_ms_min_max"][0],
                           r["new_ms_min_max"][1], r["min_MB"], r["GB_per_s_of_min_bytes"], r["host_twin_1thread_ms"],
                           r["parent_path_ms"], r["torch_only_ms"], r["torch_only_equal"]))
    return res


if __name__ == "__main__":
    main()
