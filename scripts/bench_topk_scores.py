"""The fused masked top-k retrieval (pgl_amd.embedding_ops.topk_scores) beside the torch composition of the same build: matmul, indexed
-inf fill from the same exclusion pairs, topk, in user batches small enough that a [batch, N] score block fits (2^28 elements).  A timed
window is `inner` back-to-back calls between two device synchronisations, `inner` sized so that a window lasts about 50 ms; fused and
torch windows alternate; a figure is the median of --repeats windows per call and "spread" is (max - min) / median over them.  Peak
memory is that of one call of its own, above what was allocated before it.  End-to-end call times, not kernel times.  Prints one JSON
line per row; a row where the fused path loses is marked "fused_loses": true.  The last row is a ranking pass (64 queries against
2^17 entities, d = 400, k = 10, no exclusion) beside kge_scores + topk.

    python scripts/bench_topk_scores.py [--repeats 7] [--warmup 2] [--quick]"""
import argparse
import json
import math
import statistics
import time
import types

import torch

from pgl_amd import embedding_ops as E

BLOCK_ELEMS = 1 << 28


def torch_topk(query, table, k, col, per_row):
    """The composition, batch by batch: col [Q * per_row] int32 holds every query's excluded ids."""
    Q, N = query.shape[0], table.shape[0]
    B = max(1, min(Q, BLOCK_ELEMS // N))
    ids, scores = [], []
    for b0 in range(0, Q, B):
        b1 = min(Q, b0 + B)
        s = query[b0:b1] @ table.t()
        if col is not None:
            rows = torch.arange(b1 - b0, device=s.device).repeat_interleave(per_row)
            s[rows, col[b0 * per_row:b1 * per_row].long()] = -float("inf")
        top = s.topk(k, dim=1)
        ids.append(top.indices); scores.append(top.values)
    return torch.cat(ids), torch.cat(scores)


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def compare(fns, warmup, repeats):
    """{name: fn} -> {name: (median ms per call, spread, peak MiB)}; the candidates take turns, window by window."""
    peak, inner, ts = {}, {}, {k: [] for k in fns}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        inner[k] = max(1, min(50, math.ceil(50.0 / max(window(fn, 1), 1e-3))))
    for _ in range(repeats):
        for k, fn in fns.items():
            ts[k].append(window(fn, inner[k]))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v), peak[k]) for k, v in ts.items()}


def report(row, res, partner):
    for name, (ms, spread, mib) in res.items():
        row[name + "_ms"], row[name + "_spread"], row[name + "_MiB"] = round(ms, 3), round(spread, 3), round(mib, 1)
    row["fused_loses"] = res["fused"][0] > res[partner][0]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev, k, per_row = torch.device("cuda:0"), 20, 50
    for N in ((50_000,) if args.quick else (50_000, 1_000_000)):
        for Q in ((2048,) if args.quick else (2048, 16384)):
            for d in (64, 128):
                query, table = torch.randn(Q, d, device=dev) * 0.3, torch.randn(N, d, device=dev) * 0.3
                col = torch.randint(0, N, (Q, per_row), device=dev).sort(1).values.to(torch.int32).reshape(-1).contiguous()
                index = types.SimpleNamespace(indptr=torch.arange(Q + 1, device=dev) * per_row, col32=col, num_nodes=Q)
                qids = torch.arange(Q, device=dev)
                res = compare({"fused": lambda: E.topk_scores(query, table, k, exclude=index, query_ids=qids),
                               "torch": lambda: torch_topk(query, table, k, col, per_row)}, args.warmup, args.repeats)
                report({"Q": Q, "N": N, "d": d, "k": k, "excluded_per_query": per_row}, res, "torch")
    d, n, Nq = 400, 1 << 17, 64
    ent, rel = torch.randn(n, d, device=dev) * 0.3, torch.ones(1, d, device=dev)
    h, t, r = torch.randint(0, n, (Nq,), device=dev), torch.randint(0, n, (Nq,), device=dev), torch.zeros(Nq, dtype=torch.int64, device=dev)
    everyone = torch.arange(n, device=dev)[None]
    res = compare({"fused": lambda: E.topk_scores(ent[h], ent, 10),
                   "kge_scores_topk": lambda: E.kge_scores(ent, rel, h, r, t, everyone, "distmult", check_range=False)[1].reshape(Nq, n).topk(10, dim=1)},
                  args.warmup, args.repeats)
    report({"ranking": "inner product", "Q": Nq, "N": n, "d": d, "k": 10}, res, "kge_scores_topk")


if __name__ == "__main__":
    main()
