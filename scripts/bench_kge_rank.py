"""The fused link-prediction ranks (pgl_amd.embedding_ops.kge_ranks) beside the route the parent commit offers: kge_scores against one
chunk holding every entity (a [Q, Ne] fp32 tensor), then a torch comparison with the true entity's score -- which cannot filter.  Rows:
Q = 64 / 1024 / 8192 test triples, Ne = 2^17 / 2^20 entities, d = 200 / 400, all four models, with a filter of about 50 ids per query and
without one (the score-block route is the same unfiltered call in both).  A timed window is `inner` back-to-back calls between two
device synchronisations, `inner` sized so that a window lasts about 50 ms; fused and score-block windows alternate; a figure is the
median of --repeats windows per call and "spread" is (max - min) / median over them.  Peak memory is that of one call of its own, above
what was allocated before it.  End-to-end call times, not kernel times.  Prints one JSON line per row; a row where the fused path loses
is marked "fused_loses": true.  --slices S adds the fused time with S forced (the slice rule's constants come from such rows).

    python scripts/bench_kge_rank.py [--repeats 5] [--warmup 1] [--quick] [--max_pairs N] [--slices S ...]"""
import argparse
import json
import math
import statistics
import time
import types

import torch

from pgl_amd import embedding_ops as E


def score_block(ent, rel, h, r, t, everyone, model, gamma):
    _, s = E.kge_scores(ent, rel, h, r, t, everyone, model, gamma=gamma, check_range=False)
    s = s[0]
    return (s > s.gather(1, t[:, None])).sum(1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--quick", action="store_true", help="Q = 64 / 1024, Ne = 2^17, d = 200")
    ap.add_argument("--max_pairs", type=int, default=0, help="skip rows with more than this many (query, entity) pairs (0: none)")
    ap.add_argument("--slices", type=int, nargs="*", default=[], help="also time the fused call with these slice counts forced")
    args = ap.parse_args()
    dev, Nr, gamma, per_row = torch.device("cuda:0"), 64, 12.0, 50
    for Ne in ((1 << 17,) if args.quick else (1 << 17, 1 << 20)):
        for d in ((200,) if args.quick else (200, 400)):
            ent = torch.randn(Ne, d, device=dev) * 0.3
            everyone = torch.arange(Ne, device=dev)[None]
            for Q in ((64, 1024) if args.quick else (64, 1024, 8192)):
                if args.max_pairs and Q * Ne > args.max_pairs:
                    print(json.dumps({"Q": Q, "Ne": Ne, "d": d, "skipped": "more than --max_pairs pairs"}), flush=True)
                    continue
                h, t, r = (torch.randint(0, m, (Q,), device=dev) for m in (Ne, Ne, Nr))
                col = torch.randint(0, Ne, (Q, per_row), device=dev).sort(1).values.to(torch.int32).reshape(-1).contiguous()
                index = types.SimpleNamespace(indptr=torch.arange(Q + 1, device=dev) * per_row, col32=col)
                frows = torch.arange(Q, device=dev)
                for model in ("transe", "distmult", "complex", "rotate"):
                    rel = torch.randn(Nr, d // 2 if model == "rotate" else d, device=dev) * 0.3
                    run = lambda **kw: E.kge_ranks(ent, rel, h, r, t, model, gamma=gamma, check_range=False, **kw)
                    fns = {"fused": run, "fused_filtered": lambda: run(filter=index, filter_rows=frows),
                           "score_block": lambda: score_block(ent, rel, h, r, t, everyone, model, gamma)}
                    fns.update({"fused_S%d" % s: (lambda s=s: run(slices=s)) for s in args.slices})
                    res = compare(fns, args.warmup, args.repeats)
                    row = {"model": model, "Q": Q, "Ne": Ne, "d": d, "slices": int(E._ffi.lib().pglamd_kge_rank_slices(Q, Ne))}
                    for name, (ms, spread, mib) in res.items():
                        row[name + "_ms"], row[name + "_spread"], row[name + "_MiB"] = round(ms, 3), round(spread, 3), round(mib, 1)
                    row["fused_loses"] = max(res["fused"][0], res["fused_filtered"][0]) > res["score_block"][0]
                    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
