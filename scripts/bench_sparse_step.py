#!/usr/bin/env python3
"""The sparse embedding step (csrc/sparse_step.hip; pgl_amd.nn.functional.skip_gram_step / kge_step / sparse_step) on one MI355X next to
what the examples ran before it, on the same build, the same tables and the same ids, in the same process.

  step    fused route: skip_gram_step (fused loss + sparse step, lazy Adam)        comparison: skip_gram_loss + backward +
          torch.optim.Adam over both whole tables.  Two tables of N rows, d = 128, P pairs, K = 5, uniform ids.
  kge     kge_step (TransE, lazy Adam) against kge_loss + backward + torch.optim.Adam: P = 1024 in 8 chunks, neg = 256, d = 400,
          2^20 entities, 1024 relations.
  op      sparse_step alone (explicit rows [M, d], M = P (2 + K) entries, the sort included) against torch.optim.SparseAdam / Adagrad
          fed the same gradient as a coalesced sparse tensor (the coalescing is not timed: it is given to torch for free).

Device events around every call, median of --reps after --warmup, minimum and maximum next to it.  Peak memory:
torch.cuda.max_memory_allocated over one call, above what is allocated before it (tables, optimiser state, ids).  The two routes of a
row are different optimisers (lazy against dense Adam), so only time and memory are compared here, not the tables.

    python scripts/bench_sparse_step.py [--reps 5] [--rows 20 24] [--out profiles/sparse_step/bench_sparse_step.md]
"""
import argparse
import gc
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd.nn.functional as PF  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms)), peak


def row(name, shape, fused, other):
    mark = "" if fused[0] <= other[0] else " **loses**"
    return "| %s | %s | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.2fx%s | %.0f | %.0f |" % (
        name, shape, *fused[:3], *other[:3], other[0] / fused[0], mark, fused[3], other[3])


def dense_adam(loss_fn, params):
    opt = torch.optim.Adam(params, lr=0.025)

    def step():
        opt.zero_grad(set_to_none=True)
        loss_fn().backward()
        opt.step()
    return step


def bench_step(lgN, lgP, K, d, a):
    N, P, dev = 1 << lgN, 1 << lgP, torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    src, dst = (torch.randint(0, N, (P,), device=dev, generator=gen) for _ in range(2))
    neg = torch.randint(0, N, (P, K), device=dev, generator=gen)
    out = []
    emb, ctx = (torch.nn.Parameter(torch.randn(N, d, device=dev) * 0.1) for _ in range(2))
    states = [PF.SparseState(w, "lazy_adam", 0.025) for w in (emb, ctx)]
    fused = timed(lambda: PF.skip_gram_step(emb, ctx, src, dst, neg, *states), a.warmup, a.reps)
    del states
    other = timed(dense_adam(lambda: PF.skip_gram_loss(emb, ctx, src, dst, neg), [emb, ctx]), a.warmup, a.reps)
    out.append(row("step: skip_gram_step / loss + backward + dense Adam", "N = 2^%d, P = 2^%d, K = %d, d = %d" % (lgN, lgP, K, d), fused, other))
    # the op alone: M entries with explicit rows against torch's sparse optimisers on the coalesced gradient
    ids = torch.cat([src, dst, neg.reshape(-1)])
    rows = torch.randn(ids.shape[0], d, device=dev) * 0.01
    for kind, topt in (("lazy_adam", torch.optim.SparseAdam), ("adagrad", torch.optim.Adagrad)):
        gc.collect()
        torch.cuda.empty_cache()
        state = PF.SparseState(emb, kind, 0.025)
        fused = timed(lambda: PF.sparse_step(emb, ids, rows, state), a.warmup, a.reps)
        del state
        emb.grad = torch.sparse_coo_tensor(ids[None], rows, (N, d)).coalesce()
        opt = topt([emb], lr=0.025)
        other = timed(opt.step, a.warmup, a.reps)
        emb.grad = None
        del opt
        out.append(row("op: sparse_step(%s) / %s" % (kind, topt.__name__), "N = 2^%d, M = %d, d = %d" % (lgN, ids.shape[0], d), fused, other))
    return out


def bench_kge(a, lgN=20, P=1024, C=8, n_neg=256, d=400):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2)
    ent = torch.nn.Parameter(torch.rand(1 << lgN, d, device=dev) - 0.5)
    rel = torch.nn.Parameter(torch.rand(1024, d, device=dev) - 0.5)
    h, t = (torch.randint(0, 1 << lgN, (P,), device=dev, generator=gen) for _ in range(2))
    r = torch.randint(0, 1024, (P,), device=dev, generator=gen)
    neg = torch.randint(0, 1 << lgN, (C, n_neg), device=dev, generator=gen)
    kw = dict(gamma=12.0, adv_temp=1.0, check_range=False)
    states = [PF.SparseState(w, "lazy_adam", 0.02) for w in (ent, rel)]
    fused = timed(lambda: PF.kge_step(ent, rel, h, r, t, neg, "transe", *states, **kw), a.warmup, a.reps)
    del states
    other = timed(dense_adam(lambda: PF.kge_loss(ent, rel, h, r, t, neg, "transe", **kw), [ent, rel]), a.warmup, a.reps)
    return [row("kge: kge_step / kge_loss + backward + dense Adam", "2^%d entities, P = %d, neg = %d, d = %d" % (lgN, P, n_neg, d), fused, other)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="+", default=[20, 24], help="log2 of the table heights")
    ap.add_argument("--pairs", type=int, nargs="+", default=[16, 20], help="log2 of the pair counts")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["| what | shape | fused route ms (min-max) | comparison ms (min-max) | ratio | fused peak MiB | comparison peak MiB |",
             "|---|---|---|---|---|---|---|"]
    jobs = [lambda lgN=lgN, lgP=lgP: bench_step(lgN, lgP, 5, 128, a) for lgN in a.rows for lgP in a.pairs] + [lambda: bench_kge(a)]
    for job in jobs:
        for line in job():
            lines.append(line)
            print(line, flush=True)
        gc.collect()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
