#!/usr/bin/env python3
"""The fused skip-gram / BPR loss (csrc/pair_loss.hip, pgl_amd.nn.functional.skip_gram_loss / bpr_loss) on one MI355X next to the torch
composition the examples run without --fused_loss (F.embedding gathers, bmm / mul + sum, logsigmoid / softplus, mean; its backward
through embedding_dense_backward), on the same build, the same tables and the same ids, in the same process.

Workload: RMAT scale 20 with 20 M edges (pgl_amd/utils/rmat.py, seed 42).  Pairs: uniform walks -> ops.skip_gram_pairs, the first P of
them; negatives: ops.sample_negatives (checked against the graph; a row without one is clamped to id 0 for both paths).  P in
{2^16, 2^20, 2^22}, K in {1, 5}, d in {64, 100, 128}, two tables of 2^20 rows.  One BPR batch: sampling.bpr_triples for 2^20 users, one
table of d = 64 passed as both (the LightGCN shape).

Before anything is timed the two losses (1e-5 relative) and both gradients (1e-4 of the largest entry) must agree, or the run stops.
Device events around every call, median of --reps after --warmup, minimum and maximum next to it.  "sort": pglamd_csr_build over the
P sources alone, which every fused call contains.  Peak memory: torch.cuda.max_memory_allocated over one forward + backward, above
what the tables and ids hold.

    python scripts/bench_pair_loss.py [--reps 5] [--out profiles/pair_loss/bench_pair_loss.md]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402
from pgl_amd import embedding_ops  # noqa: E402
from pgl_amd.utils.rmat import rmat_edges  # noqa: E402


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


def torch_skipgram(emb, ctx, src, dst, neg):
    u = F.embedding(src, emb)
    pos = (u * F.embedding(dst, ctx)).sum(-1)
    negs = torch.bmm(F.embedding(neg, ctx), u.unsqueeze(-1)).squeeze(-1)
    return -(F.logsigmoid(pos) + F.logsigmoid(-negs).sum(-1)).mean()


def torch_bpr(z, users, pos, neg):
    return F.softplus((z[users] * z[neg]).sum(-1) - (z[users] * z[pos]).sum(-1)).mean()


def both_ways(loss_fn, tables):
    """-> (forward alone under no_grad, forward + backward returning [loss, grads...])."""
    def fwd():
        with torch.no_grad():
            return loss_fn(*tables)

    def fb():
        xs = [t.detach().requires_grad_(True) for t in tables]
        loss = loss_fn(*xs)
        loss.backward()
        return [loss.detach()] + [x.grad for x in xs]
    return fwd, fb


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def compare(what, fused, plain, sort_fn, args):
    """fused / plain: (forward, forward + backward) callables -> one result row; stops the run when the two paths disagree."""
    got, want = fused[1](), plain[1]()
    if abs(float(got[0]) - float(want[0])) > 1e-5 * abs(float(want[0])):
        raise SystemExit("bench_pair_loss: the losses differ at %s (%r, %r): nothing is timed" % (what, float(got[0]), float(want[0])))
    for a, b in zip(got[1:], want[1:]):
        if not bool(((a - b).abs() <= 1e-4 * b.abs().max()).all()):
            raise SystemExit("bench_pair_loss: the gradients differ at %s: nothing is timed" % what)
    del got, want
    r = dict(case=what, sort_ms=timed(sort_fn, args.warmup, args.reps)[0])
    for kind, i in (("fwd", 0), ("f+b", 1)):
        r["fused_" + kind], r["torch_" + kind] = timed(fused[i], args.warmup, args.reps), timed(plain[i], args.warmup, args.reps)
    r["fused_peak_mib"], r["torch_peak_mib"] = peak_of(fused[1]), peak_of(plain[1])
    print(json.dumps(r), flush=True)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--log_pairs", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--negs", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 100, 128])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    N = 1 << args.scale
    g = pgl.Graph(edges=rmat_edges(args.scale, args.edges, seed=42, device=dev), num_nodes=N).tensor()
    succ = g._csr_succ_sorted()
    gen = torch.Generator(device=dev).manual_seed(0)
    P_max = 1 << max(args.log_pairs)
    starts = torch.randint(0, N, (max(P_max // 16, 1024),), device=dev, generator=gen)
    paths, lengths = pgl.sampling.walks(g, starts, 19, seed=1)
    src_all, dst_all = pgl.ops.skip_gram_pairs(paths, lengths, 5, seed=1)
    if src_all.shape[0] < P_max:
        raise SystemExit("bench_pair_loss: the walks gave %d pairs, %d are needed" % (src_all.shape[0], P_max))
    rows = []
    sort_of = lambda key, n: (lambda: pgl.ops.csr_build(key, key, n + 1, want_i64=False, check_range=False))
    for d in args.dims:
        emb, ctx = (torch.randn(N, d, device=dev, generator=gen) / d ** 0.25 for _ in range(2))
        for lp in args.log_pairs:
            src, dst = src_all[:1 << lp].contiguous(), dst_all[:1 << lp].contiguous()
            for K in args.negs:
                neg = pgl.ops.sample_negatives(succ, src, K, seed=3, check=False).clamp_min(0)
                fused = both_ways(lambda e, c: pgl.nn.functional.skip_gram_loss(e, c, src, dst, neg), (emb, ctx))
                plain = both_ways(lambda e, c: torch_skipgram(e, c, src, dst, neg), (emb, ctx))
                before = embedding_ops.LAUNCHES["pair_loss"]
                fused[0]()
                assert embedding_ops.LAUNCHES["pair_loss"] == before + 1
                rows.append(compare("skip-gram P=2^%d K=%d d=%d" % (lp, K, d), fused, plain, sort_of(src, N), args))
                del neg
        del emb, ctx
        torch.cuda.empty_cache()
    users, pos, neg = pgl.sampling.bpr_triples(g, torch.randint(0, N, (1 << 20,), device=dev, generator=gen), (0, N), seed=5)
    z = torch.randn(N, 64, device=dev, generator=gen) / 64 ** 0.25
    rows.append(compare("BPR %d triples d=64, one table" % users.shape[0],
                        both_ways(lambda t: pgl.nn.functional.bpr_loss(t, t, users, pos, neg), (z,)),
                        both_ways(lambda t: torch_bpr(t, users, pos, neg), (z,)), sort_of(users, N), args))

    fmt = lambda t: "%.3f (%.3f .. %.3f)" % t
    lines = ["rmat%d: %d nodes, %d edges; median of %d after %d warm-up calls, device events; ms (min .. max)" %
             (args.scale, N, g.num_edges, args.reps, args.warmup), "",
             "| case | fused fwd | torch fwd | torch / fused | fused f+b | torch f+b | torch / fused | sort ms (share of fused f+b) | peak MiB fused | peak MiB torch |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %s | %.2f | %s | %s | %.2f | %.3f (%.0f %%) | %.0f | %.0f |" %
                     (r["case"], fmt(r["fused_fwd"]), fmt(r["torch_fwd"]), r["torch_fwd"][0] / r["fused_fwd"][0], fmt(r["fused_f+b"]),
                      fmt(r["torch_f+b"]), r["torch_f+b"][0] / r["fused_f+b"][0], r["sort_ms"], 100 * r["sort_ms"] / r["fused_f+b"][0],
                      r["fused_peak_mib"], r["torch_peak_mib"]))
    lost = [r["case"] for r in rows if r["torch_fwd"][0] < r["fused_fwd"][0] or r["torch_f+b"][0] < r["fused_f+b"][0]]
    lines += ["", "Rows in which the fused path LOSES (forward or forward + backward): " + ("; ".join(lost) if lost else "none") + "."]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return rows


if __name__ == "__main__":
    main()
