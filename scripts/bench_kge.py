"""The fused KGE loss (pgl_amd.embedding_ops.kge_loss) beside the torch composition of the same definition in the reference's own tensor
recipe (bmm for the bilinear models and TransE's cdist expansion, the tiled [C, cs, neg, d] form for RotatE): forward and forward +
backward, with peak memory; and one scores-only ranking row.  A timed window is --inner back-to-back calls between two device
synchronisations; fused and torch windows alternate; a figure is the median of --repeats windows per call, and "spread" is (max - min) /
median over those windows.  The figures are end-to-end call times (the front end's launches included: 3 for the fused forward against
about 15 torch ops), not kernel times.  Prints one JSON line per row; a row where the fused path loses is marked "fused_loses": true.

    python scripts/bench_kge.py [--repeats 20] [--warmup 5] [--inner 20] [--quick]"""
import argparse
import json
import math
import statistics
import time

import torch
import torch.nn.functional as F

from pgl_amd import embedding_ops as E


def torch_loss(ent, rel, h, r, t, neg, model, gamma, tau):
    H, R, T, N = ent[h], rel[r], ent[t], ent[neg]
    C, n, d = N.shape
    if model == "transe":
        a = (H + R).reshape(C, -1, d)
        pos = gamma - (H + R - T).norm(dim=-1)
        q = -2 * torch.bmm(a, N.transpose(1, 2)) + N.norm(dim=-1).pow(2).unsqueeze(-2) + a.norm(dim=-1).pow(2).unsqueeze(-1)
        s = gamma - q.clamp(min=1e-30).sqrt()
    elif model == "distmult":
        pos, s = (H * R * T).sum(-1), torch.bmm((H * R).reshape(C, -1, d), N.transpose(1, 2))
    else:
        h_re, h_im = H.chunk(2, -1)
        if model == "complex":
            r_re, r_im = R.chunk(2, -1)
        else:
            th = R / ((gamma + 2.0) / (d // 2) / math.pi)
            r_re, r_im = th.cos(), th.sin()
        a = torch.cat([h_re * r_re - h_im * r_im, h_re * r_im + h_im * r_re], -1)
        if model == "complex":
            pos, s = (a * T).sum(-1), torch.bmm(a.reshape(C, -1, d), N.transpose(1, 2))
        else:
            mod = lambda x: gamma - (x[..., :d // 2].square() + x[..., d // 2:].square() + 1e-12).sqrt().sum(-1)
            pos = mod(a - T)
            cs = a.shape[0] // C
            s = mod(a.reshape(C, cs, 1, d).tile(1, 1, n, 1) - N.reshape(C, 1, n, d).tile(1, cs, 1, 1))
    w = torch.softmax(tau * s, -1).detach() if tau > 0 else 1.0 / n
    return (F.softplus(-pos).mean() + (w * F.softplus(s)).sum(-1).mean()) / 2


def window(fn, inner):
    """One timed window: `inner` back-to-back calls between two device synchronisations -> ms per call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def compare(fns, warmup, repeats, inner):
    """{name: fn} -> {name: (median ms per call, (max - min) / median over the windows, peak MiB)}.  The candidates take turns, window by
    window, so clock and cache drift falls on all of them alike; the peak is measured in one call of its own."""
    out, ts = {}, {k: [] for k in fns}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        out[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for _ in range(repeats):
        for k, fn in fns.items():
            ts[k].append(window(fn, inner))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v), out[k]) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev, Ne, Nr, C, cs, tau = torch.device("cuda:0"), 100000, 64, 8, 128, 1.0
    gen = torch.Generator().manual_seed(0)
    for model in ("transe", "distmult", "complex", "rotate"):
        for d in ((200,) if args.quick else (200, 400, 800)):
            for n in ((256,) if args.quick else (256, 1024)):
                row = {"model": model, "P": C * cs, "neg": n, "d": d}
                gamma = 12.0
                ent = (torch.randn(Ne, d, generator=gen) * 0.3).to(dev).requires_grad_(True)
                rel = (torch.randn(Nr, d // 2 if model == "rotate" else d, generator=gen) * 0.3).to(dev).requires_grad_(True)
                h, t = (torch.randint(0, Ne, (C * cs,), generator=gen).to(dev) for _ in range(2))
                r, neg = torch.randint(0, Nr, (C * cs,), generator=gen).to(dev), torch.randint(0, Ne, (C, n), generator=gen).to(dev)
                calls = {"fused": lambda: E.kge_loss(ent, rel, h, r, t, neg, model, gamma=gamma, adv_temp=tau, check_range=False),
                         "torch": lambda: torch_loss(ent, rel, h, r, t, neg, model, gamma, tau)}

                def fwd(fn):
                    def run():
                        with torch.no_grad():
                            fn()
                    return run

                def both(fn):
                    def run():
                        ent.grad = rel.grad = None
                        fn().backward()
                    return run
                for what, wrap in (("fwd", fwd), ("fwdbwd", both)):
                    for name, (ms, spread, mib) in compare({k: wrap(v) for k, v in calls.items()}, args.warmup, args.repeats, args.inner).items():
                        row["%s_%s_ms" % (name, what)], row["%s_%s_spread" % (name, what)], row["%s_%s_MiB" % (name, what)] = ms, spread, mib
                row["fused_loses"] = row["fused_fwd_ms"] > row["torch_fwd_ms"] or row["fused_fwdbwd_ms"] > row["torch_fwdbwd_ms"]
                print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    # ranking: 64 positives against 2^17 entities, scores only
    d, n = 400, 1 << 17
    ent, rel = torch.randn(n, d, device=dev) * 0.3, torch.randn(Nr, d, device=dev) * 0.3
    h, t, r = (torch.randint(0, m, (64,), device=dev) for m in (n, n, Nr))
    everyone = torch.arange(n, device=dev)[None]
    res = compare({"fused": lambda: E.kge_scores(ent, rel, h, r, t, everyone, "transe", check_range=False),
                   "torch_cdist": lambda: 12.0 - torch.cdist((ent[h] + rel[r])[None], ent[None])}, args.warmup, args.repeats, args.inner)
    row = {"ranking": "transe", "P": 64, "neg": n, "d": d, "fused_loses": res["fused"][0] > res["torch_cdist"][0]}
    for name, (ms, spread, mib) in res.items():
        row[name + "_ms"], row[name + "_spread"], row[name + "_MiB"] = round(ms, 3), round(spread, 3), round(mib, 1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
