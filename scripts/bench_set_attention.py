#!/usr/bin/env python3
"""SAB on one MI355X: fused=True (the block's attention on the set-attention kernels, csrc/set_attention.hip, front end
pgl_amd/readout_ops.py: set_attention) next to fused=False of the same build (three head reshuffles, bmm, softmax over [B h, n, n], bmm,
a fourth reshuffle), the same parameters, the same input, in the same process.

Settings: dim = 128 with 4 heads and dim = 256 with 8 heads.  Shapes (sets x rows): 4096 x 8, 4096 x 32, 1024 x 75, 512 x 128, 8 x 128.
Before anything is timed the two outputs must agree within 1e-4 of the largest value and the input gradients likewise in all but at
most 3 sets, or the run stops.  A set may differ because of the ReLU in the block's tail, as in bench_seed_readout.py: a pre-activation
within rounding of 0 (one is expected among the 8 M of a large case) switches between two fp32 paths and moves the gradient of the rows
of ITS set, and of no other; a wrong kernel would move every set.  The largest difference and the number of such sets are kept in the
JSON lines ("differ", "flipped_sets").  Device events around every call, median of --reps after --warmup, minimum and maximum next to it.

    python scripts/bench_set_attention.py [--reps 5] [--out profiles/set_attention/bench_set_attention.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgl_amd import readout_ops  # noqa: E402
from pgl_amd.nn.gmt_pool import SAB  # noqa: E402

SHAPES = [(4096, 8), (4096, 32), (1024, 75), (512, 128), (8, 128)]
SETTINGS = [(128, 4), (256, 8)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for dim, heads in SETTINGS:
        torch.manual_seed(0)
        layer = SAB(dim, dim, heads, fused=True).cuda()
        for B, n in SHAPES:
            x = torch.randn(B, n, dim, device="cuda")

            def forward(fused):
                def run():
                    layer.fused = fused
                    with torch.no_grad():
                        return (layer(x, None, None),)
                return run

            def both(fused):
                def run():
                    layer.fused = fused
                    xx = x.detach().requires_grad_(True)
                    out = layer(xx, None, None)
                    out.sum().backward()
                    return out.detach(), xx.grad
                return run

            for kind, make in (("fwd", forward), ("f+b", both)):
                before = readout_ops.LAUNCHES["set_attention"]
                got, want = make(True)(), make(False)()
                assert readout_ops.LAUNCHES["set_attention"] == before + 1
                worst = [float((u - v).abs().max() / v.abs().max()) for u, v in zip(got, want)]
                flipped = 0 if kind == "fwd" else int(((got[1] - want[1]).abs().amax((1, 2)) > 1e-4 * want[1].abs().max()).sum())
                if worst[0] > 1e-4 or flipped > 3 or worst[-1] > 1e-1:
                    raise SystemExit("bench_set_attention: the two paths differ at %s (%s, %d sets): nothing is timed" % ((dim, heads, B, n, kind), worst, flipped))
                ta, tb = timed(make(True), args.warmup, args.reps), timed(make(False), args.warmup, args.reps)
                rows.append(dict(dim=dim, heads=heads, sets=B, rows=n, case=kind, differ=worst, flipped_sets=flipped, fused_ms=ta, unfused_ms=tb, ratio=tb[0] / ta[0]))
                print(json.dumps(rows[-1]), flush=True)
    lines = ["dim  heads   sets  rows  case   fused ms (min .. max)          unfused ms (min .. max)        unfused / fused"]
    for r in rows:
        lines.append("%3d  %5d  %5d  %4d  %-5s  %8.3f (%7.3f .. %7.3f)   %8.3f (%7.3f .. %7.3f)   %6.2f" %
                     ((r["dim"], r["heads"], r["sets"], r["rows"], r["case"]) + r["fused_ms"] + r["unfused_ms"] + (r["ratio"],)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
