#!/usr/bin/env python3
"""Attention read-outs on one MI355X: the fused read-out kernels (csrc/readout.hip, front end pgl_amd/readout_ops.py) next to the
unfused tensor code of the same build (fused=False: segment softmax, the [N, d] product, the segment sum -- and for Set2Set the same
chain once per round), on the same batched graphs, in the same process.

Shapes (graphs x nodes per graph; the read-outs use no edge):  (a) 128 x 30,  (b) 4096 x 64,  (c) 64 x 4000  -- the batches of
scripts/bench_pool.py -- and (d) 1 x 2**20, one large graph (the multi-piece path and its merge launch).  Widths d = 64 and 128.
Cases per shape and width, forward (fwd) and forward + backward (f+b):
    op gate      readout_ops.attention_readout(x, plan, score=s)              | segment_softmax(s) -> a * x -> segment_sum
    op query     readout_ops.attention_readout(x, plan, query=q)              | q[gid] -> row dot -> the same chain
    GlobalAttention(Linear(d, 1), Linear(d, d), fused=True)                   | the same layer, fused=False
    Set2Set(d, n_iters=3, fused=True)                                         | the same layer, fused=False

Before anything is timed the two results of every case are compared (within 1e-4 of each row's largest value; a score's gradient [N] as one row); they must agree or
the run stops.  Device events around every call, median of --reps after --warmup, minimum and maximum next to it.  A host read
inside a call is part of what is timed (the events bracket the whole call).

    python scripts/bench_readout.py [--reps 5] [--out profiles/readout/bench_readout.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pgl_amd as pgl  # noqa: E402
from pgl_amd import readout_ops  # noqa: E402

SHAPES = [("a", 128, 30), ("b", 4096, 64), ("c", 64, 4000), ("d", 1, 1 << 20)]
WIDTHS = (64, 128)


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


def batch(n_graphs, n_nodes, dim, seed):
    rng = np.random.default_rng(seed)
    n = n_graphs * n_nodes
    index = np.arange(n_graphs + 1, dtype=np.int64) * n_nodes
    edges = torch.zeros((0, 2), dtype=torch.int64, device="cuda")
    g = pgl.Graph(edges=edges, num_nodes=n, _num_graph=n_graphs, _graph_node_index=index, _graph_edge_index=np.zeros(n_graphs + 1, np.int64))
    x = torch.as_tensor(rng.standard_normal((n, dim)).astype(np.float32)).cuda()
    return g, x, index


def close(a, b, what):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for u, v in zip(a, b):
        u, v = (t.reshape(t.shape[0] if t.dim() > 1 else 1, -1).double() for t in (u, v))       # (a [N] gradient: one row)
        tol = 1e-4 * v.abs().amax(1, keepdim=True) + 1e-30
        if not bool(((u - v).abs() <= tol).all()):
            raise SystemExit("bench_readout: the two paths differ at %s: nothing is timed" % what)


def with_backward(forward, leaves):
    def run():
        xs = [t.detach().requires_grad_(True) for t in leaves]
        out = forward(*xs)
        out.sum().backward()
        return (out.detach(),) + tuple(t.grad for t in xs)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for tag, G, m in SHAPES:
        for d in WIDTHS:
            g, x, index = batch(G, m, d, seed=1)
            gid = g.graph_node_id
            plan = readout_ops.readout_plan(index, x.device)
            gen = torch.Generator(device="cuda"); gen.manual_seed(2)
            score = torch.randn(G * m, generator=gen, device="cuda")
            query = torch.randn((G, d), generator=gen, device="cuda") / d ** 0.5
            gl = gid.long()

            def chain(xx, e):
                a = pgl.math.segment_softmax(e.reshape(-1, 1), gid, num_segments=G)
                return pgl.math.segment_sum(a * xx, gid, num_segments=G)

            cases = [("op gate", lambda xx, s: readout_ops.attention_readout(xx, plan, score=s), lambda xx, s: chain(xx, s), (x, score)),
                     ("op query", lambda xx, q: readout_ops.attention_readout(xx, plan, query=q),
                      lambda xx, q: chain(xx, (xx * q[gl]).sum(-1)), (x, query))]
            torch.manual_seed(0)
            ga = pgl.nn.GlobalAttention(torch.nn.Linear(d, 1), torch.nn.Linear(d, d)).cuda()
            ga_f = pgl.nn.GlobalAttention(ga.gate, ga.nn, fused=True)
            s2s = pgl.nn.Set2Set(d, 3).cuda()
            s2s_f = pgl.nn.Set2Set(d, 3, fused=True).cuda()
            s2s_f.load_state_dict(s2s.state_dict())
            assert ga_f._takes_fused(g, x) and s2s_f._takes_fused(g, x)
            cases.append(("GlobalAttention", lambda xx: ga_f(g, xx), lambda xx: ga(g, xx), (x,)))
            cases.append(("Set2Set n_iters=3", lambda xx: s2s_f(g, xx), lambda xx: s2s(g, xx), (x,)))
            for name, fused, plain, leaves in cases:
                def no_grad(fn):
                    def run():
                        with torch.no_grad():
                            return fn(*leaves)
                    return run
                for kind, a, b in (("fwd", no_grad(fused), no_grad(plain)), ("f+b", with_backward(fused, leaves), with_backward(plain, leaves))):
                    close(a(), b(), "%s %s %s d=%d" % (name, kind, tag, d))
                    ta, tb = timed(a, args.warmup, args.reps), timed(b, args.warmup, args.reps)
                    rows.append(dict(shape=tag, graphs=G, nodes_per_graph=m, d=d, case="%s %s" % (name, kind), fused_ms=ta, unfused_ms=tb,
                                     ratio=tb[0] / ta[0]))
                    print(json.dumps(rows[-1]), flush=True)
            del g, x, plan, score, query, gid, gl
            torch.cuda.empty_cache()
    lines = ["shape  graphs x nodes      d    case                     fused ms (min .. max)          unfused ms (min .. max)        unfused / fused"]
    for r in rows:
        lines.append("%-5s  %5d x %-8d  %4d  %-22s  %8.3f (%7.3f .. %7.3f)   %8.3f (%7.3f .. %7.3f)   %6.2f" %
                     ((r["shape"], r["graphs"], r["nodes_per_graph"], r["d"], r["case"]) + r["fused_ms"] + r["unfused_ms"] + (r["ratio"],)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
