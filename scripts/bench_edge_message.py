"""Times Graph.send_edge_message and one GINEConv / GENConv layer on an MI355X, every row beside the fused=False composition of the same
build (message_ops.edge_message_composed), forward and forward + backward.

    python scripts/bench_edge_message.py [--full_graph] [--out profiles/edge_message/bench_edge_message.txt]

Batch rows: 256 and 1024 molecule-like graphs of about 25 nodes (degree <= 4), d = 100, 300, 600, coded bond features (5, 6, 2).
Full-graph rows (--full_graph): the 20 M-edge RMAT graph at d = 64, 128 with a dense edge feature, both reductions.
Method: warm-up, then the median of 5 batches of `iters` back-to-back calls between two device synchronisations (host launch cost is
part of a call); a row where the fused path is slower is marked LOSES."""
import argparse
import statistics
import sys
import time

import torch

import pgl_amd as pgl
from pgl_amd import message_ops

VOCAB = (5, 6, 2)


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize(); times.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(times)


def molecules(num_graphs, gen):
    edges, base = [], 0
    for _ in range(num_graphs):
        n = int(torch.randint(18, 33, (1,), generator=gen))
        u = torch.arange(n - 1)
        edges.append(torch.cat([torch.stack([u, u + 1], 1), torch.stack([u + 1, u], 1)]) + base)
        base += n
    return torch.cat(edges), base


def rows_for(name, g, x, edge_feat, codes, tables, reduce, act, iters, out):
    src, dst = g.edges[:, 0], g.edges[:, 1]
    table, offsets, _ = message_ops.stack_tables(tables) if tables else (None, None, None)
    fused = lambda: g.send_edge_message(x, edge_feat, codes, tables, act, reduce, 1e-7, 1.0, check_range=False)
    comp = lambda: message_ops.edge_message_composed(x, src, dst, g.num_nodes, edge_feat, codes, table, offsets, act, reduce, 1e-7, 1.0)
    both = lambda f: (lambda: f().sum().backward())
    for what, a, b in (("forward", fused, comp), ("forward + backward", both(fused), both(comp))):
        ta, tb = timed(a, iters), timed(b, iters)
        line = "%-34s %-8s %-18s fused %8.3f ms   composition %8.3f ms   %5.2fx%s" % (name, reduce, what, ta, tb, tb / ta, "   LOSES" if ta > tb else "")
        print(line); out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full_graph", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    out = []
    for num_graphs in (256, 1024):
        edges, n = molecules(num_graphs, gen)
        g = pgl.Graph(edges=edges.cuda(), num_nodes=n)
        for d in (100, 300, 600):
            x = torch.randn(n, d, device="cuda", requires_grad=True)
            tables = [torch.randn(v, d, device="cuda", requires_grad=True) for v in VOCAB]
            codes = torch.stack([torch.randint(0, v, (edges.shape[0],), generator=gen) for v in VOCAB], 1).int().cuda()
            name = "%d molecules, d = %d, coded" % (num_graphs, d)
            rows_for(name, g, x, None, codes, tables, "sum", "relu", 50, out)
            rows_for(name, g, x, None, codes, tables, "softmax", "swish", 50, out)
        for layer, make in (("GINEConv", lambda f: pgl.nn.GINEConv(300, 300, edge_vocab=VOCAB, fused=f)), ("GENConv", lambda f: pgl.nn.GENConv(300, edge_vocab=VOCAB, fused=f))):
            x = torch.randn(n, 300, device="cuda", requires_grad=True)
            mf, mc = make(True).cuda(), make(False).cuda()
            for what, run in (("forward", lambda m: (lambda: m(g, x, codes))), ("forward + backward", lambda m: (lambda: m(g, x, codes).sum().backward()))):
                ta, tb = timed(run(mf), 50), timed(run(mc), 50)
                line = "%-34s %-8s %-18s fused %8.3f ms   composition %8.3f ms   %5.2fx%s" % ("%d molecules, %s(300)" % (num_graphs, layer), "layer", what, ta, tb, tb / ta, "   LOSES" if ta > tb else "")
                print(line); out.append(line)
    if args.full_graph:
        from pgl_amd.utils.rmat import rmat_edges
        n = 1 << 20
        g = pgl.Graph(edges=rmat_edges(20, 20_000_000, seed=42, device="cuda"), num_nodes=n)
        for d in (64, 128):
            x = torch.randn(n, d, device="cuda", requires_grad=True)
            ef = torch.randn(20_000_000, d, device="cuda", requires_grad=True)
            for reduce, act in (("sum", "relu"), ("softmax", "swish")):
                rows_for("RMAT-20, 20 M edges, d = %d, dense" % d, g, x, ef, None, None, reduce, act, 5, out)
    if args.out:
        open(args.out, "w").write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
