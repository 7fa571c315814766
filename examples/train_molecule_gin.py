"""Graph regression on synthetic molecule-like batches with GINEConv or GENConv layers and a mean read-out (the shape of the reference's
ogb_examples/lsc/PCQM4M and examples/kddcup2021/PCQM4M models): degree <= 4, three categorical bond features with vocabularies (5, 6, 2),
a planted target.  --fused takes the layers' messages through Graph.send_edge_message (csrc/edge_message.hip); without it they run the
torch composition of the same definition.  Both print the same loss to the two printed decimals over the default 30 steps (the sums are taken in another order).

    python examples/train_molecule_gin.py --layer gine --fused
"""
import argparse

import torch

import pgl_amd as pgl

VOCAB = (5, 6, 2)


def make_batch(num_graphs, gen, device):
    """-> (graph, atom ids [N], bond codes [E, 3], graph id of every node [N], target [num_graphs])."""
    edges, atoms, codes, gid, target, base = [], [], [], [], [], 0
    for i in range(num_graphs):
        n = int(torch.randint(18, 33, (1,), generator=gen))
        a = torch.randint(0, 8, (n,), generator=gen)
        u = torch.arange(n - 1)                                       # a chain plus a few ring closures: degree <= 4
        v = u + 1
        extra = torch.randint(0, n - 3, (n // 6,), generator=gen).unique()
        u, v = torch.cat([u, extra]), torch.cat([v, extra + 3])
        c = torch.stack([torch.randint(0, s, (u.shape[0],), generator=gen) for s in VOCAB], 1)
        edges.append(torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)]) + base)
        codes.append(torch.cat([c, c]))
        atoms.append(a); gid.append(torch.full((n,), i))
        target.append(a.float().mean() + 0.3 * c[:, 0].float().mean())        # planted: atoms and the first bond feature
        base += n
    g = pgl.Graph(edges=torch.cat(edges).to(device), num_nodes=base)
    return g, torch.cat(atoms).to(device), torch.cat(codes).int().to(device), torch.cat(gid).to(device), torch.stack(target).to(device)


class Model(torch.nn.Module):
    def __init__(self, layer, hidden, depth, fused):
        super().__init__()
        self.embed = torch.nn.Embedding(8, hidden)
        make = (lambda: pgl.nn.GINEConv(hidden, hidden, edge_vocab=VOCAB, fused=fused)) if layer == "gine" else \
               (lambda: pgl.nn.GENConv(hidden, edge_vocab=VOCAB, learn_t=True, fused=fused))
        self.layers = torch.nn.ModuleList([make() for _ in range(depth)])
        self.head = torch.nn.Linear(hidden, 1)

    def forward(self, g, atoms, codes, gid, num_graphs):
        h = self.embed(atoms)
        for layer in self.layers:
            h = torch.relu(layer(g, h, codes))
        ones = torch.ones(h.shape[0], 1, device=h.device)
        pooled = torch.zeros(num_graphs, h.shape[1], device=h.device).index_add_(0, gid, h)
        return (self.head(pooled / torch.zeros(num_graphs, 1, device=h.device).index_add_(0, gid, ones))).squeeze(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layer", choices=["gine", "gen"], default="gine")
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args()
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    model = Model(args.layer, args.hidden, args.depth, args.fused).to(args.device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    batches = [make_batch(args.graphs, gen, args.device) for _ in range(4)]
    for step in range(args.steps):
        g, atoms, codes, gid, target = batches[step % len(batches)]
        loss = torch.nn.functional.mse_loss(model(g, atoms, codes, gid, args.graphs), target)
        opt.zero_grad(); loss.backward(); opt.step()
        if step % 5 == 0 or step == args.steps - 1:
            print("step %3d  loss %.2f" % (step, float(loss.detach())))


if __name__ == "__main__":
    main()
