"""The seed-attention read-out (pgl_amd/csrc/seed_readout.hip, pgl_amd.readout_ops.seed_attention_readout) and
GraphMultisetTransformer(fused=True) on the MI355X, held to the definition below: out, dK, dV and dQ within
8 * max(max|def32 - def64|, eps32 * max|def64|) of the fp64 definition, both terms taken from the host definition and never from the
kernel (the 8 covers a summation order that differs from torch's: row slots, pieces, W partials against a serial einsum).  With O(1)
inputs a dropped row, seed or head moves an element by 1e-2 or more, three orders above the bar.  In the key_bias cases the fp32
definition itself departs from fp64 (-1e9 swallows the score in fp32 only), which the bar measures and follows.
Largest ratio |got - def64| / (the bar / 8) measured on the MI355X: 1.13 (out at dim = 256, 4 heads, 32 seeds;
profiles/seed_readout/README.md)."""
import math

import numpy as np
import pytest
import torch

import readout_defs as R
from gpu_common import pgl  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

CASES = [(4, 1, 1), (32, 4, 8), (128, 4, 8), (128, 8, 5), (256, 4, 32), (64, 1, 3)]      # (dim, heads, seeds)
EPS32 = float(np.finfo(np.float32).eps)


def definition(k, v, q, seg_ptr, heads, key_bias=None, residual=True):
    """k, v [N, dim], q [seeds, dim] -> out [S, seeds, dim]: the softmax over the SEED axis, a per-segment loop."""
    dim, hd = k.shape[1], k.shape[1] // heads
    kh, vh, qh = (t.reshape(t.shape[0], heads, hd) for t in (k, v, q))
    s = torch.einsum("jhc,nhc->njh", qh, kh) / math.sqrt(dim)
    if key_bias is not None:
        s = key_bias[:, None, None] + s
    a = torch.softmax(s, dim=1)
    out = [float(residual) * qh + torch.einsum("njh,nhc->jhc", a[b:e], vh[b:e]) for b, e in zip(seg_ptr[:-1], seg_ptr[1:])]
    return torch.stack(out).reshape(len(seg_ptr) - 1, q.shape[0], dim)


def evaluate(dtype, k, v, q, cot, seg_ptr, heads, key_bias=None):
    """The definition and its gradients by autograd on the host in `dtype` -> [out, dK, dV, dQ]."""
    xs = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (k, v, q)]
    bias = None if key_bias is None else key_bias.detach().cpu().to(dtype)
    out = definition(xs[0], xs[1], xs[2], seg_ptr, heads, bias)
    out.backward(cot.detach().cpu().to(dtype))
    return [out.detach()] + [t.grad for t in xs]


def inputs(lengths, dim, seeds, seed=0):
    gen = torch.Generator().manual_seed(1000 * dim + seeds + seed)
    n, s = int(np.sum(lengths)), len(lengths)
    return [torch.randn(shape, generator=gen).cuda() for shape in ((n, dim), (n, dim), (seeds, dim), (s, seeds, dim))]


def run(plan, k, v, q, cot, heads, key_bias=None, need=(True, True, True), residual=True):
    from pgl_amd import readout_ops
    xs = [t.detach().requires_grad_(bool(n)) for t, n in zip((k, v, q), need)]
    out = readout_ops.seed_attention_readout(xs[0], xs[1], xs[2], plan, heads, key_bias=key_bias, residual=residual)
    out.backward(cot)
    return [out.detach()] + [t.grad for t in xs]


def plan_of(lengths):
    from pgl_amd import readout_ops
    return readout_ops.readout_plan(R.seg_ptr_of(lengths), "cuda")


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "key_bias"])
@pytest.mark.parametrize("dim,heads,seeds", CASES)
def test_definition(pgl, dim, heads, seeds, with_bias):
    """Over readout_defs.LENGTHS (0 .. 3 PIECE + 5 rows: empty, shorter than a pass, one, two and four pieces).  The bias case sets -1e9
    on a handful of rows, among them a segment's first row and the whole one-row segment."""
    from pgl_amd import readout_ops
    seg_ptr = R.seg_ptr_of(R.LENGTHS)
    k, v, q, cot = inputs(R.LENGTHS, dim, seeds)
    bias = None
    if with_bias:
        bias = torch.zeros(k.shape[0], device="cuda")
        bias[[0, int(seg_ptr[4]), int(seg_ptr[4]) + 7, int(seg_ptr[8]) + 100, int(seg_ptr[10]) + 3 * R.PIECE]] = -1e9
    before = dict(readout_ops.LAUNCHES)
    got = run(plan_of(R.LENGTHS), k, v, q, cot, heads, bias)
    assert readout_ops.LAUNCHES["seed_readout"] == before.get("seed_readout", 0) + 1
    assert readout_ops.LAUNCHES["seed_readout_backward"] == before.get("seed_readout_backward", 0) + 1
    d64 = evaluate(torch.float64, k, v, q, cot, seg_ptr, heads, bias)
    d32 = evaluate(torch.float32, k, v, q, cot, seg_ptr, heads, bias)
    ratios = {}
    for name, g, w64, w32 in zip(("out", "dK", "dV", "dQ"), got, d64, d32):
        unit = max(float((w32.double() - w64).abs().max()), EPS32 * float(w64.abs().max()))
        err = float((g.cpu().double() - w64).abs().max())
        ratios[name] = err / unit if unit > 0.0 else (0.0 if err == 0.0 else float("inf"))       # (one seed: dK is exactly 0)
    print("seed_readout dim=%d heads=%d seeds=%d bias=%s: |got - def64| / unit = %s" %
          (dim, heads, seeds, with_bias, ", ".join("%s %.2f" % kv for kv in ratios.items())))
    assert all(r <= 8.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("lengths", [[0, 5, 0, 0, 300, 0], [0]])
def test_empty_segments_and_residual(pgl, lengths, residual):
    k, v, q, cot = inputs(lengths, 32, 8)
    out, _, _, dq = run(plan_of(lengths), k, v, q, cot, 4, residual=residual)
    want = q if residual else torch.zeros_like(q)
    for g, n in enumerate(lengths):
        if n == 0:
            assert same_bits(out[g], want), g
        else:
            assert not same_bits(out[g], want), g
    assert bool(torch.isfinite(dq).all())


def test_bits(pgl):
    """The same call twice; a subset of the gradients; a uniform plan (the plain block's, 7 segments of 8 rows) against the general one."""
    k, v, q, cot = inputs(R.LENGTHS, 128, 8)
    bias = torch.zeros(k.shape[0], device="cuda")
    bias[5] = -1e9
    plan = plan_of(R.LENGTHS)
    first = run(plan, k, v, q, cot, 4, bias)
    again = run(plan, k, v, q, cot, 4, bias)
    assert all(same_bits(a, b) for a, b in zip(first, again))
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        part = run(plan, k, v, q, cot, 4, bias, need=need)
        assert same_bits(part[0], first[0])
        for n, a, b in zip(need, part[1:], first[1:]):
            assert (a is None) if not n else same_bits(a, b), need
    k, v, q, cot = inputs([8] * 7, 32, 8)
    from pgl_amd.nn.gmt_pool import MAB
    mab = MAB(32, 32, 32, 4, fused=True)
    uniform = mab._seed_plan(q, k.reshape(7, 8, 32), None)
    assert uniform is not None and uniform is mab._seed_plan(q, k.reshape(7, 8, 32), None)
    assert all(same_bits(a, b) for a, b in zip(run(uniform, k, v, q, cot, 4), run(plan_of([8] * 7), k, v, q, cot, 4)))


@pytest.mark.parametrize("what", ["k = 33", "dim = 260", "hd = 12", "cpu", "plan"])
def test_refusals(pgl, what):
    from pgl_amd import readout_ops
    n, dim, seeds, heads = {"k = 33": (9, 32, 33, 4), "dim = 260": (9, 260, 8, 5), "hd = 12": (9, 48, 8, 4)}.get(what, (9, 32, 8, 4))
    assert readout_ops.seed_readout_supported(seeds, dim, heads) == (what in ("cpu", "plan"))
    dev = "cpu" if what == "cpu" else "cuda"
    k, v, q = torch.randn(n, dim, device=dev), torch.randn(n, dim, device=dev), torch.randn(seeds, dim, device=dev)
    plan = plan_of([4, 6] if what == "plan" else [4, 5])
    before = dict(readout_ops.LAUNCHES)
    with pytest.raises(ValueError):
        readout_ops.seed_attention_readout(k, v, q, plan, heads)
    assert dict(readout_ops.LAUNCHES) == before


def test_layer_against_its_unfused_self(pgl):
    """GraphMultisetTransformer(fused=True) against the same parameters with .fused off, graphs of 1, 7, 30 and 300 nodes; one node's
    features and lin1's bias are zero, so the -1e9 branch runs on a real node.  Output, d x and every parameter gradient within
    5e-5 * max|unfused| + 1e-6 (the bar of the fused-vs-unfused layer gradients in tests/test_a13_f1_layers.py)."""
    from pgl_amd import readout_ops
    rng = np.random.default_rng(3)
    graphs = [pgl.Graph(edges=rng.integers(0, m, (3 * m, 2)).astype(np.int64), num_nodes=m) for m in (1, 7, 30, 300)]
    bg = pgl.Graph.disjoint(graphs)
    bg.tensor()
    torch.manual_seed(0)
    layer = pgl.nn.GraphMultisetTransformer(16, 32, 8, num_nodes=30, num_heads=4, fused=True).cuda()
    with torch.no_grad():
        layer.lin1.bias.zero_()
    x = torch.randn(338, 16, device="cuda")
    x[11] = 0.0
    cot = torch.randn(4, 8, device="cuda")

    def step(xx):
        layer.zero_grad()
        xx = xx.detach().requires_grad_(True)
        before = dict(readout_ops.LAUNCHES)
        out = layer(bg, xx)
        launched = readout_ops.LAUNCHES["seed_readout"] - before.get("seed_readout", 0)
        out.backward(cot.to(out.dtype))
        return launched, [out.detach(), xx.grad] + [p.grad.clone() for p in layer.parameters()]

    assert layer.fused and layer._takes_fused(bg, layer.lin1(x))
    n_fused, fused = step(x)
    layer.fused = False
    n_plain, plain = step(x)
    layer.fused = True
    assert (n_fused, n_plain) == (2, 0)                     # GMPool_G and GMPool_I; SelfAtt stays dense
    layer.double()
    assert step(x.double())[0] == 0                         # an fp64 input runs the unfused code
    names = ["out", "d x"] + [n for n, _ in layer.named_parameters()]
    for name, a, b in zip(names, fused, plain):
        assert bool(((a - b).abs() <= 5e-5 * b.abs().max() + 1e-6).all()), (name, float((a - b).abs().max()), float(b.abs().max()))
