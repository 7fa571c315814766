"""The set-attention op (pgl_amd/csrc/set_attention.hip, pgl_amd.readout_ops.set_attention) and SAB / GraphMultisetTransformer on it, on
the MI355X.  out, dq, dk and dv are held to the three-line definition below evaluated in fp64, within
8 * max(max|def32 - def64|, eps32 * max|def64|): both terms come from the host definition, never from the kernel; the 8 is the allowance
of tests/test_seed_readout_gpu.py for a summation order other than torch's (here MFMA accumulation and key order).  In the key_bias
cases the fp32 definition itself departs from fp64 (-1e9 swallows the score in fp32 only), which the bar measures and follows.
Largest ratio |got - def64| / (the bar / 8) measured on the MI355X: 1.20 (dk at (2, 75, 75, 64, 1);
profiles/set_attention/README.md)."""
import math

import numpy as np
import pytest
import torch

from gpu_common import pgl  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1, 4, 1), (5, 7, 7, 32, 4), (3, 32, 32, 128, 4), (3, 33, 33, 128, 4), (2, 8, 100, 64, 8), (2, 100, 8, 64, 8),
         (2, 128, 128, 256, 4), (2, 75, 75, 64, 1)]                                         # (B, nq, nk, dim, heads)
EPS32 = float(np.finfo(np.float32).eps)


def definition(q, k, v, heads, key_bias=None, residual=True):
    B, nq, dim = q.shape
    qh, kh, vh = (t.reshape(B, t.shape[1], heads, dim // heads) for t in (q, k, v))
    s = torch.einsum("bihc,bjhc->bijh", qh, kh) / math.sqrt(dim) + (0 if key_bias is None else key_bias[:, None, :, None])
    return float(residual) * q + torch.einsum("bijh,bjhc->bihc", torch.softmax(s, dim=1), vh).reshape(B, nq, dim)


def evaluate(dtype, q, k, v, cot, heads, key_bias=None):
    xs = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (q, k, v)]
    out = definition(xs[0], xs[1], xs[2], heads, None if key_bias is None else key_bias.cpu().to(dtype))
    out.backward(cot.cpu().to(dtype))
    return [out.detach()] + [t.grad for t in xs]


def inputs(B, nq, nk, dim, with_bias=False):
    gen = torch.Generator().manual_seed(1000 * nq + nk + dim)
    q, k, v, cot = (torch.randn(shape, generator=gen).cuda() for shape in ((B, nq, dim), (B, nk, dim), (B, nk, dim), (B, nq, dim)))
    bias = None
    if with_bias:       # -1e9 on a first column, a last one, one on a tile edge and the whole key set of the last graph
        bias = torch.zeros(B, nk, device="cuda")
        bias[0, 0] = bias[0, nk - 1] = bias[0, min(32, nk - 1)] = -1e9
        bias[B - 1, :] = -1e9
    return q, k, v, cot, bias


def run(q, k, v, cot, heads, key_bias=None, need=(True, True, True), residual=True):
    from pgl_amd import readout_ops
    xs = [t.detach().requires_grad_(bool(n)) for t, n in zip((q, k, v), need)]
    out = readout_ops.set_attention(xs[0], xs[1], xs[2], heads, key_bias=key_bias, residual=residual)
    if any(need):
        out.backward(cot)
    return [out.detach()] + [t.grad for t in xs]


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "key_bias"])
@pytest.mark.parametrize("B,nq,nk,dim,heads", CASES)
def test_definition(pgl, B, nq, nk, dim, heads, with_bias):
    from pgl_amd import readout_ops
    q, k, v, cot, bias = inputs(B, nq, nk, dim, with_bias)
    before = dict(readout_ops.LAUNCHES)
    got = run(q, k, v, cot, heads, bias)
    assert readout_ops.LAUNCHES["set_attention"] == before.get("set_attention", 0) + 1
    assert readout_ops.LAUNCHES["set_attention_backward"] == before.get("set_attention_backward", 0) + 1
    d64, d32 = evaluate(torch.float64, q, k, v, cot, heads, bias), evaluate(torch.float32, q, k, v, cot, heads, bias)
    ratios = {}
    for name, g, w64, w32 in zip(("out", "dq", "dk", "dv"), got, d64, d32):
        unit = max(float((w32.double() - w64).abs().max()), EPS32 * float(w64.abs().max()))
        err = float((g.cpu().double() - w64).abs().max())
        ratios[name] = err / unit if unit > 0.0 else (0.0 if err == 0.0 else float("inf"))       # (one query: dk is exactly 0)
    print("set_attention %s bias=%s: |got - def64| / unit = %s" % ((B, nq, nk, dim, heads), with_bias, ", ".join("%s %.2f" % kv for kv in ratios.items())))
    assert all(r <= 8.0 for r in ratios.values()), ratios


def test_bits(pgl):
    """The same call twice; every subset of the gradients; residual=False; one query; a misaligned view and a non-contiguous q."""
    q, k, v, cot, bias = inputs(3, 33, 70, 128, True)
    first = run(q, k, v, cot, 4, bias)
    assert all(same_bits(a, b) for a, b in zip(first, run(q, k, v, cot, 4, bias)))
    for need in [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)][1:]:
        part = run(q, k, v, cot, 4, bias, need=need)
        assert same_bits(part[0], first[0])
        for n, a, b in zip(need, part[1:], first[1:]):
            assert (a is None) if not n else same_bits(a, b), need
    plain = run(q, k, v, cot, 4, bias, residual=False)                 # out = A V: the residual is one fp32 add at the store
    assert same_bits(q + plain[0], first[0]) and all(same_bits(a, b) for a, b in zip(plain[2:], first[2:]))
    q1, k1, v1, cot1, _ = inputs(2, 1, 1, 32)
    one = run(q1, k1, v1, cot1, 4)                                     # one query: A is exactly 1, ds exactly 0
    assert same_bits(one[0], q1 + v1) and not bool(one[2].any()) and same_bits(one[3], cot1)
    shifted = [torch.cat([t.new_zeros(1), t.flatten()])[1:].view(t.shape) for t in (q, k, v)]
    assert shifted[0].data_ptr() % 16 != 0
    assert all(same_bits(a, b) for a, b in zip(run(*shifted, cot, 4, bias), first))
    strided = q.transpose(0, 1).contiguous().transpose(0, 1)
    assert not strided.is_contiguous()
    assert all(same_bits(a, b) for a, b in zip(run(strided, k, v, cot, 4, bias), first))


@pytest.mark.parametrize("what", ["nq = 129", "nk = 129", "dim = 260", "hd = 12", "cpu", "k != v", "key_bias"])
def test_refusals(pgl, what):
    from pgl_amd import readout_ops
    nq, nk, dim, heads = {"nq = 129": (129, 9, 32, 4), "nk = 129": (9, 129, 32, 4), "dim = 260": (9, 9, 260, 5),
                          "hd = 12": (9, 9, 48, 4)}.get(what, (9, 9, 32, 4))
    assert readout_ops.set_attention_supported(nq, nk, dim, heads) == (what in ("cpu", "k != v", "key_bias"))
    dev = "cpu" if what == "cpu" else "cuda"
    q, k, v = torch.randn(2, nq, dim, device=dev), torch.randn(2, nk, dim, device=dev), torch.randn(2, nk + (what == "k != v"), dim, device=dev)
    bias = torch.zeros(2, nk + 1, device=dev) if what == "key_bias" else None
    before = dict(readout_ops.LAUNCHES)
    with pytest.raises(ValueError):
        readout_ops.set_attention(q, k, v, heads, key_bias=bias)
    assert dict(readout_ops.LAUNCHES) == before


def compare(step, switch, names):
    """step() -> (launch counts, tensors) with the flags on, then off after switch(); the tensors within 5e-5 * max|unfused| + 1e-6."""
    n_on, on = step()
    switch()
    n_off, off = step()
    for name, a, b in zip(names, on, off):
        assert bool(((a - b).abs() <= 5e-5 * b.abs().max() + 1e-6).all()), (name, float((a - b).abs().max()), float(b.abs().max()))
    return n_on, n_off


@pytest.mark.parametrize("with_mask", [False, True], ids=["plain", "mask"])
def test_sab_against_its_unfused_self(pgl, with_mask):
    from pgl_amd import readout_ops
    from pgl_amd.nn.gmt_pool import SAB
    torch.manual_seed(0)
    layer = SAB(32, 32, 4, fused=True).cuda()
    x, cot = torch.randn(6, 9, 32, device="cuda"), torch.randn(6, 9, 32, device="cuda")
    x[2, 5:] = 0.0
    mask = (x.sum(-1) == 0).to(torch.int64).unsqueeze(0) * -1e9 if with_mask else None

    def step():
        layer.zero_grad()
        xx = x.detach().requires_grad_(True)
        before = readout_ops.LAUNCHES["set_attention"]
        out = layer(xx, None, mask)
        out.backward(cot)
        return readout_ops.LAUNCHES["set_attention"] - before, [out.detach(), xx.grad] + [p.grad.clone() for p in layer.parameters()]

    assert compare(step, lambda: setattr(layer, "fused", False), ["out", "d x"] + [n for n, _ in layer.named_parameters()]) == (1, 0)


def test_layer_against_its_unfused_self(pgl):
    """GraphMultisetTransformer(fused=True, fused_self_att=True) against the same parameters with both flags off on the batch of
    tests/test_seed_readout_gpu.py (1 / 7 / 30 / 300 nodes), and the routing of the two flags."""
    from pgl_amd import readout_ops
    rng = np.random.default_rng(3)
    bg = pgl.Graph.disjoint([pgl.Graph(edges=rng.integers(0, m, (3 * m, 2)).astype(np.int64), num_nodes=m) for m in (1, 7, 30, 300)])
    bg.tensor()
    torch.manual_seed(0)
    layer = pgl.nn.GraphMultisetTransformer(16, 32, 8, num_nodes=30, fused=True, fused_self_att=True).cuda()
    with torch.no_grad():
        layer.lin1.bias.zero_()                              # (that test's setup: with x[11] = 0 the -1e9 branch runs on a real node)
    x = torch.randn(338, 16, device="cuda")
    x[11] = 0.0
    cot = torch.randn(4, 8, device="cuda")

    def step(xx=x):
        layer.zero_grad()
        xx = xx.detach().requires_grad_(True)
        before = dict(readout_ops.LAUNCHES)
        out = layer(bg, xx)
        out.backward(cot.to(out.dtype))
        return (tuple(readout_ops.LAUNCHES[n] - before.get(n, 0) for n in ("set_attention", "seed_readout")),
                [out.detach(), xx.grad] + [p.grad.clone() for p in layer.parameters()])

    def off():
        layer.fused = layer.fused_self_att = False

    assert layer.fused and layer.fused_self_att
    assert compare(step, off, ["out", "d x"] + [n for n, _ in layer.named_parameters()]) == ((1, 2), (0, 0))
    layer.fused = True
    assert step()[0] == (0, 2)                               # fused alone: the pooling blocks only
    layer.fused_self_att = True
    layer.double()
    assert step(x.double())[0] == (0, 0)                     # an fp64 module runs the unfused code


def test_graph_replay(pgl):
    """Forward + backward of the op captured once in a torch.cuda.graph replays to the eager bits, several times."""
    q, k, v, cot, bias = inputs(3, 33, 33, 128, True)
    eager = run(q, k, v, cot, 4, bias)
    qs, ks, vs = (torch.zeros_like(t).requires_grad_(True) for t in (q, k, v))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(q, k, v, cot, 4, bias)
    torch.cuda.current_stream().wait_stream(side)
    from pgl_amd import readout_ops
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = readout_ops.set_attention(qs, ks, vs, 4, key_bias=bias)
        grads = torch.autograd.grad(out, (qs, ks, vs), cot)
    with torch.no_grad():
        for dst, src in zip((qs, ks, vs), (q, k, v)):
            dst.copy_(src)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip([out.detach()] + list(grads), eager))
