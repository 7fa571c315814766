"""The fused edge-feature messages (pgl_amd/csrc/edge_message.hip, pgl_amd.message_ops, Graph.send_edge_message, nn.GINEConv / GENConv)
on the MI355X, held element by element to the fp64 restatement below of the definition in message_ops' module text.

Bars (none comes from the kernel), per element:
  sum with relu     the fp32 re-association bar n eps sum |terms| of the definition's own sums (gpu_common).  The inputs lie on a grid
                    (multiples of 1/4, feature 0's table or ef shifted by 1/8) on which pre is exact and at least 1/8 from zero, so the
                    relu mask cannot differ between fp32 and fp64 and no element is left out.
  softmax, swish    the fp32 torch composition of the same definition is evaluated on the same inputs; the kernel is allowed 4 x its
                    per-element distance from fp64 plus the re-association bar of the outer sums (the rule of test_kge_gpu.py).
Terms (|m_k| stands for |act(pre_k)| + eps): out: the (softmax-weighted) |m_k| of a row, n = in-degree + F + 2.  d pre_k: |g| a_k (1 + t (|m_k| + sum_j a_j |m_j|)) act'_abs, which
cannot cancel, with n_k = F + 2 roundings of its own (swish: F + 8, the chain through exp, the reciprocal and swish' two parts) plus, for the softmax, the in-degree of its destination (a_k and out[v] are sums over
that row); d ef is that, d x and d table the sums of those terms times (n_k + how many are summed); d t: every |g| a |m| (|m| + sum a |m|),
n = E d + E.  Observed maxima: profiles/edge_message/README.md."""
import numpy as np
import pytest
import torch

from gpu_common import pgl, check_grad_elements, reassociation_bound, RTOL  # noqa: F401  (pgl: the fixture)

pytestmark = pytest.mark.gpu

VOCABS = {"coded3": (5, 6, 2), "coded1": (7,)}


def make_graph(kind):
    gen = torch.Generator().manual_seed(5)
    if kind == "empty":
        return 5, torch.zeros((0, 2), dtype=torch.int64)
    if kind == "mol":                                   # in-degree <= 4; the nodes 30 .. 39 are isolated
        dst = torch.arange(90) % 30
        return 40, torch.stack([torch.randint(0, 30, (90,), generator=gen), dst], 1)[torch.randperm(90, generator=gen)]
    # hub: 5000 edges into node 7 and 600 into node 11 (at 64 edges a chunk: more than kFixShort pieces, and fewer); out of node 7 2600
    # edges and out of node 11 600, for the backward's walk by source
    src, dst = torch.randint(0, 300, (6000,), generator=gen), torch.randint(0, 300, (6000,), generator=gen)
    dst[:5000], dst[5000:5600], src[3000:5600], src[:600] = 7, 11, 7, 11
    return 300, torch.stack([src, dst], 1)[torch.randperm(6000, generator=gen)]


def make_inputs(n, E, d, source, act, seed):
    """-> x, ef or None, codes or None, tables or None (fp32, host).  relu: the exact grid; swish: normal draws."""
    gen = torch.Generator().manual_seed(seed)
    draw = (lambda *s: torch.randint(-8, 9, s, generator=gen).float() / 4) if act == "relu" else (lambda *s: torch.randn(*s, generator=gen))
    shift = 0.125 if act == "relu" else 0.0
    x = draw(n, d)
    if source == "dense":
        return x, draw(E, d) + shift, None, None
    vocab = VOCABS.get(source, (20,))
    tables = [draw(v, d) + (shift if f == 0 else 0.0) for f, v in enumerate(vocab)]
    codes = torch.stack([torch.randint(0, v - 1, (E,), generator=gen) for v in vocab], 1).int()       # the last row of each: nobody's
    return x, None, codes, tables


def definition(x, ef, codes, tables, edges, n, act, reduce, eps, t, cot):
    """The definition in x's dtype with autograd -> dict of out, the gradients and the per-edge terms the bars are made of."""
    src, dst = edges[:, 0], edges[:, 1]
    leaves = [v.clone().requires_grad_(True) for v in ([x, ef] if tables is None else [x] + list(tables))]
    tt = torch.tensor([t], dtype=x.dtype, requires_grad=True)
    e = leaves[1]
    if tables is not None:
        e = leaves[1][codes[:, 0].long()]
        for f in range(1, len(tables)):
            e = e + leaves[1 + f][codes[:, f].long()]
    pre = leaves[0][src] + e
    pre.retain_grad()
    m = (torch.relu(pre) if act == "relu" else pre * torch.sigmoid(pre)) + eps
    seg = lambda v: torch.zeros((n, x.shape[1]), dtype=x.dtype).index_add_(0, dst, v)
    a = torch.ones_like(m)
    if reduce == "softmax" and len(src):
        l = tt * m
        mx = torch.full((n, x.shape[1]), -np.inf, dtype=x.dtype).scatter_reduce_(0, dst[:, None].expand_as(l), l.detach(), "amax")
        w = torch.exp(l - mx[dst])
        a = w / seg(w)[dst]
    out = seg(a * m)
    # what an edge's d pre_k is made of, without cancellation: |g| a (1 + t (|m| + sum a |m|)) |act'|, and its own term count n_k
    m_abs = (m.detach() - eps).abs() + eps                 # m_k = act(pre_k) + eps can cancel: its two terms, added
    out_abs = seg(a.detach() * m_abs)
    sg = torch.sigmoid(pre.detach())
    slope = (pre.detach() > 0).to(x.dtype) if act == "relu" else sg * (1.0 + pre.detach().abs() * (1.0 - sg))    # (swish': its two parts added)
    indeg = torch.zeros(n, 1, dtype=x.dtype).index_add_(0, dst, torch.ones(len(src), 1, dtype=x.dtype))
    soft = float(reduce == "softmax")
    g_abs = (cot.to(x.dtype)[dst] * a).detach().abs()
    (out * cot.to(x.dtype)).sum().backward()
    r = dict(out=out.detach(), dx=leaves[0].grad, de=torch.cat([v.grad for v in leaves[1:]]), dt=tt.grad, pre=pre.detach(), out_abs=out_abs,
             dpre_abs=g_abs * (1.0 + soft * t * (m_abs + out_abs[dst])) * slope, n_k=soft * indeg[dst] + len(leaves) + (1 if act == "relu" else 7))
    r["dt_abs"] = (g_abs * m_abs * (m_abs + out_abs[dst])).sum().reshape(1)
    return {k: (torch.zeros_like(tt) if v is None else v) for k, v in r.items()}


CASES = [(g, d) for g in ("empty", "mol", "hub") for d in (1, 100, 260, 1024) if not (g == "hub" and d == 1024)]


def run(pgl, kind, d, source, act, reduce, t=0.7, eps=0.05):
    n, edges = make_graph(kind)
    x, ef, codes, tables = make_inputs(n, edges.shape[0], d, source, act, seed=3 * d + len(source))
    cot = torch.randn(n, d, generator=torch.Generator().manual_seed(d))
    g = pgl.Graph(edges=edges.cuda(), num_nodes=n).tensor()
    leaves = [v.cuda().requires_grad_(True) for v in ([x, ef] if tables is None else [x] + tables)]
    tt = torch.tensor([t], device="cuda", requires_grad=True)
    out = g.send_edge_message(leaves[0], edge_feat=leaves[1] if tables is None else None, edge_codes=None if codes is None else codes.cuda(),
                              edge_tables=None if tables is None else leaves[1:], act=act, reduce_op=reduce, eps=eps, temperature=tt)
    (out * cot.cuda()).sum().backward()
    got = dict(out=out.detach(), dx=leaves[0].grad, de=torch.cat([v.grad for v in leaves[1:]]),
               dt=tt.grad if tt.grad is not None else torch.zeros(1))
    args = (codes, tables, edges, n, act, reduce, eps, t, cot)
    return {k: v.cpu() for k, v in got.items()}, args, (x, ef)


@pytest.mark.parametrize("kind,d", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("source", ["dense", "coded3", "coded1"])
@pytest.mark.parametrize("act", ["relu", "swish"])
@pytest.mark.parametrize("reduce", ["sum", "softmax"])
def test_parity(pgl, reduce, act, source, kind, d):
    got, args, (x, ef) = run(pgl, kind, d, source, act, reduce)
    check(got, args, x, ef, exact_grid=(reduce == "sum" and act == "relu"), tag="%s %s %s %s d=%d" % (reduce, act, source, kind, d))


def check(got, args, x, ef, exact_grid, tag):
    codes, tables, edges, n, act, reduce = args[:6]
    dbl = lambda v: None if v is None else ([u.double() for u in v] if isinstance(v, list) else v.double())
    w = definition(dbl(x), dbl(ef), codes, dbl(tables), *args[2:])
    src, dst, E, d = edges[:, 0], edges[:, 1], edges.shape[0], x.shape[1]
    F = 1 if tables is None else len(tables)
    if act == "relu" and E:
        assert float(w["pre"].abs().min()) >= 0.125                    # the mask is the same in fp32 and fp64
    ones = torch.ones(E, 1, dtype=torch.float64)
    by = lambda ids, v, rows: torch.zeros((rows, v.shape[1]), dtype=torch.float64).index_add_(0, ids, v)
    one = torch.ones(1, 1, dtype=torch.float64)
    # a sum of c terms, term k carrying n_k roundings of its own: sum_k |term_k| (c + n_k), as one "term" of the bar
    summed = lambda ids, rows: by(ids, w["dpre_abs"].repeat(len(ids) // max(E, 1), 1) * w["n_k"].repeat(len(ids) // max(E, 1), 1), rows) + \
        by(ids, w["dpre_abs"].repeat(len(ids) // max(E, 1), 1), rows) * by(ids, ones.repeat(len(ids) // max(E, 1), 1), rows)
    if tables is None:
        de_abs = w["dpre_abs"] * w["n_k"]
    else:
        off = np.cumsum([0] + [int(v.shape[0]) for v in tables])
        rows = torch.cat([codes[:, f].long() + int(off[f]) for f in range(F)])
        de_abs = summed(rows, int(off[-1]))
        unused = [int(o) - 1 for o in off[1:]]
        assert not bool(got["de"][unused].view(torch.int32).any())     # rows nobody uses: exactly +0.0
    terms = dict(out=(w["out_abs"], by(dst, ones, n) + F + 2), dx=(summed(src, n), one), de=(de_abs, one),
                 dt=(w["dt_abs"], torch.tensor([float(E * d + E)], dtype=torch.float64)))
    empty = by(dst, ones, n)[:, 0] == 0
    assert not bool(got["out"][empty].view(torch.int32).any())         # rows without in-edges: exactly +0.0
    c32 = None if exact_grid else definition(x, ef, codes, tables, *args[2:])
    for k in ("out", "dx", "de", "dt"):
        if k == "dt" and reduce == "sum":
            continue
        ab, nt = terms[k]
        if exact_grid:
            check_grad_elements(got[k], w[k], ab, nt, what=tag + " " + k)
            continue
        f = lambda v: v.detach().double().numpy()
        bar = 4.0 * np.abs(f(c32[k]) - f(w[k])) + reassociation_bound(f(ab), f(nt))
        err = np.abs(f(got[k]) - f(w[k]))
        print("edge_message %s %s: max err %.3e, fp32 composition %.3e, max err / bar %.2f"
              % (tag, k, err.max(initial=0.0), np.abs(f(c32[k]) - f(w[k])).max(initial=0.0), (err / bar).max(initial=0.0)))
        assert (err <= bar).all(), (tag, k, float((err / bar).max()))


def test_wide_table_takes_the_fallback(pgl):
    """A table of 20 rows at d = 260 is beyond edge_message_supported: the same answer from the composition."""
    from pgl_amd import message_ops
    assert not message_ops.edge_message_supported(260, 20) and message_ops.edge_message_supported(600, 13)
    got, args, (x, ef) = run(pgl, "mol", 260, "wide", "swish", "softmax")
    check(got, args, x, ef, exact_grid=False, tag="fallback")


@pytest.mark.parametrize("reduce,act,source", [("sum", "relu", "coded3"), ("softmax", "swish", "dense"), ("softmax", "swish", "coded3")])
def test_two_calls_same_bits(pgl, reduce, act, source):
    first, again = run(pgl, "hub", 100, source, act, reduce)[0], run(pgl, "hub", 100, source, act, reduce)[0]
    assert all(bool((first[k].view(torch.int32) == again[k].view(torch.int32)).all()) for k in first)


@pytest.mark.parametrize("layer", ["gine", "gen"])
def test_layers_fused_against_composition(pgl, layer):
    """fused=True against the fused=False layer with the same parameters: outputs and parameter gradients, 4 x the distance of the fp32
    composition from its fp64 self plus gpu_common's bar for composite results (close_rows: RTOL of the element and of its row's largest)."""
    n, edges = make_graph("mol")
    d = 100
    torch.manual_seed(1)
    make = (lambda fused: pgl.nn.GINEConv(d, d, edge_vocab=(5, 6, 2), train_eps=True, fused=fused)) if layer == "gine" else \
           (lambda fused: pgl.nn.GENConv(d, edge_vocab=(5, 6, 2), learn_t=True, fused=fused))
    ref = make(False)
    x, _, codes, _ = make_inputs(n, 90, d, "coded3", "swish", seed=9)
    res = {}
    for name, fused, dt, dev in (("fused", True, torch.float32, "cuda"), ("c32", False, torch.float32, "cpu"), ("c64", False, torch.float64, "cpu")):
        m = make(fused)
        m.load_state_dict(ref.state_dict())
        m = m.to(dev).to(dt)
        g = pgl.Graph(edges=edges.cuda() if dev == "cuda" else edges.numpy(), num_nodes=n)
        out = m(g, x.to(dev).to(dt), codes.to(dev))
        out.square().sum().backward()
        res[name] = [out.detach().cpu().double().numpy()] + [p.grad.cpu().double().numpy() for p in m.parameters()]
    # (close_rows' `cancel`: the bias ahead of a BatchNorm has an analytically zero gradient, a column sum of terms of the size of the
    #  other parameter gradients -- the largest of them is the magnitude handed in for every parameter gradient)
    scale = max(float(np.abs(c).max()) for c in res["c64"][1:])
    for i, (got, c32, c64) in enumerate(zip(res["fused"], res["c32"], res["c64"])):
        row = np.abs(c64).reshape(c64.shape[0], -1).max(1).reshape((-1,) + (1,) * (c64.ndim - 1))
        bar = 4.0 * np.abs(c32 - c64) + RTOL * (np.abs(c64) + row + (scale if i else 0.0))
        assert (np.abs(got - c64) <= bar).all(), (layer, float((np.abs(got - c64) / bar).max()))


@pytest.mark.parametrize("what", ["fp64", "code >= vocabulary", "F = 5", "d = 1025", "ef rows"])
def test_refusals_before_any_launch(pgl, what, monkeypatch):
    from pgl_amd import message_ops as M
    launches = []
    monkeypatch.setattr(M, "_launch", lambda *a, **k: launches.append(a))
    n, edges = make_graph("mol")
    csr = pgl.Graph(edges=edges.cuda(), num_nodes=n).tensor()._csr_dst()
    d = 1025 if what == "d = 1025" else 8
    x = torch.zeros(n, d, device="cuda", dtype=torch.float64 if what == "fp64" else torch.float32)
    kw = dict(ef=torch.zeros(89 if what == "ef rows" else 90, d, device="cuda", dtype=x.dtype))
    if what in ("code >= vocabulary", "F = 5"):
        F = 5 if what == "F = 5" else 2
        codes = torch.zeros(90, F, dtype=torch.int32, device="cuda")
        codes[17, 1] = 3 if what == "code >= vocabulary" else 0
        kw = dict(codes=codes, table=torch.zeros(3 * F, d, device="cuda"), offsets=[3 * f for f in range(F)], sizes=[3] * F)
    with pytest.raises((ValueError, TypeError)):
        M.edge_message_aggregate(x, csr, **kw)
    assert not launches and not M.edge_message_supported(1025) and M.edge_message_supported(1) and M.edge_message_supported(1024)
