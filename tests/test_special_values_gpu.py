"""NaN, +-inf, subnormals and integer wrap-around through every kernel family on the MI355X (DESIGN.md "Special values").

The definition is the fp64 restatement of each op evaluated with IEEE semantics (tests/special_defs.py); per output element the class
(NaN / +inf / -inf / finite) must match exactly and a finite element must lie inside its existing bound WITHOUT an absolute floor
(special_defs.classify_and_check).  All ids are in range: the special values are data only, nothing here can fault a kernel.

Families: aggregation at every width and storage type and through every path (two tables, column blocks, accumulate, out_size,
segment_reduce, raw indices, the hub table), edge operands that produce the values, segment / edge softmax forward and backward, the
fused GAT with masked sources, the fused layer forms against their unfused compositions, casts and 16-bit stores, subnormals, integers.
"""
import numpy as np
import pytest
import torch

import ref_ops as R
import special_defs as S
from special_defs import NAN, INF
from gpu_common import pgl, dev, host, _dense_gat_fp64  # noqa: F401  (pgl: the fixture)

pytestmark = pytest.mark.gpu

OPS = ["sum", "mean", "max", "min"]
F16, BF16 = torch.float16, torch.bfloat16
DT_NAME = {np.float32: "fp32", np.float64: "fp64", F16: "fp16", BF16: "bf16", np.int32: "i32", np.int64: "i64"}


def to_dev(x):
    return x.cuda() if isinstance(x, torch.Tensor) else dev(x)


def to_np(t):
    t = t.detach()
    return (t.float() if t.dtype in (F16, BF16) else t).cpu().numpy()


@pytest.fixture(scope="module")
def SG(pgl):
    G = S.SpecialGraph(0)
    g = pgl.Graph(edges=G.edges, num_nodes=G.n).tensor()
    return G, g, S.planted_cases(G)


class Collect(object):
    """Runs every case of a test and reports ALL that fail (one line each), so that one parametrised test names each failing case."""

    def __init__(self):
        self.fails, self.n = [], 0

    def check(self, got, want, bound, what):
        self.n += 1
        try:
            S.classify_and_check(got, want, bound, what)
        except AssertionError as e:
            self.fails.append(str(e))

    def done(self):
        assert not self.fails, "%d of %d cases:\n%s" % (len(self.fails), self.n, "\n".join(self.fails))


# ------------------------------------------------------------------------------------------------
# aggregation: every kernel (narrow d <= 16, grouped 17..32, flat beyond), every storage type, every planted case
# ------------------------------------------------------------------------------------------------
AGG = [(np.float32, d) for d in (1, 8, 16, 17, 32, 33, 64, 128, 130, 256)] + [(np.float64, d) for d in (1, 8, 9, 16, 17, 32, 33, 130)] + \
      [(t, d) for t in (F16, BF16) for d in (8, 16, 33, 64, 130, 256)]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype,d", AGG, ids=["%s-%d" % (DT_NAME[t], d) for t, d in AGG])
def test_aggregate_special_values(SG, op, dtype, d):
    G, g, cases = SG
    x = G.features(d, dtype)
    C = Collect()
    for name, pl in cases.items():
        xp = S.plant(G, x, pl)
        want, bound = S.expect(G, xp, op)
        got = g.send_recv(to_dev(xp), op)
        C.check(to_np(got), want, bound, "%s %s %s d=%d" % (name, op, DT_NAME[dtype], d))
        assert (to_np(got)[list(S.EMPTY_ROWS)] == 0).all()                       # a row without edges stays 0
    C.done()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("d", [8, 20, 130])
def test_aggregate_paths(pgl, SG, op, d):
    """The two-table path (the planted values live in the SECOND table), column-block views, accumulate 1 and 2 over old contents
    holding NaN and inf, out_size beyond the nodes, segment_reduce with int32 and int64 ids, ops.send_u_recv on raw indices (d = 8:
    below its atomic crossover for sum, d = 130: above)."""
    G, g, cases = SG
    ops, csr = pgl.ops, g.adj_dst_index.csr
    x = G.features(d)
    has = (G.indeg > 0)[:, None]
    rng = np.random.default_rng(9)
    old = rng.standard_normal((G.n, d)).astype(np.float32)
    old[[0, 5, 11, 13, 25, 401]] = NAN
    old[[3, 8, 14, 26, 402]] = INF
    old[[9, 15, 27]] = -INF
    order = np.argsort(G.dst, kind="stable")
    C = Collect()
    for name in ("nan", "pinf", "inf_and_minus_inf", "all_nan_rows", "all_ninf_rows"):
        xp = S.plant(G, x, cases[name])
        want, bound = S.expect(G, xp, op)
        w = "%s %s d=%d" % (name, op, d)
        xd = to_dev(xp)
        # x2: rows >= N_GENERIC (every carrier) are read from the second table
        got = ops.aggregate(xd[:S.N_GENERIC].contiguous(), csr, op, out_size=G.n, x2=xd[S.N_GENERIC:].contiguous())
        C.check(to_np(got), want, bound, w + " two tables")
        # column blocks of wider matrices, in and out
        big = torch.full((G.n, 3 * d), 7.0, device="cuda"); big[:, d:2 * d] = xd
        outb = torch.full((G.n, 3 * d + 1), 5.0, device="cuda")
        ops.aggregate(big[:, d:2 * d], csr, op, out=outb[:, d:2 * d])
        C.check(to_np(outb[:, d:2 * d]), want, bound, w + " column blocks")
        assert bool((outb[:, :d] == 5).all()) and bool((outb[:, 2 * d:] == 5).all())
        # accumulate
        with np.errstate(invalid="ignore"):
            comb = {"sum": old.astype(np.float64) + want, "mean": old.astype(np.float64) + want,
                    "max": np.maximum(old, want), "min": np.minimum(old, want)}[op]
            b1 = bound if op in ("max", "min") else bound + S.EPS32 * np.abs(comb)
        o1 = dev(old)
        if op == "mean":                                                         # (the library defines no accumulating mean)
            with pytest.raises(ValueError, match="accumulate with MEAN"):
                ops.aggregate(xd, csr, op, out=o1, accumulate=1)
        else:
            ops.aggregate(xd, csr, op, out=o1, accumulate=1)
            C.check(to_np(o1), np.where(has, comb, old), np.where(has, b1, 0.0), w + " accumulate=1")
        if op != "mean":
            o2 = dev(old); ops.aggregate(xd, csr, op, out=o2, accumulate=2)
            C.check(to_np(o2), np.where(has, want, old), np.where(has, bound, 0.0), w + " accumulate=2")
        # out_size beyond the nodes
        wantL, boundL = S.expect(G, xp, op, out_size=G.n + 37)
        C.check(to_np(g.send_recv(xd, op, out_size=G.n + 37)), wantL, boundL, w + " out_size")
        # segment_reduce over the destination-sorted messages
        data, ids = xp[G.src[order]], G.dst[order]
        n_seg = int(ids[-1]) + 1
        with np.errstate(invalid="ignore"):
            assert np.array_equal(R.np_segment(data.astype(np.float64), ids, op), want[:n_seg], equal_nan=True)
        for idt in (np.int32, np.int64):
            got = ops.segment_reduce(dev(data), dev(ids.astype(idt)), op)
            C.check(to_np(got), want[:n_seg], bound[:n_seg], w + " segment_reduce %s ids" % DT_NAME[idt])
        # raw indices
        got = ops.send_u_recv(xd, dev(G.src), dev(G.dst), op)
        C.check(to_np(got), want, bound, w + " ops.send_u_recv")
    assert (G.E * 8 <= ops._COO_ONCE_MAX < G.E * 130)                              # d = 8 / 130 sit on either side of the crossover
    C.done()


@pytest.mark.parametrize("op", OPS)
def test_hub_table_path(pgl, monkeypatch, op):
    """The hub-table path (ops.hub_plan): the top out-degree sources packed into a second table per call.  NaN / inf planted in hub
    sources and in ordinary ones."""
    ops = pgl.ops
    rng = np.random.default_rng(4)
    n, e, d = 16384, 300000, 128
    src = np.where(rng.random(e) < 0.6, rng.integers(0, 1500, e), rng.integers(0, n, e)).astype(np.int64)
    dst = rng.integers(0, n - 100, e).astype(np.int64)
    dst[:20000] = 77
    g = pgl.Graph(edges=np.stack([src, dst], 1), num_nodes=n).tensor()
    csr = g.adj_dst_index.csr
    monkeypatch.setattr(ops, "_HUB_TABLE", True)
    monkeypatch.setattr(ops, "_HUB_MIN_EDGES", 0)
    x = rng.standard_normal((n, d)).astype(np.float32)
    C = Collect()
    for name, v in (("nan", NAN), ("pinf", INF), ("ninf", -INF)):
        xp = x.copy()
        xp[[3, 700, 1499], 0] = v                      # hub sources (one column)
        xp[[5000, 16000]] = v                          # ordinary sources (whole rows)
        x64 = xp.astype(np.float64)
        with np.errstate(invalid="ignore"):
            want = R.np_send_u_recv(x64, src, dst, op)
            absx = R.np_send_u_recv(np.abs(x64), src, dst, op if op == "mean" else "sum")
        bound = 0.0 if op in ("max", "min") else S.rebound(absx, np.bincount(dst, minlength=n)[:, None] + 1.0)
        got = ops.aggregate(dev(xp), csr, op, n)
        C.check(to_np(got), want, bound, "hub table %s %s" % (name, op))
    plan = next(iter(csr._hub.values()))
    assert plan is not None and int((plan[1] >= n).sum()) > 0                      # the table was in use
    C.done()


# ------------------------------------------------------------------------------------------------
# edge operands: message ops that PRODUCE the special value
# ------------------------------------------------------------------------------------------------
PRODUCERS = [("mul", 0.0, INF), ("mul", INF, 0.0), ("sub", INF, INF), ("add", INF, -INF), ("div", 1.0, 0.0), ("div", -1.0, 0.0), ("div", 0.0, 0.0),
             ("div", INF, INF), ("add", NAN, 1.0), ("mul", 1.0, NAN)]


@pytest.mark.parametrize("rop", ["sum", "max"])
@pytest.mark.parametrize("shape", ["E", "E1-8", "Ed-8", "E1-130", "Ed-130"])
def test_edge_operand_produces_special_values(SG, rop, shape):
    G, g, _ = SG
    rng = np.random.default_rng(12)
    d = 1 if shape == "E" else int(shape.split("-")[1])
    xshape = (G.n,) if shape == "E" else (G.n, d)
    yshape = (G.E,) if shape == "E" else (G.E, 1) if shape.startswith("E1") else (G.E, d)
    slots = [(0, 0), (5, 0), (8, 256), (10, S.resolve(G, 10, "late")), (11, 0), (11, S.resolve(G, 11, "late")), (11, S.ROW_LENS[11] - 1)]
    C = Collect()
    for mop, xv, yv in PRODUCERS:
        x = rng.standard_normal(xshape).astype(np.float32)
        y = (rng.standard_normal(yshape) + 3.0).astype(np.float32)                  # (divisors away from 0)
        for r, p in slots:
            x[G.carrier[(r, p)]] = xv
            y[G.edge_of[(r, p)]] = yv
        want, bound = S.expect(G, x, rop, y=y, mop=mop)
        assert rop == "max" or all(not np.isfinite(want[r]).any() for r in (0, 5, 8, 10, 11))      # (max{-inf, ...} is finite)
        got = g.send_ue_recv(dev(x), dev(y), mop, rop)
        C.check(to_np(got), want, bound, "%s(%r, %r) -> %s, y %s" % (mop, xv, yv, rop, shape))
    C.done()


# ------------------------------------------------------------------------------------------------
# softmax
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("d", [1, 8, 16, 100])
def test_segment_softmax(pgl, d, dtype):
    xs, ids, n_seg, names = S.softmax_segments(d)
    xs = xs.astype(dtype)
    want = S.softmax_def(xs, ids, n_seg)
    bound = S.softmax_bound(xs, ids, n_seg, want, S.EPS64 if dtype == np.float64 else S.EPS32)
    got = to_np(pgl.math.segment_softmax(dev(xs), dev(ids)))
    C = Collect()
    for s, name in enumerate(names):                                             # per segment: each case is named, neighbours included
        sel = ids == s
        C.check(got[sel], want[sel], bound[sel], "segment_softmax d=%d %s: segment %d (%s)" % (d, DT_NAME[dtype], s, name))
        if name == "all_3e38":
            assert (got[sel] == dtype(1.0 / 256)).all(), "equal logits at 3e38 give exactly uniform weights"
    C.done()


@pytest.mark.parametrize("by", ["dst", "src"])
@pytest.mark.parametrize("d", [1, 8, 100])
def test_edge_softmax(pgl, SG, by, d):
    G, g, _ = SG
    rng = np.random.default_rng(13)
    ids = G.dst if by == "dst" else G.src
    key_rows = {}
    order = np.argsort(ids, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=G.n))])
    x = (rng.standard_normal((G.E, d)) * 3).astype(np.float32)

    def seg(r):
        return order[starts[r]:starts[r + 1]]

    heavy = np.argsort(-np.bincount(ids, minlength=G.n))[:6]                       # the longest segments of this side
    a, b, c, e_, f_, h_ = (int(v) for v in heavy)
    npre = min(300, len(seg(a)) // 2)
    x[seg(a)[:npre]] = -INF                                                      # masked prefix (by dst: 300 edges of the hub, spanning chunks)
    x[seg(b)[0]] = -INF; x[seg(b)[len(seg(b)) // 2]] = -INF; x[seg(b)[-1]] = -INF
    x[seg(c)] = -INF                                                             # all masked: NaN
    x[seg(e_)[len(seg(e_)) // 2]] = INF
    x[seg(f_)[-1]] = NAN
    x[seg(h_)] = 3e38
    want = S.softmax_def(x, ids, G.n)
    bound = S.softmax_bound(x, ids, G.n, want)
    assert np.isnan(want[seg(c)]).all() and np.isfinite(want[seg(a)]).all() and (want[seg(a)[:npre]] == 0).all()
    got = to_np(pgl.nn.functional.edge_softmax(g, dev(x), by))
    C = Collect()
    for name, r in (("masked prefix", a), ("-inf first, middle, last", b), ("all -inf", c), ("one +inf", e_), ("NaN last", f_), ("all 3e38", h_)):
        C.check(got[seg(r)], want[seg(r)], bound[seg(r)], "edge_softmax by %s d=%d: %s" % (by, d, name))
    rest = ~np.isin(ids, heavy)
    C.check(got[rest], want[rest], bound[rest], "edge_softmax by %s d=%d: the other segments" % (by, d))
    C.done()


@pytest.mark.parametrize("d", [1, 8, 100])
def test_softmax_backward_of_a_masked_segment(pgl, d):
    """Masked (-inf) elements get gradient exactly 0; the others stay inside the softmax family's bound (K = 1.7456) of the terms of
    grad_defs.segment_softmax_terms."""
    import grad_defs as D
    rng = np.random.default_rng(14)
    lens = [40, 70, 30000, 50, 600]
    ids = np.concatenate([np.full(L, i, np.int64) for i, L in enumerate(lens)])
    x = (rng.standard_normal((len(ids), d)) * 3).astype(np.float32)
    masked = np.zeros(len(ids), bool)
    o = np.concatenate([[0], np.cumsum(lens)])
    masked[o[1]] = masked[o[1] + 35] = masked[o[2] - 1] = True
    masked[o[2]:o[2] + 300] = True; masked[o[2] + 15000:o[2] + 15300] = True
    masked[o[4] + 1:o[4] + 600:2] = True
    x[masked] = -INF
    cot = rng.standard_normal(x.shape).astype(np.float32)
    xt = dev(x).requires_grad_(True)
    pgl.math.segment_softmax(xt, dev(ids)).backward(dev(cot))
    got = to_np(xt.grad)
    assert (got[masked] == 0).all(), "masked elements must get gradient exactly 0"
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    ids_t = torch.from_numpy(ids)
    out64 = D.segment_softmax(x64, ids_t, len(lens))
    out64.backward(torch.from_numpy(cot).double())
    want = x64.grad.numpy()
    assert (want[masked] == 0).all() and np.isfinite(want).all()
    # terms p |g| + p sum_seg p |g| over the segment's length + 3 (grad_defs.segment_softmax_terms, written for p = 0 rows)
    p = out64.detach().numpy()
    pg = p * np.abs(cot)
    ssum = np.zeros((len(lens), d)); np.add.at(ssum, ids, pg)
    terms = pg + p * ssum[ids]
    n = np.asarray(lens, np.float64)[ids][:, None] + 3.0
    S.classify_and_check(got, want, D.K_FAMILY["softmax"] * S.rebound(terms, n), "softmax backward d=%d" % d)


# ------------------------------------------------------------------------------------------------
# fused GAT: masked sources (attn_src[u] = -inf)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,D_", [(8, 16), (4, 8), (1, 64), (2, 32)])
def test_fused_gat_masked_sources(SG, H, D_):
    """attn_src[u] = -inf on chosen sources gives the edge logit -inf: weight 0, the rest of the row correct.  Masked edge first in
    its row, last in its row, a masked prefix of 300 edges (whole first chunks of 64) of a 4096-edge row and of the 40 000-edge hub
    (the long fix-up, more than kFixShort = 16 further pieces) and of the 257-edge row (the short one, 200 edges); rows whose edges are
    ALL masked are NaN; rows without edges stay 0.  Against the edge-by-edge fp64 formula (_dense_gat_fp64)."""
    G, g, _ = SG
    rng = np.random.default_rng(15 + H)
    f = rng.standard_normal((G.n, H, D_)).astype(np.float32)
    a_s = rng.standard_normal((G.n, H)).astype(np.float32)
    a_d = rng.standard_normal((G.n, H)).astype(np.float32)
    mask = [(3, 0), (4, S.ROW_LENS[4] - 1), (5, 0), (5, 63), (6, 127), (7, 0), (7, 255), (10, 0), (10, S.resolve(G, 10, "late")), (10, 4352)]
    mask += [(8, p) for p in range(200)] + [(9, p) for p in range(300)] + [(11, p) for p in range(300)] + [(11, 20000), (11, 39999)]
    mask += [(r, p) for r in (0, 1, 2) for p in G.slots[r]]                      # rows 0, 1, 2: every edge masked -> NaN
    for r, p in mask:
        a_s[G.carrier[(r, p)]] = -INF
    a_s[G.carrier[(6, 0)], 0] = -INF                                             # one head only
    edges = torch.from_numpy(G.edges)
    o64, al64 = _dense_gat_fp64(edges, torch.from_numpy(f).double(), torch.from_numpy(a_s).double(), torch.from_numpy(a_d).double())
    want = o64.numpy()
    assert np.isnan(want[[0, 1, 2]]).all() and np.isfinite(want[3:12]).all() and (want[list(S.EMPTY_ROWS)] == 0).all()
    absterms = torch.zeros_like(o64).index_add(0, edges[:, 1], al64[:, :, None] * torch.from_numpy(f).double()[edges[:, 0]].abs()).numpy()
    nterm = G.indeg.astype(np.float64)[:, None, None] + 16.0                     # + exp / logit roundings: the count the C3 test uses
    got = to_np(g.gat_aggregate(dev(f), dev(a_s), dev(a_d), 0.2))
    C = Collect()
    for r in list(range(12)) + [12, 400]:
        C.check(got[r], want[r], S.rebound(absterms[r], nterm[r]), "fused GAT %dx%d row %d (%d edges)" % (H, D_, r, G.indeg[r]))
    C.check(got[20:400], want[20:400], S.rebound(absterms[20:400], nterm[20:400]), "fused GAT %dx%d the short rows" % (H, D_))
    # one +inf / one NaN source: the rows it feeds are NaN, the others untouched
    for v in (INF, NAN):
        a2 = a_s.copy(); a2[G.carrier[(11, 20000)]] = v; a2[G.carrier[(7, 255)]] = v
        o2 = _dense_gat_fp64(edges, torch.from_numpy(f).double(), torch.from_numpy(a2).double(), torch.from_numpy(a_d).double())[0].numpy()
        assert np.isnan(o2[[7, 11]]).all()
        got2 = to_np(g.gat_aggregate(dev(f), dev(a2), dev(a_d), 0.2))
        C.check(got2[:12], o2[:12], S.rebound(absterms[:12], nterm[:12]), "fused GAT %dx%d with a %r logit" % (H, D_, v))
    C.done()


# ------------------------------------------------------------------------------------------------
# fused layer forms against their unfused compositions
# ------------------------------------------------------------------------------------------------
def _dense_case(G, d_in, rng):
    x = rng.standard_normal((G.n, d_in)).astype(np.float32)
    x[G.carrier[(5, 0)]] = NAN                       # a NaN source row feeding rows 5, 9 and the hub (through its carriers)
    x[G.carrier[(9, 2048)], 3] = NAN
    x[G.carrier[(11, 39990)]] = NAN
    x[G.carrier[(6, 0)]] = INF                       # an inf source row
    x[G.carrier[(10, 4200)], 0] = -INF
    return x


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "src_scale"])
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("d_in,d_out", [(64, 32), (128, 128)])
def test_aggregate_dense_relu_of_nan(pgl, SG, d_in, d_out, act, scaled):
    """aggregate_dense against aggregate -> torch linear -> torch.relu, in class; rows no special value reaches stay in their bound.
    Rows without edges give act(bias)."""
    G, g, _ = SG
    ops, csr = pgl.ops, g.adj_dst_index.csr
    rng = np.random.default_rng(16 + d_in)
    x = _dense_case(G, d_in, rng)
    w = (rng.standard_normal((d_in, d_out)) / np.sqrt(d_in)).astype(np.float32)
    bias = rng.standard_normal(d_out).astype(np.float32)
    ss = (rng.random(G.n) + 0.5).astype(np.float32) if scaled else None
    ds = (rng.random(G.n) + 0.5).astype(np.float32) if scaled else None
    out, _ = ops.aggregate_dense(dev(x), csr, dev(w), dev(bias), act, "sum", None if ds is None else dev(ds), None, False, None if ss is None else dev(ss))
    # the unfused composition, on the GPU in fp32 (class) and in fp64 on the host (values)
    agg = ops.aggregate(dev(x), csr, "sum", src_scale=None if ss is None else dev(ss), dst_scale=None if ds is None else dev(ds))
    z = torch.nn.functional.linear(agg, dev(w).t().contiguous(), dev(bias))
    unf = to_np(torch.relu(z) if act else z)
    xs64 = x.astype(np.float64) * (1.0 if ss is None else ss.astype(np.float64)[:, None])
    with np.errstate(invalid="ignore"):
        a64 = R.np_send_u_recv(xs64, G.src, G.dst, "sum") * (1.0 if ds is None else ds.astype(np.float64)[:, None])
        aabs = R.np_send_u_recv(np.abs(xs64), G.src, G.dst, "sum") * (1.0 if ds is None else ds.astype(np.float64)[:, None])
        z64 = a64 @ w.astype(np.float64) + bias
        want = torch.relu(torch.from_numpy(z64)).numpy() if act else z64
        terms = aabs @ np.abs(w).astype(np.float64) + np.abs(bias)
    n = G.indeg.astype(np.float64)[:, None] + d_in + 3.0
    bound = S.rebound(terms, n)
    touched = ~np.isfinite(a64).all(1)
    assert touched[[5, 6, 9, 10, 11]].all() and touched.sum() == 5
    assert np.array_equal(S.classes(unf), S.classes(want))                       # the unfused fp32 chain has the definition's classes
    if act:
        assert np.isnan(want[5]).all()                                           # relu(NaN) is NaN
    S.classify_and_check(to_np(out), want, bound, "aggregate_dense %d->%d act=%s scaled=%s" % (d_in, d_out, act, scaled))
    S.classify_and_check(to_np(out), unf.astype(np.float64), np.where(np.isfinite(bound), 2.0 * bound, 0.0), "aggregate_dense vs the unfused chain")


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("d", [7, 64, 256])
def test_row_epilogue(pgl, d, act, normalize):
    """normalize_L2(relu(z + bias)) against torch (torch.relu, F.normalize): NaN / inf elements, an all-zero row under normalize."""
    rng = np.random.default_rng(17 + d)
    n = 300
    z = rng.standard_normal((n, d)).astype(np.float32)
    bias = rng.standard_normal(d).astype(np.float32)
    z[3, 0] = NAN; z[4] = NAN; z[5, d - 1] = INF; z[6, 1 % d] = -INF; z[7, 0] = INF; z[7, d - 1] = -INF
    z[8] = -bias                                                                 # an all-zero row after the bias
    z[9] = -np.abs(z[9]) - np.abs(bias) - 1.0                                    # all negative: zero after relu
    z[299, d // 2] = NAN
    y, _ = pgl.ops.row_epilogue(dev(z), dev(bias), act, normalize)
    a = torch.from_numpy(z).double() + torch.from_numpy(bias).double()
    if act:
        a = torch.relu(a)
    want = (torch.nn.functional.normalize(a, dim=1, eps=1e-12) if normalize else a).numpy()
    with np.errstate(invalid="ignore"):
        pre = np.abs(z.astype(np.float64)) + np.abs(bias)
        nrm = np.maximum(np.sqrt((a.numpy() ** 2).sum(1, keepdims=True)), 1e-12)
        bound = S.rebound(pre / nrm, d + 3.0) if normalize else S.rebound(pre, 2.0)
    bound = np.where(np.isfinite(bound), bound, 0.0)                             # (relu(-inf) = 0 beside an inf norm: exactly 0)
    if normalize:
        assert np.isnan(want[3]).all() and (want[8] == 0).all()                  # a NaN norm makes the row NaN; 0 / eps = 0
    S.classify_and_check(to_np(y), want, bound, "row_epilogue d=%d act=%s normalize=%s" % (d, act, normalize))


# ------------------------------------------------------------------------------------------------
# casts and 16-bit stores
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", [F16, BF16], ids=["fp16", "bf16"])
def test_cast_16_to_32_every_bit_pattern(pgl, tdt):
    bits = np.arange(65536, dtype=np.int64).astype(np.uint16)
    t = torch.from_numpy(bits.view(np.int16)).view(tdt)
    want = t.float().numpy()
    for shape in ((4096, 16), (65536, 1), (8192, 8)):
        got = to_np(pgl.ops.gather_rows_cast(t.reshape(shape).cuda(), None, torch.float32)).reshape(-1)
        S.assert_bits_equal(got.view(np.uint32), want.view(np.uint32), np.isnan(want), np.isnan(got), "%s -> fp32 %s" % (DT_NAME[tdt], shape))
    idx = torch.from_numpy(np.random.default_rng(1).permutation(4096)).cuda()
    got = to_np(pgl.ops.gather_rows_cast(t.reshape(4096, 16).cuda(), idx, torch.float32))
    w2 = want.reshape(4096, 16)[idx.cpu().numpy()]
    S.assert_bits_equal(got.view(np.uint32), w2.view(np.uint32), np.isnan(w2), np.isnan(got), "%s -> fp32 gathered" % DT_NAME[tdt])


@pytest.mark.parametrize("tdt", [F16, BF16], ids=["fp16", "bf16"])
def test_cast_32_to_16_is_one_round_to_nearest_even(pgl, tdt):
    x = S.f32_from_bits(S.cast_set("fp16" if tdt == F16 else "bf16"))
    pad = (-len(x)) % 8
    x = np.concatenate([x, np.zeros(pad, np.float32)])
    wb, wn = S.torch_cast_bits(x, tdt)
    for cols in (8, 1):
        got = pgl.ops.gather_rows_cast(dev(x.reshape(-1, cols)), None, tdt).cpu().reshape(-1)
        S.assert_bits_equal(got.view(torch.int16).numpy().view(np.uint16), wb, wn, torch.isnan(got).numpy(), "fp32 -> %s [n, %d]" % (DT_NAME[tdt], cols))


@pytest.mark.parametrize("tdt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("d", [8, 3, 33, 64, 130, "view"])
def test_16bit_aggregate_store_is_one_rounding(pgl, tdt, d):
    """The 16-bit store of `aggregate` (from_acc) equals torch's CPU cast of the fp32 accumulator, bit for bit and sign included.
    The accumulator is made to hold values of the cast set EXACTLY: a value x is written as a sum of up to three stored 16-bit terms
    (successive truncations, so every partial sum is exact in any order) and reduced with `sum`; 2x and 4x are written as two / four
    terms and reduced with `mean`, which reaches values below the smallest 16-bit subnormal.  The kept values include finite
    accumulators that round to inf, non-zero ones that round to zero, and subnormal results (asserted).  Rows of a single message
    carry every 16-bit value of the set, NaN and inf included: the store is then the identity.  d % 4 == 0 takes the 4-element
    store, odd d the 1-element store, "view" a column block at an odd element offset."""
    kind = "fp16" if tdt == F16 else "bf16"
    x32 = S.f32_from_bits(S.cast_set(kind))
    tiny_normal = 2.0 ** -14 if tdt == F16 else 2.0 ** -126
    width = 8 if d == "view" else d
    groups, src, dst, feats, n_rows, n_nodes = [], [], [], [], 0, 0
    for op, n_terms, scale in (("sum", 3, 1.0), ("mean", 2, 2.0), ("mean", 4, 4.0)):
        terms, ok = S.split16(x32, tdt, n_terms, scale)
        keep = np.nonzero(ok)[0]
        m = len(keep)
        groups.append((op, keep, n_rows))
        for t in range(n_terms):
            feats.append(torch.from_numpy(terms[keep, t]).to(tdt))
            src.append(n_nodes + np.arange(m)); dst.append(n_rows + np.arange(m))
            n_nodes += m
        n_rows += m
    singles = torch.unique(torch.from_numpy(x32).to(tdt).view(torch.int16)).view(tdt)
    k = len(singles)
    feats.append(singles); src.append(n_nodes + np.arange(k)); dst.append(n_rows + np.arange(k))
    n = max(n_nodes + k, n_rows + k)
    ft = torch.zeros(n, dtype=tdt); ft[:n_nodes + k] = torch.cat(feats)
    assert bool((ft[:n_nodes].float() == torch.cat(feats[:-1]).float()).all())           # every term IS a stored value
    ft = ft[:, None].repeat(1, width)
    g = pgl.Graph(edges=np.stack([np.concatenate(src), np.concatenate(dst)], 1).astype(np.int64), num_nodes=n).tensor()
    csr = g.adj_dst_index.csr

    def run(op):
        if d == "view":
            big = torch.zeros((n, 3 * width + 1), dtype=tdt, device="cuda")
            big[:, 1:1 + width] = ft.cuda()                # a column block at an odd element offset: no 8-byte alignment
            outb = torch.zeros((n, 3 * width + 1), dtype=tdt, device="cuda")
            pgl.ops.aggregate(big[:, 1:1 + width], csr, op, out=outb[:, 1:1 + width])
            return outb[:, 1:1 + width].cpu().contiguous()
        return g.send_recv(ft.cuda(), op).cpu().contiguous()

    out = {"sum": run("sum"), "mean": run("mean")}
    seen = {"overflow": 0, "underflow": 0, "subnormal": 0}
    for op, keep, r0 in groups:
        wb, wn = S.torch_cast_bits(x32[keep], tdt)
        back = torch.from_numpy(wb.view(np.int16)).view(tdt).float().numpy()
        seen["overflow"] += int(np.isinf(back).sum()); seen["underflow"] += int((back == 0).sum())
        seen["subnormal"] += int(((back != 0) & (np.abs(back) < tiny_normal)).sum())
        got = out[op][r0:r0 + len(keep)]
        gb = got.view(torch.int16).numpy().view(np.uint16)
        for j in range(width):
            S.assert_bits_equal(gb[:, j], wb, wn, torch.isnan(got[:, j]).numpy(), "%s store after %s, column %d of %s" % (kind, op, j, d))
    assert min(seen.values()) >= 4, seen                  # finite accumulators that round to inf, to zero and to subnormals all went through
    sb = singles.view(torch.int16).numpy().view(np.uint16)
    g1 = out["sum"][n_rows:n_rows + k]
    for j in range(width):                                # (0 + -0 = +0 in the accumulator: arithmetic, the zero's sign is open)
        S.assert_bits_equal(g1.view(torch.int16).numpy().view(np.uint16)[:, j], sb, torch.isnan(singles).numpy(), torch.isnan(g1[:, j]).numpy(),
                            "%s store of a single message, column %d of %s" % (kind, j, d), zero_sign_free=True)


# ------------------------------------------------------------------------------------------------
# subnormals are numbers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 8, 16, 20, 32, 33, 130])
def test_subnormal_aggregation_is_exact(SG, d):
    G, g, _ = SG
    x = S.subnormal_features(G, d)
    C = Collect()
    for op in OPS:
        want, _ = S.expect(G, x, op)
        got = to_np(g.send_recv(dev(x), op))
        C.check(got, want, 0.5 * S.SUB_UNIT if op == "mean" else 0.0, "subnormal %s d=%d" % (op, d))     # mean: one rounding of a subnormal quotient
    C.done()


def test_subnormal_send_uv_scaled_aggregation_and_row_moves(pgl, SG):
    G, g, _ = SG
    ops = pgl.ops
    C = Collect()
    for d in (8, 130):
        x = S.subnormal_features(G, d)
        y = S.subnormal_features(G, d, seed=6)
        s32, d32 = dev(G.src.astype(np.int32)), dev(G.dst.astype(np.int32))
        for mop in ("add", "sub"):                                               # sums of two multiples of 2**-149 below 2**-125: exact
            want = R.np_send_uv(x.astype(np.float64), y.astype(np.float64), G.src, G.dst, mop)
            C.check(to_np(ops.send_uv(dev(x), dev(y), s32, d32, mop)), want, 0.0, "subnormal send_uv %s d=%d" % (mop, d))
        one = np.ones_like(y); two = np.full_like(y, 2.0)
        want = R.np_send_uv(x.astype(np.float64), two.astype(np.float64), G.src, G.dst, "mul")            # doubling is exact
        C.check(to_np(ops.send_uv(dev(x), dev(two), s32, d32, "mul")), want, 0.0, "subnormal send_uv mul by 2 d=%d" % d)
        want = R.np_send_uv(x.astype(np.float64), one.astype(np.float64), G.src, G.dst, "div")
        C.check(to_np(ops.send_uv(dev(x), dev(one), s32, d32, "div")), want, 0.0, "subnormal send_uv div by 1 d=%d" % d)
        # degree_norm-scaled aggregation: the scale of a node of degree 4**k is 2**-k exactly; the features are multiples of 2**-149 * 2**6
        # so that the scaled terms stay multiples of 2**-149 (nothing is rounded) -- and every node gets the scale of degree 1, 4 or 16
        deg = np.asarray([1, 4, 16], np.int64)[np.arange(G.n) % 3]
        nrm = to_np(ops.degree_norm(dev(deg)))
        assert np.array_equal(nrm[:, 0], np.asarray([1.0, 0.5, 0.25], np.float32)[np.arange(G.n) % 3])
        k = np.random.default_rng(8).integers(-6, 7, (G.n, d))
        xs = (k * 64 * S.SUB_UNIT).astype(np.float32)
        x64 = xs.astype(np.float64) * nrm.astype(np.float64)
        want = R.np_send_u_recv(x64, G.src, G.dst, "sum") * nrm.astype(np.float64)
        assert np.abs(want).max() < 2.0 ** -125 and np.array_equal(want.astype(np.float32).astype(np.float64), want)
        got = g.send_recv_scaled(dev(xs), dev(nrm.reshape(-1)), dev(nrm.reshape(-1)))
        C.check(to_np(got), want, 0.0, "subnormal degree_norm-scaled aggregation d=%d" % d)
        # gather / scatter_rows move bits
        idx = np.random.default_rng(9).permutation(G.n)
        got = to_np(ops.gather_rows(dev(x), dev(idx)))
        assert np.array_equal(got.view(np.uint32), x[idx].view(np.uint32))
        out = torch.zeros(G.n, d, device="cuda")
        ops.scatter_rows(out, dev(idx), dev(x))
        w = np.zeros_like(x); w[idx] = x
        assert np.array_equal(to_np(out).view(np.uint32), w.view(np.uint32))
    C.done()


@pytest.mark.parametrize("d", [8, 128])
def test_subnormal_atomic_scatter_add(pgl, SG, d):
    """ops.scatter_add_coo adds with the hardware fp32 atomic; it is documented as order-dependent in the last bits.  The exact-sum
    inputs have no order dependence at all, so the path is exact too unless the atomic flushes subnormals -- in which case (a property
    of the instruction, recorded in DESIGN.md) each of the n terms of an element may lose at most 2**-126."""
    G, g, _ = SG
    x = S.subnormal_features(G, d)
    want, _ = S.expect(G, x, "sum")
    got = to_np(pgl.ops.scatter_add_coo(dev(x), dev(G.src.astype(np.int32)), dev(G.dst.astype(np.int32)), G.n))
    exact = np.array_equal(got.astype(np.float64), want)
    print("scatter_add_coo on subnormals d=%d: %s; worst |err| %.3e = %.1f units of 2**-149; elements flushed to 0: %d of %d nonzero"
          % (d, "EXACT" if exact else "NOT exact", np.abs(got - want).max(), np.abs(got - want).max() / S.SUB_UNIT,
             int(((got == 0) & (want != 0)).sum()), int((want != 0).sum())))
    S.classify_and_check(got, want, G.indeg.astype(np.float64)[:, None] * 2.0 ** -126, "subnormal scatter_add_coo d=%d" % d)


# ------------------------------------------------------------------------------------------------
# integers: wrap-around, INT_MIN / INT_MAX
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("d", [8, 12, 40, 130])
def test_integer_wrap_and_extremes(SG, dtype, d):
    G, g, _ = SG
    ii = np.iinfo(dtype)
    rng = np.random.default_rng(20 + d)
    x = rng.integers(-1000, 1000, (G.n, d)).astype(dtype)
    big = ii.max // 2 + 1                                                        # 2**30 / 2**62: three of them wrap once, five wrap twice
    for r, cnt in ((3, 3), (5, 3), (8, 5), (10, 3), (11, 5)):                    # rows that wrap once (3 x 2**30) and twice (5 x 2**30)
        for p in G.slots[r][:cnt]:
            x[G.carrier[(r, p)]] = big
    x[G.carrier[(6, 0)]] = ii.max; x[G.carrier[(6, 127)]] = 5                    # INT_MAX + 5 (+ small terms)
    x[G.carrier[(7, 0)]] = ii.min; x[G.carrier[(7, 255)]] = -7
    x[G.carrier[(9, 2048)], 0] = ii.min; x[G.carrier[(9, 4095)], 1 % d] = ii.max
    x[G.carrier[(4, 0)]] = ii.max; x[G.carrier[(4, 16)]] = ii.min
    for p in G.slots[1]: x[G.carrier[(1, p)]] = ii.min                            # a row of only INT_MIN: max must give INT_MIN (min runs as ~x)
    for p in G.slots[2]: x[G.carrier[(2, p)]] = ii.max
    C = Collect()
    for op in OPS:
        with np.errstate(over="ignore"):
            want = R.c_send_u_recv(x, G.src, G.dst, op) if op == "mean" else R.np_send_u_recv(x, G.src, G.dst, op)   # integer mean follows the oracle
        if op == "sum":
            wide = R.np_send_u_recv(x.astype(object), G.src, G.dst, "sum") if dtype == np.int64 else R.np_send_u_recv(x.astype(np.int64), G.src, G.dst, "sum")
            assert all(int(wide[r, 0]) > ii.max for r in (3, 8, 11)) and int(wide[8, 0]) > 2 * (ii.max + 1)      # wraps once and twice
            assert np.array_equal(want, R.c_send_u_recv(x, G.src, G.dst, "sum"))
        C.check(to_np(g.send_recv(dev(x), op)), want, 0, "integer %s %s d=%d" % (op, DT_NAME[dtype], d))
    C.done()
