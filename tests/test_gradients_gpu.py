"""Every autograd node of pgl_amd/autograd.py held to fp64 gradients ELEMENT BY ELEMENT on the MI355X.

`assert_grads` runs the engine's forward and backward, evaluates the plain definition of the same op (tests/grad_defs.py) in fp64 on
the same data, and compares the forward and every gradient per element inside the fp32 re-association bound of THAT ELEMENT'S OWN
terms (gpu_common.reassociation_bound, slack 4 -- the constant the forward tests use); then it repeats the backward and requires
identical bits (every backward here is atomic-free).  No tolerance is tied to a tensor's largest element, no element is left out.

Data: node and cotangent rows are scaled per row by 10**U(-4, 0), so small rows exist; divisors lie in [0.5, 1.5]; max / min draw from
a small integer set (operands: powers of two for div), so ties are exact in every precision.  The kinked ops (leaky relu, relu) take
their pre-activations from a binary lattice (odd + even multiples of 2**-9: never closer to 0 than 2**-9 > 1e-4, asserted on the fp64
side) -- for those the per-row scaling is on the cotangent alone, since a scaled row would land inside the margin.

Composite gradients (softmax, GAT, the additive score, the normalising epilogue, the dense forms) also carry the forward's rounding
(exp of a difference, a GEMM); they use the same abs-terms bound times a factor K per family.  K = max(1, 4 x the worst err / bound of
the PLAIN DEFINITION evaluated in fp32 torch on the same inputs) -- never measured from the engine; 4 because a differently ordered fp32
evaluation may use a few times more of its bound than torch's does.  Measured with `_measure_definitions()` (fp32 torch on the host):

    family         worst err / bound of the fp32 definition      K
    softmax        0.4364                                         1.7456
    gat            0.063                                          1
    gat_proj       0.033                                          1
    add_score      0.092                                          1
    row_epilogue   0.032                                          1
    dense          0.023                                          1
    dual_linear    0.021                                          1
    gat_drop       0.061                                          1
    gat_proj_drop  0.027                                          1

(the numbers live in grad_defs.FP32_DEFINITION_RATIO / K_FAMILY and tests/test_grad_defs.py re-measures them; the worst softmax case is edge_softmax by source, d = 100;
gat_drop / gat_proj_drop: gat / gat_proj with attention dropout on, the cases of tests/test_gat_dropout_gpu.py -- worst: the classes graph, 8 x 16, p = 0.6)
"""
import numpy as np
import pytest
import torch

import grad_defs as D
from gpu_common import pgl, _assert_elementwise, reassociation_bound, EPS  # noqa: F401  (pgl: the fixture)
from layout_defs import misaligned          # the same values as a contiguous view 4 bytes past a 16-byte boundary (tests/layout_defs.py)

pytestmark = pytest.mark.gpu

K = D.K_FAMILY

DEVICE = "cuda"
_MEASURED = None            # a dict while _measure_definitions() runs: family -> worst err / bound of the fp32 definition; the engine is not called
Q = 2.0 ** -9               # the lattice step of the kinked ops' pre-activations
EPS32, EPS64 = EPS[np.dtype(np.float32)], EPS[np.dtype(np.float64)]
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


# ------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().double().cpu().numpy()


def _compare(got, want64, abs_terms, n_terms, K_, eps, rel_round, terms_round, abs_round, what):
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    want, terms = _np(want64), _np(abs_terms)
    bound = K_ * reassociation_bound(terms, _np(n_terms), 4.0, eps) + rel_round * 1.01 * np.abs(want) + terms_round * terms + abs_round
    err = np.abs(_np(got) - want)
    assert np.isfinite(_np(got)).all(), what + ": not finite"
    _assert_elementwise(err, np.broadcast_to(bound, err.shape), want, what)
    return float((err / np.broadcast_to(bound, err.shape)).max()) if err.size else 0.0


def assert_grads(engine_fn, def_fn, inputs, cotangent, n_out=1.0, n_terms=None, frozen_fn=None, terms=None, family=None, eps=EPS32,
                 check=None, prescaled=False, forward=True, what=""):
    """engine_fn(*tensors) -> the engine's output (tensors: the inputs, requiring a gradient where `check` names them);
    def_fn(*tensors, frozen=None): the definition.  inputs / cotangent: device tensors in their STORAGE type (the fp64 side reads the
    stored values).  n_out, n_terms, frozen_fn, terms: see grad_defs.grad_and_terms.  family: a key of K (None: K = 1).
    check: indices of the inputs whose gradient is taken and compared (default: all).  forward=False: the forward is not compared
    (the self-checks against a mutated definition, which must be refused BY A GRADIENT).
    16-bit storage (fp16 / bf16 inputs): sums run in fp32 and the result is rounded to 16 bits once -- half an output ulp, u16 * |want|
    (fp16: at least half its subnormal spacing, 2**-25).  prescaled (the mean of a 16-bit gradient): 1 / deg and every scaled cotangent
    element are rounded to 16 bits before the sum -- two more roundings of every term, 2 * u16 * abs_terms (fp16: + 2**-25 per term
    times the operand it is multiplied by, at most 1.5).  These absolute fp16 terms are not in the issue's wording; they are the
    format's own rounding where rows scaled by 1e-4 (and then by 1 / deg) are subnormal in fp16.  Measured on the MI355X (each case
    prints it): of 192 000 gradient elements 0 (sum), 1 (sum x mul), 9 (mean) and 4 (mean x add) need them at all; of the terms alone
    the worst element uses 0.88 for the single output rounding and 0.18 of the pre-scaled mean's n-term allowance."""
    check = list(range(len(inputs))) if check is None else list(check)
    r = D.grad_and_terms(def_fn, inputs, cotangent, n_out, n_terms, frozen_fn, terms)
    k = 1.0 if family is None else K[family]
    if _MEASURED is not None:
        out32, g32 = D.evaluate(def_fn, inputs, cotangent, torch.float32, frozen_fn)
        ratio = max([D.worst_ratio(out32, r.out64, r.out_abs, r.out_n)] +
                    [D.worst_ratio(g32[i], r.want64[i], r.abs_terms64[i], r.n_terms[i]) for i in check])
        print("%s: the fp32 definition uses %.3f of the bound" % (what or family, ratio))
        _MEASURED[family] = max(_MEASURED.get(family, 0.0), ratio)
        return
    u16 = U16.get(inputs[0].dtype, 0.0)
    sub16 = 2.0 ** -25 if inputs[0].dtype == torch.float16 else 0.0

    def run():
        xs = [t.detach().requires_grad_(i in check) for i, t in enumerate(inputs)]     # (detach keeps a view's storage offset)
        out = engine_fn(*xs)
        out = out if isinstance(out, torch.Tensor) else out.materialize()
        out.backward(cotangent)
        for i in check:
            assert xs[i].grad is not None, "%s: input %d received no gradient" % (what, i)
        return out.detach(), [xs[i].grad for i in check]

    out, grads = run()
    used = []
    if forward:
        used.append(("forward", _compare(out, r.out64, r.out_abs, r.out_n, k, eps, u16, 0.0, sub16, what + " forward")))
    for i, g in zip(check, grads):
        pre = 1.0 if prescaled else 0.0
        used.append(("d input %d" % i, _compare(g, r.want64[i], r.abs_terms64[i], r.n_terms[i], k, eps, u16, pre * 2.0 * u16 * 1.01,
                                                sub16 * (1.0 + pre * 1.5 * _np(r.n_terms[i])), "%s d input %d" % (what, i))))
        if sub16:                                      # how much the fp16 subnormal terms are needed: the same element check without them
            err = np.abs(_np(g) - _np(r.want64[i]))
            rel = reassociation_bound(_np(r.abs_terms64[i]), _np(r.n_terms[i]), 4.0, eps) + u16 * 1.01 * np.abs(_np(r.want64[i])) + \
                pre * 2.0 * u16 * 1.01 * _np(r.abs_terms64[i])
            print("%s d input %d: %d of %d elements need the fp16 subnormal terms; of those terms alone the worst element uses %.3f"
                  % (what, i, int((err > rel).sum()), err.size,
                     float((np.maximum(err - rel, 0.0) / (sub16 * (1.0 + pre * 1.5 * _np(r.n_terms[i])))).max())))
    print("%s: the engine uses %s of the bound" % (what, ", ".join("%.3f (%s)" % (v, name) for name, v in used)))
    out2, grads2 = run()
    assert torch.equal(out2, out), what + ": forward not reproducible"
    for i, a, b in zip(check, grads, grads2):
        assert torch.equal(a, b), "%s: d input %d not bit-reproducible" % (what, i)


# ------------------------------------------------------------------------------------------------
# graphs (built once per module) and data
# ------------------------------------------------------------------------------------------------
class _G(object):
    """edges on the host and the device; `.g`: the engine's graph (edge tensors handed out in ORIGINAL edge order)."""

    def __init__(self, pgl_, n, src, dst):
        self.n, self.e = int(n), int(src.shape[0])
        self.src_np, self.dst_np = src.astype(np.int64), dst.astype(np.int64)
        self.src, self.dst = (torch.as_tensor(a, device=DEVICE) for a in (self.src_np, self.dst_np))
        self.g = None
        if pgl_ is not None:
            self.g = pgl_.Graph(edges=np.stack([self.src_np, self.dst_np], 1).reshape(-1, 2), num_nodes=self.n).tensor()
            self.g.lazy_edge_order = False
        self.indeg, self.outdeg = D.degree(self.dst, n).double(), D.degree(self.src, n).double()


def _hub_edges(n=3000, e=40000, seed=5):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n - 100, e), rng.integers(50, n, e)       # nodes 0..49: no in-edge; the last 100: no out-edge
    src[rng.choice(e, 3000, replace=False)] = 60                         # a hub source and a hub destination of > 2 chunks of 256 edges:
    dst[rng.choice(e, 3000, replace=False)] = 70                         #   both walks split rows and run the fix-up
    src[:40], dst[:40] = 100, 200                                        # multi-edges
    src[40:80] = dst[40:80] = np.arange(300, 340)                        # self-loops
    return n, src, dst


CHUNK = 64                               # edges per chunk below 5 M edges (chunk_edges_for): what every graph of this module runs with
CLASS_ROWS = (1025, 63, 1089, 100, 3000)  # at the head of a sorted stream: 16 further pieces, not split, 17, 1, 47


def _classes_edges(n=3000, fill=2000, seed=6):
    """Every class of split row, on the dst-sorted AND the src-sorted stream: nodes 0..4 receive CLASS_ROWS edges each and send
    CLASS_ROWS edges each, so both streams open with rows of these lengths -- a row inside one chunk, one with 1 further piece, one
    with exactly 16 (the last a single wave finishes), one with exactly 17 (the first handed to the block-parallel pass) and a hub.
    Nodes 5..49 receive no edge, the last 100 send none; the edge list itself is in random order."""
    rng = np.random.default_rng(seed)
    k, heavy = int(sum(CLASS_ROWS)), np.repeat(np.arange(len(CLASS_ROWS)), CLASS_ROWS)
    src = np.concatenate([rng.integers(100, n - 100, k), heavy, rng.integers(100, n - 100, fill)])
    dst = np.concatenate([heavy, rng.integers(50, n, k), rng.integers(50, n, fill)])
    order = rng.permutation(src.shape[0])
    return n, src[order], dst[order]


def further_pieces(ids, n, chunk=CHUNK):
    """Per row of the stream sorted by `ids`: in how many chunks beyond the one of its first edge the row has edges (0: not split)."""
    indptr = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=n))])
    lo, hi = indptr[:-1], indptr[1:]
    return np.where(hi > lo, (hi - 1) // chunk - lo // chunk, 0)


@pytest.fixture(scope="module")
def graphs(pgl):
    return _graphs(pgl)


def _graphs(pgl_):
    n, src, dst = _hub_edges()
    z = np.zeros(0, np.int64)
    return dict(hub=_G(pgl_, n, src, dst), classes=_G(pgl_, *_classes_edges()), E0=_G(pgl_, 5, z, z), E1=_G(pgl_, 4, np.array([2]), np.array([1])),
                N1=_G(pgl_, 1, np.zeros(3, np.int64), np.zeros(3, np.int64)))


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEVICE).to(dtype)


def rows(rng, *shape):
    """standard normal rows, each scaled by 10**U(-4, 0)."""
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-4, 0, (shape[0],) + (1,) * (len(shape) - 1))


def ints(rng, *shape):
    return rng.integers(-3, 4, shape).astype(np.float64)


def lattice(rng, odd, *shape):
    """multiples of Q in about [-2, 2]: odd ones, or even ones."""
    k = rng.integers(-512, 512, shape) * 2
    return (k + 1 if odd else k) * Q


# ------------------------------------------------------------------------------------------------
# _Aggregate
# ------------------------------------------------------------------------------------------------
def _agg_case(G, rop, mop, xs, ys, out_size=None, dtype=torch.float32, seed=0, misalign=False, check=None, what=""):
    rng = np.random.default_rng(seed)
    n, e = G.n, G.e
    exact = rop in ("max", "min")
    x = ints(rng, n, *xs) if exact else rows(rng, n, *xs)
    y = None
    if mop is not None:
        if exact:
            y = 2.0 ** rng.integers(-1, 2, (e,) + ys) if mop in ("mul", "div") else ints(rng, e, *ys)
        else:
            y = rng.random((e,) + ys) + 0.5
    out_tail = xs if mop is None else tuple(np.broadcast_shapes(xs, ys))
    m = out_size or n
    cot = _t(rows(rng, m, *out_tail), dtype)
    inputs = [_t(x, dtype)] + ([] if y is None else [_t(y, dtype)])
    if misalign:
        inputs, cot = [misaligned(t) for t in inputs], misaligned(cot)
    ysh = None if y is None else (e,) + ys
    n_out, n_terms = D.aggregate_n_terms(G.src, G.dst, (n,) + xs, ysh, rop, out_size)
    if y is None:
        eng = lambda a: G.g.send_recv(a, rop, out_size)
        fn = lambda a, frozen=None: D.send_recv(a, G.src, G.dst, rop, out_size, frozen=frozen)
        fr = lambda a: D.winner_mask(a, G.src, G.dst, rop, out_size)
    else:
        eng = lambda a, b: G.g.send_ue_recv(a, b, mop, rop, out_size)
        fn = lambda a, b, frozen=None: D.send_recv(a, G.src, G.dst, rop, out_size, b, mop, frozen=frozen)
        fr = lambda a, b: D.winner_mask(a, G.src, G.dst, rop, out_size, b, mop)
    assert_grads(eng, fn, inputs, cot, n_out, n_terms[:len(inputs)], fr, eps=EPS64 if dtype == torch.float64 else EPS32, check=check,
                 prescaled=rop == "mean" and dtype in U16,
                 what=what or "%s/%s x%s y%s" % (rop, mop, xs, ys))


ROPS, MOPS = ("sum", "mean", "max", "min"), (None, "add", "sub", "mul", "div")


@pytest.mark.parametrize("mop", MOPS)
@pytest.mark.parametrize("rop", ROPS)
def test_aggregate_every_reduce_and_message_op(graphs, rop, mop):
    _agg_case(graphs["hub"], rop, mop, (16,), (16,), seed=1)


# y: [E], [E,1], [E,d], [E,H,D], [E,H,1]; x [N,H,1] and x [N,D] against y [E,H,D] (d x unbroadcast); y [E,1,D] and y [E,D] against
# x [N,H,D]: general broadcasts the fast d y kernel refuses (composed from gathers)
OPERAND_SHAPES = {"E": ((128,), ()), "E1": ((128,), (1,)), "Ed": ((128,), (128,)), "EHD": ((8, 16), (8, 16)), "EH1": ((8, 16), (8, 1)),
                  "xH1": ((8, 1), (8, 16)), "xD": ((16,), (8, 16)), "general": ((8, 16), (1, 16)), "yD": ((8, 16), (16,))}


@pytest.mark.parametrize("shape", sorted(OPERAND_SHAPES))
@pytest.mark.parametrize("mop,rop", [("mul", "sum"), ("add", "mean"), ("sub", "sum"), ("div", "mean"), ("mul", "mean"), ("add", "max"),
                                     ("div", "min")])
def test_aggregate_operand_shapes(graphs, shape, mop, rop):
    xs, ys = OPERAND_SHAPES[shape]
    _agg_case(graphs["hub"], rop, mop, xs, ys, seed=2)


# narrow (<= 64 B), grouped (64..128 B), flat rows; both sides of pglamd_winner_grad's lane boundaries (64 | 65, 66: 2-element lanes need an
# even d; 128 | 130, 132: 4-element lanes need d % 4 == 0; 256 | 260: the kernel's limit)
WIDTHS = [1, 8, 16, 17, 24, 32, 33, 64, 65, 66, 128, 130, 132, 256, 260]


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("rop", ROPS)
def test_aggregate_widths_without_an_operand(graphs, rop, d):
    _agg_case(graphs["hub"], rop, None, (d,), (d,), seed=3)


# pglamd_edge_operand_grad: a group of d / dy columns must span a power-of-two number of lanes (lanes of 1, 2, 4 elements for d <= 64,
# <= 128, <= 256) -- shapes on both sides of that rule, and of the d <= 256 limit
GROUPS = [((24,), ()), ((3, 8), (3, 1)), ((96,), ()), ((3, 32), (3, 1)), ((192,), (1,)), ((3, 64), (3, 1)), ((2, 65), (2, 1)),
          ((65,), (65,)), ((130,), (130,)), ((2, 130), (2, 1)), ((260,), (1,)), ((4, 64), (4, 1)), ((256,), (256,)), ((6,), (6,))]


@pytest.mark.parametrize("xs,ys", GROUPS)
@pytest.mark.parametrize("mop,rop", [("mul", "mean"), ("add", "sum"), ("div", "sum")])
def test_aggregate_operand_group_spans(graphs, mop, rop, xs, ys):
    _agg_case(graphs["hub"], rop, mop, xs, ys, seed=4)


@pytest.mark.parametrize("d", [16, 65, 128, 300])
@pytest.mark.parametrize("rop,mop", [("max", None), ("min", None), ("max", "mul"), ("min", "sub")])
def test_aggregate_composed_winner_path(graphs, rop, mop, d):
    """max / min through the gather composition: with an edge operand, and at widths winner_grad_supported turns away."""
    _agg_case(graphs["hub"], rop, mop, (d,), (d,) if d != 128 else (1,), seed=5)


@pytest.mark.parametrize("rop,mop,ys", [("sum", None, None), ("mean", None, None), ("max", None, None), ("min", "add", (1,)), ("sum", "mul", (40,)),
                                        ("mean", "div", (40,)), ("mean", "sub", ())])
def test_aggregate_fp64(graphs, rop, mop, ys):
    _agg_case(graphs["hub"], rop, mop, (40,), ys, dtype=torch.float64, seed=6)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("rop,mop", [("sum", None), ("mean", None), ("sum", "mul"), ("mean", "add")])
def test_aggregate_16_bit_storage(graphs, rop, mop, dtype):
    """d x of sum / mean with the features stored in 16 bits (mean: the pre-scale branch)."""
    _agg_case(graphs["hub"], rop, mop, (64,), (64,), dtype=dtype, seed=7, check=[0])


@pytest.mark.parametrize("rop,mop,ys", [("sum", None, None), ("mean", None, None), ("max", None, None), ("mean", "mul", (32,)), ("sum", "add", (1,)),
                                        ("max", "add", (32,)), ("mean", "div", ())])
def test_aggregate_out_size_beyond_the_nodes(graphs, rop, mop, ys):
    G = graphs["hub"]
    _agg_case(G, rop, mop, (32,), ys, out_size=G.n + 77, seed=8)


@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("rop,mop,ys", [("max", None, None), ("min", None, None), ("sum", "mul", "d"), ("mean", "add", ()), ("mean", "div", (1,)),
                                        ("sum", "sub", "d"), ("sum", None, None), ("mean", "mul", (1,))])
def test_aggregate_operands_at_a_misaligned_storage_offset(pgl, graphs, monkeypatch, rop, mop, ys, d):
    """x, y and the cotangent are contiguous views 4 bytes into their storage: the gradient kernels cannot use their 2- / 4-element lanes
    on them.  Expected: the same values, never an exception -- through the composed path; the ALIGNED twin of the same case still
    takes pglamd_winner_grad (max / min) / pglamd_edge_operand_grad (an operand), so the alignment term of the gates turns away
    nothing else."""
    calls = []
    for name in ("winner_grad", "edge_operand_grad"):
        real = getattr(pgl.ops, name)
        monkeypatch.setattr(pgl.ops, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    fast = None if mop is None and rop in ("sum", "mean") else "winner_grad" if mop is None else "edge_operand_grad"
    _agg_case(graphs["hub"], rop, mop, (d,), (d,) if ys == "d" else ys, seed=9, misalign=False)
    assert set(calls) == ({fast} if fast else set()), ("aligned operands", calls)
    del calls[:]
    _agg_case(graphs["hub"], rop, mop, (d,), (d,) if ys == "d" else ys, seed=9, misalign=True)
    assert not calls, ("misaligned operands", calls)


@pytest.mark.parametrize("name", ["E0", "E1", "N1"])
@pytest.mark.parametrize("rop,mop", [("sum", None), ("mean", "mul"), ("max", None), ("min", "add"), ("max", "div")])
def test_aggregate_degenerate_sizes(graphs, name, rop, mop):
    for d in (8, 128):
        _agg_case(graphs[name], rop, mop, (d,), (d,), seed=10)


def test_send_recv_scaled(graphs):
    G = graphs["hub"]
    rng = np.random.default_rng(11)
    for d in (16, 128):
        x, cot = _t(rows(rng, G.n, d)), _t(rows(rng, G.n, d))
        ss, ds = _t(rng.random(G.n) + 0.5), _t(rng.random(G.n) + 0.5)
        for a, b in ((ss, ds), (None, ds), (ss, None)):
            assert_grads(lambda t: G.g.send_recv_scaled(t, a, b), lambda t, frozen=None: D.send_recv_scaled(t, G.src, G.dst, a, b),
                         [x], cot, G.indeg + 2, [G.outdeg + 2], what="send_recv_scaled d=%d" % d)


# ------------------------------------------------------------------------------------------------
# _SendUV, _SegmentReduce, _GatherRows, _ScatterRows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xs,ys", [((48,), (48,)), ((4, 12), (4, 1)), ((1,), (48,))], ids=["d.d", "HD.H1", "1.d"])
@pytest.mark.parametrize("mop", ["add", "sub", "mul", "div"])
def test_send_uv(graphs, mop, xs, ys):
    G = graphs["hub"]
    rng = np.random.default_rng(12)
    x, y = _t(rows(rng, G.n, *xs)), _t(rng.random((G.n,) + ys) + 0.5)
    out_tail = tuple(np.broadcast_shapes(xs, ys))
    cot = _t(rows(rng, G.e, *out_tail))
    fx, fy = np.prod(out_tail) / np.prod(xs), np.prod(out_tail) / np.prod(ys)
    assert_grads(lambda a, b: G.g.send_uv(a, b, mop), lambda a, b, frozen=None: D.send_uv(a, b, G.src, G.dst, mop, frozen=frozen),
                 [x, y], cot, 1.0, [G.outdeg * fx + 2, G.indeg * fy + 2], what="send_uv %s" % mop)
    for name in ("E0", "E1", "N1"):
        g = graphs[name]
        x, y, cot = _t(rows(rng, g.n, *xs)), _t(rng.random((g.n,) + ys) + 0.5), _t(rows(rng, g.e, *out_tail))
        assert_grads(lambda a, b: g.g.send_uv(a, b, mop), lambda a, b, frozen=None: D.send_uv(a, b, g.src, g.dst, mop, frozen=frozen),
                     [x, y], cot, 1.0, [g.outdeg * fx + 2, g.indeg * fy + 2], what="send_uv %s %s" % (mop, name))


def _segment_ids(rng, n_rows=20000, n_seg=400, long=6000):
    """sorted ids with one long segment and absent ids (every 7th, and a run in the middle)."""
    present = np.array([s for s in range(n_seg) if s % 7 != 3 and not 100 <= s < 120])
    ids = np.sort(np.concatenate([rng.choice(present, n_rows - long), np.full(long, 50)]))
    ids[-1] = n_seg - 1
    return ids.astype(np.int64), n_seg


@pytest.mark.parametrize("d", [1, 33, 128])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("pool", ROPS)
def test_segment_pools(pgl, pool, idt, d):
    rng = np.random.default_rng(13)
    ids_np, n_seg = _segment_ids(rng)
    ids = torch.as_tensor(ids_np, device=DEVICE)
    data = _t(ints(rng, len(ids_np), d) if pool in ("max", "min") else rows(rng, len(ids_np), d))
    cot = _t(rows(rng, n_seg, d))
    cnt = D.degree(ids, n_seg).double()
    assert_grads(lambda a: getattr(pgl.math, "segment_" + pool)(a, ids.to(idt)),
                 lambda a, frozen=None: D.segment_pool(a, ids, pool, n_seg, frozen=frozen), [data], cot,
                 cnt + (1.0 if pool == "mean" else 0.0), [2.0], lambda a: D.segment_frozen(a, ids, pool, n_seg), what="segment_%s d=%d" % (pool, d))


def test_gather_and_scatter_rows(graphs):
    from pgl_amd import autograd as ag
    G = graphs["hub"]
    rng = np.random.default_rng(14)
    for d in (5, 128):
        x = _t(rows(rng, G.n, d))
        src32, _ = G.g._edge_cols32()
        # the graph's own index (the backward is one aggregation over the cached src-keyed CSR)
        assert_grads(lambda a: ag.gather_rows(a, src32, G.g._csr_src), lambda a, frozen=None: D.gather(a, G.src), [x], _t(rows(rng, G.e, d)),
                     1.0, [G.outdeg + 1], what="gather by src d=%d" % d)
        # an arbitrary repeated index, int64 and int32 (the backward keys it on the fly); some rows never read, one read 5000 times
        idx = rng.integers(0, G.n // 2, 30000); idx[rng.choice(30000, 5000, replace=False)] = 7
        idx = torch.as_tensor(idx, device=DEVICE)
        for ix in (idx, idx.to(torch.int32)):
            assert_grads(lambda a: ag.gather_rows(a, ix), lambda a, frozen=None: D.gather(a, idx), [x], _t(rows(rng, 30000, d)),
                         1.0, [D.degree(idx, G.n).double() + 1], what="gather by an arbitrary index d=%d" % d)
        uniq = torch.as_tensor(rng.permutation(G.n + 50)[:G.n], device=DEVICE)
        assert_grads(lambda a: ag.scatter_into_zeros(G.n + 50, uniq, a), lambda a, frozen=None: D.scatter_into_zeros(a, uniq, G.n + 50),
                     [x], _t(rows(rng, G.n + 50, d)), 1.0, [1.0], what="scatter d=%d" % d)
    empty = torch.zeros(0, dtype=torch.int64, device=DEVICE)
    x = _t(rows(rng, 6, 8))
    assert_grads(lambda a: ag.gather_rows(a, empty), lambda a, frozen=None: D.gather(a, empty), [x], _t(np.zeros((0, 8))), 1.0, [1.0],
                 what="gather by an empty index")


# ------------------------------------------------------------------------------------------------
# _SegmentSoftmax
# ------------------------------------------------------------------------------------------------
def _softmax_case(eng, ids, n_seg, n_rows, d, seed, what):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_rows, d)) * 3
    x[n_rows // 3] += 80.0                                                # one row of large logits
    x, cot = _t(x), _t(rows(rng, n_rows, d))
    out_t, g_t, n_t = D.segment_softmax_terms(x, ids, n_seg, cot)
    assert_grads(eng, lambda a, frozen=None: D.segment_softmax(a, ids, n_seg), [x], cot, terms={"out": (out_t, n_t), 0: (g_t, n_t)},
                 family="softmax", what=what)


SOFTMAX_D = [1, 8, 100]


@pytest.mark.parametrize("d", SOFTMAX_D)
def test_segment_softmax_over_sorted_data(pgl, d):
    rng = np.random.default_rng(15)
    ids_np = np.sort(np.concatenate([rng.integers(0, 500, 20000), np.full(30000, 250)])).astype(np.int64)    # one segment of 30 k rows
    ids_np[-1] = 499
    ids = torch.as_tensor(ids_np, device=DEVICE)
    _softmax_case(lambda a: pgl.math.segment_softmax(a, ids), ids, 500, len(ids_np), d, 16, "segment_softmax d=%d" % d)


@pytest.fixture(scope="module")
def softmax_graph(pgl):
    return _softmax_graph(pgl)


def _softmax_graph(pgl_):
    rng = np.random.default_rng(17)
    n, e = 2000, 50000
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    dst[:30000] = 11                                                      # a destination and a source with 30 k edges each
    src[20000:50000] = 13
    return _G(pgl_, n, src, dst)


@pytest.mark.parametrize("d", SOFTMAX_D)
@pytest.mark.parametrize("by", ["dst", "src"])
def test_edge_softmax(pgl, softmax_graph, by, d):
    G = softmax_graph
    ids = G.dst if by == "dst" else G.src
    _softmax_case(lambda a: pgl.nn.functional.edge_softmax(G.g, a, by), ids, G.n, G.e, d, 18, "edge_softmax by %s d=%d" % (by, d))


# ------------------------------------------------------------------------------------------------
# _SDDMM, _AddScore, _GatAttention, _GatAttentionProj
# ------------------------------------------------------------------------------------------------
def _both_graphs(hds):
    """(graph, H, D) over the hub graph (ids as before the classes graph existed: H-D) and the classes graph (classes-H-D)."""
    return [pytest.param(name, H, D_, id=("%d-%d" if name == "hub" else name + "-%d-%d") % (H, D_)) for name in ("hub", "classes") for H, D_ in hds]


def test_classes_graph_has_every_class_of_split_row(pgl, graphs):
    """The classes graph keeps a row on each side of the short / long fix-up boundary (16 | 17 further pieces) on both streams, for
    the chunk length the library really uses at this size: a change of the chunk rule fails here instead of moving the boundary away
    from every graph of the suite."""
    G = graphs["classes"]
    assert 10000 <= G.e <= 15000 and G.n == 3000
    assert int(pgl.ops._ffi.lib().pglamd_add_score_chunks(G.e)) == -(-G.e // CHUNK)
    for ids in (G.dst_np, G.src_np):
        pieces = further_pieces(ids, G.n)
        assert pieces[:5].tolist() == [16, 0, 17, 1, 47]
        assert {1, 16, 17} <= set(pieces.tolist()) and pieces.max() >= 40
        assert np.bincount(ids, minlength=G.n)[pieces == 0].max() >= 63       # an unsplit row that nearly fills a chunk


def _orders(G):
    """(dst-keyed index, src-keyed index, src, dst) with edge tensors in original edge order, and in destination-sorted order."""
    if G.g is None:
        return [("edge", None, None, G.src, G.dst), ("csr", None, None, G.src, G.dst)]
    cd, cs = G.g._csr_dst(), G.g._csr_src()
    vd, vs = G.g._csr_order_views()
    return [("edge", cd, cs, G.src, G.dst), ("csr", vd, vs, vd.col32.long(), vd.row32.long())]


# (4, 8) / (8, 16) / (8, 32): one lane holds 1 / 2 / 4 columns -- gat_vec takes the smallest width that fits 64 lanes
@pytest.mark.parametrize("graph,H,D_", _both_graphs([(4, 8), (8, 16), (2, 32), (1, 64), (8, 32)]))
def test_sddmm(graphs, graph, H, D_):
    from pgl_amd import autograd as ag
    G = graphs[graph]
    rng = np.random.default_rng(19 + H)
    x, y = _t(rows(rng, G.n, H, D_)), _t(rows(rng, G.n, H, D_))
    cot = _t(rows(rng, G.e, H))
    for name, cd, cs, src, dst in _orders(G):
        assert_grads(lambda a, b: ag.sddmm(a, b, cd, lambda: cs), lambda a, b, frozen=None: D.sddmm(a, b, src, dst), [x, y], cot,
                     D_ + 1.0, [G.outdeg + 2, G.indeg + 2], what="sddmm %s %dx%d %s order" % (graph, H, D_, name))
    assert_grads(lambda a, b: G.g.sddmm(a, b), lambda a, b, frozen=None: D.sddmm(a, b, G.src, G.dst), [x, y], cot,
                 D_ + 1.0, [G.outdeg + 2, G.indeg + 2], what="Graph.sddmm %s %dx%d" % (graph, H, D_))


SCORE_HD, GAT_HD, GAT_PROJ_HD = [(4, 8), (8, 16), (1, 64), (3, 4), (8, 32)], [(8, 16), (4, 8), (1, 64), (2, 32), (8, 32)], [(8, 16), (4, 8)]


@pytest.mark.parametrize("graph,H,D_", _both_graphs(SCORE_HD))
def test_additive_score(graphs, graph, H, D_):
    from pgl_amd import autograd as ag
    G = graphs[graph]
    rng = np.random.default_rng(23 + H)
    x, y = lattice(rng, True, G.n, H, D_), lattice(rng, False, G.n, H, D_)
    assert np.abs(x[G.src_np] + y[G.dst_np]).min() >= Q > 1e-4               # no pre-activation near the kink (fp64 side)
    x, y, w = _t(x), _t(y), _t(rows(rng, H, D_))
    cot = _t(rows(rng, G.e, H))
    for name, cd, cs, src, dst in _orders(G):
        assert_grads(lambda a, b, c: ag.add_score(a, b, c, cd, lambda: cs, 0.2),
                     lambda a, b, c, frozen=None: D.add_score(a, b, c, src, dst, 0.2, frozen=frozen), [x, y, w], cot,
                     D_ + 2.0, [G.outdeg + 2, G.indeg + 2, float(G.e) + 2], lambda a, b, c: D.add_score_frozen(a, b, c, src, dst, 0.2),
                     family="add_score", what="add_score %s %dx%d %s order" % (graph, H, D_, name))


def _gat_terms(res, keys):
    t = {"out": res["out"]}
    t.update({i: res[k] for i, k in enumerate(keys)})
    return t


@pytest.mark.parametrize("graph,H,D_", _both_graphs(GAT_HD))
def test_gat_attention(graphs, graph, H, D_):
    G = graphs[graph]
    rng = np.random.default_rng(29 + H)
    a_s, a_d = lattice(rng, True, G.n, H), lattice(rng, False, G.n, H)
    assert np.abs(a_s[G.src_np] + a_d[G.dst_np]).min() >= Q > 1e-4
    f, a_s, a_d, cot = _t(rows(rng, G.n, H, D_)), _t(a_s), _t(a_d), _t(rows(rng, G.n, H, D_))
    terms = _gat_terms(D.gat_terms(f, a_s, a_d, G.src, G.dst, cot), ("f", "a_s", "a_d"))
    assert_grads(lambda a, b, c: G.g.gat_aggregate(a, b, c, 0.2), lambda a, b, c, frozen=None: D.gat(a, b, c, G.src, G.dst, 0.2),
                 [f, a_s, a_d], cot, terms=terms, family="gat", what="gat %s %dx%d" % (graph, H, D_))


GAT_BACKWARD_ROUTES = {"positive-part statistics": (True, True), "edge buffer": (False, True), "two walks": (False, False)}


@pytest.mark.parametrize("H,D_", [(4, 8), (8, 16), (8, 32)])
@pytest.mark.parametrize("route", list(GAT_BACKWARD_ROUTES))
def test_gat_attention_over_every_backward_route(pgl, graphs, route, H, D_):
    """The three ways to d a_dst (tests/test_a13_f1_layers.py test_gat_backward_variants_agree), each held to the fp64 gradients on the
    classes graph: the forward with and without the positive-part statistics, the src-sorted walk with and without the d pre_e buffer,
    and the dst-sorted walk -- at 1, 2 and 4 columns per lane."""
    keep = (pgl.ops._GAT_POS_STATS, pgl.ops._GAT_BWD_EDGE_BUFFER)
    try:
        pgl.ops._GAT_POS_STATS, pgl.ops._GAT_BWD_EDGE_BUFFER = GAT_BACKWARD_ROUTES[route]
        test_gat_attention(graphs, "classes", H, D_)
    finally:
        pgl.ops._GAT_POS_STATS, pgl.ops._GAT_BWD_EDGE_BUFFER = keep


def _gat_proj_data(G, H, D_):
    """feature integers with a constant-1 column per head, proj even multiples of Q except the rows of those columns, which add Q to
    a_src: every a_src is an odd, every a_dst an even multiple of Q -- exactly, in any summation order.
    -> (f, proj, cot, att = f2d @ proj) on the device."""
    rng = np.random.default_rng(31 + H)
    f = rng.integers(-2, 3, (G.n, H, D_)).astype(np.float64)
    f[:, :, 0] = 1.0
    proj = rng.integers(-3, 4, (H * D_, 2 * H)) * 2 * Q
    proj = proj * (np.arange(H * D_)[:, None] // D_ == np.arange(2 * H)[None, :] % H)          # block diagonal, as GATConv builds it
    for h in range(H):
        proj[h * D_, :] = 0.0
        proj[h * D_, h] = Q
    att = f.reshape(G.n, -1) @ proj
    assert np.abs(att[G.src_np, :H] + att[G.dst_np, H:]).min() >= Q > 1e-4
    return _t(f), _t(proj), _t(rows(rng, G.n, H, D_)), _t(att)


def _gat_proj_case(G, H, D_, check=None, what=""):
    f, proj, cot, att = _gat_proj_data(G, H, D_)
    terms = _gat_terms(D.gat_terms(f, att[:, :H], att[:, H:], G.src, G.dst, cot, proj=proj), ("f", "proj"))
    assert_grads(lambda a, p: G.g.gat_aggregate_proj(a, p, 0.2), lambda a, p, frozen=None: D.gat_proj(a, p, G.src, G.dst, 0.2),
                 [f, proj], cot, terms=terms, family="gat_proj", check=check, what="gat_proj %dx%d%s" % (H, D_, what))


@pytest.mark.parametrize("H,D_", GAT_PROJ_HD)
def test_gat_attention_with_the_projection_inside(graphs, H, D_):
    _gat_proj_case(graphs["hub"], H, D_)


# Attention dropout (the cases of tests/test_gat_dropout_gpu.py; they live here so that _measure_definitions() runs them too).  The
# engine regenerates its mask from (seed, original edge id, head); the definition takes the keep factor grad_defs.attention_keep
# restates from include/pgl_amd.h -- G.src / G.dst are in original edge order, so edge e's factor is row e.
GAT_DROP_SEEDS = {0.6: 1234, 0.1: 3000000019, 0.9: 2 ** 32 - 5}          # (two of them >= 2**31, passed as Python ints)


def _gat_drop_case(G, graph, H, D_, p, keep=None, mutant=None, forward=True, check=None, what=""):
    """test_gat_attention's data through g.gat_aggregate(..., p, seed) against D.gat(keep=...).  keep / mutant: a WRONG definition
    (the self-checks); default: the documented mask."""
    seed = GAT_DROP_SEEDS[p]
    rng = np.random.default_rng(29 + H)
    a_s, a_d = lattice(rng, True, G.n, H), lattice(rng, False, G.n, H)
    assert np.abs(a_s[G.src_np] + a_d[G.dst_np]).min() >= Q > 1e-4
    f, a_s, a_d, cot = _t(rows(rng, G.n, H, D_)), _t(a_s), _t(a_d), _t(rows(rng, G.n, H, D_))
    kd = _t(D.attention_keep(seed, np.arange(G.e), H, p) if keep is None else keep)
    terms = _gat_terms(D.gat_terms(f, a_s, a_d, G.src, G.dst, cot, keep=kd), ("f", "a_s", "a_d"))
    assert_grads(lambda a, b, c: G.g.gat_aggregate(a, b, c, 0.2, p, seed),
                 lambda a, b, c, frozen=None: D.gat(a, b, c, G.src, G.dst, 0.2, keep=kd, mutant=mutant),
                 [f, a_s, a_d], cot, terms=terms, family="gat_drop", forward=forward, check=check,
                 what="gat %s %dx%d p=%g%s" % (graph, H, D_, p, what))
    return f, a_s, a_d, cot, kd, seed


def _gat_proj_drop_case(G, H, D_, p):
    """_gat_proj_case's data with dropout on."""
    seed = GAT_DROP_SEEDS[p]
    f, proj, cot, att = _gat_proj_data(G, H, D_)
    kd = _t(D.attention_keep(seed, np.arange(G.e), H, p))
    terms = _gat_terms(D.gat_terms(f, att[:, :H], att[:, H:], G.src, G.dst, cot, proj=proj, keep=kd), ("f", "proj"))
    assert_grads(lambda a, q: G.g.gat_aggregate_proj(a, q, 0.2, p, seed), lambda a, q, frozen=None: D.gat_proj(a, q, G.src, G.dst, 0.2, keep=kd),
                 [f, proj], cot, terms=terms, family="gat_proj_drop", what="gat_proj %dx%d p=%g" % (H, D_, p))


GAT_DROP_EXTRA_P = [(0.1, 8, 16), (0.9, 8, 16)]


# ------------------------------------------------------------------------------------------------
# _PropagateStep, _RowEpilogue, _AggregateDense, _DualLinear, _AggregateDualLinear
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 128])
def test_propagate_step(graphs, d):
    G = graphs["hub"]
    rng = np.random.default_rng(37)
    x, res, cot, ds = _t(rows(rng, G.n, d)), _t(rows(rng, G.n, d)), _t(rows(rng, G.n, d)), _t(rng.random(G.n) + 0.5)
    assert_grads(lambda a: G.g.propagate_step(a, ds), lambda a, frozen=None: D.propagate_step(a, None, G.src, G.dst, ds), [x], cot,
                 G.indeg + 2, [G.outdeg + 2], what="propagate d=%d" % d)
    assert_grads(lambda a, r: G.g.propagate_step(a, ds, r, -0.3),
                 lambda a, r, frozen=None: D.propagate_step(a, r, G.src, G.dst, ds, -0.3, frozen=frozen), [x, res], cot,
                 G.indeg + 3, [G.outdeg + 2, 1.0], what="propagate with a residual d=%d" % d)


EPILOGUE_D = [7, 64, 100, 256]
EPILOGUE_MODES = [(None, True, True), ("relu", True, True), ("relu", False, True), ("relu", True, False), (None, False, True)]


@pytest.mark.parametrize("d", EPILOGUE_D)
@pytest.mark.parametrize("act,normalize,bias", EPILOGUE_MODES)
def test_row_epilogue(pgl, act, normalize, bias, d):
    from pgl_amd import autograd as ag
    rng = np.random.default_rng(41 + d)
    n = 5000
    z, b = lattice(rng, True, n, d), lattice(rng, False, d) if bias else None
    assert np.abs(z + (b if bias else 0.0)).min() >= Q > 1e-4             # no pre-activation near relu's kink (fp64 side)
    z, b, cot = _t(z), (_t(b) if bias else None), _t(rows(rng, n, d))
    res = D.row_epilogue_terms(z, b, act, normalize, cot)
    if bias:
        assert_grads(lambda a, c: ag.row_epilogue(a, c, act, normalize), lambda a, c, frozen=None: D.row_epilogue(a, c, act, normalize),
                     [z, b], cot, terms={"out": res["out"], 0: res["z"], 1: res["bias"]}, family="row_epilogue",
                     what="row_epilogue %s normalize=%s d=%d" % (act, normalize, d))
    else:
        assert_grads(lambda a: ag.row_epilogue(a, None, act, normalize), lambda a, frozen=None: D.row_epilogue(a, None, act, normalize),
                     [z], cot, terms={"out": res["out"], 0: res["z"]}, family="row_epilogue",
                     what="row_epilogue %s normalize=%s no bias d=%d" % (act, normalize, d))


def _dense_counts(G, d_in, d_out, n_agg_out, n_agg_in):
    """out: an aggregation then d_in products; d x: d_out products then the transposed aggregation; d W: one product per node of an
    aggregated row; d b: a column sum."""
    n_x = n_agg_in + d_out + 3
    return n_agg_out + d_in + 3, [n_x, float(G.n) + float(G.indeg.max()) + 3, float(G.n) + 1]


DENSE_CASES = [(64, 32, "sum", "relu", True), (128, 64, "sum", "relu", False), (128, 48, "mean", None, True), (64, 128, "sum", None, True),
               (128, 16, "mean", None, False)]
DUAL_CASES = [(64, 32), (128, 128), (100, 47)]


def _dense_case(G, d_in, d_out, rop, act, scaled):
    """relu: integers, power-of-two scales and weights on a lattice, the bias an ODD multiple of a finer step -- the pre-activation is
    never 0 and at least 2**-8 from it; without an activation: free data with scaled rows."""
    rng = np.random.default_rng(43 + d_in + d_out)
    ss = ds = None
    if act == "relu":
        x = rng.integers(-1, 2, (G.n, d_in)).astype(np.float64)
        w = rng.integers(-4, 5, (d_out, d_in)) / 8.0
        b = (rng.integers(-64, 64, d_out) * 2 + 1) * 2.0 ** -8
        if scaled:
            ss, ds = 2.0 ** -rng.integers(0, 3, G.n).astype(np.float64), 2.0 ** -rng.integers(0, 3, G.n).astype(np.float64)
    else:
        x, w, b = rows(rng, G.n, d_in), rng.standard_normal((d_out, d_in)) / np.sqrt(d_in), rng.standard_normal(d_out)
        if scaled:
            ss, ds = rng.random(G.n) + 0.5, rng.random(G.n) + 0.5
    x, w, b, cot = _t(x), _t(w), _t(b), _t(rows(rng, G.n, d_out))
    ss, ds = (None if ss is None else _t(ss)), (None if ds is None else _t(ds))
    fr = lambda a, ww, bb: D.dense_frozen(a, ww, bb, G.src, G.dst, act, ss, ds, rop)
    if act == "relu":
        pre = fr(x.double(), w.double(), b.double())["pre"]
        assert float(pre.abs().min()) >= 2.0 ** -8 > 1e-4
    n_out, n_terms = _dense_counts(G, d_in, d_out, G.indeg, G.outdeg)
    assert_grads(lambda a, ww, bb: G.g.send_recv_dense(a, ww, bb, act, ss, ds, rop),
                 lambda a, ww, bb, frozen=None: D.aggregate_dense(a, ww, bb, G.src, G.dst, act, ss, ds, rop, frozen=frozen),
                 [x, w, b], cot, n_out, n_terms, fr, family="dense", what="dense %d->%d %s %s" % (d_in, d_out, rop, act))


@pytest.mark.parametrize("d_in,d_out,rop,act,scaled", DENSE_CASES)
def test_aggregate_dense(graphs, d_in, d_out, rop, act, scaled):
    _dense_case(graphs["hub"], d_in, d_out, rop, act, scaled)


def _dual_case(G, d_in, d_out):
    from pgl_amd import autograd as ag
    rng = np.random.default_rng(47 + d_in)
    x, y, cot = _t(rows(rng, G.n, d_in)), _t(rows(rng, G.n, d_in)), _t(rows(rng, G.n, d_out))
    wa, wb = (_t(rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)) for _ in range(2))
    assert_grads(lambda a, b, p, q: ag.dual_linear(a, b, p, q), lambda a, b, p, q, frozen=None: D.dual_linear(a, b, p, q), [x, y, wa, wb], cot,
                 2.0 * d_in + 1, [d_out + 1.0, d_out + 1.0, float(G.n) + 1, float(G.n) + 1], family="dual_linear", what="dual_linear %d->%d" % (d_in, d_out))
    for rop in ("sum", "mean"):
        n_out, n_terms = _dense_counts(G, 2 * d_in, d_out, G.indeg, G.outdeg)
        assert_grads(lambda a, p, q: G.g.send_recv_dual_linear(a, p, q, rop),
                     lambda a, p, q, frozen=None: D.aggregate_dual_linear(a, p, q, G.src, G.dst, rop), [x, wa, wb], cot,
                     n_out, [n_terms[0], n_terms[1], n_terms[1]], family="dual_linear", what="aggregate_dual_linear %d->%d %s" % (d_in, d_out, rop))


@pytest.mark.parametrize("d_in,d_out", DUAL_CASES)
def test_dual_linear_forms(graphs, d_in, d_out):
    _dual_case(graphs["hub"], d_in, d_out)


@pytest.fixture(scope="module")
def tall_graph(pgl):
    return _tall_graph(pgl)


def _tall_graph(pgl_):
    rng = np.random.default_rng(67)
    n, e = 70001, 200000                                                  # 70001 = 256 * 273 + 113: the split reductions leave a remainder slab
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    dst[:600], src[600:1200] = 9, 11
    return _G(pgl_, n, src, dst)


TALL_CASES = ["dense", "dual", "gat_proj", "gat_proj weights only"]


@pytest.mark.parametrize("case", TALL_CASES)
def test_weight_gradients_over_more_than_65536_rows(tall_graph, case):
    """N >= 65536: weight and bias gradients take the split reductions (_tall_wgrad's batched slabs, column_sum's two stages); and the
    projection's gradient alone, the feature needing none."""
    if case == "dense":
        _dense_case(tall_graph, 128, 32, "sum", None, False)
    elif case == "dual":
        _dual_case(tall_graph, 64, 32)
    else:
        _gat_proj_case(tall_graph, 4, 8, check=None if case == "gat_proj" else [1], what=" N=%d %s" % (tall_graph.n, case))


# ------------------------------------------------------------------------------------------------
# the harness checks itself ON THE DEVICE: the real kernels' gradients against a MUTATED definition must be refused
# ------------------------------------------------------------------------------------------------
def test_the_bound_refuses_a_dropped_edge_on_a_small_row(graphs):
    """The mutant loses one edge whose destination's cotangent is 1e-4 of the others: d x of its source (a node of ordinary out-degree)
    is wrong by a term 1e-4 of the row's others -- what a tolerance tied to max|want| cannot see.  The forward is NOT compared here:
    the refusal has to come from d x."""
    G = graphs["hub"]
    rng = np.random.default_rng(53)
    d = 32
    x, y = _t(rng.standard_normal((G.n, d))), _t(rng.random((G.e, d)) + 0.5)
    ok = (G.dst_np != 70) & (G.src_np != 60)
    k = int(np.flatnonzero(ok)[np.argmin(np.bincount(G.src_np, minlength=G.n)[G.src_np[ok]])])   # the edge the mutant loses: its source has the fewest out-edges
    w = rng.standard_normal((G.n, d)); w[G.dst_np[k]] *= 1e-4
    n_out, n_terms = D.aggregate_n_terms(G.src, G.dst, x.shape, y.shape, "sum")
    eng = lambda a, b: G.g.send_ue_recv(a, b, "mul", "sum")
    good = lambda a, b, frozen=None: D.send_recv(a, G.src, G.dst, "sum", None, b, "mul", frozen=frozen)
    bad = lambda a, b, frozen=None: D.send_recv(a, G.src, G.dst, "sum", None, b, "mul", frozen=frozen, mutant={"drop_edge": k})
    assert_grads(eng, good, [x, y], _t(w), n_out, n_terms, what="mul/sum")
    with pytest.raises(AssertionError, match="d input 0: .*out of bound"):
        assert_grads(eng, bad, [x, y], _t(w), n_out, n_terms, forward=False, what="mul/sum vs a definition that drops edge %d" % k)
    with pytest.raises(AssertionError, match="d input 1: .*out of bound"):
        assert_grads(eng, bad, [x, y], _t(w), n_out, n_terms, forward=False, check=[1], what="mul/sum vs a definition that drops edge %d" % k)
    # and the old tolerance would have let the engine's d x pass against the mutant's
    r = D.grad_and_terms(bad, [x, y], _t(w), n_out, n_terms)
    xs = x.detach().requires_grad_(True)
    eng(xs, y).backward(_t(w))
    assert float((xs.grad.double() - r.want64[0]).abs().max()) <= 2e-5 * float(r.want64[0].abs().max()) + 1e-7


@pytest.mark.parametrize("rop", ["max", "min"])
def test_the_bound_refuses_evenly_split_ties(graphs, rop):
    G = graphs["hub"]
    rng = np.random.default_rng(59)
    x, cot = _t(ints(rng, G.n, 64)), _t(rows(rng, G.n, 64))
    n_out, n_terms = D.aggregate_n_terms(G.src, G.dst, x.shape, None, rop)
    eng = lambda a: G.g.send_recv(a, rop)
    fr = lambda a: D.winner_mask(a, G.src, G.dst, rop)
    assert_grads(eng, lambda a, frozen=None: D.send_recv(a, G.src, G.dst, rop, frozen=frozen), [x], cot, n_out, n_terms[:1], fr, what=rop)
    with pytest.raises(AssertionError, match="d input 0: .*out of bound"):
        assert_grads(eng, lambda a, frozen=None: D.send_recv(a, G.src, G.dst, rop, frozen=frozen, mutant={"split_ties": True}), [x], cot,
                     n_out, n_terms[:1], fr, forward=False, what=rop + " vs a definition that splits ties")


def test_the_bound_refuses_a_forgotten_mean_divisor(graphs):
    G = graphs["hub"]
    rng = np.random.default_rng(61)
    x, cot = _t(rows(rng, G.n, 128)), _t(rows(rng, G.n, 128))
    n_out, n_terms = D.aggregate_n_terms(G.src, G.dst, x.shape, None, "mean")
    eng = lambda a: G.g.send_recv(a, "mean")
    assert_grads(eng, lambda a, frozen=None: D.send_recv(a, G.src, G.dst, "mean"), [x], cot, n_out, n_terms[:1], what="mean")
    with pytest.raises(AssertionError, match="d input 0: .*out of bound"):
        assert_grads(eng, lambda a, frozen=None: D.send_recv(a, G.src, G.dst, "mean", mutant={"no_deg_row": 70}), [x], cot, n_out, n_terms[:1],
                     forward=False, what="mean vs a definition without 1 / deg on the hub row")


# ------------------------------------------------------------------------------------------------
# how the K table in the module docstring was measured (fp32 torch on the host; nothing of the engine runs)
# ------------------------------------------------------------------------------------------------
def _measure_definitions():
    """-> {family: the worst err / bound of the fp32 definition over the family's cases}."""
    global DEVICE, _MEASURED
    keep, DEVICE, _MEASURED = DEVICE, "cpu", {}
    try:
        gs, sg = _graphs(None), _softmax_graph(None)
        for d in SOFTMAX_D:
            test_segment_softmax_over_sorted_data(None, d)
            for by in ("dst", "src"):
                test_edge_softmax(None, sg, by, d)
        for graph in ("hub", "classes"):
            for hd in SCORE_HD:
                test_additive_score(gs, graph, *hd)
            for hd in GAT_HD:
                test_gat_attention(gs, graph, *hd)
        for hd in GAT_PROJ_HD:
            test_gat_attention_with_the_projection_inside(gs, *hd)
        for graph in ("hub", "classes"):                                 # attention dropout: tests/test_gat_dropout_gpu.py
            for hd in GAT_HD:
                _gat_drop_case(gs[graph], graph, *hd, 0.6)
            for p, H, D_ in GAT_DROP_EXTRA_P:
                _gat_drop_case(gs[graph], graph, H, D_, p)
        for hd in GAT_PROJ_HD:
            _gat_proj_drop_case(gs["hub"], *hd, 0.6)
        for d in EPILOGUE_D:
            for mode in EPILOGUE_MODES:
                test_row_epilogue(None, *mode, d)
        for case in DENSE_CASES:
            test_aggregate_dense(gs, *case)
        for case in DUAL_CASES:
            test_dual_linear_forms(gs, *case)
        tall = _tall_graph(None)
        for case in TALL_CASES:
            test_weight_gradients_over_more_than_65536_rows(tall, case)
        return dict(_MEASURED)
    finally:
        DEVICE, _MEASURED = keep, None
