"""The gradient DEFINITIONS (tests/grad_defs.py) and the per-element bound, checked without a GPU.

Why this file exists: a gradient tolerance tied to the LARGEST element of the tensor cannot see an error on a small row.
`test_dropped_edge_on_a_small_row_*` drops one edge's term on a destination whose cotangent is 1e-4 of the others: the old checks
(`<= 2e-5 * want.abs().max() + 1e-7`) pass the wrong gradient, the per-element bound flags it."""
import numpy as np
import pytest
import torch

import grad_defs as D
import ref_ops as R


def t64(a):
    return torch.as_tensor(np.ascontiguousarray(a))


def small_graph(n=12, e=30, seed=0):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e), rng.integers(0, n - 2, e)          # (the last two nodes receive nothing)
    src[:3], dst[:3] = 1, 2                                              # multi-edges
    src[3], dst[3] = 4, 4                                                # a self-loop
    return rng, n, e, src.astype(np.int64), dst.astype(np.int64)


ROPS, MOPS = ("sum", "mean", "max", "min"), ("add", "sub", "mul", "div")
SHAPES = [((6,), (6,)), ((6,), (1,)), ((6,), ()), ((2, 3), (2, 3)), ((2, 3), (2, 1)), ((2, 1), (2, 3)), ((2, 3), (1, 3))]


# ------------------------------------------------------------------------------------------------
# forwards == the oracle's numpy restatements, in fp64
# ------------------------------------------------------------------------------------------------
def _same(got, want, exact=False):
    got = got.numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    if exact:
        assert np.array_equal(got, want)
    else:
        assert (np.abs(got - want) <= 1e-12 * np.abs(want) + 1e-300).all()


@pytest.mark.parametrize("out_size", [None, 15])
@pytest.mark.parametrize("rop", ROPS)
def test_send_u_recv_forward_equals_the_oracle(rop, out_size):
    rng, n, e, src, dst = small_graph()
    x = rng.standard_normal((n, 5))
    _same(D.send_recv(t64(x), t64(src), t64(dst), rop, out_size), R.np_send_u_recv(x, src, dst, rop, out_size), rop in ("max", "min"))


@pytest.mark.parametrize("xs,ys", SHAPES)
@pytest.mark.parametrize("mop", MOPS)
@pytest.mark.parametrize("rop", ROPS)
def test_send_ue_recv_forward_equals_the_oracle(rop, mop, xs, ys):
    rng, n, e, src, dst = small_graph(seed=1)
    x, y = rng.standard_normal((n,) + xs), rng.random((e,) + ys) + 0.5
    for out_size in (None, 14):
        got = D.send_recv(t64(x), t64(src), t64(dst), rop, out_size, t64(y), mop)
        y_np = y if ys else y.reshape((e,) + (1,) * len(xs))           # (the oracle takes [E] as the column it stands for)
        _same(got, R.np_send_ue_recv(x, y_np, src, dst, mop, rop, out_size), rop in ("max", "min"))


@pytest.mark.parametrize("mop", MOPS)
def test_send_uv_forward_equals_the_oracle(mop):
    rng, n, e, src, dst = small_graph(seed=2)
    for xs, ys in (((6,), (6,)), ((2, 3), (2, 1)), ((1,), (6,))):
        x, y = rng.standard_normal((n,) + xs), rng.random((n,) + ys) + 0.5
        _same(D.send_uv(t64(x), t64(y), t64(src), t64(dst), mop), R.np_send_uv(x, y, src, dst, mop), True)


@pytest.mark.parametrize("pool", ROPS)
def test_segment_forward_equals_the_oracle(pool):
    rng = np.random.default_rng(3)
    ids = np.sort(rng.choice([0, 1, 2, 4, 7], 40)).astype(np.int64)     # ids 3, 5, 6 absent
    ids[-1] = 7
    data = rng.standard_normal((40, 4))
    _same(D.segment_pool(t64(data), t64(ids), pool, 8), R.np_segment(data, ids, pool), pool in ("max", "min"))


def test_softmax_forwards_equal_the_oracle():
    rng, n, e, src, dst = small_graph(seed=4)
    ids = np.sort(rng.integers(0, 6, 40)).astype(np.int64); ids[-1] = 5
    data = rng.standard_normal((40, 3)) * 3
    _same(D.segment_softmax(t64(data), t64(ids), 6), R.np_segment_softmax(data, ids))
    logits = rng.standard_normal((e, 4)) * 3
    edges = np.stack([src, dst], 1)
    _same(D.segment_softmax(t64(logits), t64(dst), n), R.np_edge_softmax(edges, n, logits, "dst"))
    _same(D.segment_softmax(t64(logits), t64(src), n), R.np_edge_softmax(edges, n, logits, "src"))


# ------------------------------------------------------------------------------------------------
# the smooth definitions pass gradcheck
# ------------------------------------------------------------------------------------------------
def _away_from_zero(a, margin=0.05):
    return np.where(np.abs(a) < margin, np.sign(a + 1e-30) * margin * 2, a)


def _gradcheck(fn, *arrays):
    xs = [t64(a).double().requires_grad_(True) for a in arrays]
    assert torch.autograd.gradcheck(fn, xs, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("mop", (None,) + MOPS)
@pytest.mark.parametrize("rop", ("sum", "mean"))
def test_gradcheck_aggregations(rop, mop):
    rng, n, e, src, dst = small_graph(seed=5)
    s, d = t64(src), t64(dst)
    x = rng.standard_normal((n, 2, 3))
    if mop is None:
        _gradcheck(lambda a: D.send_recv(a, s, d, rop, 14), x)
    else:
        for ys in ((2, 3), (2, 1), ()):
            _gradcheck(lambda a, b: D.send_recv(a, s, d, rop, None, b, mop), x, rng.random((e,) + ys) + 0.5)


def test_gradcheck_the_other_smooth_definitions():
    rng, n, e, src, dst = small_graph(seed=6)
    s, d = t64(src), t64(dst)
    H, Dh = 2, 3
    x, y = rng.standard_normal((n, H, Dh)), rng.random((n, H, Dh)) + 0.5
    for mop in MOPS:
        _gradcheck(lambda a, b: D.send_uv(a, b, s, d, mop), x, y)
        _gradcheck(lambda a, b: D.send_uv(a, b, s, d, mop), x, y[:, :, :1])
    ids = t64(np.sort(rng.choice([0, 1, 3], 20)))
    data = rng.standard_normal((20, 4))
    for pool in ("sum", "mean"):
        _gradcheck(lambda a: D.segment_pool(a, ids, pool, 5), data)
    _gradcheck(lambda a: D.segment_softmax(a, ids, 5), data)
    _gradcheck(lambda a: D.segment_softmax(a, d, n), rng.standard_normal((e, 3)))
    _gradcheck(lambda a: D.segment_softmax(a, s, n), rng.standard_normal((e, 3)))
    _gradcheck(lambda a: D.gather(a, s), x)
    uniq = t64(rng.permutation(n)[:7])
    _gradcheck(lambda a: D.scatter_into_zeros(a, uniq, n), rng.standard_normal((7, 4)))
    _gradcheck(lambda a, b: D.sddmm(a, b, s, d), x, y)
    ss, ds = t64(rng.random(n) + 0.5), t64(rng.random(n) + 0.5)
    x2 = rng.standard_normal((n, 4))
    _gradcheck(lambda a: D.send_recv_scaled(a, s, d, ss, ds), x2)
    _gradcheck(lambda a, r: D.propagate_step(a, r, s, d, ds, -0.3), x2, rng.standard_normal((n, 4)))
    _gradcheck(lambda a: D.propagate_step(a, None, s, d, ds), x2)
    _gradcheck(lambda z, b: D.row_epilogue(z, b, None, True), x2 + 2.0, rng.standard_normal(4))
    w, b = rng.standard_normal((5, 4)), rng.standard_normal(5)
    for rop in ("sum", "mean"):
        _gradcheck(lambda a, ww, bb: D.aggregate_dense(a, ww, bb, s, d, None, ss, ds, rop), x2, w, b)
        _gradcheck(lambda a, wa, wb: D.aggregate_dual_linear(a, wa, wb, s, d, rop), x2, w, rng.standard_normal((5, 4)))
    _gradcheck(lambda a, c, wa, wb: D.dual_linear(a, c, wa, wb), x2, rng.standard_normal((n, 3)), w, rng.standard_normal((5, 3)))
    # kinked: inputs kept away from the kink so that the finite difference does not straddle it
    a_s, a_d = rng.standard_normal((n, H)), rng.standard_normal((n, H))
    pre = a_s[src] + a_d[dst]
    assert np.abs(pre).min() > 1e-4
    _gradcheck(lambda f, p, q: D.gat(f, p, q, s, d), x, a_s, a_d)
    assert np.abs(x[src] + y[dst]).min() > 1e-4
    _gradcheck(lambda a, b, ww: D.add_score(a, b, ww, s, d), x, y, rng.standard_normal((H, Dh)))
    z = _away_from_zero(rng.standard_normal((n, 4)))
    _gradcheck(lambda a: D.row_epilogue(a, None, "relu", True), z)


# ------------------------------------------------------------------------------------------------
# Paddle's tie rule, by hand
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rop", ("max", "min"))
def test_two_equal_winners_both_receive_the_whole_gradient(rop):
    # node 3 receives from 0, 1, 2; x[0] == x[1] is the winner in column 0; column 1 has a single winner (node 2)
    hi, lo = (5.0, 1.0) if rop == "max" else (1.0, 5.0)
    x = torch.tensor([[hi, lo], [hi, lo], [lo, hi], [0.0, 0.0]], dtype=torch.float64)
    src, dst = torch.tensor([0, 1, 2]), torch.tensor([3, 3, 3])
    cot = torch.tensor([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [7.0, 11.0]], dtype=torch.float64)
    out, (gx,) = D.evaluate(lambda a, frozen=None: D.send_recv(a, src, dst, rop, frozen=frozen), [x], cot)
    assert torch.equal(out[3], torch.tensor([hi, hi], dtype=torch.float64)) and torch.equal(out[:3], torch.zeros(3, 2, dtype=torch.float64))
    assert torch.equal(gx, torch.tensor([[7.0, 0.0], [7.0, 0.0], [0.0, 11.0], [0.0, 0.0]], dtype=torch.float64))
    # the same through the segment pools, and with an edge operand: x[0] + 1 == x[1] + 1
    _, (gd,) = D.evaluate(lambda a, frozen=None: D.segment_pool(a, torch.tensor([0, 0, 0, 1]), rop, 2, frozen=frozen), [x], cot[[3, 0]])
    assert torch.equal(gd[:3, 0], torch.tensor([7.0, 7.0, 0.0], dtype=torch.float64))
    y = torch.ones(3, 1, dtype=torch.float64)
    _, (gx2, gy2) = D.evaluate(lambda a, b, frozen=None: D.send_recv(a, src, dst, rop, None, b, "add", frozen=frozen), [x, y], cot)
    assert torch.equal(gx2, gx) and torch.equal(gy2, torch.tensor([[7.0], [7.0], [11.0]], dtype=torch.float64))
    # torch's own rule (the wrong reference) splits 7 into 3.5 + 3.5: the mutant reproduces it
    _, (gs,) = D.evaluate(lambda a, frozen=None: D.send_recv(a, src, dst, rop, frozen=frozen, mutant={"split_ties": True}), [x], cot)
    assert torch.equal(gs[:2, 0], torch.tensor([3.5, 3.5], dtype=torch.float64))


# ------------------------------------------------------------------------------------------------
# abs_terms == an explicit enumeration, edge by edge
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mop", MOPS)
@pytest.mark.parametrize("rop", ROPS)
def test_abs_terms_equal_a_per_edge_enumeration(rop, mop):
    rng, n, e, src, dst = small_graph(n=7, e=16, seed=8)
    d = 3
    x = rng.integers(-2, 3, (n, d)).astype(np.float64) if rop in ("max", "min") else rng.standard_normal((n, d))
    y = 2.0 ** rng.integers(-1, 2, (e, 1)) if rop in ("max", "min") else rng.random((e, 1)) + 0.5
    w = rng.standard_normal((n, d))
    s, t = t64(src), t64(dst)
    fn = lambda a, b, frozen=None: D.send_recv(a, s, t, rop, None, b, mop, frozen=frozen)
    r = D.grad_and_terms(fn, [t64(x), t64(y)], t64(w), frozen_fn=lambda a, b: D.winner_mask(a, s, t, rop, None, b, mop))
    msg = {"add": x[src] + y, "sub": x[src] - y, "mul": x[src] * y, "div": x[src] / y}[mop]
    deg = np.maximum(np.bincount(dst, minlength=n), 1)
    if rop in ("max", "min"):
        win = np.zeros((n, d))
        for v in range(n):
            if (dst == v).any():
                win[v] = msg[dst == v].max(0) if rop == "max" else msg[dst == v].min(0)
        coef = (msg == win[dst]).astype(np.float64)
    else:
        coef = np.ones((e, d)) / (deg[dst][:, None] if rop == "mean" else 1.0)
    dmsg_dx = {"add": 1.0, "sub": 1.0, "mul": np.abs(y), "div": 1.0 / np.abs(y)}[mop] * np.ones((e, d))
    dmsg_dy = {"add": 1.0, "sub": 1.0, "mul": np.abs(x[src]), "div": np.abs(x[src]) / y ** 2}[mop] * np.ones((e, d))
    ax, ay = np.zeros((n, d)), np.zeros((e, 1))
    for k in range(e):                                                   # one term per edge and column
        ax[src[k]] += coef[k] * np.abs(w[dst[k]]) * dmsg_dx[k]
        ay[k, 0] = (coef[k] * np.abs(w[dst[k]]) * dmsg_dy[k]).sum()
    assert np.allclose(r.abs_terms64[0].numpy(), ax, rtol=1e-12, atol=0)
    assert np.allclose(r.abs_terms64[1].numpy(), ay, rtol=1e-12, atol=0)
    assert (r.abs_terms64[0] >= r.want64[0].abs() * (1 - 1e-12)).all() and (r.abs_terms64[1] >= r.want64[1].abs() * (1 - 1e-12)).all()


def test_softmax_terms_dominate_and_count_the_segment():
    rng = np.random.default_rng(9)
    ids = t64(np.sort(rng.integers(0, 4, 50)))
    x, g = t64(rng.standard_normal((50, 3)) * 4), t64(rng.standard_normal((50, 3)))
    _, terms, n = D.segment_softmax_terms(x, ids, 4, g)
    _, (want,) = D.evaluate(lambda a: D.segment_softmax(a, ids, 4), [x], g)
    assert (terms >= want.abs() * (1 - 1e-12)).all()
    assert torch.equal(n[:, 0], (torch.bincount(ids, minlength=4)[ids] + 3).double())


# ------------------------------------------------------------------------------------------------
# sensitivity: the fp32 evaluation of a MUTATED definition breaches the bound, the unmutated one stays inside
# ------------------------------------------------------------------------------------------------
def _sens_graph(seed=11, n=400, e=6000, d=16):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n - 1, e), rng.integers(0, n - 1, e)
    src[rng.choice(e, 1500, replace=False)] = 5                          # a hub source: the largest gradient rows of d x
    dst[rng.choice(e, 900, replace=False)] = 9                           # a hub destination
    small = 17                                                           # the destination whose cotangent is 1e-4 of the others
    dst[dst == small] = 18
    src[-1], dst[-1] = n - 1, small                                      # node n - 1 has this one out-edge, `small` this one in-edge ...
    dst[-3:-1] = small                                                   # ... and two more
    return rng, n, e, d, t64(src.astype(np.int64)), t64(dst.astype(np.int64)), small


def _flagged(fn, frozen_fn, inputs, cot, n_out, n_terms, mutant):
    """-> (# GRADIENT elements of the mutated fp32 evaluation out of bound -- the forward, which most mutants change too, is not
    counted; # forward and gradient elements of the unmutated one out of bound; the two lists of gradients; the GradTerms)."""
    r = D.grad_and_terms(fn, inputs, cot, n_out, n_terms, frozen_fn)
    counts, grads = [], []
    for m in (mutant, None):
        out, g = D.evaluate(fn, inputs, cot, torch.float32, frozen_fn, mutant=m)
        c = 0 if m is not None else D.count_out_of_bound(out, r.out64, r.out_abs, r.out_n)
        c += sum(D.count_out_of_bound(gi, wi, ai, ni) for gi, wi, ai, ni in zip(g, r.want64, r.abs_terms64, r.n_terms))
        counts.append(c); grads.append(g)
    return counts[0], counts[1], grads[0], grads[1], r


def _old_max_tied_check_passes(got, want):
    """tests/test_a7_a9_attention_ops.py before this change: `<= 2e-5 * want.abs().max() + 1e-7`."""
    return float((got.double() - want).abs().max()) <= 2e-5 * float(want.abs().max()) + 1e-7


@pytest.mark.parametrize("mop,rop", [("mul", "sum"), ("add", "mean"), ("div", "mean")])
def test_dropped_edge_on_a_small_row_is_caught_where_the_max_tied_tolerance_missed_it(mop, rop):
    rng, n, e, d, src, dst, small = _sens_graph()
    x = t64(rng.standard_normal((n, d)).astype(np.float32))
    y = t64((rng.random((e, d)) + 0.5).astype(np.float32))
    w = rng.standard_normal((n, d)).astype(np.float32)
    w[small] *= 1e-4
    w = t64(w)
    fn = lambda a, b, frozen=None, mutant=None: D.send_recv(a, src, dst, rop, None, b, mop, frozen=frozen, mutant=mutant)
    n_out, n_terms = D.aggregate_n_terms(src, dst, x.shape, y.shape, rop)
    bad, good, g_mut, g_ok, r = _flagged(fn, None, [x, y], w, n_out, n_terms, {"drop_edge": e - 1})
    print("%s/%s: %d gradient elements flagged for the mutant, %d for the plain fp32 evaluation; worst use of the bound %.3f"
          % (mop, rop, bad, good, max(D.worst_ratio(g, wt, a, nt) for g, wt, a, nt in zip(g_ok, r.want64, r.abs_terms64, r.n_terms))))
    assert good == 0
    assert bad >= 3
    # d x of the mutant differs from the truth on row n - 1 alone, by the size of that row -- 1e-4 of the others: the documented miss
    assert _old_max_tied_check_passes(g_mut[0], r.want64[0])
    assert D.count_out_of_bound(g_mut[0], r.want64[0], r.abs_terms64[0], r.n_terms[0]) >= 3


@pytest.mark.parametrize("rop", ("max", "min"))
def test_evenly_split_ties_are_caught(rop):
    rng, n, e, d, src, dst, _ = _sens_graph(seed=12)
    x = t64(rng.integers(-3, 4, (n, d)).astype(np.float32))
    w = t64((rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-4, 0, (n, 1))).astype(np.float32))
    fn = lambda a, frozen=None, mutant=None: D.send_recv(a, src, dst, rop, frozen=frozen, mutant=mutant)
    n_out, n_terms = D.aggregate_n_terms(src, dst, x.shape, None, rop)
    bad, good, _, _, _ = _flagged(fn, lambda a: D.winner_mask(a, src, dst, rop), [x], w, n_out, n_terms[:1], {"split_ties": True})
    assert good == 0 and bad > 0


def test_a_forgotten_mean_divisor_on_a_hub_row_is_caught():
    rng, n, e, d, src, dst, _ = _sens_graph(seed=13)
    x = t64((rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-4, 0, (n, 1))).astype(np.float32))
    w = t64((rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-4, 0, (n, 1))).astype(np.float32))
    fn = lambda a, frozen=None, mutant=None: D.send_recv(a, src, dst, "mean", frozen=frozen, mutant=mutant)
    n_out, n_terms = D.aggregate_n_terms(src, dst, x.shape, None, "mean")
    bad, good, _, _, _ = _flagged(fn, None, [x], w, n_out, n_terms[:1], {"no_deg_row": 9})
    assert good == 0 and bad > 0


@pytest.mark.parametrize("rop", ("sum", "mean"))
def test_a_wrong_power_in_the_divisor_gradient_is_caught(rop):
    rng, n, e, d, src, dst, _ = _sens_graph(seed=14)
    x = t64((rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-4, 0, (n, 1))).astype(np.float32))
    y = t64((rng.random((e, 1)) + 0.5).astype(np.float32))
    w = t64((rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-4, 0, (n, 1))).astype(np.float32))
    fn = lambda a, b, frozen=None, mutant=None: D.send_recv(a, src, dst, rop, None, b, "div", frozen=frozen, mutant=mutant)
    n_out, n_terms = D.aggregate_n_terms(src, dst, x.shape, y.shape, rop)
    bad, good, _, _, _ = _flagged(fn, None, [x, y], w, n_out, n_terms, {"div_dy": True})
    assert good == 0 and bad > 0


def test_a_wrong_leaky_slope_is_caught():
    rng, n, e, d, src, dst, _ = _sens_graph(seed=15)
    H, Dh = 4, 4
    x = rng.standard_normal((n, H, Dh)).astype(np.float32)
    y = rng.standard_normal((n, H, Dh)).astype(np.float32)
    pre = x[src.numpy()] + y[dst.numpy()]
    assert np.abs(pre).min() > 0                                          # (the fp32 and fp64 evaluations take the same side)
    x, y = t64(x), t64(y)
    wt = t64(rng.standard_normal((H, Dh)).astype(np.float32))
    cot = t64((rng.standard_normal((e, H)) * 10.0 ** rng.uniform(-4, 0, (e, 1))).astype(np.float32))
    fn = lambda a, b, c, frozen=None, mutant=None: D.add_score(a, b, c, src, dst, 0.2, frozen=frozen, mutant=mutant)
    outdeg, indeg = D.degree(src, n).double() + 2, D.degree(dst, n).double() + 2
    bad, good, _, _, _ = _flagged(fn, lambda a, b, c: D.add_score_frozen(a, b, c, src, dst, 0.2), [x, y, wt], cot, Dh + 2.0,
                                  [outdeg, indeg, float(e) + 2], {"leaky_slope": 0.25})
    assert good == 0 and bad > 0


# ------------------------------------------------------------------------------------------------
# attention dropout: the keep factor restated from include/pgl_amd.h (grad_defs.attention_keep) and the definitions that take it
# ------------------------------------------------------------------------------------------------
# kept (1) / dropped (0) per (edge id, head), from the kernels' own drop_factor text compiled for the host
KEEP_TABLE = [
    (1234, 0.4, (0, 1, 7, 63), 1.6666666269302368,
     {0: (0, 0, 1, 0), 1: (1, 0, 1, 0), 2: (0, 1, 1, 1), 65535: (1, 1, 1, 1), 65536: (1, 1, 0, 0), 19999999: (1, 1, 1, 1),
      2 ** 31 - 1: (1, 1, 1, 0)}),
    (0xFFFFFFFF, 0.6, (0, 5), 2.500000238418579, {0: (0, 0), 3: (0, 0), 70001: (0, 1)}),
]


@pytest.mark.parametrize("seed,p,heads,factor,rows", KEEP_TABLE, ids=["seed1234-p0.4", "seed0xFFFFFFFF-p0.6"])
def test_attention_keep_reproduces_the_kernels_values(seed, p, heads, factor, rows):
    eids = sorted(rows)
    keep = D.attention_keep(seed, np.array(eids), max(heads) + 1, p)
    assert keep.dtype == np.float32 and keep.shape == (len(eids), max(heads) + 1)
    assert set(np.unique(keep).tolist()) <= {0.0, factor}                # the factor: 1 / (1 - p) rounded once in fp32
    assert np.float32(factor) == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    for i, e in enumerate(eids):
        assert tuple(int(k > 0) for k in keep[i, list(heads)]) == rows[e], (seed, p, e)
    # the seed is taken modulo 2**32, and one edge's row does not depend on which others are asked for
    assert np.array_equal(D.attention_keep(seed + 2 ** 32, np.array(eids), max(heads) + 1, p), keep)
    assert np.array_equal(D.attention_keep(seed, np.array(eids[-1:]), max(heads) + 1, p), keep[-1:])


def test_attention_keep_without_dropout_keeps_everything():
    keep = D.attention_keep(77, np.arange(5000), 8, 0.0)
    assert keep.dtype == np.float32 and (keep == 1.0).all()


KEEP_P, KEEP_SEEDS = (0.1, 0.4, 0.6, 0.9), (0, 1234, 2 ** 31 - 2, 2 ** 32 - 1)


@pytest.mark.parametrize("seed", KEEP_SEEDS)
@pytest.mark.parametrize("p", KEEP_P)
def test_attention_keep_share_and_independence(p, seed):
    """Conditions on the documented hash: the kept share over 70 000 edges x 8 heads within 4 binomial standard deviations of 1 - p
    overall and 5 per head (u >= p on the 2**-24 grid keeps 1 - ceil(p 2**24) / 2**24: 1 - p to 6e-8); the keep bit of edge e is
    uncorrelated with that of e + 1, and head 0's with head 1's (|r| < 0.05; 1 / sqrt(70 000) = 0.004)."""
    E, H = 70000, 8
    bit = (D.attention_keep(seed, np.arange(E), H, p) > 0).astype(np.float64)
    q = 1.0 - float(np.float32(p))
    z_all = (bit.mean() - q) / np.sqrt(q * (1 - q) / (E * H))
    z_head = (bit.mean(0) - q) / np.sqrt(q * (1 - q) / E)
    corr = lambda a, b: float(np.corrcoef(a, b)[0, 1])
    r_edge = max(abs(corr(bit[:-1, h], bit[1:, h])) for h in range(H))
    r_head = abs(corr(bit[:, 0], bit[:, 1]))
    print("p=%g seed=%d: z overall %.2f, per head max |z| %.2f; |r| edge %.4f head %.4f" % (p, seed, z_all, np.abs(z_head).max(), r_edge, r_head))
    assert abs(z_all) <= 4.0 and np.abs(z_head).max() <= 5.0
    assert r_edge < 0.05 and r_head < 0.05


def _keep_graph():
    rng, n, e, src, dst = small_graph(n=30, e=90, seed=21)
    H, Dh = 2, 3
    keep = D.attention_keep(1234, np.arange(e), H, 0.4)
    assert 0 < (keep > 0).mean() < 1
    return rng, n, e, t64(src), t64(dst), H, Dh, keep


def test_gradcheck_gat_with_a_keep_factor():
    rng, n, e, s, d, H, Dh, keep = _keep_graph()
    x, a_s, a_d = rng.standard_normal((n, H, Dh)), rng.standard_normal((n, H)), rng.standard_normal((n, H))
    assert np.abs(a_s[s.numpy()] + a_d[d.numpy()]).min() > 1e-4
    _gradcheck(lambda f, p, q: D.gat(f, p, q, s, d, keep=keep), x, a_s, a_d)
    proj = rng.standard_normal((H * Dh, 2 * H))
    att = x.reshape(n, -1) @ proj
    assert np.abs(att[s.numpy(), :H] + att[d.numpy(), H:]).min() > 1e-4
    _gradcheck(lambda f, pr: D.gat_proj(f, pr, s, d, keep=keep), x, proj)
    # out[v] = sum_e keep_e alpha_e f[u] with alpha the UNDROPPED softmax: written out edge by edge
    f, p_, q_ = t64(x), t64(a_s), t64(a_d)
    _, alpha = D._dense_gat_fp64(torch.stack([s, d], 1), f, p_, q_)
    want = np.zeros((n, H, Dh))
    for k in range(e):
        want[int(d[k])] += (keep[k].astype(np.float64) * alpha[k].numpy())[:, None] * x[int(s[k])]
    assert np.allclose(D.gat(f, p_, q_, s, d, keep=keep).numpy(), want, rtol=1e-12, atol=1e-300)


def test_gat_terms_with_a_keep_factor():
    """keep = ones reproduces the terms without one (the counts: one more term for the multiplication); a real mask lowers the terms
    where it drops, raises them by the factor where it keeps, and they still dominate the gradients they bound; the mutant whose
    row term t[v] forgets the mask has the same forward and d f, and other score gradients."""
    rng, n, e, s, d, H, Dh, keep = _keep_graph()
    f, a_s, a_d = (t64(rng.standard_normal(sh)) for sh in ((n, H, Dh), (n, H), (n, H)))
    cot = t64(rng.standard_normal((n, H, Dh)))
    plain, ones = D.gat_terms(f, a_s, a_d, s, d, cot), D.gat_terms(f, a_s, a_d, s, d, cot, keep=np.ones((e, H), np.float32))
    for k in plain:
        assert torch.equal(plain[k][0], ones[k][0]) and torch.equal(plain[k][1] + 1, ones[k][1]), k
    masked = D.gat_terms(f, a_s, a_d, s, d, cot, keep=keep)
    fn = lambda a, b, c, frozen=None, mutant=None: D.gat(a, b, c, s, d, keep=keep, mutant=mutant)
    out, grads = D.evaluate(fn, [f, a_s, a_d], cot)
    for got, key in zip([out] + grads, ("out", "f", "a_s", "a_d")):
        assert (masked[key][0] >= got.abs() * (1 - 1e-12)).all(), key
    out_m, grads_m = D.evaluate(fn, [f, a_s, a_d], cot, mutant={"t_without_mask": True})
    assert torch.allclose(out_m, out, rtol=1e-14, atol=0) and torch.allclose(grads_m[0], grads[0], rtol=1e-14, atol=0)
    assert not torch.allclose(grads_m[1], grads[1], rtol=1e-3) and not torch.allclose(grads_m[2], grads[2], rtol=1e-3)


# ------------------------------------------------------------------------------------------------
# the committed K table is what the definitions give
# ------------------------------------------------------------------------------------------------
def test_the_k_table_is_what_the_fp32_definitions_measure():
    """Re-measures, on the inputs of tests/test_gradients_gpu.py, how much of its bound the fp32 torch evaluation of every composite
    definition uses, and holds grad_defs.FP32_DEFINITION_RATIO to it: the committed figure is never below the measured one (1 % for
    a differently rounding host) -- so K is never below max(1, 4 x measured) -- and has not drifted above it by more than a quarter."""
    import test_gradients_gpu as T
    measured = T._measure_definitions()
    assert sorted(measured) == sorted(D.FP32_DEFINITION_RATIO)
    for family, table in D.FP32_DEFINITION_RATIO.items():
        got = measured[family]
        print("%-14s measured %.4f, committed %.4f, K %.4f" % (family, got, table, D.K_FAMILY[family]))
        assert got <= table * 1.01, (family, got, table)
        assert got >= table * 0.75 - 0.002, (family, got, table)
        assert D.K_FAMILY[family] == max(1.0, 4.0 * table) <= 64.0
