"""CPU checks of tests/special_defs.py (DESIGN.md "Special values"): the checker refuses mutants of the definitions, the definitions
agree with the serial C oracle wherever the oracle does not depend on edge order, and the inputs of the GPU cases satisfy the
conditions the contract states (no overflow of a finite-class element in any order; exact subnormal sums)."""
import numpy as np
import pytest
import torch

import ref_ops as R
import special_defs as S
from special_defs import NAN, INF


@pytest.fixture(scope="module")
def G():
    return S.SpecialGraph(0)


# ------------------------------------------------------------------------------------------------
# the checker itself
# ------------------------------------------------------------------------------------------------
def test_checker_accepts_the_definition_and_has_no_floor():
    w = np.array([[1.0, NAN, INF, -INF, 0.0, -0.0, 2.0 ** -140]])
    S.classify_and_check(w.astype(np.float32), w, 0.0)
    S.classify_and_check(np.array([[1.0, NAN, INF, -INF, -0.0, 0.0, 2.0 ** -140]], np.float32), w, 0.0)      # +-0 compare equal
    for j, v in enumerate([NAN, 1.0, NAN, INF, NAN, INF, 0.0]):                      # any change of class, and a flush to zero
        g = w.copy(); g[0, j] = v
        assert S.refuses(S.classify_and_check, g, w, 0.0), j
    g = w.copy(); g[0, 6] = 0.0
    with pytest.raises(AssertionError, match=r"element \(0, 6\): class finite"):
        S.classify_and_check(g, w, 0.0)
    with pytest.raises(AssertionError, match=r"element \(0, 1\): class finite, the definition's is NaN"):
        S.classify_and_check(np.array([[1.0, 5.0, INF, -INF, 0.0, 0.0, 2.0 ** -140]]), w, 0.0)
    assert S.refuses(S.classify_and_check, np.array([1.0]), np.array([1.0 + 1e-6]), np.array([NAN]))       # a NaN bound is no bound
    S.classify_and_check(np.array([1.0]), np.array([1.0 + 1e-6]), 2e-6)
    # inside gpu_common.reassociation_bound a flushed subnormal PASSES (its floor is finfo(float32).tiny): the reason for `rebound`
    from gpu_common import reassociation_bound
    assert abs(0.0 - 2.0 ** -140) <= reassociation_bound(2.0 ** -140, 1)
    assert not abs(0.0 - 2.0 ** -140) <= S.rebound(2.0 ** -140, 1)


def _mutant_reduce(x64, src, dst, op, kind):
    """np_send_u_recv with one defect."""
    m = x64.shape[0]
    msg = x64[src]
    if kind == "fmax":                                            # a NaN-dropping max / min (fmaxf)
        out = np.zeros((m,) + msg.shape[1:])
        tmp = np.full_like(out, -np.inf if op == "max" else np.inf)
        (np.fmax if op == "max" else np.fmin).at(tmp, dst, msg)
        has = np.bincount(dst, minlength=m) > 0
        out[has] = tmp[has]
        return out
    raise KeyError(kind)


def test_mutants_of_max_and_min_are_refused(G):
    cases = S.planted_cases(G)
    for d in (1, 20):
        x = G.features(d)
        for op in ("max", "min"):
            xp = S.plant(G, x, cases["nan"])
            want, bound = S.expect(G, xp, op)
            assert np.isnan(want[11]).all() and np.isnan(want[8, 0]) and np.isfinite(want[20:400]).all()
            S.classify_and_check(want.astype(np.float32), want, bound)
            assert S.refuses(S.classify_and_check, _mutant_reduce(S.as_f64(xp), G.src, G.dst, op, "fmax"), want, bound)
            # an all-NaN row answered with the accumulator's start value
            xa = S.plant(G, x, cases["all_nan_rows"])
            want, bound = S.expect(G, xa, op)
            assert all(np.isnan(want[r]).all() for r in S.ALL_CARRIER_ROWS)
            got = want.copy(); got[list(S.ALL_CARRIER_ROWS)] = -INF if op == "max" else INF
            assert S.refuses(S.classify_and_check, got, want, bound)
            assert S.refuses(S.classify_and_check, _mutant_reduce(S.as_f64(xa), G.src, G.dst, op, "fmax"), want, bound)
            # a row of only -inf is -inf, a row without edges stays 0
            xi = S.plant(G, x, cases["all_ninf_rows"])
            want, bound = S.expect(G, xi, op)
            assert all((want[r] == -INF).all() for r in S.ALL_CARRIER_ROWS) and (want[list(S.EMPTY_ROWS)] == 0).all()
            got = want.copy(); got[8] = NAN                         # inf turned to NaN
            assert S.refuses(S.classify_and_check, got, want, bound)


def test_mutants_of_relu_flush_wrap_and_bf16_store_are_refused(G):
    # relu that zeroes a NaN
    z = np.array([[-1.0, NAN, 2.0, -INF, INF, 0.0]])
    want = torch.relu(torch.from_numpy(z)).numpy()
    assert np.isnan(want[0, 1]) and want[0, 3] == 0 and want[0, 4] == INF
    S.classify_and_check(np.where(z < 0, 0.0, z), want, 0.0)
    assert S.refuses(S.classify_and_check, np.where(z > 0, z, 0.0), want, 0.0)
    # flush to zero of subnormal operands or results
    x = S.subnormal_features(G, 4)
    want, _ = S.expect(G, x, "sum")
    exact = want.astype(np.float32)
    assert np.array_equal(exact.astype(np.float64), want) and (np.abs(want[want != 0]) < 2.0 ** -125).all()      # the sums are exact in fp32
    S.classify_and_check(exact, want, 0.0)
    ftz = np.where(np.abs(want) < 2.0 ** -126, 0.0, want)
    assert (ftz != want).any() and S.refuses(S.classify_and_check, ftz, want, 0.0)
    xf = np.where(np.abs(x) < 2.0 ** -126, 0.0, x)                 # operands flushed
    assert S.refuses(S.classify_and_check, R.np_send_u_recv(xf.astype(np.float64), G.src, G.dst, "sum"), want, 0.0)
    # an int32 sum that does not wrap
    xi = np.abs(G.features(3, np.int32)) % 3
    xi[G.carrier[(11, 0)]] = 2 ** 31 - 1
    xi[G.carrier[(11, 1 if (11, 1) in G.carrier else S.resolve(G, 11, "mid"))]] = 5
    with np.errstate(over="ignore"):
        want = R.np_send_u_recv(xi, G.src, G.dst, "sum")
    wide = R.np_send_u_recv(xi.astype(np.int64), G.src, G.dst, "sum")
    assert want.dtype == np.int32 and (wide[11] > 2 ** 31 - 1).all() and np.array_equal(want, wide.astype(np.int32))
    S.classify_and_check(want, want)
    assert S.refuses(S.classify_and_check, np.clip(wide, -2 ** 31, 2 ** 31 - 1).astype(np.int32), want)
    assert int((np.array([2 ** 31 - 1], np.int32) + np.array([5], np.int32))[0]) == -2147483644          # numpy's wrap is the contract
    # a bf16 store that turns a NaN into inf: round-to-nearest-even on the bits without a NaN test
    bits = S.cast_set("bf16")
    x32 = S.f32_from_bits(bits)
    wb, wn = S.torch_cast_bits(x32, torch.bfloat16)
    S.assert_bits_equal(wb, wb, wn, wn)
    b64 = bits.astype(np.uint64)
    naive = (((b64 + 0x7FFF + ((b64 >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)
    naive_nan = ((naive & 0x7F80) == 0x7F80) & ((naive & 0x7F) != 0)
    fin = ~np.isnan(x32)
    assert np.array_equal(naive[fin], wb[fin])                       # (on numbers the bit trick IS round-to-nearest-even ...)
    assert (np.isnan(x32) & ~naive_nan).any()                        # (... and it turns NaNs of small payload into inf)
    assert S.refuses(S.assert_bits_equal, naive, wb, wn, naive_nan)


def test_cast_sets_hold_the_edges():
    for kind, tdt, big, tiny_sub in (("fp16", torch.float16, 65504.0, 2.0 ** -24), ("bf16", torch.bfloat16, 3.3895313892515355e38, 2.0 ** -133)):
        bits = S.cast_set(kind)
        x = S.f32_from_bits(bits)
        assert len(np.unique(bits)) == len(bits)
        assert set(range(256)) <= set(int(v) for v in (bits >> 23) & 0xFF)                       # every exponent
        wb, wn = S.torch_cast_bits(x, tdt)
        back = torch.from_numpy(wb.view(np.int16)).view(tdt).float().numpy()
        fin_in = np.isfinite(x)
        assert (np.isinf(back) & fin_in).any() and (np.abs(back[fin_in & np.isfinite(back)]).max() == big)   # overflow to inf, and the largest finite
        assert ((back == 0) & (x != 0)).any() and (np.abs(back) == tiny_sub).any()               # underflow to 0, and the smallest subnormal
        assert wn.sum() >= 8 and np.isnan(x).sum() == wn.sum()                                    # NaNs stay NaNs
        assert (np.isinf(x) & np.isinf(back)).sum() == 2


# ------------------------------------------------------------------------------------------------
# the definitions against the serial C oracle
# ------------------------------------------------------------------------------------------------
def test_definitions_agree_with_the_oracle_where_it_is_order_independent(G):
    cases = S.planted_cases(G)
    for d in (1, 20):
        x = G.features(d)
        for name, pl in cases.items():
            xp = S.plant(G, x, pl)
            for op in ("sum", "mean", "max", "min"):
                if op in ("max", "min") and "nan" in name:
                    continue                                          # the documented exception: next test
                want, bound = S.expect(G, xp, op)
                got = R.c_send_u_recv(xp, G.src, G.dst, op)
                S.classify_and_check(got, want, 2.0 * bound, "%s %s d=%d vs the oracle" % (name, op, d))
    # message ops that PRODUCE the value: 0 * inf, inf - inf, x / 0, 0 / 0
    rng = np.random.default_rng(2)
    x = G.features(4)
    for mop, xv, yv in (("mul", 0.0, INF), ("sub", INF, INF), ("div", 1.0, 0.0), ("div", 0.0, 0.0), ("add", INF, -INF)):
        y = rng.standard_normal((G.E, 4)).astype(np.float32) + 3.0
        xp = S.plant(G, x, [(11, S.resolve(G, 11, "late"), None, xv), (5, 0, None, xv)])
        y[G.edge_of[(11, S.resolve(G, 11, "late"))]] = yv
        y[G.edge_of[(5, 0)]] = yv
        for op in ("sum", "max"):
            want, bound = S.expect(G, xp, op, y=y, mop=mop)
            assert not np.isfinite(want[11]).any() and not np.isfinite(want[5]).any()
            if op == "max" and np.isnan(want[11]).any():
                continue
            with np.errstate(all="ignore"):
                got = R.c_send_ue_recv(xp, y, G.src, G.dst, mop, op)
            S.classify_and_check(got, want, 2.0 * bound, "%s -> %s vs the oracle" % (mop, op))
    # softmax
    for d in (1, 8):
        xs, ids, n_seg, names = S.softmax_segments(d)
        want = S.softmax_def(xs, ids, n_seg)
        for s, name in enumerate(names):
            w = want[ids == s]
            if name in ("all_ninf", "all_ninf_700", "one_pinf", "one_nan", "nan_last_of_600", "single_ninf"):
                assert np.isnan(w).all(), name
            else:
                assert np.isfinite(w).all() and np.allclose(w.sum(0), 1.0), name
            if name.startswith("ninf_"):
                assert (w[np.isneginf(xs[ids == s])] == 0).all()
            if name == "all_3e38":
                assert (w == 1.0 / 256).all()
        with np.errstate(all="ignore"):
            got = R.c_segment_softmax(xs, ids)
        sel = ~np.isin(np.asarray(names)[ids], ["one_nan", "nan_last_of_600"])       # (the oracle's max drops or keeps a NaN by position)
        S.classify_and_check(got[sel], want[sel], 2.0 * S.softmax_bound(xs, ids, n_seg, want)[sel], "softmax d=%d vs the oracle" % d)


def test_the_oracle_keeps_a_nan_in_max_only_when_it_comes_first():
    """DOCUMENTED EXCEPTION (DESIGN.md "Special values"): the serial C port of the Paddle CPU kernel compares `msg > acc`, so a NaN
    message survives only as a row's FIRST message; its answer depends on edge order, which the engine does not keep.  The contract
    is therefore the fp64 restatement (NaN whatever the order), and the oracle is not consulted for NaN under max / min."""
    x = np.array([[NAN], [1.0]], np.float32)
    dst = np.array([0, 0], np.int64)
    for op in ("max", "min"):
        first = R.c_send_u_recv(x, np.array([0, 1], np.int64), dst, op, out_size=1)
        second = R.c_send_u_recv(x, np.array([1, 0], np.int64), dst, op, out_size=1)
        assert np.isnan(first[0, 0]) and second[0, 0] == 1.0
        for src in ([0, 1], [1, 0]):
            assert np.isnan(R.np_send_u_recv(x.astype(np.float64), np.array(src), dst, op, 1)[0, 0])
        assert np.isnan(getattr(torch, "a" + op)(torch.tensor([NAN, 1.0]), 0)) and np.isnan(getattr(torch, "a" + op)(torch.tensor([1.0, NAN]), 0))


# ------------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU cases
# ------------------------------------------------------------------------------------------------
def test_graph_has_the_rows_and_slots_the_cases_need(G):
    assert G.indeg[0] == 1 and G.indeg[6] == 255 and G.indeg[7] == 256 and G.indeg[8] == 257
    assert G.indeg[9] == 4096 and G.indeg[10] == 4353 and G.indeg[11] == 40000 and len(S.EMPTY_ROWS) > 100
    order = np.argsort(G.dst, kind="stable")
    start = np.concatenate([[0], np.cumsum(G.indeg)])
    for (r, p), node in G.carrier.items():
        e = order[start[r] + p]
        assert G.src[e] == node and G.edge_of[(r, p)] == e
    for r in (9, 10, 11):                                                # a slot beyond the first chunk of every longer split row (row 8's second chunk IS its last edge)
        assert any(p >= 256 and p != S.ROW_LENS[r] - 1 for p in G.slots[r])
    assert S.resolve(G, 11, "late") == 39990 and S.resolve(G, 8, "late") == 255 and S.resolve(G, 10, "late") == 4200


def test_no_finite_element_can_overflow_in_any_order(G):
    cases = S.planted_cases(G)
    for d in (1, 33):
        for dtype in (np.float32, np.float64, torch.float16, torch.bfloat16):
            x = G.features(d, dtype)
            for name, pl in cases.items():
                xp = S.plant(G, x, pl)
                for op in ("sum", "mean", "max", "min"):
                    want, bound = S.expect(G, xp, op)                     # (asserts the condition: assert_no_overflow)
                    fin = S.classes(want) == S.FINITE
                    assert np.isfinite(bound[fin]).all() and fin[20:400].all() and not fin.all()
    with pytest.raises(AssertionError):
        S.assert_no_overflow(np.array([1.0]), np.array([2.0 ** 126]))


def test_subnormal_inputs_sum_exactly_in_any_order(G):
    for d in (8, 20, 130):
        x = S.subnormal_features(G, d)
        units = np.rint(x.astype(np.float64) / S.SUB_UNIT).astype(np.int64)
        assert np.array_equal(units * S.SUB_UNIT, x.astype(np.float64))
        for op in ("sum", "max", "min"):
            want, bound = S.expect(G, x, op)
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want)          # representable: comparable bit for bit
            got = R.c_send_u_recv(x, G.src, G.dst, op)                                      # the serial fp32 loop, one particular order
            S.classify_and_check(got, want, 0.0, "subnormal %s" % op)
        rng = np.random.default_rng(0)
        perm = rng.permutation(G.E)                                                          # another order: the same bits
        assert np.array_equal(R.c_send_u_recv(x, G.src[perm], G.dst[perm], "sum"), R.c_send_u_recv(x, G.src, G.dst, "sum"))
        want, _ = S.expect(G, x, "mean")
        got = R.c_send_u_recv(x, G.src, G.dst, "mean")
        S.classify_and_check(got, want, 0.5 * S.SUB_UNIT, "subnormal mean: one rounding")
