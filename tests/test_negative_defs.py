"""The numpy restatement of checked negative sampling (tests/negative_defs.py) held to itself: the fallback as the definition
walks it == the brute force over the sorted complement / the rebuilt prefix sums, the fixture's rows are what the cases need, and
the fixed-seed uniformity counts that the device test compares with pass on the restatement alone."""
import numpy as np
import pytest

import negative_defs as D


@pytest.fixture(scope="module")
def index():
    return D.succ_index(D.fixture_edges(), D.N)


def test_fixture_rows_are_the_cases(index):
    indptr, col = index
    row = lambda v: col[indptr[v]:indptr[v + 1]].tolist()
    assert all(row(v) == sorted(row(v)) for v in range(D.N)) and len(indptr) == D.N + 1
    assert D.excluded(indptr, col, D.ALL_BUT_17, D.LO, D.HI, False) == [x for x in range(D.LO, D.HI) if x != 17]
    assert min(row(D.ALL_BUT_17)) < D.LO and max(row(D.ALL_BUT_17)) >= D.HI
    assert D.excluded(indptr, col, D.ALL, D.LO, D.HI, False) == list(range(D.LO, D.HI))
    assert row(D.EMPTY) == [] and row(D.MULTI).count(12) == 3
    assert D.excluded(indptr, col, D.SELF_IN_LOOP, D.LO, D.HI, True) == D.excluded(indptr, col, D.SELF_IN_LOOP, D.LO, D.HI, False) == [15, 16, 18]
    assert D.excluded(indptr, col, D.SELF_IN, D.LO, D.HI, True) == [10, 11, 16] and D.excluded(indptr, col, D.SELF_OUT, D.LO, D.HI, True) == [12]
    assert sorted(set(range(D.N)) - set(row(D.SIXTEEN))) == D.COMPLEMENT_16
    cum = D.quantise(D.WEIGHTS)
    assert np.diff(np.concatenate([[0], cum]))[[17, 25, 29]].tolist() == [1 << 29, 1 << 30, 1 << 31] and cum[-1] == 21 << 29


@pytest.mark.parametrize("lo,hi,weighted,exclude_self,max_trials", D.MODES)
def test_the_walked_fallback_is_the_brute_force(index, lo, hi, weighted, exclude_self, max_trials):
    indptr, col = index
    cum = D.quantise(D.WEIGHTS) if weighted else None
    src = np.concatenate([D.batch(120), [D.ALL, D.W_NONE]])
    for trials in (0, max_trials):
        a = D.negatives_restated(indptr, col, src, 4, seed=11, lo=lo, hi=hi, cum=cum, exclude_self=exclude_self, max_trials=trials)
        b = D.negatives_restated(indptr, col, src, 4, seed=11, lo=lo, hi=hi, cum=cum, exclude_self=exclude_self, max_trials=trials,
                                 brute=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        neg = a[0]
        ok = neg >= 0
        assert ((neg[ok] >= lo) & (neg[ok] < hi)).all()
        for v, r in zip(src.tolist(), neg.tolist()):
            X = set(D.excluded(indptr, col, v, lo, hi, exclude_self))
            assert not (X & set(r)), (v, r)
        if weighted:
            assert (D.WEIGHTS[neg[ok]] > 0).all()                               # a zero weight is never drawn


def test_uniformity_counts_of_the_fixed_seed(index):
    """64 000 draws for a source whose complement has 16 ids: every id within 5 binomial standard deviations of 4 000; the same
    with weights 1 : 2 : 4 over three allowed ids.  The device test asserts equality with these counts."""
    for counts, probs in D.uniformity_counts(index):
        print(counts.tolist())
        assert counts.sum() == D.UNIFORM_DRAWS and D.within_five_sigma(counts, probs, D.UNIFORM_DRAWS)
