"""Shared by tests/test_negative_defs.py, test_negatives_host.py and test_negatives_gpu.py: the definition of
pglamd_sample_negatives (pgl_amd/csrc/negative_core.hpp) restated in plain Python integers, bit for bit; a brute-force reference
of its exact fallback (uniform: sort the complement and index it; weighted: zero the excluded weights, rebuild the prefix sums,
search them); and a hand-built graph of 70 nodes with the cases a checked negative has to get right."""
import bisect

import numpy as np

M = (1 << 64) - 1
FLAG_RANGE, FLAG_EMPTY = 1, 2
MAX_TRIALS = 16


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def walker_key(seed, w):
    return mix64((seed & M) ^ mix64(w))


def draw(key, step, trial):
    return mix64(key ^ mix64((step << 20) | trial))


def scale64(r, n):
    return (r * n) >> 64


def succ_index(edges, n):
    """(indptr int64 [n+1], col int32 [E]): key = src, rows ascending by dst (what Graph._csr_succ_sorted holds)."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    order = np.lexsort((e[:, 1], e[:, 0]))
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=n), out=indptr[1:])
    return indptr, e[order, 1].astype(np.int32)


def pred_index(edges, n):
    """The mirror: key = dst, rows ascending by src (Graph._csr_pred_sorted)."""
    return succ_index(np.asarray(edges, np.int64).reshape(-1, 2)[:, ::-1], n)


def quantise(w):
    """cum of ops.weight_table(w): q = 0 for w == 0, else max(1, floor(w / max * 2^32)) (one fp64 division)."""
    w = np.asarray(w, np.float64)
    m = float(w.max()) if w.size else 0.0
    q = [0 if (x == 0 or m == 0) else max(1, int(np.float64(x) / np.float64(m) * 4294967296.0)) for x in w.tolist()]
    return np.cumsum(np.asarray(q, np.int64)).astype(np.int64)


def excluded(indptr, col, v, lo, hi, exclude_self):
    """X_i, ascending: the distinct entries of row v inside [lo, hi), plus v when excluded and inside the range."""
    x = set(int(c) for c in col[indptr[v]:indptr[v + 1]].tolist() if lo <= c < hi)
    if exclude_self and lo <= v < hi:
        x.add(int(v))
    return sorted(x)


def fallback_walk(X, lo, hi, cum, r):
    """The exact fallback as the definition walks it."""
    if cum is None:
        c = (hi - lo) - len(X)
        if c == 0:
            return -1
        x = lo + scale64(r, c)
        for e in X:
            if e > x:
                break
            x += 1
        return x
    prev = lambda e: cum[e - 1] if e > 0 else 0
    rest = cum[hi - 1] - sum(cum[e] - prev(e) for e in X)
    if rest == 0:
        return -1
    t, s = scale64(r, rest), 0
    for e in X:
        if t < prev(e) - s:
            break
        s += cum[e] - prev(e)
    return bisect.bisect_right(cum, t + s, 0, hi)


def fallback_brute(X, lo, hi, cum, r):
    """The same draw by brute force."""
    if cum is None:
        comp = sorted(set(range(lo, hi)) - set(X))
        return comp[scale64(r, len(comp))] if comp else -1
    q = np.diff(np.concatenate([[0], np.asarray(cum[:hi], np.int64)]))
    q[np.asarray(X, np.int64)] = 0
    cum2 = np.cumsum(q).tolist()
    return bisect.bisect_right(cum2, scale64(r, cum2[-1])) if cum2[-1] else -1


def negatives_restated(indptr, col, src, num_neg, seed=0, lo=0, hi=None, cum=None, exclude_self=False, max_trials=MAX_TRIALS,
                       brute=False):
    """-> (neg int64 [n, K], pos int64 [n], flags): pglamd_sample_negatives by its definition.  brute: the fallback by brute force."""
    n_nodes = len(indptr) - 1
    hi = (n_nodes if cum is None else len(cum)) if hi is None else hi
    cum = None if cum is None else [int(c) for c in np.asarray(cum).tolist()]
    fb = fallback_brute if brute else fallback_walk
    src = np.asarray(src, np.int64).reshape(-1)
    neg = np.full((len(src), num_neg), -1, np.int64)
    pos = np.full(len(src), -1, np.int64)
    flags = 0
    for i, v in enumerate(src.tolist()):
        if not 0 <= v < n_nodes:
            flags |= FLAG_RANGE
            continue
        key = walker_key(seed, i)
        b, end = int(indptr[v]), int(indptr[v + 1])
        X = excluded(indptr, col, v, lo, hi, exclude_self)
        inX = set(X)
        total = (hi - lo) if cum is None else cum[hi - 1]
        for k in range(num_neg):
            ans = None
            if total:
                for tr in range(max_trials):
                    r = scale64(draw(key, k, tr), total)
                    x = lo + r if cum is None else bisect.bisect_right(cum, r, 0, hi)
                    if x not in inX:
                        ans = x
                        break
            if ans is None:
                ans = fb(X, lo, hi, cum, draw(key, k, max_trials))
            if ans < 0:
                flags |= FLAG_EMPTY
            neg[i, k] = ans
        if end > b:
            pos[i] = int(col[b + scale64(draw(key, num_neg, 0), end - b)])
    return neg, pos, flags


def assert_no_successor(indptr, col, src, neg, what=""):
    """No returned id is a successor of its source (numpy set test)."""
    for v, row in zip(np.asarray(src).tolist(), np.asarray(neg).tolist()):
        hit = set(col[indptr[v]:indptr[v + 1]].tolist()) & set(row)
        assert not hit, (what, v, sorted(hit))


# ---- the hand-built graph ----------------------------------------------------------------------------------------------------------
N = 70
LO, HI = 10, 30                                   # the sub-range most cases draw from
ALL_BUT_17, ALL, MULTI, EMPTY, SELF_LOOP, SELF_IN_LOOP, SELF_IN, ONLY_25, SIXTEEN, W_124, W_NONE, W_ONLY_29, SELF_OUT = \
    0, 1, 2, 3, 4, 15, 16, 20, 6, 7, 8, 9, 50
COMPLEMENT_16 = [1, 8, 9, 22, 23, 24, 33, 41, 42, 43, 44, 57, 58, 66, 68, 69]
WEIGHTS = np.zeros(N, np.float64)
WEIGHTS[[12, 17, 25, 29, 40, 41, 60]] = [3, 1, 2, 4, 8, 1, 2]      # the maximum is a power of two: q is exactly w * 2^29


def fixture_edges():
    rows = {
        ALL_BUT_17: [3, 5] + [x for x in range(LO, HI) if x != 17] + [40, 69],           # + successors below lo and at or above hi
        ALL: list(range(LO, HI)) + [30, 9],
        MULTI: [12, 12, 12, 15, 15, 20, 29, 29, 2, 45, 45],
        EMPTY: [],
        SELF_LOOP: [4, 4, 11, 13],
        SELF_IN_LOOP: [15, 15, 16, 18],                                                 # inside [LO, HI), already its own successor
        SELF_IN: [10, 11],                                                              # inside [LO, HI), no self-loop
        ONLY_25: [x for x in range(LO, HI) if x not in (20, 25)],                       # exclude_self leaves 25 alone
        SIXTEEN: [x for x in range(N) if x not in COMPLEMENT_16] + [6, 10, 10],
        W_124: [12, 40, 41, 60, 60],
        W_NONE: [12, 17, 25, 29, 40, 41, 60, 0],
        W_ONLY_29: [12, 17, 25, 40, 41, 60],
        SELF_OUT: [12, 50, 60],
    }
    rng = np.random.default_rng(5)
    for v in range(31, N):                                                              # ordinary rows, some with multi-edges
        if v not in rows:
            rows[v] = rng.integers(0, N, int(rng.integers(1, 12))).tolist()
    e = np.array([(v, x) for v, xs in rows.items() for x in xs], np.int64)
    return e[rng.permutation(len(e))]


def batch(n, rng=None):
    """n sources over every node of the fixture but ALL / W_NONE (the rows that can have no negative), each special row included."""
    rng = rng or np.random.default_rng(n)
    ok = np.array([v for v in range(N) if v not in (ALL, W_NONE)], np.int64)
    head = np.array([ALL_BUT_17, MULTI, EMPTY, SELF_LOOP, SELF_IN_LOOP, SELF_IN, ONLY_25, SIXTEEN, W_124, W_ONLY_29, SELF_OUT, MULTI], np.int64)
    return np.concatenate([head, rng.choice(ok, max(0, n - len(head)))])[:n]


# (n, K) with n * K = 63, 64, 65, 257 -- wave and block tails -- and K = 1
SHAPES = [(63, 1), (8, 8), (13, 5), (257, 1)]
# every way of drawing: (lo, hi, weighted, exclude_self, max_trials)
MODES = [(0, N, False, False, 16), (LO, HI, False, True, 16), (LO, HI, False, False, 0), (0, N, False, True, 1),
         (0, N, True, False, 16), (0, N, True, True, 0), (0, N, True, False, 1)]


# ---- uniformity ---------------------------------------------------------------------------------------------------------------------
UNIFORM_DRAWS = 64000
UNIFORM_SEED = 2024


def within_five_sigma(counts, probs, draws):
    p = np.asarray(probs, np.float64)
    return bool((np.abs(np.asarray(counts, np.float64) - draws * p) <= 5.0 * np.sqrt(draws * p * (1 - p))).all())


def uniformity_counts(index, sampler=None):
    """[(counts, probabilities)] of the two uniformity runs; sampler(src, K, cum) -> neg, the restatement when None."""
    indptr, col = index
    cum = quantise(WEIGHTS)
    if sampler is None:
        sampler = lambda src, K, c: negatives_restated(indptr, col, src, K, seed=UNIFORM_SEED, cum=c)[0]
    out = []
    for v, ids, probs, c in ((SIXTEEN, COMPLEMENT_16, [1 / 16.0] * 16, None), (W_124, [17, 25, 29], [1 / 7.0, 2 / 7.0, 4 / 7.0], cum)):
        neg = np.asarray(sampler(np.full(UNIFORM_DRAWS // 5, v, np.int64), 5, c)).ravel()
        assert set(neg.tolist()) <= set(ids)
        out.append((np.array([(neg == x).sum() for x in ids]), probs))
    return out
