"""The two definitions of the graph-pooling ops (include/pgl_amd.h: pglamd_segment_topk, pglamd_filter_edges_*), restated in plain
numpy.  No torch, no engine: what the kernels (csrc/pool.hip) and their host twins are held to, bit for bit.

Top-k permutation.  scores fp32 [n], seg_ptr int64 [S+1] (contiguous segments), out_ptr int64 [S+1], k_s = out_ptr[s+1] - out_ptr[s],
0 <= k_s <= len_s.  Segment s's positions ordered by (score descending, position ascending); equality is IEEE equality (-0.0 ties
with +0.0); every NaN is greater than every number and ties with every other NaN.  perm[out_ptr[s] + j] = the global position of
the j-th element of that order, j < k_s.

Edge filter.  edges int64 [E, 2], perm int64 [m] distinct ids in [0, n): new_id[perm[i]] = i, -1 elsewhere; edge e is kept iff both
ends have new_id >= 0; out_edges [kept, 2] relabelled, out_pos [kept] the kept edges' positions, both in input order."""
import functools

import numpy as np


def _before(a, b):
    """True when element a = (score, position) comes before b in the order of the definition."""
    (sa, pa), (sb, pb) = a, b
    na, nb = np.isnan(sa), np.isnan(sb)
    if na != nb:
        return bool(na)                  # a NaN is greater than every number: it comes first
    if not na and sa != sb:              # IEEE comparison: -0.0 == +0.0
        return bool(sa > sb)
    return pa < pb


def topk_perm_by_comparison(scores, seg_ptr, out_ptr):
    """The definition word for word (a comparison sort with the definition's own predicate): slow, for small inputs."""
    scores = np.asarray(scores, np.float32)
    perm = np.full(int(out_ptr[-1]), -1, np.int64)
    cmp = lambda a, b: -1 if _before(a, b) else (1 if _before(b, a) else 0)
    for s in range(len(seg_ptr) - 1):
        b, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
        order = sorted(((scores[i], i) for i in range(b, e)), key=functools.cmp_to_key(cmp))
        k = int(out_ptr[s + 1] - out_ptr[s])
        assert 0 <= k <= e - b
        perm[int(out_ptr[s]):int(out_ptr[s]) + k] = [i for _, i in order[:k]]
    return perm


def topk_perm_restated(scores, seg_ptr, out_ptr):
    """The same permutation, vectorised: rank values that fall with the score (NaN -> -1, every number -> its negation with
    +-0.0 -> 0.0, in float64, which holds every fp32 exactly), then a stable lexsort by (segment, rank value, position)."""
    scores = np.asarray(scores, np.float32)
    seg_ptr, out_ptr = np.asarray(seg_ptr, np.int64), np.asarray(out_ptr, np.int64)
    n, S = scores.shape[0], len(seg_ptr) - 1
    lens, k = np.diff(seg_ptr), np.diff(out_ptr)
    assert seg_ptr[0] >= 0 and seg_ptr[-1] <= n and (lens >= 0).all() and (k >= 0).all() and (k <= lens).all() and out_ptr[0] == 0
    nan = np.isnan(scores)
    with np.errstate(invalid="ignore"):
        val = np.where(nan, 0.0, -scores.astype(np.float64)) + 0.0          # (-0.0 + 0.0 == +0.0: one value for both zeros)
    cls = np.where(nan, 0, 1)                                                # NaN first
    seg = np.repeat(np.arange(S), lens)
    pos = np.arange(int(seg_ptr[0]), int(seg_ptr[0]) + int(lens.sum()))
    sl = slice(int(seg_ptr[0]), int(seg_ptr[0]) + int(lens.sum()))
    order = pos[np.lexsort((pos, val[sl], cls[sl], seg))]                    # last key is the primary one
    j = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)  # rank inside the segment
    return order[j < np.repeat(k, lens)].astype(np.int64)


def filter_edges_restated(edges, perm, n):
    """-> (out_edges [kept, 2], out_pos [kept])."""
    edges, perm = np.asarray(edges, np.int64).reshape(-1, 2), np.asarray(perm, np.int64)
    assert ((perm >= 0) & (perm < n)).all() and len(np.unique(perm)) == len(perm)
    assert ((edges >= 0) & (edges < n)).all()
    new_id = np.full(n, -1, np.int64)
    new_id[perm] = np.arange(len(perm))
    ends = new_id[edges]
    keep = (ends >= 0).all(axis=1)
    return ends[keep], np.flatnonzero(keep).astype(np.int64)


def ptr(lens):
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(lens, np.int64))])


SPECIALS = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-20, -1e20, -3e38, 1.0, -1.0, 3e38],
                    np.float32)


def special_scores(n, rng):
    """n scores drawn from the special values (NaN with both sign bits, +-inf, +-0.0, subnormals, -1e20, -3e38 ...)."""
    s = SPECIALS[rng.integers(0, len(SPECIALS), n)].copy()
    bits = s.view(np.uint32)
    flip = np.isnan(s) & (rng.random(n) < 0.5)
    bits[flip] ^= np.uint32(0x80000000)                                      # NaNs of both signs whatever the platform's -nan is
    return s


def score_flavour(kind, n, rng):
    if kind == "distinct":
        return rng.permutation(n).astype(np.float32) - np.float32(n // 2)
    if kind == "ties":
        return rng.integers(-2, 3, n).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.25, np.float32)
    if kind == "special":
        return special_scores(n, rng)
    raise ValueError(kind)


FLAVOURS = ("distinct", "ties", "equal", "special")
