// negative_core.hpp -- negative sampling checked against the graph: the draw logic shared by the kernel (negative.hip) and its
// host twin (host_ops.cpp), so the two cannot drift.  The RNG, the scaling, the prefix-sum search and the row membership test
// are walk_core.hpp's.
//
// Definition (restated in numpy in tests/negative_defs.py).  Inputs: a successor index indptr [N+1] / col [E] whose rows are
// ascending by dst (multi-edges allowed); sources src [n]; K = num_neg >= 1; a candidate range [lo, hi), 0 <= lo < hi <= N;
// exclude_self; max_trials in [0, walk::kMaxTrials]; seed; optionally cum [hi], the inclusive prefix sums of a single-row
// table of integer weights q (pglamd_edge_weight_table over a plain vector) -- then lo == 0 and hi is the table's length.
//
// Excluded set of position i: X_i = the DISTINCT entries of row src[i] that lie in [lo, hi), plus src[i] itself when
// exclude_self is set and src[i] lies in [lo, hi).  Successors outside the range are ignored.
// key_i = walker_key(seed, i): the POSITION in the batch, not the node id -- a source listed twice gets different negatives.
//
// Negative k of position i:
//   trials tr = 0 .. max_trials-1:  r = draw(key_i, k, tr);  uniform: x = lo + scale64(r, hi - lo);  weighted, with
//     T = cum[hi-1] > 0: x = upper_bound_i64(cum, 0, hi, scale64(r, T)) (T == 0: no trial is made).  The first x outside X_i is
//     the answer: one binary search of the row plus the self test per trial.
//   exact fallback (after max_trials rejections; the only path when max_trials == 0):  r = draw(key_i, k, max_trials).
//     uniform:  C = (hi - lo) - |X_i|; C == 0 answers -1; else t = scale64(r, C) and the answer is the t-th id (0-based,
//       ascending) of [lo, hi) outside X_i: start at x = lo + t and add one for every excluded id <= x, in ONE ascending walk
//       of the row merged with the self id.
//     weighted: q[e] = cum[e] - cum[e-1]; R = T - sum of q over X_i; R == 0 answers -1; else t = scale64(r, R); walk X_i
//       ascending with s = the weight removed so far: stop at the first e with t < cum[e-1] - s, else s += q[e]; the answer is
//       upper_bound_i64(cum, 0, hi, t + s).  Every sum stays below T < 2^63: integer-exact.
//     Conditioned on the rejections the fallback draws from the same law as a trial, so the combination is exact.
//   A -1 sets kFlagEmpty in *flags.
// Positive (optional): pos[i] = col[b + scale64(draw(key_i, K, 0), deg)] -- a uniform POSITION of the row (a multi-edge counts
// twice, as in uniform_step), -1 for an empty row; the range does not apply to it.
// A source outside [0, N) is never dereferenced: kFlagRange, its negatives and its positive are -1.
// Every output is a pure function of the arguments: it depends neither on the launch nor on the host thread count.
#pragma once
#include "../../include/pgl_amd.h"
#include "walk_core.hpp"

#if defined(__HIP__)
#define PGLAMD_NEG_SLOW __host__ __device__ __attribute__((noinline)) inline      // the fallback stays out of the trial loop's registers
#else
#define PGLAMD_NEG_SLOW inline
#endif

namespace pglamd {
namespace negative {

constexpr int32_t kFlagRange = 1;      // a source outside [0, N)
constexpr int32_t kFlagEmpty = 2;      // a position whose complement is empty (uniform) or weightless (weighted)

struct Args {
    const int64_t* indptr; const int32_t* col; int64_t num_nodes; const int64_t* cum; int64_t lo, hi; const int64_t* src;
    int64_t n, num_neg; int32_t exclude_self, max_trials; uint64_t seed; int64_t* neg; int64_t* pos; int32_t* flags;
};

// the id the self test compares with: src when it is excluded and inside the range, else -1 (no id is -1)
PGLAMD_WALK_HD int64_t self_id(const Args& a, int64_t v) { return (a.exclude_self && v >= a.lo && v < a.hi) ? v : -1; }

// q[e] of the single-row table
PGLAMD_WALK_HD uint64_t table_weight(const int64_t* cum, int64_t e) { return (uint64_t)(cum[e] - (e > 0 ? cum[e - 1] : 0)); }

// f(e) for every id of X_i, ascending, each once: the row's entries inside [lo, hi) merged with the self id.  f returns false to
// stop the walk.  [b, end) = the row.
template <class F>
PGLAMD_WALK_HD void for_each_excluded(const int32_t* col, int64_t b, int64_t end, int64_t lo, int64_t hi, int64_t self, F f) {
    int64_t p = b, e1 = end;
    while (p < e1) {                                       // first position of the row with col >= lo
        const int64_t mid = p + ((e1 - p) >> 1);
        if ((int64_t)col[mid] < lo) p = mid + 1;
        else e1 = mid;
    }
    int64_t last = -1;
    bool self_pending = self >= 0;
    for (; p < end; ++p) {
        const int64_t e = col[p];
        if (e >= hi) break;
        if (e == last) continue;                           // a multi-edge: one id
        if (self_pending && self <= e) {
            self_pending = false;
            if (self < e && !f(self)) return;              // (self == e: a self-loop, counted once)
        }
        last = e;
        if (!f(e)) return;
    }
    if (self_pending) f(self);
}

// The exact fallback of one draw: r = draw(key_i, k, max_trials).  -1 for an empty complement.
PGLAMD_NEG_SLOW int64_t fallback(const int32_t* col, const int64_t* cum, int64_t b, int64_t end, int64_t lo, int64_t hi, int64_t self,
                                 uint64_t r) {
    if (!cum) {
        int64_t excluded = 0;
        for_each_excluded(col, b, end, lo, hi, self, [&](int64_t) { ++excluded; return true; });
        const int64_t c = (hi - lo) - excluded;
        if (c == 0) return -1;
        int64_t x = lo + (int64_t)walk::scale64(r, (uint64_t)c);
        for_each_excluded(col, b, end, lo, hi, self, [&](int64_t e) { if (e > x) return false; ++x; return true; });
        return x;
    }
    uint64_t rest = (uint64_t)cum[hi - 1];
    for_each_excluded(col, b, end, lo, hi, self, [&](int64_t e) { rest -= table_weight(cum, e); return true; });
    if (rest == 0) return -1;
    const uint64_t t = walk::scale64(r, rest);
    uint64_t s = 0;
    for_each_excluded(col, b, end, lo, hi, self, [&](int64_t e) {
        if (t + s < (uint64_t)(e > 0 ? cum[e - 1] : 0)) return false;          // t < cum[e-1] - s, without the subtraction
        s += table_weight(cum, e);
        return true;
    });
    return walk::upper_bound_i64(cum, 0, hi, t + s);
}

// Negative k of position i (source v inside [0, N), row [b, end), key = walker_key(seed, i)).
PGLAMD_WALK_HD int64_t draw_negative(const Args& a, int64_t v, int64_t b, int64_t end, uint64_t key, int64_t k) {
    const int64_t self = self_id(a, v);
    const uint64_t total = a.cum ? (uint64_t)a.cum[a.hi - 1] : (uint64_t)(a.hi - a.lo);
    if (total)
        for (int32_t tr = 0; tr < a.max_trials; ++tr) {
            const uint64_t r = walk::scale64(walk::draw(key, k, (uint32_t)tr), total);
            const int64_t x = a.cum ? walk::upper_bound_i64(a.cum, 0, a.hi, r) : a.lo + (int64_t)r;
            if (x != self && !walk::has_successor(a.indptr, a.col, v, (int32_t)x)) return x;
        }
    return fallback(a.col, a.cum, b, end, a.lo, a.hi, self, walk::draw(key, k, (uint32_t)a.max_trials));
}

// pos[i]: a uniform position of the row
PGLAMD_WALK_HD int64_t draw_positive(const Args& a, int64_t b, int64_t end, uint64_t key) {
    return end > b ? (int64_t)a.col[b + (int64_t)walk::scale64(walk::draw(key, a.num_neg, 0), (uint64_t)(end - b))] : -1;
}

// What both entry points refuse.  PGLAMD_OK when the arguments are legal, else the PGLAMD_E_* code with *why set.
inline int32_t check_args(const Args& a, const char** why) {
    if (a.n < 0 || a.num_nodes < 0 || (a.n > 0 && (!a.indptr || !a.col || !a.src || !a.neg))) { *why = "bad argument (negative size or NULL pointer)"; return PGLAMD_E_ARG; }
    if (a.num_neg < 1) { *why = "num_neg must be >= 1"; return PGLAMD_E_ARG; }
    if (a.max_trials < 0 || a.max_trials > walk::kMaxTrials) { *why = "max_trials outside [0, 2^20)"; return PGLAMD_E_ARG; }
    if (a.lo < 0 || a.hi > a.num_nodes) { *why = "the candidate range [lo, hi) must lie inside [0, num_nodes]"; return PGLAMD_E_RANGE; }
    if (a.lo >= a.hi) { *why = "the candidate range [lo, hi) is empty"; return PGLAMD_E_SHAPE; }
    if (a.cum && a.lo != 0) { *why = "weighted noise over a sub-range is not provided: with cum, lo must be 0 and hi the table's length"; return PGLAMD_E_RANGE; }
    if (a.num_nodes > INT32_MAX || a.n > ((int64_t)1 << 40) || a.num_neg > ((int64_t)1 << 40) / (a.n > 0 ? a.n : 1)) {
        *why = "num_nodes / n / n * num_neg out of range"; return PGLAMD_E_RANGE;
    }
    return PGLAMD_OK;
}

}  // namespace negative
}  // namespace pglamd
