// walk_core.hpp -- the random-walk step logic shared by the kernel (walk.hip) and its host twin (host_ops.cpp), so the two
// cannot drift: the same counter-based RNG, the same integer acceptance test, the same exact fallback scan.
//
// A walk follows successors (src -> dst) over a successor index whose rows are sorted ascending by dst (membership tests are
// binary searches).  Every random number is a pure function of (seed, walker, step, trial): results depend neither on the
// grid nor on how many walkers a lane carries, and the host twin reproduces the device bit for bit.
//
// node2vec / plus draw a position of succ(cur) uniformly and accept it with probability thr[class] / 2^32, where class 0 =
// "x == prev" (weight 1/p), 1 = "x in the set" (weight 1), 2 = otherwise (weight 1/q), and thr[c] = floor(2^32 * w_c / wmax)
// (computed once by the caller, in exact arithmetic).  After max_trials rejections one exact scan draws from the integer
// weights thr[class(x)]; conditioned on the rejections it has the same target law, so the combination is exact.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define PGLAMD_WALK_HD __host__ __device__ inline
#else
#define PGLAMD_WALK_HD inline
#endif

namespace pglamd {
namespace walk {

enum Mode : int32_t { kUniform = 0, kNode2vec = 1, kPlus = 2, kWeighted = 3 };     // kWeighted: pglamd_random_walk_weighted only
constexpr int32_t kMaxTrials = (1 << 20) - 1;     // the trial number shares a 20-bit field with nothing else in the draw key
constexpr uint64_t kSkipGramSalt = 0x5EED5EED5EED5EEDull;

PGLAMD_WALK_HD uint64_t mix64(uint64_t z) {        // splitmix64 finaliser (the one sampling.hip uses)
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// key of walker w: every draw of that walker is mix64(key ^ mix64(step << 20 | trial))
PGLAMD_WALK_HD uint64_t walker_key(uint64_t seed, int64_t w) { return mix64(seed ^ mix64((uint64_t)w)); }

PGLAMD_WALK_HD uint64_t draw(uint64_t key, int64_t step, uint32_t trial) {
    return mix64(key ^ mix64(((uint64_t)step << 20) | (uint64_t)trial));
}

// floor(r * n / 2^64): a uniform index in [0, n) from a 64-bit draw (the high word of the 128-bit product, from 32-bit halves)
PGLAMD_WALK_HD uint64_t scale64(uint64_t r, uint64_t n) {
    const uint64_t r0 = r & 0xFFFFFFFFull, r1 = r >> 32, n0 = n & 0xFFFFFFFFull, n1 = n >> 32;
    const uint64_t t = r1 * n0 + ((r0 * n0) >> 32);
    const uint64_t u = (t & 0xFFFFFFFFull) + r0 * n1;
    return r1 * n1 + (t >> 32) + (u >> 32);
}

// smallest position j of [lo, hi) with cum[j] > r (cum non-decreasing); hi when there is none
PGLAMD_WALK_HD int64_t upper_bound_i64(const int64_t* cum, int64_t lo, int64_t hi, uint64_t r) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)cum[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the acceptance draw of a trial: 32 bits of a second hash of the position draw
PGLAMD_WALK_HD uint64_t accept_bits(uint64_t r) { return mix64(r ^ 0xA0761D6478BD642Full) >> 32; }

// window of position i of walker w for the skip-gram pairs: 1 + floor(h * win / 2^32), h = the top 32 bits of the hash
PGLAMD_WALK_HD int64_t skip_gram_window(uint64_t seed, int64_t w, int64_t i, int64_t win) {
    const uint64_t h = mix64(walker_key(seed ^ kSkipGramSalt, w) ^ mix64((uint64_t)i)) >> 32;
    return 1 + (int64_t)((h * (uint64_t)win) >> 32);
}

// x in col[indptr[v] .. indptr[v+1]) (sorted ascending)
PGLAMD_WALK_HD bool has_successor(const int64_t* indptr, const int32_t* col, int64_t v, int32_t x) {
    int64_t lo = indptr[v], hi = indptr[v + 1];
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (col[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < indptr[v + 1] && col[lo] == x;
}

// Weight class of candidate x at position t of a walk (cur = walk[t], prev = walk[t - 1], t >= 1).  plus: the set is the
// union of succ(walk[0 .. t-1]), searched most recent first; hist(j) returns walk[j].
template <class Hist>
PGLAMD_WALK_HD int weight_class(const int64_t* indptr, const int32_t* col, int32_t x, int64_t prev, bool plus, int64_t t,
                                const Hist& hist) {
    if ((int64_t)x == prev) return 0;
    if (has_successor(indptr, col, prev, x)) return 1;
    if (plus)
        for (int64_t j = t - 2; j >= 0; --j)
            if (has_successor(indptr, col, hist(j), x)) return 1;
    return 2;
}

// Node at position t + 1 of a second-order walk standing at cur = walk[t] (t >= 1, deg = |succ(cur)| > 0, row start b).
template <class Hist>
PGLAMD_WALK_HD int64_t second_order_step(const int64_t* indptr, const int32_t* col, int64_t b, int64_t deg, int64_t prev,
                                         bool plus, int64_t t, const Hist& hist, const uint64_t* thr, int32_t max_trials,
                                         uint64_t key) {
    for (int32_t tr = 0; tr < max_trials; ++tr) {
        const uint64_t r = draw(key, t + 1, (uint32_t)tr);
        const int32_t x = col[b + (int64_t)scale64(r, (uint64_t)deg)];
        if (accept_bits(r) < thr[weight_class(indptr, col, x, prev, plus, t, hist)]) return x;
    }
    uint64_t total = 0;                                   // deg < 2^31 and thr <= 2^32: no overflow
    for (int64_t j = 0; j < deg; ++j) total += thr[weight_class(indptr, col, col[b + j], prev, plus, t, hist)];
    uint64_t r = scale64(draw(key, t + 1, (uint32_t)max_trials), total);
    for (int64_t j = 0; j < deg; ++j) {
        const int32_t x = col[b + j];
        const uint64_t w = thr[weight_class(indptr, col, x, prev, plus, t, hist)];
        if (r < w) return x;
        r -= w;
    }
    return col[b + deg - 1];                              // not reached (r < total)
}

// First step, and every step of a uniform walk: a uniform position of succ(cur).
PGLAMD_WALK_HD int64_t uniform_step(const int32_t* col, int64_t b, int64_t deg, int64_t t, uint64_t key) {
    return col[b + (int64_t)scale64(draw(key, t + 1, 0), (uint64_t)deg)];
}

// ---- integer edge weights (pglamd_edge_weight_table and its host twin) --------------------------------------------------------
// Which PGLAMD_WEIGHT_* condition a weight violates (0 = a legal weight: finite and >= 0; -0.0 counts as 0).
PGLAMD_WALK_HD int32_t weight_flag(double w) {
    if (w != w) return 1;                                  // PGLAMD_WEIGHT_NAN
    if (w < 0) return 2;                                   // PGLAMD_WEIGHT_NEGATIVE
    if (w > 1.7976931348623157e308) return 4;              // PGLAMD_WEIGHT_INF
    return 0;
}

// q of a legal weight w in a row of maximum m: 0 for w == 0 (or m == 0), else max(1, floor(w / m * 2^32)) -- one correctly
// rounded fp64 division, one exact multiply by a power of two, one floor: the same bits on every IEEE machine.  q <= 2^32.
PGLAMD_WALK_HD uint64_t quantise_weight(double w, double m) {
    if (w == 0 || m == 0) return 0;
    const uint64_t q = (uint64_t)(w / m * 4294967296.0);   // (the value is >= 0: truncation is floor)
    return q > 0 ? q : 1;
}

// Every step of an edge-weighted walk: position j of succ(cur) with probability q[j] / T, where cum[b .. b + deg) holds the
// inclusive prefix sums of the row's integer weights q (pglamd_edge_weight_table) and T = cum[b + deg - 1] is the row total.
// One draw, no rejection: r = scale64(draw, T) and the smallest j with cum[j] > r.  -1 when T == 0 (every weight of the row is
// zero: a dead end, like an empty row).  deg > 0.
PGLAMD_WALK_HD int64_t weighted_step(const int32_t* col, const int64_t* cum, int64_t b, int64_t deg, int64_t t, uint64_t key) {
    const uint64_t total = (uint64_t)cum[b + deg - 1];
    if (total == 0) return -1;
    return col[upper_bound_i64(cum, b, b + deg - 1, scale64(draw(key, t + 1, 0), total))];
}

// ---- which rows of the index a step reads ----------------------------------------------------------------------------------------
// A relation-stacked successor index (pglamd_metapath_walk) is R blocks of N + 1 indptr entries over ONE col / cum array: block r
// is relation r's indptr plus the edges of relations 0 .. r-1, so its entries are absolute positions and every step function
// above reads col / cum through them unchanged.  rows(indptr, t) is the block the step FROM position t reads.  It depends on the
// position alone, never on the walker: a kernel looks it up once per position for the whole block.
constexpr int32_t kMaxMetapath = 64;

struct OneRelation {                               // every walk over a plain index: the index is its only block
    PGLAMD_WALK_HD const int64_t* rows(const int64_t* indptr, int64_t) const { return indptr; }
};

struct Metapath {                                  // relation rel[(phase + t) % len] at position t; stride = N + 1
    int32_t rel[kMaxMetapath]; int32_t len, phase; int64_t stride;
    PGLAMD_WALK_HD const int64_t* rows(const int64_t* indptr, int64_t t) const {
        const uint64_t u = (uint64_t)(phase + t);          // (a 32-bit remainder wherever the position fits: a tenth of the 64-bit one)
        const uint32_t i = (u >> 32) ? (uint32_t)(u % (uint32_t)len) : (uint32_t)u % (uint32_t)len;
        return indptr + (int64_t)rel[i] * stride;
    }
};

// What pglamd_metapath_walk and its host twin refuse: NULL when (metapath, len, phase) is a legal metapath over R relations,
// else the reason.  On success *mp holds it for an index of num_nodes nodes.
inline const char* make_metapath(const int32_t* metapath, int32_t len, int32_t phase, int32_t num_relations, int64_t num_nodes,
                                 Metapath* mp) {
    if (num_relations < 1) return "num_relations must be >= 1";
    if (len < 1 || len > kMaxMetapath) return "metapath_len must lie in [1, 64]";
    if (!metapath) return "NULL metapath";
    if (phase < 0 || phase >= len) return "phase must lie in [0, metapath_len)";
    for (int32_t i = 0; i < len; ++i) {
        if (metapath[i] < 0 || metapath[i] >= num_relations) return "a metapath entry is no relation number in [0, num_relations)";
        mp->rel[i] = metapath[i];
    }
    for (int32_t i = len; i < kMaxMetapath; ++i) mp->rel[i] = 0;
    mp->len = len; mp->phase = phase; mp->stride = num_nodes + 1;
    return nullptr;
}

}  // namespace walk
}  // namespace pglamd
