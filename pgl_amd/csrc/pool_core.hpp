// pool_core.hpp -- the sort word of the per-segment top-k, shared by the kernels (pool.hip) and the host twin (host_ops.cpp:
// pglamd_segment_topk_host) so the two cannot drift.  tests/pool_defs.py restates the order in numpy.
//
// The order of a segment is (score descending, position ascending) with IEEE equality (-0.0 ties with +0.0), every NaN greater
// than every number and tied with every other NaN.  order_key maps the fp32 bits to a 32-bit integer that DEcreases with that
// rank: the usual monotone image (negative numbers bit-flipped, the others with the sign bit set), -0.0 folded onto +0.0 and
// every NaN folded onto the top value first, then complemented.  An ASCENDING sort of  order_key << 32 | position  is the
// definition's order; the words of a segment are distinct (distinct positions), so an unstable sort is deterministic.
//   NaN -> 0, +inf -> 0x007FFFFF, +-0.0 -> 0x7FFFFFFF, -inf -> 0xFF800000 (the largest key of any score): the pad word ~0 sorts
//   behind every element.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIP__)
#define PGLAMD_POOL_HD __host__ __device__ inline
#else
#define PGLAMD_POOL_HD inline
#endif

namespace pglamd {
namespace pool {

constexpr uint64_t kPadWord = ~0ull;
constexpr int64_t kFlagSegment = 1, kFlagK = 2;          // status bits of pglamd_segment_topk
constexpr int64_t kFlagRange = 1, kFlagRepeat = 2;       // status[1] bits of pglamd_filter_edges_count

PGLAMD_POOL_HD uint32_t order_key(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return 0u;                   // NaN, either sign, any payload: the greatest
    if (bits == 0x80000000u) bits = 0u;                                  // -0.0 == +0.0
    const uint32_t asc = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return ~asc;
}

PGLAMD_POOL_HD uint64_t sort_word(uint32_t score_bits, uint32_t pos) { return ((uint64_t)order_key(score_bits) << 32) | pos; }

}  // namespace pool
}  // namespace pglamd
