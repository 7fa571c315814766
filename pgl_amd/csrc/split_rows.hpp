// split_rows.hpp -- the ONE definition of what the chunked edge kernels leave behind for rows that straddle chunks, and of how
// those leftovers are scheduled: the workspace layout, the counter block, the chunk-size rule, the fix-up grids and the
// short-row / hub-row classification.  Every producer of partials (flat, grouped, narrow, dense sink, dense-2, winner gradient,
// softmax statistics, fused GAT) carves its workspace and resets its counters through this header.
//
// Workspace layout (SplitWs):
//     [ head partials | tail partials | counter block + list 1 | list 2 ]
//   head / tail partials: [n_chunks, partial_cols] accumulator values each (H[c]: a piece of a row that began earlier;
//                         T[c]: the first piece of a row that continues), every slice rounded up to 256 bytes
//   counter block:        kSplitCounterInts ints at the head of list 1's slice (see the slot constants below)
//   list 1 / list 2:      up to n_chunks chunk ids each -- at most one split row starts per chunk
#pragma once
#include "common.hpp"

#include <algorithm>

namespace pglamd {

// ---- counter block -----------------------------------------------------------------------------------------------------------
constexpr int kSplitCounterInts = 64;   // ints reserved ahead of list 1 (one 256-byte slice)
constexpr int kSplitCountList1 = 0;     // long_count[0]: tasks on list 1 (every task, or the short rows when the producer classifies)
constexpr int kSplitCountList2 = 1;     // long_count[1]: tasks on list 2 (hub rows)
constexpr int kSplitXcdCounters = 8;    // long_count[8 .. 8 + kXcds): aggregate_dense2.hpp's per-XCD chunk-batch counters
static_assert(kSplitCountList2 < kSplitXcdCounters && kSplitXcdCounters + kXcds <= kSplitCounterInts, "counter slots overlap");

// ---- fix-up geometry ---------------------------------------------------------------------------------------------------------
constexpr int kFixShort = 16;           // rows with at most this many further pieces are finished by one wave
constexpr int kFixWaves = 16;           // waves of a long-role block: they split one hub row's partial list
constexpr int kFixGridShort = 2048;
constexpr int kFixGridLong = 512;
constexpr int kFixGridMergedShort = 1024;  // merged launch: blocks of kFixWaves waves, every wave of a short-role block takes its own tasks
                                           // (C2: 15 035 split rows, 211 of them hub rows -- one task per wave.  Measured: 1 024 blocks 19.6 us,
                                           //  4 096 blocks 21.1 us at C2 and 66.6 against 70.5 us at C2': more blocks than tasks cost their dispatch)
// short role: one wave per task, `waves` waves per block; long role: one block per task
inline unsigned fixup_grid_short(int64_t n_chunks, int cap, int waves) { return (unsigned)std::min<int64_t>(cap, ceil_div(n_chunks, waves)); }
inline unsigned fixup_grid_long(int64_t n_chunks) { return (unsigned)std::min<int64_t>(kFixGridLong, n_chunks); }

// The classification, for the producer that files its tasks by class (agg_flat_kernel) and for the consumer that classifies
// list 1 itself (fixup_tasks): a row whose first edge lies in chunk a and whose last edge, indptr[r + 1] - 1, lies in chunk b has
// b - a further pieces.  (chunk_of_edge takes the edge position, not the row: the caller reads indptr and the chunk size in the
// order the flat kernel's store path always did -- with the reads inside the helper two instantiations of that kernel came out
// with another SGPR count.)
__device__ __forceinline__ int chunk_of_edge(int64_t e, int chunk) { return (int)(e / chunk); }
__device__ __forceinline__ bool fixup_is_long(int a, int b) { return b - a > kFixShort; }

// ---- chunk size (aggregate.hip) ----------------------------------------------------------------------------------------------
int chunk_edges();                          // PGLAMD_CHUNK, else 256
int chunk_edges_for(int64_t num_edges);     // size-aware default; PGLAMD_CHUNK pins one value (stress tests)

// ---- workspace layout --------------------------------------------------------------------------------------------------------
struct SplitWs {
    size_t half, list;
    SplitWs(int64_t n_chunks, int64_t partial_cols, size_t acc_bytes)
        : half(align_up((size_t)n_chunks * partial_cols * acc_bytes, 256)),
          list(align_up((size_t)(n_chunks + kSplitCounterInts) * sizeof(int), 256)) {}
    size_t bytes() const { return 2 * half + 2 * list; }
    // P: AggParams (void* partials) or GatParams (float* partials)
    template <typename P> void carve(P& p, void* ws) const {
        char* w = static_cast<char*>(ws);
        p.part_head = reinterpret_cast<decltype(p.part_head)>(w);
        p.part_tail = reinterpret_cast<decltype(p.part_tail)>(w + half);
        p.long_count = reinterpret_cast<int*>(w + 2 * half);
        p.long_list = p.long_count + kSplitCounterInts;
        p.long_list2 = reinterpret_cast<int*>(w + 2 * half + list);
    }
};

// zeroes the two list counts before a producer runs; xcd_counters: and everything up to the end of dense-2's per-XCD counters
// (pglamd_aggregate_sliced does not call this: its hub-table gather, the launch ahead of its producer, stores the two zeros)
template <typename P>
int32_t reset_split_counters(const P& p, hipStream_t st, bool xcd_counters = false) {
    const int n = xcd_counters ? kSplitXcdCounters + kXcds : kSplitCountList2 + 1;
    PGLAMD_HIP_CHECK(hipMemsetAsync(p.long_count, 0, n * sizeof(int), st));
    return PGLAMD_OK;
}

}  // namespace pglamd
