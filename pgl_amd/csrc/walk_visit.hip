// walk_visit.hip -- PinSAGE neighbourhoods on the GPU: for every seed, the top_k nodes most often visited by num_walks short
// random walks from it, with their visit counts (the importance weights of pgl.nn.PinSageConv).  The reference has the layer
// and no sampler; a composition of ops.random_walk + sort + unique + top-k writes S * R * (L + 1) int64 positions to HBM only
// to throw them away.  Here ONE launch walks, counts and selects; no path ever leaves the chip.
//
// Contract (include/pgl_amd.h; host twin: pglamd_walk_visit_topk_host in host_ops.cpp): walker w = s * R + r of seed s takes
// exactly the walk row w of pglamd_random_walk(_weighted) takes from starts = repeat(seeds, R) -- the same walker_key, the same
// uniform_step / weighted_step (walk_core.hpp), the same dead-end rule.  The visits of seed s are positions 1 .. len-1 of its
// R walks without the entries equal to seeds[s]; they are counted per distinct node, ordered by (count descending, node id
// ascending) and cut at top_k.  Everything is integer: no floating point anywhere, so the result is a pure function of the
// arguments -- independent of the grid, of the tier and of the order in which lanes deposit their visits.
//
// How: a group of G lanes (one wave64 in the wave tier, one kBlock workgroup in the block tier) owns one seed and one LDS
// array a[n2] of 64-bit words, n2 = the power of two >= R * L.
//   1. walk    lane l carries walkers l, l + G, ... (kCarry at a time, their row-bound loads issued together, as walk.hip does)
//              and writes the node of walker r's step t to a[t * R + r] (consecutive lanes, consecutive words), kEmpty for a
//              step after a dead end or a visit of the seed itself; the words from R * L to n2 are kEmpty too.
//   2. sort    bitonic, ascending: equal nodes become runs, the kEmpty words go last.
//   3. count   the head of every run becomes the selection key  count << 32 | (0xFFFFFFFF - node)  (count = the run's length,
//              found by one binary search of the sorted array), every other word 0.
//   4. sort    bitonic, descending: the larger key wins, which IS (count descending, node ascending).  Keys are distinct.
//   5. write   the first min(top_k, distinct) words, as contiguous runs of the seed's nbr / cnt rows; padding -1 / 0.
// Sorting instead of a hash table of (node, count): no probe loop, no full-table case and hence no error flag, and the table
// needs 8 bytes per visit instead of 16 (capacity 2 * cap of a key and a count).
//
// Tiers, chosen from R * L alone (work per seed runs from 10 x 2 to 200 x 10 visits):
//   wave tier   R * L <= 256: one wave64 per seed, kWavesPerBlock seeds per workgroup, 2 KiB of LDS per wave (8 KiB per
//               workgroup: the 32-waves-per-CU limit binds, not LDS); the wave's own LDS traffic is ordered by wave-scope
//               fences only -- no workgroup barrier anywhere, so a wave whose seed is out of range or past the end just leaves.
//   block tier  R * L <= PGLAMD_VISIT_MAX = 4096: one kBlock workgroup per seed, a[4096] = 32 KiB of static LDS: five workgroups
//               (20 waves) per CU by LDS (160 KiB / 32 KiB), against 64 KiB and two workgroups for a hash table of 2 * cap
//               (node, count) pairs.  The walk phase is two dependent random reads per step, so the waves matter.
// Every loop is bounded by R, L, top_k or n2.
#include "common.hpp"
#include "group_sort.hpp"
#include "walk_core.hpp"

namespace pglamd {

constexpr int kVisitWaveMax = 256;                  // largest R * L of the wave tier (a[256] per wave)
constexpr int kCarry = 4;                           // walkers a lane walks at a time (their loads are issued together)
constexpr uint64_t kEmpty = ~0ull;                  // no visit: sorts behind every node id

struct VisitArgs {
    const int64_t* indptr; const int32_t* col; const int64_t* cum; int64_t num_nodes; const int64_t* seeds; int64_t num_seeds;
    int32_t num_walks; int32_t num_steps; int32_t top_k; int32_t n2; uint64_t seed; int64_t* nbr; int32_t* cnt; int32_t* num;
    int32_t* range_flag;
};

// group_sync / group_sort: group_sort.hpp.

// One seed by one group.  a: the group's n2 words of LDS; s < num_seeds.
template <int G, bool WEIGHTED>
__device__ __forceinline__ void visit_seed(const VisitArgs& v, uint64_t* a, int64_t s, int lane) {
    constexpr int kPer = (G == kWave ? kVisitWaveMax : PGLAMD_VISIT_MAX) / G;      // words of a[] per lane, at most
    const int R = v.num_walks, L = v.num_steps, T = v.top_k, n2 = v.n2;
    const int64_t start = v.seeds[s];
    int64_t* nbr = v.nbr + s * T;
    int32_t* cnt = v.cnt + s * T;
    if (start < 0 || start >= v.num_nodes) {                  // (uniform over the group: the whole group leaves)
        for (int j = lane; j < T; j += G) { nbr[j] = -1; cnt[j] = 0; }
        if (lane == 0) { v.num[s] = 0; if (v.range_flag) atomicOr(v.range_flag, 1); }
        return;
    }
    // ---- 1. walk
    for (int i = R * L + lane; i < n2; i += G) a[i] = kEmpty;
    for (int r0 = 0; r0 < R; r0 += kCarry * G) {
        int64_t cur[kCarry];
        uint64_t key[kCarry];
        bool alive[kCarry];
#pragma unroll
        for (int c = 0; c < kCarry; ++c) {
            const int r = r0 + c * G + lane;
            alive[c] = r < R;
            cur[c] = start;
            key[c] = walk::walker_key(v.seed, s * R + r);
        }
        for (int t = 0; t < L; ++t) {                          // cur = position t of the walk; this step writes position t + 1
            int64_t b[kCarry], deg[kCarry];
#pragma unroll
            for (int c = 0; c < kCarry; ++c) {
                b[c] = 0; deg[c] = 0;
                if (alive[c]) { b[c] = v.indptr[cur[c]]; deg[c] = v.indptr[cur[c] + 1] - b[c]; }
            }
#pragma unroll
            for (int c = 0; c < kCarry; ++c) {
                const int r = r0 + c * G + lane;
                int64_t nxt = -1;
                if (alive[c] && deg[c] > 0)
                    nxt = WEIGHTED ? walk::weighted_step(v.col, v.cum, b[c], deg[c], t, key[c])
                                   : walk::uniform_step(v.col, b[c], deg[c], t, key[c]);
                if (nxt < 0) alive[c] = false;                 // an empty row or a row of zero weights: the walk ends here
                else cur[c] = nxt;
                if (r < R) a[t * R + r] = (nxt >= 0 && nxt != start) ? (uint64_t)nxt : kEmpty;
            }
        }
    }
    group_sync<G>();
    // ---- 2. equal nodes become runs
    group_sort<G, false>(a, n2, lane);
    // ---- 3. run heads become selection keys (read everything, then write in place)
    uint64_t sel[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = k * G + lane;
        sel[k] = 0;
        if (i < n2) {
            const uint64_t x = a[i];
            if (x != kEmpty && (i == 0 || a[i - 1] != x)) {
                int lo = i + 1, hi = n2;                       // the first word after the run: the smallest index with a[] > x
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (a[mid] > x) hi = mid;
                    else lo = mid + 1;
                }
                sel[k] = ((uint64_t)(uint32_t)(lo - i) << 32) | (0xFFFFFFFFull - x);
            }
        }
    }
    group_sync<G>();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = k * G + lane;
        if (i < n2) a[i] = sel[k];
    }
    group_sync<G>();
    // ---- 4. (count descending, node ascending)
    group_sort<G, true>(a, n2, lane);
    // ---- 5. the filled prefix, then the padding
    for (int j = lane; j < T; j += G) {
        const uint64_t x = j < n2 ? a[j] : 0;
        nbr[j] = x ? (int64_t)(0xFFFFFFFFull - (x & 0xFFFFFFFFull)) : -1;
        cnt[j] = (int32_t)(x >> 32);
        const uint64_t after = (j + 1 < T && j + 1 < n2) ? a[j + 1] : 0;
        if (x && !after) v.num[s] = j + 1;                     // the last filled entry of the row (exactly one lane sees it)
    }
    if (lane == 0 && a[0] == 0) v.num[s] = 0;
}

template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void visit_wave_kernel(VisitArgs v) {
    __shared__ uint64_t table[kWavesPerBlock][kVisitWaveMax];
    const int wave = threadIdx.x / kWave;
    const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (s >= v.num_seeds) return;                              // (no workgroup barrier in this tier)
    visit_seed<kWave, WEIGHTED>(v, table[wave], s, threadIdx.x % kWave);
}

template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void visit_block_kernel(VisitArgs v) {
    __shared__ uint64_t table[PGLAMD_VISIT_MAX];
    visit_seed<kBlock, WEIGHTED>(v, table, (int64_t)blockIdx.x, threadIdx.x);
}

}  // namespace pglamd

using namespace pglamd;

extern "C" int32_t pglamd_walk_visit_topk(const int64_t* indptr, const int32_t* col, const int64_t* cum, int64_t num_nodes,
                                          const int64_t* seeds, int64_t num_seeds, int64_t num_walks, int64_t num_steps,
                                          int64_t top_k, uint64_t seed, int64_t* nbr, int32_t* cnt, int32_t* num,
                                          int32_t* range_flag, void* stream) {
    if (num_seeds < 0 || num_nodes < 0 || num_walks < 1 || num_steps < 1 || top_k < 1)
        return fail(PGLAMD_E_ARG, "walk_visit_topk: num_seeds / num_nodes must be >= 0 and num_walks / num_steps / top_k >= 1");
    if (num_seeds > 0 && (!indptr || !col || !seeds || !nbr || !cnt || !num)) return fail(PGLAMD_E_ARG, "walk_visit_topk: NULL pointer");
    if (num_walks > PGLAMD_VISIT_MAX || num_steps > PGLAMD_VISIT_MAX || num_walks * num_steps > PGLAMD_VISIT_MAX)
        return fail(PGLAMD_E_RANGE, "walk_visit_topk: num_walks * num_steps = %lld x %lld exceeds PGLAMD_VISIT_MAX = %d",
                    (long long)num_walks, (long long)num_steps, PGLAMD_VISIT_MAX);
    if (top_k > PGLAMD_VISIT_MAX_TOPK)
        return fail(PGLAMD_E_RANGE, "walk_visit_topk: top_k %lld exceeds PGLAMD_VISIT_MAX_TOPK = %d", (long long)top_k, PGLAMD_VISIT_MAX_TOPK);
    if (num_nodes > INT32_MAX || num_seeds > INT32_MAX) return fail(PGLAMD_E_RANGE, "walk_visit_topk: num_nodes / num_seeds out of range");
    if (num_seeds == 0) return PGLAMD_OK;
    const int visits = (int)(num_walks * num_steps);
    int n2 = 1;
    while (n2 < visits) n2 <<= 1;
    const VisitArgs v{indptr, col, cum, num_nodes, seeds, num_seeds, (int32_t)num_walks, (int32_t)num_steps, (int32_t)top_k, n2, seed,
                      nbr, cnt, num, range_flag};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (visits <= kVisitWaveMax) {
        const dim3 grid((unsigned)ceil_div(num_seeds, kWavesPerBlock));
        if (cum) hipLaunchKernelGGL(visit_wave_kernel<true>, grid, dim3(kBlock), 0, st, v);
        else hipLaunchKernelGGL(visit_wave_kernel<false>, grid, dim3(kBlock), 0, st, v);
    } else {
        const dim3 grid((unsigned)num_seeds);
        if (cum) hipLaunchKernelGGL(visit_block_kernel<true>, grid, dim3(kBlock), 0, st, v);
        else hipLaunchKernelGGL(visit_block_kernel<false>, grid, dim3(kBlock), 0, st, v);
    }
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}
