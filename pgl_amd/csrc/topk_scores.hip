// topk_scores.hip -- masked top-k retrieval over an embedding table: "score every candidate, drop what the graph already links, keep
// the k best" (the evaluation loop of examples/lightgcn/train.py:93-106 and examples/ngcf: getUsersRating -> rating[exclude_index,
// exclude_items] = -(1 << 10) -> topk) without a [Q, N] score tensor, without a host read, and with bits that do not depend on the
// launch.  The definition is in include/pgl_amd.h (pglamd_topk_scores) and pgl_amd/embedding_ops.py.
//
// UNIT OF WORK.  (a tile of 32 queries) x (one of S slices of the candidate range [lo, hi)); a workgroup of 4 waves sweeps its slice
// in SUPERBLOCKS of 128 candidates, wave w owning the 32 x 32 tile of pairs of candidates 32 w .. 32 w + 31.
//   operands   d is walked in chunks of CH components; query and table rows are staged with 16-byte lane loads into LDS rows CH + 1
//              floats apart (kge_score.hip's geometry); rows past Q or the slice are staged as zeros and masked out of the selection.
//   scores     S^T = B A^T on v_mfma_f32_32x32x2_f32: a LANE is a query (lane & 31) and its 16 accumulator registers in each of the two
//              half-waves are candidates.  One accumulator chain over all of d per tile, components ascending, bias added once after
//              it: the bits of s[q, j] depend on (q, j) alone.
//   exclusion  candidates are swept in ascending id and the index rows are sorted, so every lane keeps a CURSOR into its query's row:
//              one binary search at the start of the slice, then per 32-candidate tile the cursor advances while col < j0 + 32 and
//              sets bits of a 32-bit mask.  O(row length) per (query, slice, wave), no search per pair.
//   selection  per query: K2 = pow2(k) KEPT words (pool::sort_word, ascending = best first, pad words behind) and 8 private SEGMENTS of
//              16 words, one per (wave, half-wave) lane of the query, so appends need no LDS atomic and do not depend on arrival
//              order.  thr[q] = the k-th kept word (the pad word until k are kept); a lane appends the words below it.  A query whose
//              lane could not append (segment full) is CUT first by the wave that owns it: group_sort of the 128 segment words, the
//              bitonic half-merge  kept[i] = min(kept[i], seg[K2 - 1 - i])  (the K2 smallest of two ascending runs), group_sort of the
//              K2 kept words, thr refreshed, segments refilled with pad words.  A cut keeps the exact K2 smallest words of what it
//              saw and a word above thr can never be among the k smallest, so the kept set is the same whatever the cut schedule.
//   result     S = 1: the unit writes ids / scores.  S > 1: its k words go to the workspace [Qtiles, S, 32, k] and a second launch, one
//              wave per query, sorts the S k words in LDS and writes the result.  An exact top-k of a total order: every S gives the
//              same bits.  No atomics, caller-owned workspace: the call is capturable.
// DEVIATIONS from the design of record: (1) the query tile is restaged per superblock for every d -- the 64 KB go to the selection
// area (40 KB of segments and kept words at k <= 32, 48 KB at k <= 64), which leaves no room for a resident [32, d] tile beyond d = 32;
// (2) the k <= 64 tier walks d in chunks of 16 components instead of 32 so that its larger area fits in 64 KB (same chain, same bits).
#include "common.hpp"
#include "group_sort.hpp"
#include "pool_core.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace pglamd {
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kTopTile = 32;                          // queries per tile, candidates per wave tile
constexpr int kTopSuper = kTopTile * kWavesPerBlock;  // candidates per superblock
constexpr int kTopSegs = 2 * kWavesPerBlock;          // private segments per query: one per (wave, half-wave)
constexpr int kTopSeg = 16;                           // words per segment = candidates per lane and superblock
constexpr int kTopPend = kTopSegs * kTopSeg;          // segment words per query (a power of two: sorted as they lie)
constexpr int kTopMaxD = 1024;
constexpr int kTopMaxSlices = 32;                     // kTopMaxSlices * PGLAMD_TOPK_MAX_K words per query fit the merge's LDS
constexpr int kTopMergeWords = kTopMaxSlices * PGLAMD_TOPK_MAX_K;
constexpr int64_t kTopGridCap = 256 * 8;
constexpr int64_t kTopUnitsAim = 256 * 4;             // units a launch aims at: a few per CU

struct TopkArgs {
    const float* query; const float* table; const float* bias;
    const int64_t* indptr; const int32_t* col; const int64_t* query_ids;
    int64_t* ids; float* scores; uint64_t* ws;
    int64_t units, num_nodes, num_edges, lo, hi, slice_len;
    int Q, d, k, S;
};

__device__ __forceinline__ int acc_row(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }
__device__ __forceinline__ f16v mfma(float a, float b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// `rows` rows of tab (row stride d), components c0 .. c0 + ch - 1 -> dst [rows][ld]; row r is tab[first + r], zeros from `end` on
__device__ __forceinline__ void stage_rows(float* dst, int ld, int rows, const float* tab, int d, int64_t first, int64_t end, int c0, int ch) {
    const int q4 = ch >> 2;
    for (int idx = threadIdx.x; idx < rows * q4; idx += kBlock) {
        const int r = idx / q4, cc = (idx - r * q4) << 2;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (first + r < end) x = *reinterpret_cast<const float4*>(tab + (first + r) * d + c0 + cc);
        float* o = dst + r * ld + cc;
        o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w;
    }
}

// word -> (id, score) of the result: the pad word is (-1, -inf)
__device__ __forceinline__ void put_result(uint64_t word, int64_t* id, float* score) {
    const bool pad = word == pool::kPadWord;
    *id = pad ? -1 : (int64_t)(uint32_t)word;
    *score = pad ? -INFINITY : __uint_as_float(pool::key_score_bits((uint32_t)(word >> 32)));
}

// The wave's cut of query q: kept <- the K2 smallest of kept and the segment words, both left as the next superblock expects them.
template <int K2>
__device__ __forceinline__ void cut(uint64_t* kept, uint64_t* pend, int* segcnt, uint64_t* thr, int* flag, int k, int lane) {
    group_sort<kWave, false>(pend, kTopPend, lane);
    if (lane < K2) {
        const uint64_t a = kept[lane], b = pend[K2 - 1 - lane];
        kept[lane] = a < b ? a : b;
    }
    group_sync<kWave>();
    group_sort<kWave, false>(kept, K2, lane);
    pend[lane] = pool::kPadWord;
    pend[lane + kWave] = pool::kPadWord;
    if (lane < kTopSegs) segcnt[lane] = 0;
    if (lane == 0) { *thr = kept[k - 1]; *flag = 0; }
    group_sync<kWave>();
}

template <int K2, int CH>
__global__ __launch_bounds__(kBlock) void topk_scores_kernel(TopkArgs a) {
    constexpr int LD = CH + 1;
    __shared__ __align__(16) float sx[kTopTile * LD];              // queries [32][LD]
    __shared__ __align__(16) float sy[kTopSuper * LD];             // candidates [128][LD]
    __shared__ uint64_t s_kept[kTopTile * K2];
    __shared__ uint64_t s_pend[kTopTile * kTopPend];
    __shared__ uint64_t s_thr[kTopTile];
    __shared__ int s_segcnt[kTopTile * kTopSegs];
    __shared__ int s_flag[kTopTile];
    static_assert(sizeof(float) * (kTopTile + kTopSuper) * LD + 8 * kTopTile * (K2 + kTopPend + 1) + 4 * kTopTile * (kTopSegs + 1) <= 65536, "LDS");
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int l32 = lane & 31, half = lane >> 5, seg = 2 * w + half;
    for (int64_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const int s = (int)(unit % a.S);
        const int64_t qt = unit / a.S, q0 = qt * kTopTile;
        const int64_t slo = a.lo + s * a.slice_len, shi = min(a.hi, slo + a.slice_len);     // (an empty slice: slo >= shi)
        const bool qok = q0 + l32 < a.Q;
        for (int i = threadIdx.x; i < kTopTile * K2; i += kBlock) s_kept[i] = pool::kPadWord;
        for (int i = threadIdx.x; i < kTopTile * kTopPend; i += kBlock) s_pend[i] = pool::kPadWord;
        for (int i = threadIdx.x; i < kTopTile * kTopSegs; i += kBlock) s_segcnt[i] = 0;
        if (threadIdx.x < kTopTile) { s_thr[threadIdx.x] = pool::kPadWord; s_flag[threadIdx.x] = 0; }
        // the lane's cursor into its query's row of the exclusion index: the first entry >= slo
        int64_t cur = 0, end = 0;
        if (a.indptr && qok) {
            const int64_t qid = a.query_ids[q0 + l32];
            if (qid >= 0 && qid < a.num_nodes) {
                cur = max((int64_t)0, a.indptr[qid]);
                end = min(a.num_edges, a.indptr[qid + 1]);
                int64_t hi2 = end;
                while (cur < hi2) {
                    const int64_t mid = (cur + hi2) >> 1;
                    if (a.col[mid] < slo) cur = mid + 1; else hi2 = mid;
                }
            }
        }
        __syncthreads();
        for (int64_t j0 = slo; j0 < shi; j0 += kTopSuper) {
            const int64_t jw = j0 + w * kTopTile;
            const bool mine = jw < shi;
            f16v t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = 0.f;
            for (int c0 = 0; c0 < a.d; c0 += CH) {
                const int ch = min(CH, a.d - c0);
                stage_rows(sx, LD, kTopTile, a.query, a.d, q0, a.Q, c0, ch);
                stage_rows(sy, LD, kTopSuper, a.table, a.d, j0, shi, c0, ch);
                __syncthreads();
                if (mine) {
                    const float* x = sx + l32 * LD + half;
                    const float* y = sy + (w * kTopTile + l32) * LD + half;
                    for (int c = 0; c < ch; c += 2) t = mfma(y[c], x[c], t);
                }
                __syncthreads();
            }
            // the excluded candidates of the wave's tile (both half-waves walk the same row)
            uint32_t mask = 0;
            while (cur < end) {
                const int64_t c = a.col[cur];
                if (c >= jw + kTopTile) break;
                if (c >= jw) mask |= 1u << (int)(c - jw);
                ++cur;
            }
            uint64_t word[16];
            uint32_t live = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = acc_row(r, half);
                const int64_t j = jw + row;
                word[r] = pool::kPadWord;
                if (mine && qok && j < shi && !((mask >> row) & 1u)) {
                    const float sc = a.bias ? t[r] + a.bias[j] : t[r];
                    word[r] = pool::sort_word(__float_as_uint(sc), (uint32_t)j);
                    live |= 1u << r;
                }
            }
            // phase A: would the lane's survivors overflow its segment?
            {
                const uint64_t th = s_thr[l32];
                int ns = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) ns += ((live >> r) & 1u) && word[r] < th;
                if (ns && s_segcnt[l32 * kTopSegs + seg] + ns > kTopSeg) s_flag[l32] = 1;
            }
            __syncthreads();
            // phase B: the owner wave cuts the flagged queries
            for (int qq = 0; qq < kTopTile / kWavesPerBlock; ++qq) {
                const int q = w * (kTopTile / kWavesPerBlock) + qq;
                if (wave_uniform(s_flag[q]))
                    cut<K2>(s_kept + q * K2, s_pend + q * kTopPend, s_segcnt + q * kTopSegs, s_thr + q, s_flag + q, a.k, lane);
            }
            __syncthreads();
            // phase C: append under the (possibly refreshed) threshold
            {
                const uint64_t th = s_thr[l32];
                int cnt = s_segcnt[l32 * kTopSegs + seg];
                uint64_t* dst = s_pend + l32 * kTopPend + seg * kTopSeg;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (((live >> r) & 1u) && word[r] < th && cnt < kTopSeg) dst[cnt++] = word[r];
                s_segcnt[l32 * kTopSegs + seg] = cnt;
            }
        }
        __syncthreads();
        for (int qq = 0; qq < kTopTile / kWavesPerBlock; ++qq) {
            const int q = w * (kTopTile / kWavesPerBlock) + qq;
            if (q0 + q >= a.Q) break;
            cut<K2>(s_kept + q * K2, s_pend + q * kTopPend, s_segcnt + q * kTopSegs, s_thr + q, s_flag + q, a.k, lane);
            if (lane < a.k) {
                const uint64_t wd = s_kept[q * K2 + lane];
                if (a.S == 1) put_result(wd, a.ids + (q0 + q) * a.k + lane, a.scores + (q0 + q) * a.k + lane);
                else a.ws[((qt * a.S + s) * kTopTile + q) * a.k + lane] = wd;
            }
        }
        __syncthreads();
    }
}

// one wave per query: the S k words of its slices, sorted in LDS; the first k are the result
__global__ __launch_bounds__(kBlock) void topk_merge_kernel(const uint64_t* __restrict__ ws, int Q, int k, int S, int n2,
                                                            int64_t* __restrict__ ids, float* __restrict__ scores) {
    extern __shared__ __align__(16) uint64_t s_merge[];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + w;
    if (q >= Q) return;                                        // (wave-uniform; the kernel has no workgroup barrier)
    uint64_t* m = s_merge + w * n2;
    const int64_t qt = q / kTopTile, ql = q % kTopTile;
    for (int i = lane; i < n2; i += kWave) {
        const int s = i / k, r = i - s * k;
        m[i] = s < S ? ws[((qt * S + s) * kTopTile + ql) * k + r] : pool::kPadWord;
    }
    group_sync<kWave>();
    group_sort<kWave, false>(m, n2, lane);
    if (lane < k) put_result(m[lane], ids + q * k + lane, scores + q * k + lane);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int pow2_ceil(int64_t n) { int p = 1; while (p < n) p <<= 1; return p; }

}  // namespace
}  // namespace pglamd

using namespace pglamd;

extern "C" int64_t pglamd_topk_scores_slices(int64_t num_queries, int64_t num_candidates) {
    if (num_queries < 1 || num_candidates < 1) return 1;
    const int64_t by_units = ceil_div(kTopUnitsAim, ceil_div(num_queries, kTopTile));
    const int64_t by_length = std::max<int64_t>(1, ceil_div(num_candidates, kTopSuper) / 4);     // at least 4 superblocks a slice
    return std::max<int64_t>(1, std::min<int64_t>({by_units, by_length, (int64_t)kTopMaxSlices}));
}

extern "C" size_t pglamd_topk_scores_workspace_bytes(int64_t num_queries, int64_t k, int64_t slices) {
    if (num_queries < 1 || k < 1 || slices <= 1) return 0;
    return align_up((size_t)ceil_div(num_queries, kTopTile) * slices * kTopTile * k * sizeof(uint64_t), 256);
}

extern "C" int32_t pglamd_topk_scores(const float* query, int64_t num_queries, const float* table, int64_t num_rows, int64_t d,
                                      const float* bias, const int64_t* indptr, const int32_t* col, int64_t num_nodes, int64_t num_edges,
                                      const int64_t* query_ids, int64_t lo, int64_t hi, int64_t k, int64_t slices, int64_t* ids,
                                      float* scores, void* workspace, size_t workspace_bytes, void* stream) {
    if (!query || !table || !ids || !scores || num_queries < 1 || num_rows < 1) return fail(PGLAMD_E_ARG, "topk_scores: bad argument");
    if (d < 4 || d % 4 || d > kTopMaxD) return fail(PGLAMD_E_SHAPE, "topk_scores: d = %lld must be a multiple of 4 from 4 to %d", (long long)d, kTopMaxD);
    if (k < 1 || k > PGLAMD_TOPK_MAX_K) return fail(PGLAMD_E_SHAPE, "topk_scores: k = %lld must be in 1 .. %d", (long long)k, PGLAMD_TOPK_MAX_K);
    if (num_rows >= INT32_MAX || num_queries >= INT32_MAX / 2) return fail(PGLAMD_E_RANGE, "topk_scores: sizes beyond int32 engine range");
    if (lo < 0 || hi > num_rows || hi - lo < 1) return fail(PGLAMD_E_ARG, "topk_scores: [lo, hi) = [%lld, %lld) is not a range of the %lld rows", (long long)lo, (long long)hi, (long long)num_rows);
    if (!aligned16(query) || !aligned16(table)) return fail(PGLAMD_E_ARG, "topk_scores: query and table must be 16-byte aligned");
    const bool excl = indptr || col || query_ids;
    if (excl && (!indptr || !col || !query_ids || num_nodes < 0 || num_edges < 0))
        return fail(PGLAMD_E_ARG, "topk_scores: the exclusion needs indptr, col and query_ids together");
    const int64_t S = slices > 0 ? slices : pglamd_topk_scores_slices(num_queries, hi - lo);
    if (S > kTopMaxSlices || S * k > kTopMergeWords) return fail(PGLAMD_E_ARG, "topk_scores: at most %d slices", kTopMaxSlices);
    if (S > 1 && (!workspace || !aligned16(workspace) || workspace_bytes < pglamd_topk_scores_workspace_bytes(num_queries, k, S)))
        return fail(PGLAMD_E_WORKSPACE, "topk_scores: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    TopkArgs a{};
    a.query = query; a.table = table; a.bias = bias;
    a.indptr = excl ? indptr : nullptr; a.col = col; a.query_ids = query_ids;
    a.ids = ids; a.scores = scores; a.ws = static_cast<uint64_t*>(workspace);
    a.num_nodes = num_nodes; a.num_edges = num_edges; a.lo = lo; a.hi = hi;
    a.slice_len = ceil_div(ceil_div(hi - lo, S), kTopSuper) * kTopSuper;
    a.Q = (int)num_queries; a.d = (int)d; a.k = (int)k; a.S = (int)S;
    a.units = ceil_div(num_queries, kTopTile) * S;
    const dim3 grid((unsigned)std::min<int64_t>(a.units, kTopGridCap));
    if (k <= 32) hipLaunchKernelGGL((topk_scores_kernel<32, 32>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((topk_scores_kernel<64, 16>), grid, dim3(kBlock), 0, st, a);
    PGLAMD_LAUNCH_CHECK();
    if (S > 1) {
        const int n2 = pow2_ceil(S * k);
        const size_t lds = (size_t)kWavesPerBlock * n2 * sizeof(uint64_t);
        static bool attr_set = false;                         // (idempotent, so a race only repeats it)
        if (!attr_set) {
            PGLAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(kWavesPerBlock * kTopMergeWords * sizeof(uint64_t))));
            attr_set = true;
        }
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)ceil_div(num_queries, kWavesPerBlock)), dim3(kBlock), lds, st, a.ws, a.Q, a.k, a.S, n2,
                           ids, scores);
        PGLAMD_LAUNCH_CHECK();
    }
    return PGLAMD_OK;
}
