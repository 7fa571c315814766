// pool.hip -- graph pooling on the device: the per-graph top-k permutation behind pgl.math.segment_topk (pgl/math.py:276-364) and
// the edge filter behind pgl.utils.transform.filter_adj (pgl/utils/transform.py:138-168); together the index work of SAGPool.
// tests/pool_defs.py restates both definitions in numpy; the kernels and the host twins (host_ops.cpp) are held to it bit for bit.
//
// ---- top-k.  scores fp32 [n]; seg_ptr int64 [S + 1] (contiguous segments); out_ptr int64 [S + 1], k_s = out_ptr[s + 1] - out_ptr[s].
// perm[out_ptr[s] + j] = the global position of the j-th element of segment s in the order (score descending, position
// ascending), j < k_s; IEEE equality, NaN above every number (pool_core.hpp: order_key).  The reference scatters the scores into
// a dense [S, max_len] matrix, argsorts all of it and selects by a mask; here a group of G lanes owns one segment:
//   load   element i of the segment becomes the LDS word  order_key(score) << 32 | i ; the words from len to n2 (the power of two
//          >= len) are the pad word, which sorts last.
//   sort   bitonic, ascending (group_sort.hpp).  The words are distinct, so the unstable network is deterministic.
//   write  the low halves of the first k_s words plus the segment's start, one contiguous run of perm.
// Tiers, chosen per segment from its length; each launch strides over ALL segments and takes the ones of its tier:
//   wave tier   len <= 256: one wave64 per segment, kWavesPerBlock segments per workgroup, a[256] = 2 KiB of LDS per wave (8 KiB per
//               workgroup: the 32-waves-per-CU limit binds, not LDS); wave-scope fences only, no workgroup barrier anywhere, so a
//               wave whose segment is of the other tier, flagged or empty just goes on to its next one.
//   block tier  256 < len <= PGLAMD_TOPK_MAX_SEG = 4096: one kBlock workgroup per segment, a[4096] = 32 KiB of static LDS: five
//               workgroups (20 waves) per CU by LDS (160 KiB / 32 KiB).  8192 words would be the 64 KiB static limit and two
//               workgroups (8 waves) per CU for a sort that is all LDS latency between barriers -- the waves matter more than the
//               cap: a graph-classification batch with a member graph above 4096 nodes keeps the dense path.
//               Every condition around a __syncthreads is a function of seg_ptr / out_ptr alone: uniform over the workgroup.
// A segment with len < 0 or len > PGLAMD_TOPK_MAX_SEG sets bit 0 of *status, a k_s outside [0, len] bit 1; such a segment is
// skipped (nothing of it is read or written).  Every loop is bounded by len, k_s or n2.  No workspace, no host read.
//
// ---- edge filter.  edges int64 [E, 2] (row stride in elements), perm int64 [m] distinct ids in [0, n).
// new_id[perm[i]] = i, -1 elsewhere; edge e is kept iff both ends have new_id >= 0; out_edges [kept, 2] = the relabelled ends,
// out_pos [kept] = e, both in input order.  count -> scan -> fill as subgraph.hip, the unit of work being the edge position:
//   mark   memset(new_id, -1); one lane per perm entry: range check BEFORE the id indexes anything, atomicCAS(new_id[v], -1, i)
//          claims the slot -- a lost swap is a repeated id.
//   count  tiles of kTile = 1024 edge positions; keep = both ends in range and relabelled; tile_count[t].
//   scan   tile_off = exclusive scan of tile_count (scan.hpp); status = {kept, flags}.
//   fill   the same predicate; a kept edge's rank inside its wave is popcount(__ballot(keep) & lanes below), wave totals are
//          combined through LDS in wave order, pass by pass: output order == input order.  Deterministic.
// The host reads ONE status pair between count and fill.
#include "common.hpp"

#include "group_sort.hpp"
#include "pool_core.hpp"
#include "scan.hpp"

namespace pglamd {

constexpr int kTopkWaveMax = 256;                 // longest segment of the wave tier (a[256] per wave)
constexpr int64_t kTopkGridCap = 256 * 8;         // workgroups per launch; the kernels stride beyond it
constexpr int kEdgeTile = 1024;                   // edge positions per tile (4 passes of one 256-lane block)
constexpr int64_t kFilterGridCap = 256 * 8;       // workgroups per launch; the kernels stride beyond it

struct TopkArgs {
    const float* scores; const int64_t* seg_ptr; const int64_t* out_ptr; int64_t num_segments; int64_t* perm;
    unsigned long long* status;
};

// Segment s by one group: a = the group's LDS words.  WAVE: this is the wave tier (which also raises the flags: it sees every
// segment exactly once).  Everything decided here depends on (seg_ptr, out_ptr, s) only: uniform over the group.
template <int G>
__device__ __forceinline__ void topk_segment(const TopkArgs& v, uint64_t* a, int64_t s, int lane) {
    constexpr bool WAVE = G == kWave;
    const int64_t b = v.seg_ptr[s], o = v.out_ptr[s];
    const int64_t len = v.seg_ptr[s + 1] - b, k = v.out_ptr[s + 1] - o;
    if (len < 0 || len > PGLAMD_TOPK_MAX_SEG) {
        if (WAVE && lane == 0) atomicOr(v.status, (unsigned long long)pool::kFlagSegment);
        return;
    }
    if (k < 0 || k > len) {
        if (WAVE && lane == 0) atomicOr(v.status, (unsigned long long)pool::kFlagK);
        return;
    }
    if ((len <= kTopkWaveMax) != WAVE || k == 0) return;
    int n2 = 1;
    while (n2 < (int)len) n2 <<= 1;                                          // <= kTopkWaveMax / PGLAMD_TOPK_MAX_SEG
    for (int i = lane; i < n2; i += G) {
        uint64_t w = pool::kPadWord;
        if (i < (int)len) w = pool::sort_word(__float_as_uint(v.scores[b + i]), (uint32_t)i);
        a[i] = w;
    }
    group_sync<G>();
    group_sort<G, false>(a, n2, lane);
    for (int j = lane; j < (int)k; j += G) v.perm[o + j] = b + (int64_t)(a[j] & 0xFFFFFFFFull);
    group_sync<G>();                                                         // (a[] is rewritten by the group's next segment)
}

__global__ __launch_bounds__(kBlock) void topk_wave_kernel(TopkArgs v) {
    __shared__ uint64_t table[kWavesPerBlock][kTopkWaveMax];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + wave; s < v.num_segments; s += (int64_t)gridDim.x * kWavesPerBlock)
        topk_segment<kWave>(v, table[wave], s, lane);                        // (no workgroup barrier in this tier)
}

__global__ __launch_bounds__(kBlock) void topk_block_kernel(TopkArgs v) {
    __shared__ uint64_t table[PGLAMD_TOPK_MAX_SEG];
    for (int64_t s = blockIdx.x; s < v.num_segments; s += gridDim.x) topk_segment<kBlock>(v, table, s, threadIdx.x);
}

// ---- edge filter
__global__ __launch_bounds__(kBlock) void filter_mark_kernel(const int64_t* __restrict__ perm, int64_t m, int64_t num_nodes,
                                                             int* __restrict__ new_id, unsigned long long* __restrict__ status) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        const int64_t v = perm[i];
        if (v < 0 || v >= num_nodes) atomicOr(&status[1], (unsigned long long)pool::kFlagRange);
        else if (atomicCAS(&new_id[v], -1, (int)i) != -1) atomicOr(&status[1], (unsigned long long)pool::kFlagRepeat);
    }
}

// FILL = false: tile_count[t] = kept edges of tile t (and the range flag).  FILL = true: the kept edges written at tile_off[t] + rank.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void filter_tile_kernel(const int64_t* __restrict__ edges, int64_t edge_stride, int64_t num_edges,
                                                             int64_t num_nodes, const int* __restrict__ new_id,
                                                             int64_t* __restrict__ tile_count, const int64_t* __restrict__ tile_off,
                                                             int64_t* __restrict__ out_edges, int64_t* __restrict__ out_pos,
                                                             unsigned long long* __restrict__ status) {
    __shared__ int s_wave[kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int64_t tiles = ((num_edges > 0 ? num_edges : 1) + kEdgeTile - 1) / kEdgeTile;      // filter_tiles: at least one (its count is read)
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        int64_t base = FILL ? tile_off[t] : 0;
#pragma unroll
        for (int pass = 0; pass < kEdgeTile / kBlock; ++pass) {
            const int64_t e = t * kEdgeTile + pass * kBlock + threadIdx.x;
            bool keep = false;
            int a = -1, b = -1;
            if (e < num_edges) {
                const int64_t u = edges[e * edge_stride], x = edges[e * edge_stride + 1];
                if (u < 0 || u >= num_nodes || x < 0 || x >= num_nodes) {      // never dereferenced
                    if (!FILL) atomicOr(&status[1], (unsigned long long)pool::kFlagRange);
                } else {
                    a = new_id[u]; b = new_id[x];
                    keep = a >= 0 && b >= 0;
                }
            }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_wave[w] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int ww = 0; ww < kWavesPerBlock; ++ww) { const int c = s_wave[ww]; if (ww < w) before += c; total += c; }
            if (FILL && keep) {
                const int64_t o = base + before + __popcll(m & ((1ull << lane) - 1ull));
                out_edges[2 * o] = a;
                out_edges[2 * o + 1] = b;
                out_pos[o] = e;
            }
            base += total;
            __syncthreads();                                                   // (s_wave is rewritten by the next pass)
        }
        if (!FILL && threadIdx.x == 0) tile_count[t] = base;
    }
}

struct LoadTilePadded {          // tile_count[0 .. tiles-1], 0 at tiles: the scan's entry `tiles` is the total
    const int64_t* tile_count; int64_t tiles;
    __device__ int64_t operator()(int64_t t) const { return t < tiles ? tile_count[t] : 0; }
};

__global__ void filter_status_kernel(const int64_t* __restrict__ tile_off, int64_t tiles, unsigned long long* __restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = (unsigned long long)tile_off[tiles];
}

static unsigned capped_grid(int64_t work_items, int64_t cap) {
    const int64_t g = work_items > 0 ? work_items : 1;
    return (unsigned)(g < cap ? g : cap);
}

static int64_t filter_tiles(int64_t num_edges) { return ceil_div(num_edges > 0 ? num_edges : 1, (int64_t)kEdgeTile); }

struct FilterWs {
    int* new_id; int64_t* tile_count; int64_t* tile_off; void* temp;
    bool ok;
    FilterWs(void* ws, size_t bytes, int64_t num_nodes, int64_t num_edges) {
        const int64_t tiles = filter_tiles(num_edges);
        Carver cv(ws, bytes);
        new_id = cv.take<int>((size_t)(num_nodes > 0 ? num_nodes : 1));
        tile_count = cv.take<int64_t>((size_t)tiles);
        tile_off = cv.take<int64_t>((size_t)tiles + 1);
        temp = cv.take<char>(exclusive_scan64_temp_bytes(tiles + 1));
        ok = cv.ok();
    }
};

}  // namespace pglamd

using namespace pglamd;

extern "C" int32_t pglamd_segment_topk(const float* scores, const int64_t* seg_ptr, const int64_t* out_ptr, int64_t num_segments,
                                       int64_t* perm, int64_t* status, void* stream) {
    if (num_segments < 0 || !status || (num_segments > 0 && (!seg_ptr || !out_ptr)))
        return fail(PGLAMD_E_ARG, "segment_topk: num_segments must be >= 0 and seg_ptr / out_ptr / status not NULL");
    if (num_segments == 0) return PGLAMD_OK;
    const TopkArgs v{scores, seg_ptr, out_ptr, num_segments, perm, reinterpret_cast<unsigned long long*>(status)};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(topk_wave_kernel, dim3(capped_grid(ceil_div(num_segments, kWavesPerBlock), kTopkGridCap)), dim3(kBlock), 0, st, v);
    PGLAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(topk_block_kernel, dim3(capped_grid(num_segments, kTopkGridCap)), dim3(kBlock), 0, st, v);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

extern "C" int64_t pglamd_filter_edges_launch_threads(void) { return kFilterGridCap * kBlock; }

extern "C" size_t pglamd_filter_edges_workspace_bytes(int64_t num_nodes, int64_t num_edges) {
    if (num_nodes < 0 || num_edges < 0) return 0;
    const int64_t tiles = filter_tiles(num_edges);
    return align_up((size_t)(num_nodes > 0 ? num_nodes : 1) * 4, 256) + align_up((size_t)tiles * 8, 256) +
           align_up((size_t)(tiles + 1) * 8, 256) + align_up(exclusive_scan64_temp_bytes(tiles + 1), 256) + 256;
}

extern "C" int32_t pglamd_filter_edges_count(const int64_t* edges, int64_t edge_stride, int64_t num_edges, const int64_t* perm, int64_t m,
                                             int64_t num_nodes, int64_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (num_edges < 0 || m < 0 || num_nodes < 0 || edge_stride < 2 || !status || (num_edges > 0 && !edges) || (m > 0 && !perm))
        return fail(PGLAMD_E_ARG, "filter_edges_count: bad argument (sizes >= 0, edge_stride >= 2, pointers not NULL)");
    if (num_nodes > INT32_MAX || m > INT32_MAX || num_edges > kMaxEdges)
        return fail(PGLAMD_E_RANGE, "filter_edges: num_nodes / m / num_edges beyond the int32 engine range");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PGLAMD_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st));
    if (!workspace || workspace_bytes < pglamd_filter_edges_workspace_bytes(num_nodes, num_edges))
        return fail(PGLAMD_E_WORKSPACE, "filter_edges_count: workspace too small");
    FilterWs ws(workspace, workspace_bytes, num_nodes, num_edges);
    if (!ws.ok) return fail(PGLAMD_E_WORKSPACE, "filter_edges_count: workspace too small");
    unsigned long long* st_u = reinterpret_cast<unsigned long long*>(status);
    const int64_t tiles = filter_tiles(num_edges);
    if (num_nodes > 0) PGLAMD_HIP_CHECK(hipMemsetAsync(ws.new_id, 0xFF, (size_t)num_nodes * sizeof(int), st));      // all bits set == -1
    if (m > 0) {
        hipLaunchKernelGGL(filter_mark_kernel, dim3(capped_grid(ceil_div(m, kBlock), kFilterGridCap)), dim3(kBlock), 0, st, perm, m, num_nodes,
                           ws.new_id, st_u);
        PGLAMD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((filter_tile_kernel<false>), dim3(capped_grid(tiles, kFilterGridCap)), dim3(kBlock), 0, st, edges, edge_stride, num_edges,
                       num_nodes, ws.new_id, ws.tile_count, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr, st_u);
    PGLAMD_LAUNCH_CHECK();
    PGLAMD_TRY(exclusive_scan64(LoadTilePadded{ws.tile_count, tiles}, tiles + 1, ws.tile_off, ws.temp, st));
    hipLaunchKernelGGL(filter_status_kernel, dim3(1), dim3(kWave), 0, st, ws.tile_off, tiles, st_u);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_filter_edges_fill(const int64_t* edges, int64_t edge_stride, int64_t num_edges, int64_t num_nodes,
                                            int64_t* out_edges, int64_t* out_pos, void* workspace, size_t workspace_bytes, void* stream) {
    if (num_edges < 0 || num_nodes < 0 || edge_stride < 2 || (num_edges > 0 && (!edges || !out_edges || !out_pos)))
        return fail(PGLAMD_E_ARG, "filter_edges_fill: bad argument");
    if (num_nodes > INT32_MAX || num_edges > kMaxEdges) return fail(PGLAMD_E_RANGE, "filter_edges: num_nodes / num_edges beyond the int32 engine range");
    if (num_edges == 0) return PGLAMD_OK;
    if (!workspace || workspace_bytes < pglamd_filter_edges_workspace_bytes(num_nodes, num_edges))
        return fail(PGLAMD_E_WORKSPACE, "filter_edges_fill: workspace too small");
    FilterWs ws(workspace, workspace_bytes, num_nodes, num_edges);
    if (!ws.ok) return fail(PGLAMD_E_WORKSPACE, "filter_edges_fill: workspace too small");
    hipLaunchKernelGGL((filter_tile_kernel<true>), dim3(capped_grid(filter_tiles(num_edges), kFilterGridCap)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), edges, edge_stride, num_edges, num_nodes, ws.new_id, (int64_t*)nullptr, ws.tile_off,
                       out_edges, out_pos, (unsigned long long*)nullptr);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}
