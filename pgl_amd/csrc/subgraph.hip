// subgraph.hip -- S2: the subgraph INDUCED by a node set, on the device.  Stands in for
//   graph_kernel.extract_edges_from_nodes                    (pgl/graph_kernel.pyx:394-432)
//   pgl.sampling.custom.subgraph's relabel through map_edges  (pgl/sampling/custom.py:23-83)
// for tensor graphs: the batch construction of Cluster-GCN / GraphSAINT style training.
//
// Definition (tests/subgraph_defs.py restates it in numpy; the result is held to it bit for bit):
//   local = full(num_nodes, -1); local[nodes] = arange(n)
//   for i, v in enumerate(nodes):                  rows in the order given
//       for j in indptr[v] .. indptr[v+1]-1:       positions in CSR order
//           if local[col[j]] >= 0: emit (local[col[j]], i, eid[j])
// so the output is grouped by dst_local, non-decreasing: the subgraph's dst index needs no sort.
//
// count -> scan -> fill, like pglamd_sample_neighbors_*, but the unit of work is the CANDIDATE EDGE, not the row:
//   mark   one lane per selected node: the id is range-checked BEFORE it indexes anything, atomicCAS(local[v], -1, i) claims
//          the table slot (a slot already claimed = a repeated id), deg[i] = the row's length (0 for a refused id).
//   scan   cand[i] = sum of deg[0 .. i-1], i = 0 .. n (scan.hpp); cand[n] = S, the number of candidate positions.
//   count  candidate positions are cut into tiles of kTile = 1024; tile t holds the positions [t * kTile, (t + 1) * kTile).  A
//          block finds the rows of its tile's first and last position by binary search in cand[] (two lanes), every lane then
//          searches only between those two rows for the row of ITS position: a 100 000-edge hub row is 98 tiles walked by 98
//          blocks, three-edge rows share a tile -- time follows S = sum deg(nodes), never max deg.  keep = local[col[j]] >= 0;
//          the tile's kept count goes to tile_count[t].
//   scan   tile_off = exclusive scan of tile_count over the launch's tile bound; `status` = {kept, flags, S}.
//   fill   the same walk; the rank of a kept position inside its wave is popcount(__ballot(keep) & lanes below), wave totals
//          are combined through LDS in wave order, pass by pass: output order == candidate order.  Deterministic.
// S is known on the device only (the host reads ONE status word between count and fill: kept + flags); the tile kernels are
// launched for the bound ceil(E / kTile) + 1 tiles (distinct nodes: S <= E), capped, and stride over the tiles that exist.
#include "common.hpp"

#include "scan.hpp"

namespace pglamd {

constexpr int kTile = 1024;                       // candidate positions per tile (4 passes of one 256-lane block)
constexpr int64_t kGridCap = 256 * 16;            // blocks per launch; the kernels stride beyond it
constexpr unsigned long long kBadRange = 1, kBadRepeat = 2;

__global__ __launch_bounds__(kBlock) void induced_mark_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ nodes,
                                                              int64_t n, int64_t num_nodes, int* __restrict__ local,
                                                              int64_t* __restrict__ deg, unsigned long long* __restrict__ status) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t v = nodes[i];
        int64_t d = 0;
        if (v < 0 || v >= num_nodes) {
            atomicOr(&status[1], kBadRange);
        } else if (atomicCAS(&local[v], -1, (int)i) != -1) {
            atomicOr(&status[1], kBadRepeat);
        } else {
            d = indptr[v + 1] - indptr[v];
        }
        deg[i] = d;
    }
}

struct LoadDegPadded {          // deg[0 .. n-1], 0 at n: the scan's entry n is the total
    const int64_t* deg; int64_t n;
    __device__ int64_t operator()(int64_t i) const { return i < n ? deg[i] : 0; }
};

struct LoadTileCount {          // tile_count[t] for the tiles that exist (t * kTile < S), 0 beyond
    const int64_t* tile_count; const int64_t* cand; int64_t n;
    __device__ int64_t operator()(int64_t t) const { return t * kTile < cand[n] ? tile_count[t] : 0; }
};

// largest r in [lo, hi] with cand[r] <= p   (cand non-decreasing, cand[lo] <= p)
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ cand, int64_t lo, int64_t hi, int64_t p) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (cand[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// FILL = false: tile_count[t] = kept positions of tile t.  FILL = true: the kept positions written at tile_off[t] + rank.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void induced_tile_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                              const int32_t* __restrict__ eid, const int64_t* __restrict__ nodes,
                                                              int64_t n, const int* __restrict__ local, const int64_t* __restrict__ cand,
                                                              int64_t* __restrict__ tile_count, const int64_t* __restrict__ tile_off,
                                                              int64_t* __restrict__ out_src, int64_t* __restrict__ out_dst,
                                                              int64_t* __restrict__ out_eid) {
    __shared__ int64_t s_row[2];
    __shared__ int s_wave[kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int64_t S = cand[n];
    const int64_t tiles = (S + kTile - 1) / kTile;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t p0 = t * kTile, p1 = (p0 + kTile < S ? p0 + kTile : S) - 1;      // first and last position of the tile
        __syncthreads();                                                               // (s_row / s_wave of the previous tile are read)
        if (threadIdx.x < 2) s_row[threadIdx.x] = row_of(cand, 0, n - 1, threadIdx.x ? p1 : p0);
        __syncthreads();
        const int64_t r_lo = s_row[0], r_hi = s_row[1];
        int64_t base = FILL ? tile_off[t] : 0;
#pragma unroll
        for (int pass = 0; pass < kTile / kBlock; ++pass) {
            const int64_t p = p0 + pass * kBlock + threadIdx.x;
            bool keep = false;
            int64_t r = 0, j = 0;
            int src = -1;
            if (p <= p1) {
                r = row_of(cand, r_lo, r_hi, p);
                j = indptr[nodes[r]] + (p - cand[r]);
                src = local[col[j]];
                keep = src >= 0;
            }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_wave[w] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int ww = 0; ww < kWavesPerBlock; ++ww) { const int c = s_wave[ww]; if (ww < w) before += c; total += c; }
            if (FILL && keep) {
                const int64_t o = base + before + __popcll(m & ((1ull << lane) - 1ull));
                out_src[o] = src;
                out_dst[o] = r;
                out_eid[o] = eid ? (int64_t)eid[j] : j;
            }
            base += total;
            __syncthreads();                                                           // (s_wave is rewritten by the next pass)
        }
        if (!FILL && threadIdx.x == 0) tile_count[t] = base;
    }
}

__global__ void induced_status_kernel(const int64_t* __restrict__ tile_off, int64_t tile_bound, const int64_t* __restrict__ cand,
                                      int64_t n, unsigned long long* __restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        status[0] = (unsigned long long)tile_off[tile_bound];
        status[2] = (unsigned long long)cand[n];
    }
}

static unsigned induced_grid(int64_t work_items) {
    const int64_t g = work_items > 0 ? work_items : 1;
    return (unsigned)(g < kGridCap ? g : kGridCap);
}

static int64_t induced_tile_bound(int64_t num_edges) { return ceil_div(num_edges > 0 ? num_edges : 1, (int64_t)kTile) + 1; }

struct InducedWs {
    int* local; int64_t* deg; int64_t* cand; int64_t* tile_count; int64_t* tile_off; void* temp;
    bool ok;
    InducedWs(void* ws, size_t bytes, int64_t num_nodes, int64_t n, int64_t num_edges) {
        const int64_t tb = induced_tile_bound(num_edges);
        const int64_t longest = (n + 1 > tb + 1) ? n + 1 : tb + 1;
        Carver cv(ws, bytes);
        local = cv.take<int>((size_t)(num_nodes > 0 ? num_nodes : 1));
        deg = cv.take<int64_t>((size_t)(n > 0 ? n : 1));
        cand = cv.take<int64_t>((size_t)n + 1);
        tile_count = cv.take<int64_t>((size_t)tb);
        tile_off = cv.take<int64_t>((size_t)tb + 1);
        temp = cv.take<char>(exclusive_scan64_temp_bytes(longest));
        ok = cv.ok();
    }
};

}  // namespace pglamd

using namespace pglamd;

extern "C" int64_t pglamd_induced_subgraph_launch_threads(void) { return kGridCap * kBlock; }

extern "C" size_t pglamd_induced_subgraph_workspace_bytes(int64_t num_nodes, int64_t n, int64_t num_edges) {
    if (num_nodes < 0 || n < 0 || num_edges < 0) return 0;
    const int64_t tb = induced_tile_bound(num_edges);
    const int64_t longest = (n + 1 > tb + 1) ? n + 1 : tb + 1;
    return align_up((size_t)(num_nodes > 0 ? num_nodes : 1) * 4, 256) + align_up((size_t)(n > 0 ? n : 1) * 8, 256) +
           align_up((size_t)(n + 1) * 8, 256) + align_up((size_t)tb * 8, 256) + align_up((size_t)(tb + 1) * 8, 256) +
           align_up(exclusive_scan64_temp_bytes(longest), 256) + 256;
}

extern "C" int32_t pglamd_induced_subgraph_count(const int64_t* indptr, const int32_t* col, int64_t num_nodes, int64_t num_edges,
                                                 const int64_t* nodes, int64_t n, int64_t* status, void* workspace,
                                                 size_t workspace_bytes, void* stream) {
    if (num_nodes < 0 || num_edges < 0 || n < 0 || !status || (n > 0 && (!indptr || !nodes)) || (num_edges > 0 && !col))
        return fail(PGLAMD_E_ARG, "induced_subgraph_count: bad argument");
    if (num_nodes > INT32_MAX || num_edges > kMaxEdges) return fail(PGLAMD_E_RANGE, "induced_subgraph: num_nodes / num_edges beyond the int32 engine range");
    if (n > num_nodes) return fail(PGLAMD_E_SHAPE, "induced_subgraph: %lld node ids for a graph of %lld nodes: ids must be distinct", (long long)n, (long long)num_nodes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PGLAMD_HIP_CHECK(hipMemsetAsync(status, 0, 4 * sizeof(int64_t), st));
    if (n == 0) return PGLAMD_OK;
    if (!workspace || workspace_bytes < pglamd_induced_subgraph_workspace_bytes(num_nodes, n, num_edges))
        return fail(PGLAMD_E_WORKSPACE, "induced_subgraph_count: workspace too small");
    InducedWs ws(workspace, workspace_bytes, num_nodes, n, num_edges);
    if (!ws.ok) return fail(PGLAMD_E_WORKSPACE, "induced_subgraph_count: workspace too small");
    const int64_t tb = induced_tile_bound(num_edges);
    unsigned long long* st_u = reinterpret_cast<unsigned long long*>(status);
    PGLAMD_HIP_CHECK(hipMemsetAsync(ws.local, 0xFF, (size_t)num_nodes * sizeof(int), st));           // all bits set == -1: no slot claimed
    hipLaunchKernelGGL(induced_mark_kernel, dim3(induced_grid(ceil_div(n, kBlock))), dim3(kBlock), 0, st, indptr, nodes, n, num_nodes,
                       ws.local, ws.deg, st_u);
    PGLAMD_LAUNCH_CHECK();
    { const int32_t rc = exclusive_scan64(LoadDegPadded{ws.deg, n}, n + 1, ws.cand, ws.temp, st); if (rc != PGLAMD_OK) return rc; }
    hipLaunchKernelGGL((induced_tile_kernel<false>), dim3(induced_grid(tb)), dim3(kBlock), 0, st, indptr, col, (const int32_t*)nullptr, nodes, n,
                       ws.local, ws.cand, ws.tile_count, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr);
    PGLAMD_LAUNCH_CHECK();
    { const int32_t rc = exclusive_scan64(LoadTileCount{ws.tile_count, ws.cand, n}, tb + 1, ws.tile_off, ws.temp, st); if (rc != PGLAMD_OK) return rc; }
    hipLaunchKernelGGL(induced_status_kernel, dim3(1), dim3(kWave), 0, st, ws.tile_off, tb, ws.cand, n, st_u);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_induced_subgraph_fill(const int64_t* indptr, const int32_t* col, const int32_t* eid, int64_t num_nodes,
                                                int64_t num_edges, const int64_t* nodes, int64_t n, int64_t* out_src, int64_t* out_dst,
                                                int64_t* out_eid, void* workspace, size_t workspace_bytes, void* stream) {
    if (num_nodes < 0 || num_edges < 0 || n < 0 || (n > 0 && (!indptr || !col || !nodes || !out_src || !out_dst || !out_eid)))
        return fail(PGLAMD_E_ARG, "induced_subgraph_fill: bad argument");
    if (n == 0 || num_edges == 0) return PGLAMD_OK;
    if (n > num_nodes) return fail(PGLAMD_E_SHAPE, "induced_subgraph: more node ids than nodes");
    if (!workspace || workspace_bytes < pglamd_induced_subgraph_workspace_bytes(num_nodes, n, num_edges))
        return fail(PGLAMD_E_WORKSPACE, "induced_subgraph_fill: workspace too small");
    InducedWs ws(workspace, workspace_bytes, num_nodes, n, num_edges);
    if (!ws.ok) return fail(PGLAMD_E_WORKSPACE, "induced_subgraph_fill: workspace too small");
    hipLaunchKernelGGL((induced_tile_kernel<true>), dim3(induced_grid(induced_tile_bound(num_edges))), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), indptr, col, eid, nodes, n, ws.local, ws.cand, (int64_t*)nullptr, ws.tile_off,
                       out_src, out_dst, out_eid);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}
