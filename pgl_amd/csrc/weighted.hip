// weighted.hip -- edge-weighted sampling on the GPU: the integer weight table every weighted draw reads, neighbour sampling
// without replacement by weight, and independent draws from a single-row table.  (The weighted walk is a mode of walk.hip's
// kernel; its step lives in walk_core.hpp.)  The reference has no counterpart: graph_kernel.alias_sample_build_table
// (pgl/graph_kernel.pyx:366-392) is never called from pgl/, and paddle.geometric.sample_neighbors draws uniformly.
//
// Table: row v with positions b .. b + deg - 1 and maximum weight m gets q[j] = 0 for a zero weight, else
//   max(1, floor((double)w[j] / (double)m * 2^32)), and cum[j] = q[b] + .. + q[j] (int64, inclusive, WITHIN the row); npos[v] =
//   the number of positions with q > 0.  Everything after the one fp64 division is integer arithmetic, the row maximum and the
//   sums are order-independent, so the table does not depend on the launch and the host twin (host_ops.cpp) and a numpy
//   restatement (tests/weighted_defs.py) give the same bits.  No lane walks a row: the maximum is a segmented wave reduction
//   over POSITIONS plus one atomicMax per (wave, row) run, the sums are the int64 scan of scan.hpp over all positions minus
//   the scan value at the row's start, npos one atomicAdd per (wave, row) run.
// Sampler: one lane per seed node (as sampling.hip).  The whole positive set in row order when k < 0 or npos <= k; otherwise
//   successive sampling: draw c picks position j with probability q[j] / (row total - q of the positions already chosen).
//   The chosen positions are kept sorted with their q, so a pick is one walk over the chosen (<= 64) and one binary search of
//   cum: O(k^2 + k log deg) per seed.  A lane that copies a whole positive set still reads its row once (deg reads).
#include "common.hpp"
#include "scan.hpp"
#include "walk_core.hpp"

namespace pglamd {

// Inclusive segmented scan of v over the lanes of a wave, segments = runs of equal `row` (rows ascend with the position, so
// equal rows are adjacent); the LAST lane of a run then holds the run's reduction.  -> true for that lane.
template <typename T, typename Op>
__device__ __forceinline__ bool wave_run_reduce(int64_t row, T& v, Op op) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T t = __shfl_up(v, off, kWave);
        const int64_t r = __shfl_up(row, off, kWave);
        if (lane >= off && r == row) v = op(v, t);
    }
    const int64_t next = __shfl_down(row, 1, kWave);
    return lane == kWave - 1 || next != row;
}

struct MaxU64 { __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; } };
struct AddU64 { __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; } };

// the weight of position j, its legality, and the row it belongs to
template <typename T>
struct WeightAt {
    const int32_t* row; const int32_t* eid; const T* weight; int64_t num_nodes, num_weights;
    // -> flag bits of position j (0 = legal); w = the weight as fp64 (0 when illegal), r = its row (-1 when out of range)
    __device__ int32_t operator()(int64_t j, double& w, int64_t& r) const {
        r = row ? (int64_t)row[j] : 0;
        const int64_t k = eid ? (int64_t)eid[j] : j;
        w = 0.0;
        if (r < 0 || r >= num_nodes) { r = -1; return PGLAMD_WEIGHT_BAD_EID; }
        if (k < 0 || k >= num_weights) return PGLAMD_WEIGHT_BAD_EID;
        const double x = (double)weight[k];
        const int32_t f = walk::weight_flag(x);
        if (!f) w = x;
        return f;
    }
};

// rowmax[r] = bits of the largest legal weight of row r (non-negative doubles order like their bit patterns)
template <typename T>
__global__ __launch_bounds__(kBlock) void weight_row_max_kernel(WeightAt<T> at, int64_t num_edges, unsigned long long* __restrict__ rowmax,
                                                                int32_t* __restrict__ flag) {
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < num_edges; base += (int64_t)gridDim.x * kBlock) {
        const int64_t j = base + threadIdx.x;
        double w = 0.0; int64_t r = -1;
        if (j < num_edges) {
            const int32_t f = at(j, w, r);
            if (f) atomicOr(flag, f);
        }
        unsigned long long bits = w > 0 ? (unsigned long long)__double_as_longlong(w) : 0ull;
        const bool last = wave_run_reduce(r, bits, MaxU64());
        if (last && r >= 0 && bits) atomicMax(&rowmax[r], bits);
    }
}

template <typename T>
struct QuantAt {
    WeightAt<T> at; const unsigned long long* rowmax;
    __device__ int64_t operator()(int64_t j) const {
        double w; int64_t r;
        (void)at(j, w, r);
        if (r < 0) return 0;
        return (int64_t)walk::quantise_weight(w, __longlong_as_double((long long)rowmax[r]));
    }
};

// cum[j] = excl[j] + q[j] - excl[start of j's row]; npos[r] += positions with q > 0
template <typename T>
__global__ __launch_bounds__(kBlock) void weight_finish_kernel(QuantAt<T> qa, const int64_t* __restrict__ indptr, int64_t num_edges,
                                                               const int64_t* __restrict__ excl, int64_t* __restrict__ cum,
                                                               unsigned long long* __restrict__ npos) {
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < num_edges; base += (int64_t)gridDim.x * kBlock) {
        const int64_t j = base + threadIdx.x;
        int64_t r = -1;
        unsigned long long pos = 0;
        if (j < num_edges) {
            double w;
            (void)qa.at(j, w, r);
            const int64_t q = qa(j);
            int64_t start = r >= 0 ? indptr[r] : j;
            if (start < 0 || start > j) start = j;            // (an index whose rows do not match its positions: stay inside excl)
            cum[j] = excl[j] + q - excl[start];
            pos = q > 0;
        }
        const bool last = wave_run_reduce(r, pos, AddU64());
        if (last && r >= 0 && pos) atomicAdd(&npos[r], pos);
    }
}

// ---- weighted neighbour sampling ---------------------------------------------------------------------------------------
constexpr int kMaxSampleW = 64;          // kMaxSample of sampling.hip

__global__ __launch_bounds__(kBlock) void sample_weighted_count_kernel(const int64_t* __restrict__ npos, const int64_t* __restrict__ nodes,
                                                                       int64_t n, int64_t k, int64_t* __restrict__ count) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t np = npos[nodes[i]];
        count[i] = (k < 0 || np <= k) ? np : k;
    }
}

__global__ __launch_bounds__(kBlock) void sample_weighted_fill_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                                      const int32_t* __restrict__ eid, const int64_t* __restrict__ cum,
                                                                      const int64_t* __restrict__ npos, const int64_t* __restrict__ nodes,
                                                                      int64_t n, int64_t k, uint64_t seed, const int64_t* __restrict__ offsets,
                                                                      int64_t* __restrict__ out_nbr, int64_t* __restrict__ out_eid) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t v = nodes[i];
        const int64_t b = indptr[v], deg = indptr[v + 1] - b;
        const int64_t np = npos[v], o = offsets[i];
        if (k < 0 || np <= k) {                                // the whole positive set, in row order
            int64_t before = 0, w = 0;
            for (int64_t j = 0; j < deg && w < np; ++j) {
                const int64_t c = cum[b + j];
                if (c > before) {
                    out_nbr[o + w] = col[b + j];
                    if (out_eid) out_eid[o + w] = eid[b + j];
                    ++w;
                }
                before = c;
            }
            continue;
        }
        // successive sampling; the chosen positions sorted ascending: rel (position in the row), qv (its q), cv (cum there)
        int32_t rel[kMaxSampleW];
        int64_t qv[kMaxSampleW], cv[kMaxSampleW];
        int cnt = 0;
        uint64_t rest = (uint64_t)cum[b + deg - 1];
        for (int64_t c = 0; c < k; ++c) {
            const uint64_t r = walk::scale64(walk::mix64(seed ^ walk::mix64((uint64_t)v * 0x100000001B3ull + (uint64_t)c)), rest);
            // S(j) = cum[j] - (q of the chosen positions <= j) is the running sum over the positions not yet chosen; it does
            // not move at a chosen position, so the smallest j with S(j) > r lies strictly between two chosen ones
            int64_t removed = 0, lo = 0;
            int at = 0;
            while (at < cnt && (uint64_t)(cv[at] - removed - qv[at]) <= r) { removed += qv[at]; lo = (int64_t)rel[at] + 1; ++at; }
            const int64_t hi = at < cnt ? (int64_t)rel[at] - 1 : deg - 1;
            int64_t j = walk::upper_bound_i64(cum, b + lo, b + hi, r + (uint64_t)removed);
            if (j > b + deg - 1) j = b + deg - 1;              // (not reached with a table of this index)
            const int64_t cj = cum[j], qj = cj - (j > b ? cum[j - 1] : 0);
            for (int s = cnt; s > at; --s) { rel[s] = rel[s - 1]; qv[s] = qv[s - 1]; cv[s] = cv[s - 1]; }
            rel[at] = (int32_t)(j - b); qv[at] = qj; cv[at] = cj;
            ++cnt;
            rest -= (uint64_t)qj;
            out_nbr[o + c] = col[j];
            if (out_eid) out_eid[o + c] = eid[j];
        }
    }
}

// ---- draws from a single-row table -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sample_from_table_kernel(const int64_t* __restrict__ cum, int64_t n, int64_t count, uint64_t seed,
                                                                   int64_t* __restrict__ out) {
    const uint64_t total = (uint64_t)cum[n - 1];
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock)
        out[i] = total ? walk::upper_bound_i64(cum, 0, n - 1, walk::scale64(walk::mix64(seed ^ walk::mix64((uint64_t)i)), total)) : -1;
}

static unsigned grid_for(int64_t n) {
    const int64_t g = ceil_div(n > 0 ? n : 1, kBlock);
    return (unsigned)(g < 256 * 16 ? g : 256 * 16);
}

template <typename T>
static int32_t build_table(const int64_t* indptr, const int32_t* row, const int32_t* eid, const T* weight, int64_t num_nodes,
                           int64_t num_edges, int64_t num_weights, int64_t* cum, int64_t* npos, int32_t* flag,
                           unsigned long long* rowmax, int64_t* excl, void* temp, hipStream_t st) {
    const WeightAt<T> at{row, eid, weight, num_nodes, num_weights};
    const QuantAt<T> qa{at, rowmax};
    hipLaunchKernelGGL((weight_row_max_kernel<T>), dim3(grid_for(num_edges)), dim3(kBlock), 0, st, at, num_edges, rowmax, flag);
    PGLAMD_LAUNCH_CHECK();
    PGLAMD_TRY(exclusive_scan64(qa, num_edges, excl, temp, st));
    hipLaunchKernelGGL((weight_finish_kernel<T>), dim3(grid_for(num_edges)), dim3(kBlock), 0, st, qa, indptr, num_edges, excl, cum,
                       reinterpret_cast<unsigned long long*>(npos));
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_edge_weight_table_workspace_bytes(int64_t num_nodes, int64_t num_edges) {
    const size_t n = (size_t)(num_nodes > 0 ? num_nodes : 1), e = (size_t)(num_edges > 0 ? num_edges : 1);
    return align_up(n * 8, 256) + align_up(e * 8, 256) + align_up(exclusive_scan64_temp_bytes(num_edges), 256) + 256;
}

extern "C" int32_t pglamd_edge_weight_table(const int64_t* indptr, const int32_t* row, const int32_t* eid, const void* weight,
                                            int32_t weight_f64, int64_t num_nodes, int64_t num_edges, int64_t num_weights,
                                            int64_t* cum, int64_t* npos, int32_t* flag, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    if (num_nodes < 0 || num_edges < 0 || num_weights < 0 || !flag || (num_nodes > 0 && (!indptr || !npos)) ||
        (num_edges > 0 && (!weight || !cum)) || (!row && num_nodes > 1 && num_edges > 0))
        return fail(PGLAMD_E_ARG, "edge_weight_table: bad argument (row may be NULL only for a single-row table)");
    if (num_edges > kMaxEdges || num_nodes > INT32_MAX)
        return fail(PGLAMD_E_RANGE, "edge_weight_table: %lld edges / %lld nodes out of range", (long long)num_edges, (long long)num_nodes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PGLAMD_HIP_CHECK(hipMemsetAsync(flag, 0, 4, st));
    if (num_nodes > 0) PGLAMD_HIP_CHECK(hipMemsetAsync(npos, 0, (size_t)num_nodes * 8, st));
    if (num_edges == 0) return PGLAMD_OK;
    if (!workspace || workspace_bytes < pglamd_edge_weight_table_workspace_bytes(num_nodes, num_edges))
        return fail(PGLAMD_E_WORKSPACE, "edge_weight_table: workspace too small");
    Carver cv(workspace, workspace_bytes);
    unsigned long long* rowmax = cv.take<unsigned long long>((size_t)num_nodes);
    int64_t* excl = cv.take<int64_t>((size_t)num_edges);
    void* temp = cv.take<char>(exclusive_scan64_temp_bytes(num_edges));
    PGLAMD_HIP_CHECK(hipMemsetAsync(rowmax, 0, (size_t)num_nodes * 8, st));
    return weight_f64 ? build_table(indptr, row, eid, static_cast<const double*>(weight), num_nodes, num_edges, num_weights, cum, npos,
                                    flag, rowmax, excl, temp, st)
                      : build_table(indptr, row, eid, static_cast<const float*>(weight), num_nodes, num_edges, num_weights, cum, npos,
                                    flag, rowmax, excl, temp, st);
}

extern "C" int32_t pglamd_sample_neighbors_weighted_count(const int64_t* npos, const int64_t* nodes, int64_t n, int64_t k,
                                                          int64_t* count, void* stream) {
    if (n < 0 || (n > 0 && (!npos || !nodes || !count))) return fail(PGLAMD_E_ARG, "sample_neighbors_weighted_count: bad argument");
    if (k > kMaxSampleW) return fail(PGLAMD_E_SHAPE, "sample_neighbors_weighted: sample size %lld > %d", (long long)k, kMaxSampleW);
    if (n == 0) return PGLAMD_OK;
    hipLaunchKernelGGL(sample_weighted_count_kernel, dim3(grid_for(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), npos, nodes, n, k, count);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_sample_neighbors_weighted_fill(const int64_t* indptr, const int32_t* col, const int32_t* eid, const int64_t* cum,
                                                         const int64_t* npos, const int64_t* nodes, int64_t n, int64_t k, uint64_t seed,
                                                         const int64_t* offsets, int64_t* out_neighbors, int64_t* out_eids, void* stream) {
    if (n < 0 || (n > 0 && (!indptr || !col || !cum || !npos || !nodes || !offsets || !out_neighbors)) || (out_eids && !eid))
        return fail(PGLAMD_E_ARG, "sample_neighbors_weighted_fill: bad argument");
    if (k > kMaxSampleW) return fail(PGLAMD_E_SHAPE, "sample_neighbors_weighted: sample size %lld > %d", (long long)k, kMaxSampleW);
    if (n == 0) return PGLAMD_OK;
    hipLaunchKernelGGL(sample_weighted_fill_kernel, dim3(grid_for(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), indptr, col, eid,
                       cum, npos, nodes, n, k, seed, offsets, out_neighbors, out_eids);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_sample_from_table(const int64_t* cum, int64_t n, int64_t count, uint64_t seed, int64_t* out, void* stream) {
    if (n < 0 || count < 0 || (count > 0 && (!out || n == 0 || !cum)))
        return fail(PGLAMD_E_ARG, "sample_from_table: bad argument (draws from an empty table)");
    if (count == 0) return PGLAMD_OK;
    hipLaunchKernelGGL(sample_from_table_kernel, dim3(grid_for(count)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), cum, n, count, seed, out);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}
