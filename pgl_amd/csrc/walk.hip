// walk.hip -- random walks (uniform, node2vec, node2vec-plus, edge-weighted) and their skip-gram pairs on the GPU.  Stands in for
//   pgl.sampling.random_walk / node2vec_walk / node2vec_walk_plus       (pgl/sampling/walk.py:23-185)
//   graph_kernel.node2vec_sample / node2vec_plus_sample                  (pgl/graph_kernel.pyx:140-224)
//   graph_kernel.skip_gram_gen_pair                                      (pgl/graph_kernel.pyx:341-364)
//
// Walk: ONE launch runs every step of every walker (the reference loops over steps in Python with a per-walker inner loop).
// A step is two dependent random reads (indptr[cur], indptr[cur + 1]; then col[b + r]); their latency is hidden by occupancy
// and by K walkers per lane whose loads are issued together.  The step logic itself lives in walk_core.hpp, shared with the
// host twin.  The edge-weighted mode (pglamd_random_walk_weighted; the reference has none) adds one binary search of the row's
// integer prefix sums (weighted.hip builds them) to the uniform step.  Paths are not stored step by step (one step of 64
// walkers would be 64 stores into 64 different rows): a block stages its walkers' last kSeg positions in LDS as int32 ids and
// flushes each walker's kSeg-position segment as one contiguous run of its row.
//
// Metapath walks over a HeterGraph (pglamd_metapath_walk; the reference: metapath_randomwalk,
// examples/metapath2vec/datasets/sampling.py:285-398, one sample_successor call per step) are the uniform / weighted modes of
// the same kernel over a relation-stacked index: the only difference is which block of indptr a position's step reads
// (walk::Metapath, walk_core.hpp), looked up once per position for the whole workgroup from the kernel's argument block.
//
// Skip-gram: one thread per (walker, position) counts the pairs of that position, the caller scans the counts, a second pass
// writes them.  The window of a position is a hash of (seed, walker, position), so both passes agree.
#include "common.hpp"
#include "walk_core.hpp"

namespace pglamd {

constexpr int kSeg = 8;                 // positions staged per flush
constexpr int kSegStride = kSeg + 1;    // LDS row stride in dwords (odd: the per-step writes of a wave hit distinct banks)

template <int K>
struct WalkArgs {
    const int64_t* indptr; const int32_t* col; int64_t num_nodes; const int64_t* starts; int64_t num_walkers; int64_t num_steps;
    uint64_t thr[3]; int32_t max_trials; uint64_t seed; int64_t* paths; int64_t* lengths; int32_t* range_flag;
    const int64_t* cum;       // kWeighted: the row-wise prefix sums of the integer edge weights (pglamd_edge_weight_table), else unused
};

// History of one walker for the plus mode: positions of the current segment from LDS, older ones from its flushed row.
struct Hist {
    const int32_t* stage; const int64_t* row; int64_t seg0;
    __device__ int64_t operator()(int64_t j) const { return j >= seg0 ? (int64_t)stage[j - seg0] : row[j]; }
};

// Rows (walk_core.hpp): which block of the index the step from a position reads -- OneRelation for the walks over a plain index
// (a.indptr itself: nothing is added to them), Metapath for pglamd_metapath_walk's relation-stacked index.
template <int MODE, int K, class Rows>
__global__ __launch_bounds__(kBlock) void walk_kernel(WalkArgs<K> a, Rows rows) {
    __shared__ int32_t stage[K * kBlock * kSegStride];
    const int64_t width = a.num_steps + 1;
    const int64_t base = (int64_t)blockIdx.x * (K * kBlock);
    int64_t cur[K], prev[K], len[K];
    uint64_t key[K];
    bool alive[K];
    const uint64_t thr[3] = {a.thr[0], a.thr[1], a.thr[2]};
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t w = base + k * kBlock + threadIdx.x;
        key[k] = walk::walker_key(a.seed, w);
        cur[k] = -1; prev[k] = -1; len[k] = 0; alive[k] = false;
        if (w < a.num_walkers) {
            const int64_t s = a.starts[w];
            cur[k] = s; len[k] = 1;
            alive[k] = s >= 0 && s < a.num_nodes;
            if (!alive[k] && a.range_flag) atomicOr(a.range_flag, 1);
        }
    }
    for (int64_t seg0 = 0; seg0 < width; seg0 += kSeg) {
        const int nseg = (int)(width - seg0 < kSeg ? width - seg0 : kSeg);
        for (int j = 0; j < nseg; ++j) {
            const int64_t t = seg0 + j;          // position being written
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) stage[(k * kBlock + threadIdx.x) * kSegStride] = (int32_t)cur[k];
                continue;
            }
            // position t - 1 holds cur: load every walker's row bounds first (K independent loads in flight) ...
            const int64_t* ip = rows.rows(a.indptr, t - 1);      // (the same for every walker of the block: one scalar look-up)
            int64_t b[K], deg[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                b[k] = 0; deg[k] = 0;
                if (alive[k]) { b[k] = ip[cur[k]]; deg[k] = ip[cur[k] + 1] - b[k]; }
            }
            int64_t nxt[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                nxt[k] = -1;
                if (alive[k] && deg[k] == 0) alive[k] = false;
                if (!alive[k]) continue;
                if (MODE == walk::kWeighted) {
                    nxt[k] = walk::weighted_step(a.col, a.cum, b[k], deg[k], t - 1, key[k]);
                    if (nxt[k] < 0) alive[k] = false;      // a row of zero weights: a dead end
                } else if (MODE == walk::kUniform || t == 1) {
                    nxt[k] = walk::uniform_step(a.col, b[k], deg[k], t - 1, key[k]);
                } else {
                    const int slot = k * kBlock + threadIdx.x;
                    const Hist h{stage + slot * kSegStride, a.paths + (base + slot) * width, seg0};
                    nxt[k] = walk::second_order_step(a.indptr, a.col, b[k], deg[k], prev[k], MODE == walk::kPlus, t - 1, h,
                                                     thr, a.max_trials, key[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (nxt[k] >= 0) { prev[k] = cur[k]; cur[k] = nxt[k]; len[k] = t + 1; }
                stage[(k * kBlock + threadIdx.x) * kSegStride + j] = (int32_t)nxt[k];
            }
        }
        __syncthreads();
        // flush: consecutive threads write consecutive positions of one walker's row (nseg-long contiguous runs)
        for (int i = threadIdx.x; i < K * kBlock * nseg; i += kBlock) {
            const int slot = i / nseg, j = i - slot * nseg;
            const int64_t w = base + slot;
            if (w < a.num_walkers) {
                const int32_t v = stage[slot * kSegStride + j];
                // position 0 keeps the start id as given (it may lie outside [0, N) and beyond int32)
                a.paths[w * width + seg0 + j] = (seg0 + j == 0) ? a.starts[w] : (int64_t)v;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t w = base + k * kBlock + threadIdx.x;
        if (w < a.num_walkers) a.lengths[w] = len[k];
    }
}

// ---- skip-gram pairs ---------------------------------------------------------------------------------------------------
// Position i of walker w (length l) pairs walk[i] with every walk[j], j in [max(0, i - r), min(l - 1, i + r)], j ascending,
// walk[j] != walk[i]; r = skip_gram_window(seed, w, i, win).
template <bool FILL>
__global__ __launch_bounds__(kBlock) void skip_gram_kernel(const int64_t* __restrict__ paths, const int64_t* __restrict__ lengths,
                                                           int64_t num_walkers, int64_t width, int64_t win, uint64_t seed,
                                                           int64_t* __restrict__ count, const int64_t* __restrict__ offsets,
                                                           int64_t* __restrict__ src, int64_t* __restrict__ dst) {
    const int64_t total = num_walkers * width;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < total; g += (int64_t)gridDim.x * kBlock) {
        const int64_t w = g / width, i = g - w * width;
        const int64_t l = lengths[w] < width ? lengths[w] : width;     // (a row holds at most width nodes)
        if (i >= l) {
            if (!FILL) count[g] = 0;
            continue;
        }
        const int64_t* row = paths + w * width;
        const int64_t r = walk::skip_gram_window(seed, w, i, win);
        const int64_t lo = i - r < 0 ? 0 : i - r, hi = i + r > l - 1 ? l - 1 : i + r;
        const int64_t c = row[i];
        int64_t o = FILL ? offsets[g] : 0;
        for (int64_t j = lo; j <= hi; ++j) {
            const int64_t x = row[j];
            if (x == c) continue;
            if (FILL) { src[o] = c; dst[o] = x; }
            ++o;
        }
        if (!FILL) count[g] = o;
    }
}

static unsigned grid_for(int64_t n) {
    const int64_t g = ceil_div(n > 0 ? n : 1, kBlock);
    return (unsigned)(g < 256 * 32 ? g : 256 * 32);
}

template <int MODE, int K, class Rows = walk::OneRelation>
static int32_t launch_walk(const WalkArgs<K>& a, hipStream_t st, const Rows& rows = Rows()) {
    const int64_t blocks = ceil_div(a.num_walkers, K * kBlock);
    hipLaunchKernelGGL((walk_kernel<MODE, K, Rows>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a, rows);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

}  // namespace pglamd

using namespace pglamd;

extern "C" int32_t pglamd_random_walk(const int64_t* indptr, const int32_t* col, int64_t num_nodes, const int64_t* starts,
                                      int64_t num_walkers, int64_t num_steps, int32_t mode, uint64_t thr_return, uint64_t thr_in,
                                      uint64_t thr_out, int32_t max_trials, uint64_t seed, int64_t* paths, int64_t* lengths,
                                      int32_t* range_flag, void* stream) {
    if (num_walkers < 0 || num_steps < 0 || num_nodes < 0 || (num_walkers > 0 && (!indptr || !col || !starts || !paths || !lengths)))
        return fail(PGLAMD_E_ARG, "random_walk: bad argument");
    if (mode < walk::kUniform || mode > walk::kPlus) return fail(PGLAMD_E_ARG, "random_walk: mode %d not in {0, 1, 2}", (int)mode);
    if (max_trials < 0 || max_trials > walk::kMaxTrials) return fail(PGLAMD_E_ARG, "random_walk: max_trials %d outside [0, %d]", (int)max_trials, walk::kMaxTrials);
    if (thr_return > (1ull << 32) || thr_in > (1ull << 32) || thr_out > (1ull << 32))
        return fail(PGLAMD_E_ARG, "random_walk: acceptance thresholds must lie in [0, 2^32]");
    if (num_nodes > INT32_MAX || num_steps > ((int64_t)1 << 40) || num_walkers > ((int64_t)1 << 40))
        return fail(PGLAMD_E_RANGE, "random_walk: num_nodes / num_steps / num_walkers out of range");
    if (num_walkers == 0) return PGLAMD_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == walk::kUniform) {
        WalkArgs<2> a{indptr, col, num_nodes, starts, num_walkers, num_steps, {thr_return, thr_in, thr_out}, max_trials, seed, paths, lengths, range_flag, nullptr};
        return launch_walk<walk::kUniform, 2>(a, st);
    }
    WalkArgs<1> a{indptr, col, num_nodes, starts, num_walkers, num_steps, {thr_return, thr_in, thr_out}, max_trials, seed, paths, lengths, range_flag, nullptr};
    return mode == walk::kNode2vec ? launch_walk<walk::kNode2vec, 1>(a, st) : launch_walk<walk::kPlus, 1>(a, st);
}

extern "C" int32_t pglamd_random_walk_weighted(const int64_t* indptr, const int32_t* col, const int64_t* cum, int64_t num_nodes,
                                               const int64_t* starts, int64_t num_walkers, int64_t num_steps, uint64_t seed,
                                               int64_t* paths, int64_t* lengths, int32_t* range_flag, void* stream) {
    if (num_walkers < 0 || num_steps < 0 || num_nodes < 0 ||
        (num_walkers > 0 && (!indptr || !col || !cum || !starts || !paths || !lengths)))
        return fail(PGLAMD_E_ARG, "random_walk_weighted: bad argument");
    if (num_nodes > INT32_MAX || num_steps > ((int64_t)1 << 40) || num_walkers > ((int64_t)1 << 40))
        return fail(PGLAMD_E_RANGE, "random_walk_weighted: num_nodes / num_steps / num_walkers out of range");
    if (num_walkers == 0) return PGLAMD_OK;
    WalkArgs<2> a{indptr, col, num_nodes, starts, num_walkers, num_steps, {0, 0, 0}, 0, seed, paths, lengths, range_flag, cum};
    return launch_walk<walk::kWeighted, 2>(a, static_cast<hipStream_t>(stream));
}

extern "C" int32_t pglamd_metapath_walk(const int64_t* indptr, const int32_t* col, const int64_t* cum, int64_t num_nodes,
                                        int32_t num_relations, const int32_t* metapath, int32_t metapath_len, int32_t phase,
                                        const int64_t* starts, int64_t num_walkers, int64_t num_steps, uint64_t seed, int64_t* paths,
                                        int64_t* lengths, int32_t* range_flag, void* stream) {
    if (num_walkers < 0 || num_steps < 0 || num_nodes < 0 || (num_walkers > 0 && (!indptr || !col || !starts || !paths || !lengths)))
        return fail(PGLAMD_E_ARG, "metapath_walk: bad argument");
    walk::Metapath mp;
    if (const char* why = walk::make_metapath(metapath, metapath_len, phase, num_relations, num_nodes, &mp))
        return fail(PGLAMD_E_ARG, "metapath_walk: %s (metapath_len %d, phase %d, num_relations %d)", why, (int)metapath_len, (int)phase,
                    (int)num_relations);
    if (num_nodes > INT32_MAX || num_steps > ((int64_t)1 << 40) || num_walkers > ((int64_t)1 << 40))
        return fail(PGLAMD_E_RANGE, "metapath_walk: num_nodes / num_steps / num_walkers out of range");
    if (num_walkers == 0) return PGLAMD_OK;
    WalkArgs<2> a{indptr, col, num_nodes, starts, num_walkers, num_steps, {0, 0, 0}, 0, seed, paths, lengths, range_flag, cum};
    hipStream_t st = static_cast<hipStream_t>(stream);
    return cum ? launch_walk<walk::kWeighted, 2>(a, st, mp) : launch_walk<walk::kUniform, 2>(a, st, mp);
}

static int32_t skip_gram_check(const int64_t* paths, const int64_t* lengths, int64_t num_walkers, int64_t width, int64_t win) {
    if (num_walkers < 0 || width < 1 || win < 1 || (num_walkers > 0 && (!paths || !lengths)))
        return fail(PGLAMD_E_ARG, "skip_gram: bad argument");
    if (win > INT32_MAX) return fail(PGLAMD_E_RANGE, "skip_gram: win_size %lld too large", (long long)win);
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_skip_gram_count(const int64_t* paths, const int64_t* lengths, int64_t num_walkers, int64_t width,
                                          int64_t win_size, uint64_t seed, int64_t* count, void* stream) {
    const int32_t rc = skip_gram_check(paths, lengths, num_walkers, width, win_size);
    if (rc != PGLAMD_OK) return rc;
    if (num_walkers == 0) return PGLAMD_OK;
    if (!count) return fail(PGLAMD_E_ARG, "skip_gram_count: NULL count");
    hipLaunchKernelGGL(skip_gram_kernel<false>, dim3(grid_for(num_walkers * width)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       paths, lengths, num_walkers, width, win_size, seed, count, nullptr, nullptr, nullptr);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_skip_gram_fill(const int64_t* paths, const int64_t* lengths, int64_t num_walkers, int64_t width,
                                         int64_t win_size, uint64_t seed, const int64_t* offsets, int64_t* src, int64_t* dst,
                                         void* stream) {
    const int32_t rc = skip_gram_check(paths, lengths, num_walkers, width, win_size);
    if (rc != PGLAMD_OK) return rc;
    if (num_walkers == 0) return PGLAMD_OK;
    if (!offsets || !src || !dst) return fail(PGLAMD_E_ARG, "skip_gram_fill: NULL pointer");
    hipLaunchKernelGGL(skip_gram_kernel<true>, dim3(grid_for(num_walkers * width)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       paths, lengths, num_walkers, width, win_size, seed, nullptr, offsets, src, dst);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}
