// negative.hip -- negative sampling checked against the graph, on the GPU: for every source of a batch, K ids of a candidate range
// that are NOT successors of the source (and optionally not the source), uniform or by a noise table, plus optionally one uniform
// positive per source -- a BPR triple per (source, k) in one launch.  Stands in for
//   UniformSample_original_python          (examples/lightgcn/utils.py: per user a positive, then `while True: negitem =
//                                           randint(...)` until the item is not in posForUser; examples/ngcf does the same)
//   the unchecked torch.randint / sample_from_table negatives of a skip-gram loop (examples/train_deepwalk.py)
// The definition and the draw logic live in negative_core.hpp, shared with the host twin (host_ops.cpp).
//
// One lane per (i, k) draw, the K lanes of one source next to each other: they read the same row bounds and, in their binary
// searches, the same cache lines of the row.  A trial is one hash, one multiply-high and one binary search of the row; with
// max_trials = 16 the exact fallback (a walk of the row: divergent and slow) runs with probability (|X_i| / (hi - lo))^16 and is
// kept out of line.  Grid-stride loop over a capped launch, no workspace, no host read.
#include "common.hpp"
#include "negative_core.hpp"

namespace pglamd {

// SMALL: n * K < 2^32, the lane's (i, k) split is a 32-bit division (a tenth of the 64-bit one)
template <bool SMALL>
__global__ __launch_bounds__(kBlock) void negative_kernel(negative::Args a) {
    const int64_t total = a.n * a.num_neg;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < total; g += (int64_t)gridDim.x * kBlock) {
        const int64_t i = SMALL ? (int64_t)((uint32_t)g / (uint32_t)a.num_neg) : g / a.num_neg;
        const int64_t k = g - i * a.num_neg;
        const int64_t v = a.src[i];
        if (v < 0 || v >= a.num_nodes) {                   // never dereferenced
            a.neg[g] = -1;
            if (k == 0) {
                if (a.pos) a.pos[i] = -1;
                if (a.flags) atomicOr(a.flags, negative::kFlagRange);
            }
            continue;
        }
        const int64_t b = a.indptr[v], end = a.indptr[v + 1];
        const uint64_t key = walk::walker_key(a.seed, i);
        const int64_t x = negative::draw_negative(a, v, b, end, key, k);
        a.neg[g] = x;
        if (x < 0 && a.flags) atomicOr(a.flags, negative::kFlagEmpty);
        if (k == 0 && a.pos) a.pos[i] = negative::draw_positive(a, b, end, key);
    }
}

}  // namespace pglamd

using namespace pglamd;

extern "C" int32_t pglamd_sample_negatives(const int64_t* indptr, const int32_t* col, int64_t num_nodes, const int64_t* cum, int64_t lo,
                                           int64_t hi, const int64_t* src, int64_t n, int64_t num_neg, int32_t exclude_self,
                                           int32_t max_trials, uint64_t seed, int64_t* neg, int64_t* pos, int32_t* flags, void* stream) {
    const negative::Args a{indptr, col, num_nodes, cum, lo, hi, src, n, num_neg, exclude_self, max_trials, seed, neg, pos, flags};
    const char* why = nullptr;
    if (const int32_t rc = negative::check_args(a, &why))
        return fail(rc, "sample_negatives: %s (lo %lld, hi %lld, num_nodes %lld, n %lld, num_neg %lld, max_trials %d)", why, (long long)lo,
                    (long long)hi, (long long)num_nodes, (long long)n, (long long)num_neg, (int)max_trials);
    if (n == 0) return PGLAMD_OK;
    const int64_t total = n * num_neg, blocks = ceil_div(total, kBlock);
    const dim3 grid((unsigned)(blocks < 256 * 32 ? blocks : 256 * 32));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (total <= (int64_t)UINT32_MAX && num_neg <= (int64_t)UINT32_MAX)
        hipLaunchKernelGGL(negative_kernel<true>, grid, dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL(negative_kernel<false>, grid, dim3(kBlock), 0, st, a);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}
