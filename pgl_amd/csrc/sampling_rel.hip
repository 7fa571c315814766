// sampling_rel.hip -- relation-wise neighbour sampling over a relation-stacked predecessor index: the mini-batch step of the
// relational models (RGCN, R-UniMP).  Stands in for the loop the reference's MAG240M example writes by hand
//   for each edge type: paddle.geometric.sample_neighbors(...)        (examples/NeurIPS2022-OGB-Challenge/MAG240M/dataset/
//   paddle.geometric.reindex_heter_graph(...) + an edge_split array    new_dataset_p2p.py:163-193)
// and for pgl.sampling.HeteroNeighborSampler, which the reference declares and leaves unimplemented (pgl/sampling/sage.py:158-162).
//
// The index: R blocks of N + 1 indptr entries over ONE col / eid array, block r = relation r's dst-sorted indptr plus the edges of
// relations 0 .. r-1 (absolute positions); eid holds relation-LOCAL edge ids.  One lane per (relation, seed): lane r * n + i
// samples seed i under relation r with fan-out f[r] and seed relation_seed(seed, r) -- exactly the picks pglamd_sample_neighbors_*
// makes over relation r's own index with that seed (sample_core.hpp: the same Floyd draws in the same order, the same whole-row
// copy).  The output is relation-major, then seed position, then draw order, so ONE exclusive scan of count[R * n] places every
// relation: a launch per relation, a scan per relation and a host read per relation become one of each.  The fill also writes the
// seed position of every slot (what reindex_graph's repeat_interleave produced, one more synchronisation).
//
// A whole-row copy longer than a wave (fan-out -1 on a hub) is done by the wave together, 64 consecutive entries per pass, after
// the lanes' own short rows: the same values to the same slots, only coalesced.  Batches are a few hundred seeds, so the launch
// is latency-bound and the grid is sized by R * n alone; the fan-outs travel in the kernel's argument block (no device copy).
#include "common.hpp"

#include "sample_core.hpp"

namespace pglamd {

struct Fanouts { int64_t f[sample::kMaxRelations]; };

__global__ __launch_bounds__(kBlock) void sample_relations_count_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ nodes,
                                                                        int64_t n, int64_t stride, int64_t total, Fanouts fan,
                                                                        int64_t* __restrict__ count) {
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlock) {
        const int64_t r = idx / n, i = idx - r * n;
        const int64_t k = fan.f[r];
        const int64_t v = nodes[i];
        const int64_t* ip = indptr + r * stride;
        count[idx] = k == 0 ? 0 : sample::sample_count(ip[v + 1] - ip[v], k);
    }
}

__global__ __launch_bounds__(kBlock) void sample_relations_fill_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ col,
                                                                       const int32_t* __restrict__ eid, const int64_t* __restrict__ nodes,
                                                                       int64_t n, int64_t stride, int64_t total, Fanouts fan, uint64_t seed,
                                                                       const int64_t* __restrict__ offsets, int64_t* __restrict__ out_nbr,
                                                                       int64_t* __restrict__ out_dst, int64_t* __restrict__ out_eid) {
    const int lane = threadIdx.x & (kWave - 1);
    // (the trip count is the block's, not the lane's: every lane of a wave reaches the ballot and the shuffles below)
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < total; base += (int64_t)gridDim.x * kBlock) {
        const int64_t idx = base + threadIdx.x;
        const bool valid = idx < total;
        int64_t r = 0, i = 0, k = 0, v = 0, b = 0, deg = 0, o = 0;
        if (valid) {
            r = idx / n; i = idx - r * n;
            k = fan.f[r];
            v = nodes[i];
            const int64_t* ip = indptr + r * stride;
            b = ip[v]; deg = ip[v + 1] - b;
            o = offsets[idx];
        }
        const bool copy = valid && k != 0 && (k < 0 || deg <= k);
        const bool wide = copy && deg > kWave;
        if (copy && !wide) {
            for (int64_t j = 0; j < deg; ++j) {
                out_nbr[o + j] = col[b + j];
                out_dst[o + j] = i;
                if (out_eid) out_eid[o + j] = eid[b + j];
            }
        } else if (valid && k > 0 && deg > k) {
            const uint64_t rs = sample::relation_seed(seed, r);
            int64_t chosen[sample::kMaxSample];
            int cnt = 0;
            for (; cnt < (int)k; ++cnt) chosen[cnt] = sample::floyd_draw(rs, v, deg, k, cnt, chosen);
            for (int q = 0; q < cnt; ++q) {
                out_nbr[o + q] = col[b + chosen[q]];
                out_dst[o + q] = i;
                if (out_eid) out_eid[o + q] = eid[b + chosen[q]];
            }
        }
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int owner = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t wb = __shfl(b, owner, kWave), wdeg = __shfl(deg, owner, kWave), wo = __shfl(o, owner, kWave),
                          wi = __shfl(i, owner, kWave);
            for (int64_t j = lane; j < wdeg; j += kWave) {
                out_nbr[wo + j] = col[wb + j];
                out_dst[wo + j] = wi;
                if (out_eid) out_eid[wo + j] = eid[wb + j];
            }
        }
    }
}

static unsigned rel_grid_for(int64_t total) {
    int64_t g = ceil_div(total > 0 ? total : 1, kBlock);
    return (unsigned)(g < 256 * 16 ? g : 256 * 16);
}

// What both entries refuse; on success *fan holds the fan-outs.
static int32_t check_relations(const char* what, int64_t n, int64_t num_nodes, int32_t num_relations, const int64_t* fanouts, Fanouts* fan) {
    if (n < 0 || num_nodes < 0 || !fanouts) return fail(PGLAMD_E_ARG, "%s: bad argument", what);
    if (num_relations < 1 || num_relations > sample::kMaxRelations)
        return fail(PGLAMD_E_SHAPE, "%s: num_relations %d outside [1, %d]", what, (int)num_relations, sample::kMaxRelations);
    if (num_nodes > INT32_MAX || n > ((int64_t)1 << 40)) return fail(PGLAMD_E_RANGE, "%s: num_nodes / n out of range", what);
    for (int32_t r = 0; r < sample::kMaxRelations; ++r) {
        fan->f[r] = r < num_relations ? fanouts[r] : 0;
        if (fan->f[r] > sample::kMaxSample)
            return fail(PGLAMD_E_SHAPE, "%s: fan-out %lld of relation %d > %d", what, (long long)fan->f[r], (int)r, sample::kMaxSample);
    }
    return PGLAMD_OK;
}

}  // namespace pglamd

using namespace pglamd;

extern "C" int32_t pglamd_sample_relations_count(const int64_t* indptr, int64_t num_nodes, int32_t num_relations, const int64_t* fanouts,
                                                 const int64_t* nodes, int64_t n, int64_t* count, void* stream) {
    Fanouts fan;
    PGLAMD_TRY(check_relations("sample_relations_count", n, num_nodes, num_relations, fanouts, &fan));
    if (n > 0 && (!indptr || !nodes || !count)) return fail(PGLAMD_E_ARG, "sample_relations_count: NULL pointer");
    if (n == 0) return PGLAMD_OK;
    const int64_t total = n * num_relations;
    hipLaunchKernelGGL(sample_relations_count_kernel, dim3(rel_grid_for(total)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), indptr,
                       nodes, n, num_nodes + 1, total, fan, count);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_sample_relations_fill(const int64_t* indptr, const int32_t* col, const int32_t* eid, int64_t num_nodes,
                                                int32_t num_relations, const int64_t* fanouts, const int64_t* nodes, int64_t n,
                                                uint64_t seed, const int64_t* offsets, int64_t* out_neighbors, int64_t* out_dst,
                                                int64_t* out_eids, void* stream) {
    Fanouts fan;
    PGLAMD_TRY(check_relations("sample_relations_fill", n, num_nodes, num_relations, fanouts, &fan));
    if ((n > 0 && (!indptr || !col || !nodes || !offsets || !out_neighbors || !out_dst)) || (out_eids && !eid))
        return fail(PGLAMD_E_ARG, "sample_relations_fill: NULL pointer");
    if (n == 0) return PGLAMD_OK;
    const int64_t total = n * num_relations;
    hipLaunchKernelGGL(sample_relations_fill_kernel, dim3(rel_grid_for(total)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), indptr,
                       col, eid, nodes, n, num_nodes + 1, total, fan, seed, offsets, out_neighbors, out_dst, out_eids);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}
