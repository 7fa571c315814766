// host_ops.cpp -- CPU-side helpers of libpglamd (HOST pointers): the host CSR build, id relabel and the halo plan of a
// row-partitioned graph.  (The engine's own partitioner -- what stands behind pgl.partition.metis_partition -- lives in
// partition.cpp; no METIS code is linked, opened or built by the product.)
//
// pglamd_build_index_host <- graph_kernel.build_index (pgl/graph_kernel.pyx:59-88)
// pglamd_map_ids          <- graph_kernel.map_edges / map_nodes (pgl/graph_kernel.pyx:104-138)
// pglamd_induced_subgraph_host <- graph_kernel.extract_edges_from_nodes (pgl/graph_kernel.pyx:394-432) + the relabel of
//                            pgl.sampling.custom.subgraph (pgl/sampling/custom.py:23-83)
// pglamd_random_walk_host <- pgl.sampling.random_walk / node2vec_walk(_plus) (pgl/sampling/walk.py:23-185,
//                            pgl/graph_kernel.pyx:140-224) for numpy-mode graphs
// pglamd_random_walk_weighted_host / pglamd_edge_weight_table_host: the host twins of the edge-weighted walk and of the integer
//                            weight table (weighted.hip); no reference counterpart
// pglamd_walk_visit_topk_host: the host twin of the PinSAGE visit counts (walk_visit.hip); no reference counterpart
// pglamd_sample_relations_host: the host twin of the relation-wise neighbour sampler (sampling_rel.hip) <- the per-edge-type
//                            sample_neighbors loop of examples/NeurIPS2022-OGB-Challenge/MAG240M/dataset/new_dataset_p2p.py:163-193
// pglamd_segment_topk_host / pglamd_filter_edges_host: the host twins of the pooling kernels (pool.hip) <- pgl/math.py:276-364,
//                            pgl/utils/transform.py:138-168
#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <unordered_map>
#include <vector>
#include <mutex>
#include <string>
#include <thread>

#include "../../include/pgl_amd.h"
#include "sample_core.hpp"
#include "walk_core.hpp"
#include "negative_core.hpp"
#include "pool_core.hpp"

namespace pglamd {
int32_t fail(int32_t code, const char* fmt, ...);
}

extern "C" int32_t pglamd_build_index_host(const int64_t* u, int64_t u_stride, const int64_t* v, int64_t v_stride,
                                           int64_t num_edges, int64_t num_nodes, int64_t* degree, int64_t* sorted_v,
                                           int64_t* sorted_u, int64_t* sorted_eid, int64_t* indptr) {
    if (num_edges < 0 || num_nodes < 0 || !indptr || (num_nodes > 0 && !degree) ||
        (num_edges > 0 && (!u || !v || !sorted_v || !sorted_u || !sorted_eid)))
        return pglamd::fail(PGLAMD_E_ARG, "build_index_host: bad argument");
    // histogram -> offsets -> stable placement (a cursor per row walks forward, so equal keys keep
    // their original edge order: the order the reference's counting sort produces)
    std::fill(degree, degree + num_nodes, int64_t(0));
    for (int64_t e = 0; e < num_edges; ++e) {
        const int64_t k = u[e * u_stride];
        if (k < 0 || k >= num_nodes) return pglamd::fail(PGLAMD_E_RANGE, "build_index_host: key %lld out of [0,%lld)", (long long)k, (long long)num_nodes);
        ++degree[k];
    }
    indptr[0] = 0;
    std::partial_sum(degree, degree + num_nodes, indptr + 1);
    std::vector<int64_t> cursor(indptr, indptr + num_nodes);
    for (int64_t e = 0; e < num_edges; ++e) {
        const int64_t k = u[e * u_stride];
        const int64_t slot = cursor[k]++;
        sorted_u[slot] = k;
        sorted_v[slot] = v[e * v_stride];
        sorted_eid[slot] = e;
    }
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_map_ids(const int64_t* keys, const int64_t* vals, int64_t n_keys, const int64_t* in,
                                  int64_t n_in, int64_t* out) {
    if (n_keys < 0 || n_in < 0 || (n_keys > 0 && (!keys || !vals)) || (n_in > 0 && (!in || !out)))
        return pglamd::fail(PGLAMD_E_ARG, "map_ids: bad argument");
    std::unordered_map<int64_t, int64_t> m;
    m.reserve((size_t)n_keys * 2);
    for (int64_t i = 0; i < n_keys; ++i) m[keys[i]] = vals[i];
    for (int64_t i = 0; i < n_in; ++i) {
        auto it = m.find(in[i]);
        out[i] = it == m.end() ? 0 : it->second;   // reference: unordered_map::operator[] -> 0
    }
    return PGLAMD_OK;
}

// Host twin of pglamd_induced_subgraph_count / _fill (subgraph.hip): the same three arrays from the same definition, one thread.
extern "C" int32_t pglamd_induced_subgraph_host(const int64_t* indptr, const int64_t* col, const int64_t* eid, int64_t num_nodes,
                                                const int64_t* nodes, int64_t n, int64_t* out_src, int64_t* out_dst,
                                                int64_t* out_eid, int64_t* num_out) {
    if (num_nodes < 0 || n < 0 || !num_out || (n > 0 && (!indptr || !nodes)))
        return pglamd::fail(PGLAMD_E_ARG, "induced_subgraph_host: bad argument");
    *num_out = 0;
    std::vector<int64_t> local((size_t)num_nodes, int64_t(-1));
    for (int64_t i = 0; i < n; ++i) {                       // every id is checked before it indexes anything
        const int64_t v = nodes[i];
        if (v < 0 || v >= num_nodes)
            return pglamd::fail(PGLAMD_E_ARG, "induced_subgraph_host: node id %lld out of [0,%lld)", (long long)v, (long long)num_nodes);
        if (local[v] >= 0)
            return pglamd::fail(PGLAMD_E_ARG, "induced_subgraph_host: node id %lld is repeated (positions %lld and %lld)", (long long)v,
                                (long long)local[v], (long long)i);
        local[v] = i;
    }
    int64_t o = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t v = nodes[i];
        for (int64_t j = indptr[v]; j < indptr[v + 1]; ++j) {
            const int64_t s = local[col[j]];
            if (s < 0) continue;
            if (!out_src || !out_dst || !out_eid) return pglamd::fail(PGLAMD_E_ARG, "induced_subgraph_host: NULL output");
            out_src[o] = s; out_dst[o] = i; out_eid[o] = eid ? eid[j] : j;
            ++o;
        }
    }
    *num_out = o;
    return PGLAMD_OK;
}

// ------------------------------------------------------------------------------------------------
// Halo plan of one rank of a row-partitioned graph (host side; SURVEY 8b pglhip_halo_plan_build).  Same arrays, element for
// element, as pgl_amd.distributed.HaloPlan builds with torch (pull plan): relabel so every part owns a contiguous id range
// (apps/GNNAutoScale/graph_partition.py:70-101), keep the in-edges of the owned rows split into local-source and
// halo-source edges, list the distinct halo sources grouped by owner and the owned rows every peer pulls.
// ------------------------------------------------------------------------------------------------
namespace {
struct PlanScratch {
    std::vector<int64_t> offsets, new_id, own_global, loc_rows, loc_cols, loc_eid, hal_src, hal_rows, hal_eid, halo_global,
        send_keys, in_degree, out_degree;
};

int32_t build_plan(const int64_t* src, int64_t ss, const int64_t* dst, int64_t ds, int64_t E, int64_t N, const int64_t* part,
                   int32_t rank, int32_t world, PlanScratch& s) {
    if (E < 0 || N < 0 || world < 1 || rank < 0 || rank >= world || (N > 0 && !part) || (E > 0 && (!src || !dst)))
        return pglamd::fail(PGLAMD_E_ARG, "halo_plan: bad argument");
    s.offsets.assign(world + 1, 0);
    for (int64_t v = 0; v < N; ++v) {
        if (part[v] < 0 || part[v] >= world) return pglamd::fail(PGLAMD_E_RANGE, "halo_plan: part[%lld] = %lld outside [0,%d)", (long long)v, (long long)part[v], world);
        ++s.offsets[part[v] + 1];
    }
    for (int p = 0; p < world; ++p) s.offsets[p + 1] += s.offsets[p];
    std::vector<int64_t> pos(s.offsets.begin(), s.offsets.end() - 1);
    s.new_id.resize(N);
    const int64_t lo = s.offsets[rank], n_own = s.offsets[rank + 1] - lo;
    s.own_global.clear(); s.own_global.reserve(n_own);
    for (int64_t v = 0; v < N; ++v) {                     // stable: ascending original id inside a part
        s.new_id[v] = pos[part[v]]++;
        if (part[v] == rank) s.own_global.push_back(v);
    }
    s.in_degree.assign(n_own, 0); s.out_degree.assign(n_own, 0);
    for (int64_t e = 0; e < E; ++e) {
        const int64_t u = src[e * ss], v = dst[e * ds];
        if (u < 0 || u >= N || v < 0 || v >= N) return pglamd::fail(PGLAMD_E_RANGE, "halo_plan: edge %lld outside [0,%lld)", (long long)e, (long long)N);
        const int64_t pu = part[u], pv = part[v], nu = s.new_id[u], nv = s.new_id[v];
        if (pv == rank) {
            ++s.in_degree[nv - lo];
            if (pu == rank) { s.loc_rows.push_back(nv - lo); s.loc_cols.push_back(nu - lo); s.loc_eid.push_back(e); }
            else { s.hal_src.push_back(nu); s.hal_rows.push_back(nv - lo); s.hal_eid.push_back(e); }
        }
        if (pu == rank) {
            ++s.out_degree[nu - lo];
            if (pv != rank) s.send_keys.push_back(pv * N + nu);
        }
    }
    s.halo_global = s.hal_src;
    std::sort(s.halo_global.begin(), s.halo_global.end());
    s.halo_global.erase(std::unique(s.halo_global.begin(), s.halo_global.end()), s.halo_global.end());
    std::sort(s.send_keys.begin(), s.send_keys.end());
    s.send_keys.erase(std::unique(s.send_keys.begin(), s.send_keys.end()), s.send_keys.end());
    return PGLAMD_OK;
}
}  // namespace

extern "C" int32_t pglamd_halo_plan_sizes(const int64_t* src, int64_t src_stride, const int64_t* dst, int64_t dst_stride,
                                          int64_t num_edges, int64_t num_nodes, const int64_t* part, int32_t rank, int32_t world,
                                          int64_t* sizes) {
    if (!sizes) return pglamd::fail(PGLAMD_E_ARG, "halo_plan_sizes: NULL sizes");
    PlanScratch s;
    const int32_t rc = build_plan(src, src_stride, dst, dst_stride, num_edges, num_nodes, part, rank, world, s);
    if (rc != PGLAMD_OK) return rc;
    sizes[0] = (int64_t)s.own_global.size(); sizes[1] = (int64_t)s.loc_rows.size(); sizes[2] = (int64_t)s.hal_rows.size();
    sizes[3] = (int64_t)s.halo_global.size(); sizes[4] = (int64_t)s.send_keys.size();
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_halo_plan_fill(const int64_t* src, int64_t src_stride, const int64_t* dst, int64_t dst_stride,
                                         int64_t num_edges, int64_t num_nodes, const int64_t* part, int32_t rank, int32_t world,
                                         int64_t* offsets, int64_t* own_global, int64_t* loc_rows, int64_t* loc_cols,
                                         int64_t* hal_rows, int64_t* hal_cols, int64_t* halo_global, int64_t* send_idx,
                                         int64_t* halo_splits, int64_t* pull_splits, int64_t* in_degree, int64_t* out_degree,
                                         int64_t* edge_global) {
    PlanScratch s;
    const int32_t rc = build_plan(src, src_stride, dst, dst_stride, num_edges, num_nodes, part, rank, world, s);
    if (rc != PGLAMD_OK) return rc;
    if (!offsets || !halo_splits || !pull_splits) return pglamd::fail(PGLAMD_E_ARG, "halo_plan_fill: NULL pointer");
    const int64_t N = num_nodes, lo = s.offsets[rank];
    auto put = [](int64_t* d, const std::vector<int64_t>& v) { if (d && !v.empty()) std::memcpy(d, v.data(), v.size() * sizeof(int64_t)); };
    put(offsets, s.offsets); put(own_global, s.own_global); put(loc_rows, s.loc_rows); put(loc_cols, s.loc_cols);
    put(hal_rows, s.hal_rows); put(halo_global, s.halo_global); put(in_degree, s.in_degree); put(out_degree, s.out_degree);
    if (hal_cols)
        for (size_t i = 0; i < s.hal_src.size(); ++i)
            hal_cols[i] = std::lower_bound(s.halo_global.begin(), s.halo_global.end(), s.hal_src[i]) - s.halo_global.begin();
    std::fill(halo_splits, halo_splits + world, (int64_t)0);
    for (int64_t g : s.halo_global) ++halo_splits[std::upper_bound(s.offsets.begin(), s.offsets.end(), g) - s.offsets.begin() - 1];
    std::fill(pull_splits, pull_splits + world, (int64_t)0);
    for (size_t i = 0; i < s.send_keys.size(); ++i) {
        ++pull_splits[s.send_keys[i] / N];
        if (send_idx) send_idx[i] = s.send_keys[i] % N - lo;
    }
    if (edge_global) {
        put(edge_global, s.loc_eid);
        if (!s.hal_eid.empty()) std::memcpy(edge_global + s.loc_eid.size(), s.hal_eid.data(), s.hal_eid.size() * sizeof(int64_t));
    }
    return PGLAMD_OK;
}

// ------------------------------------------------------------------------------------------------
// Host twin of pglamd_random_walk (walk.hip): the same step logic (walk_core.hpp), the same RNG, HOST pointers.  Walkers are
// independent and every draw is a function of (seed, walker, step, trial), so the split over threads changes nothing.
// ------------------------------------------------------------------------------------------------
namespace {
struct RowHist {
    const int64_t* row;
    int64_t operator()(int64_t j) const { return row[j]; }
};

// Rows (walk_core.hpp): OneRelation for a plain index, Metapath for a relation-stacked one (pglamd_metapath_walk_host; its
// callers pass num_nodes >= 0: a start outside [0, num_nodes) then stays a walk of the start alone, as on the device).
template <class Rows>
void walk_range(const int64_t* indptr, const int32_t* col, const int64_t* cum, const int64_t* starts, int64_t w0, int64_t w1, int64_t num_steps,
                int32_t mode, const uint64_t* thr, int32_t max_trials, uint64_t seed, int64_t* paths, int64_t* lengths, Rows rows,
                int64_t num_nodes) {
    using namespace pglamd::walk;
    const int64_t width = num_steps + 1;
    for (int64_t w = w0; w < w1; ++w) {
        int64_t* row = paths + w * width;
        const uint64_t key = walker_key(seed, w);
        int64_t cur = starts[w], prev = -1, len = 1;
        row[0] = cur;
        const bool outside = num_nodes >= 0 && (cur < 0 || cur >= num_nodes);
        for (int64_t t = 0; t < num_steps && !outside; ++t) {      // cur = row[t]
            const int64_t* ip = rows.rows(indptr, t);
            const int64_t b = ip[cur], deg = ip[cur + 1] - b;
            if (deg == 0) break;
            const int64_t nxt = mode == kWeighted ? weighted_step(col, cum, b, deg, t, key)
                : (mode == kUniform || t == 0)
                ? uniform_step(col, b, deg, t, key)
                : second_order_step(indptr, col, b, deg, prev, mode == kPlus, t, RowHist{row}, thr, max_trials, key);
            if (nxt < 0) break;                         // (kWeighted: every weight of the row is zero)
            prev = cur; cur = nxt;
            row[++len - 1] = cur;
        }
        for (int64_t t = len; t < width; ++t) row[t] = -1;
        lengths[w] = len;
    }
}

template <class Rows = pglamd::walk::OneRelation>
void walk_threads(const int64_t* indptr, const int32_t* col, const int64_t* cum, const int64_t* starts, int64_t num_walkers,
                  int64_t num_steps, int32_t mode, const uint64_t* thr, int32_t max_trials, uint64_t seed, int32_t threads,
                  int64_t* paths, int64_t* lengths, Rows rows = Rows(), int64_t num_nodes = -1) {
    int64_t nt = threads > 0 ? threads : (int64_t)std::thread::hardware_concurrency();
    nt = std::max<int64_t>(1, std::min<int64_t>({nt, 16, (num_walkers + 1023) / 1024}));
    if (nt == 1) {
        walk_range<Rows>(indptr, col, cum, starts, 0, num_walkers, num_steps, mode, thr, max_trials, seed, paths, lengths, rows, num_nodes);
        return;
    }
    std::vector<std::thread> pool;
    const int64_t per = (num_walkers + nt - 1) / nt;
    for (int64_t i = 0; i < nt; ++i) {
        const int64_t w0 = i * per, w1 = std::min(num_walkers, w0 + per);
        if (w0 < w1) pool.emplace_back(walk_range<Rows>, indptr, col, cum, starts, w0, w1, num_steps, mode, thr, max_trials, seed, paths, lengths, rows, num_nodes);
    }
    for (auto& th : pool) th.join();
}
}  // namespace

extern "C" int32_t pglamd_random_walk_host(const int64_t* indptr, const int32_t* col, int64_t num_nodes, const int64_t* starts,
                                           int64_t num_walkers, int64_t num_steps, int32_t mode, uint64_t thr_return,
                                           uint64_t thr_in, uint64_t thr_out, int32_t max_trials, uint64_t seed, int32_t threads,
                                           int64_t* paths, int64_t* lengths) {
    using namespace pglamd::walk;
    if (num_walkers < 0 || num_steps < 0 || num_nodes < 0 || (num_walkers > 0 && (!indptr || !col || !starts || !paths || !lengths)))
        return pglamd::fail(PGLAMD_E_ARG, "random_walk_host: bad argument");
    if (mode < kUniform || mode > kPlus) return pglamd::fail(PGLAMD_E_ARG, "random_walk_host: mode %d not in {0, 1, 2}", (int)mode);
    if (max_trials < 0 || max_trials > kMaxTrials)
        return pglamd::fail(PGLAMD_E_ARG, "random_walk_host: max_trials %d outside [0, %d]", (int)max_trials, kMaxTrials);
    if (thr_return > (1ull << 32) || thr_in > (1ull << 32) || thr_out > (1ull << 32))
        return pglamd::fail(PGLAMD_E_ARG, "random_walk_host: acceptance thresholds must lie in [0, 2^32]");
    if (num_nodes > INT32_MAX || num_steps > ((int64_t)1 << 40) || num_walkers > ((int64_t)1 << 40))
        return pglamd::fail(PGLAMD_E_RANGE, "random_walk_host: num_nodes / num_steps / num_walkers out of range");
    for (int64_t w = 0; w < num_walkers; ++w)
        if (starts[w] < 0 || starts[w] >= num_nodes)
            return pglamd::fail(PGLAMD_E_RANGE, "random_walk_host: start node %lld out of [0,%lld)", (long long)starts[w], (long long)num_nodes);
    const uint64_t thr[3] = {thr_return, thr_in, thr_out};
    walk_threads(indptr, col, nullptr, starts, num_walkers, num_steps, mode, thr, max_trials, seed, threads, paths, lengths);
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_random_walk_weighted_host(const int64_t* indptr, const int32_t* col, const int64_t* cum, int64_t num_nodes,
                                                    const int64_t* starts, int64_t num_walkers, int64_t num_steps, uint64_t seed,
                                                    int32_t threads, int64_t* paths, int64_t* lengths) {
    if (num_walkers < 0 || num_steps < 0 || num_nodes < 0 ||
        (num_walkers > 0 && (!indptr || !col || !cum || !starts || !paths || !lengths)))
        return pglamd::fail(PGLAMD_E_ARG, "random_walk_weighted_host: bad argument");
    if (num_nodes > INT32_MAX || num_steps > ((int64_t)1 << 40) || num_walkers > ((int64_t)1 << 40))
        return pglamd::fail(PGLAMD_E_RANGE, "random_walk_weighted_host: num_nodes / num_steps / num_walkers out of range");
    for (int64_t w = 0; w < num_walkers; ++w)
        if (starts[w] < 0 || starts[w] >= num_nodes)
            return pglamd::fail(PGLAMD_E_RANGE, "random_walk_weighted_host: start node %lld out of [0,%lld)", (long long)starts[w], (long long)num_nodes);
    const uint64_t thr[3] = {0, 0, 0};
    walk_threads(indptr, col, cum, starts, num_walkers, num_steps, pglamd::walk::kWeighted, thr, 0, seed, threads, paths, lengths);
    return PGLAMD_OK;
}

// Host twin of pglamd_metapath_walk (walk.hip): the walk above over a relation-stacked index, the block of a step chosen by the
// same walk::Metapath the kernel reads.  A start outside [0, N) raises *range_flag and keeps its length-1 walk, as on the device.
extern "C" int32_t pglamd_metapath_walk_host(const int64_t* indptr, const int32_t* col, const int64_t* cum, int64_t num_nodes,
                                             int32_t num_relations, const int32_t* metapath, int32_t metapath_len, int32_t phase,
                                             const int64_t* starts, int64_t num_walkers, int64_t num_steps, uint64_t seed,
                                             int32_t threads, int64_t* paths, int64_t* lengths, int32_t* range_flag) {
    if (num_walkers < 0 || num_steps < 0 || num_nodes < 0 || (num_walkers > 0 && (!indptr || !col || !starts || !paths || !lengths)))
        return pglamd::fail(PGLAMD_E_ARG, "metapath_walk_host: bad argument");
    pglamd::walk::Metapath mp;
    if (const char* why = pglamd::walk::make_metapath(metapath, metapath_len, phase, num_relations, num_nodes, &mp))
        return pglamd::fail(PGLAMD_E_ARG, "metapath_walk_host: %s (metapath_len %d, phase %d, num_relations %d)", why, (int)metapath_len,
                            (int)phase, (int)num_relations);
    if (num_nodes > INT32_MAX || num_steps > ((int64_t)1 << 40) || num_walkers > ((int64_t)1 << 40))
        return pglamd::fail(PGLAMD_E_RANGE, "metapath_walk_host: num_nodes / num_steps / num_walkers out of range");
    if (range_flag)
        for (int64_t w = 0; w < num_walkers; ++w)
            if (starts[w] < 0 || starts[w] >= num_nodes) { *range_flag |= 1; break; }
    const uint64_t thr[3] = {0, 0, 0};
    walk_threads(indptr, col, cum, starts, num_walkers, num_steps, cum ? pglamd::walk::kWeighted : pglamd::walk::kUniform, thr, 0, seed,
                 threads, paths, lengths, mp, num_nodes);
    return PGLAMD_OK;
}

// Host twin of pglamd_sample_negatives (negative.hip): the same draws (negative_core.hpp), HOST pointers.  Positions are
// independent and every draw is a function of (seed, position, k, trial), so the split over threads changes nothing.  A source
// outside [0, N) is an error here (PGLAMD_E_RANGE, as pglamd_random_walk_host), so only kFlagEmpty is ever raised.
extern "C" int32_t pglamd_sample_negatives_host(const int64_t* indptr, const int32_t* col, int64_t num_nodes, const int64_t* cum,
                                                int64_t lo, int64_t hi, const int64_t* src, int64_t n, int64_t num_neg,
                                                int32_t exclude_self, int32_t max_trials, uint64_t seed, int32_t threads, int64_t* neg,
                                                int64_t* pos, int32_t* flags) {
    namespace ng = pglamd::negative;
    const ng::Args a{indptr, col, num_nodes, cum, lo, hi, src, n, num_neg, exclude_self, max_trials, seed, neg, pos, flags};
    const char* why = nullptr;
    if (const int32_t rc = ng::check_args(a, &why))
        return pglamd::fail(rc, "sample_negatives_host: %s (lo %lld, hi %lld, num_nodes %lld, n %lld, num_neg %lld, max_trials %d)", why,
                            (long long)lo, (long long)hi, (long long)num_nodes, (long long)n, (long long)num_neg, (int)max_trials);
    for (int64_t i = 0; i < n; ++i)
        if (src[i] < 0 || src[i] >= num_nodes)
            return pglamd::fail(PGLAMD_E_RANGE, "sample_negatives_host: source %lld out of [0,%lld)", (long long)src[i], (long long)num_nodes);
    std::atomic<int32_t> raised{0};
    auto range = [&](int64_t i0, int64_t i1) {
        int32_t f = 0;
        for (int64_t i = i0; i < i1; ++i) {
            const int64_t v = src[i], b = indptr[v], end = indptr[v + 1];
            const uint64_t key = pglamd::walk::walker_key(seed, i);
            for (int64_t k = 0; k < num_neg; ++k) {
                const int64_t x = ng::draw_negative(a, v, b, end, key, k);
                neg[i * num_neg + k] = x;
                if (x < 0) f |= ng::kFlagEmpty;
            }
            if (pos) pos[i] = ng::draw_positive(a, b, end, key);
        }
        if (f) raised.fetch_or(f);
    };
    int64_t nt = threads > 0 ? threads : (int64_t)std::thread::hardware_concurrency();
    nt = std::max<int64_t>(1, std::min<int64_t>({nt, 16, (n * num_neg + 1023) / 1024}));
    if (nt == 1) {
        range(0, n);
    } else {
        std::vector<std::thread> pool;
        const int64_t per = (n + nt - 1) / nt;
        for (int64_t t = 0; t < nt; ++t) {
            const int64_t i0 = t * per, i1 = std::min(n, i0 + per);
            if (i0 < i1) pool.emplace_back(range, i0, i1);
        }
        for (auto& th : pool) th.join();
    }
    if (flags && raised.load()) *flags |= raised.load();
    return PGLAMD_OK;
}

// Host twin of pglamd_walk_visit_topk (walk_visit.hip): walker s * R + r walks with the step functions of walk_core.hpp, the
// visits of a seed are sorted, run-length encoded and ordered by the same packed key (count << 32 | 0xFFFFFFFF - node).
// Seeds are independent, so the split over threads changes nothing.
namespace {
void visit_range(const int64_t* indptr, const int32_t* col, const int64_t* cum, int64_t num_nodes, const int64_t* seeds, int64_t s0,
                 int64_t s1, int64_t R, int64_t L, int64_t T, uint64_t seed, int64_t* nbr, int32_t* cnt, int32_t* num,
                 std::atomic<int32_t>* flag) {
    using namespace pglamd::walk;
    std::vector<int64_t> visits;
    std::vector<uint64_t> keys;
    for (int64_t s = s0; s < s1; ++s) {
        int64_t* nrow = nbr + s * T;
        int32_t* crow = cnt + s * T;
        std::fill(nrow, nrow + T, (int64_t)-1);
        std::fill(crow, crow + T, (int32_t)0);
        num[s] = 0;
        const int64_t start = seeds[s];
        if (start < 0 || start >= num_nodes) { flag->fetch_or(1); continue; }
        visits.clear(); keys.clear();
        for (int64_t r = 0; r < R; ++r) {
            const uint64_t key = walker_key(seed, s * R + r);
            int64_t cur = start;
            for (int64_t t = 0; t < L; ++t) {
                const int64_t b = indptr[cur], deg = indptr[cur + 1] - b;
                if (deg == 0) break;
                const int64_t nxt = cum ? weighted_step(col, cum, b, deg, t, key) : uniform_step(col, b, deg, t, key);
                if (nxt < 0) break;
                cur = nxt;
                if (cur != start) visits.push_back(cur);
            }
        }
        std::sort(visits.begin(), visits.end());
        for (size_t i = 0; i < visits.size();) {
            size_t j = i;
            while (j < visits.size() && visits[j] == visits[i]) ++j;
            keys.push_back(((uint64_t)(j - i) << 32) | (0xFFFFFFFFull - (uint64_t)visits[i]));
            i = j;
        }
        std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
        const int64_t n = std::min<int64_t>(T, (int64_t)keys.size());
        for (int64_t j = 0; j < n; ++j) {
            nrow[j] = (int64_t)(0xFFFFFFFFull - (keys[j] & 0xFFFFFFFFull));
            crow[j] = (int32_t)(keys[j] >> 32);
        }
        num[s] = (int32_t)n;
    }
}
}  // namespace

extern "C" int32_t pglamd_walk_visit_topk_host(const int64_t* indptr, const int32_t* col, const int64_t* cum, int64_t num_nodes,
                                               const int64_t* seeds, int64_t num_seeds, int64_t num_walks, int64_t num_steps,
                                               int64_t top_k, uint64_t seed, int32_t threads, int64_t* nbr, int32_t* cnt,
                                               int32_t* num, int32_t* range_flag) {
    if (num_seeds < 0 || num_nodes < 0 || num_walks < 1 || num_steps < 1 || top_k < 1)
        return pglamd::fail(PGLAMD_E_ARG, "walk_visit_topk_host: num_seeds / num_nodes must be >= 0 and num_walks / num_steps / top_k >= 1");
    if (num_seeds > 0 && (!indptr || !col || !seeds || !nbr || !cnt || !num))
        return pglamd::fail(PGLAMD_E_ARG, "walk_visit_topk_host: NULL pointer");
    if (num_walks > PGLAMD_VISIT_MAX || num_steps > PGLAMD_VISIT_MAX || num_walks * num_steps > PGLAMD_VISIT_MAX)
        return pglamd::fail(PGLAMD_E_RANGE, "walk_visit_topk_host: num_walks * num_steps = %lld x %lld exceeds PGLAMD_VISIT_MAX = %d",
                            (long long)num_walks, (long long)num_steps, PGLAMD_VISIT_MAX);
    if (top_k > PGLAMD_VISIT_MAX_TOPK)
        return pglamd::fail(PGLAMD_E_RANGE, "walk_visit_topk_host: top_k %lld exceeds PGLAMD_VISIT_MAX_TOPK = %d", (long long)top_k,
                            PGLAMD_VISIT_MAX_TOPK);
    if (num_nodes > INT32_MAX || num_seeds > INT32_MAX)
        return pglamd::fail(PGLAMD_E_RANGE, "walk_visit_topk_host: num_nodes / num_seeds out of range");
    std::atomic<int32_t> flag{0};
    int64_t nt = threads > 0 ? threads : (int64_t)std::thread::hardware_concurrency();
    nt = std::max<int64_t>(1, std::min<int64_t>({nt, 16, (num_seeds * num_walks + 1023) / 1024, num_seeds}));
    if (nt == 1) {
        visit_range(indptr, col, cum, num_nodes, seeds, 0, num_seeds, num_walks, num_steps, top_k, seed, nbr, cnt, num, &flag);
    } else {
        std::vector<std::thread> pool;
        const int64_t per = (num_seeds + nt - 1) / nt;
        for (int64_t i = 0; i < nt; ++i) {
            const int64_t s0 = i * per, s1 = std::min(num_seeds, s0 + per);
            if (s0 < s1) pool.emplace_back(visit_range, indptr, col, cum, num_nodes, seeds, s0, s1, num_walks, num_steps, top_k, seed,
                                           nbr, cnt, num, &flag);
        }
        for (auto& th : pool) th.join();
    }
    if (range_flag && flag.load()) *range_flag |= flag.load();
    return PGLAMD_OK;
}

// Host twin of pglamd_edge_weight_table: the same quantisation (one fp64 division, one exact multiply, floor) and the same
// integer prefix sums, row by row.
namespace {
template <typename T>
int32_t weight_table_rows(const int64_t* indptr, const int32_t* eid, const T* weight, int64_t num_nodes, int64_t num_weights,
                          int64_t* cum, int64_t* npos) {
    int32_t flag = 0;
    for (int64_t v = 0; v < num_nodes; ++v) {
        const int64_t b = indptr[v], e = indptr[v + 1];
        double m = 0.0;
        for (int64_t j = b; j < e; ++j) {
            const int64_t k = eid ? (int64_t)eid[j] : j;
            if (k < 0 || k >= num_weights) { flag |= PGLAMD_WEIGHT_BAD_EID; continue; }
            const int32_t f = pglamd::walk::weight_flag((double)weight[k]);
            flag |= f;
            if (!f && (double)weight[k] > m) m = (double)weight[k];
        }
        int64_t run = 0, pos = 0;
        for (int64_t j = b; j < e; ++j) {
            const int64_t k = eid ? (int64_t)eid[j] : j;
            const bool ok = k >= 0 && k < num_weights && !pglamd::walk::weight_flag((double)weight[k]);
            const uint64_t q = ok ? pglamd::walk::quantise_weight((double)weight[k], m) : 0;
            run += (int64_t)q; pos += q > 0;
            cum[j] = run;
        }
        npos[v] = pos;
    }
    return flag;
}
}  // namespace

extern "C" int32_t pglamd_edge_weight_table_host(const int64_t* indptr, const int32_t* eid, const void* weight, int32_t weight_f64,
                                                 int64_t num_nodes, int64_t num_edges, int64_t num_weights, int64_t* cum,
                                                 int64_t* npos, int32_t* flag) {
    if (num_nodes < 0 || num_edges < 0 || num_weights < 0 || !indptr || !flag || (num_nodes > 0 && !npos) ||
        (num_edges > 0 && (!weight || !cum)))
        return pglamd::fail(PGLAMD_E_ARG, "edge_weight_table_host: bad argument");
    if (num_edges > INT32_MAX) return pglamd::fail(PGLAMD_E_RANGE, "edge_weight_table_host: %lld edges", (long long)num_edges);
    if (indptr[0] != 0 || indptr[num_nodes] != num_edges) return pglamd::fail(PGLAMD_E_ARG, "edge_weight_table_host: indptr does not span [0, num_edges]");
    for (int64_t v = 0; v < num_nodes; ++v)
        if (indptr[v] > indptr[v + 1]) return pglamd::fail(PGLAMD_E_ARG, "edge_weight_table_host: indptr decreases at row %lld", (long long)v);
    *flag = weight_f64 ? weight_table_rows(indptr, eid, static_cast<const double*>(weight), num_nodes, num_weights, cum, npos)
                       : weight_table_rows(indptr, eid, static_cast<const float*>(weight), num_nodes, num_weights, cum, npos);
    return PGLAMD_OK;
}

// ------------------------------------------------------------------------------------------------
// Host twin of pglamd_sample_relations_count / _fill (sampling_rel.hip): the same count rule, the same Floyd draws under the same
// per-relation seed (sample_core.hpp), HOST pointers.  Slot r * n + i is a function of (seed, r, nodes[i]) alone and its place in
// the output comes from one serial prefix sum, so the split over threads changes nothing.
// ------------------------------------------------------------------------------------------------
namespace {
void sample_relations_range(const int64_t* indptr, const int32_t* col, const int32_t* eid, int64_t stride, const int64_t* fanouts,
                            const int64_t* nodes, int64_t n, uint64_t seed, const int64_t* offsets, int64_t s0, int64_t s1,
                            int64_t* out_nbr, int64_t* out_dst, int64_t* out_eid) {
    using namespace pglamd::sample;
    int64_t chosen[kMaxSample];
    for (int64_t idx = s0; idx < s1; ++idx) {
        const int64_t r = idx / n, i = idx - r * n, k = fanouts[r], v = nodes[i];
        const int64_t* ip = indptr + r * stride;
        const int64_t b = ip[v], deg = ip[v + 1] - b, o = offsets[idx];
        if (k == 0) continue;
        if (k < 0 || deg <= k) {
            for (int64_t j = 0; j < deg; ++j) {
                out_nbr[o + j] = col[b + j]; out_dst[o + j] = i;
                if (out_eid) out_eid[o + j] = eid[b + j];
            }
            continue;
        }
        const uint64_t rs = relation_seed(seed, r);
        for (int c = 0; c < (int)k; ++c) chosen[c] = floyd_draw(rs, v, deg, k, c, chosen);
        for (int q = 0; q < (int)k; ++q) {
            out_nbr[o + q] = col[b + chosen[q]]; out_dst[o + q] = i;
            if (out_eid) out_eid[o + q] = eid[b + chosen[q]];
        }
    }
}
}  // namespace

extern "C" int32_t pglamd_sample_relations_host(const int64_t* indptr, const int32_t* col, const int32_t* eid, int64_t num_nodes,
                                                int32_t num_relations, const int64_t* fanouts, const int64_t* nodes, int64_t n,
                                                uint64_t seed, int32_t threads, int64_t* count, int64_t* edge_split,
                                                int64_t* out_neighbors, int64_t* out_dst, int64_t* out_eids, int64_t num_out) {
    using namespace pglamd::sample;
    if (n < 0 || num_nodes < 0 || num_out < 0 || !fanouts || !edge_split || (n > 0 && (!indptr || !nodes || !count)) || (out_eids && !eid))
        return pglamd::fail(PGLAMD_E_ARG, "sample_relations_host: bad argument");
    if (num_relations < 1 || num_relations > kMaxRelations)
        return pglamd::fail(PGLAMD_E_SHAPE, "sample_relations_host: num_relations %d outside [1, %d]", (int)num_relations, kMaxRelations);
    if (num_nodes > INT32_MAX || n > ((int64_t)1 << 40)) return pglamd::fail(PGLAMD_E_RANGE, "sample_relations_host: num_nodes / n out of range");
    for (int32_t r = 0; r < num_relations; ++r)
        if (fanouts[r] > kMaxSample)
            return pglamd::fail(PGLAMD_E_SHAPE, "sample_relations_host: fan-out %lld of relation %d > %d", (long long)fanouts[r], (int)r, kMaxSample);
    for (int64_t i = 0; i < n; ++i)                             // every id is checked before it indexes anything
        if (nodes[i] < 0 || nodes[i] >= num_nodes)
            return pglamd::fail(PGLAMD_E_SHAPE, "sample_relations_host: node id %lld out of [0,%lld)", (long long)nodes[i], (long long)num_nodes);
    const int64_t total = n * num_relations, stride = num_nodes + 1;
    std::vector<int64_t> offsets((size_t)total + 1, 0);
    for (int64_t idx = 0; idx < total; ++idx) {
        const int64_t r = idx / n, k = fanouts[r], v = nodes[idx - r * n];
        const int64_t* ip = indptr + r * stride;
        count[idx] = k == 0 ? 0 : sample_count(ip[v + 1] - ip[v], k);
        offsets[idx + 1] = offsets[idx] + count[idx];
    }
    for (int32_t r = 0; r <= num_relations; ++r) edge_split[r] = offsets[(size_t)r * n];
    if (!out_neighbors) return PGLAMD_OK;                       // the counting pass: the caller sizes the outputs from edge_split
    if (!out_dst || num_out != offsets[total])
        return pglamd::fail(PGLAMD_E_ARG, "sample_relations_host: outputs of %lld entries for %lld samples", (long long)num_out, (long long)offsets[total]);
    int64_t nt = threads > 0 ? threads : (int64_t)std::thread::hardware_concurrency();
    nt = std::max<int64_t>(1, std::min<int64_t>({nt, 16, (total + 1023) / 1024}));
    if (nt == 1) {
        sample_relations_range(indptr, col, eid, stride, fanouts, nodes, n, seed, offsets.data(), 0, total, out_neighbors, out_dst, out_eids);
        return PGLAMD_OK;
    }
    std::vector<std::thread> pool;
    const int64_t per = (total + nt - 1) / nt;
    for (int64_t t = 0; t < nt; ++t) {
        const int64_t s0 = t * per, s1 = std::min(total, s0 + per);
        if (s0 < s1) pool.emplace_back(sample_relations_range, indptr, col, eid, stride, fanouts, nodes, n, seed, offsets.data(), s0, s1,
                                       out_neighbors, out_dst, out_eids);
    }
    for (auto& th : pool) th.join();
    return PGLAMD_OK;
}

// ------------------------------------------------------------------------------------------------
// Host twins of pool.hip: the per-segment top-k permutation (pgl/math.py:276-364) and the edge filter
// (pgl/utils/transform.py:138-168), one thread; the same definitions (tests/pool_defs.py), the same bits.
// ------------------------------------------------------------------------------------------------
extern "C" int32_t pglamd_segment_topk_host(const float* scores, const int64_t* seg_ptr, const int64_t* out_ptr, int64_t num_segments,
                                            int64_t* perm, int64_t* status) {
    namespace P = pglamd::pool;
    if (num_segments < 0 || !status || (num_segments > 0 && (!seg_ptr || !out_ptr)))
        return pglamd::fail(PGLAMD_E_ARG, "segment_topk_host: num_segments must be >= 0 and seg_ptr / out_ptr / status not NULL");
    std::vector<uint64_t> a;
    for (int64_t s = 0; s < num_segments; ++s) {
        const int64_t b = seg_ptr[s], o = out_ptr[s], len = seg_ptr[s + 1] - b, k = out_ptr[s + 1] - o;
        if (len < 0 || len > PGLAMD_TOPK_MAX_SEG) { *status |= P::kFlagSegment; continue; }       // skipped, as on the device
        if (k < 0 || k > len) { *status |= P::kFlagK; continue; }
        if (k == 0) continue;
        a.resize((size_t)len);
        for (int64_t i = 0; i < len; ++i) {
            uint32_t bits;
            std::memcpy(&bits, scores + b + i, 4);
            a[(size_t)i] = P::sort_word(bits, (uint32_t)i);
        }
        std::partial_sort(a.begin(), a.begin() + k, a.end());
        for (int64_t j = 0; j < k; ++j) perm[o + j] = b + (int64_t)(a[(size_t)j] & 0xFFFFFFFFull);
    }
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_filter_edges_host(const int64_t* edges, int64_t edge_stride, int64_t num_edges, const int64_t* perm, int64_t m,
                                            int64_t num_nodes, int64_t* out_edges, int64_t* out_pos, int64_t* status) {
    namespace P = pglamd::pool;
    if (num_edges < 0 || m < 0 || num_nodes < 0 || edge_stride < 2 || !status || (num_edges > 0 && !edges) || (m > 0 && !perm))
        return pglamd::fail(PGLAMD_E_ARG, "filter_edges_host: bad argument (sizes >= 0, edge_stride >= 2, pointers not NULL)");
    if (num_nodes > INT32_MAX || m > INT32_MAX) return pglamd::fail(PGLAMD_E_RANGE, "filter_edges_host: num_nodes / m beyond the int32 engine range");
    status[0] = status[1] = 0;
    std::vector<int32_t> new_id((size_t)num_nodes, -1);
    for (int64_t i = 0; i < m; ++i) {                           // every id is checked before it indexes anything
        const int64_t v = perm[i];
        if (v < 0 || v >= num_nodes) status[1] |= P::kFlagRange;
        else if (new_id[(size_t)v] != -1) status[1] |= P::kFlagRepeat;
        else new_id[(size_t)v] = (int32_t)i;
    }
    int64_t o = 0;
    for (int64_t e = 0; e < num_edges; ++e) {
        const int64_t u = edges[e * edge_stride], x = edges[e * edge_stride + 1];
        if (u < 0 || u >= num_nodes || x < 0 || x >= num_nodes) { status[1] |= P::kFlagRange; continue; }
        const int32_t a = new_id[(size_t)u], b = new_id[(size_t)x];
        if (a < 0 || b < 0) continue;
        if (out_edges && out_pos) { out_edges[2 * o] = a; out_edges[2 * o + 1] = b; out_pos[o] = e; }
        ++o;
    }
    status[0] = o;
    return PGLAMD_OK;
}
