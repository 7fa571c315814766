// fa_attention.hip -- FAGCN's frequency-adaptive attention over a graph (FAConv, pgl/nn/conv.py:1287-1341), forward AND backward,
// without ever materialising the [E,H] gate in the forward.  With x [N,H,D], the two halves of the gate p_src, p_dst [N,H] and the
// constant node scales s_src, s_dst [N] (the layer's degree norms):
//     t_e,h      = tanh(p_src[u,h] + p_dst[v,h])                      e = (u -> v)
//     w_e,h      = t_e,h * s_src[u] * s_dst[v]
//     out[v,h,:] = sum_{e into v} keep_e,h w_e,h x[u,h,:]
// The reference's chain (two send_uv, a tanh, a product, a dropout, a send_ue_recv) writes and re-reads [E,1] tensors five times and
// its backward goes through the generic edge-operand gradient.  The gate is signed and has NO softmax: no row statistics, no online
// maximum, no rescaling -- the walk is the flat aggregation plus two gathered scalars per edge.
//
// FORWARD (fa_flat_kernel<VEC, 0>): the walk of gv2_flat_kernel (gatv2_attention.hip) -- a wave per chunk of the dst-sorted stream,
//   scalar index loads, lanes across the H*D columns (VEC floats of one head per lane), several edges in flight -- behind a GATE PASS
//   in which the wave's lanes take one (edge, head) pair each and leave the gates in LDS (see the kernel), so that the walk gathers
//   nothing but x[u].  The scale of the ROW node multiplies the finished sum once (out[v] = s_dst[v] * sum keep t s_src[u] x[u]), the
//   scale of the gathered node every gate.
// BACKWARD (fa_flat_kernel<VEC, 1>), SRC-sorted stream: row = u carries x[u], p_src[u,.], s_src[u]; gathers g[v], p_dst[v,.], s_dst[v].
//   With c_e = keep_e <g[v,h,:], x[u,h,:]> (group_sum over the head's lanes) and r_e = c_e s_src[u] s_dst[v] (1 - t_e^2):
//             d x[u,h,:]   = sum_{e out of u} keep_e w_e g[v,h,:]
//             d p_src[u,h] = sum_{e out of u} r_e
//             r_edge[e,h]  = r_e, stored edge by edge in THIS stream's order (optional): d p_dst[v,h] = sum_{e into v} r_e is the
//                            caller's sum of that buffer by destination (ops.fa_backward: the aggregation over an edge_rows view)
// tanh is the device library's tanhf everywhere (no fast approximation, no exp formula: 1 - t^2 needs t's relative accuracy near 0).
// Attention dropout: drop_factor(seed, original edge id, head), the function and the mask of the GAT kernels.
// Rows longer than a chunk leave partials (one float per column forward; the column and the head's d p_src backward) that
// fa_fixup_kernel adds in chunk order through the lists of split_rows.hpp: plain fp32 sums in a fixed order, no atomic.
#include "attention_common.hpp"

#include <algorithm>
#include <initializer_list>

namespace pglamd {

struct FaParams {
    const float* row_x;             // MODE 1: x[u], the row node's vector
    const float* col_x;             // gathered by col: x[u] (MODE 0) / g[v] (MODE 1)
    const float* row_p;             // [N,H] gate half of the row node: p_dst (MODE 0) / p_src (MODE 1)
    const float* col_p;             // [N,H] gate half gathered by col
    const float* row_s;             // [N] scale of the row node, NULL: 1
    const float* col_s;             // [N] scale gathered by col, NULL: 1
    float* out;                     // out (MODE 0) / d x (MODE 1; NULL: not stored)
    float* dp_row;                  // MODE 1: d p_src [N,H] (NULL: neither it nor r_edge is formed)
    float* r_edge;                  // MODE 1: [E,H] r_e at the edge's position in this stream (NULL: not stored)
    const int* row; const int* col; const int* eid; const int64_t* indptr;
    float* part_head; float* part_tail;         // [n_chunks, PW, d]
    int* long_count; int* long_list; int* long_list2;
    int64_t out_rows, n_csr_rows;
    int E, n_chunks, chunk, n_blocks, n_grid_chunks;
    int d, H, D;
    float drop_p, drop_scale;
    unsigned seed;
};

// floats per column a chunk parks for a split row: the sum (forward); the sum and the head's d p_src (backward)
constexpr int fa_partial_width(int mode) { return mode == 0 ? 1 : 2; }

// Edges per batch of the walk (two batches of gathered rows are live).  The counts are gv2_edges_in_flight's without dropout (the mask
// is applied in the gate pass, the walk never sees it).  Eight in the forward at VEC 2 and 4 was timed too (RMAT-20, 20 M edges,
// d = 128 / 256: 1.668 / 3.184 ms against 1.679 / 3.208 with four -- no difference, at 88 VGPRs instead of 56 for VEC 4); other counts
// have not been timed.
constexpr int fa_edges_in_flight(int vec, int mode) { return mode == 0 ? (vec == 1 ? 8 : 4) : (vec == 4 ? 2 : 4); }

// (edge, head) gates a wave stages in LDS at a time: a chunk is walked in segments of kFaGateCap / H edges (512 at H = 1: a whole
// chunk of the default sizes, which walks at most 2 * 256 - 1 edges)
constexpr int kFaGateCap = 512;

// The walk in two passes per segment.  GATE PASS: lane l takes the segment's (edge, head) pairs l, l + 64, ...: it loads the edge's
// two nodes, gathers p_src, p_dst and the gathered node's scale, takes ONE tanhf per pair and leaves in the wave's own LDS slice
//     w = keep * (t * s_col)               and, backward,     q = (keep * s_col) * (1 - t * t)
// -- 64 gates per pass of the tanhf sequence instead of one (every lane of a head would compute the same value), and two scalar
// gathers per 64 pairs instead of per edge.  ROW PASS: the walk of gv2_flat_kernel over the same edges, which gathers only the rows
// and reads w (and q) back by (edge, head): one broadcast LDS read per edge at H = 1.
template <int VEC, int MODE, bool DROP>
__global__ __launch_bounds__(kBlock) void fa_flat_kernel(FaParams p) {
    constexpr int U = fa_edges_in_flight(VEC, MODE);
    constexpr int PW = fa_partial_width(MODE);
    using V = FV<VEC>;
    __shared__ float gate_w[kWavesPerBlock][kFaGateCap];
    __shared__ float gate_q[MODE == 1 ? kWavesPerBlock : 1][MODE == 1 ? kFaGateCap : 1];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform(threadIdx.x >> 6);
    const int j0 = lane * VEC;
    const bool act = j0 < p.d;
    const int head = act ? j0 / p.D : 0;
    const int lph = p.D / VEC;                          // lanes per head: a power of two
    const bool head_lane = act && (j0 % p.D) == 0;
    const bool want_dx = MODE == 0 || p.out != nullptr;
    const bool want_dp = MODE == 1 && p.dp_row != nullptr;

    if ((int)blockIdx.x >= p.n_grid_chunks) {
        zero_fill_role(p, lane, wib, [&](int64_t r) {
            if (act && want_dx) *reinterpret_cast<V*>(p.out + r * p.d + j0) = V{};
            if (want_dp && lane < p.H) p.dp_row[r * p.H + lane] = 0.f;
        });
        return;
    }
    const int64_t lb = xcd_swizzle(blockIdx.x, p.n_blocks);
    if (lb < 0) return;
    const int c = wave_uniform((int)lb * kWavesPerBlock + wib);
    if (c >= p.n_chunks) return;
    const cptr<int> rowp = as_const(p.row);
    const cptr<int> colp = as_const(p.col);
    const int e0 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk, p.chunk, p.E);
    const int e1 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk + p.chunk, p.chunk, p.E);
    if (e0 >= e1) return;
    const float* __restrict__ rx = p.row_x;
    const float* __restrict__ cx = p.col_x;
    const float* __restrict__ rp = p.row_p;
    const float* __restrict__ cp = p.col_p;
    const float* __restrict__ rs = p.row_s;
    const float* __restrict__ cs = p.col_s;
    float* gw = gate_w[wib];
    float* gq = gate_q[MODE == 1 ? wib : 0];

    float acc[VEC], dp = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

    int cur = rowp[e0];
    bool head_open = e0 > 0 && rowp[e0 - 1] == cur;

    auto store_partial = [&](bool headp) {
        if (act) {
            float* dst = (headp ? p.part_head : p.part_tail) + (int64_t)c * PW * p.d;
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
            *reinterpret_cast<V*>(dst + j0) = o;
            if constexpr (MODE == 1) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = dp;
                *reinterpret_cast<V*>(dst + p.d + j0) = o;
            }
        }
        if (!headp && lane == 0) p.long_list[atomicAdd(p.long_count, 1)] = c;
    };
    // what belongs to the ROW node is fetched at the row change and held in registers until the next one
    V x_held{}; float s_held = 1.f;
    auto open_row = [&](int r) {
        if (rs) s_held = rs[r];
        if constexpr (MODE == 1) {
            if (act) x_held = *reinterpret_cast<const V*>(rx + (int64_t)r * p.d + j0);
        }
    };
    auto store_final = [&](int r) {
        if (r >= p.out_rows || !act) return;
        if (want_dx) {
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = acc[k] * s_held;
            *reinterpret_cast<V*>(p.out + (int64_t)r * p.d + j0) = o;
        }
        if (want_dp && head_lane) p.dp_row[(int64_t)r * p.H + head] = dp * s_held;
    };
    open_row(cur);
    const int seg_edges = kFaGateCap / p.H;             // (H <= 64: at least 8 edges)
    for (int sb = e0; sb < e1; sb += seg_edges) {
        const int se = min(sb + seg_edges, e1);
        // GATE PASS over the pairs of [sb, se): entry i = (edge sb + i / H, head i % H), i < (se - sb) * H <= kFaGateCap
        const int n_ent = (se - sb) * p.H;
        for (int i = lane; i < n_ent; i += kWave) {
            const int ee = sb + (p.H == 1 ? i : i / p.H), hh = p.H == 1 ? 0 : i % p.H;
            const int cc = p.col[ee], rr = p.row[ee];
            const float sc = cs ? cs[cc] : 1.f;
            const float t = tanhf(cp[(int64_t)cc * p.H + hh] + rp[(int64_t)rr * p.H + hh]);
            const float df = DROP ? drop_factor(p.seed, p.eid[ee], hh, p.drop_p, p.drop_scale) : 1.f;
            gw[i] = df * (t * sc);                      // (the row node's scale multiplies the finished sum)
            if constexpr (MODE == 1) gq[i] = (df * sc) * (1.f - t * t);
        }
        // the slice is this wave's own: its LDS operations complete in order, the fence keeps the compiler from moving the reads up
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        auto consume = [&](int r, int pos, const V& xv) {
            if (r != cur) {
                if (head_open) store_partial(true); else store_final(cur);
                head_open = false;
                cur = r;
                dp = 0.f;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
                open_row(r);
            }
            const int gi = (pos - sb) * p.H + head;
            const float w = gw[gi];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] += w * xv.v[k];
            if constexpr (MODE == 1) {
                if (want_dp) {
                    float dt = 0.f;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) dt += xv.v[k] * x_held.v[k];
                    dt = group_sum(dt, lph);            // <g[v,h,:], x[u,h,:]>
                    const float rr = dt * gq[gi];
                    dp += rr;
                    if (p.r_edge && head_lane) p.r_edge[(int64_t)pos * p.H + head] = rr * s_held;
                }
            }
        };
        auto load_idx = [&](int e, int (&cc)[U], int (&rr)[U]) {
#pragma unroll
            for (int i = 0; i < U; ++i) { rr[i] = rowp[e + i]; cc[i] = colp[e + i]; }
        };
        auto load_rows = [&](const int (&cc)[U], V (&vx)[U]) {
            if (!act) return;
#pragma unroll
            for (int i = 0; i < U; ++i) vx[i] = *reinterpret_cast<const V*>(cx + (int64_t)cc[i] * p.d + j0);
        };
        // three stages deep, as the GAT walks: rows of batch g consumed, rows of g+1 in flight, (scalar) indices of g+2 being fetched
        int e = sb;
        const int n_full = (se - sb) / U;
        int cA[U], rA[U]; V xA[U] = {};
        int cB[U], rB[U];
        if (n_full > 0) { load_idx(e, cA, rA); load_rows(cA, xA); }
        if (n_full > 1) load_idx(e + U, cB, rB);
        for (int g = 0; g < n_full; ++g) {
            int cC[U], rC[U]; V xB[U] = {};
            const bool more = g + 1 < n_full, more2 = g + 2 < n_full;
            if (more) load_rows(cB, xB);
            if (more2) load_idx(e + 2 * U, cC, rC);
#pragma unroll
            for (int i = 0; i < U; ++i) consume(rA[i], e + i, xA[i]);
            if (more) {
#pragma unroll
                for (int i = 0; i < U; ++i) { rA[i] = rB[i]; xA[i] = xB[i]; }
            }
            if (more2) {
#pragma unroll
                for (int i = 0; i < U; ++i) { cB[i] = cC[i]; rB[i] = rC[i]; }
            }
            e += U;
        }
        for (; e < se; ++e) {
            const int r = rowp[e], cc = colp[e];
            V xv{};
            if (act) xv = *reinterpret_cast<const V*>(cx + (int64_t)cc * p.d + j0);
            consume(r, e, xv);
        }
        // (the next segment's gate pass overwrites the slice: not before this segment's reads)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    const bool tail_open = e1 < p.E && rowp[e1] == cur;
    if (head_open) store_partial(true);
    else if (tail_open) store_partial(false);
    else store_final(cur);
}

// adds the partials of the rows longer than a chunk, from the work list the flat kernel filled: the two passes and lists of
// gv2_fixup_kernel (split_rows.hpp) with plain fp32 sums.  Order: the tail partial of the row's first chunk, then the head partials
// in chunk order (short rows); hub rows: wave w of the block adds the chunks a + 1 + w, a + 1 + w + kFixWaves, ... and wave 0 then adds
// the tail partial and the wave sums in wave order.  PW 2: the second slice holds the head's d p_src, replicated over its columns.
template <int VEC, bool LONG, int PW>
__global__ __launch_bounds__(LONG ? kFixWaves * kWave : kBlock) void fa_fixup_kernel(FaParams p) {
    using V = FV<VEC>;
    constexpr int NW = LONG ? kFixWaves : 1;
    __shared__ float red_v[LONG ? kFixWaves : 1][LONG ? kWave * VEC : 1];
    __shared__ float red_p[LONG ? kFixWaves : 1][LONG ? kWave : 1];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform(threadIdx.x >> 6);
    const cptr<int> rowp = as_const(p.row);
    const cptr<int64_t> ip = as_const(p.indptr);
    const int j0 = lane * VEC;
    const bool act = j0 < p.d;
    const int* list = LONG ? p.long_list2 : p.long_list;
    const int n_tasks = LONG ? p.long_count[1] : p.long_count[0];
    const int first = LONG ? (int)blockIdx.x : (int)blockIdx.x * kWavesPerBlock + wib;
    const int stride = LONG ? (int)gridDim.x : (int)gridDim.x * kWavesPerBlock;
    for (int t_id = first; t_id < n_tasks; t_id += stride) {
        const int a = wave_uniform(list[t_id]);
        const int e1 = (a + 1) * p.chunk;
        const int r = rowp[e1 - 1];
        const int64_t re = ip[r + 1];
        const int b = chunk_of_edge(re - 1, p.chunk);           // last chunk holding a piece of row r
        if constexpr (!LONG) {
            if (fixup_is_long(a, b)) {                  // hub row: defer to the block-parallel pass
                if (lane == 0) p.long_list2[atomicAdd(p.long_count + 1, 1)] = a;
                continue;
            }
        }
        float acc[VEC], dp = 0.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        auto merge = [&](const float* base) {
            const V v0 = *reinterpret_cast<const V*>(base + j0);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] += v0.v[k];
            if constexpr (PW == 2) dp += base[p.d + j0];
        };
        if constexpr (!LONG) {
            if (act) {
                merge(p.part_tail + (int64_t)a * PW * p.d);
#pragma unroll 4
                for (int c = a + 1; c <= b; ++c) merge(p.part_head + (int64_t)c * PW * p.d);
            }
        } else {
            if (act)
                for (int c = a + 1 + wib; c <= b; c += NW) merge(p.part_head + (int64_t)c * PW * p.d);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < VEC; ++k) red_v[wib][lane * VEC + k] = acc[k];
            red_p[wib][lane] = dp;
            __syncthreads();
            if (wib != 0) continue;
            // wave 0: tail partial of chunk a first, then the wave sums in wave order (a wave without a partial adds its zeros)
            dp = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
            if (act) {
                merge(p.part_tail + (int64_t)a * PW * p.d);
                for (int w = 0; w < NW; ++w) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[k] += red_v[w][lane * VEC + k];
                    dp += red_p[w][lane];
                }
            }
        }
        if (!act || r >= p.out_rows) continue;
        const float s = p.row_s ? p.row_s[r] : 1.f;
        if (p.out) {
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = acc[k] * s;
            *reinterpret_cast<V*>(p.out + (int64_t)r * p.d + j0) = o;
        }
        if (PW == 2 && p.dp_row && (j0 % p.D) == 0) p.dp_row[(int64_t)r * p.H + j0 / p.D] = dp * s;
    }
}

// Host side.

static void fa_set_geometry(FaParams& p, int64_t heads, int64_t head_dim, float drop_p, uint32_t seed, int64_t num_edges, int64_t num_nodes) {
    p.H = (int)heads; p.D = (int)head_dim; p.d = (int)(heads * head_dim);
    p.drop_p = drop_p; p.drop_scale = 1.f / (1.f - drop_p); p.seed = seed;
    p.E = (int)num_edges; p.chunk = chunk_edges_for(num_edges); p.n_chunks = (int)ceil_div(num_edges, p.chunk);
    p.out_rows = num_nodes; p.n_csr_rows = num_nodes;
}

template <int VEC, int PW>
static int32_t launch_fa_fixups(const FaParams& p, hipStream_t st) {
    hipLaunchKernelGGL((fa_fixup_kernel<VEC, false, PW>), dim3(fixup_grid_short(p.n_chunks, kFixGridShort, kWavesPerBlock)), dim3(kBlock), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((fa_fixup_kernel<VEC, true, PW>), dim3(fixup_grid_long(p.n_chunks)), dim3(kFixWaves * kWave), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

template <int MODE>
static int32_t launch_fa(int vec, FaParams p, void* workspace, hipStream_t st) {
    SplitWs(p.n_chunks, (int64_t)fa_partial_width(MODE) * p.d, sizeof(float)).carve(p, workspace);
    return with_vec(vec, [&](auto v) {
        constexpr int VEC = decltype(v)::value;
        return launch_chunked_rows(p, st, [&](dim3 grid, const FaParams& q) {
            if (q.drop_p > 0.f) hipLaunchKernelGGL((fa_flat_kernel<VEC, MODE, true>), grid, dim3(kBlock), 0, st, q);
            else hipLaunchKernelGGL((fa_flat_kernel<VEC, MODE, false>), grid, dim3(kBlock), 0, st, q);
        }, [&](const FaParams& q) { return launch_fa_fixups<VEC, fa_partial_width(MODE)>(q, st); });
    });
}

static const void* fa_ptr_or(std::initializer_list<const void*> ps) {
    uintptr_t a = 0;
    for (const void* q : ps) a |= reinterpret_cast<uintptr_t>(q);
    return reinterpret_cast<const void*>(a);
}

static int64_t fa_chunks(int64_t num_edges) { return num_edges > 0 ? ceil_div(num_edges, chunk_edges_for(num_edges)) : 0; }

}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_fa_aggregate_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim) {
    if (num_edges <= 0 || heads <= 0 || head_dim <= 0) return 256;
    return SplitWs(fa_chunks(num_edges), fa_partial_width(0) * heads * head_dim, sizeof(float)).bytes() + 256;
}

extern "C" int32_t pglamd_fa_aggregate(const float* x, const float* p_src, const float* p_dst, const float* s_src, const float* s_dst,
                                       int64_t heads, int64_t head_dim, float drop_p, uint32_t seed, const int32_t* row, const int32_t* col,
                                       const int32_t* eid, const int64_t* indptr, int64_t num_edges, int64_t num_nodes, float* out,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!out || !indptr || heads <= 0 || head_dim <= 0 || num_nodes < 0 || (num_edges > 0 && (!x || !p_src || !p_dst || !row || !col)))
        return fail(PGLAMD_E_ARG, "fa_aggregate: bad argument");
    if (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && num_edges > 0 && !eid)) return fail(PGLAMD_E_ARG, "fa_aggregate: dropout needs 0 <= p < 1 and eid");
    if (num_edges < 0 || num_edges > kMaxEdges || num_nodes >= INT32_MAX) return fail(PGLAMD_E_RANGE, "fa_aggregate: sizes beyond int32 engine range");
    const int64_t d = heads * head_dim;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_nodes == 0) return PGLAMD_OK;
    if (num_edges == 0) {
        PGLAMD_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)num_nodes * d * sizeof(float), st));
        return PGLAMD_OK;
    }
    const int vec = gat_vec(heads, head_dim, x, out, workspace, true);
    if (vec == 0 || heads > kWave)
        return fail(PGLAMD_E_SHAPE, "fa_aggregate: heads*head_dim = %lld needs one 64-lane tile, head_dim/VEC a power of two and operands aligned to their lanes",
                    (long long)d);
    if (!workspace || workspace_bytes < pglamd_fa_aggregate_workspace_bytes(num_edges, heads, head_dim))
        return fail(PGLAMD_E_WORKSPACE, "fa_aggregate: workspace too small");
    FaParams p{};
    fa_set_geometry(p, heads, head_dim, drop_p, seed, num_edges, num_nodes);
    p.col_x = x; p.col_p = p_src; p.row_p = p_dst; p.col_s = s_src; p.row_s = s_dst; p.out = out;
    p.row = row; p.col = col; p.eid = eid; p.indptr = indptr;
    return launch_fa<0>(vec, p, workspace, st);
}

extern "C" size_t pglamd_fa_backward_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim) {
    if (num_edges <= 0 || heads <= 0 || head_dim <= 0) return 256;
    return SplitWs(fa_chunks(num_edges), fa_partial_width(1) * heads * head_dim, sizeof(float)).bytes() + 256;
}

extern "C" int32_t pglamd_fa_backward(const float* grad_out, const float* x, const float* p_src, const float* p_dst, const float* s_src,
                                      const float* s_dst, int64_t heads, int64_t head_dim, float drop_p, uint32_t seed,
                                      const int32_t* src_row, const int32_t* src_col, const int32_t* src_eid, const int64_t* src_indptr,
                                      int64_t num_edges, int64_t num_nodes, float* grad_x, float* grad_p_src, float* grad_edge,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (heads <= 0 || head_dim <= 0 || num_nodes < 0 || num_edges < 0 || (!grad_x && !grad_p_src) || (grad_edge && !grad_p_src) ||
        (num_edges > 0 && (!grad_out || !x || !p_src || !p_dst || !src_row || !src_col || !src_indptr)))
        return fail(PGLAMD_E_ARG, "fa_backward: bad argument");
    if (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && num_edges > 0 && !src_eid))
        return fail(PGLAMD_E_ARG, "fa_backward: dropout needs 0 <= p < 1 and eid");
    if (num_edges > kMaxEdges || num_nodes >= INT32_MAX) return fail(PGLAMD_E_RANGE, "fa_backward: sizes beyond int32 engine range");
    const int64_t d = heads * head_dim;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_nodes == 0) return PGLAMD_OK;
    if (num_edges == 0) {
        if (grad_x) PGLAMD_HIP_CHECK(hipMemsetAsync(grad_x, 0, (size_t)num_nodes * d * sizeof(float), st));
        if (grad_p_src) PGLAMD_HIP_CHECK(hipMemsetAsync(grad_p_src, 0, (size_t)num_nodes * heads * sizeof(float), st));
        return PGLAMD_OK;
    }
    const int vec = gat_vec(heads, head_dim, fa_ptr_or({grad_out, x}), grad_x, workspace, true);
    if (vec == 0 || heads > kWave)
        return fail(PGLAMD_E_SHAPE, "fa_backward: heads*head_dim = %lld needs one 64-lane tile, head_dim/VEC a power of two and operands aligned to their lanes",
                    (long long)d);
    if (!workspace || workspace_bytes < pglamd_fa_backward_workspace_bytes(num_edges, heads, head_dim))
        return fail(PGLAMD_E_WORKSPACE, "fa_backward: workspace too small");
    FaParams p{};
    fa_set_geometry(p, heads, head_dim, drop_p, seed, num_edges, num_nodes);
    p.row_x = x; p.col_x = grad_out; p.row_p = p_src; p.col_p = p_dst; p.row_s = s_src; p.col_s = s_dst;
    p.out = grad_x; p.dp_row = grad_p_src; p.r_edge = grad_edge;
    p.row = src_row; p.col = src_col; p.eid = src_eid; p.indptr = src_indptr;
    return launch_fa<1>(vec, p, workspace, st);
}
