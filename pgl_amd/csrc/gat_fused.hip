// gat_fused.hip -- the whole attention aggregation of GATConv (pgl/nn/conv.py:331-339), forward AND
// backward, without ever materialising an [E,H] tensor:
//     alpha = send_uv(a_src, a_dst, "add") ; leaky_relu ; edge_softmax(by dst) ; dropout ;
//     out   = send_ue_recv(f, alpha, "mul", "sum")
// i.e.  out[v,h,:] = sum_{e=(u->v)} drop_e * softmax_v( leaky(a_src[u,h] + a_dst[v,h]) ) * f[u,h,:]
//
// The reference materialises four [E,H] tensors and makes ~14 passes over them.
//
// FORWARD (gat_flat_kernel<T, VEC, 0>): each wave walks its chunk of the dst-sorted edge stream (same
//   geometry as agg_flat_kernel: scalar index loads, lanes across the H*D columns, 8 edges in
//   flight, double buffered) carrying an ONLINE softmax state per lane (running max m, running sum
//   s, running weighted row acc -- flash-attention style rescaling).  HBM traffic = one gather of
//   f[u] (H*D*4 B) + a_src[u] (H*4 B) + 8 B of index per edge + one output row: a plain SpMM + 6 %.
//   The per-row statistics (m, s) are optionally written out ([N,H] each): they are all a backward
//   pass needs to recompute alpha_e = exp(leaky(a_src[u]+a_dst[v]) - m[v]) / s[v] on the fly.
// BACKWARD: two symmetric walks, each a plain gather pass that keeps everything it produces in registers per row
//   alpha_e   = exp(leaky(pre_e) - m[v]) / s[v],  pre_e = a_src[u] + a_dst[v]        (recomputed from the forward's statistics)
//   d pre_e   = alpha_e (drop_e <g[v], f[u]>_h - t[v,h]) * (pre_e > 0 ? 1 : slope),  t[v,h] = <g[v,h,:], out[v,h,:]>
//   MODE 2, SRC-sorted stream (row = u, gathers g[v] and the scalars of v):
//             d f[u]     = sum_{e=(u->v)} drop_e alpha_e g[v]        and        d a_src[u,h] = sum_{e=(u->v)} d pre_e
//   MODE 3, DST-sorted stream (row = v, gathers f[u] and a_src[u]):             d a_dst[v,h] = sum_{e=(u->v)} d pre_e
//   The row's own vector (f[u] resp. g[v]) rides along with every edge like the per-row scalars do (an L1 hit after the
//   row's first edge); the per-head dot product is a xor-shuffle over the lanes of a head.  No [E,H] tensor exists at
//   any point (the reference-style composition writes and re-reads four of them).
// Attention dropout is a counter-based hash of (seed, original edge id, head): forward and both
// backward kernels regenerate the same mask, nothing is stored.
// Rows longer than a chunk leave partials merged in a fixed order by gat_fixup_kernel (associative
// softmax merge, or plain sums for the backward): atomic-free, bit-reproducible.
// The kernels and launchers of the GAT family live in gat_fused.hpp, templated on the storage type of the rows: this file holds their
// fp32 entry points and the score kernels (sddmm, additive score); gat_fused_16.hip the fp16 / bf16 entry points.
#include "gat_fused.hpp"

namespace pglamd {

// SDDMM over a dst-sorted edge stream: out[eid[p], h] = < x[col[p], h, :], y[row[p], h, :] >.
// This is d loss / d (edge feature) of send_ue_recv(x, e, "mul", "sum") when e is [E,H,1]
// (x = node features gathered by source, y = the incoming gradient rows): the reference composes it
// from two [E,H,D] gathers; here neither is materialised.  Lanes span the H*D columns; the per-head dot
// product is a xor-shuffle reduction over the D/VEC lanes of a head (a power of two); lane 0 of each head writes.
// ADDLEAKY: out = sum_d w[h,d] * leaky(x[col] + y[row]) instead of the plain dot product (GATv2's score, pgl/nn/conv.py:421-424)
template <int VEC, bool ADDLEAKY = false>
__global__ __launch_bounds__(kBlock) void sddmm_kernel(GatParams p) {
    constexpr int U = 8;
    using V = FV<VEC>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform(threadIdx.x >> 6);
    const int j0 = lane * VEC;
    const bool act = j0 < p.d;
    const int lph = p.D / VEC;
    const int head = act ? j0 / p.D : 0;
    const bool writer = act && (lane % lph) == 0;
    const int64_t lb = xcd_swizzle(blockIdx.x, p.n_blocks);
    if (lb < 0) return;
    const int c = wave_uniform((int)lb * kWavesPerBlock + wib);
    if (c >= p.n_chunks) return;
    const int e0 = c * p.chunk, e1 = min(e0 + p.chunk, p.E);
    const cptr<int> rowp = as_const(p.row);
    const cptr<int> colp = as_const(p.col);
    const cptr<int> eidp = as_const(p.eid);
    int cur = -1;
    V gv{}, wv{};
    if constexpr (ADDLEAKY) { if (act) wv = *reinterpret_cast<const V*>(p.w + j0); }
    auto emit = [&](int r, int ed, const V& fx) {
        if (r != cur) { cur = r; if (act) gv = *reinterpret_cast<const V*>(p.g + (int64_t)cur * p.d + j0); }
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if constexpr (ADDLEAKY) { const float z = gv.v[k] + fx.v[k]; dot += wv.v[k] * (z > 0.f ? z : p.slope * z); }
            else dot += gv.v[k] * fx.v[k];
        }
        dot = group_sum(dot, lph);
        if (writer) p.dpre[(int64_t)ed * p.H + head] = dot;
    };
    // three stages, as in agg_flat_kernel: rows of batch g consumed, rows of g+1 in flight, scalar ids of g+2 being fetched
    auto load_idx = [&](int e, int (&rr)[U], int (&cc)[U], int (&ee)[U]) {
#pragma unroll
        for (int i = 0; i < U; ++i) { rr[i] = rowp[e + i]; cc[i] = colp[e + i]; ee[i] = eidp ? eidp[e + i] : e + i; }
    };
    auto load_rows = [&](const int (&cc)[U], V (&fx)[U]) {
#pragma unroll
        for (int i = 0; i < U; ++i)
            if (act) fx[i] = *reinterpret_cast<const V*>(p.f + (int64_t)cc[i] * p.d + j0);
    };
    int e = e0;
    const int n_full = (e1 - e0) / U;
    int rA[U], cA[U], eA[U], rB[U], cB[U], eB[U];
    V fA[U];
    if (n_full > 0) { load_idx(e, rA, cA, eA); load_rows(cA, fA); }
    if (n_full > 1) load_idx(e + U, rB, cB, eB);
    for (int g = 0; g < n_full; ++g) {
        int rC[U], cC[U], eC[U];
        V fB[U];
        const bool more = g + 1 < n_full, more2 = g + 2 < n_full;
        if (more) load_rows(cB, fB);
        if (more2) load_idx(e + 2 * U, rC, cC, eC);
#pragma unroll
        for (int i = 0; i < U; ++i) emit(rA[i], eA[i], fA[i]);
        if (more) {
#pragma unroll
            for (int i = 0; i < U; ++i) { rA[i] = rB[i]; eA[i] = eB[i]; fA[i] = fB[i]; }
        }
        if (more2) {
#pragma unroll
            for (int i = 0; i < U; ++i) { rB[i] = rC[i]; cB[i] = cC[i]; eB[i] = eC[i]; }
        }
        e += U;
    }
    for (; e < e1; ++e) {
        V fx{};
        const int cc = colp[e];
        if (act) fx = *reinterpret_cast<const V*>(p.f + (int64_t)cc * p.d + j0);
        emit(rowp[e], eidp ? eidp[e] : e, fx);
    }
}

// Backward of the additive score  s[p,h] = sum_d w[h,d] * leaky(x[col_p,h,d] + y[row_p,h,d])  w.r.t. the ROW node's operand:
//     out[r,h,d]      = sum_{p in row r} ge[gi_p,h] * w[h,d] * leaky'(x[col_p,h,d] + y[r,h,d])
//     part_w[c,h*D+d] = sum_{p in chunk c} ge[gi_p,h] * leaky(x[col_p,h,d] + y[r,h,d])            (optional: d/dw partials)
// gi_p = eid[p] (or p when eid is NULL).  Same chunk walk, partials and fix-up as the additive mode of gat_flat_kernel; the
// row node's own vector is fetched only where a row may open.  Called once per orientation of the edge list.
template <int VEC>
__global__ __launch_bounds__(kBlock) void add_score_bwd_kernel(GatParams p) {
    constexpr int U = 4;
    using V = FV<VEC>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform(threadIdx.x >> 6);
    const int j0 = lane * VEC;
    const bool act = j0 < p.d;
    const int head = act ? j0 / p.D : 0;
    if ((int)blockIdx.x >= p.n_grid_chunks) {
        zero_fill_role(p, lane, wib, [&](int64_t r) { if (act) *reinterpret_cast<V*>(p.out + r * p.d + j0) = V{}; });
        return;
    }
    const int64_t lb = xcd_swizzle(blockIdx.x, p.n_blocks);
    if (lb < 0) return;
    const int c = wave_uniform((int)lb * kWavesPerBlock + wib);
    if (c >= p.n_chunks) return;
    const cptr<int> rowp = as_const(p.row);
    const cptr<int> colp = as_const(p.col);
    const cptr<int> eidp = as_const(p.eid);
    const int e0 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk, p.chunk, p.E);
    const int e1 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk + p.chunk, p.chunk, p.E);
    V accw{};
    if (e0 < e1) {
        const float* __restrict__ x = p.x;
        const float* __restrict__ rvec = p.row_vec;
        const float* __restrict__ ge = p.ge;
        const float slope = p.slope;
        V wv{};
        if (act) wv = *reinterpret_cast<const V*>(p.w + j0);
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        int cur = rowp[e0];
        bool head_open = e0 > 0 && rowp[e0 - 1] == cur;
        V y_held{};
        if (act) y_held = *reinterpret_cast<const V*>(rvec + (int64_t)cur * p.d + j0);
        auto store_row = [&](bool partial, bool headp) {
            if (!act) return;
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
            if (partial) *reinterpret_cast<V*>((headp ? p.part_head : p.part_tail) + (int64_t)c * p.d + j0) = o;
            else if (cur < p.out_rows) *reinterpret_cast<V*>(p.out + (int64_t)cur * p.d + j0) = o;
        };
        auto consume = [&](int r, float gv, const V& xv, const V& yo) {
            if (r != cur) {
                store_row(head_open, true);
                head_open = false;
                cur = r;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
                y_held = yo;
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float z = xv.v[k] + y_held.v[k];
                acc[k] += gv * wv.v[k] * (z > 0.f ? 1.f : slope);
                accw.v[k] += gv * (z > 0.f ? z : slope * z);
            }
        };
        auto load_batch = [&](int e, int nb, int (&rr)[U], V (&vx)[U], float (&gg)[U], V (&yo)[U]) {
#pragma unroll
            for (int i = 0; i < U; ++i)
                if (i < nb) {
                    rr[i] = rowp[e + i];
                    const int cc = colp[e + i];
                    const int gi = eidp ? eidp[e + i] : e + i;
                    if (act) {
                        vx[i] = *reinterpret_cast<const V*>(x + (int64_t)cc * p.d + j0);
                        gg[i] = ge[(int64_t)gi * p.H + head];
                        if (i == 0 || rr[i] != rr[i - 1]) yo[i] = *reinterpret_cast<const V*>(rvec + (int64_t)rr[i] * p.d + j0);
                    }
                }
        };
        int rA[U]; V xA[U], yA[U]; float gA[U];
        int nA = min(U, e1 - e0);
        load_batch(e0, nA, rA, xA, gA, yA);
        for (int e = e0; e < e1; e += U) {
            int rB[U]; V xB[U], yB[U]; float gB[U];
            const int nB = max(0, min(U, e1 - (e + U)));
            if (nB > 0) load_batch(e + U, nB, rB, xB, gB, yB);
#pragma unroll
            for (int i = 0; i < U; ++i)
                if (i < nA) consume(rA[i], gA[i], xA[i], yA[i]);
#pragma unroll
            for (int i = 0; i < U; ++i) { rA[i] = rB[i]; xA[i] = xB[i]; yA[i] = yB[i]; gA[i] = gB[i]; }
            nA = nB;
        }
        const bool tail_open = e1 < p.E && rowp[e1] == cur;
        if (head_open) store_row(true, true);
        else if (tail_open) { store_row(true, false); if (lane == 0) p.long_list[atomicAdd(p.long_count, 1)] = c; }
        else store_row(false, false);
    }
    if (p.part_w && act) *reinterpret_cast<V*>(p.part_w + (int64_t)c * p.d + j0) = accw;     // every chunk writes (zeros if empty)
}

// sddmm (ADDLEAKY = false) and the additive score: one launch over plain chunks, nothing left to fix up
template <bool ADDLEAKY>
static int32_t launch_score(int vec, const float* x_by_col, const float* y_by_row, const float* w, int64_t heads, int64_t head_dim,
                            float slope, const int32_t* row, const int32_t* col, const int32_t* eid, int64_t num_edges, float* out,
                            void* stream) {
    GatParams p{};
    gat_set_geometry(p, heads, head_dim, slope, num_edges);
    p.row = row; p.col = col; p.eid = eid; p.f = x_by_col; p.g = y_by_row; p.w = w; p.dpre = out;
    const int64_t nb = ceil_div(p.n_chunks, kWavesPerBlock);
    p.n_blocks = (int)nb;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_vec(vec, [&](auto v) {
        hipLaunchKernelGGL((sddmm_kernel<decltype(v)::value, ADDLEAKY>), dim3((unsigned)xcd_grid(nb)), dim3(kBlock), 0, st, p);
        PGLAMD_LAUNCH_CHECK();
        return (int32_t)PGLAMD_OK;
    });
}

}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_gat_aggregate_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim) {
    if (num_edges <= 0) return 256;
    const int64_t n_chunks = ceil_div(num_edges, chunk_edges_for(num_edges));
    return SplitWs(n_chunks, 5 * heads * head_dim, sizeof(float)).bytes() + 256;
}

extern "C" int32_t pglamd_gat_aggregate(const float* feature, const float* attn_src, const float* attn_dst, int64_t heads,
                                        int64_t head_dim, float negative_slope, float drop_p, uint32_t seed,
                                        const int32_t* row, const int32_t* col, const int32_t* eid, const int64_t* indptr,
                                        int64_t num_edges, int64_t n_csr_rows, int64_t out_rows, float* out, float* row_max,
                                        float* row_sum, float* out_pos, float* sum_pos, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    return gat_aggregate_entry<float>(feature, attn_src, attn_dst, heads, head_dim, negative_slope, drop_p, seed, row, col, eid, indptr,
                                      num_edges, n_csr_rows, out_rows, out, row_max, row_sum, out_pos, sum_pos, workspace,
                                      workspace_bytes, stream);
}

extern "C" size_t pglamd_gat_backward_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t heads, int64_t head_dim) {
    return align_up((size_t)(num_nodes > 0 ? num_nodes : 1) * heads * sizeof(F4), 256) +
           pglamd_gat_aggregate_workspace_bytes(num_edges, heads, head_dim);
}

extern "C" int32_t pglamd_gat_backward(const float* grad_out, const float* feature, const float* attn_src,
                                       const float* attn_dst, const float* row_max, const float* row_sum, const float* out,
                                       int64_t heads, int64_t head_dim, float negative_slope, float drop_p, uint32_t seed,
                                       const int32_t* dst_row, const int32_t* dst_col, const int32_t* dst_eid,
                                       const int64_t* dst_indptr, const int32_t* src_row, const int32_t* src_col,
                                       const int32_t* src_eid, const int64_t* src_indptr, int64_t num_edges, int64_t num_nodes,
                                       float* grad_feature, float* grad_attn_src, float* grad_attn_dst, float* grad_pre,
                                       const float* out_pos, const float* sum_pos, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return gat_backward_entry<float>(grad_out, feature, attn_src, attn_dst, row_max, row_sum, out, heads, head_dim, negative_slope,
                                     drop_p, seed, dst_row, dst_col, dst_eid, dst_indptr, src_row, src_col, src_eid, src_indptr,
                                     num_edges, num_nodes, grad_feature, grad_attn_src, grad_attn_dst, grad_pre, out_pos, sum_pos,
                                     workspace, workspace_bytes, stream);
}

extern "C" int32_t pglamd_sddmm(const float* x_by_col, const float* y_by_row, int64_t heads, int64_t head_dim,
                                const int32_t* row, const int32_t* col, const int32_t* eid, int64_t num_edges, float* out,
                                void* stream) {
    if (heads <= 0 || head_dim <= 0 || num_edges < 0 || (num_edges > 0 && (!x_by_col || !y_by_row || !row || !col || !out)))
        return fail(PGLAMD_E_ARG, "sddmm: bad argument");
    if (num_edges > kMaxEdges) return fail(PGLAMD_E_RANGE, "sddmm: sizes beyond int32 engine range");
    if (num_edges == 0) return PGLAMD_OK;
    const int vec = gat_vec(heads, head_dim, x_by_col, y_by_row, nullptr, true);
    if (vec == 0 || heads > kWave)
        return fail(PGLAMD_E_SHAPE, "sddmm: heads*head_dim = %lld needs one 64-lane tile and head_dim/VEC a power of two", (long long)(heads * head_dim));
    return launch_score<false>(vec, x_by_col, y_by_row, nullptr, heads, head_dim, 0.f, row, col, eid, num_edges, out, stream);
}

extern "C" int64_t pglamd_add_score_chunks(int64_t num_edges) {
    if (num_edges <= 0) return 0;
    GatParams p{};
    gat_set_geometry(p, 1, 1, 0.f, num_edges);
    return p.n_chunks;
}

extern "C" int32_t pglamd_add_score(const float* x_by_col, const float* y_by_row, const float* w, int64_t heads, int64_t head_dim,
                                    float negative_slope, const int32_t* row, const int32_t* col, const int32_t* eid,
                                    int64_t num_edges, float* out, void* stream) {
    if (heads <= 0 || head_dim <= 0 || num_edges < 0 || (num_edges > 0 && (!x_by_col || !y_by_row || !w || !row || !col || !out)))
        return fail(PGLAMD_E_ARG, "add_score: bad argument");
    if (num_edges > kMaxEdges) return fail(PGLAMD_E_RANGE, "add_score: sizes beyond int32 engine range");
    if (num_edges == 0) return PGLAMD_OK;
    const int vec = gat_vec(heads, head_dim, x_by_col, y_by_row, w, true);
    if (vec == 0 || heads > kWave)
        return fail(PGLAMD_E_SHAPE, "add_score: heads*head_dim = %lld needs one 64-lane tile and head_dim/VEC a power of two", (long long)(heads * head_dim));
    return launch_score<true>(vec, x_by_col, y_by_row, w, heads, head_dim, negative_slope, row, col, eid, num_edges, out, stream);
}

extern "C" int32_t pglamd_add_score_backward(const float* x_by_col, const float* y_by_row, const float* w, const float* grad_score,
                                             int64_t heads, int64_t head_dim, float negative_slope, const int32_t* row,
                                             const int32_t* col, const int32_t* eid, const int64_t* indptr, int64_t num_edges,
                                             int64_t num_rows, float* grad_rows, float* grad_w_partials, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    if (heads <= 0 || head_dim <= 0 || num_edges < 0 || num_rows < 0 || !grad_rows ||
        (num_edges > 0 && (!x_by_col || !y_by_row || !w || !grad_score || !row || !col || !indptr)))
        return fail(PGLAMD_E_ARG, "add_score_backward: bad argument");
    if (num_edges > kMaxEdges || num_rows >= INT32_MAX) return fail(PGLAMD_E_RANGE, "add_score_backward: sizes beyond int32 engine range");
    const int64_t d = heads * head_dim;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_rows == 0) return PGLAMD_OK;
    if (num_edges == 0) {
        PGLAMD_HIP_CHECK(hipMemsetAsync(grad_rows, 0, (size_t)num_rows * d * sizeof(float), st));
        return PGLAMD_OK;
    }
    const int vec = gat_vec(heads, head_dim, x_by_col, y_by_row, grad_rows, false);
    if (vec == 0 || heads > kWave || reinterpret_cast<uintptr_t>(w) % 16 || reinterpret_cast<uintptr_t>(workspace) % 16 ||
        (grad_w_partials && reinterpret_cast<uintptr_t>(grad_w_partials) % 16))
        return fail(PGLAMD_E_SHAPE, "add_score_backward: heads*head_dim = %lld does not fit one 64-lane tile", (long long)d);
    if (!workspace || workspace_bytes < pglamd_gat_aggregate_workspace_bytes(num_edges, heads, head_dim))
        return fail(PGLAMD_E_WORKSPACE, "add_score_backward: workspace too small");
    GatParams p{};
    gat_set_geometry(p, heads, head_dim, negative_slope, num_edges);
    p.row = row; p.col = col; p.eid = eid; p.indptr = indptr;
    p.x = x_by_col; p.row_vec = y_by_row; p.w = w; p.ge = grad_score; p.out = grad_rows; p.part_w = grad_w_partials;
    p.out_rows = num_rows; p.n_csr_rows = num_rows;
    gat_setup_partials(p, workspace, 1);
    return with_vec(vec, [&](auto v) {
        constexpr int VEC = decltype(v)::value;
        return launch_chunked<float, VEC, 1, false>(p, st, [&](dim3 grid, const GatParams& q) {
            hipLaunchKernelGGL(add_score_bwd_kernel<VEC>, grid, dim3(kBlock), 0, st, q);
        });
    });
}
