// gatv2_attention.hip -- GATv2's attention over a graph (GATv2Conv, pgl/nn/conv.py:349-435), forward AND backward, without ever
// materialising an [E,H] tensor.  PGL's GATv2 uses ONE projection for score and value, so with x_src, x_dst [N,H,D] and a [H,D]:
//     z_e,h,d    = x_src[u,h,d] + x_dst[v,h,d]                        e = (u -> v)
//     s_e,h      = sum_d a[h,d] * L(z_e,h,d)                          L = leaky_relu(.; slope)
//     alpha_e,h  = softmax over the in-edges of v of s_e,h
//     out[v,h,:] = sum_e keep_e,h alpha_e,h x_src[u,h,:]
// The three-op composition (add_score -> segment_softmax -> aggregate with an edge operand) writes and re-reads two [E,H] tensors,
// gathers x[u] twice in the forward and walks the edges once per op of the chain in the backward.
//
// FORWARD (gv2_flat_kernel<VEC, 0>): the walk of dot_flat_kernel<VEC, 0> (dot_attention.hip) -- a wave per chunk of the dst-sorted
//   stream, scalar index loads, lanes across the H*D columns (VEC floats of one head per lane), several edges in flight.  x_dst[v] is
//   fetched at the row change and held, every lane holds its VEC values of a, every edge gathers x_src[u] ONCE and uses it for the score
//   and for the value; the per-head sum is a group_sum over the head's lanes and the online softmax is dot_flat_kernel's (one exponential
//   per edge, the same treatment of +-inf and NaN).  HBM traffic per edge: one gathered row (H*D*4 B) + 8 B of index (+ 4 B of edge id
//   under dropout).
// BACKWARD: alpha_e = exp(s_e - m[v]) / sum[v] recomputed from the forward's statistics; a pack kernel leaves
//   (m, 1 / sum, t = <g[v,h], out[v,h]>) per (node, head) as one 16-byte record.  With T_e = <g[v,h], x_src[u,h]>,
//   ds_e = alpha_e (keep_e T_e - t[v,h]) and L' = leaky_relu' (slope at z == 0: `z > 0 ? 1 : slope`, torch's convention and the one
//   of pglamd_add_score_backward, gat_fused.hip, which also tests `z > 0.f`):
//   MODE 1, DST-sorted stream (row = v: x_dst[v], g[v] and the record ride with the row; gathers x_src[u]):
//             d x_dst[v,h,d] = sum_{e into v} ds_e a[h,d] L'(z_e,h,d)
//             d a[h,d]       = sum_e ds_e L(z_e,h,d)       accumulated over the wave's WHOLE chunk (across row changes), one partial
//                              per chunk; the chunk partials are summed in a fixed order by a small reduce kernel, gv2_colsum_kernel,
//                              run twice (slices of chunks, then the slice sums): no atomic, bit-reproducible
//   MODE 2, SRC-sorted stream (row = u: x_src[u] rides with the row; gathers x_dst[v], g[v] and the record of v):
//             d x_src[u,h,d] = sum_{e out of u} keep_e alpha_e g[v,h,d] + ds_e a[h,d] L'(z_e,h,d)
// Attention dropout: drop_factor(seed, original edge id, head), the function and the mask of the GAT kernels.
// Rows longer than a chunk leave partials (acc | m | s forward, one float per column backward) merged in a fixed order by
// gv2_fixup_kernel (the associative softmax merge, or plain sums) through the lists of split_rows.hpp: atomic-free sums.
#include "attention_common.hpp"

#include <algorithm>
#include <initializer_list>

namespace pglamd {

struct alignas(16) Gv2Stat { float m, inv_s, t, pad; };   // per (node, head): softmax max, 1 / softmax sum, <g, out>

struct Gv2Params {
    const float* row_x;             // the row node's vector: x_dst[v] (MODE 0, 1) / x_src[u] (MODE 2)
    const float* row_g;             // the row node's cotangent g[v] (MODE 1)
    const float* col_x;             // gathered by col: x_src[u] (MODE 0, 1) / x_dst[v] (MODE 2)
    const float* col_g;             // gathered by col: g[v] (MODE 2)
    const float* attn;              // a [H,D]
    const Gv2Stat* packed;          // backward: [N,H] records of every node as a destination
    float* out;                     // out (MODE 0) / d x_dst (MODE 1) / d x_src (MODE 2)
    float* da_part;                 // MODE 1: [n_chunks, d] partials of d a, one per chunk
    float* row_max; float* row_sum; // forward: optional statistics output [out_rows,H]
    const int* row; const int* col; const int* eid; const int64_t* indptr;
    float* part_head; float* part_tail;         // [n_chunks, PW, d]
    int* long_count; int* long_list; int* long_list2;
    int64_t out_rows, n_csr_rows;
    int E, n_chunks, chunk, n_blocks, n_grid_chunks;
    int d, H, D;
    float slope, drop_p, drop_scale;
    unsigned seed;
};

// floats per column a chunk parks for a split row: acc | m | s (forward), one gradient (MODE 1, 2)
constexpr int gv2_partial_width(int mode) { return mode == 0 ? 3 : 1; }

// Edges per batch (two batches of gathered rows are live: one consumed, one in flight).  A batch element is ONE lane vector in MODE 0
// and 1 and two (and the 16-byte record) in MODE 2, on top of the held row vectors, the lane's values of a and the accumulators
// (two in MODE 1: d x_dst and d a).  The counts are dot_attention's, under which no instantiation uses scratch
// (profiles/gatv2_attention/kernel_resources.txt); other counts have not been timed.
constexpr int gv2_edges_in_flight(int vec, int mode, bool drop) {
    return mode == 0 ? (vec == 1 && !drop ? 8 : 4) : (vec == 4 ? 2 : 4);
}

template <int VEC, int MODE, bool DROP>
__global__ __launch_bounds__(kBlock) void gv2_flat_kernel(Gv2Params p) {
    constexpr int U = gv2_edges_in_flight(VEC, MODE, DROP);
    constexpr int PW = gv2_partial_width(MODE);
    using V = FV<VEC>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform(threadIdx.x >> 6);
    const int j0 = lane * VEC;
    const bool act = j0 < p.d;
    const int head = act ? j0 / p.D : 0;
    const int lph = p.D / VEC;                          // lanes per head: a power of two
    const bool head_lane = act && (j0 % p.D) == 0;

    if ((int)blockIdx.x >= p.n_grid_chunks) {
        zero_fill_role(p, lane, wib, [&](int64_t r) {
            if (act) *reinterpret_cast<V*>(p.out + r * p.d + j0) = V{};
            if (MODE == 0 && p.row_max && lane < p.H) { p.row_max[r * p.H + lane] = 0.f; p.row_sum[r * p.H + lane] = 0.f; }
        });
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

    float m = -INFINITY, s = 0.f, acc[VEC], da[MODE == 1 ? VEC : 1];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
    for (int k = 0; k < (MODE == 1 ? VEC : 1); ++k) da[k] = 0.f;
    // every chunk leaves its partial of d a, an empty one zeros: the reduce reads all n_chunks of them
    auto store_da = [&]() {
        if constexpr (MODE == 1) {
            if (!act) return;
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = da[k];
            *reinterpret_cast<V*>(p.da_part + (int64_t)c * p.d + j0) = o;
        }
    };
    if (e0 >= e1) { store_da(); return; }
    const float* __restrict__ rx = p.row_x;
    const float* __restrict__ rg = p.row_g;
    const float* __restrict__ cx = p.col_x;
    const float* __restrict__ cg = p.col_g;
    const Gv2Stat* __restrict__ pk = p.packed;
    const float slope = p.slope;
    V a_l{};                                            // this lane's VEC values of a
    if (act) a_l = *reinterpret_cast<const V*>(p.attn + j0);

    int cur = rowp[e0];
    bool head_open = e0 > 0 && rowp[e0 - 1] == cur;

    auto store_partial = [&](bool headp) {
        if (act) {
            float* dst = (headp ? p.part_head : p.part_tail) + (int64_t)c * PW * p.d;
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
            *reinterpret_cast<V*>(dst + j0) = o;
            if constexpr (MODE == 0) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = m;
                *reinterpret_cast<V*>(dst + p.d + j0) = o;
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = s;
                *reinterpret_cast<V*>(dst + 2 * p.d + j0) = o;
            }
        }
        if (!headp && lane == 0) p.long_list[atomicAdd(p.long_count, 1)] = c;
    };
    auto store_final = [&](int r) {
        if (r >= p.out_rows || !act) return;
        V o;
        const float f = MODE == 0 ? 1.f / s : 1.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = acc[k] * f;
        *reinterpret_cast<V*>(p.out + (int64_t)r * p.d + j0) = o;
        if (MODE == 0 && p.row_max && head_lane) { p.row_max[(int64_t)r * p.H + head] = m; p.row_sum[(int64_t)r * p.H + head] = s; }
    };
    // what belongs to the ROW node is fetched at the row change and held in registers until the next one
    V x_held{}, g_held{}; Gv2Stat s_held{};
    auto open_row = [&](int r) {
        if (!act) return;
        x_held = *reinterpret_cast<const V*>(rx + (int64_t)r * p.d + j0);
        if constexpr (MODE == 1) { g_held = *reinterpret_cast<const V*>(rg + (int64_t)r * p.d + j0); s_held = pk[(int64_t)r * p.H + head]; }
    };
    open_row(cur);
    auto consume = [&](int r, int ed, const V& xv, const V& gv, const Gv2Stat& sc) {
        if (r != cur) {
            if (head_open) store_partial(true); else store_final(cur);
            head_open = false;
            cur = r;
            m = -INFINITY; s = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
            open_row(r);
        }
        float lr[VEC], dl[VEC], dot = 0.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float z = x_held.v[k] + xv.v[k];
            lr[k] = z > 0.f ? z : slope * z;                                   // (a NaN stays one)
            dl[k] = z > 0.f ? 1.f : slope;                                     // L' = slope at z == 0
            dot += a_l.v[k] * lr[k];
        }
        const float l = group_sum(dot, lph);
        const float df = DROP ? drop_factor(p.seed, ed, head, p.drop_p, p.drop_scale) : 1.f;
        if constexpr (MODE == 0) {
            // online softmax: one of exp(m - mn), exp(l - mn) is always exp(0) = 1, so ONE exponential per edge.  Special values as
            // dot_flat_kernel: a -inf score weighs 0 and leaves (m, s) alone, a +inf or NaN score makes the (row, head) NaN.
            const float dlt = l - m;                 // +inf on the first edge of a row (m = -inf): e^{-inf} = 0
            const float ed2 = l == -INFINITY ? 0.f : expf(-fabsf(dlt));
            const bool up = dlt > 0.f;
            const float rs = up ? ed2 : 1.f, pe = l == INFINITY ? NAN : (up ? 1.f : ed2);
            s = s * rs + pe;
            const float w = pe * df;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * rs + w * xv.v[k];
            m = up ? l : m;
        } else {
            // T_e = <g[v], x_src[u]>: g rides with the row and x_src is gathered (MODE 1), or the other way round (MODE 2)
            float dt = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) dt += MODE == 1 ? g_held.v[k] * xv.v[k] : gv.v[k] * x_held.v[k];
            dt = group_sum(dt, lph);
            const Gv2Stat st = MODE == 1 ? s_held : sc;                       // the record of the destination v
            // expf, not the bare hardware exp2 of the GAT gradients: that one flushes a result below 2^-126 to 0, and with scores of
            // a few hundred an alpha of 1e-39 times a (T - t) a of a few hundred is a gradient term far above the smallest normal number
            const float alpha = expf(l - st.m) * st.inv_s;
            const float ds = alpha * (df * dt - st.t);
            if constexpr (MODE == 1) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) { acc[k] += ds * (a_l.v[k] * dl[k]); da[k] += ds * lr[k]; }
            } else {
                const float w = alpha * df;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += w * gv.v[k] + ds * (a_l.v[k] * dl[k]);
            }
        }
    };
    auto load_idx = [&](int e, int (&cc)[U], int (&rr)[U], int (&ee)[U]) {
#pragma unroll
        for (int i = 0; i < U; ++i) { rr[i] = rowp[e + i]; cc[i] = colp[e + i]; ee[i] = DROP ? eidp[e + i] : 0; }
    };
    auto load_rows = [&](const int (&cc)[U], V (&vx)[U], V (&vg)[U], Gv2Stat (&sc)[U]) {
        if (!act) return;
#pragma unroll
        for (int i = 0; i < U; ++i) {
            vx[i] = *reinterpret_cast<const V*>(cx + (int64_t)cc[i] * p.d + j0);
            if constexpr (MODE == 2) { vg[i] = *reinterpret_cast<const V*>(cg + (int64_t)cc[i] * p.d + j0); sc[i] = pk[(int64_t)cc[i] * p.H + head]; }
        }
    };
    // three stages deep, as the GAT walks: rows of batch g consumed, rows of g+1 in flight, (scalar) indices of g+2 being fetched
    int e = e0;
    const int n_full = (e1 - e0) / U;
    int cA[U], rA[U], eA[U]; V xA[U] = {}, gA[U] = {}; Gv2Stat sA[U] = {};   // (g and the records: MODE 2 only)
    int cB[U], rB[U], eB[U];
    if (n_full > 0) { load_idx(e, cA, rA, eA); load_rows(cA, xA, gA, sA); }
    if (n_full > 1) load_idx(e + U, cB, rB, eB);
    for (int g = 0; g < n_full; ++g) {
        int cC[U], rC[U], eC[U]; V xB[U] = {}, gB[U] = {}; Gv2Stat sB[U] = {};
        const bool more = g + 1 < n_full, more2 = g + 2 < n_full;
        if (more) load_rows(cB, xB, gB, sB);
        if (more2) load_idx(e + 2 * U, cC, rC, eC);
#pragma unroll
        for (int i = 0; i < U; ++i) consume(rA[i], eA[i], xA[i], gA[i], sA[i]);
        if (more) {
#pragma unroll
            for (int i = 0; i < U; ++i) {
                rA[i] = rB[i]; eA[i] = eB[i]; xA[i] = xB[i];
                if constexpr (MODE == 2) { gA[i] = gB[i]; sA[i] = sB[i]; }
            }
        }
        if (more2) {
#pragma unroll
            for (int i = 0; i < U; ++i) { cB[i] = cC[i]; rB[i] = rC[i]; eB[i] = eC[i]; }
        }
        e += U;
    }
    for (; e < e1; ++e) {
        const int r = rowp[e], cc = colp[e];
        const int ed = DROP ? eidp[e] : 0;
        V xv{}, gv{}; Gv2Stat sc{};
        if (act) {
            xv = *reinterpret_cast<const V*>(cx + (int64_t)cc * p.d + j0);
            if constexpr (MODE == 2) { gv = *reinterpret_cast<const V*>(cg + (int64_t)cc * p.d + j0); sc = pk[(int64_t)cc * p.H + head]; }
        }
        consume(r, ed, xv, gv, sc);
    }
    const bool tail_open = e1 < p.E && rowp[e1] == cur;
    if (head_open) store_partial(true);
    else if (tail_open) store_partial(false);
    else store_final(cur);
    store_da();
}

// merges the partials of the rows longer than a chunk, from the work list the flat kernel filled: the two passes, lists and merge
// order of dot_fixup_kernel (split_rows.hpp).  SOFTMAX: the associative softmax merge of (acc, m, s); else the sum of one vector per
// column.
template <int VEC, bool LONG, bool SOFTMAX>
__global__ __launch_bounds__(LONG ? kFixWaves * kWave : kBlock) void gv2_fixup_kernel(Gv2Params p) {
    using V = FV<VEC>;
    constexpr int NW = LONG ? kFixWaves : 1;
    constexpr int PW = SOFTMAX ? 3 : 1;
    __shared__ float red_v[LONG ? kFixWaves : 1][LONG ? kWave * VEC : 1];
    __shared__ float red_s[LONG ? kFixWaves : 1][2][LONG ? kWave : 1];
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
        float m, s, acc[VEC];                            // additive mode: s counts the partials merged (0: none)
        auto reset = [&]() {
            m = SOFTMAX ? -INFINITY : 0.f; s = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        };
        auto merge_vals = [&](const V& v0, float m2, float s2) {
            if constexpr (SOFTMAX) {
                const float mn = fmaxf(m, m2);
                const float c1 = m == mn ? 1.f : expf(m - mn), c2 = m2 == mn ? 1.f : expf(m2 - mn);   // (both -inf: every edge so far masked)
                s = s * c1 + s2 * c2;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * c1 + v0.v[k] * c2;
                m = mn;
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += v0.v[k];
                s += s2;
            }
        };
        auto merge = [&](const float* base) {
            if constexpr (SOFTMAX) merge_vals(*reinterpret_cast<const V*>(base + j0), base[p.d + j0], base[2 * p.d + j0]);
            else merge_vals(*reinterpret_cast<const V*>(base + j0), 0.f, 1.f);
        };
        reset();
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
            red_s[wib][0][lane] = m; red_s[wib][1][lane] = s;
            __syncthreads();
            if (wib != 0) continue;
            // wave 0: tail partial of chunk a first, then the wave results in wave order
            reset();
            if (act) {
                merge(p.part_tail + (int64_t)a * PW * p.d);
                for (int w = 0; w < NW; ++w) {
                    const float s2 = red_s[w][1][lane];
                    if (s2 == 0.f) continue;                     // that wave had no partial
                    V v0;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) v0.v[k] = red_v[w][lane * VEC + k];
                    merge_vals(v0, red_s[w][0][lane], s2);
                }
            }
        }
        if (!act || r >= p.out_rows) continue;
        V o;
        const float f = SOFTMAX ? 1.f / s : 1.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = acc[k] * f;
        *reinterpret_cast<V*>(p.out + (int64_t)r * p.d + j0) = o;
        if (SOFTMAX && p.row_max && (j0 % p.D) == 0) { p.row_max[(int64_t)r * p.H + j0 / p.D] = m; p.row_sum[(int64_t)r * p.H + j0 / p.D] = s; }
    }
}

// t[v,h] = <g[v,h,:], out[v,h,:]> (the softmax-backward row term) with the destination's statistics, one 16-byte record per
// (node, head): dot_pack_kernel's layout.  LANES = head_dim / 4 lanes share one pair (LANES = 0: one thread per pair).  A row without
// in-edges (sum 0) gets 1 / sum = 0; no edge reads its record.
template <int LANES>
__global__ __launch_bounds__(kBlock) void gv2_pack_kernel(const float* __restrict__ m, const float* __restrict__ sm, const float* __restrict__ g,
                                                         const float* __restrict__ out, int64_t n, int D, Gv2Stat* __restrict__ packed) {
    auto record = [&](int64_t i, float t) { const float s = sm[i]; return Gv2Stat{m[i], s > 0.f ? 1.f / s : 0.f, t, 0.f}; };
    if constexpr (LANES == 0) {
        const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (i >= n) return;
        float t = 0.f;
        for (int k = 0; k < D; ++k) t += g[i * D + k] * out[i * D + k];
        packed[i] = record(i, t);
    } else {
        const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;          // float4 index into [n, D]
        const bool live = q < n * LANES;
        float t = 0.f;
        if (live) {
            const float4 a = reinterpret_cast<const float4*>(g)[q], b = reinterpret_cast<const float4*>(out)[q];
            t = a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
        }
        t = group_sum(t, LANES);
        if (live && (q % LANES) == 0) packed[q / LANES] = record(q / LANES, t);
    }
}

// out[b, col] = the sum of in[r, col] over the rows r of slice b = [b * per, min(n, (b + 1) * per)), d <= kBlock columns, in a fixed
// order: thread (sub, col) adds the rows lo + sub, lo + sub + nsub, ... and thread (0, col) then adds the nsub sums in order.
__global__ __launch_bounds__(kBlock) void gv2_colsum_kernel(const float* __restrict__ in, int n, int d, int per, float* __restrict__ out) {
    __shared__ float red[kBlock];
    const int nsub = kBlock / d;
    const int col = threadIdx.x % d, sub = threadIdx.x / d;
    const int lo = (int)blockIdx.x * per, hi = min(n, lo + per);
    float s = 0.f;
    if (sub < nsub)
        for (int r = lo + sub; r < hi; r += nsub) s += in[(int64_t)r * d + col];
    red[threadIdx.x] = s;
    __syncthreads();
    if (sub != 0) return;
    float t = 0.f;
    for (int i = 0; i < nsub; ++i) t += red[i * d + col];
    out[(int64_t)blockIdx.x * d + col] = t;
}

// Host side.

constexpr int kGv2SumSlices = 256;      // slices of the chunk partials of d a in the first pass of the reduce (at least 64 chunks each)

static void gv2_set_geometry(Gv2Params& p, int64_t heads, int64_t head_dim, float slope, float drop_p, uint32_t seed, int64_t num_edges,
                             int64_t num_nodes) {
    p.H = (int)heads; p.D = (int)head_dim; p.d = (int)(heads * head_dim); p.slope = slope;
    p.drop_p = drop_p; p.drop_scale = 1.f / (1.f - drop_p); p.seed = seed;
    p.E = (int)num_edges; p.chunk = chunk_edges_for(num_edges); p.n_chunks = (int)ceil_div(num_edges, p.chunk);
    p.out_rows = num_nodes; p.n_csr_rows = num_nodes;
}

template <int VEC, bool SOFTMAX>
static int32_t launch_gv2_fixups(const Gv2Params& p, hipStream_t st) {
    hipLaunchKernelGGL((gv2_fixup_kernel<VEC, false, SOFTMAX>), dim3(fixup_grid_short(p.n_chunks, kFixGridShort, kWavesPerBlock)), dim3(kBlock), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((gv2_fixup_kernel<VEC, true, SOFTMAX>), dim3(fixup_grid_long(p.n_chunks)), dim3(kFixWaves * kWave), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

// one walk and its fix-up; the workspace holds the partials of THIS walk (the walks of a backward run one after the other)
template <int MODE>
static int32_t launch_gv2(int vec, Gv2Params p, void* workspace, hipStream_t st) {
    SplitWs(p.n_chunks, (int64_t)gv2_partial_width(MODE) * p.d, sizeof(float)).carve(p, workspace);
    return with_vec(vec, [&](auto v) {
        constexpr int VEC = decltype(v)::value;
        return launch_chunked_rows(p, st, [&](dim3 grid, const Gv2Params& q) {
            if (q.drop_p > 0.f) hipLaunchKernelGGL((gv2_flat_kernel<VEC, MODE, true>), grid, dim3(kBlock), 0, st, q);
            else hipLaunchKernelGGL((gv2_flat_kernel<VEC, MODE, false>), grid, dim3(kBlock), 0, st, q);
        }, [&](const Gv2Params& q) { return launch_gv2_fixups<VEC, MODE == 0>(q, st); });
    });
}

static const void* gv2_ptr_or(std::initializer_list<const void*> ps) {
    uintptr_t a = 0;
    for (const void* q : ps) a |= reinterpret_cast<uintptr_t>(q);
    return reinterpret_cast<const void*>(a);
}

static int64_t gv2_chunks(int64_t num_edges) { return num_edges > 0 ? ceil_div(num_edges, chunk_edges_for(num_edges)) : 0; }

}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_gatv2_attention_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim) {
    if (num_edges <= 0 || heads <= 0 || head_dim <= 0) return 256;
    return SplitWs(gv2_chunks(num_edges), 3 * heads * head_dim, sizeof(float)).bytes() + 256;
}

extern "C" int32_t pglamd_gatv2_attention(const float* x_src, const float* x_dst, const float* attn, int64_t heads, int64_t head_dim,
                                          float negative_slope, float drop_p, uint32_t seed, const int32_t* row, const int32_t* col,
                                          const int32_t* eid, const int64_t* indptr, int64_t num_edges, int64_t num_nodes, float* out,
                                          float* row_max, float* row_sum, void* workspace, size_t workspace_bytes, void* stream) {
    if (!out || !indptr || heads <= 0 || head_dim <= 0 || num_nodes < 0 || (num_edges > 0 && (!x_src || !x_dst || !attn || !row || !col)))
        return fail(PGLAMD_E_ARG, "gatv2_attention: bad argument");
    if ((row_max == nullptr) != (row_sum == nullptr)) return fail(PGLAMD_E_ARG, "gatv2_attention: row_max/row_sum must both be given or both NULL");
    if (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && num_edges > 0 && !eid)) return fail(PGLAMD_E_ARG, "gatv2_attention: dropout needs 0 <= p < 1 and eid");
    if (num_edges < 0 || num_edges > kMaxEdges || num_nodes >= INT32_MAX) return fail(PGLAMD_E_RANGE, "gatv2_attention: sizes beyond int32 engine range");
    const int64_t d = heads * head_dim;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_nodes == 0) return PGLAMD_OK;
    if (num_edges == 0) {
        PGLAMD_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)num_nodes * d * sizeof(float), st));
        if (row_max) {
            PGLAMD_HIP_CHECK(hipMemsetAsync(row_max, 0, (size_t)num_nodes * heads * sizeof(float), st));
            PGLAMD_HIP_CHECK(hipMemsetAsync(row_sum, 0, (size_t)num_nodes * heads * sizeof(float), st));
        }
        return PGLAMD_OK;
    }
    const int vec = gat_vec(heads, head_dim, gv2_ptr_or({x_src, x_dst, attn}), out, workspace, true);
    if (vec == 0 || heads > kWave)
        return fail(PGLAMD_E_SHAPE, "gatv2_attention: heads*head_dim = %lld needs one 64-lane tile, head_dim/VEC a power of two and operands aligned to their lanes",
                    (long long)d);
    if (!workspace || workspace_bytes < pglamd_gatv2_attention_workspace_bytes(num_edges, heads, head_dim))
        return fail(PGLAMD_E_WORKSPACE, "gatv2_attention: workspace too small");
    Gv2Params p{};
    gv2_set_geometry(p, heads, head_dim, negative_slope, drop_p, seed, num_edges, num_nodes);
    p.row_x = x_dst; p.col_x = x_src; p.attn = attn; p.out = out; p.row_max = row_max; p.row_sum = row_sum;
    p.row = row; p.col = col; p.eid = eid; p.indptr = indptr;
    return launch_gv2<0>(vec, p, workspace, st);
}

// [ records | chunk partials of d a | slice sums of d a | the partials of one walk ]
extern "C" size_t pglamd_gatv2_attention_backward_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t heads, int64_t head_dim) {
    if (heads <= 0 || head_dim <= 0) return 256;
    const size_t d = (size_t)(heads * head_dim);
    return align_up((size_t)(num_nodes > 0 ? num_nodes : 1) * heads * sizeof(Gv2Stat), 256) +
           align_up((size_t)std::max<int64_t>(gv2_chunks(num_edges), 1) * d * sizeof(float), 256) +
           align_up((size_t)kGv2SumSlices * d * sizeof(float), 256) + pglamd_gatv2_attention_workspace_bytes(num_edges, heads, head_dim);
}

extern "C" int32_t pglamd_gatv2_attention_backward(const float* grad_out, const float* x_src, const float* x_dst, const float* attn,
                                                   const float* out, const float* row_max, const float* row_sum, int64_t heads,
                                                   int64_t head_dim, float negative_slope, float drop_p, uint32_t seed,
                                                   const int32_t* dst_row, const int32_t* dst_col, const int32_t* dst_eid,
                                                   const int64_t* dst_indptr, const int32_t* src_row, const int32_t* src_col,
                                                   const int32_t* src_eid, const int64_t* src_indptr, int64_t num_edges,
                                                   int64_t num_nodes, float* grad_x_src, float* grad_x_dst, float* grad_attn,
                                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (heads <= 0 || head_dim <= 0 || num_nodes < 0 || num_edges < 0 || !grad_x_src || !grad_x_dst || !grad_attn ||
        (num_edges > 0 && (!grad_out || !x_src || !x_dst || !attn || !out || !row_max || !row_sum || !dst_row || !dst_col || !dst_indptr ||
                           !src_row || !src_col || !src_indptr)))
        return fail(PGLAMD_E_ARG, "gatv2_attention_backward: bad argument");
    if (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && num_edges > 0 && (!dst_eid || !src_eid)))
        return fail(PGLAMD_E_ARG, "gatv2_attention_backward: dropout needs 0 <= p < 1 and both eid arrays");
    if (num_edges > kMaxEdges || num_nodes >= INT32_MAX) return fail(PGLAMD_E_RANGE, "gatv2_attention_backward: sizes beyond int32 engine range");
    const int64_t d = heads * head_dim;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_nodes == 0 || num_edges == 0) {                    // (d a is a sum over the edges: 0 without any, whatever the nodes)
        PGLAMD_HIP_CHECK(hipMemsetAsync(grad_attn, 0, (size_t)d * sizeof(float), st));
        for (float* gp : {grad_x_src, grad_x_dst})
            if (num_nodes > 0) PGLAMD_HIP_CHECK(hipMemsetAsync(gp, 0, (size_t)num_nodes * d * sizeof(float), st));
        return PGLAMD_OK;
    }
    const int vec = gat_vec(heads, head_dim, gv2_ptr_or({grad_out, x_src, x_dst, attn}), gv2_ptr_or({grad_x_src, grad_x_dst}), nullptr, true);
    if (vec == 0 || heads > kWave || reinterpret_cast<uintptr_t>(workspace) % 256 ||
        (head_dim % 4 == 0 && (reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(grad_out)) % 16))
        return fail(PGLAMD_E_SHAPE, "gatv2_attention_backward: heads*head_dim = %lld needs one 64-lane tile, head_dim/VEC a power of two and operands aligned to their lanes",
                    (long long)d);
    if (!workspace || workspace_bytes < pglamd_gatv2_attention_backward_workspace_bytes(num_edges, num_nodes, heads, head_dim))
        return fail(PGLAMD_E_WORKSPACE, "gatv2_attention_backward: workspace too small");
    Gv2Params p{};
    gv2_set_geometry(p, heads, head_dim, negative_slope, drop_p, seed, num_edges, num_nodes);
    Carver ws(workspace, workspace_bytes);
    Gv2Stat* packed = ws.take<Gv2Stat>((size_t)num_nodes * heads);
    float* da_part = ws.take<float>((size_t)p.n_chunks * d);
    float* da_slices = ws.take<float>((size_t)kGv2SumSlices * d);
    void* walk_ws = static_cast<char*>(workspace) + ws.off;
    // (0) the destination-side scalars of every (node, head), packed so that an edge fetches them with one 16-byte load
    {
        const int64_t pairs = num_nodes * heads;
        const int lanes = (head_dim % 4 == 0 && head_dim / 4 <= 16 && ((head_dim / 4) & (head_dim / 4 - 1)) == 0) ? (int)(head_dim / 4) : 0;
#define PGLAMD_PACK(L) hipLaunchKernelGGL(gv2_pack_kernel<L>, dim3((unsigned)ceil_div(pairs * (L ? L : 1), kBlock)), dim3(kBlock), 0, st, \
                                          row_max, row_sum, grad_out, out, pairs, (int)head_dim, packed)
        switch (lanes) {
            case 1: PGLAMD_PACK(1); break;
            case 2: PGLAMD_PACK(2); break;
            case 4: PGLAMD_PACK(4); break;
            case 8: PGLAMD_PACK(8); break;
            case 16: PGLAMD_PACK(16); break;
            default: PGLAMD_PACK(0); break;
        }
#undef PGLAMD_PACK
    }
    PGLAMD_LAUNCH_CHECK();
    p.packed = packed; p.attn = attn;
    // (1) dst-sorted walk: row = v carries x_dst[v], g[v] and its record; gathers x_src[u]; writes d x_dst[v] and the chunk partials of d a
    Gv2Params a = p;
    a.row = dst_row; a.col = dst_col; a.eid = dst_eid; a.indptr = dst_indptr;
    a.row_x = x_dst; a.row_g = grad_out; a.col_x = x_src; a.out = grad_x_dst; a.da_part = da_part;
    PGLAMD_TRY(launch_gv2<1>(vec, a, walk_ws, st));
    // (1') d a: the chunk partials summed slice by slice, then the slice sums, each in a fixed order
    {
        const int slices = (int)std::min<int64_t>(kGv2SumSlices, ceil_div(p.n_chunks, 64));
        const int per = (int)ceil_div(p.n_chunks, slices);
        const int used = (int)ceil_div(p.n_chunks, per);
        hipLaunchKernelGGL(gv2_colsum_kernel, dim3(used), dim3(kBlock), 0, st, da_part, p.n_chunks, (int)d, per, da_slices);
        PGLAMD_LAUNCH_CHECK();
        hipLaunchKernelGGL(gv2_colsum_kernel, dim3(1), dim3(kBlock), 0, st, da_slices, used, (int)d, used, grad_attn);
        PGLAMD_LAUNCH_CHECK();
    }
    // (2) src-sorted walk: row = u carries x_src[u]; gathers x_dst[v], g[v] and v's record; writes d x_src[u]
    p.row = src_row; p.col = src_col; p.eid = src_eid; p.indptr = src_indptr;
    p.row_x = x_src; p.col_x = x_dst; p.col_g = grad_out; p.out = grad_x_src;
    return launch_gv2<2>(vec, p, walk_ws, st);
}
