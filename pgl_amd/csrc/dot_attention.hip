// dot_attention.hip -- scaled dot-product attention over a graph (TransformerConv, pgl/nn/conv.py:796-847), forward AND backward,
// without ever materialising an [E,H] tensor:
//     s_e,h      = scale * <q[v,h,:], k[u,h,:]>                      e = (u -> v)
//     alpha_e,h  = softmax over the in-edges of v of s_e,h
//     out[v,h,:] = sum_e keep_e,h alpha_e,h v[u,h,:]
// and, with the compile-time switch EDGE, the same with a per-edge feature ef[e] added to the key and to the value (the layer's
// message function with edge_feat, pgl/nn/conv.py:808-815): k[u] + ef_e in the score, v[u] + ef_e in the sum.
// The three-op composition (sddmm -> segment_softmax -> aggregate with an edge operand) writes and re-reads two [E,H] tensors in
// the forward and walks the edges five more times in the backward.
//
// FORWARD (dot_flat_kernel<VEC, 0>): the walk of gat_flat_kernel<VEC, 0> -- a wave per chunk of the dst-sorted stream, scalar index
//   loads, lanes across the H*D columns (VEC floats of one head per lane), several edges in flight -- with the score formed inside:
//   q[v] is fetched at the row change and held, every edge gathers k[u] and v[u], the per-head dot product is a group_sum over
//   the head's lanes, and the online softmax state (running max m, running sum s, rescaled accumulator) is flash-attention's.
//   HBM traffic per edge: two gathered rows (2 * H*D*4 B) + 8 B of index (+ 4 B of edge id under dropout).
// BACKWARD: alpha_e = exp(s_e - m[v]) / sum[v] recomputed from the forward's statistics; a pack kernel leaves
//   (m, 1 / sum, t = <g[v,h], out[v,h]>) per (node, head) as one 16-byte record.  With ds_e = alpha_e (keep_e <g[v], v[u]>_h - t[v,h]):
//   MODE 1, DST-sorted stream (row = v: g[v], q[v] and the record ride with the row; gathers k[u], v[u]):
//             dq[v] = scale * sum_{e into v} ds_e k[u]
//   MODE 2, SRC-sorted stream (row = u: k[u], v[u] ride with the row; gathers q[v], g[v] and the record of v):
//             dk[u] = scale * sum_{e out of u} ds_e q[v]        dv[u] = sum_{e out of u} keep_e alpha_e g[v]
//   Two dot products per edge in each walk, nothing per edge stored.
// EDGE: every walk gathers a third lane vector per edge, ef[eid[e]] (eid NULL: the position itself).  MODE 0, 1: it is added to the two
//   gathered rows (k[u] + ef, v[u] + ef) before anything reads them; MODE 2: to the two held rows (k[u], v[u] ride with the row, ef
//   changes per edge).  The gradient of ef is edge e's own contribution to dk[u] + dv[u],
//             def[e] = scale * ds_e q[v] + keep_e alpha_e g[v]
//   and MODE 2 holds every factor of it: one plain vector store to row eid[e] per edge, each edge visited once, no atomics.
// Attention dropout: drop_factor(seed, original edge id, head), the function and the mask of the GAT kernels.
// Rows longer than a chunk leave partials (acc | m | s forward, 1 resp. 2 floats per column backward) merged in a fixed order by
// dot_fixup_kernel (the associative softmax merge, or plain sums): atomic-free sums, bit-reproducible.
#include "attention_common.hpp"

#include <algorithm>
#include <initializer_list>

namespace pglamd {

struct alignas(16) DotStat { float m, inv_s, t, pad; };   // per (node, head): softmax max, 1 / softmax sum, <g, out>

struct DotParams {
    const float* row_a;             // the row node's vector the score reads: q[v] (MODE 0, 1) / k[u] (MODE 2)
    const float* row_b;             // the row node's second vector: g[v] (MODE 1) / v[u] (MODE 2)
    const float* col_x;             // gathered by col, the score's other factor: k[u] (MODE 0, 1) / q[v] (MODE 2)
    const float* col_y;             // gathered by col: v[u] (MODE 0, 1) / g[v] (MODE 2)
    const DotStat* packed;          // backward: [N,H] records of every node as a destination
    float* out;                     // out (MODE 0) / dq (MODE 1) / dk (MODE 2)
    float* out2;                    // dv (MODE 2)
    float* row_max; float* row_sum; // forward: optional statistics output [out_rows,H]
    const int* row; const int* col; const int* eid; const int64_t* indptr;
    float* part_head; float* part_tail;         // [n_chunks, PW, d]
    int* long_count; int* long_list; int* long_list2;
    int64_t out_rows, n_csr_rows;
    int E, n_chunks, chunk, n_blocks, n_grid_chunks;
    int d, H, D;
    float scale, drop_p, drop_scale;
    unsigned seed;
    const float* edge;              // EDGE: [E,H,D] per-edge feature, row eid[e] (eid NULL: row e)
    float* grad_edge;               // EDGE, MODE 2: its gradient, same rows (NULL: not wanted)
};

// floats per column a chunk parks: acc | m | s (forward), dq (MODE 1), dk | dv (MODE 2)
constexpr int dot_partial_width(int mode) { return mode == 0 ? 3 : mode; }

// Edges per batch (two batches of gathered rows are live: one consumed, one in flight).  A batch element is two lane vectors (and
// the 16-byte record in MODE 2) on top of the two held row vectors and the one or two accumulators, so the widest lanes take
// shorter batches in the gradient walks and the narrowest longer ones in the forward: no instantiation spills
// (profiles/dot_attention/kernel_resources.txt), and batches of 2 / 4 / 8 measured in profiles/dot_attention/README.md.
// EDGE: a batch element is three lane vectors and its edge id is always loaded, so four floats per lane take batches of 2 in every
// walk and the narrower lanes batches of 4 (profiles/dot_attention_edge/kernel_resources.txt: no scratch, no VGPR spill).
constexpr int dot_edges_in_flight(int vec, int mode, bool drop, bool edge = false) {
    if (edge) return vec == 4 ? 2 : 4;
    return mode == 0 ? (vec == 1 && !drop ? 8 : 4) : (vec == 4 ? 2 : 4);   // (8 with the edge ids of dropout: the indices of three batches overflow the SGPRs into scratch)
}

template <int VEC, int MODE, bool DROP, bool EDGE = false>
__global__ __launch_bounds__(kBlock) void dot_flat_kernel(DotParams p) {
    constexpr int U = dot_edges_in_flight(VEC, MODE, DROP, EDGE);
    constexpr int UE = EDGE ? U : 1;                    // the batch's edge-feature vectors (none without EDGE)
    constexpr int PW = dot_partial_width(MODE);
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
            if (act) {
                *reinterpret_cast<V*>(p.out + r * p.d + j0) = V{};
                if constexpr (MODE == 2) *reinterpret_cast<V*>(p.out2 + r * p.d + j0) = V{};
            }
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
    if (e0 >= e1) return;
    const float* __restrict__ ra = p.row_a;
    const float* __restrict__ rb = p.row_b;
    const float* __restrict__ cx = p.col_x;
    const float* __restrict__ cy = p.col_y;
    const DotStat* __restrict__ pk = p.packed;
    const float* __restrict__ ef = p.edge;
    const bool has_eid = p.eid != nullptr;
    const float scale = p.scale;

    float m = -INFINITY, s = 0.f, acc[VEC], acc2[MODE == 2 ? VEC : 1];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
    for (int k = 0; k < (MODE == 2 ? VEC : 1); ++k) acc2[k] = 0.f;
    int cur = rowp[e0];
    bool head_open = e0 > 0 && rowp[e0 - 1] == cur;

    auto store_partial = [&](bool headp) {
        if (act) {
            float* dst = (headp ? p.part_head : p.part_tail) + (int64_t)c * PW * p.d;
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
            *reinterpret_cast<V*>(dst + j0) = o;
            if constexpr (MODE == 2) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = acc2[k];
                *reinterpret_cast<V*>(dst + p.d + j0) = o;
            }
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
        const float f = MODE == 0 ? 1.f / s : scale;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = acc[k] * f;
        *reinterpret_cast<V*>(p.out + (int64_t)r * p.d + j0) = o;
        if constexpr (MODE == 2) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = acc2[k];
            *reinterpret_cast<V*>(p.out2 + (int64_t)r * p.d + j0) = o;
        }
        if (MODE == 0 && p.row_max && head_lane) { p.row_max[(int64_t)r * p.H + head] = m; p.row_sum[(int64_t)r * p.H + head] = s; }
    };
    // what belongs to the ROW node is fetched at the row change and held in registers until the next one
    V a_held{}, b_held{}; DotStat s_held{};
    auto open_row = [&](int r) {
        if (!act) return;
        a_held = *reinterpret_cast<const V*>(ra + (int64_t)r * p.d + j0);
        if constexpr (MODE >= 1) b_held = *reinterpret_cast<const V*>(rb + (int64_t)r * p.d + j0);
        if constexpr (MODE == 1) s_held = pk[(int64_t)r * p.H + head];
    };
    open_row(cur);
    auto consume = [&](int r, int ed, const V& xv, const V& yv, const V& ev, const DotStat& sc) {
        if (r != cur) {
            if (head_open) store_partial(true); else store_final(cur);
            head_open = false;
            cur = r;
            m = -INFINITY; s = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int k = 0; k < (MODE == 2 ? VEC : 1); ++k) acc2[k] = 0.f;
            open_row(r);
        }
        // what the score and the weighted sums read: with EDGE the key and the value carry ef_e -- on the gathered side where they are
        // gathered (MODE 0, 1), on the held side where they ride with the row (MODE 2).  (Every condition below is a compile-time
        // constant: without EDGE the four names are the operands themselves and with_a / with_b do not exist in the code.)
        V with_a{}, with_b{};
        if constexpr (EDGE) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                with_a.v[k] = (MODE == 2 ? a_held.v[k] : xv.v[k]) + ev.v[k];
                with_b.v[k] = (MODE == 2 ? b_held.v[k] : yv.v[k]) + ev.v[k];
            }
        }
        const V& ah = EDGE && MODE == 2 ? with_a : a_held;
        const V& bh = EDGE && MODE == 2 ? with_b : b_held;
        const V& xe = EDGE && MODE != 2 ? with_a : xv;
        const V& ye = EDGE && MODE != 2 ? with_b : yv;
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) dot += ah.v[k] * xe.v[k];               // <q[v], k[u]> restricted to this lane
        const float l = scale * group_sum(dot, lph);
        const float df = DROP ? drop_factor(p.seed, ed, head, p.drop_p, p.drop_scale) : 1.f;
        if constexpr (MODE == 0) {
            // online softmax: one of exp(m - mn), exp(l - mn) is always exp(0) = 1, so ONE exponential per edge.  Special values as
            // gat_flat_kernel: a -inf score weighs 0 and leaves (m, s) alone, a +inf or NaN score makes the (row, head) NaN.
            const float dlt = l - m;                 // +inf on the first edge of a row (m = -inf): e^{-inf} = 0
            const float ed2 = l == -INFINITY ? 0.f : expf(-fabsf(dlt));
            const bool up = dlt > 0.f;
            const float rs = up ? ed2 : 1.f, pe = l == INFINITY ? NAN : (up ? 1.f : ed2);
            s = s * rs + pe;
            const float w = pe * df;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * rs + w * ye.v[k];
            m = up ? l : m;
        } else {
            float dt = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) dt += bh.v[k] * ye.v[k];            // <g[v], v[u]> restricted to this lane
            dt = group_sum(dt, lph);
            const DotStat st = MODE == 1 ? s_held : sc;                       // the record of the destination v
            const float alpha = __expf(l - st.m) * st.inv_s;                  // hardware exp2, as the GAT gradients
            const float ds = alpha * (df * dt - st.t);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] += ds * xe.v[k];
            if constexpr (MODE == 2) {
                const float w = alpha * df;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc2[k] += w * ye.v[k];
                if constexpr (EDGE) {
                    if (p.grad_edge && act) {                                 // def[e]: this edge's term of dk[u] + dv[u], written once
                        V o;
#pragma unroll
                        for (int k = 0; k < VEC; ++k) o.v[k] = scale * ds * xv.v[k] + w * yv.v[k];
                        *reinterpret_cast<V*>(p.grad_edge + (int64_t)ed * p.d + j0) = o;
                    }
                }
            }
        }
    };
    auto load_idx = [&](int e, int (&cc)[U], int (&rr)[U], int (&ee)[U]) {
#pragma unroll
        for (int i = 0; i < U; ++i) {
            rr[i] = rowp[e + i]; cc[i] = colp[e + i];
            if constexpr (EDGE) ee[i] = has_eid ? eidp[e + i] : e + i;
            else ee[i] = DROP ? eidp[e + i] : 0;
        }
    };
    auto load_rows = [&](const int (&cc)[U], const int (&ee)[U], V (&vx)[U], V (&vy)[U], V (&vz)[UE], DotStat (&sc)[U]) {
        if (!act) return;
#pragma unroll
        for (int i = 0; i < U; ++i) {
            vx[i] = *reinterpret_cast<const V*>(cx + (int64_t)cc[i] * p.d + j0);
            vy[i] = *reinterpret_cast<const V*>(cy + (int64_t)cc[i] * p.d + j0);
            if constexpr (EDGE) vz[i] = *reinterpret_cast<const V*>(ef + (int64_t)ee[i] * p.d + j0);
            if constexpr (MODE == 2) sc[i] = pk[(int64_t)cc[i] * p.H + head];
        }
    };
    // three stages deep, as the GAT walks: rows of batch g consumed, rows of g+1 in flight, (scalar) indices of g+2 being fetched
    int e = e0;
    const int n_full = (e1 - e0) / U;
    int cA[U], rA[U], eA[U]; V xA[U], yA[U], zA[UE]; DotStat sA[U] = {};   // (the records: MODE 2 only, elsewhere they ride with the row)
    int cB[U], rB[U], eB[U];
    if (n_full > 0) { load_idx(e, cA, rA, eA); load_rows(cA, eA, xA, yA, zA, sA); }
    if (n_full > 1) load_idx(e + U, cB, rB, eB);
    for (int g = 0; g < n_full; ++g) {
        int cC[U], rC[U], eC[U]; V xB[U], yB[U], zB[UE]; DotStat sB[U];
        const bool more = g + 1 < n_full, more2 = g + 2 < n_full;
        if (more) load_rows(cB, eB, xB, yB, zB, sB);
        if (more2) load_idx(e + 2 * U, cC, rC, eC);
#pragma unroll
        for (int i = 0; i < U; ++i) consume(rA[i], eA[i], xA[i], yA[i], zA[EDGE ? i : 0], sA[i]);
        if (more) {
#pragma unroll
            for (int i = 0; i < U; ++i) {
                rA[i] = rB[i]; eA[i] = eB[i]; xA[i] = xB[i]; yA[i] = yB[i];
                if constexpr (EDGE) zA[i] = zB[i];
                if constexpr (MODE == 2) sA[i] = sB[i];
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
        const int ed = EDGE ? (has_eid ? eidp[e] : e) : (DROP ? eidp[e] : 0);
        V xv{}, yv{}, ev{}; DotStat sc{};
        if (act) {
            xv = *reinterpret_cast<const V*>(cx + (int64_t)cc * p.d + j0);
            yv = *reinterpret_cast<const V*>(cy + (int64_t)cc * p.d + j0);
            if constexpr (EDGE) ev = *reinterpret_cast<const V*>(ef + (int64_t)ed * p.d + j0);
            if constexpr (MODE == 2) sc = pk[(int64_t)cc * p.H + head];
        }
        consume(r, ed, xv, yv, ev, sc);
    }
    const bool tail_open = e1 < p.E && rowp[e1] == cur;
    if (head_open) store_partial(true);
    else if (tail_open) store_partial(false);
    else store_final(cur);
}

// merges the partials of the rows longer than a chunk, from the work list the flat kernel filled: the two passes, lists and merge
// order of gat_fixup_kernel (split_rows.hpp).  MODE 0: the associative softmax merge of (acc, m, s); MODE 1 / 2: sums of one / two
// vectors per column, the scale applied once at the end.
template <int VEC, bool LONG, int MODE>
__global__ __launch_bounds__(LONG ? kFixWaves * kWave : kBlock) void dot_fixup_kernel(DotParams p) {
    using V = FV<VEC>;
    constexpr int NW = LONG ? kFixWaves : 1;
    constexpr int PW = dot_partial_width(MODE);
    constexpr int NV = MODE == 2 ? 2 : 1;
    __shared__ float red_v[LONG ? kFixWaves : 1][NV][LONG ? kWave * VEC : 1];
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
        float m, s, acc[NV][VEC];                        // additive modes: s counts the partials merged (0: none)
        auto reset = [&]() {
            m = MODE == 0 ? -INFINITY : 0.f; s = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[i][k] = 0.f;
        };
        auto merge_vals = [&](const V& v0, const V& v1, float m2, float s2) {
            if constexpr (MODE == 0) {
                const float mn = fmaxf(m, m2);
                const float c1 = m == mn ? 1.f : expf(m - mn), c2 = m2 == mn ? 1.f : expf(m2 - mn);   // (both -inf: every edge so far masked)
                s = s * c1 + s2 * c2;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[0][k] = acc[0][k] * c1 + v0.v[k] * c2;
                m = mn;
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[0][k] += v0.v[k];
                if constexpr (NV == 2) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc[NV - 1][k] += v1.v[k];
                }
                s += s2;
            }
        };
        auto merge = [&](const float* base) {
            if constexpr (MODE == 0) merge_vals(*reinterpret_cast<const V*>(base + j0), V{}, base[p.d + j0], base[2 * p.d + j0]);
            else if constexpr (MODE == 2) merge_vals(*reinterpret_cast<const V*>(base + j0), *reinterpret_cast<const V*>(base + p.d + j0), 0.f, 1.f);
            else merge_vals(*reinterpret_cast<const V*>(base + j0), V{}, 0.f, 1.f);
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
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int k = 0; k < VEC; ++k) red_v[wib][i][lane * VEC + k] = acc[i][k];
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
                    V v0, v1{};
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        v0.v[k] = red_v[w][0][lane * VEC + k];
                        if constexpr (NV == 2) v1.v[k] = red_v[w][NV - 1][lane * VEC + k];
                    }
                    merge_vals(v0, v1, red_s[w][0][lane], s2);
                }
            }
        }
        if (!act || r >= p.out_rows) continue;
        V o;
        const float f = MODE == 0 ? 1.f / s : p.scale;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = acc[0][k] * f;
        *reinterpret_cast<V*>(p.out + (int64_t)r * p.d + j0) = o;
        if constexpr (MODE == 2) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = acc[NV - 1][k];
            *reinterpret_cast<V*>(p.out2 + (int64_t)r * p.d + j0) = o;
        }
        if (MODE == 0 && p.row_max && (j0 % p.D) == 0) { p.row_max[(int64_t)r * p.H + j0 / p.D] = m; p.row_sum[(int64_t)r * p.H + j0 / p.D] = s; }
    }
}

// t[v,h] = <g[v,h,:], out[v,h,:]> (the softmax-backward row term) with the destination's statistics, one 16-byte record per
// (node, head).  LANES = head_dim / 4 lanes share one pair: coalesced float4 reads, a DPP group sum, one 16-byte store (LANES = 0:
// one thread per pair).  A row without in-edges (sum 0) gets 1 / sum = 0; no edge reads its record.
template <int LANES>
__global__ __launch_bounds__(kBlock) void dot_pack_kernel(const float* __restrict__ m, const float* __restrict__ sm, const float* __restrict__ g,
                                                         const float* __restrict__ out, int64_t n, int D, DotStat* __restrict__ packed) {
    auto record = [&](int64_t i, float t) { const float s = sm[i]; return DotStat{m[i], s > 0.f ? 1.f / s : 0.f, t, 0.f}; };
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

// Host side.

static void dot_set_geometry(DotParams& p, int64_t heads, int64_t head_dim, float scale, float drop_p, uint32_t seed, int64_t num_edges,
                             int64_t num_nodes) {
    p.H = (int)heads; p.D = (int)head_dim; p.d = (int)(heads * head_dim); p.scale = scale;
    p.drop_p = drop_p; p.drop_scale = 1.f / (1.f - drop_p); p.seed = seed;
    p.E = (int)num_edges; p.chunk = chunk_edges_for(num_edges); p.n_chunks = (int)ceil_div(num_edges, p.chunk);
    p.out_rows = num_nodes; p.n_csr_rows = num_nodes;
}

template <int VEC, int MODE>
static int32_t launch_dot_fixups(const DotParams& p, hipStream_t st) {
    hipLaunchKernelGGL((dot_fixup_kernel<VEC, false, MODE>), dim3(fixup_grid_short(p.n_chunks, kFixGridShort, kWavesPerBlock)), dim3(kBlock), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((dot_fixup_kernel<VEC, true, MODE>), dim3(fixup_grid_long(p.n_chunks)), dim3(kFixWaves * kWave), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

// one walk and its fix-up; the workspace holds the partials of THIS walk (the walks of a backward run one after the other)
template <int MODE, bool EDGE = false>
static int32_t launch_dot(int vec, DotParams p, void* workspace, hipStream_t st) {
    SplitWs(p.n_chunks, (int64_t)dot_partial_width(MODE) * p.d, sizeof(float)).carve(p, workspace);
    return with_vec(vec, [&](auto v) {
        constexpr int VEC = decltype(v)::value;
        return launch_chunked_rows(p, st, [&](dim3 grid, const DotParams& q) {
            if (q.drop_p > 0.f) hipLaunchKernelGGL((dot_flat_kernel<VEC, MODE, true, EDGE>), grid, dim3(kBlock), 0, st, q);
            else hipLaunchKernelGGL((dot_flat_kernel<VEC, MODE, false, EDGE>), grid, dim3(kBlock), 0, st, q);
        }, [&](const DotParams& q) { return launch_dot_fixups<VEC, MODE>(q, st); });
    });
}

static const void* ptr_or(std::initializer_list<const void*> ps) {
    uintptr_t a = 0;
    for (const void* q : ps) a |= reinterpret_cast<uintptr_t>(q);
    return reinterpret_cast<const void*>(a);
}

}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_dot_attention_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim) {
    if (num_edges <= 0 || heads <= 0 || head_dim <= 0) return 256;
    const int64_t n_chunks = ceil_div(num_edges, chunk_edges_for(num_edges));
    return SplitWs(n_chunks, 3 * heads * head_dim, sizeof(float)).bytes() + 256;
}

extern "C" size_t pglamd_dot_attention_backward_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t heads, int64_t head_dim) {
    if (heads <= 0 || head_dim <= 0) return 256;
    return align_up((size_t)(num_nodes > 0 ? num_nodes : 1) * heads * sizeof(DotStat), 256) +
           pglamd_dot_attention_workspace_bytes(num_edges, heads, head_dim);
}

// the partials hold the same columns with and without the edge feature
extern "C" size_t pglamd_dot_attention_edge_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim) {
    return pglamd_dot_attention_workspace_bytes(num_edges, heads, head_dim);
}

extern "C" size_t pglamd_dot_attention_edge_backward_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t heads, int64_t head_dim) {
    return pglamd_dot_attention_backward_workspace_bytes(num_edges, num_nodes, heads, head_dim);
}

namespace pglamd {

// both forward entry points; EDGE: edge_feat [num_edges, heads, head_dim] is the third gathered operand
template <bool EDGE>
static int32_t dot_forward(const char* what, const float* q, const float* k, const float* v, const float* edge_feat, int64_t heads,
                           int64_t head_dim, float scale, float drop_p, uint32_t seed, const int32_t* row, const int32_t* col,
                           const int32_t* eid, const int64_t* indptr, int64_t num_edges, int64_t num_nodes, float* out, float* row_max,
                           float* row_sum, void* workspace, size_t workspace_bytes, void* stream) {
    if (!out || !indptr || heads <= 0 || head_dim <= 0 || num_nodes < 0 ||
        (num_edges > 0 && (!q || !k || !v || !row || !col || (EDGE && !edge_feat))))
        return fail(PGLAMD_E_ARG, "%s: bad argument", what);
    if ((row_max == nullptr) != (row_sum == nullptr)) return fail(PGLAMD_E_ARG, "%s: row_max/row_sum must both be given or both NULL", what);
    if (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && num_edges > 0 && !eid)) return fail(PGLAMD_E_ARG, "%s: dropout needs 0 <= p < 1 and eid", what);
    if (num_edges < 0 || num_edges > kMaxEdges || num_nodes >= INT32_MAX) return fail(PGLAMD_E_RANGE, "%s: sizes beyond int32 engine range", what);
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
    const int vec = gat_vec(heads, head_dim, ptr_or({q, k, v, edge_feat}), out, workspace, true);
    if (vec == 0 || heads > kWave)
        return fail(PGLAMD_E_SHAPE, "%s: heads*head_dim = %lld needs one 64-lane tile, head_dim/VEC a power of two and operands aligned to their lanes",
                    what, (long long)d);
    if (!workspace || workspace_bytes < pglamd_dot_attention_workspace_bytes(num_edges, heads, head_dim))
        return fail(PGLAMD_E_WORKSPACE, "%s: workspace too small", what);
    DotParams p{};
    dot_set_geometry(p, heads, head_dim, scale, drop_p, seed, num_edges, num_nodes);
    p.row_a = q; p.col_x = k; p.col_y = v; p.edge = edge_feat; p.out = out; p.row_max = row_max; p.row_sum = row_sum;
    p.row = row; p.col = col; p.eid = eid; p.indptr = indptr;
    return launch_dot<0, EDGE>(vec, p, workspace, st);
}

// both backward entry points; EDGE: both walks gather edge_feat, the src-sorted one writes grad_edge_feat (NULL: not wanted)
template <bool EDGE>
static int32_t dot_backward(const char* what, const float* grad_out, const float* q, const float* k, const float* v, const float* edge_feat,
                            const float* out, const float* row_max, const float* row_sum, int64_t heads, int64_t head_dim, float scale,
                            float drop_p, uint32_t seed, const int32_t* dst_row, const int32_t* dst_col, const int32_t* dst_eid,
                            const int64_t* dst_indptr, const int32_t* src_row, const int32_t* src_col, const int32_t* src_eid,
                            const int64_t* src_indptr, int64_t num_edges, int64_t num_nodes, float* grad_q, float* grad_k, float* grad_v,
                            float* grad_edge_feat, void* workspace, size_t workspace_bytes, void* stream) {
    if (heads <= 0 || head_dim <= 0 || num_nodes < 0 || num_edges < 0 || !grad_q || !grad_k || !grad_v ||
        (num_edges > 0 && (!grad_out || !q || !k || !v || !out || !row_max || !row_sum || !dst_row || !dst_col || !dst_indptr || !src_row ||
                           !src_col || !src_indptr || (EDGE && !edge_feat))))
        return fail(PGLAMD_E_ARG, "%s: bad argument", what);
    if (!(drop_p >= 0.f && drop_p < 1.f) || (drop_p > 0.f && num_edges > 0 && (!dst_eid || !src_eid)))
        return fail(PGLAMD_E_ARG, "%s: dropout needs 0 <= p < 1 and both eid arrays", what);
    if (num_edges > kMaxEdges || num_nodes >= INT32_MAX) return fail(PGLAMD_E_RANGE, "%s: sizes beyond int32 engine range", what);
    const int64_t d = heads * head_dim;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_nodes == 0) return PGLAMD_OK;
    if (num_edges == 0) {
        for (float* gp : {grad_q, grad_k, grad_v}) PGLAMD_HIP_CHECK(hipMemsetAsync(gp, 0, (size_t)num_nodes * d * sizeof(float), st));
        return PGLAMD_OK;
    }
    const int vec = gat_vec(heads, head_dim, ptr_or({grad_out, q, k, v, edge_feat}), ptr_or({grad_q, grad_k, grad_v, grad_edge_feat}), nullptr, true);
    if (vec == 0 || heads > kWave || reinterpret_cast<uintptr_t>(workspace) % 256 ||
        (head_dim % 4 == 0 && (reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(grad_out)) % 16))
        return fail(PGLAMD_E_SHAPE, "%s: heads*head_dim = %lld needs one 64-lane tile, head_dim/VEC a power of two and operands aligned to their lanes",
                    what, (long long)d);
    if (!workspace || workspace_bytes < pglamd_dot_attention_backward_workspace_bytes(num_edges, num_nodes, heads, head_dim))
        return fail(PGLAMD_E_WORKSPACE, "%s: workspace too small", what);
    // (0) the destination-side scalars of every (node, head), packed so that an edge fetches them with one 16-byte load
    const size_t pack_bytes = align_up((size_t)num_nodes * heads * sizeof(DotStat), 256);
    DotStat* packed = static_cast<DotStat*>(workspace);
    workspace = static_cast<char*>(workspace) + pack_bytes;
    {
        const int64_t pairs = num_nodes * heads;
        const int lanes = (head_dim % 4 == 0 && head_dim / 4 <= 16 && ((head_dim / 4) & (head_dim / 4 - 1)) == 0) ? (int)(head_dim / 4) : 0;
#define PGLAMD_PACK(L) hipLaunchKernelGGL(dot_pack_kernel<L>, dim3((unsigned)ceil_div(pairs * (L ? L : 1), kBlock)), dim3(kBlock), 0, st, \
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
    DotParams p{};
    dot_set_geometry(p, heads, head_dim, scale, drop_p, seed, num_edges, num_nodes);
    p.packed = packed; p.edge = edge_feat; p.grad_edge = grad_edge_feat;
    // (1) dst-sorted walk: row = v carries q[v], g[v] and its record; gathers k[u], v[u] (and ef_e); writes dq[v]
    DotParams a = p;
    a.row = dst_row; a.col = dst_col; a.eid = dst_eid; a.indptr = dst_indptr;
    a.row_a = q; a.row_b = grad_out; a.col_x = k; a.col_y = v; a.out = grad_q;
    PGLAMD_TRY((launch_dot<1, EDGE>(vec, a, workspace, st)));
    // (2) src-sorted walk: row = u carries k[u], v[u]; gathers q[v], g[v] and v's record (and ef_e); writes dk[u], dv[u] (and def[e])
    p.row = src_row; p.col = src_col; p.eid = src_eid; p.indptr = src_indptr;
    p.row_a = k; p.row_b = v; p.col_x = q; p.col_y = grad_out; p.out = grad_k; p.out2 = grad_v;
    return launch_dot<2, EDGE>(vec, p, workspace, st);
}

}  // namespace pglamd

extern "C" int32_t pglamd_dot_attention(const float* q, const float* k, const float* v, int64_t heads, int64_t head_dim, float scale,
                                        float drop_p, uint32_t seed, const int32_t* row, const int32_t* col, const int32_t* eid,
                                        const int64_t* indptr, int64_t num_edges, int64_t num_nodes, float* out, float* row_max,
                                        float* row_sum, void* workspace, size_t workspace_bytes, void* stream) {
    return dot_forward<false>("dot_attention", q, k, v, nullptr, heads, head_dim, scale, drop_p, seed, row, col, eid, indptr, num_edges,
                              num_nodes, out, row_max, row_sum, workspace, workspace_bytes, stream);
}

extern "C" int32_t pglamd_dot_attention_edge(const float* q, const float* k, const float* v, const float* edge_feat, int64_t heads,
                                             int64_t head_dim, float scale, float drop_p, uint32_t seed, const int32_t* row,
                                             const int32_t* col, const int32_t* eid, const int64_t* indptr, int64_t num_edges,
                                             int64_t num_nodes, float* out, float* row_max, float* row_sum, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    return dot_forward<true>("dot_attention_edge", q, k, v, edge_feat, heads, head_dim, scale, drop_p, seed, row, col, eid, indptr, num_edges,
                             num_nodes, out, row_max, row_sum, workspace, workspace_bytes, stream);
}

extern "C" int32_t pglamd_dot_attention_backward(const float* grad_out, const float* q, const float* k, const float* v, const float* out,
                                                 const float* row_max, const float* row_sum, int64_t heads, int64_t head_dim, float scale,
                                                 float drop_p, uint32_t seed, const int32_t* dst_row, const int32_t* dst_col,
                                                 const int32_t* dst_eid, const int64_t* dst_indptr, const int32_t* src_row,
                                                 const int32_t* src_col, const int32_t* src_eid, const int64_t* src_indptr,
                                                 int64_t num_edges, int64_t num_nodes, float* grad_q, float* grad_k, float* grad_v,
                                                 void* workspace, size_t workspace_bytes, void* stream) {
    return dot_backward<false>("dot_attention_backward", grad_out, q, k, v, nullptr, out, row_max, row_sum, heads, head_dim, scale, drop_p, seed,
                               dst_row, dst_col, dst_eid, dst_indptr, src_row, src_col, src_eid, src_indptr, num_edges, num_nodes, grad_q,
                               grad_k, grad_v, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int32_t pglamd_dot_attention_edge_backward(const float* grad_out, const float* q, const float* k, const float* v,
                                                      const float* edge_feat, const float* out, const float* row_max, const float* row_sum,
                                                      int64_t heads, int64_t head_dim, float scale, float drop_p, uint32_t seed,
                                                      const int32_t* dst_row, const int32_t* dst_col, const int32_t* dst_eid,
                                                      const int64_t* dst_indptr, const int32_t* src_row, const int32_t* src_col,
                                                      const int32_t* src_eid, const int64_t* src_indptr, int64_t num_edges,
                                                      int64_t num_nodes, float* grad_q, float* grad_k, float* grad_v,
                                                      float* grad_edge_feat, void* workspace, size_t workspace_bytes, void* stream) {
    return dot_backward<true>("dot_attention_edge_backward", grad_out, q, k, v, edge_feat, out, row_max, row_sum, heads, head_dim, scale, drop_p,
                              seed, dst_row, dst_col, dst_eid, dst_indptr, src_row, src_col, src_eid, src_indptr, num_edges, num_nodes,
                              grad_q, grad_k, grad_v, grad_edge_feat, workspace, workspace_bytes, stream);
}
