// gat_fused.hpp -- the kernels and launchers of the fused GAT attention (description: gat_fused.hip), templated on the STORAGE type T
// of the row operands.  gat_fused.hip instantiates T = float, gat_fused_16.hip T = __half and __hip_bfloat16.
//
// Stored as T: the gathered rows (feature, grad_out), the row node's own vector, and the rows written (out, out_pos, grad_feature).
// Everything else is fp32 for every T: the per-(node, head) scalars (attn_*, row_max, row_sum, sum_pos, grad_attn_*, grad_pre), the
// packed F4 records, every accumulator and the split-row partials in the workspace.  A stored value is converted when it is loaded
// (to_acc, aggregate.hpp) and a result is rounded to T ONCE, on its final store (from_acc: to nearest even) -- a row split over
// chunks after the fix-up has merged its fp32 partials.  The geometry does not depend on T: a lane owns VEC elements by the rule of
// gat_vec (its alignment unit is sizeof(T) * VEC), the edge order, the chunk size, the batch width, the online-softmax update and the
// merge order are the fp32 ones, so a 16-bit call computes the fp32 call's values on the up-cast operands and rounds them.
#pragma once
#include "aggregate.hpp"
#include "attention_common.hpp"

#include <algorithm>

namespace pglamd {

struct alignas(16) F4 { float a, m, s, t; };       // per (node, head): a_dst, softmax max, 1 / softmax sum, <g, out>

template <typename T>
struct GatParamsT {
    const T* x;                     // gathered by col: f (forward) or g = dL/dout (backward-feature)
    const float* p_col;             // per-col scalar [*,H]: a_src (forward) / a_dst (backward-feature)
    const float* p_row;             // per-row scalar [*,H]: a_dst (forward) / a_src (backward-feature)
    const float* stat_m; const float* stat_s;   // backward: softmax statistics of the dst node [N,H]
    T* out;
    float* row_max; float* row_sum;             // forward: optional statistics output [out_rows,H]
    T* out_pos; float* sum_pos;                 // forward, optional (training): out restricted to the edges with pre_e > 0 [out_rows,d], their softmax mass [out_rows,H]
    const int* row; const int* col; const int* eid; const int64_t* indptr;
    float* part_head; float* part_tail;         // [n_chunks, 3, d]: acc | m | s (forward) ; [n_chunks, d] (backward)
    int* long_count; int* long_list; int* long_list2;
    int64_t out_rows, n_csr_rows;
    int E, n_chunks, chunk, n_blocks, n_grid_chunks;
    int d, H, D;
    float slope, drop_p, drop_scale;
    unsigned seed;
    // backward with attention gradients (MODE 2 / 3)
    const T* row_vec;               // the row node's own vector: f[u] (MODE 2) / g[v] (MODE 3)
    const F4* packed;               // [N,H] (a_dst, m, 1/s, t) of every node as a destination
    float* out_a;                   // [out_rows,H] d a_src (MODE 2) / d a_dst (MODE 3)
    // sddmm / additive score
    const float* f; const float* g; float* dpre;
    const float* w;                 // [H*D] score weights (additive score)
    const float* ge; float* part_w; // additive-score backward: upstream gradient [E,H]; per-chunk partials of d/dw [n_chunks, H*D]
};
using GatParams = GatParamsT<float>;

// VEC stored elements of one lane as they travel: the raw bits while a load is in flight, fp32 once consumed
template <typename T, int VEC> struct RowVec { using type = VecT<T, VEC>; };
template <int VEC> struct RowVec<float, VEC> { using type = FV<VEC>; };
template <typename T, int VEC> __device__ __forceinline__ typename RowVec<T, VEC>::type load_raw(const T* p) {
    return *reinterpret_cast<const typename RowVec<T, VEC>::type*>(p);
}
template <int VEC> __device__ __forceinline__ const FV<VEC>& widen(const FV<VEC>& r) { return r; }
template <typename T, int VEC> __device__ __forceinline__ FV<VEC> widen(const VecT<T, VEC>& r) {
    FV<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = to_acc(r.v[k]);
    return o;
}
// the final store of a row: the one rounding to T
template <typename T, int VEC> __device__ __forceinline__ void store_row(T* p, const FV<VEC>& v) {
    if constexpr (std::is_same_v<T, float>) {
        *reinterpret_cast<FV<VEC>*>(p) = v;
    } else {
        // The value to round is the fp32 one, as the fp32 kernel computes it.  Left to itself the compiler fuses the last fp32 operation
        // (acc * 1 / s) with the conversion into one v_fma_mixlo_f16, which rounds the exact product to 16 bits: another result than
        // the fp32 kernel's, rounded, where the product lies within an fp32 rounding of a 16-bit tie.  The empty statement pins the
        // fp32 values in registers -- as ONE vector of VEC floats, the shape of the fp32 kernel's own store: the vectoriser grows its
        // trees from that shape, and which multiply-adds of the merge loops above it end up fused follows from those trees.
        VecT<T, VEC> o;
        if constexpr (VEC == 1) {
            float r = v.v[0];
            asm("" : "+v"(r));
            o.v[0] = from_acc<T>(r);
        } else {
            typedef float FN __attribute__((ext_vector_type(VEC)));
            FN r;
#pragma unroll
            for (int k = 0; k < VEC; ++k) r[k] = v.v[k];
            asm("" : "+v"(r));
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = from_acc<T>(r[k]);
        }
        *reinterpret_cast<VecT<T, VEC>*>(p) = o;
    }
}

// MODE 0: forward (online softmax).  MODE 1: backward w.r.t. features only (additive, alpha recomputed).
// MODE 2: MODE 1 + d a_src over the src-sorted stream.  MODE 3: d a_dst over the dst-sorted stream (no feature output).
// POS (forward only): also accumulate the part of the row that comes from edges with pre_e > 0 (out_pos, and its softmax mass
// sum_pos).  With them the backward gets d a_dst[v,h] = sum_e d pre_e WITHOUT any per-edge pass:
//     sum_e alpha_e l'_e (drop_e <g,f_u> - t) = <g, out_pos> + slope <g, out - out_pos> - t (s_pos + slope (1 - s_pos)),
// l'_e = 1 where pre_e > 0 and slope elsewhere -- a per-(node, head) formula evaluated in the pack kernel.  It replaces the
// [E,H] d pre buffer of round 1 (0.64 GB written by the src-sorted walk, gathered back through a permutation by a 0.51 ms
// segment sum) by one more [N, H*D] row written per destination in the forward.
template <typename T, int VEC, int MODE, bool DROP, bool POS = false>
// (MODE 2 needs 106 VGPRs = 4 waves per SIMD against the forward's 68 = 7.  Forcing 5 / 6 waves with amdgpu_waves_per_eu makes the
//  compiler spill 11 / 32 VGPRs into the hot loop: fwd + bwd 5.09 -> 5.43 / 10.0 ms at C3, profiles/r04/gat_backward_occupancy_variants.txt.)
__global__ __launch_bounds__(kBlock) void gat_flat_kernel(GatParamsT<T> p) {
#ifndef PGLAMD_GAT_ATT_U
#define PGLAMD_GAT_ATT_U 4                                  // edges per batch of the attention-gradient walks (variant builds: 3, 2)
#endif
    constexpr int U = MODE >= 2 ? PGLAMD_GAT_ATT_U : 4;
    constexpr int PW = MODE == 0 ? (POS ? 5 : 3) : MODE == 2 ? 2 : 1;   // floats per column in a partial
    constexpr bool ATT = MODE >= 2;                     // accumulates the attention-score gradient of the row node
    constexpr bool FEAT = MODE != 3;                    // accumulates / writes a feature row
    using V = FV<VEC>;
    using R = typename RowVec<T, VEC>::type;            // a gathered row's share of this lane, as stored
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform(threadIdx.x >> 6);
    const int j0 = lane * VEC;
    const bool act = j0 < p.d;
    const int head = act ? j0 / p.D : 0;
    const int lph = p.D / VEC;                          // lanes per head (a power of two when ATT)

    if ((int)blockIdx.x >= p.n_grid_chunks) {
        zero_fill_role(p, lane, wib, [&](int64_t r) {
            if (FEAT && act) store_row<T, VEC>(p.out + r * p.d + j0, V{});
            if (ATT && lane < p.H) p.out_a[r * p.H + lane] = 0.f;
            if (MODE == 0 && p.row_max && lane < p.H) { p.row_max[r * p.H + lane] = 0.f; p.row_sum[r * p.H + lane] = 0.f; }
            if constexpr (POS) {
                if (act) store_row<T, VEC>(p.out_pos + r * p.d + j0, V{});
                if (lane < p.H) p.sum_pos[r * p.H + lane] = 0.f;
            }
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
    const T* __restrict__ x = p.x;
    const float* __restrict__ pcol = p.p_col;
    const float* __restrict__ prow = p.p_row;
    const float* __restrict__ sm = p.stat_m;
    const float* __restrict__ ss = p.stat_s;
    const float slope = p.slope;
    constexpr bool drop = DROP;
    const bool need_eid = drop;                                   // original edge ids only feed the dropout hash

    float m = -INFINITY, s = 0.f, acc[VEC], acc_a = 0.f;
    float accp[POS ? VEC : 1], sp = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
    for (int k = 0; k < (POS ? VEC : 1); ++k) accp[k] = 0.f;
    int cur = rowp[e0];
    bool head_open = e0 > 0 && rowp[e0 - 1] == cur;

    auto store_partial = [&](bool headp) {
        if (act) {
            float* dst = (headp ? p.part_head : p.part_tail) + (int64_t)c * PW * p.d;
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = FEAT ? acc[k] : acc_a;
            *reinterpret_cast<V*>(dst + j0) = o;
            if constexpr (MODE == 2) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = acc_a;
                *reinterpret_cast<V*>(dst + p.d + j0) = o;
            }
            if constexpr (MODE == 0) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = m;
                *reinterpret_cast<V*>(dst + p.d + j0) = o;
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = s;
                *reinterpret_cast<V*>(dst + 2 * p.d + j0) = o;
                if constexpr (POS) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) o.v[k] = accp[k];
                    *reinterpret_cast<V*>(dst + 3 * p.d + j0) = o;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) o.v[k] = sp;
                    *reinterpret_cast<V*>(dst + 4 * p.d + j0) = o;
                }
            }
        }
        if (!headp && lane == 0) p.long_list[atomicAdd(p.long_count, 1)] = c;
    };
    auto store_final = [&](int r) {
        if (r >= p.out_rows || !act) return;
        if constexpr (ATT) { if ((j0 % p.D) == 0) p.out_a[(int64_t)r * p.H + head] = acc_a; }
        if constexpr (!FEAT) return;
        V o;
        const float inv = MODE == 0 ? 1.f / s : 1.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = acc[k] * inv;
        store_row<T, VEC>(p.out + (int64_t)r * p.d + j0, o);
        if (MODE == 0 && p.row_max && (j0 % p.D) == 0) { p.row_max[(int64_t)r * p.H + head] = m; p.row_sum[(int64_t)r * p.H + head] = s; }
        if constexpr (POS) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = accp[k] * inv;
            store_row<T, VEC>(p.out_pos + (int64_t)r * p.d + j0, o);
            if ((j0 % p.D) == 0) p.sum_pos[(int64_t)r * p.H + head] = sp * inv;
        }
    };
    // the row node's scalar is fetched (asynchronously, with the batch) only for edges that may OPEN a row and held
    // in a register until the next row change: no stall on the change, no per-edge reload either.
    float vr_held = act ? prow[(int64_t)cur * p.H + head] : 0.f;
    auto consume = [&](int r, int ed, float vc, float vr, float vm, float vs, const R& xr) {
        if (r != cur) {
            if (head_open) store_partial(true); else store_final(cur);
            head_open = false;
            cur = r;
            m = -INFINITY; s = 0.f; acc_a = 0.f; sp = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int k = 0; k < (POS ? VEC : 1); ++k) accp[k] = 0.f;
            vr_held = vr;
        }
        const V xv = widen(xr);
        const float pre = vc + vr_held;
        const float l = pre > 0.f ? pre : slope * pre;
        const float df = drop ? drop_factor(p.seed, ed, head, p.drop_p, p.drop_scale) : 1.f;
        if constexpr (MODE == 0) {
            // online softmax: one of exp(m - mn), exp(l - mn) is always exp(0) = 1, so ONE exponential per edge
            // Special values: a -inf logit (a masked edge) weighs 0 and leaves (m, s) alone -- also while m is still
            // -inf, where l - m is NaN; a +inf logit makes the row NaN, as exp(inf - inf) does in the three-pass definition
            const float dlt = l - m;                 // +inf on the first edge of a row (m = -inf): e^{-inf} = 0
            const float ed2 = l == -INFINITY ? 0.f : expf(-fabsf(dlt));
            const bool up = dlt > 0.f;
            const float sc = up ? ed2 : 1.f, pe = l == INFINITY ? NAN : (up ? 1.f : ed2);
            s = s * sc + pe;
            const float w = pe * df;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * sc + w * xv.v[k];
            if constexpr (POS) {
                const float pp = pre > 0.f ? 1.f : 0.f;
                sp = sp * sc + pe * pp;
                const float wp = w * pp;
#pragma unroll
                for (int k = 0; k < VEC; ++k) accp[k] = accp[k] * sc + wp * xv.v[k];
            }
            m = up ? l : m;
        } else {
            const float alpha = expf(l - vm) / vs;   // alpha_e of the destination's softmax, recomputed
            if constexpr (FEAT) {
                const float w = alpha * df;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += w * xv.v[k];
            }
        }
    };
    const T* __restrict__ rvec = p.row_vec;
    auto load_idx = [&](int e, int (&cc)[U], int (&rr)[U], int (&ee)[U]) {
#pragma unroll
        for (int i = 0; i < U; ++i) { rr[i] = rowp[e + i]; cc[i] = colp[e + i]; ee[i] = need_eid ? eidp[e + i] : 0; }
    };
    // the destination's statistics (and t) are indexed by col on the src-sorted stream, by row on the dst-sorted one
    auto load_rows = [&](const int (&cc)[U], const int (&rr)[U], R (&vx)[U], float (&vc)[U], float (&vr)[U], float (&vm)[U], float (&vs)[U]) {
#pragma unroll
        for (int i = 0; i < U; ++i)
            if (act) {
                vx[i] = load_raw<T, VEC>(x + (int64_t)cc[i] * p.d + j0);
                vc[i] = pcol[(int64_t)cc[i] * p.H + head];
                if (i == 0 || rr[i] != rr[i - 1]) vr[i] = prow[(int64_t)rr[i] * p.H + head];   // only where a row may open
                if constexpr (MODE >= 1) {
                    const int64_t si = (int64_t)(MODE == 3 ? rr[i] : cc[i]) * p.H + head;
                    vm[i] = sm[si]; vs[i] = ss[si];
                }
            }
    };

    int e = e0;
    const int n_full = (e1 - e0) / U;
    if constexpr (!ATT) {
        // three stages deep, as in agg_flat_kernel: rows of batch g consumed, rows of g+1 in flight, (scalar) indices of
        // g+2 being fetched -- the scalar-load latency is off the per-batch critical path
        int cA[U], rA[U], eA[U]; R xA[U]; float vcA[U], vrA[U], vmA[U], vsA[U];
        int cB[U], rB[U], eB[U];
        if (n_full > 0) { load_idx(e, cA, rA, eA); load_rows(cA, rA, xA, vcA, vrA, vmA, vsA); }
        if (n_full > 1) load_idx(e + U, cB, rB, eB);
        for (int g = 0; g < n_full; ++g) {
            int cC[U], rC[U], eC[U]; R xB[U]; float vcB[U], vrB[U], vmB[U], vsB[U];
            const bool more = g + 1 < n_full, more2 = g + 2 < n_full;
            if (more) load_rows(cB, rB, xB, vcB, vrB, vmB, vsB);
            if (more2) load_idx(e + 2 * U, cC, rC, eC);
#pragma unroll
            for (int i = 0; i < U; ++i) consume(rA[i], eA[i], vcA[i], vrA[i], vmA[i], vsA[i], xA[i]);
            if (more) {
#pragma unroll
                for (int i = 0; i < U; ++i) {
                    rA[i] = rB[i]; eA[i] = eB[i]; xA[i] = xB[i]; vcA[i] = vcB[i]; vrA[i] = vrB[i];
                    if constexpr (MODE >= 1) { vmA[i] = vmB[i]; vsA[i] = vsB[i]; }
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
            const int ed = drop ? eidp[e] : 0;
            R xv{}; float vc = 0.f, vr = 0.f, vm = 0.f, vs = 1.f;
            if (act) {
                xv = load_raw<T, VEC>(x + (int64_t)cc * p.d + j0);
                vc = pcol[(int64_t)cc * p.H + head];
                vr = prow[(int64_t)r * p.H + head];
                if constexpr (MODE >= 1) {
                    const int64_t si = (int64_t)(MODE == 3 ? r : cc) * p.H + head;
                    vm = sm[si]; vs = ss[si];
                }
            }
            consume(r, ed, vc, vr, vm, vs, xv);
        }
    } else {
        // Attention-gradient walks.  The destination's four per-head scalars come PACKED (a_dst, m, s, t: one 16-byte
        // load); what belongs to the row node itself (its vector, and a_src[u] resp. the packed scalars of v) is fetched
        // only for edges that OPEN a row inside the batch and held in registers until the next row change -- on a
        // power-law graph most edges continue a row, so an edge costs two vector loads, not seven.
        const F4* __restrict__ pk = p.packed;
        float* __restrict__ dpre_out = p.dpre;
        V y_held{}; F4 p_held{}; float a_held = 0.f;
        if (act) {
            y_held = widen(load_raw<T, VEC>(rvec + (int64_t)cur * p.d + j0));
            if constexpr (MODE == 2) a_held = prow[(int64_t)cur * p.H + head];
            else p_held = pk[(int64_t)cur * p.H + head];
        }
        // Round 5: what belongs to the ROW node is no longer prefetched per batch element "in case this edge opens a row" (three to
        // seven VGPRs per element and stage: 106 VGPRs = 4 waves per SIMD) but fetched at the row change itself -- a row change
        // happens once per ~19 edges at C3, the fetch is a vector load of consecutive rows (the walk's own row order), and the 24
        // registers it frees buy two more resident waves per SIMD.
        auto open_row = [&](int r) {
            if (!act) return;
            y_held = widen(load_raw<T, VEC>(rvec + (int64_t)r * p.d + j0));
            if constexpr (MODE == 2) a_held = prow[(int64_t)r * p.H + head];
            else p_held = pk[(int64_t)r * p.H + head];
        };
        auto consume_att = [&](int r, int ed, int pos, const R& xr, const F4& pc, float ac) {
            if (r != cur) {
                if (head_open) store_partial(true); else store_final(cur);
                head_open = false;
                cur = r;
                acc_a = 0.f;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
                open_row(r);
            }
            const V xv = widen(xr);
            const F4 q = MODE == 2 ? pc : p_held;                  // (a_dst, m, s, t) of the destination v
            const float pre = q.a + (MODE == 2 ? a_held : ac);     // + a_src[u]
            const float l = pre > 0.f ? pre : slope * pre;
            const float df = drop ? drop_factor(p.seed, ed, head, p.drop_p, p.drop_scale) : 1.f;
            const float alpha = __expf(l - q.m) * q.s;              // q.s = 1 / softmax sum; hardware exp2 (rel. error < 1e-6 where alpha is not negligible): gradients only
            if constexpr (FEAT) {
                const float w = alpha * df;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += w * xv.v[k];
            }
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) dot += xv.v[k] * y_held.v[k];       // <g[v], f[u]> restricted to this lane
            dot = group_sum(dot, lph);
            const float dl = alpha * (df * dot - q.t);
            const float dp = pre > 0.f ? dl : slope * dl;
            acc_a += dp;
            // [E,H] in the order of THIS walk (sequential 32-byte rows; written in original edge order it was one more random
            // line per edge, and the caller's reduction by destination gathers through a permutation either way)
            if (dpre_out && (lane & (lph - 1)) == 0 && act) dpre_out[(int64_t)pos * p.H + head] = dp;
        };
        auto load_att = [&](const int (&cc)[U], R (&vx)[U], F4 (&pc)[U], float (&ac)[U]) {
            if (!act) return;
#pragma unroll
            for (int i = 0; i < U; ++i) {
                vx[i] = load_raw<T, VEC>(x + (int64_t)cc[i] * p.d + j0);
                if constexpr (MODE == 2) pc[i] = pk[(int64_t)cc[i] * p.H + head];
                else ac[i] = pcol[(int64_t)cc[i] * p.H + head];
            }
        };
        // three stages deep, as the forward walk: rows of batch g consumed, rows of g+1 in flight, (scalar) indices of g+2 being fetched
        int cA[U], rA[U], eA[U]; R xA[U]; F4 pcA[U]; float acA[U];
        int cB[U], rB[U], eB[U];
        if (n_full > 0) { load_idx(e, cA, rA, eA); load_att(cA, xA, pcA, acA); }
        if (n_full > 1) load_idx(e + U, cB, rB, eB);
        for (int g = 0; g < n_full; ++g) {
            int cC[U], rC[U], eC[U]; R xB[U]; F4 pcB[U]; float acB[U];
            const bool more = g + 1 < n_full, more2 = g + 2 < n_full;
            if (more) load_att(cB, xB, pcB, acB);
            if (more2) load_idx(e + 2 * U, cC, rC, eC);
#pragma unroll
            for (int i = 0; i < U; ++i) consume_att(rA[i], eA[i], e + i, xA[i], pcA[i], acA[i]);
            if (more) {
#pragma unroll
                for (int i = 0; i < U; ++i) {
                    rA[i] = rB[i]; eA[i] = eB[i]; xA[i] = xB[i];
                    if constexpr (MODE == 2) pcA[i] = pcB[i]; else acA[i] = acB[i];
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
            const int ed = need_eid ? eidp[e] : 0;
            R xv{}; F4 pc{}; float ac = 0.f;
            if (act) {
                xv = load_raw<T, VEC>(x + (int64_t)cc * p.d + j0);
                if constexpr (MODE == 2) pc = pk[(int64_t)cc * p.H + head];
                else ac = pcol[(int64_t)cc * p.H + head];
            }
            consume_att(r, ed, e, xv, pc, ac);
        }
    }
    const bool tail_open = e1 < p.E && rowp[e1] == cur;
    if (head_open) store_partial(true);
    else if (tail_open) store_partial(false);
    else store_final(cur);
}

// merges the partials of the rows longer than a chunk (only those are split), from the work list
// the flat kernel filled.  Pass 1 (LONG = false): one wave per task, rows with <= kFixShort further
// pieces are merged right there, longer ones (fixup_is_long) go to a second list.  Pass 2 (LONG = true):
// blocks of kFixWaves waves split one hub row's partial list, LDS combine in wave order.  Every row's
// own merge order is fixed => bit-reproducible.  Classes, block shapes and grids: split_rows.hpp.
// The partials are fp32 for every T: the merged row is rounded to T on its store here, never before.
template <typename T, int VEC, bool LONG, int MODE, bool POS = false>
__global__ __launch_bounds__(LONG ? kFixWaves * kWave : kBlock) void gat_fixup_kernel(GatParamsT<T> p) {
    using V = FV<VEC>;
    constexpr int NW = LONG ? kFixWaves : 1;
    constexpr int PW = MODE == 0 ? (POS ? 5 : 3) : MODE == 2 ? 2 : 1;
    // per-wave results of the LONG pass: the vectors (acc, and accp when POS) are VEC wide per lane, the scalars (m, s, sp)
    // are one value per lane -- kept apart so that VEC = 4 with POS stays under 64 KiB of LDS
    __shared__ float red_v[LONG ? kFixWaves : 1][POS ? 2 : 1][LONG ? kWave * VEC : 1];
    __shared__ float red_s[LONG ? kFixWaves : 1][3][LONG ? kWave : 1];
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
        float m = MODE == 0 ? -INFINITY : 0.f, s = 0.f, sp = 0.f, acc[VEC], accp[POS ? VEC : 1];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
        for (int k = 0; k < (POS ? VEC : 1); ++k) accp[k] = 0.f;
        auto merge_vals = [&](const V& va, float m2, float s2, const V& vp, float sp2) {
            if constexpr (MODE == 0) {
                const float mn = fmaxf(m, m2);
                const float c1 = m == mn ? 1.f : expf(m - mn), c2 = m2 == mn ? 1.f : expf(m2 - mn);   // (both -inf: every edge so far masked)
                s = s * c1 + s2 * c2;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * c1 + va.v[k] * c2;
                if constexpr (POS) {
                    sp = sp * c1 + sp2 * c2;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) accp[k] = accp[k] * c1 + vp.v[k] * c2;
                }
                m = mn;
            } else {                                   // additive modes: `m` doubles as the second component (MODE 2)
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += va.v[k];
                m += m2;
                s = 1.f;
            }
        };
        auto merge = [&](const float* base) {
            if constexpr (MODE == 0) {
                V vp{}; float sp2 = 0.f;
                if constexpr (POS) { vp = *reinterpret_cast<const V*>(base + 3 * p.d + j0); sp2 = base[4 * p.d + j0]; }
                merge_vals(*reinterpret_cast<const V*>(base + j0), base[p.d + j0], base[2 * p.d + j0], vp, sp2);
            } else if constexpr (MODE == 2) merge_vals(*reinterpret_cast<const V*>(base + j0), base[p.d + j0], 1.f, V{}, 0.f);
            else merge_vals(*reinterpret_cast<const V*>(base + j0), 0.f, 1.f, V{}, 0.f);
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
            for (int k = 0; k < VEC; ++k) {
                red_v[wib][0][lane * VEC + k] = acc[k];
                if constexpr (POS) red_v[wib][1][lane * VEC + k] = accp[k];
            }
            red_s[wib][0][lane] = m; red_s[wib][1][lane] = s; red_s[wib][2][lane] = sp;
            __syncthreads();
            if (wib != 0) continue;
            // wave 0: tail partial of chunk a first, then the wave results in wave order
            m = MODE == 0 ? -INFINITY : 0.f; s = 0.f; sp = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int k = 0; k < (POS ? VEC : 1); ++k) accp[k] = 0.f;
            if (act) {
                merge(p.part_tail + (int64_t)a * PW * p.d);
                for (int w = 0; w < NW; ++w) {
                    const float s2 = red_s[w][1][lane];
                    if (s2 == 0.f) continue;                     // that wave had no partial
                    V va, vp{};
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        va.v[k] = red_v[w][0][lane * VEC + k];
                        if constexpr (POS) vp.v[k] = red_v[w][1][lane * VEC + k];
                    }
                    merge_vals(va, red_s[w][0][lane], s2, vp, red_s[w][2][lane]);
                }
            }
        }
        if (!act || r >= p.out_rows) continue;
        if constexpr (MODE == 2) { if ((j0 % p.D) == 0) p.out_a[(int64_t)r * p.H + j0 / p.D] = m; }
        if constexpr (MODE == 3) { if ((j0 % p.D) == 0) p.out_a[(int64_t)r * p.H + j0 / p.D] = acc[0]; continue; }
        V o;
        const float inv = MODE == 0 ? 1.f / s : 1.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = acc[k] * inv;
        store_row<T, VEC>(p.out + (int64_t)r * p.d + j0, o);
        if (MODE == 0 && p.row_max && (j0 % p.D) == 0) { p.row_max[(int64_t)r * p.H + j0 / p.D] = m; p.row_sum[(int64_t)r * p.H + j0 / p.D] = s; }
        if constexpr (POS) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = accp[k] * inv;
            store_row<T, VEC>(p.out_pos + (int64_t)r * p.d + j0, o);
            if ((j0 % p.D) == 0) p.sum_pos[(int64_t)r * p.H + j0 / p.D] = sp * inv;
        }
    }
}

// t[v,h] = <g[v,h,:], out[v,h,:]> (the softmax-backward row term) and the destination-side scalars of every
// (node, head), packed so that an edge fetches them with one 16-byte load.  LANES = head_dim / 4 lanes share one
// (node, head): fully coalesced reads of four elements (16 bytes of fp32, 8 of a 16-bit T), a DPP group sum, one 16-byte
// store (LANES = 0: one thread per pair).
template <typename T, int LANES>
__global__ __launch_bounds__(kBlock) void gat_pack_kernel(const float* __restrict__ a_dst, const float* __restrict__ m,
                                                         const float* __restrict__ sm, const T* __restrict__ g,
                                                         const T* __restrict__ out, int64_t n, int D,
                                                         F4* __restrict__ packed, const T* __restrict__ out_pos,
                                                         const float* __restrict__ sum_pos, float slope,
                                                         float* __restrict__ grad_a_dst) {
    // with the forward's positive-part statistics the attention-score gradient of the DESTINATION is a per-(node, head)
    // formula (see gat_flat_kernel, POS): u = <g, out_pos>, t = <g, out>  =>  d a_dst = u + slope (t - u) - t (sp + slope (1 - sp))
    auto d_adst = [&](float t, float u, float spv) { return u + slope * (t - u) - t * (spv + slope * (1.f - spv)); };
    if constexpr (LANES == 0) {
        const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (i >= n) return;
        float t = 0.f, u = 0.f;
        for (int k = 0; k < D; ++k) { t += to_acc(g[i * D + k]) * to_acc(out[i * D + k]); if (out_pos) u += to_acc(g[i * D + k]) * to_acc(out_pos[i * D + k]); }
        packed[i] = F4{a_dst[i], m[i], 1.f / sm[i], t};
        if (out_pos) grad_a_dst[i] = d_adst(t, u, sum_pos[i]);
    } else {
        const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;          // index of a 4-element group of [n, D]
        const bool live = q < n * LANES;
        float t = 0.f, u = 0.f;
        if (live) {
            const FV<4> a = widen(load_raw<T, 4>(g + 4 * q)), b = widen(load_raw<T, 4>(out + 4 * q));
            t = a.v[0] * b.v[0] + a.v[1] * b.v[1] + a.v[2] * b.v[2] + a.v[3] * b.v[3];
            if (out_pos) {
                const FV<4> c = widen(load_raw<T, 4>(out_pos + 4 * q));
                u = a.v[0] * c.v[0] + a.v[1] * c.v[1] + a.v[2] * c.v[2] + a.v[3] * c.v[3];
            }
        }
        t = group_sum(t, LANES);
        if (out_pos) u = group_sum(u, LANES);
        if (live && (q % LANES) == 0) {
            const int64_t i = q / LANES;
            packed[i] = F4{a_dst[i], m[i], 1.f / sm[i], t};
            if (out_pos) grad_a_dst[i] = d_adst(t, u, sum_pos[i]);
        }
    }
}

// Host side.  Every entry point of the family fills its launch through these helpers.

// head geometry and chunk geometry of a launch
template <typename P>
static void gat_set_geometry(P& p, int64_t heads, int64_t head_dim, float slope, int64_t num_edges) {
    p.H = (int)heads; p.D = (int)head_dim; p.d = (int)(heads * head_dim); p.slope = slope;
    p.E = (int)num_edges; p.chunk = chunk_edges_for(num_edges); p.n_chunks = (int)ceil_div(num_edges, p.chunk);
}

// the short pass finishes what one wave can and defers the hub rows to the long pass
template <typename T, int VEC, int MODE, bool POS>
static int32_t launch_gat_fixups(const GatParamsT<T>& p, hipStream_t st) {
    hipLaunchKernelGGL((gat_fixup_kernel<T, VEC, false, MODE, POS>), dim3(fixup_grid_short(p.n_chunks, kFixGridShort, kWavesPerBlock)), dim3(kBlock), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((gat_fixup_kernel<T, VEC, true, MODE, POS>), dim3(fixup_grid_long(p.n_chunks)), dim3(kFixWaves * kWave), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

// A chunked producer of this family and what follows it (launch_chunked_rows, attention_common.hpp) with this family's fix-up
template <typename T, int VEC, int MODE, bool POS, typename Producer>
static int32_t launch_chunked(GatParamsT<T> p, hipStream_t st, Producer&& producer) {
    return launch_chunked_rows(p, st, producer, [&](const GatParamsT<T>& q) { return launch_gat_fixups<T, VEC, MODE, POS>(q, st); });
}

template <typename T, int VEC, int MODE, bool POS>
static int32_t launch_gat_pos(const GatParamsT<T>& p, hipStream_t st) {
    return launch_chunked<T, VEC, MODE, POS>(p, st, [&](dim3 grid, const GatParamsT<T>& q) {
        if (q.drop_p > 0.f) hipLaunchKernelGGL((gat_flat_kernel<T, VEC, MODE, true, POS>), grid, dim3(kBlock), 0, st, q);
        else hipLaunchKernelGGL((gat_flat_kernel<T, VEC, MODE, false, POS>), grid, dim3(kBlock), 0, st, q);
    });
}

template <int MODE, typename T>
static int32_t launch_gat(int vec, const GatParamsT<T>& p, hipStream_t st) {
    return with_vec(vec, [&](auto v) {
        constexpr int VEC = decltype(v)::value;
        if constexpr (MODE == 0) { if (p.out_pos) return launch_gat_pos<T, VEC, 0, true>(p, st); }
        return launch_gat_pos<T, VEC, MODE, false>(p, st);
    });
}

// pw: floats per column a chunk parks (forward: acc | m | s, + the positive-part pair; backward: 1 or 2) -- fp32 for every T
template <typename P>
static void gat_setup_partials(P& p, void* workspace, int pw) {
    SplitWs(p.n_chunks, (int64_t)pw * p.d, sizeof(float)).carve(p, workspace);
}

// pglamd_gat_aggregate (T = float) and pglamd_gat_aggregate_16: contract in include/pgl_amd.h
template <typename T>
static int32_t gat_aggregate_entry(const T* feature, const float* attn_src, const float* attn_dst, int64_t heads,
                                   int64_t head_dim, float negative_slope, float drop_p, uint32_t seed,
                                   const int32_t* row, const int32_t* col, const int32_t* eid, const int64_t* indptr,
                                   int64_t num_edges, int64_t n_csr_rows, int64_t out_rows, T* out, float* row_max,
                                   float* row_sum, T* out_pos, float* sum_pos, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    constexpr bool F32 = sizeof(T) == sizeof(float);
    if (!out || !indptr || heads <= 0 || head_dim <= 0 || out_rows < 0 || (num_edges > 0 && (!feature || !attn_src || !attn_dst || !row || !col)))
        return fail(PGLAMD_E_ARG, "gat_aggregate: bad argument");
    if ((row_max == nullptr) != (row_sum == nullptr)) return fail(PGLAMD_E_ARG, "gat_aggregate: row_max/row_sum must both be given or both NULL");
    if (drop_p < 0.f || drop_p >= 1.f || (drop_p > 0.f && !eid)) return fail(PGLAMD_E_ARG, "gat_aggregate: dropout needs 0 <= p < 1 and eid");
    if (num_edges < 0 || num_edges > kMaxEdges || out_rows >= INT32_MAX) return fail(PGLAMD_E_RANGE, "gat_aggregate: sizes beyond int32 engine range");
    const int64_t d = heads * head_dim;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (out_rows == 0) return PGLAMD_OK;
    if (num_edges == 0) {
        PGLAMD_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)out_rows * d * sizeof(T), st));
        if (row_max) {
            PGLAMD_HIP_CHECK(hipMemsetAsync(row_max, 0, (size_t)out_rows * heads * sizeof(float), st));
            PGLAMD_HIP_CHECK(hipMemsetAsync(row_sum, 0, (size_t)out_rows * heads * sizeof(float), st));
        }
        if (out_pos) {
            PGLAMD_HIP_CHECK(hipMemsetAsync(out_pos, 0, (size_t)out_rows * d * sizeof(T), st));
            PGLAMD_HIP_CHECK(hipMemsetAsync(sum_pos, 0, (size_t)out_rows * heads * sizeof(float), st));
        }
        return PGLAMD_OK;
    }
    if ((out_pos == nullptr) != (sum_pos == nullptr) || (out_pos && reinterpret_cast<uintptr_t>(out_pos) % (4 * sizeof(T))))
        return fail(PGLAMD_E_ARG, "gat_aggregate: out_pos and sum_pos come together (out_pos aligned to four elements)");
    // the lane unit is sizeof(T) * VEC bytes; the workspace holds fp32 partials in lanes of VEC floats either way
    const int vec = gat_vec(heads, head_dim, feature, out, F32 ? workspace : nullptr, false, sizeof(T));
    if (vec == 0 || heads > kWave || (!F32 && reinterpret_cast<uintptr_t>(workspace) % 16))
        return fail(PGLAMD_E_SHAPE, "gat_aggregate: heads*head_dim = %lld does not fit one 64-lane tile (max 256 with head_dim %% 4 == 0)", (long long)d);
    if (!workspace || workspace_bytes < pglamd_gat_aggregate_workspace_bytes(num_edges, heads, head_dim))
        return fail(PGLAMD_E_WORKSPACE, "gat_aggregate: workspace too small");
    GatParamsT<T> p{};
    gat_set_geometry(p, heads, head_dim, negative_slope, num_edges);
    p.x = feature; p.p_col = attn_src; p.p_row = attn_dst; p.out = out; p.row_max = row_max; p.row_sum = row_sum;
    p.out_pos = out_pos; p.sum_pos = sum_pos;
    p.row = row; p.col = col; p.eid = eid; p.indptr = indptr;
    p.out_rows = out_rows; p.n_csr_rows = n_csr_rows;
    p.drop_p = drop_p; p.drop_scale = 1.f / (1.f - drop_p); p.seed = seed;
    gat_setup_partials(p, workspace, out_pos ? 5 : 3);
    return launch_gat<0>(vec, p, st);
}

// pglamd_gat_backward (T = float) and pglamd_gat_backward_16: contract in include/pgl_amd.h
template <typename T>
static int32_t gat_backward_entry(const T* grad_out, const T* feature, const float* attn_src,
                                  const float* attn_dst, const float* row_max, const float* row_sum, const T* out,
                                  int64_t heads, int64_t head_dim, float negative_slope, float drop_p, uint32_t seed,
                                  const int32_t* dst_row, const int32_t* dst_col, const int32_t* dst_eid,
                                  const int64_t* dst_indptr, const int32_t* src_row, const int32_t* src_col,
                                  const int32_t* src_eid, const int64_t* src_indptr, int64_t num_edges, int64_t num_nodes,
                                  T* grad_feature, float* grad_attn_src, float* grad_attn_dst, float* grad_pre,
                                  const T* out_pos, const float* sum_pos, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    constexpr size_t kGroup = 4 * sizeof(T);     // the pack kernel reads groups of four elements
    if ((out_pos == nullptr) != (sum_pos == nullptr) || (out_pos && (!grad_attn_dst || reinterpret_cast<uintptr_t>(out_pos) % kGroup)))
        return fail(PGLAMD_E_ARG, "gat_backward: out_pos and sum_pos come together, with grad_attn_dst (out_pos aligned to four elements)");
    if (out_pos) grad_pre = nullptr;             // d a_dst comes out of the pack kernel: neither the edge buffer nor the dst-sorted walk
    if (heads <= 0 || head_dim <= 0 || num_nodes < 0 || num_edges < 0 || !grad_feature || !grad_attn_src || (!grad_attn_dst && !grad_pre) ||
        (num_edges > 0 && (!grad_out || !feature || !attn_src || !attn_dst || !row_max || !row_sum || !out || !dst_row || !dst_col ||
                           !dst_eid || !dst_indptr || !src_row || !src_col || !src_eid || !src_indptr)))
        return fail(PGLAMD_E_ARG, "gat_backward: bad argument");
    if (drop_p < 0.f || drop_p >= 1.f) return fail(PGLAMD_E_ARG, "gat_backward: dropout needs 0 <= p < 1");
    if (num_edges > kMaxEdges || num_nodes >= INT32_MAX) return fail(PGLAMD_E_RANGE, "gat_backward: sizes beyond int32 engine range");
    const int64_t d = heads * head_dim;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_nodes == 0) return PGLAMD_OK;
    if (num_edges == 0) {
        PGLAMD_HIP_CHECK(hipMemsetAsync(grad_feature, 0, (size_t)num_nodes * d * sizeof(T), st));
        PGLAMD_HIP_CHECK(hipMemsetAsync(grad_attn_src, 0, (size_t)num_nodes * heads * sizeof(float), st));
        if (grad_attn_dst) PGLAMD_HIP_CHECK(hipMemsetAsync(grad_attn_dst, 0, (size_t)num_nodes * heads * sizeof(float), st));
        return PGLAMD_OK;
    }
    const int vec = gat_vec(heads, head_dim, feature, grad_out, grad_feature, true, sizeof(T));
    if (vec == 0 || heads > kWave || reinterpret_cast<uintptr_t>(workspace) % 256 || (reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(grad_out)) % kGroup)
        return fail(PGLAMD_E_SHAPE, "gat_backward: heads*head_dim = %lld needs one 64-lane tile and head_dim/VEC a power of two", (long long)d);
    if (!workspace || workspace_bytes < pglamd_gat_backward_workspace_bytes(num_edges, num_nodes, heads, head_dim))
        return fail(PGLAMD_E_WORKSPACE, "gat_backward: workspace too small");
    // (0) the destination-side scalars of every (node, head), packed so that an edge fetches them with one 16-byte load
    const size_t pack_bytes = align_up((size_t)num_nodes * heads * sizeof(F4), 256);
    F4* packed = static_cast<F4*>(workspace);
    workspace = static_cast<char*>(workspace) + pack_bytes;
    {
        const int64_t pairs = num_nodes * heads;
        const int lanes = (head_dim % 4 == 0) ? (int)(head_dim / 4) : 0;
#define PGLAMD_PACK(L) hipLaunchKernelGGL((gat_pack_kernel<T, L>), dim3((unsigned)ceil_div(pairs * (L ? L : 1), kBlock)), dim3(kBlock), 0, st, \
                                          attn_dst, row_max, row_sum, grad_out, out, pairs, (int)head_dim, packed, out_pos, sum_pos, negative_slope, \
                                          grad_attn_dst)
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
    GatParamsT<T> p{};
    gat_set_geometry(p, heads, head_dim, negative_slope, num_edges);
    p.drop_p = drop_p; p.drop_scale = 1.f / (1.f - drop_p); p.seed = seed;
    p.packed = packed;
    p.out_rows = num_nodes; p.n_csr_rows = num_nodes;
    // (1) dst-sorted walk: row = v gathers f[u], a_src[u]; accumulates d a_dst[v].  Skipped when the caller takes
    //     d pre_e [E,H] from walk (2) instead and segment-sums it by destination itself (faster, 4*E*H bytes more memory).
    if (!grad_pre && !out_pos) {
        GatParamsT<T> q = p;
        q.row = dst_row; q.col = dst_col; q.eid = dst_eid; q.indptr = dst_indptr;
        q.x = feature; q.p_col = attn_src; q.p_row = attn_dst; q.row_vec = grad_out; q.out = nullptr; q.out_a = grad_attn_dst;
        gat_setup_partials(q, workspace, 1);
        PGLAMD_TRY(launch_gat<3>(vec, q, st));
    }
    // (2) src-sorted walk: row = u gathers g[v] and v's scalars; accumulates d f[u] and d a_src[u]
    p.row = src_row; p.col = src_col; p.eid = src_eid; p.indptr = src_indptr;
    p.x = grad_out; p.p_col = attn_dst; p.p_row = attn_src; p.row_vec = feature; p.out = grad_feature; p.out_a = grad_attn_src;
    p.dpre = grad_pre;
    gat_setup_partials(p, workspace, 2);
    return launch_gat<2>(vec, p, st);
}

}  // namespace pglamd
