// edge_message.hip -- the molecular models' message act(x[u] + e_k) + eps over a graph, reduced per destination by a plain sum (GINE:
// ogb_examples/graphproppred/ogbg_molpcba/model.py:266-273, ogb_examples/lsc/PCQM4M/conv.py:46-50, 77-81,
// examples/kddcup2021/PCQM4M/models/layers.py:196-200, 238-245) or by a softmax PER CHANNEL (DeeperGCN's GENConv,
// examples/kddcup2021/PCQM4M/models/layers.py:73-90), forward AND backward, without an [E, d] tensor of x[u], e, their sum or alpha:
//     pre_k = x[u] + e_k      m_k = act(pre_k) + eps      k = (u -> v),  act = relu | swish
//     sum:      out[v, c] = sum_k m_k[c]
//     softmax:  out[v, c] = sum_k softmax_k(t m_k[c]) m_k[c]             (over the in-edges of v, every channel on its own)
// e_k is a row of a dense ef [E, d] (row eid[p] for position p of the index) or, CODED, the sum of F <= 4 embedding rows
// table[off[f] + codes[k, f]] taken in the order f = 0 .. F - 1 (the BondEncoder of mol_encoder.py:42-58), the same bits in both passes.
//
// Geometry: no channel talks to another, so a lane owns VEC channels and a wave a tile of 64 VEC columns; blockIdx.y is the column
// tile (d <= 1024: up to four tiles of 256 columns with VEC = 4, more of the narrower ones when d is odd).  The work unit is
// (edge chunk, column tile): a wave per chunk of the sorted edge stream, as every chunked producer here (split_rows.hpp).
// FORWARD (em_forward_kernel): one walk of the dst-sorted index, scalar index loads, batches of gathered rows in flight.  softmax is an
//   online softmax per lane and channel (running max, sum and weighted sum in registers, ONE exponential per element); it saves
//   lse[v, c] = max + log(sum) beside out for the backward, sum saves nothing.  CODED: the block copies its tile's columns of the
//   stacked table into LDS once ([T, tile columns]); an edge then costs F scalar code loads and one gathered x row.
// BACKWARD (em_backward_kernel): one walk of the src-sorted index.  x[u] rides with the row; pre_k and m_k are recomputed; g[v] (softmax:
//   and lse[v], out[v]) are gathered.  a_k = exp(t m_k - lse[v]),  d m_k = g a_k (1 + t (m_k - out[v]))  (sum: d m_k = g),
//   d pre_k = d m_k act'(pre_k).  d x[u] is summed in registers along the row; d ef[k] is one plain store per edge (not at all when not
//   wanted).  CODED: d table is accumulated in LDS, one [T, tile columns] copy PER WAVE of which a lane touches only its own columns (a
//   single writer per element), the four copies are added in wave order at the end of the block and leave one partial per block; the
//   walk runs on a CAPPED grid (a block takes several chunk groups), so the partials are few, and em_sum_partials_kernel adds them in
//   block order.  d t: a scalar per lane -> wave -> block by the same route.  (The backward reads the table itself through the caches:
//   with the four gradient copies a fifth, read-only one would not leave room for OGB's 13 rows of a 256-column tile in 64 KB.)
// Rows longer than a chunk leave partials ((acc, max, sum) per channel for the softmax, one value else), merged in a fixed order by
// em_fixup_kernel.  No atomics on results: two calls give the same bits.  Rows without edges, and table rows nobody uses, are +0.0.
#include "attention_common.hpp"

namespace pglamd {

constexpr int kEmMaxD = 1024;
constexpr int kEmMaxFeats = 4;
constexpr int kEmLdsFloats = 16320;          // 4 copies of [T, tile columns] in 64 KB less a little: T * tile columns <= 4080
constexpr int kEmGridCoded = 512;            // walk blocks of a CODED backward: one [T, d] partial each
constexpr int kEmGridDense = 2048;           // walk blocks of a dense backward (8192 waves: the chip's wave slots)

struct EmParams {
    const float* x;                 // [N, d]: gathered by col (forward) / the row node's (backward)
    const float* ef;                // dense: [E, d], row eid[p]
    const int* codes;               // CODED: [E, F], row eid[p]
    const float* table;             // CODED: [T, d]
    const float* g;                 // backward: d loss / d out [N, d], gathered by col
    const float* fwd_out;           // backward, softmax: out [N, d]
    const float* lse;               // backward, softmax: lse [N, d]
    float* out;                     // out (forward) / d x (backward; NULL: not wanted)
    float* lse_out;                 // forward, softmax: [N, d]
    float* grad_ef;                 // backward, dense: [E, d] (NULL: not wanted)
    float* tab_part;                // backward, CODED: [walk blocks, T, d] (NULL: d table not wanted)
    float* dt_part;                 // backward, softmax: [walk blocks, tiles] (NULL: d t not wanted)
    const int* row; const int* col; const int* eid; const int64_t* indptr;
    float* part_head; float* part_tail;         // [n_chunks, PW, d]
    int* long_count; int* long_list; int* long_list2;
    int64_t out_rows, n_csr_rows;
    int E, n_chunks, chunk, n_blocks, n_grid_chunks, n_logical;
    int d, F, T, tcols, act;
    int off[kEmMaxFeats];
    float eps, t;
};

__device__ __forceinline__ float em_act(float z, int act) { return act == 0 ? relu_f(z) : z / (1.f + expf(-z)); }
__device__ __forceinline__ float em_act_grad(float z, int act) {
    if (act == 0) return z > 0.f ? 1.f : 0.f;
    const float s = 1.f / (1.f + expf(-z));
    return s * (1.f + z * (1.f - s));
}

// e_k of a CODED edge for one lane: table rows read from `tab` (LDS or global), row stride `stride`, the lane's columns at `jl`
template <int VEC>
__device__ __forceinline__ FV<VEC> em_coded_row(const float* tab, int stride, int jl, const int (&rows)[kEmMaxFeats], int F) {
    FV<VEC> e = *reinterpret_cast<const FV<VEC>*>(tab + (int64_t)rows[0] * stride + jl);
    for (int f = 1; f < F; ++f) {
        const FV<VEC> r = *reinterpret_cast<const FV<VEC>*>(tab + (int64_t)rows[f] * stride + jl);
#pragma unroll
        for (int k = 0; k < VEC; ++k) e.v[k] += r.v[k];
    }
    return e;
}

// the F table rows of the edge with original id `ed` (wave-uniform: scalar loads), clamped into the table
__device__ __forceinline__ void em_code_rows(cptr<int> codes, int ed, const EmParams& p, int (&rows)[kEmMaxFeats]) {
#pragma unroll
    for (int f = 0; f < kEmMaxFeats; ++f) {
        rows[f] = 0;
        if (f < p.F) rows[f] = min(max(p.off[f] + codes[(int64_t)ed * p.F + f], 0), p.T - 1);
    }
}

constexpr int em_batch(int vec) { return vec == 4 ? 2 : 4; }     // edges whose rows are in flight together

template <int VEC, bool SOFTMAX, bool CODED>
__global__ __launch_bounds__(kBlock) void em_forward_kernel(EmParams p) {
    extern __shared__ float em_lds[];                       // CODED: [T, tcols]
    constexpr int U = em_batch(VEC);
    constexpr int PW = SOFTMAX ? 3 : 1;
    using V = FV<VEC>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform(threadIdx.x >> 6);
    const int jl = lane * VEC;
    const int j0 = (int)blockIdx.y * kWave * VEC + jl;
    const bool live = j0 < p.d;

    if ((int)blockIdx.x >= p.n_grid_chunks) {
        zero_fill_role(p, lane, wib, [&](int64_t r) {
            if (!live) return;
            *reinterpret_cast<V*>(p.out + r * p.d + j0) = V{};
            if constexpr (SOFTMAX) *reinterpret_cast<V*>(p.lse_out + r * p.d + j0) = V{};
        });
        return;
    }
    if constexpr (CODED) {
        const int n = p.T * p.tcols;
        for (int i = threadIdx.x; i < n; i += kBlock) {
            const int col = (int)blockIdx.y * kWave * VEC + i % p.tcols;
            em_lds[i] = col < p.d ? p.table[(int64_t)(i / p.tcols) * p.d + col] : 0.f;
        }
        __syncthreads();
    }
    const int64_t lb = xcd_swizzle(blockIdx.x, p.n_blocks);
    if (lb < 0) return;
    const int c = wave_uniform((int)lb * kWavesPerBlock + wib);
    if (c >= p.n_chunks) return;
    const cptr<int> rowp = as_const(p.row);
    const cptr<int> colp = as_const(p.col);
    const cptr<int> eidp = as_const(p.eid);
    const cptr<int> codep = as_const(p.codes);
    const int e0 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk, p.chunk, p.E);
    const int e1 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk + p.chunk, p.chunk, p.E);
    if (e0 >= e1) return;
    const float* __restrict__ xp = p.x;
    const float* __restrict__ efp = p.ef;
    const bool has_eid = p.eid != nullptr;
    const float eps = p.eps, tt = p.t;
    const int actf = p.act;

    float acc[VEC], m[VEC], s[VEC];
    auto reset = [&]() {
#pragma unroll
        for (int k = 0; k < VEC; ++k) { acc[k] = 0.f; m[k] = -INFINITY; s[k] = 0.f; }
    };
    reset();
    int cur = rowp[e0];
    bool head_open = e0 > 0 && rowp[e0 - 1] == cur;

    auto put = [&](float* dst, const float (&a)[VEC]) {
        V o;
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = a[k];
        *reinterpret_cast<V*>(dst) = o;
    };
    auto store_partial = [&](bool headp) {
        if (live) {
            float* dst = (headp ? p.part_head : p.part_tail) + (int64_t)c * PW * p.d + j0;
            put(dst, acc);
            if constexpr (SOFTMAX) { put(dst + p.d, m); put(dst + 2 * p.d, s); }
        }
        if (!headp && lane == 0 && blockIdx.y == 0) p.long_list[atomicAdd(p.long_count, 1)] = c;
    };
    auto store_final = [&](int r) {
        if (r >= p.out_rows || !live) return;
        if constexpr (SOFTMAX) {
            float o[VEC], l[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) { o[k] = acc[k] / s[k]; l[k] = m[k] + logf(s[k]); }
            put(p.out + (int64_t)r * p.d + j0, o);
            put(p.lse_out + (int64_t)r * p.d + j0, l);
        } else {
            put(p.out + (int64_t)r * p.d + j0, acc);
        }
    };
    auto consume = [&](int r, const V& xv, const V& ev) {
        if (r != cur) {
            if (head_open) store_partial(true); else store_final(cur);
            head_open = false;
            cur = r;
            reset();
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float mk = em_act(xv.v[k] + ev.v[k], actf) + eps;
            if constexpr (SOFTMAX) {
                // online softmax: one of exp(m - mn), exp(l - mn) is exp(0) = 1, so ONE exponential per element
                const float l = tt * mk;
                const float dlt = l - m[k];                  // +inf on the first edge of a row (m = -inf): e^{-inf} = 0
                const float ex = expf(-fabsf(dlt));
                const bool up = dlt > 0.f;
                const float rs = up ? ex : 1.f, pe = up ? 1.f : ex;
                s[k] = s[k] * rs + pe;
                acc[k] = acc[k] * rs + pe * mk;
                m[k] = up ? l : m[k];
            } else {
                acc[k] += mk;
            }
        }
    };
    auto edge_id = [&](int e) { return has_eid ? eidp[e] : e; };
    auto load_e = [&](int ed) {
        V ev{};
        if constexpr (CODED) {
            int rows[kEmMaxFeats];
            em_code_rows(codep, ed, p, rows);
            if (live) ev = em_coded_row<VEC>(em_lds, p.tcols, jl, rows, p.F);
        } else {
            if (live) ev = *reinterpret_cast<const V*>(efp + (int64_t)ed * p.d + j0);
        }
        return ev;
    };
    int e = e0;
    for (; e + U <= e1; e += U) {
        int rr[U]; V xv[U], ev[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            rr[i] = rowp[e + i];
            const int cc = colp[e + i];
            xv[i] = live ? *reinterpret_cast<const V*>(xp + (int64_t)cc * p.d + j0) : V{};
            ev[i] = load_e(edge_id(e + i));
        }
#pragma unroll
        for (int i = 0; i < U; ++i) consume(rr[i], xv[i], ev[i]);
    }
    for (; e < e1; ++e) {
        const int cc = colp[e];
        const V xv = live ? *reinterpret_cast<const V*>(xp + (int64_t)cc * p.d + j0) : V{};
        consume(rowp[e], xv, load_e(edge_id(e)));
    }
    const bool tail_open = e1 < p.E && rowp[e1] == cur;
    if (head_open) store_partial(true);
    else if (tail_open) store_partial(false);
    else store_final(cur);
}

template <int VEC, bool SOFTMAX, bool CODED>
__global__ __launch_bounds__(kBlock) void em_backward_kernel(EmParams p) {
    extern __shared__ float em_lds[];                       // CODED: [kWavesPerBlock][T, tcols] gradient copies, one per wave
    __shared__ float dt_wave[kWavesPerBlock];
    constexpr int U = em_batch(VEC);
    using V = FV<VEC>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform(threadIdx.x >> 6);
    const int jl = lane * VEC;
    const int j0 = (int)blockIdx.y * kWave * VEC + jl;
    const bool live = j0 < p.d;

    if ((int)blockIdx.x >= p.n_grid_chunks) {
        if (p.out)
            zero_fill_role(p, lane, wib, [&](int64_t r) {
                if (live) *reinterpret_cast<V*>(p.out + r * p.d + j0) = V{};
            });
        return;
    }
    const bool want_tab = CODED && p.tab_part != nullptr;
    const int tab_n = p.T * p.tcols;
    float* my_tab = em_lds + wib * tab_n;                   // this wave's copy; a lane adds only to its own columns
    if (want_tab)
        for (int i = lane; i < tab_n; i += kWave) my_tab[i] = 0.f;
    const cptr<int> rowp = as_const(p.row);
    const cptr<int> colp = as_const(p.col);
    const cptr<int> eidp = as_const(p.eid);
    const cptr<int> codep = as_const(p.codes);
    const float* __restrict__ xp = p.x;
    const float* __restrict__ efp = p.ef;
    const float* __restrict__ gp = p.g;
    const float* __restrict__ op = p.fwd_out;
    const float* __restrict__ lp = p.lse;
    const float* __restrict__ tabp = p.table;
    const bool has_eid = p.eid != nullptr;
    const float eps = p.eps, tt = p.t;
    const int actf = p.act;
    float dt_lane = 0.f;

    auto walk_chunk = [&](int c) {
        const int e0 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk, p.chunk, p.E);
        const int e1 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk + p.chunk, p.chunk, p.E);
        if (e0 >= e1) return;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        int cur = rowp[e0];
        bool head_open = e0 > 0 && rowp[e0 - 1] == cur;
        V x_held{};
        auto open_row = [&](int r) { if (live) x_held = *reinterpret_cast<const V*>(xp + (int64_t)r * p.d + j0); };
        open_row(cur);
        auto store = [&](float* dst) {
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
            *reinterpret_cast<V*>(dst) = o;
        };
        auto store_partial = [&](bool headp) {
            if (live && p.out) store((headp ? p.part_head : p.part_tail) + (int64_t)c * p.d + j0);
            if (!headp && lane == 0 && blockIdx.y == 0) p.long_list[atomicAdd(p.long_count, 1)] = c;
        };
        auto store_final = [&](int r) {
            if (r < p.out_rows && live && p.out) store(p.out + (int64_t)r * p.d + j0);
        };
        struct Edge { int r, ed; int rows[kEmMaxFeats]; V ev, gv, ov, lv; };
        auto load = [&](int e, Edge& q) {
            q.r = rowp[e];
            const int cc = colp[e];
            q.ed = has_eid ? eidp[e] : e;
            q.ev = V{}; q.gv = V{}; q.ov = V{}; q.lv = V{};
            if constexpr (CODED) em_code_rows(codep, q.ed, p, q.rows);
            if (!live) return;
            if constexpr (CODED) q.ev = em_coded_row<VEC>(tabp + j0, p.d, 0, q.rows, p.F);
            else q.ev = *reinterpret_cast<const V*>(efp + (int64_t)q.ed * p.d + j0);
            q.gv = *reinterpret_cast<const V*>(gp + (int64_t)cc * p.d + j0);
            if constexpr (SOFTMAX) {
                q.ov = *reinterpret_cast<const V*>(op + (int64_t)cc * p.d + j0);
                q.lv = *reinterpret_cast<const V*>(lp + (int64_t)cc * p.d + j0);
            }
        };
        auto consume = [&](const Edge& q) {
            if (q.r != cur) {
                if (head_open) store_partial(true); else store_final(cur);
                head_open = false;
                cur = q.r;
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
                open_row(cur);
            }
            V dp;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float pre = x_held.v[k] + q.ev.v[k];
                float dm = q.gv.v[k];
                if constexpr (SOFTMAX) {
                    const float mk = em_act(pre, actf) + eps;
                    const float ga = q.gv.v[k] * expf(tt * mk - q.lv.v[k]);
                    const float dev = mk - q.ov.v[k];
                    dm = ga * (1.f + tt * dev);
                    dt_lane += ga * mk * dev;
                }
                dp.v[k] = dm * em_act_grad(pre, actf);
                acc[k] += dp.v[k];
            }
            if (!live) return;
            if constexpr (CODED) {
                if (want_tab)
                    for (int f = 0; f < p.F; ++f) {
                        float* dst = my_tab + q.rows[f] * p.tcols + jl;
#pragma unroll
                        for (int k = 0; k < VEC; ++k) dst[k] += dp.v[k];
                    }
            } else {
                if (p.grad_ef) *reinterpret_cast<V*>(p.grad_ef + (int64_t)q.ed * p.d + j0) = dp;
            }
        };
        int e = e0;
        for (; e + U <= e1; e += U) {
            Edge q[U];
#pragma unroll
            for (int i = 0; i < U; ++i) load(e + i, q[i]);
#pragma unroll
            for (int i = 0; i < U; ++i) consume(q[i]);
        }
        for (; e < e1; ++e) { Edge q; load(e, q); consume(q); }
        const bool tail_open = e1 < p.E && rowp[e1] == cur;
        if (head_open) store_partial(true);
        else if (tail_open) store_partial(false);
        else store_final(cur);
    };
    // a block takes the chunk groups b, b + walk blocks, ...: the grid is capped, so the per-block partials are few
    for (int b = blockIdx.x; b < p.n_logical; b += p.n_grid_chunks) {
        const int64_t lb = xcd_swizzle(b, p.n_blocks);
        if (lb < 0) continue;
        const int c = wave_uniform((int)lb * kWavesPerBlock + wib);
        if (c < p.n_chunks) walk_chunk(c);
    }
    if (want_tab) {                                         // the four copies in wave order -> this block's partial
        __syncthreads();
        for (int i = threadIdx.x; i < tab_n; i += kBlock) {
            const int col = (int)blockIdx.y * kWave * VEC + i % p.tcols;
            float sum = em_lds[i];
#pragma unroll
            for (int w = 1; w < kWavesPerBlock; ++w) sum += em_lds[w * tab_n + i];
            if (col < p.d) p.tab_part[((int64_t)blockIdx.x * p.T + i / p.tcols) * p.d + col] = sum;
        }
    }
    if (SOFTMAX && p.dt_part) {
        const float w = group_sum(live ? dt_lane : 0.f, kWave);
        if (lane == 0) dt_wave[wib] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            float sum = dt_wave[0];
#pragma unroll
            for (int i = 1; i < kWavesPerBlock; ++i) sum += dt_wave[i];
            p.dt_part[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = sum;
        }
    }
}

// merges the partials of the rows longer than a chunk (the lists and the order of dot_fixup_kernel, split_rows.hpp), a column tile per
// blockIdx.y.  SOFTMAX: the associative merge of (acc, max, sum) per channel, then out = acc / sum and lse; else plain sums.
template <int VEC, bool LONG, bool SOFTMAX>
__global__ __launch_bounds__(LONG ? kFixWaves * kWave : kBlock) void em_fixup_kernel(EmParams p) {
    using V = FV<VEC>;
    constexpr int NW = LONG ? kFixWaves : 1;
    constexpr int PW = SOFTMAX ? 3 : 1;
    __shared__ float red[LONG ? kFixWaves : 1][PW][LONG ? kWave * VEC : 1];
    __shared__ int red_n[LONG ? kFixWaves : 1];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform(threadIdx.x >> 6);
    const cptr<int> rowp = as_const(p.row);
    const cptr<int64_t> ip = as_const(p.indptr);
    const int j0 = (int)blockIdx.y * kWave * VEC + lane * VEC;
    const bool live = j0 < p.d;
    const int* list = LONG ? p.long_list2 : p.long_list;
    const int n_tasks = LONG ? p.long_count[1] : p.long_count[0];
    const int first = LONG ? (int)blockIdx.x : (int)blockIdx.x * kWavesPerBlock + wib;
    const int stride = LONG ? (int)gridDim.x : (int)gridDim.x * kWavesPerBlock;
    for (int t_id = first; t_id < n_tasks; t_id += stride) {
        const int a = wave_uniform(list[t_id]);
        const int e1 = (a + 1) * p.chunk;
        const int r = rowp[e1 - 1];
        const int b = chunk_of_edge(ip[r + 1] - 1, p.chunk);    // last chunk holding a piece of row r
        if constexpr (!LONG) {
            if (fixup_is_long(a, b)) {                  // hub row: defer to the block-parallel pass
                if (lane == 0 && blockIdx.y == 0) p.long_list2[atomicAdd(p.long_count + 1, 1)] = a;
                continue;
            }
        }
        float acc[VEC], m[VEC], s[VEC];
        auto reset = [&]() {
#pragma unroll
            for (int k = 0; k < VEC; ++k) { acc[k] = 0.f; m[k] = -INFINITY; s[k] = 0.f; }
        };
        auto merge_vals = [&](const V& a2, const V& m2, const V& s2) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                if constexpr (SOFTMAX) {
                    const float mn = fmaxf(m[k], m2.v[k]);
                    const float c1 = m[k] == mn ? 1.f : expf(m[k] - mn), c2 = m2.v[k] == mn ? 1.f : expf(m2.v[k] - mn);
                    s[k] = s[k] * c1 + s2.v[k] * c2;
                    acc[k] = acc[k] * c1 + a2.v[k] * c2;
                    m[k] = mn;
                } else {
                    acc[k] += a2.v[k];
                }
            }
        };
        auto merge = [&](const float* base) {
            base += j0;
            if constexpr (SOFTMAX) merge_vals(*reinterpret_cast<const V*>(base), *reinterpret_cast<const V*>(base + p.d), *reinterpret_cast<const V*>(base + 2 * p.d));
            else merge_vals(*reinterpret_cast<const V*>(base), V{}, V{});
        };
        reset();
        if constexpr (!LONG) {
            if (live) {
                merge(p.part_tail + (int64_t)a * PW * p.d);
                for (int c = a + 1; c <= b; ++c) merge(p.part_head + (int64_t)c * PW * p.d);
            }
        } else {
            if (live)
                for (int c = a + 1 + wib; c <= b; c += NW) merge(p.part_head + (int64_t)c * PW * p.d);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                red[wib][0][lane * VEC + k] = acc[k];
                if constexpr (SOFTMAX) { red[wib][1][lane * VEC + k] = m[k]; red[wib][PW - 1][lane * VEC + k] = s[k]; }
            }
            if (lane == 0) red_n[wib] = a + 1 + wib <= b;
            __syncthreads();
            if (wib != 0) continue;
            // wave 0: the tail partial of chunk a first, then the wave results in wave order
            reset();
            if (live) {
                merge(p.part_tail + (int64_t)a * PW * p.d);
                for (int w = 0; w < NW; ++w) {
                    if (!red_n[w]) continue;                    // that wave had no partial
                    V a2, m2{}, s2{};
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        a2.v[k] = red[w][0][lane * VEC + k];
                        if constexpr (SOFTMAX) { m2.v[k] = red[w][1][lane * VEC + k]; s2.v[k] = red[w][PW - 1][lane * VEC + k]; }
                    }
                    merge_vals(a2, m2, s2);
                }
            }
        }
        if (!live || r >= p.out_rows) continue;
        V o, l;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            o.v[k] = SOFTMAX ? acc[k] / s[k] : acc[k];
            l.v[k] = SOFTMAX ? m[k] + logf(s[k]) : 0.f;
        }
        *reinterpret_cast<V*>(p.out + (int64_t)r * p.d + j0) = o;
        if constexpr (SOFTMAX) *reinterpret_cast<V*>(p.lse_out + (int64_t)r * p.d + j0) = l;
    }
}

// out[i] = part[0][i] + part[1][i] + ... in block order (d table: n = T d), a thread per element
__global__ __launch_bounds__(kBlock) void em_sum_partials_kernel(const float* __restrict__ part, int n_parts, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float sum = 0.f;
    for (int b = 0; b < n_parts; ++b) sum += part[(int64_t)b * n + i];
    out[i] = sum;
}

// out[0] = the sum of n scalars (d t): thread i adds the values i, i + 256, ... in order, thread 0 the 256 results in order
__global__ __launch_bounds__(kBlock) void em_sum_scalars_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ float red[kBlock];
    float sum = 0.f;
    for (int i = threadIdx.x; i < n; i += kBlock) sum += part[i];
    red[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x) return;
    sum = 0.f;
    for (int i = 0; i < kBlock; ++i) sum += red[i];
    out[0] = sum;
}

__global__ __launch_bounds__(kBlock) void em_zero_kernel(float* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = 0.f;
}

// Host side.

static int em_vec(int64_t d, std::initializer_list<const void*> ps) {
    uintptr_t al = 0;
    for (const void* q : ps) al |= reinterpret_cast<uintptr_t>(q);
    for (int v = 4; v > 1; v >>= 1)
        if (d % v == 0 && al % (4 * v) == 0) return v;
    return 1;
}
static int em_vec_of(int64_t d) { return d % 4 == 0 ? 4 : d % 2 == 0 ? 2 : 1; }
static int64_t em_tile_cols(int64_t d, int vec) { return std::min<int64_t>(d, (int64_t)kWave * vec); }
static int64_t em_walk_blocks(int64_t n_chunks, bool coded) {
    return std::min<int64_t>(xcd_grid(ceil_div(n_chunks, kWavesPerBlock)), coded ? kEmGridCoded : kEmGridDense);
}

static int32_t em_zero(float* out, int64_t n, hipStream_t st) {
    if (!out || n <= 0) return PGLAMD_OK;
    hipLaunchKernelGGL(em_zero_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, st, out, n);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

template <int VEC, bool SOFTMAX>
static int32_t launch_em_fixups(const EmParams& p, unsigned tiles, hipStream_t st) {
    hipLaunchKernelGGL((em_fixup_kernel<VEC, false, SOFTMAX>), dim3(fixup_grid_short(p.n_chunks, kFixGridShort, kWavesPerBlock), tiles), dim3(kBlock), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((em_fixup_kernel<VEC, true, SOFTMAX>), dim3(fixup_grid_long(p.n_chunks), tiles), dim3(kFixWaves * kWave), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

// fn(VEC, SOFTMAX, CODED as integral constants) for the runtime choice
template <typename Fn>
static int32_t em_dispatch(int vec, bool softmax, bool coded, Fn&& fn) {
    return with_vec(vec, [&](auto v) {
        using T = std::true_type; using F = std::false_type;
        if (softmax) return coded ? fn(v, T{}, T{}) : fn(v, T{}, F{});
        return coded ? fn(v, F{}, T{}) : fn(v, F{}, F{});
    });
}

static int32_t em_check(const char* what, const float* x, const float* ef, const int32_t* codes, const float* table, const int32_t* offsets,
                        int64_t num_feats, int64_t table_rows, int64_t d, int32_t act, int32_t reduce, float eps, float t,
                        int64_t num_edges, int64_t num_nodes, bool backward) {
    if (d < 1 || d > kEmMaxD) return fail(PGLAMD_E_SHAPE, "%s: d = %lld must be in 1 .. %d", what, (long long)d, kEmMaxD);
    if (num_nodes < 0 || num_edges < 0 || (act != 0 && act != 1) || (reduce != 0 && reduce != 1) || !(eps >= 0.f) || (reduce == 1 && !(t > 0.f)))
        return fail(PGLAMD_E_ARG, "%s: bad argument (act 0 | 1, reduce 0 | 1, eps >= 0, t > 0)", what);
    if (num_edges > kMaxEdges || num_nodes >= INT32_MAX) return fail(PGLAMD_E_RANGE, "%s: sizes beyond int32 engine range", what);
    const bool coded = table != nullptr;
    if (coded == (ef != nullptr) && num_edges > 0) return fail(PGLAMD_E_ARG, "%s: exactly one of edge_feat and codes must be given", what);
    if (num_edges > 0 && !x) return fail(PGLAMD_E_ARG, "%s: bad argument", what);
    if (coded) {
        if ((num_edges > 0 && !codes) || !offsets || num_feats < 1 || num_feats > kEmMaxFeats || table_rows < 1)
            return fail(PGLAMD_E_ARG, "%s: codes need a table, offsets and 1 <= F <= %d", what, kEmMaxFeats);
        if (table_rows * em_tile_cols(d, em_vec_of(d)) * (backward ? kWavesPerBlock : 1) > kEmLdsFloats)
            return fail(PGLAMD_E_SHAPE, "%s: a table of %lld rows of d = %lld does not fit the LDS budget", what, (long long)table_rows, (long long)d);
        for (int64_t f = 0; f < num_feats; ++f)
            if (offsets[f] < 0 || offsets[f] >= table_rows) return fail(PGLAMD_E_ARG, "%s: offsets[%lld] outside the table", what, (long long)f);
    }
    return PGLAMD_OK;
}

static void em_set(EmParams& p, const float* x, const float* ef, const int32_t* codes, const float* table, const int32_t* offsets,
                   int64_t num_feats, int64_t table_rows, int64_t d, int vec, int32_t act, float eps, float t, const int32_t* row,
                   const int32_t* col, const int32_t* eid, const int64_t* indptr, int64_t num_edges, int64_t num_nodes) {
    p.x = x; p.ef = ef; p.codes = codes; p.table = table;
    p.F = (int)num_feats; p.T = (int)table_rows; p.d = (int)d; p.tcols = (int)em_tile_cols(d, vec); p.act = act; p.eps = eps; p.t = t;
    for (int f = 0; f < kEmMaxFeats; ++f) p.off[f] = codes && f < num_feats ? offsets[f] : 0;
    p.row = row; p.col = col; p.eid = eid; p.indptr = indptr;
    p.E = (int)num_edges; p.chunk = chunk_edges_for(num_edges); p.n_chunks = (int)ceil_div(num_edges, p.chunk);
    p.out_rows = num_nodes; p.n_csr_rows = num_nodes;
}

}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_edge_message_workspace_bytes(int64_t num_edges, int64_t d, int32_t reduce) {
    if (num_edges <= 0 || d <= 0) return 256;
    const int64_t n_chunks = ceil_div(num_edges, chunk_edges_for(num_edges));
    return SplitWs(n_chunks, (reduce == 1 ? 3 : 1) * d, sizeof(float)).bytes() + 256;
}

extern "C" size_t pglamd_edge_message_backward_workspace_bytes(int64_t num_edges, int64_t d, int64_t table_rows) {
    if (num_edges <= 0 || d <= 0) return 256;
    const int64_t n_chunks = ceil_div(num_edges, chunk_edges_for(num_edges));
    const int64_t nb = em_walk_blocks(n_chunks, table_rows > 0);
    return SplitWs(n_chunks, d, sizeof(float)).bytes() + align_up((size_t)nb * (table_rows > 0 ? table_rows : 0) * d * sizeof(float), 256) +
           align_up((size_t)nb * 16 * kWave * sizeof(float), 256) + 256;
}

extern "C" int32_t pglamd_edge_message(const float* x, const float* edge_feat, const int32_t* codes, const float* table,
                                       const int32_t* offsets, int64_t num_feats, int64_t table_rows, int64_t d, int32_t act,
                                       int32_t reduce, float eps, float t, const int32_t* row, const int32_t* col, const int32_t* eid,
                                       const int64_t* indptr, int64_t num_edges, int64_t num_nodes, float* out, float* lse,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    PGLAMD_TRY(em_check("edge_message", x, edge_feat, codes, table, offsets, num_feats, table_rows, d, act, reduce, eps, t, num_edges, num_nodes, false));
    const bool softmax = reduce == 1, coded = table != nullptr;
    if (!out || !indptr || (softmax && !lse) || (num_edges > 0 && (!row || !col))) return fail(PGLAMD_E_ARG, "edge_message: bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_nodes == 0) return PGLAMD_OK;
    if (num_edges == 0) {
        PGLAMD_TRY(em_zero(out, num_nodes * d, st));
        return softmax ? em_zero(lse, num_nodes * d, st) : PGLAMD_OK;
    }
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 256 || workspace_bytes < pglamd_edge_message_workspace_bytes(num_edges, d, reduce))
        return fail(PGLAMD_E_WORKSPACE, "edge_message: workspace too small or misaligned");
    const int vec = em_vec(d, {x, edge_feat, table, out, lse});
    EmParams p{};
    em_set(p, x, edge_feat, codes, table, offsets, num_feats, table_rows, d, vec, act, eps, t, row, col, eid, indptr, num_edges, num_nodes);
    p.out = out; p.lse_out = lse;
    SplitWs(p.n_chunks, (int64_t)(softmax ? 3 : 1) * d, sizeof(float)).carve(p, workspace);
    const unsigned tiles = (unsigned)ceil_div(d, (int64_t)kWave * vec);
    const size_t lds = coded ? (size_t)p.T * p.tcols * sizeof(float) : 0;
    return em_dispatch(vec, softmax, coded, [&](auto v, auto sm, auto cd) {
        constexpr int VEC = decltype(v)::value;
        constexpr bool SM = decltype(sm)::value, CD = decltype(cd)::value;
        return launch_chunked_rows(p, st, [&](dim3 grid, const EmParams& q) {
            hipLaunchKernelGGL((em_forward_kernel<VEC, SM, CD>), dim3(grid.x, tiles), dim3(kBlock), lds, st, q);
        }, [&](const EmParams& q) { return launch_em_fixups<VEC, SM>(q, tiles, st); });
    });
}

extern "C" int32_t pglamd_edge_message_backward(const float* grad_out, const float* x, const float* edge_feat, const int32_t* codes,
                                                const float* table, const int32_t* offsets, int64_t num_feats, int64_t table_rows,
                                                int64_t d, int32_t act, int32_t reduce, float eps, float t, const float* out,
                                                const float* lse, const int32_t* src_row, const int32_t* src_col,
                                                const int32_t* src_eid, const int64_t* src_indptr, int64_t num_edges,
                                                int64_t num_nodes, float* grad_x, float* grad_edge_feat, float* grad_table,
                                                float* grad_t, void* workspace, size_t workspace_bytes, void* stream) {
    PGLAMD_TRY(em_check("edge_message_backward", x, edge_feat, codes, table, offsets, num_feats, table_rows, d, act, reduce, eps, t, num_edges,
                        num_nodes, true));
    const bool softmax = reduce == 1, coded = table != nullptr;
    if (num_edges > 0 && (!grad_out || !src_row || !src_col || !src_indptr || (softmax && (!out || !lse))))
        return fail(PGLAMD_E_ARG, "edge_message_backward: bad argument");
    if ((grad_table && !coded) || (grad_edge_feat && coded) || (grad_t && !softmax))
        return fail(PGLAMD_E_ARG, "edge_message_backward: a gradient was asked of an operand the call does not have");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_edges == 0 || num_nodes == 0) {
        PGLAMD_TRY(em_zero(grad_x, num_nodes * d, st));
        PGLAMD_TRY(em_zero(grad_table, table_rows * d, st));
        return em_zero(grad_t, 1, st);
    }
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 256 ||
        workspace_bytes < pglamd_edge_message_backward_workspace_bytes(num_edges, d, coded ? table_rows : 0))
        return fail(PGLAMD_E_WORKSPACE, "edge_message_backward: workspace too small or misaligned");
    const int vec = em_vec(d, {grad_out, x, edge_feat, table, out, lse, grad_x, grad_edge_feat});
    EmParams p{};
    em_set(p, x, edge_feat, codes, table, offsets, num_feats, table_rows, d, vec, act, eps, t, src_row, src_col, src_eid, src_indptr, num_edges,
           num_nodes);
    p.g = grad_out; p.fwd_out = out; p.lse = lse; p.out = grad_x; p.grad_ef = grad_edge_feat;
    const SplitWs split(p.n_chunks, d, sizeof(float));
    split.carve(p, workspace);
    const int64_t walk = em_walk_blocks(p.n_chunks, coded);
    const unsigned tiles = (unsigned)ceil_div(d, (int64_t)kWave * vec);
    float* tab_part = reinterpret_cast<float*>(static_cast<char*>(workspace) + split.bytes());
    float* dt_part = tab_part + align_up((size_t)walk * (coded ? table_rows : 0) * d * sizeof(float), 256) / sizeof(float);
    p.tab_part = grad_table ? tab_part : nullptr;
    p.dt_part = grad_t ? dt_part : nullptr;
    const size_t lds = coded && grad_table ? (size_t)kWavesPerBlock * p.T * p.tcols * sizeof(float) : 0;
    PGLAMD_TRY(em_dispatch(vec, softmax, coded, [&](auto v, auto sm, auto cd) {
        constexpr int VEC = decltype(v)::value;
        constexpr bool SM = decltype(sm)::value, CD = decltype(cd)::value;
        return launch_chunked_rows(p, st, [&](dim3 grid, const EmParams& q) {
            EmParams w = q;                                 // the capped walk: `walk` blocks share the q.n_grid_chunks chunk groups
            w.n_logical = q.n_grid_chunks; w.n_grid_chunks = (int)walk;
            hipLaunchKernelGGL((em_backward_kernel<VEC, SM, CD>), dim3(grid.x - q.n_grid_chunks + (unsigned)walk, tiles), dim3(kBlock), lds, st, w);
        }, [&](const EmParams& q) { return q.out ? launch_em_fixups<VEC, false>(q, tiles, st) : PGLAMD_OK; });
    }));
    if (grad_table) {
        const int64_t n = table_rows * d;
        hipLaunchKernelGGL(em_sum_partials_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, st, tab_part, (int)walk, n, grad_table);
        PGLAMD_LAUNCH_CHECK();
    }
    if (grad_t) {
        hipLaunchKernelGGL(em_sum_scalars_kernel, dim3(1), dim3(kBlock), 0, st, dt_part, (int)(walk * tiles), grad_t);
        PGLAMD_LAUNCH_CHECK();
    }
    return PGLAMD_OK;
}
