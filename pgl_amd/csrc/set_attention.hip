// set_attention.hip -- the dense attention of a multi-head attention block over small sets (SelfAtt of GraphMultisetTransformer: MAB,
// pgl/nn/gmt_pool.py:28-112) on fp32 MFMA tiles, one launch per direction.  The reference takes the softmax over the QUERY axis
// (pgl/nn/gmt_pool.py:97-100), so a key column's weights depend on that column and on all the queries: a wave that owns a block of key
// columns holds the whole softmax, forward and backward, with no running maximum and no saved statistics.
//
//   s[b,i,j,h]      = key_bias[b,j] + scale <Q[b,i, head h], K[b,j, head h]>      head h = columns h hd .. (h + 1) hd - 1, scale = 1 / sqrt(dim)
//   A[b,:,j,h]      = softmax of s[b,:,j,h] over i
//   out[b,i, head h] = residual Q[b,i, head h] + sum_j A[b,i,j,h] V[b,j, head h]
// backward from G = d out, S and A recomputed by the forward's own expressions (the same bits), t[i,j] = <G[i], V[j]> per head,
// ds[i,j] = A[i,j] (t[i,j] - sum_i' A[i',j] t[i',j]):
//   dV[j] = sum_i A[i,j] G[i]      dK[j] = scale sum_i ds[i,j] Q[i]      dQ[i] = residual G[i] + scale sum_j ds[i,j] K[j]
// Nothing is saved for the backward but the inputs.
//
// Unit of work: a PAIR (graph b, head h).  nq, nk <= 128: at most 4 query tiles x 4 key blocks of 32.
//   waves     a workgroup is 4 waves; a pair takes WPP = 1 / 2 / 4 of them (the key blocks rounded up to a power of two; more when
//             4 / WPP pairs would not fit the LDS), so
//             4 / WPP pairs are packed into a workgroup and sets of <= 32 keys still give every wave a tile.  Wave kb of a pair owns
//             the key columns 32 kb .. 32 kb + 31.  The grid strides over the groups of pairs under kSetGridCap.
//   operands  the head slices of Q, K (and G, V in the backward) go to LDS with 16-byte lane loads, CH = min(hd, 32) columns at a
//             time (any hd up to 256 passes through the same 32-column chunk loop), rows 33 floats apart: the MFMA operand reads
//             (lane -> row) then fall on distinct banks.  Only rows < nq / nk are staged; a tile row past the end reads the last
//             real row and its weight is forced to exactly 0, so nothing outside the operands is read or written.
//   scores    S = Q K^T by v_mfma_f32_32x32x2_f32, QT = ceil(nq / 32) accumulator tiles per wave (a compile-time tier).  In the
//             accumulator a LANE is a key column (lane % 32) and the 16 registers x QT tiles x 2 half-waves are its query rows: the
//             column's maximum and sum are taken over the lane's registers in order, then with the other half-wave (a + b == b + a).
//   A V       contracts over the lane index, so A is laid out through LDS once ([nq][32 KB + 1]) and the output tiles (query tile x
//             32 head columns) are dealt to the pair's waves; each tile contracts over ALL nk keys in one accumulator chain, in key
//             order: no partial outputs exist and nothing is added across waves.  residual Q is added at the store.
//   backward  t = G V^T beside S in a second set of accumulators; the column sums of A t are lane-local like the softmax.  dV = A^T G
//             and dK = ds^T Q contract over the REGISTER index: the accumulators are the MFMA operand as they stand (step (tile, r)
//             takes register r of both half-waves, i.e. two query rows), wave-local, no LDS round trip.  Only ds goes through LDS,
//             for dQ = ds K, dealt to the waves like the forward's A V.
// LDS per pair: 33 (nq8 + nk) floats of operands, nq8 = nq rounded up to 8 (twice that in the backward) + nq (32 KB + 1) of A / ds: <= 100 KiB forward,
// <= 134 KiB backward at 128 x 128, 2.7 KiB at 8 x 8; occupancy figures in profiles/set_attention/kernel_resources.txt.
// No atomics, no workspace; every sum has one fixed order that depends on the shape alone, so results are a pure function of the
// arguments, bit for bit, whichever gradients are asked for.  Addresses are int64; every loop is bounded by nq, nk, hd or a tile count.
#include "common.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace pglamd {
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kSetMaxN = 128, kSetMinDim = 4, kSetMaxDim = 256;
constexpr int kSetTile = 32;
constexpr int kSetChunk = 32;                        // head columns staged at a time
constexpr int kSetLd = kSetChunk + 1;                // floats between staged rows (a constant: the operand reads take immediate offsets)
constexpr int64_t kSetGridCap = 256 * 8;            // workgroups per launch; the kernel strides beyond it
constexpr size_t kSetLdsMax = 160 * 1024;

struct SetArgs {
    const float* Q; const float* K; const float* V; const float* bias;         // bias NULL: nothing is added
    const float* G;                                                            // d out (backward)
    float* out; float* dQ; float* dK; float* dV;                               // a NULL gradient is not computed
    int64_t pairs, groups;                           // B * heads; ceil(pairs / pairs per workgroup)
    int nq, nk, nq8, dim, hd, heads, ch, nkb, wpp_shift, residual;    // nq8: nq rounded up to 8
    int pair_floats;                                 // LDS floats of one pair
    float scale;
};

// Row of accumulator register r in a 32 x 32 tile for the half-wave `half` (the column is lane % 32).
__device__ __forceinline__ int acc_row(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }

__device__ __forceinline__ f16v mfma(float a, float b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ f16v zero16() {
    f16v z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// rows x ch floats from src (row stride dim, 16-byte aligned rows) -> dst (row stride kSetLd), by the `threads` threads of a pair; the
// rows from `rows` up to `pad` are filled with zeros.
__device__ __forceinline__ void stage(float* dst, const float* src, int rows, int pad, int ch, int dim, int tid, int threads) {
    const int q4 = ch >> 2;
    for (int idx = tid; idx < pad * q4; idx += threads) {
        const int r = idx / q4, c = (idx - r * q4) << 2;
        const float4 v = r < rows ? *reinterpret_cast<const float4*>(src + (int64_t)r * dim + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        float* d = dst + r * kSetLd + c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}

// acc[qt] += X[32 qt .. , :ch] Y[32 kb .. , :ch]^T over the staged chunk (sx: nx rows, sy: ny rows; rows past the end: the last row).
template <int QT>
__device__ __forceinline__ void score_tiles(f16v (&acc)[QT], const float* sx, int nx, const float* sy, int ny, int kb, int ch, int l32, int half) {
    constexpr int ld = kSetLd;
    const float* y = sy + min(kb * kSetTile + l32, ny - 1) * ld + half;
    const float* x[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) x[qt] = sx + min(qt * kSetTile + l32, nx - 1) * ld + half;
    for (int c = 0; c < ch; c += 2) {
        const float b = y[c];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[qt] = mfma(x[qt][c], b, acc[qt]);
    }
}

// The raw dots of this lane's key column -> its softmax over the nq queries of bias + scale dot; rows >= nq and a column >= nk: exactly 0.
template <int QT>
__device__ __forceinline__ void column_softmax(f16v (&s)[QT], float bias, float scale, int nq, bool col_ok, int half) {
    float m = -INFINITY, l = 0.f;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (qt * kSetTile + acc_row(r, half) < nq) { s[qt][r] = fmaf(scale, s[qt][r], bias); m = fmaxf(m, s[qt][r]); }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 32, kWave));
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (qt * kSetTile + acc_row(r, half) < nq) { s[qt][r] = expf(s[qt][r] - m); l += s[qt][r]; }
        }
    }
    l += __shfl_xor(l, 32, kWave);
    const float inv = 1.f / l;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[qt][r] = (col_ok && qt * kSetTile + acc_row(r, half) < nq) ? s[qt][r] * inv : 0.f;
    }
}

// The lane's column of `w` (rows < nq) -> sw [nq][lw] at column kb 32 + l32.
template <int QT>
__device__ __forceinline__ void put_columns(float* sw, int lw, const f16v (&w)[QT], int nq, int kb, int l32, int half) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = qt * kSetTile + acc_row(r, half);
            if (i < nq) sw[i * lw + kb * kSetTile + l32] = w[qt][r];
        }
    }
}

// sum_j sw[32 qt + lane row][j] sy[j][lane column] over ALL nk keys, in key order: one output tile (32 queries x 32 head columns).
__device__ __forceinline__ f16v row_tile(const float* sw, int lw, int nq, const float* sy, int nk, int ch, int qt, int l32, int half) {
    const float* a = sw + min(qt * kSetTile + l32, nq - 1) * lw + half;
    const float* b = sy + min(l32, ch - 1);
    constexpr int ld = kSetLd;
    f16v acc = zero16();
    for (int j = 0; j < nk; j += 2) {
        const int jj = j + half;                                                  // (jj == nk: a column whose weights are 0)
        acc = mfma(a[j], jj < nk ? b[jj * ld] : 0.f, acc);
    }
    return acc;
}

// sum_i w[i][lane's key] sx[i][lane column]: the accumulators are the operand; step (qt, r) contracts the rows acc_row(r, 0 / 1).  A
// group of 8 rows that lies past nq is skipped; sx is zero-filled up to the next multiple of 8 rows and w is exactly 0 there.
template <int QT>
__device__ __forceinline__ f16v column_tile(const f16v (&w)[QT], const float* sx, int nq, int ch, int l32, int half) {
    const float* x = sx + min(l32, ch - 1) + 4 * half * kSetLd;
    f16v acc = zero16();
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (qt * kSetTile + 8 * (r >> 2) < nq) acc = mfma(w[qt][r], x[(qt * kSetTile + acc_row(r, 0)) * kSetLd], acc);
        }
    }
    return acc;
}

struct Where {
    int wave, lane, l32, half, slot, kb, wpp, tid, threads;
    int64_t pair, b; int h; bool ok;
};

__device__ __forceinline__ Where where(const SetArgs& a, int64_t group) {
    Where w;
    w.wave = threadIdx.x >> 6; w.lane = threadIdx.x & (kWave - 1);
    w.l32 = w.lane & 31; w.half = w.lane >> 5;
    w.wpp = 1 << a.wpp_shift;
    w.slot = w.wave >> a.wpp_shift; w.kb = w.wave & (w.wpp - 1);
    w.tid = w.kb * kWave + w.lane; w.threads = w.wpp * kWave;
    w.pair = group * (kWavesPerBlock >> a.wpp_shift) + w.slot;
    w.ok = w.pair < a.pairs;
    w.b = w.ok ? w.pair / a.heads : 0; w.h = w.ok ? (int)(w.pair % a.heads) : 0;
    return w;
}

template <int QT>
__global__ __launch_bounds__(kBlock, QT <= 2 ? 4 : 2) void set_forward_kernel(SetArgs a) {
    extern __shared__ __align__(16) float s_set[];
    const int nq = a.nq, nk = a.nk, dim = a.dim, ch = a.ch, ld = kSetLd, lw = a.nkb * kSetTile + 1;
    for (int64_t group = blockIdx.x; group < a.groups; group += gridDim.x) {
        const Where w = where(a, group);
        float* sx = s_set + w.slot * a.pair_floats;          // Q chunk [nq][ld]
        float* sy = sx + a.nq8 * ld;                         // K chunk, then V chunk [nk][ld]
        float* sw = sy + nk * ld;                            // A [nq][lw]
        const int64_t qoff = w.b * nq * (int64_t)dim + w.h * a.hd, koff = w.b * nk * (int64_t)dim + w.h * a.hd;
        const bool mine = w.ok && w.kb < a.nkb;
        f16v s[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) s[qt] = zero16();
        for (int c0 = 0; c0 < a.hd; c0 += ch) {
            if (w.ok) {
                stage(sx, a.Q + qoff + c0, nq, a.nq8, ch, dim, w.tid, w.threads);
                stage(sy, a.K + koff + c0, nk, nk, ch, dim, w.tid, w.threads);
            }
            __syncthreads();
            if (mine) score_tiles<QT>(s, sx, nq, sy, nk, w.kb, ch, w.l32, w.half);
            __syncthreads();
        }
        if (mine) {
            const int j = w.kb * kSetTile + w.l32;
            const float bias = (a.bias && j < nk) ? a.bias[w.b * nk + j] : 0.f;
            column_softmax<QT>(s, bias, a.scale, nq, j < nk, w.half);
            put_columns<QT>(sw, lw, s, nq, w.kb, w.l32, w.half);
        }
        for (int c0 = 0; c0 < a.hd; c0 += ch) {
            if (w.ok) stage(sy, a.V + koff + c0, nk, nk, ch, dim, w.tid, w.threads);
            __syncthreads();                                                      // (the first pass: A is complete too)
            if (w.ok) {
                for (int qt = w.kb; qt < QT; qt += w.wpp) {
                    const f16v acc = row_tile(sw, lw, nq, sy, nk, ch, qt, w.l32, w.half);
                    if (w.l32 < ch) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int i = qt * kSetTile + acc_row(r, w.half);
                            if (i < nq) {
                                const int64_t at = qoff + (int64_t)i * dim + c0 + w.l32;
                                a.out[at] = a.residual ? a.Q[at] + acc[r] : acc[r];
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

template <int QT>
__global__ __launch_bounds__(kBlock, QT <= 2 ? 2 : 1) void set_backward_kernel(SetArgs a) {
    extern __shared__ __align__(16) float s_set[];
    const int nq = a.nq, nk = a.nk, dim = a.dim, ch = a.ch, ld = kSetLd, lw = a.nkb * kSetTile + 1;
    for (int64_t group = blockIdx.x; group < a.groups; group += gridDim.x) {
        const Where w = where(a, group);
        float* sx = s_set + w.slot * a.pair_floats;          // Q chunk [nq8][ld], rows nq .. nq8 - 1 zero
        float* sy = sx + a.nq8 * ld;                         // K chunk [nk][ld]
        float* sg = sy + nk * ld;                            // G chunk [nq8][ld]
        float* sv = sg + a.nq8 * ld;                            // V chunk [nk][ld]
        float* sw = sv + nk * ld;                            // ds [nq][lw]
        const int64_t qoff = w.b * nq * (int64_t)dim + w.h * a.hd, koff = w.b * nk * (int64_t)dim + w.h * a.hd;
        const bool mine = w.ok && w.kb < a.nkb;
        f16v s[QT], t[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) { s[qt] = zero16(); t[qt] = zero16(); }
        for (int c0 = 0; c0 < a.hd; c0 += ch) {
            if (w.ok) {
                stage(sx, a.Q + qoff + c0, nq, a.nq8, ch, dim, w.tid, w.threads);
                stage(sy, a.K + koff + c0, nk, nk, ch, dim, w.tid, w.threads);
                stage(sg, a.G + qoff + c0, nq, a.nq8, ch, dim, w.tid, w.threads);
                stage(sv, a.V + koff + c0, nk, nk, ch, dim, w.tid, w.threads);
            }
            __syncthreads();
            if (mine) {
                score_tiles<QT>(s, sx, nq, sy, nk, w.kb, ch, w.l32, w.half);      // (the forward's expressions: the same bits)
                score_tiles<QT>(t, sg, nq, sv, nk, w.kb, ch, w.l32, w.half);
            }
            __syncthreads();
        }
        const int j = w.kb * kSetTile + w.l32;
        if (mine) {
            const float bias = (a.bias && j < nk) ? a.bias[w.b * nk + j] : 0.f;
            column_softmax<QT>(s, bias, a.scale, nq, j < nk, w.half);
            float c = 0.f;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (qt * kSetTile + acc_row(r, w.half) < nq) c = fmaf(s[qt][r], t[qt][r], c);
            }
            c += __shfl_xor(c, 32, kWave);
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    t[qt][r] = (j < nk && qt * kSetTile + acc_row(r, w.half) < nq) ? s[qt][r] * (t[qt][r] - c) : 0.f;
            }
            if (a.dQ) put_columns<QT>(sw, lw, t, nq, w.kb, w.l32, w.half);
        }
        for (int c0 = 0; c0 < a.hd; c0 += ch) {
            if (w.ok && a.hd > ch) {                                              // (one chunk: it is still there)
                if (a.dK) stage(sx, a.Q + qoff + c0, nq, a.nq8, ch, dim, w.tid, w.threads);
                if (a.dQ) stage(sy, a.K + koff + c0, nk, nk, ch, dim, w.tid, w.threads);
                if (a.dV) stage(sg, a.G + qoff + c0, nq, a.nq8, ch, dim, w.tid, w.threads);
            }
            __syncthreads();                                                      // (the first pass: ds is complete too)
            if (mine) {                                                          // dV, then dK: one output tile alive at a time
                for (int which = 0; which < 2; ++which) {
                    float* dst = which ? a.dK : a.dV;
                    if (!dst) continue;
                    const f16v acc = which ? column_tile<QT>(t, sx, nq, ch, w.l32, w.half) : column_tile<QT>(s, sg, nq, ch, w.l32, w.half);
                    if (w.l32 < ch) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int jr = w.kb * kSetTile + acc_row(r, w.half);
                            if (jr < nk) dst[koff + (int64_t)jr * dim + c0 + w.l32] = which ? a.scale * acc[r] : acc[r];
                        }
                    }
                }
            }
            if (w.ok && a.dQ) {
                for (int qt = w.kb; qt < QT; qt += w.wpp) {
                    const f16v acc = row_tile(sw, lw, nq, sy, nk, ch, qt, w.l32, w.half);
                    if (w.l32 < ch) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int i = qt * kSetTile + acc_row(r, w.half);
                            if (i < nq) {
                                const int64_t at = qoff + (int64_t)i * dim + c0 + w.l32;
                                a.dQ[at] = a.residual ? fmaf(a.scale, acc[r], a.G[at]) : a.scale * acc[r];
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool shape_ok(int64_t nq, int64_t nk, int64_t dim, int64_t heads) {
    if (nq < 1 || nq > kSetMaxN || nk < 1 || nk > kSetMaxN || dim < kSetMinDim || dim > kSetMaxDim || heads < 1 || dim % heads != 0) return false;
    const int64_t hd = dim / heads;
    return hd >= 4 && (hd & (hd - 1)) == 0;
}

// The checks both entry points share; fills everything of `a` but the outputs.  -> the dynamic LDS bytes through *lds.
int32_t set_common(const char* what, SetArgs& a, const float* Q, const float* K, const float* V, const float* key_bias, int64_t batch,
                   int64_t nq, int64_t nk, int64_t dim, int64_t heads, bool backward, size_t* lds) {
    if (!shape_ok(nq, nk, dim, heads))
        return fail(PGLAMD_E_ARG, "%s: (nq, nk, dim, heads) = (%lld, %lld, %lld, %lld) outside 1 <= nq, nk <= %d, %d <= dim <= %d, dim %% heads == 0, dim / heads a power of two >= 4",
                    what, (long long)nq, (long long)nk, (long long)dim, (long long)heads, kSetMaxN, kSetMinDim, kSetMaxDim);
    if (batch < 0 || batch > (INT64_MAX >> 20)) return fail(PGLAMD_E_ARG, "%s: bad batch count", what);
    if (batch > 0 && (!Q || !K || !V)) return fail(PGLAMD_E_ARG, "%s: NULL operand", what);
    if (!aligned16(Q) || !aligned16(K) || !aligned16(V)) return fail(PGLAMD_E_ARG, "%s: Q, K and V must be 16-byte aligned", what);
    a.Q = Q; a.K = K; a.V = V; a.bias = key_bias;
    a.nq = (int)nq; a.nk = (int)nk; a.dim = (int)dim; a.heads = (int)heads; a.hd = (int)(dim / heads);
    a.ch = std::min(a.hd, kSetChunk);
    a.nkb = (int)ceil_div(nk, kSetTile);
    a.wpp_shift = a.nkb <= 1 ? 0 : (a.nkb <= 2 ? 1 : 2);
    a.pairs = batch * heads;
    a.nq8 = (a.nq + 7) & ~7;
    a.pair_floats = (int)((backward ? 2 : 1) * (a.nq8 + nk) * kSetLd + nq * (a.nkb * kSetTile + 1));
    a.pair_floats = (a.pair_floats + 3) & ~3;
    // fewer pairs per workgroup when four or two of them do not fit the LDS (many queries on few keys): the pair's spare waves
    // still take output tiles
    while (a.wpp_shift < 2 && (size_t)(kWavesPerBlock >> a.wpp_shift) * a.pair_floats * sizeof(float) > kSetLdsMax) ++a.wpp_shift;
    const int per_group = kWavesPerBlock >> a.wpp_shift;
    a.groups = ceil_div(a.pairs, per_group);
    a.scale = 1.0f / sqrtf((float)dim);
    *lds = (size_t)per_group * a.pair_floats * sizeof(float);
    if (*lds > kSetLdsMax) return fail(PGLAMD_E_ARG, "%s: %zu bytes of LDS", what, *lds);
    return PGLAMD_OK;
}

template <int QT, bool BACKWARD> int32_t launch(const SetArgs& a, size_t lds, hipStream_t st) {
    const void* fn = BACKWARD ? reinterpret_cast<const void*>(&set_backward_kernel<QT>) : reinterpret_cast<const void*>(&set_forward_kernel<QT>);
    static bool attr_set = false;                             // (per instantiation; idempotent, so a race only repeats it)
    if (!attr_set) {
        PGLAMD_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSetLdsMax));
        attr_set = true;
    }
    const dim3 grid((unsigned)std::min<int64_t>(a.groups, kSetGridCap));
    if (BACKWARD) hipLaunchKernelGGL((set_backward_kernel<QT>), grid, dim3(kBlock), lds, st, a);
    else hipLaunchKernelGGL((set_forward_kernel<QT>), grid, dim3(kBlock), lds, st, a);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

template <bool BACKWARD> int32_t launch_tier(const SetArgs& a, size_t lds, hipStream_t st) {
    if (a.nq <= 32) return launch<1, BACKWARD>(a, lds, st);
    if (a.nq <= 64) return launch<2, BACKWARD>(a, lds, st);
    if (a.nq <= 96) return launch<3, BACKWARD>(a, lds, st);
    return launch<4, BACKWARD>(a, lds, st);
}

}  // namespace
}  // namespace pglamd

using namespace pglamd;

extern "C" int32_t pglamd_set_attention(const float* Q, const float* K, const float* V, const float* key_bias, int64_t batch, int64_t nq,
                                        int64_t nk, int64_t dim, int64_t heads, int32_t residual, float* out, void* stream) {
    SetArgs a{};
    size_t lds = 0;
    PGLAMD_TRY(set_common("set_attention", a, Q, K, V, key_bias, batch, nq, nk, dim, heads, false, &lds));
    if (batch > 0 && !out) return fail(PGLAMD_E_ARG, "set_attention: out is NULL");
    a.out = out; a.residual = residual != 0;
    if (a.pairs == 0) return PGLAMD_OK;
    return launch_tier<false>(a, lds, static_cast<hipStream_t>(stream));
}

extern "C" int32_t pglamd_set_attention_backward(const float* grad_out, const float* Q, const float* K, const float* V, const float* key_bias,
                                                 int64_t batch, int64_t nq, int64_t nk, int64_t dim, int64_t heads, int32_t residual,
                                                 float* grad_Q, float* grad_K, float* grad_V, void* stream) {
    SetArgs a{};
    size_t lds = 0;
    PGLAMD_TRY(set_common("set_attention_backward", a, Q, K, V, key_bias, batch, nq, nk, dim, heads, true, &lds));
    if ((batch > 0 && !grad_out) || !aligned16(grad_out)) return fail(PGLAMD_E_ARG, "set_attention_backward: grad_out NULL or not 16-byte aligned");
    if (!grad_Q && !grad_K && !grad_V) return fail(PGLAMD_E_ARG, "set_attention_backward: no gradient is needed");
    a.G = grad_out; a.residual = residual != 0;
    a.dQ = grad_Q; a.dK = grad_K; a.dV = grad_V;
    if (a.pairs == 0) return PGLAMD_OK;
    return launch_tier<true>(a, lds, static_cast<hipStream_t>(stream));
}
