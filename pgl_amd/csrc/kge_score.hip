// kge_score.hip -- knowledge-graph-embedding scores and loss over chunked negatives (apps/Graph4KG/models/score_funcs.py:76-257,
// loss_func.py:70-103): C chunks, each scoring cs positive triples against the SAME neg corrupted entities, without a [C, cs, neg]
// score tensor (training) and without the [C, cs, neg, d] operands the tensor recipe of RotatE tiles (score_funcs.py:167-217).
//
// ent [Ne, d], rel [Nr, dr] fp32 (dr = d; RotatE: d / 2), h, r, t int64 [P], P = C cs (positive i of chunk c is p = c cs + i),
// neg int64 [C, neg]; neg_head: the negatives replace the head (else the tail).  a = the query of a positive (its kept end combined with
// the relation), b = an entity row; pos[p] = phi(a_p, other end of p), s[c,i,j] = phi(a_{c,i}, ent[neg[c,j]]):
//     PGLAMD_KGE_TRANSE    a = h + r | t - r                   phi = gamma - sqrt(max(sum_k (a_k - b_k)^2, 1e-30))
//     PGLAMD_KGE_DISTMULT  a = h o r | t o r                   phi = sum_k a_k b_k
//     PGLAMD_KGE_COMPLEX   a = h r | t conj(r)   (complex)     phi = sum_k a_k b_k         (over all d floats: re and im halves)
//     PGLAMD_KGE_ROTATE    a = h e^{i th} | t e^{-i th}        phi = gamma - sum_{k < d/2} sqrt((a_re,k - b_re,k)^2 + (a_im,k - b_im,k)^2 + 1e-12)
//                          th = rel / ((gamma + 2) / (d / 2) / pi)
// (re = the first half of a row, im = the second).  TransE takes the difference directly, not the |a|^2 + |b|^2 - 2ab expansion of
// score_funcs.py:100-108, which cancels in fp32.  Loss ("Logsigmoid", not pairwise, weights = None), tau = the adversarial temperature:
//     loss = (mean_p softplus(-pos_p) + mean_p sum_j w[p,j] softplus(s[p,j])) / 2,   w[p,:] = softmax_j(tau s[p,:]), no gradient through w
// tau = 0 gives w = 1 / neg, the plain mean, through the same expressions.
//
// FORWARD.  Unit of work: (chunk c, a tile of 32 positives, a SUPERBLOCK of 128 negatives); each of the 4 waves owns one 32 x 32 tile
// of pairs.  (The design of record let a workgroup sweep all negatives of its tile; at C cs = 1024 that is 32 workgroups on 256 CUs, so
// the sweep is dealt to workgroups instead and the per-positive softmax state (m, Z, W) = (max tau s, sum e^{tau s - m}, sum e^{tau s - m}
// softplus(s)) of every 32-negative block goes to a [P, neg / 32, 3] workspace, merged in block order by kge_finish_kernel.)
//   operands  the components are walked in chunks of 32; for the complex models re and im of the same 32 components are staged side
//             by side.  The query rows are formed at staging: gather the kept end and the relation by id, combine, one sincosf per
//             (positive, component) for RotatE.  Negatives are gathered by id with 16-byte lane loads.  LDS rows are 33 floats apart.
//   scores    bilinear family: S^T = B A^T on v_mfma_f32_32x32x2_f32, so a LANE is a positive and its 16 registers (x 2 half-waves)
//             are negatives: the softmax state of a positive is lane-local (the scores-only entry swaps the operands: a lane is a
//             negative and the stores run along j).  Distance family: a 4 x 4 register micro-tile of pairs per lane on the VALU, 8 LDS
//             reads per 16 pairs; the 8 lanes that share 4 positives merge their states by a butterfly.
//   positive  score by the unit of superblock 0 (the other end is one more gathered row), 8 lanes a positive.
// BACKWARD.  c[i,j] = d loss / d s[i,j] = w[i,j] sigma(s[i,j]) / (2P) from scores recomputed tile by tile and the saved (m, Z) [P].
//   pass 1    workgroup owns (c, 32 positives), sweeps the negatives: d a_i = sum_j c[i,j] d phi / d a, then the positive score's
//             gradient and the chain rule to the gathered rows: g_kept, g_other [P, d], g_rel [P, dr].
//   pass 2    workgroup owns (c, 32 negatives), sweeps the chunk's positives: g_neg [C, neg, d].
//   Both: per superblock of 128 swept rows, phase A recomputes the score tiles and leaves the coefficients in LDS [32][129]; phase B
//   walks the component chunks again, a thread owning (owner row, 4 components) and summing over the swept rows in order.  The owner's
//   row gradient accumulates in its own output row (same thread, same address).  Every output row has one owner and one order: no
//   atomics, bit-reproducible.  The sums by id into d ent / d rel are the caller's (the engine's aggregation).
// Tile rows and columns past cs / neg are staged as zeros and masked out of every sum; an id outside its table reads nothing.
#include "common.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace pglamd {
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kKgeTile = 32;                          // positives per tile, negatives per wave tile
constexpr int kKgeSuper = kKgeTile * kWavesPerBlock;  // swept rows per superblock
constexpr int kKgeChunk = 32;                         // components staged at a time
constexpr int kKgeLd = kKgeChunk + 1;                 // floats between staged rows
constexpr int kKgeLdc = kKgeSuper + 1;                // floats between coefficient rows
constexpr int kKgeMaxD = 1024;                        // the widest row tested; the column-chunk loop itself has no limit
constexpr int64_t kKgeGridCap = 256 * 8;

struct KgeArgs {
    const float* ent; const float* rel;
    const int64_t* h; const int64_t* r; const int64_t* t; const int64_t* neg;
    float* pos; float* scores;                        // [P]; [C, cs, neg] (scores-only entry)
    float* part;                                      // [P, njb, 3]
    const float* mz;                                  // [P, 2] (backward)
    float* g_kept; float* g_other; float* g_rel; float* g_neg;
    int64_t units, num_ent, num_rel;
    int C, cs, nneg, d, nc, n_it, n_sb, njb, neg_head;
    float gamma, tau, scale, inv_2p;                  // scale: RotatE's (gamma + 2) / (d / 2) / pi
};

constexpr bool kge_dist(int M) { return M == PGLAMD_KGE_TRANSE || M == PGLAMD_KGE_ROTATE; }
constexpr int kge_planes(int M) { return M >= PGLAMD_KGE_COMPLEX ? 2 : 1; }

__device__ __forceinline__ int acc_row(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }
__device__ __forceinline__ f16v mfma(float a, float b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f16v zero16() {
    f16v z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

struct F4 { float v[4]; };
__device__ __forceinline__ F4 row4(const float* tab, int64_t id, int64_t n, int64_t ld, int off) {
    F4 o{};
    if (id >= 0 && id < n) {
        const float4 x = *reinterpret_cast<const float4*>(tab + id * ld + off);
        o.v[0] = x.x; o.v[1] = x.y; o.v[2] = x.z; o.v[3] = x.w;
    }
    return o;
}
__device__ __forceinline__ void put4(float* d, const F4& x) { d[0] = x.v[0]; d[1] = x.v[1]; d[2] = x.v[2]; d[3] = x.v[3]; }

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid(float x) {
    const float t = expf(-fabsf(x));
    return x >= 0.f ? 1.f / (1.f + t) : t / (1.f + t);
}

// (m, Z, W) of two sets of negatives -> of their union; symmetric in its arguments bit for bit; m = -inf: the empty set
__device__ __forceinline__ void merge(float& m, float& Z, float& W, float m2, float Z2, float W2) {
    const float mm = fmaxf(m, m2);
    const float ea = m == -INFINITY ? 0.f : expf(m - mm), eb = m2 == -INFINITY ? 0.f : expf(m2 - mm);
    Z = Z * ea + Z2 * eb;
    W = W * ea + W2 * eb;
    m = mm;
}

// `rows` entity rows, components c0 .. c0 + ch - 1 -> dst [planes][rows][kKgeLd]; row r is ent[ids[first + r]], zeros past `count`
template <int M>
__device__ __forceinline__ void stage_ent(const KgeArgs& a, float* dst, int rows, const int64_t* ids, int first, int count, int c0, int ch) {
    constexpr int PL = kge_planes(M);
    const int q4 = ch >> 2;
    for (int idx = threadIdx.x; idx < rows * q4; idx += kBlock) {
        const int r = idx / q4, cc = (idx - r * q4) << 2;
        const int64_t id = first + r < count ? ids[first + r] : -1;
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) put4(dst + (pl * rows + r) * kKgeLd + cc, row4(a.ent, id, a.num_ent, a.d, pl * a.nc + c0 + cc));
    }
}

// the queries of the positives first .. first + rows - 1 of chunk c -> sa; optionally the kept end -> se, the relation (RotatE: cos,
// sin) -> sr, the other end -> so, all [planes][rows][ld]; zeros past cs
template <int M>
__device__ __forceinline__ void stage_query(const KgeArgs& a, int rows, int c, int first, int c0, int ch, float* sa, float* se, float* sr, float* so,
                                            int ld = kKgeLd) {
    constexpr int PL = kge_planes(M);
    const int q4 = ch >> 2;
    for (int idx = threadIdx.x; idx < rows * q4; idx += kBlock) {
        const int r = idx / q4, cc = (idx - r * q4) << 2;
        const bool ok = first + r < a.cs;
        const int64_t p = (int64_t)c * a.cs + first + r;
        const int64_t hid = ok ? a.h[p] : -1, tid = ok ? a.t[p] : -1, rid = ok ? a.r[p] : -1;
        const int64_t kept = a.neg_head ? tid : hid, other = a.neg_head ? hid : tid;
        F4 e[PL], rr[PL], q[PL];
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) e[pl] = row4(a.ent, kept, a.num_ent, a.d, pl * a.nc + c0 + cc);
        if constexpr (M == PGLAMD_KGE_ROTATE) {
            const F4 th = row4(a.rel, rid, a.num_rel, a.nc, c0 + cc);
#pragma unroll
            for (int k = 0; k < 4; ++k) sincosf(th.v[k] / a.scale, &rr[1].v[k], &rr[0].v[k]);
        } else {
#pragma unroll
            for (int pl = 0; pl < PL; ++pl) rr[pl] = row4(a.rel, rid, a.num_rel, a.d, pl * a.nc + c0 + cc);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (M == PGLAMD_KGE_TRANSE) q[0].v[k] = a.neg_head ? e[0].v[k] - rr[0].v[k] : e[0].v[k] + rr[0].v[k];
            else if constexpr (M == PGLAMD_KGE_DISTMULT) q[0].v[k] = e[0].v[k] * rr[0].v[k];
            else if (a.neg_head) {
                q[0].v[k] = e[0].v[k] * rr[0].v[k] + e[1].v[k] * rr[1].v[k];
                q[1].v[k] = e[1].v[k] * rr[0].v[k] - e[0].v[k] * rr[1].v[k];
            } else {
                q[0].v[k] = e[0].v[k] * rr[0].v[k] - e[1].v[k] * rr[1].v[k];
                q[1].v[k] = e[0].v[k] * rr[1].v[k] + e[1].v[k] * rr[0].v[k];
            }
        }
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) {
            const int at = (pl * rows + r) * ld + cc;
            put4(sa + at, q[pl]);
            if (se) put4(se + at, e[pl]);
            if (sr) put4(sr + at, rr[pl]);
            if (so) put4(so + at, row4(a.ent, other, a.num_ent, a.d, pl * a.nc + c0 + cc));
        }
    }
}

// the pair (x row, y row of the wave's 32) that element e of a lane's tile stands for
template <int M, bool SWAP> __device__ __forceinline__ int tile_x(int e, int lane) {
    if constexpr (kge_dist(M)) return (lane >> 3) * 4 + (e >> 2);
    else return SWAP ? acc_row(e, lane >> 5) : (lane & 31);
}
template <int M, bool SWAP> __device__ __forceinline__ int tile_y(int e, int lane) {
    if constexpr (kge_dist(M)) return (lane & 7) * 4 + (e & 3);
    else return SWAP ? (lane & 31) : acc_row(e, lane >> 5);
}

// (s, lo) += t without losing t's low bits: s + lo carries the sum over d to about an ulp of its terms, however long the row (a plain
// fp32 chain over d = 512 loses ~1e-4 of a RotatE score, which the softmax weights and sigma then multiply into every coefficient)
__device__ __forceinline__ void two_sum(f16v& s, f16v& lo, const f16v& t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const float sum = s[e] + t[e], bp = sum - s[e];
        lo[e] += (s[e] - (sum - bp)) + (t[e] - bp);
        s[e] = sum;
    }
}

// (s, lo) += the staged chunk's part of phi's sum for the 32 x rows against the y rows 32 w .. 32 w + 31: a plain fp32 partial over
// the chunk (bilinear family, on the MFMA) or over 4 components at a time (distance family), each added by two_sum.  The x rows lie
// ldx floats apart (the y rows always kKgeLd)
template <int M, bool SWAP>
__device__ __forceinline__ void tile_accumulate(f16v& s, f16v& lo, const float* sx, int xrows, const float* sy, int yrows, int w, int ch, int lane,
                                                int ldx = kKgeLd) {
    if constexpr (!kge_dist(M)) {
        const int l32 = lane & 31, half = lane >> 5;
        f16v t = zero16();
#pragma unroll
        for (int pl = 0; pl < kge_planes(M); ++pl) {
            const float* x = sx + (pl * xrows + l32) * ldx + half;
            const float* y = sy + (pl * yrows + w * kKgeTile + l32) * kKgeLd + half;
            for (int c = 0; c < ch; c += 2) t = SWAP ? mfma(x[c], y[c], t) : mfma(y[c], x[c], t);
        }
        two_sum(s, lo, t);
    } else {
        const float* x = sx + (lane >> 3) * 4 * ldx;
        const float* y = sy + (w * kKgeTile + (lane & 7) * 4) * kKgeLd;
        for (int k0 = 0; k0 < ch; k0 += 4) {                  // (ch is a multiple of 4)
            f16v t = zero16();
#pragma unroll
            for (int k = k0; k < k0 + 4; ++k) {
                float xa[4], yb[4], xi[4], yi[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    xa[u] = x[u * ldx + k];
                    yb[u] = y[u * kKgeLd + k];
                    if constexpr (M == PGLAMD_KGE_ROTATE) {
                        xi[u] = x[(xrows + u) * ldx + k];
                        yi[u] = y[(yrows + u) * kKgeLd + k];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float dre = xa[u] - yb[v];
                        if constexpr (M == PGLAMD_KGE_ROTATE) {
                            const float dim = xi[u] - yi[v];
                            t[u * 4 + v] += sqrtf(fmaf(dim, dim, dre * dre) + 1e-12f);
                        } else {
                            t[u * 4 + v] = fmaf(dre, dre, t[u * 4 + v]);
                        }
                    }
                }
            }
            two_sum(s, lo, t);
        }
    }
}

// the accumulated sum q + lo -> the score; dist: TransE's distance
template <int M> __device__ __forceinline__ float finish_score(float q, float lo, float gamma, float& dist) {
    if constexpr (M == PGLAMD_KGE_TRANSE) { dist = sqrtf(fmaxf(q + lo, 1e-30f)); return gamma - dist; }
    else if constexpr (M == PGLAMD_KGE_ROTATE) { dist = 1.f; return (gamma - q) - lo; }
    else { dist = 1.f; return q + lo; }
}
// the same from the fp64 sum of the positive's own score
template <int M> __device__ __forceinline__ float finish_score(double q, float gamma, float& dist) {
    const float hi = (float)q;
    return finish_score<M>(hi, (float)(q - (double)hi), gamma, dist);
}

template <int M, bool SCORES>
__global__ __launch_bounds__(kBlock) void kge_forward_kernel(KgeArgs a) {
    extern __shared__ __align__(16) float s_kge[];
    constexpr int PL = kge_planes(M);
    constexpr int NG = kge_dist(M) ? 4 : 1, EPG = 16 / NG;         // groups of elements that share a positive
    float* sx = s_kge;                                             // queries [PL][32][ld]
    float* so = sx + PL * kKgeTile * kKgeLd;                       // other ends [PL][32][ld]
    float* sy = so + PL * kKgeTile * kKgeLd;                       // negatives [PL][128][ld]
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int pi = threadIdx.x >> 3, pk = threadIdx.x & 7;         // the positive score: 8 lanes a positive
    for (int64_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const int sb = (int)(unit % a.n_sb);
        const int64_t rest = unit / a.n_sb;
        const int it = (int)(rest % a.n_it), c = (int)(rest / a.n_it);
        const int i0 = it * kKgeTile, j0 = sb * kKgeSuper, jw = j0 + w * kKgeTile;
        const bool mine = jw < a.nneg;
        const int64_t* negc = a.neg + (int64_t)c * a.nneg;
        f16v s = zero16(), lo = zero16();
        double pacc = 0.0;                                 // the positive's own score: 8 lanes' partials, in fp64
        for (int c0 = 0; c0 < a.nc; c0 += kKgeChunk) {
            const int ch = min(kKgeChunk, a.nc - c0);
            stage_query<M>(a, kKgeTile, c, i0, c0, ch, sx, nullptr, nullptr, sb == 0 ? so : nullptr);
            stage_ent<M>(a, sy, kKgeSuper, negc, j0, a.nneg, c0, ch);
            __syncthreads();
            if (mine) tile_accumulate<M, SCORES>(s, lo, sx, kKgeTile, sy, kKgeSuper, w, ch, lane);
            if (sb == 0) {
                for (int k = pk; k < ch; k += 8) {
                    const float dre = sx[pi * kKgeLd + k], ore = so[pi * kKgeLd + k];
                    if constexpr (M == PGLAMD_KGE_TRANSE) pacc += (double)(dre - ore) * (double)(dre - ore);
                    else if constexpr (M == PGLAMD_KGE_DISTMULT) pacc += (double)dre * (double)ore;
                    else {
                        const float dim = sx[(kKgeTile + pi) * kKgeLd + k], oim = so[(kKgeTile + pi) * kKgeLd + k];
                        if constexpr (M == PGLAMD_KGE_COMPLEX) pacc += (double)dre * (double)ore + (double)dim * (double)oim;
                        else pacc += (double)sqrtf(fmaf(dim - oim, dim - oim, (dre - ore) * (dre - ore)) + 1e-12f);
                    }
                }
            }
            __syncthreads();
        }
        if (sb == 0) {
            pacc += __shfl_xor(pacc, 1, kWave);
            pacc += __shfl_xor(pacc, 2, kWave);
            pacc += __shfl_xor(pacc, 4, kWave);
            float dist;
            if (pk == 0 && i0 + pi < a.cs) a.pos[(int64_t)c * a.cs + i0 + pi] = finish_score<M>(pacc, a.gamma, dist);
        }
        if (!mine) continue;
        if constexpr (SCORES) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = i0 + tile_x<M, SCORES>(e, lane), j = jw + tile_y<M, SCORES>(e, lane);
                float dist;
                if (i < a.cs && j < a.nneg) a.scores[((int64_t)c * a.cs + i) * a.nneg + j] = finish_score<M>(s[e], lo[e], a.gamma, dist);
            }
        } else {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                float sv[EPG], m = -INFINITY, Z = 0.f, W = 0.f;
#pragma unroll
                for (int e = 0; e < EPG; ++e) {
                    float dist;
                    sv[e] = finish_score<M>(s[g * EPG + e], lo[g * EPG + e], a.gamma, dist);
                    if (jw + tile_y<M, false>(g * EPG + e, lane) < a.nneg) m = fmaxf(m, a.tau * sv[e]);
                }
#pragma unroll
                for (int e = 0; e < EPG; ++e) {
                    if (jw + tile_y<M, false>(g * EPG + e, lane) < a.nneg) {
                        const float ex = expf(a.tau * sv[e] - m);
                        Z += ex;
                        W = fmaf(ex, softplus(sv[e]), W);
                    }
                }
                if constexpr (kge_dist(M)) {
#pragma unroll
                    for (int mask = 1; mask < 8; mask <<= 1)
                        merge(m, Z, W, __shfl_xor(m, mask, kWave), __shfl_xor(Z, mask, kWave), __shfl_xor(W, mask, kWave));
                } else {
                    merge(m, Z, W, __shfl_xor(m, 32, kWave), __shfl_xor(Z, 32, kWave), __shfl_xor(W, 32, kWave));
                }
                const int i = i0 + tile_x<M, false>(g * EPG, lane);
                const bool writer = kge_dist(M) ? (lane & 7) == 0 : lane < 32;
                if (writer && i < a.cs) {
                    float* o = a.part + (((int64_t)c * a.cs + i) * a.njb + (jw >> 5)) * 3;
                    o[0] = m; o[1] = Z; o[2] = W;
                }
            }
        }
    }
}

// per positive: the blocks' states merged in block order -> (m, Z) and the positive's loss terms; a workgroup's terms summed in fp64
__global__ __launch_bounds__(kBlock) void kge_finish_kernel(const float* __restrict__ part, const float* __restrict__ pos, int64_t P, int njb,
                                                            float* __restrict__ mz, double* __restrict__ block_part) {
    __shared__ double red[kBlock];
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double term = 0.0;
    if (p < P) {
        float m = -INFINITY, Z = 0.f, W = 0.f;
        for (int jb = 0; jb < njb; ++jb) {
            const float* q = part + (p * njb + jb) * 3;
            merge(m, Z, W, q[0], q[1], q[2]);
        }
        mz[2 * p] = m;
        mz[2 * p + 1] = Z;
        term = (double)softplus(-pos[p]) + (double)(W / Z);
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kBlock) void kge_sum_kernel(const double* __restrict__ part, int n, double scale, float* __restrict__ loss) {
    __shared__ double red[kBlock];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(red[0] * scale);
}

// PASS 1: the owner rows x are 32 positives (queries), the swept rows y the chunk's negatives; PASS 2: x are 32 negatives, y the
// chunk's positives.  phi is symmetric in its two rows, and d phi / d owner = coefficient * (swept | owner - swept) in both passes.
template <int M, int PASS>
__global__ __launch_bounds__(kBlock) void kge_backward_kernel(KgeArgs a) {
    extern __shared__ __align__(16) float s_kge[];
    constexpr int PL = kge_planes(M);
    float* sx = s_kge;                                             // owner rows [PL][32][ld]
    float* sy = sx + PL * kKgeTile * kKgeLd;                       // swept rows [PL][128][ld]
    float* sc = sy + PL * kKgeSuper * kKgeLd;                      // coefficients [32][ldc]
    float* se = sc + kKgeTile * kKgeLdc;                           // pass 1: kept ends, relations, other ends [PL][32][ld] each
    float* sr = se + PL * kKgeTile * kKgeLd;
    float* so = sr + PL * kKgeTile * kKgeLd;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int xi = threadIdx.x >> 3, xk = threadIdx.x & 7;         // phase B: 8 lanes an owner row
    const int xcount = PASS == 1 ? a.cs : a.nneg, ycount = PASS == 1 ? a.nneg : a.cs;
    const int nxt = PASS == 1 ? a.n_it : a.njb, nsb = (ycount + kKgeSuper - 1) / kKgeSuper;
    for (int64_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const int x0 = (int)(unit % nxt) * kKgeTile, c = (int)(unit / nxt);
        const int64_t* negc = a.neg + (int64_t)c * a.nneg;
        auto stage = [&](int y0, int c0, int ch, bool full) {
            if constexpr (PASS == 1) {
                stage_query<M>(a, kKgeTile, c, x0, c0, ch, sx, full ? se : nullptr, full ? sr : nullptr, full ? so : nullptr);
                stage_ent<M>(a, sy, kKgeSuper, negc, y0, a.nneg, c0, ch);
            } else {
                stage_ent<M>(a, sx, kKgeTile, negc, x0, a.nneg, c0, ch);
                stage_query<M>(a, kKgeSuper, c, y0, c0, ch, sy, nullptr, nullptr, nullptr);
            }
        };
        for (int sb = 0; sb < nsb; ++sb) {
            const int y0 = sb * kKgeSuper, yw = y0 + w * kKgeTile, yv = min(kKgeSuper, ycount - y0);
            const bool mine = yw < ycount, last = sb == nsb - 1;
            // phase A: the score tiles again, then the coefficients
            f16v s = zero16(), lo = zero16();
            for (int c0 = 0; c0 < a.nc; c0 += kKgeChunk) {
                const int ch = min(kKgeChunk, a.nc - c0);
                stage(y0, c0, ch, false);
                __syncthreads();
                if (mine) tile_accumulate<M, false>(s, lo, sx, kKgeTile, sy, kKgeSuper, w, ch, lane);
                __syncthreads();
            }
            if (mine) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int x = tile_x<M, false>(e, lane), y = tile_y<M, false>(e, lane);
                    float cf = 0.f;
                    if (x0 + x < xcount && yw + y < ycount) {
                        const int64_t p = (int64_t)c * a.cs + (PASS == 1 ? x0 + x : yw + y);
                        float dist;
                        const float sv = finish_score<M>(s[e], lo[e], a.gamma, dist);
                        cf = expf(a.tau * sv - a.mz[2 * p]) / a.mz[2 * p + 1] * sigmoid(sv) * a.inv_2p;
                        if constexpr (M == PGLAMD_KGE_TRANSE) cf = -cf / dist;
                        if constexpr (M == PGLAMD_KGE_ROTATE) cf = -cf;
                    }
                    sc[x * kKgeLdc + w * kKgeTile + y] = cf;
                }
            }
            __syncthreads();
            // phase B: the owner rows' gradient, chunk by chunk
            for (int c0 = 0; c0 < a.nc; c0 += kKgeChunk) {
                const int ch = min(kKgeChunk, a.nc - c0);
                stage(y0, c0, ch, PASS == 1 && last);
                __syncthreads();
                if (x0 + xi < xcount) {
                    const float* cfr = sc + xi * kKgeLdc;
                    for (int k = xk; k < ch; k += 8) {
                        const float a0 = sx[xi * kKgeLd + k], a1 = PL == 2 ? sx[(kKgeTile + xi) * kKgeLd + k] : 0.f;
                        float acc0 = 0.f, acc1 = 0.f;
                        for (int y = 0; y < yv; ++y) {
                            const float cf = cfr[y], b0 = sy[y * kKgeLd + k];
                            if constexpr (M == PGLAMD_KGE_TRANSE) acc0 = fmaf(cf, a0 - b0, acc0);
                            else if constexpr (M == PGLAMD_KGE_DISTMULT) acc0 = fmaf(cf, b0, acc0);
                            else {
                                const float b1 = sy[(kKgeSuper + y) * kKgeLd + k];
                                if constexpr (M == PGLAMD_KGE_COMPLEX) { acc0 = fmaf(cf, b0, acc0); acc1 = fmaf(cf, b1, acc1); }
                                else {
                                    const float dre = a0 - b0, dim = a1 - b1;
                                    const float tq = cf * rsqrtf(fmaf(dim, dim, dre * dre) + 1e-12f);
                                    acc0 = fmaf(tq, dre, acc0);
                                    acc1 = fmaf(tq, dim, acc1);
                                }
                            }
                        }
                        const int64_t row = PASS == 1 ? (int64_t)c * a.cs + x0 + xi : (int64_t)c * a.nneg + x0 + xi;
                        float* dst = (PASS == 1 ? a.g_kept : a.g_neg) + row * a.d + c0 + k;
                        if (sb > 0) { acc0 += dst[0]; if (PL == 2) acc1 += dst[a.nc]; }
                        if (PASS == 1 && last) {
                            // the positive score's gradient, then the chain rule to the gathered rows
                            const float ps = a.pos[row], cp = -sigmoid(-ps) * a.inv_2p;
                            const float e0 = se[xi * kKgeLd + k], r0 = sr[xi * kKgeLd + k], o0 = so[xi * kKgeLd + k];
                            float* go = a.g_other + row * a.d + c0 + k;
                            if constexpr (M == PGLAMD_KGE_TRANSE) {
                                const float f = cp * ((a0 - o0) / fmaxf(a.gamma - ps, 1e-15f));
                                const float da = acc0 - f;
                                go[0] = f;
                                dst[0] = da;
                                a.g_rel[row * a.d + c0 + k] = a.neg_head ? -da : da;
                            } else if constexpr (M == PGLAMD_KGE_DISTMULT) {
                                const float da = fmaf(cp, o0, acc0);
                                go[0] = cp * a0;
                                dst[0] = da * r0;
                                a.g_rel[row * a.d + c0 + k] = da * e0;
                            } else {
                                const int at = (kKgeTile + xi) * kKgeLd + k;
                                const float e1 = se[at], r1 = sr[at], o1 = so[at];
                                float da0, da1;
                                if constexpr (M == PGLAMD_KGE_COMPLEX) {
                                    da0 = fmaf(cp, o0, acc0); da1 = fmaf(cp, o1, acc1);
                                    go[0] = cp * a0; go[a.nc] = cp * a1;
                                } else {
                                    const float dre = a0 - o0, dim = a1 - o1;
                                    const float tq = cp * rsqrtf(fmaf(dim, dim, dre * dre) + 1e-12f);
                                    da0 = acc0 - tq * dre; da1 = acc1 - tq * dim;
                                    go[0] = tq * dre; go[a.nc] = tq * dim;
                                }
                                if (a.neg_head) { dst[0] = da0 * r0 - da1 * r1; dst[a.nc] = da0 * r1 + da1 * r0; }
                                else { dst[0] = da0 * r0 + da1 * r1; dst[a.nc] = da1 * r0 - da0 * r1; }
                                if constexpr (M == PGLAMD_KGE_COMPLEX) {
                                    float* gr = a.g_rel + row * a.d + c0 + k;
                                    gr[0] = da0 * e0 + da1 * e1;
                                    gr[a.nc] = a.neg_head ? da0 * e1 - da1 * e0 : da1 * e0 - da0 * e1;
                                } else {
                                    const float gth = a.neg_head ? da0 * a1 - da1 * a0 : da1 * a0 - da0 * a1;
                                    a.g_rel[row * a.nc + c0 + k] = gth / a.scale;
                                }
                            }
                        } else {
                            dst[0] = acc0;
                            if (PL == 2) dst[a.nc] = acc1;
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
}

// RANKS (pglamd_kge_rank).  Per query q -- the kept end and the relation of a test triple -- and the entity range [lo, hi):
// greater[q] / equal[q] = how many candidates j != the true entity, not listed in the query's filter row, score above / exactly
// ref_q = phi(a_q, ent[true entity]).  Nothing of size [Q, Ne] exists: a unit sweeps a slice of the table and keeps two integers.
//   unit      (a tile of 32 queries) x (one of S slices of the range, a whole number of superblocks each).  The candidates are
//             CONSECUTIVE rows of ent: staged straight from the table, no id gather.  The 32 query rows are formed ONCE per unit into
//             rows nc + 1 floats apart when they fit beside the candidate stage (kRankResidentLds); beyond that they are restaged per
//             superblock as the forward does.
//   ref       the unit first runs its tile against its own 32 gathered true rows through the same tile_accumulate / finish_score
//             code and keeps the diagonal.  A score's bits follow from the two rows alone (one MFMA chain, or one fmaf chain, per
//             32-component chunk, the chunks added in order by two_sum): a bitwise copy of the true row ties with it exactly.
//   counts    in registers across the slice: bilinear family one query a lane (x 2 half-waves x 4 waves), distance family 4 queries
//             a lane (x 8 lanes x 4 waves); summed through LDS at the end of the unit.
//   filter    per query a cursor into its sorted filter row (one binary search at the start of the slice) and the id under it in a
//             register: a 32-candidate tile costs one compare unless an entry falls inside it; only then the tile's mask is built.
//   result    S = 1: the unit writes greater / equal.  S > 1: int32 counts to the workspace [Q, S, 2], summed in slice order by a
//             second launch.  Integer sums: every S gives the same result.  No atomics, no host read: capturable.
constexpr int kRankMaxSlices = 512;
constexpr int64_t kRankUnitsAim = 1024;               // units a launch aims at: four per CU (profiles/kge_rank/README.md)
constexpr int64_t kRankMinSuper = 2;                  // superblocks per slice at least: the query tile and ref are formed per unit
constexpr size_t kRankResidentLds = 80 * 1024;        // two workgroups a CU
constexpr int64_t kRankNone = INT64_MAX;

struct KgeRankArgs {
    KgeArgs k;                                        // C = 1, cs = Q: stage_query's view of the queries
    const int64_t* other;                             // the end being ranked: t, or h when neg_head
    const int64_t* indptr; const int32_t* col; const int64_t* filter_rows;
    int64_t num_rows, num_cols, lo, hi, slice_len, units;
    int64_t* greater; int64_t* equal; int32_t* ws;
    int S, ldq;                                       // ldq: floats between resident query rows; 0: restaged per superblock
};

// the 128 consecutive entity rows from `first`, components c0 .. c0 + ch - 1 -> dst [planes][128][kKgeLd]; zeros from `end` on
template <int M>
__device__ __forceinline__ void stage_range(const KgeArgs& a, float* dst, int64_t first, int64_t end, int c0, int ch) {
    constexpr int PL = kge_planes(M);
    const int q4 = ch >> 2;
    for (int idx = threadIdx.x; idx < kKgeSuper * q4; idx += kBlock) {
        const int r = idx / q4, cc = (idx - r * q4) << 2;
        const int64_t id = first + r < end ? first + r : -1;
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) put4(dst + (pl * kKgeSuper + r) * kKgeLd + cc, row4(a.ent, id, a.num_ent, a.d, pl * a.nc + c0 + cc));
    }
}

// one walk over the component chunks: the query tile q0 against its own true rows (REF; wave 0's tile) or against the superblock at j0
template <int M, bool REF>
__device__ __forceinline__ void rank_pass(const KgeRankArgs& a, float* sq, float* sy, int q0, int64_t j0, int64_t shi, bool mine, int w, int lane,
                                          f16v& s, f16v& lo) {
    const KgeArgs& k = a.k;
    const int ldq = a.ldq > 0 ? a.ldq : kKgeLd;
    for (int c0 = 0; c0 < k.nc; c0 += kKgeChunk) {
        const int ch = min(kKgeChunk, k.nc - c0);
        if (a.ldq == 0) stage_query<M>(k, kKgeTile, 0, q0, c0, ch, sq, nullptr, nullptr, nullptr);
        if constexpr (REF) stage_ent<M>(k, sy, kKgeTile, a.other, q0, k.cs, c0, ch);
        else stage_range<M>(k, sy, j0, shi, c0, ch);
        __syncthreads();
        if (mine) tile_accumulate<M, false>(s, lo, a.ldq > 0 ? sq + c0 : sq, kKgeTile, sy, REF ? kKgeTile : kKgeSuper, REF ? 0 : w, ch, lane, ldq);
        __syncthreads();
    }
}

template <int M>
__global__ __launch_bounds__(kBlock) void kge_rank_kernel(KgeRankArgs a) {
    extern __shared__ __align__(16) float s_kge[];
    constexpr int PL = kge_planes(M);
    constexpr int NG = kge_dist(M) ? 4 : 1, EPG = 16 / NG;         // groups of elements that share a query
    const KgeArgs& k = a.k;
    float* sq = s_kge;                                             // queries [PL][32][ldq | kKgeLd]
    float* sy = sq + PL * kKgeTile * (a.ldq > 0 ? a.ldq : kKgeLd); // candidates [PL][128][ld]
    float* s_ref = sy + PL * kKgeSuper * kKgeLd;                   // [32]
    int* s_cnt = reinterpret_cast<int*>(s_ref + kKgeTile);         // [waves][32][2]
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    for (int64_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const int sl = (int)(unit % a.S), q0 = (int)(unit / a.S) * kKgeTile;
        const int64_t slo = a.lo + sl * a.slice_len, shi = min(a.hi, slo + a.slice_len);   // (an empty slice: slo >= shi)
        if (a.ldq > 0) {
            for (int c0 = 0; c0 < k.nc; c0 += kKgeChunk)
                stage_query<M>(k, kKgeTile, 0, q0, c0, min(kKgeChunk, k.nc - c0), sq + c0, nullptr, nullptr, nullptr, a.ldq);
        }
        {
            f16v s = zero16(), lo = zero16();
            rank_pass<M, true>(a, sq, sy, q0, 0, 0, w == 0, w, lane, s, lo);
            if (w == 0) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int x = tile_x<M, false>(e, lane);
                    float dist;
                    if (x == tile_y<M, false>(e, lane)) s_ref[x] = finish_score<M>(s[e], lo[e], k.gamma, dist);
                }
            }
            __syncthreads();
        }
        // per query group of the lane: the true entity, ref, the cursor into the filter row and the id under it
        bool qok[NG];
        int64_t oth[NG], cur[NG], end[NG], nxt[NG];
        float rf[NG];
        int gt[NG], eq[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int x = tile_x<M, false>(g * EPG, lane);
            qok[g] = q0 + x < k.cs;
            oth[g] = qok[g] ? a.other[q0 + x] : -1;
            rf[g] = s_ref[x];
            gt[g] = eq[g] = 0;
            cur[g] = end[g] = 0;
            nxt[g] = kRankNone;
            if (a.indptr && qok[g]) {
                const int64_t fr = a.filter_rows[q0 + x];
                if (fr >= 0 && fr < a.num_rows) {
                    cur[g] = max((int64_t)0, a.indptr[fr]);
                    end[g] = min(a.num_cols, a.indptr[fr + 1]);
                    int64_t hi2 = end[g];
                    while (cur[g] < hi2) {
                        const int64_t mid = (cur[g] + hi2) >> 1;
                        if (a.col[mid] < slo) cur[g] = mid + 1; else hi2 = mid;
                    }
                    if (cur[g] < end[g]) nxt[g] = a.col[cur[g]];
                }
            }
        }
        for (int64_t j0 = slo; j0 < shi; j0 += kKgeSuper) {
            const int64_t jw = j0 + w * kKgeTile;
            const bool mine = jw < shi;
            f16v s = zero16(), lo = zero16();
            rank_pass<M, false>(a, sq, sy, q0, j0, shi, mine, w, lane, s, lo);
            if (!mine) continue;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                uint32_t mask = 0;
                while (nxt[g] < jw + kKgeTile) {                   // (rarely entered: most windows are empty)
                    if (nxt[g] >= jw) mask |= 1u << (int)(nxt[g] - jw);
                    ++cur[g];
                    nxt[g] = cur[g] < end[g] ? (int64_t)a.col[cur[g]] : kRankNone;
                }
#pragma unroll
                for (int e = g * EPG; e < (g + 1) * EPG; ++e) {
                    const int y = tile_y<M, false>(e, lane);
                    const int64_t j = jw + y;
                    float dist;
                    const float sv = finish_score<M>(s[e], lo[e], k.gamma, dist);
                    const bool ok = qok[g] && j < shi && j != oth[g] && !((mask >> y) & 1u);
                    gt[g] += ok && sv > rf[g];
                    eq[g] += ok && sv == rf[g];
                }
            }
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            int ng = gt[g], ne = eq[g];
            if constexpr (kge_dist(M)) {
#pragma unroll
                for (int m = 1; m < 8; m <<= 1) { ng += __shfl_xor(ng, m, kWave); ne += __shfl_xor(ne, m, kWave); }
            } else {
                ng += __shfl_xor(ng, 32, kWave); ne += __shfl_xor(ne, 32, kWave);
            }
            const bool writer = kge_dist(M) ? (lane & 7) == 0 : lane < 32;
            if (writer) {
                int* o = s_cnt + (w * kKgeTile + tile_x<M, false>(g * EPG, lane)) * 2;
                o[0] = ng; o[1] = ne;
            }
        }
        __syncthreads();
        if (threadIdx.x < kKgeTile && q0 + (int)threadIdx.x < k.cs) {
            int ng = 0, ne = 0;
#pragma unroll
            for (int ww = 0; ww < kWavesPerBlock; ++ww) {
                ng += s_cnt[(ww * kKgeTile + threadIdx.x) * 2];
                ne += s_cnt[(ww * kKgeTile + threadIdx.x) * 2 + 1];
            }
            const int64_t q = q0 + threadIdx.x;
            if (a.S == 1) { a.greater[q] = ng; a.equal[q] = ne; }
            else { a.ws[(q * a.S + sl) * 2] = ng; a.ws[(q * a.S + sl) * 2 + 1] = ne; }
        }
        __syncthreads();
    }
}

// per query: the slices' counts summed in slice order
__global__ __launch_bounds__(kBlock) void kge_rank_sum_kernel(const int32_t* __restrict__ ws, int64_t Q, int S, int64_t* __restrict__ greater,
                                                              int64_t* __restrict__ equal) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= Q) return;
    int64_t ng = 0, ne = 0;
    for (int s = 0; s < S; ++s) { ng += ws[(q * S + s) * 2]; ne += ws[(q * S + s) * 2 + 1]; }
    greater[q] = ng;
    equal[q] = ne;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the dynamic LDS of a rank unit whose query rows lie ldq floats apart
size_t rank_lds(int model, int ldq) {
    return ((size_t)kge_planes(model) * (kKgeTile * ldq + kKgeSuper * kKgeLd) + kKgeTile) * sizeof(float) + kWavesPerBlock * kKgeTile * 2 * sizeof(int);
}

size_t forward_lds(int model) { return (size_t)kge_planes(model) * (2 * kKgeTile + kKgeSuper) * kKgeLd * sizeof(float); }
size_t backward_lds(int model) {
    return ((size_t)kge_planes(model) * (4 * kKgeTile + kKgeSuper) * kKgeLd + kKgeTile * kKgeLdc) * sizeof(float);
}
size_t part_bytes(int64_t P, int64_t nneg) { return align_up((size_t)P * ceil_div(nneg, kKgeTile) * 3 * sizeof(float), 256); }

int32_t kge_common(const char* what, KgeArgs& a, const float* ent, int64_t num_ent, const float* rel, int64_t num_rel, int64_t d, const int64_t* h,
                   const int64_t* r, const int64_t* t, const int64_t* neg, int64_t C, int64_t cs, int64_t nneg, int32_t model, int32_t neg_head,
                   float gamma) {
    if (model < PGLAMD_KGE_TRANSE || model > PGLAMD_KGE_ROTATE) return fail(PGLAMD_E_ARG, "%s: unknown model %d", what, (int)model);
    if (!ent || !rel || !h || !r || !t || !neg || num_ent < 1 || num_rel < 1 || C < 1 || cs < 1 || nneg < 1) return fail(PGLAMD_E_ARG, "%s: bad argument", what);
    if (d < 8 || d % 8 || d > kKgeMaxD) return fail(PGLAMD_E_SHAPE, "%s: d = %lld must be a multiple of 8 from 8 to %d", what, (long long)d, kKgeMaxD);
    if (!aligned16(ent) || !aligned16(rel)) return fail(PGLAMD_E_ARG, "%s: ent and rel must be 16-byte aligned", what);
    if (C * cs >= INT32_MAX / 4 || C * nneg >= INT32_MAX / 4 || num_ent >= INT32_MAX || num_rel >= INT32_MAX)
        return fail(PGLAMD_E_RANGE, "%s: sizes beyond int32 engine range", what);
    a.ent = ent; a.rel = rel; a.h = h; a.r = r; a.t = t; a.neg = neg;
    a.num_ent = num_ent; a.num_rel = num_rel;
    a.C = (int)C; a.cs = (int)cs; a.nneg = (int)nneg; a.d = (int)d;
    a.nc = kge_planes(model) == 2 ? (int)d / 2 : (int)d;
    a.n_it = (int)ceil_div(cs, kKgeTile); a.n_sb = (int)ceil_div(nneg, kKgeSuper); a.njb = (int)ceil_div(nneg, kKgeTile);
    a.neg_head = neg_head != 0; a.gamma = gamma;
    a.scale = (float)(((double)gamma + 2.0) / (double)(d / 2) / 3.14159265358979323846);
    a.inv_2p = (float)(0.5 / (double)(C * cs));
    return PGLAMD_OK;
}

template <typename K> int32_t launch(K kernel, const KgeArgs& a, size_t lds, hipStream_t st) {
    static bool attr_set = false;                             // (per instantiation; idempotent, so a race only repeats it)
    if (!attr_set) {
        PGLAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set = true;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<int64_t>(a.units, kKgeGridCap)), dim3(kBlock), lds, st, a);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

template <bool SCORES> int32_t launch_forward(int model, const KgeArgs& a, hipStream_t st) {
    const size_t lds = forward_lds(model);
    switch (model) {
        case PGLAMD_KGE_TRANSE: return launch(&kge_forward_kernel<PGLAMD_KGE_TRANSE, SCORES>, a, lds, st);
        case PGLAMD_KGE_DISTMULT: return launch(&kge_forward_kernel<PGLAMD_KGE_DISTMULT, SCORES>, a, lds, st);
        case PGLAMD_KGE_COMPLEX: return launch(&kge_forward_kernel<PGLAMD_KGE_COMPLEX, SCORES>, a, lds, st);
        default: return launch(&kge_forward_kernel<PGLAMD_KGE_ROTATE, SCORES>, a, lds, st);
    }
}

template <int PASS> int32_t launch_backward(int model, const KgeArgs& a, hipStream_t st) {
    const size_t lds = backward_lds(model);
    switch (model) {
        case PGLAMD_KGE_TRANSE: return launch(&kge_backward_kernel<PGLAMD_KGE_TRANSE, PASS>, a, lds, st);
        case PGLAMD_KGE_DISTMULT: return launch(&kge_backward_kernel<PGLAMD_KGE_DISTMULT, PASS>, a, lds, st);
        case PGLAMD_KGE_COMPLEX: return launch(&kge_backward_kernel<PGLAMD_KGE_COMPLEX, PASS>, a, lds, st);
        default: return launch(&kge_backward_kernel<PGLAMD_KGE_ROTATE, PASS>, a, lds, st);
    }
}

}  // namespace
}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_kge_workspace_bytes(int64_t num_pos, int64_t num_neg) {
    if (num_pos <= 0 || num_neg <= 0) return 256;
    return part_bytes(num_pos, num_neg) + align_up((size_t)ceil_div(num_pos, kBlock) * sizeof(double), 256);
}

extern "C" int32_t pglamd_kge_scores(const float* ent, int64_t num_ent, const float* rel, int64_t num_rel, int64_t d, const int64_t* h,
                                     const int64_t* r, const int64_t* t, const int64_t* neg, int64_t num_chunks, int64_t chunk_size,
                                     int64_t num_neg, int32_t model, int32_t neg_head, float gamma, float* pos, float* scores, void* stream) {
    KgeArgs a{};
    PGLAMD_TRY(kge_common("kge_scores", a, ent, num_ent, rel, num_rel, d, h, r, t, neg, num_chunks, chunk_size, num_neg, model, neg_head, gamma));
    if (!pos || !scores) return fail(PGLAMD_E_ARG, "kge_scores: NULL output");
    a.pos = pos; a.scores = scores;
    a.units = (int64_t)a.C * a.n_it * a.n_sb;
    return launch_forward<true>(model, a, static_cast<hipStream_t>(stream));
}

extern "C" int32_t pglamd_kge_loss(const float* ent, int64_t num_ent, const float* rel, int64_t num_rel, int64_t d, const int64_t* h,
                                   const int64_t* r, const int64_t* t, const int64_t* neg, int64_t num_chunks, int64_t chunk_size,
                                   int64_t num_neg, int32_t model, int32_t neg_head, float gamma, float adv_temp, float* pos, float* mz,
                                   float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    KgeArgs a{};
    PGLAMD_TRY(kge_common("kge_loss", a, ent, num_ent, rel, num_rel, d, h, r, t, neg, num_chunks, chunk_size, num_neg, model, neg_head, gamma));
    if (!pos || !mz || !loss || !(adv_temp >= 0.f)) return fail(PGLAMD_E_ARG, "kge_loss: NULL output or a negative temperature");
    const int64_t P = num_chunks * chunk_size;
    if (!workspace || !aligned16(workspace) || workspace_bytes < pglamd_kge_workspace_bytes(P, num_neg))
        return fail(PGLAMD_E_WORKSPACE, "kge_loss: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.pos = pos; a.tau = adv_temp;
    a.part = static_cast<float*>(workspace);
    double* block_part = reinterpret_cast<double*>(static_cast<char*>(workspace) + part_bytes(P, num_neg));
    a.units = (int64_t)a.C * a.n_it * a.n_sb;
    PGLAMD_TRY(launch_forward<false>(model, a, st));
    const int nb = (int)ceil_div(P, kBlock);
    hipLaunchKernelGGL(kge_finish_kernel, dim3(nb), dim3(kBlock), 0, st, a.part, pos, P, a.njb, mz, block_part);
    PGLAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(kge_sum_kernel, dim3(1), dim3(kBlock), 0, st, block_part, nb, 0.5 / (double)P, loss);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_kge_loss_backward(const float* ent, int64_t num_ent, const float* rel, int64_t num_rel, int64_t d, const int64_t* h,
                                            const int64_t* r, const int64_t* t, const int64_t* neg, int64_t num_chunks, int64_t chunk_size,
                                            int64_t num_neg, int32_t model, int32_t neg_head, float gamma, float adv_temp, const float* pos,
                                            const float* mz, float* g_kept, float* g_other, float* g_rel, float* g_neg, void* stream) {
    KgeArgs a{};
    PGLAMD_TRY(kge_common("kge_loss_backward", a, ent, num_ent, rel, num_rel, d, h, r, t, neg, num_chunks, chunk_size, num_neg, model, neg_head, gamma));
    if (!pos || !mz || !g_kept || !g_other || !g_rel || !g_neg) return fail(PGLAMD_E_ARG, "kge_loss_backward: NULL operand");
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.pos = const_cast<float*>(pos); a.mz = mz; a.tau = adv_temp;
    a.g_kept = g_kept; a.g_other = g_other; a.g_rel = g_rel; a.g_neg = g_neg;
    a.units = (int64_t)a.C * a.n_it;
    PGLAMD_TRY(launch_backward<1>(model, a, st));
    a.units = (int64_t)a.C * a.njb;
    return launch_backward<2>(model, a, st);
}

extern "C" int64_t pglamd_kge_rank_slices(int64_t num_queries, int64_t num_candidates) {
    if (num_queries < 1 || num_candidates < 1) return 1;
    const int64_t by_units = ceil_div(kRankUnitsAim, ceil_div(num_queries, kKgeTile));
    const int64_t by_length = std::max<int64_t>(1, ceil_div(num_candidates, kKgeSuper) / kRankMinSuper);
    return std::max<int64_t>(1, std::min<int64_t>({by_units, by_length, (int64_t)kRankMaxSlices}));
}

extern "C" size_t pglamd_kge_rank_workspace_bytes(int64_t num_queries, int64_t slices) {
    if (num_queries < 1 || slices <= 1) return 0;
    return align_up((size_t)num_queries * slices * 2 * sizeof(int32_t), 256);
}

extern "C" int32_t pglamd_kge_rank(const float* ent, int64_t num_ent, const float* rel, int64_t num_rel, int64_t d, const int64_t* h,
                                   const int64_t* r, const int64_t* t, int64_t num_queries, int32_t model, int32_t neg_head, float gamma,
                                   const int64_t* indptr, const int32_t* col, int64_t num_rows, int64_t num_cols, const int64_t* filter_rows,
                                   int64_t lo, int64_t hi, int64_t slices, int64_t* greater, int64_t* equal, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    KgeRankArgs a{};
    // (no negatives: the candidates are a range of the table; kge_common's neg is never read)
    PGLAMD_TRY(kge_common("kge_rank", a.k, ent, num_ent, rel, num_rel, d, h, r, t, h, 1, num_queries, 1, model, neg_head, gamma));
    if (!greater || !equal) return fail(PGLAMD_E_ARG, "kge_rank: NULL output");
    if (lo < 0 || hi > num_ent || hi - lo < 1)
        return fail(PGLAMD_E_ARG, "kge_rank: [lo, hi) = [%lld, %lld) is not a range of the %lld entities", (long long)lo, (long long)hi, (long long)num_ent);
    const bool filt = indptr || col || filter_rows;
    if (filt && (!indptr || !col || !filter_rows || num_rows < 0 || num_cols < 0))
        return fail(PGLAMD_E_ARG, "kge_rank: the filter needs indptr, col and filter_rows together");
    const int64_t S = slices > 0 ? slices : pglamd_kge_rank_slices(num_queries, hi - lo);
    if (S > kRankMaxSlices) return fail(PGLAMD_E_ARG, "kge_rank: at most %d slices", kRankMaxSlices);
    if (S > 1 && (!workspace || !aligned16(workspace) || workspace_bytes < pglamd_kge_rank_workspace_bytes(num_queries, S)))
        return fail(PGLAMD_E_WORKSPACE, "kge_rank: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.other = neg_head ? h : t;
    a.indptr = filt ? indptr : nullptr; a.col = col; a.filter_rows = filter_rows;
    a.num_rows = num_rows; a.num_cols = num_cols; a.lo = lo; a.hi = hi;
    a.slice_len = ceil_div(ceil_div(hi - lo, S), kKgeSuper) * kKgeSuper;
    a.greater = greater; a.equal = equal; a.ws = static_cast<int32_t*>(workspace);
    a.S = (int)S;
    a.units = ceil_div(num_queries, kKgeTile) * S;
    a.ldq = rank_lds(model, a.k.nc + 1) <= kRankResidentLds ? a.k.nc + 1 : 0;     // (nc + 1 is odd: no bank conflicts along the rows)
    const size_t lds = rank_lds(model, a.ldq > 0 ? a.ldq : kKgeLd);
    auto go = [&](auto kernel) -> int32_t {
        static bool attr_set = false;                         // (per instantiation; idempotent, so a race only repeats it)
        if (!attr_set) {
            PGLAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRankResidentLds));
            attr_set = true;
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<int64_t>(a.units, kKgeGridCap)), dim3(kBlock), lds, st, a);
        PGLAMD_LAUNCH_CHECK();
        return PGLAMD_OK;
    };
    switch (model) {
        case PGLAMD_KGE_TRANSE: PGLAMD_TRY(go(&kge_rank_kernel<PGLAMD_KGE_TRANSE>)); break;
        case PGLAMD_KGE_DISTMULT: PGLAMD_TRY(go(&kge_rank_kernel<PGLAMD_KGE_DISTMULT>)); break;
        case PGLAMD_KGE_COMPLEX: PGLAMD_TRY(go(&kge_rank_kernel<PGLAMD_KGE_COMPLEX>)); break;
        default: PGLAMD_TRY(go(&kge_rank_kernel<PGLAMD_KGE_ROTATE>)); break;
    }
    if (S > 1) {
        hipLaunchKernelGGL(kge_rank_sum_kernel, dim3((unsigned)ceil_div(num_queries, kBlock)), dim3(kBlock), 0, st, a.ws, num_queries, a.S, greater, equal);
        PGLAMD_LAUNCH_CHECK();
    }
    return PGLAMD_OK;
}
