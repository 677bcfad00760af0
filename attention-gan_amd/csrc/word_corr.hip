// Word-level discriminator score (ControlGAN, Li et al., NeurIPS 2019, section 3.2; include/agan.h states the formulas): B chosen
// (image b, caption (b + shift) mod B) pairs, per pair func_attention of the caption's L words over the image's S regions, the cosine
// r_l of every word with its context, a word self-attention weight g_l and the pooled probability p_b = sum_l g_l sigmoid(gamma2 r_l).
//
// One 320-thread workgroup per pair, ONE launch per direction, one form for the whole domain (D, S <= 320, T <= 32).  Three matrices
// live in LDS with a common row stride LDW (T rounded up to the MFMA's k step of 4, plus 4 where that would be a multiple of 8 words
// and put the 16 rows of an operand read on 8 banks):  w[D][LDW] the caption's words (0 beyond L), a[S][LDW] scores -> attention,
// c[D][LDW] the contexts.  At the limits that is 3 * 320 * 36 floats = 135 KB of the 160 KB.  The image's [D, S] slab (400 KB at
// the limits) never fits: it is the MFMA operand that streams from global memory, read as it lies -- for a region-indexed result
// a lane group reads 16 consecutive regions of one channel, for a channel-indexed one 4 consecutive regions of 16 channels, four
// such loads covering 64 consecutive bytes of every row before the MFMAs that consume them.  No transposed or padded copy, so no
// second launch and no workspace.
//
// Both contractions (scores over D, contexts over S) and their three backward counterparts run on v_mfma_f32_16x16x4_f32: exact fp32
// products, fp32 accumulation, k ascending inside a tile, tiles independent -- every run gives the same bits.  The 16-wide j axis
// holds the words: one column tile for T <= 16, two above (the only template parameter; both sides of T = 16 | 17 are test cases).
// Everything indexed by region (the two softmaxes and their backward) is owned by thread r = region, as in damsm.hip.
//
// The backward recomputes scores, attention and contexts of its pair from the regions, takes the per-word statistics (<ctx, w>, |w|,
// |ctx|, r, g) from the forward's `save` [B][5][T], and writes dregions[b] -- image b is in exactly one pair, so the slab has one
// owner: no atomics, no slab sum.  The words take no gradient (the text encoder is frozen in the GAN step).  The buffer that held
// the words is re-used for d(attention) and then d(scores); the last contraction reads its word operand from global memory (L2).
#include "agan_common.h"
#include "dispatch.h"
#include "mfma_tile.h"

using namespace agan;

namespace {

constexpr int kNT = 320;           // threads per pair workgroup (5 waves): >= S and >= D
constexpr int kNW = kNT / 64;
constexpr int kMaxB = 128;
constexpr int kMaxT = 32;
constexpr int kSaveRows = 5;       // save[b][k][T]: k = 0 <ctx_l, w_l>, 1 |w_l|, 2 |ctx_l|, 3 r_l, 4 g_l

// the shape of a pair as the kernels use it
struct PairDims {
    int D, S, T, L;      // channels, regions, padded caption length, words of this caption (0 <= L <= T)
    int RD, RS;          // D and S rounded up to whole 16-row tiles
    int TP, LDW;         // T rounded up to a multiple of 4 (the k steps of the last contraction); LDS row stride >= TP
};

struct Small {
    float num[kMaxT], n1[kMaxT], n2[kMaxT], r[kMaxT], g[kMaxT];
    float colmax[kMaxT], colsum[kMaxT];
    float ca[kMaxT], cb[kMaxT];          // backward: d ctx = ca * w + cb * ctx
    float dotw[kNW][kMaxT];
    float wsum[kNT];                     // forward: sum of the caption's words per channel
};

__host__ __device__ inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
__host__ __device__ inline int row_stride(int T) {
    const int tp = round_up(T, 4);
    return (tp % 8 == 0) ? tp + 4 : tp;
}

// the 16-row tiles of a wave: tile wave, wave + 5, ...; how many of `ntiles` that is (at most 4: 20 tiles of 16 rows = 320)
__device__ __forceinline__ int tiles_of_wave(int ntiles, int wave) { return ntiles > wave ? (ntiles - wave + kNW - 1) / kNW : 0; }

// out[s][l] = sum_d n[d][s] * bm[d][l]  for s < RS, l < LDW (rows s >= S come out 0).  n: the image's [D][S] slab in global memory;
// bm: [>= round_up(D, 4)][LDW] in LDS, finite everywhere (rows >= D are multiplied by 0).
template <int NLT>
__device__ __forceinline__ void region_rows(const float* __restrict__ n, const float* bm, float* out, const PairDims& g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mi = lane & 15, kq = lane >> 4;
    const int nq = tiles_of_wave(g.RS >> 4, wave);
    if (nq == 0) return;                                         // (wave-uniform; no barrier inside)
    f32x4 acc[4][NLT];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < NLT; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    int col[NLT];
#pragma unroll
    for (int t = 0; t < NLT; ++t) col[t] = min(16 * t + mi, g.LDW - 1);      // (columns past the row: a clamped read, never stored)
    for (int d0 = 0; d0 < g.D; d0 += 4) {
        const int d = d0 + kq;                                   // k = d
        const bool dl = d < g.D;
        float b[NLT], a[4];
#pragma unroll
        for (int t = 0; t < NLT; ++t) b[t] = bm[d * g.LDW + col[t]];         // B[k = d][j = l]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int s = (wave + kNW * q) * 16 + mi;            // A[i = s][k = d]: 16 consecutive regions of channel d
            a[q] = (q < nq && dl && s < g.S) ? n[(size_t)d * g.S + s] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < nq) {
#pragma unroll
                for (int t = 0; t < NLT; ++t) acc[q][t] = mfma4(a[q], b[t], acc[q][t]);
            }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < nq) {
#pragma unroll
            for (int t = 0; t < NLT; ++t) {
                const int c = 16 * t + mi;
                if (c < g.LDW) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) out[((wave + kNW * q) * 16 + 4 * kq + r) * g.LDW + c] = acc[q][t][r];   // D[i = 4 kq + r][j = mi]
                }
            }
        }
}

// out[d][l] = sum_s n[d][s] * bm[s][l]  for d < RD, l < LDW (rows d >= D come out 0).  bm: [RS][LDW] in LDS, finite everywhere.
// A k block is 16 regions: lane (mi, kq) loads regions s0 + 4 kq + 0..3 of channel mi of its tile, MFMA t multiplies the t-th.
template <int NLT>
__device__ __forceinline__ void channel_rows(const float* __restrict__ n, const float* bm, float* out, const PairDims& g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mi = lane & 15, kq = lane >> 4;
    const int nq = tiles_of_wave(g.RD >> 4, wave);
    if (nq == 0) return;
    f32x4 acc[4][NLT];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < NLT; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    int col[NLT];
#pragma unroll
    for (int t = 0; t < NLT; ++t) col[t] = min(16 * t + mi, g.LDW - 1);
    for (int s0 = 0; s0 < g.RS; s0 += 16) {
        float a[4][4], b[4][NLT];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = s0 + 4 * kq + k;                       // < RS
#pragma unroll
            for (int t = 0; t < NLT; ++t) b[k][t] = bm[s * g.LDW + col[t]];  // B[k = s][j = l]
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = (wave + kNW * q) * 16 + mi;        // A[i = d][k = s]
                a[q][k] = (q < nq && d < g.D && s < g.S) ? n[(size_t)d * g.S + s] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nq) {
#pragma unroll
                    for (int t = 0; t < NLT; ++t) acc[q][t] = mfma4(a[q][k], b[k][t], acc[q][t]);
                }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < nq) {
#pragma unroll
            for (int t = 0; t < NLT; ++t) {
                const int c = 16 * t + mi;
                if (c < g.LDW) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) out[((wave + kNW * q) * 16 + 4 * kq + r) * g.LDW + c] = acc[q][t][r];
                }
            }
        }
}

// func_attention of one pair.  On return (after the trailing barrier): wbuf = w[RD][LDW] (0 for d >= D or l >= L), abuf = alpha[RS][LDW]
// (0 for s >= S or l >= L), cbuf = ctx[RD][LDW]; a1[] = thread r's row of sbar (0 for l >= L or r >= S); sm.colmax / colsum.
template <int NLT>
__device__ __forceinline__ void pair_attention(const float* __restrict__ n, const float* __restrict__ wc, const PairDims& g, float gamma1,
                                               float* wbuf, float* abuf, float* cbuf, Small& sm, float (&a1)[16 * NLT]) {
    constexpr int TM = 16 * NLT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < g.RD * g.LDW; i += kNT) {
        const int d = i / g.LDW, l = i - d * g.LDW;
        wbuf[i] = (d < g.D && l < g.L) ? wc[(size_t)d * g.T + l] : 0.f;      // (words beyond the caption's length are never read)
    }
    __syncthreads();
    region_rows<NLT>(n, wbuf, abuf, g);                          // m[s][l] = <w_l, n_s>
    __syncthreads();
    const int r = tid;
#pragma unroll
    for (int l = 0; l < TM; ++l) a1[l] = 0.f;
    if (r < g.S) {                                               // sbar = softmax over the L words
        float* row = abuf + r * g.LDW;
        float mx = -INFINITY;
#pragma unroll
        for (int l = 0; l < TM; ++l)
            if (l < g.L) { a1[l] = row[l]; mx = fmaxf(mx, a1[l]); }
        float sum = 0.f;
#pragma unroll
        for (int l = 0; l < TM; ++l)
            if (l < g.L) { a1[l] = expf(a1[l] - mx); sum += a1[l]; }
        const float inv = 1.f / sum;
#pragma unroll
        for (int l = 0; l < TM; ++l)
            if (l < g.L) { a1[l] *= inv; row[l] = gamma1 * a1[l]; }
    } else if (r < g.RS) {
        for (int l = 0; l < g.LDW; ++l) abuf[r * g.LDW + l] = 0.f;           // the padded tail of the contexts' k axis
    }
    __syncthreads();
    for (int l = wave; l < g.L; l += kNW) {                      // alpha = softmax over the S regions, one word per wave
        float mx = -INFINITY;
        for (int s = lane; s < g.S; s += 64) mx = fmaxf(mx, abuf[s * g.LDW + l]);
        mx = wave_max(mx);
        float sum = 0.f;
        for (int s = lane; s < g.S; s += 64) sum += expf(abuf[s * g.LDW + l] - mx);
        sum = wave_sum(sum);
        if (lane == 0) { sm.colmax[l] = mx; sm.colsum[l] = sum; }
    }
    __syncthreads();
    if (r < g.S) {
        float* row = abuf + r * g.LDW;
        for (int l = 0; l < g.LDW; ++l) row[l] = l < g.L ? expf(row[l] - sm.colmax[l]) / sm.colsum[l] : 0.f;
    }
    __syncthreads();
    channel_rows<NLT>(n, abuf, cbuf, g);                         // ctx[d][l] = sum_s alpha[s][l] n[d][s]
    __syncthreads();
}

__device__ __forceinline__ PairDims pair_dims(int D, int T, int S, int L) {
    PairDims g;
    g.D = D, g.S = S, g.T = T, g.L = L;
    g.RD = round_up(D, 16), g.RS = round_up(S, 16);
    g.TP = round_up(T, 4), g.LDW = row_stride(T);
    return g;
}
__device__ __forceinline__ int caption_len(const int64_t* __restrict__ lens, int c, int T) {
    const int64_t v = lens[c];
    return v < 0 ? 0 : (v > T ? T : (int)v);
}

template <int NLT>
__global__ __launch_bounds__(kNT) void word_corr_fwd_kernel(const float* __restrict__ regions, const float* __restrict__ words,
                                                            const int64_t* __restrict__ lens, int shift, float gamma1, float gamma2,
                                                            float eps, float* __restrict__ p, float* __restrict__ r_out,
                                                            float* __restrict__ g_out, float* __restrict__ save, int B, int D, int T, int S) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    Small& sm = *reinterpret_cast<Small*>(smem_raw);
    const int b = blockIdx.x, c = (b + shift) % B;
    const PairDims g = pair_dims(D, T, S, caption_len(lens, c, T));
    float* wbuf = reinterpret_cast<float*>(smem_raw + sizeof(Small));
    float* abuf = wbuf + g.RD * g.LDW;
    float* cbuf = abuf + g.RS * g.LDW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float a1[16 * NLT];
    pair_attention<NLT>(regions + (size_t)b * D * S, words + (size_t)c * D * T, g, gamma1, wbuf, abuf, cbuf, sm, a1);
    if (tid < g.RD) {                                            // L * mean_k w_k, per channel
        float s = 0.f;
        for (int l = 0; l < g.L; ++l) s += wbuf[tid * g.LDW + l];
        sm.wsum[tid] = s;
    }
    __syncthreads();
    for (int l = wave; l < g.L; l += kNW) {                      // cosine and self-attention score per word, one word per wave
        float nu = 0.f, s1 = 0.f, s2 = 0.f, qv = 0.f;
        for (int d = lane; d < g.D; d += 64) {
            const float wv = wbuf[d * g.LDW + l], cv = cbuf[d * g.LDW + l];
            nu += wv * cv; s1 += wv * wv; s2 += cv * cv; qv += sm.wsum[d] * wv;
        }
        nu = wave_sum(nu); s1 = wave_sum(s1); s2 = wave_sum(s2); qv = wave_sum(qv);
        if (lane == 0) {
            const float na = sqrtf(s1), nb = sqrtf(s2);
            sm.num[l] = nu; sm.n1[l] = na; sm.n2[l] = nb;
            sm.r[l] = nu / fmaxf(na * nb, eps);
            sm.g[l] = qv / (float)g.L;                           // <mean_k w_k, w_l>, before the softmax
        }
    }
    __syncthreads();
    if (wave == 0) {                                             // lane l = word l (T <= 32 < 64)
        const bool live = lane < g.L;
        const float q = live ? sm.g[lane] : -INFINITY;
        const float mx = wave_max(q);
        const float e = live ? expf(q - mx) : 0.f;
        const float sum = wave_sum(e);
        const float gl = live ? e / sum : 0.f;
        const float rl = live ? sm.r[lane] : 0.f;
        const float pv = wave_sum(live ? gl * sigmoid_exact(gamma2 * rl) : 0.f);
        if (lane < T) {
            r_out[(size_t)b * T + lane] = rl;
            g_out[(size_t)b * T + lane] = gl;
            float* sv = save + (size_t)b * kSaveRows * T + lane;
            sv[0] = live ? sm.num[lane] : 0.f;
            sv[T] = live ? sm.n1[lane] : 0.f;
            sv[2 * T] = live ? sm.n2[lane] : 0.f;
            sv[3 * T] = rl;
            sv[4 * T] = gl;
        }
        if (lane == 0) p[b] = pv;
    }
}

template <int NLT>
__global__ __launch_bounds__(kNT) void word_corr_bwd_kernel(const float* __restrict__ regions, const float* __restrict__ words,
                                                            const int64_t* __restrict__ lens, int shift, const float* __restrict__ save,
                                                            const float* __restrict__ dp, float gamma1, float gamma2, float eps,
                                                            float* __restrict__ dregions, int B, int D, int T, int S) {
    constexpr int TM = 16 * NLT, KTM = 4 * NLT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    Small& sm = *reinterpret_cast<Small*>(smem_raw);
    const int b = blockIdx.x, c = (b + shift) % B;
    const PairDims g = pair_dims(D, T, S, caption_len(lens, c, T));
    float* wbuf = reinterpret_cast<float*>(smem_raw + sizeof(Small));        // words, then d alpha, then d m: max(RD, RS) rows
    float* abuf = wbuf + max(g.RD, g.RS) * g.LDW;
    float* cbuf = abuf + g.RS * g.LDW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mi = lane & 15, kq = lane >> 4;
    const float* n = regions + (size_t)b * D * S;
    const float* wc = words + (size_t)c * D * T;
    float a1[TM];
    pair_attention<NLT>(n, wc, g, gamma1, wbuf, abuf, cbuf, sm, a1);

    // --- d p -> d r_l -> the two coefficients of d ctx_l = ca_l w_l + cb_l ctx_l (the words are constants) ---
    if (tid < kMaxT) {
        float ca = 0.f, cb = 0.f;
        if (tid < g.L) {
            const float* sv = save + (size_t)b * kSaveRows * T + tid;
            const float num = sv[0], n1 = sv[T], n2 = sv[2 * T], rl = sv[3 * T], gl = sv[4 * T];
            const float sg = sigmoid_exact(gamma2 * rl);
            const float dr = dp[b] * gl * gamma2 * sg * (1.f - sg);
            const float nn = n1 * n2;
            if (nn > eps) {
                ca = dr / nn;
                if (n2 > 0.f) cb = -dr * num / (nn * nn) * n1 / n2;
            } else {
                ca = dr / eps;                                   // clamp(min=eps) active: the denominator is a constant
            }
        }
        sm.ca[tid] = ca; sm.cb[tid] = cb;
    }
    __syncthreads();
    for (int i = tid; i < g.RD * g.LDW; i += kNT) {
        const int l = i % g.LDW;
        cbuf[i] = l < g.L ? sm.ca[l] * wbuf[i] + sm.cb[l] * cbuf[i] : 0.f;
    }
    __syncthreads();
    region_rows<NLT>(n, cbuf, wbuf, g);                          // d alpha[s][l] = sum_d n[d][s] d ctx[d][l]  (over the words' storage)
    __syncthreads();
    const int r = tid;
    const bool rlive = r < g.S;
    float a2r[TM], da[TM];
#pragma unroll
    for (int l = 0; l < TM; ++l) {
        const bool live = rlive && l < g.L;
        a2r[l] = live ? abuf[r * g.LDW + l] : 0.f;
        da[l] = live ? wbuf[r * g.LDW + l] : 0.f;
    }
#pragma unroll
    for (int l = 0; l < TM; ++l) {
        const float v = wave_sum(a2r[l] * da[l]);
        if (lane == 0) sm.dotw[wave][l] = v;
    }
    __syncthreads();
    {
        float inner = 0.f;
#pragma unroll
        for (int l = 0; l < TM; ++l) {
            float dot = 0.f;
#pragma unroll
            for (int q = 0; q < kNW; ++q) dot += sm.dotw[q][l];                  // fixed order over the five waves
            da[l] = gamma1 * a2r[l] * (da[l] - dot);                             // softmax over regions backward = d sbar
            inner += a1[l] * da[l];
        }
#pragma unroll
        for (int l = 0; l < TM; ++l) da[l] = (rlive && l < g.L) ? a1[l] * (da[l] - inner) : 0.f;      // softmax over words backward = d m
    }
    if (r < g.RS) {
#pragma unroll
        for (int l = 0; l < TM; ++l)
            if (l < g.LDW) wbuf[r * g.LDW + l] = da[l];          // (zero for the padded rows and for l >= L)
    }
    __syncthreads();
    // --- dregions[d][s] = sum_l d ctx[d][l] alpha[s][l] + w[d][l] d m[s][l]: 16 x 16 tiles, k = the TP words of each term ---
    {
        const int nrt = g.RS >> 4, ndt = g.RD >> 4, KT = g.TP >> 2;
        const int nq = tiles_of_wave(nrt, wave);
        float ba[4][KTM], bd[4][KTM];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = min((wave + kNW * q) * 16 + mi, g.RS - 1);           // B[k = l][j = s]
#pragma unroll
            for (int t = 0; t < KTM; ++t) {
                ba[q][t] = t < KT ? abuf[row * g.LDW + 4 * t + kq] : 0.f;
                bd[q][t] = t < KT ? wbuf[row * g.LDW + 4 * t + kq] : 0.f;
            }
        }
        float* dn = dregions + (size_t)b * D * S;
        for (int dt = 0; dt < ndt; ++dt) {
            const int d = dt * 16 + mi;                                          // A[i = d][k = l]
            float ac[KTM], ae[KTM];
#pragma unroll
            for (int t = 0; t < KTM; ++t) {
                const int l = 4 * t + kq;
                ac[t] = t < KT ? cbuf[d * g.LDW + l] : 0.f;
                ae[t] = (d < g.D && l < g.L) ? wc[(size_t)d * g.T + l] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nq) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int t = 0; t < KTM; ++t)
                        if (t < KT) acc = mfma4(ac[t], ba[q][t], acc);
#pragma unroll
                    for (int t = 0; t < KTM; ++t)
                        if (t < KT) acc = mfma4(ae[t], bd[q][t], acc);
                    const int s = (wave + kNW * q) * 16 + mi;
                    if (s < g.S) {
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) {
                            const int dd = dt * 16 + 4 * kq + rr;
                            if (dd < g.D) dn[(size_t)dd * g.S + s] = acc[rr];
                        }
                    }
                }
        }
    }
}

inline bool shape_ok(int B, int D, int T, int S) { return B >= 1 && B <= kMaxB && D >= 1 && D <= kNT && S >= 1 && S <= kNT && T >= 1 && T <= kMaxT; }

inline size_t lds_bytes(int D, int T, int S, bool bwd) {
    const int RD = round_up(D, 16), RS = round_up(S, 16);
    return sizeof(Small) + (size_t)((bwd ? std::max(RD, RS) : RD) + RS + RD) * row_stride(T) * sizeof(float);
}
// the most any shape of the domain asks for: what the kernels are allowed once per process
inline int lds_limit(bool bwd) { return (int)lds_bytes(kNT, kMaxT, kNT, bwd); }

#define WORD_CORR_SHAPE(what)                                                                                                              \
    AGAN_REQUIRE(shape_ok(B, D, T, S), what ": shape B=%d D=%d T=%d S=%d out of range (B in [1,%d], D and S in [1,%d], T in [1,%d])", B, D, \
                 T, S, kMaxB, kNT, kMaxT);                                                                                                 \
    AGAN_REQUIRE(shift >= 0 && shift < B, what ": shift %d outside [0, B = %d)", shift, B)

}  // namespace

extern "C" {

size_t agan_word_corr_save_elems(int B, int D, int T, int S) {
    if (!shape_ok(B, D, T, S)) {                                  // (a size has no error code: 0 elements and the message)
        set_error("word_corr_save_elems: shape B=%d D=%d T=%d S=%d out of range (B in [1,%d], D and S in [1,%d], T in [1,%d])", B, D, T, S,
                  kMaxB, kNT, kMaxT);
        return 0;
    }
    return (size_t)B * kSaveRows * T;
}

int agan_word_corr_fwd(const float* regions, const float* words, const int64_t* lens, int shift, float gamma1, float gamma2, float eps,
                       float* p, float* r, float* g, float* save, int B, int D, int T, int S, void* stream) {
    WORD_CORR_SHAPE("word_corr_fwd");
    AGAN_REQUIRE(regions && words && lens && p && r && g && save, "word_corr_fwd: null pointer");
    with_tier<16, 32>(T, [&](auto TM) {
        constexpr int NLT = TM() / 16;
        allow_dynamic_lds<word_corr_fwd_kernel<NLT>>(lds_limit(false));
        hipLaunchKernelGGL((word_corr_fwd_kernel<NLT>), dim3(B), dim3(kNT), lds_bytes(D, T, S, false), as_stream(stream), regions, words, lens,
                           shift, gamma1, gamma2, eps, p, r, g, save, B, D, T, S);
    });
    return check_launch("word_corr_fwd");
}

size_t agan_word_corr_bwd_ws_bytes(int B, int D, int T, int S) {
    if (!shape_ok(B, D, T, S))
        set_error("word_corr_bwd_ws_bytes: shape B=%d D=%d T=%d S=%d out of range (B in [1,%d], D and S in [1,%d], T in [1,%d])", B, D, T, S,
                  kMaxB, kNT, kMaxT);
    return 0;                                                     // every dregions slab has one owner: nothing to stage
}

int agan_word_corr_bwd(const float* regions, const float* words, const int64_t* lens, int shift, const float* save, const float* dp,
                       float gamma1, float gamma2, float eps, float* dregions, int B, int D, int T, int S, void* ws, size_t ws_bytes,
                       void* stream) {
    WORD_CORR_SHAPE("word_corr_bwd");
    AGAN_REQUIRE(regions && words && lens && save && dp && dregions, "word_corr_bwd: null pointer");
    (void)ws, (void)ws_bytes;
    with_tier<16, 32>(T, [&](auto TM) {
        constexpr int NLT = TM() / 16;
        allow_dynamic_lds<word_corr_bwd_kernel<NLT>>(lds_limit(true));
        hipLaunchKernelGGL((word_corr_bwd_kernel<NLT>), dim3(B), dim3(kNT), lds_bytes(D, T, S, true), as_stream(stream), regions, words, lens,
                           shift, save, dp, gamma1, gamma2, eps, dregions, B, D, T, S);
    });
    return check_launch("word_corr_bwd");
}

}  // extern "C"
