// Dynamic memory of a refinement stage (networks/memory.py: DynamicMemory; DM-GAN, Zhu et al., CVPR 2019), fp32.
//
//   write    m[b,t,d]  = relu(U[b,t,d]) g + relu(Q[b,d]) (1 - g),   g = sigmoid(U[b,t,Md] + Q[b,Md])                 (B x T sized: tiny)
//   read     s[t] = sum_c k[b,t,c] h[b,c,p], masked words -inf,  alpha = softmax_t(s),  o[c] = sum_t v[b,t,c] alpha[t]
//   respond  z = sum_c (rw[c] h[b,c,p] + rw[C+c] o[c]) + rb,  g_r = sigmoid(z),  r[c] = h[b,c,p] (1 - g_r) + g_r o[c],  x = cat(r, r)
//
// with k = kv[:, :, :C] and v = kv[:, :, C:].  Read and respond are ONE streaming pass per direction in the form of attention.hip: a
// lane owns a pixel, k and v sit in LDS (transposed to [channel][word], zero-padded to the TMAX tier, every read a broadcast), the
// scores stay in registers.  The forward reads h once (the channels wait in registers for the gate) and writes both halves of x and
// the attention map: 4 (C + 2C + T) bytes per pixel.  The gate needs sum_c rw[C+c] o[c] BEFORE the o[c] can be blended; it is taken as
// sum_t alpha[t] vw[t] with vw[t] = sum_c rw[C+c] v[t,c] (one value per word, made once per workgroup), so no o[] array is kept.
// The backward keeps nothing but the attention map: o and g_r are recomputed.
#include "agan_common.h"
#include "dispatch.h"
#include "mfma_tile.h"

using namespace agan;

namespace {

constexpr int kMaxC = 64;   // channels of h (k and v have as many)
constexpr int kMaxT = 64;   // words
constexpr int kCU = 4;      // channels whose loads are issued together in the backward's channel loops
constexpr int kMemLd = 68;  // row stride (floats) of the per-wave transposition tiles of the backward (attention.hip: kAttLd)

// ---------------------------------------------------------------------------------------------------------------------- write
__global__ __launch_bounds__(256) void mem_write_fwd_kernel(const float* __restrict__ U, const float* __restrict__ Q,
                                                            float* __restrict__ m, int T, int Md, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int d = i % Md, bt = i / Md, b = bt / T;
    const float* u = U + (size_t)bt * (Md + 1);
    const float* q = Q + (size_t)b * (Md + 1);
    const float g = sigmoid_fast(u[Md] + q[Md]);
    m[i] = fmaxf(u[d], 0.f) * g + fmaxf(q[d], 0.f) * (1.f - g);
}

// one workgroup per sample.  Pass 1, a wave per word: dU of the word and its gate gradient (one butterfly over d).  Pass 2, a thread
// per d: dQ[b,d] summed over the words in word order.  No atomics.
__global__ __launch_bounds__(256) void mem_write_bwd_kernel(const float* __restrict__ U, const float* __restrict__ Q,
                                                            const float* __restrict__ dm, float* __restrict__ dU,
                                                            float* __restrict__ dQ, int T, int Md) {
    __shared__ float gs[kMaxT], dgs[kMaxT];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* q = Q + (size_t)b * (Md + 1);
    for (int t = wave; t < T; t += 4) {                                       // wave-uniform
        const size_t bt = (size_t)b * T + t;
        const float* u = U + bt * (Md + 1);
        const float* dr = dm + bt * Md;
        float* du = dU + bt * (Md + 1);
        const float g = sigmoid_fast(u[Md] + q[Md]);
        float s = 0.f;
        for (int d = lane; d < Md; d += 64) {
            const float uv = u[d], qv = q[d], dv = dr[d];
            s += dv * (fmaxf(uv, 0.f) - fmaxf(qv, 0.f));
            du[d] = uv > 0.f ? dv * g : 0.f;
        }
        s = wave_sum(s) * g * (1.f - g);
        if (lane == 0) {
            gs[t] = g;
            dgs[t] = s;
            du[Md] = s;
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d <= Md; d += 256) {
        float s = 0.f;
        if (d == Md) {
            for (int t = 0; t < T; ++t) s += dgs[t];
        } else if (q[d] > 0.f) {
            for (int t = 0; t < T; ++t) s += dm[((size_t)b * T + t) * Md + d] * (1.f - gs[t]);
        }
        dQ[(size_t)b * (Md + 1) + d] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- read
// ks[c][t] = kv[b,t,c], vs[c][t] = kv[b,t,C+c], zero outside C x T; rows of TMAX floats
template <int TMAX>
__device__ __forceinline__ void stage_kv(const float* __restrict__ kv, float* __restrict__ ks, float* __restrict__ vs, int b, int C,
                                         int T, int rows) {
    for (int i = threadIdx.x; i < rows * TMAX; i += 256) {
        const int t = i / rows, c = i - t * rows;                           // c fastest: the global reads of a word are contiguous
        const bool on = t < T && c < C;
        const float* src = kv + ((size_t)b * T + t) * 2 * C + c;
        ks[c * TMAX + t] = on ? src[0] : 0.f;
        vs[c * TMAX + t] = on ? src[C] : 0.f;
    }
}

template <int TMAX, int CMAX>
__global__ __launch_bounds__(256) void mem_read_fwd_kernel(const float* __restrict__ h, const float* __restrict__ kv,
                                                           const int64_t* __restrict__ mask, const float* __restrict__ rw,
                                                           const float* __restrict__ rb, float* __restrict__ x,
                                                           float* __restrict__ attn, int C, int T, int HW) {
    __shared__ __attribute__((aligned(16))) float ks[CMAX * TMAX];
    __shared__ __attribute__((aligned(16))) float vs[CMAX * TMAX];
    __shared__ float neg[TMAX];          // 0 for a live word, -inf for masked / padded
    __shared__ float vw[TMAX];           // sum_c rw[C+c] v[t,c]
    __shared__ float rws[2 * CMAX];      // rw[c] | rw[C+c], zero-padded
    const int b = blockIdx.y;
    stage_kv<TMAX>(kv, ks, vs, b, C, T, CMAX);
    for (int i = threadIdx.x; i < 2 * CMAX; i += 256) {
        const int half = i / CMAX, c = i - half * CMAX;
        rws[i] = c < C ? rw[half * C + c] : 0.f;
    }
    for (int t = threadIdx.x; t < TMAX; t += 256) neg[t] = (t < T && mask[(size_t)b * T + t] != 0) ? 0.f : -INFINITY;
    __syncthreads();
    for (int t = threadIdx.x; t < TMAX; t += 256) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += rws[CMAX + c] * vs[c * TMAX + t];
        vw[t] = s;
    }
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const size_t h0 = (size_t)b * C * HW + p, x0 = (size_t)b * 2 * C * HW + p;
    float hr[CMAX];                      // the pixel's channels: read once, used by the scores, the gate and the blend
#pragma unroll
    for (int c = 0; c < CMAX; ++c) hr[c] = c < C ? h[h0 + (size_t)c * HW] : 0.f;
    float sc[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) sc[t] = 0.f;
    float z = rb[0];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (c < C) {                                                          // workgroup-uniform
            z += rws[c] * hr[c];
#pragma unroll
            for (int t = 0; t < TMAX; ++t) sc[t] += hr[c] * ks[c * TMAX + t];
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        sc[t] += neg[t];
        mx = fmaxf(mx, sc[t]);
    }
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        sc[t] = __expf(sc[t] - mx);      // all-masked row: exp(-inf - -inf) = NaN, like AttentionModule
        sum += sc[t];
    }
    const float inv = 1.f / sum;
    float* ao = attn + (size_t)b * T * HW + p;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        sc[t] *= inv;
        z += sc[t] * vw[t];
        if (t < T) ao[(size_t)t * HW] = sc[t];
    }
    const float g = sigmoid_fast(z);
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (c < C) {
            float o = 0.f;
#pragma unroll
            for (int t = 0; t < TMAX; ++t) o += vs[c * TMAX + t] * sc[t];
            const float r = hr[c] * (1.f - g) + g * o;
            x[x0 + (size_t)c * HW] = r;
            x[x0 + (size_t)(C + c) * HW] = r;
        }
    }
}

// Backward of the streaming pass.  Per pixel, with d[c] = dx[c] + dx[C+c] (the gradient of r):
//   pass A   o[c], z, g_r recomputed;  dg = sum_c d[c] (o[c] - h[c]);  e[t] = sum_c d[c] v[t,c]
//            dz = dg g_r (1 - g_r);  dalpha[t] = g_r e[t] + dz vw[t] (+ dattn[t]);  ds[t] = alpha[t] (dalpha[t] - sum_u alpha[u] dalpha[u])
//   pass K   dh[c] = (1 - g_r) d[c] + dz rw[c] + sum_t ds[t] k[t,c];  dk[t,c] += ds[t] h[c];  drw[c] += dz h[c]
//   pass V   dv[t,c] += (g_r d[c] + dz rw[C+c]) alpha[t]
// and drw[C+c] = sum_t v[t,c] W[t] with W[t] = sum over the pixels of dz alpha[t], drb = sum dz.  Sums over the pixels of a workgroup
// run WITHOUT atomics, as in attn_bwd_kernel: a reduction inside each wave, one LDS row per wave, a fixed-order sum of the four rows,
// one partial slab per workgroup that mem_read_reduce_kernel sums in workgroup order.  dk and dv go through the SAME four wave rows one
// after the other (the two together would take the whole LDS at C = T = 64), which costs another read of dx; h is read twice (gate,
// then dh / dk).
// The reduction inside a wave is a (channels x words x 64 pixels) contraction whose reduction axis is the LANE axis.  TMAX 16 and 32:
// each wave transposes its 64 pixels through a private LDS tile and lets v_mfma_f32_16x16x4_f32 reduce them, 16 channels at a time
// (A[i = channel][k = pixel], B[k = pixel][j = word], 16 k-steps per 16 x 16 tile; row stride kMemLd = 68 floats: conflict-free
// operand reads) -- as a butterfly the same sums cost TMAX + 1 cross-lane shuffles per channel and reduction and made the kernel 2x
// the time of attn_bwd_kernel.  TMAX 64 keeps the butterfly: with the tiles its LDS would pass 160 KB.
// LDS: 6 C TMAX floats + 6 TMAX + 6 kMaxC + 4, + 4 (TMAX + 16) kMemLd for the tiles.
template <int TMAX>
__global__ __launch_bounds__(256) void mem_read_bwd_kernel(const float* __restrict__ h, const float* __restrict__ kv,
                                                           const float* __restrict__ rw, const float* __restrict__ rb,
                                                           const float* __restrict__ attn, const float* __restrict__ dx,
                                                           const float* __restrict__ dattn, float* __restrict__ dh,
                                                           float* __restrict__ part_kv, float* __restrict__ part_rw, int C, int T,
                                                           int HW) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* ks = reinterpret_cast<float*>(smem_raw);      // [C][TMAX]
    float* vs = ks + C * TMAX;                           // [C][TMAX]
    float* acc = vs + C * TMAX;                          // [4 waves][C][TMAX]
    float* vw = acc + 4 * C * TMAX;                      // [TMAX]
    float* wt = vw + TMAX;                               // [4 waves][TMAX]: W[t] per wave
    float* wts = wt + 4 * TMAX;                          // [TMAX]: W[t] of the workgroup
    float* rws = wts + TMAX;                             // [2][kMaxC]
    float* accw = rws + 2 * kMaxC;                       // [4 waves][kMaxC + 1]: drw[c] per wave, drb in the last column
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr bool kMfma = TMAX <= 32;
    constexpr int NT = TMAX / 16;                        // 16-word tiles
    float* Yw = accw + 4 * (kMaxC + 1) + wave * ((TMAX + 16) * kMemLd);      // (kMfma) [TMAX][kMemLd]: ds, then alpha, pixel along the row
    float* Xw = Yw + TMAX * kMemLd;                                            // (kMfma) [16][kMemLd]: 16 channels of h, then of do
    const int mi = lane & 15, kq = lane >> 4;
    stage_kv<TMAX>(kv, ks, vs, b, C, T, C);
    for (int i = threadIdx.x; i < 2 * kMaxC; i += 256) {
        const int half = i / kMaxC, c = i - half * kMaxC;
        rws[i] = c < C ? rw[half * C + c] : 0.f;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < TMAX; t += 256) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += rws[kMaxC + c] * vs[c * TMAX + t];
        vw[t] = s;
    }
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool live = p < HW;                            // a lane past the map carries zeros through every sum (no early return: the
    const size_t pp = live ? p : 0;                      // butterflies need all 64 lanes)
    const size_t h0 = (size_t)b * C * HW + pp, x0 = (size_t)b * 2 * C * HW + pp;
    float a[TMAX], ds[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        a[t] = (live && t < T) ? attn[((size_t)b * T + t) * HW + pp] : 0.f;
        ds[t] = 0.f;                                     // e[t] first, then dalpha[t], then ds[t]
    }
    // ---- pass A
    float z = rb[0], dg = 0.f;
    for (int c0 = 0; c0 < C; c0 += kCU) {
        float hv[kCU], dv[kCU];
#pragma unroll
        for (int j = 0; j < kCU; ++j) {
            const bool on = live && c0 + j < C;
            hv[j] = on ? h[h0 + (size_t)(c0 + j) * HW] : 0.f;
            dv[j] = on ? dx[x0 + (size_t)(c0 + j) * HW] + dx[x0 + (size_t)(C + c0 + j) * HW] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kCU; ++j) {
            const int c = c0 + j;
            if (c < C) {                                                     // workgroup-uniform
                z += rws[c] * hv[j];
                float o = 0.f;
#pragma unroll
                for (int t = 0; t < TMAX; ++t) {
                    const float v = vs[c * TMAX + t];
                    o += v * a[t];
                    ds[t] += dv[j] * v;
                }
                dg += dv[j] * (o - hv[j]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t) z += a[t] * vw[t];
    const float g = sigmoid_fast(z);
    const float dz = dg * g * (1.f - g);                 // 0 in a lane past the map (dg = 0)
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        ds[t] = g * ds[t] + dz * vw[t];
        if (dattn && live && t < T) ds[t] += dattn[((size_t)b * T + t) * HW + pp];
        dot += a[t] * ds[t];
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t) ds[t] = a[t] * (ds[t] - dot);
    {
        float part[TMAX];
#pragma unroll
        for (int t = 0; t < TMAX; ++t) part[t] = dz * a[t];
        int t_own;
        const float r = wave_sum_scatter<TMAX>(part, lane, t_own);
        if ((lane & (64 / TMAX - 1)) == 0) wt[wave * TMAX + t_own] = r;
        const float sb = wave_sum(dz);
        if (lane == 0) accw[wave * (kMaxC + 1) + kMaxC] = sb;
    }
    // ---- pass K
    if constexpr (kMfma) {
#pragma unroll
        for (int t = 0; t < TMAX; ++t) Yw[t * kMemLd + lane] = ds[t];
        wave_lds_sync();
        float Bd[NT][16];
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int k = 0; k < 16; ++k) Bd[n][k] = Yw[(16 * n + mi) * kMemLd + 4 * k + kq];
        for (int c0 = 0; c0 < C; c0 += 16) {
            float hv[16], dv[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const bool on = live && c0 + j < C;
                hv[j] = on ? h[h0 + (size_t)(c0 + j) * HW] : 0.f;
                dv[j] = on ? dx[x0 + (size_t)(c0 + j) * HW] + dx[x0 + (size_t)(C + c0 + j) * HW] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) Xw[j * kMemLd + lane] = hv[j];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = c0 + j;
                if (c < C) {                                                     // workgroup-uniform
                    float s = (1.f - g) * dv[j] + dz * rws[c];
#pragma unroll
                    for (int t = 0; t < TMAX; ++t) s += ds[t] * ks[c * TMAX + t];
                    if (live) dh[h0 + (size_t)c * HW] = s;
                    const float sw = wave_sum(dz * hv[j]);
                    if (lane == 0) accw[wave * (kMaxC + 1) + c] = sw;
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 16; ++k) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(Xw[mi * kMemLd + 4 * k + kq], Bd[n][k], dp, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {                                    // D[i = 4 (l >> 4) + r][j = l & 15]
                    const int c = c0 + 4 * kq + r;
                    if (c < C) acc[(wave * C + c) * TMAX + 16 * n + mi] = dp[r];
                }
            }
            wave_lds_sync();
        }
    } else {
    for (int c0 = 0; c0 < C; c0 += kCU) {
        float hv[kCU], dv[kCU];
#pragma unroll
        for (int j = 0; j < kCU; ++j) {
            const bool on = live && c0 + j < C;
            hv[j] = on ? h[h0 + (size_t)(c0 + j) * HW] : 0.f;
            dv[j] = on ? dx[x0 + (size_t)(c0 + j) * HW] + dx[x0 + (size_t)(C + c0 + j) * HW] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kCU; ++j) {
            const int c = c0 + j;
            if (c < C) {
                float s = (1.f - g) * dv[j] + dz * rws[c];
                float part[TMAX];
#pragma unroll
                for (int t = 0; t < TMAX; ++t) {
                    s += ds[t] * ks[c * TMAX + t];
                    part[t] = ds[t] * hv[j];
                }
                if (live) dh[h0 + (size_t)c * HW] = s;
                int t_own;
                const float r = wave_sum_scatter<TMAX>(part, lane, t_own);
                if ((lane & (64 / TMAX - 1)) == 0) acc[(wave * C + c) * TMAX + t_own] = r;
                const float sw = wave_sum(dz * hv[j]);
                if (lane == 0) accw[wave * (kMaxC + 1) + c] = sw;
            }
        }
    }
    }
    __syncthreads();
    float* dst = part_kv + ((size_t)b * gridDim.x + blockIdx.x) * T * 2 * C;      // [T][2C] like kv
    for (int i = threadIdx.x; i < C * T; i += 256) {
        const int t = i / C, c = i - t * C;
        const int e = c * TMAX + t;
        dst[t * 2 * C + c] = ((acc[e] + acc[C * TMAX + e]) + acc[2 * C * TMAX + e]) + acc[3 * C * TMAX + e];
    }
    for (int t = threadIdx.x; t < TMAX; t += 256) wts[t] = ((wt[t] + wt[TMAX + t]) + wt[2 * TMAX + t]) + wt[3 * TMAX + t];
    __syncthreads();
    float* dsw = part_rw + ((size_t)b * gridDim.x + blockIdx.x) * (2 * C + 1);       // drw[2C] | drb
    for (int i = threadIdx.x; i <= 2 * C; i += 256) {
        float s = 0.f;
        if (i < C) {
            s = ((accw[i] + accw[kMaxC + 1 + i]) + accw[2 * (kMaxC + 1) + i]) + accw[3 * (kMaxC + 1) + i];
        } else if (i < 2 * C) {
            for (int t = 0; t < T; ++t) s += vs[(i - C) * TMAX + t] * wts[t];
        } else {
            s = ((accw[kMaxC] + accw[kMaxC + 1 + kMaxC]) + accw[2 * (kMaxC + 1) + kMaxC]) + accw[3 * (kMaxC + 1) + kMaxC];
        }
        dsw[i] = s;
    }
    // ---- pass V (the wave rows are free again: every thread is past the barrier above)
    if constexpr (kMfma) {
        wave_lds_sync();
#pragma unroll
        for (int t = 0; t < TMAX; ++t) Yw[t * kMemLd + lane] = a[t];
        wave_lds_sync();
        float Ba[NT][16];
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int k = 0; k < 16; ++k) Ba[n][k] = Yw[(16 * n + mi) * kMemLd + 4 * k + kq];
        for (int c0 = 0; c0 < C; c0 += 16) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const bool on = live && c0 + j < C;
                const float dv = on ? dx[x0 + (size_t)(c0 + j) * HW] + dx[x0 + (size_t)(C + c0 + j) * HW] : 0.f;
                Xw[j * kMemLd + lane] = on ? g * dv + dz * rws[kMaxC + c0 + j] : 0.f;
            }
            wave_lds_sync();
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 16; ++k) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(Xw[mi * kMemLd + 4 * k + kq], Ba[n][k], dp, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = c0 + 4 * kq + r;
                    if (c < C) acc[(wave * C + c) * TMAX + 16 * n + mi] = dp[r];
                }
            }
            wave_lds_sync();
        }
    } else {
    for (int c0 = 0; c0 < C; c0 += kCU) {
        float dv[kCU];
#pragma unroll
        for (int j = 0; j < kCU; ++j) {
            const bool on = live && c0 + j < C;
            dv[j] = on ? dx[x0 + (size_t)(c0 + j) * HW] + dx[x0 + (size_t)(C + c0 + j) * HW] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kCU; ++j) {
            const int c = c0 + j;
            if (c < C) {
                const float dco = g * dv[j] + dz * rws[kMaxC + c];
                float part[TMAX];
#pragma unroll
                for (int t = 0; t < TMAX; ++t) part[t] = dco * a[t];
                int t_own;
                const float r = wave_sum_scatter<TMAX>(part, lane, t_own);
                if ((lane & (64 / TMAX - 1)) == 0) acc[(wave * C + c) * TMAX + t_own] = r;
            }
        }
    }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * T; i += 256) {
        const int t = i / C, c = i - t * C;
        const int e = c * TMAX + t;
        dst[t * 2 * C + C + c] = ((acc[e] + acc[C * TMAX + e]) + acc[2 * C * TMAX + e]) + acc[3 * C * TMAX + e];
    }
}

// dkv[b][t][j] = sum over the pixel workgroups of their slabs, in workgroup order; drw[j] / drb = the same over samples and workgroups
__global__ __launch_bounds__(256) void mem_read_reduce_kernel(const float* __restrict__ part_kv, const float* __restrict__ part_rw,
                                                              float* __restrict__ dkv, float* __restrict__ drw,
                                                              float* __restrict__ drb, int B, int nblk, int TC2, int C2, int acc_rw,
                                                              int acc_rb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int nkv = B * TC2;
    if (i < nkv) {
        const int b = i / TC2, e = i - b * TC2;
        const float* p = part_kv + (size_t)b * nblk * TC2 + e;
        float s = 0.f;
        for (int k = 0; k < nblk; ++k) s += p[(size_t)k * TC2];
        dkv[i] = s;
    } else if (i <= nkv + C2) {
        const int j = i - nkv;
        float s = 0.f;
        for (int r = 0; r < B * nblk; ++r) s += part_rw[(size_t)r * (C2 + 1) + j];
        if (j < C2) drw[j] = acc_rw ? drw[j] + s : s;
        else drb[0] = acc_rb ? drb[0] + s : s;
    }
}

size_t read_bwd_lds(int C, int TM) {
    return sizeof(float) * ((size_t)6 * C * TM + 6 * TM + 6 * kMaxC + 4 + (TM <= 32 ? 4 * (TM + 16) * kMemLd : 0));
}

bool read_shape_ok(int B, int C, int T, int HW) {
    return B > 0 && C > 0 && T > 0 && HW > 0 && C <= kMaxC && T <= kMaxT && B <= 65535 &&
           (long long)B * 2 * C * HW < (1LL << 31) && (long long)B * T * HW < (1LL << 31);
}

}  // namespace

extern "C" {

int agan_mem_write_fwd(const float* U, const float* Q, float* m, int B, int T, int Md, void* stream) {
    AGAN_REQUIRE(U && Q && m, "mem_write_fwd: null pointer");
    AGAN_REQUIRE(B > 0 && T > 0 && Md > 0, "mem_write_fwd: non-positive dimension");
    AGAN_REQUIRE(T <= kMaxT, "mem_write_fwd: seq_len %d > %d", T, kMaxT);
    AGAN_REQUIRE((long long)B * T * ((long long)Md + 1) < (1LL << 31), "mem_write_fwd: B * T * (memory_dim + 1) must stay below 2^31");
    const int n = B * T * Md;
    hipLaunchKernelGGL(mem_write_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), U, Q, m, T, Md, n);
    return check_launch("mem_write_fwd");
}

int agan_mem_write_bwd(const float* U, const float* Q, const float* dm, float* dU, float* dQ, int B, int T, int Md, void* stream) {
    AGAN_REQUIRE(U && Q && dm && dU && dQ, "mem_write_bwd: null pointer");
    AGAN_REQUIRE(B > 0 && T > 0 && Md > 0, "mem_write_bwd: non-positive dimension");
    AGAN_REQUIRE(T <= kMaxT, "mem_write_bwd: seq_len %d > %d", T, kMaxT);
    AGAN_REQUIRE((long long)B * T * ((long long)Md + 1) < (1LL << 31), "mem_write_bwd: B * T * (memory_dim + 1) must stay below 2^31");
    hipLaunchKernelGGL(mem_write_bwd_kernel, dim3(B), dim3(256), 0, as_stream(stream), U, Q, dm, dU, dQ, T, Md);
    return check_launch("mem_write_bwd");
}

int agan_mem_read_fwd(const float* h, const float* kv, const int64_t* mask, const float* rw, const float* rb, float* x, float* attn,
                      int B, int C, int T, int HW, void* stream) {
    AGAN_REQUIRE(h && kv && mask && rw && rb && x && attn, "mem_read_fwd: null pointer");
    AGAN_REQUIRE(B > 0 && C > 0 && T > 0 && HW > 0, "mem_read_fwd: non-positive dimension");
    AGAN_REQUIRE(C <= kMaxC, "mem_read_fwd: nc_in %d > %d", C, kMaxC);
    AGAN_REQUIRE(T <= kMaxT, "mem_read_fwd: seq_len %d > %d", T, kMaxT);
    AGAN_REQUIRE(read_shape_ok(B, C, T, HW), "mem_read_fwd: B * 2 nc_in * HW and B * seq_len * HW must stay below 2^31, B below 65536");
    hipStream_t st = as_stream(stream);
    const dim3 grid(cdiv(HW, 256), B);
    with_tier<16, 32, 64>(T, [&](auto TM) { with_tier<16, 32, 64>(C, [&](auto CM) {
        hipLaunchKernelGGL((mem_read_fwd_kernel<TM(), CM()>), grid, dim3(256), 0, st, h, kv, mask, rw, rb, x, attn, C, T, HW);
    }); });
    return check_launch("mem_read_fwd");
}

size_t agan_mem_read_bwd_ws_bytes(int B, int C, int T, int HW) {
    if (!read_shape_ok(B, C, T, HW)) return 0;
    return (size_t)B * cdiv(HW, 256) * ((size_t)T * 2 * C + 2 * C + 1) * sizeof(float);      // a dkv slab and a drw | drb slab per workgroup
}

int agan_mem_read_bwd(const float* h, const float* kv, const int64_t* mask, const float* rw, const float* rb, const float* attn,
                      const float* dx, const float* dattn, float* dh, float* dkv, float* drw, float* drb, int B, int C, int T, int HW,
                      int accumulate_rw, int accumulate_rb, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(h && kv && mask && rw && rb && attn && dx && dh && dkv && drw && drb && ws, "mem_read_bwd: null pointer");
    AGAN_REQUIRE(B > 0 && C > 0 && T > 0 && HW > 0, "mem_read_bwd: non-positive dimension");
    AGAN_REQUIRE(C <= kMaxC && T <= kMaxT, "mem_read_bwd: nc_in %d / seq_len %d out of range", C, T);
    AGAN_REQUIRE(read_shape_ok(B, C, T, HW), "mem_read_bwd: B * 2 nc_in * HW and B * seq_len * HW must stay below 2^31, B below 65536");
    if (int e = check_ws("mem_read_bwd", agan_mem_read_bwd_ws_bytes(B, C, T, HW), ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    const int nblk = cdiv(HW, 256);
    float* part_kv = static_cast<float*>(ws);
    float* part_rw = part_kv + (size_t)B * nblk * T * 2 * C;
    with_tier<16, 32, 64>(T, [&](auto TM) {
        allow_dynamic_lds<mem_read_bwd_kernel<TM()>>((int)read_bwd_lds(kMaxC, TM()));
        hipLaunchKernelGGL((mem_read_bwd_kernel<TM()>), dim3(nblk, B), dim3(256), read_bwd_lds(C, TM()), st, h, kv, rw, rb, attn, dx, dattn,
                           dh, part_kv, part_rw, C, T, HW);
    });
    hipLaunchKernelGGL(mem_read_reduce_kernel, dim3(cdiv(B * T * 2 * C + 2 * C + 1, 256)), dim3(256), 0, st, part_kv, part_rw, dkv, drw, drb, B,
                       nblk, T * 2 * C, 2 * C, accumulate_rw, accumulate_rb);
    return check_launch("mem_read_bwd");
}

}  // extern "C"
