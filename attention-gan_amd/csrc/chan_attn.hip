// Channel-wise word attention of a refinement stage (networks/attention.py: ChannelAttention; ControlGAN, Li et al., NeurIPS 2019), fp32.
//
//   score    m[b,c,t] = scale * sum_p h[b,c,p] wt[b,t,p], masked words -inf          (wt [B, T, HW]: the perception layer's output)
//   attend   alpha[b,c,:] = softmax_t m[b,c,:]
//   read     f[b,c,p] = sum_t alpha[b,c,t] wt[b,t,p]
//
// Where AttentionModule's kernels contract over the channels of one pixel, the score here contracts over the PIXELS (4096 .. 65536 of
// them), so it cannot stay inside a lane.  Three launches per direction:
//   1. chan_contract_kernel: a workgroup takes 256 pixels, a wave 64 of them.  The wave loads its pixels of every word and channel
//      coalesced (a lane owns a pixel), stages them through a private LDS tile into the operand layout of v_mfma_f32_16x16x4_f32
//      (A[i = channel][k = pixel], B[k = pixel][j = word], 16 k-steps; the technique of mem_read_bwd_kernel / attn_bwd_kernel<16>) and
//      keeps all C x T accumulators in registers -- every tier of T, no butterfly form.  The four waves' results meet in LDS in a fixed
//      order and leave as ONE partial [C, T] slab per workgroup.  The backward's dalpha = df . wt is the same kernel on df.
//   2. chan_softmax_kernel / chan_softmax_bwd_kernel: a wave per (b, c) row, a lane per word; sums the slabs in workgroup order, then
//      the softmax (or its backward) with two wave reductions.  B C T values: a launch of its own because the alternative, summing the
//      slabs in the prologue of pass 3, would have every one of the B * HW / 256 workgroups re-read all HW / 256 slabs of its sample.
//   3. chan_read_kernel / chan_bwd_kernel: one pixel per lane in the form of attn_fwd_kernel -- the pixel's T values of wt in
//      registers, alpha (and dm) in LDS zero-padded to the tiers so the inner loops carry no bounds checks and every LDS read is a
//      broadcast, coalesced stores.  dwt is written once per element by the lane that owns the pixel.
// No float atomics anywhere: two runs give the same bits.
// Algorithmic bytes per pixel: forward 4 (C + T) + 4 (T + C); backward 4 (C + T) + 4 (2C + T + C + T).
#include "agan_common.h"
#include "dispatch.h"
#include "mfma_tile.h"

using namespace agan;

namespace {

constexpr int kMaxC = 64;   // channels of h
constexpr int kMaxT = 64;   // words
constexpr int kCU = 4;      // channels whose loads are issued together in the backward's channel loop
// Row stride (floats) of the per-wave operand tiles.  The operand read of lane (i = l & 15, k = l >> 4) is a 4-byte LDS read at
// i * kChLd + 4 step + k: served per 32-lane half (k in {0, 1} or {2, 3}) over 32 banks, bank 2 i + k (+ 4 step) -- all distinct.
constexpr int kChLd = 66;

constexpr int contract_tile(int TM, int CM) { return (TM + CM) * kChLd; }                               // floats per wave
constexpr size_t contract_lds(int TM, int CM) { return sizeof(float) * 4 * contract_tile(TM, CM); }     // bytes per workgroup

// part[b][workgroup][c][t] = sum over the workgroup's 256 pixels of x[b,c,p] wt[b,t,p];  x = h (scores) or df (dalpha)
template <int TMAX, int CMAX>
__global__ __launch_bounds__(256) void chan_contract_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                            float* __restrict__ part, int C, int T, int HW) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NT = TMAX / 16, CT = CMAX / 16, kTile = contract_tile(TMAX, CMAX);
    static_assert(CMAX * TMAX <= kTile, "a wave's results go back into its own tile");
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* Yw = reinterpret_cast<float*>(smem_raw) + wave * kTile;      // [TMAX][kChLd]: the words, pixel along the row
    float* Xw = Yw + TMAX * kChLd;                                      // [CMAX][kChLd]: the channels
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool live = p < HW;                                           // a lane past the map carries zeros into the sums
    const size_t pp = live ? p : 0;
    const float* wr = wt + (size_t)b * T * HW + pp;
    const float* xr = x + (size_t)b * C * HW + pp;
    // 16 rows per trip: their loads are all in flight before the first LDS write waits for one (row by row the wave would pay a
    // dependent HBM round trip per row, with the 2 .. 3 waves per SIMD that the tiles leave room for)
#pragma unroll
    for (int r0 = 0; r0 < TMAX + CMAX; r0 += 16) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int r = r0 + j;                                       // compile-time: rows [0, TMAX) are words, the rest channels
            if (r < TMAX) v[j] = (live && r < T) ? wr[(size_t)r * HW] : 0.f;
            else v[j] = (live && r - TMAX < C) ? xr[(size_t)(r - TMAX) * HW] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) Yw[(r0 + j) * kChLd + lane] = v[j];       // Xw follows Yw: one [TMAX + CMAX][kChLd] tile
    }
    wave_lds_sync();
    const int mi = lane & 15, kq = lane >> 4;
    f32x4 acc[CT][NT];
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float av[CT], bv[NT];
#pragma unroll
        for (int i = 0; i < CT; ++i) av[i] = Xw[(16 * i + mi) * kChLd + 4 * k + kq];
#pragma unroll
        for (int n = 0; n < NT; ++n) bv[n] = Yw[(16 * n + mi) * kChLd + 4 * k + kq];
#pragma unroll
        for (int i = 0; i < CT; ++i)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[n], acc[i][n], 0, 0, 0);
    }
    wave_lds_sync();                                                    // the wave is done reading its tile: it now holds [CMAX][TMAX] results
#pragma unroll
    for (int i = 0; i < CT; ++i)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) Yw[(16 * i + 4 * kq + r) * TMAX + 16 * n + mi] = acc[i][n][r];      // D[i = 4 (l >> 4) + r][j = l & 15]
    __syncthreads();
    const float* R = reinterpret_cast<const float*>(smem_raw);
    float* dst = part + ((size_t)b * gridDim.x + blockIdx.x) * C * T;
    for (int i = threadIdx.x; i < C * T; i += 256) {
        const int c = i / T, t = i - c * T;
        const int e = c * TMAX + t;
        dst[i] = ((R[e] + R[kTile + e]) + R[2 * kTile + e]) + R[3 * kTile + e];
    }
}

// a wave per (b, c) row, a lane per word: the slabs summed in workgroup order, then the masked softmax
__global__ __launch_bounds__(256) void chan_softmax_kernel(const float* __restrict__ part, const int64_t* __restrict__ mask, float scale,
                                                           float* __restrict__ alpha, int BC, int C, int T, int nblk) {
    const int lane = threadIdx.x & 63;
    const int bc = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bc >= BC) return;                                               // wave-uniform
    const int b = bc / C, c = bc - b * C;
    const bool on = lane < T;
    float s = 0.f;
    if (on) {
        const float* p = part + (size_t)b * nblk * C * T + c * T + lane;
        for (int k = 0; k < nblk; ++k) s += p[(size_t)k * C * T];
    }
    const bool word = on && mask[(size_t)b * T + lane] != 0;
    const float m = word ? s * scale : -INFINITY;
    const float mx = wave_max(m);
    const float e = __expf(m - mx);                                     // all-masked row: exp(-inf - -inf) = NaN, like AttentionModule
    const float sum = wave_sum(e);
    if (on) alpha[(size_t)bc * T + lane] = e / sum;
}

// dms[b,c,t] = scale * alpha (dalpha - sum_t alpha dalpha), dalpha = the slabs summed in workgroup order (+ dalpha_out)
__global__ __launch_bounds__(256) void chan_softmax_bwd_kernel(const float* __restrict__ part, const float* __restrict__ alpha,
                                                               const float* __restrict__ dalpha_out, float scale,
                                                               float* __restrict__ dms, int BC, int C, int T, int nblk) {
    const int lane = threadIdx.x & 63;
    const int bc = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bc >= BC) return;                                               // wave-uniform
    const int b = bc / C, c = bc - b * C;
    const bool on = lane < T;
    float da = 0.f, a = 0.f;
    if (on) {
        const float* p = part + (size_t)b * nblk * C * T + c * T + lane;
        for (int k = 0; k < nblk; ++k) da += p[(size_t)k * C * T];
        if (dalpha_out) da += dalpha_out[(size_t)bc * T + lane];
        a = alpha[(size_t)bc * T + lane];
    }
    const float dot = wave_sum(a * da);
    if (on) dms[(size_t)bc * T + lane] = scale * (a * (da - dot));
}

// dst[c][t] (rows of TMAX floats, CMAX rows) = src[b,c,t], zero outside C x T
template <int TMAX, int CMAX>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, float* __restrict__ dst, int b, int C, int T) {
    for (int i = threadIdx.x; i < CMAX * TMAX; i += 256) {
        const int c = i / TMAX, t = i - c * TMAX;
        dst[i] = (c < C && t < T) ? src[((size_t)b * C + c) * T + t] : 0.f;
    }
}

template <int TMAX, int CMAX>
__global__ __launch_bounds__(256) void chan_read_kernel(const float* __restrict__ wt, const float* __restrict__ alpha,
                                                        float* __restrict__ f, int C, int T, int HW) {
    __shared__ float as[CMAX * TMAX];
    const int b = blockIdx.y;
    stage_rows<TMAX, CMAX>(alpha, as, b, C, T);
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float* wr = wt + (size_t)b * T * HW + p;
    float w[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) w[t] = t < T ? wr[(size_t)t * HW] : 0.f;
    float* fo = f + (size_t)b * C * HW + p;
    for (int c = 0; c < C; ++c) {
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) s += as[c * TMAX + t] * w[t];
        fo[(size_t)c * HW] = s;
    }
}

// dh[b,c,p] = sum_t dms[b,c,t] wt[b,t,p];  dwt[b,t,p] = sum_c (alpha[b,c,t] df[b,c,p] + dms[b,c,t] h[b,c,p]);  dh or dwt may be null
template <int TMAX, int CMAX>
__global__ __launch_bounds__(256) void chan_bwd_kernel(const float* __restrict__ h, const float* __restrict__ wt,
                                                       const float* __restrict__ alpha, const float* __restrict__ dms,
                                                       const float* __restrict__ df, float* __restrict__ dh, float* __restrict__ dwt,
                                                       int C, int T, int HW) {
    __shared__ float as[CMAX * TMAX];
    __shared__ float ds[CMAX * TMAX];
    const int b = blockIdx.y;
    stage_rows<TMAX, CMAX>(alpha, as, b, C, T);
    stage_rows<TMAX, CMAX>(dms, ds, b, C, T);
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const bool want_h = dh != nullptr, want_w = dwt != nullptr;         // workgroup-uniform
    const size_t c0p = (size_t)b * C * HW + p, t0p = (size_t)b * T * HW + p;
    float w[TMAX], acc[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        w[t] = (want_h && t < T) ? wt[t0p + (size_t)t * HW] : 0.f;
        acc[t] = 0.f;
    }
    for (int c0 = 0; c0 < C; c0 += kCU) {
        float hv[kCU], dv[kCU];
#pragma unroll
        for (int j = 0; j < kCU; ++j) {
            const bool on = want_w && c0 + j < C;
            hv[j] = on ? h[c0p + (size_t)(c0 + j) * HW] : 0.f;
            dv[j] = on ? df[c0p + (size_t)(c0 + j) * HW] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kCU; ++j) {
            const int c = c0 + j;
            if (c < C) {                                                // workgroup-uniform
                if (want_h) {
                    float s = 0.f;
#pragma unroll
                    for (int t = 0; t < TMAX; ++t) s += ds[c * TMAX + t] * w[t];
                    dh[c0p + (size_t)c * HW] = s;
                }
                if (want_w) {
#pragma unroll
                    for (int t = 0; t < TMAX; ++t) acc[t] += as[c * TMAX + t] * dv[j] + ds[c * TMAX + t] * hv[j];
                }
            }
        }
    }
    if (want_w) {
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
            if (t < T) dwt[t0p + (size_t)t * HW] = acc[t];
    }
}

bool shape_ok(int B, int C, int T, int HW) {
    return B > 0 && C > 0 && T > 0 && HW > 0 && C <= kMaxC && T <= kMaxT && B <= 65535 && (long long)B * C * HW < (1LL << 31) &&
           (long long)B * T * HW < (1LL << 31);
}

size_t slab_floats(int B, int C, int T, int HW) { return (size_t)B * cdiv(HW, 256) * C * T; }

void launch_contract(const float* x, const float* wt, float* part, int B, int C, int T, int HW, hipStream_t st) {
    with_tier<16, 32, 64>(T, [&](auto TM) { with_tier<16, 32, 64>(C, [&](auto CM) {
        allow_dynamic_lds<chan_contract_kernel<TM(), CM()>>((int)contract_lds(TM(), CM()));
        hipLaunchKernelGGL((chan_contract_kernel<TM(), CM()>), dim3(cdiv(HW, 256), B), dim3(256), contract_lds(TM(), CM()), st, x, wt, part,
                           C, T, HW);
    }); });
}

}  // namespace

#define CHAN_REQUIRE_SHAPE(name)                                                                                                        \
    AGAN_REQUIRE(B > 0 && C > 0 && T > 0 && HW > 0, name ": non-positive dimension");                                                 \
    AGAN_REQUIRE(C <= kMaxC, name ": nc_in %d > %d", C, kMaxC);                                                                       \
    AGAN_REQUIRE(T <= kMaxT, name ": seq_len %d > %d", T, kMaxT);                                                                     \
    AGAN_REQUIRE(shape_ok(B, C, T, HW), name ": B * nc_in * HW and B * seq_len * HW must stay below 2^31, B below 65536")

extern "C" {

size_t agan_chan_attn_fwd_ws_bytes(int B, int C, int T, int HW) {
    if (!shape_ok(B, C, T, HW)) return 0;
    return slab_floats(B, C, T, HW) * sizeof(float);                    // a score slab per workgroup
}

int agan_chan_attn_fwd(const float* h, const float* wt, const int64_t* mask, float scale, float* alpha, float* f, int B, int C, int T,
                       int HW, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(h && wt && mask && alpha && f && ws, "chan_attn_fwd: null pointer");
    CHAN_REQUIRE_SHAPE("chan_attn_fwd");
    if (int e = check_ws("chan_attn_fwd", agan_chan_attn_fwd_ws_bytes(B, C, T, HW), ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    float* part = static_cast<float*>(ws);
    const int nblk = cdiv(HW, 256);
    launch_contract(h, wt, part, B, C, T, HW, st);
    hipLaunchKernelGGL(chan_softmax_kernel, dim3(cdiv(B * C, 4)), dim3(256), 0, st, part, mask, scale, alpha, B * C, C, T, nblk);
    with_tier<16, 32, 64>(T, [&](auto TM) { with_tier<16, 32, 64>(C, [&](auto CM) {
        hipLaunchKernelGGL((chan_read_kernel<TM(), CM()>), dim3(nblk, B), dim3(256), 0, st, wt, alpha, f, C, T, HW);
    }); });
    return check_launch("chan_attn_fwd");
}

size_t agan_chan_attn_bwd_ws_bytes(int B, int C, int T, int HW) {
    if (!shape_ok(B, C, T, HW)) return 0;
    return (slab_floats(B, C, T, HW) + (size_t)B * C * T) * sizeof(float);      // a dalpha slab per workgroup, then scale * dm
}

int agan_chan_attn_bwd(const float* h, const float* wt, const float* alpha, const float* df, const float* dalpha_out, float scale,
                       float* dh, float* dwt, int B, int C, int T, int HW, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(h && wt && alpha && df && (dh || dwt) && ws, "chan_attn_bwd: null pointer");
    CHAN_REQUIRE_SHAPE("chan_attn_bwd");
    if (int e = check_ws("chan_attn_bwd", agan_chan_attn_bwd_ws_bytes(B, C, T, HW), ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    float* part = static_cast<float*>(ws);
    float* dms = part + slab_floats(B, C, T, HW);
    const int nblk = cdiv(HW, 256);
    launch_contract(df, wt, part, B, C, T, HW, st);
    hipLaunchKernelGGL(chan_softmax_bwd_kernel, dim3(cdiv(B * C, 4)), dim3(256), 0, st, part, alpha, dalpha_out, scale, dms, B * C, C, T, nblk);
    with_tier<16, 32, 64>(T, [&](auto TM) { with_tier<16, 32, 64>(C, [&](auto CM) {
        hipLaunchKernelGGL((chan_bwd_kernel<TM(), CM()>), dim3(nblk, B), dim3(256), 0, st, h, wt, alpha, dms, df, dh, dwt, C, T, HW);
    }); });
    return check_launch("chan_attn_bwd");
}

}  // extern "C"
