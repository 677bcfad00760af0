// Sentence-conditioned BatchNorm (+GLU) forward and backward: train-mode BatchNorm over (B, HW) per channel, as bn_act.hip, with the
// affine terms looked up per (sample, channel): g[b, c] = gamma[c] + delta[b, c], t[b, c] = beta[c] + delta[b, C + c], delta [B, 2C].
// fp32 storage.  The statistics are bn_act.hip's (bn_common.h: bn_train_stats); the apply passes stream x once with 16-byte accesses
// like bn_act's; the backward's reduction pass yields the per-sample sums S[b, c] = sum_p dz and Q[b, c] = sum_p dz * xhat, which ARE
// delta's gradient, and a final pass per channel adds them over b in index order -- fp64 sums, no atomics, one order.
#include "bn_common.h"

using namespace agan;

namespace {

// ---- launch log: one integer per kernel launch of the last agan_cbn_* call (agan_cbn_last_launch) ------------------------------
thread_local LaunchLog<16> g_log;
// kernel kinds of a log code (include/agan.h: agan_cbn_last_launch)
enum { kLogStatsRows = 1, kLogStatsSmall, kLogStatsTwoPass, kLogFwdApply, kLogBwdPartialWave, kLogBwdPartialBlock, kLogBwdFinal, kLogBwdApply };
inline void log_launch(int kind, int act, int width) { g_log.add(kind * 100000 + act * 10000 + width); }

// Planes (one sample's values of one channel, contiguous) of at most kWavePlane values are summed by ONE WAVE each, four planes per
// workgroup: the 8x8 .. 32x32 maps have thousands of them (24 x 512 of 64 values) and a 256-thread workgroup per plane would idle.
// Larger planes take one workgroup per chunk of a plane.
constexpr int kWavePlane = 1024;

// chunks per plane of the workgroup form: about 2048 workgroups in all (counting the B * C/2 plane pairs of GLU, whatever the
// activation, so that the workspace size needs only B, C, HW), each over at least 2048 values
inline int cbn_chunks(int B, int C, int HW) {
    if (HW <= kWavePlane) return 1;
    const long long planes = (long long)B * std::max(C / 2, 1);
    const long long nchunk = std::max<long long>(1, 2048 / planes);
    return (int)std::min<long long>(nchunk, std::max(1, HW / 2048));
}

int ew_blocks(size_t work) { return (int)std::max<size_t>(1, std::min<size_t>(cdivz(work, 256), 256 * 8)); }

// the affine map of sample row `drow` = delta + b * 2C and channel c
__device__ __forceinline__ Affine cond_affine(const float* mean, const float* invstd, const float* gamma, const float* beta,
                                              const float* drow, int C, int c) {
    return make_affine(mean[c], invstd[c], gamma[c] + drow[c], beta[c] + drow[C + c]);
}

// ---------------------------------------------------------------------------------------------------------
// forward apply
// ---------------------------------------------------------------------------------------------------------
// V: elements per thread and iteration (4 where HW is a multiple of 4: 16-byte accesses, else 1)
template <int ACT, int V>
__global__ __launch_bounds__(256) void cbn_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ delta,
                                                      float* __restrict__ out, int B, int C, int HW, float* __restrict__ amax) {
    const int Co = (ACT == AGAN_ACT_GLU) ? C / 2 : C;
    const size_t total = (size_t)B * Co * HW / V;
    float mx = 0.f;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e * V;
        const int p = (int)(i % HW);
        const size_t t = i / HW;
        const int c = (int)(t % Co), b = (int)(t / Co);
        const size_t xi = ((size_t)b * C + c) * HW + p;
        const float* drow = delta + (size_t)b * 2 * C;
        const Affine a = cond_affine(mean, invstd, gamma, beta, drow, C, c);
        float xv[V], yv[V];
        ldv<AGAN_DT_F32, V>(x, xi, xv);
        if (ACT == AGAN_ACT_GLU) {
            const Affine g = cond_affine(mean, invstd, gamma, beta, drow, C, c + Co);
            float gv[V];
            ldv<AGAN_DT_F32, V>(x, xi + (size_t)Co * HW, gv);
#pragma unroll
            for (int k = 0; k < V; ++k) yv[k] = norm_of(a, xv[k]) * sigmoid_fast(norm_of(g, gv[k]));
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) yv[k] = norm_of(a, xv[k]);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) mx = fmaxf(mx, fabsf(yv[k]));
        stv<AGAN_DT_F32, V>(out, i, yv);
    }
    if (amax) amax_commit(mx, amax);
}

// ---------------------------------------------------------------------------------------------------------
// backward: pass 1 = per-plane sums of dz and dz * xhat, pass 2 = the sums over the batch, pass 3 = dx
// ---------------------------------------------------------------------------------------------------------
// What one thread adds up over positions beg, beg + step, ... < end of plane (b, c) -- under GLU of the plane pair (c, c + C/2):
// s = {sum dz_a, sum dz_a * xhat_a, sum dz_g, sum dz_g * xhat_g} (the dz sums of V values in fp32, the running chains in fp64, as
// bn_bwd_partial_kernel keeps them).
template <int ACT, int V>
__device__ __forceinline__ void plane_sums(const float* __restrict__ x, const float* __restrict__ dout, const float* __restrict__ mean,
                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, const float* __restrict__ delta, int C, int HW, int b, int c,
                                           int beg, int end, int step, double (&s)[4]) {
    constexpr bool GLU = ACT == AGAN_ACT_GLU;
    const int Co = GLU ? C / 2 : C;
    const float* drow = delta + (size_t)b * 2 * C;
    const Affine a = cond_affine(mean, invstd, gamma, beta, drow, C, c);
    const Affine g = GLU ? cond_affine(mean, invstd, gamma, beta, drow, C, c + Co) : a;
    // xhat of the Q sums in fp64 from the stored fp32 statistics: a per-sample Q is a short sum that may cancel, and fp32 roundings of
    // (x - mean) * invstd would then show at its own scale (the passes wait on memory, the DP operations are free)
    const double ma = mean[c], ia = invstd[c];
    const double mg = GLU ? mean[c + Co] : 0.f, ig = GLU ? invstd[c + Co] : 0.f;
    const size_t xb = ((size_t)b * C + c) * HW, db = ((size_t)b * Co + c) * HW;
    s[0] = s[1] = s[2] = s[3] = 0.0;
    for (int p = beg; p < end; p += step) {
        float xa[V], xg[V], d[V];
        ldv<AGAN_DT_F32, V>(x, xb + p, xa);
        ldv<AGAN_DT_F32, V>(dout, db + p, d);
        if (GLU) ldv<AGAN_DT_F32, V>(x, xb + (size_t)Co * HW + p, xg);
        float t0 = 0.f, t2 = 0.f;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float dza, dzg;
            dz_of<ACT>(xa[k], GLU ? xg[k] : 0.f, d[k], a, g, dza, dzg);
            t0 += dza;
            s[1] += (double)dza * (((double)xa[k] - ma) * ia);
            if (GLU) {
                t2 += dzg;
                s[3] += (double)dzg * (((double)xg[k] - mg) * ig);
            }
        }
        s[0] += (double)t0;
        if (GLU) s[2] += (double)t2;
    }
}

// part[plane][chunk][4], plane = b * Cc + c with Cc = C/2 plane pairs under GLU, else C planes

// planes of HW <= kWavePlane: wave w of workgroup i sums plane 4 i + w
template <int ACT, int V>
__global__ __launch_bounds__(256) void cbn_bwd_partial_wave_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                                   const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   const float* __restrict__ delta, int B, int C, int HW,
                                                                   double* __restrict__ part) {
    const int Cc = (ACT == AGAN_ACT_GLU) ? C / 2 : C;
    const int lane = threadIdx.x & 63;
    const long long plane = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= (long long)B * Cc) return;          // (whole waves leave; the kernel has no barrier)
    const int b = (int)(plane / Cc), c = (int)(plane - (long long)b * Cc);
    double s[4];
    plane_sums<ACT, V>(x, dout, mean, invstd, gamma, beta, delta, C, HW, b, c, lane * V, HW, 64 * V, s);
    constexpr int NS = (ACT == AGAN_ACT_GLU) ? 4 : 2;
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = wave_sum_d(s[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part[(size_t)plane * 4 + k] = k < NS ? s[k] : 0.0;
    }
}

// larger planes: workgroup (plane, chunk) sums one chunk of the plane
template <int ACT, int V>
__global__ __launch_bounds__(256) void cbn_bwd_partial_block_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                                    const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    const float* __restrict__ delta, int B, int C, int HW, int nchunk,
                                                                    double* __restrict__ part) {
    __shared__ double red[4][4];
    const int Cc = (ACT == AGAN_ACT_GLU) ? C / 2 : C;
    const int plane = blockIdx.x, chunk = blockIdx.y;
    const int b = plane / Cc, c = plane - b * Cc;
    const Chunk ch = chunk_of(HW, nchunk, chunk);
    double s[4];
    plane_sums<ACT, V>(x, dout, mean, invstd, gamma, beta, delta, C, HW, b, c, ch.beg + threadIdx.x * V, ch.end, 256 * V, s);
    constexpr int NS = (ACT == AGAN_ACT_GLU) ? 4 : 2;      // (the gate half's sums stay 0 without GLU)
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = wave_sum_d(s[k]);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = s[0]; red[1][w] = s[1]; red[2][w] = s[2]; red[3][w] = s[3]; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        part[((size_t)plane * nchunk + chunk) * 4 + k] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
    }
}

// One wave per channel.  Lane l takes samples b = l, l + 64, ...: S[b, c], Q[b, c] from the chunks in chunk order -> ddelta; lane 0 then
// adds each tile of 64 samples in index order -> dgamma, dbeta and coef[c] = {sum_b g[b, c] S[b, c] / n, sum_b g[b, c] Q[b, c] / n}.
// (One THREAD per channel walking the samples itself measured 16-20 us at B = 24, C = 64: a chain of dependent loads in one wave.)
__global__ __launch_bounds__(64) void cbn_bwd_final_kernel(const double* __restrict__ part, const float* __restrict__ gamma,
                                                           const float* __restrict__ delta, int B, int C, int Cc, int nchunk, int n,
                                                           bool glu, float* __restrict__ ddelta, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, float* __restrict__ coef, int accumulate) {
    __shared__ double tile[64][4];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int pc = (glu && c >= Cc) ? c - Cc : c;
    const int off = (glu && c >= Cc) ? 2 : 0;
    const float gm = gamma[c];
    double ss = 0, sq = 0, gs = 0, gq = 0;          // (lane 0's)
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + lane;
        if (b < B) {
            const double* pp = part + ((size_t)b * Cc + pc) * nchunk * 4 + off;
            double s = 0, q = 0;
            for (int k = 0; k < nchunk; ++k) {
                s += pp[(size_t)k * 4];
                q += pp[(size_t)k * 4 + 1];
            }
            const size_t row = (size_t)b * 2 * C;
            const float g = gm + delta[row + c];
            ddelta[row + c] = (float)q;
            ddelta[row + C + c] = (float)s;
            tile[lane][0] = s;
            tile[lane][1] = q;
            tile[lane][2] = (double)g * s;
            tile[lane][3] = (double)g * q;
        }
        __syncthreads();
        if (lane == 0) {
            const int cnt = min(64, B - b0);
            for (int i = 0; i < cnt; ++i) {
                ss += tile[i][0];
                sq += tile[i][1];
                gs += tile[i][2];
                gq += tile[i][3];
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        dbeta[c] = accumulate ? dbeta[c] + (float)ss : (float)ss;
        dgamma[c] = accumulate ? dgamma[c] + (float)sq : (float)sq;
        coef[2 * c] = (float)(gs / n);
        coef[2 * c + 1] = (float)(gq / n);
    }
}

// dx = invstd[c] * (g[b, c] * dz - c0[c] - xhat * c1[c])
template <int ACT, int V>
__global__ __launch_bounds__(256) void cbn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ delta, const float* __restrict__ coef,
                                                            float* __restrict__ dx, int B, int C, int HW, float* __restrict__ amax) {
    constexpr bool GLU = ACT == AGAN_ACT_GLU;
    const int Co = GLU ? C / 2 : C;
    const size_t total = (size_t)B * Co * HW / V;
    float mx = 0.f;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e * V;
        const int p = (int)(i % HW);
        const size_t t = i / HW;
        const int c = (int)(t % Co), b = (int)(t / Co);
        const size_t xi = ((size_t)b * C + c) * HW + p;
        const float* drow = delta + (size_t)b * 2 * C;
        const Affine a = cond_affine(mean, invstd, gamma, beta, drow, C, c);
        const Affine g = GLU ? cond_affine(mean, invstd, gamma, beta, drow, C, c + Co) : a;
        const float ma = mean[c], ia = invstd[c], c0 = coef[2 * c], c1 = coef[2 * c + 1], ga = gamma[c] + drow[c];
        float mg = 0, ig = 0, g0 = 0, g1 = 0, gg = 0;
        if (GLU) { mg = mean[c + Co]; ig = invstd[c + Co]; g0 = coef[2 * (c + Co)]; g1 = coef[2 * (c + Co) + 1]; gg = gamma[c + Co] + drow[c + Co]; }
        float xa[V], xg[V], d[V], oa[V], og[V];
#pragma unroll
        for (int k = 0; k < V; ++k) xg[k] = 0.f;
        ldv<AGAN_DT_F32, V>(x, xi, xa);
        ldv<AGAN_DT_F32, V>(dout, i, d);
        if (GLU) ldv<AGAN_DT_F32, V>(x, xi + (size_t)Co * HW, xg);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float dza, dzg;
            dz_of<ACT>(xa[k], xg[k], d[k], a, g, dza, dzg);
            oa[k] = ia * (ga * dza - c0 - (xa[k] - ma) * ia * c1);
            mx = fmaxf(mx, fabsf(oa[k]));
            if (GLU) { og[k] = ig * (gg * dzg - g0 - (xg[k] - mg) * ig * g1); mx = fmaxf(mx, fabsf(og[k])); }
        }
        stv<AGAN_DT_F32, V>(dx, xi, oa);
        if (GLU) stv<AGAN_DT_F32, V>(dx, xi + (size_t)Co * HW, og);
    }
    if (amax) amax_commit(mx, amax);
}

// ---------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------
// f(Int<ACT>, Int<V>) for the two activations and the two widths (check_cbn_args has admitted act)
template <class F> void cbn_variant(int act, int HW, F&& f) {
    with_bool(act == AGAN_ACT_GLU, [&](auto G) {
        with_bool((HW & 3) == 0, [&](auto W) { f(Int<G() ? AGAN_ACT_GLU : AGAN_ACT_NONE>{}, Int<W() ? 4 : 1>{}); });
    });
}

int check_cbn_args(const char* who, bool present, int act, int B, int C, int HW) {
    AGAN_REQUIRE(present, "%s: null pointer", who);
    AGAN_REQUIRE(act == AGAN_ACT_NONE || act == AGAN_ACT_GLU, "%s: activation %d (NONE or GLU)", who, act);
    AGAN_REQUIRE(B >= 1 && C >= 1 && HW >= 1 && (long long)B * HW <= 0x7fffffffLL, "%s: B %d, C %d, HW %d", who, B, C, HW);
    AGAN_REQUIRE(act != AGAN_ACT_GLU || (C % 2 == 0), "%s: GLU needs an even channel count, got %d", who, C);
    return AGAN_OK;
}

int cbn_fwd_launch(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const float* delta,
                   float* out, int B, int C, int HW, int act, void* stream, float* out_amax) {
    const int Co = act == AGAN_ACT_GLU ? C / 2 : C;
    cbn_variant(act, HW, [&](auto A, auto V) {
        log_launch(kLogFwdApply, A(), V());
        hipLaunchKernelGGL((cbn_fwd_kernel<A(), V()>), dim3(ew_blocks((size_t)B * Co * HW / V())), dim3(256), 0, as_stream(stream), x, mean,
                           invstd, gamma, beta, delta, out, B, C, HW, out_amax);
    });
    return check_launch("cbn_act_fwd");
}

}  // namespace

extern "C" {

int agan_cbn_last_launch(int* codes, int capacity) { return g_log.copy_out(codes, capacity); }

size_t agan_cbn_train_fwd_ws_bytes(int B, int C, int HW) {
    if (B < 1 || C < 1 || HW < 1) return 0;
    return agan_bn_train_fwd_ws_bytes(B, C, HW);
}

int agan_cbn_train_fwd(const float* x, const float* gamma, const float* beta, const float* delta, float* out, float* mean, float* invstd,
                       float* running_mean, float* running_var, int64_t* nbt, int B, int C, int HW, float eps, float momentum, int act,
                       void* ws, size_t ws_bytes, void* stream, float* out_amax) {
    g_log.reset();
    if (int e = check_cbn_args("cbn_train_fwd", x && gamma && beta && delta && out && mean && invstd, act, B, C, HW)) return e;
    AGAN_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "cbn_train_fwd: running_mean/var must come together");
    if (int e = check_ws("cbn_train_fwd", agan_cbn_train_fwd_ws_bytes(B, C, HW), ws, ws_bytes)) return e;
    int form = 0, width = 0;
    if (int e = bn_train_stats(x, B, C, HW, eps, mean, invstd, running_mean, running_var, nbt, momentum, ws, ws_bytes, stream, &form, &width))
        return e;
    log_launch(form == 1 ? kLogStatsRows : form == 2 ? kLogStatsSmall : kLogStatsTwoPass, 0, width);
    return cbn_fwd_launch(x, mean, invstd, gamma, beta, delta, out, B, C, HW, act, stream, out_amax);
}

int agan_cbn_act_fwd(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const float* delta,
                     float* out, int B, int C, int HW, int act, void* stream, float* out_amax) {
    g_log.reset();
    if (int e = check_cbn_args("cbn_act_fwd", x && mean && invstd && gamma && beta && delta && out, act, B, C, HW)) return e;
    return cbn_fwd_launch(x, mean, invstd, gamma, beta, delta, out, B, C, HW, act, stream, out_amax);
}

size_t agan_cbn_act_bwd_ws_bytes(int B, int C, int HW) {
    if (B < 1 || C < 1 || HW < 1) return 0;
    return (size_t)B * C * cbn_chunks(B, C, HW) * 4 * sizeof(double) + (size_t)C * 2 * sizeof(float) + 64;
}

int agan_cbn_act_bwd(const float* x, const float* dout, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     const float* delta, float* dx, float* ddelta, float* dgamma, float* dbeta, int B, int C, int HW, int act,
                     int accumulate, void* ws, size_t ws_bytes, void* stream, float* dx_amax) {
    g_log.reset();
    if (int e = check_cbn_args("cbn_act_bwd", x && dout && mean && invstd && gamma && beta && delta && dx && ddelta && dgamma && dbeta && ws,
                               act, B, C, HW))
        return e;
    if (int e = check_ws("cbn_act_bwd", agan_cbn_act_bwd_ws_bytes(B, C, HW), ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    const bool glu = act == AGAN_ACT_GLU;
    const int Cc = glu ? C / 2 : C;
    const int nchunk = cbn_chunks(B, C, HW);
    const long long planes = (long long)B * Cc;
    AGAN_REQUIRE(planes <= 0x7fffffffLL, "cbn_act_bwd: %lld planes", planes);
    double* part = static_cast<double*>(ws);
    float* coef = reinterpret_cast<float*>(part + (size_t)planes * nchunk * 4);
    cbn_variant(act, HW, [&](auto A, auto V) {
        if (HW <= kWavePlane) {
            log_launch(kLogBwdPartialWave, A(), V());
            hipLaunchKernelGGL((cbn_bwd_partial_wave_kernel<A(), V()>), dim3((unsigned)((planes + 3) / 4)), dim3(256), 0, st, x, dout, mean,
                               invstd, gamma, beta, delta, B, C, HW, part);
        } else {
            log_launch(kLogBwdPartialBlock, A(), V());
            hipLaunchKernelGGL((cbn_bwd_partial_block_kernel<A(), V()>), dim3((unsigned)planes, nchunk), dim3(256), 0, st, x, dout, mean,
                               invstd, gamma, beta, delta, B, C, HW, nchunk, part);
        }
    });
    log_launch(kLogBwdFinal, act, 1);
    hipLaunchKernelGGL(cbn_bwd_final_kernel, dim3(C), dim3(64), 0, st, part, gamma, delta, B, C, Cc, nchunk, B * HW, glu, ddelta,
                       dgamma, dbeta, coef, accumulate);
    cbn_variant(act, HW, [&](auto A, auto V) {
        log_launch(kLogBwdApply, A(), V());
        hipLaunchKernelGGL((cbn_bwd_apply_kernel<A(), V()>), dim3(ew_blocks((size_t)B * Cc * HW / V())), dim3(256), 0, st, x, dout, mean,
                           invstd, gamma, beta, delta, coef, dx, B, C, HW, dx_amax);
    });
    return check_launch("cbn_act_bwd");
}

}  // extern "C"
