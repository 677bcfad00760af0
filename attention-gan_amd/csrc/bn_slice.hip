// Train-mode BatchNorm + ReLU of the Inception-v3 trunk (CNNEncoder(backend="hip", hip_train=True)): the BatchNorm of one conv whose
// output feeds a CHANNEL SLICE of a block output.  The forward reads the contiguous raw conv output x [B, C, HW] and writes
// relu(BN(x)) into channels [out_c0, out_c0 + C) of a [B, out_ctot, HW] tensor; the backward reads dy from such a slice and writes a
// contiguous dx.  No activation in the backward (the trunk's backward masks every gradient of a ReLU output when it writes it) and no
// gamma / beta gradients (the trunk is frozen).  Per-channel sums in fp64 in a fixed order, no atomics: run-to-run identical.
//
// Two size regimes, as in bn_act.hip: n = B*HW <= kSmallN (the 17x17 and 8x8 layers at B = 24) is ONE launch, a workgroup per channel
// holding the channel's values in registers between the statistics and the apply; larger channels are agan_bn_stats (partial sums +
// final, the library's statistics kernels) followed by a plane-wise apply.
#include "bn_common.h"

using namespace agan;

namespace {

// ---- forward ------------------------------------------------------------------------------------------------------------------
// one workgroup per channel; PER values per thread (n <= 256 * PER)
template <int PER>
__global__ __launch_bounds__(kThreads) void bn_relu_slice_small_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, float* __restrict__ out, int out_c0,
                                                                       int out_ctot, float* __restrict__ mean, float* __restrict__ invstd,
                                                                       float* __restrict__ rmean, float* __restrict__ rvar,
                                                                       int64_t* __restrict__ nbt, int B, int C, int HW, float eps,
                                                                       float momentum) {
    __shared__ double red[2][4];
    const int c = blockIdx.x, n = B * HW;
    if (c == 0 && threadIdx.x == 0 && nbt) *nbt += 1;
    float v[PER];
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = threadIdx.x + j * kThreads;
        v[j] = 0.f;
        if (i < n) {
            const int b = i / HW, p = i - b * HW;
            v[j] = x[((size_t)b * C + c) * HW + p];
            s += v[j];
            q += (double)v[j] * v[j];
        }
    }
    block_sum2(s, q, red);
    const BnStats st = bn_finish_channel(s, q, n, eps, momentum, c, threadIdx.x == 0, mean, invstd, rmean, rvar);
    const float mf = st.mean, is = st.invstd;
    const float sc = gamma[c] * is, bc = beta[c];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = threadIdx.x + j * kThreads;
        if (i < n) {
            const int b = i / HW, p = i - b * HW;
            const float z = (v[j] - mf) * sc + bc;
            out[((size_t)b * out_ctot + out_c0 + c) * HW + p] = z > 0.f ? z : 0.f;
        }
    }
}

// one workgroup per (b, c) plane: relu(gamma*(x-mean)*invstd + beta) into the slice
__global__ __launch_bounds__(kThreads) void bn_relu_slice_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                                       const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, float* __restrict__ out, int out_c0,
                                                                       int out_ctot, int C, int HW) {
    const int plane = blockIdx.x, b = plane / C, c = plane - b * C;
    const float m = mean[c], sc = gamma[c] * invstd[c], bc = beta[c];
    const float* xp = x + (size_t)plane * HW;
    float* op = out + ((size_t)b * out_ctot + out_c0 + c) * HW;
    for (int p = threadIdx.x; p < HW; p += kThreads) {
        const float z = (xp[p] - m) * sc + bc;
        op[p] = z > 0.f ? z : 0.f;
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// dx = gamma*invstd * (dy - mean(dy) - xhat * mean(dy * xhat)),  xhat = (x - mean) * invstd
template <int PER>
__global__ __launch_bounds__(kThreads) void bn_slice_small_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                                      int dout_c0, int dout_ctot, const float* __restrict__ mean,
                                                                      const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                      float* __restrict__ dx, int B, int C, int HW) {
    __shared__ double red[2][4];
    const int c = blockIdx.x, n = B * HW;
    const float m = mean[c], is = invstd[c];
    float xh[PER], d[PER];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = threadIdx.x + j * kThreads;
        xh[j] = 0.f;
        d[j] = 0.f;
        if (i < n) {
            const int b = i / HW, p = i - b * HW;
            xh[j] = (x[((size_t)b * C + c) * HW + p] - m) * is;
            d[j] = dout[((size_t)b * dout_ctot + dout_c0 + c) * HW + p];
            s0 += d[j];
            s1 += (double)d[j] * xh[j];
        }
    }
    block_sum2(s0, s1, red);
    const float c0 = (float)(s0 / n), c1 = (float)(s1 / n), sc = gamma[c] * is;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = threadIdx.x + j * kThreads;
        if (i < n) {
            const int b = i / HW, p = i - b * HW;
            dx[((size_t)b * C + c) * HW + p] = sc * (d[j] - c0 - xh[j] * c1);
        }
    }
}

// pass 1 of the large path: part[c][chunk] = {sum dy, sum dy*xhat} over the chunk's share of channel c's n = B*HW values
__global__ __launch_bounds__(kThreads) void bn_slice_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                                        int dout_c0, int dout_ctot, const float* __restrict__ mean,
                                                                        const float* __restrict__ invstd, int B, int C, int HW,
                                                                        int nchunk, double* __restrict__ part) {
    __shared__ double red[2][4];
    const int c = blockIdx.x, chunk = blockIdx.y, n = B * HW;
    const int len = cdiv(n, nchunk);
    const int beg = min(n, chunk * len), end = min(n, beg + len);
    const float m = mean[c], is = invstd[c];
    double s0 = 0.0, s1 = 0.0;
    for (int i = beg + threadIdx.x; i < end; i += kThreads) {
        const int b = i / HW, p = i - b * HW;
        const float xh = (x[((size_t)b * C + c) * HW + p] - m) * is;
        const float d = dout[((size_t)b * dout_ctot + dout_c0 + c) * HW + p];
        s0 += d;
        s1 += (double)d * xh;
    }
    block_sum2(s0, s1, red);
    if (threadIdx.x == 0) {
        part[((size_t)c * nchunk + chunk) * 2 + 0] = s0;
        part[((size_t)c * nchunk + chunk) * 2 + 1] = s1;
    }
}

// pass 2: coef[c] = {mean dy, mean dy*xhat}, the chunks added in index order
__global__ __launch_bounds__(kThreads) void bn_slice_bwd_final_kernel(const double* __restrict__ part, int C, int nchunk, int n,
                                                                      float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        s0 += part[((size_t)c * nchunk + k) * 2 + 0];
        s1 += part[((size_t)c * nchunk + k) * 2 + 1];
    }
    coef[2 * c] = (float)(s0 / n);
    coef[2 * c + 1] = (float)(s1 / n);
}

// pass 3: one workgroup per (b, c) plane
__global__ __launch_bounds__(kThreads) void bn_slice_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                                      int dout_c0, int dout_ctot, const float* __restrict__ mean,
                                                                      const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                      const float* __restrict__ coef, float* __restrict__ dx, int C, int HW) {
    const int plane = blockIdx.x, b = plane / C, c = plane - b * C;
    const float m = mean[c], is = invstd[c], sc = gamma[c] * is, c0 = coef[2 * c], c1 = coef[2 * c + 1];
    const float* xp = x + (size_t)plane * HW;
    const float* dp = dout + ((size_t)b * dout_ctot + dout_c0 + c) * HW;
    float* op = dx + (size_t)plane * HW;
    for (int p = threadIdx.x; p < HW; p += kThreads) {
        const float xh = (xp[p] - m) * is;
        op[p] = sc * (dp[p] - c0 - xh * c1);
    }
}

bool small_path(int B, int HW) { return (long long)B * HW <= kSmallN; }

bool slice_ok(int B, int C, int HW, int c0, int ctot) {
    return B > 0 && C > 0 && HW > 0 && c0 >= 0 && ctot > 0 && (long long)c0 + C <= ctot;
}

}  // namespace

extern "C" {

size_t agan_bn_relu_slice_fwd_ws_bytes(int B, int C, int HW) {
    if (B <= 0 || C <= 0 || HW <= 0 || small_path(B, HW)) return 0;
    return agan_bn_stats_ws_bytes(B, C, HW);
}

int agan_bn_relu_slice_fwd(const float* x, const float* gamma, const float* beta, float* out, int out_c0, int out_ctot, float* mean,
                           float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, int B, int C, int HW,
                           float eps, float momentum, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(x && gamma && beta && out && mean && invstd, "bn_relu_slice_fwd: null pointer");
    AGAN_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_relu_slice_fwd: running_mean/var must come together");
    AGAN_REQUIRE(slice_ok(B, C, HW, out_c0, out_ctot), "bn_relu_slice_fwd: bad sizes B=%d C=%d HW=%d, channels [%d, %d) of %d", B, C, HW,
                 out_c0, out_c0 + C, out_ctot);
    hipStream_t st = as_stream(stream);
    if (small_path(B, HW)) {
        with_per(B * HW, [&](auto P) {
            hipLaunchKernelGGL((bn_relu_slice_small_kernel<P()>), dim3(C), dim3(kThreads), 0, st, x, gamma, beta, out, out_c0, out_ctot, mean,
                               invstd, running_mean, running_var, num_batches_tracked, B, C, HW, eps, momentum);
        });
        return check_launch("bn_relu_slice_fwd/small");
    }
    if (!ws) {
        set_error("bn_relu_slice_fwd: no workspace");
        return AGAN_EWORKSPACE;
    }
    if (int e = check_ws("bn_relu_slice_fwd", agan_bn_relu_slice_fwd_ws_bytes(B, C, HW), ws, ws_bytes)) return e;
    if (int e = agan_bn_stats(x, B, C, HW, eps, mean, invstd, running_mean, running_var, num_batches_tracked, momentum, ws, ws_bytes,
                              stream))
        return e;
    hipLaunchKernelGGL(bn_relu_slice_apply_kernel, dim3((unsigned)B * C), dim3(kThreads), 0, st, x, mean, invstd, gamma, beta, out, out_c0,
                       out_ctot, C, HW);
    return check_launch("bn_relu_slice_fwd");
}

size_t agan_bn_slice_bwd_ws_bytes(int B, int C, int HW) {
    if (B <= 0 || C <= 0 || HW <= 0 || small_path(B, HW)) return 0;
    return (size_t)C * bn_chunks(B, C, HW) * 2 * sizeof(double) + (size_t)C * 2 * sizeof(float);
}

int agan_bn_slice_bwd(const float* x, const float* dout, int dout_c0, int dout_ctot, const float* mean, const float* invstd,
                      const float* gamma, float* dx, int B, int C, int HW, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(x && dout && mean && invstd && gamma && dx, "bn_slice_bwd: null pointer");
    AGAN_REQUIRE(slice_ok(B, C, HW, dout_c0, dout_ctot), "bn_slice_bwd: bad sizes B=%d C=%d HW=%d, channels [%d, %d) of %d", B, C, HW,
                 dout_c0, dout_c0 + C, dout_ctot);
    hipStream_t st = as_stream(stream);
    if (small_path(B, HW)) {
        with_per(B * HW, [&](auto P) {
            hipLaunchKernelGGL((bn_slice_small_bwd_kernel<P()>), dim3(C), dim3(kThreads), 0, st, x, dout, dout_c0, dout_ctot, mean, invstd,
                               gamma, dx, B, C, HW);
        });
        return check_launch("bn_slice_bwd/small");
    }
    if (!ws) {
        set_error("bn_slice_bwd: no workspace");
        return AGAN_EWORKSPACE;
    }
    if (int e = check_ws("bn_slice_bwd", agan_bn_slice_bwd_ws_bytes(B, C, HW), ws, ws_bytes)) return e;
    const int nchunk = bn_chunks(B, C, HW);
    double* part = static_cast<double*>(ws);
    float* coef = reinterpret_cast<float*>(part + (size_t)C * nchunk * 2);
    hipLaunchKernelGGL(bn_slice_bwd_partial_kernel, dim3(C, nchunk), dim3(kThreads), 0, st, x, dout, dout_c0, dout_ctot, mean, invstd, B, C,
                       HW, nchunk, part);
    hipLaunchKernelGGL(bn_slice_bwd_final_kernel, dim3(cdiv(C, kThreads)), dim3(kThreads), 0, st, part, C, nchunk, B * HW, coef);
    hipLaunchKernelGGL(bn_slice_bwd_apply_kernel, dim3((unsigned)B * C), dim3(kThreads), 0, st, x, dout, dout_c0, dout_ctot, mean, invstd,
                       gamma, coef, dx, C, HW);
    return check_launch("bn_slice_bwd");
}

}  // extern "C"
