// Pools and bilinear resize of the frozen Inception-v3 image-encoder trunk (reference networks/cnn_encoder.py:75-101; torchvision's
// inception_v3 layer order), forward and backward, NCHW fp32.  One thread per output element in the forwards, one per input element
// in the backwards: every backward is a gather that sums the outputs reading its pixel in a fixed order (no atomics, run-to-run
// identical).  Optional relu_mask / accumulate on every backward (include/agan.h).
#include "agan_common.h"

using namespace agan;

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float masked_store(float v, const float* __restrict__ relu_mask, float* __restrict__ dx, size_t i, int accumulate) {
    if (relu_mask && !(relu_mask[i] > 0.f)) v = 0.f;
    if (accumulate) v += dx[i];
    dx[i] = v;
    return v;
}

// ---- max pool 3x3 stride 2, no padding ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void maxpool3s2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ am,
                                                                 int B, int C, int H, int W, int OH, int OW, int out_c0, int out_ctot) {
    const size_t n = (size_t)B * C * OH * OW;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const size_t bc = i / ((size_t)OH * OW);
    const int c = (int)(bc % C), b = (int)(bc / C);
    const float* src = x + bc * H * W + (size_t)(2 * oy) * W + 2 * ox;
    float m = -__builtin_inff();
    int arg = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float v = src[(t / 3) * W + t % 3];
        if (v > m || v != v) {          // torch's rule: strictly greater, or NaN
            m = v;
            arg = t;
        }
    }
    y[((size_t)b * out_ctot + out_c0 + c) * OH * OW + (size_t)oy * OW + ox] = m;
    am[i] = (uint8_t)arg;
}

__global__ __launch_bounds__(kThreads) void maxpool3s2_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ am,
                                                                 const float* __restrict__ relu_mask, float* __restrict__ dx, int B, int C,
                                                                 int H, int W, int OH, int OW, int out_c0, int out_ctot, int accumulate) {
    const size_t n = (size_t)B * C * H * W;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int ix = (int)(i % W), iy = (int)((i / W) % H);
    const size_t bc = i / ((size_t)H * W);
    const int c = (int)(bc % C), b = (int)(bc / C);
    const float* g = dy + ((size_t)b * out_ctot + out_c0 + c) * OH * OW;
    const uint8_t* a = am + bc * OH * OW;
    // windows oy with 2*oy <= iy <= 2*oy + 2, ascending oy then ox
    const int oy0 = iy >= 2 ? (iy - 1) >> 1 : 0, oy1 = min(iy >> 1, OH - 1);
    const int ox0 = ix >= 2 ? (ix - 1) >> 1 : 0, ox1 = min(ix >> 1, OW - 1);
    float s = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
            const int t = (iy - 2 * oy) * 3 + (ix - 2 * ox);
            if (a[(size_t)oy * OW + ox] == t) s += g[(size_t)oy * OW + ox];
        }
    masked_store(s, relu_mask, dx, i, accumulate);
}

// ---- avg pool 3x3 stride 1, padding 1, count_include_pad (/9) --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void avgpool3s1_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, int H, int W) {
    const size_t n = (size_t)B * C * H * W;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int ox = (int)(i % W), oy = (int)((i / W) % H);
    const float* src = x + (i / ((size_t)H * W)) * H * W;
    float s = 0.f;
    for (int yy = max(oy - 1, 0); yy <= min(oy + 1, H - 1); ++yy)
        for (int xx = max(ox - 1, 0); xx <= min(ox + 1, W - 1); ++xx) s += src[(size_t)yy * W + xx];
    y[i] = s / 9.f;
}

__global__ __launch_bounds__(kThreads) void avgpool3s1_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ relu_mask,
                                                                 float* __restrict__ dx, int B, int C, int H, int W, int accumulate) {
    const size_t n = (size_t)B * C * H * W;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int ix = (int)(i % W), iy = (int)((i / W) % H);
    const float* g = dy + (i / ((size_t)H * W)) * H * W;
    float s = 0.f;
    for (int yy = max(iy - 1, 0); yy <= min(iy + 1, H - 1); ++yy)
        for (int xx = max(ix - 1, 0); xx <= min(ix + 1, W - 1); ++xx) s += g[(size_t)yy * W + xx];
    masked_store(s / 9.f, relu_mask, dx, i, accumulate);
}

// ---- global average pool: one wave per (b, c), fixed-order lane partials then a fixed tree --------------------------------------
__global__ __launch_bounds__(64) void global_avgpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int HW) {
    const float* src = x + (size_t)blockIdx.x * HW;
    float s = 0.f;
    for (int j = threadIdx.x; j < HW; j += 64) s += src[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) y[blockIdx.x] = s / (float)HW;
}

__global__ __launch_bounds__(kThreads) void global_avgpool_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ relu_mask,
                                                                     float* __restrict__ dx, size_t n, int HW, int accumulate) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    masked_store(dy[i / HW] / (float)HW, relu_mask, dx, i, accumulate);
}

// ---- bilinear resize, align_corners=False ---------------------------------------------------------------------------------------
struct Src {
    int i0, i1;
    float l0, l1;
};
// src = (o + 0.5) * in / out - 0.5 = ((2o + 1) * in - out) / (2 * out), clamped at 0: integer part and remainder exactly, so the weights
// carry one rounding (torch's fp32 kernel rounds in / out first and loses ~log2(in) bits of the fraction; the fp64 rule is what this
// matches)
__device__ __forceinline__ Src src_index(int o, int in, int out) {
    const int num = max((2 * o + 1) * in - out, 0), den = 2 * out;
    Src r;
    r.i0 = min(num / den, in - 1);
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = (float)(num - r.i0 * den) / (float)den;
    r.l0 = 1.f - r.l1;
    return r;
}

__global__ __launch_bounds__(kThreads) void resize_bilinear_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, int IH,
                                                                      int IW, int OH, int OW) {
    const size_t n = (size_t)B * C * OH * OW;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const float* src = x + (i / ((size_t)OH * OW)) * IH * IW;
    const Src ry = src_index(oy, IH, OH), rx = src_index(ox, IW, OW);
    const float* r0 = src + (size_t)ry.i0 * IW;
    const float* r1 = src + (size_t)ry.i1 * IW;
    y[i] = ry.l0 * (rx.l0 * r0[rx.i0] + rx.l1 * r0[rx.i1]) + ry.l1 * (rx.l0 * r1[rx.i0] + rx.l1 * r1[rx.i1]);
}

// weight of input index `in_i` in output `o` along one axis (0 if it is neither neighbour; both if they coincide at the edge)
__device__ __forceinline__ float axis_weight(int o, int in_i, int in, int out) {
    const Src r = src_index(o, in, out);
    return (r.i0 == in_i ? r.l0 : 0.f) + (r.i1 == in_i ? r.l1 : 0.f);
}

// outputs whose source interval can touch input index i: a superset of [first o with i1(o) >= i, last o with i0(o) <= i]
__device__ __forceinline__ void out_range(int i, int in, int out, int& lo, int& hi) {
    const float r = (float)out / (float)in;
    lo = max(0, (int)floorf((i - 1 + 0.5f) * r - 0.5f) - 2);
    hi = min(out - 1, (int)ceilf((i + 1 + 0.5f) * r - 0.5f) + 2);
}

__global__ __launch_bounds__(kThreads) void resize_bilinear_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int C, int IH,
                                                                      int IW, int OH, int OW) {
    const size_t n = (size_t)B * C * IH * IW;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int ix = (int)(i % IW), iy = (int)((i / IW) % IH);
    const float* g = dy + (i / ((size_t)IH * IW)) * OH * OW;
    int ylo, yhi, xlo, xhi;
    out_range(iy, IH, OH, ylo, yhi);
    out_range(ix, IW, OW, xlo, xhi);
    float s = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = axis_weight(oy, iy, IH, OH);
        if (wy == 0.f) continue;
        float t = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            const float wx = axis_weight(ox, ix, IW, OW);
            if (wx != 0.f) t += wx * g[(size_t)oy * OW + ox];
        }
        s += wy * t;
    }
    dx[i] = s;
}

__global__ __launch_bounds__(kThreads) void relu_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx,
                                                           size_t n, int accumulate) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    masked_store(dy[i], y, dx, i, accumulate);
}

unsigned blocks_for(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" {

int agan_maxpool3s2_fwd(const float* x, float* y, uint8_t* argmax, int B, int C, int H, int W, int out_c0, int out_ctot, void* stream) {
    AGAN_REQUIRE(x && y && argmax, "maxpool3s2_fwd: null pointer");
    AGAN_REQUIRE(B > 0 && C > 0 && H >= 3 && W >= 3 && out_c0 >= 0 && out_c0 + C <= out_ctot, "maxpool3s2_fwd: bad shape");
    const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
    const size_t n = (size_t)B * C * OH * OW;
    hipLaunchKernelGGL(maxpool3s2_fwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), x, y, argmax, B, C, H, W, OH, OW, out_c0,
                out_ctot);
    return check_launch("maxpool3s2_fwd");
}

int agan_maxpool3s2_bwd(const float* dy, const uint8_t* argmax, const float* relu_mask, float* dx, int B, int C, int H, int W, int out_c0,
                        int out_ctot, int accumulate, void* stream) {
    AGAN_REQUIRE(dy && argmax && dx, "maxpool3s2_bwd: null pointer");
    AGAN_REQUIRE(B > 0 && C > 0 && H >= 3 && W >= 3 && out_c0 >= 0 && out_c0 + C <= out_ctot, "maxpool3s2_bwd: bad shape");
    const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
    const size_t n = (size_t)B * C * H * W;
    hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), dy, argmax, relu_mask, dx, B, C, H, W, OH, OW,
                out_c0, out_ctot, accumulate);
    return check_launch("maxpool3s2_bwd");
}

int agan_avgpool3s1_fwd(const float* x, float* y, int B, int C, int H, int W, void* stream) {
    AGAN_REQUIRE(x && y && B > 0 && C > 0 && H > 0 && W > 0, "avgpool3s1_fwd: bad argument");
    const size_t n = (size_t)B * C * H * W;
    hipLaunchKernelGGL(avgpool3s1_fwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), x, y, B, C, H, W);
    return check_launch("avgpool3s1_fwd");
}

int agan_avgpool3s1_bwd(const float* dy, const float* relu_mask, float* dx, int B, int C, int H, int W, int accumulate, void* stream) {
    AGAN_REQUIRE(dy && dx && B > 0 && C > 0 && H > 0 && W > 0, "avgpool3s1_bwd: bad argument");
    const size_t n = (size_t)B * C * H * W;
    hipLaunchKernelGGL(avgpool3s1_bwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), dy, relu_mask, dx, B, C, H, W, accumulate);
    return check_launch("avgpool3s1_bwd");
}

int agan_global_avgpool_fwd(const float* x, float* y, int B, int C, int HW, void* stream) {
    AGAN_REQUIRE(x && y && B > 0 && C > 0 && HW > 0, "global_avgpool_fwd: bad argument");
    hipLaunchKernelGGL(global_avgpool_fwd_kernel, dim3((unsigned)(B * C)), dim3(64), 0, as_stream(stream), x, y, HW);
    return check_launch("global_avgpool_fwd");
}

int agan_global_avgpool_bwd(const float* dy, const float* relu_mask, float* dx, int B, int C, int HW, int accumulate, void* stream) {
    AGAN_REQUIRE(dy && dx && B > 0 && C > 0 && HW > 0, "global_avgpool_bwd: bad argument");
    const size_t n = (size_t)B * C * HW;
    hipLaunchKernelGGL(global_avgpool_bwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), dy, relu_mask, dx, n, HW, accumulate);
    return check_launch("global_avgpool_bwd");
}

int agan_resize_bilinear_fwd(const float* x, float* y, int B, int C, int IH, int IW, int OH, int OW, void* stream) {
    AGAN_REQUIRE(x && y && B > 0 && C > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0, "resize_bilinear_fwd: bad argument");
    const size_t n = (size_t)B * C * OH * OW;
    hipLaunchKernelGGL(resize_bilinear_fwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), x, y, B, C, IH, IW, OH, OW);
    return check_launch("resize_bilinear_fwd");
}

int agan_resize_bilinear_bwd(const float* dy, float* dx, int B, int C, int IH, int IW, int OH, int OW, void* stream) {
    AGAN_REQUIRE(dy && dx && B > 0 && C > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0, "resize_bilinear_bwd: bad argument");
    const size_t n = (size_t)B * C * IH * IW;
    hipLaunchKernelGGL(resize_bilinear_bwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), dy, dx, B, C, IH, IW, OH, OW);
    return check_launch("resize_bilinear_bwd");
}

int agan_relu_bwd(const float* y, const float* dy, float* dx, size_t n, int accumulate, void* stream) {
    AGAN_REQUIRE(y && dy && dx && n > 0, "relu_bwd: bad argument");
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), y, dy, dx, n, accumulate);
    return check_launch("relu_bwd");
}

}  // extern "C"
