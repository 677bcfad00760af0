// The join of the text-conditional discriminator head (include/agan.h: agan_cond_join_fwd / agan_cond_join_bwd;
// backend/functional.py: cond_join, cond_join_reference; networks/discriminators.py: COND_DNET).
//
// AttnGAN's jointConv is a 3x3 conv over cat(h, rep(s)) on the 4x4 code.  The sentence channels are constant over the map, so
//     conv3x3(cat(h, rep(s)), W)[n, c, i, j] = conv3x3(h, W[:, :8df])[n, c, i, j] + sum_{t valid at (i, j)} P[n, c, t]
//     P[n, c, t] = sum_e s[n, e] * W[c, 8df + e, t]
// with t = 3 (di + 1) + (dj + 1) the tap that reads input (i + di, j + dj), valid iff that position is inside the 4x4 map.  The image
// term comes from the library's conv, P from its linear; this file adds the two, and transposes the addition.
//
// Work mapping: one lane owns one (row, channel): 64 contiguous bytes of yi / y (four 16-byte accesses) and 36 contiguous bytes of p;
// neighbouring lanes own neighbouring channels, so a wave covers 4 KB of yi and 2.3 KB of p without gaps.  No LDS.  Every sum has one
// order (written at each loop), no atomics: two runs give the same bits.
#include "agan_common.h"

using namespace agan;

namespace {

constexpr int kThreads = 256;

// tap t = 3 * (di + 1) + (dj + 1) reads input (i + di, j + dj): inside the 4x4 map?
__device__ __forceinline__ bool tap_valid(int t, int i, int j) {
    const int ii = i + t / 3 - 1, jj = j + t % 3 - 1;
    return ii >= 0 && ii < 4 && jj >= 0 && jj < 4;
}

// y[n] = yi[src(n)] + S(p[cap(n)]), taps added in ascending t starting from yi.
// rows n < k * B: src = n, cap = n mod B; wrong rows k * B + b: src = b (the FIRST group's image term), cap = (b + 1) mod B
__global__ __launch_bounds__(kThreads) void cond_join_fwd_kernel(const float* __restrict__ yi, const float* __restrict__ p,
                                                                 float* __restrict__ y, int B, int k, int C, int rows) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= rows * C) return;
    const int n = idx / C, c = idx - n * C;
    const int src = n < k * B ? n : n - k * B;
    const int cap = n < k * B ? n % B : (n - k * B + 1) % B;
    float v[16], q[9];
    const float4* in = reinterpret_cast<const float4*>(yi + ((size_t)src * C + c) * 16);
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<float4*>(v + 4 * r) = in[r];
    const float* pp = p + ((size_t)cap * C + c) * 9;
#pragma unroll
    for (int t = 0; t < 9; ++t) q[t] = pp[t];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 9; ++t)
                if (tap_valid(t, i, j)) v[4 * i + j] += q[t];
    float4* out = reinterpret_cast<float4*>(y + (size_t)idx * 16);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = *reinterpret_cast<const float4*>(v + 4 * r);
}

// lane (n < k * B, c):  dyi[n] = dy[n] (+ dy[k * B + n] for n < B when wrong).
// lanes n < B also own dp[n, c, :]: over the rows that used caption n -- row n of group 0, 1, ..., then wrong row (n - 1 + B) mod B --
// and inside a row over the positions (i, j) in ascending order, every tap valid there takes dy: ONE running sum per tap.
__global__ __launch_bounds__(kThreads) void cond_join_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dyi,
                                                                 float* __restrict__ dp, int B, int k, int C, int wrong) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= k * B * C) return;
    const int n = idx / C, c = idx - n * C;
    if (dyi) {
        float v[16];
        const float4* a = reinterpret_cast<const float4*>(dy + (size_t)idx * 16);
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<float4*>(v + 4 * r) = a[r];
        if (wrong && n < B) {
            const float4* w = reinterpret_cast<const float4*>(dy + ((size_t)(k * B + n) * C + c) * 16);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float4 u = w[r];
                v[4 * r] += u.x, v[4 * r + 1] += u.y, v[4 * r + 2] += u.z, v[4 * r + 3] += u.w;
            }
        }
        float4* out = reinterpret_cast<float4*>(dyi + (size_t)idx * 16);
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r] = *reinterpret_cast<const float4*>(v + 4 * r);
    }
    if (dp && n < B) {
        float acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = 0.f;
        const int users = k + (wrong ? 1 : 0);
        for (int g = 0; g < users; ++g) {
            const int row = g < k ? g * B + n : k * B + (n - 1 + B) % B;
            float v[16];
            const float4* a = reinterpret_cast<const float4*>(dy + ((size_t)row * C + c) * 16);
#pragma unroll
            for (int r = 0; r < 4; ++r) *reinterpret_cast<float4*>(v + 4 * r) = a[r];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int t = 0; t < 9; ++t)
                        if (tap_valid(t, i, j)) acc[t] += v[4 * i + j];
        }
        float* out = dp + (size_t)idx * 9;              // (n < B: idx = n * C + c)
#pragma unroll
        for (int t = 0; t < 9; ++t) out[t] = acc[t];
    }
}

// lanes (rows * C) must fit an int with room for the grid arithmetic; element offsets are size_t
bool sizes_ok(int B, int k, int C, int wrong) {
    return B >= 1 && k >= 1 && C >= 1 && (long long)(k + 1) * B * C <= (1ll << 30) && !(wrong && B < 2);
}
bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }          // (a null pointer passes)

}  // namespace

extern "C" {

int agan_cond_join_fwd(const float* yi, const float* p, float* y, int B, int k, int C, int wrong, void* stream) {
    AGAN_REQUIRE(yi && p && y, "cond_join_fwd: null pointer");
    AGAN_REQUIRE(sizes_ok(B, k, C, wrong), "cond_join_fwd: B %d, k %d, C %d, wrong %d (B, k, C >= 1; wrong needs B >= 2)", B, k, C, wrong);
    AGAN_REQUIRE(aligned16(yi) && aligned16(y), "cond_join_fwd: yi and y must be 16-byte aligned");
    const int rows = (k + (wrong ? 1 : 0)) * B;
    hipLaunchKernelGGL(cond_join_fwd_kernel, dim3(cdiv(rows * C, kThreads)), dim3(kThreads), 0, as_stream(stream), yi, p, y, B, k, C, rows);
    return check_launch("cond_join_fwd");
}

int agan_cond_join_bwd(const float* dy, float* dyi, float* dp, int B, int k, int C, int wrong, void* stream) {
    AGAN_REQUIRE(dy, "cond_join_bwd: null pointer");
    AGAN_REQUIRE(sizes_ok(B, k, C, wrong), "cond_join_bwd: B %d, k %d, C %d, wrong %d (B, k, C >= 1; wrong needs B >= 2)", B, k, C, wrong);
    AGAN_REQUIRE(aligned16(dy) && aligned16(dyi), "cond_join_bwd: dy and dyi must be 16-byte aligned");
    if (!dyi && !dp) return AGAN_OK;
    const int lanes = (dyi ? k : 1) * B * C;            // dp alone needs the first group's lanes only
    hipLaunchKernelGGL(cond_join_bwd_kernel, dim3(cdiv(lanes, kThreads)), dim3(kThreads), 0, as_stream(stream), dy, dyi, dp, B, k, C,
                       wrong ? 1 : 0);
    return check_launch("cond_join_bwd");
}

}  // extern "C"
