// Differentiable augmentation of discriminator inputs (include/agan.h: agan_diffaug_fwd / agan_diffaug_bwd; augment.py states the
// transform in torch ops).
//
// Per sample the map x -> y is   colour (brightness, saturation, contrast)  ->  translation with zero fill  ->  cutout,   linear in x
// for fixed uniforms u, and the backward is its transpose.  Both directions are the same two launches:
//   1. sum:    the per-sample sum the colour stage needs -- forward: of x (M = mean(x) + b, because saturation keeps every pixel's
//              channel mean); backward: of the gathered gradient g, taken over the positions of dy that survive translation and
//              cutout.  A sample is cut into P <= 64 chunks, one workgroup each; threads add in fp64, the wave and the workgroup
//              combine in a fixed order, and the P partials land in the workspace.  Skipped without the COLOR bit.
//   2. apply:  a thread owns V = 4 pixels side by side (1 where a row is not whole 16-byte chunks) in ALL C channels, because
//              saturation mixes the channels of a pixel.  It adds its sample's partials in chunk order (every workgroup of a sample
//              repeats the same P additions: same bits), gathers, applies the colour map or its transpose and stores 16 bytes per
//              lane and channel.
// The translated source row starts tx floats off the 16-byte grid.  tx is one number per sample and a workgroup lies inside one
// sample, so the misalignment r = (x - tx) & 3 is wave-uniform: a lane loads the two ALIGNED float4 that cover its four sources and
// a uniform switch on r picks them out of the eight registers (no LDS, no unaligned access; the second float4 is the neighbour
// lane's first and comes from L1).
//
// Colour arithmetic, forward:  v = x + b;  m = mean_C(v);  w = fma(s, v, (1 - s) m);  z = fma(c, w, (1 - c) M)   -- the issue's
// s (v - m) + m and c (w - M) + M regrouped so that s = 1 and c = 1 are the identity bit for bit.  Backward:  dw = fma(c, g, (1 - c) G),
// dx = fma(s, dw, (1 - s) mean_C(dw)).  No atomics, no allocation, no synchronisation; the workspace is written before it is read.
//
// The gated entries (agan_diffaug_gated_*) are the same kernels with GATED = true: a sample's policy is the call's policy with the bit
// of every stage k cleared whose uniform q[n][k] is not below *p (three scalar loads and compares per workgroup -- a workgroup lies
// inside one sample, so the gate is wave-uniform).  Whatever the ungated kernels decide from the policy, these decide from that
// per-sample mask: the sum workgroups of a sample without colour return before loading, and its apply workgroups never touch the partials.
#include <algorithm>

#include "agan_common.h"
#include "dispatch.h"

namespace {
using namespace agan;

constexpr int kThreads = 256;
constexpr int kMaxPartials = 64;       // most chunks (= partial sums) per sample
constexpr int kChunk = 4096;           // fewest elements per chunk

struct Geom {
    int C, H, W, HW, E;                // E = C * H * W elements per sample
    int Sy, Sx;                        // largest shift
    int ch, cw;                        // cutout size
    int policy;
    int P, chunk;                      // chunks per sample, elements per chunk (a multiple of 4)
};

struct Sample {
    int ty, tx;                        // out[y][x] = z[y - ty][x - tx]
    int cy0, cy1, cx0, cx1;            // cut rows / columns, clipped to the image (empty without the bit)
    float b, s, c;
};

__device__ __forceinline__ int offset_of(float u, int count, int top) { return min(max((int)(u * (float)count), 0), top); }

// the pointers of the gated entries (unused, and null, where GATED is false)
struct Gate {
    const float* q;                    // [N, 4] uniforms
    const float* p;                    // one fp32, device memory
};

// sample n's own policy: the stages whose bit is set AND whose uniform lies below *p (fp32 compare; false for a NaN)
template <bool GATED>
__device__ __forceinline__ int policy_of(const Geom& g, const Gate& gate, int n) {
    if constexpr (!GATED) return g.policy;
    else {
        const float p = *gate.p;
        const float* qn = gate.q + (size_t)n * 4;
        int pol = 0;
        if (qn[0] < p) pol |= AGAN_DIFFAUG_COLOR;
        if (qn[1] < p) pol |= AGAN_DIFFAUG_TRANSLATION;
        if (qn[2] < p) pol |= AGAN_DIFFAUG_CUTOUT;
        return pol & g.policy;
    }
}

__device__ __forceinline__ Sample sample_of(const Geom& g, const float* __restrict__ u, int n, int policy) {
    const float* un = u + (size_t)n * 8;
    Sample p;
    p.ty = p.tx = 0;
    p.cy0 = p.cy1 = p.cx0 = p.cx1 = 0;
    p.b = 0.f, p.s = 1.f, p.c = 1.f;
    if (policy & AGAN_DIFFAUG_COLOR) {
        p.b = un[0] - 0.5f;
        p.s = 2.f * un[1];
        p.c = un[2] + 0.5f;
    }
    if (policy & AGAN_DIFFAUG_TRANSLATION) {
        p.ty = offset_of(un[3], 2 * g.Sy + 1, 2 * g.Sy) - g.Sy;
        p.tx = offset_of(un[4], 2 * g.Sx + 1, 2 * g.Sx) - g.Sx;
    }
    if (policy & AGAN_DIFFAUG_CUTOUT) {
        const int oy = offset_of(un[5], g.H + 1 - g.ch % 2, g.H - g.ch % 2);
        const int ox = offset_of(un[6], g.W + 1 - g.cw % 2, g.W - g.cw % 2);
        p.cy0 = max(0, oy - g.ch / 2), p.cy1 = min(g.H, oy - g.ch / 2 + g.ch);
        p.cx0 = max(0, ox - g.cw / 2), p.cx1 = min(g.W, ox - g.cw / 2 + g.cw);
    }
    return p;
}

__device__ __forceinline__ bool in_cut(const Sample& p, int y, int x) { return y >= p.cy0 && y < p.cy1 && x >= p.cx0 && x < p.cx1; }

// does OUTPUT position (y, x) of the forward keep a value: its source lies inside the image and the position is not cut
__device__ __forceinline__ bool kept(const Geom& g, const Sample& p, int y, int x) {
    return (unsigned)(y - p.ty) < (unsigned)g.H && (unsigned)(x - p.tx) < (unsigned)g.W && !in_cut(p, y, x);
}

__device__ __forceinline__ const float* sample_ptr(const float* x0, const float* x1, int n0, int n, int E) {
    return n < n0 ? x0 + (size_t)n * E : x1 + (size_t)(n - n0) * E;
}

// partial[n * P + chunk] = fp64 sum of the chunk's elements; `masked`: only the positions the forward keeps (the backward's sum of g)
// (GATED: a sample whose colour gate is off needs no sum -- its workgroups leave at once and write nothing)
template <bool VEC, bool GATED>
__global__ __launch_bounds__(kThreads) void sum_kernel(const float* __restrict__ x0, const float* __restrict__ x1, int n0,
                                                       const float* __restrict__ u, const Geom g, int masked,
                                                       double* __restrict__ partial, const Gate gate) {
    __shared__ double red[kThreads / kWave];
    const int n = blockIdx.x / g.P, blk = blockIdx.x % g.P;
    const int policy = policy_of<GATED>(g, gate, n);
    if (GATED && !(policy & AGAN_DIFFAUG_COLOR)) return;
    const float* __restrict__ src = sample_ptr(x0, x1, n0, n, g.E);
    const int lo = min(g.E, blk * g.chunk);                            // (blk * chunk < E + 4 P: no overflow)
    const int cnt = min(g.chunk, g.E - lo);
    Sample p;
    if (masked) p = sample_of(g, u, n, policy);
    double acc = 0.0;
    if (VEC) {                                                          // E, chunk, lo and cnt are multiples of 4, and so is W
        for (int k = 4 * (int)threadIdx.x; k < cnt; k += 4 * kThreads) {
            const int i = lo + k;
            float4 q = *reinterpret_cast<const float4*>(src + i);
            if (masked) {
                const int r = i % g.HW, y = r / g.W, x = r % g.W;
                if (!kept(g, p, y, x)) q.x = 0.f;
                if (!kept(g, p, y, x + 1)) q.y = 0.f;
                if (!kept(g, p, y, x + 2)) q.z = 0.f;
                if (!kept(g, p, y, x + 3)) q.w = 0.f;
            }
            acc += (double)q.x;
            acc += (double)q.y;
            acc += (double)q.z;
            acc += (double)q.w;
        }
    } else {
        for (int k = threadIdx.x; k < cnt; k += kThreads) {
            const int i = lo + k;
            float v = src[i];
            if (masked) {
                const int r = i % g.HW;
                if (!kept(g, p, r / g.W, r % g.W)) v = 0.f;
            }
            acc += (double)v;
        }
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kThreads / kWave; ++w) s += red[w];
        partial[blockIdx.x] = s;
    }
}

// V pixels side by side in all C channels per thread.  Forward: out = y, sources (x0, x1); backward: out = dx, source x0 = dy.
template <int C, int V, bool BWD, bool GATED>
__global__ __launch_bounds__(kThreads) void apply_kernel(const float* __restrict__ x0, const float* __restrict__ x1, int n0,
                                                         const float* __restrict__ u, const Geom g, const double* __restrict__ partial,
                                                         float* __restrict__ out, int blocks_per_sample, const Gate gate) {
    __shared__ double s_part[kMaxPartials];
    __shared__ float s_mean;
    const int t = threadIdx.x;
    const int n = blockIdx.x / blocks_per_sample, blk = blockIdx.x % blocks_per_sample;
    const int policy = policy_of<GATED>(g, gate, n);
    const Sample p = sample_of(g, u, n, policy);
    const bool color = (policy & AGAN_DIFFAUG_COLOR) != 0;            // (workgroup-uniform: the barriers below are safe)
    float mean = 0.f;                                                   // forward: M = mean(x) + b; backward: G = mean(g)
    if (color) {
        if (t < g.P) s_part[t] = partial[(size_t)n * g.P + t];
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int i = 0; i < g.P; ++i) s += s_part[i];
            s /= (double)g.E;
            s_mean = (float)(BWD ? s : s + (double)p.b);
        }
        __syncthreads();
        mean = s_mean;
    }
    const int upr = g.W / V;                                            // units per row
    const int unit = blk * kThreads + t;
    if (unit >= g.H * upr) return;
    const int y = unit / upr, x = (unit % upr) * V;
    // the value at (y, x) comes from (y - ty, x - tx) going forward and from (y + ty, x + tx) going back
    const int sy = BWD ? y + p.ty : y - p.ty;
    const int sx = BWD ? x + p.tx : x - p.tx;
    const bool row_ok = (unsigned)sy < (unsigned)g.H;
    const float* __restrict__ src = sample_ptr(x0, x1, n0, n, g.E);

    float v[C][V];
    bool ok[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int sxj = sx + j;
        // the cut is a rectangle of forward OUTPUT positions: (y, x + j) going forward, the source position going back
        ok[j] = row_ok && (unsigned)sxj < (unsigned)g.W && !(BWD ? in_cut(p, sy, sxj) : in_cut(p, y, x + j));
    }
    if constexpr (V == 4) {
        const int a = sx & ~3, r = sx & 3;                              // (two's complement: floors a negative sx as well)
        float e[C][8];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
            if (row_ok) {
                const float* row = src + ((size_t)c * g.H + sy) * g.W;
                if (a >= 0 && a < g.W) q0 = *reinterpret_cast<const float4*>(row + a);
                if (r != 0 && a + 4 >= 0 && a + 4 < g.W) q1 = *reinterpret_cast<const float4*>(row + a + 4);
            }
            e[c][0] = q0.x, e[c][1] = q0.y, e[c][2] = q0.z, e[c][3] = q0.w;
            e[c][4] = q1.x, e[c][5] = q1.y, e[c][6] = q1.z, e[c][7] = q1.w;
        }
        switch (r) {                                                    // wave-uniform: one tx per sample, x a multiple of 4
#define AGAN_PICK(R)                                      \
    _Pragma("unroll") for (int c = 0; c < C; ++c)         \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) v[c][j] = e[c][R + j];
            case 0: AGAN_PICK(0) break;
            case 1: AGAN_PICK(1) break;
            case 2: AGAN_PICK(2) break;
            default: AGAN_PICK(3) break;
#undef AGAN_PICK
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][0] = ok[0] ? src[((size_t)c * g.H + sy) * g.W + sx] : 0.f;
    }

    constexpr float inv_c = 1.0f / (float)C;
    const float s1 = 1.f - p.s, c1 = (1.f - p.c) * mean;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if (!color) {
#pragma unroll
            for (int c = 0; c < C; ++c) v[c][j] = ok[j] ? v[c][j] : 0.f;
        } else if (!BWD) {
            float m = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                v[c][j] += p.b;
                m += v[c][j];
            }
            m = s1 * (m * inv_c);
#pragma unroll
            for (int c = 0; c < C; ++c) v[c][j] = ok[j] ? fmaf(p.c, fmaf(p.s, v[c][j], m), c1) : 0.f;
        } else {
            float m = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                v[c][j] = fmaf(p.c, ok[j] ? v[c][j] : 0.f, c1);
                m += v[c][j];
            }
            m = s1 * (m * inv_c);
#pragma unroll
            for (int c = 0; c < C; ++c) v[c][j] = fmaf(p.s, v[c][j], m);
        }
    }
    float* __restrict__ dst = out + (size_t)n * g.E + (size_t)y * g.W + x;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if constexpr (V == 4) *reinterpret_cast<float4*>(dst + (size_t)c * g.HW) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        else dst[(size_t)c * g.HW] = v[c][0];
    }
}

bool in_domain(long long N, int C, int H, int W) {
    const long long lim = 1ll << 31;                                    // (factor by factor: the full product may not fit 64 bits)
    return N >= 1 && N < lim && C >= 1 && C <= 4 && H >= 1 && W >= 1 && (long long)H * W < lim && (long long)H * W * C < lim &&
           (long long)H * W * C * N < lim;
}

Geom geom_of(int C, int H, int W, int policy) {
    Geom g;
    g.C = C, g.H = H, g.W = W, g.HW = H * W, g.E = C * H * W;
    g.Sy = (int)(0.125 * H + 0.5), g.Sx = (int)(0.125 * W + 0.5);
    g.ch = (int)(0.5 * H + 0.5), g.cw = (int)(0.5 * W + 0.5);
    g.policy = policy;
    g.P = std::min(kMaxPartials, cdiv(g.E, kChunk));
    g.chunk = (cdiv(g.E, g.P) + 3) & ~3;
    return g;
}

size_t ws_bytes_of(long long N, const Geom& g) { return up16((size_t)N * g.P * sizeof(double)); }

template <int V, bool BWD, bool GATED>
void launch_apply(const Geom& g, unsigned blocks, hipStream_t st, const float* x0, const float* x1, int n0, const float* u,
                  const double* partial, float* out, int bps, const Gate& gate) {
    const auto launch = [&](auto CC) {
        hipLaunchKernelGGL((apply_kernel<CC(), V, BWD, GATED>), dim3(blocks), dim3(kThreads), 0, st, x0, x1, n0, u, g, partial, out, bps,
                           gate);
    };
    if (!with_int<1, 2, 3>(g.C, launch)) launch(Int<4>{});
}

// gate == nullptr: the ungated entries
template <bool BWD>
int run(const char* what, const float* x0, const float* x1, int n0, int n1, const float* u, const Gate* gate, int policy, float* out, int C,
        int H, int W, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(n0 >= 1 && n1 >= 0 && H >= 1 && W >= 1, "%s: bad shape (N %d + %d, C %d, H %d, W %d)", what, n0, n1, C, H, W);
    AGAN_REQUIRE(C >= 1 && C <= 4, "%s: C %d outside 1..4", what, C);
    AGAN_REQUIRE(policy >= 0 && policy <= 7, "%s: policy %d outside 0..7", what, policy);
    const long long N = (long long)n0 + n1;
    AGAN_REQUIRE(in_domain(N, C, H, W), "%s: N * C * H * W is 2^31 or more (N %lld, C %d, H %d, W %d)", what, N, C, H, W);
    AGAN_REQUIRE(x0 && u && out && (n1 == 0 || x1), "%s: null pointer", what);
    AGAN_REQUIRE(!gate || (gate->q && gate->p), "%s: null q or p", what);
    const Geom g = geom_of(C, H, W, policy);
    const size_t need = ws_bytes_of(N, g);
    AGAN_REQUIRE(ws, "%s: no workspace (agan_diffaug_ws_bytes: %zu bytes)", what, need);
    if (int e = check_ws(what, need, ws, ws_bytes)) return e;
    double* partial = static_cast<double*>(ws);
    hipStream_t st = as_stream(stream);
    // 16-byte accesses need rows of whole float4s and aligned bases (checked, not assumed); a sample's offset is then aligned too
    uintptr_t bases = reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(out);
    if (n1) bases |= reinterpret_cast<uintptr_t>(x1);
    const bool vec = W % 4 == 0 && bases % 16 == 0;
    const int bps = cdiv(vec ? g.HW / 4 : g.HW, kThreads);
    const Gate gt = gate ? *gate : Gate{nullptr, nullptr};
    with_bool(gate != nullptr, [&](auto GATED) {
        with_bool(vec, [&](auto VEC) {
            if (policy & AGAN_DIFFAUG_COLOR)
                hipLaunchKernelGGL((sum_kernel<VEC(), GATED()>), dim3((unsigned)(N * g.P)), dim3(kThreads), 0, st, x0, x1, n0, u, g,
                                   BWD ? 1 : 0, partial, gt);
            launch_apply<VEC() ? 4 : 1, BWD, GATED()>(g, (unsigned)(N * bps), st, x0, x1, n0, u, partial, out, bps, gt);
        });
    });
    return check_launch(what);
}

}  // namespace

extern "C" size_t agan_diffaug_ws_bytes(int N, int C, int H, int W) {
    return in_domain(N, C, H, W) ? ws_bytes_of(N, geom_of(C, H, W, 0)) : 0;
}

extern "C" int agan_diffaug_fwd(const float* x0, const float* x1, int n0, int n1, const float* u, int policy, float* y, int C, int H, int W,
                                void* ws, size_t ws_bytes, void* stream) {
    return run<false>("diffaug_fwd", x0, x1, n0, x1 ? n1 : 0, u, nullptr, policy, y, C, H, W, ws, ws_bytes, stream);
}

extern "C" int agan_diffaug_bwd(const float* dy, const float* u, int policy, float* dx, int N, int C, int H, int W, void* ws,
                                size_t ws_bytes, void* stream) {
    return run<true>("diffaug_bwd", dy, nullptr, N, 0, u, nullptr, policy, dx, C, H, W, ws, ws_bytes, stream);
}

extern "C" int agan_diffaug_gated_fwd(const float* x0, const float* x1, int n0, int n1, const float* u, const float* q, const float* p,
                                      int policy, float* y, int C, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    const Gate gate{q, p};
    return run<false>("diffaug_gated_fwd", x0, x1, n0, x1 ? n1 : 0, u, &gate, policy, y, C, H, W, ws, ws_bytes, stream);
}

extern "C" int agan_diffaug_gated_bwd(const float* dy, const float* u, const float* q, const float* p, int policy, float* dx, int N, int C,
                                      int H, int W, void* ws, size_t ws_bytes, void* stream) {
    const Gate gate{q, p};
    return run<true>("diffaug_gated_bwd", dy, nullptr, N, 0, u, &gate, policy, dx, C, H, W, ws, ws_bytes, stream);
}
