// Geometric augmentation of discriminator inputs (include/agan.h: agan_geoaug_matrix / agan_affine_warp_fwd / agan_affine_warp_bwd;
// augment.py states all three in torch ops).
//
//   matrix:  one thread per sample builds the sample's output -> source map (a, b, 0, c, d, 0) from its sixteen uniforms, the stage
//            mask and -- with a p -- the per-stage gates, the way ada.hip's update works: device memory in, device memory out, so a
//            captured HIP graph follows a p that the controller moves between replays.
//   forward: a bilinear gather.  A thread owns V = 4 output pixels side by side (1 where a row is not whole 16-byte chunks) in ALL C
//            channels: the coordinates, floors and weights of a pixel are computed once and serve every channel.  The four taps are
//            dword gathers: under a rotation the sources of a lane's neighbours lie along a slanted line, so nothing wider is
//            aligned.  What a gather instruction costs is the number of cache lines its 64 addresses touch, so a wave owns a BLOCK of
//            outputs, 8 lanes by 8 rows (32 x 8 pixels at V = 4), not a run of one row: turned by any angle the block's sources
//            span at most 33 rows (25 on average) where a 256-pixel run spans up to 181, an unturned block still reads and
//            writes whole 128-byte lines, and the four waves of a workgroup make a 16 V x 16 tile whose taps the CU's vector cache
//            serves about four times each.  (Measured on MI355X at [48, 3, 256, 256], all five stages: 0.167 ms with a wave on a
//            run of one row, profiles/geoaug_micro.txt has the block's figure.)
//   backward: the exact transpose, as a GATHER over dy.  A thread owns one input pixel (j, i) in all C channels; workgroups are 32 x 8
//            tiles of input pixels, so that the candidates of a tile are a compact patch of dy.  The outputs whose taps can touch the
//            pixel have their source inside the open 2 x 2 square around it; the preimage of that square under the map is a
//            parallelogram around  o = ctr + L^-1 ((j, i) - t)  whose bounding box has the half-extents
//                ex = |inv00| + |inv01|,   ey = |inv10| + |inv11|        (inv = L^-1; the square's half-width is 1).
//            The thread walks the integers of [o - e, o + e] padded by one on every side, (floor(2 e) + 3) per axis, the same count
//            for every thread of a sample.  For EVERY candidate it recomputes the forward's source coordinates, floors and fractions
//            with the forward's own function (source_of), and adds dy * weight where one of the four taps is (j, i), in row-major
//            candidate order.  Membership is decided by the forward's own bits, so the box only has to be a superset (the padding
//            absorbs the rounding of inv and o); the sum has one order; there are no atomics.
//            The box for the stages of agan_geoaug_matrix: L is a product of a reflection / rotations (orthogonal), s I and
//            diag(r, 1 / r) with s, r in [2^-0.35, 2^0.35], so every singular value of L^-1 lies in [2^-0.7, 2^0.7] and a row of
//            inv has 1-norm <= sqrt(2) * 2^0.7 = 2.30: at most floor(4.6) + 3 = 7 candidates per axis, 5 for a pure flip or quarter
//            turn.  For caller-supplied matrices each extent is clamped at 32 (67 candidates per axis): the backward is specified
//            for linear parts that shrink no axis below 1/16, and no matrix can make a launch run away.
// Every dy / x load is guarded by its own bounds check, so no matrix -- singular, huge, NaN -- makes an address leave the tensor.
// Coordinate arithmetic is written without contraction, operation by operation as include/agan.h states it: the fp32 torch
// restatement then computes the same bits, and forward and backward cannot disagree about a floor.
#include "agan_common.h"
#include "dispatch.h"

namespace {
using namespace agan;

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 8;     // the backward's tile of input pixels (kTileW * kTileH == kThreads)
constexpr int kFwdLanesX = 16, kFwdRows = 16;   // the forward's tile: 16 lanes of V pixels by 16 rows (kFwdLanesX * kFwdRows == kThreads)
constexpr float kMaxExtent = 32.f;

struct Shape {
    int C, H, W, HW, E;
    float cx, cy;                          // (W - 1) / 2, (H - 1) / 2
};

// a sample's map: source = (a, b; c, d) (o - ctr) + (t0x, t0y),   t0x = tx W + cx, t0y = ty H + cy
struct Affine {
    float a, b, c, d, t0x, t0y;
};

struct Source {
    int x0, y0;                            // floor of the source position, clamped to [-2, W] / [-2, H] (anything outside has no tap inside)
    float fx, fy;
};

__device__ __forceinline__ Affine affine_of(const float* __restrict__ M, int n, const Shape& s) {
#pragma clang fp contract(off)
    const float* m = M + (size_t)n * 6;
    Affine A;
    A.a = m[0], A.b = m[1], A.c = m[3], A.d = m[4];
    A.t0x = m[2] * (float)s.W + s.cx;
    A.t0y = m[5] * (float)s.H + s.cy;
    return A;
}

// THE coordinate function of both directions
__device__ __forceinline__ Source source_of(const Affine& A, const Shape& s, int ox, int oy) {
#pragma clang fp contract(off)
    const float dx = (float)ox - s.cx, dy = (float)oy - s.cy;
    const float sx = (A.a * dx + A.b * dy) + A.t0x;
    const float sy = (A.c * dx + A.d * dy) + A.t0y;
    const float x0 = floorf(sx), y0 = floorf(sy);
    Source r;
    r.fx = sx - x0, r.fy = sy - y0;
    // (the clamp is taken in float: a huge or NaN coordinate becomes -2, which no tap test accepts)
    r.x0 = (int)fminf(fmaxf(x0, -2.f), (float)s.W);
    r.y0 = (int)fminf(fmaxf(y0, -2.f), (float)s.H);
    return r;
}

__device__ __forceinline__ const float* sample_ptr(const float* x0, const float* x1, int n0, int n, int E) {
    return n < n0 ? x0 + (size_t)n * E : x1 + (size_t)(n - n0) * E;
}

template <int C, int V>
__global__ __launch_bounds__(kThreads) void warp_fwd_kernel(const float* __restrict__ x0, const float* __restrict__ x1, int n0,
                                                            const float* __restrict__ M, const Shape s, float* __restrict__ out,
                                                            int tiles_x, int tiles_per_sample) {
#pragma clang fp contract(off)
    const int n = blockIdx.x / tiles_per_sample, tile = blockIdx.x % tiles_per_sample;
    const Affine A = affine_of(M, n, s);
    // a workgroup is 2 x 2 waves, a wave 8 lanes x 8 rows, a lane V pixels of one row: a 16 V x 16 tile of outputs
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int ox = (tile % tiles_x) * (kFwdLanesX * V) + ((wave & 1) * 8 + (lane & 7)) * V;
    const int oy = (tile / tiles_x) * kFwdRows + (wave >> 1) * 8 + (lane >> 3);
    if (ox >= s.W || oy >= s.H) return;                                 // (W is a multiple of V: a lane's pixels are all inside or all outside)
    const float* __restrict__ src = sample_ptr(x0, x1, n0, n, s.E);

    float v[C][V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const Source p = source_of(A, s, ox + j, oy);
        const float wx[2] = {1.f - p.fx, p.fx}, wy[2] = {1.f - p.fy, p.fy};
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][j] = 0.f;
#pragma unroll
        for (int ty = 0; ty < 2; ++ty) {
#pragma unroll
            for (int tx = 0; tx < 2; ++tx) {
                const int yy = p.y0 + ty, xx = p.x0 + tx;
                if ((unsigned)yy < (unsigned)s.H && (unsigned)xx < (unsigned)s.W) {
                    const float w = wy[ty] * wx[tx];
                    const float* tap = src + (size_t)yy * s.W + xx;
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c][j] = v[c][j] + tap[(size_t)c * s.HW] * w;
                }
            }
        }
    }
    float* __restrict__ dst = out + (size_t)n * s.E + (size_t)oy * s.W + ox;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if constexpr (V == 4) *reinterpret_cast<float4*>(dst + (size_t)c * s.HW) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        else dst[(size_t)c * s.HW] = v[c][0];
    }
}

template <int C>
__global__ __launch_bounds__(kThreads) void warp_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ M, const Shape s,
                                                            float* __restrict__ dx, int tiles_x, int tiles_per_sample) {
#pragma clang fp contract(off)
    const int n = blockIdx.x / tiles_per_sample, tile = blockIdx.x % tiles_per_sample;
    const Affine A = affine_of(M, n, s);
    // the inverse of the linear part and the box's half-extents: the same numbers in every thread of the sample
    const float det = A.a * A.d - A.b * A.c;
    const float i00 = A.d / det, i01 = -A.b / det, i10 = -A.c / det, i11 = A.a / det;
    const float ex = fminf(fabsf(i00) + fabsf(i01), kMaxExtent), ey = fminf(fabsf(i10) + fabsf(i11), kMaxExtent);   // (fminf: a NaN becomes 32)
    const int nx = (int)floorf(2.f * ex) + 3, ny = (int)floorf(2.f * ey) + 3;

    const int j = (tile % tiles_x) * kTileW + (int)(threadIdx.x % kTileW);
    const int i = (tile / tiles_x) * kTileH + (int)(threadIdx.x / kTileW);
    if (j >= s.W || i >= s.H) return;
    // the output position whose source is (j, i); clamped in float so that the int below is defined for any matrix
    const float px = (float)j - A.t0x, py = (float)i - A.t0y;
    const float ocx = fminf(fmaxf((i00 * px + i01 * py) + s.cx, -1.0e9f), 1.0e9f);
    const float ocy = fminf(fmaxf((i10 * px + i11 * py) + s.cy, -1.0e9f), 1.0e9f);
    const int lox = (int)ceilf(ocx - ex) - 1, loy = (int)ceilf(ocy - ey) - 1;

    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    const float* __restrict__ g = dy + (size_t)n * s.E;
    for (int ky = 0; ky < ny; ++ky) {
        const int oy = loy + ky;
        if ((unsigned)oy >= (unsigned)s.H) continue;
        for (int kx = 0; kx < nx; ++kx) {
            const int ox = lox + kx;
            if ((unsigned)ox >= (unsigned)s.W) continue;
            const Source p = source_of(A, s, ox, oy);
            const int tx = j - p.x0, ty = i - p.y0;                    // which of the candidate's taps this pixel is, if any
            if ((unsigned)tx < 2u && (unsigned)ty < 2u) {
                const float w = (ty ? p.fy : 1.f - p.fy) * (tx ? p.fx : 1.f - p.fx);
                const float* q = g + (size_t)oy * s.W + ox;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = acc[c] + q[(size_t)c * s.HW] * w;
            }
        }
    }
    float* __restrict__ dst = dx + (size_t)n * s.E + (size_t)i * s.W + j;
#pragma unroll
    for (int c = 0; c < C; ++c) dst[(size_t)c * s.HW] = acc[c];
}

// L <- L S for the stages that apply, left to right; (c, s) of a quarter turn come from a table, never from trig
__global__ __launch_bounds__(kThreads) void matrix_kernel(const float* __restrict__ g, const float* __restrict__ p, int geometry,
                                                          float* __restrict__ M, int n) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kThreads + (int)threadIdx.x;
    if (i >= n) return;
    const float* gi = g + (size_t)i * AGAN_GEOAUG_UNIFORMS;
    int on = geometry;
    if (p) {                                                            // stage k passes iff g[8 + k] < *p (false for a NaN p)
        const float pv = *p;
        on = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (gi[8 + k] < pv) on |= 1 << k;
        on &= geometry;
    }
    float a = 1.f, b = 0.f, c = 0.f, d = 1.f;
    const auto mul = [&](float s00, float s01, float s10, float s11) {
        const float na = a * s00 + b * s10, nb = a * s01 + b * s11, nc = c * s00 + d * s10, nd = c * s01 + d * s11;
        a = na, b = nb, c = nc, d = nd;
    };
    if ((on & AGAN_GEOAUG_XFLIP) && gi[0] >= 0.5f) mul(-1.f, 0.f, 0.f, 1.f);
    if (on & AGAN_GEOAUG_ROT90) {
        const int k = min((int)(4.f * gi[1]), 3);
        const float co = k == 0 ? 1.f : k == 2 ? -1.f : 0.f, si = k == 1 ? 1.f : k == 3 ? -1.f : 0.f;
        mul(co, -si, si, co);
    }
    if (on & AGAN_GEOAUG_SCALE) {
        const float s = exp2f(0.7f * gi[2] - 0.35f);
        mul(s, 0.f, 0.f, s);
    }
    if (on & AGAN_GEOAUG_ROTATE) {
        const float th = (2.f * gi[3] - 1.f) * 3.14159265358979323846f;
        float si, co;
        sincosf(th, &si, &co);
        mul(co, -si, si, co);
    }
    if (on & AGAN_GEOAUG_ANISO) {
        const float r = exp2f(0.7f * gi[4] - 0.35f);
        mul(r, 0.f, 0.f, 1.f / r);
    }
    float* m = M + (size_t)i * 6;
    m[0] = a, m[1] = b, m[2] = 0.f, m[3] = c, m[4] = d, m[5] = 0.f;
}

bool in_domain(long long N, int C, int H, int W) {
    const long long lim = 1ll << 31;                                    // (factor by factor: the full product may not fit 64 bits)
    return N >= 1 && N < lim && C >= 1 && C <= 4 && H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24) && (long long)H * W < lim &&
           (long long)H * W * C < lim && (long long)H * W * C * N < lim;
}

Shape shape_of(int C, int H, int W) {
    Shape s;
    s.C = C, s.H = H, s.W = W, s.HW = H * W, s.E = C * H * W;
    s.cx = (float)(W - 1) * 0.5f, s.cy = (float)(H - 1) * 0.5f;        // (exact: W - 1 < 2^24)
    return s;
}

int check_shape(const char* what, long long N, int C, int H, int W) {
    AGAN_REQUIRE(C >= 1 && C <= 4, "%s: C %d outside 1..4", what, C);
    AGAN_REQUIRE(in_domain(N, C, H, W), "%s: a size above 2^24 or N * C * H * W of 2^31 or more (N %lld, C %d, H %d, W %d)", what, N, C, H, W);
    return AGAN_OK;
}

}  // namespace

extern "C" int agan_geoaug_matrix(const float* g, const float* p, int geometry, float* M, int n, void* stream) {
    AGAN_REQUIRE(g && M, "geoaug_matrix: null pointer");
    AGAN_REQUIRE(n >= 1, "geoaug_matrix: %d samples", n);
    AGAN_REQUIRE(geometry >= 0 && geometry <= AGAN_GEOAUG_ALL, "geoaug_matrix: geometry %d outside 0..%d", geometry, AGAN_GEOAUG_ALL);
    hipLaunchKernelGGL(matrix_kernel, dim3((unsigned)cdiv(n, kThreads)), dim3(kThreads), 0, as_stream(stream), g, p, geometry, M, n);
    return check_launch("geoaug_matrix");
}

extern "C" int agan_affine_warp_fwd(const float* x0, const float* x1, int n0, int n1, const float* M, float* y, int C, int H, int W,
                                    void* stream) {
    const char* what = "affine_warp_fwd";
    if (!x1) n1 = 0;
    AGAN_REQUIRE(n0 >= 1 && n1 >= 0 && H >= 1 && W >= 1, "%s: bad shape (N %d + %d, C %d, H %d, W %d)", what, n0, n1, C, H, W);
    const long long N = (long long)n0 + n1;
    if (int e = check_shape(what, N, C, H, W)) return e;
    AGAN_REQUIRE(x0 && M && y, "%s: null pointer", what);
    const Shape s = shape_of(C, H, W);
    // 16-byte stores need rows of whole float4s and an aligned base (checked, not assumed); the taps are dwords either way
    const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0;
    const int tiles_x = cdiv(W, kFwdLanesX * (vec ? 4 : 1));
    const long long tps = (long long)tiles_x * cdiv(H, kFwdRows);
    AGAN_REQUIRE(tps * N < (1ll << 31), "%s: too many tiles (N %lld, H %d, W %d)", what, N, H, W);
    const unsigned blocks = (unsigned)(tps * N);
    hipStream_t st = as_stream(stream);
    with_bool(vec, [&](auto VEC) {
        const auto launch = [&](auto CC) {
            hipLaunchKernelGGL((warp_fwd_kernel<CC(), VEC() ? 4 : 1>), dim3(blocks), dim3(kThreads), 0, st, x0, x1, n0, M, s, y, tiles_x,
                               (int)tps);
        };
        if (!with_int<1, 2, 3>(C, launch)) launch(Int<4>{});
    });
    return check_launch(what);
}

extern "C" int agan_affine_warp_bwd(const float* dy, const float* M, float* dx, int N, int C, int H, int W, void* stream) {
    const char* what = "affine_warp_bwd";
    AGAN_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: bad shape (N %d, C %d, H %d, W %d)", what, N, C, H, W);
    if (int e = check_shape(what, N, C, H, W)) return e;
    AGAN_REQUIRE(dy && M && dx, "%s: null pointer", what);
    const Shape s = shape_of(C, H, W);
    const int tiles_x = cdiv(W, kTileW);
    const long long tps = (long long)tiles_x * cdiv(H, kTileH);
    AGAN_REQUIRE(tps * N < (1ll << 31), "%s: too many tiles (N %d, H %d, W %d)", what, N, H, W);
    hipStream_t st = as_stream(stream);
    const auto launch = [&](auto CC) {
        hipLaunchKernelGGL((warp_bwd_kernel<CC()>), dim3((unsigned)(tps * N)), dim3(kThreads), 0, st, dy, M, s, dx, tiles_x, (int)tps);
    };
    if (!with_int<1, 2, 3>(C, launch)) launch(Int<4>{});
    return check_launch(what);
}
