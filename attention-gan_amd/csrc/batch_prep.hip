// Batch preparation from device-resident uint8 shards (include/agan.h: agan_image_prep; data/batches.py: DeviceShardBatches).
//
// One launch turns the rows of a resident [n_src, C, H, W] uint8 array that a batch names into the fp32 images in [-1, 1] the train step
// reads, at up to three resolutions: the gather (rows[b]), the horizontal mirror (flip[b]) and the reference's scale_255_to_1
// ((x - 127.5) / 127.5) in one pass.  The grid is the concatenation of the planes' block ranges; a block finds its plane by comparing
// blockIdx.x with the ranges' first blocks (wave-uniform).
//
// Arithmetic.  Every output is ONE IEEE fp32 division of two integers below 2^24 held exactly in fp32:
//   direct plane   (2 x - 255) / 255                      -- the same real quotient as (float(x) - 127.5f) / 127.5f, whose operands are
//                                                            exact too, so both round to the same fp32: bit-identical to scale_255_to_1;
//   derived plane  (2 num - 255 den) / (255 den)          -- num = sum of w * byte over the antialiased triangle window, den = sum of w
//                                                            (integer weights, den <= 32 * 32, num <= 255 * 1024): the correctly
//                                                            rounded fp32 of the exact resampled value, whatever the summation order.
// No reciprocal multiply anywhere (this file is built without fast-math like the rest of the library).
//
// Memory shape.  A direct plane whose rows are whole 16-byte chunks moves one chunk per lane: a 16-byte load of 16 pixels, four 16-byte
// stores of fp32 (dealt out through LDS so that a wave's store covers consecutive addresses); a mirrored row reads the mirrored chunk
// and reverses its bytes in registers.  Other widths take a one-pixel-per-lane path.  A derived plane stages a band of plane-0 rows plus the filter's halo in LDS (already mirrored), so the 2F x 2F taps of an output
// come from LDS and a source byte is fetched once per band.
#include <algorithm>

#include "agan_common.h"

namespace {
using namespace agan;

constexpr int kThreads = 256;
constexpr int kBandBytes = 24 * 1024;          // LDS of one derived-plane band: (F * rows + F) source rows of round_up(W0, 16) bytes

struct PlaneJob {
    const uint8_t* src;      // direct plane: [n_src, C, H, W]; derived: unused (plane 0's src)
    float* dst;              // [B, C, H, W]
    int H, W;
    int factor;              // 0 = direct, 2 / 4 = derived from plane 0
    int vec;                 // direct: W % 16 == 0 (chunk path); derived: W % 4 == 0 (16-byte stores)
    int band_rows;           // derived: output rows per block
    int bands;               // derived: cdiv(H, band_rows)
    unsigned first_block;    // this plane's blocks are [first_block, next plane's first_block)
};

struct PrepArgs {
    PlaneJob plane[3];
    int n_planes;
    const int32_t* rows;
    const uint8_t* flip;
    int B, C, n_src;
};

__device__ __forceinline__ float scale_u8(int x) { return (float)(2 * x - 255) / 255.0f; }

__device__ __forceinline__ uint4 reverse16(uint4 v) {
    return make_uint4(__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x));
}

// source row of batch sample b, or -1 when it lies outside [0, n_src): that sample is written as zeros and nothing is read
__device__ __forceinline__ int source_row(const PrepArgs& a, int b) {
    const int r = a.rows ? a.rows[b] : b;
    return (r >= 0 && r < a.n_src) ? r : -1;
}

// One 16-byte chunk per lane in, but the four 16-byte stores of a lane would land 64 bytes apart from its neighbours'.  The block's 256
// chunks go through LDS instead: lane t then converts dwords t, 256 + t, 512 + t and 768 + t of the block's 4 KiB of pixels, so every
// store instruction of a wave writes 1 KiB of consecutive addresses.  `ok` (one word per chunk) marks chunks of samples that have a
// source row; the others are written as zeros.
__device__ __forceinline__ void direct_chunks(const PrepArgs& a, const PlaneJob& p, unsigned blk, uint8_t* lds) {
    const int cpr = p.W >> 4;                                            // chunks per image row
    const unsigned per_sample = (unsigned)(a.C * p.H * cpr);            // (the host checked B * C * H * W < 2^31)
    const unsigned total = per_sample * a.B;
    const unsigned q = blk * kThreads + threadIdx.x;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    unsigned ok = 0;
    if (q < total) {
        const int b = (int)(q / per_sample);
        const unsigned r = q % per_sample;
        const int cx = (int)(r % cpr);
        const unsigned line = r / cpr;                                   // c * H + y
        const int row = source_row(a, b);
        if (row >= 0) {
            const bool mirror = a.flip && a.flip[b];
            const size_t s = ((size_t)row * a.C * p.H + line) * p.W + (size_t)(mirror ? cpr - 1 - cx : cx) * 16;
            v = *reinterpret_cast<const uint4*>(p.src + s);
            if (mirror) v = reverse16(v);
            ok = 1;
        }
    }
    unsigned* words = reinterpret_cast<unsigned*>(lds);                  // [4 * kThreads] pixels, then [kThreads] ok flags
    reinterpret_cast<uint4*>(lds)[threadIdx.x] = v;
    words[4 * kThreads + threadIdx.x] = ok;
    __syncthreads();
    float4* out = reinterpret_cast<float4*>(p.dst) + (size_t)blk * (4 * kThreads);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned i = k * kThreads + threadIdx.x;                   // dword of the block's span; its chunk is i / 4
        if (blk * kThreads + (i >> 2) >= total) continue;
        const unsigned w = words[i];
        out[i] = words[4 * kThreads + (i >> 2)]
                     ? make_float4(scale_u8(w & 255), scale_u8((w >> 8) & 255), scale_u8((w >> 16) & 255), scale_u8(w >> 24))
                     : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__device__ __forceinline__ void direct_pixels(const PrepArgs& a, const PlaneJob& p, unsigned blk) {
    const unsigned per_sample = (unsigned)(a.C * p.H * p.W);
    const unsigned i = blk * kThreads + threadIdx.x;
    if (i >= per_sample * a.B) return;
    const int b = (int)(i / per_sample);
    const unsigned r = i % per_sample;
    const int x = (int)(r % p.W);
    const int row = source_row(a, b);
    if (row < 0) { p.dst[i] = 0.f; return; }
    const bool mirror = a.flip && a.flip[b];
    p.dst[i] = scale_u8(p.src[(size_t)row * per_sample + (r - x) + (mirror ? p.W - 1 - x : x)]);
}

// F = 2: taps F*o - 1 .. F*o + 2, weights 1 3 3 1;  F = 4: taps F*o - 2 .. F*o + 5, weights 1 3 5 7 7 5 3 1 (the triangle filter of
// torch's antialiased bilinear resize at scale F, times 8 / 32); taps outside the image drop out of numerator and denominator alike
template <int F> __device__ __forceinline__ int tap_weight(int k) { return min(2 * k + 1, 4 * F - 1 - 2 * k); }

template <int F, int V>
__device__ __forceinline__ void derived_band(const PrepArgs& a, const PlaneJob& p, unsigned blk, uint8_t* lds) {
    const PlaneJob& p0 = a.plane[0];
    const int H0 = p0.H, W0 = p0.W, pitch = (W0 + 15) & ~15;
    const int band = (int)(blk % p.bands);
    const int bc = (int)(blk / p.bands);                                 // b * C + c
    const int b = bc / a.C, c = bc % a.C;
    const int o0 = band * p.band_rows, o1 = min(p.H, o0 + p.band_rows);
    const int row = source_row(a, b);                                    // uniform over the block
    float* dst = p.dst + ((size_t)bc * p.H) * p.W;
    const int units_per_row = p.W / V;
    const int units = (o1 - o0) * units_per_row;
    if (row < 0) {
        for (int u = threadIdx.x; u < units; u += kThreads) {
            const int oy = o0 + u / units_per_row, ox = (u % units_per_row) * V;
            float* d = dst + (size_t)oy * p.W + ox;
            if (V == 4) *reinterpret_cast<float4*>(d) = make_float4(0.f, 0.f, 0.f, 0.f);
            else *d = 0.f;
        }
        return;
    }
    // ---- stage source rows [y_lo, y_hi) of channel c, mirrored if asked, at LDS row (y - y_base)
    const int y_base = F * o0 - F / 2;
    const int y_lo = max(0, y_base), y_hi = min(H0, F * o1 + F / 2);
    const bool mirror = a.flip && a.flip[b];
    const uint8_t* src = p0.src + ((size_t)row * a.C + c) * H0 * W0;
    if (p0.vec) {
        const int cpr = W0 >> 4, n = (y_hi - y_lo) * cpr;
        for (int q = threadIdx.x; q < n; q += kThreads) {
            const int y = y_lo + q / cpr, cx = q % cpr;
            uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)y * W0 + (mirror ? cpr - 1 - cx : cx) * 16);
            if (mirror) v = reverse16(v);
            *reinterpret_cast<uint4*>(lds + (y - y_base) * pitch + cx * 16) = v;
        }
    } else {
        const int n = (y_hi - y_lo) * W0;
        for (int q = threadIdx.x; q < n; q += kThreads) {
            const int y = y_lo + q / W0, x = q % W0;
            lds[(y - y_base) * pitch + x] = src[(size_t)y * W0 + (mirror ? W0 - 1 - x : x)];
        }
    }
    __syncthreads();
    // ---- each unit: V outputs side by side; per tap row the V horizontal sums share one window of F * V + F bytes
    for (int u = threadIdx.x; u < units; u += kThreads) {
        const int oy = o0 + u / units_per_row, ox = (u % units_per_row) * V;
        const int x_base = F * ox - F / 2;
        int num[V] = {}, den_x[V] = {}, den_y = 0;
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int k = 0; k < 2 * F; ++k) {
                const int x = x_base + F * v + k;
                den_x[v] += (x >= 0 && x < W0) ? tap_weight<F>(k) : 0;
            }
#pragma unroll
        for (int j = 0; j < 2 * F; ++j) {
            const int y = F * oy - F / 2 + j;
            if (y < 0 || y >= H0) continue;
            const int wy = tap_weight<F>(j);
            den_y += wy;
            const uint8_t* line = lds + (y - y_base) * pitch;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                int h = 0;
#pragma unroll
                for (int k = 0; k < 2 * F; ++k) {
                    const int x = x_base + F * v + k;
                    if (x >= 0 && x < W0) h += tap_weight<F>(k) * line[x];
                }
                num[v] += wy * h;
            }
        }
        float r[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int den = den_y * den_x[v];
            r[v] = (float)(2 * num[v] - 255 * den) / (float)(255 * den);
        }
        float* d = dst + (size_t)oy * p.W + ox;
        if (V == 4) *reinterpret_cast<float4*>(d) = make_float4(r[0], r[1], r[2], r[3]);
        else *d = r[0];
    }
}

__global__ __launch_bounds__(kThreads) void image_prep_kernel(const PrepArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kBandBytes];
    int i = 0;
    if (a.n_planes > 1 && blockIdx.x >= a.plane[1].first_block) i = 1;
    if (a.n_planes > 2 && blockIdx.x >= a.plane[2].first_block) i = 2;
    const PlaneJob& p = a.plane[i];
    const unsigned blk = blockIdx.x - p.first_block;
    if (p.factor == 0) {
        if (p.vec) direct_chunks(a, p, blk, lds);
        else direct_pixels(a, p, blk);
    } else if (p.factor == 2) {
        if (p.vec) derived_band<2, 4>(a, p, blk, lds);
        else derived_band<2, 1>(a, p, blk, lds);
    } else {
        if (p.vec) derived_band<4, 4>(a, p, blk, lds);
        else derived_band<4, 1>(a, p, blk, lds);
    }
}

}  // namespace

extern "C" int agan_image_prep(const agan_image_plane* planes, int n_planes, const int32_t* rows, const uint8_t* flip, int B, int C,
                               int n_src, void* stream) {
    AGAN_REQUIRE(planes, "image_prep: null plane array");
    AGAN_REQUIRE(n_planes >= 1 && n_planes <= 3, "image_prep: n_planes %d outside 1..3", n_planes);
    AGAN_REQUIRE(B > 0 && C > 0 && n_src > 0, "image_prep: bad shape (B %d, C %d, n_src %d)", B, C, n_src);
    AGAN_REQUIRE(planes[0].src, "image_prep: plane 0 has no source (only planes 1.. may be derived)");
    PrepArgs a;
    memset(&a, 0, sizeof(a));
    a.n_planes = n_planes;
    a.rows = rows;
    a.flip = flip;
    a.B = B, a.C = C, a.n_src = n_src;
    size_t blocks = 0;
    for (int i = 0; i < n_planes; ++i) {
        const agan_image_plane& in = planes[i];
        PlaneJob& p = a.plane[i];
        AGAN_REQUIRE(in.dst, "image_prep: plane %d has no destination", i);
        AGAN_REQUIRE(in.H > 0 && in.W > 0, "image_prep: plane %d has bad size %d x %d", i, in.H, in.W);
        const size_t elems = (size_t)B * C * in.H * in.W;
        AGAN_REQUIRE(elems < ((size_t)1 << 31), "image_prep: plane %d is too large (B %d, C %d, %d x %d)", i, B, C, in.H, in.W);
        p.src = in.src, p.dst = in.dst, p.H = in.H, p.W = in.W;
        p.first_block = (unsigned)blocks;
        if (in.src) {
            p.factor = 0;
            p.vec = in.W % 16 == 0;
            blocks += cdivz(p.vec ? elems / 16 : elems, kThreads);
        } else {
            const int H0 = planes[0].H, W0 = planes[0].W;
            const int f = (H0 == 2 * in.H && W0 == 2 * in.W) ? 2 : (H0 == 4 * in.H && W0 == 4 * in.W) ? 4 : 0;
            AGAN_REQUIRE(f, "image_prep: derived plane %d is %d x %d, plane 0 is %d x %d: not plane 0 / 2 or / 4 on both axes", i, in.H, in.W, H0, W0);
            const int pitch = (W0 + 15) & ~15;
            const int max_rows = (kBandBytes / pitch - f) / f;            // (f * rows + f) * pitch <= kBandBytes
            AGAN_REQUIRE(max_rows >= 1, "image_prep: plane 0 is %d wide, a derived plane needs %d of its rows in %d bytes of LDS", W0, 2 * f, kBandBytes);
            p.factor = f;
            p.vec = in.W % 4 == 0;
            p.band_rows = std::max(1, std::min(std::min(max_rows, in.H), cdiv(4 * kThreads, in.W)));
            p.bands = cdiv(in.H, p.band_rows);
            blocks += (size_t)B * C * p.bands;
        }
        AGAN_REQUIRE(blocks < ((size_t)1 << 31), "image_prep: %zu blocks", blocks);
    }
    hipLaunchKernelGGL(image_prep_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, as_stream(stream), a);
    return check_launch("image_prep");
}
