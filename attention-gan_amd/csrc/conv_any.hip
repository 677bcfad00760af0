// Trainable general 2-D convolution (include/agan.h: agan_conv2d_train_*): forward, data gradient and weight gradient of any conv
// `Layers.conv` can return -- per axis K in 1..5, stride 1..3, padding 0..3 (padding >= K included), channel slices on both sides.
//
// Three implicit GEMMs on v_mfma_f32_32x32x2_f32, fp32 operands in every precision mode, no atomics, every sum in index order:
//
//   forward   D[n][pixel of y]   = sum_{c,r,s}   w[n][c][r][s]  * x [b, c, oy*SH + r - PH, ox*SW + s - PW]
//   dgrad     D[c][pixel of dx]  = sum_{n,t,tt}  w[n][c][r][s]  * dy[b, n, u + qa - t, v + qb - tt]          per residue class (a, b)
//   wgrad     D[n][(c, r, s)]    = sum_{b,oy,ox} dy[b, n, oy, ox] * x [b, c, oy*SH + r - PH, ox*SW + s - PW]   per slab of the pixel range
//
// The MFMA's A operand (row index of D, 16 registers per lane) is the channel-like dimension, its B operand (column = lane) the
// dimension that is contiguous in the produced tensor, so every store instruction writes runs of 32 consecutive floats.
//
// Data gradient: dx splits into SH*SW residue classes; class (a, b) holds the pixels iy = a + SH*u, ix = b + SW*v and receives the
// taps r = r0 + SH*t, r0 = (a + PH) % SH (likewise s), read at dy row u + (a + PH) / SH - t: a stride-1 gather.  The classes are
// the z dimension of one launch.  A class without a tap (K < S) and pixels no window reaches gather nothing and are stored as
// zero (left as they are under `accumulate`, where zero is added).
//
// Weight gradient: the pixel range B*OH*OW is cut into slabs (plan_slabs: from the descriptor alone); each slab's partial dw goes to
// the workspace and conv_any_slab_sum_kernel adds the slabs in index order -- two runs give the same bits.
//
// Weights: forward and data gradient read a transposed copy [reduction row][row of D] that the call itself writes into its
// workspace (conv_any_pack_kernel: a training step changes the weights between calls anyway), so there is no pack cache to keep.
#include "conv_common.h"

namespace agan {
namespace conv {
namespace {

constexpr int kTI = 64;      // rows of D per workgroup (channel-like)
constexpr int kTJ = 128;     // columns of D per workgroup (pixel-like)
constexpr int kKS = 16;      // reduction steps per LDS tile
constexpr int kNT = 256;     // 4 waves: wave w computes rows 32*(w & 1) .., columns 64*(w >> 1) ..
// LDS row strides (floats).  The gather kernels write a row with the lane on the column: any stride is conflict-free on the
// write, and a stride = 32 (mod 64) puts the two k rows an MFMA operand load reads on disjoint banks.  The weight-gradient kernel
// writes with the lane on the REDUCTION index (16 lanes x 4 column groups 16 apart): a stride = 33 (mod 64) keeps those 64
// addresses on 64 banks, and the operand load collides on one bank only.
constexpr int kSA = kTI + 32, kSB = kTJ + 32;
constexpr int kSAW = kTI + 33, kSBW = kTJ + 33;
constexpr int kChain = 256;         // reduction steps of one accumulator chain in the gather kernel (a multiple of kKS)
constexpr int kMaxSlabLen = 2048;   // pixels per weight-gradient slab at most: bounds the length of one fp32 accumulation chain

// what one launch (forward) or one residue class of it (data gradient) gathers and where it stores
struct View {
    int NI, NC, nr, ns, K;                    // rows of D, reduction channels, taps, reduction length NC * nr * ns
    int JH, JW, NJ;                           // pixel grid of D per image, columns of D (B * JH * JW)
    int srcH, srcW, srcHW, srcB, src0;        // gathered tensor: size, channel stride, batch stride, offset of the slice
    int uy, ty, oy, ux, tx, ox;               // source row = u * uy + t * ty + oy (u: row of D's grid, t: tap), likewise columns
    int dstB, dst0, dstHW, dstW, dsy, dy0, dsx, dx0;   // produced tensor: row u * dsy + dy0, column v * dsx + dx0
    int KH, KW, r0, rs, s0, ss;               // tap t is kernel row r0 + t * rs (packed-weight row (c * KH + r) * KW + s)
};

__host__ __device__ inline View make_view(const agan_conv2d_desc& d, int dgrad, int cls) {
    View v;
    v.KH = d.KH; v.KW = d.KW;
    if (!dgrad) {
        v.NI = d.Cout; v.NC = d.Cin; v.nr = d.KH; v.ns = d.KW;
        v.JH = d.OH; v.JW = d.OW;
        v.srcH = d.IH; v.srcW = d.IW; v.srcHW = d.IH * d.IW; v.srcB = d.in_ctot * v.srcHW; v.src0 = d.in_c0 * v.srcHW;
        v.uy = d.SH; v.ty = 1; v.oy = -d.PH; v.ux = d.SW; v.tx = 1; v.ox = -d.PW;
        v.dstHW = d.OH * d.OW; v.dstB = d.out_ctot * v.dstHW; v.dst0 = d.out_c0 * v.dstHW; v.dstW = d.OW;
        v.dsy = 1; v.dy0 = 0; v.dsx = 1; v.dx0 = 0;
        v.r0 = 0; v.rs = 1; v.s0 = 0; v.ss = 1;
    } else {
        const int a = cls / d.SW, b = cls - a * d.SW;
        v.NI = d.Cin; v.NC = d.Cout;
        v.r0 = (a + d.PH) % d.SH; v.rs = d.SH; v.nr = v.r0 < d.KH ? (d.KH - v.r0 + d.SH - 1) / d.SH : 0;
        v.s0 = (b + d.PW) % d.SW; v.ss = d.SW; v.ns = v.s0 < d.KW ? (d.KW - v.s0 + d.SW - 1) / d.SW : 0;
        v.JH = a < d.IH ? (d.IH - a + d.SH - 1) / d.SH : 0;
        v.JW = b < d.IW ? (d.IW - b + d.SW - 1) / d.SW : 0;
        v.srcH = d.OH; v.srcW = d.OW; v.srcHW = d.OH * d.OW; v.srcB = d.out_ctot * v.srcHW; v.src0 = d.out_c0 * v.srcHW;
        v.uy = 1; v.ty = -1; v.oy = (a + d.PH) / d.SH; v.ux = 1; v.tx = -1; v.ox = (b + d.PW) / d.SW;
        v.dstHW = d.IH * d.IW; v.dstB = d.in_ctot * v.dstHW; v.dst0 = d.in_c0 * v.dstHW; v.dstW = d.IW;
        v.dsy = d.SH; v.dy0 = a; v.dsx = d.SW; v.dx0 = b;
    }
    v.K = v.NC * v.nr * v.ns;
    v.NJ = d.B * v.JH * v.JW;
    return v;
}

// one LDS tile: 8 k pairs, a 32-row A fragment against two 32-column B fragments
template <int SA, int SB>
__device__ __forceinline__ void mfma_tile(const float* As, const float* Bs, int lane, int wi, int wj, f32x16& acc0, f32x16& acc1) {
    const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int p = 0; p < kKS / 2; ++p) {
        const float a = As[(2 * p + half) * SA + 32 * wi + l31];
        const float b0 = Bs[(2 * p + half) * SB + 64 * wj + l31];
        const float b1 = Bs[(2 * p + half) * SB + 64 * wj + 32 + l31];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
    }
}

// row of D that accumulator register r of this lane holds (C/D layout of the 32x32 MFMAs)
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// wk[((a * KH + r) * KW + s) * NI + i] = w[n][c][r][s]   with (a, i) = (c, n) for the forward, (n, c) for the data gradient
__global__ __launch_bounds__(256) void conv_any_pack_kernel(const float* __restrict__ w, float* __restrict__ wk, int Cout, int Cin, int KH,
                                                             int KW, int dgrad) {
    const int total = Cout * Cin * KH * KW, NI = dgrad ? Cin : Cout;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int i = idx % NI, row = idx / NI;
        const int s = row % KW, r = (row / KW) % KH, a = row / (KW * KH);
        const int n = dgrad ? a : i, c = dgrad ? i : a;
        wk[idx] = w[((n * Cin + c) * KH + r) * KW + s];
    }
}

// forward (dgrad = 0) and data gradient (dgrad = 1; blockIdx.z = residue class)
__global__ __launch_bounds__(kNT) void conv_any_gather_kernel(const float* __restrict__ src, const float* __restrict__ wk,
                                                               const float* __restrict__ bias, float* __restrict__ dst, agan_conv2d_desc d,
                                                               int dgrad, int accumulate) {
    __shared__ float As[kKS * kSA];
    __shared__ float Bs[kKS * kSB];
    const View v = make_view(d, dgrad, blockIdx.z);
    const int j0 = blockIdx.x * kTJ, i0 = blockIdx.y * kTI;
    if (j0 >= v.NJ) return;                                       // a smaller class than the one the grid was sized for
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wi = wave & 1, wj = wave >> 1;
    const int JHW = v.JH * v.JW, ntap = v.nr * v.ns;

    // the two columns of D this lane gathers: batch offset and source coordinates of tap (0, 0)
    int pb[2], py[2], px[2];
    bool pv[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = j0 + lane + 64 * h;
        pv[h] = j < v.NJ;
        const int jj = pv[h] ? j : 0;
        const int b = jj / JHW, rem = jj - b * JHW, u = rem / v.JW, c = rem - u * v.JW;
        pb[h] = b * v.srcB + v.src0;
        py[h] = u * v.uy + v.oy;
        px[h] = c * v.ux + v.ox;
    }
    const bool iv = i0 + lane < v.NI;

    float ra[4], rb[4][2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + wave + 4 * q;                      // wave-uniform: decoded on the scalar unit
            ra[q] = 0.f; rb[q][0] = 0.f; rb[q][1] = 0.f;
            if (k < v.K) {
                const int c = k / ntap, tap = k - c * ntap, t = tap / v.ns, tt = tap - t * v.ns;
                const int row = (c * v.KH + v.r0 + t * v.rs) * v.KW + v.s0 + tt * v.ss;
                if (iv) ra[q] = wk[row * v.NI + i0 + lane];
                const int choff = c * v.srcHW, sy_off = t * v.ty, sx_off = tt * v.tx;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int sy = py[h] + sy_off, sx = px[h] + sx_off;
                    if (pv[h] && (unsigned)sy < (unsigned)v.srcH && (unsigned)sx < (unsigned)v.srcW)
                        rb[q][h] = src[pb[h] + choff + sy * v.srcW + sx];
                }
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kk = wave + 4 * q;
            As[kk * kSA + lane] = ra[q];
            Bs[kk * kSB + lane] = rb[q][0];
            Bs[kk * kSB + 64 + lane] = rb[q][1];
        }
    };

    // An MFMA accumulator is one fp32 chain over its k range.  A chain stops after kChain reduction steps and is added, in index order,
    // to a running total: the rounding error then grows with sqrt(kChain) + sqrt(K / kChain) instead of sqrt(K) (measured against
    // float64 at K = 1024: 5.5e-7 relative as one chain -- twice torch's CPU fp32 conv -- DESIGN.md section 11 has the figures after)
    f32x16 acc0 = {0}, acc1 = {0}, tot0 = {0}, tot1 = {0};
    if (v.K > 0) {
        fetch(0);
        stash();
        __syncthreads();
        for (int k0 = 0; k0 < v.K; k0 += kKS) {
            const bool more = k0 + kKS < v.K;
            if (more) fetch(k0 + kKS);                            // the next tile's loads are in flight under this tile's MFMAs
            mfma_tile<kSA, kSB>(As, Bs, lane, wi, wj, acc0, acc1);
            if ((k0 + kKS) % kChain == 0) {
                tot0 += acc0; tot1 += acc1;
                acc0 = f32x16{0}; acc1 = f32x16{0};
            }
            __syncthreads();
            if (more) stash();
            __syncthreads();
        }
        acc0 += tot0; acc1 += tot1;
    }

#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int j = j0 + 64 * wj + 32 * e + (lane & 31);
        if (j >= v.NJ) continue;
        const int b = j / JHW, rem = j - b * JHW, u = rem / v.JW, c = rem - u * v.JW;
        const int base = b * v.dstB + v.dst0 + (u * v.dsy + v.dy0) * v.dstW + c * v.dsx + v.dx0;
        const f32x16& acc = e ? acc1 : acc0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + 32 * wi + acc_row(r, lane);
            if (i >= v.NI) continue;
            float val = acc[r];
            if (bias) val += bias[i];
            const int idx = base + i * v.dstHW;
            if (accumulate) val = dst[idx] + val;
            dst[idx] = val;
        }
    }
}

// weight gradient of one slab of the pixel range: slabs[blockIdx.z][n][(c, r, s)]
__global__ __launch_bounds__(kNT) void conv_any_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ slabs,
                                                              agan_conv2d_desc d, int slab_len) {
    __shared__ float As[kKS * kSAW];
    __shared__ float Bs[kKS * kSBW];
    const int taps = d.KH * d.KW, Nn = d.Cin * taps, OHW = d.OH * d.OW, IHW = d.IH * d.IW, P = d.B * OHW;
    const int j0 = blockIdx.x * kTJ, i0 = blockIdx.y * kTI;
    const int p_lo = blockIdx.z * slab_len, p_hi = min(P, p_lo + slab_len);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wi = wave & 1, wj = wave >> 1;
    const int pp = lane & 15, col = 16 * (lane >> 4) + wave;      // this lane loads reduction index pp of columns col + 4q (+ 64)
    const int xB = d.in_ctot * IHW, x0 = d.in_c0 * IHW, dyB = d.out_ctot * OHW, dy0 = d.out_c0 * OHW;

    // the 8 columns (c, r, s) of D this lane gathers: offset from the window origin, tap position relative to it
    int joff[8], jdr[8], jds[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const int j = j0 + 64 * (n >> 2) + col + 4 * (n & 3);
        const int jj = j < Nn ? j : 0;
        const int c = jj / taps, rem = jj - c * taps, r = rem / d.KW, s = rem - r * d.KW;
        jdr[n] = j < Nn ? r - d.PH : -(1 << 29);                  // a column past the matrix fails every range check
        jds[n] = s - d.PW;
        joff[n] = c * IHW + (r - d.PH) * d.IW + (s - d.PW);
    }

    float ra[4], rb[8];
    auto fetch = [&](int p0) {
        const int p = p0 + pp;
        const bool pvalid = p < p_hi;
        const int pc = pvalid ? p : 0;
        const int b = pc / OHW, pix = pc - b * OHW, oy = pix / d.OW, ox = pix - oy * d.OW;
        const int dybase = b * dyB + dy0 + pix;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + col + 4 * q;
            ra[q] = (pvalid && i < d.Cout) ? dy[dybase + i * OHW] : 0.f;
        }
        const int iy0 = oy * d.SH, ix0 = ox * d.SW;
        const int xbase = b * xB + x0 + iy0 * d.IW + ix0;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int iy = iy0 + jdr[n], ix = ix0 + jds[n];
            rb[n] = (pvalid && (unsigned)iy < (unsigned)d.IH && (unsigned)ix < (unsigned)d.IW) ? x[xbase + joff[n]] : 0.f;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) As[pp * kSAW + col + 4 * q] = ra[q];
#pragma unroll
        for (int n = 0; n < 8; ++n) Bs[pp * kSBW + 64 * (n >> 2) + col + 4 * (n & 3)] = rb[n];
    };

    f32x16 acc0 = {0}, acc1 = {0};
    if (p_lo < p_hi) {
        fetch(p_lo);
        stash();
        __syncthreads();
        for (int p0 = p_lo; p0 < p_hi; p0 += kKS) {
            const bool more = p0 + kKS < p_hi;
            if (more) fetch(p0 + kKS);
            mfma_tile<kSAW, kSBW>(As, Bs, lane, wi, wj, acc0, acc1);
            __syncthreads();
            if (more) stash();
            __syncthreads();
        }
    }

    float* out = slabs + (size_t)blockIdx.z * d.Cout * Nn;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int j = j0 + 64 * wj + 32 * e + (lane & 31);
        if (j >= Nn) continue;
        const f32x16& acc = e ? acc1 : acc0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + 32 * wi + acc_row(r, lane);
            if (i < d.Cout) out[(size_t)i * Nn + j] = acc[r];
        }
    }
}

// dw (+)= slab 0 + slab 1 + ... in index order
__global__ __launch_bounds__(256) void conv_any_slab_sum_kernel(const float* __restrict__ slabs, float* __restrict__ dw, int n, int nslab,
                                                                 int accumulate) {
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
        float s = slabs[idx];
        for (int k = 1; k < nslab; ++k) s += slabs[(size_t)k * n + idx];
        dw[idx] = accumulate ? dw[idx] + s : s;
    }
}

constexpr long long kMaxElems = 1ll << 30;

int check_desc(const agan_conv2d_desc* d, const char* who) {
    AGAN_REQUIRE(d != nullptr, "%s: null descriptor", who);
    AGAN_REQUIRE(d->B > 0 && d->Cin > 0 && d->IH > 0 && d->IW > 0 && d->Cout > 0 && d->OH > 0 && d->OW > 0, "%s: non-positive dimension", who);
    AGAN_REQUIRE(d->KH >= 1 && d->KH <= 5 && d->KW >= 1 && d->KW <= 5 && d->KH * d->KW <= 25, "%s: taps %dx%d outside 1..5", who, d->KH, d->KW);
    AGAN_REQUIRE(d->SH >= 1 && d->SH <= 3 && d->SW >= 1 && d->SW <= 3, "%s: stride %dx%d outside 1..3", who, d->SH, d->SW);
    AGAN_REQUIRE(d->PH >= 0 && d->PH <= 3 && d->PW >= 0 && d->PW <= 3, "%s: padding %dx%d outside 0..3", who, d->PH, d->PW);
    AGAN_REQUIRE(d->IH + 2 * d->PH >= d->KH && d->IW + 2 * d->PW >= d->KW, "%s: kernel larger than the padded input", who);
    AGAN_REQUIRE(d->OH == (d->IH + 2 * d->PH - d->KH) / d->SH + 1 && d->OW == (d->IW + 2 * d->PW - d->KW) / d->SW + 1,
                 "%s: output %dx%d does not follow from the geometry", who, d->OH, d->OW);
    AGAN_REQUIRE(d->in_c0 >= 0 && d->in_ctot > 0 && d->in_c0 <= d->in_ctot - d->Cin, "%s: input slice [%d, %d) outside %d channels", who, d->in_c0,
                 d->in_c0 + d->Cin, d->in_ctot);
    AGAN_REQUIRE(d->out_c0 >= 0 && d->out_ctot > 0 && d->out_c0 <= d->out_ctot - d->Cout, "%s: output slice [%d, %d) outside %d channels", who,
                 d->out_c0, d->out_c0 + d->Cout, d->out_ctot);
    AGAN_REQUIRE((long long)d->B * d->in_ctot * d->IH * d->IW < kMaxElems && (long long)d->B * d->out_ctot * d->OH * d->OW < kMaxElems &&
                     (long long)d->Cout * d->Cin * d->KH * d->KW < kMaxElems,
                 "%s: a tensor of 2^30 elements or more", who);
    return AGAN_OK;
}

struct SlabPlan { int nslab, slab_len; };
// slabs of the weight gradient's pixel range: enough workgroups to fill the chip, accumulation chains of at most kMaxSlabLen terms
SlabPlan plan_slabs(const agan_conv2d_desc& d) {
    const int P = d.B * d.OH * d.OW;
    const int tiles = cdiv(d.Cin * d.KH * d.KW, kTJ) * cdiv(d.Cout, kTI);
    int nslab = std::max(cdiv(1024, tiles), cdiv(P, kMaxSlabLen));
    int len = std::max(64, cdiv(cdiv(P, nslab), kKS) * kKS);
    if (cdiv(P, len) > 32768) len = cdiv(cdiv(P, 32768), kKS) * kKS;        // (the slab index is the grid's z dimension)
    SlabPlan s;
    s.slab_len = len;
    s.nslab = cdiv(P, len);
    return s;
}

size_t weight_bytes(const agan_conv2d_desc& d) { return (size_t)d.Cout * d.Cin * d.KH * d.KW * sizeof(float); }

int need_ws(const char* who, size_t need, const void* ws, size_t ws_bytes) {
    if (!ws) {
        set_error("%s: no workspace", who);
        return AGAN_EWORKSPACE;
    }
    if (int e = check_ws(who, need, ws, ws_bytes)) return e;
    AGAN_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace not 16-byte aligned", who);
    return AGAN_OK;
}

int run_gather(const char* who, const float* src, const float* w, const float* bias, float* dst, const agan_conv2d_desc& d, int dgrad,
               int accumulate, void* ws, hipStream_t st) {
    float* wk = static_cast<float*>(ws);
    const int total = d.Cout * d.Cin * d.KH * d.KW;
    hipLaunchKernelGGL(conv_any_pack_kernel, dim3(std::min(cdiv(total, 256), 2048)), dim3(256), 0, st, w, wk, d.Cout, d.Cin, d.KH, d.KW, dgrad);
    const View v0 = make_view(d, dgrad, 0);                      // class (0, 0) is the largest
    const dim3 grid(cdiv(v0.NJ, kTJ), cdiv(v0.NI, kTI), dgrad ? d.SH * d.SW : 1);
    timed_begin(st);
    AGAN_LAUNCH(conv_any_gather_kernel, grid, dim3(kNT), 0, st, src, wk, bias, dst, d, dgrad, accumulate);
    timed_end(st, 1);
    return check_launch(who);
}

}  // namespace
}  // namespace conv
}  // namespace agan

using namespace agan;
using namespace agan::conv;

extern "C" {

int agan_conv2d_train_supported(const agan_conv2d_desc* d) { return check_desc(d, "conv2d_train") == AGAN_OK ? 1 : 0; }

int agan_conv2d_train_slabs(const agan_conv2d_desc* d) {
    if (check_desc(d, "conv2d_train_slabs")) return AGAN_EINVAL;
    return plan_slabs(*d).nslab;
}

size_t agan_conv2d_train_ws_bytes(const agan_conv2d_desc* d, int direction) {
    if (check_desc(d, "conv2d_train_ws_bytes") || direction < 0 || direction > 2) return 0;
    if (direction < 2) return weight_bytes(*d);
    return (size_t)plan_slabs(*d).nslab * weight_bytes(*d);
}

int agan_conv2d_train_fwd(const float* x, const float* w, const float* bias, float* y, const agan_conv2d_desc* d, void* ws, size_t ws_bytes,
                          void* stream) {
    if (int e = check_desc(d, "conv2d_train_fwd")) return e;
    AGAN_REQUIRE(x && w && y, "conv2d_train_fwd: null tensor");
    if (int e = need_ws("conv2d_train_fwd", weight_bytes(*d), ws, ws_bytes)) return e;
    return run_gather("conv2d_train_fwd", x, w, bias, y, *d, 0, 0, ws, as_stream(stream));
}

int agan_conv2d_train_dgrad(const float* dy, const float* w, float* dx, const agan_conv2d_desc* d, int accumulate, void* ws, size_t ws_bytes,
                            void* stream) {
    if (int e = check_desc(d, "conv2d_train_dgrad")) return e;
    AGAN_REQUIRE(dy && w && dx, "conv2d_train_dgrad: null tensor");
    if (int e = need_ws("conv2d_train_dgrad", weight_bytes(*d), ws, ws_bytes)) return e;
    return run_gather("conv2d_train_dgrad", dy, w, nullptr, dx, *d, 1, accumulate != 0, ws, as_stream(stream));
}

int agan_conv2d_train_wgrad(const float* x, const float* dy, float* dw, const agan_conv2d_desc* d, int accumulate, void* ws, size_t ws_bytes,
                            void* stream) {
    if (int e = check_desc(d, "conv2d_train_wgrad")) return e;
    AGAN_REQUIRE(x && dy && dw, "conv2d_train_wgrad: null tensor");
    const SlabPlan sp = plan_slabs(*d);
    if (int e = need_ws("conv2d_train_wgrad", (size_t)sp.nslab * weight_bytes(*d), ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    float* slabs = static_cast<float*>(ws);
    const int Nn = d->Cin * d->KH * d->KW, n = d->Cout * Nn;
    const dim3 grid(cdiv(Nn, kTJ), cdiv(d->Cout, kTI), sp.nslab);
    timed_begin(st);
    AGAN_LAUNCH(conv_any_wgrad_kernel, grid, dim3(kNT), 0, st, x, dy, slabs, *d, sp.slab_len);
    timed_end(st, sp.nslab);
    if (int e = check_launch("conv2d_train_wgrad")) return e;
    hipLaunchKernelGGL(conv_any_slab_sum_kernel, dim3(std::min(cdiv(n, 256), 4096)), dim3(256), 0, st, slabs, dw, n, sp.nslab, accumulate != 0);
    return check_launch("conv2d_train_wgrad (slab sum)");
}

}  // extern "C"
