// What the BatchNorm files (bn_act.hip, bn_slice.hip, cond_bn.hip) share: the one-launch bound and its values-per-thread tiers, the chunk count of
// the two-pass reductions, the block reduction of two doubles, and the finish of one channel's statistics.
#pragma once
#include "agan_common.h"
#include "dispatch.h"

#include <algorithm>

namespace agan {

constexpr int kThreads = 256;                    // threads per workgroup of the one-launch kernels
constexpr int kSmallN = 8192;                    // channels of n = B*HW <= kSmallN values take ONE launch, the values held in registers
constexpr int kSmallPer = kSmallN / kThreads;    // values per thread that cover kSmallN

// values per thread of a one-launch kernel, f(Int<PER>): the 4x4 / 8x8 maps (n <= 512 / 2048) take 2 / 8 -- the 32-deep form spent
// most of its ~11 us on 30 dead, fully unrolled iterations (an integer division and four predicated loads each)
template <class F> void with_per(int n, F&& f) {
    if (n <= 2 * kThreads) f(Int<2>{});
    else if (n <= 8 * kThreads) f(Int<8>{});
    else f(Int<kSmallPer>{});
}

// partial sums per channel of the two-pass reductions: about 2048 workgroups in all, each over at least 2048 values
inline int bn_chunks(int B, int C, int HW) {
    const long long n = (long long)B * HW;
    const int nchunk = std::max(1, 2048 / std::max(C, 1));
    return (int)std::min<long long>(nchunk, std::max<long long>(1, n / 2048));
}

// sums a and b over the workgroup's four waves, the result in every thread (red may be reused straight away: it syncs first)
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[4]) {
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[0][w] = a; red[1][w] = b; }
    __syncthreads();
    a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
}

// Finishes channel c from its fp64 sum s and sum of squares q over n values: the biased variance clamped at 0, mean and invstd rounded
// once to fp32 (returned; what a kernel that goes on to normalise uses), and, where `write`, mean[c], invstd[c] and the momentum update
// of the running statistics (unbiased variance; running_mean / running_var may both be null).
struct BnStats { float mean, invstd; };
__device__ __forceinline__ BnStats bn_finish_channel(double s, double q, int n, float eps, float momentum, int c, bool write,
                                                     float* mean, float* invstd, float* rmean, float* rvar) {
    const double m = s / n;
    double var = q / n - m * m;
    if (var < 0.0) var = 0.0;
    const BnStats r = {(float)m, (float)(1.0 / sqrt(var + (double)eps))};
    if (write) {
        mean[c] = r.mean;
        invstd[c] = r.invstd;
        if (rmean) {
            const double unbiased = n > 1 ? var * ((double)n / (n - 1)) : var;
            rmean[c] = (float)((1.0 - momentum) * rmean[c] + momentum * m);
            rvar[c] = (float)((1.0 - momentum) * rvar[c] + momentum * unbiased);
        }
    }
    return r;
}

// ---- device pieces the BatchNorm files with an activation share (bn_act.hip, cond_bn.hip) ---------------------------------------
constexpr float kSlope = 0.2f;   // LeakyReLU slope, utilities/layers.py:124

// Values per thread and loop step of the streaming sweeps: 8 where a 16-bit tensor is involved and rows are whole 8-groups (16-byte
// accesses on it), else 4, else 1.  The host's choice of template width and the in-kernel loop choice both call this.
__host__ __device__ __forceinline__ int vec_width(bool any16, int HW) { return (any16 && (HW & 7) == 0) ? 8 : ((HW & 3) == 0 ? 4 : 1); }

// chunk `chunk` of nchunk equal parts [beg, end) of n values
struct Chunk { int beg, end; };

__device__ __forceinline__ Chunk chunk_of(int n, int nchunk, int chunk) {
    int len = (cdiv(n, nchunk) + 7) & ~7;          // (whole 8-element groups: the widest vector access of the kernels below)
    Chunk c;
    c.beg = min(n, chunk * len);
    c.end = min(n, c.beg + len);
    return c;
}

// z = (x - m) * s + b with s = gamma * invstd.  Most channels take the folded form m = 0, b = beta - mean * s (one FMA per value).
// Where the mean is more than kCentreAt standard deviations from 0 the fold cancels two values of magnitude |mean * s| >> |z| and
// loses z's own scale: such a channel is centred first, m = mean, b = beta ((x - mean) is exact there).  x - 0 = x exactly, so the
// folded channels compute exactly what the plain x * s + (beta - mean * s) computes.
constexpr float kCentreAt = 16.f;
struct Affine { float s, m, b; };
__device__ __forceinline__ Affine make_affine(float mean, float invstd, float gamma, float beta) {
    Affine a;
    a.s = gamma * invstd;
    const bool centre = fabsf(mean * invstd) > kCentreAt;
    a.m = centre ? mean : 0.f;
    a.b = centre ? beta : beta - mean * a.s;
    return a;
}
__device__ __forceinline__ float norm_of(const Affine& a, float x) { return (x - a.m) * a.s + a.b; }

// dz for one element.  GLU: returns dz of the value half in dza and of the gate half in dzg.
template <int ACT>
__device__ __forceinline__ void dz_of(float xa, float xg, float d, const Affine& a, const Affine& g, float& dza, float& dzg) {
    if (ACT == AGAN_ACT_GLU) {
        const float za = norm_of(a, xa);
        const float sg = sigmoid_fast(norm_of(g, xg));
        dza = d * sg;
        dzg = d * za * sg * (1.f - sg);
    } else if (ACT == AGAN_ACT_LRELU) {
        const float z = norm_of(a, xa);
        dza = z > 0.f ? d : d * kSlope;         // torch's leaky_relu_backward: slope 1 only where the input is > 0
        dzg = 0.f;
    } else {
        dza = d;
        dzg = 0.f;
    }
}

// The batch statistics of agan_bn_train_fwd on fp32 x, without its apply pass (bn_act.hip): mean / invstd, the running-statistics
// update and ++*nbt come out bit for bit as that call writes them, because each shape takes the same sums in the same order --
// the [B, C] rows kernel for HW == 1, a statistics-only twin of the one-launch kernel's first phase for B * HW <= kSmallN, else the
// two statistics passes.  ws as agan_bn_train_fwd_ws_bytes says.  *form: 1 rows, 2 one launch, 3 two passes; *width: values per thread.
int bn_train_stats(const float* x, int B, int C, int HW, float eps, float* mean, float* invstd, float* running_mean, float* running_var,
                   int64_t* nbt, float momentum, void* ws, size_t ws_bytes, void* stream, int* form, int* width);

}  // namespace agan
