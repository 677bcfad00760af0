// What the BatchNorm files (bn_act.hip, bn_slice.hip) share: the one-launch bound and its values-per-thread tiers, the chunk count of
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

}  // namespace agan
