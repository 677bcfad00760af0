// The controller of the augmentation probability (include/agan.h: agan_ada_observe / agan_ada_update; augment.py: AdaController,
// ada_reference): p of the gated augmentation entries (csrc/diffaug.hip) follows r_t = E[sign(D(real) - threshold)].
//   observe: one workgroup counts the scores above and below the threshold -- integers, so the order of the reduction cannot show --
//            and WRITES the difference and n into the caller's slot (one slot per discriminator, each written from its own stream).
//   update:  one thread folds the slots into the window, and at the end of a window moves p by the window's share of `rate` towards
//            the target, in double, from device memory to device memory -- like ema.hip's tick, a captured HIP graph keeps adapting on
//            replay without a host read.
// Plain loads and stores, no atomics.
#include "agan_common.h"

using namespace agan;

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void ada_observe_kernel(const float* __restrict__ score, int n, float threshold,
                                                               int32_t* __restrict__ slot) {
    __shared__ int red[kThreads / kWave];
    int tally = 0;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const float v = score[i];
        tally += (v > threshold) - (v < threshold);                    // a NaN is neither
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tally += __shfl_xor(tally, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = tally;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kThreads / kWave; ++w) s += red[w];
        slot[0] = s;
        slot[1] = n;
    }
}

// sum, p and r stay exactly the expressions of include/agan.h: one rounding per operation, no fused multiply-add
__global__ void ada_update_kernel(int32_t* __restrict__ state, int nslots, int interval, double target, double rate, double p_max) {
#pragma clang fp contract(off)
    int sum = state[0], count = state[1];
    for (int i = 0; i < nslots; ++i) {
        int32_t* slot = state + AGAN_ADA_SLOT_WORD + 2 * i;
        if (slot[1] > 0) {
            sum += slot[0];
            count += slot[1];
            slot[0] = 0;
            slot[1] = 0;
        }
    }
    const int calls = state[2] + 1;
    if (calls < interval) {
        state[0] = sum, state[1] = count, state[2] = calls;
        return;
    }
    state[0] = 0, state[1] = 0, state[2] = 0;
    if (count <= 0) return;                                             // an empty window: p stays
    float* f = reinterpret_cast<float*>(state);
    const double r = (double)sum / (double)count;
    const double d = (double)count * rate;
    double p = (double)f[AGAN_ADA_P_WORD];
    if (r > target) p = p + d;
    else if (r < target) p = p - d;
    p = fmin(fmax(p, 0.0), p_max);
    f[AGAN_ADA_P_WORD] = (float)p;
    f[AGAN_ADA_P_WORD + 1] = (float)r;
    state[3] += 1;
}

}  // namespace

extern "C" {

int agan_ada_observe(const float* score, int n, float threshold, int32_t* slot, void* stream) {
    AGAN_REQUIRE(score && slot, "ada_observe: null pointer");
    AGAN_REQUIRE(n >= 1, "ada_observe: %d scores", n);
    AGAN_REQUIRE(threshold == threshold, "ada_observe: the threshold is NaN");
    hipLaunchKernelGGL(ada_observe_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), score, n, threshold, slot);
    return check_launch("ada_observe");
}

int agan_ada_update(int32_t* state, int nslots, int interval, double target, double rate, double p_max, void* stream) {
    AGAN_REQUIRE(state, "ada_update: null state");
    AGAN_REQUIRE(nslots >= 1 && nslots <= 4, "ada_update: %d slots outside 1..4", nslots);
    AGAN_REQUIRE(interval >= 1, "ada_update: interval %d", interval);
    AGAN_REQUIRE(rate >= 0.0, "ada_update: rate %g is negative or NaN", rate);
    AGAN_REQUIRE(p_max > 0.0 && p_max <= 1.0, "ada_update: p_max %g outside (0, 1]", p_max);
    AGAN_REQUIRE(target == target, "ada_update: the target is NaN");
    hipLaunchKernelGGL(ada_update_kernel, dim3(1), dim3(1), 0, as_stream(stream), state, nslots, interval, target, rate, p_max);
    return check_launch("ada_update");
}

}  // extern "C"
