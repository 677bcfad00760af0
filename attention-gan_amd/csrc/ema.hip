// Exponential moving average of a module's weights and BatchNorm statistics (include/agan.h: agan_ema_update; optim.py: FlatEMA):
// dst += omb * (src - dst) over a device-resident table of segments in ONE launch, behind a one-thread tick that derives omb from the
// update count in device memory -- so a captured HIP graph keeps counting on replay, like agan_adam_step.
#include "agan_common.h"

using namespace agan;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSegBlocks = 2048;       // per segment: a memory-bound pass caps its grid and strides the rest (as adam_kernel does)

// workgroups of a segment of n floats: one float4 per thread and pass
inline int seg_blocks(int64_t n) {
    const int64_t b = (n / 4 + kThreads) / kThreads;
    return (int)(b > kMaxSegBlocks ? kMaxSegBlocks : b);
}

// state[0] = updates so far (int), state[2] = omb = 1 - beta_t (float) for the update that follows on this stream
__global__ void ema_tick_kernel(int32_t* __restrict__ state, double decay, int warmup) {
    const int t = state[0];
    const double beta = warmup ? fmin(decay, (1.0 + t) / (10.0 + t)) : decay;
    reinterpret_cast<float*>(state)[2] = (float)(1.0 - beta);
    state[0] = t + 1;
}

// the table's pointers come out of memory, so the compiler cannot know that they are global addresses: say so (global_load / global_store
// in place of the flat forms)
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) agan_f32x4 gfloat4;

// one rounding of the difference, one of the fused multiply-add -- written out so that the 16-byte path, the scalar path and the
// tails give the same bits whatever the compiler's contraction setting
__device__ __forceinline__ float ema1(float s, float d, float omb) { return fmaf(omb, s - d, d); }

__global__ __launch_bounds__(kThreads) void ema_kernel(const agan_ema_seg* __restrict__ table, int nseg, const int32_t* __restrict__ state) {
    __shared__ int which;
    const int b = blockIdx.x, nblocks = gridDim.x;
    if (threadIdx.x == 0) which = -1;
    __syncthreads();
    for (int t = threadIdx.x; t < nseg; t += kThreads) {
        const int lo = table[t].first_block, hi = t + 1 < nseg ? table[t + 1].first_block : nblocks;
        if (b >= lo && b < hi) which = t;
    }
    __syncthreads();
    const int s = which;
    if (s < 0) return;                       // a workgroup no segment owns (total_blocks larger than the table's sum): nothing to do
    const agan_ema_seg seg = table[s];
    const int nb = (s + 1 < nseg ? table[s + 1].first_block : nblocks) - seg.first_block;
    const int local = b - seg.first_block;
    const float omb = reinterpret_cast<const float*>(state)[2];
    const size_t n = (size_t)seg.n, stride = (size_t)nb * kThreads, i0 = (size_t)local * kThreads + threadIdx.x;
    if (((reinterpret_cast<uintptr_t>(seg.src) | reinterpret_cast<uintptr_t>(seg.dst)) & 15) == 0) {
        const gfloat4* __restrict__ s4 = (const gfloat4*)seg.src;
        gfloat4* __restrict__ d4 = (gfloat4*)seg.dst;
        const size_t n4 = n / 4;
        for (size_t i = i0; i < n4; i += stride) {
            const agan_f32x4 sv = s4[i];
            agan_f32x4 dv = d4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) dv[k] = ema1(sv[k], dv[k], omb);
            d4[i] = dv;
        }
        if (local == 0 && threadIdx.x < (n & 3)) {
            const size_t e = n4 * 4 + threadIdx.x;
            gfloat* dst = (gfloat*)seg.dst;
            dst[e] = ema1(((const gfloat*)seg.src)[e], dst[e], omb);
        }
    } else {                                 // 4-byte alignment only (BatchNorm statistics inside a module): dword loads and stores
        const gfloat* __restrict__ src = (const gfloat*)seg.src;
        gfloat* __restrict__ dst = (gfloat*)seg.dst;
        for (size_t i = i0; i < n; i += stride) dst[i] = ema1(src[i], dst[i], omb);
    }
}

}  // namespace

extern "C" {

int agan_ema_plan(agan_ema_seg* segs, int nseg) {
    AGAN_REQUIRE(segs && nseg >= 1, "ema_plan: empty segment list");
    int64_t first = 0;
    for (int i = 0; i < nseg; ++i) {
        agan_ema_seg& s = segs[i];
        AGAN_REQUIRE(s.src && s.dst, "ema_plan: segment %d has a null pointer", i);
        AGAN_REQUIRE(s.n >= 1, "ema_plan: segment %d has %lld elements", i, (long long)s.n);
        AGAN_REQUIRE(((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst)) & 3) == 0, "ema_plan: segment %d is not 4-byte aligned", i);
        s.first_block = (int32_t)first;
        s.reserved = 0;
        first += seg_blocks(s.n);
        AGAN_REQUIRE(first < ((int64_t)1 << 31), "ema_plan: too many segments for one launch");
    }
    return (int)first;
}

int agan_ema_update(const agan_ema_seg* table, int nseg, int total_blocks, int32_t* state, double decay, int warmup, void* stream) {
    AGAN_REQUIRE(table && state, "ema_update: null pointer");
    AGAN_REQUIRE(nseg >= 1 && total_blocks >= nseg, "ema_update: %d segments in %d workgroups", nseg, total_blocks);
    AGAN_REQUIRE(decay > 0.0 && decay < 1.0, "ema_update: decay %g is not inside (0, 1)", decay);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(1), 0, st, state, decay, warmup != 0);
    hipLaunchKernelGGL(ema_kernel, dim3(total_blocks), dim3(kThreads), 0, st, table, nseg, state);
    return check_launch("ema_update");
}

}  // extern "C"
