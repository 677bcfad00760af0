// The pieces of an fp32 "scores never leave the registers" contraction that kmeans.hip (assign) and manifold.hip share: a workgroup of
// kTileThreads threads stages R rows x kStep columns of a row-major matrix through registers into a k-major LDS image, and a wave
// multiplies such images with v_mfma_f32_32x32x2_f32.  Nothing here depends on what the caller does with the accumulators.
#pragma once
#include "agan_common.h"

namespace agan {

typedef float f32x16 __attribute__((ext_vector_type(16)));        // accumulator of a 32 x 32 MFMA tile
typedef float f32x4 __attribute__((ext_vector_type(4)));          // accumulator of a 16 x 16 MFMA tile; a 16-byte access
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int kTileThreads = 256;      // threads of a workgroup that uses TileRegs
constexpr int kStep = 32;              // columns of D per LDS stage
constexpr int kPad = 2;                // LDS row pad.  Row stride R + 2 = 2 (mod 64 banks): a wave's k-major stores hit 64 different banks on both load
                                       // paths (16-byte path: bank 8 (t & 7) + (t >> 3) + const; 4-byte path: 2 (t & 31) + (t >> 5) + const), and the two
                                       // lane halves of an MFMA operand read, 16 rows apart, lie 16 * 130 = 32 (mod 64) banks apart

// R rows x kStep columns of a row-major [n_rows, D] matrix, from (row0, d0), into registers; rows and columns past the matrix read 0.
// VEC (D % 4 == 0): lane -> 4 columns (t & 7) * 4 of row (t >> 3) + 32 j; else lane -> column t & 31 of row (t >> 5) + 8 j.
template <int R, bool VEC>
struct TileRegs {
    static constexpr int kN = R * kStep / kTileThreads;     // floats per thread
    float v[kN];
    __device__ __forceinline__ void load(const float* __restrict__ m, int n_rows, int D, int row0, int d0) {
        const int t = threadIdx.x;
        const int left = n_rows - row0;                             // (row0 + a tile row may pass 2^31: compare tile rows with what is left)
        if (VEC) {
            const int col = d0 + (t & 7) * 4;
#pragma unroll
            for (int j = 0; j < kN / 4; ++j) {
                const int row = (t >> 3) + 32 * j;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < left && col < D) q = *reinterpret_cast<const float4*>(m + ((size_t)row0 + row) * D + col);
                v[4 * j] = q.x, v[4 * j + 1] = q.y, v[4 * j + 2] = q.z, v[4 * j + 3] = q.w;
            }
        } else {
            const int col = d0 + (t & 31);
#pragma unroll
            for (int j = 0; j < kN; ++j) {
                const int row = (t >> 5) + 8 * j;
                v[j] = (row < left && col < D) ? m[((size_t)row0 + row) * D + col] : 0.f;
            }
        }
    }
    // -> the k-major LDS image s[k][R + kPad]
    __device__ __forceinline__ void store(float* s) const {
        const int t = threadIdx.x;
        if (VEC) {
#pragma unroll
            for (int j = 0; j < kN / 4; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) s[((t & 7) * 4 + q) * (R + kPad) + (t >> 3) + 32 * j] = v[4 * j + q];
        } else {
#pragma unroll
            for (int j = 0; j < kN; ++j) s[(t & 31) * (R + kPad) + (t >> 5) + 8 * j] = v[j];
        }
    }
    // adds the squares of this thread's part of each of its rows to sq[] (VEC: kN / 4 rows, else kN rows)
    __device__ __forceinline__ void add_squares(float* sq) const {
        if (VEC) {
#pragma unroll
            for (int j = 0; j < kN / 4; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) sq[j] = fmaf(v[4 * j + q], v[4 * j + q], sq[j]);
        } else {
#pragma unroll
            for (int j = 0; j < kN; ++j) sq[j] = fmaf(v[j], v[j], sq[j]);
        }
    }
};

// One LDS stage of the contraction A . B^T: as[k][RA + kPad] holds the A rows (MFMA operand A: the accumulator's registers walk them),
// bs[k][RB + kPad] the B rows (operand B: the accumulator's lane & 31).  The wave owns TA x TB tiles of 32 x 32 from tile (ta0, tb0).
// MFMA j of the stage multiplies columns j (lane half 0) and j + 16 (half 1): any pairing gives the same sum order on every run.
template <int RA, int RB, int TA, int TB>
__device__ __forceinline__ void mfma_stage(const float* as, const float* bs, int ta0, int tb0, int half, int l32, f32x16 (&acc)[TA][TB]) {
#pragma unroll 4
    for (int j = 0; j < kStep / 2; ++j) {
        const int k = j + (kStep / 2) * half;
        float a[TA], b[TB];
#pragma unroll
        for (int i = 0; i < TA; ++i) a[i] = as[k * (RA + kPad) + (ta0 + i) * 32 + l32];
#pragma unroll
        for (int r = 0; r < TB; ++r) b[r] = bs[k * (RB + kPad) + (tb0 + r) * 32 + l32];
#pragma unroll
        for (int i = 0; i < TA; ++i)
#pragma unroll
            for (int r = 0; r < TB; ++r) acc[i][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[r], acc[i][r], 0, 0, 0);
    }
}

// register e of a 32 x 32 accumulator tile: A row (e & 3) + 8 (e >> 2) + 4 half of the tile (ascending in e for a lane), B row lane & 31
__device__ __forceinline__ int mfma_a_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

}  // namespace agan
