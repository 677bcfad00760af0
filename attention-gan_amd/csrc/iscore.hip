// The Inception Score's reduction over a matrix of classifier logits (include/agan.h: agan_inception_score; evaluation.py: inception_score).
// Per split s of the rows: IS_s = exp(Hm_s - Hc_s) with Hm_s the entropy of the split's mean class distribution and Hc_s the mean entropy
// of its rows' distributions.  The logits [N, C] are fp32 and are read twice; everything after the load is fp64 (fp32 -> fp64 is exact),
// and nothing of size N x C is ever stored: the probabilities are recomputed where they are needed.
//
// FOUR PASSES, EACH SUM IN ONE FIXED ORDER.
//   * row pass:    one wave per row, the row in registers.  Lane l holds the float4 groups l, l + 64, l + 128, ... of the row (elements
//                  4 (64 j + l) .. + 3; past the row's end they read -inf, whose exp is an exact 0).  m = max by a butterfly (fp32 max is
//                  exact); sum_y exp(l - m) and sum_y p logp (logp = l - lse, p = exp(logp), a term with p == 0 counts as 0) are each the
//                  lane's chain in ascending element order followed by an xor butterfly, which leaves the same bits in every lane.  The
//                  16-byte and the 4-byte load paths place the same elements in the same lanes: the bits do not depend on the path.
//                  lse[k] and t[k] = sum_y p logp go to the workspace as doubles.
//   * column pass: a lane owns one class y and one PIECE of kPiece consecutive rows of one split, counted from the SPLIT'S first row, and
//                  adds exp(l[k][y] - lse[k]) over the piece's rows in ascending order: one fp64 partial per (split, piece, class).
//                  Neighbouring lanes read neighbouring addresses of a row; lse[k] is the same for the whole wave.
//   * class pass:  a lane owns one class of one split: q = (the pieces' partials added in piece order) / n_s, and leaves the class's term
//                  q log q (0 for q == 0) in the workspace.
//   * finish:      one workgroup per split: the class terms and the rows' t[k] are each added thread-strided in ascending order and then
//                  through one LDS tree; Hm = -sum q log q, Hc = -(sum_k t[k]) / n_s, IS = exp(Hm - Hc).
// A split's numbers depend on its own rows only, and on no launch geometry: the same rows passed alone with splits = 1 give the same bits.
// The grids of the row and column passes are capped and strided, so the largest shapes of the domain launch no more threads than a grid
// can hold; N reaches 2^31 - 1 at C = 1, so every ceiling of a row count is taken in 64 bits (ceil_rows: N + 63 does not fit an int).
// The finish is one workgroup per split: with few splits of very many rows its sum over t[k] (n_s doubles) and the class pass's walk over
// the pieces (n_s / 64 partials per class) run on few compute units -- 7 and 6 us of a 116 us call at 30 000 x 1000 in 10 splits.
// NON-FINITE INPUT needs no branch: fmaxf drops a NaN, so a row with a NaN has a finite or infinite m and a NaN sum; a +inf gives inf - inf
// and a row of nothing but -inf gives -inf - -inf, NaN both.  lse[k] and t[k] of such a row are NaN and so is every number of its split;
// the zero tests are written `== 0 ? 0 : ...`, which a NaN fails.  A -inf logit beside finite ones is p == 0: it contributes nothing.  No
// address depends on the data.  No atomics.
#include <algorithm>

#include "agan_common.h"

namespace {
using namespace agan;

constexpr int kThreads = 256;
constexpr int kRowWaves = kThreads / kWave;   // rows per workgroup of the row pass
constexpr int kMaxClasses = 4096;             // largest C: 16 float4 groups per lane
constexpr int kMaxSplits = 1024;
constexpr int kPiece = 64;                    // rows per piece of the column pass
constexpr int kClassThreads = 64;             // classes per workgroup of the class pass
constexpr int kMaxGridX = 1 << 16;            // cap of the strided grids

// ceil(a / b) for a row count a up to 2^31 - 1 (agan::cdiv adds in int)
__host__ __device__ inline int ceil_rows(int a, int b) { return (int)(((long long)a + b - 1) / b); }

// rows [first, first + count) of split s
struct SplitRows {
    int first, count;
    __host__ __device__ SplitRows(int s, int N, int S) {
        first = (int)((long long)s * N / S);
        count = (int)((long long)(s + 1) * N / S) - first;
    }
};

// J float4 groups per lane: C <= 256 J
template <int J, bool VEC>
__global__ __launch_bounds__(kThreads) void iscore_row_kernel(const float* __restrict__ logits, double* __restrict__ lse, double* __restrict__ t,
                                                              int N, int C) {
    const int lane = threadIdx.x & 63;
    // (a whole wave per row; 64-bit: row + the stride may pass 2^31)
    for (long long row = blockIdx.x * kRowWaves + (threadIdx.x >> 6); row < N; row += (long long)gridDim.x * kRowWaves) {
        const float* __restrict__ x = logits + (size_t)row * C;
        float v[J][4];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int e = (j * kWave + lane) * 4;
            if (VEC) {                                                                  // C % 4 == 0: e < C covers e + 3
                const float4 f = e < C ? *reinterpret_cast<const float4*>(x + e) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                v[j][0] = f.x, v[j][1] = f.y, v[j][2] = f.z, v[j][3] = f.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[j][c] = e + c < C ? x[e + c] : -INFINITY;
            }
        }
        float mf = -INFINITY;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) mf = fmaxf(mf, v[j][c]);
        const double m = (double)wave_max(mf);
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j)
            if (j * kWave * 4 < C) {                                                    // (the skipped groups would add exact zeros)
#pragma unroll
                for (int c = 0; c < 4; ++c) s += exp((double)v[j][c] - m);
            }
        const double row_lse = m + log(wave_sum_d(s));
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j)
            if (j * kWave * 4 < C) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double logp = (double)v[j][c] - row_lse;
                    const double p = exp(logp);
                    a += p == 0.0 ? 0.0 : p * logp;
                }
            }
        a = wave_sum_d(a);
        if (lane == 0) lse[row] = row_lse, t[row] = a;
    }
}

// grid: pieces (strided) x class chunks x splits.  part[(s * P + piece) * C + y]
__global__ __launch_bounds__(kThreads) void iscore_col_kernel(const float* __restrict__ logits, const double* __restrict__ lse,
                                                              double* __restrict__ part, int N, int C, int S, int P) {
    const int y = blockIdx.y * kThreads + threadIdx.x;
    const int s = blockIdx.z;
    const SplitRows sr(s, N, S);
    const int pieces = ceil_rows(sr.count, kPiece);
    if (y >= C) return;
    for (int piece = blockIdx.x; piece < pieces; piece += gridDim.x) {
        const int k0 = sr.first + piece * kPiece;
        const int rows = min(kPiece, sr.first + sr.count - k0);
        const float* __restrict__ x = logits + (size_t)k0 * C + y;
        double acc = 0.0;
#pragma unroll 4
        for (int i = 0; i < rows; ++i) acc += exp((double)x[(size_t)i * C] - lse[k0 + i]);
        part[((size_t)s * P + piece) * C + y] = acc;
    }
}

// grid: class chunks x splits.  term[s * C + y] = q log q
__global__ __launch_bounds__(kClassThreads) void iscore_class_kernel(const double* __restrict__ part, double* __restrict__ term, int N, int C, int S,
                                                                     int P) {
    const int y = blockIdx.x * kClassThreads + threadIdx.x;
    const int s = blockIdx.y;
    if (y >= C) return;
    const SplitRows sr(s, N, S);
    const int pieces = ceil_rows(sr.count, kPiece);
    const double* __restrict__ src = part + (size_t)s * P * C + y;
    double acc = 0.0;
#pragma unroll 8
    for (int p = 0; p < pieces; ++p) acc += src[(size_t)p * C];
    const double q = acc / (double)sr.count;
    term[(size_t)s * C + y] = q == 0.0 ? 0.0 : q * log(q);
}

// thread i adds values i, i + 256, ... in index order; the threads' sums are then added by a fixed tree
__device__ __forceinline__ double block_tree_sum(const double* __restrict__ v, int n, double* red) {
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += kThreads) s += v[i];
    __syncthreads();                                                // (red may still be read from the previous sum)
    block_tree_sum_d<kThreads>(s, red);
    return red[0];
}

__global__ __launch_bounds__(kThreads) void iscore_finish_kernel(const double* __restrict__ term, const double* __restrict__ t,
                                                                 double* __restrict__ scores, int N, int C, int S) {
    __shared__ double red[kThreads];
    const int s = blockIdx.x;
    const SplitRows sr(s, N, S);
    const double hm = -block_tree_sum(term + (size_t)s * C, C, red);
    const double hc = -block_tree_sum(t + sr.first, sr.count, red) / (double)sr.count;
    if (threadIdx.x == 0) {
        scores[3 * s + 0] = exp(hm - hc);
        scores[3 * s + 1] = hm;
        scores[3 * s + 2] = hc;
    }
}

bool in_domain(int N, int C, int splits) {
    return N >= 1 && C >= 1 && C <= kMaxClasses && (long long)N * C < (1ll << 31) && splits >= 1 && splits <= std::min(N, kMaxSplits);
}

// pieces of the largest split (ceil(N / splits) rows)
int max_pieces(int N, int splits) { return ceil_rows(ceil_rows(N, splits), kPiece); }

struct Workspace {
    size_t lse, t, part, term, bytes;       // byte offsets
    Workspace(int N, int C, int splits) {
        lse = 0;
        t = lse + up16((size_t)N * sizeof(double));
        part = t + up16((size_t)N * sizeof(double));
        term = part + up16((size_t)splits * max_pieces(N, splits) * C * sizeof(double));
        bytes = term + up16((size_t)splits * C * sizeof(double));
    }
};

template <bool VEC>
void launch_rows(hipStream_t st, const float* logits, double* lse, double* t, int N, int C) {
    const dim3 grid(std::min(ceil_rows(N, kRowWaves), kMaxGridX)), block(kThreads);
    if (C <= 256) hipLaunchKernelGGL((iscore_row_kernel<1, VEC>), grid, block, 0, st, logits, lse, t, N, C);
    else if (C <= 512) hipLaunchKernelGGL((iscore_row_kernel<2, VEC>), grid, block, 0, st, logits, lse, t, N, C);
    else if (C <= 1024) hipLaunchKernelGGL((iscore_row_kernel<4, VEC>), grid, block, 0, st, logits, lse, t, N, C);
    else if (C <= 2048) hipLaunchKernelGGL((iscore_row_kernel<8, VEC>), grid, block, 0, st, logits, lse, t, N, C);
    else hipLaunchKernelGGL((iscore_row_kernel<16, VEC>), grid, block, 0, st, logits, lse, t, N, C);
}

}  // namespace

extern "C" size_t agan_inception_score_ws_bytes(int N, int C, int splits) {
    return in_domain(N, C, splits) ? Workspace(N, C, splits).bytes : 0;
}

extern "C" int agan_inception_score(const float* logits, int N, int C, int splits, double* scores, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(N >= 1, "inception_score: N %d rows", N);
    AGAN_REQUIRE(C >= 1 && C <= kMaxClasses, "inception_score: C %d outside 1..%d", C, kMaxClasses);
    AGAN_REQUIRE((long long)N * C < (1ll << 31), "inception_score: N * C = %lld is 2^31 or more", (long long)N * C);
    AGAN_REQUIRE(splits >= 1 && splits <= std::min(N, kMaxSplits), "inception_score: %d splits outside 1..min(N = %d, %d)", splits, N, kMaxSplits);
    AGAN_REQUIRE(logits && scores, "inception_score: null pointer");
    const Workspace w(N, C, splits);
    AGAN_REQUIRE(ws, "inception_score: no workspace (agan_inception_score_ws_bytes: %zu bytes)", w.bytes);
    if (int e = check_ws("inception_score", w.bytes, ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    char* base = static_cast<char*>(ws);
    double* lse = reinterpret_cast<double*>(base + w.lse);
    double* t = reinterpret_cast<double*>(base + w.t);
    double* part = reinterpret_cast<double*>(base + w.part);
    double* term = reinterpret_cast<double*>(base + w.term);
    // 16-byte loads need whole float4s per row and an aligned base (checked, not assumed)
    if (C % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0) launch_rows<true>(st, logits, lse, t, N, C);
    else launch_rows<false>(st, logits, lse, t, N, C);
    const int P = max_pieces(N, splits);
    hipLaunchKernelGGL(iscore_col_kernel, dim3(std::min(P, kMaxGridX), cdiv(C, kThreads), splits), dim3(kThreads), 0, st, logits, lse, part, N, C,
                       splits, P);
    hipLaunchKernelGGL(iscore_class_kernel, dim3(cdiv(C, kClassThreads), splits), dim3(kClassThreads), 0, st, part, term, N, C, splits, P);
    hipLaunchKernelGGL(iscore_finish_kernel, dim3(splits), dim3(kThreads), 0, st, term, t, scores, N, C, splits);
    return check_launch("inception_score");
}
