// The reductions at the end of a generator's evaluation (include/agan.h: agan_moments_* / agan_retrieval_rank; evaluation.py).
//
// MOMENTS.  sum[j] += sum_k x[k][j] and gram[i][j] += sum_k x[k][i] x[k][j] for j >= i, in fp64, over the n rows of one batch.  The
// contraction runs on v_mfma_f64_16x16x4_f64.  X [n, D] is k-major for BOTH operands (row k holds columns i and j side by side), so the
// LDS images are plain fp32 rows -- one of the tile's row-side columns, one of its column-side columns -- and lane l reads its A operand
// x[k = l >> 4][i = l & 15] and its B operand x[k = l >> 4][j = l & 15] with one ds_read_b32 each and converts AFTER the read (fp32 ->
// fp64 is exact, so is the product of two such values: only the additions round).  A workgroup is 2 x 2 waves, a wave owns TW x TW tiles
// of 16 x 16 and reuses its TW + TW converted operands over TW^2 MFMAs per k-step of 4 rows.  The C/D layout of the fp64 MFMA is not the
// fp32 one: col = lane & 15, row = (lane >> 4) + 4 reg.  Only workgroup tiles with tile_col >= tile_row exist (a linear grid over the
// upper triangle); what lies below the diagonal inside a diagonal tile is computed along and means nothing.  Each output element is
// owned by one lane of one workgroup, whose accumulator STARTS from gram and walks the rows in ascending order: one fixed chain of
// additions per element, no partial sums, no atomics.  The next chunk's global loads are in flight while the current one multiplies.
//   sum: pieces of kSumPiece rows are added per column in row order into the workspace, then onto sum in piece order.
//   finish: mean = sum / count; cov[i][j] = (gram[lo][hi] - count mean[lo] mean[hi]) / (count - 1) with lo = min(i, j), hi = max(i, j):
// both halves are computed from the same upper-triangle entry by the same expression, so cov is symmetric bit for bit.
//
// RETRIEVAL RANK.  A gather, not a GEMM: one wave per query keeps the query in registers (lane l holds elements 256 c + 4 l .. + 3 of
// every 256-element slice c), reads each candidate row of the bank with whole contiguous 1-KiB wave instructions (U rows in flight),
// and sums dot product and squared norm in one fixed order (per lane over its elements, then a butterfly over the lanes).  The
// candidate index is compared with [0, M) BEFORE it becomes an address; a query with a bad candidate gets rank -1 (and NaN for that
// score): the host cannot see device indices without a synchronisation, so the verdict travels in the output.
#include <math.h>

#include "agan_common.h"

namespace {
using namespace agan;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kMaxDim = 4096;          // largest D of either entry
constexpr int kMaxCand = 1024;         // largest R
constexpr int kChunk = 32;             // rows of X per LDS stage
constexpr int kPad = 16;               // LDS row pad (floats): consecutive rows of a 16-column operand read lie 16 banks apart
constexpr int kSumPiece = 512;         // rows per partial column sum
#ifndef AGAN_GRAM_TW
#define AGAN_GRAM_TW 2                 // 16 x 16 tiles per wave each way: 2 -> 64 x 64 workgroup tiles, 4 -> 128 x 128
#endif

// ---------------------------------------------------------------------------------------------------------------------------------
// moments
// ---------------------------------------------------------------------------------------------------------------------------------
template <int TW>
__global__ __launch_bounds__(kThreads) void gram_kernel(const float* __restrict__ x, double* __restrict__ gram, int n, int D) {
    constexpr int T = 32 * TW;                     // columns of the workgroup tile, each way
    constexpr int S = T + kPad;
    constexpr int NL = kChunk * T / kThreads;      // floats per thread and operand
    constexpr int RS = kThreads / T;               // rows between a thread's loads
    __shared__ float as[kChunk * S];
    __shared__ float bs[kChunk * S];

    const int nt = cdiv(D, T);
    int ti = 0, rest = blockIdx.x;                 // tile row ti holds the nt - ti tiles (ti, ti .. nt - 1)
    while (rest >= nt - ti) rest -= nt - ti, ++ti;
    const int i0 = ti * T, j0 = (ti + rest) * T;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l16 = lane & 15, lk = lane >> 4;

    f64x4 acc[TW][TW];
#pragma unroll
    for (int a = 0; a < TW; ++a)
#pragma unroll
        for (int b = 0; b < TW; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = i0 + (wr * TW + a) * 16 + lk + 4 * e, col = j0 + (wc * TW + b) * 16 + l16;
                acc[a][b][e] = (row < D && col < D) ? gram[(size_t)row * D + col] : 0.0;
            }

    const int lc = t % T, lr = t / T;              // this thread's column of the tile and its first row of a chunk
    const bool a_in = i0 + lc < D, b_in = j0 + lc < D;
    float ra[NL], rb[NL];
    auto load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int row = lr + RS * q;
            const bool in = row < n - k0;
            const float* p = x + (size_t)(k0 + row) * D;
            ra[q] = (in && a_in) ? p[i0 + lc] : 0.f;
            rb[q] = (in && b_in) ? p[j0 + lc] : 0.f;
        }
    };
    load(0);
    for (int k0 = 0; k0 < n; k0 += kChunk) {
        __syncthreads();                           // the previous chunk's LDS reads are done
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            as[(lr + RS * q) * S + lc] = ra[q];
            bs[(lr + RS * q) * S + lc] = rb[q];
        }
        __syncthreads();
        if (k0 + kChunk < n) load(k0 + kChunk);
        const int kend = min(kChunk, n - k0);      // (rows past n are zeros: whole k-steps of them are skipped, the last one's add 0)
        for (int ks = 0; ks < kend; ks += 4) {
            double a[TW], b[TW];
#pragma unroll
            for (int i = 0; i < TW; ++i) {
                a[i] = (double)as[(ks + lk) * S + (wr * TW + i) * 16 + l16];
                b[i] = (double)bs[(ks + lk) * S + (wc * TW + i) * 16 + l16];
            }
#pragma unroll
            for (int i = 0; i < TW; ++i)
#pragma unroll
                for (int j = 0; j < TW; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int a = 0; a < TW; ++a)
#pragma unroll
        for (int b = 0; b < TW; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = i0 + (wr * TW + a) * 16 + lk + 4 * e, col = j0 + (wc * TW + b) * 16 + l16;
                if (row < D && col < D) gram[(size_t)row * D + col] = acc[a][b][e];
            }
}

__global__ __launch_bounds__(kThreads) void sum_piece_kernel(const float* __restrict__ x, double* __restrict__ partial, int n, int D) {
    const int col = blockIdx.y * kThreads + threadIdx.x, piece = blockIdx.x;      // (pieces on x: there may be more than 65535)
    if (col >= D) return;
    const int lo = piece * kSumPiece, hi = lo + min(kSumPiece, n - lo);
    double s = 0.0;
    int k = lo;
    for (; k + 8 <= hi; k += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = x[(size_t)(k + u) * D + col];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)v[u];
    }
    for (; k < hi; ++k) s += (double)x[(size_t)k * D + col];
    partial[(size_t)piece * D + col] = s;
}

__global__ __launch_bounds__(kThreads) void sum_final_kernel(const double* __restrict__ partial, double* __restrict__ sum, int pieces, int D) {
    const int col = blockIdx.x * kThreads + threadIdx.x;
    if (col >= D) return;
    double s = sum[col];
    for (int p = 0; p < pieces; ++p) s += partial[(size_t)p * D + col];
    sum[col] = s;
}

__global__ __launch_bounds__(kThreads) void moments_finish_kernel(const double* __restrict__ sum, const double* __restrict__ gram, double count,
                                                                  int D, double* __restrict__ mean, double* __restrict__ cov) {
    const int i = blockIdx.y, j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= D) return;
    const int lo = min(i, j), hi = max(i, j);
    const double m_lo = sum[lo] / count, m_hi = sum[hi] / count;
    if (i == 0) mean[j] = m_hi;
    cov[(size_t)i * D + j] = count > 1.0 ? (gram[(size_t)lo * D + hi] - count * m_lo * m_hi) / (count - 1.0) : 0.0;
}

bool moments_in_domain(int n, int D) { return n >= 1 && D >= 1 && D <= kMaxDim && (long long)n * D < (1ll << 31); }

// ---------------------------------------------------------------------------------------------------------------------------------
// retrieval rank
// ---------------------------------------------------------------------------------------------------------------------------------
// elements 256 c + 4 lane .. + 3 of a row of D floats, c < NC; past D reads 0.  VEC: D % 4 == 0 and a 16-byte aligned table
template <int NC, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int D, int lane, float4 (&v)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int e = 256 * c + 4 * lane;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (VEC) {
            if (e < D) q = *reinterpret_cast<const float4*>(row + e);
        } else {
            if (e < D) q.x = row[e];
            if (e + 1 < D) q.y = row[e + 1];
            if (e + 2 < D) q.z = row[e + 2];
            if (e + 3 < D) q.w = row[e + 3];
        }
        v[c] = q;
    }
}

template <int NC>
__device__ __forceinline__ float lane_dot(const float4 (&a)[NC], const float4 (&b)[NC]) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        s = fmaf(a[c].x, b[c].x, s);
        s = fmaf(a[c].y, b[c].y, s);
        s = fmaf(a[c].z, b[c].z, s);
        s = fmaf(a[c].w, b[c].w, s);
    }
    return s;
}

template <int NC, bool VEC>
__global__ __launch_bounds__(kThreads) void retrieval_rank_kernel(const float* __restrict__ query, const float* __restrict__ bank,
                                                                  const int32_t* __restrict__ cand, int N, int M, int D, int R,
                                                                  float* __restrict__ scores, int32_t* __restrict__ rank) {
    constexpr int U = NC >= 4 ? 1 : 4 / NC;        // candidate rows in flight
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    if (i >= N) return;                            // (a whole wave)
    float4 q[NC];
    load_row<NC, VEC>(query + (size_t)i * D, D, lane, q);
    const float qn = sqrtf(wave_sum(lane_dot<NC>(q, q)));

    float s0 = 0.f;
    int worse = 0;
    bool bad = false;
    for (int base = 0; base < R; base += kWave) {
        const int cnt = min(kWave, R - base);
        const int c_lane = lane < cnt ? cand[(size_t)i * R + base + lane] : 0;
        float s_lane = 0.f;                        // the score of candidate base + lane
        for (int j = 0; j < cnt; j += U) {
            float4 b[U][NC];
            bool live[U], ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = __shfl(c_lane, min(j + u, cnt - 1), 64);
                live[u] = j + u < cnt;
                ok[u] = live[u] && c >= 0 && c < M;                      // checked before c is ever part of an address
                bad = bad || (live[u] && !ok[u]);
                load_row<NC, VEC>(bank + (size_t)(ok[u] ? c : 0) * D, ok[u] ? D : 0, lane, b[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float dot = wave_sum(lane_dot<NC>(q, b[u]));
                const float bn = sqrtf(wave_sum(lane_dot<NC>(b[u], b[u])));
                const float s = ok[u] ? dot / fmaxf(qn * bn, 1e-8f) : NAN;
                if (lane == j + u) s_lane = s;
                if (base + j + u == 0) s0 = s;
                else if (live[u]) worse += s >= s0;
            }
        }
        if (scores && lane < cnt) scores[(size_t)i * R + base + lane] = s_lane;
    }
    if (lane == 0) rank[i] = bad ? -1 : worse;
}

template <int NC>
void launch_retrieval(bool vec, hipStream_t st, const float* query, const float* bank, const int32_t* cand, int N, int M, int D, int R,
                      float* scores, int32_t* rank) {
    const dim3 grid(cdiv(N, kThreads / kWave)), block(kThreads);
    if (vec)
        hipLaunchKernelGGL((retrieval_rank_kernel<NC, true>), grid, block, 0, st, query, bank, cand, N, M, D, R, scores, rank);
    else
        hipLaunchKernelGGL((retrieval_rank_kernel<NC, false>), grid, block, 0, st, query, bank, cand, N, M, D, R, scores, rank);
}

}  // namespace

extern "C" size_t agan_moments_update_ws_bytes(int n, int D) {
    return moments_in_domain(n, D) ? up16((size_t)cdiv(n, kSumPiece) * D * sizeof(double)) : 0;
}

extern "C" int agan_moments_update(const float* x, int n, int D, double* sum, double* gram, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(n >= 1 && D >= 1, "moments_update: bad shape (n %d, D %d)", n, D);
    AGAN_REQUIRE(D <= kMaxDim, "moments_update: D %d above %d", D, kMaxDim);
    AGAN_REQUIRE((long long)n * D < (1ll << 31), "moments_update: n * D = %lld is 2^31 or more", (long long)n * D);
    AGAN_REQUIRE(x && sum && gram, "moments_update: null pointer");
    const size_t need = agan_moments_update_ws_bytes(n, D);
    AGAN_REQUIRE(ws, "moments_update: no workspace (agan_moments_update_ws_bytes: %zu bytes)", need);
    if (int e = check_ws("moments_update", need, ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    double* partial = static_cast<double*>(ws);
    const int pieces = cdiv(n, kSumPiece), col_blocks = cdiv(D, kThreads);
    hipLaunchKernelGGL(sum_piece_kernel, dim3(pieces, col_blocks), dim3(kThreads), 0, st, x, partial, n, D);
    hipLaunchKernelGGL(sum_final_kernel, dim3(col_blocks), dim3(kThreads), 0, st, partial, sum, pieces, D);
    const int nt = cdiv(D, 32 * AGAN_GRAM_TW);
    hipLaunchKernelGGL((gram_kernel<AGAN_GRAM_TW>), dim3(nt * (nt + 1) / 2), dim3(kThreads), 0, st, x, gram, n, D);
    return check_launch("moments_update");
}

extern "C" int agan_moments_finish(const double* sum, const double* gram, long long count, int D, double* mean, double* cov, void* stream) {
    AGAN_REQUIRE(D >= 1 && D <= kMaxDim, "moments_finish: D %d outside 1..%d", D, kMaxDim);
    AGAN_REQUIRE(count >= 1 && count < (1ll << 53), "moments_finish: count %lld outside 1..2^53", count);
    AGAN_REQUIRE(sum && gram && mean && cov, "moments_finish: null pointer");
    hipLaunchKernelGGL(moments_finish_kernel, dim3(cdiv(D, kThreads), D), dim3(kThreads), 0, as_stream(stream), sum, gram, (double)count, D,
                       mean, cov);
    return check_launch("moments_finish");
}

extern "C" int agan_retrieval_rank(const float* query, const float* bank, const int32_t* cand, int N, int M, int D, int R, float* scores,
                                   int32_t* rank, void* stream) {
    AGAN_REQUIRE(N >= 1 && M >= 1, "retrieval_rank: bad shape (N %d, M %d)", N, M);
    AGAN_REQUIRE(D >= 1 && D <= kMaxDim, "retrieval_rank: D %d outside 1..%d", D, kMaxDim);
    AGAN_REQUIRE(R >= 1 && R <= kMaxCand, "retrieval_rank: R %d outside 1..%d", R, kMaxCand);
    AGAN_REQUIRE(query && bank && cand && rank, "retrieval_rank: null pointer");
    hipStream_t st = as_stream(stream);
    // 16-byte loads need whole float4s per row and aligned bases (checked, not assumed)
    const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(bank)) % 16 == 0;
    const int slices = cdiv(D, 256);
    if (slices <= 1) launch_retrieval<1>(vec, st, query, bank, cand, N, M, D, R, scores, rank);
    else if (slices <= 2) launch_retrieval<2>(vec, st, query, bank, cand, N, M, D, R, scores, rank);
    else if (slices <= 4) launch_retrieval<4>(vec, st, query, bank, cand, N, M, D, R, scores, rank);
    else if (slices <= 8) launch_retrieval<8>(vec, st, query, bank, cand, N, M, D, R, scores, rank);
    else launch_retrieval<16>(vec, st, query, bank, cand, N, M, D, R, scores, rank);
    return check_launch("retrieval_rank");
}
