// Pixel-to-pixel attention of the generator's self-attention block (include/agan.h: agan_self_attn_*; utilities/layers.py:
// SelfAttention2d) and the block's learned gate (agan_scaled_residual_*).  fp32.  Per sample, with positions n (queries) and m (keys):
//     s[n, m] = scale * sum_d q[d, n] k[d, m]      p[n, :] = softmax_m s[n, :]      o[e, n] = sum_m v[e, m] p[n, m]
// Nothing of size N x M is ever written: the forward keeps a running maximum and sum per query (online softmax) and leaves
// lse[n] = log sum_m exp s[n, m]; the backward recomputes p = exp(s - lse) tile by tile.
//
// OPERANDS.  q [Dk, N], k [Dk, M], v [Dv, M] of a sample are channel rows contiguous over positions (NCHW), which is the k-major
// image v_mfma_f32_32x32x2_f32 wants: an LDS tile img[row][kLd] holds 32 positions of every channel row, zero past the channel count
// and past the last position.  Read "straight" (lane -> img[2 j + half][lane & 31]) it is an MFMA operand of a product that sums over
// channels; read "across" (lane -> img[32 t + (lane & 31)][position r]) it is the A operand of a product that sums over positions.
//
// ACCUMULATORS AS OPERANDS.  A 32 x 32 fp32 accumulator tile has its column on lane & 31 and its 16 registers on rows
// mfma_a_row(e, half).  Register e of such a tile X is the B operand of the MFMA that contracts rows mfma_a_row(e, 0) and
// mfma_a_row(e, 1) of X, so Y = A . X needs no lane movement and no LDS for X.  Each kernel therefore puts the index its SECOND
// product sums over on the registers of the first:
//   * forward and dq kernel: S^T[m, n] (keys on the registers, queries on the lane).  A query's maximum, sum, lse and delta are one
//     value per lane; the two lane halves see different keys and merge once per chunk (maximum) or once at the end (sum).
//     Then o[e, n] += v[e, m] p[m, n] and dq[d, n] += k[d, m] ds[m, n].
//   * dk / dv kernel: S[n, m] (queries on the registers, keys on the lane); lse and delta of the chunk's queries sit in LDS.
//     Then dv[e, m] += do[e, n] p[n, m] and dk[d, m] += q[d, n] ds[n, m].
// A workgroup of W waves owns 32 W positions of one sample (wave w the tile w) and walks the other axis in chunks of 32; W is 4, 2
// or 1, the largest whose LDS fits and that still gives 256 workgroups (a function of the shape alone).  A chunk's tiles pass through
// registers (StagedTile), so the next chunk's global loads are in flight while the current chunk multiplies.  Every output element is
// produced by one wave in one fixed order: no atomics, no hand-off between workgroups, the same bits on every run.  That costs the
// backward 7 MFMA products per tile pair (S and dP are formed in both kernels) instead of 5.
#include <algorithm>
#include <cmath>

#include "dispatch.h"
#include "mfma_tile.h"

using namespace agan;

namespace {

constexpr int kT = 32;                 // positions per tile and per chunk
constexpr int kLd = kT + 1;            // LDS row stride of a tile image (odd: the "across" read is at most a 2-way bank conflict)
constexpr int kMaxDk = 64, kMaxDv = 128;
constexpr size_t kLdsLimit = 65536;
constexpr int kTargetGroups = 256;

// ---- launch log: one integer per kernel launch of the last agan_self_attn_* / agan_scaled_residual_* call -------------------------
thread_local LaunchLog<8> g_log;
enum { kLogFwd = 1, kLogDelta, kLogBwdKV, kLogBwdQ, kLogGateFwd, kLogGateBwd, kLogGateFinal };
inline void log_launch(int kind, int W, int dkt, int dvt) { g_log.add(kind * 100000 + (W * kT) * 100 + dkt * 10 + dvt); }

// img[rows][kLd] <- columns c0 .. c0 + 31 of the first `valid` rows of src (row stride n_cols); everything else reads 0
// (the resident tiles, once per workgroup)
__device__ __forceinline__ void fill_tile(float* img, const float* __restrict__ src, int rows, int valid, int n_cols, long long c0) {
    const long long left = n_cols - c0;                                   // (<= 0 for a tile wholly past the end)
    for (int i = threadIdx.x; i < rows * kT; i += blockDim.x) {
        const int r = i >> 5, c = i & 31;
        img[r * kLd + c] = (r < valid && c < left) ? src[(size_t)r * n_cols + c0 + c] : 0.f;
    }
}

// The same tile by way of registers, so that the next chunk's global loads are in flight while the current chunk multiplies: load()
// fills up to MAXV values per thread of a workgroup of NT threads (enough for MAXV * NT / 32 image rows), store() writes the image.
template <int MAXV, int NT>
struct StagedTile {
    float v[MAXV];
    __device__ __forceinline__ void load(const float* __restrict__ src, int valid, int n_cols, long long c0) {
        const long long left = n_cols - c0;
#pragma unroll
        for (int u = 0; u < MAXV; ++u) {
            const int i = threadIdx.x + u * NT, r = i >> 5, c = i & 31;
            v[u] = (r < valid && c < left) ? src[(size_t)r * n_cols + c0 + c] : 0.f;
        }
    }
    __device__ __forceinline__ void store(float* img, int rows) const {
#pragma unroll
        for (int u = 0; u < MAXV; ++u) {
            const int i = threadIdx.x + u * NT;
            if (i < rows * kT) img[(i >> 5) * kLd + (i & 31)] = v[u];
        }
    }
};

// acc += sum over the image rows 0 .. 2 steps - 1 of a[row][i] b[row][j] (a: rows of the accumulator, b: its lanes)
__device__ __forceinline__ void mfma_rows(const float* a, const float* b, int steps, int half, int l32, f32x16& acc) {
    for (int j = 0; j < steps; ++j) {
        const int r = (2 * j + half) * kLd + l32;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[r], b[r], acc, 0, 0, 0);
    }
}

// acc[t] += a[32 t + i][r] x[r][j] over the 32 rows r of the accumulator tile x (a read "across").  BLOCKED: the 32 terms are summed
// on their own and added to acc once, so a sweep over L positions is a sum of L / 32 block sums instead of one chain of L terms (the
// backward sums signed terms over up to 2^31 / max(Dk, Dv) positions; one fp32 chain of 16384 missed the tests' bound)
template <int T, bool BLOCKED>
__device__ __forceinline__ void mfma_acc(const float* a, const f32x16& x, int half, int l32, f32x16 (&acc)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
        f32x16 part = BLOCKED ? f32x16{0} : acc[t];
#pragma unroll
        for (int e = 0; e < 16; ++e)
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(a[(t * kT + l32) * kLd + mfma_a_row(e, half)], x[e], part, 0, 0, 0);
        if (BLOCKED) acc[t] += part;
        else acc[t] = part;
    }
}

// a * b rounded on its own: never contracted into an fma with a following add
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// next chunk start (c0 + kT may pass 2^31)
__device__ __forceinline__ int next_chunk(int c0, int n) { return n - c0 > kT ? c0 + kT : n; }

// out[row][pos] = mul * acc for the rows below `rows` (pos is in range)
template <int T>
__device__ __forceinline__ void store_rows(float* __restrict__ out, int n_cols, int pos, int rows, int half, const f32x16 (&acc)[T], float mul) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = t * kT + mfma_a_row(e, half);
            if (row < rows) out[(size_t)row * n_cols + pos] = mul_rn(mul, acc[t][e]);
        }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W, int DVT>
__global__ __launch_bounds__(64 * W) void sa_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                        float* __restrict__ o, float* __restrict__ lse, int N, int M, int Dk, int Dv,
                                                        long long q_bs, long long k_bs, long long v_bs, long long o_bs, float scale, int blocks) {
    extern __shared__ float smem[];
    const int DkP = (Dk + 1) & ~1;
    float* qs = smem;                           // [W][DkP][kLd]   resident
    float* ks = qs + W * DkP * kLd;             // [DkP][kLd]      chunk, read straight
    float* vs = ks + DkP * kLd;                 // [32 DVT][kLd]   chunk, read across
    const int b = blockIdx.x / blocks, n0 = (blockIdx.x % blocks) * (kT * W);
    const int wave = threadIdx.x >> 6, half = (threadIdx.x >> 5) & 1, l32 = threadIdx.x & 31;
    q += (size_t)b * q_bs, k += (size_t)b * k_bs, v += (size_t)b * v_bs, o += (size_t)b * o_bs;
#pragma unroll
    for (int w = 0; w < W; ++w) fill_tile(qs + w * DkP * kLd, q, DkP, Dk, N, (long long)n0 + w * kT);
    const float* qw = qs + wave * DkP * kLd;
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 acc[DVT];
#pragma unroll
    for (int t = 0; t < DVT; ++t) acc[t] = f32x16{0};
    StagedTile<kMaxDk / (2 * W), 64 * W> next_k;
    StagedTile<16 * DVT / W, 64 * W> next_v;
    next_k.load(k, Dk, M, 0);
    next_v.load(v, Dv, M, 0);
    for (int c0 = 0; c0 < M; c0 = next_chunk(c0, M)) {
        __syncthreads();                                            // the previous chunk's reads are done
        next_k.store(ks, DkP);
        next_v.store(vs, kT * DVT);
        __syncthreads();
        if (next_chunk(c0, M) < M) {                                // in flight while this chunk multiplies
            next_k.load(k, Dk, M, next_chunk(c0, M));
            next_v.load(v, Dv, M, next_chunk(c0, M));
        }
        f32x16 s = f32x16{0};
        mfma_rows(ks, qw, DkP / 2, half, l32, s);                   // s[e] = q . k of key c0 + mfma_a_row(e, half), query l32
        const int left = M - c0;
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[e] = mfma_a_row(e, half) < left ? mul_rn(s[e], scale) : -INFINITY;
            mx = fmaxf(mx, s[e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                     // key c0 is in range: finite from the first chunk on
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __expf(m_run - m_new);                  // 0 on the first chunk
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[e] = mfma_a_row(e, half) < left ? __expf(s[e] - m_new) : 0.f;      // a masked key adds exactly 0
            ps += s[e];
        }
        l_run = fmaf(l_run, alpha, ps);
        m_run = m_new;
        if (__any(alpha != 1.f)) {                                  // (wave-uniform; after a few chunks the maximum seldom moves)
#pragma unroll
            for (int t = 0; t < DVT; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t][e] *= alpha;
        }
        mfma_acc<DVT, false>(vs, s, half, l32, acc);                 // (rescaled every chunk: one chain)
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const int nl = wave * kT + l32;
    if (nl < N - n0) {
        const int n = n0 + nl;
#pragma unroll
        for (int t = 0; t < DVT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = t * kT + mfma_a_row(e, half);
                if (row < Dv) o[(size_t)row * N + n] = acc[t][e] / l_tot;
            }
        if (half == 0) lse[(size_t)b * N + n] = m_run + logf(l_tot);
    }
}

// delta[b, n] = sum_e do[e, n] o[e, n], one ascending fma chain (the order of the MFMA that forms dP)
__global__ __launch_bounds__(256) void sa_delta_kernel(const float* __restrict__ dout, const float* __restrict__ o, float* __restrict__ delta,
                                                       int N, int Dv, long long do_bs, long long o_bs, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = i / N, n = i % N;
    const float* d = dout + (size_t)b * do_bs + n;
    const float* y = o + (size_t)b * o_bs + n;
    float s = 0.f;
    for (int e = 0; e < Dv; ++e) s = fmaf(d[(size_t)e * N], y[(size_t)e * N], s);
    delta[i] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward: dk and dv.  The workgroup owns 32 W keys and sweeps the queries.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W, int DKT, int DVT>
__global__ __launch_bounds__(64 * W) void sa_bwd_kv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           const float* __restrict__ lse, const float* __restrict__ delta,
                                                           const float* __restrict__ dout, float* __restrict__ dk, float* __restrict__ dv,
                                                           int N, int M, int Dk, int Dv, long long q_bs, long long k_bs, long long v_bs,
                                                           long long do_bs, long long dk_bs, long long dv_bs, float scale, int blocks) {
    extern __shared__ float smem[];
    const int DkP = (Dk + 1) & ~1, DvP = (Dv + 1) & ~1;
    float* ks = smem;                           // [W][DkP][kLd]   resident
    float* vs = ks + W * DkP * kLd;             // [W][DvP][kLd]   resident
    float* qs = vs + W * DvP * kLd;             // [32 DKT][kLd]   chunk, read straight and across
    float* ds = qs + kT * DKT * kLd;            // [32 DVT][kLd]   chunk (do), read straight and across
    float* lse_s = ds + kT * DVT * kLd;         // [32]
    float* del_s = lse_s + kT;                  // [32]
    const int b = blockIdx.x / blocks, m0 = (blockIdx.x % blocks) * (kT * W);
    const int wave = threadIdx.x >> 6, half = (threadIdx.x >> 5) & 1, l32 = threadIdx.x & 31;
    q += (size_t)b * q_bs, k += (size_t)b * k_bs, v += (size_t)b * v_bs, dout += (size_t)b * do_bs;
    dk += (size_t)b * dk_bs, dv += (size_t)b * dv_bs, lse += (size_t)b * N, delta += (size_t)b * N;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        fill_tile(ks + w * DkP * kLd, k, DkP, Dk, M, (long long)m0 + w * kT);
        fill_tile(vs + w * DvP * kLd, v, DvP, Dv, M, (long long)m0 + w * kT);
    }
    const float* kw = ks + wave * DkP * kLd;
    const float* vw = vs + wave * DvP * kLd;
    const int ml = wave * kT + l32;
    const bool m_in = ml < M - m0;
    f32x16 acc_k[DKT], acc_v[DVT];
#pragma unroll
    for (int t = 0; t < DKT; ++t) acc_k[t] = f32x16{0};
#pragma unroll
    for (int t = 0; t < DVT; ++t) acc_v[t] = f32x16{0};
    StagedTile<16 * DKT / W, 64 * W> next_q;
    StagedTile<16 * DVT / W, 64 * W> next_do;
    float next_lse = 0.f, next_del = 0.f;                           // (threads 0..31: the chunk's queries)
    const auto load_chunk = [&](int c0) {
        next_q.load(q, Dk, N, c0);
        next_do.load(dout, Dv, N, c0);
        const bool in = (int)threadIdx.x < kT && (int)threadIdx.x < N - c0;
        next_lse = in ? lse[c0 + threadIdx.x] : 0.f;
        next_del = in ? delta[c0 + threadIdx.x] : 0.f;
    };
    load_chunk(0);
    for (int c0 = 0; c0 < N; c0 = next_chunk(c0, N)) {
        __syncthreads();
        next_q.store(qs, kT * DKT);
        next_do.store(ds, kT * DVT);
        if (threadIdx.x < kT) lse_s[threadIdx.x] = next_lse, del_s[threadIdx.x] = next_del;
        const int left = N - c0;
        __syncthreads();
        if (next_chunk(c0, N) < N) load_chunk(next_chunk(c0, N));   // in flight while this chunk multiplies
        f32x16 s = f32x16{0}, dp = f32x16{0};
        mfma_rows(qs, kw, DkP / 2, half, l32, s);                   // s[e]: query c0 + mfma_a_row(e, half), key l32
        mfma_rows(ds, vw, DvP / 2, half, l32, dp);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = mfma_a_row(e, half);
            const float p = (m_in && r < left) ? __expf(mul_rn(s[e], scale) - lse_s[r]) : 0.f;
            s[e] = p;
            dp[e] = p * (dp[e] - del_s[r]);
        }
        mfma_acc<DVT, true>(ds, s, half, l32, acc_v);                     // dv[e, m] += do[e, n] p[n, m]
        mfma_acc<DKT, true>(qs, dp, half, l32, acc_k);                    // dk[d, m] += q[d, n] ds[n, m]
    }
    if (m_in) {
        store_rows<DVT>(dv, M, m0 + ml, Dv, half, acc_v, 1.f);
        store_rows<DKT>(dk, M, m0 + ml, Dk, half, acc_k, scale);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward: dq.  The workgroup owns 32 W queries and sweeps the keys.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int W, int DKT>
__global__ __launch_bounds__(64 * W) void sa_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          const float* __restrict__ dout, float* __restrict__ dq, int N, int M, int Dk, int Dv,
                                                          long long q_bs, long long k_bs, long long v_bs, long long do_bs, long long dq_bs,
                                                          float scale, int blocks) {
    extern __shared__ float smem[];
    const int DkP = (Dk + 1) & ~1, DvP = (Dv + 1) & ~1;
    float* qs = smem;                           // [W][DkP][kLd]   resident
    float* ds = qs + W * DkP * kLd;             // [W][DvP][kLd]   resident (do)
    float* ks = ds + W * DvP * kLd;             // [32 DKT][kLd]   chunk, read straight and across
    float* vs = ks + kT * DKT * kLd;            // [DvP][kLd]      chunk, read straight
    const int b = blockIdx.x / blocks, n0 = (blockIdx.x % blocks) * (kT * W);
    const int wave = threadIdx.x >> 6, half = (threadIdx.x >> 5) & 1, l32 = threadIdx.x & 31;
    q += (size_t)b * q_bs, k += (size_t)b * k_bs, v += (size_t)b * v_bs, dout += (size_t)b * do_bs, dq += (size_t)b * dq_bs;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        fill_tile(qs + w * DkP * kLd, q, DkP, Dk, N, (long long)n0 + w * kT);
        fill_tile(ds + w * DvP * kLd, dout, DvP, Dv, N, (long long)n0 + w * kT);
    }
    const float* qw = qs + wave * DkP * kLd;
    const float* dw = ds + wave * DvP * kLd;
    const int nl = wave * kT + l32;
    const bool n_in = nl < N - n0;
    const float lse_n = n_in ? lse[(size_t)b * N + n0 + nl] : 0.f;
    const float del_n = n_in ? delta[(size_t)b * N + n0 + nl] : 0.f;
    f32x16 acc[DKT];
#pragma unroll
    for (int t = 0; t < DKT; ++t) acc[t] = f32x16{0};
    StagedTile<16 * DKT / W, 64 * W> next_k;
    StagedTile<kMaxDv / (2 * W), 64 * W> next_v;
    next_k.load(k, Dk, M, 0);
    next_v.load(v, Dv, M, 0);
    for (int c0 = 0; c0 < M; c0 = next_chunk(c0, M)) {
        __syncthreads();
        next_k.store(ks, kT * DKT);
        next_v.store(vs, DvP);
        __syncthreads();
        if (next_chunk(c0, M) < M) {                                // in flight while this chunk multiplies
            next_k.load(k, Dk, M, next_chunk(c0, M));
            next_v.load(v, Dv, M, next_chunk(c0, M));
        }
        f32x16 s = f32x16{0}, dp = f32x16{0};
        mfma_rows(ks, qw, DkP / 2, half, l32, s);                   // s[e]: key c0 + mfma_a_row(e, half), query l32
        mfma_rows(vs, dw, DvP / 2, half, l32, dp);
        const int left = M - c0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float p = (n_in && mfma_a_row(e, half) < left) ? __expf(mul_rn(s[e], scale) - lse_n) : 0.f;
            dp[e] = p * (dp[e] - del_n);
        }
        mfma_acc<DKT, true>(ks, dp, half, l32, acc);                      // dq[d, n] += k[d, m] ds[m, n]
    }
    if (n_in) store_rows<DKT>(dq, N, n0 + nl, Dk, half, acc, scale);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the gate: out = x + g[0] * y
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kGateThreads = 256;
constexpr int kGateMaxBlocks = 1024;
int gate_blocks(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>(cdivz(n, 4 * kGateThreads), kGateMaxBlocks)); }

__global__ __launch_bounds__(kGateThreads) void gate_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g,
                                                                float* __restrict__ out, size_t n) {
    const float gv = g[0];
    for (size_t i = (size_t)blockIdx.x * kGateThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kGateThreads)
        out[i] = add_rn(x[i], mul_rn(gv, y[i]));               // two roundings, as the torch statement
}

// dy = g[0] * dout; partial[block] = the block's part of sum dout * y: fp64 products, each thread in index order, then a fixed tree
__global__ __launch_bounds__(kGateThreads) void gate_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ y,
                                                                const float* __restrict__ g, float* __restrict__ dy, double* __restrict__ partial,
                                                                size_t n) {
    __shared__ double red[kGateThreads];
    const float gv = g[0];
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * kGateThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kGateThreads) {
        const float d = dout[i];
        dy[i] = mul_rn(gv, d);
        s += (double)d * (double)y[i];
    }
    block_tree_sum_d<kGateThreads>(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kGateThreads) void gate_final_kernel(const double* __restrict__ partial, int blocks, float* __restrict__ dg, int accumulate) {
    __shared__ double red[kGateThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kGateThreads) s += partial[i];
    block_tree_sum_d<kGateThreads>(s, red);
    if (threadIdx.x == 0) dg[0] = (float)((accumulate ? (double)dg[0] : 0.0) + red[0]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
int even(int d) { return (d + 1) & ~1; }
int dk_tiles(int Dk) { return Dk <= kT ? 1 : 2; }
int dv_tiles(int Dv) { return Dv <= kT ? 1 : Dv <= 2 * kT ? 2 : 4; }

size_t fwd_lds(int W, int Dk, int Dv) { return sizeof(float) * kLd * ((size_t)(W + 1) * even(Dk) + kT * dv_tiles(Dv)); }
size_t kv_lds(int W, int Dk, int Dv) {
    return sizeof(float) * (kLd * ((size_t)W * (even(Dk) + even(Dv)) + kT * dk_tiles(Dk) + kT * dv_tiles(Dv)) + 2 * kT);
}
size_t q_lds(int W, int Dk, int Dv) { return sizeof(float) * kLd * ((size_t)W * (even(Dk) + even(Dv)) + kT * dk_tiles(Dk) + even(Dv)); }

// waves per workgroup: the largest of 4, 2 whose LDS fits and that still gives kTargetGroups workgroups, else 1
template <class Lds>
int pick_waves(int B, int len, int Dk, int Dv, Lds lds) {
    for (int W = 4; W > 1; W >>= 1)
        if (lds(W, Dk, Dv) <= kLdsLimit && (long long)B * cdiv(len, kT * W) >= kTargetGroups) return W;
    return 1;
}

bool shape_ok(int B, int N, int M, int Dk, int Dv) {
    if (B < 1 || N < 1 || M < 1 || Dk < 1 || Dk > kMaxDk || Dv < 1 || Dv > kMaxDv) return false;
    const long long d = std::max(Dk, Dv);
    return (long long)B * N * d < (1ll << 31) && (long long)B * M * d < (1ll << 31);
}

int check_shape(const char* what, int B, int N, int M, int Dk, int Dv, float scale) {
    AGAN_REQUIRE(B >= 1 && N >= 1 && M >= 1, "%s: bad shape (B %d, N %d, M %d)", what, B, N, M);
    AGAN_REQUIRE(Dk >= 1 && Dk <= kMaxDk, "%s: Dk %d outside 1..%d", what, Dk, kMaxDk);
    AGAN_REQUIRE(Dv >= 1 && Dv <= kMaxDv, "%s: Dv %d outside 1..%d", what, Dv, kMaxDv);
    AGAN_REQUIRE(shape_ok(B, N, M, Dk, Dv), "%s: B * N * max(Dk, Dv) or B * M * max(Dk, Dv) is 2^31 or more", what);
    AGAN_REQUIRE(std::isfinite(scale), "%s: scale is not finite", what);
    return AGAN_OK;
}

int check_stride(const char* what, const char* name, long long bs, int rows, int len) {
    AGAN_REQUIRE(bs >= (long long)rows * len, "%s: batch stride of %s is %lld, below %d rows of %d", what, name, bs, rows, len);
    return AGAN_OK;
}

}  // namespace

extern "C" {

int agan_self_attn_last_launch(int* codes, int capacity) { return g_log.copy_out(codes, capacity); }

int agan_self_attn_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int N, int M, int Dk, int Dv, long long q_bs,
                       long long k_bs, long long v_bs, long long o_bs, float scale, void* stream) {
    g_log.reset();
    if (int e = check_shape("self_attn_fwd", B, N, M, Dk, Dv, scale)) return e;
    if (int e = check_stride("self_attn_fwd", "q", q_bs, Dk, N)) return e;
    if (int e = check_stride("self_attn_fwd", "k", k_bs, Dk, M)) return e;
    if (int e = check_stride("self_attn_fwd", "v", v_bs, Dv, M)) return e;
    if (int e = check_stride("self_attn_fwd", "o", o_bs, Dv, N)) return e;
    AGAN_REQUIRE(q && k && v && o && lse, "self_attn_fwd: null pointer");
    hipStream_t st = as_stream(stream);
    const int W = pick_waves(B, N, Dk, Dv, fwd_lds), T = dv_tiles(Dv), blocks = cdiv(N, kT * W);
    const size_t lds = fwd_lds(W, Dk, Dv);
    with_int<1, 2, 4>(W, [&](auto w) {
        with_int<1, 2, 4>(T, [&](auto t) {
            hipLaunchKernelGGL((sa_fwd_kernel<w(), t()>), dim3(B * blocks), dim3(64 * w()), lds, st, q, k, v, o, lse, N, M, Dk, Dv, q_bs, k_bs, v_bs,
                               o_bs, scale, blocks);
        });
    });
    log_launch(kLogFwd, W, 0, T);
    return check_launch("self_attn_fwd");
}

size_t agan_self_attn_bwd_ws_bytes(int B, int N, int M, int Dk, int Dv) {
    return shape_ok(B, N, M, Dk, Dv) ? up16((size_t)B * N * sizeof(float)) : 0;
}

int agan_self_attn_bwd(const float* q, const float* k, const float* v, const float* o, const float* lse, const float* dout, float* dq, float* dk,
                       float* dv, int B, int N, int M, int Dk, int Dv, long long q_bs, long long k_bs, long long v_bs, long long o_bs,
                       long long do_bs, long long dq_bs, long long dk_bs, long long dv_bs, float scale, void* ws, size_t ws_bytes, void* stream) {
    g_log.reset();
    const char* what = "self_attn_bwd";
    if (int e = check_shape(what, B, N, M, Dk, Dv, scale)) return e;
    if (int e = check_stride(what, "q", q_bs, Dk, N)) return e;
    if (int e = check_stride(what, "k", k_bs, Dk, M)) return e;
    if (int e = check_stride(what, "v", v_bs, Dv, M)) return e;
    if (int e = check_stride(what, "o", o_bs, Dv, N)) return e;
    if (int e = check_stride(what, "dout", do_bs, Dv, N)) return e;
    if (int e = check_stride(what, "dq", dq_bs, Dk, N)) return e;
    if (int e = check_stride(what, "dk", dk_bs, Dk, M)) return e;
    if (int e = check_stride(what, "dv", dv_bs, Dv, M)) return e;
    AGAN_REQUIRE(q && k && v && o && lse && dout && dq && dk && dv && ws, "self_attn_bwd: null pointer");
    if (int e = check_ws(what, agan_self_attn_bwd_ws_bytes(B, N, M, Dk, Dv), ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    float* delta = static_cast<float*>(ws);
    const int total = B * N;
    hipLaunchKernelGGL(sa_delta_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, dout, o, delta, N, Dv, do_bs, o_bs, total);
    log_launch(kLogDelta, 0, 0, 0);
    const int KT = dk_tiles(Dk), VT = dv_tiles(Dv);
    {
        const int W = pick_waves(B, M, Dk, Dv, kv_lds), blocks = cdiv(M, kT * W);
        const size_t lds = kv_lds(W, Dk, Dv);
        with_int<1, 2, 4>(W, [&](auto w) {
            with_int<1, 2>(KT, [&](auto kt) {
                with_int<1, 2, 4>(VT, [&](auto vt) {
                    hipLaunchKernelGGL((sa_bwd_kv_kernel<w(), kt(), vt()>), dim3(B * blocks), dim3(64 * w()), lds, st, q, k, v, lse, delta, dout, dk,
                                       dv, N, M, Dk, Dv, q_bs, k_bs, v_bs, do_bs, dk_bs, dv_bs, scale, blocks);
                });
            });
        });
        log_launch(kLogBwdKV, W, KT, VT);
    }
    {
        const int W = pick_waves(B, N, Dk, Dv, q_lds), blocks = cdiv(N, kT * W);
        const size_t lds = q_lds(W, Dk, Dv);
        with_int<1, 2, 4>(W, [&](auto w) {
            with_int<1, 2>(KT, [&](auto kt) {
                hipLaunchKernelGGL((sa_bwd_q_kernel<w(), kt()>), dim3(B * blocks), dim3(64 * w()), lds, st, q, k, v, lse, delta, dout, dq, N, M, Dk,
                                   Dv, q_bs, k_bs, v_bs, do_bs, dq_bs, scale, blocks);
            });
        });
        log_launch(kLogBwdQ, W, KT, 0);
    }
    return check_launch("self_attn_bwd");
}

int agan_scaled_residual_fwd(const float* x, const float* y, const float* g, float* out, size_t n, void* stream) {
    g_log.reset();
    AGAN_REQUIRE(n >= 1, "scaled_residual_fwd: no elements");
    AGAN_REQUIRE(x && y && g && out, "scaled_residual_fwd: null pointer");
    hipLaunchKernelGGL(gate_fwd_kernel, dim3(gate_blocks(n)), dim3(kGateThreads), 0, as_stream(stream), x, y, g, out, n);
    log_launch(kLogGateFwd, 0, 0, 0);
    return check_launch("scaled_residual_fwd");
}

size_t agan_scaled_residual_bwd_ws_bytes(size_t n) { return n >= 1 ? up16((size_t)gate_blocks(n) * sizeof(double)) : 0; }

int agan_scaled_residual_bwd(const float* dout, const float* y, const float* g, float* dy, float* dg, size_t n, int accumulate, void* ws,
                             size_t ws_bytes, void* stream) {
    g_log.reset();
    AGAN_REQUIRE(n >= 1, "scaled_residual_bwd: no elements");
    AGAN_REQUIRE(dout && y && g && dy && dg && ws, "scaled_residual_bwd: null pointer");
    if (int e = check_ws("scaled_residual_bwd", agan_scaled_residual_bwd_ws_bytes(n), ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    double* partial = static_cast<double*>(ws);
    const int blocks = gate_blocks(n);
    hipLaunchKernelGGL(gate_bwd_kernel, dim3(blocks), dim3(kGateThreads), 0, st, dout, y, g, dy, partial, n);
    log_launch(kLogGateBwd, 0, 0, 0);
    hipLaunchKernelGGL(gate_final_kernel, dim3(1), dim3(kGateThreads), 0, st, partial, blocks, dg, accumulate ? 1 : 0);
    log_launch(kLogGateFinal, 0, 0, 0);
    return check_launch("scaled_residual_bwd");
}

}  // extern "C"
