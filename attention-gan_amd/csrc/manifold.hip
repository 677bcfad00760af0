// Reductions over the pairwise geometry of two feature sets (include/agan.h: agan_knn_radius / agan_manifold_scan / agan_poly_kernel_sum;
// evaluation.py: manifold_metrics, kernel_distance).  The n x m matrix of distances or kernel values never exists in memory.
//
// ONE SKELETON, THREE EPILOGUES.  A workgroup (4 waves, 2 x 2) owns kRows = 128 QUERY rows and walks the REFERENCE rows in chunks of
// kRefs = 128; per chunk the contraction R_chunk . Q_tile^T runs over D in stages of kStep = 32 columns through k-major LDS images on
// v_mfma_f32_32x32x2_f32 (mfma_tile.h, shared with kmeans.hip's assign kernel), the next stage's global loads in flight while the
// current one multiplies.  The references are the A operand and the queries the B operand: every accumulator register of a lane
// belongs to ONE query row per tile column (row = lane & 31), and the lane meets that row's references in ascending index order.  The
// epilogue object keeps its per-row state in registers through every chunk (all indices are compile-time after unrolling) and sees
// each (query row, reference, dot product) exactly once:
//   * KnnEpilogue:   d2 = max(0, |q|^2 + |r|^2 - 2 q.r); the 8 smallest d2 of the row, the row itself skipped BY INDEX, as a sorted
//                    register list under an unrolled min/max insertion.  The four partial lists of a row (two lane halves, two waves
//                    along the references) are merged as multisets by the same insertion, so the k-th smallest does not depend on the
//                    tiling.  k <= 8 is a run-time choice of the list's entry at the very end.
//   * ScanEpilogue:  count += d2 <= rad2[ref] (the chunk's radii sit in LDS beside its norms; without radii they read -1 and nothing
//                    counts), and the running (min d2, argmin) on strict <; the four partial winners merge by (d2, index): the lowest
//                    index wins a tie whatever the tiling.
//   * PolyEpilogue:  ((double)q.r / D + 1)^3 added to the lane's fp64 sum in the fixed order of the walk: the dot product is the fp32
//                    MFMA's, everything after it is fp64 ("convert after").  Lanes, then waves, are added in index order into the
//                    workgroup's partial in the workspace; a one-workgroup pass adds the partials in one fixed order.
// THE GRID.  blocks of 128 query rows x ranges of whole reference chunks (Split: one range when the row blocks alone fill the chip, else
// as many as keep the grid within 512 workgroups -- a function of the shape alone).  Every workgroup leaves its rows' partial result
// for its range in the workspace and a small pass per entry merges the ranges by the same rules: lists as multisets, counts added,
// winners by (d2, index), fp64 partials in index order.
// Squared norms come from a pass of their own (one wave per row, one fixed order).  Tails in rows and D read zeros and are masked by
// index in the epilogue.  No address depends on feature data; no atomics; the same bits on every run.
#include <algorithm>

#include "mfma_tile.h"

namespace {
using namespace agan;

constexpr int kThreads = kTileThreads;
constexpr int kRows = 128;             // query rows per workgroup
constexpr int kRefs = 128;             // reference rows per chunk
constexpr int WR = 2, WC = 2;          // waves along the queries / along the references
constexpr int TR = 2, TC = 2;          // 32 x 32 tiles per wave along the queries / along the references
constexpr int kParts = 2 * WC;         // partial results per query row: two lane halves x WC waves
constexpr int kMaxDim = 4096;          // largest D
constexpr int kMaxK = 8;               // largest k (the length of the register list)
static_assert(WR * WC * kWave == kThreads && WR * TR * 32 == kRows && WC * TC * 32 == kRefs, "tiling");

__global__ __launch_bounds__(kThreads) void row_norm_kernel(const float* __restrict__ x, float* __restrict__ norm, int n, int D) {
    const int row = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    if (row >= n) return;                                           // (a whole wave)
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int d = lane; d < D; d += kWave) { const float v = x[(size_t)row * D + d]; s = fmaf(v, v, s); }
    s = wave_sum(s);
    if (lane == 0) norm[row] = s;
}

struct Lane {
    int wr, wc, half, l32;
    __device__ __forceinline__ Lane() {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        wr = wave / WC, wc = wave % WC, half = lane >> 5, l32 = lane & 31;
    }
    __device__ __forceinline__ int row(int r) const { return (wr * TR + r) * 32 + l32; }      // the lane's query row r, within the workgroup
    __device__ __forceinline__ int part() const { return wc * 2 + half; }
};

// Walks every (query row of this workgroup, reference in [c_lo, c_hi)) pair once.  epi.stage(c0) runs once per chunk between two barriers (LDS that the
// epilogue reads per reference is filled there); epi.element(r, cl, dot) sees reference c0 + cl of the lane's query row r.
template <bool VEC, class Epi>
__device__ __forceinline__ void contract(const float* __restrict__ q, const float* __restrict__ ref, int m, int n, int D, int row0, int c_lo,
                                         int c_hi, float* qs, float* rs, const Lane& ln, Epi& epi) {
    const int steps = cdiv(D, kStep);
    TileRegs<kRows, VEC> qr;
    TileRegs<kRefs, VEC> rr;
    for (int c0 = c_lo; c0 < c_hi; c0 = c_hi - c0 > kRefs ? c0 + kRefs : c_hi) {          // (c0 + kRefs may pass 2^31)
        f32x16 acc[TC][TR];
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int r = 0; r < TR; ++r) acc[a][r] = f32x16{0};
        qr.load(q, m, D, row0, 0);
        rr.load(ref, n, D, c0, 0);
        for (int s = 0; s < steps; ++s) {
            __syncthreads();                                       // the previous stage's LDS reads and the previous chunk's epilogue are done
            qr.store(qs);
            rr.store(rs);
            if (s == 0) epi.stage(c0);
            __syncthreads();
            if (s + 1 < steps) {
                qr.load(q, m, D, row0, (s + 1) * kStep);
                rr.load(ref, n, D, c0, (s + 1) * kStep);
            }
            mfma_stage<kRefs, kRows, TC, TR>(rs, qs, ln.wc * TC, ln.wr * TR, ln.half, ln.l32, acc);
        }
#pragma unroll
        for (int r = 0; r < TR; ++r)
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) epi.element(r, c0, (ln.wc * TC + i) * 32 + mfma_a_row(e, ln.half), acc[i][r][e]);
    }
}

// keeps list[0] <= ... <= list[kMaxK - 1], the kMaxK smallest values inserted so far
__device__ __forceinline__ void insert_sorted(float (&list)[kMaxK], float v) {
#pragma unroll
    for (int s = 0; s < kMaxK; ++s) {
        const float lo = fminf(list[s], v);
        v = fmaxf(list[s], v);
        list[s] = lo;
    }
}

__device__ __forceinline__ float dist2(float qn, float rn, float dot) { return fmaxf(0.f, fmaf(-2.f, dot, qn + rn)); }

// ---------------------------------------------------------------------------------------------------------------------------------
// k-th nearest neighbour radius
// ---------------------------------------------------------------------------------------------------------------------------------
struct KnnEpilogue {
    const float* __restrict__ norm;
    float* rn_s;
    int n, row0;
    Lane ln;
    float qn[TR];
    float list[TR][kMaxK];
    __device__ __forceinline__ KnnEpilogue(const float* norm_, float* rn_s_, int n_, int row0_, const Lane& ln_)
        : norm(norm_), rn_s(rn_s_), n(n_), row0(row0_), ln(ln_) {
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            qn[r] = ln.row(r) < n - row0 ? norm[row0 + ln.row(r)] : 0.f;
#pragma unroll
            for (int s = 0; s < kMaxK; ++s) list[r][s] = INFINITY;
        }
    }
    __device__ __forceinline__ void stage(int c0) {
        const int t = threadIdx.x;
        if (t < kRefs) rn_s[t] = t < n - c0 ? norm[c0 + t] : 0.f;
    }
    __device__ __forceinline__ void element(int r, int c0, int cl, float dot) {
        const float d2 = dist2(qn[r], rn_s[cl], dot);
        if (cl < n - c0 && c0 + cl != row0 + ln.row(r) && d2 < list[r][kMaxK - 1]) insert_sorted(list[r], d2);
    }
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void knn_kernel(const float* __restrict__ x, const float* __restrict__ norm, float* __restrict__ part,
                                                       int n, int D, int refs_per_split) {
    __shared__ float qs[kStep * (kRows + kPad)];
    __shared__ float rs[kStep * (kRefs + kPad)];
    __shared__ float rn_s[kRefs];
    __shared__ float cand[kParts][kMaxK][kRows];
    const Lane ln;
    const int row0 = blockIdx.x * kRows;
    const int c_lo = blockIdx.y * refs_per_split;                  // (a multiple of kRefs below n: Split)
    KnnEpilogue epi(norm, rn_s, n, row0, ln);
    contract<VEC>(x, x, n, n, D, row0, c_lo, min(n - c_lo, refs_per_split) + c_lo, qs, rs, ln, epi);
#pragma unroll
    for (int r = 0; r < TR; ++r)
#pragma unroll
        for (int s = 0; s < kMaxK; ++s) cand[ln.part()][s][ln.row(r)] = epi.list[r][s];
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kRows && t < n - row0) {
        float list[kMaxK];
#pragma unroll
        for (int s = 0; s < kMaxK; ++s) list[s] = cand[0][s][t];
#pragma unroll
        for (int p = 1; p < kParts; ++p)
#pragma unroll
            for (int s = 0; s < kMaxK; ++s) insert_sorted(list, cand[p][s][t]);
#pragma unroll
        for (int s = 0; s < kMaxK; ++s) part[((size_t)blockIdx.y * kMaxK + s) * n + row0 + t] = list[s];       // part[split][slot][row]
    }
}

// merges the splits' lists of a row (as multisets again) and picks the k-th smallest
__global__ __launch_bounds__(kThreads) void knn_final_kernel(const float* __restrict__ part, float* __restrict__ rad2, int n, int splits, int k) {
    const int row = blockIdx.x * kThreads + threadIdx.x;
    if (row >= n) return;
    float list[kMaxK];
#pragma unroll
    for (int s = 0; s < kMaxK; ++s) list[s] = part[(size_t)s * n + row];
    for (int p = 1; p < splits; ++p)
#pragma unroll
        for (int s = 0; s < kMaxK; ++s) insert_sorted(list, part[((size_t)p * kMaxK + s) * n + row]);
    float out = list[0];
#pragma unroll
    for (int s = 1; s < kMaxK; ++s) out = (s == k - 1) ? list[s] : out;
    rad2[row] = out;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// scan of queries against references with radii
// ---------------------------------------------------------------------------------------------------------------------------------
struct ScanEpilogue {
    const float* __restrict__ rnorm;
    const float* __restrict__ rad2;                                 // may be null
    float *rn_s, *rad_s;
    int m, n, row0;
    Lane ln;
    float qn[TR], best[TR];
    int count[TR], best_j[TR];
    __device__ __forceinline__ ScanEpilogue(const float* qnorm, const float* rnorm_, const float* rad2_, float* rn_s_, float* rad_s_, int m_,
                                            int n_, int row0_, const Lane& ln_)
        : rnorm(rnorm_), rad2(rad2_), rn_s(rn_s_), rad_s(rad_s_), m(m_), n(n_), row0(row0_), ln(ln_) {
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            qn[r] = ln.row(r) < m - row0 ? qnorm[row0 + ln.row(r)] : 0.f;
            best[r] = INFINITY, best_j[r] = 0, count[r] = 0;
        }
    }
    __device__ __forceinline__ void stage(int c0) {
        const int t = threadIdx.x;
        if (t < kRefs) {
            const bool in = t < n - c0;
            rn_s[t] = in ? rnorm[c0 + t] : 0.f;
            rad_s[t] = (in && rad2) ? rad2[c0 + t] : -1.f;         // d2 >= 0: -1 counts nothing
        }
    }
    __device__ __forceinline__ void element(int r, int c0, int cl, float dot) {
        const float d2 = dist2(qn[r], rn_s[cl], dot);
        if (cl < n - c0) {
            count[r] += d2 <= rad_s[cl];
            if (d2 < best[r]) best[r] = d2, best_j[r] = c0 + cl;
        }
    }
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void scan_kernel(const float* __restrict__ q, const float* __restrict__ ref, const float* __restrict__ qnorm,
                                                        const float* __restrict__ rnorm, const float* __restrict__ rad2,
                                                        int32_t* __restrict__ part_n, float* __restrict__ part_d, int32_t* __restrict__ part_j,
                                                        int m, int n, int D, int refs_per_split) {
    __shared__ float qs[kStep * (kRows + kPad)];
    __shared__ float rs[kStep * (kRefs + kPad)];
    __shared__ float rn_s[kRefs];
    __shared__ float rad_s[kRefs];
    __shared__ float cand_d[kParts][kRows];
    __shared__ int cand_j[kParts][kRows];
    __shared__ int cand_n[kParts][kRows];
    const Lane ln;
    const int row0 = blockIdx.x * kRows;
    const int c_lo = blockIdx.y * refs_per_split;
    ScanEpilogue epi(qnorm, rnorm, rad2, rn_s, rad_s, m, n, row0, ln);
    contract<VEC>(q, ref, m, n, D, row0, c_lo, min(n - c_lo, refs_per_split) + c_lo, qs, rs, ln, epi);
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        cand_d[ln.part()][ln.row(r)] = epi.best[r];
        cand_j[ln.part()][ln.row(r)] = epi.best_j[r];
        cand_n[ln.part()][ln.row(r)] = epi.count[r];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kRows && t < m - row0) {
        float d = cand_d[0][t];
        int j = cand_j[0][t], c = cand_n[0][t];
#pragma unroll
        for (int p = 1; p < kParts; ++p) {
            const float dp = cand_d[p][t];
            const int jp = cand_j[p][t];
            if (dp < d || (dp == d && jp < j)) d = dp, j = jp;
            c += cand_n[p][t];
        }
        const size_t o = (size_t)blockIdx.y * m + row0 + t;         // part_*[split][row]
        part_n[o] = c;
        part_d[o] = d;
        part_j[o] = j;
    }
}

// adds the splits' counts of a row and merges their winners by (d2, index)
__global__ __launch_bounds__(kThreads) void scan_final_kernel(const int32_t* __restrict__ part_n, const float* __restrict__ part_d,
                                                              const int32_t* __restrict__ part_j, int32_t* __restrict__ count,
                                                              float* __restrict__ near_d2, int32_t* __restrict__ near_idx, int m, int splits) {
    const int row = blockIdx.x * kThreads + threadIdx.x;
    if (row >= m) return;
    int c = part_n[row], j = part_j[row];
    float d = part_d[row];
    for (int p = 1; p < splits; ++p) {
        const size_t o = (size_t)p * m + row;
        const float dp = part_d[o];
        const int jp = part_j[o];
        if (dp < d || (dp == d && jp < j)) d = dp, j = jp;
        c += part_n[o];
    }
    count[row] = c;
    near_d2[row] = d;
    near_idx[row] = j;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sum of the cubic polynomial kernel
// ---------------------------------------------------------------------------------------------------------------------------------
struct PolyEpilogue {
    int n, m, row0, skip_diagonal;
    double dim, sum;
    Lane ln;
    __device__ __forceinline__ PolyEpilogue(int n_, int m_, int D, int row0_, int skip, const Lane& ln_)
        : n(n_), m(m_), row0(row0_), skip_diagonal(skip), dim((double)D), sum(0.0), ln(ln_) {}
    __device__ __forceinline__ void stage(int) {}
    __device__ __forceinline__ void element(int r, int c0, int cl, float dot) {
        const double v = (double)dot / dim + 1.0;
        const bool in = ln.row(r) < n - row0 && cl < m - c0 && !(skip_diagonal && c0 + cl == row0 + ln.row(r));
        sum += in ? v * v * v : 0.0;
    }
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void poly_kernel(const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ partial,
                                                        int n, int m, int D, int skip_diagonal, int refs_per_split) {
    __shared__ float qs[kStep * (kRows + kPad)];
    __shared__ float rs[kStep * (kRefs + kPad)];
    __shared__ double red[kThreads / kWave];
    const Lane ln;
    const int row0 = blockIdx.x * kRows;
    const int c_lo = blockIdx.y * refs_per_split;
    PolyEpilogue epi(n, m, D, row0, skip_diagonal, ln);
    contract<VEC>(x, y, n, m, D, row0, c_lo, min(m - c_lo, refs_per_split) + c_lo, qs, rs, ln, epi);
    const double s = wave_sum_d(epi.sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int w = 0; w < kThreads / kWave; ++w) total += red[w];
        partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
    }
}

// thread t adds partials t, t + 256, ... in index order; the threads' sums are then added by a fixed tree
__global__ __launch_bounds__(kThreads) void poly_final_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
    __shared__ double red[kThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kThreads) s += partial[i];
    block_tree_sum_d<kThreads>(s, red);
    if (threadIdx.x == 0) *out = red[0];
}

bool rows_in_domain(int n, int D) { return n >= 1 && D >= 1 && D <= kMaxDim && (long long)n * D < (1ll << 31); }
bool knn_in_domain(int n, int D, int k) { return k >= 1 && k <= kMaxK && n >= k + 1 && rows_in_domain(n, D); }

// 16-byte loads need whole float4s per row and aligned bases (checked, not assumed)
bool can_vec(int D, const void* a, const void* b) {
    return D % 4 == 0 && (reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 16 == 0;
}

// The grid: `blocks` blocks of kRows query rows x `splits` ranges of `refs` reference rows (whole chunks).  One range per block of query
// rows when those alone fill the chip; otherwise as many as keep the grid within kTargetGroups workgroups, all resident at once.  A
// function of the shape alone: the same grid, and the same order of every sum, on every run.
constexpr int kTargetGroups = 512;
struct Split {
    int blocks, splits, refs;
    Split(int rows, int n_refs) {
        blocks = cdiv(rows, kRows);
        const int chunks = cdiv(n_refs, kRefs);
        const int want = std::max(1, std::min(chunks, kTargetGroups / blocks));
        const int per = cdiv(chunks, want);
        splits = cdiv(chunks, per);                                 // no empty range
        refs = per * kRefs;
    }
};

void launch_norm(hipStream_t st, const float* x, float* norm, int n, int D) {
    hipLaunchKernelGGL(row_norm_kernel, dim3(cdiv(n, kThreads / kWave)), dim3(kThreads), 0, st, x, norm, n, D);
}

}  // namespace

extern "C" size_t agan_knn_radius_ws_bytes(int n, int D, int k) {
    return knn_in_domain(n, D, k) ? up16((size_t)n * sizeof(float)) + up16((size_t)Split(n, n).splits * kMaxK * n * sizeof(float)) : 0;
}

extern "C" int agan_knn_radius(const float* x, int n, int D, int k, float* rad2, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(k >= 1 && k <= kMaxK, "knn_radius: k %d outside 1..%d", k, kMaxK);
    AGAN_REQUIRE(n >= k + 1, "knn_radius: n %d rows have no %d-th neighbour", n, k);
    AGAN_REQUIRE(D >= 1 && D <= kMaxDim, "knn_radius: D %d outside 1..%d", D, kMaxDim);
    AGAN_REQUIRE((long long)n * D < (1ll << 31), "knn_radius: n * D = %lld is 2^31 or more", (long long)n * D);
    AGAN_REQUIRE(x && rad2, "knn_radius: null pointer");
    const size_t need = agan_knn_radius_ws_bytes(n, D, k);
    AGAN_REQUIRE(ws, "knn_radius: no workspace (agan_knn_radius_ws_bytes: %zu bytes)", need);
    if (int e = check_ws("knn_radius", need, ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    const Split sp(n, n);
    float* norm = static_cast<float*>(ws);
    float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + up16((size_t)n * sizeof(float)));
    launch_norm(st, x, norm, n, D);
    const dim3 grid(sp.blocks, sp.splits), block(kThreads);
    if (can_vec(D, x, x)) hipLaunchKernelGGL(knn_kernel<true>, grid, block, 0, st, x, norm, part, n, D, sp.refs);
    else hipLaunchKernelGGL(knn_kernel<false>, grid, block, 0, st, x, norm, part, n, D, sp.refs);
    hipLaunchKernelGGL(knn_final_kernel, dim3(cdiv(n, kThreads)), block, 0, st, part, rad2, n, sp.splits, k);
    return check_launch("knn_radius");
}

extern "C" size_t agan_manifold_scan_ws_bytes(int m, int n, int D) {
    if (!rows_in_domain(m, D) || !rows_in_domain(n, D)) return 0;
    return up16((size_t)m * sizeof(float)) + up16((size_t)n * sizeof(float)) + 3 * up16((size_t)Split(m, n).splits * m * sizeof(float));
}

extern "C" int agan_manifold_scan(const float* q, const float* ref, const float* rad2, int m, int n, int D, int32_t* count, float* near_d2,
                                  int32_t* near_idx, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(m >= 1 && n >= 1, "manifold_scan: bad shape (m %d, n %d)", m, n);
    AGAN_REQUIRE(D >= 1 && D <= kMaxDim, "manifold_scan: D %d outside 1..%d", D, kMaxDim);
    AGAN_REQUIRE((long long)m * D < (1ll << 31) && (long long)n * D < (1ll << 31), "manifold_scan: m * D = %lld or n * D = %lld is 2^31 or more",
                 (long long)m * D, (long long)n * D);
    AGAN_REQUIRE(q && ref && count && near_d2 && near_idx, "manifold_scan: null pointer");
    const size_t need = agan_manifold_scan_ws_bytes(m, n, D);
    AGAN_REQUIRE(ws, "manifold_scan: no workspace (agan_manifold_scan_ws_bytes: %zu bytes)", need);
    if (int e = check_ws("manifold_scan", need, ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    const Split sp(m, n);
    const size_t part_bytes = up16((size_t)sp.splits * m * sizeof(float));
    char* base = static_cast<char*>(ws);
    float* qnorm = reinterpret_cast<float*>(base);
    float* rnorm = reinterpret_cast<float*>(base + up16((size_t)m * sizeof(float)));
    char* parts = base + up16((size_t)m * sizeof(float)) + up16((size_t)n * sizeof(float));
    int32_t* part_n = reinterpret_cast<int32_t*>(parts);
    float* part_d = reinterpret_cast<float*>(parts + part_bytes);
    int32_t* part_j = reinterpret_cast<int32_t*>(parts + 2 * part_bytes);
    launch_norm(st, q, qnorm, m, D);
    launch_norm(st, ref, rnorm, n, D);
    const dim3 grid(sp.blocks, sp.splits), block(kThreads);
    if (can_vec(D, q, ref))
        hipLaunchKernelGGL(scan_kernel<true>, grid, block, 0, st, q, ref, qnorm, rnorm, rad2, part_n, part_d, part_j, m, n, D, sp.refs);
    else
        hipLaunchKernelGGL(scan_kernel<false>, grid, block, 0, st, q, ref, qnorm, rnorm, rad2, part_n, part_d, part_j, m, n, D, sp.refs);
    hipLaunchKernelGGL(scan_final_kernel, dim3(cdiv(m, kThreads)), block, 0, st, part_n, part_d, part_j, count, near_d2, near_idx, m, sp.splits);
    return check_launch("manifold_scan");
}

extern "C" size_t agan_poly_kernel_sum_ws_bytes(int n, int m, int D) {
    if (!rows_in_domain(n, D) || !rows_in_domain(m, D)) return 0;
    const Split sp(n, m);
    return up16((size_t)sp.blocks * sp.splits * sizeof(double));
}

extern "C" int agan_poly_kernel_sum(const float* x, const float* y, int n, int m, int D, int exclude_diagonal, double* out, void* ws,
                                    size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(n >= 1 && m >= 1, "poly_kernel_sum: bad shape (n %d, m %d)", n, m);
    AGAN_REQUIRE(D >= 1 && D <= kMaxDim, "poly_kernel_sum: D %d outside 1..%d", D, kMaxDim);
    AGAN_REQUIRE((long long)n * D < (1ll << 31) && (long long)m * D < (1ll << 31), "poly_kernel_sum: n * D = %lld or m * D = %lld is 2^31 or more",
                 (long long)n * D, (long long)m * D);
    AGAN_REQUIRE(!exclude_diagonal || n == m, "poly_kernel_sum: exclude_diagonal with n %d != m %d", n, m);
    AGAN_REQUIRE(x && y && out, "poly_kernel_sum: null pointer");
    const size_t need = agan_poly_kernel_sum_ws_bytes(n, m, D);
    AGAN_REQUIRE(ws, "poly_kernel_sum: no workspace (agan_poly_kernel_sum_ws_bytes: %zu bytes)", need);
    if (int e = check_ws("poly_kernel_sum", need, ws, ws_bytes)) return e;
    hipStream_t st = as_stream(stream);
    double* partial = static_cast<double*>(ws);
    const Split sp(n, m);
    const dim3 grid(sp.blocks, sp.splits), block(kThreads);
    if (can_vec(D, x, y)) hipLaunchKernelGGL(poly_kernel<true>, grid, block, 0, st, x, y, partial, n, m, D, exclude_diagonal ? 1 : 0, sp.refs);
    else hipLaunchKernelGGL(poly_kernel<false>, grid, block, 0, st, x, y, partial, n, m, D, exclude_diagonal ? 1 : 0, sp.refs);
    hipLaunchKernelGGL(poly_final_kernel, dim3(1), block, 0, st, partial, sp.blocks * sp.splits, out);
    return check_launch("poly_kernel_sum");
}
