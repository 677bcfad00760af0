// Lloyd's k-means on the fp32 matrix cores (include/agan.h: agan_kmeans_assign / agan_kmeans_update; data/captions.py: kmeans).
//
// ASSIGN.  labels[i] = argmin_c (|c|^2 - 2 x_i.c), lowest c on a tie.  A workgroup (4 waves) owns kRows = 128 rows of X and walks the
// centroids in chunks; per chunk the contraction C_chunk . X_tile^T runs over D in steps of kStep = 32 columns staged through LDS
// (k-major images, so that lane l of a v_mfma_f32_32x32x2_f32 reads its [k][i = l & 31] operand with one ds_read_b32), the next step's
// global loads in flight while the current one multiplies.  The CENTROIDS are the A operand and the ROWS the B operand: an accumulator
// register then holds one centroid of the lane's own row (column = lane & 31), so the running (min, argmin) of a row is a plain
// register pair that lives through every chunk, and the N x K scores never leave the registers.  A lane sees its centroids in
// ascending order and takes a challenger on strict <; the 2 * WC partial winners of a row (two lane halves, WC waves along the
// centroids) are merged at the very end by (score, index), so the lowest index wins a tie whatever the tiling.  Two tilings: centroid
// chunks of 128 (2 x 2 waves, 2 x 2 tiles each) and, for K <= 32, one chunk of 32 (4 x 1 waves, one tile each).
//   |x_i|^2 is summed by the threads that load the row, during the first chunk, in a fixed order; |c|^2 by one wave per centroid in a
// pass of its own.  dist = max(0, |x|^2 + score).  Each workgroup leaves its fp64 sum of dist and its count of changed labels in the
// workspace and a one-workgroup pass adds them in index order: no atomics at all, the same bits on every run.
//
// UPDATE.  A stable counting sort of the row indices by label, then sums over whole gathered rows:
//   1. hist:    at most 1024 blocks of consecutive rows count their rows per cluster (LDS integer atomics: order-free) -> hist[block][c];
//   2. prefix:  per cluster the running sum over the blocks (hist becomes each block's first rank in its cluster), counts[c], the
//               clusters' first slots and first pieces (scans over K);
//   3. scatter: one wave per block walks its rows 64 at a time IN ORDER; a row's slot is its cluster's next free slot plus the number of
//               lower lanes with the same label: sorted[] lists every cluster's rows in ascending row order;
//   4. sums:    a cluster is cut into pieces of kPiece = 512 sorted rows; block (piece, 256 columns) streams its rows in order, a thread
//               owns one column and adds in fp64 -> partial[piece][D];
//   5. final:   thread (c, column) adds its cluster's pieces in piece order, divides by the count and rounds once to fp32.  An empty
//               cluster is not written.
// A label outside [0, K) is counted nowhere and indexes nothing.  Every sum has one fixed order: the same bits on every run.
#include <algorithm>

#include "mfma_tile.h"

namespace {
using namespace agan;

constexpr int kThreads = kTileThreads;        // (TileRegs, the k-major store and the MFMA stage: mfma_tile.h)
constexpr int kRows = 128;             // rows of X per assign workgroup
constexpr int kMaxDim = 4096;          // largest D and K
constexpr int kSmallK = 32;            // K <= kSmallK: the one-chunk tiling
constexpr int kPiece = 512;            // sorted rows per partial sum of the update
constexpr int kHistBlocks = 1024;      // most blocks of the counting sort
constexpr int kHistRows = 1024;        // fewest rows per block of the counting sort

// ---------------------------------------------------------------------------------------------------------------------------------
// assign
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void centroid_norm_kernel(const float* __restrict__ c, float* __restrict__ cnorm, int D, int K) {
    const int k = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    if (k >= K) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int d = lane; d < D; d += kWave) { const float v = c[(size_t)k * D + d]; s = fmaf(v, v, s); }
    s = wave_sum(s);
    if (lane == 0) cnorm[k] = s;
}

// WR x WC waves (rows x centroids), TR x TC tiles of 32 x 32 per wave: kRows = WR * TR * 32 rows, a chunk of KC = WC * TC * 32 centroids
template <int WR, int WC, int TR, int TC, bool VEC>
__global__ __launch_bounds__(kThreads) void assign_kernel(const float* __restrict__ x, const float* __restrict__ cen,
                                                          const float* __restrict__ cnorm, int32_t* __restrict__ labels,
                                                          float* __restrict__ dist, double* __restrict__ part_sum,
                                                          int32_t* __restrict__ part_changed, int N, int D, int K) {
    static_assert(WR * WC * kWave == kThreads && WR * TR * 32 == kRows, "tiling");
    constexpr int KC = WC * TC * 32;
    constexpr int XR = VEC ? kRows / 32 : kRows / 8;              // rows of X a loading thread touches
    __shared__ float xs[kStep * (kRows + kPad)];
    __shared__ float cs[kStep * (KC + kPad)];
    __shared__ float cn_s[KC];
    __shared__ float xn_s[kRows];
    __shared__ float cand_score[2 * WC][kRows];
    __shared__ int cand_index[2 * WC][kRows];
    __shared__ double red_sum[kThreads / kWave];
    __shared__ int red_changed[kThreads / kWave];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave / WC, wc = wave % WC;
    const int half = lane >> 5, l32 = lane & 31;
    const int row0 = blockIdx.x * kRows;
    const int steps = cdiv(D, kStep);

    float best[TR];
    int best_c[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r) best[r] = INFINITY, best_c[r] = 0;
    float sq[XR] = {};

    TileRegs<kRows, VEC> xr;
    TileRegs<KC, VEC> cr;
    for (int c0 = 0; c0 < K; c0 += KC) {
        f32x16 acc[TC][TR];
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int r = 0; r < TR; ++r) acc[a][r] = f32x16{0};
        xr.load(x, N, D, row0, 0);
        cr.load(cen, K, D, c0, 0);
        for (int s = 0; s < steps; ++s) {
            __syncthreads();                                       // the previous step's (and chunk's) LDS reads are done
            xr.store(xs);
            cr.store(cs);
            if (s == 0 && t < KC) cn_s[t] = (c0 + t < K) ? cnorm[c0 + t] : 0.f;
            if (c0 == 0) xr.add_squares(sq);
            __syncthreads();
            if (s + 1 < steps) {
                xr.load(x, N, D, row0, (s + 1) * kStep);
                cr.load(cen, K, D, c0, (s + 1) * kStep);
            }
            mfma_stage<KC, kRows, TC, TR>(cs, xs, wc * TC, wr * TR, half, l32, acc);
        }
        // register e of tile (i, r): centroid (e & 3) + 8 (e >> 2) + 4 half of the tile, row l32 -- ascending in (i, e) for a lane
#pragma unroll
        for (int r = 0; r < TR; ++r)
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int cl = (wc * TC + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
                    const float score = fmaf(-2.f, acc[i][r][e], cn_s[cl]);
                    if (c0 + cl < K && score < best[r]) best[r] = score, best_c[r] = c0 + cl;
                }
    }
    // |x|^2: the G consecutive lanes that loaded a row hold its parts
    {
        constexpr int G = VEC ? 8 : 32;
#pragma unroll
        for (int j = 0; j < XR; ++j) {
            float v = sq[j];
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if ((t & (G - 1)) == 0) xn_s[(VEC ? (t >> 3) + 32 * j : (t >> 5) + 8 * j)] = v;
        }
    }
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int row = (wr * TR + r) * 32 + l32;
        cand_score[wc * 2 + half][row] = best[r];
        cand_index[wc * 2 + half][row] = best_c[r];
    }
    __syncthreads();
    double d_sum = 0.0;
    int changed = 0;
    if (t < kRows && t < N - row0) {
        float s = cand_score[0][t];
        int c = cand_index[0][t];
#pragma unroll
        for (int j = 1; j < 2 * WC; ++j) {
            const float sj = cand_score[j][t];
            const int cj = cand_index[j][t];
            if (sj < s || (sj == s && cj < c)) s = sj, c = cj;
        }
        const float d = fmaxf(0.f, xn_s[t] + s);
        const int row = row0 + t;
        changed = labels[row] != c;
        labels[row] = c;
        dist[row] = d;
        d_sum = (double)d;
    }
    d_sum = wave_sum_d(d_sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) changed += __shfl_xor(changed, o, 64);
    if (lane == 0) red_sum[wave] = d_sum, red_changed[wave] = changed;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        int n = 0;
        for (int w = 0; w < kThreads / kWave; ++w) s += red_sum[w], n += red_changed[w];
        part_sum[blockIdx.x] = s;
        part_changed[blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(kThreads) void assign_final_kernel(const double* __restrict__ part_sum, const int32_t* __restrict__ part_changed,
                                                                int blocks, double* __restrict__ inertia, int32_t* __restrict__ n_changed) {
    __shared__ double red_sum[kThreads];
    __shared__ int red_changed[kThreads];
    double s = 0.0;
    int n = 0;
    for (int i = threadIdx.x; i < blocks; i += kThreads) s += part_sum[i], n += part_changed[i];
    red_sum[threadIdx.x] = s;
    red_changed[threadIdx.x] = n;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red_sum[threadIdx.x] += red_sum[threadIdx.x + o], red_changed[threadIdx.x] += red_changed[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *inertia = red_sum[0], *n_changed = red_changed[0];
}

bool in_domain(int N, int D, int K) {
    return N >= 1 && D >= 1 && D <= kMaxDim && K >= 1 && K <= kMaxDim && (long long)N * D < (1ll << 31);
}

struct AssignWs {
    size_t cnorm, part_sum, part_changed, total;
    int blocks;
    AssignWs(int N, int K) {
        blocks = cdiv(N, kRows);
        cnorm = 0;
        part_sum = up16((size_t)K * sizeof(float));
        part_changed = part_sum + up16((size_t)blocks * sizeof(double));
        total = part_changed + up16((size_t)blocks * sizeof(int32_t));
    }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// update
// ---------------------------------------------------------------------------------------------------------------------------------
struct UpdateWs {
    size_t hist, first_slot, first_piece, sorted, partial, total;
    int hist_rows, hist_blocks, max_pieces;
    UpdateWs(int N, int D, int K) {
        hist_rows = std::max(kHistRows, cdiv(N, kHistBlocks));
        hist_blocks = cdiv(N, hist_rows);
        max_pieces = N / kPiece + K;                               // sum_c ceil(n_c / kPiece) <= floor(N / kPiece) + K
        hist = 0;
        first_slot = hist + up16((size_t)hist_blocks * K * sizeof(int32_t));
        first_piece = first_slot + up16((size_t)(K + 1) * sizeof(int32_t));
        sorted = first_piece + up16((size_t)(K + 1) * sizeof(int32_t));
        partial = sorted + up16((size_t)N * sizeof(int32_t));
        total = partial + up16((size_t)max_pieces * D * sizeof(double));
    }
};

__global__ __launch_bounds__(kThreads) void hist_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ hist, int N, int K,
                                                        int hist_rows) {
    __shared__ int h[kMaxDim];
    for (int c = threadIdx.x; c < K; c += kThreads) h[c] = 0;
    __syncthreads();
    const int lo = blockIdx.x * hist_rows, n = min(hist_rows, N - lo);         // (lo < N; lo + hist_rows may pass 2^31)
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int c = labels[lo + i];
        if (c >= 0 && c < K) atomicAdd(&h[c], 1);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < K; c += kThreads) hist[(size_t)blockIdx.x * K + c] = h[c];
}

// one workgroup of 1024 threads: thread t owns clusters 4 t .. 4 t + 3
__global__ __launch_bounds__(1024) void prefix_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ counts, int32_t* __restrict__ first_slot,
                                                      int32_t* __restrict__ first_piece, int K, int hist_blocks) {
    __shared__ int s_rows[1024], s_pieces[1024];
    const int t = threadIdx.x;
    int n[4], rows = 0, pieces = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = 4 * t + q;
        int run = 0;
        if (c < K) {
            for (int b = 0; b < hist_blocks; ++b) {
                const size_t i = (size_t)b * K + c;
                const int v = hist[i];
                hist[i] = run;
                run += v;
            }
            counts[c] = run;
        }
        n[q] = run;
        rows += run;
        pieces += cdiv(run, kPiece);
    }
    s_rows[t] = rows, s_pieces[t] = pieces;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                            // inclusive scan (integers: any order gives the same sums)
        const int r = t >= o ? s_rows[t - o] : 0, p = t >= o ? s_pieces[t - o] : 0;
        __syncthreads();
        s_rows[t] += r, s_pieces[t] += p;
        __syncthreads();
    }
    int slot = s_rows[t] - rows, piece = s_pieces[t] - pieces;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = 4 * t + q;
        if (c < K) first_slot[c] = slot, first_piece[c] = piece;
        slot += n[q], piece += cdiv(n[q], kPiece);
    }
    if (t == 1023) first_slot[K] = s_rows[t], first_piece[K] = s_pieces[t];      // entry K: the totals (K = 4096 has no thread 1024)
}

// one wave per block of rows
__global__ __launch_bounds__(kWave) void scatter_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ hist,
                                                        const int32_t* __restrict__ first_slot, int32_t* __restrict__ sorted, int N, int K,
                                                        int hist_rows) {
    __shared__ int next[kMaxDim];
    const int lane = threadIdx.x;
    for (int c = lane; c < K; c += kWave) next[c] = first_slot[c] + hist[(size_t)blockIdx.x * K + c];
    __syncthreads();
    const int lo = blockIdx.x * hist_rows, n = min(hist_rows, N - lo);
    for (int base = 0; base < n; base += kWave) {
        const int i = lo + min(base + lane, n - 1);
        int c = base + lane < n ? labels[i] : -1;
        if (c < 0 || c >= K) c = -1;
        int lower = 0, same = 0;
        for (int j = 0; j < kWave; ++j) {
            const int eq = __shfl(c, j, 64) == c;
            same += eq;
            lower += eq && j < lane;
        }
        int slot = 0;
        if (c >= 0) {
            slot = next[c] + lower;
            sorted[slot] = i;
        }
        __syncthreads();
        if (c >= 0 && lower == same - 1) next[c] = slot + 1;       // the cluster's last lane of this step
        __syncthreads();
    }
}

__device__ __forceinline__ int cluster_of_piece(const int32_t* __restrict__ first_piece, int K, int piece) {
    int lo = 0, hi = K;                                             // the c with first_piece[c] <= piece < first_piece[c + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first_piece[mid] <= piece) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void piece_sum_kernel(const float* __restrict__ x, const int32_t* __restrict__ sorted,
                                                             const int32_t* __restrict__ counts, const int32_t* __restrict__ first_slot,
                                                             const int32_t* __restrict__ first_piece, double* __restrict__ partial, int D,
                                                             int K) {
    const int piece = blockIdx.x;
    if (piece >= first_piece[K]) return;
    const int c = cluster_of_piece(first_piece, K, piece);
    const int in_cluster = (piece - first_piece[c]) * kPiece;
    const int lo = first_slot[c] + in_cluster, hi = lo + min(kPiece, counts[c] - in_cluster);
    const int col = blockIdx.y * kThreads + threadIdx.x;
    if (col >= D) return;
    double s = 0.0;
    int q = lo;
    for (; q + 8 <= hi; q += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = sorted[q + u];
            v[u] = x[(size_t)i * D + col];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)v[u];
    }
    for (; q < hi; ++q) {
        const int i = sorted[q];
        s += (double)x[(size_t)i * D + col];
    }
    partial[(size_t)piece * D + col] = s;
}

__global__ __launch_bounds__(kThreads) void centroid_kernel(const double* __restrict__ partial, const int32_t* __restrict__ counts,
                                                            const int32_t* __restrict__ first_piece, float* __restrict__ centroids, int D) {
    const int c = blockIdx.x;
    const int col = blockIdx.y * kThreads + threadIdx.x;
    const int n = counts[c];
    if (col >= D || n <= 0) return;
    double s = 0.0;
    for (int p = first_piece[c]; p < first_piece[c + 1]; ++p) s += partial[(size_t)p * D + col];
    centroids[(size_t)c * D + col] = (float)(s / (double)n);
}

template <int WR, int WC, int TR, int TC>
void launch_assign(bool vec, int blocks, hipStream_t st, const float* x, const float* cen, const float* cnorm, int32_t* labels, float* dist,
                   double* part_sum, int32_t* part_changed, int N, int D, int K) {
    if (vec)
        hipLaunchKernelGGL((assign_kernel<WR, WC, TR, TC, true>), dim3(blocks), dim3(kThreads), 0, st, x, cen, cnorm, labels, dist, part_sum,
                           part_changed, N, D, K);
    else
        hipLaunchKernelGGL((assign_kernel<WR, WC, TR, TC, false>), dim3(blocks), dim3(kThreads), 0, st, x, cen, cnorm, labels, dist, part_sum,
                           part_changed, N, D, K);
}

}  // namespace

extern "C" size_t agan_kmeans_assign_ws_bytes(int N, int D, int K) { return in_domain(N, D, K) ? AssignWs(N, K).total : 0; }

extern "C" int agan_kmeans_assign(const float* x, const float* centroids, int32_t* labels, float* dist, int32_t* n_changed, double* inertia,
                                  int N, int D, int K, void* ws, size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(N >= 1 && D >= 1 && K >= 1, "kmeans_assign: bad shape (N %d, D %d, K %d)", N, D, K);
    AGAN_REQUIRE(D <= kMaxDim && K <= kMaxDim, "kmeans_assign: D %d or K %d above %d", D, K, kMaxDim);
    AGAN_REQUIRE((long long)N * D < (1ll << 31), "kmeans_assign: N * D = %lld is 2^31 or more", (long long)N * D);
    AGAN_REQUIRE(x && centroids && labels && dist && n_changed && inertia, "kmeans_assign: null pointer");
    const AssignWs w(N, K);
    AGAN_REQUIRE(ws, "kmeans_assign: no workspace (agan_kmeans_assign_ws_bytes: %zu bytes)", w.total);
    if (int e = check_ws("kmeans_assign", w.total, ws, ws_bytes)) return e;
    char* base = static_cast<char*>(ws);
    float* cnorm = reinterpret_cast<float*>(base + w.cnorm);
    double* part_sum = reinterpret_cast<double*>(base + w.part_sum);
    int32_t* part_changed = reinterpret_cast<int32_t*>(base + w.part_changed);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(centroid_norm_kernel, dim3(cdiv(K, kThreads / kWave)), dim3(kThreads), 0, st, centroids, cnorm, D, K);
    // 16-byte loads need whole float4s per row and an aligned base (the header's convention; checked, not assumed)
    const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(centroids)) % 16 == 0;
    if (K <= kSmallK)
        launch_assign<4, 1, 1, 1>(vec, w.blocks, st, x, centroids, cnorm, labels, dist, part_sum, part_changed, N, D, K);
    else
        launch_assign<2, 2, 2, 2>(vec, w.blocks, st, x, centroids, cnorm, labels, dist, part_sum, part_changed, N, D, K);
    hipLaunchKernelGGL(assign_final_kernel, dim3(1), dim3(kThreads), 0, st, part_sum, part_changed, w.blocks, inertia, n_changed);
    return check_launch("kmeans_assign");
}

extern "C" size_t agan_kmeans_update_ws_bytes(int N, int D, int K) { return in_domain(N, D, K) ? UpdateWs(N, D, K).total : 0; }

extern "C" int agan_kmeans_update(const float* x, const int32_t* labels, float* centroids, int32_t* counts, int N, int D, int K, void* ws,
                                  size_t ws_bytes, void* stream) {
    AGAN_REQUIRE(N >= 1 && D >= 1 && K >= 1, "kmeans_update: bad shape (N %d, D %d, K %d)", N, D, K);
    AGAN_REQUIRE(D <= kMaxDim && K <= kMaxDim, "kmeans_update: D %d or K %d above %d", D, K, kMaxDim);
    AGAN_REQUIRE((long long)N * D < (1ll << 31), "kmeans_update: N * D = %lld is 2^31 or more", (long long)N * D);
    AGAN_REQUIRE(x && labels && centroids && counts, "kmeans_update: null pointer");
    const UpdateWs w(N, D, K);
    AGAN_REQUIRE(ws, "kmeans_update: no workspace (agan_kmeans_update_ws_bytes: %zu bytes)", w.total);
    if (int e = check_ws("kmeans_update", w.total, ws, ws_bytes)) return e;
    char* base = static_cast<char*>(ws);
    int32_t* hist = reinterpret_cast<int32_t*>(base + w.hist);
    int32_t* first_slot = reinterpret_cast<int32_t*>(base + w.first_slot);
    int32_t* first_piece = reinterpret_cast<int32_t*>(base + w.first_piece);
    int32_t* sorted = reinterpret_cast<int32_t*>(base + w.sorted);
    double* partial = reinterpret_cast<double*>(base + w.partial);
    hipStream_t st = as_stream(stream);
    const int col_blocks = cdiv(D, kThreads);
    hipLaunchKernelGGL(hist_kernel, dim3(w.hist_blocks), dim3(kThreads), 0, st, labels, hist, N, K, w.hist_rows);
    hipLaunchKernelGGL(prefix_kernel, dim3(1), dim3(1024), 0, st, hist, counts, first_slot, first_piece, K, w.hist_blocks);
    hipLaunchKernelGGL(scatter_kernel, dim3(w.hist_blocks), dim3(kWave), 0, st, labels, hist, first_slot, sorted, N, K, w.hist_rows);
    hipLaunchKernelGGL(piece_sum_kernel, dim3(w.max_pieces, col_blocks), dim3(kThreads), 0, st, x, sorted, counts, first_slot, first_piece,
                       partial, D, K);
    hipLaunchKernelGGL(centroid_kernel, dim3(K, col_blocks), dim3(kThreads), 0, st, partial, counts, first_piece, centroids, D);
    return check_launch("kmeans_update");
}
