// Spectral normalisation of a weight matrix (Miyato et al., ICLR 2018; include/agan.h states the operation): one power iteration,
// sigma, W_sn = W / sigma, and the backward's rank-1 correction.  W is [Cout, K0 | K1]: one or two column segments, each a contiguous
// row-major tensor of its own (the second is the sentence part of the conditional head's joint conv).  fp32 throughout.
//
// Nothing here is compute: a forward reads W three times and writes it once, a backward the same.  Every sum over rows or columns
// goes through per-workgroup partials in the caller's workspace and is finished in one fixed order by whoever needs it -- no
// atomics, no grid-wide synchronisation, the same bits every run.
//
// Two forms, chosen by size alone (the one dispatch seam: Cout * (K0 + K1) <= kSmallElems | above):
//   small  one 256-thread workgroup does a whole direction in ONE launch, the vectors in LDS (the first conv, the logit heads, the
//          joint conv of a narrow discriminator); no workspace.
//   big    forward in four launches, each of which needs a chip-wide value of the one before:
//          (a) colsum   v_raw = W^T u.  A workgroup owns a strip of 256 columns of one segment and a block of rows; its four waves take
//                       rows in turn, a lane 16 bytes of a row; one partial slab [K] per row block.
//          (b) rowdot   a workgroup owns a block of rows and a chunk of kChunk columns: it sums the chunk of the slabs in slab order
//                       into LDS (and its |v_raw|^2 part), then a wave per row forms the row's part of t_raw = W v_raw.
//          (c) scalars  ONE workgroup rebuilds |v_raw|, t = t_raw / |v_raw|, |t| and sigma from the (small) partials in a fixed order
//                       and writes u', sigma and the two scalars the copy needs.
//          (d) finish   every workgroup writes its share of v = v_raw / |v_raw|, then W_sn = W / sigma as a streaming copy.
//          v is normalised in (c) / (d), not in (b) as the plain statement has it: t = W (v_raw / n) = (W v_raw) / n, so (b) needs
//          no norm and no workgroup reads slabs outside its own chunk.  (c) is a launch of its own because every workgroup of the copy
//          would otherwise sum all chunks x Cout partials itself.
//          backward in two: partial dots of c = <dW_sn, W_sn>, then dW = (dW_sn - c u v^T) / sigma with the accumulate flags.
// Rows are 16-byte aligned only where a segment's K is a multiple of 4 (and its base is aligned): per segment the row kernels take
// 16 bytes per lane then, and a lane-per-column scalar form otherwise.  The streaming kernels (the copy, the dot) see each segment as a flat
// array: 16 bytes per lane whenever the bases are aligned, with a scalar tail.
#include <algorithm>

#include "agan_common.h"

using namespace agan;

namespace {

constexpr int kNT = 256;
constexpr int kNW = kNT / 64;
constexpr int kNTS = 1024;             // threads of the one workgroup that reduces the forward's scalars
constexpr int kStrip = 256;             // columns of a colsum strip: 64 lanes x 4
constexpr int kChunk = 1024;            // columns of a rowdot chunk (4 KB of LDS)
constexpr int kMaxSlabs = 8;
constexpr int kMaxStream = 1024;        // workgroups of a streaming kernel
constexpr int kSmallElems = 8192;       // the dispatch seam: at most this many weights -> the one-workgroup form
constexpr float kEps = 1e-12f;

struct Mat {
    const float* w[2];
    int cout, k[2];
    unsigned vec;                       // bit s: segment s has 16-byte aligned rows (base aligned, K a multiple of 4)
};

thread_local int g_log[4];              // the form of the last forward and backward: [0] fwd form, [1] slabs, [2] chunks, [3] bwd form
enum { kFormNone = 0, kFormSmall = 1, kFormBig = 2 };

__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// sum over the block, the same value in every thread; fixed order (xor butterfly inside a wave, waves ascending)
__device__ __forceinline__ float bsum(float v, float* red) { return block_sum<kNT>(v, red); }

// ---- (a) column sums --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void colsum_kernel(Mat m, const float* __restrict__ u, float* __restrict__ part, int nstrip0,
                                                     int rows_per_block) {
    __shared__ float red[kNW][kStrip];
    const int seg = (int)blockIdx.x >= nstrip0;
    const int c0 = ((int)blockIdx.x - (seg ? nstrip0 : 0)) * kStrip;
    const float* __restrict__ w = m.w[seg];
    const int ks = m.k[seg], koff = seg ? m.k[0] : 0, K = m.k[0] + m.k[1];
    const int r0 = blockIdx.y * rows_per_block, r1 = min(m.cout, r0 + rows_per_block);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if ((m.vec >> seg) & 1) {
        const int col = c0 + 4 * lane;
        if (col < ks) {                                         // (ks is a multiple of 4: the whole quad is inside)
#pragma unroll 4
            for (int r = r0 + wave; r < r1; r += kNW) {
                const float4 x = *reinterpret_cast<const float4*>(w + (size_t)r * ks + col);
                const float ur = u[r];
                acc[0] += x.x * ur; acc[1] += x.y * ur; acc[2] += x.z * ur; acc[3] += x.w * ur;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) red[wave][4 * lane + j] = acc[j];
    } else {
        for (int r = r0 + wave; r < r1; r += kNW) {
            const float ur = u[r];
            const float* row = w + (size_t)r * ks;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = c0 + lane + 64 * j;
                if (col < ks) acc[j] += row[col] * ur;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) red[wave][lane + 64 * j] = acc[j];
    }
    __syncthreads();
    const int col = c0 + tid;
    if (col < ks) part[(size_t)blockIdx.y * K + koff + col] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ---- (b) row dots with the slab sum ---------------------------------------------------------------------------------------------------
// vsrc: `nslab` slabs [K] whose ordered sum is the vector (nslab = 1 and the stored v when nothing is iterated)
__global__ __launch_bounds__(kNT) void rowdot_kernel(Mat m, const float* __restrict__ vsrc, int nslab, float* __restrict__ tpart,
                                                     float* __restrict__ vnpart, int nchunk0, int rows_per_block) {
    __shared__ __attribute__((aligned(16))) float vs[kChunk];
    __shared__ float red[kNW];
    const int chunk = blockIdx.x, seg = chunk >= nchunk0;
    const int c0 = (chunk - (seg ? nchunk0 : 0)) * kChunk;
    const float* __restrict__ w = m.w[seg];
    const int ks = m.k[seg], koff = seg ? m.k[0] : 0, K = m.k[0] + m.k[1];
    const int len = min(kChunk, ks - c0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float sq = 0.f;
    for (int c = tid; c < kChunk; c += kNT) {
        float v = 0.f;
        if (c < len)
            for (int s = 0; s < nslab; ++s) v += vsrc[(size_t)s * K + koff + c0 + c];
        vs[c] = v;                                              // (0 past the chunk's end: the quads of the vector form stay finite)
        sq += v * v;
    }
    sq = bsum(sq, red);                                          // (its barriers also publish vs)
    if (blockIdx.y == 0 && tid == 0) vnpart[chunk] = sq;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(m.cout, r0 + rows_per_block);
    const bool vec = (m.vec >> seg) & 1;
    for (int r = r0 + wave; r < r1; r += kNW) {
        const float* row = w + (size_t)r * ks + c0;
        float acc = 0.f;
        if (vec) {
#pragma unroll 4
            for (int c = 4 * lane; c < len; c += 256) acc += dot4(*reinterpret_cast<const float4*>(row + c), *reinterpret_cast<const float4*>(vs + c));
        } else {
#pragma unroll 4
            for (int c = lane; c < len; c += 64) acc += row[c] * vs[c];
        }
        acc = wave_sum(acc);
        if (lane == 0) tpart[(size_t)chunk * m.cout + r] = acc;
    }
}

// what (c) derives from t_raw: sigma, and what to divide t_raw by to get u'
struct Scalars { float vn, tn, sigma; };

// (u, v, u_out and v_out carry no __restrict__ in the forward kernels: include/agan.h lets the outputs be the state itself)
// t_raw[r] = sum over the chunks of tpart, in chunk order
__device__ __forceinline__ float t_raw_of(const float* __restrict__ tpart, int nchunk, int cout, int r) {
    float t = 0.f;
    for (int c = 0; c < nchunk; ++c) t += tpart[(size_t)c * cout + r];
    return t;
}

// ---- (c) the scalars and u': ONE workgroup of 1024 threads ----------------------------------------------------------------------------
// The partials are small (chunks + chunks x Cout floats) but every consumer needs all of them: summed once here, not by each of the
// copy's workgroups (at 2048 x 16384 that was 256 KB per workgroup, as much L2 traffic in total as the copy moves through HBM).
// scal[0] = max(|v_raw|, eps) (1 without an iteration), scal[1] = sigma.
__global__ __launch_bounds__(kNTS) void scalars_kernel(const float* __restrict__ tpart, const float* __restrict__ vnpart, int nchunk, int cout,
                                                       const float* u, int iterate, float* u_out, float* __restrict__ sigma_out,
                                                       float* __restrict__ scal) {
    __shared__ float red[kNTS / 64];
    Scalars s;
    const int tid = threadIdx.x;
    s.vn = 1.f;
    if (iterate) {
        float q = 0.f;
        for (int c = tid; c < nchunk; c += kNTS) q += vnpart[c];
        s.vn = fmaxf(sqrtf(block_sum<kNTS>(q, red)), kEps);
    }
    float q = 0.f;
    for (int r = tid; r < cout; r += kNTS) {
        const float t = t_raw_of(tpart, nchunk, cout, r) / s.vn;
        q += iterate ? t * t : u[r] * t;
    }
    q = block_sum<kNTS>(q, red);
    s.sigma = q;                                                 // without an iteration: <u, W v>
    if (iterate) {
        s.tn = fmaxf(sqrtf(q), kEps);
        q = 0.f;
        for (int r = tid; r < cout; r += kNTS) {                 // u' = t / |t| and sigma = <u', W v>
            const float t = t_raw_of(tpart, nchunk, cout, r) / s.vn, up = t / s.tn;
            u_out[r] = up;
            q += up * t;
        }
        s.sigma = block_sum<kNTS>(q, red);
    }
    if (tid == 0) { sigma_out[0] = s.sigma; scal[0] = s.vn; scal[1] = s.sigma; }
}

// out = in / sigma over a flat array, grid-strided; 16 bytes per lane when both bases are aligned
__device__ __forceinline__ void scaled_copy(const float* __restrict__ in, float* __restrict__ out, size_t n, float sigma, size_t gtid, size_t gsize) {
    if ((((uintptr_t)in | (uintptr_t)out) & 15) == 0) {
        const size_t n4 = n >> 2;
        for (size_t i = gtid; i < n4; i += gsize) {
            float4 x = reinterpret_cast<const float4*>(in)[i];
            x.x /= sigma; x.y /= sigma; x.z /= sigma; x.w /= sigma;
            reinterpret_cast<float4*>(out)[i] = x;
        }
        for (size_t i = (n4 << 2) + gtid; i < n; i += gsize) out[i] = in[i] / sigma;
    } else {
        for (size_t i = gtid; i < n; i += gsize) out[i] = in[i] / sigma;
    }
}

// ---- (d) v and the scaled copy ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void finish_kernel(Mat m, const float* __restrict__ part, int nslab, const float* __restrict__ scal,
                                                     int iterate, float* v_out, float* __restrict__ o0, float* __restrict__ o1) {
    const int tid = threadIdx.x, K = m.k[0] + m.k[1];
    const float vn = scal[0], sigma = scal[1];
    if (iterate)
        for (size_t k = (size_t)blockIdx.x * kNT + tid; k < (size_t)K; k += (size_t)gridDim.x * kNT) {
            float v = 0.f;
            for (int i = 0; i < nslab; ++i) v += part[(size_t)i * K + k];
            v_out[k] = v / vn;
        }
    const size_t gtid = (size_t)blockIdx.x * kNT + tid, gsize = (size_t)gridDim.x * kNT;
    scaled_copy(m.w[0], o0, (size_t)m.cout * m.k[0], sigma, gtid, gsize);
    if (m.k[1] > 0) scaled_copy(m.w[1], o1, (size_t)m.cout * m.k[1], sigma, gtid, gsize);
}

__device__ __forceinline__ float elem(const Mat& m, int r, int k) {
    return k < m.k[0] ? m.w[0][(size_t)r * m.k[0] + k] : m.w[1][(size_t)r * m.k[1] + (k - m.k[0])];
}

// ---- the small form's forward: one workgroup, the vectors in LDS -------------------------------------------------------------------------
// dynamic LDS: v [K], the row parts [max(Cout, kNW)] (t in place where a row has one part), 4 more floats for t otherwise
__global__ __launch_bounds__(kNT) void small_fwd_kernel(Mat m, const float* u, const float* v, int iterate,
                                                        float* u_out, float* v_out, float* __restrict__ sigma_out,
                                                        float* __restrict__ o0, float* __restrict__ o1) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float red[kNW];
    const int K = m.k[0] + m.k[1], cout = m.cout;
    float* vs = lds;
    float* rp = vs + K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float vn = 1.f;
    if (iterate) {
        float q = 0.f;
        for (int k = tid; k < K; k += kNT) {                    // a thread per column, rows ascending
            float a = 0.f;
            for (int r = 0; r < cout; ++r) a += elem(m, r, k) * u[r];
            vs[k] = a;
            q += a * a;
        }
        vn = fmaxf(sqrtf(bsum(q, red)), kEps);
    } else {
        for (int k = tid; k < K; k += kNT) vs[k] = v[k];
        __syncthreads();
    }
    // t_raw: a wave per (row, column part); a row has S = kNW / Cout parts where there are fewer rows than waves
    const int S = cout >= kNW ? 1 : kNW / cout, plen = cdiv(K, S);
    float* ts = S == 1 ? rp : rp + kNW;
    for (int i = wave; i < cout * S; i += kNW) {
        const int r = i / S, p = i - r * S;
        const int k1 = min(K, (p + 1) * plen);
        float a = 0.f;
        for (int k = p * plen + lane; k < k1; k += 64) a += elem(m, r, k) * vs[k];
        a = wave_sum(a);
        if (lane == 0) rp[i] = a;
    }
    __syncthreads();
    float q = 0.f;
    for (int r = tid; r < cout; r += kNT) {
        float t = 0.f;
        for (int p = 0; p < S; ++p) t += rp[r * S + p];
        t /= vn;
        ts[r] = t;
        q += iterate ? t * t : u[r] * t;
    }
    q = bsum(q, red);
    float sigma = q;
    if (iterate) {
        const float tn = fmaxf(sqrtf(q), kEps);
        q = 0.f;
        for (int r = tid; r < cout; r += kNT) {
            const float up = ts[r] / tn;
            u_out[r] = up;
            q += up * ts[r];
        }
        sigma = bsum(q, red);
        for (int k = tid; k < K; k += kNT) v_out[k] = vs[k] / vn;
    }
    if (tid == 0) sigma_out[0] = sigma;
    scaled_copy(m.w[0], o0, (size_t)cout * m.k[0], sigma, tid, kNT);
    if (m.k[1] > 0) scaled_copy(m.w[1], o1, (size_t)cout * m.k[1], sigma, tid, kNT);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float flat_dot(const float* __restrict__ a, const float* __restrict__ b, size_t n, size_t gtid, size_t gsize) {
    float acc = 0.f;
    if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) {
        const size_t n4 = n >> 2;
        for (size_t i = gtid; i < n4; i += gsize) acc += dot4(reinterpret_cast<const float4*>(a)[i], reinterpret_cast<const float4*>(b)[i]);
        for (size_t i = (n4 << 2) + gtid; i < n; i += gsize) acc += a[i] * b[i];
    } else {
        for (size_t i = gtid; i < n; i += gsize) acc += a[i] * b[i];
    }
    return acc;
}

struct Grad {
    const float* d[2];                  // dW_sn
    const float* wsn[2];
    float* out[2];
    int acc[2];
    int cout, k[2];
};

// one partial of c = <dW_sn, W_sn> per workgroup
__global__ __launch_bounds__(kNT) void dot_kernel(Grad g, float* __restrict__ cpart) {
    __shared__ float red[kNW];
    const size_t gtid = (size_t)blockIdx.x * kNT + threadIdx.x, gsize = (size_t)gridDim.x * kNT;
    float acc = flat_dot(g.d[0], g.wsn[0], (size_t)g.cout * g.k[0], gtid, gsize);
    if (g.k[1] > 0) acc += flat_dot(g.d[1], g.wsn[1], (size_t)g.cout * g.k[1], gtid, gsize);
    acc = bsum(acc, red);
    if (threadIdx.x == 0) cpart[blockIdx.x] = acc;
}

// out (+)= (d - c u[r] v[koff + k]) / sigma over one segment, flat and grid-strided; the row of an element by one division
__device__ __forceinline__ void corrected(const float* __restrict__ d, float* __restrict__ out, int acc, int cout, int ks, int koff,
                                          const float* __restrict__ u, const float* __restrict__ v, float c, float sigma, size_t gtid, size_t gsize) {
    const unsigned n = (unsigned)cout * (unsigned)ks;
    if ((ks & 3) == 0 && (((uintptr_t)d | (uintptr_t)out) & 15) == 0) {
        for (size_t i = gtid; i < (n >> 2); i += gsize) {
            const unsigned e = (unsigned)i << 2, r = e / (unsigned)ks, k = e - r * (unsigned)ks;
            const float cu = c * u[r];
            const float* vk = v + koff + k;
            const float4 x = reinterpret_cast<const float4*>(d)[i];
            float4 y = make_float4((x.x - cu * vk[0]) / sigma, (x.y - cu * vk[1]) / sigma, (x.z - cu * vk[2]) / sigma, (x.w - cu * vk[3]) / sigma);
            if (acc) {
                const float4 o = reinterpret_cast<const float4*>(out)[i];
                y.x += o.x; y.y += o.y; y.z += o.z; y.w += o.w;
            }
            reinterpret_cast<float4*>(out)[i] = y;
        }
    } else {
        for (size_t i = gtid; i < n; i += gsize) {
            const unsigned e = (unsigned)i, r = e / (unsigned)ks, k = e - r * (unsigned)ks;
            const float y = (d[i] - c * u[r] * v[koff + k]) / sigma;
            out[i] = acc ? out[i] + y : y;
        }
    }
}

// the corrected, scaled write.  ncpart partials of c, summed by every workgroup in the same order.
__global__ __launch_bounds__(kNT) void correct_kernel(Grad g, const float* __restrict__ cpart, int ncpart, const float* __restrict__ u,
                                                      const float* __restrict__ v, const float* __restrict__ sigma) {
    __shared__ float red[kNW];
    float q = 0.f;
    for (int i = threadIdx.x; i < ncpart; i += kNT) q += cpart[i];
    const float c = bsum(q, red), s = sigma[0];
    const size_t gtid = (size_t)blockIdx.x * kNT + threadIdx.x, gsize = (size_t)gridDim.x * kNT;
    corrected(g.d[0], g.out[0], g.acc[0], g.cout, g.k[0], 0, u, v, c, s, gtid, gsize);
    if (g.k[1] > 0) corrected(g.d[1], g.out[1], g.acc[1], g.cout, g.k[1], g.k[0], u, v, c, s, gtid, gsize);
}

// the small form's backward: both steps in one workgroup
__global__ __launch_bounds__(kNT) void small_bwd_kernel(Grad g, const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ sigma) {
    __shared__ float red[kNW];
    float acc = flat_dot(g.d[0], g.wsn[0], (size_t)g.cout * g.k[0], threadIdx.x, kNT);
    if (g.k[1] > 0) acc += flat_dot(g.d[1], g.wsn[1], (size_t)g.cout * g.k[1], threadIdx.x, kNT);
    const float c = bsum(acc, red), s = sigma[0];
    corrected(g.d[0], g.out[0], g.acc[0], g.cout, g.k[0], 0, u, v, c, s, threadIdx.x, kNT);
    if (g.k[1] > 0) corrected(g.d[1], g.out[1], g.acc[1], g.cout, g.k[1], g.k[0], u, v, c, s, threadIdx.x, kNT);
}

// ---- host side: the domain, the form and the grids of a shape -----------------------------------------------------------------------------
inline bool shape_ok(int cout, int k0, int k1) {
    return cout >= 1 && k0 >= 1 && k1 >= 0 && (long long)cout * ((long long)k0 + k1) < (1LL << 31);
}
inline bool is_small(int cout, int k0, int k1) { return (long long)cout * ((long long)k0 + k1) <= kSmallElems; }
inline int round_up4(int v) { return (v + 3) / 4 * 4; }

struct Plan {
    int nstrip0, nstrip, nslab, rows_a;          // (a): strips of segment 0 / all, row blocks = slabs, rows of one
    int nchunk0, nchunk, nrowblk, rows_b;        // (b)
    int nstream;                                 // (c), (d), (e)
    size_t part_off, tpart_off, vn_off, scal_off, fwd_floats;
};

inline Plan plan_of(int cout, int k0, int k1) {
    Plan p;
    const long long K = (long long)k0 + k1, total = (long long)cout * K;
    p.nstrip0 = cdiv(k0, kStrip);
    p.nstrip = p.nstrip0 + cdiv(k1, kStrip);
    p.nslab = std::max(1, std::min({cdiv(512, p.nstrip), kMaxSlabs, cdiv(cout, 8)}));
    p.rows_a = cdiv(cout, p.nslab);
    p.nslab = cdiv(cout, p.rows_a);
    p.nchunk0 = cdiv(k0, kChunk);
    p.nchunk = p.nchunk0 + cdiv(k1, kChunk);
    // rows of a block: at least twice the slabs its workgroup sums (the slab reads stay below half of its weight reads), and no more
    // than 2048 workgroups
    p.rows_b = std::max({8, 2 * p.nslab, round_up4((int)cdivz((size_t)cout * p.nchunk, 2048))});
    p.rows_b = std::min(p.rows_b, round_up4(cout));
    p.nrowblk = cdiv(cout, p.rows_b);
    p.nstream = (int)std::max<long long>(1, std::min<long long>(kMaxStream, (total + 4095) / 4096));
    p.part_off = 0;
    p.tpart_off = p.part_off + (size_t)p.nslab * K;
    p.vn_off = p.tpart_off + (size_t)p.nchunk * cout;
    p.scal_off = p.vn_off + p.nchunk;
    p.fwd_floats = p.scal_off + 4;
    return p;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define SPECTRAL_SHAPE(what) \
    AGAN_REQUIRE(shape_ok(cout, k0, k1), what ": shape Cout=%d K0=%d K1=%d out of range (Cout >= 1, K0 >= 1, K1 >= 0, Cout * (K0 + K1) < 2^31)", cout, k0, k1)

}  // namespace

extern "C" {

size_t agan_spectral_fwd_ws_bytes(int cout, int k0, int k1) {
    if (!shape_ok(cout, k0, k1)) {
        set_error("spectral_fwd_ws_bytes: shape Cout=%d K0=%d K1=%d out of range", cout, k0, k1);
        return 0;
    }
    return is_small(cout, k0, k1) ? 0 : plan_of(cout, k0, k1).fwd_floats * sizeof(float);
}

int agan_spectral_fwd(const float* w0, const float* w1, const float* u, const float* v, float* u_out, float* v_out, float* sigma, float* wsn0,
                      float* wsn1, int cout, int k0, int k1, int iterate, void* ws, size_t ws_bytes, void* stream) {
    SPECTRAL_SHAPE("spectral_fwd");
    AGAN_REQUIRE(iterate == 0 || iterate == 1, "spectral_fwd: iterate must be 0 or 1, got %d", iterate);
    AGAN_REQUIRE(w0 && u && sigma && wsn0 && (k1 == 0 || (w1 && wsn1)), "spectral_fwd: null pointer");
    AGAN_REQUIRE(iterate ? (u_out && v_out) : v != nullptr, "spectral_fwd: null pointer (u_out and v_out with iterate = 1, v with iterate = 0)");
    if (int e = check_ws("spectral_fwd", agan_spectral_fwd_ws_bytes(cout, k0, k1), ws, ws_bytes)) return e;
    Mat m;
    m.w[0] = w0, m.w[1] = k1 > 0 ? w1 : w0, m.cout = cout, m.k[0] = k0, m.k[1] = k1;
    m.vec = (unsigned)(k0 % 4 == 0 && aligned16(w0)) | ((unsigned)(k1 > 0 && k1 % 4 == 0 && aligned16(w1)) << 1);
    hipStream_t st = as_stream(stream);
    if (is_small(cout, k0, k1)) {
        g_log[0] = kFormSmall, g_log[1] = g_log[2] = 0;
        const size_t lds = ((size_t)k0 + k1 + std::max(cout, kNW) + 4) * sizeof(float);      // <= 8192 + 9 floats
        hipLaunchKernelGGL(small_fwd_kernel, dim3(1), dim3(kNT), lds, st, m, u, v, iterate, u_out, v_out, sigma, wsn0, wsn1);
        return check_launch("spectral_fwd");
    }
    const Plan p = plan_of(cout, k0, k1);
    g_log[0] = kFormBig, g_log[1] = iterate ? p.nslab : 0, g_log[2] = p.nchunk;
    float* f = static_cast<float*>(ws);
    float *part = f + p.part_off, *tpart = f + p.tpart_off, *vnpart = f + p.vn_off, *scal = f + p.scal_off;
    if (iterate)
        hipLaunchKernelGGL(colsum_kernel, dim3(p.nstrip, p.nslab), dim3(kNT), 0, st, m, u, part, p.nstrip0, p.rows_a);
    hipLaunchKernelGGL(rowdot_kernel, dim3(p.nchunk, p.nrowblk), dim3(kNT), 0, st, m, iterate ? part : v, iterate ? p.nslab : 1, tpart, vnpart,
                       p.nchunk0, p.rows_b);
    hipLaunchKernelGGL(scalars_kernel, dim3(1), dim3(kNTS), 0, st, tpart, vnpart, p.nchunk, cout, u, iterate, u_out, sigma, scal);
    hipLaunchKernelGGL(finish_kernel, dim3(p.nstream), dim3(kNT), 0, st, m, part, p.nslab, scal, iterate, v_out, wsn0, wsn1);
    return check_launch("spectral_fwd");
}

size_t agan_spectral_bwd_ws_bytes(int cout, int k0, int k1) {
    if (!shape_ok(cout, k0, k1)) {
        set_error("spectral_bwd_ws_bytes: shape Cout=%d K0=%d K1=%d out of range", cout, k0, k1);
        return 0;
    }
    return is_small(cout, k0, k1) ? 0 : (size_t)plan_of(cout, k0, k1).nstream * sizeof(float);
}

int agan_spectral_bwd(const float* dwsn0, const float* dwsn1, const float* wsn0, const float* wsn1, const float* u, const float* v,
                      const float* sigma, float* dw0, float* dw1, int cout, int k0, int k1, int accumulate0, int accumulate1, void* ws,
                      size_t ws_bytes, void* stream) {
    SPECTRAL_SHAPE("spectral_bwd");
    AGAN_REQUIRE(dwsn0 && wsn0 && u && v && sigma && dw0 && (k1 == 0 || (dwsn1 && wsn1 && dw1)), "spectral_bwd: null pointer");
    if (int e = check_ws("spectral_bwd", agan_spectral_bwd_ws_bytes(cout, k0, k1), ws, ws_bytes)) return e;
    Grad g;
    g.d[0] = dwsn0, g.wsn[0] = wsn0, g.out[0] = dw0, g.acc[0] = accumulate0 != 0;
    g.d[1] = dwsn1, g.wsn[1] = wsn1, g.out[1] = dw1, g.acc[1] = accumulate1 != 0;
    g.cout = cout, g.k[0] = k0, g.k[1] = k1;
    hipStream_t st = as_stream(stream);
    if (is_small(cout, k0, k1)) {
        g_log[3] = kFormSmall;
        hipLaunchKernelGGL(small_bwd_kernel, dim3(1), dim3(kNT), 0, st, g, u, v, sigma);
        return check_launch("spectral_bwd");
    }
    const Plan p = plan_of(cout, k0, k1);
    g_log[3] = kFormBig;
    float* cpart = static_cast<float*>(ws);
    hipLaunchKernelGGL(dot_kernel, dim3(p.nstream), dim3(kNT), 0, st, g, cpart);
    hipLaunchKernelGGL(correct_kernel, dim3(p.nstream), dim3(kNT), 0, st, g, cpart, p.nstream, u, v, sigma);
    return check_launch("spectral_bwd");
}

int agan_spectral_last_launch(int* codes, int capacity) {
    for (int i = 0; i < std::min(capacity, 4); ++i) codes[i] = g_log[i];
    return 4;
}

}  // extern "C"
