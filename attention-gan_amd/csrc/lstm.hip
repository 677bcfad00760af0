// Bidirectional single-layer LSTM of the caption encoder (reference networks/rnn_encoder.py:68-96; networks/rnn_encoder.py,
// backend="hip"), fp32 in every precision mode.  The input projection x W_ih^T + b_ih runs on the linear-layer engine; this file
// holds the embedding gather, the recurrence and its backward-through-time.
//
// Recurrence layout (lstm_fwd_kernel / lstm_bwd_kernel): one workgroup per (group of kRows = 4 batch rows, direction), 4H threads,
// for the whole sequence: no inter-workgroup barrier, no atomics.
//   forward : thread j owns gate row j of W_hh (H fp32 in registers: 128 VGPRs at H = 128) and computes that row's pre-activation for
//             the 4 batch rows from h(t-1), which the workgroup broadcasts through LDS; thread (b = j / H, u = j % H) then owns cell u
//             of batch row b (c in a register) and applies torch's gate equations (order i, f, g, o).
//   backward: thread (q = j / H, k = j % H) owns column k of gate block q of W_hh (H fp32 in registers) and forms its share of
//             dh(t-1) = W_hh^T dgates; the 4 shares are added in q order through LDS.
// Each row runs its own length: the forward direction t = 0 .. len-1, the reverse one t = len-1 .. 0, both from h = c = 0.
// lstm_wgrad_kernel reduces dW_hh and db_hh over (b, t) in a fixed order, one thread per output element.
#include "agan_common.h"
#include "dispatch.h"

using namespace agan;

namespace {

constexpr int kRows = 4;         // batch rows per recurrence workgroup
constexpr int kThreads = 256;

__device__ __forceinline__ int clamp_len(const int32_t* lens, int b, int T) { return min(max(lens[b], 0), T); }

// ---- embedding --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void embedding_fwd_kernel(const int64_t* __restrict__ ids, int ids_ld, const float* __restrict__ table,
                                                                float* __restrict__ y, int B, int T, int V, int E) {
    const size_t n = (size_t)B * T * E;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int e = (int)(i % E);
    const size_t bt = i / E;
    const int t = (int)(bt % T), b = (int)(bt / T);
    const int64_t id = ids[(size_t)b * ids_ld + t];
    y[i] = (id >= 0 && id < V) ? table[(size_t)id * E + e] : 0.f;
}

// one workgroup per table row v: the (b, t) positions holding v summed in ascending b*T + t; rows nobody uses get 0
__global__ __launch_bounds__(kThreads) void embedding_bwd_kernel(const int64_t* __restrict__ ids, int ids_ld, const float* __restrict__ dy,
                                                                float* __restrict__ dtable, int B, int T, int E) {
    const int64_t v = blockIdx.x;
    for (int e = threadIdx.x; e < E; e += kThreads) {
        float s = 0.f;
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T; ++t)
                if (ids[(size_t)b * ids_ld + t] == v) s += dy[((size_t)b * T + t) * E + e];
        dtable[(size_t)v * E + e] = s;
    }
}

// ---- recurrence forward -----------------------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(4 * H) void lstm_fwd_kernel(const float* __restrict__ xg0, const float* __restrict__ xg1,
                                                         const float* __restrict__ whh0, const float* __restrict__ whh1,
                                                         const float* __restrict__ bhh0, const float* __restrict__ bhh1,
                                                         const int32_t* __restrict__ lens, float* __restrict__ out, float* __restrict__ hN,
                                                         float* __restrict__ gsave, float* __restrict__ csave, int B, int T, int D) {
    constexpr int G = 4 * H;
    __shared__ __align__(16) float hs[kRows][H];
    __shared__ float gs[kRows][G];
    const int tid = threadIdx.x, dir = blockIdx.y, b0 = blockIdx.x * kRows;
    const float* __restrict__ xg = dir ? xg1 : xg0;
    const float* __restrict__ whh = dir ? whh1 : whh0;
    const int DH = D * H;

    float w[H];                                    // (dword loads: a parameter inside a flat buffer is only 4-byte aligned)
#pragma unroll
    for (int k = 0; k < H; ++k) w[k] = whh[(size_t)tid * H + k];
    const float bias = (dir ? bhh1 : bhh0)[tid];

    int len[kRows], maxlen = 0;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        len[r] = b0 + r < B ? clamp_len(lens, b0 + r, T) : 0;
        maxlen = max(maxlen, len[r]);
    }
    const int cb = tid / H, cu = tid % H, b = b0 + cb;
    const int mylen = len[cb];
    float c = 0.f, h = 0.f;
    hs[cb][cu] = 0.f;
    __syncthreads();

    for (int s = 0; s < maxlen; ++s) {
        // gate pre-activations of row tid for the 4 batch rows: W_hh h(t-1) + b_hh + (x W_ih^T + b_ih)
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (s >= len[r]) continue;
            const float4* h4 = reinterpret_cast<const float4*>(hs[r]);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < H / 4; ++k) {
                const float4 v = h4[k];
                acc = fmaf(w[4 * k], v.x, acc);
                acc = fmaf(w[4 * k + 1], v.y, acc);
                acc = fmaf(w[4 * k + 2], v.z, acc);
                acc = fmaf(w[4 * k + 3], v.w, acc);
            }
            const int t = dir ? len[r] - 1 - s : s;
            gs[r][tid] = xg[((size_t)(b0 + r) * T + t) * G + tid] + (acc + bias);
        }
        __syncthreads();
        if (s < mylen) {
            const int t = dir ? mylen - 1 - s : s;
            const float gi = sigmoid_exact(gs[cb][cu]), gf = sigmoid_exact(gs[cb][H + cu]), gg = tanhf(gs[cb][2 * H + cu]),
                        go = sigmoid_exact(gs[cb][3 * H + cu]);
            c = gf * c + gi * gg;
            h = go * tanhf(c);
            const size_t bt = (size_t)b * T + t;
            out[bt * DH + dir * H + cu] = h;
            if (gsave) {
                float* g = gsave + ((size_t)dir * B * T + bt) * G;
                g[cu] = gi, g[H + cu] = gf, g[2 * H + cu] = gg, g[3 * H + cu] = go;
                csave[((size_t)dir * B * T + bt) * H + cu] = c;
            }
            hs[cb][cu] = h;
        }
        __syncthreads();
    }
    if (b < B) {
        hN[(size_t)b * DH + dir * H + cu] = h;
        for (int t = mylen; t < T; ++t) out[((size_t)b * T + t) * DH + dir * H + cu] = 0.f;
    }
}

// ---- recurrence backward (BPTT) ---------------------------------------------------------------------------------------------------
// dg0 / dg1 [B, T, 4H]: gradient of the gate pre-activations (= of the projection output x W_ih^T + b_ih), 0 at t >= len
template <int H>
__global__ __launch_bounds__(4 * H) void lstm_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ dhN,
                                                         const float* __restrict__ whh0, const float* __restrict__ whh1,
                                                         const float* __restrict__ gsave, const float* __restrict__ csave,
                                                         const int32_t* __restrict__ lens, float* __restrict__ dg0, float* __restrict__ dg1,
                                                         int B, int T, int D) {
    constexpr int G = 4 * H;
    __shared__ float dgs[kRows][G];
    __shared__ float part[4][kRows][H];
    const int tid = threadIdx.x, dir = blockIdx.y, b0 = blockIdx.x * kRows;
    const float* __restrict__ whh = dir ? whh1 : whh0;
    float* __restrict__ dg = dir ? dg1 : dg0;
    const int DH = D * H;

    const int q = tid / H, k = tid % H;            // W_hh^T share: column k of gate block q
    float w[H];
#pragma unroll
    for (int i = 0; i < H; ++i) w[i] = whh[(size_t)(q * H + i) * H + k];

    int len[kRows], maxlen = 0;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        len[r] = b0 + r < B ? clamp_len(lens, b0 + r, T) : 0;
        maxlen = max(maxlen, len[r]);
    }
    const int cb = tid / H, cu = tid % H, b = b0 + cb;
    const int mylen = len[cb];
    float dh_carry = 0.f, dc_carry = 0.f;
    if (b < B) {
        if (dhN) dh_carry = dhN[(size_t)b * DH + dir * H + cu];
        for (int t = mylen; t < T; ++t) {
            float* g = dg + ((size_t)b * T + t) * G;
            g[cu] = 0.f, g[H + cu] = 0.f, g[2 * H + cu] = 0.f, g[3 * H + cu] = 0.f;
        }
    }

    for (int s = maxlen - 1; s >= 0; --s) {
        if (s < mylen) {
            const int t = dir ? mylen - 1 - s : s;
            const size_t bt = (size_t)b * T + t;
            const float dh = dh_carry + (dout ? dout[bt * DH + dir * H + cu] : 0.f);
            const float* gsv = gsave + ((size_t)dir * B * T + bt) * G;
            const float gi = gsv[cu], gf = gsv[H + cu], gg = gsv[2 * H + cu], go = gsv[3 * H + cu];
            const float* cs = csave + (size_t)dir * B * T * H;
            const float cc = cs[bt * H + cu];
            const float cprev = s > 0 ? cs[((size_t)b * T + (dir ? t + 1 : t - 1)) * H + cu] : 0.f;
            const float tc = tanhf(cc);
            const float dc = dc_carry + dh * go * (1.f - tc * tc);
            dc_carry = dc * gf;
            const float di = dc * gg * gi * (1.f - gi);
            const float df = dc * cprev * gf * (1.f - gf);
            const float dgg = dc * gi * (1.f - gg * gg);
            const float dgo = dh * tc * go * (1.f - go);
            dgs[cb][cu] = di, dgs[cb][H + cu] = df, dgs[cb][2 * H + cu] = dgg, dgs[cb][3 * H + cu] = dgo;
            float* g = dg + bt * G;
            g[cu] = di, g[H + cu] = df, g[2 * H + cu] = dgg, g[3 * H + cu] = dgo;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (s >= len[r]) continue;
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < H; ++i) acc = fmaf(w[i], dgs[r][q * H + i], acc);
            part[q][r][k] = acc;
        }
        __syncthreads();
        if (s < mylen) dh_carry = ((part[0][cb][cu] + part[1][cb][cu]) + part[2][cb][cu]) + part[3][cb][cu];
    }
}

// dW_hh[d][j][k] = sum_(b, t) dg_d[b, t, j] h_prev(b, t)[k], db_hh[d][j] = sum_(b, t) dg_d[b, t, j]; ascending b, then t.
// h_prev is out at t-1 (forward) or t+1 (reverse), 0 outside [0, T); out is 0 at t >= len, which is the reverse direction's h = 0 start.
__global__ __launch_bounds__(kThreads) void lstm_wgrad_kernel(const float* __restrict__ dg0, const float* __restrict__ dg1,
                                                              const float* __restrict__ out, float* __restrict__ dwhh, float* __restrict__ dbhh,
                                                              int B, int T, int H, int D) {
    const int G = 4 * H, cols = H + 1;
    const size_t n = (size_t)D * G * cols;
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int k = (int)(i % cols);
    const int j = (int)((i / cols) % G);
    const int dir = (int)(i / ((size_t)cols * G));
    const float* __restrict__ dg = dir ? dg1 : dg0;
    const int DH = D * H, step = dir ? 1 : -1;
    float s = 0.f;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            const float g = dg[((size_t)b * T + t) * G + j];
            if (k == H) {
                s += g;
            } else {
                const int tp = t + step;
                const float hp = (tp >= 0 && tp < T) ? out[((size_t)b * T + tp) * DH + dir * H + k] : 0.f;
                s = fmaf(g, hp, s);
            }
        }
    if (k == H)
        dbhh[(size_t)dir * G + j] = s;
    else
        dwhh[((size_t)dir * G + j) * H + k] = s;
}

unsigned blocks_for(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

bool lstm_shape_ok(int B, int T, int H, int D) { return B > 0 && T > 0 && (D == 1 || D == 2) && H >= 16 && H <= 128 && H % 16 == 0; }

// f(Int<H>) for a hidden size; the recurrent kernels run 4 * H threads (one per gate row)
template <class F> void with_hidden(int H, F&& f) {
    if (!with_int<16, 32, 48, 64, 80, 96, 112>(H, f)) f(Int<128>{});
}

}  // namespace

extern "C" {

int agan_embedding_fwd(const int64_t* ids, int ids_ld, const float* table, float* y, int B, int T, int V, int E, void* stream) {
    AGAN_REQUIRE(ids && table && y, "embedding_fwd: null pointer");
    AGAN_REQUIRE(B > 0 && T > 0 && ids_ld >= T && V > 0 && E > 0, "embedding_fwd: bad shape (B %d, T %d, ids_ld %d, V %d, E %d)", B, T, ids_ld,
                 V, E);
    const size_t n = (size_t)B * T * E;
    hipLaunchKernelGGL(embedding_fwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), ids, ids_ld, table, y, B, T, V, E);
    return check_launch("embedding_fwd");
}

int agan_embedding_bwd(const int64_t* ids, int ids_ld, const float* dy, float* dtable, int B, int T, int V, int E, void* stream) {
    AGAN_REQUIRE(ids && dy && dtable, "embedding_bwd: null pointer");
    AGAN_REQUIRE(B > 0 && T > 0 && ids_ld >= T && V > 0 && E > 0, "embedding_bwd: bad shape (B %d, T %d, ids_ld %d, V %d, E %d)", B, T, ids_ld,
                 V, E);
    hipLaunchKernelGGL(embedding_bwd_kernel, dim3((unsigned)V), dim3(kThreads), 0, as_stream(stream), ids, ids_ld, dy, dtable, B, T, E);
    return check_launch("embedding_bwd");
}

int agan_lstm_fwd(const float* xg0, const float* xg1, const float* whh0, const float* whh1, const float* bhh0, const float* bhh1,
                  const int32_t* lens, float* out, float* hN, float* gates, float* cells, int B, int T, int H, int D, void* stream) {
    AGAN_REQUIRE(lstm_shape_ok(B, T, H, D), "lstm_fwd: unsupported shape (B %d, T %d, H %d, D %d): needs B, T >= 1, D in {1, 2}, H a "
                 "multiple of 16 in 16..128", B, T, H, D);
    AGAN_REQUIRE(xg0 && whh0 && bhh0 && lens && out && hN, "lstm_fwd: null pointer");
    AGAN_REQUIRE(D == 1 || (xg1 && whh1 && bhh1), "lstm_fwd: null pointer for the reverse direction");
    AGAN_REQUIRE((gates == nullptr) == (cells == nullptr), "lstm_fwd: gates and cells are saved together or not at all");
    const dim3 grid((unsigned)cdiv(B, kRows), (unsigned)D);
    with_hidden(H, [&](auto HH) {
        hipLaunchKernelGGL(lstm_fwd_kernel<HH()>, grid, dim3(4 * HH()), 0, as_stream(stream), xg0, xg1, whh0, whh1, bhh0, bhh1, lens, out, hN, gates,
                           cells, B, T, D);
    });
    return check_launch("lstm_fwd");
}

int agan_lstm_bwd(const float* dout, const float* dhN, const float* whh0, const float* whh1, const float* gates, const float* cells,
                  const int32_t* lens, float* dg0, float* dg1, int B, int T, int H, int D, void* stream) {
    AGAN_REQUIRE(lstm_shape_ok(B, T, H, D), "lstm_bwd: unsupported shape (B %d, T %d, H %d, D %d): needs B, T >= 1, D in {1, 2}, H a "
                 "multiple of 16 in 16..128", B, T, H, D);
    AGAN_REQUIRE(whh0 && gates && cells && lens && dg0, "lstm_bwd: null pointer");
    AGAN_REQUIRE(D == 1 || (whh1 && dg1), "lstm_bwd: null pointer for the reverse direction");
    const dim3 grid((unsigned)cdiv(B, kRows), (unsigned)D);
    with_hidden(H, [&](auto HH) {
        hipLaunchKernelGGL(lstm_bwd_kernel<HH()>, grid, dim3(4 * HH()), 0, as_stream(stream), dout, dhN, whh0, whh1, gates, cells, lens, dg0, dg1, B, T, D);
    });
    return check_launch("lstm_bwd");
}

int agan_lstm_wgrad(const float* dg0, const float* dg1, const float* out, float* dwhh, float* dbhh, int B, int T, int H, int D, void* stream) {
    AGAN_REQUIRE(lstm_shape_ok(B, T, H, D), "lstm_wgrad: unsupported shape (B %d, T %d, H %d, D %d): needs B, T >= 1, D in {1, 2}, H a "
                 "multiple of 16 in 16..128", B, T, H, D);
    AGAN_REQUIRE(dg0 && out && dwhh && dbhh && (D == 1 || dg1), "lstm_wgrad: null pointer");
    const size_t n = (size_t)D * 4 * H * (H + 1);
    hipLaunchKernelGGL(lstm_wgrad_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, as_stream(stream), dg0, dg1, out, dwhh, dbhh, B, T, H, D);
    return check_launch("lstm_wgrad");
}

}  // extern "C"
