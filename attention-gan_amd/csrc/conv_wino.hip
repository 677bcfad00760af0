// Winograd F(2x2, 3x3) for the fp32 3x3 stride-1 convolutions (round 3): 16 multiplications per 2x2 outputs and channel pair instead of 36.
//
//     Y = A^T [ (G g G^T) (.) (B^T d B) ] A            d: 4x4 input patch, g: 3x3 kernel, Y: 2x2 outputs   (Lavin & Gray, correlation form)
//
// The fp32 conv kernels of this path sit at the sustained rate of the fp32 matrix pipe: the only way to make the
// generator's 3x3 layers faster in exact fp32 arithmetic is to issue fewer MFMAs.  One workgroup owns 32 Winograd tiles (2x2 outputs each:
// a 4 x 8 block of tiles, or smaller blocks of several images) x 128 (64) output channels and walks the input channels 8 at a time:
//   * the raw 8-channel patch (tiles + 1-pixel halo) goes through LDS once; thread (tile, channel) transforms its 4x4 patch (32 adds) and
//     writes the 16 transformed values V[position][tile][channel] back to LDS;
//   * wave w multiplies the four positions (xi = 0..3, nu = w): D[cout][tile] += U[pos][cout][ci] V[pos][tile][ci] on
//     v_mfma_f32_32x32x2_f32, four MFMAs per 16-byte fragment pair (a lane's 4 floats are k-steps j = 0..3, channel 4 * lh + j) --
//     the transformed weights U come from a small transform pass over the mode's ordinary packed weights ([K][Nld]: forward and
//     data-gradient packs alike, the latter already hold the flipped taps), laid out [pos][channel octet][cout][8];
//   * the output transform runs along xi in registers (a lane holds all four xi of its tile and cout), along nu through LDS (the four
//     waves), and leaves 2 x 2 pixels per lane as two 8-byte stores.
// 16 accumulator fragments per wave (256 registers): one wave per SIMD.  No bias / activation epilogue: the layers that come here are
// followed by BatchNorm (utilities/layers.py:45-53); calls with one fall back to the direct kernel.
#include "conv_common.h"

#include <cstring>
#include <type_traits>

using namespace agan;
using namespace agan::conv;

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void lds_barrier_w() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// U[pos][ch8][n][8] = (G g G^T)[pos] of g = packed[k = (c, r, s)][n]
__global__ __launch_bounds__(256) void wino_weight_transform_kernel(const float* __restrict__ wk, float* __restrict__ U, int Kin, int Nld, int N) {
    const int total = Kin * Nld;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int n = e % Nld, c = e / Nld;
        float gk[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) gk[r][s] = n < N ? wk[(size_t)(c * 9 + r * 3 + s) * Nld + n] : 0.f;
        // t = G g  (4 x 3),  u = t G^T (4 x 4);  G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
        float t[4][3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            t[0][s] = gk[0][s];
            t[1][s] = 0.5f * (gk[0][s] + gk[1][s] + gk[2][s]);
            t[2][s] = 0.5f * (gk[0][s] - gk[1][s] + gk[2][s]);
            t[3][s] = gk[2][s];
        }
        const int nch8 = Kin >> 3;
#pragma unroll
        for (int xi = 0; xi < 4; ++xi) {
            const float u0 = t[xi][0], u1 = 0.5f * (t[xi][0] + t[xi][1] + t[xi][2]), u2 = 0.5f * (t[xi][0] - t[xi][1] + t[xi][2]), u3 = t[xi][2];
            const float u[4] = {u0, u1, u2, u3};
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) U[((size_t)((xi * 4 + nu) * nch8 + (c >> 3)) * Nld + n) * 8 + (c & 7)] = u[nu];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The gather kernels are ONE program in four variants (WinoKind).  A workgroup owns a block of 32 or 64 Winograd tiles x some output
// channels and walks the input channels a chunk at a time; per chunk every wave runs `stages` groups of 4 MFMAs, and everything else the
// chunk needs stands between those groups (WinoGather::accumulate).  What differs between the variants is in this record, which
// plan_wino reads for its sizes and limits and the kernels read for theirs: one place to change.
struct WinoTraits {
    int step, extra, origin;    // raw patch of a block of T tiles per dimension: step * T + extra rows / columns from input row step * t0 + origin (class form: + py / px)
    int cch;                    // input channels per chunk
    int planes, classes;        // transformed-weight planes [plane][Cin / 8][Nld][8] in the workspace; grid entries per block that share them out (parity classes)
    int threads;                // threads of a workgroup: 256 = one wave per SIMD; 512 = two, the positions of a cout fragment split over the wave pair (w, w + 4)
    int stages, nacc;           // 4-MFMA stages per chunk and wave (wave pair: of the longer wave); accumulator fragments of a cout fragment
    int vfrags;                 // V fragments [tile][8 channels] per chunk = stages of all the waves of a cout fragment
    int pieces;                 // input-transform pieces per 32-tile group and chunk
    int ni32, ni64;             // raw staging values per thread and chunk, 32- / 64-tile blocks (0: that block size is not built)
    int lds_cap;                // dynamic LDS the kernel may ask for (80 KB: two workgroups per CU)
    int s_u_second, s_raw_load, s_u_next, s_transform, s_raw_store;      // slots of the chunk loop: the stage in front of whose MFMAs each piece of other work stands
    bool mulshift;              // item -> (row, column) of the staging map by multiply-shift (WinoPlan::mpc / mpr) instead of % and /: exact only for
                                //   items < 2048 and divisors <= 18, i.e. the 32-tile 3x3 blocks; the others stage up to 21 * 256 items with divisors up to 34
    bool store1_late;           // prologue: chunk 1's patch is loaded after chunk 0's is stored and stored after the first transform (one register set)
};
constexpr WinoTraits wino_traits(WinoKind k) {
    WinoTraits t{};
    t.origin = -1; t.classes = 1; t.lds_cap = 160 * 1024; t.s_u_second = 0; t.s_raw_load = 1; t.threads = 256;
    switch (k) {
    case WinoKind::conv3x3:             // F(2x2, 3x3), a wave = all 16 positions of one cout fragment
        t.step = 2; t.extra = 2; t.cch = 8; t.planes = 16; t.stages = 16; t.nacc = 16; t.vfrags = 16; t.pieces = 4; t.ni32 = 7; t.ni64 = 11;
        t.s_u_next = 8; t.s_transform = 1; t.s_raw_store = 14;
        break;
    case WinoKind::conv3x3_half:        // the same, a wave = half the positions; 32-tile blocks only
        t.step = 2; t.extra = 2; t.cch = 8; t.planes = 16; t.stages = 8; t.nacc = 8; t.vfrags = 16; t.pieces = 4; t.ni32 = 7;
        t.s_u_next = 4; t.s_transform = 1; t.s_raw_store = 6; t.lds_cap = 80 * 1024; t.mulshift = true;
        break;
    case WinoKind::conv4x4_s2:          // four phases of F(2x2, 2x2): 36 (phase, position) planes into 9 accumulators; built for 128-channel tiles.
                                        // Wave pair: waves 0-3 positions 0-4 of every phase (20 stages), waves 4-7 positions 5-8 (16)
        t.step = 4; t.extra = 2; t.cch = 8; t.planes = 36; t.threads = 512; t.stages = 20; t.nacc = 9; t.vfrags = 36; t.pieces = 4; t.ni32 = 11;
        t.s_transform = 2; t.s_raw_store = 14; t.store1_late = true;
        break;
    case WinoKind::dgrad2x2_class:      // F(2x2, 2x2) per parity class, 16 channels per chunk = (position, 8-channel half); 128-channel tiles.
                                        // Wave pair: waves 0-3 positions 0-4 of both octets (10 stages), waves 4-7 positions 5-8 (8)
        t.step = 2; t.extra = 1; t.cch = 16; t.planes = 36; t.classes = 4; t.threads = 512; t.stages = 10; t.nacc = 9; t.vfrags = 18; t.pieces = 2; t.ni32 = 6;
        t.s_transform = 2; t.s_raw_store = 7; t.store1_late = true;
        break;
    }
    return t;
}

// F(2x2, 2x2) input transform B^T d B of the 3x3 patch at src, every D-th row (pitch `pcp` floats) and column, B^T = [[1,-1,0],[0,1,0],[0,-1,1]]:
// nine values, `pp` floats apart from o on
template <int D>
__device__ __forceinline__ void wino_input_f22(const float* src, int pcp, float* o, int pp) {
    float t[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float d0 = src[D * j], d1 = src[D * pcp + D * j], d2 = src[2 * D * pcp + D * j];
        t[0][j] = d0 - d1; t[1][j] = d1; t[2][j] = d2 - d1;
    }
#pragma unroll
    for (int xi = 0; xi < 3; ++xi) {
        o[(xi * 3 + 0) * pp] = t[xi][0] - t[xi][1]; o[(xi * 3 + 1) * pp] = t[xi][1]; o[(xi * 3 + 2) * pp] = t[xi][2] - t[xi][1];
    }
}

// output transform Y = A^T M A of register r of the accumulators M[xi][nu] = acc[xi * N + nu]: y = {y00, y01, y10, y11}.
// 16 accumulators: A^T = [[1, 1, 1, 0], [0, 1, -1, -1]] (F(2x2, 3x3)); 9: A^T = [[1, 1, 0], [0, 1, 1]] (F(2x2, 2x2))
template <int NACC>
__device__ __forceinline__ void wino_output_2x2(const f32x16 (&acc)[NACC], int r, float (&y)[4]) {
    if constexpr (NACC == 16) {
        float c0[4], c1[4];
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) {
            c0[nu] = acc[0 + nu][r] + acc[4 + nu][r] + acc[8 + nu][r];
            c1[nu] = acc[4 + nu][r] - acc[8 + nu][r] - acc[12 + nu][r];
        }
        y[0] = c0[0] + c0[1] + c0[2]; y[1] = c0[1] - c0[2] - c0[3];
        y[2] = c1[0] + c1[1] + c1[2]; y[3] = c1[1] - c1[2] - c1[3];
    } else {
        static_assert(NACC == 9, "F(2x2, 3x3) or F(2x2, 2x2)");
        float c0[3], c1[3];
#pragma unroll
        for (int nu = 0; nu < 3; ++nu) {
            c0[nu] = acc[nu][r] + acc[3 + nu][r];
            c1[nu] = acc[3 + nu][r] + acc[6 + nu][r];
        }
        y[0] = c0[0] + c0[1]; y[1] = c0[1] + c0[2];
        y[2] = c1[0] + c1[1]; y[3] = c1[1] + c1[2];
    }
}

// The state and the pieces of one gather workgroup; NTG = 32-tile groups per workgroup (tiles = 32 NTG, cout fragments = 4 / NTG).
// Wave w owns cout fragment fw and ALL positions of tile group tg (16 / 9 accumulator fragments, one wave per SIMD): a lane then holds the
// whole product of its (tile, output channel) and the output transform never leaves its registers.  (The first version gave every wave
// one nu of all cout fragments: the nu-direction of the output transform went through 64 KB of LDS and four barriers per workgroup -- with
// one workgroup per CU that epilogue and the prologue were a third of its time.)  The half form splits the positions over the wave pair
// (fw, hh) instead: see conv_wino_h_f32_kernel.  The two F(2x2, 2x2) forms run 512 threads: the waves (fw, hh = 0 / 1) split the POSITIONS
// of their cout fragment 5 + 4 and swap accumulator halves for the output transform -- see accumulate_pair / epilogue_pair.
template <WinoKind K, int NTG>
struct WinoGather {
    static constexpr WinoTraits T = wino_traits(K);
    static constexpr bool kHalf = K == WinoKind::conv3x3_half, kS2 = K == WinoKind::conv4x4_s2, kCls = K == WinoKind::dgrad2x2_class;
    static constexpr bool k3x3 = T.nacc != 9;
    static constexpr int NT = T.threads;                           // threads of the workgroup
    static constexpr bool kPair = NT == 512;                       // two waves per SIMD: waves w and w + 4 share the stages of a cout fragment (hh = w / 4)
    static constexpr int NFW = kHalf ? 2 : 4 / NTG;                // cout fragments per workgroup
    static constexpr int NTL = 32 * NTG, LT = NTG == 1 ? 5 : 6;    // tiles per workgroup, log2 of that
    static constexpr int NI = NTG == 1 ? T.ni32 : T.ni64;          // raw staging values per thread and chunk
    static constexpr int CCH = T.cch, C8 = T.cch / 8;              // channels / channel octets per chunk
    static constexpr int S = T.stages, SH = T.stages / 2, NACC = T.nacc;
    static constexpr int NPIECE = T.pieces * NTG * 256 / NT;       // input-transform pieces per thread and chunk
    static constexpr int VBUF = T.vfrags * NTL * 8;                // floats per V buffer
    static constexpr int STEP = T.step;
    static_assert(NI > 0, "this block size of the variant is not built: plan_wino must not route to it");
    static_assert((kPair || T.s_u_next == SH) && T.s_transform + NPIECE <= S && T.s_raw_store < S, "slots of the chunk loop");
    static_assert(!kPair || (NTG == 1 && !k3x3), "wave pairs: the F(2x2, 2x2) forms on 32-tile blocks");

    const Geom& g;
    const WinoPlan& wp;
    int tid, lane, w, fw, tg, hh, l31, lh;
    int mt, nt, ks, py, px;               // ks: which part of the input channels (stride 2: partial sums to slab ks);  (py, px): parity class
    int n0, txl, tyl, TX, TY, tx0, ty0, tb0, ihw, ohw, PR, PC, PCP, RAWBUF;
    float *raw, *V;                       // LDS: raw [2 buffers][tb][CCH ci][PR][PCP];  V [2 buffers][vfrags (x C8: position)][NTL tiles][8 (CCH) ci]
    __amdgpu_buffer_rsrc_t rx, rU;
    int nch8, c_beg, nch;                 // channel octets of the layer; this workgroup's chunks: c_beg .. c_beg + nch
    int iy0, ix0;                         // first input row / column of the block's raw patch

    // (Scalars only: the register arrays of a kernel -- staging maps, patch values, weights, accumulators -- are locals of accumulate and of
    //  the kernels, each on its own, so that the compiler sees every one of them as registers from the start.)
    // ---- block and lane decode ----
    __device__ __forceinline__ WinoGather(const float* x, const float* U, const Geom& g_, const WinoPlan& wp_) : g(g_), wp(wp_) {
        extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
        tid = threadIdx.x; lane = tid & 63;
        w = __builtin_amdgcn_readfirstlane(tid >> 6);
        fw = w % NFW; tg = kHalf || kPair ? 0 : w / NFW; hh = kHalf || kPair ? w / NFW : 0;
        l31 = lane & 31; lh = lane >> 5;
        ks = py = px = 0;
        {
            int F = xcd_contiguous(linear_block_id(), wp.mtiles * wp.ntiles * (kS2 ? wp.ksplit : T.classes));
            nt = F % wp.ntiles; F /= wp.ntiles;
            if constexpr (kS2) { mt = F % wp.mtiles; ks = F / wp.mtiles; }
            else if constexpr (kCls) { py = (F & 3) >> 1; px = F & 1; mt = F >> 2; }       // (the four classes of a block read the same dy patch: neighbours)
            else mt = F;
        }
        n0 = nt * (NFW * 32);
        txl = wp.txl; tyl = wp.tyl;                                 // log2 of the tile block's columns / rows; images = NTL >> (txl + tyl)
        TX = 1 << txl; TY = 1 << tyl;
        const int bxi = mt % wp.blocks_x, byi = (mt / wp.blocks_x) % wp.blocks_y, bbi = mt / (wp.blocks_x * wp.blocks_y);
        tx0 = bxi << txl; ty0 = byi << tyl; tb0 = bbi << (LT - txl - tyl);
        ihw = g.IH * g.IW; ohw = g.OH * g.OW;
        PR = STEP * TY + T.extra; PC = STEP * TX + T.extra;       // raw patch rows / columns per image
        PCP = wp.pcp;                                              // row pitch (floats)
        raw = reinterpret_cast<float*>(lds);
        RAWBUF = wp.raw_bytes >> 2;                                // floats per raw buffer
        V = reinterpret_cast<float*>(lds + 2 * wp.raw_bytes);
        nch8 = g.Cin >> 3;
        if constexpr (kS2) { c_beg = ks * wp.chunks_per_split; nch = min(nch8, c_beg + wp.chunks_per_split) - c_beg; }
        else { c_beg = 0; nch = g.Cin >> (CCH == 8 ? 3 : 4); }
        constexpr int PPC = T.planes / T.classes;                  // weight planes of one class
        rx = make_rsrc(x, (size_t)g.B * g.Cin * ihw * sizeof(float));
        rU = make_rsrc(U + (size_t)(py * 2 + px) * PPC * nch8 * g.Nld * 8, (size_t)PPC * nch8 * g.Nld * 8 * sizeof(float));
        iy0 = STEP * ty0 + T.origin + py; ix0 = STEP * tx0 + T.origin + px;
    }

    // ---- raw staging items: (image, channel, row, column), column fastest.  it_off: element offset of (b, ci, row, col) relative to channel
    //      chunk 0, or -1;  it_lds: float offset in a raw buffer ----
    __device__ __forceinline__ void stage_items(int (&it_off)[NI], unsigned (&it_lds)[NI]) const {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            // (wave pairs: a thread past the patch's last item takes the last item again -- the same value to the same place -- so that
            //  neither the loads nor the LDS stores of the chunk loop need a per-item predicate)
            const int e = kPair ? min(tid + i * NT, wp.raw_items - 1) : tid + i * NT;
            int col, row, t2;                                // t2 = (image of the block, channel of the chunk)
            if constexpr (T.mulshift) {                            // e / d = (e * ceil(65536 / d)) >> 16: two VALU instructions instead of the ~12 of a
                const int t1 = (int)(__umul24(e, wp.mpc) >> 16);   // general division; 24-bit multiplies are full rate
                col = e - (int)__umul24(t1, PC);
                t2 = (int)(__umul24(t1, wp.mpr) >> 16); row = t1 - (int)__umul24(t2, PR);
            } else {
                col = e % PC; const int t1 = e / PC;
                row = t1 % PR; t2 = t1 / PR;
            }
            const int ci = t2 & (CCH - 1), b = tb0 + (t2 >> (CCH == 8 ? 3 : 4)), iy = iy0 + row, ix = ix0 + col;
            const bool ok = (e < wp.raw_items) & (b < g.B) & ((unsigned)iy < (unsigned)g.IH) & ((unsigned)ix < (unsigned)g.IW);
            if constexpr (T.mulshift) {
                it_off[i] = ok ? (int)__umul24(b * g.Cin + ci, ihw) + iy * g.IW + ix : -1;
                it_lds[i] = (unsigned)((int)__umul24(__umul24(t2, PR) + row, PCP) + col);
            } else {
                // wave pairs: the byte offset of the load, or kOOB (= -1), formed here once
                it_off[i] = ok ? ((b * g.Cin + ci) * ihw + iy * g.IW + ix) * (kPair ? 4 : 1) : -1;
                it_lds[i] = (unsigned)((t2 * PR + row) * PCP + col);
            }
        }
    }

    __device__ __forceinline__ void load_raw(const int (&it_off)[NI], int ch, float (&rv)[NI]) const {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if constexpr (kPair) rv[i] = buf_load_s(rx, (unsigned)it_off[i], (unsigned)((c_beg + ch) * CCH * ihw) * 4u);
            else rv[i] = buf_load_s(rx, it_off[i] >= 0 ? (unsigned)it_off[i] * 4u : kOOB, (unsigned)((c_beg + ch) * CCH * ihw) * 4u);
        }
    }
    __device__ __forceinline__ void store_raw(const unsigned (&it_lds)[NI], int ch, const float (&rv)[NI]) const {      // chunk ch's patch -> raw buffer ch & 1
        float* const rb = raw + (ch & 1) * RAWBUF;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (kPair || tid + i * NT < wp.raw_items) rb[it_lds[i]] = rv[i];
    }
    // half a chunk's stages at a time, so that two register sets of SH fragments suffice.  Stage s of wave half hh: plane hh * S + s / C8,
    // channel octet s % C8 of the chunk (past the last chunk: a harmless repeat of it)
    __device__ __forceinline__ void load_u(int ch, int half, u32x4 (&uf)[SH]) const {
        // this wave's cout fragment of U: 16 bytes (channels 4 * lh ..) per lane and plane  (rows past Cout are zero in U)
        const unsigned ulane = (unsigned)(min(n0 + fw * 32 + l31, g.Nld - 1) * 32 + lh * 16);
#pragma unroll
        for (int q = 0; q < SH; ++q) {
            const int s = half * SH + q;
            uf[q] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                rU, ulane, (unsigned)(((hh * S + s / C8) * nch8 + (c_beg + min(ch, nch - 1)) * C8 + s % C8) * g.Nld) * 32u, 0));
        }
    }

    // ---- input transform of the raw patch rb into Vb, piece pi of NPIECE: thread (tile tt = (tid >> 3) + 32 k, channel tid & 7 (+ 8)).
    //      F(2x2, 3x3): one output row xi of tile group k (t = B^T d at xi = 0: rows (d0 - d2, d1 + d2, d2 - d1, d1 - d3); v = t B: columns
    //      likewise; td keeps t between the pieces);  stride 2: one phase (p, q) -- every second row / column of the tile's 6 x 6 pixels;
    //      class form: one channel half ----
    __device__ __forceinline__ void transform_piece(const float* rb, float* Vb, int pi, float (&td)[NTG][4][4]) const {
        // (wave pairs: threads 256 .. 511 -- waves 4 - 7, hh = 1 -- take the second half of the pieces: stride 2 phases 2, 3, class form channels 8 - 15)
        const int k = kPair ? 0 : pi / T.pieces, sub = kPair ? hh * NPIECE + pi : pi % T.pieces;
        const int tt = (kPair ? (tid >> 3) & 31 : tid >> 3) + 32 * k, ci = (tid & 7) + (kCls ? 8 * sub : 0);
        const int p = kS2 ? sub >> 1 : 0, q = kS2 ? sub & 1 : 0;
        if (!k3x3 || sub == 0) {
            const int ttx = tt & (TX - 1), tty = (tt >> txl) & (TY - 1), ttb = tt >> (txl + tyl);
            const float* const src = rb + ((ttb * CCH + ci) * PR + STEP * tty + p) * PCP + STEP * ttx + q;
            if constexpr (k3x3) {
                float d[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float2 a = *reinterpret_cast<const float2*>(src + i * PCP), b = *reinterpret_cast<const float2*>(src + i * PCP + 2);
                    d[i][0] = a.x; d[i][1] = a.y; d[i][2] = b.x; d[i][3] = b.y;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    td[k][0][j] = d[0][j] - d[2][j];
                    td[k][1][j] = d[1][j] + d[2][j];
                    td[k][2][j] = d[2][j] - d[1][j];
                    td[k][3][j] = d[1][j] - d[3][j];
                }
            } else if constexpr (kS2) wino_input_f22<2>(src, PCP, Vb + (sub * 9 * NTL + tt) * 8 + ci, NTL * 8);
            else wino_input_f22<1>(src, PCP, Vb + tt * 16 + ci, NTL * 16);
        }
        if constexpr (k3x3) {
            const float (&t)[4] = td[k][sub];
            float* const o = Vb + (sub * 4 * NTL + tt) * 8 + ci;
            o[0] = t[0] - t[2]; o[NTL * 8] = t[1] + t[2]; o[2 * NTL * 8] = t[2] - t[1]; o[3 * NTL * 8] = t[1] - t[3];
        }
    }

    // ---- acc = this wave's products over the workgroup's input channels ----
    __device__ __forceinline__ void accumulate(f32x16 (&acc)[NACC]) const {
        int it_off[NI];
        unsigned it_lds[NI];
        stage_items(it_off, it_lds);
        float rawv[NI];
        float td[NTG][4][4];
        u32x4 ua[SH], ub[SH];             // weights of the first / second half of the stages: each set is reloaded while the other one's products run
#pragma unroll
        for (int q = 0; q < NACC; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
        {   // prologue: the patches of chunks 0 and 1 on their way, chunk 0 transformed, the first weights loaded
            float rawv1[NI];
            load_raw(it_off, 0, rawv);
            if (!T.store1_late && nch > 1) load_raw(it_off, 1, rawv1);
            load_u(0, 0, ua);
            store_raw(it_lds, 0, rawv);
            if (nch > 1) {
                if constexpr (T.store1_late) load_raw(it_off, 1, rawv);
                else store_raw(it_lds, 1, rawv1);
            }
            lds_barrier_w();
#pragma unroll
            for (int pi = 0; pi < NPIECE; ++pi) transform_piece(raw, V, pi, td);
            if (T.store1_late && nch > 1) store_raw(it_lds, 1, rawv);
            lds_barrier_w();
        }
        // S stages per chunk: [V fragment of the NEXT stage] [a piece of the other work] [this stage's 4 MFMAs = 256 cycles of the matrix
        // pipe].  The wave issues in order, so whatever must hide behind the MFMAs has to stand between them in program order;
        // sched_barrier pins the stages.  Other work of chunk ch, at the slots of WinoTraits: the second half of its weights and the first
        // half of the next chunk's, the global loads of chunk ch + 2's raw patch and, late, their LDS stores (into the buffer chunk ch's
        // patch has left), the input transform of chunk ch + 1 piece by piece.  ONE barrier per chunk.
        // (unroll 1: the body is one pinned schedule -- left alone, the compiler peels the last chunk off the loop: every MFMA twice in the code)
#pragma unroll 1
        for (int ch = 0; ch < nch; ++ch) {
            const float* Vc = V + (ch & 1) * VBUF;
            float* Vn = V + ((ch + 1) & 1) * VBUF;
            const float* rn = raw + ((ch + 1) & 1) * RAWBUF;      // the raw patch of chunk ch + 1: in LDS since the last barrier
            const bool more = ch + 1 < nch;
            // stage st reads V fragment hh * S + st: position st / C8 (pitch NTL * CCH), channel octet st % C8, and feeds accumulator st / C8
            // (stride 2: st % 9 -- the four phases share the nine)
            const unsigned vlane = (unsigned)(hh * S * NTL * 8 + (tg * 32 + l31) * CCH + lh * 4);
            u32x4 vf[2];
            vf[0] = *reinterpret_cast<const u32x4*>(Vc + vlane);
#pragma unroll
            for (int st = 0; st < S; ++st) {
                if (st + 1 < S) vf[(st + 1) & 1] = *reinterpret_cast<const u32x4*>(Vc + ((st + 1) / C8) * NTL * CCH + ((st + 1) % C8) * 8 + vlane);
                if (st == T.s_u_second) load_u(ch, 1, ub);
                if (st == T.s_raw_load && ch + 2 < nch) load_raw(it_off, ch + 2, rawv);
                if (st == T.s_u_next) load_u(ch + 1, 0, ua);
                if (more && st >= T.s_transform && st < T.s_transform + NPIECE) transform_piece(rn, Vn, st - T.s_transform, td);
                if (st == T.s_raw_store && ch + 2 < nch) store_raw(it_lds, ch + 2, rawv);
                const u32x4 uf = st < SH ? ua[st % SH] : ub[st % SH];
                const int a = kS2 ? st % NACC : st / C8;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(uf[j]), __uint_as_float(vf[st & 1][j]), acc[a], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            lds_barrier_w();                                      // V of chunk ch + 1 and the raw patch of chunk ch + 2 are complete; every wave is done with chunk ch
        }
    }

    // ---- the same for a wave pair (512 threads, two waves per SIMD): waves (fw, hh = 0 / 1) split the POSITIONS of their cout fragment --
    //      hh = 0 positions 0 - 4 (five accumulator fragments), hh = 1 positions 5 - 8 (four) -- and run every phase / channel octet of
    //      theirs, in the order the one-wave form runs them: an accumulator sums the same products in the same order as before, so the
    //      results are bit for bit what they were.  Stride 2: stage st = (phase st / NP, position P0 + st % NP); class form: (position
    //      P0 + st / 2, channel octet st % 2).  Every thread stages half the raw items and transforms half the pieces.  A wave's own VALU
    //      instructions are not hidden by its own MFMAs, its partner's are.  epilogue_pair exchanges accumulator halves. ----
    template <int HH>
    struct Half {
        static constexpr int P0 = HH ? 5 : 0, NP = HH ? 4 : 5;      // this wave's positions: P0 .. P0 + NP - 1
        static constexpr int SW = (kS2 ? 4 : 2) * NP, SWH = SW / 2; // stages per chunk of this wave; per weight register set
        static constexpr int pos(int st) { return P0 + (kS2 ? st % NP : st / 2); }
        static constexpr int sub(int st) { return kS2 ? st / NP : st % 2; }      // phase / channel octet of the stage
    };
    template <int HH>
    __device__ __forceinline__ void load_u_half(int ch, int half, u32x4 (&uf)[Half<0>::SWH]) const {
        using H = Half<HH>;
        const unsigned ulane = (unsigned)(min(n0 + fw * 32 + l31, g.Nld - 1) * 32 + lh * 16);
        const int c = c_beg + min(ch, nch - 1);
#pragma unroll
        for (int q = 0; q < H::SWH; ++q) {
            const int st = half * H::SWH + q;
            const int row = kS2 ? (H::sub(st) * 9 + H::pos(st)) * nch8 + c : H::pos(st) * nch8 + c * C8 + H::sub(st);      // (plane, channel octet)
            uf[q] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rU, ulane, (unsigned)(row * g.Nld) * 32u, 0));
        }
    }
    template <int HH>
    __device__ __forceinline__ void accumulate_pair(f32x16 (&acc)[Half<0>::NP]) const {
        using H = Half<HH>;
        static_assert(T.s_transform + NPIECE <= Half<1>::SW && T.s_raw_store < Half<1>::SW && T.s_raw_load < T.s_raw_store, "slots of the chunk loop");
        int it_off[NI];
        unsigned it_lds[NI];
        stage_items(it_off, it_lds);
        float rawv[NI];
        float td[NTG][4][4];              // (F(2x2, 3x3) only: unused here)
        u32x4 ua[Half<0>::SWH], ub[Half<0>::SWH];      // weights of the first / second half of the stages, as in accumulate
#pragma unroll
        for (int q = 0; q < H::NP; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
        {   // prologue, as accumulate's with one raw register set
            load_raw(it_off, 0, rawv);
            load_u_half<HH>(0, 0, ua);
            store_raw(it_lds, 0, rawv);
            if (nch > 1) load_raw(it_off, 1, rawv);
            lds_barrier_w();
#pragma unroll
            for (int pi = 0; pi < NPIECE; ++pi) transform_piece(raw, V, pi, td);
            if (nch > 1) store_raw(it_lds, 1, rawv);
            lds_barrier_w();
        }
        // V fragment of a stage: stride 2 fragment (phase, position), pitch NTL * 8; class form position (pitch NTL * 16), channel octet
        const unsigned vlane = (unsigned)(l31 * CCH + lh * 4);
        auto voff = [](int st) { return kS2 ? (H::sub(st) * 9 + H::pos(st)) * NTL * 8 : H::pos(st) * NTL * 16 + H::sub(st) * 8; };
#pragma unroll 1
        for (int ch = 0; ch < nch; ++ch) {
            const float* Vc = V + (ch & 1) * VBUF + vlane;
            float* Vn = V + ((ch + 1) & 1) * VBUF;
            const float* rn = raw + ((ch + 1) & 1) * RAWBUF;
            u32x4 vf[2];
            vf[0] = *reinterpret_cast<const u32x4*>(Vc + voff(0));
#pragma unroll
            for (int st = 0; st < H::SW; ++st) {
                if (st + 1 < H::SW) vf[(st + 1) & 1] = *reinterpret_cast<const u32x4*>(Vc + voff(st + 1));
                if (st == 0) load_u_half<HH>(ch, 1, ub);
                if (st == H::SWH) load_u_half<HH>(ch + 1, 0, ua);
                // no branch around the other work (past the last chunk it loads the last patch again and transforms into the buffers nobody
                // reads any more): one basic block per stage, so that the pieces can be issued BETWEEN the stage's four MFMAs (below)
                if (st == T.s_raw_load) load_raw(it_off, min(ch + 2, nch - 1), rawv);
                if (st >= T.s_transform && st < T.s_transform + NPIECE) transform_piece(rn, Vn, st - T.s_transform, td);
                if (st == T.s_raw_store) store_raw(it_lds, ch + 2, rawv);
                const u32x4 uf = st < H::SWH ? ua[st % H::SWH] : ub[st % H::SWH];
                const int a = H::pos(st) - H::P0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(uf[j]), __uint_as_float(vf[st & 1][j]), acc[a], 0, 0, 0);
                // a wave issues in order: what FOLLOWS four back-to-back MFMAs waits for all of them, what stands in front delays them.  The
                // stage's other instructions are spread over the four 64-cycle shadows instead (as in conv_wino_wgrad_f32_kernel)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);          // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);          // DS read
                    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);          // VALU
                    __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);          // VMEM read
                    __builtin_amdgcn_sched_group_barrier(0x200, 3, 0);          // DS write
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            lds_barrier_w();
        }
    }

    // ---- output transform in registers, 2 x 2 pixels per lane and register: two 8-byte stores; class form: lattice point (yq, xq) -> pixel
    //      (2 yq + py, 2 xq + px), the four outputs lie two pixels apart (scalar stores) ----
    __device__ __forceinline__ void epilogue(const f32x16 (&acc)[NACC], float* out) const {
        typedef float f32x2_ __attribute__((ext_vector_type(2)));
        typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
        const int lt = tg * 32 + l31;
        const int tx = lt & (TX - 1), ty = (lt >> txl) & (TY - 1), tb = lt >> (txl + tyl);
        const int b = tb0 + tb, oy = 2 * (ty0 + ty), ox = 2 * (tx0 + tx);
        const bool pvalid = (b < g.B) & (oy < (kCls ? g.OHs : g.OH)) & (ox < (kCls ? g.OWs : g.OW));
        const __amdgpu_buffer_rsrc_t ro = make_rsrc(out + (size_t)ks * wp.slab, (size_t)g.B * g.Cout * ohw * sizeof(float));
        const int nw = n0 + fw * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float y[4];
            wino_output_2x2(acc, r, y);
            const int n = nw + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const bool ok = pvalid & (n < g.Cout);
            if constexpr (kCls) {
                const unsigned off = (unsigned)((b * g.Cout + n) * ohw + (2 * oy + py) * g.OW + 2 * ox + px) * 4u;
                buf_store(ro, ok ? off : kOOB, y[0]);
                buf_store(ro, ok ? off + 8u : kOOB, y[1]);
                buf_store(ro, ok ? off + (unsigned)(2 * g.OW) * 4u : kOOB, y[2]);
                buf_store(ro, ok ? off + (unsigned)(2 * g.OW + 2) * 4u : kOOB, y[3]);
            } else {
                const unsigned off = (unsigned)((b * g.Cout + n) * ohw + oy * g.OW + ox) * 4u;
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_, f32x2_{y[0], y[1]}), ro, ok ? off : kOOB, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_, f32x2_{y[2], y[3]}), ro, ok ? off + (unsigned)g.OW * 4u : kOOB, 0, 0);
            }
        }
    }

    // ---- the epilogue of a wave pair: the output transform needs the nine positions of a (tile, cout) pair in one lane.  After the chunk
    //      loop the operand buffers are dead: every wave leaves the half of its accumulators that its partner finishes (its positions x 8
    //      registers, 16 bytes per lane and slot, at most 10 slots: 80 KB per workgroup) in LDS, ONE barrier, and the lower group
    //      finishes registers 0 - 7 of the fragment, the upper group registers 8 - 15, with the additions of wino_output_2x2 in the
    //      order they have there ----
    template <int HH>
    __device__ __forceinline__ void epilogue_pair(const f32x16 (&acc)[Half<0>::NP], float* out) const {
        using H = Half<HH>;
        using O = Half<1 - HH>;
        typedef float f32x2_ __attribute__((ext_vector_type(2)));
        typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
        const int tx = l31 & (TX - 1), ty = (l31 >> txl) & (TY - 1), tb = l31 >> (txl + tyl);
        const int b = tb0 + tb, oy = 2 * (ty0 + ty), ox = 2 * (tx0 + tx);
        const bool pvalid = (b < g.B) & (oy < (kCls ? g.OHs : g.OH)) & (ox < (kCls ? g.OWs : g.OW));
        const __amdgpu_buffer_rsrc_t ro = make_rsrc(out + (size_t)ks * wp.slab, (size_t)g.B * g.Cout * ohw * sizeof(float));
        // lane part of the addresses once; the register's channel (r & 3) + 8 (r >> 2) goes into the scalar offset
        const int nl = n0 + fw * 32 + 4 * lh;
        const unsigned vp = pvalid ? (unsigned)((b * g.Cout + nl) * ohw + (kCls ? (2 * oy + py) * g.OW + 2 * ox + px : oy * g.OW + ox)) * 4u : kOOB;
        f32x4* const X = reinterpret_cast<f32x4*>(raw);          // [wave 8][slot 10][lane 64]
#pragma unroll
        for (int q = 0; q < H::NP; ++q)
#pragma unroll
            for (int rq = 0; rq < 2; ++rq) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[q][8 * (1 - HH) + 4 * rq + e];
                X[(w * 10 + q * 2 + rq) * 64 + lane] = v;
            }
        lds_barrier_w();
#pragma unroll
        for (int rq = 0; rq < 2; ++rq) {
            f32x4 oth[O::NP];                                    // the partner's positions of registers 8 HH + 4 rq ... + 3
#pragma unroll
            for (int q = 0; q < O::NP; ++q) oth[q] = X[((w ^ 4) * 10 + q * 2 + rq) * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 8 * HH + 4 * rq + e;
                float m[9];
#pragma unroll
                for (int p = 0; p < 9; ++p) m[p] = (p >= H::P0 && p < H::P0 + H::NP) ? acc[p - H::P0][r] : oth[p - O::P0][e];
                float c0[3], c1[3];                              // wino_output_2x2's F(2x2, 2x2) form, term for term
#pragma unroll
                for (int nu = 0; nu < 3; ++nu) {
                    c0[nu] = m[nu] + m[3 + nu];
                    c1[nu] = m[3 + nu] + m[6 + nu];
                }
                const float y[4] = {c0[0] + c0[1], c0[1] + c0[2], c1[0] + c1[1], c1[1] + c1[2]};
                const int dn = (r & 3) + 8 * (r >> 2);
                const unsigned vo = nl + dn < g.Cout ? vp : kOOB;
                const unsigned so = (unsigned)(dn * ohw) * 4u;
                if constexpr (kCls) {
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[0]), ro, vo, so, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[1]), ro, vo, so + 8u, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[2]), ro, vo, so + (unsigned)(2 * g.OW) * 4u, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[3]), ro, vo, so + (unsigned)(2 * g.OW + 2) * 4u, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_, f32x2_{y[0], y[1]}), ro, vo, so, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_, f32x2_{y[2], y[3]}), ro, vo, so + (unsigned)g.OW * 4u, 0);
                }
            }
        }
    }
    // one wave of the pair, start to end
    template <int HH>
    __device__ __forceinline__ void run_pair(float* out) const {
        f32x16 acc[Half<0>::NP];
        accumulate_pair<HH>(acc);
        epilogue_pair<HH>(acc, out);
    }
};

// F(2x2, 3x3), conv3x3 stride 1.  NFW = cout fragments per workgroup: 4 (128 output channels x 32 tiles) or 2 (64 output channels x 64 tiles).
template <int NFW>
__global__ __launch_bounds__(256, 1) void conv_wino_f32_kernel(const float* __restrict__ x, const float* __restrict__ U, float* __restrict__ out,
                                                               const Geom g, const WinoPlan wp) {
    WinoGather<WinoKind::conv3x3, 4 / NFW> k(x, U, g, wp);
    f32x16 acc[k.NACC];
    k.accumulate(acc);
    k.epilogue(acc, out);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same F(2x2, 3x3) gather with TWO workgroups per CU: 32 tiles x 64 output channels per workgroup, a wave = one cout fragment x HALF
// the positions (rows xi = 2 h, 2 h + 1 of the 4 x 4 product: 128 accumulator registers).  One workgroup per CU left its fixed cost --
// first loads, last stores, every barrier -- uncovered (~5 us of 26); two co-resident workgroups cover each other's.  The price: every
// (tile, channel) patch is transformed by both cout halves, and the output transform's row direction crosses the two waves of a cout
// fragment: each wave reduces its two rows to the partial sums of the two output rows and hands ONE of them to its partner through LDS
// (32 floats per lane), then finishes the other.
__global__ __launch_bounds__(256, 2) void conv_wino_h_f32_kernel(const float* __restrict__ x, const float* __restrict__ U, float* __restrict__ out,
                                                                 const Geom g, const WinoPlan wp) {
    WinoGather<WinoKind::conv3x3_half, 1> k(x, U, g, wp);
    f32x16 acc[8];
    k.accumulate(acc);

    // ---- output transform: columns in registers, rows across the wave pair (fw, hh = 0 / 1).  acc[x2 * 4 + nu] = M[2 hh + x2][nu].
    //      hh = 0 holds rows 0, 1: output row 0 gets M0 + M1, row 1 gets M1;   hh = 1 holds rows 2, 3: row 0 gets M2, row 1 gets -M2 - M3.
    //      Wave hh finishes output row hh and sends its contribution to the other row to its partner.
    //      The fp32 MFMA and the vector ALU do not overlap on gfx950 (profiles/micro/mfma_issue.hip) and this kernel runs only 256 MFMAs per
    //      wave: every VALU instruction here is ~0.04 % of the workgroup.  So: packed adds on (r, r + 1) register pairs (consecutive
    //      accumulator registers: no moves), one code path per hh (no selects), the register-dependent part of the store address in
    //      the scalar offset. ----
    const int w = k.w, lane = k.lane, hh = k.hh, ohw = k.ohw;
    float* const X = k.raw;                                     // [wave 4][32 values][64 lanes]
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
    const int tx = k.l31 & (k.TX - 1), ty = (k.l31 >> k.txl) & (k.TY - 1), tb = k.l31 >> (k.txl + k.tyl);
    const int b = k.tb0 + tb, oy = 2 * (k.ty0 + ty) + hh, ox = 2 * (k.tx0 + tx);
    const bool pvalid = (b < g.B) & (oy < g.OH) & (ox < g.OW);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out, (size_t)g.B * g.Cout * ohw * sizeof(float));
    const int nw = k.n0 + k.fw * 32, pw = w ^ 2;                // partner wave: same cout fragment, other position half
    const unsigned vo = pvalid ? (unsigned)((b * g.Cout + nw + 4 * k.lh) * ohw + oy * g.OW + ox) * 4u : kOOB;
    auto finish = [&](auto hc) {
        constexpr int HH = decltype(hc)::value;
        f32x2_ keep[8][2];                                       // [register pair][output column]; HH = 1: the NEGATIVE of its share
#pragma unroll
        for (int rp = 0; rp < 8; ++rp) {
            f32x2_ t[2][2];                                      // [x2][output column]
#pragma unroll
            for (int x2 = 0; x2 < 2; ++x2) {
                const f32x2_ m0 = {acc[x2 * 4 + 0][2 * rp], acc[x2 * 4 + 0][2 * rp + 1]};
                const f32x2_ m1 = {acc[x2 * 4 + 1][2 * rp], acc[x2 * 4 + 1][2 * rp + 1]};
                const f32x2_ m2 = {acc[x2 * 4 + 2][2 * rp], acc[x2 * 4 + 2][2 * rp + 1]};
                const f32x2_ m3 = {acc[x2 * 4 + 3][2 * rp], acc[x2 * 4 + 3][2 * rp + 1]};
                t[x2][0] = m0 + m1 + m2;
                t[x2][1] = m1 - m2 - m3;
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                keep[rp][c] = t[0][c] + t[1][c];
                const f32x2_ send = HH == 0 ? t[1][c] : t[0][c];
                X[(w * 32 + (2 * rp) * 2 + c) * 64 + lane] = send[0];
                X[(w * 32 + (2 * rp + 1) * 2 + c) * 64 + lane] = send[1];
            }
        }
        lds_barrier_w();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // channels nw + (r & 3) + 8 (r >> 2) + 4 lh: a group of 8 is valid or not as a whole (Cout is a multiple of 8: plan_wino)
            if (nw + 8 * (r >> 2) < g.Cout) {
                const float x0 = X[(pw * 32 + r * 2 + 0) * 64 + lane], x1 = X[(pw * 32 + r * 2 + 1) * 64 + lane];
                const float k0 = keep[r >> 1][0][r & 1], k1 = keep[r >> 1][1][r & 1];
                const f32x2_ y = HH == 0 ? f32x2_{x0 + k0, x1 + k1} : f32x2_{x0 - k0, x1 - k1};
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_, y), ro, vo, (unsigned)(((r & 3) + 8 * (r >> 2)) * ohw) * 4u, 0);
            }
        }
    };
    if (hh == 0) finish(std::integral_constant<int, 0>{});
    else finish(std::integral_constant<int, 1>{});
}

// ---------------------------------------------------------------------------------------------------------------------------------
// conv4x4 stride 2 pad 1 (the discriminators' down-sampling convs), forward: polyphase + Winograd F(2x2, 2x2).
//     out[oy][ox] = sum_{r,s} w[r][s] x[2 oy + r - 1][2 ox + s - 1]:  the odd input rows O[i] = x[2i + 1] see the taps r = 0, 2 (at O[oy - 1],
//     O[oy]), the even rows E[i] = x[2i] the taps r = 1, 3 (at E[oy], E[oy + 1]) -- per dimension two 2-tap stride-1 filters on the two
//     phase images, in 2-D four phases (p, q) of 2x2 taps.  Each is F(2x2, 2x2): 2x2 outputs from a 3x3 phase patch with 9 products
//     instead of 16:   B^T = [[1,-1,0],[0,1,0],[0,-1,1]],  G = [[1,0],[1,1],[0,1]],  A^T = [[1,1,0],[0,1,1]]  (all +-1: exact transforms
//     up to the adds).  The output transform is the same for the four phases, so their products are summed in the SAME nine
//     accumulators: 36 products per 2x2 outputs and input channel instead of 64.
// 32 tiles x 128 output channels per workgroup, input channels 8 at a time = 36 stages (phase, position); the raw patch of a tile is 6 x 6
// pixels (rows / columns 4 t .. 4 t + 5 of the block's patch).  8 waves, two per SIMD: waves w and w + 4 share cout fragment w -- positions
// 0-4 of the four phases in waves 0-3 (80 accumulator registers, 20 stages), positions 5-8 in waves 4-7 (64, 16 stages); every
// accumulator sums its products in the order of the one-wave form -- and swap accumulator halves once, in the epilogue
// (WinoGather::accumulate_pair / epilogue_pair).
template <int NFW>
__global__ __launch_bounds__(512, 1) void conv_wino_s2_f32_kernel(const float* __restrict__ x, const float* __restrict__ U, float* __restrict__ out,
                                                                  const Geom g, const WinoPlan wp) {
    WinoGather<WinoKind::conv4x4_s2, 4 / NFW> k(x, U, g, wp);
    if (k.hh == 0) k.template run_pair<0>(out);
    else k.template run_pair<1>(out);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Data gradient of conv4x4 stride 2: four parity classes of the output, each a 2x2-tap stride-1 gather over dy with taps running backwards
// (include/agan.h: DY = -1, offsets (0, 1)).  Per class Winograd F(2x2, 2x2) on the class lattice: 9 products per 2x2 lattice points instead of
// 16.  out[2 yq + py][2 xq + px] = sum_{r,s} Wc[r][s] dy[yq + py - r][xq + px - s] = correlation of the ascending window
// (dy[yq + py - 1], dy[yq + py]) with g = (Wc[1], Wc[0]).  A channel chunk is 16 channels = 18 stages (position, 8-channel half); the
// four classes are grid entries.  8 waves, two per SIMD: waves w and w + 4 share cout fragment w, positions 0-4 / 5-8 of both channel
// octets (10 / 8 stages per wave), and swap accumulator halves in the epilogue as the stride-2 forward does.
template <int NFW>
__global__ __launch_bounds__(512, 1) void conv_wino_cls_f32_kernel(const float* __restrict__ x, const float* __restrict__ U, float* __restrict__ out,
                                                                   const Geom g, const WinoPlan wp) {
    WinoGather<WinoKind::dgrad2x2_class, 4 / NFW> k(x, U, g, wp);
    if (k.hh == 0) k.template run_pair<0>(out);
    else k.template run_pair<1>(out);
}

// (G g G^T) of a 2x2 kernel g, G = [[1,0],[1,1],[0,1]]: nine planes [xi * 3 + nu], `pp` floats apart from o on
__device__ __forceinline__ void wino_weights_f22(const float (&gk)[2][2], float* o, size_t pp) {
    const float t[3][2] = {{gk[0][0], gk[0][1]}, {gk[0][0] + gk[1][0], gk[0][1] + gk[1][1]}, {gk[1][0], gk[1][1]}};
#pragma unroll
    for (int xi = 0; xi < 3; ++xi) {
        const float u[3] = {t[xi][0], t[xi][0] + t[xi][1], t[xi][1]};
#pragma unroll
        for (int nu = 0; nu < 3; ++nu) o[(xi * 3 + nu) * pp] = u[nu];
    }
}

// U[cls][xi * 3 + nu][ch8][n][8] = (G g G^T)[xi][nu],  g[a][b] = packed_cls[(c, r = 1 - a, s = 1 - b)][n]   (taps run backwards: DY = -1)
__global__ __launch_bounds__(256) void wino_cls_weight_transform_kernel(const float* __restrict__ wk, float* __restrict__ U, int Kin, int Nld, int N) {
    const int total = 4 * Kin * Nld, nch8 = Kin >> 3;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int n = e % Nld, t1 = e / Nld, c = t1 % Kin, cls = t1 / Kin;
        const float* wc = wk + (size_t)cls * Kin * 4 * Nld;
        float gk[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) gk[a][b] = n < N ? wc[(size_t)(c * 4 + (1 - a) * 2 + (1 - b)) * Nld + n] : 0.f;
        wino_weights_f22(gk, U + ((size_t)(cls * 9 * nch8 + (c >> 3)) * Nld + n) * 8 + (c & 7), (size_t)nch8 * Nld * 8);
    }
}

// U[(p * 2 + q) * 9 + xi * 3 + nu][ch8][n][8] = (G g_pq G^T)[xi][nu],  g_pq[a][b] = packed[(c, r = 2a + p, s = 2b + q)][n]
__global__ __launch_bounds__(256) void wino_s2_weight_transform_kernel(const float* __restrict__ wk, float* __restrict__ U, int Kin, int Nld, int N) {
    const int total = Kin * Nld, nch8 = Kin >> 3;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int n = e % Nld, c = e / Nld;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float gk[2][2];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) gk[a][b] = n < N ? wk[(size_t)(c * 16 + (2 * a + p) * 4 + 2 * b + q) * Nld + n] : 0.f;
                wino_weights_f22(gk, U + ((size_t)((p * 2 + q) * 9 * nch8 + (c >> 3)) * Nld + n) * 8 + (c & 7), (size_t)nch8 * Nld * 8);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Weight gradient of the same layers, Winograd F(3x3, 2x2):  dw[r][s] = sum over 2x2 dy tiles e  of  corr(d, e)[r][s],  d = the tile's
// 4x4 x patch:   dw = A^T [ sum_tiles (G e G^T) (.) (B^T d B) ] A     A^T = [[1,1,1,0],[0,1,-1,0],[0,1,1,1]],
//                G = [[1,0],[.5,.5],[.5,-.5],[0,1]],  B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,-1,0,1]]      (16 products per tile instead of 36).
// The contraction index of the 16 products is the TILE: both operands are transformed activations, staged [position][channel][8 tiles]
// in LDS (a lane's 16 bytes = 4 k-steps of its channel), produced by the threads straight from global memory (a thread loads its tile's
// 4x4 x patch / 2x2 dy tile, transforms it and writes 16 values; no raw copy in LDS).  A workgroup owns 64 output x 64 input channels
// and a range of tile octets.  It has 8 waves, TWO per SIMD: waves 0-3 hold one 32 x 32 fragment pair each for positions 0-7, waves 4-7
// the same fragment pairs for positions 8-15 (128 accumulator registers per wave, 32 MFMAs per octet), and each of the 512 threads
// produces ONE (tile, channel) pair of each operand.  A wave's own VALU work is not hidden by its own MFMAs, another wave's is (DESIGN
// section 4), and two waves running the same program stay in phase -- so the two groups are offset by construction: the lower group
// transforms / loads in the first four of its eight stages of an octet and only multiplies in the last four, the upper group the other
// way round (measured: no faster than both groups on the same stages -- what pays is two waves per SIMD and few VALU instructions
// per wave).  ONE barrier per octet.  The output transform needs all 16 positions: after the octet loop the groups swap halves of their
// accumulators through LDS (the operand buffers are dead by then) -- the lower group finishes registers 0-7 of the fragment, the upper
// group registers 8-15.  Partial results [tap][cout][cin] per pixel split, summed by wino_wgrad_sum_kernel.
__global__ __launch_bounds__(512, 1) void conv_wino_wgrad_f32_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
                                                                     const Geom g, const WinoWgradPlan wp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int ZV = 16 * 64 * 8;                               // floats of one operand image [pos][64 channels][8 tiles]
    float* const L = reinterpret_cast<float*>(lds);               // [2 buffers][Z | V]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int up = w >> 2;                                        // position half of this wave: positions 8 * up ... + 7
    const int fj = w & 1, fi = (w >> 1) & 1;                      // cout / cin fragment of this wave
    const int l31 = lane & 31, lh = lane >> 5;
    int jt, it, split;
    {
        int F = xcd_contiguous(linear_block_id(), wp.jtiles * wp.itiles * wp.psplit);
        jt = F % wp.jtiles; F /= wp.jtiles;
        it = F % wp.itiles; split = F / wp.itiles;
    }
    const int j0 = jt * 64, i0 = it * 64;
    const int ihw = g.IH * g.IW;
    const int o_beg = split * wp.octs_per_split, o_end = min(wp.noct, o_beg + wp.octs_per_split);
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x, (size_t)g.B * g.Cin * ihw * sizeof(float));
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(dy, (size_t)g.B * g.Cout * ihw * sizeof(float));
    const int tw8 = g.OW >> 4, th = g.OH >> 1;                    // tile octets per row, tile rows per image

    // this thread's (tile, channel) pair of each operand: tile = tid & 7, channel = tid >> 3
    const int tj = tid & 7, tc = tid >> 3;
    float xr[16];
    float2 dr[2];
    // A foreign VALU instruction gets an issue slot about every 21 cycles beside the other wave's MFMAs: the address
    // arithmetic of the loads is kept to one add per row -- the thread's part of an offset (channel plane, tile column) is formed here
    // once, the octet's part (image, tile row, octet column; row validity) is scalar -- and the two inner columns of a patch row, always
    // inside the image and 8-byte aligned (IW and the plane size are even), come as one 8-byte load.
    const int xthr = (i0 + tc) * ihw + 2 * tj - 1, dthr = (j0 + tc) * ihw + 2 * tj;
    const bool cvx = i0 + tc < g.Cin, cvd = j0 + tc < g.Cout;
    const bool tj_first = tj == 0, tj_last = tj == 7;
    // loads of octet o in 3 pieces (x rows 0-1, x rows 2-3, the dy tile)
    auto load_piece = [&](int o, int lp) {
        const bool ov = o < o_end;
        const int txo = o % tw8, t1 = o / tw8;
        const int ty = t1 % th, b = t1 / th;
        if (lp < 2) {
            const int sx = b * g.Cin * ihw + 16 * txo;
            const bool c0ok = !(tj_first & (txo == 0)), c3ok = !(tj_last & (txo == tw8 - 1));      // patch columns -1 / IW of the edge tiles
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int i = 2 * lp + ii;
                const int iy = 2 * ty - 1 + i;
                const bool rv = cvx & (ov & ((unsigned)iy < (unsigned)g.IH));
                const unsigned ro = (unsigned)(xthr + (sx + iy * g.IW)) * 4u;
                xr[i * 4 + 0] = buf_load(rx, (rv & c0ok) ? ro : kOOB);
                const float2 mid = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rx, rv ? ro + 4u : kOOB, 0, 0));
                xr[i * 4 + 1] = mid.x;
                xr[i * 4 + 2] = mid.y;
                xr[i * 4 + 3] = buf_load(rx, (rv & c3ok) ? ro + 12u : kOOB);
            }
        } else {
            const bool dv = cvd & ov;
            const int sd = b * g.Cout * ihw + 2 * ty * g.OW + 16 * txo;
#pragma unroll
            for (int a = 0; a < 2; ++a)
                dr[a] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rd, dv ? (unsigned)(dthr + (sd + a * g.OW)) * 4u : kOOB, 0, 0));
        }
    };
    auto load_oct = [&](int o) {
#pragma unroll
        for (int lp = 0; lp < 3; ++lp) load_piece(o, lp);
    };
    // transform + LDS stores of the loaded octet in 4 pieces (V rows 0-1, V rows 2-3, Z rows 0-1, Z rows 2-3)
    float tt_[4][4];                                             // t = B^T d, kept between the two V pieces
    auto transform_piece = [&](float* buf, int sub) {            // buf: Z at 0, V at ZV
        if (sub == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d0 = xr[c], d1 = xr[4 + c], d2 = xr[8 + c], d3 = xr[12 + c];
                tt_[0][c] = d0 - d2; tt_[1][c] = d1 + d2; tt_[2][c] = d2 - d1; tt_[3][c] = d3 - d1;
            }
        }
        if (sub < 2) {                                           // V = (B^T d) B, rows 2 * sub, + 1
#pragma unroll
            for (int x2 = 0; x2 < 2; ++x2) {
                const int xi = 2 * sub + x2;
                const float* t = tt_[xi];
                float* o = buf + ZV + ((xi * 4) * 64 + tc) * 8 + tj;
                o[0] = t[0] - t[2]; o[64 * 8] = t[1] + t[2]; o[2 * 64 * 8] = t[2] - t[1]; o[3 * 64 * 8] = t[3] - t[1];
            }
        } else {                                                 // Z = G e G^T, rows 2 * (sub - 2), + 1
            const float e00 = dr[0].x, e01 = dr[0].y, e10 = dr[1].x, e11 = dr[1].y;
#pragma unroll
            for (int x2 = 0; x2 < 2; ++x2) {
                const int xi = 2 * (sub - 2) + x2;
                const float u0 = xi == 0 ? e00 : (xi == 1 ? 0.5f * (e00 + e10) : (xi == 2 ? 0.5f * (e00 - e10) : e10));
                const float u1 = xi == 0 ? e01 : (xi == 1 ? 0.5f * (e01 + e11) : (xi == 2 ? 0.5f * (e01 - e11) : e11));
                float* o = buf + ((xi * 4) * 64 + tc) * 8 + tj;
                o[0] = u0; o[64 * 8] = 0.5f * (u0 + u1); o[2 * 64 * 8] = 0.5f * (u0 - u1); o[3 * 64 * 8] = u1;
            }
        }
    };
    auto transform_store = [&](float* buf) {
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) transform_piece(buf, tp);
    };

    f32x16 acc[8];                                               // positions 8 * up + q
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    if (o_beg < o_end) {
        load_oct(o_beg);
        transform_store(L);
        load_oct(o_beg + 1);
        lds_barrier_w();
        const unsigned zl = (unsigned)(up * 8 * 64 * 8 + (fj * 32 + l31) * 8 + lh * 4), vl = (unsigned)(ZV + up * 8 * 64 * 8 + (fi * 32 + l31) * 8 + lh * 4);
        // one octet of a wave: 8 stages of [next stage's fragments][a piece of the other work][4 MFMAs].  The other work -- the next
        // octet's transform (its patches were loaded one octet ago) and the loads of the octet after that -- stands in the four stages
        // from S0 on; the other four are MFMAs and their fragment reads only.  S0 = 0 for the lower group and 4 for the upper one: while
        // one wave of a SIMD issues VALU / memory instructions between its MFMAs, the other one keeps the matrix pipe fed.
        auto octet = [&](auto s0, int o) {
            constexpr int S0 = decltype(s0)::value;
            const float* cur = L + ((o - o_beg) & 1) * (2 * ZV);
            float* nxt = L + (((o - o_beg) & 1) ^ 1) * (2 * ZV);
            u32x4 zf[2], vf[2];
            zf[0] = *reinterpret_cast<const u32x4*>(cur + zl);
            vf[0] = *reinterpret_cast<const u32x4*>(cur + vl);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (q + 1 < 8) {
                    zf[(q + 1) & 1] = *reinterpret_cast<const u32x4*>(cur + (q + 1) * 64 * 8 + zl);
                    vf[(q + 1) & 1] = *reinterpret_cast<const u32x4*>(cur + (q + 1) * 64 * 8 + vl);
                }
                // no branch around the pieces (after the last octet they transform zeros into the buffer nobody reads): one basic block per
                // stage, so that the pieces can be issued BETWEEN the four MFMAs of the stage (below).  xr is dead once piece 0 has formed
                // B^T d, dr after piece 3: the loads of octet o + 2 follow them (past the range: zero range, nothing is fetched)
                if (q >= S0 && q < S0 + 4) transform_piece(nxt, q - S0);
                if (q >= S0 + 1 && q < S0 + 4) load_piece(o + 2, q - S0 - 1);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(zf[q & 1][j]), __uint_as_float(vf[q & 1][j]), acc[q], 0, 0, 0);
                // a wave issues in order: whatever FOLLOWS four back-to-back MFMAs in program order waits for all of them to issue.  The
                // scalar / LDS / global-load instructions of the piece are spread over the four 64-cycle shadows instead; the VALU ones
                // cost this wave ~6 cycles each wherever they stand (profiles/micro/mfma_issue.hip) -- cycles in which the SIMD's other
                // wave, in its MFMA-only half, has the matrix pipe
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);          // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);          // DS read (the next stage's fragments)
                    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);          // VALU
                    __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);          // VMEM read
                    __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);          // DS write
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            lds_barrier_w();
        };
        if (up == 0) {
            for (int o = o_beg; o < o_end; ++o) octet(std::integral_constant<int, 0>{}, o);
        } else {
            for (int o = o_beg; o < o_end; ++o) octet(std::integral_constant<int, 4>{}, o);
        }
    }

    // ---- dw = A^T M A needs the 16 positions of a (cout, cin) pair in one lane.  The two waves of a fragment pair swap halves: wave w
    //      leaves the accumulator registers its partner finishes -- 8 positions x 8 registers, as 16 float4 per lane -- in its 16 KB of
    //      the (now dead) operand buffers: the lower group finishes registers 0-7, the upper group registers 8-15.  Once per workgroup. ----
    auto hand_over = [&](auto upc) {
        constexpr int R0 = decltype(upc)::value ? 0 : 8;         // the registers the partner finishes
        f32x4* const mine = reinterpret_cast<f32x4*>(L) + w * (16 * 64) + lane;
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int rq = 0; rq < 2; ++rq) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[q][R0 + 4 * rq + e];
                mine[(q * 2 + rq) * 64] = v;
            }
    };
    if (up == 0) hand_over(std::integral_constant<int, 0>{});
    else hand_over(std::integral_constant<int, 1>{});
    lds_barrier_w();

    // ---- D[cout][cin]: lane l31 = input channel, register -> output channel.  The slab is [tap][cout][cin]:
    //      a store instruction writes 128 contiguous bytes per half wave (OIHW would scatter its lanes 36 bytes apart: the 38 MB of slabs
    //      of a 128-way pixel split took 30 us that way); wino_wgrad_sum_kernel transposes while it sums.  Addresses: lane part in the
    //      vector offset once, (register, tap) part in the scalar offset. ----
    float* const o = part + (size_t)split * wp.slab;
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(o, (size_t)9 * g.Cout * g.Cin * sizeof(float));
    const int ci = i0 + fi * 32 + l31;
    const int cob = j0 + fj * 32;                                // + (r & 3) + 8 (r >> 2) + 4 lh
    const unsigned vo = ci < g.Cin ? (unsigned)(4 * lh * g.Cin + ci) * 4u : kOOB;
    const unsigned tapb = (unsigned)(g.Cout * g.Cin) * 4u;
    const f32x4* const theirs = reinterpret_cast<const f32x4*>(L) + (w ^ 4) * (16 * 64) + lane;
    auto finish = [&](auto upc) {
        constexpr int UP = decltype(upc)::value;
#pragma unroll
        for (int rq = 0; rq < 2; ++rq) {
            const int rg = 2 * UP + rq;                          // r >> 2 of the four registers of this round
            if (cob + 8 * rg >= g.Cout) continue;                // (a group of 8 channels is valid as a whole: Cout is a multiple of 8)
            f32x4 oth[8];                                        // the partner's positions 8 * (1 - UP) + q of registers 4 * rg ... + 3
#pragma unroll
            for (int q = 0; q < 8; ++q) oth[q] = theirs[(q * 2 + rq) * 64];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * rg + e;
                float c[3][4];                                   // rows of A^T M
#pragma unroll
                for (int nu = 0; nu < 4; ++nu) {
                    const float m0 = UP ? oth[nu][e] : acc[nu][r], m1 = UP ? oth[4 + nu][e] : acc[4 + nu][r];
                    const float m2 = UP ? acc[nu][r] : oth[nu][e], m3 = UP ? acc[4 + nu][r] : oth[4 + nu][e];
                    c[0][nu] = m0 + m1 + m2;
                    c[1][nu] = m1 - m2;
                    c[2][nu] = m1 + m2 + m3;
                }
                const unsigned so = (unsigned)((cob + e + 8 * rg) * g.Cin) * 4u;
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) {
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, c[rr][0] + c[rr][1] + c[rr][2]), ro, vo, so + (unsigned)(rr * 3 + 0) * tapb, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, c[rr][1] - c[rr][2]), ro, vo, so + (unsigned)(rr * 3 + 1) * tapb, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, c[rr][1] + c[rr][2] + c[rr][3]), ro, vo, so + (unsigned)(rr * 3 + 2) * tapb, 0);
                }
            }
        }
    };
    if (up == 0) finish(std::integral_constant<int, 0>{});
    else finish(std::integral_constant<int, 1>{});
}

// dw[cout][cin][tap] (+)= sum over the pixel-split slabs [tap][cout][cin].  As conv.hip's sum_slabs_kernel: a workgroup covers 32 float4
// elements (4 consecutive input channels of one (tap, cout)) x 8 slab groups, a thread adds every 8th slab with 4 loads in flight, the 8
// partial sums meet in LDS; the first group transposes on the way out.  Fixed summation order: reproducible.
__global__ __launch_bounds__(256) void wino_wgrad_sum_kernel(const float* __restrict__ part, int nslabs, size_t slab, int cout, int cin,
                                                             float* __restrict__ dw, int accumulate) {
    __shared__ f32x4 red[8][32];
    const int q4 = cin >> 2, n4 = 9 * cout * q4;
    const int el = threadIdx.x & 31, grp = threadIdx.x >> 5;
    for (int base = blockIdx.x * 32; base < n4; base += gridDim.x * 32) {
        const int e = base + el;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (e < n4) {
            const float* src = part + (size_t)e * 4;
            int sp = grp;
            for (; sp + 24 < nslabs; sp += 32) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + (size_t)sp * slab);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + (size_t)(sp + 8) * slab);
                const f32x4 v2 = *reinterpret_cast<const f32x4*>(src + (size_t)(sp + 16) * slab);
                const f32x4 v3 = *reinterpret_cast<const f32x4*>(src + (size_t)(sp + 24) * slab);
                a += (v0 + v1) + (v2 + v3);
            }
            for (; sp < nslabs; sp += 8) a += *reinterpret_cast<const f32x4*>(src + (size_t)sp * slab);
        }
        red[grp][el] = a;
        __syncthreads();
        if (grp == 0 && e < n4) {
#pragma unroll
            for (int k = 1; k < 8; ++k) a += red[k][el];
            const int c4 = e % q4, t1 = e / q4;
            const int co = t1 % cout, tap = t1 / cout;
            float* dst = dw + ((size_t)co * cin + 4 * c4) * 9 + tap;
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[k * 9] = accumulate ? dst[k * 9] + a[k] : a[k];
        }
        __syncthreads();
    }
}

int pow2floor_log(int v) {
    int l = 0;
    while ((2 << l) <= v) ++l;
    return l;
}

}  // namespace

namespace agan {
namespace conv {

// Plan of the Winograd gather for geometry g: the forward or data gradient of a conv3x3 stride 1 pad 1, the forward of a conv4x4 stride 2
// pad 1, or the data gradient of one (a 2x2-tap gather per parity class); p.ok == 0: not taken.
WinoPlan plan_wino(const Geom& g) {
    WinoPlan p;
    memset(&p, 0, sizeof(p));
    if (g.SY == 1 && g.R == 3 && g.S == 3 && g.DY == 1 && g.OS == 1 && g.OY0 == -1 && g.IH == g.OH && g.IW == g.OW)
        p.kind = (g.Cout & 7) == 0 ? WinoKind::conv3x3_half : WinoKind::conv3x3;     // half: 32 tiles x 64 channels, two workgroups per CU
    else if (g.SY == 2 && g.R == 4 && g.S == 4 && g.DY == 1 && g.OS == 1 && g.OY0 == -1 && g.IH == 2 * g.OH && g.IW == 2 * g.OW) p.kind = WinoKind::conv4x4_s2;
    else if (g.SY == 1 && g.R == 2 && g.S == 2 && g.DY == -1 && g.OS == 2 && g.OY0 == 0 && g.OY1 == 1 && g.OH == 2 * g.IH && g.OW == 2 * g.IW) p.kind = WinoKind::dgrad2x2_class;
    else return p;
    const WinoTraits T = wino_traits(p.kind);
    const bool k3x3 = p.kind == WinoKind::conv3x3 || p.kind == WinoKind::conv3x3_half;
    if ((g.OHs & 1) || (g.OWs & 1) || (g.Cin & (T.cch - 1)) || g.Cout < 32) return p;
    // the stride-2 forward kernel is built for 128-channel tiles.  So is the class kernel: with 64 output channels -- 64-tile blocks, short K
    // loops, 64 scalar stores per lane -- it measured 15 % SLOWER than the direct kernel, with 128+ 15 % faster
    if (!k3x3 && g.Cout < 96) return p;
    const int tw = g.OWs / 2, th = g.OHs / 2;                 // tiles per row / column of the output lattice
    if (tw < 4) return p;                                     // (4x4 maps: two tiles per row -- the direct kernel's K split serves them better)
    p.nf = (g.Cout >= 96 || p.kind == WinoKind::conv3x3_half) ? 4 : 2;      // tile geometry: 4: 32-tile blocks, 2: 64-tile blocks (of 64 output channels)
    const int lt = p.nf == 4 ? 5 : 6;
    p.txl = std::min(3, pow2floor_log(tw));
    p.tyl = std::min(lt - p.txl, pow2floor_log(th));
    const int TX = 1 << p.txl, TY = 1 << p.tyl, TB = (1 << lt) >> (p.txl + p.tyl);
    p.blocks_x = cdiv(tw, TX);
    p.blocks_y = cdiv(th, TY);
    p.blocks_b = cdiv(g.B, TB);
    p.mtiles = p.blocks_x * p.blocks_y * p.blocks_b;
    p.ntiles = p.kind == WinoKind::conv3x3_half ? cdiv(g.Cout, 64) : cdiv(g.Cout, p.nf * 32);
    // the 32 x 32 x 2 product needs thousands of tiles to pay for a workgroup's 256 accumulators: small layers stay on the direct kernel
    // (stride 2, measured: 384 workgroups = 1.5 rounds of the chip gain nothing, 768+ do: such layers split their input channels over two
    //  workgroups and sum the halves -- their outputs are small)
    p.ksplit = 1;
    if (p.kind == WinoKind::conv4x4_s2 && p.mtiles * p.ntiles < 512 && p.mtiles * p.ntiles >= 256 && g.Cin >= 128) p.ksplit = 2;
    if (p.mtiles * p.ntiles * p.ksplit * T.classes < (k3x3 ? 256 : 512)) return p;
    p.chunks_per_split = cdiv(g.Cin / 8, p.ksplit);
    p.slab = ((size_t)g.B * g.Cout * g.OH * g.OW + 3) / 4 * 4;
    const int PR = T.step * TY + T.extra, PC = T.step * TX + T.extra;
    p.pcp = (PC + 1) & ~1;
    p.mpc = (65536 + PC - 1) / PC;
    p.mpr = (65536 + PR - 1) / PR;
    p.raw_items = TB * T.cch * PR * PC;
    if (p.raw_items > (lt == 5 ? T.ni32 : T.ni64) * T.threads) return p;      // (the kernel's staging registers: WinoGather::NI)
    p.raw_bytes = (TB * T.cch * PR * p.pcp * 4 + 15) & ~15;
    p.smem_bytes = 2 * p.raw_bytes + 2 * T.vfrags * (1 << lt) * 8 * 4;      // two raw patches, two V buffers
    if (T.threads == 512) p.smem_bytes = std::max(p.smem_bytes, 8 * 10 * 64 * 16);     // the wave pairs' exchange of accumulator halves (WinoGather::epilogue_pair)
    if (p.smem_bytes > T.lds_cap) return p;
    p.u_bytes = ((size_t)T.planes * (g.Cin / 8) * g.Nld * 8 * sizeof(float) + 255) / 256 * 256;
    p.ws_bytes = p.u_bytes + (p.ksplit > 1 ? p.slab * p.ksplit * sizeof(float) : 0);
    p.ok = 1;
    return p;
}

namespace {
template <auto Kernel, WinoKind K>
void launch_gather_kernel(dim3 grid, const float* in, const float* U, float* out, const Geom& g, const WinoPlan& p, hipStream_t st) {
    allow_dynamic_lds<Kernel>(wino_traits(K).lds_cap);
    AGAN_LAUNCH(Kernel, grid, dim3(wino_traits(K).threads), (size_t)p.smem_bytes, st, in, U, out, g, p);
}
}  // namespace

// wk: the mode's ordinary fp32 pack [K = (c, r, s)][Nld]; ws: >= p.u_bytes
void launch_wino(const float* in, const float* wk, float* out, const Geom& g, const WinoPlan& p, void* ws, hipStream_t st) {
    float* U = static_cast<float*>(ws);
    const int total = g.Cin * g.Nld;
    const dim3 grid(p.mtiles * p.ntiles * p.ksplit * wino_traits(p.kind).classes), tgrid(std::min(cdiv(total, 256), 2048));
    switch (p.kind) {
    case WinoKind::dgrad2x2_class:
        AGAN_LAUNCH(wino_cls_weight_transform_kernel, dim3(std::min(cdiv(4 * total, 256), 4096)), dim3(256), 0, st, wk, U, g.Cin, g.Nld, g.Cout);
        launch_gather_kernel<conv_wino_cls_f32_kernel<4>, WinoKind::dgrad2x2_class>(grid, in, U, out, g, p, st);
        break;
    case WinoKind::conv4x4_s2:
        AGAN_LAUNCH(wino_s2_weight_transform_kernel, tgrid, dim3(256), 0, st, wk, U, g.Cin, g.Nld, g.Cout);
        // (a split launch writes its partial sums to the slabs behind U in the workspace: the caller sums them into `out`)
        launch_gather_kernel<conv_wino_s2_f32_kernel<4>, WinoKind::conv4x4_s2>(
            grid, in, U, p.ksplit > 1 ? reinterpret_cast<float*>(static_cast<char*>(ws) + p.u_bytes) : out, g, p, st);
        break;
    case WinoKind::conv3x3_half:
        AGAN_LAUNCH(wino_weight_transform_kernel, tgrid, dim3(256), 0, st, wk, U, g.Cin, g.Nld, g.Cout);
        launch_gather_kernel<conv_wino_h_f32_kernel, WinoKind::conv3x3_half>(grid, in, U, out, g, p, st);
        break;
    case WinoKind::conv3x3:
        AGAN_LAUNCH(wino_weight_transform_kernel, tgrid, dim3(256), 0, st, wk, U, g.Cin, g.Nld, g.Cout);
        if (p.nf == 4) launch_gather_kernel<conv_wino_f32_kernel<4>, WinoKind::conv3x3>(grid, in, U, out, g, p, st);
        else launch_gather_kernel<conv_wino_f32_kernel<2>, WinoKind::conv3x3>(grid, in, U, out, g, p, st);
        break;
    }
}

// Winograd weight gradient of a conv3x3 stride 1 pad 1 (forward geometry g); p.ok == 0: not taken.
WinoWgradPlan plan_wino_wgrad(const Geom& g) {
    WinoWgradPlan p;
    memset(&p, 0, sizeof(p));
    if (!(g.SY == 1 && g.R == 3 && g.S == 3 && g.DY == 1 && g.OS == 1 && g.OY0 == -1)) return p;
    if (g.IH != g.OH || g.IW != g.OW || (g.OH & 1) || (g.OW & 15) || g.Cin < 32 || g.Cout < 32 || (g.Cin & 3) || (g.Cout & 7)) return p;
    p.noct = g.B * (g.OH / 2) * (g.OW / 16);
    p.jtiles = cdiv(g.Cout, 64);
    p.itiles = cdiv(g.Cin, 64);
    const int wgs = p.jtiles * p.itiles;
    if (p.noct < 64 * 16 || wgs > 256) return p;               // enough pixels to split over the chip with long loops; (many-channel layers have few pixels here)
    const int ps = std::max(1, std::min(256 / wgs, p.noct / 16));
    p.octs_per_split = cdiv(p.noct, ps);
    p.psplit = cdiv(p.noct, p.octs_per_split);
    p.slab = ((size_t)g.Cout * g.Cin * 9 + 3) / 4 * 4;
    p.ws_bytes = p.slab * p.psplit * sizeof(float);
    p.smem_bytes = 2 * 2 * 16 * 64 * 8 * 4;
    p.ok = 1;
    return p;
}

void launch_wino_wgrad(const float* x, const float* dy, float* part, const Geom& g, const WinoWgradPlan& p, hipStream_t st) {
    allow_dynamic_lds<conv_wino_wgrad_f32_kernel>(160 * 1024);
    AGAN_LAUNCH(conv_wino_wgrad_f32_kernel, dim3(p.jtiles * p.itiles * p.psplit), dim3(512), (size_t)p.smem_bytes, st, x, dy, part, g, p);
}

void launch_wino_wgrad_sum(const float* part, const Geom& g, const WinoWgradPlan& p, float* dw, int accumulate, hipStream_t st) {
    const int n4 = 9 * g.Cout * (g.Cin >> 2);
    AGAN_LAUNCH(wino_wgrad_sum_kernel, dim3(std::min(cdiv(n4, 32), 8192)), dim3(256), 0, st, part, p.psplit, p.slab, g.Cout, g.Cin, dw, accumulate);
}

}  // namespace conv
}  // namespace agan
