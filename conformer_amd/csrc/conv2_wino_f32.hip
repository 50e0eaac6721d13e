// Stem conv2 (3x3, stride 2, fp32 inference) as polyphase Winograd F(2x2, 2x2) pattern GEMMs.
//
// A 2x2 block of conv2 outputs (t2 = 2i + r, f2 = 2j + s) reads the 5x5 h1 patch d[0..4] x d[0..4] at (4i, 4j).  Per
// dimension the even taps (w0, w2 on d0, d2, d4) are a 2-output 2-tap correlation, computed by F(2,2):
//   m0 = (d0 - d2) w0,  m1 = d2 (w0 + w2),  m2 = (d4 - d2) w2,   y0 = m0 + m1,  y1 = m1 + m2,
// and the odd tap (w1 on d1, d3) contributes d1 w1 to y0 only and d3 w1 to y1 only -- the output patterns of m0 and m2.  So
// every product lands in one of three patterns per dimension (0: y0 only, 1: both, 2: y1 only), 9 in 2-D, and pattern
// (a, b) is one plain GEMM whose K walks its terms: a dimension in pattern 0 or 2 has two terms ("side" sg = 0 / 1):
//   term 0: h1 pixels d[4 sg] - d[2], tap w[2 sg];   term 1: pixel d[1 + 2 sg], tap w1;
// in pattern 1 one term: pixel d[2], tap w0 + w2.  2-D terms are the products (ut, uf): 4 corners x 4 terms + 4 edges x 2 + 1
// centre = 25 channel contractions per output block against 36 for the direct implicit GEMM.  The pattern GEMMs write planes
// P_ab (M x C, M = B * ceil(T2/2) * ceil(F2/2) blocks); the combine kernel forms y[r][s] = sum_{a in S(r), b in S(s)} P_ab,
// S(0) = {0, 1}, S(1) = {1, 2}, adds the bias and applies the ReLU.
//
// The GEMM is the 8-wave 256x256 tile of conv2_f32_wide_kernel (gemm_f32.hip): same MFMA, fragment order, padded LDS rows,
// channel-chunk-major K walk (the terms of a 32-channel chunk reuse the same h1 lines) and row-major epilogue.  The staging
// differs: an A element is a +-1 combination of 1, 2 or 4 h1 pixels, so the raw pixels of a K-tile take up to 4x the staging
// registers; the tile is staged ONE K-tile ahead in one register set (the direct kernel: two ahead in two sets).  A K-tile
// of 64 MFMAs per wave at two waves per SIMD covers about 8000 cycles of load latency (two ahead for the centre and edge
// problems, which have the registers for it, measured no faster).  The whole 32-channel chunk is unrolled, so every K-tile's
// term -- its pixel count and signs -- is a compile-time constant and no load sits behind a branch.  A load's offset is one
// per-row register plus a wave-uniform part (pixel, channel chunk, K position) that rides in the instruction's scalar offset:
// added per lane instead, the sums took address registers that pushed the corner loop to 256 VGPRs and into spills, whose
// reloads queue behind the K-tile's loads (4.27 -> 3.94 ms at B = 32; DESIGN.md section 5, "Tuning pass").
#include <algorithm>
#include <utility>

#include "gemm_shared.h"

namespace {

#define WINO_MFMA_SLICE(FA, FB)                                                                             \
    _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                           \
    _Pragma("unroll") for (int mt = 0; mt < TM; ++mt)                                                       \
    _Pragma("unroll") for (int nt = 0; nt < TN; ++nt)                                                       \
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(FB[nt][e], FA[mt][e], acc[mt][nt], 0, 0, 0)

template <typename Fn, int... I>
__device__ __forceinline__ void static_for_seq(Fn& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename Fn>
__device__ __forceinline__ void static_for(Fn&& f) {   // f(integral_constant<int, 0>), ..., f(integral_constant<int, N - 1>)
    static_for_seq(f, std::make_integer_sequence<int, N>{});
}

// pattern p = 3 a + b (a: time, b: frequency); terms per dimension and the K offset of each pattern's block in the pack
__host__ __device__ constexpr int wino_nt(int a) { return a == 1 ? 1 : 2; }
__host__ __device__ constexpr int wino_terms(int p) { return wino_nt(p / 3) * wino_nt(p % 3); }

// Dead rows.  With F2 odd the s = 1 output of the last frequency block (jb = TJ - 1) does not exist, and the b = 2 patterns
// feed nothing else; likewise a = 2 at ib = TI - 1 with T2 odd.  Those patterns run over TJ - 1 (TI - 1) blocks: pattern p's
// rows are the blocks (bb, ib, jb) of its own TI_p x TJ_p grid, stored densely at the head of its plane (the plane stride
// stays M), and the combine kernel reads a short plane only at the blocks it holds.
struct WinoArgs {
    const float* h1; const float* w; float* planes;
    int64_t M;                      // output blocks nb * TI * TJ (plane stride in rows)
    unsigned h1_bytes;
    int T1, F1, C, TI, TJ, nb;
    int odd_t, odd_f;               // T2 / F2 odd: the a = 2 / b = 2 patterns have one block less in that dimension
    unsigned tiles_n;
    unsigned grp_blk[4];            // workgroup ranges of the corner / edge / centre groups (starts are multiples of 8)
    unsigned grp_tm[3][4];          // per group: row tiles of its patterns, ascending (the centre: 0, 0, 0, tiles)
    unsigned grp_pat[3];            // per group: the patterns in that order, one nibble each
};

// Launch order: the four corner patterns (K = 4C), then the four edges (2C), then the centre (C) -- the long problems first so
// the last round holds short tiles.  Within a group, the tile list (tm, pattern, tn) is cut into 8 contiguous ranges, one per
// XCD (workgroup w runs on XCD w % 8), so the 2 x 4 tiles of one row block (they read the same h1 lines) share an L2.  A
// pattern with fewer row tiles than the others of its group simply drops out of the list from its last tile on.

template <int ST, int SF>
__device__ __forceinline__ void wino_tile(const WinoArgs& g, int p, int64_t m0, int n0, float* lds) {
    constexpr int BM = 256, BN = 256, WN = 4, TM = 4, TN = 2, BK = 16, LDSR = BK + 4, NT = ST * SF, SPC = 2 * NT;
    constexpr int NPX = (ST == 2 ? 2 : 1) * (SF == 2 ? 2 : 1);   // most pixels of one term
    float* As = lds;
    float* Bs = lds + 2 * BM * LDSR;
    const int a = p / 3, b = p - 3 * (p / 3);
    const int sg_t = a >> 1, sg_f = b >> 1;                       // side of a two-term dimension (pattern 0 or 2)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WN, wc = wave % WN;
    const int li = lane & 31, hf = lane >> 5;

    constexpr int CPR = BK / 4, RPP = 512 / CPR, PA = BM / RPP, PB = BN / RPP;
    const int chunk = tid & (CPR - 1), srow = tid / CPR;
    // per staged row: byte offset of its 5x5 patch in h1 (h1 < 4 GiB: the entry point splits the batch).  The pixels of a term
    // are the uniform offsets of the distinct d used per dimension (index 0: d[4 sg], or d[2] in a one-term dimension; 1: d[2];
    // 2: d[1 + 2 sg]).  No pixel of a VALID output lies outside T1 x F1 (t2 < T2 gives 4 i + 4 <= T1 - 1), and the blocks
    // whose pattern-2 terms would reach beyond the edge are not among a pattern-2 problem's rows: every load is inside h1 and
    // needs no select.  (It has to be: the scalar offset is not part of the buffer's range check.)
    unsigned row_off[PA];
    const int TJp = g.TJ - (b == 2 ? g.odd_f : 0);                  // this pattern's block grid (see WinoArgs)
    const int64_t pos_per_b = (int64_t)(g.TI - (a == 2 ? g.odd_t : 0)) * TJp, Mp = g.nb * pos_per_b;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        int64_t m = m0 + srow + RPP * i;
        if (m >= Mp) m = Mp - 1;                                    // loaded, never stored
        const int64_t bb = m / pos_per_b;
        const int r = (int)(m - bb * pos_per_b);
        const int ib = r / TJp, jb = r - ib * TJp;
        row_off[i] = (unsigned)((((bb * g.T1 + 4 * ib) * g.F1 + 4 * jb) * (int64_t)g.C + chunk * 4) * 4);
    }
    const __amdgpu_buffer_rsrc_t h1_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.h1), (short)0, (int)g.h1_bytes, 0x00020000);
    const unsigned pix_t[3] = {(unsigned)((ST == 2 ? 4 * sg_t : 2) * g.F1 * g.C * 4), (unsigned)(2 * g.F1 * g.C * 4),
                               (unsigned)((1 + 2 * sg_t) * g.F1 * g.C * 4)};
    const unsigned pix_f[3] = {(unsigned)((SF == 2 ? 4 * sg_f : 2) * g.C * 4), (unsigned)(2 * g.C * 4), (unsigned)((1 + 2 * sg_f) * g.C * 4)};
    int64_t woff = 0;
    for (int q = 0; q < p; ++q) woff += wino_terms(q);
    const int K = NT * g.C;
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.w + woff * g.C * g.C), (short)0,
                                                                            K * g.C * 4, 0x00020000);
    const unsigned w_off = (unsigned)(((n0 + srow) * K + chunk * 4) * 4), w_step = (unsigned)(RPP * K * 4);

    // term u = ut * SF + uf is the product of a time and a frequency term: a two-pixel dimension term is d-index 0 minus
    // d-index 1, a one-pixel term d-index 2 (two-term dimension) or 0 (one-term dimension); raw[i][x * NYF + y]
    f32x4 raw[PA][NPX], rb[PB];
    auto load_tile = [&](auto U_, int c32, int half) __attribute__((always_inline)) {
        constexpr int U = decltype(U_)::value, UT = U / SF, UF = U % SF;
        constexpr int NXT = (ST == 2 && UT == 0) ? 2 : 1, NYF = (SF == 2 && UF == 0) ? 2 : 1;
        constexpr int X1 = ST == 2 ? (UT == 0 ? 0 : 2) : 0, Y1 = SF == 2 ? (UF == 0 ? 0 : 2) : 0;
        const unsigned ci4 = (unsigned)(32 * c32 + 16 * half) * 4;
#pragma unroll
        for (int x = 0; x < NXT; ++x)
#pragma unroll
            for (int y = 0; y < NYF; ++y) {
                const unsigned po = pix_t[X1 + x] + pix_f[Y1 + y] + ci4;
#pragma unroll
                for (int i = 0; i < PA; ++i)
                    raw[i][x * NYF + y] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(h1_rsrc, row_off[i], po, 0));
            }
        const unsigned k4 = (unsigned)(NT * 32 * c32 + 32 * U + 16 * half) * 4;
#pragma unroll
        for (int i = 0; i < PB; ++i) rb[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_off, k4 + w_step * i, 0));
    };
    auto store_tile = [&](auto U_, int buf) __attribute__((always_inline)) {
        constexpr int U = decltype(U_)::value, UT = U / SF, UF = U % SF;
        constexpr int NXT = (ST == 2 && UT == 0) ? 2 : 1, NYF = (SF == 2 && UF == 0) ? 2 : 1;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const f32x4* px = raw[i];
            f32x4 v;
            if constexpr (NXT == 2 && NYF == 2) v = (px[0] - px[1]) - (px[2] - px[3]);
            else if constexpr (NXT * NYF == 2) v = px[0] - px[1];
            else v = px[0];
            *reinterpret_cast<f32x4*>(As + (buf * BM + srow + RPP * i) * LDSR + chunk * 4) = v;
        }
#pragma unroll
        for (int i = 0; i < PB; ++i)
            *reinterpret_cast<f32x4*>(Bs + (buf * BN + srow + RPP * i) * LDSR + chunk * 4) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int a_row = wr * (BM / 2) + li, b_row = wc * (BN / WN) + li;
    f32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
    auto read_frags = [&](f32x4 (&fa)[TM], f32x4 (&fb)[TN], int buf, int c) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < TM; ++t)
            fa[t] = *reinterpret_cast<const f32x4*>(As + (buf * BM + a_row + 32 * t) * LDSR + 8 * c + 4 * hf);
#pragma unroll
        for (int t = 0; t < TN; ++t)
            fb[t] = *reinterpret_cast<const f32x4*>(Bs + (buf * BN + b_row + 32 * t) * LDSR + 8 * c + 4 * hf);
    };

    // K-tile kt = SPC * c32 + 2 u + half; the registers hold K-tile kt + 1 when step kt begins
    const int nch = g.C / 32;
    load_tile(std::integral_constant<int, 0>{}, 0, 0);
    store_tile(std::integral_constant<int, 0>{}, 0);
    load_tile(std::integral_constant<int, 0>{}, 0, 1);
    __syncthreads();
    read_frags(fa0, fb0, 0, 0);
    for (int c32 = 0; c32 < nch; ++c32) {
        static_for<SPC>([&](auto S_) __attribute__((always_inline)) {
            constexpr int S = decltype(S_)::value;
            constexpr int S1 = (S + 1) % SPC, S2 = (S + 2) % SPC;
            const int cur = S & 1;                                   // (SPC is even: kt & 1 == S & 1)
            const bool more = S + 1 < SPC || c32 + 1 < nch;
            read_frags(fa1, fb1, cur, 1);
            __builtin_amdgcn_sched_barrier(0);
            WINO_MFMA_SLICE(fa0, fb0);
            __builtin_amdgcn_sched_barrier(0);
            if (more) store_tile(std::integral_constant<int, S1 / 2>{}, cur ^ 1);
            load_tile(std::integral_constant<int, S2 / 2>{}, S + 2 < SPC ? c32 : min(c32 + 1, nch - 1), S2 & 1);
            __syncthreads();
            if (more) read_frags(fa0, fb0, cur ^ 1, 0);
            __builtin_amdgcn_sched_barrier(0);
            WINO_MFMA_SLICE(fa1, fb1);
            __builtin_amdgcn_sched_barrier(0);
        });
    }

    __syncthreads();
    GemmArgs ge{};
    ge.C = g.planes + (int64_t)p * g.M * g.C;
    ge.M = Mp; ge.N = g.C; ge.K = K; ge.ldc = g.C; ge.alpha = 1.f;
    gemm_epilogue_rows<BM, BN, EPI_BIAS, TM, TN, 2, false, EPF_INFER | EPF_NO_BIAS, WN>(ge, acc, m0, n0, wr, wc, lane,
                                                                                        lds + wave * 32 * (32 * TN + 4));
}

__global__ __launch_bounds__(512, 2) void conv2_wino_gemm_kernel(const WinoArgs g) {
    constexpr int LDS_STAGE = 2 * (256 + 256) * 20;
    static_assert(8 * 32 * (32 * 2 + 4) <= LDS_STAGE, "the row-major epilogue scratch must fit the staging buffers");
    __shared__ __attribute__((aligned(16))) float lds[LDS_STAGE];
    const unsigned bid = blockIdx.x;
    const int grp = bid < g.grp_blk[1] ? 0 : (bid < g.grp_blk[2] ? 1 : 2);
    const unsigned local = bid - g.grp_blk[grp], per_xcd = (g.grp_blk[grp + 1] - g.grp_blk[grp]) / 8;
    unsigned tile = (local & 7u) * per_xcd + (local >> 3);
    // row tiles [grp_tm[k - 1], grp_tm[k]) are run by the patterns k .. 3 of the sorted list
    unsigned k = 0, lo = 0;
    for (; k < 4; ++k) {
        const unsigned seg = (g.grp_tm[grp][k] - lo) * (4 - k) * g.tiles_n;
        if (tile < seg) break;
        tile -= seg;
        lo = g.grp_tm[grp][k];
    }
    if (k == 4) return;                                              // (padding of the group to a multiple of 8)
    const unsigned tn = tile % g.tiles_n, rest = tile / g.tiles_n;
    const unsigned pi = k + rest % (4 - k), tm = lo + rest / (4 - k);
    const int p = (int)((g.grp_pat[grp] >> (4 * pi)) & 15u);
    const int64_t m0 = (int64_t)tm * 256;
    const int n0 = (int)tn * 256;
    const int nta = wino_nt(p / 3), ntb = wino_nt(p % 3);
    if (nta == 2 && ntb == 2) wino_tile<2, 2>(g, p, m0, n0, lds);
    else if (nta == 2) wino_tile<2, 1>(g, p, m0, n0, lds);
    else if (ntb == 2) wino_tile<1, 2>(g, p, m0, n0, lds);
    else wino_tile<1, 1>(g, p, m0, n0, lds);
}

// h2[b][t2][f2][c] = relu(b2[c] + sum of the four planes of (t2 & 1, f2 & 1)), one thread per (block, 4 channels): the nine
// plane values are read once and the block's (up to) four valid outputs written.  Fixed summation order:
// ((P_a0 + P_a1) for a = r, then r + 1 ...) -- see the body.  A short plane (a = 2 with T2 odd, b = 2 with F2 odd) has no row
// for a block of the last time / frequency column; it is not read there, and feeds no output that exists.
__global__ __launch_bounds__(256) void conv2_wino_combine_kernel(const float* __restrict__ planes, const float* __restrict__ b2,
                                                                 float* __restrict__ h2, int64_t M, int T2, int F2, int TI,
                                                                 int TJ, int C) {
    const int c4n = C / 4;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * c4n) return;
    const int64_t m = idx / c4n;
    const int c = (int)(idx - m * c4n) * 4;
    const int64_t per_b = (int64_t)TI * TJ;
    const int64_t bb = m / per_b;
    const int r = (int)(m - bb * per_b);
    const int ib = r / TJ, jb = r - ib * TJ;
    const int64_t plane = M * (int64_t)C;
    const int TIs = TI - (T2 & 1), TJs = TJ - (F2 & 1);
    f32x4 P[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const bool st = q / 3 == 2, sf = q % 3 == 2;                  // pattern q's rows: its own (TI or TIs) x (TJ or TJs) grid
        const int64_t mq = (bb * (st ? TIs : TI) + ib) * (sf ? TJs : TJ) + jb;
        P[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if ((!st || ib < TIs) && (!sf || jb < TJs))
            P[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(planes + q * plane + mq * C + c));
    }
    const f32x4 bias = *reinterpret_cast<const f32x4*>(b2 + c);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int t2 = 2 * ib + rt;
        if (t2 >= T2) continue;
        // column sums over the frequency patterns of each output column s: (P[a][s] + P[a][s + 1]), then the two time patterns
        const f32x4 u0 = P[3 * rt + 0] + P[3 * rt + 1], u1 = P[3 * rt + 1] + P[3 * rt + 2];
        const f32x4 v0 = P[3 * rt + 3] + P[3 * rt + 4], v1 = P[3 * rt + 4] + P[3 * rt + 5];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int f2 = 2 * jb + s;
            if (f2 >= F2) continue;
            const f32x4 y = (s == 0 ? u0 + v0 : u1 + v1) + bias;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaxf(y[e], 0.f);
            *reinterpret_cast<f32x4*>(h2 + (((bb * T2 + t2) * F2) + f2) * (int64_t)C + c) = o;
        }
    }
}

// w2 (Co, Ci, 3(kf), 3(kt)) -> the 25 transformed matrices in the GEMM's walk order: pattern p's block is (Co, NT_p C) with
// row co, column NT_p * 32 * (ci / 32) + 32 u + ci % 32 = sum of w2[co][ci][kf][kt] over the term's taps (summed in double,
// rounded once).
__global__ __launch_bounds__(256) void pack_conv2_wino_kernel(const float* __restrict__ w2, float* __restrict__ wp, int C) {
    const int p = blockIdx.y, nt = wino_terms(p);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t K = (int64_t)nt * C;
    if (idx >= K * C) return;
    const int64_t co = idx / K;
    const int k = (int)(idx - co * K);
    const int c32 = k / (32 * nt), rem = k - c32 * 32 * nt, u = rem / 32, ci = 32 * c32 + (rem & 31);
    int64_t off = 0;
    for (int q = 0; q < p; ++q) off += wino_terms(q);
    const int a = p / 3, b = p % 3, sfn = wino_nt(b);
    const int ut = u / sfn, uf = u % sfn;
    // taps of a dimension term: two-term dimension, side sg = a >> 1: term 0 -> {2 sg}, term 1 -> {1}; one-term -> {0, 2}
    auto taps = [](int pat, int term, int (&tp)[2]) {
        if (pat == 1) { tp[0] = 0; tp[1] = 2; return 2; }
        tp[0] = term == 0 ? 2 * (pat >> 1) : 1;
        return 1;
    };
    int tt[2], tf[2];
    const int ntt = taps(a, ut, tt), ntf = taps(b, uf, tf);
    double s = 0.0;
    const float* wc = w2 + (co * C + ci) * 9;
    for (int x = 0; x < ntt; ++x)
        for (int y = 0; y < ntf; ++y) s += (double)wc[tf[y] * 3 + tt[x]];
    wp[off * C * C + idx] = (float)s;
}

}  // namespace

extern "C" int64_t cfm_conv2_wino_plane_elems(int B, int F1, int T1, int C) {
    if (B <= 0 || F1 < 3 || T1 < 3 || C <= 0) return 0;
    const int64_t TI = ((T1 - 1) / 2 + 1) / 2, TJ = ((F1 - 1) / 2 + 1) / 2;
    return 9 * (int64_t)B * TI * TJ * C;
}

extern "C" int cfm_pack_conv2_wino_weight_f32(const float* w2, float* wp, int C, cfm_stream_t stream) {
    CFM_REQUIRE(w2 && wp, CFM_ERR_NULL);
    CFM_REQUIRE(C > 0 && C % 32 == 0, CFM_ERR_BAD_SHAPE);
    const int64_t most = 4 * (int64_t)C * C;
    hipLaunchKernelGGL(pack_conv2_wino_kernel, dim3((unsigned)((most + 255) / 256), 9), dim3(256), 0,
                       static_cast<hipStream_t>(stream), w2, wp, C);
    return cfm_launch_status();
}

// planes: cfm_conv2_wino_plane_elems(B, F1, T1, C) floats of scratch.  The batch runs in groups of utterances whose h1 spans
// less than 4 GiB (32-bit buffer offsets); every group is one pattern-GEMM launch and one combine launch over its own 9 planes.
extern "C" int cfm_subsample_conv2_wino_relu_f32(const float* h1, const float* wp, const float* b2, float* planes, float* h2,
                                                 int B, int F1, int T1, int C, cfm_stream_t stream) {
    CFM_REQUIRE(h1 && wp && b2 && planes && h2, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && F1 >= 3 && T1 >= 3, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(C > 0 && C % 256 == 0, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(CFM_ALIGNED16(h1) && CFM_ALIGNED16(wp) && CFM_ALIGNED16(b2) && CFM_ALIGNED16(planes) && CFM_ALIGNED16(h2),
                CFM_ERR_ALIGN);
    const int64_t utt_bytes = (int64_t)T1 * F1 * C * 4, limit = (1LL << 32) - (1LL << 26);
    CFM_REQUIRE(utt_bytes <= limit && 5LL * F1 * C * 4 < (1LL << 26), CFM_ERR_UNSUPPORTED);
    const int T2 = (T1 - 1) / 2, F2 = (F1 - 1) / 2;
    WinoArgs g{};
    g.w = wp;
    g.T1 = T1; g.F1 = F1; g.C = C; g.TI = (T2 + 1) / 2; g.TJ = (F2 + 1) / 2;
    g.odd_t = T2 & 1; g.odd_f = F2 & 1;
    g.tiles_n = (unsigned)(C / 256);
    const int64_t per_b = (int64_t)g.TI * g.TJ;
    const int group = (int)std::min<int64_t>(B, limit / utt_bytes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int b0 = 0; b0 < B; b0 += group) {
        const int nb = std::min(group, B - b0);
        g.h1 = h1 + b0 * (utt_bytes / 4);
        g.h1_bytes = (unsigned)(nb * utt_bytes);
        g.M = nb * per_b;
        g.nb = nb;
        g.planes = planes + 9 * (b0 * per_b) * C;
        // per group: its patterns sorted by row tiles, ascending and stable (conv2_wino_gemm_kernel walks them from the back)
        static const int group_pat[3][4] = {{0, 2, 6, 8}, {1, 7, 3, 5}, {-1, -1, -1, 4}};
        g.grp_blk[0] = 0;
        for (int q = 0; q < 3; ++q) {
            int pat[4];
            unsigned tm[4], total = 0;
            for (int i = 0; i < 4; ++i) {
                const int p = group_pat[q][i];
                const int64_t Mp = p < 0 ? 0 : (int64_t)nb * (g.TI - (p / 3 == 2 ? g.odd_t : 0)) * (g.TJ - (p % 3 == 2 ? g.odd_f : 0));
                const unsigned t = (unsigned)((Mp + 255) / 256);
                int j = i;
                for (; j > 0 && tm[j - 1] > t; --j) { tm[j] = tm[j - 1]; pat[j] = pat[j - 1]; }
                tm[j] = t; pat[j] = p < 0 ? 0 : p;
                total += t;
            }
            g.grp_pat[q] = 0;
            for (int i = 0; i < 4; ++i) { g.grp_tm[q][i] = tm[i]; g.grp_pat[q] |= (unsigned)pat[i] << (4 * i); }
            g.grp_blk[q + 1] = g.grp_blk[q] + (total * g.tiles_n + 7) / 8 * 8;
        }
        hipLaunchKernelGGL(conv2_wino_gemm_kernel, dim3(g.grp_blk[3]), dim3(512), 0, s, g);
        int st = cfm_launch_status();
        if (st) return st;
        const int64_t threads = g.M * (C / 4);
        hipLaunchKernelGGL(conv2_wino_combine_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, g.planes, b2,
                           h2 + (int64_t)b0 * T2 * F2 * C, g.M, T2, F2, g.TI, g.TJ, C);
        st = cfm_launch_status();
        if (st) return st;
    }
    return 0;
}
