// Middle of ConvolutionModule in ONE kernel (fp32 inference, LayerNorm folded):
//     c = Swish(BN_eval(depthwise_K(GLU(LN(x).W1^T + b1))))                     convolution.py:22-28
// The depthwise convolution is local in time per utterance.  A GEMM tile of 256 rows x 64 GLU channels that is one stretch
// of ONE utterance holds everything the depthwise conv of those 64 channels needs, so the conv runs in the GEMM's epilogue
// out of LDS: the (B, T, C) GLU tensor is neither written nor re-read (the depthwise kernel reads it ~2.9 x), and a launch
// leaves the block.
//
// Work unit: 512 threads = 8 waves (4 x 2) on 256 GEMM rows x 128 GEMM columns -- the 64 value columns of a channel group
// and their 64 gate columns; a wave owns 64 x 64 = 2 x 2 MFMA tiles, n-tile 0 = values, n-tile 1 = the gates of the same 32
// channels (the EPI_GLU convention of gemm_shared.h).  K loop: that of conv2_f32_wide_kernel (gemm_f32.hip): K-tile 16, padded
// LDS rows, two-ahead register staging, unconditional clamped refills, one 16-byte LDS read feeding four MFMA steps, one
// accumulation chain per output tile with k ascending -- the chain of gemm_f32_kernel<64, 128, EPI_GLU>.  The epilogue uses
// that kernel's helpers (statistics merge, rstd * (acc - mean * colsum) + bias_f, v * sigmoid(gate)) and the depthwise stage
// the arithmetic order of dwconv_bn_swish_kernel: the result is bit-identical to the two kernels it replaces.
//
// Time chunks: chunk i holds the GLU rows of frames [i * OUT, i * OUT + 256), OUT = 256 - (K - 1).  It owns the output frames
// whose whole window it holds: from i * OUT + (K-1)/2 (frame 0 for the first chunk, which keeps its outer margin) up to
// i * OUT + 256 - (K-1)/2 (T for the last chunk).  T <= 256 is one chunk and no recomputation; neighbouring chunks exchange
// nothing.  Rows whose frame is >= T load a clamped row and enter the LDS tile as exact zeros (the conv's zero padding).
#include "gemm_shared.h"

namespace {

#define CONVMOD_MFMA_SLICE(FA, FB)                                                                          \
    _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                           \
    _Pragma("unroll") for (int mt = 0; mt < TM; ++mt)                                                       \
    _Pragma("unroll") for (int nt = 0; nt < TN; ++nt)                                                       \
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(FB[nt][e], FA[mt][e], acc[mt][nt], 0, 0, 0)

struct ConvModArgs {
    GemmArgs g;                     // A = x, W = Wf (2C, C), bias = bias_f, ln_*: as cfm_gemm_lnfold_f32 with EPI_GLU; K = n_out = C
    const float* dw_w; const float* dw_b; const float* bn_w; const float* bn_b; const float* bn_mean; const float* bn_var;
    float bn_eps;
    float* y; int64_t ldy;
    int T, nchunks, ncg;            // frames per utterance, time chunks per utterance, channel groups (C / 64)
    int variant;                    // diagnostics: 1 = no depthwise stage (the GLU rows are stored: wrong results, same GEMM)
};

template <int K>
__global__ __launch_bounds__(512, 2) void convmod_fused_kernel(const ConvModArgs a) {
    constexpr int BM = 256, BN = 128, TM = 2, TN = 2, BK = 16, LDSR = BK + 4;
    constexpr int HALF = (K - 1) / 2, OUT = BM - (K - 1);
    constexpr int F = EPF_INFER | EPF_LN_CONSUME;
    constexpr int LDS_STAGE = 2 * (BM + BN) * LDSR;
    constexpr int TP = 64 + 4;                              // pitch of the GLU tile: 16-byte row-slab writes spread over the banks
    constexpr int LDS_TILE = (BM + K - 1) * TP;
    constexpr int LDS_MAIN = LDS_TILE > LDS_STAGE ? LDS_TILE : LDS_STAGE;
    __shared__ __attribute__((aligned(16))) float lds[LDS_MAIN + 2 * BM + 64 * K];
    float* rowstats = lds + LDS_MAIN;   // [BM][2] = (mean, rstd) of the tile's rows of x
    float* taps = rowstats + 2 * BM;    // [64][K]
    float* As = lds;                    // [2][BM][LDSR]
    float* Bs = lds + 2 * BM * LDSR;    // [2][BN][LDSR]
    float* tile = lds;                  // [BM + K - 1][TP]: row HALF + r = GLU row r of this chunk (aliases the dead staging buffers)
    const GemmArgs& g = a.g;

    // channel group fastest: the C / 64 workgroups of one (utterance, chunk) run back to back on one XCD and share its x rows in L2
    const unsigned tl = xcd_remap(blockIdx.x, gridDim.x);
    const int cg = (int)(tl % (unsigned)a.ncg);
    const unsigned uc = tl / (unsigned)a.ncg;
    const int b = (int)(uc / (unsigned)a.nchunks), ch = (int)(uc % (unsigned)a.nchunks);
    const int f0 = ch * OUT;                                // frame of GLU row 0 (< T: the launcher's chunk count)
    const int64_t m0 = (int64_t)b * a.T + f0;               // row of x of GLU row 0
    const int rows_here = min(BM, a.T - f0);                // GLU rows inside the utterance
    const int n0 = cg * 64;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, hf = lane >> 5;

    constexpr int CPR = BK / 4, RPP = 512 / CPR, PA = BM / RPP, PB = BN / RPP;   // 2 rows of x and 1 of W per thread
    const int chunk = tid & (CPR - 1), srow = tid / CPR;
    const float* a_ptr[PA];
    const float* w_ptr[PB];
#pragma unroll
    for (int i = 0; i < PA; ++i) a_ptr[i] = g.A + (m0 + min(srow + RPP * i, rows_here - 1)) * g.lda + chunk * 4;   // clamped: never stored
#pragma unroll
    for (int i = 0; i < PB; ++i) w_ptr[i] = w_row_ptr<EPI_GLU, BN>(g, n0, srow + RPP * i) + chunk * 4;

    const int nkt = g.K / BK;                               // (C % 64 == 0: no K guard)
    f32x4 ra0[PA], rb0[PB], ra1[PA], rb1[PB];               // tiles t+1 and t+2 in flight
    auto load_tile = [&](f32x4 (&ra)[PA], f32x4 (&rb)[PB], int kt) __attribute__((always_inline)) {
        const int k = kt * BK;
#pragma unroll
        for (int i = 0; i < PA; ++i) ra[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + k);
#pragma unroll
        for (int i = 0; i < PB; ++i) rb[i] = *reinterpret_cast<const f32x4*>(w_ptr[i] + k);
    };
    auto store_tile = [&](const f32x4 (&ra)[PA], const f32x4 (&rb)[PB], int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PA; ++i)
            *reinterpret_cast<f32x4*>(As + (buf * BM + srow + RPP * i) * LDSR + chunk * 4) = ra[i];
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

    const int a_row = wr * (BM / 4) + li, b_row = wc * (BN / 2) + li;
    f32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
    auto read_frags = [&](f32x4 (&fa)[TM], f32x4 (&fb)[TN], int buf, int c) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < TM; ++t)
            fa[t] = *reinterpret_cast<const f32x4*>(As + (buf * BM + a_row + 32 * t) * LDSR + 8 * c + 4 * hf);
#pragma unroll
        for (int t = 0; t < TN; ++t)
            fb[t] = *reinterpret_cast<const f32x4*>(Bs + (buf * BN + b_row + 32 * t) * LDSR + 8 * c + 4 * hf);
    };

    // the statistics partials of the tile's rows: one contiguous block, requested first (see gemm_f32_kernel, LN == 1)
    constexpr int LN_NL = (BM * 16 / 2 + 511) / 512;                   // float4 loads per thread at 16 partials per row
    f32x4 lnq[LN_NL];
    float2 ln1 = {0.f, 0.f};
    if (g.ln_parts >= 2) {
        const int nf4 = rows_here * (g.ln_parts >> 1);
        const f32x4* sp = reinterpret_cast<const f32x4*>(g.ln_stats + m0 * g.ln_parts * 2);
#pragma unroll
        for (int i = 0; i < LN_NL; ++i) lnq[i] = sp[min(tid + 512 * i, nf4 - 1)];
    } else {
        ln1 = reinterpret_cast<const float2*>(g.ln_stats)[m0 + min(tid, rows_here - 1)];
    }
    load_tile(ra0, rb0, 0);
    store_tile(ra0, rb0, 0);
    load_tile(ra1, rb1, min(1, nkt - 1));
    load_tile(ra0, rb0, min(2, nkt - 1));
    {
        // Merge (Chan, equal counts at every level, fixed tree order): the arithmetic of gemm_f32_kernel's LN == 1 prologue
        const float ni = (float)(g.K / g.ln_parts), inv_ni = 1.0f / ni, inv_k = 1.0f / (float)g.K;
        if (g.ln_parts >= 2) {
            const int lpr = g.ln_parts >> 1;                             // lanes per row: 1, 2, 4 or 8
#pragma unroll
            for (int i = 0; i < LN_NL; ++i) {
                const float ma = lnq[i][0] * inv_ni, mb = lnq[i][2] * inv_ni, d0 = mb - ma;
                float mean = 0.5f * (ma + mb), m2 = lnq[i][1] + lnq[i][3] + d0 * d0 * (0.5f * ni), cnt = 2.0f * ni;
                for (int st = 1; st < lpr; st <<= 1) {                    // (kernel-uniform trip count)
                    const float mo = __shfl_xor(mean, st, 64), m2o = __shfl_xor(m2, st, 64), dl = mo - mean;
                    mean = 0.5f * (mean + mo);
                    m2 = m2 + m2o + dl * dl * (0.5f * cnt);
                    cnt *= 2.0f;
                }
                const int f = tid + 512 * i, row = f / lpr;
                if ((f & (lpr - 1)) == 0 && row < BM) {
                    rowstats[2 * row] = mean;
                    rowstats[2 * row + 1] = 1.0f / sqrtf(m2 * inv_k + g.ln_eps);
                }
            }
        } else if (tid < BM) {
            rowstats[2 * tid] = ln1.x * inv_k;
            rowstats[2 * tid + 1] = 1.0f / sqrtf(ln1.y * inv_k + g.ln_eps);
        }
    }
    __syncthreads();
    read_frags(fa0, fb0, 0, 0);
    auto k_step = [&](int kt, f32x4 (&ra)[PA], f32x4 (&rb)[PB]) __attribute__((always_inline)) {   // (ra, rb) holds tile kt+1 on entry
        const int cur = kt & 1;
        const bool more = kt + 1 < nkt;
        read_frags(fa1, fb1, cur, 1);
        __builtin_amdgcn_sched_barrier(0);
        CONVMOD_MFMA_SLICE(fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        if (more) store_tile(ra, rb, cur ^ 1);
        load_tile(ra, rb, min(kt + 3, nkt - 1));
        __syncthreads();
        if (more) read_frags(fa0, fb0, cur ^ 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        CONVMOD_MFMA_SLICE(fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
    };
    int kt = 0;
    for (; kt + 1 < nkt; kt += 2) {
        k_step(kt, ra1, rb1);
        k_step(kt + 1, ra0, rb0);
    }
    if (kt < nkt) k_step(kt, ra1, rb1);

    // ---- epilogue 1: taps to LDS and registers; its barrier also retires the staging buffers
    float wt[K];
    load_taps<K>(a.dw_w, n0, g.n_out, taps, wt);

    // ---- epilogue 2: LN-fold consumer arithmetic + GLU of the accumulators -> the LDS tile (exact zeros outside [0, T) and in the halo)
    for (int f = tid; f < (K - 1) * 64; f += 512) {
        const int r = f >> 6;
        tile[(r < HALF ? r : BM + r) * TP + (f & 63)] = 0.f;
    }
    {
        EpiOps ob[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) gemm_epilogue_fetch_bias<EPI_GLU, F>(g, n0 + wc * 32 + 8 * q + 4 * hf, ob[q]);
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            const int lrow = wr * (BM / 4) + mt * 32 + li;
            const float mean = rowstats[2 * lrow], rstd = rowstats[2 * lrow + 1];
            const bool live = lrow < rows_here;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 av = f32x4{acc[mt][0][4 * q], acc[mt][0][4 * q + 1], acc[mt][0][4 * q + 2], acc[mt][0][4 * q + 3]};
                f32x4 gv = f32x4{acc[mt][1][4 * q], acc[mt][1][4 * q + 1], acc[mt][1][4 * q + 2], acc[mt][1][4 * q + 3]};
                av = (av - mean * ob[q].cs) * rstd;                       // (gemm_epilogue_apply, LN == 1)
                gv = (gv - mean * ob[q].cg) * rstd;
                f32x4 zpre;
                const f32x4 v = gemm_epilogue_compute<EPI_GLU, F>(g, av, gv, ob[q], m0 + lrow, n0 + wc * 32 + 8 * q + 4 * hf, zpre);
                *reinterpret_cast<f32x4*>(tile + (HALF + lrow) * TP + wc * 32 + 8 * q + 4 * hf) = live ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    __syncthreads();

    // ---- epilogue 3: depthwise conv + BatchNorm (eval) + Swish out of LDS: lane = channel, a wave takes 32 consecutive frames;
    //      the arithmetic order of dwconv_bn_swish_kernel (a zero window entry leaves an fmaf chain unchanged)
    constexpr int TT = 32;
    const int c = n0 + lane;
    const int lo0 = wave * TT;                              // first local output frame of this wave
    const int lo_begin = ch == 0 ? 0 : HALF;                // owned local output frames: [lo_begin, lo_end)
    const int lo_end = ch == a.nchunks - 1 ? a.T - f0 : BM - HALF;
    if (lo0 >= lo_end || lo0 + TT <= lo_begin) return;      // wave-uniform
    float* yb = a.y + m0 * a.ldy + c;
    if (a.variant == 1) {
#pragma unroll 4
        for (int o = 0; o < TT; ++o) {
            const int lo = lo0 + o;
            if (lo >= lo_begin && lo < lo_end) yb[(int64_t)lo * a.ldy] = tile[(HALF + lo) * TP + lane];
        }
        return;
    }
    float cacc[TT];
    const float bi = a.dw_b[c];
#pragma unroll
    for (int o = 0; o < TT; ++o) cacc[o] = bi;
    float win[TT + K - 1];
#pragma unroll
    for (int i = 0; i < TT + K - 1; ++i) win[i] = tile[(lo0 + i) * TP + lane];
#pragma unroll
    for (int o = 0; o < TT; ++o)
#pragma unroll
        for (int j = 0; j < K; ++j) cacc[o] = fmaf(wt[j], win[o + j], cacc[o]);
    const float inv = 1.0f / sqrtf(a.bn_var[c] + a.bn_eps);
    const float mu = a.bn_mean[c], ga = a.bn_w[c], be = a.bn_b[c];
#pragma unroll
    for (int o = 0; o < TT; ++o) {
        const int lo = lo0 + o;
        if (lo >= lo_begin && lo < lo_end) yb[(int64_t)lo * a.ldy] = swishf_acc((cacc[o] - mu) * inv * ga + be);
    }
}

int g_convmod_dbg = 0;

// time chunks of an utterance of T frames at tap count K (see the header comment; ops.convmod_chunks mirrors it)
inline int convmod_chunks(int T, int K) { return T <= 256 ? 1 : 1 + (T - 256 + (256 - K)) / (257 - K); }

}  // namespace

extern "C" int cfm_convmod_glu_dwconv_f32(const float* x, int64_t ldx, const float* ln_stats, int ln_parts, float ln_eps,
                                          const float* Wf, const float* bias_f, const float* colsum, const float* dw_w,
                                          const float* dw_b, const float* bn_w, const float* bn_b, const float* bn_mean,
                                          const float* bn_var, float bn_eps, float* y, int64_t ldy, int B, int T, int C, int K,
                                          cfm_stream_t stream) {
    CFM_REQUIRE(x && ln_stats && Wf && bias_f && colsum && dw_w && dw_b && bn_w && bn_b && bn_mean && bn_var && y, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && T > 0 && C > 0 && ldx >= C && ldy >= C && ln_eps >= 0.f, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(K == 31 || K == 15 || K == 7 || K == 3, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512, CFM_ERR_UNSUPPORTED);       // C % 64 == 0 and a width the LN fold carries
    CFM_REQUIRE(ln_parts >= 1 && C % ln_parts == 0, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(ln_parts <= 16 && (ln_parts & (ln_parts - 1)) == 0, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((ldx & 3) == 0 && CFM_ALIGNED16(x) && CFM_ALIGNED16(Wf) && CFM_ALIGNED16(bias_f) && CFM_ALIGNED16(colsum),
                CFM_ERR_ALIGN);
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(ln_stats) & (ln_parts >= 2 ? 15u : 7u)) == 0, CFM_ERR_ALIGN);
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(y) & 3u) == 0, CFM_ERR_ALIGN);
    ConvModArgs a{};
    a.g.A = x; a.g.W = Wf; a.g.bias = bias_f; a.g.M = (int64_t)B * T; a.g.N = 2 * C; a.g.K = C; a.g.n_out = C; a.g.lda = ldx;
    a.g.alpha = 1.f; a.g.ln_stats = ln_stats; a.g.ln_parts = ln_parts; a.g.ln_eps = ln_eps; a.g.ln_colsum = colsum;
    a.dw_w = dw_w; a.dw_b = dw_b; a.bn_w = bn_w; a.bn_b = bn_b; a.bn_mean = bn_mean; a.bn_var = bn_var; a.bn_eps = bn_eps;
    a.y = y; a.ldy = ldy; a.T = T; a.nchunks = convmod_chunks(T, K); a.ncg = C / 64; a.variant = g_convmod_dbg;
    const int64_t nwg = (int64_t)B * a.nchunks * a.ncg;
    CFM_REQUIRE(nwg < ((int64_t)1 << 31), CFM_ERR_BAD_SHAPE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)nwg), block(512);
    switch (K) {
        case 31: hipLaunchKernelGGL(convmod_fused_kernel<31>, grid, block, 0, s, a); break;
        case 15: hipLaunchKernelGGL(convmod_fused_kernel<15>, grid, block, 0, s, a); break;
        case 7: hipLaunchKernelGGL(convmod_fused_kernel<7>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(convmod_fused_kernel<3>, grid, block, 0, s, a);
    }
    return cfm_launch_status();
}

// diagnostics (tools/convmod_fused_ab.py): 0 | 1 = no depthwise stage (the GLU rows are stored: wrong results, the same GEMM).
// Returns the previous value.
extern "C" int cfm_debug_convmod_variant(int v) { const int p = g_convmod_dbg; g_convmod_dbg = v; return p; }
