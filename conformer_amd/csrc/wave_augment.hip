// Waveform augmentation in front of the log-mel: reverberation (a per-row FIR), the SNR mix with gain, and the row copy that
// gathers and scatters the speed groups.  The definitions, the tables and the refusals: conformer_hip3_waveaug.h.
#include <math.h>
#include "cfm_common.h"
#include "conformer_hip3_waveaug.h"

namespace {

constexpr int ROW_COLS = CFM3_WAVE_ROW_COLS;
constexpr int THREADS = 256;
constexpr int FIR_R = 8;                                   // consecutive outputs per lane
constexpr int FIR_T = CFM3_WAVE_FIR_TILE_T;                // outputs per workgroup
constexpr int FIR_S = CFM3_WAVE_FIR_TILE_K;                // taps per staged tile
constexpr int FIR_XS = FIR_T + FIR_S;                      // staged inputs per tap tile (index 0 is never read)
constexpr int POWER_CHUNK = CFM3_WAVE_POWER_CHUNK;
constexpr int MIX_TILE = CFM3_WAVE_MIX_TILE;
constexpr int COPY_TILE = 4096;
static_assert(FIR_T == THREADS * FIR_R && FIR_S % 16 == 0 && FIR_S <= THREADS && FIR_XS % 16 == 0, "FIR tiling");
static_assert(POWER_CHUNK % THREADS == 0 && MIX_TILE % THREADS == 0 && COPY_TILE % THREADS == 0, "tiles in whole passes");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the row's length as every kernel here reads it
__device__ __forceinline__ int row_length(const int* __restrict__ rows, int b, int64_t ld_x, int W) {
    return clampi(rows[b * ROW_COLS], 0, (int)min<int64_t>(ld_x, W));
}

// LDS image of the staged inputs: float i lies at i ^ ((i >> 4) & 4), i.e. the two 16-byte halves of every other 8-float group
// are swapped.  A lane reads whole 8-float groups, lane stride one group: the 16 lanes a ds_read_b128 serves together then hit
// 16 different 16-byte slots of the 256-byte bank row (unswizzled they pair up on 8).
__device__ __forceinline__ int xs_at(int i) { return i ^ ((i >> 4) & 4); }

__device__ __forceinline__ void load_group(const float* xs, int q, float (&w)[8]) {     // floats 8 q .. 8 q + 7
    const int flip = (q >> 1) & 4;
    const f32x4 a = *reinterpret_cast<const f32x4*>(xs + 8 * q + flip);
    const f32x4 c = *reinterpret_cast<const f32x4*>(xs + 8 * q + (flip ^ 4));
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = c.x; w[5] = c.y; w[6] = c.z; w[7] = c.w;
}

// acc[r] += h[j] * x(window position r - j), the window being lo = positions -8 .. -1 and hi = positions 0 .. 7
__device__ __forceinline__ void fir_taps8(float (&acc)[FIR_R], const float* hs, const float (&lo)[8], const float (&hi)[8]) {
    const f32x4 h0 = *reinterpret_cast<const f32x4*>(hs), h1 = *reinterpret_cast<const f32x4*>(hs + 4);
    const float h[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < FIR_R; ++r) acc[r] = fmaf(h[j], r >= j ? hi[r - j] : lo[8 + r - j], acc[r]);
}

__global__ __launch_bounds__(THREADS) void wave_fir_kernel(const float* __restrict__ x, int64_t ld_x, const int* __restrict__ rows,
                                                           const float* __restrict__ taps, const int* __restrict__ tap_offsets,
                                                           const int* __restrict__ tap_delays, int R, int n_taps, int k_max,
                                                           float* __restrict__ y, int64_t ld_y, int W) {
    __shared__ __attribute__((aligned(16))) float lds[FIR_XS + FIR_S];
    float* xs = lds;
    float* hs = lds + FIR_XS;
    const int b = blockIdx.y, tid = threadIdx.x, t0 = blockIdx.x * FIR_T;
    const int L = row_length(rows, b, ld_x, W);
    const int rir = clampi(rows[b * ROW_COLS + 1], -1, R - 1);
    const float* xr = x + (int64_t)b * ld_x;
    float* yr = y + (int64_t)b * ld_y;
    const int tl = t0 + tid * FIR_R;                        // the lane's first output
    float acc[FIR_R];
#pragma unroll
    for (int r = 0; r < FIR_R; ++r) acc[r] = 0.f;
    if (t0 < L) {
        if (rir < 0) {
#pragma unroll
            for (int r = 0; r < FIR_R; ++r) acc[r] = tl + r < L ? xr[tl + r] : 0.f;
        } else {
            const int off = clampi(tap_offsets[rir], 0, n_taps);
            const int K = clampi(tap_offsets[rir + 1] - off, 0, min(k_max, n_taps - off));
            const int d = clampi(tap_delays[rir], 0, max(K - 1, 0));
            const float* h = taps + off;
            for (int k0 = 0; k0 < K; k0 += FIR_S) {
                // staged input i is x[g0 + i]; output t0 + 8 l + r with tap k0 + kk reads i = 8 l + r + FIR_S - kk
                const int g0 = t0 + d - k0 - FIR_S;
                if (g0 + FIR_XS <= 0 || g0 >= L) continue;                       // (block-uniform) nothing but zeros in reach
                __syncthreads();                                                 // the last tile's readers are done
                for (int i = tid; i < FIR_XS; i += THREADS) {
                    const int g = g0 + i;
                    xs[xs_at(i)] = g >= 0 && g < L ? xr[g] : 0.f;
                }
                if (tid < FIR_S) hs[tid] = k0 + tid < K ? h[k0 + tid] : 0.f;
                __syncthreads();
                float wa[8], wb[8];
                load_group(xs, tid + FIR_S / 8, wa);                             // positions 0 .. 7 of the first 8 taps
                for (int c = 0; c < FIR_S / 8; c += 2) {
                    const int q = tid + FIR_S / 8 - c;                           // the group of positions 0 .. 7
                    load_group(xs, q - 1, wb);
                    fir_taps8(acc, hs + 8 * c, wb, wa);
                    load_group(xs, q - 2, wa);
                    fir_taps8(acc, hs + 8 * c + 8, wa, wb);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < FIR_R; ++r)
        if (tl + r < W) yr[tl + r] = tl + r < L ? acc[r] : 0.f;
}

// block-wide sum of a double in a fixed tree: butterfly in the wave, then the waves in order
__device__ __forceinline__ double block_sum(double v, double* scratch) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = scratch[0];
    for (int w = 1; w < THREADS / 64; ++w) s += scratch[w];
    return s;
}

struct Clip { const float* p; int n; };

__device__ __forceinline__ Clip row_clip(const int* __restrict__ rows, int b, const float* __restrict__ noise,
                                         const int* __restrict__ clip_offsets, int N, int n_noise) {
    const int c = N > 0 ? clampi(rows[b * ROW_COLS + 2], -1, N - 1) : -1;
    if (c < 0) return {nullptr, 0};
    const int off = clampi(clip_offsets[c], 0, n_noise);
    const int n = clampi(clip_offsets[c + 1] - off, 0, n_noise - off);
    return {n > 0 ? noise + off : nullptr, n};
}

__global__ __launch_bounds__(THREADS) void wave_power_kernel(const float* __restrict__ x, int64_t ld_x, const int* __restrict__ rows,
                                                             const float* __restrict__ noise, const int* __restrict__ clip_offsets,
                                                             int N, int n_noise, int l_max, double* __restrict__ partial) {
    __shared__ double scratch[THREADS / 64];
    const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    const Clip clip = row_clip(rows, b, noise, clip_offsets, N, n_noise);
    if (!clip.p) return;                                                         // (block-uniform)
    const int L = row_length(rows, b, ld_x, l_max);
    const float* xr = x + (int64_t)b * ld_x;
    const unsigned nc = (unsigned)clip.n, step = THREADS % nc;
    const unsigned s = (unsigned)max(rows[b * ROW_COLS + 3], 0) % nc;
    const int t_first = p * POWER_CHUNK + tid;
    unsigned idx = (unsigned)(((uint64_t)s + (uint64_t)t_first) % nc);
    double px = 0.0, pn = 0.0;
    for (int t = t_first; t < min(L, (p + 1) * POWER_CHUNK); t += THREADS) {
        const double xv = xr[t], nv = clip.p[idx];
        px = fma(xv, xv, px);
        pn = fma(nv, nv, pn);
        idx += step;
        if (idx >= nc) idx -= nc;
    }
    px = block_sum(px, scratch);
    pn = block_sum(pn, scratch);
    if (tid == 0) {
        partial[((int64_t)b * P + p) * 2] = px;
        partial[((int64_t)b * P + p) * 2 + 1] = pn;
    }
}

__global__ __launch_bounds__(THREADS) void wave_mix_kernel(const float* x, int64_t ld_x, const int* __restrict__ rows,
                                                           const double* __restrict__ coef, const float* __restrict__ noise,
                                                           const int* __restrict__ clip_offsets, int N, int n_noise,
                                                           const double* __restrict__ partial, int l_max, float* y, int64_t ld_y,
                                                           int W) {
    const int b = blockIdx.y, tid = threadIdx.x, t0 = blockIdx.x * MIX_TILE;
    const bool mix = rows[b * ROW_COLS + 4] != 0, in_place = x == y;
    if (!mix && in_place) return;                                                // (block-uniform) the row stays as it is
    const int Lp = row_length(rows, b, ld_x, l_max);                             // what the power kernel summed over
    const int L = min(Lp, W);
    const float* xr = x + (int64_t)b * ld_x;
    float* yr = y + (int64_t)b * ld_y;
    const int t_end = min(W, t0 + MIX_TILE);
    if (!mix) {
        for (int t = t0 + tid; t < t_end; t += THREADS) yr[t] = t < L ? xr[t] : 0.f;
        return;
    }
    const Clip clip = row_clip(rows, b, noise, clip_offsets, N, n_noise);
    const double a = coef[b * 2 + 1];
    double g = 0.0;
    if (clip.p) {
        const int P = (l_max + POWER_CHUNK - 1) / POWER_CHUNK, used = (Lp + POWER_CHUNK - 1) / POWER_CHUNK;
        double px = 0.0, pn = 0.0;
        for (int p = 0; p < used; ++p) {                                         // the chunks in order, in every thread alike
            px += partial[((int64_t)b * P + p) * 2];
            pn += partial[((int64_t)b * P + p) * 2 + 1];
        }
        if (px > 0.0 && pn > 0.0) g = sqrt(px / (pn * coef[b * 2]));
    }
    const float c1 = (float)a, c2 = (float)(a * g);
    if (!clip.p) {
        for (int t = t0 + tid; t < t_end; t += THREADS) yr[t] = t < L ? c1 * xr[t] : 0.f;
        return;
    }
    const unsigned nc = (unsigned)clip.n, step = THREADS % nc;
    const unsigned s = (unsigned)max(rows[b * ROW_COLS + 3], 0) % nc;
    unsigned idx = (unsigned)(((uint64_t)s + (uint64_t)(t0 + tid)) % nc);
    for (int t = t0 + tid; t < t_end; t += THREADS) {
        yr[t] = t < L ? fmaf(c2, clip.p[idx], c1 * xr[t]) : 0.f;
        idx += step;
        if (idx >= nc) idx -= nc;
    }
}

__global__ __launch_bounds__(THREADS) void wave_copy_rows_kernel(const float* __restrict__ x, int64_t ld_x, int n_src,
                                                                 float* __restrict__ y, int64_t ld_y, int W, int n_dst,
                                                                 const int* __restrict__ map) {
    const int e = blockIdx.y, t0 = blockIdx.x * COPY_TILE;
    const int src = clampi(map[e * 4], 0, n_src - 1), dst = clampi(map[e * 4 + 1], 0, n_dst - 1);
    const int L = clampi(map[e * 4 + 2], 0, (int)min<int64_t>(ld_x, W));
    const float* xr = x + (int64_t)src * ld_x;
    float* yr = y + (int64_t)dst * ld_y;
    for (int t = t0 + threadIdx.x; t < min(W, t0 + COPY_TILE); t += THREADS) yr[t] = t < L ? xr[t] : 0.f;
}

constexpr int64_t DIM_MAX = (int64_t)1 << 30;

}  // namespace

extern "C" int cfm3_wave_copy_rows_f32(const float* x, int64_t ld_x, int n_src, float* y, int64_t ld_y, int W, int n_dst,
                                       const int* map, int n, cfm_stream_t stream) {
    CFM_REQUIRE(x && y && map, CFM_ERR_NULL);
    CFM_REQUIRE(n >= 1 && n_src >= 1 && n_dst >= 1 && W >= 1 && ld_x >= 1 && ld_y >= W, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(n <= 65535 && W < DIM_MAX && ld_x < DIM_MAX && x != y, CFM_ERR_UNSUPPORTED);
    const dim3 grid((unsigned)((W + COPY_TILE - 1) / COPY_TILE), (unsigned)n);
    hipLaunchKernelGGL(wave_copy_rows_kernel, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, ld_x, n_src, y, ld_y, W,
                       n_dst, map);
    return cfm_launch_status();
}

extern "C" int cfm3_wave_fir_f32(const float* x, int64_t ld_x, const int* rows, const float* taps, const int* tap_offsets,
                                 const int* tap_delays, int R, int n_taps, int k_max, float* y, int64_t ld_y, int W, int B,
                                 cfm_stream_t stream) {
    CFM_REQUIRE(x && rows && taps && tap_offsets && tap_delays && y, CFM_ERR_NULL);
    CFM_REQUIRE(B >= 1 && R >= 1 && n_taps >= 1 && k_max >= 1 && k_max <= n_taps, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(W >= 1 && ld_x >= 1 && ld_y >= W, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(k_max <= CFM3_WAVE_FIR_MAX_TAPS && B <= 65535 && W < DIM_MAX && ld_x < DIM_MAX && x != y, CFM_ERR_UNSUPPORTED);
    const dim3 grid((unsigned)((W + FIR_T - 1) / FIR_T), (unsigned)B);
    hipLaunchKernelGGL(wave_fir_kernel, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, ld_x, rows, taps, tap_offsets,
                       tap_delays, R, n_taps, k_max, y, ld_y, W);
    return cfm_launch_status();
}

extern "C" int cfm3_wave_power_f64(const float* x, int64_t ld_x, const int* rows, const float* noise, const int* clip_offsets,
                                   int N, int n_noise, int l_max, double* partial, int B, cfm_stream_t stream) {
    CFM_REQUIRE(x && rows && noise && clip_offsets && partial, CFM_ERR_NULL);
    CFM_REQUIRE(B >= 1 && N >= 1 && n_noise >= 1 && l_max >= 1 && ld_x >= 1, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(B <= 65535 && l_max < DIM_MAX && ld_x < DIM_MAX, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(partial) & 7u) == 0, CFM_ERR_ALIGN);
    const dim3 grid((unsigned)((l_max + POWER_CHUNK - 1) / POWER_CHUNK), (unsigned)B);
    hipLaunchKernelGGL(wave_power_kernel, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, ld_x, rows, noise,
                       clip_offsets, N, n_noise, l_max, partial);
    return cfm_launch_status();
}

extern "C" int cfm3_wave_mix_f32(const float* x, int64_t ld_x, const int* rows, const double* coef, const float* noise,
                                 const int* clip_offsets, int N, int n_noise, const double* partial, int l_max, float* y,
                                 int64_t ld_y, int W, int B, cfm_stream_t stream) {
    CFM_REQUIRE(x && rows && coef && y, CFM_ERR_NULL);
    CFM_REQUIRE(N <= 0 || (noise && clip_offsets && partial), CFM_ERR_NULL);
    CFM_REQUIRE(B >= 1 && N >= 0 && (N == 0 || n_noise >= 1) && l_max >= 1, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(W >= 1 && ld_x >= 1 && ld_y >= W, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(B <= 65535 && W < DIM_MAX && l_max < DIM_MAX && ld_x < DIM_MAX && (x != y || ld_x == ld_y), CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(coef) & 7u) == 0 && (reinterpret_cast<uintptr_t>(partial) & 7u) == 0, CFM_ERR_ALIGN);
    const dim3 grid((unsigned)((W + MIX_TILE - 1) / MIX_TILE), (unsigned)B);
    hipLaunchKernelGGL(wave_mix_kernel, grid, dim3(THREADS), 0, static_cast<hipStream_t>(stream), x, ld_x, rows, coef, noise,
                       clip_offsets, N, n_noise, partial, l_max, y, ld_y, W);
    return cfm_launch_status();
}
