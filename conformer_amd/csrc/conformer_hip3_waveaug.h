/*
 * conformer_hip3_waveaug.h -- third-generation entries of libconformer_hip.so: waveform augmentation on the device in front
 * of the log-mel (INTEGRATION.md "Waveform augmentation"): reverberation (a per-row FIR), additive noise at a drawn SNR and a
 * gain.  Same conventions as include/conformer_hip.h (device pointers, caller-owned buffers, launches enqueued on `stream`, 0
 * or a negative cfm_status); the third generation is open, see conformer_hip3_align_wild.h.  Speed perturbation is the
 * resampler of include/conformer_hip_resample.h; the row-copy entry here gathers and scatters its groups of rows.
 *
 * THE ROW TABLE.  `rows` is (B, 8) int32 on the device, row b = {L, rir, clip, offset, mix, 0, 0, 0}:
 *      L       samples of row b that exist (x[b, t], 0 <= t < L); samples at or behind L are never read
 *      rir     the impulse response of the row, -1 = none (cfm3_wave_fir_f32)
 *      clip    the noise clip of the row, -1 = none (cfm3_wave_power_f64, cfm3_wave_mix_f32)
 *      offset  s, where the row starts in its clip, 0 <= s < N_c
 *      mix     0 = the mix leaves the row alone (neither noise nor gain)
 * `coef` is (B, 2) float64: {10^(snr_db / 10), 10^(gain_db / 20)}, formed by the host in double.
 * Every kernel clamps what it indexes with: L to [0, min(ld_x, W)], rir to [-1, R), clip to [-1, N), the tap and clip
 * offsets to [0, n_taps] and [0, n_noise], a delay to [0, K - 1], K to [0, k_max], s to s mod N_c.  A corrupt table
 * cannot read or write outside the buffers.  W is the number of columns of y that are written (t >= L: zeros), ld_y >= W its
 * pitch: the columns W .. ld_y - 1 are never touched.
 *
 * REVERB.  Bank: R responses back to back in `taps` (n_taps floats), response r = taps[tap_offsets[r] .. tap_offsets[r + 1])
 * (tap_offsets: R + 1 int32), K_r taps, direct path at tap_delays[r].  Row b with r = rir >= 0, K = K_r, d = tap_delays[r]:
 *      y[b, t] = sum_{k=0}^{K-1} h_r[k] x[b, t + d - k],  0 <= t < L,  x = 0 outside [0, L);     y[b, t] = 0,  L <= t < W.
 * A row with rir = -1: y[b, t] = x[b, t] bit for bit, t < L, zeros behind.  fp32 fused multiply-adds; the order of the K terms
 * is fixed by (t, K, d) alone, so a run repeats bit for bit.  |y - exact| <= (K + 1) 2^-24 sum_k |h[k]| |x[t + d - k]|.
 *      The kernel: a workgroup of 256 threads takes CFM3_WAVE_FIR_TILE_T = 2048 outputs of one row, 8 consecutive outputs per
 *      lane in registers.  Per tile of CFM3_WAVE_FIR_TILE_K = 256 taps it stages the 2048 + 256 inputs the tile can touch and
 *      the taps in LDS (10 KiB), then every lane slides a 16-float register window across the taps: per 8 taps two 16-byte
 *      LDS reads of inputs (conflict-free: the two halves of every other 8-float group are swapped) and two same-address
 *      reads of taps for 64 multiply-adds.  Tap tiles whose inputs lie outside [0, L) are skipped.  Grid: (ceil(W / 2048), B);
 *      tiles behind L write zeros and do nothing else.
 *
 * MIX.  Bank: N clips back to back in `noise` (n_noise floats), clip c = noise[clip_offsets[c] .. clip_offsets[c + 1]), N_c
 * samples.  Row b with mix != 0, c = clip, n[t] = clip_c[(s + t) mod N_c]:
 *      Px = sum_{t<L} x[t]^2,  Pn = sum_{t<L} n[t]^2                       (cfm3_wave_power_f64: products and sums in double)
 *      g  = sqrt(Px / (Pn 10^(snr_db / 10)))  if Px > 0 and Pn > 0,  else 0;      a = 10^(gain_db / 20)            (double)
 *      c1 = fp32(a),  c2 = fp32(a g);      y[t] = fmaf(c2, n[t], c1 x[t])   (fp32),  t < L;      y[t] = 0,  L <= t < W.
 * clip = -1: no noise sample is read, c2 = 0 and y[t] = c1 x[t].  mix = 0: y[t] = x[t] bit for bit (in place: the row is not
 * touched).  The sums are taken per CFM3_WAVE_POWER_CHUNK = 8192 samples in a fixed tree and the chunks are added in order:
 * no atomics, the same table and input give the same bits.
 */
#ifndef CONFORMER_HIP3_WAVEAUG_H
#define CONFORMER_HIP3_WAVEAUG_H

#include "../../include/conformer_hip.h"

#define CFM3_WAVE_ROW_COLS 8
#define CFM3_WAVE_FIR_TILE_T 2048
#define CFM3_WAVE_FIR_TILE_K 256
#define CFM3_WAVE_FIR_MAX_TAPS 32768
#define CFM3_WAVE_POWER_CHUNK 8192
#define CFM3_WAVE_MIX_TILE 4096

#ifdef __cplusplus
extern "C" {
#endif

/* Gather / scatter rows with zero fill: map (n, 4) int32 on the device = {src, dst, length, 0};
 *      y[dst, t] = x[src, t], t < length;   y[dst, t] = 0, length <= t < W.
 * src is clamped to [0, n_src), dst to [0, n_dst), length to [0, min(ld_x, W)].  Two entries with one dst: undefined which
 * wins.  One launch, grid (ceil(W / 4096), n).  Refused before any launch: a null x, y or map (CFM_ERR_NULL); n, n_src,
 * n_dst < 1, W < 1, ld_x < 1, ld_y < W (CFM_ERR_BAD_SHAPE); n > 65535, W or ld_x >= 2^30, x == y (CFM_ERR_UNSUPPORTED). */
int cfm3_wave_copy_rows_f32(const float* x, int64_t ld_x, int n_src, float* y, int64_t ld_y, int W, int n_dst, const int* map,
                            int n, cfm_stream_t stream);

/* REVERB, one launch for B rows.  k_max: the longest response of the bank (the host knows it; a longer one in the table is
 * cut to k_max).  Refused before any launch: a null x, rows, taps, tap_offsets, tap_delays or y (CFM_ERR_NULL); B < 1, R < 1,
 * n_taps < 1, k_max < 1, k_max > n_taps, W < 1, ld_x < 1, ld_y < W (CFM_ERR_BAD_SHAPE); k_max > CFM3_WAVE_FIR_MAX_TAPS,
 * B > 65535, W or ld_x >= 2^30, x == y (CFM_ERR_UNSUPPORTED). */
int cfm3_wave_fir_f32(const float* x, int64_t ld_x, const int* rows, const float* taps, const int* tap_offsets,
                      const int* tap_delays, int R, int n_taps, int k_max, float* y, int64_t ld_y, int W, int B,
                      cfm_stream_t stream);

/* The powers of the MIX, one launch: partial[(b * P + p) * 2 + {0, 1}] = {sum x^2, sum n^2} over the samples
 * p 8192 <= t < min(L, (p + 1) 8192) of row b, P = ceil(l_max / 8192); rows with clip = -1 write nothing.  l_max >= every L
 * (a longer row is cut to l_max).  Refused before any launch: a null x, rows, noise, clip_offsets or partial (CFM_ERR_NULL);
 * B < 1, N < 1, n_noise < 1, l_max < 1, ld_x < 1 (CFM_ERR_BAD_SHAPE); B > 65535, l_max or ld_x >= 2^30 (CFM_ERR_UNSUPPORTED);
 * partial not 8-byte aligned (CFM_ERR_ALIGN). */
int cfm3_wave_power_f64(const float* x, int64_t ld_x, const int* rows, const float* noise, const int* clip_offsets, int N,
                        int n_noise, int l_max, double* partial, int B, cfm_stream_t stream);

/* The MIX, one launch, grid (ceil(W / 4096), B).  noise, clip_offsets and partial may be null together with N = 0 (gain
 * only: every clip counts as -1).  x == y with ld_x == ld_y is the in-place form: rows with mix = 0 are not touched.
 * Refused before any launch: a null x, rows, coef or y, a null noise, clip_offsets or partial with N > 0 (CFM_ERR_NULL);
 * B < 1, N < 0, n_noise < 1 with N > 0, l_max < 1, W < 1, ld_x < 1, ld_y < W (CFM_ERR_BAD_SHAPE); B > 65535, W, l_max or
 * ld_x >= 2^30, x == y with ld_x != ld_y (CFM_ERR_UNSUPPORTED); coef or partial not 8-byte aligned (CFM_ERR_ALIGN). */
int cfm3_wave_mix_f32(const float* x, int64_t ld_x, const int* rows, const double* coef, const float* noise,
                      const int* clip_offsets, int N, int n_noise, const double* partial, int l_max, float* y, int64_t ld_y,
                      int W, int B, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
