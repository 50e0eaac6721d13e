/*
 * conformer_hip_resample.h -- extension of the C ABI of libconformer_hip.so (include/conformer_hip.h): the polyphase resampler
 * in front of the audio front end.  Same conventions as the main header (device pointers, caller-owned buffers, launches
 * enqueued on `stream`, 0 or a negative cfm_status).  Not included by conformer_hip.h and no CFM_* define of its own: the
 * entries here are ADDED to the library, so CFM_ABI_VERSION does not move; a binding looks them up separately and asks for a
 * rebuild when a library lacks them.
 */
#ifndef CONFORMER_HIP_RESAMPLE_H
#define CONFORMER_HIP_RESAMPLE_H

#include "conformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Input sample rates (INTEGRATION.md "Input sample rates"): one launch per step for S independent streams, or for the S rows
 * of an offline batch.  Rates R_in -> R_out with g = gcd, o = R_in / g, n = R_out / g; bank_t is the Hann-windowed-sinc bank
 * TRANSPOSED, (K, n) fp32 with K = 2 width + o, bank_t[m * n + j] = k[j, m].  Output q = i n + j of a stream is
 *          y[q] = sum_m k[j, m] x[i o - width + m]      (x = 0 outside the stream),
 *      accumulated in fp32 as acc = k[j,0] x[.], then acc = fma(k[j,m], x[.], acc) for m = 1 .. K-1 in that order: the order of
 *      the K terms depends on the phase alone, so how a stream is cut into steps changes no bit.
 *
 *      samples: (S, ld_samples) elements of `n_max` frames at most, a frame = C interleaved channels (1 <= C <= 8), float32
 *      (cfm_resample_f32) or int16 (cfm_resample_i16: float(v) * 2^-15).  A frame becomes one fp32 sample
 *      (x_0 + x_1 + ... + x_{C-1}) * fp32(1 / C), summed left to right.
 *      Slot b carries a tail, the samples of its stream that a later output needs (< K of them), in row b of a (S, 1024) fp32
 *      buffer.  With cat_b = [tail_in[b, :tail_len] | the n_new converted frames of samples[b]], m = tail_len + n_new, and
 *      xz[c] = cat_b[c] for 0 <= c < m, 0 otherwise, the slot's row of `table` (S, 8) int32 =
 *      {tail_len, n_new, lead, n_out, flush, keep, new_tail_len, 0} asks for
 *          y[b, r]        = sum_m k[j, m] xz[i o + m - lead],  r = i n + j,  0 <= r < n_out
 *          y[b, r]        = 0,  n_out <= r < ld_y
 *          tail_out[b, t] = cat_b[keep + t], 0 <= t < new_tail_len (0 when flush is set); the rest of the 1024 floats = 0.
 *      lead = the zeros in front of the stream that the first outputs still see (width until the first block is out).  The
 *      offline call is the same launch with tail_in = tail_out = NULL (both or neither), lead = width and every row flushed.
 *
 *      A workgroup computes RUN = 1024 outputs at most of one slot, in whole blocks of n: bpw = max(1, RUN / n) blocks,
 *      fewer if their input span bpw o + 2 width would pass the 12288 floats (48 KiB) of LDS it is staged in, converted once;
 *      K <= 1024 keeps one block inside that budget, so no supported bank is refused for LDS.  A bank of n K <= 2048 floats
 *      (n <= 2) is kept in LDS as well.
 *
 *      The kernel clamps every table value it indexes with (tail_len to [0, 1024] and 0 without tails, n_new to [0, n_max],
 *      lead to [0, width], n_out to [0, ld_y], keep to [0, m], new_tail_len to [0, min(1024, m - keep)]) and reads cat_b only at
 *      0 <= c < m: a corrupt table cannot read or write outside the buffers.
 *
 *      Refused before any launch: a null table, bank_t or y, null samples with n_max > 0, exactly one of the tails null
 *      (CFM_ERR_NULL); S <= 0, n_max < 0, C < 1, ld_samples < n_max C, o < 1, n < 1, width < 0, ld_y < 0, ld_y % 4 != 0
 *      (CFM_ERR_BAD_SHAPE); K > 1024, n > 640, C > 8, S >= 65535, ld_y >= 2^30, n_max C >= 2^30, overlapping tails
 *      (CFM_ERR_UNSUPPORTED); y, tail_in, tail_out or bank_t not 16-byte aligned, samples not aligned to its element
 *      (CFM_ERR_ALIGN). */
int cfm_resample_f32(const float* samples, int64_t ld_samples, int n_max, int C, const float* tail_in, float* tail_out,
                     const int* table, const float* bank_t, int o, int n, int width, float* y, int64_t ld_y, int S,
                     cfm_stream_t stream);
int cfm_resample_i16(const void* samples, int64_t ld_samples, int n_max, int C, const float* tail_in, float* tail_out,
                     const int* table, const float* bank_t, int o, int n, int width, float* y, int64_t ld_y, int S,
                     cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
