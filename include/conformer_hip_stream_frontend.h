/*
 * conformer_hip_stream_frontend.h -- extension of the C ABI of libconformer_hip.so (include/conformer_hip.h): the staging step
 * of the streaming audio front end.  Same conventions as the main header (device pointers, caller-owned buffers, launches
 * enqueued on `stream`, 0 or a negative cfm_status).  Not included by conformer_hip.h and no CFM_* define of its own: the entry
 * here is ADDED to the library, so CFM_ABI_VERSION does not move; a binding looks it up separately and asks for a rebuild when
 * a library lacks it.
 */
#ifndef CONFORMER_HIP_STREAM_FRONTEND_H
#define CONFORMER_HIP_STREAM_FRONTEND_H

#include "conformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Streaming audio front end (INTEGRATION.md "Streaming audio front end"): one launch per step for S independent streams.
 *      Slot b carries a tail, the last samples of its stream that a later frame needs (< n_fft of them), in row b of a
 *      (S, 512) fp32 buffer.  With cat_b = [tail_in[b, :tail_len] | samples[b, :n_new]], m = tail_len + n_new, the slot's row of
 *      `table` (S, 8) int32 = {tail_len, n_new, lead, n_frames, flush, off, keep, new_tail_len} asks for
 *          segment[i]  = cat_b[r(i - lead + off)],  0 <= i < (n_frames - 1) hop + n_fft  (no segment when n_frames = 0),
 *                        r(c) = -c for c < 0 (the opening of the utterance reflected), 2 (m - 1) - c for c >= m (its end
 *                        reflected: a flush step), c otherwise
 *          tail_out[b, j] = cat_b[keep + j], 0 <= j < new_tail_len (0 when flush is set); the rest of the 512 floats = 0.
 *      The segment is written at xp + b * rpu * hop, rpu = f_max + ceil(n_fft / hop): the layout of cfm_dft_frames_f32 (rows =
 *      S * rpu, lda = hop) and cfm_power_mel_log_mfma_f32 (T = f_max, rows_per_utt = rpu).  Every other float of the slot's
 *      pitch and the n_fft floats behind the last slot are written as 0: xp holds S * rpu * hop + n_fft floats, all written.
 *      samples: (S, ld_samples) fp32, n_max <= ld_samples the most new samples a row may claim (samples may be null when n_max
 *      is 0).  tail_in and tail_out must not overlap (the tails ping-pong); nothing the launch reads is written by it.
 *
 *      The kernel clamps every table value it indexes with (tail_len to [0, 512], n_new to [0, n_max], lead to [0, n_fft], off
 *      to [0, 512], n_frames to [0, f_max] and 0 when m = 0, keep to [0, m], new_tail_len to [0, min(512, m - keep)], every cat
 *      index to [0, m)): a corrupt table cannot read or write outside the buffers.
 *
 *      Refused before any launch: a null pointer (CFM_ERR_NULL); S <= 0, f_max < 0, n_max < 0, ld_samples < n_max, hop <= 0,
 *      hop % 4 != 0, n_fft % 4 != 0, hop > n_fft (CFM_ERR_BAD_SHAPE); n_fft > 512, S >= 65535, a pitch of 2^30 floats or
 *      more, n_max >= 2^29, overlapping tails (CFM_ERR_UNSUPPORTED); xp not 16-byte aligned (CFM_ERR_ALIGN). */
int cfm_stream_stage_f32(const float* samples, int64_t ld_samples, int n_max, const float* tail_in, float* tail_out,
                         const int* table, float* xp, int S, int f_max, int hop, int n_fft, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
