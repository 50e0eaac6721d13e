/*
 * conformer_hip_endpoint.h -- extension of the C ABI of libconformer_hip.so (include/conformer_hip.h): rule-based endpointing
 * on the CTC blank posterior.  Same conventions as the main header (device pointers, caller-owned buffers, launches enqueued
 * on `stream`, 0 or a negative cfm_status).  Not included by conformer_hip.h and no CFM_* define of its own: the entry here
 * is ADDED to the library, so CFM_ABI_VERSION does not move; a binding looks it up separately and asks for a rebuild when a
 * library lacks it.
 */
#ifndef CONFORMER_HIP_ENDPOINT_H
#define CONFORMER_HIP_ENDPOINT_H

#include "conformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Endpointing (INTEGRATION.md "Endpointing"): one launch per step for S independent streams.  logits: fp32, slot b's new
 * frames are the rows logits[b * ld_slot + r * ld_row + 0 .. V), r = 0 .. k[b]-1 (what a slot step returns: ld_row = V,
 * ld_slot = k_max V); rows at or beyond k[b] are never read.  k: (S) int64, clamped to [0, k_max].
 *
 *      A frame x of V logits is classified in fp32: m = max_v x_v, lse = m + log(sum_v exp(x_v - m)), and
 *          log p_sil = x_i - lse                           (n_silence = 1, i = silence_ids[0]: the blank)
 *          log p_sil = log(sum_i exp(x_i - lse))           (n_silence > 1, summed in the order of silence_ids)
 *      with silence_ids (n_silence) int32, every id clamped to [0, V).  The frame is SILENT iff log p_sil >= log_threshold (the
 *      caller passes the logarithm of its probability threshold).  Lane l of a wave takes x_l, x_{l+64}, ... in that order and
 *      the 64 partial maxima and sums are folded by a fixed butterfly: the flag of a frame depends on its V logits alone, so how
 *      a stream is cut into steps changes no flag.  A frame with a NaN in it is not silent (the comparison is false); neither
 *      is one whose silence logits are -inf; one whose other logits are all -inf has log p_sil = 0 and is silent.  A +inf logit
 *      makes lse +inf or NaN: not silent.
 *
 *      state: (S, 8) int32 per slot {frames, trailing, speech, rule, end_frame, end_trailing, 0, 0}: frames absorbed since the
 *      slot was armed, the length of the silent run that ends at the last frame, the non-silent frames, and the latch: rule =
 *      -1 or the index of the rule that ended the utterance, end_frame the 0-based frame at which it did, end_trailing the
 *      silent run at that frame.  rules: (n_rules, 4) int32 rows {min_trailing, min_frames, min_speech, 0}, in frames.  After
 *      frame t is absorbed (frames = t + 1, trailing and speech updated) rule r HOLDS iff trailing >= min_trailing[r], frames
 *      >= min_frames[r] and speech >= min_speech[r]; while rule < 0 the first frame at which any rule holds is latched with the
 *      lowest such r.  A latched triple never changes again; the three counters go on counting.  A slot with k[b] = 0 is not
 *      touched at all; words 6 and 7 are never written.  The caller arms a slot by writing {0, 0, 0, -1, 0, 0, 0, 0}.
 *
 *      One workgroup of 1024 threads per slot: its 16 waves classify rows w, w + 16, ... into an LDS flag per row (V <= 512:
 *      the row read once into registers, the next row's loads in flight meanwhile; beyond: read twice), then wave 0 scans the
 *      flags 64 frames at a time (4 KiB of LDS: k_max <= 4096).  No allocation, no synchronisation: capturable.
 *
 *      Refused before any launch: a null logits (with k_max > 0), k, silence_ids, rules or state (CFM_ERR_NULL); S <= 0,
 *      k_max < 0, V < 2, n_silence outside [1, 8], n_rules outside [1, 4], ld_row < V, ld_slot < k_max ld_row, a NaN
 *      log_threshold (CFM_ERR_BAD_SHAPE); k_max > 4096, S >= 65535, V > 65536 (CFM_ERR_UNSUPPORTED).  k_max = 0 launches
 *      nothing and returns 0. */
int cfm_endpoint_step_f32(const float* logits, int64_t ld_slot, int64_t ld_row, const int64_t* k, int k_max, int V,
                          const int* silence_ids, int n_silence, float log_threshold, const int* rules, int n_rules,
                          int* state, int S, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
