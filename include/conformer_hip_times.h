/*
 * conformer_hip_times.h -- extension of the C ABI of libconformer_hip.so (include/conformer_hip.h): token timestamps from the
 * resumable CTC beam search.  Same conventions as the main header (device pointers, caller-owned buffers, launches enqueued on
 * `stream`, 0 or a negative cfm_status).  Not included by conformer_hip.h and no CFM_* define of its own: the entries here are
 * ADDED to the library, so CFM_ABI_VERSION does not move; a binding looks them up separately and asks for a rebuild when a
 * library lacks them.
 */
#ifndef CONFORMER_HIP_TIMES_H
#define CONFORMER_HIP_TIMES_H

#include "conformer_hip_commit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Beam-search timestamps (INTEGRATION.md "Beam-search timestamps"; the convention of pyctcdecode's text_frames).
 *      Every token i of a returned hypothesis y gets frame[i], the absolute logit frame (from 0 at the utterance's opening) at
 *      which y[:i+1] entered the live set on the lineage that survived, and logp[i] = log_softmax(logits[frame[i]])[y[i]], the
 *      fp64 value the search added for that extension, rounded to fp32.  Frames are int32 inside the buffer and int64 in every
 *      output: an utterance of 2^31 frames or more is out of range.
 *
 *      The values live in a `times` buffer the caller owns BESIDE the stream state (the state's layout and
 *      cfm_ctc_beam_stream_state_bytes / cfm_ctc_beam_commit_state_bytes do not change).  cfm_ctc_beam_times_bytes: its size for
 *      a tree of T frames (T_max of cfm_ctc_beam_stream_*; in commit mode T_tree = max_pending + max_chunk_frames) and beam
 *      width W; max_pending_or_0 > 0 adds the commit step's scratch.  0 for arguments out of range (B < 1, T < 1, W outside
 *      [1, 256], T * W >= 2^31, max_pending_or_0 < 0 or >= T when not 0).
 *
 *      cfm_ctc_beam_times_reset: the frame counts of every utterance (slots_or_null null, n_slots 0) or of slots[0 .. n_slots)
 *      (entries outside [0, B) are skipped) back at 0.  Call it where cfm_ctc_beam_stream_init / _reset_slots are called.
 *
 *      cfm_ctc_beam_stream_step_times_f32 / cfm_ctc_beam_stream_finish_times_f32: cfm_ctc_beam_stream_step_f32 /
 *      cfm_ctc_beam_stream_finish_f32 with the same arguments, then the times buffer and token_frames (B, n_best, T_max) int64
 *      padded with -1, token_logp (B, n_best, T_max) fp32 padded with -inf, parallel to `tokens`.  Every other output is bit
 *      for bit the one of the plain entry.  A stream is stepped with the *_times entries from its opening on or not at all.
 *
 *      cfm_ctc_beam_stream_commit_times: cfm_ctc_beam_stream_commit with the same arguments, then the times buffer (sized with
 *      max_pending) and the rings log_frames (B, L) int64, log_logp (B, L) fp32: the values of the committed tokens at the
 *      positions `log` takes.  The survivors keep their values; an utterance with lengths[b] <= 0 is left as it is.
 *
 *      Null pointers and short buffers are refused before any launch. */
size_t cfm_ctc_beam_times_bytes(int B, int T, int W, int max_pending_or_0);

int cfm_ctc_beam_times_reset(int B, const int64_t* slots_or_null, int n_slots, void* times, size_t times_bytes,
                             cfm_stream_t stream);

int cfm_ctc_beam_stream_step_times_f32(const float* logits, const int64_t* lengths_or_null, int B, int Tc, int V, int blank_id,
                                       int beam_width, int max_candidates, float token_min_logp, float beam_prune_logp, int n_best,
                                       const void* lm_tables_or_null, double alpha, double beta, double unk_score_offset,
                                       int score_boundary, const void* hw_tables_or_null, double hotword_weight, void* state,
                                       size_t state_bytes, int T_max, int t_used, int64_t* tokens, int64_t* counts, float* scores,
                                       float* am_scores_or_null, int64_t* num_hyps, void* times, size_t times_bytes,
                                       int64_t* token_frames, float* token_logp, cfm_stream_t stream);

int cfm_ctc_beam_stream_finish_times_f32(int B, int beam_width, int max_candidates, int n_best, const void* lm_tables_or_null,
                                         double alpha, double beta, double unk_score_offset, int score_boundary,
                                         const void* hw_tables_or_null, double hotword_weight, void* state, size_t state_bytes,
                                         int T_max, int64_t* tokens, int64_t* counts, float* scores, float* am_scores_or_null,
                                         int64_t* num_hyps, void* times, size_t times_bytes, int64_t* token_frames,
                                         float* token_logp, cfm_stream_t stream);

int cfm_ctc_beam_stream_commit_times(int B, int max_pending, int max_chunk_frames, int beam_width, int max_candidates, int lm,
                                     int hw, const int64_t* lengths_or_null, void* state, size_t state_bytes, int* log, int L,
                                     int64_t* total, int* committed_or_null, void* times, size_t times_bytes, int64_t* log_frames,
                                     float* log_logp, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
