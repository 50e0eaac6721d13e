/*
 * conformer_hip3_hotword_rows.h -- third-generation entries of libconformer_hip.so: the CTC prefix beam search with a hotword
 * list and a hotword weight PER UTTERANCE (INTEGRATION.md "Hotword boosting", "Per-request hotwords").  Same conventions as
 * include/conformer_hip.h (device pointers, caller-owned buffers, launches enqueued on `stream`, 0 or a negative cfm_status);
 * the third generation is open, see conformer_hip3_align_wild.h.
 *
 * THE DEFINITION.  Row b of every output equals, bit for bit, what cfm_ctc_beam_hw_decode_f32 (or the stream entries) returns
 * for utterance b alone with hw_tables = hw_row_tables[b] and hotword_weight = hw_row_weights[b] and everything else the same.
 * Nothing about the scoring changes: the search kernel reads the table pointer and the weight of its own utterance where the
 * first-generation entries pass one pair for the launch.
 *
 * `hw_row_tables`: (B) device pointers, DEVICE memory, each to a cfm_hotword_pack blob on the device (256-byte aligned, as the
 * packer lays it out).  Rows may share a blob.  A list without phrases is the blob cfm_hotword_pack writes for n_unigrams =
 * n_phrases = 0: header, two empty tries, the vocabulary token sections; a row with it equals the search without hotwords
 * bit for bit.  The header's own offsets and masks bound every access, so a blob that lies in a larger region is read up to its
 * own total_bytes and no further, whatever the rest of the region holds.
 * `hw_row_weights`: (B) doubles, DEVICE memory, every one finite (the host checks: the entries cannot).
 *
 * The largest blob a list can need: cfm_hotword_pack_bytes is monotone in uni_cp_total and phrase_word_total and does not
 * depend on n_unigrams, so for lists of at most P phrases and C code points in all (the characters of every word of every
 * phrase, spaces not counted) cfm_hotword_pack_bytes(n, C, P', n, V, tok_cp_total) with P' = min(P, C), n = min(8 P', C) is an
 * upper bound.  No new size entry is needed.
 *
 * The stream state is the first-generation one (cfm_ctc_beam_stream_state_bytes / cfm_ctc_beam_commit_state_bytes with hw = 1):
 * cfm_ctc_beam_stream_init, cfm_ctc_beam_stream_reset_slots, cfm_ctc_beam_stream_commit(_times), cfm_ctc_beam_commit_reset_slots
 * and cfm_ctc_beam_times_reset use `hw_tables` / `hw` as a mode flag only (they never read a table), so they serve this family
 * unchanged with any non-null `hw_tables`.  A hypothesis' saved trie node and window ids index ITS utterance's tables: an
 * utterance's table may change only while its search is at the empty prefix (after the init or a slot reset).
 */
#ifndef CONFORMER_HIP3_HOTWORD_ROWS_H
#define CONFORMER_HIP3_HOTWORD_ROWS_H

#include "../../include/conformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cfm_ctc_beam_hw_decode_f32 with per-row tables and weights; workspace: cfm_ctc_beam_hw_workspace_bytes(B, T, W, K).
 * Refused before any HIP call: a null logits, hw_row_tables, hw_row_weights, workspace, tokens, counts, scores, am_scores or
 * num_hyps (CFM_ERR_NULL); then the rules of cfm_ctc_beam_hw_decode_f32 in its order: B, T <= 0, V < 2 (CFM_ERR_BAD_SHAPE),
 * beam_width outside [1, 256], max_candidates outside [1, 32] (CFM_ERR_UNSUPPORTED), n_best outside [1, beam_width], blank_id
 * outside [0, V) (CFM_ERR_BAD_SHAPE), V > 2^23 or T beam_width >= 2^31 (CFM_ERR_UNSUPPORTED), a NaN knob, a non-finite alpha,
 * beta or unk_score_offset, workspace_bytes too small (CFM_ERR_BAD_SHAPE). */
int cfm3_ctc_beam_hw_rows_decode_f32(const float* logits, const int64_t* lengths_or_null, int B, int T, int V, int blank_id,
                                     int beam_width, int max_candidates, float token_min_logp, float beam_prune_logp, int n_best,
                                     const void* lm_tables_or_null, double alpha, double beta, double unk_score_offset,
                                     int score_boundary, const void* const* hw_row_tables, const double* hw_row_weights,
                                     void* workspace, size_t workspace_bytes, int64_t* tokens, int64_t* counts, float* scores,
                                     float* am_scores, int64_t* num_hyps, cfm_stream_t stream);

/* cfm_ctc_beam_stream_step_f32 with per-row tables and weights.  The times group (times, times_bytes, token_frames, token_logp)
 * is that of cfm_ctc_beam_stream_step_times_f32, or all null / 0: the step without timestamps.
 * Refused before any HIP call: a null logits, hw_row_tables, hw_row_weights, state, tokens, counts, scores or num_hyps, or a
 * times group that is neither whole nor absent (CFM_ERR_NULL); Tc <= 0 (CFM_ERR_BAD_SHAPE); the shape and range rules above on
 * (B, T_max, V, beam_width, max_candidates, n_best, blank_id, knobs); t_used outside [0, T_max] or Tc > T_max - t_used, a
 * non-finite alpha, beta or unk_score_offset, state_bytes or times_bytes too small (CFM_ERR_BAD_SHAPE). */
int cfm3_ctc_beam_hw_rows_stream_step_f32(const float* logits, const int64_t* lengths_or_null, int B, int Tc, int V,
                                          int blank_id, int beam_width, int max_candidates, float token_min_logp,
                                          float beam_prune_logp, int n_best, const void* lm_tables_or_null, double alpha,
                                          double beta, double unk_score_offset, int score_boundary,
                                          const void* const* hw_row_tables, const double* hw_row_weights, void* state,
                                          size_t state_bytes, int T_max, int t_used, int64_t* tokens, int64_t* counts,
                                          float* scores, float* am_scores_or_null, int64_t* num_hyps, void* times_or_null,
                                          size_t times_bytes, int64_t* token_frames_or_null, float* token_logp_or_null,
                                          cfm_stream_t stream);

/* cfm_ctc_beam_stream_finish_f32 with per-row tables and weights, the times group as above.
 * Refused before any HIP call: a null hw_row_tables, hw_row_weights, state, tokens, counts, scores, am_scores or num_hyps, or a
 * times group that is neither whole nor absent (CFM_ERR_NULL); the shape and range rules on (B, T_max, beam_width,
 * max_candidates, n_best); a non-finite alpha, beta or unk_score_offset, state_bytes or times_bytes too small
 * (CFM_ERR_BAD_SHAPE). */
int cfm3_ctc_beam_hw_rows_stream_finish_f32(int B, int beam_width, int max_candidates, int n_best,
                                            const void* lm_tables_or_null, double alpha, double beta, double unk_score_offset,
                                            int score_boundary, const void* const* hw_row_tables, const double* hw_row_weights,
                                            void* state, size_t state_bytes, int T_max, int64_t* tokens, int64_t* counts,
                                            float* scores, float* am_scores, int64_t* num_hyps, void* times_or_null,
                                            size_t times_bytes, int64_t* token_frames_or_null, float* token_logp_or_null,
                                            cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
