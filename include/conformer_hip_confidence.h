/*
 * conformer_hip_confidence.h -- extension of the C ABI of libconformer_hip.so (include/conformer_hip.h): token and word
 * confidence from the frame posteriors.  Same conventions as the main header (device pointers, caller-owned buffers, launches
 * enqueued on `stream`, 0 or a negative cfm_status).  Not included by conformer_hip.h: the entries here are ADDED to the
 * library, so CFM_ABI_VERSION does not move; a binding looks them up separately and asks for a rebuild when a library lacks
 * them.  The defines below name the values of `method` and `aggregation`.
 */
#ifndef CONFORMER_HIP_CONFIDENCE_H
#define CONFORMER_HIP_CONFIDENCE_H

#include "conformer_hip.h"

#define CFM_CONFIDENCE_MAX_PROB 0
#define CFM_CONFIDENCE_ENTROPY 1
#define CFM_CONFIDENCE_TSALLIS 2
#define CFM_CONFIDENCE_RENYI 3

#define CFM_CONFIDENCE_MEAN 0
#define CFM_CONFIDENCE_MIN 1
#define CFM_CONFIDENCE_MAX 2
#define CFM_CONFIDENCE_PROD 3

#ifdef __cplusplus
extern "C" {
#endif

/* Frame confidence (INTEGRATION.md "Confidence"): per frame one number in [0, 1], 0 for a uniform posterior and 1 for a one-hot
 * one, and the frame's argmax; two launches per call for S independent streams, or for the B utterances of an offline batch.
 *
 *      logits: fp32, addressed as in cfm_endpoint_step_f32: slot b's new frames are the rows logits[b * ld_slot + r * ld_row +
 *      0 .. V), r = 0 .. k[b]-1; rows at or beyond k[b] are never read.  k: (S) int64, clamped to [0, k_max].
 *
 *      conf (S, R) fp32, ids (S, R) int64 and total (S) int64 are a ring of the last R frames per slot: row r < k[b] of slot b
 *      is written at ring position (total[b] + r) mod R (total[b] read once, a negative one taken as 0), and total[b] then
 *      advances by the clamped k[b], once, in a second launch behind the first.  A slot with k[b] = 0 is not touched at all.
 *      The offline form is the same entry with total = 0, R = T and k = lengths: conf[b, t] is frame t.
 *
 *      Per frame x of V logits, in fp32: m = max_v x_v, s = sum_v exp(x_v - m), lse = m + log s, lp_v = x_v - lse, p_v =
 *      exp(lp_v), S_a = sum_v exp(alpha lp_v), and
 *          CFM_CONFIDENCE_MAX_PROB     (V exp(m - lse) - 1) / (V - 1)
 *          CFM_CONFIDENCE_ENTROPY      1 + (sum_v p_v lp_v) / ln V          (a term with p_v = 0 is 0: a -inf logit makes no NaN)
 *          CFM_CONFIDENCE_TSALLIS      1 - (S_a - 1) / (V^(1 - alpha) - 1)
 *          CFM_CONFIDENCE_RENYI        1 + ln S_a / ((alpha - 1) ln V)
 *      clamped to [0, 1] by comparisons that let a NaN through: a frame with a NaN logit gives NaN (so does one with a +inf
 *      logit, or with nothing but -inf).  The normalisers ln V, V^(1 - alpha) - 1 and (alpha - 1) ln V are computed once on the
 *      host in double and rounded to fp32.  alpha is ignored by the first two methods; for the other two it must lie in [1/16,
 *      15/16] or [17/16, 8]: nearer to 1 the normaliser cancels, and CFM_CONFIDENCE_ENTROPY is that limit.  ids gets the
 *      lowest index that attains the maximum (what cfm_greedy_ctc_decode_f32 writes to frame_ids), clamped to [0, V).
 *
 *      Lane l of a wave takes x_l, x_{l+64}, ... in that order, for the maximum, for s and for the method's sum, and the 64
 *      partials are folded by a fixed xor butterfly: a frame's value depends on its V logits alone, so how a stream is cut into
 *      steps changes no bit.  One wave per frame.  V <= 512: the row is read once into registers, the next row's loads in flight
 *      meanwhile, and a workgroup of 4 waves takes 16 consecutive rows of one slot, wave w the rows w, w + 4, ... of them (grid:
 *      ceil(k_max / 16) x S, so an offline call spreads an utterance's rows over many workgroups).  Beyond: the row is walked
 *      three times, 512 logits at a time (it stays in cache), and a workgroup takes 4 rows, one per wave (grid: ceil(k_max / 4)
 *      x S).  No allocation, no synchronisation: capturable.
 *
 *      Refused before any launch: a null logits (with k_max > 0), k, conf, ids or total (CFM_ERR_NULL); S <= 0, k_max < 0, R <
 *      1, k_max > R, V < 2, ld_row < V, ld_slot < k_max ld_row, a method outside the four, an alpha outside the two ranges
 *      with TSALLIS or RENYI (CFM_ERR_BAD_SHAPE); S >= 65535, V > 65536 (CFM_ERR_UNSUPPORTED).  k_max = 0 launches nothing and
 *      returns 0. */
int cfm_confidence_frames_f32(const float* logits, int64_t ld_slot, int64_t ld_row, const int64_t* k, int k_max, int V,
                              int method, float alpha, float* conf, int64_t* ids, int64_t* total, int R, int S,
                              cfm_stream_t stream);

/* Span aggregation: the confidence of a token or word from the frames it covers; one launch, one wave per span.
 *
 *      conf, ids (S, R) and total (S): the history the entry above keeps (frame t of slot b at ring position t mod R; a
 *      negative total taken as 0).  starts, ends (S, L) int64: absolute frames, end exclusive; n_spans (S) int64, clamped to
 *      [0, L].  out (S, L) fp32, every element written.
 *
 *      Span j of slot b is clamped to [0, total[b]].  out[b, j] is NaN for j >= n_spans[b], for an empty span (end <= start
 *      after the clamp) and for a span whose start has rolled out of the ring (start < total[b] - R).  Otherwise the frames
 *      that COUNT are those whose ids entry equals none of exclude_ids (n_exclude <= 8 int32, may be 0 with a null pointer); if
 *      that leaves none, all frames of the span count (a span that is all blank still has a value).  out[b, j] is their
 *          CFM_CONFIDENCE_MEAN     sum / count
 *          CFM_CONFIDENCE_MIN      minimum
 *          CFM_CONFIDENCE_MAX      maximum
 *          CFM_CONFIDENCE_PROD     product
 *      in fp32: lane l takes frames start + l, start + l + 64, ... in that order and the 64 partials are folded by the fixed
 *      xor butterfly.  A NaN frame anywhere in the span, counted or not, makes the span NaN under every aggregation.
 *
 *      Refused before any launch: a null conf, ids, total, starts, ends, n_spans or out, a null exclude_ids with n_exclude > 0
 *      (CFM_ERR_NULL); S <= 0, L < 0, R < 1, an aggregation outside the four, n_exclude outside [0, 8] (CFM_ERR_BAD_SHAPE); S L
 *      >= 2^31 (CFM_ERR_UNSUPPORTED).  L = 0 launches nothing and returns 0. */
int cfm_confidence_spans_f32(const float* conf, const int64_t* ids, const int64_t* total, int R, const int64_t* starts,
                             const int64_t* ends, const int64_t* n_spans, int L, int aggregation, const int* exclude_ids,
                             int n_exclude, float* out, int S, cfm_stream_t stream);

/* The spans of the greedy decoder's tokens: frame_ids (B, T) int64 as cfm_greedy_ctc_decode_f32 writes them; lengths_or_null
 * (B) int64 clamped to [0, T] (NULL: all T).  The decoder's collapse is replayed: frames whose id is pad_id or unk_id are
 * dropped, and a token is emitted at a kept frame whose id differs from the previous kept one.  token_start[b, j] is the frame at
 * which token j is emitted, token_end[b, j] = token_start[b, j + 1], the last token's end is the utterance's length; both (B, T)
 * int64, -1 from the number of tokens on.  So the number of spans is the decoder's counts[b] and frame_ids[b, token_start[b, j]]
 * its tokens[b, j].  One workgroup of one wave per row: 64 frames at a time, a ballot scan with the previous kept id carried.
 * Refused: a null frame_ids, token_start or token_end (CFM_ERR_NULL); B <= 0, T <= 0 (CFM_ERR_BAD_SHAPE). */
int cfm_confidence_greedy_spans_i64(const int64_t* frame_ids, const int64_t* lengths_or_null, int64_t* token_start,
                                    int64_t* token_end, int B, int T, int pad_id, int unk_id, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
