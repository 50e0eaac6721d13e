/*
 * conformer_hip3_kws.h -- third-generation entries of libconformer_hip.so: CTC keyword spotting (spoken-term detection) on the
 * fp32 logits of the acoustic model (INTEGRATION.md "Keyword spotting").  Same conventions as include/conformer_hip.h (device
 * pointers, caller-owned buffers, launches enqueued on `stream`, 0 or a negative cfm_status); the third generation is open, see
 * conformer_hip3_align_wild.h.
 *
 * Two entries, one launch each: cfm3_kws_rowmax_f32 takes the maximum of every new frame, cfm3_kws_scan_f32 carries the
 * keywords' Viterbi states and detectors of S independent streams over those frames.  A step of a stream is the first followed
 * by the second on the same k.
 *
 * THE DEFINITION.  Input: fp32 logits x[b][t][v] = x[b * ld_slot + t * ld_row + v]; slot b's new frames are the rows
 * 0 .. k[b]-1, rows at or beyond k[b] are never read.  K keywords; keyword q is L_q non-blank token ids, 1 <= L_q <= 32, with a
 * finite threshold thr_q <= 0.  All times are encoder frames counted from when the slot was armed.
 *
 *   States.  Keyword q has n = 2 L_q - 1 states, no leading and no trailing blank: an even state i is token i / 2, an odd one
 *   the blank between two tokens; label(i) is that token or the blank id.
 *
 *   Frame score.  m_t = the maximum of row t over v in [0, V), NaNs ignored (fmaxf).  If m_t is not finite (a row of NaN, a
 *   +inf entry, a row of -inf) frame t is a BREAK.  Otherwise r_t(i) = x[t][label(i)] - m_t, ONE fp32 subtraction: the
 *   log-likelihood ratio against the best symbol of the frame, <= 0 and exactly 0 where the label is the argmax.  A NaN entry
 *   gives r = -inf; on a BREAK every r = -inf.  No softmax: log_softmax(x)[v] - max log_softmax(x) is this same difference.
 *
 *   Viterbi with a free start.  Every state carries (a, start), fp32 and int32; armed it is (-inf, 0).  At frame t the
 *   candidates for state i are, in this order: 1. stay (a[i], start[i]); 2. advance from i - 1; 3. skip from i - 2, only for
 *   even i >= 2 whose token differs from token i / 2 - 1; 4. a fresh start (0.0f, t), only for i == 0.  A later candidate
 *   replaces the held one only if it is STRICTLY greater (the smaller move wins a tie, the fresh start loses every tie).  Then
 *   a'[i] = best + r_t(i), ONE fp32 add, and start'[i] is the winner's start.  All states update from the previous frame's
 *   values.
 *
 *   Hypothesis at frame t: (start'[n-1], t, e_t) with e_t = a'[n-1]; it QUALIFIES if e_t >= thr_q (false for a NaN).
 *
 *   Detector.  Each keyword holds at most one detection (start, end, score).  A qualifying frame, in this order: 1. if one is
 *   held and the hypothesis' start is greater than the held end, the held one is EMITTED and dropped; 2. if nothing is held, or
 *   e_t >= held.score, (start, t, e_t) is held (the later frame wins a tie).  A frame that does not qualify emits the held
 *   detection, if any, and drops it.  What is still held at the end of a stream is the host's to emit.
 *
 *   Chunking.  How a stream is cut into steps changes NO BIT of any state word or detection: the state is carried whole, a
 *   frame's arithmetic is one max chain, one subtraction and one add per state.
 *
 * Buffers.  `lanes` (G, 3, 64) int32: a GROUP is 64 lanes, a lane is a state, a keyword's states are consecutive lanes of one
 * group (so L <= 32).  Row 0: label(i) (the blank id for odd states; -1 for an idle lane; the kernel clamps a label to
 * [0, V)).  Row 1: the keyword's index (clamped to [0, K)).  Row 2: CFM3_KWS_FLAG_* bits.  `threshold` (K) fp32.  `state`
 * (S, G, CFM3_KWS_STATE_ROWS, 64) 32-bit words, per lane {a, start, held, held_start, held_end, held_score, frames (lane 0
 * only), 0}; the detector's words live in the lane of the keyword's last state, `held` is 0 or 1, and a detection that is
 * emitted and dropped clears `held` alone: held_start, held_end and held_score keep the values of the last detection held
 * (all 0 before the first).  The caller arms a slot by copying a template with a = -inf (NOT by zeroing).  `detections`
 * (S, G, max_detections, 4) int32 rows {keyword, start, end, score bits}, appended at row counts[b][g]; `counts` (S, G) int32
 * goes on counting past max_detections, the rows beyond it are not written.  Within a group emissions are in the order of the
 * frames, those of one frame in the order of the lanes.  A slot with k[b] = 0 is not touched at all.
 *
 * Limits by construction: frames is an int32, so a slot has to be armed again within 2^31 frames.
 */
#ifndef CONFORMER_HIP3_KWS_H
#define CONFORMER_HIP3_KWS_H

#include "../../include/conformer_hip.h"

#define CFM3_KWS_STATE_ROWS 8
#define CFM3_KWS_GROUP_LANES 64
#define CFM3_KWS_MAX_TOKENS 32
#define CFM3_KWS_RING_FRAMES 8
#define CFM3_KWS_FLAG_FIRST 1
#define CFM3_KWS_FLAG_SKIP 2
#define CFM3_KWS_FLAG_LAST 4
#define CFM3_KWS_V_MAX 65536

#ifdef __cplusplus
extern "C" {
#endif

/* m_t for S slots: rowmax[b * ld_rowmax + t] = the maximum of row t of slot b, NaN for a BREAK frame, t < k[b] (k: (S) int64,
 * clamped to [0, k_max]); nothing else of `rowmax` is written.  One wave per row, lanes along v (coalesced), a shuffle
 * reduction; grid over (4 rows, slot).  k_max is not limited here.
 * Refused before any launch: a null k or rowmax, or x with k_max > 0 (CFM_ERR_NULL); S <= 0, k_max < 0, V < 2, ld_row < V,
 * ld_slot < k_max ld_row, ld_rowmax < k_max (CFM_ERR_BAD_SHAPE); V > 65536, S > 65535 (CFM_ERR_UNSUPPORTED).  k_max = 0
 * launches nothing and returns 0.  Capturable. */
int cfm3_kws_rowmax_f32(const float* x, int64_t ld_slot, int64_t ld_row, const int64_t* k, int k_max, int V, float* rowmax,
                        int64_t ld_rowmax, int S, cfm_stream_t stream);

/* The Viterbi step and the detector of every keyword over the rows t < k[b] of S slots, with m_t from rowmax[b * ld_rowmax + t].
 * One wave per (group, slot), grid (G, S): a lane holds its state in registers, the neighbour states i - 1 and i - 2 come by
 * lane shifts gated by the lane's own flags (nothing leaks across the keywords that share a wave), the wave walks the slot's
 * frames alone (no barrier) with the gathers x[t][label(lane)] of the next CFM3_KWS_RING_FRAMES frames in flight (two register
 * blocks of that many frames, filled in turn), and the emissions of a frame are placed by a ballot and a prefix count (no atomics).
 * Refused before any launch: a null k, lanes, threshold, state, detections or counts, or x or rowmax with k_max > 0
 * (CFM_ERR_NULL); S <= 0, k_max < 0, V < 2, G < 1, K < 1, K > 64 G, max_detections < 1, ld_row < V, ld_slot < k_max ld_row,
 * ld_rowmax < k_max (CFM_ERR_BAD_SHAPE); V > 65536, S > 65535, G > 2^20, max_detections > 2^24 (CFM_ERR_UNSUPPORTED).
 * k_max = 0 launches nothing and returns 0.  No allocation, no synchronisation: capturable. */
int cfm3_kws_scan_f32(const float* x, int64_t ld_slot, int64_t ld_row, const float* rowmax, int64_t ld_rowmax, const int64_t* k,
                      int k_max, int V, const int* lanes, const float* threshold, int G, int K, int* state, int* detections,
                      int max_detections, int* counts, int S, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
