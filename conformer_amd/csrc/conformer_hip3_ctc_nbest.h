/*
 * conformer_hip3_ctc_nbest.h -- third-generation entries of libconformer_hip.so: the exact CTC log-likelihood of every
 * hypothesis of an n-best list against ONE block of logits per utterance, its gradient, and the minimum-word-error-rate
 * (MWER) risk over the list (INTEGRATION.md "MWER training and n-best scores").  Same conventions as include/conformer_hip.h
 * (device pointers, caller-owned buffers, launches enqueued on `stream`, 0 or a negative cfm_status); the third generation is
 * open, see conformer_hip3_align_wild.h.
 *
 * THE DEFINITION.  logits (B, T, V) fp32; hyps (B, N, Lmax) int64, row (b, n) holds hyp_len[b][n] labels and positions at or
 * behind that count are never read; hyp_len (B, N) int64; in_len (B) int64; `blank` in [0, V).  A row with hyp_len < 0 is
 * UNUSED.  Clamping is the loss's (cfm_ctc_loss_fwd_f32): in_len into [0, T], hyp_len into [0, Lmax], a label into [0, V), so
 * no index derived from device data leaves a buffer.  A count of 0 is the empty hypothesis (all blanks) and is a valid row.
 *
 *   ll[b][n] = log p(hyps[b][n] | logits[b]), the sum over all CTC alignments of the row to the first in_len[b] frames of
 *   log_softmax(logits[b]): what cfm_ctc_loss_fwd_f32 leaves as -nll for that (utterance, target), computed by the same chain
 *   (an fp32 lattice re-centred into float64 per-frame offsets).  -inf for a row without an alignment, an unused row, and
 *   in_len = 0 with a non-empty row; 0 for the empty row at zero frames.
 *
 *   dlogits[b][t][:] = sum_n w[b][n] * occupancy_n(t, :) - (sum_n w[b][n]) * softmax(logits[b][t])[:], over the rows n that are
 *   used, have a finite ll and a weight != 0: sum_n w[b][n] * d ll[b][n] / d logits.  Exact zeros at frames at or behind
 *   in_len[b] and for an utterance without such a row.
 *
 * The log-sum-exp and the blank log-probability are taken once per (b, t), the label log-probabilities once per (b, n, t, i);
 * the gradient is ONE pass over the frames in which a wave folds the N weighted occupancies of its frame into the row it
 * writes: every frame is written exactly once, without atomics, and two runs give the same bits.  Nothing of B N T V elements
 * exists: the workspace holds (B, N, T) lattice rows of 2 * 64 * P floats, P = the pairs per lane for Lmax.
 *
 * Workspace (floats, 8-byte aligned), as cfm3_ctc_nbest_workspace_floats counts it: float64 {ca (B N T), cb (B N T),
 * ll (B N)}, then fp32 {lse (B T), lpb (B T), lpl (B N T Lmax), alpha (B N T 2 64 P), beta (the same)}.  The score entry fills
 * everything but cb and beta; the gradient entry reads it and fills those, so the two calls share one workspace, untouched in
 * between, with the same logits, hyps, hyp_len and in_len.
 */
#ifndef CONFORMER_HIP3_CTC_NBEST_H
#define CONFORMER_HIP3_CTC_NBEST_H

#include "../../include/conformer_hip.h"

#define CFM3_CTC_NBEST_MAX 64

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace for a shape; -1 for a shape the entries refuse (B, N, T or Lmax < 1, N > CFM3_CTC_NBEST_MAX,
 * Lmax > CFM_CTC_MAX_TARGET, B T or B N beyond 2^31 - 1).  Host arithmetic only. */
int64_t cfm3_ctc_nbest_workspace_floats(int B, int N, int T, int Lmax);

/* ll (B, N) float64.  Two launches: prepare (one wave per frame), the alpha chains (one wave per (b, n)).
 * Refused before any launch: a null logits, hyps, hyp_len, in_len, workspace or ll (CFM_ERR_NULL); B, N, T, V or Lmax < 1,
 * blank outside [0, V) (CFM_ERR_BAD_SHAPE); N > CFM3_CTC_NBEST_MAX, Lmax > CFM_CTC_MAX_TARGET, B T or B N beyond 2^31 - 1
 * (CFM_ERR_UNSUPPORTED); a workspace or ll that is not 8-byte aligned (CFM_ERR_ALIGN).  Capturable. */
int cfm3_ctc_nbest_score_f32(const float* logits, const int64_t* hyps, const int64_t* hyp_len, const int64_t* in_len, int B,
                             int N, int T, int V, int Lmax, int blank, float* workspace, double* ll, cfm_stream_t stream);

/* dlogits (B, T, V) fp32 from weight (B, N) fp32 and the workspace cfm3_ctc_nbest_score_f32 left for the same inputs.  Two
 * launches: the beta chains of the rows that count, then one wave per frame.
 * Refused before any launch: as the score entry, with weight and dlogits in the place of ll (CFM_ERR_NULL), and
 * CFM_ERR_UNSUPPORTED when a frame's row and occupancies, (V + 2 * 64 * P) floats, exceed 64 KB of LDS.  Capturable. */
int cfm3_ctc_nbest_grad_f32(const float* logits, const int64_t* hyps, const int64_t* hyp_len, const int64_t* in_len, int B,
                            int N, int T, int V, int Lmax, int blank, float* workspace, const float* weight, float* dlogits,
                            cfm_stream_t stream);

/* The MWER risk of B lists.  Per utterance, over its LIVE rows (hyp_len >= 0 and a finite ll), all in float64:
 *   P_n = softmax of ll over the live rows, W_n = errors[b][n], R_b = sum_n P_n W_n, Wbar_b = the plain mean of W_n;
 *   risk[b] = R_b - Wbar_b;  weight[b][n] = grad_scale * P_n * (W_n - R_b) / B = grad_scale * d loss / d ll[b][n]
 * (Wbar_b is a constant: it centres the number reported and does not enter the gradient), and loss[0] = the mean of risk over
 * the batch.  An utterance with fewer than two live rows has risk 0 and zero weights; a row that is not live has weight 0.
 * One wave per utterance (lane n holds row n), then one wave for the mean: two launches.
 * Refused before any launch: a null pointer (CFM_ERR_NULL); B or N < 1 (CFM_ERR_BAD_SHAPE); N > CFM3_CTC_NBEST_MAX
 * (CFM_ERR_UNSUPPORTED); an ll that is not 8-byte aligned (CFM_ERR_ALIGN).  Capturable. */
int cfm3_mwer_risk_f32(const double* ll, const int* errors, const int64_t* hyp_len, int B, int N, float grad_scale,
                       float* risk, float* loss, float* weight, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
