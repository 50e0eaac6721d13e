/*
 * conformer_hip3_rnnt.h -- third-generation entries of libconformer_hip.so: the transducer (RNN-T) loss over joint logits and
 * its gradient, the joint network's combine (tanh of a broadcast sum) forward and backward, and the bookkeeping of the
 * time-synchronous greedy decode (INTEGRATION.md "Transducer (RNN-T)").  Same conventions as include/conformer_hip.h (device
 * pointers, caller-owned buffers, launches enqueued on `stream`, 0 or a negative cfm_status); the third generation is open,
 * see conformer_hip3_align_wild.h.
 *
 * THE LOSS.  logits x (B, T, U1, V) fp32, U1 = Umax + 1; targets (B, U1 - 1) int64, padded (may be null when U1 == 1); in_len and
 * tg_len (B) int64; `blank` in [0, V).  Clamping is the CTC loss's (cfm_ctc_loss_fwd_f32): in_len into [0, T], tg_len into
 * [0, U1 - 1], a label into [0, V), so no index derived from device data leaves a buffer.  With T_b, U_b, y the clamped values,
 * lp = log_softmax(x, -1), lpb[t,u] = lp[t,u,blank] and lpl[t,u] = lp[t,u,y[u]] for u < U_b:
 *
 *   alpha[0,0] = 0;                      alpha[t,u] = logaddexp(alpha[t-1,u] + lpb[t-1,u], alpha[t,u-1] + lpl[t,u-1])
 *   beta[T_b-1,U_b] = lpb[T_b-1,U_b];    beta[t,u]  = logaddexp(beta[t+1,u] + lpb[t,u],    beta[t,u+1] + lpl[t,u])
 *   ll_b = alpha[T_b-1,U_b] + lpb[T_b-1,U_b] = beta[0,0];      nll_b = -ll_b
 *
 * a missing neighbour counting as -inf.  For a per-utterance weight w_b = d loss / d nll_b,
 *
 *   gamma = exp(alpha[t,u] + beta[t,u] - ll_b)
 *   eb    = exp(alpha[t,u] + lpb[t,u] + beta[t+1,u] - ll_b)     beta[T_b,U_b] read as 0, any other beta[T_b, .] as -inf
 *   el    = exp(alpha[t,u] + lpl[t,u] + beta[t,u+1] - ll_b)     0 at u = U_b
 *   dlogits[b,t,u,v] = w_b * (gamma * softmax(x[b,t,u])[v] - eb * [v == blank] - el * [v == y[u]])
 *
 * with exact zeros at t >= T_b or u > U_b (they are written: the buffer need not be cleared).  A label equal to `blank` is not
 * refused: both terms land on the same column.  An utterance with T_b = 0 is dead: nll = +inf, its weight is ignored and its
 * gradient is zero.
 *
 * alpha, beta and ll are float64; the two V-wide passes over the logits are fp32.  The forward reads x once (an online
 * max / sum per row, the blank's and the label's logit picked up on the way) and only the rows of the live lattice; the backward
 * reads x once and writes every element of dlogits exactly once, without atomics: two runs give the same bits.  V is arbitrary.
 * A logit of -inf is a column of probability 0.  A live row that is all -inf, holds +inf or holds a NaN has no finite lse: the
 * nll of its utterance is then not finite (NaN, or +inf), and the backward writes zeros for that utterance, whatever its weight.
 *
 * Workspace (floats, 8-byte aligned), as cfm3_rnnt_workspace_floats counts it, with n = B T U1: float64 {alpha (n), beta (n),
 * ll (B)}, then fp32 {lse (n), lpb (n), lpl (n)}: 2 (2 n + B) + 3 n floats.  The forward fills all of it (alpha and beta run
 * side by side); the backward reads it, so the two calls share one workspace, untouched in between, with the same inputs.
 *
 * THE JOINT.  e (B, Te, J) and p (B, U1, J) fp32: h[b,t,u,:] = tanh(e[b,t',:] + p[b,u,:]), (B, T, U1, J), where t' = t without
 * `frames` (then T <= Te) and t' = clamp(frames[b] + t, 0, Te - 1) with it (greedy decode: T = 1, one frame per utterance).
 * Backward, with g = dh (1 - h^2): de[b,t,j] = sum_u g, dp[b,u,j] = sum_t g, fixed summation orders, no atomics; h and dh are
 * each read twice.
 *
 * GREEDY DECODE.  Per utterance: t = 0, last = blank, the predictor state after consuming blank.  A decision takes
 * k = argmax_v logits[b,:] (the lowest index among equals).  If k != blank and fewer than max_symbols tokens were emitted at
 * this frame: tokens[b, count] = k, frames[b, count] = t, count += 1, last = k, emit = 1 (the caller's candidate state, advanced
 * by one step on k, becomes current).  Otherwise t += 1, the per-frame count returns to 0 and emit = 0.  An utterance with
 * t >= clamp(in_len[b], 0, T) is finished: nothing of it changes and emit = 0.  The capacity is T * max_symbols tokens per
 * utterance, which cannot overflow.
 */
#ifndef CONFORMER_HIP3_RNNT_H
#define CONFORMER_HIP3_RNNT_H

#include "../../include/conformer_hip.h"

#define CFM3_RNNT_MAX_U1 1024

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace for a shape; -1 for a shape the loss entries refuse (B, T or U1 < 1, U1 > CFM3_RNNT_MAX_U1, B T U1 beyond
 * 2^31 - 1).  Host arithmetic only. */
int64_t cfm3_rnnt_workspace_floats(int B, int T, int U1);

/* nll (B) float64.  Two launches: the rows (a wave or a part of one per live (b, t, u): lse, lpb, lpl), then the lattices (one
 * workgroup per utterance and direction, one lane per u, walking anti-diagonals).
 * Refused before any launch: a null logits, in_len, tg_len, workspace or nll, a null targets with U1 > 1 (CFM_ERR_NULL); B, T,
 * U1 or V < 1, blank outside [0, V) (CFM_ERR_BAD_SHAPE); U1 > CFM3_RNNT_MAX_U1, B T U1 beyond 2^31 - 1 (CFM_ERR_UNSUPPORTED); a
 * workspace or nll that is not 8-byte aligned (CFM_ERR_ALIGN).  Capturable. */
int cfm3_rnnt_loss_fwd_f32(const float* logits, const int64_t* targets, const int64_t* in_len, const int64_t* tg_len, int B, int T,
                           int U1, int V, int blank, float* workspace, double* nll, cfm_stream_t stream);

/* dlogits (B, T, U1, V) fp32 from weight (B) fp32 and the workspace cfm3_rnnt_loss_fwd_f32 left for the same inputs.  One launch.
 * Refused before any launch: as the forward, with weight and dlogits in the place of nll (CFM_ERR_NULL).  Capturable. */
int cfm3_rnnt_loss_bwd_f32(const float* logits, const int64_t* targets, const int64_t* in_len, const int64_t* tg_len, int B, int T,
                           int U1, int V, int blank, float* workspace, const float* weight, float* dlogits, cfm_stream_t stream);

/* h (B, T, U1, J).  frames: (B) int64 or null.  One launch.
 * Refused before any launch: a null e, p or h (CFM_ERR_NULL); B, Te, T, U1 or J < 1, T > Te without frames (CFM_ERR_BAD_SHAPE);
 * B T, B U1 or U1 J beyond 2^31 - 1 (CFM_ERR_UNSUPPORTED).  Capturable. */
int cfm3_rnnt_joint_fwd_f32(const float* e, const float* p, const int64_t* frames, float* h, int B, int Te, int T, int U1, int J,
                            cfm_stream_t stream);

/* de (B, T, J) and dp (B, U1, J) from h and dh (B, T, U1, J).  Two launches.
 * Refused before any launch: a null pointer (CFM_ERR_NULL); B, T, U1 or J < 1 (CFM_ERR_BAD_SHAPE); B T, B U1 or U1 J beyond
 * 2^31 - 1 (CFM_ERR_UNSUPPORTED).  Capturable. */
int cfm3_rnnt_joint_bwd_f32(const float* h, const float* dh, float* de, float* dp, int B, int T, int U1, int J, cfm_stream_t stream);

/* One decision per utterance from logits (B, V): see GREEDY DECODE.  tokens and frames (B, T max_symbols) int64; count, last, t
 * and nsym (the tokens emitted at the current frame) (B) int64; emit (B) int32.  t, count and nsym are clamped before use.  One
 * launch, one wave per utterance.
 * Refused before any launch: a null pointer (CFM_ERR_NULL); B, V, T or max_symbols < 1, blank outside [0, V)
 * (CFM_ERR_BAD_SHAPE); T max_symbols beyond 2^31 - 1 (CFM_ERR_UNSUPPORTED).  Capturable. */
int cfm3_rnnt_greedy_decide(const float* logits, const int64_t* in_len, int B, int V, int T, int blank, int max_symbols,
                            int64_t* tokens, int64_t* frames, int64_t* count, int64_t* last, int64_t* t, int64_t* nsym, int* emit,
                            cfm_stream_t stream);

/* Commit the candidate predictor state: planes (2 n_layers, B, H) fp32, state_new copied onto state_cur in the rows where emit is
 * set; active[0] = the utterances with t < clamp(in_len, 0, T), counted in a fixed order without atomics.  One launch.
 * Refused before any launch: a null pointer (CFM_ERR_NULL); planes, B, H or T < 1 (CFM_ERR_BAD_SHAPE).  Capturable. */
int cfm3_rnnt_greedy_commit(const float* state_new, float* state_cur, const int* emit, const int64_t* t, const int64_t* in_len,
                            int planes, int B, int H, int T, int* active, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
