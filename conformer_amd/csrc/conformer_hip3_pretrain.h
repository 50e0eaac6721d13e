/*
 * conformer_hip3_pretrain.h -- third-generation entries of libconformer_hip.so: the objective of wav2vec 2.0-style
 * self-supervised pretraining (INTEGRATION.md "Self-supervised pretraining"): a Gumbel vector quantizer and a contrastive loss,
 * each with its backward.  Same conventions as include/conformer_hip.h (device pointers, caller-owned buffers, launches
 * enqueued on `stream`, 0 or a negative cfm_status); the third generation is open, see conformer_hip3_align_wild.h.  Every
 * argument is checked before the first HIP call.  No float atomics anywhere: every output element is written exactly once and
 * every sum has a fixed order, so two runs give the same bits.  All entries are capturable.
 *
 * THE QUANTIZER.  logits (N, G, V) fp32; noise (N, G, V) fp32 Gumbel values or null (the eval path); codevectors (G V, dg) fp32;
 * row_mask (N) uint8 or null (every row counts); tau > 0.  Per (row, g), with x = logits + noise (fp32; x = logits without noise):
 *   codes[row][g] = argmax_v x[v], the lowest index on a tie (a NaN is never chosen);  out[row][g dg : (g+1) dg] =
 *   codevectors[g V + code], a copy;  lse[row][g] = log sum_v exp(x[v] / tau) and the noise-free lse0 = log sum_v exp(logits[v])
 *   go to the workspace.
 *   marginal[g][v] = sum over the rows with row_mask set of softmax(logits[row][g])[v] (with noise), of the one-hot of the code
 *   (without).  Workgroups of CFM3_QUANT_ROWS rows leave partial sums; ONE workgroup adds them in the order of the rows.
 *   perplexity[0] = sum_g exp(-sum_v m[g][v] log(m[g][v] + 1e-7)), m = marginal / max(count of rows set, 1); so an empty mask
 *   gives m = 0 and perplexity = G, never a NaN.
 * The backward takes dout (N, G dg) and dperplexity (1) and needs noise (the eval path is not differentiable: CFM_ERR_NULL):
 *   dlogits[row][g][v] = (1 / tau) y[v] (gy[v] - <gy, y>)  +  [row counts] dperplexity p[v] (c[g][v] - <p, c[g]>)
 *   with y = exp(x / tau - lse), gy[v] = <codevectors[g V + v], dout[row][g]> (formed in the kernel, CFM3_QUANT_BWD_ROWS rows
 *   per workgroup against one read of the group's codebook), p = exp(logits - lse0) and
 *   c[g][v] = exp(H_g) (-log(m + 1e-7) - m / (m + 1e-7)) / max(count, 1), which the forward left in the workspace;
 *   dcodevectors[g V + v] = the sum, in the order of the rows, of dout[row][g] over the rows whose code is v: one workgroup per
 *   code scans codes; a code nobody chose gets an exact zero row.
 * The backward reads the workspace the forward left for the same logits, noise, row_mask and tau, untouched in between.
 * Workspace floats: lse (N G), lse0 (N G), c (G V), 4 (the count), partial marginals (ceil(N / CFM3_QUANT_ROWS), G, V), partial
 * counts (ceil(N / CFM3_QUANT_ROWS)).
 *
 * THE CONTRASTIVE LOSS.  context, targets (B, T, D) fp32; mask (B, T) uint8; negatives (B, T, K) int32, frame indices inside the
 * same utterance, an entry outside [0, T) is an ABSENT candidate; ids (B, T) int64 or null; temperature > 0.  For a masked
 * frame (b, t) the candidates are targets[b][t] (k = 0) and targets[b][negatives[b][t][k - 1]] (k = 1 .. K);
 *   z_k = cos(context[b][t], candidate_k) / temperature, cos(a, c) = <a, c> / max(|a| |c|, 1e-8);  a negative is EXCLUDED
 *   (z = -inf) when it is absent or when ids is given and its id equals the positive's;
 *   frame_loss[b][t] = logsumexp(z) - z_0 (0 when every negative is excluded), correct[b][t] = (argmax z == 0, lowest index on a
 *   tie);  an unmasked frame has frame_loss 0 and correct 0.  loss[0] = the sum of frame_loss in frame order and n_correct[0]
 *   the count, both stored by a final one-workgroup launch.
 * The workspace keeps the norms |context[b][t]| and |targets[b][t]| (B T each; the clamp is on their product, so the norms and
 * not their inverses are kept), p = softmax(z) and cos, (B, T, K + 1) each.  Nothing of B T K D elements exists.
 * The backward takes gframe (B, T) fp32 = d L / d frame_loss and the TRANSPOSED list of the draws: `order` (B T K) int64, the
 * flat positions (b T + t) K + k sorted stably by the frame drawn, b T + negatives[b][t][k], absent entries last; `start`
 * (B T + 1) int64, where each frame's entries begin.  With w_k = gframe (p_k - [k = 0]) / temperature:
 *   dcontext[b][t] = sum_k w_k d cos_k / d context, one workgroup per frame walking k in order, zeros for an unmasked frame;
 *   dtargets[b][j] = its own row as the positive (when masked) + its entries of the list in order, one wave per frame; a frame
 *   that is unmasked and never drawn gets exact zeros.  d cos / d a = c / den - [|a| |c| > 1e-8] cos a / |a|^2, den the
 *   clamped product.  An entry of `order` or `start` outside its range, or one that does not point at a draw of that frame, is
 *   skipped: no index derived from device data leaves a buffer.
 */
#ifndef CONFORMER_HIP3_PRETRAIN_H
#define CONFORMER_HIP3_PRETRAIN_H

#include "../../include/conformer_hip.h"

#define CFM3_PRETRAIN_MAX_V 1024
#define CFM3_PRETRAIN_MAX_G 8
#define CFM3_PRETRAIN_MAX_DG 512
#define CFM3_PRETRAIN_MAX_D 1024
#define CFM3_PRETRAIN_MAX_K 256
#define CFM3_QUANT_ROWS 32
#define CFM3_QUANT_BWD_ROWS 16
/* kernel launches each entry enqueues */
#define CFM3_QUANT_FWD_LAUNCHES 2
#define CFM3_QUANT_BWD_LAUNCHES 2
#define CFM3_CONTRASTIVE_FWD_LAUNCHES 3
#define CFM3_CONTRASTIVE_BWD_LAUNCHES 2

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace; -1 for a shape the entries refuse.  Host arithmetic only. */
int64_t cfm3_quantize_workspace_floats(int N, int G, int V);

/* Two launches: the rows (CFM3_QUANT_ROWS per workgroup, one workgroup column per group), then the one-workgroup reduction.
 * Refused before any launch: a null logits, codevectors, workspace, codes, out, marginal or perplexity (CFM_ERR_NULL); N, G, V or
 * dg < 1, tau not a positive finite number (CFM_ERR_BAD_SHAPE); V, G or dg above its CFM3_PRETRAIN_MAX_*, N G beyond 2^31 - 1
 * (CFM_ERR_UNSUPPORTED); a workspace that is not 16-byte aligned (CFM_ERR_ALIGN). */
int cfm3_quantize_fwd_f32(const float* logits, const float* noise, const float* codevectors, const uint8_t* row_mask, int N,
                          int G, int V, int dg, float tau, float* workspace, int* codes, float* out, float* marginal,
                          float* perplexity, cfm_stream_t stream);

/* Two launches: dlogits (CFM3_QUANT_BWD_ROWS rows per workgroup), dcodevectors (one workgroup per code).
 * Refused before any launch: as the forward, with noise, codes, dout, dperplexity, dlogits and dcodevectors required. */
int cfm3_quantize_bwd_f32(const float* logits, const float* noise, const float* codevectors, const uint8_t* row_mask,
                          const int* codes, const float* dout, const float* dperplexity, int N, int G, int V, int dg, float tau,
                          float* workspace, float* dlogits, float* dcodevectors, cfm_stream_t stream);

/* Floats of workspace; -1 for a shape the entries refuse.  Host arithmetic only. */
int64_t cfm3_contrastive_workspace_floats(int B, int T, int K);

/* Three launches: the norms (one wave per frame), the frames (one workgroup per frame, the context row staged in LDS, sixteen
 * candidates at a time), the sums.
 * Refused before any launch: a null context, targets, mask, negatives, workspace, frame_loss, correct, loss or n_correct
 * (CFM_ERR_NULL); B, T, D or K < 1, temperature not a positive finite number (CFM_ERR_BAD_SHAPE); D or K above its
 * CFM3_PRETRAIN_MAX_*, B T K beyond 2^31 - 1 (CFM_ERR_UNSUPPORTED); a workspace that is not 16-byte aligned, or, when D is a
 * multiple of 4 (rows are then read 16 bytes at a time), a context or targets that is not (CFM_ERR_ALIGN). */
int cfm3_contrastive_fwd_f32(const float* context, const float* targets, const uint8_t* mask, const int* negatives,
                             const int64_t* ids, int B, int T, int D, int K, float temperature, float* workspace,
                             float* frame_loss, uint8_t* correct, float* loss, int* n_correct, cfm_stream_t stream);

/* Two launches: dcontext (one workgroup per frame), dtargets (one wave per frame).
 * Refused before any launch: as the forward, with order, start, gframe, dcontext and dtargets in the place of ids and the
 * outputs; order and start 8-byte aligned (CFM_ERR_ALIGN). */
int cfm3_contrastive_bwd_f32(const float* context, const float* targets, const uint8_t* mask, const int* negatives,
                             const int64_t* order, const int64_t* start, const float* gframe, int B, int T, int D, int K,
                             float temperature, float* workspace, float* dcontext, float* dtargets, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
