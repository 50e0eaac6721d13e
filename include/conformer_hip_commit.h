/*
 * conformer_hip_commit.h -- extension of the C ABI of libconformer_hip.so (include/conformer_hip.h): committed-prefix streaming
 * search.  Same conventions as the main header (device pointers, caller-owned buffers, launches enqueued on `stream`, 0 or a
 * negative cfm_status).  Not included by conformer_hip.h and no CFM_* define of its own: the entries here are ADDED to the
 * library, so CFM_ABI_VERSION does not move; a binding looks them up separately and asks for a rebuild when a library lacks them.
 */
#ifndef CONFORMER_HIP_COMMIT_H
#define CONFORMER_HIP_COMMIT_H

#include "conformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Committed-prefix streaming search (INTEGRATION.md "Committed-prefix streaming (max_pending)"; no reference counterpart).
 *      A resumable search (cfm_ctc_beam_stream_*) whose prefix tree is re-rooted after every step at the prefix that can no
 *      longer change, so the tree holds T_tree = max_pending + max_chunk_frames frames however long the stream runs.
 *
 *      cfm_ctc_beam_commit_state_bytes: the stream state of cfm_ctc_beam_stream_state_bytes(B, T_tree, W, K, lm, hw) followed
 *      by the commit step's scratch.  0 for arguments out of range (B, W, K as there; max_pending < 1, max_chunk_frames < 1,
 *      T_tree * W >= 2^31).  No argument is a stream length.
 *      The state is initialised, reset per slot, stepped and finished by the cfm_ctc_beam_stream_* entries with T_max = T_tree
 *      (they accept the larger buffer); a step passes t_used = min(max_pending, frames stepped so far) and Tc <=
 *      max_chunk_frames.
 *
 *      cfm_ctc_beam_stream_commit: after a step.  Per utterance b, with the saved hypotheses y_0 .. y_{n-1} in rank order
 *      (token sequences relative to the committed prefix C): lcp = their longest common prefix, nb = max(lcp, |y_0| -
 *      max_pending); y_r survives iff it starts with y_0[:nb] and |y_r| - nb <= max_pending; the survivors keep their order and
 *      every saved value bit for bit; y_0[:nb] is appended to log[b, total[b] mod L ...] (int32 (B, L), a ring) and total[b]
 *      (int64) advances by nb; committed[b] (int32, optional) = nb.  The tree is rewritten as one private chain per survivor and
 *      the saved lengths, nodes and frame count become relative to the new C.  lengths_or_null: the step's `lengths`; an
 *      utterance that consumed no frame in the step (lengths[b] <= 0) is left as it is, with committed[b] = 0.
 *      L >= max_pending + max_chunk_frames (one call never laps the ring).  One launch; nothing synchronises with the host.
 *
 *      cfm_ctc_beam_commit_reset_slots: total[slots[i]] = 0 for i < n_slots (entries outside [0, B) are skipped). */
size_t cfm_ctc_beam_commit_state_bytes(int B, int max_pending, int max_chunk_frames, int W, int K, int lm, int hw);

int cfm_ctc_beam_stream_commit(int B, int max_pending, int max_chunk_frames, int beam_width, int max_candidates, int lm, int hw,
                               const int64_t* lengths_or_null, void* state, size_t state_bytes, int* log, int L, int64_t* total,
                               int* committed_or_null, cfm_stream_t stream);

int cfm_ctc_beam_commit_reset_slots(int B, const int64_t* slots, int n_slots, int64_t* total, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
