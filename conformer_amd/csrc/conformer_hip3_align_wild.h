/*
 * conformer_hip3_align_wild.h -- third-generation entries of libconformer_hip.so: CTC forced alignment with wildcard
 * ("star") target positions, for transcripts that skip audio (INTEGRATION.md "Forced alignment", "Wildcards").  Same
 * conventions as include/conformer_hip.h (device pointers, caller-owned buffers, launches enqueued on `stream`, 0 or a
 * negative cfm_status).
 *
 * The third generation is OPEN: symbols cfm3_*, defines CFM3_*, one header per family in this directory named
 * conformer_hip3_<family>.h.  conformer_amd/_lib.py discovers these headers from the directory (OPEN_HEADERS), so a new
 * family is its header and its definitions and nothing else.  The entries are ADDED to the library: CFM_ABI_VERSION does
 * not move, the binding looks them up after the second generation and asks for a rebuild when a library lacks one.
 *
 * Semantics.  A target position inside target_lengths whose value is CFM3_CTC_ALIGN_WILDCARD is a wildcard: a label that
 * emits, at frame t,
 *      w[b,t] = (float)(max over v in [0,V) of x[b,t,v]) - wildcard_penalty        (one fp32 subtraction, blank included)
 * The path is BY DEFINITION the one cfm_ctc_align_f32 (cfm2_ctc_align_long_f32 for the long form) finds on the logits
 * with w appended as column V and every wildcard replaced by the id V; that tensor is never built.  So a wildcard differs
 * from every label (it may be skipped into and out of), two adjacent wildcards are a repeated label (a blank between
 * them, counted in T >= L + repeats), a wildcard takes at least one frame, ties go to the smaller move and the end tie to
 * state 2L.  Every other target value is clamped to [0,V) as ever, and positions beyond target_lengths are never read.
 *
 * Outputs: those of cfm_ctc_align_f32.  At a wildcard's frames frame_tokens is CFM3_CTC_ALIGN_WILDCARD and frame_index
 * its target position; token_start / token_end are its run; token_score is the mean over the run of
 * max_v log_softmax(x[t])[v] (normalised over the V real columns, the penalty NOT included) and score adds that same
 * quantity at those frames.  Without a wildcard inside target_lengths every output equals, bit for bit, that of the entry
 * the form extends, for any penalty.
 */
#ifndef CONFORMER_HIP3_ALIGN_WILD_H
#define CONFORMER_HIP3_ALIGN_WILD_H

#include "../../include/conformer_hip.h"

#define CFM3_CTC_ALIGN_WILDCARD -2

#ifdef __cplusplus
extern "C" {
#endif

/* The workspace of cfm_ctc_align_workspace_bytes rounded up to 16 bytes | w (B T floats, rounded up to 16 bytes).
 * 0 for the shapes cfm_ctc_align_workspace_bytes gives 0 for. */
size_t cfm3_ctc_align_wild_workspace_bytes(int B, int T, int Lmax);

/* The arguments of cfm_ctc_align_f32 with wildcard_penalty (logit units per wildcard frame, finite, >= 0) after blank_id;
 * the same limits.  Refused before any launch, in this order: a null pointer other than the two length arrays
 * (CFM_ERR_NULL); B, T or Lmax < 1, V < 2, blank_id outside [0, V), a negative or non-finite wildcard_penalty
 * (CFM_ERR_BAD_SHAPE); T or Lmax beyond the limits (CFM_ERR_UNSUPPORTED); a workspace not 16-byte aligned
 * (CFM_ERR_ALIGN); workspace_bytes below cfm3_ctc_align_wild_workspace_bytes (CFM_ERR_BAD_SHAPE).  No allocation, no
 * synchronisation: capturable. */
int cfm3_ctc_align_wild_f32(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                            const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax, int blank_id,
                            float wildcard_penalty, void* workspace, size_t workspace_bytes, int64_t* frame_tokens,
                            int64_t* frame_index, int64_t* token_start, int64_t* token_end, float* token_score, double* score,
                            unsigned char* ok, cfm_stream_t stream);

/* The workspace of cfm2_ctc_align_long_workspace_bytes | w (B T floats, rounded up to 16 bytes); 0 where that is 0. */
size_t cfm3_ctc_align_long_wild_workspace_bytes(int B, int T, int Lmax, int tile_pairs, int chunk_frames);

/* The arguments of cfm2_ctc_align_long_f32 with wildcard_penalty after blank_id; the same limits and tilings, the same
 * refusals in the same order, a negative or non-finite wildcard_penalty among the CFM_ERR_BAD_SHAPE of the second place.
 * The state is float64 on (double)x and (double)w, never re-centred: the path is exact for any finite logits. */
int cfm3_ctc_align_long_wild_f32(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                                 const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax, int blank_id,
                                 float wildcard_penalty, int tile_pairs, int chunk_frames, void* workspace,
                                 size_t workspace_bytes, int64_t* frame_tokens, int64_t* frame_index, int64_t* token_start,
                                 int64_t* token_end, float* token_score, double* score, unsigned char* ok, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
