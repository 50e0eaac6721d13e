/*
 * conformer_hip2_align_long.h -- second-generation entries of libconformer_hip.so: CTC forced alignment without a length
 * limit (INTEGRATION.md "Forced alignment", "Long form").  Same conventions as include/conformer_hip.h (device pointers,
 * caller-owned buffers, launches enqueued on `stream`, 0 or a negative cfm_status).
 *
 * Why this header lives beside the kernels and not under include/: the first-generation ABI (the headers under include/,
 * their cfm_* entries and CFM_* defines) is closed and counted.  Entry families added from now on are the second
 * generation: symbols cfm2_*, defines CFM2_*, one header per family in this directory, named in EXTRA_HEADERS of
 * conformer_amd/_lib.py.  They are ADDED to the library, so CFM_ABI_VERSION does not move; the binding looks them up after
 * the first generation and asks for a rebuild when a library lacks them.
 *
 * Semantics are those of cfm_ctc_align_f32 (conformer_hip.h): the lattice, the skip rule, raw logits, ties to the smaller
 * move, the end tie to state 2L, infeasible rows, the clamping of lengths and target ids, the same outputs and padding.
 * What differs is the chain: the lattice is cut into cells of `tile_pairs` (blank, label) state pairs x `chunk_frames`
 * frames, one workgroup per cell, cells of one anti-diagonal per launch; the state is float64 and is never re-centred, so
 * every value is the chain of IEEE double additions and comparisons of the float64 restatement, for any finite input.
 */
#ifndef CONFORMER_HIP2_ALIGN_LONG_H
#define CONFORMER_HIP2_ALIGN_LONG_H

#include "../../include/conformer_hip.h"

#define CFM2_CTC_ALIGN_LONG_MAX_FRAMES 1048576
#define CFM2_CTC_ALIGN_LONG_MAX_TARGET 262143

#ifdef __cplusplus
extern "C" {
#endif

/* tile_pairs: a multiple of 512 in [512, 8192]; chunk_frames: a multiple of 16 in [16, 65536]; 0 for either: the default,
 * which is the measured pair (tools/ctc_align_long_bench.py) cut down to the shape: tile_pairs no larger than Lmax + 1
 * rounded up to 512, chunk_frames no larger than T rounded up to 16.
 *      n_tiles = ceil((Lmax + 1) / tile_pairs), n_chunks = ceil(T / chunk_frames).
 *
 * Workspace, each part 16-byte aligned: frame_lp (B T doubles) | end_state + flags (2 B ints) | carry (B n_tiles
 * 2 tile_pairs doubles) | edge (B n_tiles T doubles) | moves (B T rows of n_tiles tile_pairs / 2 bytes).
 * Returns 0 for an unsupported shape: B, T or Lmax < 1, T > CFM2_CTC_ALIGN_LONG_MAX_FRAMES, Lmax >
 * CFM2_CTC_ALIGN_LONG_MAX_TARGET, B > 65535, or a tile_pairs / chunk_frames outside the above. */
size_t cfm2_ctc_align_long_workspace_bytes(int B, int T, int Lmax, int tile_pairs, int chunk_frames);

/* The number of chain launches, n_tiles + n_chunks - 1; 0 for an unsupported shape. */
int cfm2_ctc_align_long_launches(int T, int Lmax, int tile_pairs, int chunk_frames);

/* The arguments of cfm_ctc_align_f32 with tile_pairs, chunk_frames in front of the workspace; the same outputs.
 * Refused before any launch, in this order: a null pointer other than the two length arrays (CFM_ERR_NULL); B, T or Lmax
 * < 1, V < 2, blank_id outside [0, V) (CFM_ERR_BAD_SHAPE); a shape for which the workspace size is 0
 * (CFM_ERR_UNSUPPORTED); a workspace not 16-byte aligned (CFM_ERR_ALIGN); workspace_bytes below
 * cfm2_ctc_align_long_workspace_bytes (CFM_ERR_BAD_SHAPE).  No allocation, no synchronisation: capturable. */
int cfm2_ctc_align_long_f32(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                            const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax, int blank_id,
                            int tile_pairs, int chunk_frames, void* workspace, size_t workspace_bytes, int64_t* frame_tokens,
                            int64_t* frame_index, int64_t* token_start, int64_t* token_end, float* token_score, double* score,
                            unsigned char* ok, cfm_stream_t stream);

/* The chain stage alone (feasibility, the n_tiles + n_chunks - 1 cell launches, the end state) into the same workspace: what
 * tools/ctc_align_long_bench.py times apart from the whole call.  Same refusals as above for the arguments it has. */
int cfm2_ctc_align_long_chain_f32(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                                  const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax, int blank_id,
                                  int tile_pairs, int chunk_frames, void* workspace, size_t workspace_bytes,
                                  cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
