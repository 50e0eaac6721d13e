/*
 * conformer_hip_error_rate.h -- extension of the C ABI of libconformer_hip.so (include/conformer_hip.h): word, character and
 * token error counts on the device.  Same conventions as the main header (device pointers, caller-owned buffers, launches
 * enqueued on `stream`, 0 or a negative cfm_status).  Not included by conformer_hip.h and no CFM_* define of its own: the
 * entries here are ADDED to the library, so CFM_ABI_VERSION does not move; a binding looks them up separately and asks for a
 * rebuild when a library lacks them.
 *
 * The cap: 16384 units per side and kind.  It bounds the leading dimensions below, which the host knows before any launch.
 */
#ifndef CONFORMER_HIP_ERROR_RATE_H
#define CONFORMER_HIP_ERROR_RATE_H

#include "conformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Unit extraction (INTEGRATION.md "Error rates on the device"): one launch turns R token rows into their three unit streams.
 * ids: int64, row r is ids[r * ld_ids + 0 .. counts[r]), counts (R) int64 clamped to [0, L]; positions at or behind the count
 * are never read.  The vocabulary: tok_kind (V) int32 (0 characters, 1 delimiter, 2 skip), tok_off (V + 1) int32 and tok_cp: the
 * code points of token v are tok_cp[tok_off[v] .. tok_off[v + 1]) (none unless its kind is 0); max_token_cps is the longest such
 * run (the host's statement: a longer token is cut at the end of the row's buffer, never written behind it).  An id outside
 * [0, V) in front of the count is treated as a skip token.
 *
 *      toks  (R, ld_toks) int32: the ids whose kind is not skip, in order (delimiters included).
 *      cps   (R, ld_cps)  int32: the code points of the row's text: the tokens of kind 0 spell their code points; between two
 *            spelling tokens that have at least one delimiter between them stands exactly one U+0020; nothing stands in front
 *            of the first or behind the last.  A token of kind 0 without code points spells nothing and separates nothing.
 *      words (R, ld_words, 4) int32 {start, length, hash, 0}: the maximal runs of cps without U+0020 as spans into the row's
 *            cps, with a 32-bit FNV-1a hash of the span's code points.
 *      lens  (R, 4) int32 {code points, words, tokens, 0}.
 *      Elements of cps, words and toks at or behind the row's lengths are not written.
 *
 *      One workgroup of 256 threads per row walks the row 256 tokens at a time with two block scans (the last spelling token
 *      and the last delimiter in front of each token; then the offsets of its code points, word and token), then hashes the
 *      words, one thread per word.  No allocation, no synchronisation: capturable.
 *
 *      Refused before any launch: a null pointer (tok_cp may be null when no token has code points) (CFM_ERR_NULL); R, L or V
 *      <= 0, max_token_cps < 0, ld_ids < L, ld_toks < L, ld_words < L, ld_cps < L max(max_token_cps, 1) (CFM_ERR_BAD_SHAPE);
 *      L max(max_token_cps, 1) > 16384 or R > 2^31 - 1 workgroups (CFM_ERR_UNSUPPORTED). */
int cfm_error_rate_units(const int64_t* ids, int64_t ld_ids, const int64_t* counts, int R, int L, const int* tok_kind,
                         const int* tok_off, const int* tok_cp, int V, int max_token_cps, int* cps, int64_t ld_cps, int* words,
                         int64_t ld_words, int* toks, int64_t ld_toks, int* lens, cfm_stream_t stream);

/* Batched edit distance: reference row b against the hypothesis rows b * N + n, n = 0 .. N-1, on the streams that
 * cfm_error_rate_units wrote (the ref_* buffers hold B rows, the hyp_* buffers B N rows; every length read from ref_lens /
 * hyp_lens is clamped to [0, its leading dimension]).  unit: 0 words, 1 characters (code points), 2 tokens, 3 all three.
 *
 *      errors[b * N + n] = the Levenshtein distance (insertion, deletion and substitution cost 1 each) between the two unit
 *      sequences; two words are equal iff their lengths and all their code points are equal (the hash only rejects); a word
 *      whose span does not lie inside its row's cps equals nothing.  hyp_units[b * N + n] and ref_units[b] are the two
 *      lengths.  A hypothesis row without units (an unused n-best row) scores the reference's length.  unit = 3: errors and
 *      hyp_units hold three (B, N) planes and ref_units three (B) planes, in the order words, characters, tokens.  The
 *      result depends on the two unit sequences alone.
 *
 *      One workgroup of one wave per (n, b, kind).  Lane l owns 8 consecutive hypothesis columns of a 512-column strip and
 *      takes reference row s - l at step s, so the wave sweeps an anti-diagonal band: the value to the left of a lane's first
 *      column comes from lane l - 1 by a lane shift, the reference unit travels down the lanes the same way, and nothing
 *      waits on a barrier inside a strip.  Hypotheses longer than 512 units take further strips; the last column of a strip
 *      is handed to the next through LDS (4 bytes per reference unit, at most 64 KiB).  No workspace: the rolling state is 8
 *      registers per lane.  No allocation, no synchronisation: capturable.
 *
 *      Refused before any launch: a null pointer among those the kind uses, errors, hyp_units, ref_units, ref_lens, hyp_lens
 *      (CFM_ERR_NULL); B or N <= 0, unit outside [0, 3], a leading dimension of a used kind <= 0 (CFM_ERR_BAD_SHAPE); a
 *      leading dimension of a used kind > 16384, N > 65535 or B > 65535 (CFM_ERR_UNSUPPORTED). */
int cfm_error_rate_distance(const int* ref_cps, int64_t ld_ref_cps, const int* ref_words, int64_t ld_ref_words,
                            const int* ref_toks, int64_t ld_ref_toks, const int* ref_lens, const int* hyp_cps,
                            int64_t ld_hyp_cps, const int* hyp_words, int64_t ld_hyp_words, const int* hyp_toks,
                            int64_t ld_hyp_toks, const int* hyp_lens, int B, int N, int unit, int* errors, int* hyp_units,
                            int* ref_units, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
