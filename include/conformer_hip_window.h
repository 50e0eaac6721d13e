/*
 * conformer_hip_window.h -- extension of the C ABI of libconformer_hip.so (include/conformer_hip.h): bounded-history streaming.
 * Same conventions as the main header (device pointers, caller-owned buffers, launches enqueued on `stream`, 0 or a negative
 * cfm_status).  Not included by conformer_hip.h and no CFM_* define of its own: the entries here are ADDED to the library, so
 * CFM_ABI_VERSION does not move; a binding looks them up separately and asks for a rebuild when a library lacks them.
 */
#ifndef CONFORMER_HIP_WINDOW_H
#define CONFORMER_HIP_WINDOW_H

#include "conformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* windowed attention of independent streams over RING K/V caches (INTEGRATION.md "Bounded history (left_context)"; no reference
 *      counterpart: it is the reference's MultiHeadSelfAttentionModule under the mask (j >= chunk end) | (j < i - left)).
 *      q / k / v: the (B, R, .) ring with leading dimension ld; frame n of slot b lives in row n mod R.  Slot b computes the
 *      queries i = q_begin[b] + il, il < q_count[b], against the keys max(0, i - left) <= j < q_begin[b] + q_count[b], into the
 *      COMPACT ctx (B, q_max, ldo) rows 0 .. q_count[b]-1; rows q_count[b] .. q_max-1 are written as zeros and a slot with
 *      q_count[b] == 0 reads nothing.  pos: the projected table of 2P-1 rows, row P-1-r for the relative position r = i - j.
 *      q_begin (absolute frame index, any value < 2^62), q_count: device int64 (B), clamped on the device (q_begin to >= 0,
 *      q_count to [0, q_max]): no value makes an access outside the ring, the table or ctx.  Ring rows outside a query's window
 *      are never multiplied into a result, whatever bits they hold.
 *      R % 32 == 0, R >= left + q_max (no visible key was overwritten by this step's rows), P >= max(left + 1, q_max), left >= 0,
 *      q_max >= 1; pointers, alignment, dh and B*H as cfm_relpos_attention_slots_f32.  No key split: a workgroup walks only the
 *      key tiles that meet its rows' windows, at most (left + q_max)/32 + 1 of them wherever the stream stands. */
int cfm_relpos_attention_window_f32(const float* q, const float* k, const float* v, int64_t ld, const float* pos, int64_t ldp,
                                    int P, const float* u, const float* vbias, const int64_t* q_begin, const int64_t* q_count,
                                    float* ctx, int64_t ldo, int B, int R, int H, int dh, int q_max, int left,
                                    cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
