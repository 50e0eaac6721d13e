/*
 * conformer_hip3_vad.h -- third-generation entries of libconformer_hip.so: rule-based voice activity detection on the log-mel
 * frames of the audio front ends (INTEGRATION.md "Voice activity detection").  Same conventions as include/conformer_hip.h
 * (device pointers, caller-owned buffers, launches enqueued on `stream`, 0 or a negative cfm_status); the third generation is
 * open, see conformer_hip3_align_wild.h.
 *
 * Two entries, one launch each: cfm3_vad_energy_f32 turns mel frames into band energies, cfm3_vad_scan_f32 carries S
 * independent streams over those energies.  A step of a stream is the first followed by the second on the same k.
 *
 * THE DEFINITION.  Input: fp32 natural log of mel power, x[b][m][t] = mel[b * ld_slot + m * ld_mel + t] (frames contiguous);
 * slot b's new frames are the columns 0 .. k[b]-1, columns at or beyond k[b] are never read.  All times are in mel frames.
 * Per frame t, counted from when the slot was armed, with the band [m_lo, m_hi), smooth in [1, 16], noise_window Wn in
 * [1, 512], snr (nats), min_energy (nats, may be -inf), onset >= 1 and hangover >= 1:
 *
 *   1. Band energy: e_t = log sum_{m in band} exp(x[m][t]), computed in fp32 as M + log(sum_m exp(x[m][t] - M)), M the
 *      band's maximum, the sum taken in the order of m.  If e_t is not finite (NaN or +-inf) the frame is NOT SPEECH and is
 *      stored as +inf, so it can never lower the floor.  (A NaN bin, a band of -inf and a +inf bin all give such a frame.)
 *   2. Smoothed energy: s_t = the mean of the stored energies of the last min(smooth, t + 1) frames: summed oldest first in
 *      fp32, then divided by their number in fp32.
 *   3. Noise floor: f_t = min of s over the last min(Wn, t + 1) frames, the current one included: a trailing
 *      minimum-statistics tracker.  It is causal.
 *   4. Raw flag: raw_t = e_t finite && (e_t - f_t >= snr) && (e_t >= min_energy); a comparison with a NaN is false.
 *   5. State machine, with run_speech and run_silence the lengths of the runs of raw / not-raw frames that end at t:
 *      when not in speech and run_speech >= onset a segment OPENS at start = t - run_speech + 1; when in speech and
 *      run_silence >= hangover it CLOSES with the exclusive end = t - run_silence + 1.  A closed segment (start, end) is
 *      appended to the slot's rows of `segments` (max_segments, 2) int32 at row `count`, and count goes on counting past
 *      max_segments: the rows beyond it are not written.  (The host closes a segment still open at the end of a stream at
 *      frames - run_silence.)
 *   6. The state of a slot is (8) int32 {frames, run_speech, run_silence, in_speech, start, count, 0, 0} (start: of the open
 *      segment; words 6 and 7 are never written) and a ring of R = Wn + smooth - 1 floats: the stored energy of frame u lies
 *      at ring[u mod R].  How a stream is cut into steps changes NO BIT of any energy, flag, state word, ring word or
 *      segment: an energy depends on its column alone, s of an earlier frame is computed again from the ring by the same
 *      instructions, a minimum does not depend on its order.  A slot with k[b] = 0 is not touched.  The caller arms a slot
 *      by zeroing its state (the ring need not be cleared: frames before 0 are never read).
 *
 * Limits by construction: frames is an int32, so a slot has to be armed again within 2^31 frames; at most
 * T / (onset + hangover) + 1 segments close in T frames.
 */
#ifndef CONFORMER_HIP3_VAD_H
#define CONFORMER_HIP3_VAD_H

#include "../../include/conformer_hip.h"

#define CFM3_VAD_STATE_COLS 8
#define CFM3_VAD_SCAN_FRAMES 4096
#define CFM3_VAD_SMOOTH_MAX 16
#define CFM3_VAD_WINDOW_MAX 512
#define CFM3_VAD_BAND_MAX 128

#ifdef __cplusplus
extern "C" {
#endif

/* Step 1 for S slots: energy[b * ld_energy + t] = the stored energy of column t, t < k[b] (k: (S) int64, clamped to
 * [0, k_max]); nothing else of `energy` is written.  Grid over (frame tile of 256, slot), one lane per frame: a wave reads 64
 * consecutive frames of one mel row at a time and holds its column of the band in registers (read once).  k_max is not limited here.
 * Refused before any launch: a null mel (with k_max > 0), k or energy (CFM_ERR_NULL); S <= 0, k_max < 0, n_mel < 1, a band
 * that is not 0 <= m_lo < m_hi <= n_mel, ld_mel < k_max, ld_slot < n_mel ld_mel, ld_energy < k_max (CFM_ERR_BAD_SHAPE);
 * m_hi - m_lo > 128, S > 65535 (CFM_ERR_UNSUPPORTED).  k_max = 0 launches nothing and returns 0.  Capturable. */
int cfm3_vad_energy_f32(const float* mel, int64_t ld_slot, int64_t ld_mel, const int64_t* k, int k_max, int n_mel, int m_lo,
                        int m_hi, float* energy, int64_t ld_energy, int S, cfm_stream_t stream);

/* Steps 2 to 6 for S slots over the stored energies energy[b * ld_energy + t], t < k[b].  state (S, 8) int32, ring
 * (S, noise_window + smooth - 1) fp32, flags[b * ld_flags + t] = raw_t as a byte (t < k[b], nothing else is written),
 * segments (S, max_segments, 2) int32.  One workgroup of 1024 threads per slot: the ring and the new energies go to LDS, s is
 * computed per frame in parallel, the trailing minimum by log2(Wn) doubling passes and one combination of two overlapping
 * power-of-two windows, the flags by ballot into 64-bit words, and wave 0 runs the state machine over those words.
 * Refused before any launch: a null k, state, ring, flags, segments, or energy with k_max > 0 (CFM_ERR_NULL); S <= 0,
 * k_max < 0, smooth, noise_window, onset, hangover or max_segments < 1, ld_energy or ld_flags < k_max, a NaN snr or
 * min_energy (CFM_ERR_BAD_SHAPE); k_max > 4096, smooth > 16, noise_window > 512, onset, hangover or max_segments > 2^24,
 * S > 65535 (CFM_ERR_UNSUPPORTED).  k_max = 0 launches nothing and returns 0.  No allocation, no synchronisation:
 * capturable. */
int cfm3_vad_scan_f32(const float* energy, int64_t ld_energy, const int64_t* k, int k_max, int smooth, int noise_window,
                      float snr, float min_energy, int onset, int hangover, int* state, float* ring, unsigned char* flags,
                      int64_t ld_flags, int* segments, int max_segments, int S, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
