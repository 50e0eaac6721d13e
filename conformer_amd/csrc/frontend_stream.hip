// Streaming audio front end (INTEGRATION.md "Streaming audio front end"): the staging step that turns waveform chunks into
// the padded-wave layout cfm_dft_frames_f32 and cfm_power_mel_log_mfma_f32 take (frontend.hip, gemm_f32.hip: unchanged).
//
// Every slot carries the last samples of its stream that a later frame still needs (the tail, < n_fft of them).  Per step the
// host works out, from the per-slot sample counts alone, which frames become computable and hands the kernel one int32 row per
// slot.  With cat = [tail | new samples] (m = tail_len + n_new values) the row says
//     segment[i] = cat[r(i - lead + off)],  0 <= i < (n_frames - 1) hop + n_fft,
//     r(c) = -c below 0 (the utterance's opening reflected: only while the tail still starts at sample 0),
//            2 (m - 1) - c from m on (its end reflected: a flush step)
//     new tail[j] = cat[keep + j],  0 <= j < new_tail_len
// so the device sees offsets relative to the tail and never a position in the stream.  The segment goes to xp + b rpu hop, rpu =
// f_max + ceil(n_fft / hop); the rest of the slot's pitch and the n_fft floats behind the last slot are written as 0, so the
// junk frames of the overlapping-rows GEMM read defined memory.  The tails ping-pong between two buffers: this launch reads
// tail_in and the samples and writes tail_out and xp, nothing it reads is written by it.
// Every table value is clamped before it indexes anything: a corrupt table cannot make a read or a write leave the buffers.
#include "cfm_common.h"
#include "../../include/conformer_hip_stream_frontend.h"

namespace {

constexpr int TAIL_LD = 512, COLS = 8;               // floats per tail row, int32 per table row (the header states both)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct SlotRow {
    int tail_len, n_new, m, shift, seg_len, keep, new_tail_len;
};

__device__ __forceinline__ SlotRow read_row(const int* __restrict__ row, int n_max, int f_max, int hop, int n_fft) {
    SlotRow r;
    r.tail_len = clampi(row[0], 0, TAIL_LD);
    r.n_new = clampi(row[1], 0, n_max);
    r.m = r.tail_len + r.n_new;
    const int lead = clampi(row[2], 0, n_fft), off = clampi(row[5], 0, TAIL_LD);
    r.shift = off - lead;
    const int nf = r.m > 0 ? clampi(row[3], 0, f_max) : 0;
    r.seg_len = nf > 0 ? (nf - 1) * hop + n_fft : 0;
    r.keep = clampi(row[6], 0, r.m);
    r.new_tail_len = row[4] ? 0 : clampi(row[7], 0, min(TAIL_LD, r.m - r.keep));
    return r;
}

// cat[c], 0 <= c < m
__device__ __forceinline__ float cat_at(const float* __restrict__ tail, const float* __restrict__ fresh, const SlotRow& r, int c) {
    return c < r.tail_len ? tail[c] : fresh[c - r.tail_len];
}

// grid (ceil(pitch / 1024), S + 1): a thread writes four consecutive floats of slot blockIdx.y's pitch with one 16-byte store
// (gathered with four 4-byte loads: the tail offset is arbitrary); row S is the slack behind the last slot; block 0 of a slot
// also writes its new tail, all TAIL_LD floats of it (zeros behind new_tail_len).
__global__ __launch_bounds__(256) void stream_stage_kernel(const float* __restrict__ samples, int64_t ld_samples, int n_max,
                                                           const float* __restrict__ tail_in, float* __restrict__ tail_out,
                                                           const int* __restrict__ table, float* __restrict__ xp, int S, int f_max,
                                                           int hop, int n_fft, int pitch) {
    const int b = blockIdx.y;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (b == S) {
        if (i0 < n_fft) *reinterpret_cast<f32x4*>(xp + (int64_t)S * pitch + i0) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const SlotRow r = read_row(table + (int64_t)b * COLS, n_max, f_max, hop, n_fft);
    const float* tail = tail_in + (int64_t)b * TAIL_LD;
    const float* fresh = samples + (int64_t)b * ld_samples;
    if (i0 < pitch) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i0 + e;
            float x = 0.f;
            if (i < r.seg_len) {
                int c = i + r.shift;
                c = c < 0 ? -c : c;
                c = c >= r.m ? 2 * (r.m - 1) - c : c;
                x = cat_at(tail, fresh, r, clampi(c, 0, r.m - 1));
            }
            v[e] = x;
        }
        *reinterpret_cast<f32x4*>(xp + (int64_t)b * pitch + i0) = v;
    }
    if (blockIdx.x == 0) {
        for (int j = threadIdx.x; j < TAIL_LD; j += 256)
            tail_out[(int64_t)b * TAIL_LD + j] = j < r.new_tail_len ? cat_at(tail, fresh, r, r.keep + j) : 0.f;
    }
}

}  // namespace

extern "C" int cfm_stream_stage_f32(const float* samples, int64_t ld_samples, int n_max, const float* tail_in, float* tail_out,
                                    const int* table, float* xp, int S, int f_max, int hop, int n_fft, cfm_stream_t stream) {
    CFM_REQUIRE(tail_in && tail_out && table && xp && (samples || n_max == 0), CFM_ERR_NULL);
    CFM_REQUIRE(S > 0 && f_max >= 0 && n_max >= 0 && ld_samples >= n_max && n_fft > 0 && hop > 0, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(hop % 4 == 0 && n_fft % 4 == 0 && hop <= n_fft, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(n_fft <= TAIL_LD && S < 65535, CFM_ERR_UNSUPPORTED);                   // the tail holds up to n_fft - 1 samples
    const int64_t pitch = ((int64_t)f_max + (n_fft + hop - 1) / hop) * hop;
    CFM_REQUIRE(pitch < (1ll << 30) && n_max < (1 << 29), CFM_ERR_UNSUPPORTED);        // in-pitch and cat indices are int32
    const float* in_end = tail_in + (int64_t)S * TAIL_LD;
    const float* out_end = tail_out + (int64_t)S * TAIL_LD;
    CFM_REQUIRE(in_end <= tail_out || out_end <= tail_in, CFM_ERR_UNSUPPORTED);        // the tails ping-pong: never in place
    CFM_REQUIRE(CFM_ALIGNED16(xp), CFM_ERR_ALIGN);
    const dim3 grid((unsigned)((pitch + 1023) / 1024), (unsigned)(S + 1));
    hipLaunchKernelGGL(stream_stage_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), samples, ld_samples, n_max,
                       tail_in, tail_out, table, xp, S, f_max, hop, n_fft, (int)pitch);
    return cfm_launch_status();
}
