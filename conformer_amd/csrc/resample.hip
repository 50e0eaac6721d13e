// Input sample rates (INTEGRATION.md "Input sample rates"): the Hann-windowed-sinc polyphase resampler in front of the audio
// front end, offline and per slot in streams, one launch per step.
//
// Rates R_in -> R_out, g = gcd, o = R_in / g, n = R_out / g: output q = i n + j of a stream is sum_m k[j, m] x[i o - width + m],
// K = 2 width + o taps per phase.  Every slot carries the samples a later output still needs (the tail, < K of them).  Per step
// the host works out from the sample counts alone how many blocks of n outputs are complete and hands the kernel one int32 row
// per slot: with cat = [tail | new frames, converted and downmixed] the slot's outputs are taken at cat index i o + m - lead,
// zero outside cat (the lead zeros in front of a stream; behind its end on a flush).  The device sees tail-relative offsets
// only.  The tails ping-pong between two buffers: nothing the launch reads is written by it.
//
// A workgroup owns bpw whole blocks of one slot (bpw n <= RUN outputs): it stages their input span, bpw o + 2 width floats,
// in LDS, converted once, then every thread runs the K taps of up to four outputs at a time.  Consecutive lanes take
// consecutive outputs, that is consecutive phases of one block: they read one coalesced row of the transposed bank (K, n) per
// tap (L2 resident: 1.2 MB at 44.1 kHz) and their LDS reads of x broadcast.  With n <= 2 the lanes walk x with stride o / n and
// the bank (n K <= 2048 floats) sits in LDS too.  Products and sums are fp32 FMAs in tap order m = 0 .. K-1 for every output,
// whatever its place in the launch: chunking changes no bit.
// Every table value is clamped before it indexes anything: a corrupt table cannot make a read or a write leave the buffers.
#include "cfm_common.h"
#include "../../include/conformer_hip_resample.h"

namespace {

constexpr int TAIL_LD = 1024, COLS = 8;              // floats per tail row, int32 per table row (the header states both)
constexpr int RUN = 1024;                            // outputs per workgroup at most
constexpr int XS_FLOATS = 12288;                     // LDS floats for the staged input span (48 KiB)
constexpr int BANK_LDS_FLOATS = 2048;                // a bank this small (n <= 2 at K = 1024) is kept in LDS
constexpr int K_MAX = 1024, N_MAX = 640, C_MAX = 8;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct SlotRow {
    int tail_len, n_new, m, lead, n_out, keep, new_tail_len;
};

__device__ __forceinline__ SlotRow read_row(const int* __restrict__ row, bool tails, int n_max, int width, int ld_y) {
    SlotRow r;
    r.tail_len = tails ? clampi(row[0], 0, TAIL_LD) : 0;
    r.n_new = clampi(row[1], 0, n_max);
    r.m = r.tail_len + r.n_new;
    r.lead = clampi(row[2], 0, width);
    r.n_out = clampi(row[3], 0, ld_y);
    r.keep = clampi(row[5], 0, r.m);
    r.new_tail_len = row[4] ? 0 : clampi(row[6], 0, min(TAIL_LD, r.m - r.keep));
    return r;
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(int16_t v) { return (float)v * 0x1p-15f; }

// frame f of a row: (x_0 + ... + x_{C-1}) * fp32(1 / C), left to right, every step rounded to fp32
template <typename T>
__device__ __forceinline__ float frame_at(const T* __restrict__ fresh, int C, float inv_c, int f) {
#pragma clang fp contract(off)
    const T* p = fresh + (int64_t)f * C;
    float s = to_f32(p[0]);
    for (int c = 1; c < C; ++c) s = s + to_f32(p[c]);
    return s * inv_c;
}

// cat[c], 0 <= c < m
template <typename T>
__device__ __forceinline__ float cat_at(const float* __restrict__ tail, const T* __restrict__ fresh, int C, float inv_c,
                                        const SlotRow& r, int c) {
    return c < r.tail_len ? tail[c] : frame_at(fresh, C, inv_c, c - r.tail_len);
}

// grid (max(1, ceil(ld_y / (bpw n))), S): workgroup (x, b) writes y[b, x bpw n : (x + 1) bpw n] (outputs, then zeros up to
// ld_y); workgroup 0 of a slot also writes its new tail, all TAIL_LD floats of it (zeros behind new_tail_len).
template <typename T, bool BANK_LDS>
__global__ __launch_bounds__(256) void resample_kernel(const T* __restrict__ samples, int64_t ld_samples, int n_max, int C,
                                                       float inv_c, const float* __restrict__ tail_in,
                                                       float* __restrict__ tail_out, const int* __restrict__ table,
                                                       const float* __restrict__ bank_t, int o, int n, int width, int bpw,
                                                       float* __restrict__ y, int ld_y) {
    __shared__ float xs[XS_FLOATS];
    __shared__ float bank_s[BANK_LDS ? BANK_LDS_FLOATS : 1];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int K = 2 * width + o;
    const SlotRow r = read_row(table + (int64_t)b * COLS, tail_in != nullptr, n_max, width, ld_y);
    const float* tail = tail_in ? tail_in + (int64_t)b * TAIL_LD : nullptr;
    const T* fresh = samples + (int64_t)b * ld_samples;
    const int run = bpw * n;                                             // <= RUN (or n itself when n > RUN: not supported)
    const int64_t r0 = (int64_t)blockIdx.x * run;                        // first output of this workgroup
    if (r0 < r.n_out) {                                                  // (uniform per workgroup)
        const int span = bpw * o + 2 * width;                            // <= XS_FLOATS: the host chose bpw so
        const int64_t c0 = (int64_t)blockIdx.x * bpw * o - r.lead;       // cat index of xs[0]
        for (int s = tid; s < span; s += 256) {
            const int64_t c = c0 + s;
            xs[s] = (c >= 0 && c < r.m) ? cat_at(tail, fresh, C, inv_c, r, (int)c) : 0.f;
        }
        if (BANK_LDS)
            for (int s = tid; s < n * K; s += 256) bank_s[s] = bank_t[s];
        __syncthreads();
        const float* __restrict__ bk = BANK_LDS ? bank_s : bank_t;
        for (int base = 0; base < run; base += 1024) {
            int xo[4], j[4];
            bool live[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int rl = base + e * 256 + tid;                     // output r0 + rl: block rl / n of this workgroup, phase rl % n
                live[e] = rl < run && r0 + rl < r.n_out;
                const int il = live[e] ? rl / n : 0;
                j[e] = live[e] ? rl - il * n : 0;
                xo[e] = il * o;                                          // xo + m <= (bpw - 1) o + K - 1 < span
            }
            float acc[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = bk[j[e]] * xs[xo[e]];
            for (int m = 1; m < K; ++m) {
                const float* __restrict__ row = bk + m * n;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(row[j[e]], xs[xo[e] + m], acc[e]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (live[e]) y[(int64_t)b * ld_y + r0 + base + e * 256 + tid] = acc[e];
        }
    }
    // zeros behind the slot's outputs, up to the pitch
    for (int rl = tid; rl < run; rl += 256) {
        const int64_t q = r0 + rl;
        if (q >= r.n_out && q < ld_y) y[(int64_t)b * ld_y + q] = 0.f;
    }
    if (blockIdx.x == 0 && tail_out) {
        for (int t = tid; t < TAIL_LD; t += 256)
            tail_out[(int64_t)b * TAIL_LD + t] = t < r.new_tail_len ? cat_at(tail, fresh, C, inv_c, r, r.keep + t) : 0.f;
    }
}

template <typename T>
int resample_launch(const T* samples, int64_t ld_samples, int n_max, int C, const float* tail_in, float* tail_out,
                    const int* table, const float* bank_t, int o, int n, int width, float* y, int64_t ld_y, int S,
                    cfm_stream_t stream) {
    CFM_REQUIRE(table && bank_t && y && (samples || n_max == 0), CFM_ERR_NULL);
    CFM_REQUIRE((tail_in == nullptr) == (tail_out == nullptr), CFM_ERR_NULL);
    CFM_REQUIRE(S > 0 && n_max >= 0 && C >= 1 && o >= 1 && n >= 1 && width >= 0 && ld_y >= 0 && ld_y % 4 == 0, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(C <= C_MAX && n <= N_MAX && o <= K_MAX && width <= K_MAX && 2 * width + o <= K_MAX, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(ld_samples >= (int64_t)n_max * C, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(S < 65535 && ld_y < (1ll << 30) && (int64_t)n_max * C < (1ll << 30), CFM_ERR_UNSUPPORTED);   // int32 indices in a row
    if (tail_in) {
        const float* in_end = tail_in + (int64_t)S * TAIL_LD;
        const float* out_end = tail_out + (int64_t)S * TAIL_LD;
        CFM_REQUIRE(in_end <= tail_out || out_end <= tail_in, CFM_ERR_UNSUPPORTED);    // the tails ping-pong: never in place
    }
    CFM_REQUIRE(CFM_ALIGNED16(y) && CFM_ALIGNED16(bank_t) && CFM_ALIGNED16(tail_in) && CFM_ALIGNED16(tail_out), CFM_ERR_ALIGN);
    CFM_REQUIRE(reinterpret_cast<uintptr_t>(samples) % sizeof(T) == 0, CFM_ERR_ALIGN);
    // whole blocks per workgroup: RUN outputs at most, and an input span bpw o + 2 width inside the LDS staging buffer
    // (one block always fits: o + 2 width = K <= 1024)
    int bpw = RUN / n > 1 ? RUN / n : 1;
    const int fit = (XS_FLOATS - 2 * width) / o;
    bpw = bpw < fit ? bpw : fit;
    const int64_t run = (int64_t)bpw * n;
    const int64_t gx = ld_y > 0 ? (ld_y + run - 1) / run : 1;
    const dim3 grid((unsigned)gx, (unsigned)S);
    const float inv_c = 1.0f / (float)C;
    const int K = 2 * width + o;
    if ((int64_t)n * K <= BANK_LDS_FLOATS)
        hipLaunchKernelGGL((resample_kernel<T, true>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), samples, ld_samples,
                           n_max, C, inv_c, tail_in, tail_out, table, bank_t, o, n, width, bpw, y, (int)ld_y);
    else
        hipLaunchKernelGGL((resample_kernel<T, false>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), samples, ld_samples,
                           n_max, C, inv_c, tail_in, tail_out, table, bank_t, o, n, width, bpw, y, (int)ld_y);
    return cfm_launch_status();
}

}  // namespace

extern "C" int cfm_resample_f32(const float* samples, int64_t ld_samples, int n_max, int C, const float* tail_in, float* tail_out,
                                const int* table, const float* bank_t, int o, int n, int width, float* y, int64_t ld_y, int S,
                                cfm_stream_t stream) {
    return resample_launch<float>(samples, ld_samples, n_max, C, tail_in, tail_out, table, bank_t, o, n, width, y, ld_y, S, stream);
}

extern "C" int cfm_resample_i16(const void* samples, int64_t ld_samples, int n_max, int C, const float* tail_in, float* tail_out,
                                const int* table, const float* bank_t, int o, int n, int width, float* y, int64_t ld_y, int S,
                                cfm_stream_t stream) {
    return resample_launch<int16_t>(static_cast<const int16_t*>(samples), ld_samples, n_max, C, tail_in, tail_out, table, bank_t, o,
                                    n, width, y, ld_y, S, stream);
}
