// Voice activity detection on log-mel frames (INTEGRATION.md "Voice activity detection"): the definition is the comment of
// conformer_hip3_vad.h.  Two kernels, one per entry.
//
// Energy: grid (frame tile, slot), one lane per frame, so a wave reads 64 consecutive frames of one mel row (256 contiguous
// bytes) per load.  A lane holds its frame's band in registers (the kernel is instantiated for 32, 64, 96 and 128 rows): the band
// is read once and all of a frame's loads are in flight together; the maximum and then the sum, in the order of the rows, are
// taken from the registers.  A frame's energy depends on its column alone.
//
// Scan: one workgroup of 16 waves per slot.  LDS holds E = the H = Wn + smooth - 2 stored energies in front of the step (from the
// ring) followed by the step's own, and S = s of the Wn - 1 frames in front of the step followed by the step's own; frames before
// the slot was armed are +inf in both, the neutral element of the minimum.  s of every frame is one thread's sum, oldest first.
// The trailing minimum over Wn: p doubling passes leave the minimum over [i, i + 2^p) at i, 2^p the largest power of two <= Wn,
// and the window [i, i + Wn) is the union of [i, i + 2^p) and [i + Wn - 2^p, i + Wn).  The flags are balloted into 64-bit words;
// wave 0 then walks the words: lane l derives both run lengths after frame l from the bits at or below l and the carried runs, two
// ballots mark the frames at which a segment could open or close, and a wave-uniform loop hops from event to event.
// Every value read from the device that indexes anything is clamped first (k to [0, k_max]).
#include <math.h>
#include "cfm_common.h"
#include "conformer_hip3_vad.h"

namespace {

constexpr int K_MAX = CFM3_VAD_SCAN_FRAMES, SMOOTH_MAX = CFM3_VAD_SMOOTH_MAX, WN_MAX = CFM3_VAD_WINDOW_MAX;
constexpr int BAND_MAX = CFM3_VAD_BAND_MAX, STATE_LD = CFM3_VAD_STATE_COLS, COUNT_MAX = 1 << 24;
constexpr int HIST_MAX = WN_MAX + SMOOTH_MAX - 2;                        // stored energies in front of a step
constexpr int E_TILE = 256, THREADS = 1024;

__device__ __forceinline__ int clamp_k(int64_t kraw, int k_max) { return (int)(kraw < 0 ? 0 : kraw > k_max ? k_max : kraw); }

// NB: the band's rows rounded up to a multiple of 32.  A lane holds its column of the band in registers, so every load of a frame
// is issued before the first is used and the band is read once.
template <int NB>
__global__ __launch_bounds__(E_TILE) void vad_energy_kernel(const float* __restrict__ mel, int64_t ld_slot, int64_t ld_mel,
                                                            const int64_t* __restrict__ k, int k_max, int m_lo, int m_hi,
                                                            float* __restrict__ energy, int64_t ld_energy) {
    const int b = blockIdx.y;
    const int kb = clamp_k(k[b], k_max);
    const int64_t t = (int64_t)blockIdx.x * E_TILE + threadIdx.x;
    if (t >= kb) return;
    const float* x = mel + (int64_t)b * ld_slot + (int64_t)m_lo * ld_mel + t;
    const int nb = m_hi - m_lo;                                                // (uniform)
    float v[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) v[i] = i < nb ? x[(int64_t)i * ld_mel] : -INFINITY;
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NB; ++i) m = fmaxf(m, v[i]);                           // (fmaxf drops a NaN; the sum below keeps it)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i)
        if (i < nb) s += expf(v[i] - m);                                       // in the order of the rows
    const float e = m + logf(s);
    energy[(int64_t)b * ld_energy + t] = fabsf(e) < INFINITY ? e : INFINITY;   // (false for a NaN)
}

__global__ __launch_bounds__(THREADS) void vad_scan_kernel(const float* __restrict__ energy, int64_t ld_energy,
                                                           const int64_t* __restrict__ k, int k_max, int smooth, int Wn, float snr,
                                                           float min_energy, int onset, int hangover, int* __restrict__ state,
                                                           float* __restrict__ ring, unsigned char* __restrict__ flags,
                                                           int64_t ld_flags, int* __restrict__ segments, int max_segments) {
    __shared__ float E[HIST_MAX + K_MAX];
    __shared__ float Sa[WN_MAX - 1 + K_MAX], Sb[WN_MAX - 1 + K_MAX];
    __shared__ unsigned long long words[K_MAX / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kb = clamp_k(k[b], k_max);                                  // (uniform per workgroup)
    if (kb == 0) return;
    int* st = state + (int64_t)b * STATE_LD;
    const int F = st[0];                                                   // frames absorbed before this step
    const int R = Wn + smooth - 1, H = R - 1;
    float* rg = ring + (int64_t)b * R;
    const float* en = energy + (int64_t)b * ld_energy;

    // E[i] = the stored energy of frame F - H + i
    for (int i = tid; i < H + kb; i += THREADS) {
        float v;
        if (i < H) {
            const int u = F - H + i;
            v = u >= 0 ? rg[u % R] : INFINITY;
        } else {
            v = en[i - H];
        }
        E[i] = v;
    }
    __syncthreads();
    // the ring is read; frame u goes to u mod R (of a step longer than the ring only the last R frames)
    for (int j = max(0, kb - R) + tid; j < kb; j += THREADS) rg[(F + j) % R] = E[H + j];
    // Sa[i] = s of frame F - (Wn - 1) + i, whose energy is E[i + smooth - 1]
    const int N = Wn - 1 + kb;
    for (int i = tid; i < N; i += THREADS) {
        const int u = F - (Wn - 1) + i;
        float s = INFINITY;
        if (u >= 0) {
            const int cnt = min(smooth, u + 1), at = i + smooth - 1;
            float sum = 0.f;
            for (int j = cnt - 1; j >= 0; --j) sum += E[at - j];           // oldest first
            s = sum / (float)cnt;
        }
        Sa[i] = s;
    }
    __syncthreads();
    float* src = Sa;
    float* dst = Sb;
    int span = 1;
    while (2 * span <= Wn) {                                               // (uniform: Wn is an argument)
        for (int i = tid; i < N; i += THREADS) dst[i] = fminf(src[i], i + span < N ? src[i + span] : INFINITY);
        __syncthreads();
        float* o = src; src = dst; dst = o;
        span *= 2;
    }
    // src[i] = min of s over [i, i + span); frame j of the step has its window at [j, j + Wn)
    for (int base = wave * 64; base < kb; base += THREADS) {               // (uniform per wave)
        const int j = base + lane;
        bool raw = false;
        if (j < kb) {
            const float f = fminf(src[j], src[j + Wn - span]);
            const float e = E[H + j];
            raw = fabsf(e) < INFINITY && e - f >= snr && e >= min_energy;  // (each false for a NaN)
            flags[(int64_t)b * ld_flags + j] = raw ? 1 : 0;
        }
        const unsigned long long w = __ballot(raw);
        if (lane == 0) words[base >> 6] = w;
    }
    __syncthreads();
    if (wave != 0) return;

    int run_speech = st[1], run_silence = st[2], in_speech = st[3], start = st[4], count = st[5];
    int* seg = segments + (int64_t)b * max_segments * 2;
    for (int base = 0; base < kb; base += 64) {
        const int n = min(64, kb - base);                                  // frames of this block, 1 .. 64
        const unsigned long long valid = n == 64 ? ~0ull : (1ull << n) - 1;
        const unsigned long long raw = words[base >> 6] & valid;
        const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1;       // frames 0 .. lane of the block
        const unsigned long long speech = raw & upto, silence = ~raw & valid & upto;
        const bool is_raw = (raw >> lane) & 1;
        // the runs that end at frame `lane`: back to the last frame of the other kind, or through the whole block so far
        const int rs = !is_raw ? 0 : silence ? lane - (63 - __clzll((long long)silence)) : run_speech + lane + 1;
        const int rq = is_raw ? 0 : speech ? lane - (63 - __clzll((long long)speech)) : run_silence + lane + 1;
        const unsigned long long opens = __ballot(rs >= onset) & valid;    // (a lane behind n is not raw: rs = 0 < onset)
        const unsigned long long closes = __ballot(rq >= hangover) & valid;
        int pos = 0;
        while (pos < 64) {                                                 // (uniform: every lane holds the same state)
            const unsigned long long next = (in_speech ? closes : opens) & (~0ull << pos);
            if (!next) break;
            const int at = __ffsll((long long)next) - 1;
            if (!in_speech) {
                start = F + base + at - __shfl(rs, at, 64) + 1;
                in_speech = 1;
            } else {
                const int end = F + base + at - __shfl(rq, at, 64) + 1;
                if (lane == 0 && count < max_segments) {
                    seg[2 * count] = start;
                    seg[2 * count + 1] = end;
                }
                ++count;
                in_speech = 0;
            }
            pos = at + 1;
        }
        run_speech = __shfl(rs, n - 1, 64);
        run_silence = __shfl(rq, n - 1, 64);
    }
    if (lane == 0) {
        st[0] = F + kb; st[1] = run_speech; st[2] = run_silence; st[3] = in_speech; st[4] = start; st[5] = count;
    }
}

}  // namespace

extern "C" int cfm3_vad_energy_f32(const float* mel, int64_t ld_slot, int64_t ld_mel, const int64_t* k, int k_max, int n_mel,
                                   int m_lo, int m_hi, float* energy, int64_t ld_energy, int S, cfm_stream_t stream) {
    CFM_REQUIRE(k && energy && (mel || k_max == 0), CFM_ERR_NULL);
    CFM_REQUIRE(S > 0 && k_max >= 0 && n_mel >= 1, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(m_lo >= 0 && m_lo < m_hi && m_hi <= n_mel, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(ld_mel >= k_max && ld_slot >= 0 && ld_slot / n_mel >= ld_mel && ld_energy >= k_max, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(m_hi - m_lo <= BAND_MAX && S <= 65535, CFM_ERR_UNSUPPORTED);
    if (k_max == 0) return CFM_OK;
    const dim3 grid((unsigned)((k_max + (int64_t)E_TILE - 1) / E_TILE), (unsigned)S);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    switch ((m_hi - m_lo + 31) / 32) {
    case 1: hipLaunchKernelGGL(vad_energy_kernel<32>, grid, dim3(E_TILE), 0, s, mel, ld_slot, ld_mel, k, k_max, m_lo, m_hi, energy, ld_energy); break;
    case 2: hipLaunchKernelGGL(vad_energy_kernel<64>, grid, dim3(E_TILE), 0, s, mel, ld_slot, ld_mel, k, k_max, m_lo, m_hi, energy, ld_energy); break;
    case 3: hipLaunchKernelGGL(vad_energy_kernel<96>, grid, dim3(E_TILE), 0, s, mel, ld_slot, ld_mel, k, k_max, m_lo, m_hi, energy, ld_energy); break;
    default: hipLaunchKernelGGL(vad_energy_kernel<128>, grid, dim3(E_TILE), 0, s, mel, ld_slot, ld_mel, k, k_max, m_lo, m_hi, energy, ld_energy); break;
    }
    return cfm_launch_status();
}

extern "C" int cfm3_vad_scan_f32(const float* energy, int64_t ld_energy, const int64_t* k, int k_max, int smooth,
                                 int noise_window, float snr, float min_energy, int onset, int hangover, int* state, float* ring,
                                 unsigned char* flags, int64_t ld_flags, int* segments, int max_segments, int S,
                                 cfm_stream_t stream) {
    CFM_REQUIRE(k && state && ring && flags && segments && (energy || k_max == 0), CFM_ERR_NULL);
    CFM_REQUIRE(S > 0 && k_max >= 0, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(smooth >= 1 && noise_window >= 1 && onset >= 1 && hangover >= 1 && max_segments >= 1, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(ld_energy >= k_max && ld_flags >= k_max, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(snr == snr && min_energy == min_energy, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(k_max <= K_MAX && smooth <= SMOOTH_MAX && noise_window <= WN_MAX, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(onset <= COUNT_MAX && hangover <= COUNT_MAX && max_segments <= COUNT_MAX && S <= 65535, CFM_ERR_UNSUPPORTED);
    if (k_max == 0) return CFM_OK;
    hipLaunchKernelGGL(vad_scan_kernel, dim3((unsigned)S), dim3(THREADS), 0, static_cast<hipStream_t>(stream), energy, ld_energy,
                       k, k_max, smooth, noise_window, snr, min_energy, onset, hangover, state, ring, flags, ld_flags, segments,
                       max_segments);
    return cfm_launch_status();
}
