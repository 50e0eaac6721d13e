// Endpointing (INTEGRATION.md "Endpointing"): Kaldi's endpoint rules on the CTC blank posterior, per slot, one launch per step.
//
// A frame is silent iff log p_sil = log(sum over the silence ids of softmax(x)) >= log_threshold.  Per slot the state carries
// {frames, trailing silent run, non-silent frames} and a latch {rule, end_frame, end_trailing}: the first frame at which a rule
// (min_trailing, min_frames, min_speech) holds, with the lowest rule index.
//
// One workgroup of 16 waves per slot (a step has few slots and its rows are independent: the waves hide each other's load
// latency).  Wave w classifies rows w, w + 16, ...: lane l takes x_l, x_{l+64}, ... in that order, first for the maximum, then
// for the sum of exp(x - m), and the 64 partials are folded by the xor butterfly, which gives every lane the same bits.  Up to V
// = 512 a lane holds its 8 values in registers, the row is read once and the next row's loads are issued before this row's
// arithmetic; beyond, the row is walked twice (it stays in the vector L1 between the passes).  The order of every operation
// depends on V alone, so a frame's flag does not depend on the step it arrived in.  Lane 0 writes the flag to an LDS byte per row; after one barrier wave 0
// scans the flags 64 frames at a time: a ballot turns them into a mask, lane l derives the counters after frame l from the mask
// bits at or below l and the carried counters, evaluates the rules, and a second ballot finds the first frame at which one holds.
// Every value read from the device that indexes anything is clamped first (k to [0, k_max], the silence ids to [0, V)).
#include <math.h>
#include "cfm_common.h"
#include "../../include/conformer_hip_endpoint.h"

namespace {

constexpr int K_MAX = 4096, V_MAX = 65536, SIL_MAX = 8, RULES_MAX = 4, STATE_LD = 8, RULE_LD = 4;
constexpr int WAVES = 16, THREADS = 64 * WAVES;
constexpr int REG_VALUES = 8, REG_V = 64 * REG_VALUES;                   // a row of V <= 512 is held in registers

// log p_sil >= log_thr, given the row's maximum and sum of exp(x - m); the same in every lane of the wave
__device__ __forceinline__ bool silent_given(const float* __restrict__ x, float m, float s, const int (&sil)[SIL_MAX], int n_sil,
                                             float log_thr) {
    const float lse = m + logf(s);
    float lp = x[sil[0]] - lse;
    if (n_sil > 1) {
        float p = expf(lp);
#pragma unroll
        for (int i = 1; i < SIL_MAX; ++i)
            if (i < n_sil) p += expf(x[sil[i]] - lse);                     // in the order of silence_ids
        lp = logf(p);
    }
    return lp >= log_thr;                                                  // false for a NaN
}

// the flag of one frame of any V: two walks over the row
__device__ __forceinline__ bool frame_is_silent(const float* __restrict__ x, int V, const int (&sil)[SIL_MAX], int n_sil,
                                                float log_thr, int lane) {
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);                 // (fmaxf drops a NaN; the sum below keeps it)
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(x[v] - m);
    s = wave_sum(s);
    return silent_given(x, m, s, sil, n_sil, log_thr);
}

// V <= 512: the lane's values x_l, x_{l+64}, ... of a row, -inf behind V (which adds exp(-inf) = 0 to the sum)
__device__ __forceinline__ void load_row(const float* __restrict__ x, int V, int lane, float (&xv)[REG_VALUES]) {
#pragma unroll
    for (int j = 0; j < REG_VALUES; ++j) {
        const int v = lane + 64 * j;
        xv[j] = v < V ? x[v] : -INFINITY;
    }
}

__device__ __forceinline__ bool frame_is_silent_reg(const float* __restrict__ x, const float (&xv)[REG_VALUES],
                                                    const int (&sil)[SIL_MAX], int n_sil, float log_thr) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < REG_VALUES; ++j) m = fmaxf(m, xv[j]);
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < REG_VALUES; ++j) s += expf(xv[j] - m);
    s = wave_sum(s);
    return silent_given(x, m, s, sil, n_sil, log_thr);
}

template <bool REG>
__global__ __launch_bounds__(THREADS) void endpoint_step_kernel(const float* __restrict__ logits, int64_t ld_slot, int64_t ld_row,
                                                            const int64_t* __restrict__ k, int k_max, int V,
                                                            const int* __restrict__ silence_ids, int n_sil, float log_thr,
                                                            const int* __restrict__ rules, int n_rules, int* __restrict__ state) {
    __shared__ unsigned char flags[K_MAX];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t kraw = k[b];
    const int kb = (int)(kraw < 0 ? 0 : kraw > k_max ? k_max : kraw);      // (uniform per workgroup)
    if (kb == 0) return;
    int sil[SIL_MAX];
#pragma unroll
    for (int i = 0; i < SIL_MAX; ++i) sil[i] = i < n_sil ? min(max(silence_ids[i], 0), V - 1) : 0;
    const float* slot = logits + (int64_t)b * ld_slot;
    if (REG) {
        float cur[REG_VALUES], nxt[REG_VALUES];
        if (wave < kb) load_row(slot + (int64_t)wave * ld_row, V, lane, cur);
        for (int r = wave; r < kb; r += WAVES) {
            const bool more = r + WAVES < kb;                              // (uniform per wave)
            if (more) load_row(slot + (int64_t)(r + WAVES) * ld_row, V, lane, nxt);
            const bool silent = frame_is_silent_reg(slot + (int64_t)r * ld_row, cur, sil, n_sil, log_thr);
            if (lane == 0) flags[r] = silent ? 1 : 0;
#pragma unroll
            for (int j = 0; j < REG_VALUES; ++j) cur[j] = more ? nxt[j] : cur[j];
        }
    } else {
        for (int r = wave; r < kb; r += WAVES) {
            const bool silent = frame_is_silent(slot + (int64_t)r * ld_row, V, sil, n_sil, log_thr, lane);
            if (lane == 0) flags[r] = silent ? 1 : 0;
        }
    }
    __syncthreads();
    if (wave != 0) return;

    int mt[RULES_MAX], mf[RULES_MAX], ms[RULES_MAX];
#pragma unroll
    for (int r = 0; r < RULES_MAX; ++r) {
        const bool on = r < n_rules;
        mt[r] = on ? rules[r * RULE_LD + 0] : 0;
        mf[r] = on ? rules[r * RULE_LD + 1] : 0;
        ms[r] = on ? rules[r * RULE_LD + 2] : 0;
    }
    int* st = state + (int64_t)b * STATE_LD;
    int frames = st[0], trailing = st[1], speech = st[2], rule = st[3], end_frame = st[4], end_trailing = st[5];
    for (int base = 0; base < kb; base += 64) {
        const int n = min(64, kb - base);                                  // frames of this block, 1 .. 64
        const bool live = lane < n;
        const unsigned long long valid = n == 64 ? ~0ull : (1ull << n) - 1;
        const unsigned long long silent = __ballot(flags[live ? base + lane : 0] != 0) & valid;
        const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1;       // frames 0 .. lane of the block
        const unsigned long long spoken = ~silent & valid & upto;          // the non-silent frames at or below this lane
        // the silent run that ends at frame `lane`: back to the last non-silent frame, or through the whole block so far
        const int tr = spoken ? lane - (63 - __clzll((long long)spoken)) : trailing + lane + 1;
        const int sp = speech + __popcll(spoken);
        const int fr = frames + lane + 1;
        int hit = -1;
#pragma unroll
        for (int r = RULES_MAX - 1; r >= 0; --r)
            if (r < n_rules && tr >= mt[r] && fr >= mf[r] && sp >= ms[r]) hit = r;            // the lowest index that holds
        const unsigned long long fired = __ballot(live && hit >= 0);
        if (rule < 0 && fired) {
            const int first = __ffsll((long long)fired) - 1;
            rule = __shfl(hit, first, 64);
            end_trailing = __shfl(tr, first, 64);
            end_frame = frames + first;
        }
        trailing = __shfl(tr, n - 1, 64);
        speech = __shfl(sp, n - 1, 64);
        frames += n;
    }
    if (lane == 0) {
        st[0] = frames; st[1] = trailing; st[2] = speech; st[3] = rule; st[4] = end_frame; st[5] = end_trailing;
    }
}

}  // namespace

extern "C" int cfm_endpoint_step_f32(const float* logits, int64_t ld_slot, int64_t ld_row, const int64_t* k, int k_max, int V,
                                     const int* silence_ids, int n_silence, float log_threshold, const int* rules, int n_rules,
                                     int* state, int S, cfm_stream_t stream) {
    CFM_REQUIRE(k && silence_ids && rules && state && (logits || k_max == 0), CFM_ERR_NULL);
    CFM_REQUIRE(S > 0 && k_max >= 0 && V >= 2, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(n_silence >= 1 && n_silence <= SIL_MAX && n_rules >= 1 && n_rules <= RULES_MAX, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(log_threshold == log_threshold, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(ld_row >= V && ld_slot >= 0 && (k_max == 0 || ld_slot / k_max >= ld_row), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(k_max <= K_MAX && S < 65535 && V <= V_MAX, CFM_ERR_UNSUPPORTED);
    if (k_max == 0) return CFM_OK;
    if (V <= REG_V)
        hipLaunchKernelGGL(endpoint_step_kernel<true>, dim3((unsigned)S), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                           logits, ld_slot, ld_row, k, k_max, V, silence_ids, n_silence, log_threshold, rules, n_rules, state);
    else
        hipLaunchKernelGGL(endpoint_step_kernel<false>, dim3((unsigned)S), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                           logits, ld_slot, ld_row, k, k_max, V, silence_ids, n_silence, log_threshold, rules, n_rules, state);
    return cfm_launch_status();
}
