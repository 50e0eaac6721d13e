// CTC keyword spotting on fp32 logits (INTEGRATION.md "Keyword spotting"): the definition is the comment of
// conformer_hip3_kws.h.  Two kernels, one per entry.
//
// Row maximum: one wave per row, four rows per workgroup, lanes along v so every load instruction reads 256 contiguous bytes;
// fmaxf drops a NaN, a butterfly of shuffles leaves the maximum in every lane, lane 0 stores it (NaN when it is not finite).
//
// Scan: one wave per (group, slot).  A lane is one state of one keyword and keeps (a, start) and its keyword's detector in
// registers for the whole step.  Per frame the neighbours i - 1 and i - 2 arrive by a wave shift of one lane, applied once and
// twice (DPP wave_shr:1, no LDS); the lane's own FIRST / SKIP flags decide whether they are looked at, so a keyword never sees
// the last states of the keyword in the lanes in front of it.  The frame's operand x[t][label(lane)] does not depend on the
// state, so the gathers of the next RING frames are always in flight: two register blocks of RING frames are filled in turn, a
// block's loads all issued before the wave steps through the block in front of it (every slot a fixed register, the row index of
// a load clamped to the slot's last row instead of branched around), so a step waits for a load issued RING steps earlier.  Emissions of a frame: ballot, then each emitting lane's row is the count
// plus the emitting lanes below it.  No barrier, no atomic, no LDS.
// Every value read from the device that indexes anything is clamped first (k to [0, k_max], labels to [0, V), keyword indices
// to [0, K)).
#include <math.h>
#include "cfm_common.h"
#include "conformer_hip3_kws.h"

namespace {

constexpr int ROWS = CFM3_KWS_STATE_ROWS, LANES = CFM3_KWS_GROUP_LANES, RING = CFM3_KWS_RING_FRAMES;
constexpr int V_MAX = CFM3_KWS_V_MAX, G_MAX = 1 << 20, DET_MAX = 1 << 24;
constexpr int RM_WAVES = 4;                                              // rows per workgroup of the row-maximum kernel

__device__ __forceinline__ int clamp_k(int64_t kraw, int k_max) { return (int)(kraw < 0 ? 0 : kraw > k_max ? k_max : kraw); }

__global__ __launch_bounds__(RM_WAVES * 64) void kws_rowmax_kernel(const float* __restrict__ x, int64_t ld_slot, int64_t ld_row,
                                                                   const int64_t* __restrict__ k, int k_max, int V,
                                                                   float* __restrict__ rowmax, int64_t ld_rowmax) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int kb = clamp_k(k[b], k_max);
    const int64_t t = (int64_t)blockIdx.x * RM_WAVES + (threadIdx.x >> 6);   // (uniform per wave)
    if (t >= kb) return;
    const float* row = x + (int64_t)b * ld_slot + t * ld_row;
    float m = -INFINITY;
#pragma unroll 8
    for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);               // (fmaxf drops a NaN)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if (lane == 0) rowmax[(int64_t)b * ld_rowmax + t] = fabsf(m) < INFINITY ? m : NAN;
}

// the value of the lane below (lane 0 keeps its own: its flags never look at it)
__device__ __forceinline__ int lane_below(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float lane_below(float v) { return __int_as_float(lane_below(__float_as_int(v))); }

__global__ __launch_bounds__(64) void kws_scan_kernel(const float* __restrict__ x, int64_t ld_slot, int64_t ld_row,
                                                      const float* __restrict__ rowmax, int64_t ld_rowmax,
                                                      const int64_t* __restrict__ k, int k_max, int V,
                                                      const int* __restrict__ lanes, const float* __restrict__ threshold, int G,
                                                      int K, int* __restrict__ state, int* __restrict__ detections,
                                                      int max_detections, int* __restrict__ counts) {
    const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int kb = clamp_k(k[b], k_max);                                   // (uniform)
    if (kb == 0) return;
    const int* tab = lanes + (int64_t)g * 3 * LANES;
    const int label = tab[lane], flags = tab[2 * LANES + lane];
    const bool idle = label < 0;
    const int col = min(max(label, 0), V - 1);
    const int kw = min(max(tab[LANES + lane], 0), K - 1);
    const bool first = flags & CFM3_KWS_FLAG_FIRST, skip = flags & CFM3_KWS_FLAG_SKIP, last = (flags & CFM3_KWS_FLAG_LAST) && !idle;
    const float thr = threshold[kw];

    int* st = state + ((int64_t)b * G + g) * ROWS * LANES + lane;
    float a = __int_as_float(st[0]);
    int start = st[LANES];
    int held = st[2 * LANES], held_start = st[3 * LANES], held_end = st[4 * LANES];
    float held_score = __int_as_float(st[5 * LANES]);
    const int F = __builtin_amdgcn_readfirstlane(st[6 * LANES]);           // (lane 0's: the frames before this step)
    int count = counts[(int64_t)b * G + g];                                // (uniform)
    int* det = detections + ((int64_t)b * G + g) * max_detections * 4;
    const unsigned long long below = lane == 0 ? 0ull : ~0ull >> (64 - lane);

    const float* xs = x + (int64_t)b * ld_slot + col;
    const float* ms = rowmax + (int64_t)b * ld_rowmax;
    // one frame: (xj, mj) = x[t][label(lane)] and m_t
    auto step = [&](int t, float xj, float mj) {
        float r = xj - mj;                                                 // NaN for a NaN entry and on a BREAK (mj NaN)
        r = r == r ? r : -INFINITY;
        const float a1 = lane_below(a), a2 = lane_below(a1);
        const int s1 = lane_below(start), s2 = lane_below(s1);
        float best = a;
        int from = start;
        if (!first && a1 > best) { best = a1; from = s1; }
        if (skip && a2 > best) { best = a2; from = s2; }
        if (first && 0.0f > best) { best = 0.0f; from = t; }
        if (!idle) { a = best + r; start = from; }
        const bool qualifies = last && a >= thr;                           // (false for a NaN)
        const bool emit = last && held && (!qualifies || start > held_end);
        const unsigned long long mask = __ballot(emit);
        if (emit) {
            const int at = count + __popcll(mask & below);
            if (at < max_detections) {
                int* row = det + (int64_t)at * 4;
                row[0] = kw; row[1] = held_start; row[2] = held_end; row[3] = __float_as_int(held_score);
            }
            held = 0;
        }
        count += __popcll(mask);
        if (qualifies && (!held || a >= held_score)) { held = 1; held_start = start; held_end = t; held_score = a; }
    };
    // Two register blocks of RING frames each, filled in turn: while the wave steps through one block, the gathers of the next are
    // in flight, all issued before the block's first step (slot u of a block holds the gather of its frame u, lane u of its m
    // the frame's row maximum: one load per block).  A row index is clamped to the slot's last row instead of branched around.
    float xa[RING], xb[RING], ma, mb;
    auto fill = [&](float (&xv)[RING], float& m, int base) {
#pragma unroll
        for (int u = 0; u < RING; ++u) xv[u] = xs[(int64_t)min(base + u, kb - 1) * ld_row];
        m = ms[min(base + (lane & (RING - 1)), kb - 1)];
    };
    auto row_max = [&](float m, int u) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), u)); };
    fill(xa, ma, 0);
    int base = 0;
    for (; base + 2 * RING <= kb; base += 2 * RING) {                      // whole pairs of blocks: no condition inside
        fill(xb, mb, base + RING);
#pragma unroll
        for (int u = 0; u < RING; ++u) step(F + base + u, xa[u], row_max(ma, u));
        fill(xa, ma, base + 2 * RING);
#pragma unroll
        for (int u = 0; u < RING; ++u) step(F + base + RING + u, xb[u], row_max(mb, u));
    }
    fill(xb, mb, base + RING);                                             // fewer than 2 RING frames are left
#pragma unroll
    for (int u = 0; u < RING; ++u)
        if (base + u < kb) step(F + base + u, xa[u], row_max(ma, u));      // (uniform)
#pragma unroll
    for (int u = 0; u < RING - 1; ++u)
        if (base + RING + u < kb) step(F + base + RING + u, xb[u], row_max(mb, u));
    st[0] = __float_as_int(a);
    st[LANES] = start;
    st[2 * LANES] = held; st[3 * LANES] = held_start; st[4 * LANES] = held_end; st[5 * LANES] = __float_as_int(held_score);
    if (lane == 0) {
        st[6 * LANES] = F + kb;
        counts[(int64_t)b * G + g] = count;
    }
}

bool layout_ok(int64_t ld_slot, int64_t ld_row, int64_t ld_rowmax, int k_max, int V) {
    return ld_row >= V && ld_slot >= 0 && ld_slot / ld_row >= k_max && ld_rowmax >= k_max;
}

}  // namespace

extern "C" int cfm3_kws_rowmax_f32(const float* x, int64_t ld_slot, int64_t ld_row, const int64_t* k, int k_max, int V,
                                   float* rowmax, int64_t ld_rowmax, int S, cfm_stream_t stream) {
    CFM_REQUIRE(k && rowmax && (x || k_max == 0), CFM_ERR_NULL);
    CFM_REQUIRE(S > 0 && k_max >= 0 && V >= 2, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(layout_ok(ld_slot, ld_row, ld_rowmax, k_max, V), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(V <= V_MAX && S <= 65535, CFM_ERR_UNSUPPORTED);
    if (k_max == 0) return CFM_OK;
    const dim3 grid((unsigned)((k_max + (int64_t)RM_WAVES - 1) / RM_WAVES), (unsigned)S);
    hipLaunchKernelGGL(kws_rowmax_kernel, grid, dim3(RM_WAVES * 64), 0, static_cast<hipStream_t>(stream), x, ld_slot, ld_row, k,
                       k_max, V, rowmax, ld_rowmax);
    return cfm_launch_status();
}

extern "C" int cfm3_kws_scan_f32(const float* x, int64_t ld_slot, int64_t ld_row, const float* rowmax, int64_t ld_rowmax,
                                 const int64_t* k, int k_max, int V, const int* lanes, const float* threshold, int G, int K,
                                 int* state, int* detections, int max_detections, int* counts, int S, cfm_stream_t stream) {
    CFM_REQUIRE(k && lanes && threshold && state && detections && counts && ((x && rowmax) || k_max == 0), CFM_ERR_NULL);
    CFM_REQUIRE(S > 0 && k_max >= 0 && V >= 2 && G >= 1 && K >= 1 && max_detections >= 1, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(K <= (int64_t)G * LANES, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(layout_ok(ld_slot, ld_row, ld_rowmax, k_max, V), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(V <= V_MAX && S <= 65535 && G <= G_MAX && max_detections <= DET_MAX, CFM_ERR_UNSUPPORTED);
    if (k_max == 0) return CFM_OK;
    hipLaunchKernelGGL(kws_scan_kernel, dim3((unsigned)G, (unsigned)S), dim3(64), 0, static_cast<hipStream_t>(stream), x, ld_slot,
                       ld_row, rowmax, ld_rowmax, k, k_max, V, lanes, threshold, G, K, state, detections, max_detections, counts);
    return cfm_launch_status();
}
