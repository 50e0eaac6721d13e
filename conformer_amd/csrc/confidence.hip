// Confidence (INTEGRATION.md "Confidence"): entropy-based frame confidence from the logits, its aggregation over the frames of a
// token or word, and the frame spans of the greedy decoder's tokens.  Semantics: include/conformer_hip_confidence.h.
//
// Frames: one wave per frame, as endpoint.hip classifies a frame: lane l takes x_l, x_{l+64}, ... in that order, for the maximum
// (with the lowest index that attains it), for the sum of exp(x - m) and for the method's own sum, and the 64 partials are folded
// by the xor butterfly, which gives every lane the same bits.  Up to V = 512 a lane holds its 8 values in registers, the row is
// read once and the next row's loads are issued before this row's arithmetic; beyond, the row is walked three times, 512 logits
// at a time (the 8 loads of a lane issued together; the row stays in cache between the passes).  A workgroup of 4 waves takes 16
// consecutive rows of one slot, 4 per wave (beyond 512: 4 rows, one per wave: a long row is work enough, and more waves hide its
// latency); grid: row blocks x slots, so a step of a few rows per slot is one workgroup per slot and an offline call of T rows
// spreads over T / 16 (T / 4) of them.  Every workgroup of a slot reads total[b] for the ring position, so total advances in a
// second one-thread-per-slot launch behind it.
// Spans: one wave per span over the ring.  Greedy spans: one wave per row, train_aux.hip's collapse scan with the positions kept.
// Every value read from the device that indexes anything is clamped first (k to [0, k_max], total to >= 0, n_spans to [0, L],
// the span to [0, total], lengths to [0, T], the argmax to [0, V)).
#include <math.h>
#include "cfm_common.h"
#include "../../include/conformer_hip_confidence.h"

namespace {

constexpr int V_MAX = 65536, EXCL_MAX = 8;
constexpr int WAVES = 4, THREADS = 64 * WAVES;
constexpr int rows_per_wg(bool reg) { return reg ? 4 * WAVES : WAVES; }  // rows held in registers: 4 per wave; walked: 1
constexpr int REG_VALUES = 8, REG_V = 64 * REG_VALUES;                   // a row of V <= 512 is held in registers

// the normalisers of a call, computed once on the host in double
struct Norm { float ln_v, den, inv_vm1; };

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_prod(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v *= __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the lane's candidate (best, bi) folded over the wave: the maximum and the lowest index that attains it (frame_argmax_kernel)
__device__ __forceinline__ int wave_argmax(float best, int bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    return bi;
}

// one term of the method's sum from a log-probability (MAX_PROB has none)
__device__ __forceinline__ float method_term(int method, float alpha, float lp) {
    if (method == CFM_CONFIDENCE_ENTROPY) {
        const float p = expf(lp);
        return p == 0.f ? 0.f : p * lp;                                   // (p = 0: lp may be -inf, and 0 * -inf is a NaN)
    }
    return expf(alpha * lp);
}

// the confidence from the row's maximum, lse and the folded method sum; the same in every lane of the wave
__device__ __forceinline__ float finish(int method, const Norm& nm, int V, float m, float lse, float acc) {
    float c;
    if (method == CFM_CONFIDENCE_MAX_PROB) c = ((float)V * expf(m - lse) - 1.f) * nm.inv_vm1;
    else if (method == CFM_CONFIDENCE_ENTROPY) c = 1.f + acc / nm.ln_v;
    else if (method == CFM_CONFIDENCE_TSALLIS) c = 1.f - (acc - 1.f) / nm.den;
    else c = 1.f + logf(acc) / nm.den;
    c = c < 0.f ? 0.f : c;                                                // (comparisons: a NaN passes both)
    c = c > 1.f ? 1.f : c;
    return c;
}

// the lane's values x_l, x_{l+64}, ... of the first REG_V logits of x, -inf behind V (which adds exp(-inf) = 0 to every sum)
__device__ __forceinline__ void load_row(const float* __restrict__ x, int V, int lane, float (&xv)[REG_VALUES]) {
#pragma unroll
    for (int j = 0; j < REG_VALUES; ++j) {
        const int v = lane + 64 * j;
        xv[j] = v < V ? x[v] : -INFINITY;
    }
}

// a frame of any V: three walks over the row, REG_V logits at a time, each chunk loaded whole and folded in the lane's order
// x_l, x_{l+64}, ... (the -inf behind V add 0 to a sum: no bit changes)
__device__ __forceinline__ float frame_confidence(const float* __restrict__ x, int V, int method, float alpha, const Norm& nm,
                                                  int lane, int& id) {
    float m = -INFINITY, best = -INFINITY;
    int bi = 0x7fffffff;
    float xv[REG_VALUES];
    for (int v0 = 0; v0 < V; v0 += REG_V) {
        load_row(x + v0, V - v0, lane, xv);
#pragma unroll
        for (int j = 0; j < REG_VALUES; ++j) {
            const int v = v0 + lane + 64 * j;
            m = fmaxf(m, xv[j]);                                          // (fmaxf drops a NaN; the sum below keeps it)
            if (v < V && (xv[j] > best || (xv[j] == best && v < bi))) { best = xv[j]; bi = v; }
        }
    }
    m = wave_max(m);
    id = wave_argmax(best, bi);
    float s = 0.f;
    for (int v0 = 0; v0 < V; v0 += REG_V) {
        load_row(x + v0, V - v0, lane, xv);
#pragma unroll
        for (int j = 0; j < REG_VALUES; ++j) s += expf(xv[j] - m);
    }
    s = wave_sum(s);
    const float lse = m + logf(s);
    float acc = 0.f;
    if (method != CFM_CONFIDENCE_MAX_PROB) {
        for (int v0 = 0; v0 < V; v0 += REG_V) {
            load_row(x + v0, V - v0, lane, xv);
#pragma unroll
            for (int j = 0; j < REG_VALUES; ++j) acc += method_term(method, alpha, xv[j] - lse);
        }
        acc = wave_sum(acc);
    }
    return finish(method, nm, V, m, lse, acc);
}

__device__ __forceinline__ float frame_confidence_reg(const float (&xv)[REG_VALUES], int V, int method, float alpha,
                                                      const Norm& nm, int lane, int& id) {
    float m = -INFINITY, best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < REG_VALUES; ++j) {
        const int v = lane + 64 * j;
        m = fmaxf(m, xv[j]);
        if (v < V && (xv[j] > best || (xv[j] == best && v < bi))) { best = xv[j]; bi = v; }
    }
    m = wave_max(m);
    id = wave_argmax(best, bi);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < REG_VALUES; ++j) s += expf(xv[j] - m);
    s = wave_sum(s);
    const float lse = m + logf(s);
    float acc = 0.f;
    if (method != CFM_CONFIDENCE_MAX_PROB) {
#pragma unroll
        for (int j = 0; j < REG_VALUES; ++j) acc += method_term(method, alpha, xv[j] - lse);
        acc = wave_sum(acc);
    }
    return finish(method, nm, V, m, lse, acc);
}

template <bool REG>
__global__ __launch_bounds__(THREADS) void confidence_frames_kernel(const float* __restrict__ logits, int64_t ld_slot,
                                                                    int64_t ld_row, const int64_t* __restrict__ k, int k_max,
                                                                    int V, int method, float alpha, Norm nm,
                                                                    float* __restrict__ conf, int64_t* __restrict__ ids,
                                                                    const int64_t* __restrict__ total, int R) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t kraw = k[b];
    const int kb = (int)(kraw < 0 ? 0 : kraw > k_max ? k_max : kraw);      // (uniform per workgroup)
    constexpr int ROWS = rows_per_wg(REG);
    const int r0 = blockIdx.x * ROWS + wave;                               // this wave's rows: r0, r0 + WAVES, ... below r_end
    const int r_end = min(kb, (int)(blockIdx.x + 1) * ROWS);               // (k_max <= 2^30: no overflow)
    if (r0 >= r_end) return;
    const int64_t traw = total[b];
    const int base = (int)((traw < 0 ? 0 : traw) % R);                     // ring position of row 0, in [0, R)
    const float* slot = logits + (int64_t)b * ld_slot;
    float* conf_b = conf + (int64_t)b * R;
    int64_t* ids_b = ids + (int64_t)b * R;
    if (REG) {
        float cur[REG_VALUES], nxt[REG_VALUES];
        load_row(slot + (int64_t)r0 * ld_row, V, lane, cur);
        for (int r = r0; r < r_end; r += WAVES) {
            const bool more = r + WAVES < r_end;                           // (uniform per wave)
            if (more) load_row(slot + (int64_t)(r + WAVES) * ld_row, V, lane, nxt);
            int id;
            const float c = frame_confidence_reg(cur, V, method, alpha, nm, lane, id);
            if (lane == 0) {
                const int pos = (int)(((int64_t)base + r) % R);
                conf_b[pos] = c;
                ids_b[pos] = min(max(id, 0), V - 1);
            }
#pragma unroll
            for (int j = 0; j < REG_VALUES; ++j) cur[j] = more ? nxt[j] : cur[j];
        }
    } else {
        for (int r = r0; r < r_end; r += WAVES) {
            int id;
            const float c = frame_confidence(slot + (int64_t)r * ld_row, V, method, alpha, nm, lane, id);
            if (lane == 0) {
                const int pos = (int)(((int64_t)base + r) % R);
                conf_b[pos] = c;
                ids_b[pos] = min(max(id, 0), V - 1);
            }
        }
    }
}

__global__ __launch_bounds__(256) void confidence_advance_kernel(const int64_t* __restrict__ k, int k_max,
                                                                 int64_t* __restrict__ total, int S) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= S) return;
    const int64_t kraw = k[b];
    const int64_t kb = kraw < 0 ? 0 : kraw > k_max ? k_max : kraw;
    if (kb > 0) total[b] += kb;                                            // (a slot with k = 0 is not touched)
}

// One wave per span.  Both folds run side by side, over the frames that count and over all of them: which one holds is known
// only once the span has been read.
__global__ __launch_bounds__(THREADS) void confidence_spans_kernel(const float* __restrict__ conf, const int64_t* __restrict__ ids,
                                                                   const int64_t* __restrict__ total, int R,
                                                                   const int64_t* __restrict__ starts,
                                                                   const int64_t* __restrict__ ends,
                                                                   const int64_t* __restrict__ n_spans, int L, int agg,
                                                                   const int* __restrict__ exclude_ids, int n_excl,
                                                                   float* __restrict__ out, int64_t spans) {
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);  // (uniform per wave)
    if (idx >= spans) return;
    const int b = (int)(idx / L), j = (int)(idx % L);
    const int64_t nraw = n_spans[b], traw = total[b];
    const int64_t n = nraw < 0 ? 0 : nraw > L ? L : nraw, tot = traw < 0 ? 0 : traw;
    int64_t st = starts[idx], en = ends[idx];
    st = st < 0 ? 0 : st > tot ? tot : st;
    en = en < 0 ? 0 : en > tot ? tot : en;
    if (j >= n || en <= st || st < tot - R) {                              // (so en - st <= R: every frame is still in the ring)
        if (lane == 0) out[idx] = NAN;
        return;
    }
    int64_t excl[EXCL_MAX];
#pragma unroll
    for (int i = 0; i < EXCL_MAX; ++i) excl[i] = i < n_excl ? (int64_t)exclude_ids[i] : 0;
    const float unit = agg == CFM_CONFIDENCE_MIN ? INFINITY : agg == CFM_CONFIDENCE_MAX ? -INFINITY
                     : agg == CFM_CONFIDENCE_PROD ? 1.f : 0.f;
    const float* conf_b = conf + (int64_t)b * R;
    const int64_t* ids_b = ids + (int64_t)b * R;
    float kept = unit, all = unit;
    int n_kept = 0;
    bool bad = false;
    for (int64_t t = st + lane; t < en; t += 64) {
        const int pos = (int)(t % R);
        const float c = conf_b[pos];
        const int64_t id = ids_b[pos];
        bool counts = true;
#pragma unroll
        for (int i = 0; i < EXCL_MAX; ++i) counts = counts && !(i < n_excl && id == excl[i]);
        bad = bad || c != c;
        if (agg == CFM_CONFIDENCE_MIN) { all = fminf(all, c); if (counts) kept = fminf(kept, c); }
        else if (agg == CFM_CONFIDENCE_MAX) { all = fmaxf(all, c); if (counts) kept = fmaxf(kept, c); }
        else if (agg == CFM_CONFIDENCE_PROD) { all *= c; if (counts) kept *= c; }
        else { all += c; if (counts) kept += c; }
        n_kept += counts ? 1 : 0;
    }
    n_kept = wave_sum_int(n_kept);
    float v = n_kept > 0 ? kept : all;                                     // (uniform per wave)
    const int count = n_kept > 0 ? n_kept : (int)(en - st);
    if (agg == CFM_CONFIDENCE_MIN) v = wave_min(v);
    else if (agg == CFM_CONFIDENCE_MAX) v = wave_max(v);
    else if (agg == CFM_CONFIDENCE_PROD) v = wave_prod(v);
    else v = wave_sum(v) / (float)count;
    if (__ballot(bad)) v = NAN;
    if (lane == 0) out[idx] = v;
}

// ctc_collapse_kernel (train_aux.hip) with the frame of every kept token written instead of its id
__global__ __launch_bounds__(64) void confidence_greedy_spans_kernel(const int64_t* __restrict__ frame_ids,
                                                                     const int64_t* __restrict__ lengths,
                                                                     int64_t* __restrict__ token_start,
                                                                     int64_t* __restrict__ token_end, int T, int pad_id,
                                                                     int unk_id) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t* ids = frame_ids + (int64_t)b * T;
    int64_t* ts = token_start + (int64_t)b * T;
    int64_t* te = token_end + (int64_t)b * T;
    const int n = lengths ? (int)min((int64_t)T, max((int64_t)0, lengths[b])) : T;
    int cnt = 0;
    int64_t carry = -1;                                   // id of the last non-skipped frame so far (-1: none yet)
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane;
        const int64_t id = t < n ? ids[t] : -1;
        const bool valid = t < n && id != pad_id && id != unk_id;
        const unsigned long long vm = __ballot(valid);
        const unsigned long long below = vm & ((1ull << lane) - 1ull);
        const int src = below ? 63 - __clzll(below) : 0;
        const int64_t prev_in = __shfl(id, src, 64);
        const int64_t prev = below ? prev_in : carry;
        const bool keep = valid && id != prev;
        const unsigned long long km = __ballot(keep);
        if (keep) {
            const int p = cnt + __popcll(km & ((1ull << lane) - 1ull));    // < T: at most one token per frame
            ts[p] = t;
            if (p > 0) te[p - 1] = t;
        }
        cnt += __popcll(km);
        if (vm) carry = __shfl(id, 63 - __clzll(vm), 64);
    }
    if (lane == 0 && cnt > 0) te[cnt - 1] = n;            // (no kept frame writes the last token's end)
    for (int t = cnt + lane; t < T; t += 64) ts[t] = te[t] = -1;
}

bool alpha_ok(float a) { return (a >= 0.0625f && a <= 0.9375f) || (a >= 1.0625f && a <= 8.f); }

}  // namespace

extern "C" int cfm_confidence_frames_f32(const float* logits, int64_t ld_slot, int64_t ld_row, const int64_t* k, int k_max, int V,
                                         int method, float alpha, float* conf, int64_t* ids, int64_t* total, int R, int S,
                                         cfm_stream_t stream) {
    CFM_REQUIRE(k && conf && ids && total && (logits || k_max == 0), CFM_ERR_NULL);
    CFM_REQUIRE(S > 0 && k_max >= 0 && R >= 1 && k_max <= R && V >= 2, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(method >= CFM_CONFIDENCE_MAX_PROB && method <= CFM_CONFIDENCE_RENYI, CFM_ERR_BAD_SHAPE);
    const bool parametric = method == CFM_CONFIDENCE_TSALLIS || method == CFM_CONFIDENCE_RENYI;
    CFM_REQUIRE(!parametric || alpha_ok(alpha), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(ld_row >= V && ld_slot >= 0 && (k_max == 0 || ld_slot / k_max >= ld_row), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(S < 65535 && V <= V_MAX && k_max <= (1 << 30), CFM_ERR_UNSUPPORTED);
    if (k_max == 0) return CFM_OK;
    const double ln_v = log((double)V), a = parametric ? (double)alpha : 2.0;
    Norm nm;
    nm.ln_v = (float)ln_v;
    nm.den = (float)(method == CFM_CONFIDENCE_TSALLIS ? expm1((1.0 - a) * ln_v) : (a - 1.0) * ln_v);
    nm.inv_vm1 = (float)(1.0 / (V - 1.0));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rows = rows_per_wg(V <= REG_V);
    const dim3 grid((unsigned)((k_max + rows - 1) / rows), (unsigned)S);
    if (V <= REG_V)
        hipLaunchKernelGGL(confidence_frames_kernel<true>, grid, dim3(THREADS), 0, s, logits, ld_slot, ld_row, k, k_max, V,
                           method, alpha, nm, conf, ids, total, R);
    else
        hipLaunchKernelGGL(confidence_frames_kernel<false>, grid, dim3(THREADS), 0, s, logits, ld_slot, ld_row, k, k_max, V,
                           method, alpha, nm, conf, ids, total, R);
    hipLaunchKernelGGL(confidence_advance_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, k, k_max, total, S);
    return cfm_launch_status();
}

extern "C" int cfm_confidence_spans_f32(const float* conf, const int64_t* ids, const int64_t* total, int R, const int64_t* starts,
                                        const int64_t* ends, const int64_t* n_spans, int L, int aggregation,
                                        const int* exclude_ids, int n_exclude, float* out, int S, cfm_stream_t stream) {
    CFM_REQUIRE(conf && ids && total && starts && ends && n_spans && out, CFM_ERR_NULL);
    CFM_REQUIRE(S > 0 && L >= 0 && R >= 1 && n_exclude >= 0 && n_exclude <= EXCL_MAX, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(aggregation >= CFM_CONFIDENCE_MEAN && aggregation <= CFM_CONFIDENCE_PROD, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(exclude_ids || n_exclude == 0, CFM_ERR_NULL);
    const int64_t spans = (int64_t)S * L;
    CFM_REQUIRE(spans < ((int64_t)1 << 31), CFM_ERR_UNSUPPORTED);
    if (L == 0) return CFM_OK;
    hipLaunchKernelGGL(confidence_spans_kernel, dim3((unsigned)((spans + WAVES - 1) / WAVES)), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), conf, ids, total, R, starts, ends, n_spans, L, aggregation, exclude_ids,
                       n_exclude, out, spans);
    return cfm_launch_status();
}

extern "C" int cfm_confidence_greedy_spans_i64(const int64_t* frame_ids, const int64_t* lengths_or_null, int64_t* token_start,
                                               int64_t* token_end, int B, int T, int pad_id, int unk_id, cfm_stream_t stream) {
    CFM_REQUIRE(frame_ids && token_start && token_end, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && T > 0, CFM_ERR_BAD_SHAPE);
    hipLaunchKernelGGL(confidence_greedy_spans_kernel, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream), frame_ids,
                       lengths_or_null, token_start, token_end, T, pad_id, unk_id);
    return cfm_launch_status();
}
