// Error rates on the device (INTEGRATION.md "Error rates on the device"): token rows -> unit streams -> Levenshtein distances.
//
// units_kernel: one workgroup of 256 threads per token row.  The row is walked 256 tokens at a time.  A first block scan gives
// every token the index of the last spelling token and of the last delimiter in front of it, which decide whether the token opens
// a word and whether a U+0020 goes in front of it; a second one (three counts packed into 64 bits) gives the offsets of its code
// points, its word and its token unit.  After the walk one thread per word closes the span and hashes it (FNV-1a, 32 bit).
//
// distance_kernel: one wave per (hypothesis, reference, kind).  Lane l owns KC consecutive columns (hypothesis units) of a strip
// of 64 KC columns and takes reference row s - l at step s: the wave sweeps an anti-diagonal band down the strip.  What a lane
// needs from outside its columns is D[i][first - 1], which lane l - 1 produced one step earlier: one lane shift (a DPP row shift,
// patched across the three row seams) per step, and the reference unit travels the same way.  Lane 0 takes the reference units
// and, behind the first strip, the previous strip's last column 64 rows at a time into a register and picks them with readlane.
// Nothing inside a strip waits on a barrier or on memory latency that the batch load has not covered.  The previous strip's last
// column lives in LDS, 4 bytes per reference unit; lane 63 overwrites entry i 63 steps after lane 0 read it.  A word matches when
// its hash, its length and then its code points match.
// Every length and id read from the device that indexes anything is clamped first.
#include "cfm_common.h"
#include "../../include/conformer_hip_error_rate.h"

namespace {

constexpr int CAP = 16384;                              // units per side and kind
constexpr int TOK_CHARS = 0, TOK_DELIM = 1, TOK_SKIP = 2;
constexpr int UTHREADS = 256, UWAVES = UTHREADS / 64;
constexpr int KC = 8, STRIP = 64 * KC;
constexpr int UNIT_WORD = 0, UNIT_CHAR = 1, UNIT_TOKEN = 2, UNIT_ALL = 3;

// ---- unit extraction ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_incl_max(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v = max(v, u);
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_incl_sum(unsigned long long v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ __launch_bounds__(UTHREADS) void units_kernel(const int64_t* __restrict__ ids, int64_t ld_ids,
                                                         const int64_t* __restrict__ counts, int L,
                                                         const int* __restrict__ tok_kind, const int* __restrict__ tok_off,
                                                         const int* __restrict__ tok_cp, int V, int* __restrict__ cps, int ld_cps,
                                                         int* __restrict__ words, int ld_words, int* __restrict__ toks, int ld_toks,
                                                         int* __restrict__ lens) {
    __shared__ int w_s[UWAVES], w_d[UWAVES];
    __shared__ unsigned long long w_sum[UWAVES];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t craw = counts[row];
    const int cnt = (int)(craw < 0 ? 0 : craw > L ? L : craw);               // (uniform per workgroup)
    const int64_t* rid = ids + (int64_t)row * ld_ids;
    int* rcps = cps + (int64_t)row * ld_cps;
    int* rwords = words + (int64_t)row * ld_words * 4;
    int* rtoks = toks + (int64_t)row * ld_toks;
    int carry_s = -1, carry_d = -1;                                          // the last spelling token / delimiter so far
    int n_cp = 0, n_w = 0, n_t = 0;
    for (int base = 0; base < cnt; base += UTHREADS) {
        const int i = base + tid;
        int id = -1, kind = TOK_SKIP, c0 = 0, ncp = 0;
        if (i < cnt) {
            const int64_t raw = rid[i];
            if (raw >= 0 && raw < V) {
                id = (int)raw;
                kind = tok_kind[id];
                if (kind == TOK_CHARS) {
                    c0 = tok_off[id];
                    ncp = max(tok_off[id + 1] - c0, 0);
                } else if (kind != TOK_DELIM) {
                    kind = TOK_SKIP;
                }
            }
        }
        const bool spells = ncp > 0, delim = kind == TOK_DELIM;
        // scan 1: the last spelling token and the last delimiter at or in front of i
        int ls = wave_incl_max(spells ? i : -1, lane), ldl = wave_incl_max(delim ? i : -1, lane);
        __syncthreads();                                                     // (the previous tile's reads of w_* are done)
        if (lane == 63) { w_s[wave] = ls; w_d[wave] = ldl; }
        __syncthreads();
        int ps = carry_s, pd = carry_d, ts = carry_s, td = carry_d;          // p*: in front of this wave; t*: the whole tile
#pragma unroll
        for (int w = 0; w < UWAVES; ++w) {
            if (w < wave) { ps = max(ps, w_s[w]); pd = max(pd, w_d[w]); }
            ts = max(ts, w_s[w]); td = max(td, w_d[w]);
        }
        // exclusive: what lies strictly in front of i
        int ex_s = __shfl_up(ls, 1, 64), ex_d = __shfl_up(ldl, 1, 64);
        if (lane == 0) { ex_s = -1; ex_d = -1; }
        ex_s = max(ex_s, ps);
        ex_d = max(ex_d, pd);
        const bool opens = spells && (ex_s < 0 || ex_d > ex_s);
        const bool space = opens && ex_s >= 0;
        // scan 2: code points (with the space), words, token units in front of i
        const unsigned long long mine = (unsigned long long)(ncp + (space ? 1 : 0)) | ((unsigned long long)(opens ? 1 : 0) << 21)
                                        | ((unsigned long long)(kind != TOK_SKIP ? 1 : 0) << 42);
        const unsigned long long incl = wave_incl_sum(mine, lane);
        if (lane == 63) w_sum[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, tile = 0;
#pragma unroll
        for (int w = 0; w < UWAVES; ++w) {
            if (w < wave) before += w_sum[w];
            tile += w_sum[w];
        }
        const unsigned long long ex = before + incl - mine;
        const int o_cp = n_cp + (int)(ex & 0x1fffff), o_w = n_w + (int)((ex >> 21) & 0x1fffff), o_t = n_t + (int)(ex >> 42);
        if (kind != TOK_SKIP && o_t < ld_toks) rtoks[o_t] = id;
        if (spells) {
            if (space && o_cp < ld_cps) rcps[o_cp] = 0x20;
            const int at = o_cp + (space ? 1 : 0);
            for (int q = 0; q < ncp; ++q)
                if (at + q < ld_cps) rcps[at + q] = tok_cp[c0 + q];
            if (opens && o_w < ld_words) rwords[o_w * 4] = at;
        }
        carry_s = ts; carry_d = td;
        n_cp += (int)(tile & 0x1fffff); n_w += (int)((tile >> 21) & 0x1fffff); n_t += (int)(tile >> 42);
    }
    n_cp = min(n_cp, ld_cps); n_w = min(n_w, ld_words); n_t = min(n_t, ld_toks);
    __syncthreads();                                                         // the starts and code points are written
    for (int w = tid; w < n_w; w += UTHREADS) {
        const int start = min(rwords[w * 4], n_cp);
        const int end = w + 1 < n_w ? min(max(rwords[(w + 1) * 4] - 1, start), n_cp) : n_cp;
        unsigned h = 2166136261u;
        for (int q = start; q < end; ++q) h = (h ^ (unsigned)rcps[q]) * 16777619u;
        rwords[w * 4 + 1] = end - start;
        rwords[w * 4 + 2] = (int)h;
        rwords[w * 4 + 3] = 0;
    }
    if (tid == 0) {
        int* o = lens + (int64_t)row * 4;
        o[0] = n_cp; o[1] = n_w; o[2] = n_t; o[3] = 0;
    }
}

// ---- batched edit distance ------------------------------------------------------------------------------------------------------
// lane l takes lane l - 1's value, lane 0 keeps its own: a DPP shift by one inside each row of 16 lanes, patched at the three seams
__device__ __forceinline__ int lane_shr1(int v, int lane) {
    int r = __builtin_amdgcn_update_dpp(v, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
    const int a = __builtin_amdgcn_readlane(v, 15), b = __builtin_amdgcn_readlane(v, 31), c = __builtin_amdgcn_readlane(v, 47);
    r = lane == 16 ? a : r;
    r = lane == 32 ? b : r;
    r = lane == 48 ? c : r;
    return r;
}

struct Side {
    const int* units;       // WORD: (len, 4) {start, length, hash, 0}; else (len) int
    const int* cps;         // WORD: the row's code points
    int len, n_cps;
};

__device__ __forceinline__ bool same_word(const Side& r, int rs, int rl, const Side& h, int hs, int hl) {
    if (rl != hl || rl <= 0 || rs < 0 || hs < 0 || rs + rl > r.n_cps || hs + hl > h.n_cps) return false;
    for (int q = 0; q < rl; ++q)
        if (r.cps[rs + q] != h.cps[hs + q]) return false;
    return true;
}

template <bool WORD>
__device__ int strip_distance(const Side& ref, const Side& hyp, int* __restrict__ edge, int lane) {
    const int m = ref.len, n = hyp.len;
    if (m == 0) return n;
    if (n == 0) return m;
    const int passes = (n + STRIP - 1) / STRIP, steps = m + 63;
    int result = 0;
    for (int p = 0; p < passes; ++p) {
        const int first = p * STRIP + lane * KC;
        const bool last = p == passes - 1;
        int hk[KC], hs[KC], hl[KC], d[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const int j = first + k;
            hs[k] = 0; hl[k] = -1;
            if (WORD) {
                hk[k] = 0;
                if (j < n) { hs[k] = hyp.units[j * 4]; hl[k] = hyp.units[j * 4 + 1]; hk[k] = hyp.units[j * 4 + 2]; }
            } else {
                hk[k] = j < n ? hyp.units[j] : -1;
            }
            d[k] = j + 1;                                                    // D[0][j + 1]
        }
        int prev_left = first;                                               // D[i - 1][first], for i = 1
        int rk = 0, rs = 0, rl = 0;
        for (int s0 = 1; s0 <= steps; s0 += 64) {
            // rows s0 .. s0 + 63 for lane 0: the reference units, and D[row][p STRIP] from the strip before
            const int row = s0 + lane;
            int bk = 0, bs = 0, bl = 0, be = 0;
            if (row <= m) {
                if (WORD) { bs = ref.units[(row - 1) * 4]; bl = ref.units[(row - 1) * 4 + 1]; bk = ref.units[(row - 1) * 4 + 2]; }
                else bk = ref.units[row - 1];
                if (p > 0) be = edge[row - 1];
            }
            const int tmax = min(64, steps - s0 + 1);
            for (int t = 0; t < tmax; ++t) {
                const int s = s0 + t, i = s - lane;                          // lane l works on row i
                const int nk = __builtin_amdgcn_readlane(bk, t);
                rk = lane_shr1(rk, lane);
                rk = lane == 0 ? nk : rk;
                if (WORD) {
                    const int ns = __builtin_amdgcn_readlane(bs, t), nl = __builtin_amdgcn_readlane(bl, t);
                    rs = lane_shr1(rs, lane); rl = lane_shr1(rl, lane);
                    rs = lane == 0 ? ns : rs; rl = lane == 0 ? nl : rl;
                }
                int left = lane_shr1(d[KC - 1], lane);                       // D[i][first] of lane l - 1, from its last step
                const int e = __builtin_amdgcn_readlane(be, t);
                if (lane == 0) left = p == 0 ? s : e;
                const bool active = i >= 1 && i <= m;
                int diag = prev_left, lv = left;
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    bool eq = rk == hk[k];
                    if (WORD) eq = eq && same_word(ref, rs, rl, hyp, hs[k], hl[k]);
                    const int v = min(min(d[k], lv) + 1, diag + (eq ? 0 : 1));
                    diag = d[k];
                    d[k] = active ? v : d[k];
                    lv = v;
                }
                prev_left = active ? left : prev_left;
                if (!last && lane == 63 && active) edge[i - 1] = d[KC - 1];
            }
        }
        if (last) {
            const int idx = n - 1 - p * STRIP;                               // 0 .. STRIP-1
            int mine = 0;
#pragma unroll
            for (int k = 0; k < KC; ++k) mine = (idx % KC) == k ? d[k] : mine;
            result = __shfl(mine, idx / KC, 64);
        }
        __syncthreads();                                                     // one wave: orders the edge column between strips
    }
    return result;
}

struct DistanceArgs {
    const int *ref_cps, *ref_words, *ref_toks, *ref_lens, *hyp_cps, *hyp_words, *hyp_toks, *hyp_lens;
    int ld_ref_cps, ld_ref_words, ld_ref_toks, ld_hyp_cps, ld_hyp_words, ld_hyp_toks;
    int B, N, unit;
    int *errors, *hyp_units, *ref_units;
};

__device__ __forceinline__ int clamp_len(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

__global__ __launch_bounds__(64) void distance_kernel(const DistanceArgs a) {
    extern __shared__ int edge[];
    const int n = blockIdx.x, b = blockIdx.y, plane = blockIdx.z, lane = threadIdx.x;
    const int kind = a.unit == UNIT_ALL ? plane : a.unit;
    const int64_t hr = (int64_t)b * a.N + n;
    const int* rl = a.ref_lens + (int64_t)b * 4;
    const int* hl = a.hyp_lens + hr * 4;
    Side ref, hyp;
    int dist;
    if (kind == UNIT_WORD) {
        ref = {a.ref_words + (int64_t)b * a.ld_ref_words * 4, a.ref_cps + (int64_t)b * a.ld_ref_cps,
               clamp_len(rl[1], a.ld_ref_words), clamp_len(rl[0], a.ld_ref_cps)};
        hyp = {a.hyp_words + hr * a.ld_hyp_words * 4, a.hyp_cps + hr * a.ld_hyp_cps, clamp_len(hl[1], a.ld_hyp_words),
               clamp_len(hl[0], a.ld_hyp_cps)};
        dist = strip_distance<true>(ref, hyp, edge, lane);
    } else if (kind == UNIT_CHAR) {
        ref = {a.ref_cps + (int64_t)b * a.ld_ref_cps, nullptr, clamp_len(rl[0], a.ld_ref_cps), 0};
        hyp = {a.hyp_cps + hr * a.ld_hyp_cps, nullptr, clamp_len(hl[0], a.ld_hyp_cps), 0};
        dist = strip_distance<false>(ref, hyp, edge, lane);
    } else {
        ref = {a.ref_toks + (int64_t)b * a.ld_ref_toks, nullptr, clamp_len(rl[2], a.ld_ref_toks), 0};
        hyp = {a.hyp_toks + hr * a.ld_hyp_toks, nullptr, clamp_len(hl[2], a.ld_hyp_toks), 0};
        dist = strip_distance<false>(ref, hyp, edge, lane);
    }
    if (lane == 0) {
        const int64_t o = (int64_t)plane * a.B * a.N + hr;
        a.errors[o] = dist;
        a.hyp_units[o] = hyp.len;
        if (n == 0) a.ref_units[(int64_t)plane * a.B + b] = ref.len;
    }
}

}  // namespace

extern "C" int cfm_error_rate_units(const int64_t* ids, int64_t ld_ids, const int64_t* counts, int R, int L, const int* tok_kind,
                                    const int* tok_off, const int* tok_cp, int V, int max_token_cps, int* cps, int64_t ld_cps,
                                    int* words, int64_t ld_words, int* toks, int64_t ld_toks, int* lens, cfm_stream_t stream) {
    CFM_REQUIRE(ids && counts && tok_kind && tok_off && cps && words && toks && lens && (tok_cp || max_token_cps == 0),
                CFM_ERR_NULL);
    CFM_REQUIRE(R > 0 && L > 0 && V > 0 && max_token_cps >= 0, CFM_ERR_BAD_SHAPE);
    const int64_t need = (int64_t)L * (max_token_cps > 1 ? max_token_cps : 1);
    CFM_REQUIRE(ld_ids >= L && ld_toks >= L && ld_words >= L && ld_cps >= need, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(need <= CAP, CFM_ERR_UNSUPPORTED);
    const int big = 0x7fffffff;                                              // the kernel's bound checks are 32-bit
    hipLaunchKernelGGL(units_kernel, dim3((unsigned)R), dim3(UTHREADS), 0, static_cast<hipStream_t>(stream), ids, ld_ids, counts,
                       L, tok_kind, tok_off, tok_cp, V, cps, (int)(ld_cps > big ? big : ld_cps), words,
                       (int)(ld_words > big ? big : ld_words), toks, (int)(ld_toks > big ? big : ld_toks), lens);
    return cfm_launch_status();
}

extern "C" int cfm_error_rate_distance(const int* ref_cps, int64_t ld_ref_cps, const int* ref_words, int64_t ld_ref_words,
                                       const int* ref_toks, int64_t ld_ref_toks, const int* ref_lens, const int* hyp_cps,
                                       int64_t ld_hyp_cps, const int* hyp_words, int64_t ld_hyp_words, const int* hyp_toks,
                                       int64_t ld_hyp_toks, const int* hyp_lens, int B, int N, int unit, int* errors,
                                       int* hyp_units, int* ref_units, cfm_stream_t stream) {
    CFM_REQUIRE(unit >= 0 && unit <= UNIT_ALL, CFM_ERR_BAD_SHAPE);
    const bool use_cps = unit != UNIT_TOKEN, use_words = unit == UNIT_WORD || unit == UNIT_ALL;
    const bool use_toks = unit == UNIT_TOKEN || unit == UNIT_ALL;
    CFM_REQUIRE(errors && hyp_units && ref_units && ref_lens && hyp_lens, CFM_ERR_NULL);
    CFM_REQUIRE((!use_cps || (ref_cps && hyp_cps)) && (!use_words || (ref_words && hyp_words))
                && (!use_toks || (ref_toks && hyp_toks)), CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && N > 0, CFM_ERR_BAD_SHAPE);
    // the leading dimensions of the kinds in use: positive, within the cap; their maxima size the edge column between strips
    int64_t ref_max = 0, hyp_max = 0, ld_min = CAP;
    const auto use = [&](bool on, int64_t ld_ref, int64_t ld_hyp) {
        if (!on) return;
        ref_max = ld_ref > ref_max ? ld_ref : ref_max;
        hyp_max = ld_hyp > hyp_max ? ld_hyp : hyp_max;
        ld_min = ld_ref < ld_min ? ld_ref : ld_min;
        ld_min = ld_hyp < ld_min ? ld_hyp : ld_min;
    };
    use(use_cps, ld_ref_cps, ld_hyp_cps);
    use(use_words, ld_ref_words, ld_hyp_words);
    use(use_toks, ld_ref_toks, ld_hyp_toks);
    CFM_REQUIRE(ld_min > 0, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(ref_max <= CAP && hyp_max <= CAP && N <= 65535 && B <= 65535, CFM_ERR_UNSUPPORTED);
    // (a hypothesis of any kind in use may exceed one strip: one int per reference unit)
    const size_t lds = hyp_max > STRIP ? (size_t)ref_max * sizeof(int) : 0;  // <= 64 KiB by the cap
    DistanceArgs a;
    a.ref_cps = ref_cps; a.ref_words = ref_words; a.ref_toks = ref_toks; a.ref_lens = ref_lens;
    a.hyp_cps = hyp_cps; a.hyp_words = hyp_words; a.hyp_toks = hyp_toks; a.hyp_lens = hyp_lens;
    a.ld_ref_cps = (int)ld_ref_cps; a.ld_ref_words = (int)ld_ref_words; a.ld_ref_toks = (int)ld_ref_toks;
    a.ld_hyp_cps = (int)ld_hyp_cps; a.ld_hyp_words = (int)ld_hyp_words; a.ld_hyp_toks = (int)ld_hyp_toks;
    a.B = B; a.N = N; a.unit = unit;
    a.errors = errors; a.hyp_units = hyp_units; a.ref_units = ref_units;
    hipLaunchKernelGGL(distance_kernel, dim3((unsigned)N, (unsigned)B, unit == UNIT_ALL ? 3u : 1u), dim3(64), lds,
                       static_cast<hipStream_t>(stream), a);
    return cfm_launch_status();
}
