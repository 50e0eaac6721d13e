// CTC forced alignment (INTEGRATION.md "Forced alignment"): the max-product (Viterbi) recursion over the 2L+1 state
// lattice the loss walks (ctc.hip), with back-pointers, the back-trace and per-token / per-utterance scores.
//
//   chain  : a thread owns P consecutive (blank, label) state pairs in registers, as ctc_chain_kernel does, so a time step
//            needs ONE cross-lane value (the label state left of the thread's first pair).  One wave per utterance up to
//            L = 1023 (P = 1..16); beyond that one WORKGROUP per utterance with P = 8: the value crosses a wave boundary
//            through a double-buffered LDS word, one barrier per frame.  The recursion runs on the RAW logits (the
//            per-frame normaliser shifts all paths alike), gathered straight from the logits row a block of steps ahead:
//            no emission matrix is written.  The lattice is re-centred on its own maximum (exact on grid inputs; the
//            offset is never needed again: scores are recomputed from the path).  Each step stores the moves (0 stay,
//            1 advance, 2 skip) of the thread's 2P states, 2 bits each: state s at bits 2*(s%4) of byte s/4 of the row.
//   trace  : one wave per utterance walks the moves backwards in windows of 64 frames: a window can lower the state by at
//            most 126, so its moves are a 64 x (<= 9 dword) patch, loaded one row per lane into LDS and walked there
//            (a chain of T dependent global loads otherwise).  Writes frame_tokens / frame_index and their padding.
//   frames : one wave per frame: float64 log-sum-exp of the row (as beam_prep_kernel) -> log-probability of the emitted symbol.
//   spans  : one workgroup per utterance: run boundaries of frame_index -> token_start / token_end (each token has one
//            run, so every element has one writer: no atomics), a wave per token for the mean, a fixed-order float64
//            reduction for the utterance score.
// Latency-bound on the T sequential steps, like the loss; nothing synchronises with the host and nothing is allocated.
//
//   long   : the chain for recordings beyond one workgroup's registers (conformer_hip2_align_long.h), further down: the
//            lattice in cells of tile_pairs x chunk_frames, one workgroup per cell, an anti-diagonal of cells per launch,
//            float64 state.  It writes the same moves rows, so trace, frames and spans above serve it unchanged.
//
//   wild   : wildcard target positions (conformer_hip3_align_wild.h): the WILD instantiations of the kernels here.  A frame
//            pass writes w[t] = row maximum - penalty; a wildcard is the label V of the logits with that column appended,
//            which are never built: the chains select between the gathered logit and w[t].  WILD = false is the plain code.
#include "cfm_common.h"
#include "conformer_hip2_align_long.h"
#include "conformer_hip3_align_wild.h"

namespace {

struct AlignArgs {
    const float* logits; const int64_t* targets; const int64_t* in_len; const int64_t* tgt_len;
    const float* wild;               // (B, T) what a wildcard emits: row maximum - penalty (the WILD forms only)
    unsigned char* moves;            // (B, T, row_bytes)
    double* frame_lp;                // (B, T) log-probability of the emitted symbol
    int* end_state;                  // (B) last state of the path, -1: infeasible
    int64_t* frame_tokens; int64_t* frame_index; int64_t* token_start; int64_t* token_end;
    float* token_score; double* score; unsigned char* ok;
    int64_t tgt_numel;
    int B, T, V, Lmax, blank, P, threads, row_bytes;
    float penalty;                   // wildcard_penalty (the WILD forms only)
};

constexpr float NEG_INF = -__builtin_inff();

// utterance geometry, clamped so that no index derived from it can leave a buffer (ctc_geometry of ctc.hip, padded targets)
__device__ __forceinline__ void align_geometry(const AlignArgs& a, int b, int& Tb, int& Lb, int64_t& off) {
    off = (int64_t)b * a.Lmax;
    off = off > a.tgt_numel ? a.tgt_numel : off;
    int64_t L = a.tgt_len ? a.tgt_len[b] : a.Lmax;
    L = L < 0 ? 0 : L;
    L = L > a.Lmax ? a.Lmax : L;
    L = L > a.tgt_numel - off ? a.tgt_numel - off : L;
    Lb = (int)L;
    const int64_t t = a.in_len ? a.in_len[b] : a.T;
    Tb = (int)(t < 0 ? 0 : (t > a.T ? a.T : t));
}
__device__ __forceinline__ int align_label(const AlignArgs& a, int64_t off, int i) {
    const int64_t v = a.targets[off + i];
    return (int)(v < 0 ? 0 : (v >= a.V ? a.V - 1 : v));
}
// WILD (conformer_hip3_align_wild.h): a wildcard is the label V, the column the definition appends; one more label value
// to `hop`, the repeats and the feasibility test
template <bool WILD> __device__ __forceinline__ int align_label_w(const AlignArgs& a, int64_t off, int i) {
    if (WILD && a.targets[off + i] == CFM3_CTC_ALIGN_WILDCARD) return a.V;
    return align_label(a, off, i);
}

template <int P> struct MoveStore;       // the 4P move bits of a thread -> its P/2 bytes of the row
template <> struct MoveStore<1> {
    static __device__ __forceinline__ void put(unsigned char* row, int tid, unsigned long long bits) {
        const unsigned other = __shfl_down((unsigned)bits, 1, 64);       // two lanes share a byte
        if ((tid & 1) == 0) row[tid >> 1] = (unsigned char)((unsigned)bits | (other << 4));
    }
};
template <> struct MoveStore<2> {
    static __device__ __forceinline__ void put(unsigned char* row, int tid, unsigned long long bits) { row[tid] = (unsigned char)bits; }
};
template <> struct MoveStore<4> {
    static __device__ __forceinline__ void put(unsigned char* row, int tid, unsigned long long bits) {
        reinterpret_cast<unsigned short*>(row)[tid] = (unsigned short)bits;
    }
};
template <> struct MoveStore<8> {
    static __device__ __forceinline__ void put(unsigned char* row, int tid, unsigned long long bits) {
        reinterpret_cast<unsigned*>(row)[tid] = (unsigned)bits;
    }
};
template <> struct MoveStore<16> {
    static __device__ __forceinline__ void put(unsigned char* row, int tid, unsigned long long bits) {
        reinterpret_cast<uint2*>(row)[tid] = make_uint2((unsigned)bits, (unsigned)(bits >> 32));
    }
};

constexpr int ALIGN_MAX_WAVES = 10;      // workgroup form: 8 * 64 * 10 pairs >= CFM_CTC_ALIGN_MAX_TARGET + 1
constexpr int RECENTRE_EVERY = 64;       // workgroup form: steps between two re-centrings (two barriers each)

// Thread tid owns the pairs i = tid*P .. tid*P+P-1: blank state 2i (exists for i <= L) and label state 2i+1 (i < L).
// WG: several waves per utterance (blockDim.x = a.threads), else one.
// WILD: wildcard positions (a P-bit mask per thread) emit a.wild[t], prefetched with the block and uniform over the workgroup
// like the blank column; the emission is a select (made once per prefetched value, off the chain), the moves are the same three.
template <int P, bool WG, bool WILD = false>
__global__ __launch_bounds__(WG ? 64 * ALIGN_MAX_WAVES : 64) void align_chain_kernel(const AlignArgs a) {
    constexpr int U = 32 / P > 16 ? 16 : 32 / P;                          // time steps per prefetch block
    __shared__ float edge[2][ALIGN_MAX_WAVES];                            // last label state of each wave, double-buffered
    __shared__ float red[ALIGN_MAX_WAVES];
    __shared__ int red_i[ALIGN_MAX_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nwaves = WG ? (int)(blockDim.x >> 6) : 1;
    int Tb, Lb; int64_t off;
    align_geometry(a, b, Tb, Lb, off);

    int lab[P];
    bool hop[P];                  // state 2i+1 may be entered from 2i-1
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = tid * P + p;
        lab[p] = i < Lb ? align_label_w<WILD>(a, off, i) : -1 - i;       // distinct negatives: never equal to a neighbour
    }
    int prev_lab = __shfl_up(lab[P - 1], 1, 64);
    if (WG) {
        if (lane == 63) red_i[wave] = lab[P - 1];
        __syncthreads();
        if (lane == 0 && wave > 0) prev_lab = red_i[wave - 1];
        __syncthreads();
    }
    int repeats = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = tid * P + p;
        const int prv = p == 0 ? prev_lab : lab[p - 1];
        hop[p] = (i >= 1) && (i < Lb) && lab[p] != prv;
        repeats += (i >= 1 && i < Lb && lab[p] == prv) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) repeats += __shfl_xor(repeats, o, 64);
    if (WG) {
        if (lane == 0) red_i[wave] = repeats;
        __syncthreads();
        repeats = 0;
        for (int w = 0; w < nwaves; ++w) repeats += red_i[w];
    }
    if (Tb == 0 || Tb < Lb + repeats) {                                   // infeasible (uniform over the workgroup)
        if (tid == 0) a.end_state[b] = -1;
        return;
    }
    int col[P];                   // column of the label's logit, in range for threads past the target too
#pragma unroll
    for (int p = 0; p < P; ++p) col[p] = (lab[p] >= 0 && !(WILD && lab[p] == a.V)) ? lab[p] : a.blank;
    unsigned wmask = 0;           // WILD: bit p: pair p is a wildcard
    if (WILD) {
#pragma unroll
        for (int p = 0; p < P; ++p) wmask |= lab[p] == a.V ? 1u << p : 0u;
    }

    const float* x = a.logits + (int64_t)b * a.T * a.V;
    const float* wrow = WILD ? a.wild + (int64_t)b * a.T : nullptr;
    unsigned char* moves = a.moves + (int64_t)b * a.T * a.row_bytes;
    float sb[P], sl[P];           // current value of the thread's blank / label states
    float cb[U], cl[U][P], nb[U], nl[U][P];
    float nw[WILD ? U : 1];       // WILD: a.wild[t] of the block in flight
    auto load_block = [&](int t_first, float (&vb)[U], float (&vl)[U][P]) {      // clamped: always in range
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = min(t_first + u, Tb - 1);
            const float* row = x + (int64_t)t * a.V;
            vb[u] = row[a.blank];
            if (WILD) nw[u] = wrow[t];
#pragma unroll
            for (int p = 0; p < P; ++p) vl[u][p] = row[col[p]];
        }
    };
    // WILD, the label emission: a select on the thread's mask between the gathered logit and w[t].  It is made where a loaded
    // block becomes the current one (in place of that copy), so the T dependent steps below are those of the plain chain.
    auto emission = [&](float gathered, int u, int p) -> float {
        if (!WILD) return gathered;
        return ((wmask >> p) & 1u) ? nw[u] : gathered;
    };
    load_block(0, cb, cl);
    if (WILD) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int p = 0; p < P; ++p) cl[u][p] = emission(cl[u][p], u, p);
    }
    int par = 0;
    for (int t0 = 0; t0 < Tb; t0 += U) {
        load_block(t0 + U, nb, nl);
        __builtin_amdgcn_sched_barrier(0);
        if (t0 > 0 && (!WG || t0 % RECENTRE_EVERY == 0)) {                       // re-centre the lattice on its maximum
            float m = NEG_INF;
#pragma unroll
            for (int p = 0; p < P; ++p) m = fmaxf(m, fmaxf(sb[p], sl[p]));
            m = wave_max(m);
            if (WG) {
                if (lane == 0) red[wave] = m;
                __syncthreads();
                for (int w = 0; w < nwaves; ++w) m = fmaxf(m, red[w]);
            }
            if (m > NEG_INF && m < -NEG_INF) {
#pragma unroll
                for (int p = 0; p < P; ++p) { sb[p] -= m; sl[p] -= m; }
            }
            if (WG) {                                                            // the published edge values move with it
                if (lane == 63) edge[par][wave] = sl[P - 1];
                __syncthreads();
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t0 + u >= Tb) break;                                             // uniform
            const int t = t0 + u;
            unsigned long long bits = 0;
            if (t == 0) {
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int i = tid * P + p;
                    sb[p] = i == 0 ? cb[u] : NEG_INF;                            // state 0
                    sl[p] = (i == 0 && Lb > 0) ? cl[u][p] : NEG_INF;             // state 1
                }
            } else {
                float left = __shfl_up(sl[P - 1], 1, 64);
                if (lane == 0) left = (WG && wave > 0) ? edge[par][wave - 1] : NEG_INF;
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int i = tid * P + p;
                    const float ob = sb[p], ol = sl[p];
                    // ties take the smaller move: a larger move wins only when strictly greater
                    const unsigned mb = left > ob ? 1u : 0u;
                    const float vb = (mb ? left : ob) + cb[u];
                    unsigned ml = ob > ol ? 1u : 0u;
                    float best = ml ? ob : ol;
                    if (hop[p] && left > best) { ml = 2u; best = left; }
                    const float vl = best + cl[u][p];
                    sb[p] = i <= Lb ? vb : NEG_INF;
                    sl[p] = i < Lb ? vl : NEG_INF;
                    bits |= (unsigned long long)(mb | (ml << 2)) << (4 * p);
                    left = ol;
                }
            }
            if (WG) {
                par ^= 1;
                if (lane == 63) edge[par][wave] = sl[P - 1];
                __syncthreads();
            }
            MoveStore<P>::put(moves + (int64_t)t * a.row_bytes, tid, bits);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cb[u] = nb[u];
#pragma unroll
            for (int p = 0; p < P; ++p) cl[u][p] = emission(nl[u][p], u, p);
        }
    }
    // the path ends in state 2L or 2L-1, a tie in 2L
    float fb = NEG_INF, fl = NEG_INF;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = tid * P + p;
        if (i == Lb) fb = sb[p];
        if (i == Lb - 1) fl = sl[p];
    }
    fb = wave_max(fb); fl = wave_max(fl);
    if (WG) {
        __syncthreads();
        if (lane == 0) { red[wave] = fb; edge[0][wave] = fl; }
        __syncthreads();
        for (int w = 0; w < nwaves; ++w) { fb = fmaxf(fb, red[w]); fl = fmaxf(fl, edge[0][w]); }
    }
    if (tid == 0) a.end_state[b] = (Lb > 0 && fl > fb) ? 2 * Lb - 1 : 2 * Lb;
}

constexpr int TRACE_WIN = 64;            // frames per window = lanes
constexpr int TRACE_DW = 10;             // dwords of a row a window can touch: 127 states at any alignment span <= 9

template <bool WILD = false>
__global__ __launch_bounds__(64) void align_trace_kernel(const AlignArgs a) {
    __shared__ unsigned patch[TRACE_WIN][TRACE_DW + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    int Tb, Lb; int64_t off;
    align_geometry(a, b, Tb, Lb, off);
    int s = a.end_state[b];
    const bool ok = s >= 0 && s <= 2 * Lb && Tb > 0;
    int64_t* ftok = a.frame_tokens + (int64_t)b * a.T;
    int64_t* fidx = a.frame_index + (int64_t)b * a.T;
    for (int t = (ok ? Tb : 0) + lane; t < a.T; t += 64) { ftok[t] = -1; fidx[t] = -1; }
    if (!ok) return;
    const unsigned* moves = reinterpret_cast<const unsigned*>(a.moves + (int64_t)b * a.T * a.row_bytes);
    const int row_dw = a.row_bytes >> 2;
    for (int t_hi = Tb - 1; t_hi >= 0; t_hi -= TRACE_WIN) {
        const int d_lo = max(s - 2 * (TRACE_WIN - 1), 0) >> 4;
        const int t_mine = max(t_hi - lane, 0);
#pragma unroll
        for (int k = 0; k < TRACE_DW; ++k)
            patch[lane][k] = moves[(int64_t)t_mine * row_dw + min(d_lo + k, row_dw - 1)];
        __syncthreads();
        int mine = 0;
        const int n = min(TRACE_WIN, t_hi + 1);
        for (int c = 0; c < n; ++c) {                                    // every lane walks the same states
            if (c == lane) mine = s;
            const int d = min(max((s >> 4) - d_lo, 0), TRACE_DW - 1);
            const unsigned mv = (patch[c][d] >> (2 * (s & 15))) & 3u;
            if (t_hi - c > 0) s = max(s - (int)min(mv, 2u), 0);
        }
        __syncthreads();
        if (lane < n) {
            const int t = t_hi - lane;
            const bool is_label = (mine & 1) != 0;
            const int i = min(mine >> 1, max(Lb - 1, 0));
            int tok = is_label ? align_label_w<WILD>(a, off, i) : a.blank;
            if (WILD && tok == a.V) tok = CFM3_CTC_ALIGN_WILDCARD;
            ftok[t] = tok;
            fidx[t] = is_label ? i : -1;
        }
    }
}

// WILD: a wildcard frame (frame_tokens -2) emitted the row maximum: its log-probability is max - lse
template <bool WILD = false>
__global__ __launch_bounds__(256) void align_frame_kernel(const AlignArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t frame = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (frame >= (int64_t)a.B * a.T) return;
    const int b = (int)(frame / a.T), t = (int)(frame - (int64_t)b * a.T);
    int Tb, Lb; int64_t off;
    align_geometry(a, b, Tb, Lb, off);
    if (t >= Tb || a.end_state[b] < 0) return;
    const float* r = a.logits + frame * a.V;
    float m = NEG_INF;
    for (int c = lane; c < a.V; c += 64) m = fmaxf(m, r[c]);
    m = wave_max(m);
    double sum = 0.0;
    for (int c = lane; c < a.V; c += 64) sum += exp((double)r[c] - (double)m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const double lse = (double)m + log(sum);
    if (lane == 0) {
        const int64_t tok = a.frame_tokens[frame];
        const int c = (int)(tok < 0 ? 0 : (tok >= a.V ? a.V - 1 : tok));
        a.frame_lp[frame] = ((WILD && tok == CFM3_CTC_ALIGN_WILDCARD) ? (double)m : (double)r[c]) - lse;
    }
}

// The frame pass in front of a WILD chain, one wave per frame: w[b,t] = fl32(row maximum - penalty), the blank column included.
// Frames beyond the utterance's length are left unwritten: the chain clamps its reads to the frames before them.
__global__ __launch_bounds__(256) void align_wild_kernel(const AlignArgs a, float* wild) {
    const int lane = threadIdx.x & 63;
    const int64_t frame = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (frame >= (int64_t)a.B * a.T) return;
    const int b = (int)(frame / a.T), t = (int)(frame - (int64_t)b * a.T);
    int Tb, Lb; int64_t off;
    align_geometry(a, b, Tb, Lb, off);
    if (t >= Tb) return;
    const float* r = a.logits + frame * a.V;
    float m = NEG_INF;
    for (int c = lane; c < a.V; c += 64) m = fmaxf(m, r[c]);
    m = wave_max(m);
    if (lane == 0) wild[frame] = m - a.penalty;
}

__global__ __launch_bounds__(256) void align_span_kernel(const AlignArgs a) {
    __shared__ double part[256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int Tb, Lb; int64_t off;
    align_geometry(a, b, Tb, Lb, off);
    const bool ok = a.end_state[b] >= 0;
    int64_t* ts = a.token_start + (int64_t)b * a.Lmax;
    int64_t* te = a.token_end + (int64_t)b * a.Lmax;
    float* tsc = a.token_score + (int64_t)b * a.Lmax;
    for (int i = (ok ? Lb : 0) + tid; i < a.Lmax; i += 256) { ts[i] = -1; te[i] = -1; tsc[i] = NEG_INF; }
    if (!ok) {
        if (tid == 0) { a.score[b] = (double)NEG_INF; a.ok[b] = 0; }
        return;
    }
    const int64_t* fidx = a.frame_index + (int64_t)b * a.T;
    const double* flp = a.frame_lp + (int64_t)b * a.T;
    // each thread sums a contiguous slice of the frames, the slices are then added in order: one fixed summation order
    const int per = (Tb + 255) / 256;
    double acc = 0.0;
    for (int t = tid * per; t < min(tid * per + per, Tb); ++t) {
        acc += flp[t];
        const int64_t i = fidx[t];
        if (i < 0 || i >= Lb) continue;
        if (t == 0 || fidx[t - 1] != i) ts[i] = t;
        if (t == Tb - 1 || fidx[t + 1] != i) te[i] = t + 1;
    }
    part[tid] = acc;
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < 256; ++k) s += part[k];
        a.score[b] = s;
        a.ok[b] = 1;
    }
    for (int i = wave; i < Lb; i += 4) {                                 // a wave per token
        const int64_t t0 = ts[i], t1 = te[i];
        const bool run = t0 >= 0 && t1 > t0 && t1 <= Tb;
        double sum = 0.0;
        if (run)
            for (int t = (int)t0 + lane; t < (int)t1; t += 64) sum += flp[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0) tsc[i] = run ? (float)(sum / (double)(t1 - t0)) : NEG_INF;
    }
}

// wave form: 64*P >= Lmax + 1, P a power of two <= 16; workgroup form: P = 8, threads a multiple of 64
void align_shape(int Lmax, int& P, int& threads) {
    if (Lmax <= CFM_CTC_ALIGN_WAVE_MAX_TARGET) {
        P = 1;
        while (64 * P < Lmax + 1) P *= 2;
        threads = 64;
    } else {
        P = 8;
        threads = ((Lmax + 1 + 7) / 8 + 63) / 64 * 64;
    }
}

bool align_in_range(int B, int T, int Lmax) {
    return B > 0 && T > 0 && T <= CFM_CTC_ALIGN_MAX_FRAMES && Lmax >= 1 && Lmax <= CFM_CTC_ALIGN_MAX_TARGET;
}

// workspace: frame_lp (B*T doubles) | end_state (B ints, padded to 16 bytes) | moves (B*T rows)
size_t align_layout(int B, int T, int Lmax, AlignArgs* a) {
    int P, threads;
    align_shape(Lmax, P, threads);
    const size_t frames = (size_t)B * T, row_bytes = (size_t)threads * P / 2;
    const size_t lp_bytes = frames * sizeof(double), end_bytes = ((size_t)B * sizeof(int) + 15) / 16 * 16;
    if (a) {
        a->P = P; a->threads = threads; a->row_bytes = (int)row_bytes;
        char* base = reinterpret_cast<char*>(a->frame_lp);
        a->end_state = reinterpret_cast<int*>(base + lp_bytes);
        a->moves = reinterpret_cast<unsigned char*>(base + lp_bytes + end_bytes);
    }
    return lp_bytes + end_bytes + frames * row_bytes;
}

// ---- long form (conformer_hip2_align_long.h): the chain stage cut into cells, no limit on T or L but memory ----------------
//
// The pairs i = 0..L are cut into tiles of tile_pairs, the frames into chunks of chunk_frames; cell (k, c) is ONE workgroup
// running tile k over chunk c in the workgroup form above (a thread owns 8 pairs, one cross-lane value per step, an LDS word
// and one barrier per frame between waves).  It needs the tile's state after chunk c - 1 (the carry, rewritten in place:
// a tile has one cell per launch) and, for every frame t - 1 it steps from, the last label state of tile k - 1 (the edge
// column, one value per tile and frame).  Launch d runs the cells with k + c = d; (k, c - 1), (k - 1, c) and (k - 1, c - 1)
// lie on the diagonals d - 1 and d - 2, so the order of the stream provides both: no workgroup ever waits for another.
//
// The state is float64 and is never re-centred: a value is e + max(...) over doubles converted once from the fp32 logits,
// the very additions and comparisons of the float64 restatement, so the moves are the restatement's for any finite input.
//
// Dead cells are skipped by the whole workgroup; they store -inf in their carry and edge slice and no moves.
//   front-dead: the cell's first pair lies beyond its last frame.  Pair i cannot be entered before frame i (one pair per
//               step at the most), so every true value in the cell IS -inf: nothing changes.
//   back-dead : the cell's last pair at its first frame is more than the remaining frames away from pair L - 1, so no
//               state of the cell lies on a path that reaches the end.
// Why the second is safe: call a (frame, state) live when it lies on some path from the start to the end.  Every
// predecessor of a live state on such a path is live too, and a state that can reach the end makes every state that can
// move into it able to reach the end: the states that cannot reach the end are closed under "successor of", so lowering
// them to -inf changes only values of states that cannot reach the end either.  The trace starts at a live state and only
// ever steps to the predecessor a live state chose among values that are all unchanged or lowered dead ones (which lose
// to the live maximum exactly as before, or tie at -inf where no predecessor is live, which a live state never has).
// So the traced path and every value on it are those of the full lattice.

struct LongArgs {
    AlignArgs a;
    double* carry;                   // (B, n_tiles, 2, tile_pairs): blank states, then label states, after the tile's last chunk
    double* edge;                    // (B, n_tiles, T): the tile's last label state after every frame
    int* flags;                      // (B) 1: the target fits the frames
    int tile_pairs, chunk_frames, n_tiles, n_chunks;
};

constexpr double NEG_INF64 = -__builtin_inf();
constexpr int LONG_P = 8;

template <bool WILD = false>
__global__ __launch_bounds__(256) void align_long_feasible_kernel(const LongArgs g) {
    __shared__ int part[4];
    const AlignArgs& a = g.a;
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb, Lb; int64_t off;
    align_geometry(a, b, Tb, Lb, off);
    int repeats = 0;
    for (int i = 1 + tid; i < Lb; i += 256)
        repeats += align_label_w<WILD>(a, off, i) == align_label_w<WILD>(a, off, i - 1) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) repeats += __shfl_xor(repeats, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = repeats;
    __syncthreads();
    if (tid == 0) {
        repeats = part[0] + part[1] + part[2] + part[3];
        const bool fits = !(Tb == 0 || Tb < Lb + repeats);
        g.flags[b] = fits ? 1 : 0;
        a.end_state[b] = -1;                                             // a feasible row: align_long_end_kernel
    }
}

// WAVES: the most waves of a workgroup (tile_pairs / 512 <= WAVES); it sets the register budget and with it the prefetch depth
// WILD: as in align_chain_kernel: a P-bit mask of the thread's wildcard pairs, a.wild[t] prefetched with the block, a select
template <int WAVES, bool WILD = false>
__global__ __launch_bounds__(64 * WAVES) void align_long_cell_kernel(const LongArgs g, const int diag, const int k_lo) {
    constexpr int P = LONG_P, U = WAVES == 1 ? 8 : (WAVES <= 8 ? 4 : 2);
    constexpr bool WG = WAVES > 1;
    __shared__ double edge_lds[2][WAVES];                                // last label state of each wave, double-buffered
    const AlignArgs& a = g.a;
    const int b = blockIdx.y, k = k_lo + (int)blockIdx.x, c = diag - k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, threads = (int)blockDim.x;
    if (!g.flags[b]) return;
    int Tb, Lb; int64_t off;
    align_geometry(a, b, Tb, Lb, off);
    const int tp = g.tile_pairs;
    const int t_first = c * g.chunk_frames, i_first = k * tp;
    if (t_first >= Tb || i_first > Lb) return;                           // beyond the utterance, as every cell that reads this one
    const int t_end = min(t_first + g.chunk_frames, Tb);                 // exclusive
    double* carry = g.carry + ((int64_t)b * g.n_tiles + k) * 2 * tp;
    double* edge_out = g.edge + ((int64_t)b * g.n_tiles + k) * a.T;
    const double* edge_in = k > 0 ? edge_out - a.T : edge_out;           // tile k - 1 (read for k > 0 only)
    // dead cells (the argument stands above LongArgs); uniform over the workgroup
    const bool front_dead = i_first > t_end - 1;
    const bool back_dead = Lb - 1 - (i_first + tp - 1) > Tb - 1 - t_first;
    if (front_dead || back_dead) {
        for (int j = tid; j < 2 * tp; j += threads) carry[j] = NEG_INF64;
        for (int t = t_first + tid; t < t_end; t += threads) edge_out[t] = NEG_INF64;
        return;
    }
    const int i0 = i_first + tid * P;
    int col[P];                   // column of the label's logit, in range for threads past the target too
    bool hop[P];                  // state 2i+1 may be entered from 2i-1
    unsigned wmask = 0;           // WILD: bit p: pair p is a wildcard
    {
        int prv = (i0 >= 1 && i0 - 1 < Lb) ? align_label_w<WILD>(a, off, i0 - 1) : -i0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int i = i0 + p;
            const int lab = i < Lb ? align_label_w<WILD>(a, off, i) : -1 - i;   // distinct negatives: never equal to a neighbour
            hop[p] = (i >= 1) && (i < Lb) && lab != prv;
            col[p] = (lab >= 0 && !(WILD && lab == a.V)) ? lab : a.blank;
            if (WILD) wmask |= lab == a.V ? 1u << p : 0u;
            prv = lab;
        }
    }
    double sb[P], sl[P];          // current value of the thread's blank / label states
#pragma unroll
    for (int p = 0; p < P; ++p) {
        sb[p] = c > 0 ? carry[tid * P + p] : NEG_INF64;
        sl[p] = c > 0 ? carry[tp + tid * P + p] : NEG_INF64;
    }
    const float* x = a.logits + (int64_t)b * a.T * a.V;
    unsigned char* moves = a.moves + (int64_t)b * a.T * a.row_bytes + (int64_t)k * (tp / 2);
    const float* wrow = WILD ? a.wild + (int64_t)b * a.T : nullptr;
    float cb[U], cl[U][P], nb[U], nl[U][P];
    float nw[WILD ? U : 1];       // WILD: a.wild[t] of the block in flight
    double ce[U], ne[U];          // thread 0: the last label state of tile k - 1 at the frame stepped from
    auto load_block = [&](int t_from, float (&vb)[U], float (&vl)[U][P], double (&ve)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = min(t_from + u, t_end - 1);                    // clamped to the chunk: its edge values are all written
            const float* row = x + (int64_t)t * a.V;
            vb[u] = row[a.blank];
            if (WILD) nw[u] = wrow[t];
#pragma unroll
            for (int p = 0; p < P; ++p) vl[u][p] = row[col[p]];
            ve[u] = (tid == 0 && k > 0 && t >= 1) ? edge_in[t - 1] : NEG_INF64;
        }
    };
    // WILD, the label emission: as in align_chain_kernel, selected where a loaded block becomes the current one
    auto emission = [&](float gathered, int u, int p) -> float {
        if (!WILD) return gathered;
        return ((wmask >> p) & 1u) ? nw[u] : gathered;
    };
    load_block(t_first, cb, cl, ce);
    if (WILD) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int p = 0; p < P; ++p) cl[u][p] = emission(cl[u][p], u, p);
    }
    int par = 0;
    if (WG) {
        if (lane == 63) edge_lds[0][wave] = sl[P - 1];
        __syncthreads();
    }
    for (int t0 = t_first; t0 < t_end; t0 += U) {
        load_block(t0 + U, nb, nl, ne);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t0 + u >= t_end) break;                                  // uniform
            const int t = t0 + u;
            unsigned bits = 0;
            if (t == 0) {
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int i = i0 + p;
                    sb[p] = i == 0 ? (double)cb[u] : NEG_INF64;                       // state 0
                    sl[p] = (i == 0 && Lb > 0) ? (double)cl[u][p] : NEG_INF64;        // state 1
                }
            } else {
                double left = __shfl_up(sl[P - 1], 1, 64);
                if (lane == 0) left = (WG && wave > 0) ? edge_lds[par][wave - 1] : ce[u];
                const double eb = (double)cb[u];
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int i = i0 + p;
                    const double ob = sb[p], ol = sl[p];
                    // ties take the smaller move: a larger move wins only when strictly greater
                    const unsigned mb = left > ob ? 1u : 0u;
                    const double vb = (mb ? left : ob) + eb;
                    unsigned ml = ob > ol ? 1u : 0u;
                    double best = ml ? ob : ol;
                    if (hop[p] && left > best) { ml = 2u; best = left; }
                    const double vl = best + (double)cl[u][p];
                    sb[p] = i <= Lb ? vb : NEG_INF64;
                    sl[p] = i < Lb ? vl : NEG_INF64;
                    bits |= (mb | (ml << 2)) << (4 * p);
                    left = ol;
                }
            }
            if (WG) {
                par ^= 1;
                if (lane == 63) edge_lds[par][wave] = sl[P - 1];
                __syncthreads();
            }
            if (tid == threads - 1) edge_out[t] = sl[P - 1];
            MoveStore<P>::put(moves + (int64_t)t * a.row_bytes, tid, bits);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cb[u] = nb[u];
            ce[u] = ne[u];
#pragma unroll
            for (int p = 0; p < P; ++p) cl[u][p] = emission(nl[u][p], u, p);
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        carry[tid * P + p] = sb[p];
        carry[tp + tid * P + p] = sl[p];
    }
}

// the path ends in state 2L or 2L-1, a tie in 2L: the two values lie in the carries, possibly of two tiles
__global__ __launch_bounds__(64) void align_long_end_kernel(const LongArgs g) {
    const AlignArgs& a = g.a;
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= a.B || !g.flags[b]) return;
    int Tb, Lb; int64_t off;
    align_geometry(a, b, Tb, Lb, off);
    const int tp = g.tile_pairs;
    const double* cr = g.carry + (int64_t)b * g.n_tiles * 2 * tp;
    const double fb = cr[(int64_t)(Lb / tp) * 2 * tp + Lb % tp];
    const double fl = Lb > 0 ? cr[(int64_t)((Lb - 1) / tp) * 2 * tp + tp + (Lb - 1) % tp] : NEG_INF64;
    a.end_state[b] = (Lb > 0 && fl > fb) ? 2 * Lb - 1 : 2 * Lb;
}

constexpr int LONG_DEFAULT_TILE_PAIRS = 512;           // the fastest pair of profiles/ctc_align_long_bench.json at (90000, 30000):
constexpr int LONG_DEFAULT_CHUNK_FRAMES = 128;         // one wave per cell (no barrier in the step), 762 launches

struct LongPlan {
    int tile_pairs, chunk_frames, n_tiles, n_chunks;
    size_t lp_bytes, end_bytes, carry_bytes, edge_bytes, row_bytes, moves_bytes;
    size_t total() const { return lp_bytes + end_bytes + carry_bytes + edge_bytes + moves_bytes; }
};

// the tiling of a shape and the size of every part of its workspace; false: unsupported
bool align_long_plan(int B, int T, int Lmax, int tile_pairs, int chunk_frames, LongPlan* p) {
    if (B < 1 || B > 65535 || T < 1 || T > CFM2_CTC_ALIGN_LONG_MAX_FRAMES || Lmax < 1 || Lmax > CFM2_CTC_ALIGN_LONG_MAX_TARGET)
        return false;
    if ((int64_t)B * T > ((int64_t)1 << 31)) return false;              // the per-frame kernel: a wave per frame, 4 per workgroup
    const int l_up = (Lmax + 1 + 511) / 512 * 512, t_up = (T + 15) / 16 * 16;
    if (tile_pairs == 0) tile_pairs = LONG_DEFAULT_TILE_PAIRS < l_up ? LONG_DEFAULT_TILE_PAIRS : l_up;
    if (chunk_frames == 0) chunk_frames = LONG_DEFAULT_CHUNK_FRAMES < t_up ? LONG_DEFAULT_CHUNK_FRAMES : t_up;
    if (tile_pairs < 512 || tile_pairs > 8192 || tile_pairs % 512) return false;
    if (chunk_frames < 16 || chunk_frames > 65536 || chunk_frames % 16) return false;
    auto pad = [](size_t n) { return (n + 15) / 16 * 16; };
    p->tile_pairs = tile_pairs;
    p->chunk_frames = chunk_frames;
    p->n_tiles = (Lmax + 1 + tile_pairs - 1) / tile_pairs;
    p->n_chunks = (T + chunk_frames - 1) / chunk_frames;
    const size_t frames = (size_t)B * T, tiles = (size_t)B * p->n_tiles;
    p->lp_bytes = pad(frames * sizeof(double));
    p->end_bytes = pad((size_t)B * 2 * sizeof(int));
    p->carry_bytes = tiles * 2 * tile_pairs * sizeof(double);
    p->edge_bytes = pad(tiles * T * sizeof(double));
    p->row_bytes = (size_t)p->n_tiles * tile_pairs / 2;
    p->moves_bytes = frames * p->row_bytes;
    return true;
}

size_t wild_bytes(int B, int T) { return ((size_t)B * T * sizeof(float) + 15) / 16 * 16; }     // the w part of a WILD workspace
bool penalty_ok(float p) { return p >= 0.0f && p <= 3.402823466e38f; }                        // finite, not NaN, not negative

// WILD: the entries of conformer_hip3_align_wild.h (w behind the workspace of the plain form); else `penalty` is not read
template <bool WILD>
int align_long_run(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                   const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax, int blank_id, float penalty,
                   int tile_pairs, int chunk_frames, void* workspace, size_t workspace_bytes, int64_t* frame_tokens,
                   int64_t* frame_index, int64_t* token_start, int64_t* token_end, float* token_score, double* score,
                   unsigned char* ok, bool chain_only, cfm_stream_t stream) {
    CFM_REQUIRE(logits && targets && workspace, CFM_ERR_NULL);
    CFM_REQUIRE(chain_only || (frame_tokens && frame_index && token_start && token_end && token_score && score && ok),
                CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && T > 0 && V >= 2 && Lmax >= 1 && blank_id >= 0 && blank_id < V, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(!WILD || penalty_ok(penalty), CFM_ERR_BAD_SHAPE);
    LongPlan plan;
    CFM_REQUIRE(align_long_plan(B, T, Lmax, tile_pairs, chunk_frames, &plan), CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, CFM_ERR_ALIGN);
    CFM_REQUIRE(workspace_bytes >= plan.total() + (WILD ? wild_bytes(B, T) : 0), CFM_ERR_BAD_SHAPE);
    LongArgs g{};
    AlignArgs& a = g.a;
    a.logits = logits; a.targets = targets; a.in_len = lengths_or_null; a.tgt_len = target_lengths_or_null;
    char* base = reinterpret_cast<char*>(workspace);
    a.frame_lp = reinterpret_cast<double*>(base);
    a.end_state = reinterpret_cast<int*>(base + plan.lp_bytes);
    g.flags = a.end_state + B;
    g.carry = reinterpret_cast<double*>(base + plan.lp_bytes + plan.end_bytes);
    g.edge = reinterpret_cast<double*>(base + plan.lp_bytes + plan.end_bytes + plan.carry_bytes);
    a.moves = reinterpret_cast<unsigned char*>(base + plan.lp_bytes + plan.end_bytes + plan.carry_bytes + plan.edge_bytes);
    a.frame_tokens = frame_tokens; a.frame_index = frame_index; a.token_start = token_start; a.token_end = token_end;
    a.token_score = token_score; a.score = score; a.ok = ok;
    a.tgt_numel = (int64_t)B * Lmax;
    a.B = B; a.T = T; a.V = V; a.Lmax = Lmax; a.blank = blank_id;
    a.P = LONG_P; a.threads = plan.tile_pairs / LONG_P; a.row_bytes = (int)plan.row_bytes;
    g.tile_pairs = plan.tile_pairs; g.chunk_frames = plan.chunk_frames; g.n_tiles = plan.n_tiles; g.n_chunks = plan.n_chunks;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 per_row((unsigned)B), block((unsigned)a.threads);
    const int64_t frames = (int64_t)B * T;
    if (WILD) {
        float* wild = reinterpret_cast<float*>(base + plan.total());
        a.wild = wild; a.penalty = penalty;
        hipLaunchKernelGGL(align_wild_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, a, wild);
    }
    hipLaunchKernelGGL(align_long_feasible_kernel<WILD>, per_row, dim3(256), 0, s, g);
    for (int d = 0; d < plan.n_tiles + plan.n_chunks - 1; ++d) {         // one launch per anti-diagonal k + c = d
        const int k_lo = d > plan.n_chunks - 1 ? d - (plan.n_chunks - 1) : 0, k_hi = d < plan.n_tiles - 1 ? d : plan.n_tiles - 1;
        const dim3 grid((unsigned)(k_hi - k_lo + 1), (unsigned)B);
        if (a.threads == 64) hipLaunchKernelGGL((align_long_cell_kernel<1, WILD>), grid, block, 0, s, g, d, k_lo);
        else if (a.threads <= 512) hipLaunchKernelGGL((align_long_cell_kernel<8, WILD>), grid, block, 0, s, g, d, k_lo);
        else hipLaunchKernelGGL((align_long_cell_kernel<16, WILD>), grid, block, 0, s, g, d, k_lo);
    }
    hipLaunchKernelGGL(align_long_end_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, g);
    if (chain_only) return cfm_launch_status();
    hipLaunchKernelGGL(align_trace_kernel<WILD>, per_row, dim3(64), 0, s, a);
    hipLaunchKernelGGL(align_frame_kernel<WILD>, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(align_span_kernel, per_row, dim3(256), 0, s, a);
    return cfm_launch_status();
}

size_t align_wild_offset(int B, int T, int Lmax) { return (align_layout(B, T, Lmax, nullptr) + 15) / 16 * 16; }

template <bool WILD>
int align_run(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
              const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax, int blank_id, float penalty,
              void* workspace, size_t workspace_bytes, int64_t* frame_tokens, int64_t* frame_index,
              int64_t* token_start, int64_t* token_end, float* token_score, double* score,
              unsigned char* ok, cfm_stream_t stream) {
    CFM_REQUIRE(logits && targets && workspace && frame_tokens && frame_index && token_start && token_end && token_score &&
                score && ok, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && T > 0 && V >= 2 && Lmax >= 1 && blank_id >= 0 && blank_id < V, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(!WILD || penalty_ok(penalty), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(align_in_range(B, T, Lmax), CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, CFM_ERR_ALIGN);
    AlignArgs a{};
    a.logits = logits; a.targets = targets; a.in_len = lengths_or_null; a.tgt_len = target_lengths_or_null;
    a.frame_lp = reinterpret_cast<double*>(workspace);
    const size_t plain_bytes = align_layout(B, T, Lmax, &a);
    CFM_REQUIRE(workspace_bytes >= (WILD ? align_wild_offset(B, T, Lmax) + wild_bytes(B, T) : plain_bytes), CFM_ERR_BAD_SHAPE);
    a.frame_tokens = frame_tokens; a.frame_index = frame_index; a.token_start = token_start; a.token_end = token_end;
    a.token_score = token_score; a.score = score; a.ok = ok;
    a.tgt_numel = (int64_t)B * Lmax;
    a.B = B; a.T = T; a.V = V; a.Lmax = Lmax; a.blank = blank_id;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)B);
    const int64_t frames = (int64_t)B * T;
    if (WILD) {
        float* wild = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + align_wild_offset(B, T, Lmax));
        a.wild = wild; a.penalty = penalty;
        hipLaunchKernelGGL(align_wild_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, a, wild);
    }
    if (a.threads > 64) {
        hipLaunchKernelGGL((align_chain_kernel<8, true, WILD>), grid, dim3((unsigned)a.threads), 0, s, a);
    } else {
        switch (a.P) {
            case 1: hipLaunchKernelGGL((align_chain_kernel<1, false, WILD>), grid, dim3(64), 0, s, a); break;
            case 2: hipLaunchKernelGGL((align_chain_kernel<2, false, WILD>), grid, dim3(64), 0, s, a); break;
            case 4: hipLaunchKernelGGL((align_chain_kernel<4, false, WILD>), grid, dim3(64), 0, s, a); break;
            case 8: hipLaunchKernelGGL((align_chain_kernel<8, false, WILD>), grid, dim3(64), 0, s, a); break;
            default: hipLaunchKernelGGL((align_chain_kernel<16, false, WILD>), grid, dim3(64), 0, s, a); break;
        }
    }
    hipLaunchKernelGGL(align_trace_kernel<WILD>, grid, dim3(64), 0, s, a);
    hipLaunchKernelGGL(align_frame_kernel<WILD>, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(align_span_kernel, grid, dim3(256), 0, s, a);
    return cfm_launch_status();
}

}  // namespace

extern "C" size_t cfm_ctc_align_workspace_bytes(int B, int T, int Lmax) {
    return align_in_range(B, T, Lmax) ? align_layout(B, T, Lmax, nullptr) : 0;
}

extern "C" int cfm_ctc_align_f32(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                                 const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax, int blank_id,
                                 void* workspace, size_t workspace_bytes, int64_t* frame_tokens, int64_t* frame_index,
                                 int64_t* token_start, int64_t* token_end, float* token_score, double* score,
                                 unsigned char* ok, cfm_stream_t stream) {
    return align_run<false>(logits, targets, lengths_or_null, target_lengths_or_null, B, T, V, Lmax, blank_id, 0.0f, workspace,
                            workspace_bytes, frame_tokens, frame_index, token_start, token_end, token_score, score, ok, stream);
}

extern "C" size_t cfm3_ctc_align_wild_workspace_bytes(int B, int T, int Lmax) {
    return align_in_range(B, T, Lmax) ? align_wild_offset(B, T, Lmax) + wild_bytes(B, T) : 0;
}

extern "C" int cfm3_ctc_align_wild_f32(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                                       const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax, int blank_id,
                                       float wildcard_penalty, void* workspace, size_t workspace_bytes, int64_t* frame_tokens,
                                       int64_t* frame_index, int64_t* token_start, int64_t* token_end, float* token_score,
                                       double* score, unsigned char* ok, cfm_stream_t stream) {
    return align_run<true>(logits, targets, lengths_or_null, target_lengths_or_null, B, T, V, Lmax, blank_id, wildcard_penalty,
                           workspace, workspace_bytes, frame_tokens, frame_index, token_start, token_end, token_score, score, ok,
                           stream);
}

extern "C" size_t cfm2_ctc_align_long_workspace_bytes(int B, int T, int Lmax, int tile_pairs, int chunk_frames) {
    LongPlan plan;
    return align_long_plan(B, T, Lmax, tile_pairs, chunk_frames, &plan) ? plan.total() : 0;
}

extern "C" int cfm2_ctc_align_long_launches(int T, int Lmax, int tile_pairs, int chunk_frames) {
    LongPlan plan;
    return align_long_plan(1, T, Lmax, tile_pairs, chunk_frames, &plan) ? plan.n_tiles + plan.n_chunks - 1 : 0;
}

extern "C" int cfm2_ctc_align_long_f32(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                                       const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax, int blank_id,
                                       int tile_pairs, int chunk_frames, void* workspace, size_t workspace_bytes,
                                       int64_t* frame_tokens, int64_t* frame_index, int64_t* token_start, int64_t* token_end,
                                       float* token_score, double* score, unsigned char* ok, cfm_stream_t stream) {
    return align_long_run<false>(logits, targets, lengths_or_null, target_lengths_or_null, B, T, V, Lmax, blank_id, 0.0f,
                                 tile_pairs, chunk_frames, workspace, workspace_bytes, frame_tokens, frame_index, token_start,
                                 token_end, token_score, score, ok, false, stream);
}

extern "C" size_t cfm3_ctc_align_long_wild_workspace_bytes(int B, int T, int Lmax, int tile_pairs, int chunk_frames) {
    LongPlan plan;
    return align_long_plan(B, T, Lmax, tile_pairs, chunk_frames, &plan) ? plan.total() + wild_bytes(B, T) : 0;
}

extern "C" int cfm3_ctc_align_long_wild_f32(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                                            const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax,
                                            int blank_id, float wildcard_penalty, int tile_pairs, int chunk_frames,
                                            void* workspace, size_t workspace_bytes, int64_t* frame_tokens, int64_t* frame_index,
                                            int64_t* token_start, int64_t* token_end, float* token_score, double* score,
                                            unsigned char* ok, cfm_stream_t stream) {
    return align_long_run<true>(logits, targets, lengths_or_null, target_lengths_or_null, B, T, V, Lmax, blank_id,
                                wildcard_penalty, tile_pairs, chunk_frames, workspace, workspace_bytes, frame_tokens,
                                frame_index, token_start, token_end, token_score, score, ok, false, stream);
}

extern "C" int cfm2_ctc_align_long_chain_f32(const float* logits, const int64_t* targets, const int64_t* lengths_or_null,
                                             const int64_t* target_lengths_or_null, int B, int T, int V, int Lmax,
                                             int blank_id, int tile_pairs, int chunk_frames, void* workspace,
                                             size_t workspace_bytes, cfm_stream_t stream) {
    return align_long_run<false>(logits, targets, lengths_or_null, target_lengths_or_null, B, T, V, Lmax, blank_id, 0.0f,
                                 tile_pairs, chunk_frames, workspace, workspace_bytes, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, true, stream);
}
