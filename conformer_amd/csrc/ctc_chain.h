// The CTC alpha / beta chain of one wave over one (utterance, label sequence), shared by the loss (ctc.hip) and the n-best
// scores (ctc_nbest.hip).  Internal: not part of the C ABI.
//
// The wave holds the whole 2L+1 state lattice in registers: lane l owns the P consecutive (blank, label) state pairs
// i = l*P .. l*P+P-1, blank state 2i (exists for i <= L) and label state 2i+1 (exists for i < L), so a time step needs ONE
// cross-lane value in the alpha direction (the label state left of the lane's first pair) and two in the beta direction.  The
// log-probabilities are prefetched a block of steps ahead; the recursion touches no memory but its own row store.  The lattice
// is fp32 but RE-CENTRED every prefetch block (its maximum moves into a float64 per-frame offset), so the rounding error depends
// on the drift inside one block (~1e-5), not on |log-likelihood| of a long utterance.
#pragma once
#include "cfm_common.h"

namespace ctc_chain {

constexpr float NEG_INF = -__builtin_inff();

__device__ __forceinline__ float log_fast(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994530942f; }
__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    return m == NEG_INF ? NEG_INF : m + log_fast(exp_fast(a - m) + exp_fast(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);
    return m == NEG_INF ? NEG_INF : m + log_fast(exp_fast(a - m) + exp_fast(b - m) + exp_fast(c - m));
}

// a label as every kernel of the lattice reads it: clamped into the vocabulary
__device__ __forceinline__ int clamp_label(int64_t v, int V) { return (int)(v < 0 ? 0 : (v >= V ? V - 1 : v)); }

inline int pairs_per_lane(int Lmax) {                // 64*P >= Lmax + 1
    int P = 1;
    while (64 * P < Lmax + 1) P *= 2;
    return P;
}

// What one chain reads and writes.  Tb >= 1 frames and Lb <= Lmax labels, both already clamped by the caller; `labels` holds
// at least Lb entries; lpl is [t][Lmax] (the log-probability of label i at frame t), lpb is [t]; `out` takes the rows
// [t][2*64*P], element 2i (+1); coff[t] is the float64 offset of row t (stored value + offset = true log alpha / beta).
struct Row {
    const int64_t* labels;
    const float* lpl;
    const float* lpb;
    float* out;
    double* coff;
    int Tb, Lb, Lmax, V;
};

// All 64 lanes of the wave call it.  Returns the log-likelihood (alpha direction; every lane holds it), 0 for BETA.
template <int P, bool BETA>
__device__ __forceinline__ double run(const Row& r, const int lane) {
    constexpr int U = P >= 16 ? 1 : 16 / P;                   // time steps per prefetch block
    constexpr int NP = 64 * P;
    const int Tb = r.Tb, Lb = r.Lb;
    double* coff = r.coff;
    double C = 0.0;                                           // stored value + C = true log alpha (beta)
    float* out = r.out;
    const float* lplb = r.lpl;
    const float* lpbb = r.lpb;

    int lab[P];
    bool hop[P];                  // alpha: state 2i+1 may be entered from 2i-1; beta: 2i+1 may go to 2i+3
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = lane * P + p;
        lab[p] = i < Lb ? clamp_label(r.labels[i], r.V) : -1 - i;     // distinct negatives: never equal to a neighbour
    }
    const int nb_lab = BETA ? __shfl_down(lab[0], 1, 64) : __shfl_up(lab[P - 1], 1, 64);
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = lane * P + p;
        if (BETA) {
            const int nxt = p == P - 1 ? nb_lab : lab[p + 1];
            hop[p] = (i + 1 < Lb) && lab[p] != nxt;
        } else {
            const int prv = p == 0 ? nb_lab : lab[p - 1];
            hop[p] = (i >= 1) && (i < Lb) && lab[p] != prv;
        }
    }
    int idx[P];
#pragma unroll
    for (int p = 0; p < P; ++p) idx[p] = min(lane * P + p, r.Lmax - 1);

    float sb[P], sl[P];          // current alpha (beta) of the lane's blank / label states
    float cb[U], cl[U][P], nb[U], nl[U][P];
    auto load_block = [&](int t_first, float (&vb)[U], float (&vl)[U][P]) {      // clamped: always in range
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = min(max(BETA ? t_first - u : t_first + u, 0), Tb - 1);
            vb[u] = lpbb[t];
#pragma unroll
            for (int p = 0; p < P; ++p) vl[u][p] = lplb[(int64_t)t * r.Lmax + idx[p]];
        }
    };
    const int t_begin = BETA ? Tb - 1 : 0;
    load_block(t_begin, cb, cl);
    for (int done = 0; done < Tb; done += U) {
        const int t0 = BETA ? t_begin - done : done;
        load_block(BETA ? t0 - U : t0 + U, nb, nl);
        __builtin_amdgcn_sched_barrier(0);
        if (done > 0) {                                                      // re-centre the lattice on its maximum
            float m = NEG_INF;
#pragma unroll
            for (int p = 0; p < P; ++p) m = fmaxf(m, fmaxf(sb[p], sl[p]));
            m = wave_max(m);
            if (m > NEG_INF) {
#pragma unroll
                for (int p = 0; p < P; ++p) { sb[p] -= m; sl[p] -= m; }
                C += (double)m;
            }
        }
        if (lane < U && done + lane < Tb) coff[BETA ? t0 - lane : t0 + lane] = C;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (done + u >= Tb) break;                                       // uniform
            const int t = BETA ? t0 - u : t0 + u;
            if (done + u == 0) {
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int i = lane * P + p;
                    if (BETA) {
                        sb[p] = i == Lb ? cb[u] : NEG_INF;                       // state S-1
                        sl[p] = i == Lb - 1 ? cl[u][p] : NEG_INF;                // state S-2
                    } else {
                        sb[p] = i == 0 ? cb[u] : NEG_INF;                        // state 0
                        sl[p] = (i == 0 && Lb > 0) ? cl[u][p] : NEG_INF;         // state 1
                    }
                }
            } else if (BETA) {
                float right_b = __shfl_down(sb[0], 1, 64), right_l = __shfl_down(sl[0], 1, 64);
                if (lane == 63) { right_b = NEG_INF; right_l = NEG_INF; }
                float nsb[P], nsl[P];
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int i = lane * P + p;
                    const float rb = p == P - 1 ? right_b : sb[p + 1], rl = p == P - 1 ? right_l : sl[p + 1];
                    const float vb = lse2(sb[p], sl[p]) + cb[u];
                    const float vl = lse3(sl[p], rb, hop[p] ? rl : NEG_INF) + cl[u][p];
                    nsb[p] = i <= Lb ? vb : NEG_INF;
                    nsl[p] = i < Lb ? vl : NEG_INF;
                }
#pragma unroll
                for (int p = 0; p < P; ++p) { sb[p] = nsb[p]; sl[p] = nsl[p]; }
            } else {
                float left = __shfl_up(sl[P - 1], 1, 64);
                if (lane == 0) left = NEG_INF;
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int i = lane * P + p;
                    const float ob = sb[p], ol = sl[p];
                    const float vb = lse2(ob, left) + cb[u];
                    const float vl = lse3(ol, ob, hop[p] ? left : NEG_INF) + cl[u][p];
                    sb[p] = i <= Lb ? vb : NEG_INF;
                    sl[p] = i < Lb ? vl : NEG_INF;
                    left = ol;
                }
            }
            float* orow = out + (int64_t)t * 2 * NP + (int64_t)lane * 2 * P;
#pragma unroll
            for (int p = 0; p < P; ++p) { orow[2 * p] = sb[p]; orow[2 * p + 1] = sl[p]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cb[u] = nb[u];
#pragma unroll
            for (int p = 0; p < P; ++p) cl[u][p] = nl[u][p];
        }
    }
    if (BETA) return 0.0;
    float fb = NEG_INF, fl = NEG_INF;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = lane * P + p;
        if (i == Lb) fb = sb[p];
        if (i == Lb - 1) fl = sl[p];
    }
    fb = wave_max(fb); fl = wave_max(fl);
    return C + (double)lse2(fb, fl);
}

}  // namespace ctc_chain
