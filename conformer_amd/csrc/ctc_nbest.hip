// conformer_hip3_ctc_nbest.h: the CTC log-likelihood of every row of an n-best list against the ONE logits block of its
// utterance, the gradient of a weighted sum of them, and the MWER risk over the list.
//
//   prepare : one wave per frame (b, t)   -> lse and the blank log-probability once, then the label log-probabilities of the N
//             rows gathered from the same logits row: lpl (B, N, T, Lmax).  The vocabulary is reduced once, not N times.
//   alpha   : one wave per (b, n), the chain of ctc_chain.h (the loss's own) -> ll (B, N) float64.
//   beta    : the mirror chain, only for the rows the gradient counts (used, finite ll, weight != 0).
//   grad    : one wave per frame: the row starts as -(sum of weights) * softmax in LDS, then the wave walks the N rows of its
//             utterance in order and adds weight_n * occupancy_n folded onto the vocabulary (repeated labels summed by their
//             first occurrence), and stores the row once.  No atomics, a fixed order: two runs give the same bits.
//   risk    : one wave per utterance, lane n = row n, float64 softmax over the live rows; then a one-wave mean.
// HBM-bound on the logits (read twice, the gradient written once); the chains are latency-bound (T sequential steps), B N of
// them side by side.
#include "cfm_common.h"
#include "ctc_chain.h"
#include "conformer_hip3_ctc_nbest.h"

namespace {

using ctc_chain::NEG_INF;

struct NbestArgs {
    const float* logits; const int64_t* hyps; const int64_t* hyp_len; const int64_t* in_len;
    float* lse; float* lpb; float* lpl; float* alpha; float* beta;
    double* ca; double* cb; double* ll;          // per-frame lattice offsets (alpha, beta) and the log-likelihood per row
    double* ll_out;
    const float* weight; float* dlogits;
    int B, N, T, V, Lmax, blank, P;
};

// geometry of utterance b and of its row n, clamped so that no index derived from it can leave a buffer
__device__ __forceinline__ int nbest_frames(const NbestArgs& a, int b) {
    const int64_t t = a.in_len[b];
    return (int)(t < 0 ? 0 : (t > a.T ? a.T : t));
}
__device__ __forceinline__ int nbest_labels(const NbestArgs& a, int64_t row, bool& used) {
    const int64_t L = a.hyp_len[row];
    used = L >= 0;
    return (int)(L < 0 ? 0 : (L > a.Lmax ? a.Lmax : L));
}
__device__ __forceinline__ bool finite_ll(double ll) { return ll > (double)NEG_INF && ll == ll; }

__global__ __launch_bounds__(256) void nbest_prepare_kernel(const NbestArgs a) {
    const int64_t frame = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (frame >= (int64_t)a.B * a.T) return;
    const int b = (int)(frame / a.T), t = (int)(frame - (int64_t)b * a.T);
    if (t >= nbest_frames(a, b)) return;
    const float* row = a.logits + frame * a.V;
    float m = NEG_INF;
    for (int v = lane; v < a.V; v += 64) m = fmaxf(m, row[v]);
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < a.V; v += 64) s += exp_fast(row[v] - m);
    s = wave_sum(s);
    const float lse = m + logf(s);
    if (lane == 0) { a.lse[frame] = lse; a.lpb[frame] = row[a.blank] - lse; }
    for (int n = 0; n < a.N; ++n) {
        const int64_t r = (int64_t)b * a.N + n;
        bool used;
        const int Lb = nbest_labels(a, r, used);
        const int64_t* lab = a.hyps + r * a.Lmax;
        float* out = a.lpl + (r * a.T + t) * a.Lmax;
        for (int i = lane; i < Lb; i += 64) out[i] = row[ctc_chain::clamp_label(lab[i], a.V)] - lse;
    }
}

// One wave per (utterance, row).  BETA runs only where the gradient will read it.
template <int P, bool BETA>
__global__ __launch_bounds__(64) void nbest_chain_kernel(const NbestArgs a) {
    constexpr int NP = 64 * P;
    const int64_t r = blockIdx.x;
    const int b = (int)(r / a.N), lane = threadIdx.x;
    bool used;
    const int Lb = nbest_labels(a, r, used);
    const int Tb = nbest_frames(a, b);
    if (BETA) {
        if (!used || Tb == 0 || !finite_ll(a.ll[r]) || a.weight[r] == 0.f) return;
    } else if (!used || Tb == 0) {
        const double ll = (used && Lb == 0) ? 0.0 : (double)NEG_INF;
        if (lane == 0) { a.ll[r] = ll; a.ll_out[r] = ll; }
        return;
    }
    ctc_chain::Row row;
    row.labels = a.hyps + r * a.Lmax;
    row.lpl = a.lpl + r * a.T * a.Lmax;
    row.lpb = a.lpb + (int64_t)b * a.T;
    row.out = (BETA ? a.beta : a.alpha) + r * a.T * 2 * NP;
    row.coff = (BETA ? a.cb : a.ca) + r * a.T;
    row.Tb = Tb; row.Lb = Lb; row.Lmax = a.Lmax; row.V = a.V;
    const double ll = ctc_chain::run<P, BETA>(row, lane);
    if (!BETA && lane == 0) { a.ll[r] = ll; a.ll_out[r] = ll; }
}

// one wave per frame; dynamic LDS per wave: V floats (the row) + 64P floats (label occupancy) + 64P ints (labels).  Every wave
// of the block walks all N rows and meets every barrier; what a wave has no part in is predicated off.
__global__ __launch_bounds__(256) void nbest_grad_kernel(const NbestArgs a, int waves) {
    extern __shared__ float lds[];
    const int NP = 64 * a.P;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* g = lds + (size_t)w * (a.V + 2 * NP);
    float* occ = g + a.V;
    int* labs = reinterpret_cast<int*>(occ + NP);
    const int64_t frame = (int64_t)blockIdx.x * waves + w;
    const bool in_grid = frame < (int64_t)a.B * a.T;
    const int b = in_grid ? (int)(frame / a.T) : 0, t = in_grid ? (int)(frame - (int64_t)b * a.T) : 0;
    const int Tb = nbest_frames(a, b);
    // lane n holds row n: its weight, zero unless the row counts
    float wn = 0.f;
    if (lane < a.N) {
        const int64_t r = (int64_t)b * a.N + lane;
        const float wt = a.weight[r];
        wn = (a.hyp_len[r] >= 0 && finite_ll(a.ll[r])) ? wt : 0.f;
    }
    const bool any = __ballot(wn != 0.f) != 0;
    const float wsum = wave_sum(wn);
    const bool live = in_grid && t < Tb && any;
    if (live) {
        const float* row = a.logits + frame * a.V;
        const float lse = a.lse[frame];
        for (int v = lane; v < a.V; v += 64) g[v] = -wsum * exp_fast(row[v] - lse);
    }
    float blank_acc = 0.f;
    for (int n = 0; n < a.N; ++n) {
        const float w_n = __shfl(wn, n, 64);
        const bool on = live && w_n != 0.f;                                      // uniform over the wave
        const int64_t r = (int64_t)b * a.N + n;
        bool used;
        const int Lb = nbest_labels(a, r, used);
        if (on) {
            const int64_t rt = r * a.T + t;
            const float* al = a.alpha + (rt * 2) * NP;
            const float* be = a.beta + (rt * 2) * NP;
            const float* lpl = a.lpl + rt * a.Lmax;
            const int64_t* lab = a.hyps + r * a.Lmax;
            const float lpb = a.lpb[frame];
            const float shift = (float)(a.ca[rt] + a.cb[rt] - a.ll[r]);          // offsets of the two lattices - log-likelihood
            float blank_sum = 0.f;
            for (int i = lane; i <= Lb; i += 64) {
                blank_sum += exp_fast((al[2 * i] + be[2 * i]) + (shift - lpb));
                if (i < Lb) {
                    occ[i] = exp_fast((al[2 * i + 1] + be[2 * i + 1]) + (shift - lpl[i]));
                    labs[i] = ctc_chain::clamp_label(lab[i], a.V);
                }
            }
            blank_acc += w_n * wave_sum(blank_sum);
        }
        __syncthreads();
        if (on) {
            for (int i = lane; i < Lb; i += 64) {
                const int li = labs[i];
                bool first = true;
                for (int j = 0; j < i; ++j) first = first && labs[j] != li;
                if (!first) continue;
                float s = 0.f;
                for (int j = i; j < Lb; ++j) s += labs[j] == li ? occ[j] : 0.f;
                g[li] += w_n * s;
            }
        }
        __syncthreads();
    }
    if (live && lane == 0) g[a.blank] += blank_acc;
    __syncthreads();
    if (!in_grid) return;
    float* drow = a.dlogits + frame * a.V;
    if (live) {
        for (int v = lane; v < a.V; v += 64) drow[v] = g[v];
    } else {
        for (int v = lane; v < a.V; v += 64) drow[v] = 0.f;
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// one wave per utterance, lane n = row n (N <= 64)
__global__ __launch_bounds__(64) void mwer_risk_kernel(const double* ll, const int* errors, const int64_t* hyp_len, int B, int N,
                                                       float grad_scale, float* risk, float* weight) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t r = (int64_t)b * N + lane;
    bool live = false;
    double l = (double)NEG_INF, W = 0.0;
    if (lane < N) {
        l = ll[r];
        live = hyp_len[r] >= 0 && finite_ll(l) && l < -(double)NEG_INF;
        W = (double)errors[r];
    }
    const int count = __popcll(__ballot(live));
    const double m = wave_max_f64(live ? l : (double)NEG_INF);
    const double e = live ? exp(l - m) : 0.0;
    const double Z = wave_sum_f64(e);
    const bool scored = count >= 2;
    const double P = scored ? e / Z : 0.0;
    const double R = wave_sum_f64(P * W);
    const double Wbar = wave_sum_f64(live ? W : 0.0) / (double)max(count, 1);
    // W_n - R_b as sum_m P_m (W_n - W_m): no cancellation against R when one row holds nearly all of the mass, and exactly 0
    // when every row has the same count
    double gap = 0.0;
    for (int j = 0; j < N; ++j) gap += __shfl(P, j, 64) * (W - __shfl(W, j, 64));
    if (lane < N) weight[r] = (scored && live) ? (float)((double)grad_scale * P * gap / (double)B) : 0.f;
    if (lane == 0) risk[b] = scored ? (float)(R - Wbar) : 0.f;
}

__global__ __launch_bounds__(64) void mwer_mean_kernel(const float* risk, int B, float* loss) {
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += 64) s += risk[b];
    s = wave_sum(s);
    if (threadIdx.x == 0) loss[0] = s / (float)B;
}

template <bool BETA>
void launch_chain(const NbestArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((int64_t)a.B * a.N)), block(64);
    switch (a.P) {
        case 1: hipLaunchKernelGGL((nbest_chain_kernel<1, BETA>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((nbest_chain_kernel<2, BETA>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((nbest_chain_kernel<4, BETA>), grid, block, 0, s, a); break;
        case 8: hipLaunchKernelGGL((nbest_chain_kernel<8, BETA>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((nbest_chain_kernel<16, BETA>), grid, block, 0, s, a); break;
    }
}

constexpr int64_t kMaxGrid = 2147483647;

int fill_args(NbestArgs& a, const float* logits, const int64_t* hyps, const int64_t* hyp_len, const int64_t* in_len, int B, int N,
              int T, int V, int Lmax, int blank, float* workspace) {
    CFM_REQUIRE(logits && hyps && hyp_len && in_len && workspace, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && N > 0 && T > 0 && V > 0 && Lmax >= 1 && blank >= 0 && blank < V, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(N <= CFM3_CTC_NBEST_MAX && Lmax <= CFM_CTC_MAX_TARGET, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((int64_t)B * T <= kMaxGrid && (int64_t)B * N <= kMaxGrid, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, CFM_ERR_ALIGN);
    a = NbestArgs{};
    a.logits = logits; a.hyps = hyps; a.hyp_len = hyp_len; a.in_len = in_len;
    a.B = B; a.N = N; a.T = T; a.V = V; a.Lmax = Lmax; a.blank = blank; a.P = ctc_chain::pairs_per_lane(Lmax);
    const int64_t frames = (int64_t)B * T, rows = (int64_t)B * N, rt = rows * T, lattice = rt * 2 * 64 * a.P;
    a.ca = reinterpret_cast<double*>(workspace); a.cb = a.ca + rt; a.ll = a.cb + rt;                  // float64 part first
    a.lse = reinterpret_cast<float*>(a.ll + rows); a.lpb = a.lse + frames; a.lpl = a.lpb + frames;
    a.alpha = a.lpl + rt * Lmax; a.beta = a.alpha + lattice;
    return CFM_OK;
}

}  // namespace

extern "C" int64_t cfm3_ctc_nbest_workspace_floats(int B, int N, int T, int Lmax) {
    if (B <= 0 || N <= 0 || T <= 0 || Lmax < 1 || N > CFM3_CTC_NBEST_MAX || Lmax > CFM_CTC_MAX_TARGET) return -1;
    if ((int64_t)B * T > kMaxGrid || (int64_t)B * N > kMaxGrid) return -1;
    const int64_t frames = (int64_t)B * T, rows = (int64_t)B * N, rt = rows * T;
    return 2 * (2 * rt + rows) + 2 * frames + rt * Lmax + 2 * rt * 2 * 64 * ctc_chain::pairs_per_lane(Lmax);
}

extern "C" int cfm3_ctc_nbest_score_f32(const float* logits, const int64_t* hyps, const int64_t* hyp_len, const int64_t* in_len,
                                        int B, int N, int T, int V, int Lmax, int blank, float* workspace, double* ll,
                                        cfm_stream_t stream) {
    CFM_REQUIRE(ll, CFM_ERR_NULL);
    NbestArgs a;
    const int rc = fill_args(a, logits, hyps, hyp_len, in_len, B, N, T, V, Lmax, blank, workspace);
    if (rc != CFM_OK) return rc;
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(ll) & 7) == 0, CFM_ERR_ALIGN);
    a.ll_out = ll;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t frames = (int64_t)B * T;
    hipLaunchKernelGGL(nbest_prepare_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, a);
    launch_chain<false>(a, s);
    return cfm_launch_status();
}

extern "C" int cfm3_ctc_nbest_grad_f32(const float* logits, const int64_t* hyps, const int64_t* hyp_len, const int64_t* in_len,
                                       int B, int N, int T, int V, int Lmax, int blank, float* workspace, const float* weight,
                                       float* dlogits, cfm_stream_t stream) {
    CFM_REQUIRE(weight && dlogits, CFM_ERR_NULL);
    NbestArgs a;
    const int rc = fill_args(a, logits, hyps, hyp_len, in_len, B, N, T, V, Lmax, blank, workspace);
    if (rc != CFM_OK) return rc;
    a.weight = weight; a.dlogits = dlogits;
    const size_t per_wave = ((size_t)V + 2 * 64 * (size_t)a.P) * sizeof(float);
    CFM_REQUIRE(per_wave <= 64 * 1024, CFM_ERR_UNSUPPORTED);
    const int waves = 4 * per_wave <= 64 * 1024 ? 4 : (2 * per_wave <= 64 * 1024 ? 2 : 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_chain<true>(a, s);
    const int64_t frames = (int64_t)B * T;
    hipLaunchKernelGGL(nbest_grad_kernel, dim3((unsigned)((frames + waves - 1) / waves)), dim3(64 * waves), waves * per_wave, s,
                       a, waves);
    return cfm_launch_status();
}

extern "C" int cfm3_mwer_risk_f32(const double* ll, const int* errors, const int64_t* hyp_len, int B, int N, float grad_scale,
                                  float* risk, float* loss, float* weight, cfm_stream_t stream) {
    CFM_REQUIRE(ll && errors && hyp_len && risk && loss && weight, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && N > 0, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(N <= CFM3_CTC_NBEST_MAX, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(ll) & 7) == 0, CFM_ERR_ALIGN);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(mwer_risk_kernel, dim3((unsigned)B), dim3(64), 0, s, ll, errors, hyp_len, B, N, grad_scale, risk, weight);
    hipLaunchKernelGGL(mwer_mean_kernel, dim3(1), dim3(64), 0, s, risk, B, loss);
    return cfm_launch_status();
}
