// conformer_hip3_rnnt.h: the transducer loss over joint logits (B, T, U1, V) and its gradient, the joint network's combine and
// the bookkeeping of the greedy decode.
//
//   rows     : a group of LPR lanes (8 .. 64, by V) per live (b, t, u) -> lse, lpb, lpl.  One pass with an online max / sum, 16-byte
//              loads where the rows are 16-byte aligned (V % 4 == 0); rows outside the live lattice are not read.
//   lattice  : one workgroup per utterance and direction (blockIdx.y: 0 alpha, 1 beta), lane u walks the anti-diagonals t + u = d
//              in float64.  The value of lane u -+ 1 comes through a double-buffered LDS row (one barrier per step); the two
//              log-probabilities of the next step are loaded before the barrier of this one.
//   grad     : a group per (b, t, u), dead ones included (they store zeros): x is read once, dlogits written once.  The exponents
//              alpha + beta - ll are formed in float64 and are <= 0 up to rounding; the V-wide arithmetic is fp32.
//   joint    : h[b,t] (U1 J contiguous) = tanh(e[b,t'] (J, repeated) + p[b] (U1 J contiguous)); backward: one kernel sums over u,
//              one over t (four t-slices folded in a fixed order through LDS).
//   greedy   : decide (one wave per utterance: argmax, then lane 0 does the bookkeeping), commit (state copy under the emit mask;
//              block 0 counts the utterances still running).
// HBM-bound on the logits (read twice, the gradient written once); the lattice is a latency chain of T + U1 - 1 steps.
#include "cfm_common.h"
#include "ctc_chain.h"
#include "conformer_hip3_rnnt.h"

namespace {

constexpr float NEG_INF = -INFINITY;
constexpr int64_t kMaxGrid = 2147483647;

struct RnntArgs {
    const float* logits; const int64_t* targets; const int64_t* in_len; const int64_t* tg_len;
    double* alpha; double* beta; double* ll;     // (B T U1), (B T U1), (B)
    float* lse; float* lpb; float* lpl;          // (B T U1) each
    double* nll;
    const float* weight; float* dlogits;
    int B, T, U1, V, blank, lpr;
};

// geometry of utterance b, clamped so that no index derived from it can leave a buffer
__device__ __forceinline__ int rnnt_frames(const RnntArgs& a, int b) {
    const int64_t t = a.in_len[b];
    return (int)(t < 0 ? 0 : (t > a.T ? a.T : t));
}
__device__ __forceinline__ int rnnt_labels(const RnntArgs& a, int b) {
    const int64_t u = a.tg_len[b];
    return (int)(u < 0 ? 0 : (u > a.U1 - 1 ? a.U1 - 1 : u));
}
__device__ __forceinline__ int rnnt_label(const RnntArgs& a, int b, int u) {      // u < U_b <= U1 - 1: targets is not null
    return ctc_chain::clamp_label(a.targets[(int64_t)b * (a.U1 - 1) + u], a.V);
}

// reductions over an aligned group of `lpr` lanes (a power of two, 8 .. 64)
__device__ __forceinline__ float group_sum(float v, int lpr) {
    for (int o = lpr >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float group_max(float v, int lpr) {
    for (int o = lpr >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// row r = (b, t, u) of the group this thread belongs to; false behind the grid
__device__ __forceinline__ bool rnnt_row(const RnntArgs& a, int64_t& r, int& b, int& t, int& u, int& lane) {
    const int per_block = 256 / a.lpr;
    r = (int64_t)blockIdx.x * per_block + threadIdx.x / a.lpr;
    lane = threadIdx.x % a.lpr;
    if (r >= (int64_t)a.B * a.T * a.U1) return false;
    const int64_t bt = r / a.U1;
    u = (int)(r - bt * a.U1);
    b = (int)(bt / a.T);
    t = (int)(bt - (int64_t)b * a.T);
    return true;
}

template <bool VEC4>
__global__ __launch_bounds__(256) void rnnt_rows_kernel(const RnntArgs a) {
    int64_t r;
    int b, t, u, lane;
    if (!rnnt_row(a, r, b, t, u, lane)) return;
    const int Ub = rnnt_labels(a, b);
    if (t >= rnnt_frames(a, b) || u > Ub) return;                    // whole groups leave: the shuffles below stay inside a group
    const float* row = a.logits + r * a.V;
    const int blank = a.blank, y = u < Ub ? rnnt_label(a, b, u) : -1;
    float m = -3.0e38f, s = 0.f;                                     // finite: a logit of -inf adds exp(-inf) = 0, never inf - inf
    float xb = NEG_INF, xl = NEG_INF;                                // the blank's and the label's logit, kept by the lane that meets it
    if (VEC4) {
        const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
        for (int i = lane; i < a.V / 4; i += a.lpr) {
            const f32x4 x = row4[i];
            const float mx = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
            if (mx > m) { s *= exp_fast(m - mx); m = mx; }
            s += (exp_fast(x.x - m) + exp_fast(x.y - m)) + (exp_fast(x.z - m) + exp_fast(x.w - m));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (4 * i + k == blank) xb = x[k];
                if (4 * i + k == y) xl = x[k];
            }
        }
    } else {
        for (int v = lane; v < a.V; v += a.lpr) {
            const float x = row[v];
            if (x > m) { s *= exp_fast(m - x); m = x; }
            s += exp_fast(x - m);
            if (v == blank) xb = x;
            if (v == y) xl = x;
        }
    }
    const float M = group_max(m, a.lpr);
    s = group_sum(s * exp_fast(m - M), a.lpr);                       // a lane without an element holds s = 0
    xb = group_max(xb, a.lpr);                                       // one lane holds the value, the others -inf
    xl = group_max(xl, a.lpr);
    if (lane == 0) {
        const float lse = M + logf(s);                                // not finite for a row of -inf only, or with +inf or a NaN
        a.lse[r] = lse;
        a.lpb[r] = xb - lse;
        a.lpl[r] = u < Ub ? xl - lse : NEG_INF;
    }
}

// NaN goes through (fmax and fmin would drop it): a row without a finite lse makes its utterance's ll not finite
__device__ __forceinline__ double logaddexp64(double x, double y) {
    if (x != x || y != y) return x + y;
    const double hi = fmax(x, y), lo = fmin(x, y);
    if (lo == (double)NEG_INF) return hi;                              // also both -inf
    return hi + log1p(exp(lo - hi));
}

// blockIdx.x = utterance, blockIdx.y = direction; blockDim.x >= U1, a multiple of 64.  Lane u owns column u of the lattice.
__global__ __launch_bounds__(1024) void rnnt_lattice_kernel(const RnntArgs a) {
    __shared__ double nb[2][CFM3_RNNT_MAX_U1];
    const int b = blockIdx.x, u = threadIdx.x;
    const bool BETA = blockIdx.y == 1;
    const int Tb = rnnt_frames(a, b), Ub = rnnt_labels(a, b);
    if (Tb == 0) {                                                    // dead: nothing of the workspace but ll is read for it
        if (!BETA && u == 0) { a.ll[b] = (double)NEG_INF; a.nll[b] = (double)INFINITY; }
        return;
    }
    const int64_t base = (int64_t)b * a.T * a.U1;
    const bool lane_on = u <= Ub;
    const int steps = Tb + Ub;                                        // anti-diagonals 0 .. Tb - 1 + Ub
    double own = (double)NEG_INF;                                     // this lane's cell of the previous diagonal
    // the two log-probabilities of step i, loaded one step ahead
    auto fetch = [&](int i, float& fb, float& fl) {
        const int d = BETA ? steps - 1 - i : i;
        const int t = d - u;
        fb = NEG_INF; fl = NEG_INF;
        if (!lane_on || i >= steps || t < 0 || t >= Tb) return;
        if (BETA) {
            fb = a.lpb[base + (int64_t)t * a.U1 + u];
            if (u < Ub) fl = a.lpl[base + (int64_t)t * a.U1 + u];
        } else {
            if (t > 0) fb = a.lpb[base + (int64_t)(t - 1) * a.U1 + u];
            if (u > 0) fl = a.lpl[base + (int64_t)t * a.U1 + u - 1];
        }
    };
    float fb, fl;
    fetch(0, fb, fl);
    for (int i = 0; i < steps; ++i) {                                 // uniform over the block: every lane meets every barrier
        const int d = BETA ? steps - 1 - i : i;
        const int t = d - u;
        const bool on = lane_on && t >= 0 && t < Tb;
        float nfb, nfl;
        fetch(i + 1, nfb, nfl);
        double v = (double)NEG_INF;
        if (on) {
            const double* prev = nb[(i + 1) & 1];                     // written in step i - 1
            if (BETA) {
                if (t == Tb - 1 && u == Ub) {
                    v = (double)fb;
                } else {
                    const double down = t + 1 < Tb ? own + (double)fb : (double)NEG_INF;
                    const double right = u < Ub ? prev[u + 1] + (double)fl : (double)NEG_INF;
                    v = logaddexp64(down, right);
                }
                a.beta[base + (int64_t)t * a.U1 + u] = v;
            } else {
                if (t == 0 && u == 0) {
                    v = 0.0;
                } else {
                    const double up = t > 0 ? own + (double)fb : (double)NEG_INF;
                    const double left = u > 0 ? prev[u - 1] + (double)fl : (double)NEG_INF;
                    v = logaddexp64(up, left);
                }
                a.alpha[base + (int64_t)t * a.U1 + u] = v;
                if (t == Tb - 1 && u == Ub) {
                    const double ll = v + (double)a.lpb[base + (int64_t)t * a.U1 + u];
                    a.ll[b] = ll;
                    a.nll[b] = -ll;
                }
            }
            own = v;
        }
        nb[i & 1][u] = v;                                             // u < blockDim.x <= CFM3_RNNT_MAX_U1
        __syncthreads();
        fb = nfb; fl = nfl;
    }
}

template <bool VEC4>
__global__ __launch_bounds__(256) void rnnt_grad_kernel(const RnntArgs a) {
    int64_t r;
    int b, t, u, lane;
    if (!rnnt_row(a, r, b, t, u, lane)) return;
    const int Tb = rnnt_frames(a, b), Ub = rnnt_labels(a, b);
    float* drow = a.dlogits + r * a.V;
    const double ll = a.ll[b];
    const float w = a.weight[b];
    const bool live = t < Tb && u <= Ub && ll > (double)NEG_INF && ll < (double)INFINITY && w != 0.f;
    if (!live) {
        if (VEC4) {
            f32x4* d4 = reinterpret_cast<f32x4*>(drow);
            for (int i = lane; i < a.V / 4; i += a.lpr) d4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int v = lane; v < a.V; v += a.lpr) drow[v] = 0.f;
        }
        return;
    }
    const float* row = a.logits + r * a.V;
    const float lse = a.lse[r];
    const double al = a.alpha[r] - ll;
    const float gamma = w * exp_fast((float)(al + a.beta[r]));
    float eb = 0.f, el = 0.f;
    if (t + 1 < Tb) eb = exp_fast((float)(al + (double)a.lpb[r] + a.beta[r + a.U1]));
    else if (u == Ub) eb = exp_fast((float)(al + (double)a.lpb[r]));
    int y = -1;
    if (u < Ub) {
        y = rnnt_label(a, b, u);
        el = exp_fast((float)(al + (double)a.lpl[r] + a.beta[r + 1]));
    }
    eb *= w; el *= w;
    const int blank = a.blank;
    if (VEC4) {
        const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
        f32x4* d4 = reinterpret_cast<f32x4*>(drow);
        for (int i = lane; i < a.V / 4; i += a.lpr) {
            const f32x4 x = row4[i];
            f32x4 g;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int v = 4 * i + k;
                g[k] = gamma * exp_fast(x[k] - lse) - (v == blank ? eb : 0.f) - (v == y ? el : 0.f);
            }
            d4[i] = g;
        }
    } else {
        for (int v = lane; v < a.V; v += a.lpr)
            drow[v] = gamma * exp_fast(row[v] - lse) - (v == blank ? eb : 0.f) - (v == y ? el : 0.f);
    }
}

// ---- the joint ---------------------------------------------------------------------------------------------------------------------

// one block per (b, t): the U1 J contiguous outputs of h[b,t]
template <bool VEC4>
__global__ __launch_bounds__(256) void rnnt_joint_fwd_kernel(const float* __restrict__ e, const float* __restrict__ p,
                                                             const int64_t* __restrict__ frames, float* __restrict__ h, int Te,
                                                             int T, int U1, int J) {
    const int64_t bt = blockIdx.x;
    const int b = (int)(bt / T), t = (int)(bt - (int64_t)b * T);
    int te = t;
    if (frames) {
        const int64_t f = frames[b] + t;
        te = (int)(f < 0 ? 0 : (f > Te - 1 ? Te - 1 : f));
    }
    const float* er = e + ((int64_t)b * Te + te) * J;
    const float* pr = p + (int64_t)b * U1 * J;
    float* hr = h + bt * U1 * J;
    const int n = U1 * J;
    if (VEC4) {
        const int J4 = J / 4;
        for (int i = threadIdx.x; i < n / 4; i += 256) {
            const f32x4 x = reinterpret_cast<const f32x4*>(er)[i % J4], y = reinterpret_cast<const f32x4*>(pr)[i];
            reinterpret_cast<f32x4*>(hr)[i] = f32x4{tanhf(x.x + y.x), tanhf(x.y + y.y), tanhf(x.z + y.z), tanhf(x.w + y.w)};
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) hr[i] = tanhf(er[i % J] + pr[i]);
    }
}

// de[b,t,j] = sum_u dh (1 - h^2): one block per (b, t), thread j walks u in order
__global__ __launch_bounds__(256) void rnnt_joint_de_kernel(const float* __restrict__ h, const float* __restrict__ dh,
                                                            float* __restrict__ de, int U1, int J) {
    const int64_t bt = blockIdx.x;
    const float* hr = h + bt * U1 * J;
    const float* gr = dh + bt * U1 * J;
    for (int j = threadIdx.x; j < J; j += 256) {
        float s = 0.f;
        for (int u = 0; u < U1; ++u) {
            const float hv = hr[(int64_t)u * J + j];
            s += gr[(int64_t)u * J + j] * (1.f - hv * hv);
        }
        de[bt * J + j] = s;
    }
}

// dp[b,u,j] = sum_t dh (1 - h^2): blockIdx.x = (b, u), blockIdx.y = chunks of 64 columns; wave s sums the frames t = s, s + 4, ..
// in order, then the four partial sums are added in the order of s
__global__ __launch_bounds__(256) void rnnt_joint_dp_kernel(const float* __restrict__ h, const float* __restrict__ dh,
                                                            float* __restrict__ dp, int T, int U1, int J) {
    __shared__ float part[4][64];
    const int64_t bu = blockIdx.x;
    const int b = (int)(bu / U1), u = (int)(bu - (int64_t)b * U1);
    const int s = threadIdx.x >> 6;
    for (int64_t c0 = (int64_t)blockIdx.y * 64; c0 < J; c0 += (int64_t)gridDim.y * 64) {     // uniform over the block
        const int j = (int)c0 + (threadIdx.x & 63);
        float acc = 0.f;
        if (j < J) {
            for (int t = s; t < T; t += 4) {
                const int64_t at = (((int64_t)b * T + t) * U1 + u) * J + j;
                const float hv = h[at];
                acc += dh[at] * (1.f - hv * hv);
            }
        }
        part[s][threadIdx.x & 63] = acc;
        __syncthreads();
        if (s == 0 && j < J)
            dp[bu * J + j] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
        __syncthreads();
    }
}

// ---- the greedy decode's bookkeeping -----------------------------------------------------------------------------------------------

__device__ __forceinline__ int clamp_frames(int64_t t, int T) { return (int)(t < 0 ? 0 : (t > T ? T : t)); }

// one wave per utterance
__global__ __launch_bounds__(64) void rnnt_greedy_decide_kernel(const float* __restrict__ logits, const int64_t* __restrict__ in_len,
                                                                int V, int T, int blank, int max_symbols, int64_t* tokens,
                                                                int64_t* frames, int64_t* count, int64_t* last, int64_t* tpos,
                                                                int64_t* nsym, int* emit) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = clamp_frames(in_len[b], T);
    const int t = clamp_frames(tpos[b], T);
    if (t >= Tb) {                                                    // finished (uniform over the wave)
        if (lane == 0) emit[b] = 0;
        return;
    }
    const float* row = logits + (int64_t)b * V;
    float best = NEG_INF;
    int arg = V;                                                       // a row of NaNs picks nothing and counts as blank
    for (int v = lane; v < V; v += 64) {
        const float x = row[v];
        if (x > best) { best = x; arg = v; }                          // strict: the lowest index of a lane's equals
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane != 0) return;
    const int64_t cap = (int64_t)T * max_symbols;
    int64_t c = count[b], n = nsym[b];
    c = c < 0 ? 0 : (c > cap ? cap : c);
    n = n < 0 ? 0 : n;
    if (arg < V && arg != blank && n < max_symbols && c < cap) {
        tokens[(int64_t)b * cap + c] = arg;
        frames[(int64_t)b * cap + c] = t;
        count[b] = c + 1;
        nsym[b] = n + 1;
        last[b] = arg;
        emit[b] = 1;
    } else {
        tpos[b] = t + 1;
        nsym[b] = 0;
        emit[b] = 0;
    }
}

__global__ __launch_bounds__(256) void rnnt_greedy_commit_kernel(const float* __restrict__ state_new, float* __restrict__ state_cur,
                                                                 const int* __restrict__ emit, const int64_t* __restrict__ tpos,
                                                                 const int64_t* __restrict__ in_len, int planes, int B, int H, int T,
                                                                 int* active) {
    const int64_t n = (int64_t)planes * B * H;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int b = (int)((i / H) % B);
        if (emit[b]) state_cur[i] = state_new[i];
    }
    if (blockIdx.x == 0) {
        __shared__ int part[4];
        int c = 0;
        for (int b = threadIdx.x; b < B; b += 256) c += clamp_frames(tpos[b], T) < clamp_frames(in_len[b], T) ? 1 : 0;
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) active[0] = part[0] + part[1] + part[2] + part[3];
    }
}

int lanes_per_row(int V) {
    int lpr = 8;
    while (lpr < 64 && lpr * 4 < V) lpr *= 2;
    return lpr;
}

int fill_args(RnntArgs& a, const float* logits, const int64_t* targets, const int64_t* in_len, const int64_t* tg_len, int B, int T,
              int U1, int V, int blank, float* workspace) {
    CFM_REQUIRE(logits && in_len && tg_len && workspace && (targets || U1 <= 1), CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && T > 0 && U1 > 0 && V > 0 && blank >= 0 && blank < V, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(U1 <= CFM3_RNNT_MAX_U1, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((int64_t)B * T * U1 <= kMaxGrid, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, CFM_ERR_ALIGN);
    a = RnntArgs{};
    a.logits = logits; a.targets = targets; a.in_len = in_len; a.tg_len = tg_len;
    a.B = B; a.T = T; a.U1 = U1; a.V = V; a.blank = blank; a.lpr = lanes_per_row(V);
    const int64_t n = (int64_t)B * T * U1;
    a.alpha = reinterpret_cast<double*>(workspace); a.beta = a.alpha + n; a.ll = a.beta + n;          // float64 part first
    a.lse = reinterpret_cast<float*>(a.ll + B); a.lpb = a.lse + n; a.lpl = a.lpb + n;
    return CFM_OK;
}

unsigned row_blocks(const RnntArgs& a) {
    const int64_t per_block = 256 / a.lpr, n = (int64_t)a.B * a.T * a.U1;
    return (unsigned)((n + per_block - 1) / per_block);
}

}  // namespace

extern "C" int64_t cfm3_rnnt_workspace_floats(int B, int T, int U1) {
    if (B <= 0 || T <= 0 || U1 <= 0 || U1 > CFM3_RNNT_MAX_U1) return -1;
    if ((int64_t)B * T > kMaxGrid || (int64_t)B * T * U1 > kMaxGrid) return -1;
    const int64_t n = (int64_t)B * T * U1;
    return 2 * (2 * n + B) + 3 * n;
}

extern "C" int cfm3_rnnt_loss_fwd_f32(const float* logits, const int64_t* targets, const int64_t* in_len, const int64_t* tg_len,
                                      int B, int T, int U1, int V, int blank, float* workspace, double* nll, cfm_stream_t stream) {
    CFM_REQUIRE(nll, CFM_ERR_NULL);
    RnntArgs a;
    const int rc = fill_args(a, logits, targets, in_len, tg_len, B, T, U1, V, blank, workspace);
    if (rc != CFM_OK) return rc;
    CFM_REQUIRE((reinterpret_cast<uintptr_t>(nll) & 7) == 0, CFM_ERR_ALIGN);
    a.nll = nll;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (V % 4 == 0 && CFM_ALIGNED16(logits)) hipLaunchKernelGGL(rnnt_rows_kernel<true>, dim3(row_blocks(a)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(rnnt_rows_kernel<false>, dim3(row_blocks(a)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(rnnt_lattice_kernel, dim3((unsigned)B, 2), dim3((unsigned)((U1 + 63) / 64 * 64)), 0, s, a);
    return cfm_launch_status();
}

extern "C" int cfm3_rnnt_loss_bwd_f32(const float* logits, const int64_t* targets, const int64_t* in_len, const int64_t* tg_len,
                                      int B, int T, int U1, int V, int blank, float* workspace, const float* weight, float* dlogits,
                                      cfm_stream_t stream) {
    CFM_REQUIRE(weight && dlogits, CFM_ERR_NULL);
    RnntArgs a;
    const int rc = fill_args(a, logits, targets, in_len, tg_len, B, T, U1, V, blank, workspace);
    if (rc != CFM_OK) return rc;
    a.weight = weight; a.dlogits = dlogits;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (V % 4 == 0 && CFM_ALIGNED16(logits) && CFM_ALIGNED16(dlogits))
        hipLaunchKernelGGL(rnnt_grad_kernel<true>, dim3(row_blocks(a)), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(rnnt_grad_kernel<false>, dim3(row_blocks(a)), dim3(256), 0, s, a);
    return cfm_launch_status();
}

extern "C" int cfm3_rnnt_joint_fwd_f32(const float* e, const float* p, const int64_t* frames, float* h, int B, int Te, int T, int U1,
                                       int J, cfm_stream_t stream) {
    CFM_REQUIRE(e && p && h, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && Te > 0 && T > 0 && U1 > 0 && J > 0 && (frames || T <= Te), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE((int64_t)B * T <= kMaxGrid && (int64_t)B * U1 <= kMaxGrid && (int64_t)U1 * J <= kMaxGrid, CFM_ERR_UNSUPPORTED);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((int64_t)B * T));
    if (J % 4 == 0 && CFM_ALIGNED16(e) && CFM_ALIGNED16(p) && CFM_ALIGNED16(h))
        hipLaunchKernelGGL(rnnt_joint_fwd_kernel<true>, grid, dim3(256), 0, s, e, p, frames, h, Te, T, U1, J);
    else
        hipLaunchKernelGGL(rnnt_joint_fwd_kernel<false>, grid, dim3(256), 0, s, e, p, frames, h, Te, T, U1, J);
    return cfm_launch_status();
}

extern "C" int cfm3_rnnt_joint_bwd_f32(const float* h, const float* dh, float* de, float* dp, int B, int T, int U1, int J,
                                       cfm_stream_t stream) {
    CFM_REQUIRE(h && dh && de && dp, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && T > 0 && U1 > 0 && J > 0, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE((int64_t)B * T <= kMaxGrid && (int64_t)B * U1 <= kMaxGrid && (int64_t)U1 * J <= kMaxGrid,
                CFM_ERR_UNSUPPORTED);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(rnnt_joint_de_kernel, dim3((unsigned)((int64_t)B * T)), dim3(256), 0, s, h, dh, de, U1, J);
    const int chunks = (int)(((int64_t)J + 63) / 64);                 // of 64 columns; the kernel strides over them past 65535
    hipLaunchKernelGGL(rnnt_joint_dp_kernel, dim3((unsigned)((int64_t)B * U1), (unsigned)(chunks < 65535 ? chunks : 65535)),
                       dim3(256), 0, s, h, dh, dp, T, U1, J);
    return cfm_launch_status();
}

extern "C" int cfm3_rnnt_greedy_decide(const float* logits, const int64_t* in_len, int B, int V, int T, int blank, int max_symbols,
                                       int64_t* tokens, int64_t* frames, int64_t* count, int64_t* last, int64_t* t, int64_t* nsym,
                                       int* emit, cfm_stream_t stream) {
    CFM_REQUIRE(logits && in_len && tokens && frames && count && last && t && nsym && emit, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && V > 0 && T > 0 && max_symbols > 0 && blank >= 0 && blank < V, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE((int64_t)T * max_symbols <= kMaxGrid, CFM_ERR_UNSUPPORTED);
    hipLaunchKernelGGL(rnnt_greedy_decide_kernel, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream), logits, in_len, V,
                       T, blank, max_symbols, tokens, frames, count, last, t, nsym, emit);
    return cfm_launch_status();
}

extern "C" int cfm3_rnnt_greedy_commit(const float* state_new, float* state_cur, const int* emit, const int64_t* t,
                                       const int64_t* in_len, int planes, int B, int H, int T, int* active, cfm_stream_t stream) {
    CFM_REQUIRE(state_new && state_cur && emit && t && in_len && active, CFM_ERR_NULL);
    CFM_REQUIRE(planes > 0 && B > 0 && H > 0 && T > 0, CFM_ERR_BAD_SHAPE);
    const int64_t n = (int64_t)planes * B * H;
    const unsigned blocks = (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(rnnt_greedy_commit_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), state_new, state_cur,
                       emit, t, in_len, planes, B, H, T, active);
    return cfm_launch_status();
}
