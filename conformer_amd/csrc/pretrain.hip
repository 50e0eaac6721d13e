// conformer_hip3_pretrain.h: the Gumbel vector quantizer and the contrastive loss of self-supervised pretraining, forward and
// backward.  Gathers, row reductions and fixed-order sums: bandwidth- and latency-bound, no MFMA and no float atomics.
//
//   quant_fwd    : grid (ceil(N / 32), G), 4 waves; a wave takes 8 rows of its group one after the other: argmax of
//                  logits + noise, the two log-sum-exps, the code's row copied to out, the noise-free softmax (or the one-hot)
//                  added into the wave's own (V) slab of LDS.  The four slabs are added in wave order into the block's partial.
//   quant_reduce : ONE workgroup adds the partials in block order, forms the marginal, the perplexity and the coefficients
//                  c[g][v] of the perplexity's gradient.
//   quant_dlogits: grid (ceil(N / 16), G), 256 threads; dout of 16 rows in LDS, thread v walks its codebook row once for all 16
//                  rows (gy), then two block sums per row (<gy, y>, <p, c>) and the store.
//   quant_dcode  : one workgroup per code; scans codes 256 rows at a time (ballots), adds the rows that chose it in order.
//   con_norms    : one wave per frame, |context| and |targets|.
//   con_frames   : one workgroup per masked frame; the context row in LDS, 16 lanes per candidate, 16 candidates at a time; wave 0
//                  then forms the softmax over the K + 1 similarities.
//   con_sum      : ONE workgroup, the loss and the count.
//   con_dcontext : one workgroup per frame, walks the K + 1 candidates in order.
//   con_dtargets : one wave per target frame, walks its transposed list in order.
#include "cfm_common.h"
#include "conformer_hip3_pretrain.h"

namespace {

constexpr float kNegInf = -__builtin_huge_valf();
constexpr float kCosEps = 1e-8f, kPerpEps = 1e-7f;
constexpr int64_t kMaxGrid = 2147483647;
constexpr int QW_ROWS = CFM3_QUANT_ROWS / 4;        // rows per wave

struct QuantArgs {
    const float* logits; const float* noise; const float* cv; const uint8_t* row_mask;
    float* lse; float* lse0; float* coef; float* count; float* partial; int* cntpart;
    int* codes; float* out; float* marginal; float* perplexity;
    const int* codes_in; const float* dout; const float* dperp; float* dlogits; float* dcv;
    int N, G, V, dg, nblk;
    float inv_tau;
};

__global__ __launch_bounds__(256) void quant_fwd_kernel(const QuantArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];                                   // 4 slabs of V floats, then 4 ints
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = blockIdx.y, V = a.V;
    float* acc = lds + (size_t)w * V;
    int* cnts = reinterpret_cast<int*>(lds + 4 * (size_t)V);
    for (int v = lane; v < V; v += 64) acc[v] = 0.f;
    int cnt = 0;
    for (int i = 0; i < QW_ROWS; ++i) {
        const int64_t row = (int64_t)blockIdx.x * CFM3_QUANT_ROWS + w * QW_ROWS + i;
        if (row >= a.N) break;                                       // uniform over the wave; the barrier is behind the loop
        const int64_t rg = row * a.G + g;
        const float* l = a.logits + rg * V;
        const float* nz = a.noise ? a.noise + rg * V : nullptr;
        float mx = kNegInf, m0 = kNegInf;
        int bi = lane < V ? lane : 0x7fffffff;
        for (int v = lane; v < V; v += 64) {
            const float lv = l[v], x = nz ? lv + nz[v] : lv;
            if (x > mx) { mx = x; bi = v; }                          // ascending v: the lowest index of the lane's maximum
            m0 = fmaxf(m0, lv);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float omx = __shfl_xor(mx, o, 64);
            const int obi = __shfl_xor(bi, o, 64);
            if (omx > mx || (omx == mx && obi < bi)) { mx = omx; bi = obi; }
        }
        m0 = wave_max(m0);
        const int code = min(max(bi, 0), V - 1);
        float s = 0.f, s0 = 0.f;
        for (int v = lane; v < V; v += 64) {
            const float lv = l[v], x = nz ? lv + nz[v] : lv;
            s += expf((x - mx) * a.inv_tau);
            s0 += expf(lv - m0);
        }
        s = wave_sum(s); s0 = wave_sum(s0);
        const float lse0 = m0 + logf(s0);
        const bool counts = a.row_mask ? a.row_mask[row] != 0 : true;
        if (counts) {
            if (nz) {
                for (int v = lane; v < V; v += 64) acc[v] += expf(l[v] - lse0);
            } else if (lane == (code & 63)) {
                acc[code] += 1.f;
            }
            ++cnt;
        }
        if (lane == 0) { a.codes[rg] = code; a.lse[rg] = mx * a.inv_tau + logf(s); a.lse0[rg] = lse0; }
        const float* src = a.cv + ((int64_t)g * V + code) * a.dg;
        float* dst = a.out + rg * a.dg;
        for (int d = lane; d < a.dg; d += 64) dst[d] = src[d];
    }
    if (lane == 0) cnts[w] = cnt;
    __syncthreads();
    float* part = a.partial + ((int64_t)blockIdx.x * a.G + g) * V;
    for (int v = threadIdx.x; v < V; v += 256) part[v] = ((lds[v] + lds[V + v]) + lds[2 * V + v]) + lds[3 * V + v];
    if (g == 0 && threadIdx.x == 0) a.cntpart[blockIdx.x] = (cnts[0] + cnts[1]) + (cnts[2] + cnts[3]);
}

// the sum of v over the 1024 threads of the block, in a fixed order, returned to every thread
__device__ __forceinline__ float block_sum_1024(float v, float* red /* [16] */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += red[i];
    return s;
}

__global__ __launch_bounds__(1024) void quant_reduce_kernel(const QuantArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];                                   // G V marginals, then 16 floats and 16 ints
    float* red = lds + (size_t)a.G * a.V;
    int* redi = reinterpret_cast<int*>(red + 16);
    const int GV = a.G * a.V;
    int c = 0;
    for (int b = threadIdx.x; b < a.nblk; b += 1024) c += a.cntpart[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) redi[threadIdx.x >> 6] = c;
    __syncthreads();
    c = 0;
    for (int i = 0; i < 16; ++i) c += redi[i];
    const float count = (float)c;
    const float denom = fmaxf(count, 1.f);
    for (int i = threadIdx.x; i < GV; i += 1024) {
        float s = 0.f;
        for (int b = 0; b < a.nblk; ++b) s += a.partial[(int64_t)b * GV + i];
        a.marginal[i] = s;
        lds[i] = s / denom;
    }
    __syncthreads();
    float perp = 0.f;
    for (int g = 0; g < a.G; ++g) {
        float t = 0.f;
        for (int v = threadIdx.x; v < a.V; v += 1024) {
            const float m = lds[g * a.V + v];
            t -= m * logf(m + kPerpEps);
        }
        const float eh = expf(block_sum_1024(t, red));
        perp += eh;
        for (int v = threadIdx.x; v < a.V; v += 1024) {
            const float m = lds[g * a.V + v];
            a.coef[g * a.V + v] = eh * (-logf(m + kPerpEps) - m / (m + kPerpEps)) / denom;
        }
    }
    if (threadIdx.x == 0) { a.perplexity[0] = perp; a.count[0] = count; }
}

template <int VPT>
__global__ __launch_bounds__(256) void quant_dlogits_kernel(const QuantArgs a) {
    constexpr int R = CFM3_QUANT_BWD_ROWS;
    extern __shared__ __attribute__((aligned(16))) float lds[];      // dout tile [dg][R], then red [4][2 R]
    float* tile = lds;
    float* red = lds + (size_t)a.dg * R;
    const int g = blockIdx.y, V = a.V, dg = a.dg, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    for (int i = tid; i < R * dg; i += 256) {
        const int r = i / dg, d = i - r * dg;
        const int64_t row = r0 + r;
        tile[d * R + r] = row < a.N ? a.dout[(row * a.G + g) * dg + d] : 0.f;
    }
    __syncthreads();
    float gy[VPT][R];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
#pragma unroll
        for (int r = 0; r < R; ++r) gy[j][r] = 0.f;
        const int v = tid + 256 * j;
        if (v < V) {
            const float* c = a.cv + ((int64_t)g * V + v) * dg;
            for (int d = 0; d < dg; ++d) {
                const float cd = c[d];
                const f32x4* t4 = reinterpret_cast<const f32x4*>(tile + d * R);
#pragma unroll
                for (int q = 0; q < R / 4; ++q) {
                    const f32x4 t = t4[q];
                    gy[j][4 * q] += cd * t.x; gy[j][4 * q + 1] += cd * t.y;
                    gy[j][4 * q + 2] += cd * t.z; gy[j][4 * q + 3] += cd * t.w;
                }
            }
        }
    }
    // the two sums of every row: <gy, y> and <p, c>
    float s1[R], s2[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { s1[r] = 0.f; s2[r] = 0.f; }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = r0 + r;
        if (row >= a.N) continue;
        const int64_t rg = row * a.G + g;
        const float lse = a.lse[rg], lse0 = a.lse0[rg];
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int v = tid + 256 * j;
            if (v < V) {
                const float lv = a.logits[rg * V + v], x = lv + a.noise[rg * V + v];
                s1[r] += gy[j][r] * expf(x * a.inv_tau - lse);
                s2[r] += expf(lv - lse0) * a.coef[g * V + v];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) { s1[r] = wave_sum(s1[r]); s2[r] = wave_sum(s2[r]); }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) { red[w * 2 * R + r] = s1[r]; red[w * 2 * R + R + r] = s2[r]; }
    }
    __syncthreads();
    const float dperp = a.dperp[0];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = r0 + r;
        if (row >= a.N) continue;
        const int64_t rg = row * a.G + g;
        const float t1 = ((red[r] + red[2 * R + r]) + red[4 * R + r]) + red[6 * R + r];
        const float t2 = ((red[R + r] + red[3 * R + r]) + red[5 * R + r]) + red[7 * R + r];
        const float lse = a.lse[rg], lse0 = a.lse0[rg];
        const float pm = (a.row_mask ? a.row_mask[row] != 0 : true) ? dperp : 0.f;
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int v = tid + 256 * j;
            if (v < V) {
                const float lv = a.logits[rg * V + v], x = lv + a.noise[rg * V + v];
                const float y = expf(x * a.inv_tau - lse), p = expf(lv - lse0);
                a.dlogits[rg * V + v] = a.inv_tau * y * (gy[j][r] - t1) + pm * p * (a.coef[g * V + v] - t2);
            }
        }
    }
}

__global__ __launch_bounds__(256) void quant_dcode_kernel(const QuantArgs a) {
    __shared__ unsigned long long hits[4];
    const int code = blockIdx.x, g = code / a.V, v = code - g * a.V, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    float acc0 = 0.f, acc1 = 0.f;
    for (int64_t base = 0; base < a.N; base += 256) {
        const int64_t row = base + tid;
        const bool hit = row < a.N && a.codes_in[row * a.G + g] == v;
        const unsigned long long bal = __ballot(hit);
        __syncthreads();                                             // the previous round's reads of hits
        if (lane == 0) hits[w] = bal;
        __syncthreads();
        for (int ww = 0; ww < 4; ++ww) {
            unsigned long long m = hits[ww];
            while (m) {                                              // uniform over the block: rows in ascending order
                const int bit = __ffsll((long long)m) - 1;
                m &= m - 1;
                const float* d = a.dout + ((base + ww * 64 + bit) * a.G + g) * a.dg;
                if (tid < a.dg) acc0 += d[tid];
                if (tid + 256 < a.dg) acc1 += d[tid + 256];
            }
        }
    }
    float* out = a.dcv + (int64_t)code * a.dg;
    if (tid < a.dg) out[tid] = acc0;
    if (tid + 256 < a.dg) out[tid + 256] = acc1;
}

// ---- the contrastive loss ----------------------------------------------------------------------------------------------------

struct ConArgs {
    const float* ctx; const float* tgt; const uint8_t* mask; const int* neg; const int64_t* ids;
    float* cn; float* tn; float* p; float* cs;
    float* frame_loss; uint8_t* correct; float* loss; int* n_correct;
    const int64_t* order; const int64_t* start; const float* gframe; float* dctx; float* dtgt;
    int B, T, D, K;
    float inv_temp;
};

__global__ __launch_bounds__(256) void con_norms_kernel(const ConArgs a) {
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= (int64_t)a.B * a.T) return;
    const float* c = a.ctx + f * a.D;
    const float* t = a.tgt + f * a.D;
    float sc = 0.f, st = 0.f;
    for (int d = lane; d < a.D; d += 64) { sc += c[d] * c[d]; st += t[d] * t[d]; }
    sc = wave_sum(sc); st = wave_sum(st);
    if (lane == 0) { a.cn[f] = sqrtf(sc); a.tn[f] = sqrtf(st); }
}

// <ctx, row> over a group of 16 lanes (sub = the lane's place in its group); every lane of the group returns the sum
template <bool VEC>
__device__ __forceinline__ float dot16(const float* ctx, const float* row, int D, int sub) {
    float s = 0.f;
    if (VEC) {
        for (int d = sub * 4; d < D; d += 64) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(ctx + d), r = *reinterpret_cast<const f32x4*>(row + d);
            s += (c.x * r.x + c.y * r.y) + (c.z * r.z + c.w * r.w);
        }
    } else {
        for (int d = sub; d < D; d += 16) s += ctx[d] * row[d];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void con_frames_kernel(const ConArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // the context row (D, padded to 4), then z (K + 1)
    const int64_t f = blockIdx.x;
    const int tid = threadIdx.x, K1 = a.K + 1;
    if (a.mask[f] == 0) {                                            // uniform over the block, before any barrier
        if (tid == 0) { a.frame_loss[f] = 0.f; a.correct[f] = 0; }
        return;
    }
    float* crow = lds;
    float* z = lds + ((a.D + 3) & ~3);
    const int b = (int)(f / a.T), t = (int)(f - (int64_t)b * a.T);
    for (int d = tid; d < a.D; d += 256) crow[d] = a.ctx[f * a.D + d];
    __syncthreads();
    const float cn = a.cn[f];
    const int64_t idp = a.ids ? a.ids[f] : 0;
    const int grp = tid >> 4, sub = tid & 15;
    for (int k0 = 0; k0 < K1; k0 += 16) {
        const int k = k0 + grp;
        const bool valid = k < K1;
        int j = t;
        bool excluded = false;
        if (valid && k > 0) {
            j = a.neg[f * a.K + (k - 1)];
            excluded = j < 0 || j >= a.T;
            if (excluded) j = t;                                     // an absent candidate addresses nothing of its own
            else if (a.ids) excluded = a.ids[(int64_t)b * a.T + j] == idp;
        }
        const int64_t fj = (int64_t)b * a.T + j;
        const float dot = dot16<VEC>(crow, a.tgt + fj * a.D, a.D, sub);
        if (valid && sub == 0) {
            const float cosv = dot / fmaxf(cn * a.tn[fj], kCosEps);
            z[k] = excluded ? kNegInf : cosv * a.inv_temp;
            a.cs[f * K1 + k] = cosv;
        }
    }
    __syncthreads();
    if (tid >= 64) return;
    float m = kNegInf;
    int bi = 0x7fffffff;
    for (int k = tid; k < K1; k += 64) if (z[k] > m) { m = z[k]; bi = k; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int ob = __shfl_xor(bi, o, 64);
        if (om > m || (om == m && ob < bi)) { m = om; bi = ob; }
    }
    float s = 0.f;
    for (int k = tid; k < K1; k += 64) s += expf(z[k] - m);
    s = wave_sum(s);
    const float lse = m + logf(s);
    for (int k = tid; k < K1; k += 64) a.p[f * K1 + k] = expf(z[k] - lse);
    if (tid == 0) {
        a.frame_loss[f] = lse - z[0];
        a.correct[f] = bi == 0 ? 1 : 0;
    }
}

__global__ __launch_bounds__(1024) void con_sum_kernel(const ConArgs a) {
    __shared__ float red[16];
    __shared__ int redi[16];
    const int64_t n = (int64_t)a.B * a.T;
    float s = 0.f;
    int c = 0;
    for (int64_t f = threadIdx.x; f < n; f += 1024) { s += a.frame_loss[f]; c += a.correct[f]; }
    s = wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s; redi[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float ts = 0.f;
        int tc = 0;
        for (int i = 0; i < 16; ++i) { ts += red[i]; tc += redi[i]; }
        a.loss[0] = ts;
        a.n_correct[0] = tc;
    }
}

__global__ __launch_bounds__(256) void con_dcontext_kernel(const ConArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];                                   // per candidate: the row's weight, then its frame
    const int64_t f = blockIdx.x;
    const int tid = threadIdx.x, K1 = a.K + 1, D = a.D;
    float* drow = a.dctx + f * D;
    if (a.mask[f] == 0) {
        for (int d = tid; d < D; d += 256) drow[d] = 0.f;
        return;
    }
    float* wt = lds;
    float* wc = lds + K1;
    int* fr = reinterpret_cast<int*>(lds + 2 * K1);
    const int b = (int)(f / a.T), t = (int)(f - (int64_t)b * a.T);
    const float cn = a.cn[f], g = a.gframe[f];
    for (int k = tid; k < K1; k += 256) {
        int j = t;
        if (k > 0) {
            j = a.neg[f * a.K + (k - 1)];
            if (j < 0 || j >= a.T) j = t;                            // absent: p is 0 there, the row is never read
        }
        const float pk = a.p[f * K1 + k];
        const float w = g * (pk - (k == 0 ? 1.f : 0.f)) * a.inv_temp;
        const float prod = cn * a.tn[(int64_t)b * a.T + j];
        wt[k] = w / fmaxf(prod, kCosEps);
        wc[k] = prod > kCosEps ? w * a.cs[f * K1 + k] : 0.f;
        fr[k] = (k > 0 && pk == 0.f) ? -1 : j;                       // an excluded candidate has p = 0 exactly
    }
    __syncthreads();
    float self = 0.f;                                                // sum_k w_k cos_k over the unclamped candidates
    for (int k = 0; k < K1; ++k) if (fr[k] >= 0) self += wc[k];
    const float sc = cn > 0.f ? self / (cn * cn) : 0.f;
    for (int d = tid; d < D; d += 256) {
        float acc = 0.f;
        for (int k = 0; k < K1; ++k) {
            const int j = fr[k];
            if (j >= 0) acc += wt[k] * a.tgt[((int64_t)b * a.T + j) * D + d];
        }
        drow[d] = acc - sc * a.ctx[f * D + d];
    }
}

template <int DPL>
__global__ __launch_bounds__(256) void con_dtargets_kernel(const ConArgs a) {
    const int64_t n = (int64_t)a.B * a.T, f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), total = n * a.K;
    const int lane = threadIdx.x & 63, K1 = a.K + 1, D = a.D;
    if (f >= n) return;
    const int b = (int)(f / a.T), t = (int)(f - (int64_t)b * a.T);
    const float tn = a.tn[f];
    float acc[DPL];
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[i] = 0.f;
    float self = 0.f;
    if (a.mask[f] != 0) {                                            // its own row, as the positive
        const float w = a.gframe[f] * (a.p[f * K1] - 1.f) * a.inv_temp;
        const float prod = a.cn[f] * tn;
        const float wd = w / fmaxf(prod, kCosEps);
        if (prod > kCosEps) self += w * a.cs[f * K1];
        const float* c = a.ctx + f * D;
#pragma unroll
        for (int i = 0; i < DPL; ++i) { const int d = lane + 64 * i; if (d < D) acc[i] += wd * c[d]; }
    }
    int64_t e0 = a.start[f], e1 = a.start[f + 1];
    e0 = e0 < 0 ? 0 : (e0 > total ? total : e0);
    e1 = e1 < e0 ? e0 : (e1 > total ? total : e1);
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t pos = a.order[e];
        if (pos < 0 || pos >= total) continue;
        const int64_t src = pos / a.K;
        const int k = (int)(pos - src * a.K) + 1;
        // a draw of this frame, by a masked frame of the same utterance; anything else is skipped
        if (src / a.T != b || a.neg[pos] != t || a.mask[src] == 0) continue;
        const float w = a.gframe[src] * a.p[src * K1 + k] * a.inv_temp;
        if (w == 0.f) continue;                                      // excluded by its id, or no gradient
        const float prod = a.cn[src] * tn;
        const float wd = w / fmaxf(prod, kCosEps);
        if (prod > kCosEps) self += w * a.cs[src * K1 + k];
        const float* c = a.ctx + src * D;
#pragma unroll
        for (int i = 0; i < DPL; ++i) { const int d = lane + 64 * i; if (d < D) acc[i] += wd * c[d]; }
    }
    const float st = tn > 0.f ? self / (tn * tn) : 0.f;
    const float* trow = a.tgt + f * D;
    float* out = a.dtgt + f * D;
#pragma unroll
    for (int i = 0; i < DPL; ++i) { const int d = lane + 64 * i; if (d < D) out[d] = acc[i] - st * trow[d]; }
}

inline bool positive_finite(float x) { return x > 0.f && x <= 3.0e38f; }
inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

int quant_check(int N, int G, int V, int dg, float tau, const float* workspace) {
    CFM_REQUIRE(N > 0 && G > 0 && V > 0 && dg > 0 && positive_finite(tau), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(V <= CFM3_PRETRAIN_MAX_V && G <= CFM3_PRETRAIN_MAX_G && dg <= CFM3_PRETRAIN_MAX_DG, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((int64_t)N * G <= kMaxGrid, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(aligned(workspace, 16), CFM_ERR_ALIGN);
    return CFM_OK;
}

void quant_fill(QuantArgs& a, int N, int G, int V, int dg, float tau, float* workspace) {
    a.N = N; a.G = G; a.V = V; a.dg = dg; a.inv_tau = 1.f / tau;
    a.nblk = (N + CFM3_QUANT_ROWS - 1) / CFM3_QUANT_ROWS;
    const int64_t ng = (int64_t)N * G, gv = (int64_t)G * V;
    a.lse = workspace; a.lse0 = a.lse + ng; a.coef = a.lse0 + ng; a.count = a.coef + gv; a.partial = a.count + 4;
    a.cntpart = reinterpret_cast<int*>(a.partial + (int64_t)a.nblk * gv);
}

int con_check(const float* context, const float* targets, int B, int T, int D, int K, float temperature,
              const float* workspace) {
    CFM_REQUIRE(B > 0 && T > 0 && D > 0 && K > 0 && positive_finite(temperature), CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(D <= CFM3_PRETRAIN_MAX_D && K <= CFM3_PRETRAIN_MAX_K, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE((int64_t)B * T * K <= kMaxGrid, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(aligned(workspace, 16), CFM_ERR_ALIGN);
    CFM_REQUIRE(D % 4 != 0 || (aligned(context, 16) && aligned(targets, 16)), CFM_ERR_ALIGN);
    return CFM_OK;
}

void con_fill(ConArgs& a, int B, int T, int D, int K, float temperature, float* workspace) {
    a.B = B; a.T = T; a.D = D; a.K = K; a.inv_temp = 1.f / temperature;
    const int64_t n = (int64_t)B * T;
    a.cn = workspace; a.tn = a.cn + n; a.p = a.tn + n; a.cs = a.p + n * (K + 1);
}

}  // namespace

extern "C" int64_t cfm3_quantize_workspace_floats(int N, int G, int V) {
    if (N <= 0 || G <= 0 || V <= 0 || V > CFM3_PRETRAIN_MAX_V || G > CFM3_PRETRAIN_MAX_G || (int64_t)N * G > kMaxGrid) return -1;
    const int64_t nblk = ((int64_t)N + CFM3_QUANT_ROWS - 1) / CFM3_QUANT_ROWS;
    return 2 * (int64_t)N * G + (int64_t)G * V + 4 + nblk * G * V + nblk;
}

extern "C" int cfm3_quantize_fwd_f32(const float* logits, const float* noise, const float* codevectors, const uint8_t* row_mask,
                                     int N, int G, int V, int dg, float tau, float* workspace, int* codes, float* out,
                                     float* marginal, float* perplexity, cfm_stream_t stream) {
    CFM_REQUIRE(logits && codevectors && workspace && codes && out && marginal && perplexity, CFM_ERR_NULL);
    const int rc = quant_check(N, G, V, dg, tau, workspace);
    if (rc != CFM_OK) return rc;
    QuantArgs a{};
    a.logits = logits; a.noise = noise; a.cv = codevectors; a.row_mask = row_mask;
    a.codes = codes; a.out = out; a.marginal = marginal; a.perplexity = perplexity;
    quant_fill(a, N, G, V, dg, tau, workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(quant_fwd_kernel, dim3((unsigned)a.nblk, (unsigned)G), dim3(256), (4 * (size_t)V + 4) * sizeof(float), s, a);
    hipLaunchKernelGGL(quant_reduce_kernel, dim3(1), dim3(1024), ((size_t)G * V + 32) * sizeof(float), s, a);
    return cfm_launch_status();
}

extern "C" int cfm3_quantize_bwd_f32(const float* logits, const float* noise, const float* codevectors, const uint8_t* row_mask,
                                     const int* codes, const float* dout, const float* dperplexity, int N, int G, int V, int dg,
                                     float tau, float* workspace, float* dlogits, float* dcodevectors, cfm_stream_t stream) {
    CFM_REQUIRE(logits && noise && codevectors && codes && dout && dperplexity && workspace && dlogits && dcodevectors,
                CFM_ERR_NULL);
    const int rc = quant_check(N, G, V, dg, tau, workspace);
    if (rc != CFM_OK) return rc;
    QuantArgs a{};
    a.logits = logits; a.noise = noise; a.cv = codevectors; a.row_mask = row_mask;
    a.codes_in = codes; a.dout = dout; a.dperp = dperplexity; a.dlogits = dlogits; a.dcv = dcodevectors;
    quant_fill(a, N, G, V, dg, tau, workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((N + CFM3_QUANT_BWD_ROWS - 1) / CFM3_QUANT_BWD_ROWS), (unsigned)G), block(256);
    const size_t lds = ((size_t)dg * CFM3_QUANT_BWD_ROWS + 8 * CFM3_QUANT_BWD_ROWS) * sizeof(float);
    switch ((V + 255) / 256) {
        case 1: hipLaunchKernelGGL(quant_dlogits_kernel<1>, grid, block, lds, s, a); break;
        case 2: hipLaunchKernelGGL(quant_dlogits_kernel<2>, grid, block, lds, s, a); break;
        case 3: hipLaunchKernelGGL(quant_dlogits_kernel<3>, grid, block, lds, s, a); break;
        default: hipLaunchKernelGGL(quant_dlogits_kernel<4>, grid, block, lds, s, a); break;
    }
    hipLaunchKernelGGL(quant_dcode_kernel, dim3((unsigned)(G * V)), dim3(256), 0, s, a);
    return cfm_launch_status();
}

extern "C" int64_t cfm3_contrastive_workspace_floats(int B, int T, int K) {
    if (B <= 0 || T <= 0 || K <= 0 || K > CFM3_PRETRAIN_MAX_K || (int64_t)B * T * K > kMaxGrid) return -1;
    return 2 * (int64_t)B * T * (K + 2);
}

extern "C" int cfm3_contrastive_fwd_f32(const float* context, const float* targets, const uint8_t* mask, const int* negatives,
                                        const int64_t* ids, int B, int T, int D, int K, float temperature, float* workspace,
                                        float* frame_loss, uint8_t* correct, float* loss, int* n_correct, cfm_stream_t stream) {
    CFM_REQUIRE(context && targets && mask && negatives && workspace && frame_loss && correct && loss && n_correct, CFM_ERR_NULL);
    const int rc = con_check(context, targets, B, T, D, K, temperature, workspace);
    if (rc != CFM_OK) return rc;
    ConArgs a{};
    a.ctx = context; a.tgt = targets; a.mask = mask; a.neg = negatives; a.ids = ids;
    a.frame_loss = frame_loss; a.correct = correct; a.loss = loss; a.n_correct = n_correct;
    con_fill(a, B, T, D, K, temperature, workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)B * T;
    hipLaunchKernelGGL(con_norms_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, a);
    const size_t lds = ((size_t)((D + 3) & ~3) + K + 1) * sizeof(float);
    if (D % 4 == 0) hipLaunchKernelGGL(con_frames_kernel<true>, dim3((unsigned)n), dim3(256), lds, s, a);
    else hipLaunchKernelGGL(con_frames_kernel<false>, dim3((unsigned)n), dim3(256), lds, s, a);
    hipLaunchKernelGGL(con_sum_kernel, dim3(1), dim3(1024), 0, s, a);
    return cfm_launch_status();
}

extern "C" int cfm3_contrastive_bwd_f32(const float* context, const float* targets, const uint8_t* mask, const int* negatives,
                                        const int64_t* order, const int64_t* start, const float* gframe, int B, int T, int D,
                                        int K, float temperature, float* workspace, float* dcontext, float* dtargets,
                                        cfm_stream_t stream) {
    CFM_REQUIRE(context && targets && mask && negatives && order && start && gframe && workspace && dcontext && dtargets,
                CFM_ERR_NULL);
    const int rc = con_check(context, targets, B, T, D, K, temperature, workspace);
    if (rc != CFM_OK) return rc;
    CFM_REQUIRE(aligned(order, 8) && aligned(start, 8), CFM_ERR_ALIGN);
    ConArgs a{};
    a.ctx = context; a.tgt = targets; a.mask = mask; a.neg = negatives;
    a.order = order; a.start = start; a.gframe = gframe; a.dctx = dcontext; a.dtgt = dtargets;
    con_fill(a, B, T, D, K, temperature, workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)B * T;
    hipLaunchKernelGGL(con_dcontext_kernel, dim3((unsigned)n), dim3(256), (3 * (size_t)(K + 1)) * sizeof(float), s, a);
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    const int dpl = (D + 63) / 64;
    if (dpl <= 1) hipLaunchKernelGGL(con_dtargets_kernel<1>, grid, block, 0, s, a);
    else if (dpl <= 2) hipLaunchKernelGGL(con_dtargets_kernel<2>, grid, block, 0, s, a);
    else if (dpl <= 4) hipLaunchKernelGGL(con_dtargets_kernel<4>, grid, block, 0, s, a);
    else if (dpl <= 8) hipLaunchKernelGGL(con_dtargets_kernel<8>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(con_dtargets_kernel<16>, grid, block, 0, s, a);
    return cfm_launch_status();
}
