// Windowed relative-position attention over RING K/V caches, fp32 (cfm_relpos_attention_window_f32; bounded-history streaming).
//
// The 4-wave form of relpos_attn_fwd_kernel (attention_f32.hip) in coordinates LOCAL to a slot's step: the same transposed
// v_mfma_f32_32x32x2_f32 content / band / P.V products, the same per-wave skew tile with the carried band tile, the same
// double-buffered K / V staging with one workgroup barrier per key tile.  What differs:
//   local key   c  <->  absolute frame j = q_begin[b] - left + c, ring row (q_begin[b] - left + c) mod R
//   local query il <->  absolute frame i = q_begin[b] + il,       sits at local position il + left
//   relative position r = i - j = il + left - c, table row P - 1 - r
//   query il sees the keys  max(il, cmin) <= c < cend,  cmin = max(0, left - q_begin[b]) (frame 0), cend = left + q_count[b]
// Only (q_begin[b] - left) mod R is 64-bit arithmetic; every other index is a small int whatever the stream position.
//   * A workgroup (query rows q0 .. q0+127) walks the key tiles from max(q0, cmin) / 32 to cend / 32: <= (left + 128)/32 + 2.
//     A wave joins at ITS first visible tile, max(i0, cmin) / 32 (it computes that tile's band tile 1 explicitly, as the first
//     tile of the full-context kernel does); every row of the wave has a visible key in that tile.  Rows past the slot's count
//     (il >= q_count) may see no key at all: the running-max update takes 0 for an all-masked maximum, so it yields no NaN.
//   * Ring rows outside [cmin, cend) hold an older part of the stream or another stream: they are never loaded -- the staging
//     selects zeros for them -- and masked keys inside the range are selected away before the exponential, so no bit pattern of a
//     masked row reaches a result.
#include "attention_tile_f32.h"
#include "../../include/conformer_hip_window.h"

namespace {

using namespace attn_tile;

struct WinArgs {
    const float* q; const float* k; const float* v; int64_t ld;
    const float* pos; int64_t ldp; const float* u; const float* vb;
    const int64_t* q_begin; const int64_t* q_count; float* ctx; int64_t ldo;
    int B, R, P, H, dh, q_max, left; float inv_sqrt_dh;
};

template <int NC, int ND>
__global__ __launch_bounds__(256, 2) void relpos_attn_window_kernel(const WinArgs a) {
    constexpr int NW = 4;
    __shared__ __attribute__((aligned(16))) float smem[2 * 32 * KROW + 2 * 32 * 64 + NW * 32 * 32];
    float* Ksb = smem;                           // [2][32][KROW]
    float* Vsb = Ksb + 2 * 32 * KROW;            // [2][32][64]
    float* gs = Vsb + 2 * 32 * 64 + (threadIdx.x >> 6) * 1024;   // per-wave skew tile [32][32]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, hf = lane >> 5;
    const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
    const int R = a.R, P = a.P, dh = a.dh, left = a.left;
    // the device values are clamped, never trusted
    const int64_t qb = max(a.q_begin[b], (int64_t)0);
    const int qn = (int)min(max(a.q_count[b], (int64_t)0), (int64_t)a.q_max);
    const int q0 = (int)blockIdx.x * 32 * NW;
    const int i0 = q0 + wave * 32;
    const bool active = i0 < qn;                                         // wave-uniform; idle waves still stage + barrier
    auto zero_fill = [&]() {                                             // compact rows [qn, q_max) are zeros
        const int il = i0 + li;
        if (il >= a.q_max) return;
        zero_row<ND>(a.ctx + ((int64_t)b * a.q_max + il) * a.ldo + h * dh, dh, hf);
    };
    if (q0 >= qn) {                                                      // no query row of this slot here: Q / K / V unread
        zero_fill();
        return;
    }
    const int cmin = (int)max((int64_t)0, (int64_t)left - qb);           // local index of frame 0, or 0: <= left
    const int cend = left + qn;                                          // > cmin (qn >= 1 here)
    const int64_t off = (qb - left) % R;
    const int base = (int)(off < 0 ? off + R : off);                     // ring row of local key 0
    // ring row of local index c in [cmin, cend): base + c < 2R because c < left + q_max <= R
    auto ring_row = [&](int c) { const int x = base + c; return x >= R ? x - R : x; };
    const int kt_begin = max(q0, cmin) >> 5;                             // the workgroup's key tiles: [kt_begin, ntiles)
    const int ntiles = (cend + 31) >> 5;                                 // > kt_begin: q0 < qn <= cend, cmin < cend
    const int kt_w = max(i0, cmin) >> 5;                                 // the wave's first tile with a visible key

    const float* kbase = a.k + (int64_t)b * R * a.ld + h * dh;
    const float* vbase = a.v + (int64_t)b * R * a.ld + h * dh;
    const float* pbase = a.pos + h * dh;
    const int jmax = 2 * P - 2;

    // ---- cooperative staging: thread -> (row srow + 16*pass, 16-byte chunk sch) of a 32-row x 256-byte tile
    constexpr int RPP = 4 * NW, SP = 32 / RPP;
    const int srow = tid >> 4, sch = tid & 15;
    const bool sok = sch * 4 < dh;
    f32x4 pk[SP], pv[SP];
    auto prefetch = [&](int kt) {                                  // K/V tile kt -> registers; rows outside [cmin, cend) are zeros
        const int k0 = kt * 32;
#pragma unroll
        for (int p = 0; p < SP; ++p) {
            const int c = k0 + srow + RPP * p;
            const int64_t row = ring_row(min(max(c, cmin), cend - 1));
            const bool ok = sok && c >= cmin && c < cend;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            pk[p] = ok ? *reinterpret_cast<const f32x4*>(kbase + row * a.ld + sch * 4) : z;
            pv[p] = ok ? *reinterpret_cast<const f32x4*>(vbase + row * a.ld + sch * 4) : z;
        }
    };
    prefetch(kt_begin);
    commit<RPP>(Ksb, Vsb, 0, srow, sch, pk, pv);
    if (kt_begin + 1 < ntiles) prefetch(kt_begin + 1);
    __syncthreads();

    // ---- (Q+u)^T and (Q+v)^T as MFMA B operands: lane (query li, half hf) holds dims 8c+4hf+e at step 4c+e
    float qu[4 * NC], qv[4 * NC];
    {
        const int qi = min(i0 + li, qn - 1);                             // (rows past the count read the last row, store nothing)
        const float* qrow = a.q + ((int64_t)b * R + ring_row(left + qi)) * a.ld + h * dh;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int dd = 8 * c + 4 * hf;
            f32x4 x = {0.f, 0.f, 0.f, 0.f}, uu = x, vv = x;
            if (dd < dh) {
                x = *reinterpret_cast<const f32x4*>(qrow + dd);
                uu = *reinterpret_cast<const f32x4*>(a.u + h * dh + dd);
                vv = *reinterpret_cast<const f32x4*>(a.vb + h * dh + dd);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { qu[4 * c + e] = x[e] + uu[e]; qv[4 * c + e] = x[e] + vv[e]; }
        }
    }

    f32x16 o[ND];
#pragma unroll
    for (int n = 0; n < ND; ++n) o[n] = zero_tile();
    float mrow = -INFINITY, lrow = 0.f;                              // running maximum in the log2 domain (scores * scale2), row sum
    const float scale2 = a.inv_sqrt_dh * 1.44269504088896340736f;

    // ---- positional band G^T[jj][query], jj = 32*mt + row <-> table row j = jbase - jj, jbase = P-1-(i0+left)+k0+31, and the
    // relative shift as a per-lane column skew through the per-wave LDS tile; band tile 1 of key tile kt+1 is band tile 0 of key
    // tile kt, carried in registers (skp) -- see attention_f32.hip.  Table rows outside [0, 2P-2] belong to pairs outside every
    // window (r > left or r <= -q_max) and read a clamped row.
    const int jq = P - 1 - (i0 + left) + 31;                         // jbase of key tile kt: jq + 32 kt
    float skp[16];                                                   // band tile 1 of the current key tile, skewed (carried)
    f32x4 pf[NC];                                                    // table rows of a band tile in the A-operand layout
    if (active) {                                                    // the wave's first key tile: its band tile 1, explicitly
        band_load(pbase, a.ldp, jmax, dh, jq + 32 * kt_w, 1, li, hf, pf);
        spill_band(gs, li, hf, band_mma(pf, qv));
        skew_reads(gs, li, hf, skp);
        skew_reads_done();
    }
    const int lo = max(i0 + li, cmin);                               // this lane's query sees the local keys [lo, cend)
    const int lo_wave = max(i0 + 31, cmin);                          // the largest lower bound in the wave

    for (int kt = kt_begin; kt < ntiles; ++kt) {
        const int buf = (kt - kt_begin) & 1;
        // stage the NEXT key tile into the other buffer (its last readers passed the barrier that ended tile kt-1), then
        // request the one after it
        if (kt + 1 < ntiles) {
            commit<RPP>(Ksb, Vsb, buf ^ 1, srow, sch, pk, pv);
            if (kt + 2 < ntiles) prefetch(kt + 2);
        }
        if (active && kt >= kt_w) {
            const int k0 = kt * 32;
            // ---- phase 1: content scores S^T[key][query] and band tile 0, spilled to the wave's skew tile
            const float* Ks = Ksb + buf * 32 * KROW;
            band_load(pbase, a.ldp, jmax, dh, jq + k0, 0, li, hf, pf);
            f32x16 sc = lds_mma<NC>(Ks + li * KROW + 4 * hf, qu);
            spill_band(gs, li, hf, band_mma(pf, qv));
            // ---- phase 2: relative shift, scale + window mask, online softmax, O^T += V^T . P^T
            const float* Vs = Vsb + buf * 32 * 64;
            float skn[16];
            skew_reads(gs, li, hf, skn);
            skew_reads_done();                                      // the tile is rewritten by the next key tile
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jj = li - acc_row(r, hf) + 31;
                sc[r] += (jj >> 5) ? skp[r] : skn[r];
                skp[r] = skn[r];
            }
            float p[16];
            float tmax = -INFINITY;
            if (k0 < lo_wave || k0 + 32 > cend) {                   // (wave-uniform) a tile that holds an edge of some row's window
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = k0 + acc_row(r, hf);
                    const float s = (c >= lo && c < cend) ? sc[r] * scale2 : -INFINITY;     // a select: masked scores are never used
                    p[r] = s;
                    tmax = fmaxf(tmax, s);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) { p[r] = sc[r] * scale2; tmax = fmaxf(tmax, p[r]); }
            }
            const float mnew = running_max(mrow, tmax);
            // a row that has seen no key yet (only rows past the slot's count) keeps m = -inf: subtract 0, so alpha = p = 0, no NaN
            // (deliberately not the full-context kernels' arithmetic: they subtract mnew itself, their first key tile always holds a
            //  valid key.  The update below is otherwise theirs, written out here: see attention_tile_f32.h for why)
            const float msub = mnew == -INFINITY ? 0.f : mnew;
            const float alpha = __builtin_amdgcn_exp2f(mrow - msub);
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(p[r] - msub); psum += p[r]; }
            psum += __shfl_xor(psum, 32, 64);
            lrow = lrow * alpha + psum;
            mrow = mnew;
            rescale(o, alpha);
            // O^T += V^T . P^T ; MFMA step s contracts key (s&3)+8*(s>>2)+4*hf = the key held in register s
#pragma unroll
            for (int n = 0; n < ND; ++n)
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const float vv = Vs[((s & 3) + 8 * (s >> 2) + 4 * hf) * 64 + ((32 * n + li) & 63)];
                    o[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, p[s], o[n], 0, 0, 0);
                }
        }
        // one barrier per key tile: tile kt+1 (written above) is visible, tile kt's buffer may be overwritten next round
        if (kt + 1 < ntiles) __syncthreads();
    }

    // ---- normalise and store: lane = query row, registers = head dims (4 consecutive dims per r>>2 group)
    if (active && i0 + li < qn) {
        const float inv = 1.0f / lrow;
        float* orow = a.ctx + ((int64_t)b * a.q_max + i0 + li) * a.ldo + h * dh;
#pragma unroll
        for (int n = 0; n < ND; ++n)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int dd = 32 * n + 8 * gq + 4 * hf;
                if (dd < dh) {
                    f32x4 out = {o[n][4 * gq] * inv, o[n][4 * gq + 1] * inv, o[n][4 * gq + 2] * inv, o[n][4 * gq + 3] * inv};
                    *reinterpret_cast<f32x4*>(orow + dd) = out;
                }
            }
    } else {
        zero_fill();
    }
}

}  // namespace

extern "C" int cfm_relpos_attention_window_f32(const float* q, const float* k, const float* v, int64_t ld, const float* pos,
                                               int64_t ldp, int P, const float* u, const float* vbias, const int64_t* q_begin,
                                               const int64_t* q_count, float* ctx, int64_t ldo, int B, int R, int H, int dh,
                                               int q_max, int left, cfm_stream_t stream) {
    CFM_REQUIRE(q && k && v && pos && u && vbias && q_begin && q_count && ctx, CFM_ERR_NULL);
    CFM_REQUIRE(B > 0 && R > 0 && H > 0 && dh > 0 && (dh & 3) == 0, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE((ld & 3) == 0 && (ldp & 3) == 0 && (ldo & 3) == 0 && ldo >= (int64_t)H * dh, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE(dh <= 64, CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(CFM_ALIGNED16(q) && CFM_ALIGNED16(k) && CFM_ALIGNED16(v) && CFM_ALIGNED16(pos) && CFM_ALIGNED16(u) &&
                CFM_ALIGNED16(vbias) && CFM_ALIGNED16(ctx), CFM_ERR_ALIGN);
    CFM_REQUIRE((int64_t)B * H <= 65535 && R < (1 << 28) && P < (1 << 28), CFM_ERR_UNSUPPORTED);
    CFM_REQUIRE(q_max >= 1 && left >= 0 && (R & 31) == 0, CFM_ERR_BAD_SHAPE);
    CFM_REQUIRE((int64_t)R >= (int64_t)left + q_max, CFM_ERR_BAD_SHAPE);          // no visible key overwritten by this step's rows
    CFM_REQUIRE(P >= left + 1 && P >= q_max, CFM_ERR_BAD_SHAPE);                   // table rows for r in (-q_max, left]
    const WinArgs a{q, k, v, ld, pos, ldp, u, vbias, q_begin, q_count, ctx, ldo, B, R, P, H, dh, q_max, left,
                    1.0f / sqrtf((float)dh)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((q_max + 127) / 128), (unsigned)(B * H)), block(256);
    for_head_dim(dh, [&](auto nc, auto nd) {
        hipLaunchKernelGGL((relpos_attn_window_kernel<decltype(nc)::value, decltype(nd)::value>), grid, block, 0, s, a);
    });
    return cfm_launch_status();
}
