// The tile steps the fp32 relative-position attention forward kernels share (relpos_attn_fwd_kernel and relpos_attn_fwd8p_kernel in
// attention_f32.hip, relpos_attn_window_kernel in attention_window_f32.hip), and the head-dimension ladder of their launchers.
//
// Every product is a v_mfma_f32_32x32x2_f32 in the TRANSPOSED orientation: keys / band rows / head dims on the MFMA row axis, the
// wave's 32 queries on the lane axis.  Lane = (query li = lane & 31, half hf = lane >> 5); accumulator register r of a lane holds
// tile row acc_row(r, hf).  A step takes what it uses as parameters and keeps the order of its floating-point operations: the
// kernels that call it stay bit-identical to each other wherever they were.  What is NOT here is what makes a kernel that kernel:
// the keys and queries it walks, its mask, ring or linear addressing, the staggering / pipelining schedule, the key split, dropout,
// the trace stamps, the 8-wave positional ring and the two-chain accumulation of the staggered 8-wave form.
// A step lives here only where moving it left the device code of every instantiation with the same register, LDS and scratch figures
// and the same counts of matrix, LDS, global-memory, wait and barrier instructions.  The (Q+u) / (Q+v) operand load, the carried-band
// merge, the scale-and-mask loops, the exp2 / row-sum update and the P.V product did not pass that bar (the compiler schedules the
// loop in a helper differently from the loop in the kernel body), so each kernel still writes them out: a change to one of them has
// to be made in all three ("The fp32 attention forward's shared tile steps").
#pragma once
#include "cfm_common.h"
#include <math.h>
#include <type_traits>

namespace attn_tile {

constexpr int KROW = 68;                 // padded LDS row (floats) of a K tile / ring block: conflict-free ds_read_b128 fragment reads

// accumulator register r (0..15) of lane half hf -> row of the 32x32 tile (= the key of a score tile, the MFMA step of P.V).
// (The V reads of the P.V loops keep this map as a literal: through the call their LDS offsets are no longer folded.)
__device__ __forceinline__ int acc_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

__device__ __forceinline__ f32x16 zero_tile() {
    f32x16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.f;
    return t;
}

// staged K/V registers -> LDS buffer `buf`: thread (row srow + RPP*pass, 16-byte chunk sch)
template <int RPP, int SP>
__device__ __forceinline__ void commit(float* Ksb, float* Vsb, int buf, int srow, int sch, const f32x4 (&pk)[SP], const f32x4 (&pv)[SP]) {
#pragma unroll
    for (int p = 0; p < SP; ++p) {
        const int r = srow + RPP * p;
        *reinterpret_cast<f32x4*>(Ksb + buf * 32 * KROW + r * KROW + sch * 4) = pk[p];
        *reinterpret_cast<f32x4*>(Vsb + buf * 32 * 64 + r * 64 + sch * 4) = pv[p];
    }
}

// one accumulation chain over an A operand in LDS: `frag` = the lane's row + 4*hf of a KROW-padded tile (a K tile: content scores
// against qu; a ring block: a band tile against qv), fragments by ds_read_b128
template <int NC>
__device__ __forceinline__ f32x16 lds_mma(const float* frag, const float (&qb)[4 * NC]) {
    f32x16 acc = zero_tile();
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const f32x4 f = *reinterpret_cast<const f32x4*>(frag + 8 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f[e], qb[4 * c + e], acc, 0, 0, 0);
    }
    return acc;
}

// band tile mt of the key tile with base row jbase: table rows j = jbase - (32 mt + li), straight from global memory into the
// A-operand layout (lane (row li, half hf) holds dims 8c + 4hf + e); rows outside [0, jmax] belong to (query, key) pairs that do
// not exist and read a clamped row.  Unconditional (clamped) loads + select: no branches, no drained waits.
template <int NC>
__device__ __forceinline__ void band_load(const float* pbase, int64_t ldp, int jmax, int dh, int jbase, int mt, int li, int hf,
                                          f32x4 (&pf)[NC]) {
    const int j = max(0, min(jbase - (32 * mt + li), jmax));
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(pbase + (int64_t)j * ldp + min(8 * c + 4 * hf, dh - 4));
        pf[c] = 8 * c + 4 * hf < dh ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int NC>
__device__ __forceinline__ f32x16 band_mma(const f32x4 (&pf)[NC], const float (&qv)[4 * NC]) {
    f32x16 ga = zero_tile();
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) ga = __builtin_amdgcn_mfma_f32_32x32x2f32(pf[c][e], qv[4 * c + e], ga, 0, 0, 0);
    return ga;
}

// The relative shift S^T[kk][i] += G^T[i - kk + 31][i] as a per-lane column skew through the wave's LDS tile gs [32][32] (every
// lane only touches its own bank): the band tile is spilled, then lane (query li) reads row (jj & 31), jj = li - kk + 31, for ALL of
// its 16 keys kk; jj >> 5 says which band tile owns the key (the carried-band merge in the kernels).
__device__ __forceinline__ void spill_band(float* gs, int li, int hf, const f32x16& ga) {
#pragma unroll
    for (int r = 0; r < 16; ++r) gs[acc_row(r, hf) * 32 + li] = ga[r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void skew_reads(const float* gs, int li, int hf, float (&dst)[16]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int jj = li - acc_row(r, hf) + 31;     // 0..62
        dst[r] = gs[(jj & 31) * 32 + li];
    }
}

// the skew reads have landed before the tile is rewritten
__device__ __forceinline__ void skew_reads_done() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the row's running maximum after this tile (a row = the two lane halves of a query)
__device__ __forceinline__ float running_max(float mrow, float tmax) {
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    return fmaxf(mrow, tmax);
}

template <int ND>
__device__ __forceinline__ void rescale(f32x16 (&o)[ND], float alpha) {
#pragma unroll
    for (int n = 0; n < ND; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[n][r] *= alpha;
}

// normalise and store one row: lane = query row, registers = head dims (4 consecutive dims per r>>2 group)
template <int ND>
__device__ __forceinline__ void store_row(float* orow, int dh, int hf, const f32x16 (&o)[ND], float inv) {
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
}

// a compact row past its slot's count: zeros
template <int ND>
__device__ __forceinline__ void zero_row(float* orow, int dh, int hf) {
#pragma unroll
    for (int n = 0; n < ND; ++n)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int dd = 32 * n + 8 * gq + 4 * hf;
            if (dd < dh) *reinterpret_cast<f32x4*>(orow + dd) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
}

// host: head dimension -> (NC, ND) = (8-dim contraction slices, 32-dim output tiles), handed to f as integral constants
template <class F>
inline void for_head_dim(int dh, F&& f) {
    using std::integral_constant;
    if (dh <= 8) f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
    else if (dh <= 16) f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
    else if (dh <= 32) f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
    else if (dh <= 40) f(integral_constant<int, 5>{}, integral_constant<int, 2>{});
    else f(integral_constant<int, 8>{}, integral_constant<int, 2>{});
}

}  // namespace attn_tile
