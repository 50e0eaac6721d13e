// Carried LSTM state (streaming): the kernel the carried forward entries of lstm.hip and lstm_mfma16.hip run after their steps.
#pragma once
#include "cfm_common.h"

namespace {

// h_state[b] = y[b, n_b - 1] for the utterances that consumed n_b >= 1 frames (the others keep their state): the carried h
// after the chunk.
__global__ __launch_bounds__(256) void lstm_h_out_kernel(const float* __restrict__ y, const int64_t* __restrict__ lengths,
                                                         float* __restrict__ h_state, int B, int T, int H) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * H) return;
    const int b = (int)(i / H), u = (int)(i % H);
    const int n = lengths ? (int)min((int64_t)T, max((int64_t)0, lengths[b])) : T;
    if (n > 0) h_state[i] = y[((int64_t)b * T + n - 1) * H + u];
}

}  // namespace
