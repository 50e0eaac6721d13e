/*
 * conformer_hip3_adam.h -- third-generation entry of libconformer_hip.so: the fused multi-tensor Adam step of
 * cfm_adam_step_f32 (include/conformer_hip.h, "next" row N2) from DOUBLE scalars.  Same conventions as
 * include/conformer_hip.h; the third generation is described in conformer_hip3_align_wild.h.  The entry is ADDED to the
 * library: CFM_ABI_VERSION does not move and cfm_adam_step_f32 computes what it always did.
 *
 * Why.  cfm_adam_step_f32 takes beta1 and beta2 as floats and forms 1 - beta from them.  That difference is exact for the
 * float, but the float is not the caller's beta: 1 - (float)0.999 = 0.00099998713, 1.3e-5 below 1 - 0.999, while the bias
 * corrections the caller hands in come from the double.  exp_avg_sq then sits 1.3e-5 below torch.optim.Adam's on the first
 * steps (exp_avg, with beta1 = 0.9: 2.4e-7 above).  Here lr, beta1, beta2, eps, bias_c1 = 1 - beta1^t and
 * sqrt_bias_c2 = sqrt(1 - beta2^t) (t: the step count after the increment) arrive as doubles, 1 - beta1 and 1 - beta2 are
 * formed in double, and each of the seven values the kernel computes with is rounded to fp32 once.  Per element, in fp32:
 *      exp_avg'    = exp_avg + (grad - exp_avg) * (1 - beta1)
 *      exp_avg_sq' = beta2 * exp_avg_sq + ((1 - beta2) * grad) * grad
 *      param'      = param - ((lr / bias_c1) * exp_avg') / (sqrt(exp_avg_sq') / sqrt_bias_c2 + eps)
 * Arguments, limits, refusals (CFM_ERR_NULL: tensors or a pointer of a descriptor null; CFM_ERR_BAD_SHAPE: n_tensors < 1,
 * a numel < 1, bias_c1 or sqrt_bias_c2 not above 0 after rounding to fp32; all before the first launch) and launches
 * (ceil(n_tensors / 48), the table in the kernel arguments) are those of cfm_adam_step_f32.
 */
#ifndef CONFORMER_HIP3_ADAM_H
#define CONFORMER_HIP3_ADAM_H

#include "../../include/conformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int cfm3_adam_step_f32(const cfm_adam_tensor* tensors, int n_tensors, double lr, double beta1, double beta2, double eps,
                       double bias_c1, double sqrt_bias_c2, cfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
