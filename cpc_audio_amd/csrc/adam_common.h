// The element-wise Adam update shared by the one-launch optimiser (adam.hip) and the fused probe step (probe.hip): one
// definition, so that both produce the same bits from the same gradient.
//   m <- m + (1 - b1)(g - m)          (torch's lerp form)
//   v <- b2 v + (1 - b2) g g
//   p <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),      bc_i = 1 - b_i^step   (computed by the host in double)
#pragma once
#include "cpc_common.h"

namespace cpc {

struct AdamCoef { float b1c, b2, b2c, step_size, inv_bc2_sqrt, eps; };

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamCoef& c) {
    m = m + c.b1c * (g - m);
    v = c.b2 * v + c.b2c * g * g;
    const float denom = sqrtf(v) * c.inv_bc2_sqrt + c.eps;
    p = p - c.step_size * m / denom;
}

// formed in double like torch does (1 - 0.999f would already be off by 1.3e-5 relative), rounded to fp32 once
static inline AdamCoef adam_coef_from(double lr, double beta1, double beta2, double eps, double bias_correction1,
                                      double bias_correction2_sqrt) {
    AdamCoef c;
    c.b1c = (float)(1. - beta1); c.b2 = (float)beta2; c.b2c = (float)(1. - beta2);
    c.step_size = (float)(lr / bias_correction1); c.inv_bc2_sqrt = (float)(1. / bias_correction2_sqrt); c.eps = (float)eps;
    return c;
}

}  // namespace cpc
