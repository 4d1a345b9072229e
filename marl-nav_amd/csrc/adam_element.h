// adam_element.h - the per-element Adam update and the step's count advance,
// shared by marlnav_adam.hip (adam_advance / adam_apply) and by the finish
// kernels of marlnav_ppo.hip that fold the update into the gradient epilogue
// (DESIGN.md §11, §14). One definition, so both forms run the same fp64
// operation sequence and store the same bits.
#ifndef MARLNAV_ADAM_ELEMENT_H
#define MARLNAV_ADAM_ELEMENT_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

namespace marlnav_adam {

// MarlnavAdamBuffers.state
struct AdamState {
    int64_t step;      // steps taken
    double step_size;  // lr / (1 - beta1^step)
    double bc2_sqrt;   // sqrt(1 - beta2^step)
    double reserved;   // the clipped step's coefficient (below); unused by the unclipped step
};

struct AdamScalars {
    double beta1, beta2, omb1, omb2, eps, step_size, bc2_sqrt;
    bool maximize;
};

// one thread of one launch: the count advanced, the step's scalars published
__device__ __forceinline__ void adam_advance_one(AdamState *s, double lr, double beta1,
                                                 double beta2)
{
    const int64_t k = s->step + 1;
    s->step = k;
    const double bc1 = 1.0 - pow(beta1, (double)k);
    const double bc2 = 1.0 - pow(beta2, (double)k);
    s->step_size = lr / bc1;
    s->bc2_sqrt = sqrt(bc2);
}

__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v,
                                             const AdamScalars &c)
{
    const double gd = c.maximize ? -(double)g : (double)g;
    m = (float)__builtin_fma(c.beta1, (double)m, c.omb1 * gd);
    v = (float)__builtin_fma(c.beta2, (double)v, (c.omb2 * gd) * gd);
    const double denom = sqrt((double)v) / c.bc2_sqrt + c.eps;
    p = (float)((double)p - c.step_size * ((double)m / denom));
}

// ---- global-norm clipping. AdamState.reserved carries the
// coefficient from the launch that forms the norm to the launch that applies it.

// torch.nn.utils.clip_grad_norm_'s coefficient, its 1e-6 included. A NaN
// quotient (a non-finite norm) stays NaN: error_if_nonfinite=False poisons
// the step, as it does there.
__device__ __forceinline__ double clip_coef(double norm, double max_norm)
{
    const double q = max_norm / (norm + 1e-6);
    return q > 1.0 ? 1.0 : q;
}

// the gradient as stored back into .grad: coef == 1.0 returns g's own bits
__device__ __forceinline__ float clipped_grad(float g, double coef)
{
    return (float)((double)g * coef);
}

}  // namespace marlnav_adam

#endif  // MARLNAV_ADAM_ELEMENT_H
