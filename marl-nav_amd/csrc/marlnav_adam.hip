// marlnav_adam.hip - the optimiser half of a PPO minibatch update on gfx950:
// torch.optim.Adam as the reference constructs it (marlnav/models.py:71-74:
// weight_decay 0, amsgrad False; maximize=True for the actor) over all
// parameter tensors of one network in one launch, with the step count on the
// device, and the one-call updates that enqueue marlnav_ppo.hip's loss and
// gradient kernels and this step back to back.
//
// Two launches per step. adam_advance (one thread) adds 1 to the count in the
// state block and publishes the step's two scalars, lr / (1 - beta1^k) and
// sqrt(1 - beta2^k), in fp64. adam_apply reads them: stream order puts every
// read after the one write, and no thread of adam_apply writes the block, so
// no thread reads a count that another thread of its launch writes.
//
// adam_apply: the tensor table travels by value; the slots' elements are cut
// into items of 4 and thread = item over all slots (grid = ceil(items / 256)).
// An item of a slot whose four pointers are 16-byte aligned is one float4 load
// per stream and one float4 store per output; any other item (an unaligned
// slot, a slot's short last item) walks its 1..4 elements one by one. Nothing
// outside [0, numel) of a slot is read or written.
//
// Numerics: each element is updated in fp64 from the fp32 inputs and m, v, p
// are rounded to fp32 once on the store; p is computed from the stored
// (rounded) m and v, so a run continued from a checkpoint repeats the run
// that was not interrupted. No atomics, no reduction: equal inputs give equal
// bits. Built with -ffp-contract=off: the FMAs below are explicit.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/marlnav.h"

__attribute__((visibility("hidden"))) int marlnav_internal_fail(int code, const char *msg);

namespace {

constexpr int kThreads = 256;
constexpr int kSlots = MARLNAV_ADAM_MAX_TENSORS;
constexpr int64_t kMaxElements = (int64_t)1 << 40;  // all slots together

// MarlnavAdamBuffers.state
struct AdamState {
    int64_t step;      // steps taken
    double step_size;  // lr / (1 - beta1^step)
    double bc2_sqrt;   // sqrt(1 - beta2^step)
    double reserved;
};

struct AdamArgs {
    float *param[kSlots];
    const float *grad[kSlots];
    float *exp_avg[kSlots];
    float *exp_avg_sq[kSlots];
    int64_t numel[kSlots];
    int64_t item_end[kSlots];  // items of slots 0..i; unused slots repeat the total
    const AdamState *state;
    double beta1, beta2, omb1, omb2, eps;  // omb = 1 - beta
    uint32_t vec_mask;  // bit i: the four pointers of slot i are 16-byte aligned
    int maximize;
};

__global__ void __launch_bounds__(64) adam_advance(AdamState *s, double lr, double beta1,
                                                    double beta2)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t k = s->step + 1;
    s->step = k;
    const double bc1 = 1.0 - pow(beta1, (double)k);
    const double bc2 = 1.0 - pow(beta2, (double)k);
    s->step_size = lr / bc1;
    s->bc2_sqrt = sqrt(bc2);
}

struct AdamScalars {
    double beta1, beta2, omb1, omb2, eps, step_size, bc2_sqrt;
    bool maximize;
};

__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v,
                                             const AdamScalars &c)
{
    const double gd = c.maximize ? -(double)g : (double)g;
    m = (float)__builtin_fma(c.beta1, (double)m, c.omb1 * gd);
    v = (float)__builtin_fma(c.beta2, (double)v, (c.omb2 * gd) * gd);
    const double denom = sqrt((double)v) / c.bc2_sqrt + c.eps;
    p = (float)((double)p - c.step_size * ((double)m / denom));
}

__global__ void __launch_bounds__(kThreads) adam_apply(AdamArgs a)
{
    const int64_t item = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (item >= a.item_end[kSlots - 1]) return;
    // the slot of this item: a chain of selects over the by-value table
    float *p = a.param[0];
    const float *g = a.grad[0];
    float *m = a.exp_avg[0];
    float *v = a.exp_avg_sq[0];
    int64_t n = a.numel[0], first = 0;
    bool vec = a.vec_mask & 1u;
#pragma unroll
    for (int i = 1; i < kSlots; ++i)
        if (item >= a.item_end[i - 1]) {  // never true for an unused slot
            p = a.param[i];
            g = a.grad[i];
            m = a.exp_avg[i];
            v = a.exp_avg_sq[i];
            n = a.numel[i];
            first = a.item_end[i - 1];
            vec = (a.vec_mask >> i) & 1u;
        }
    AdamScalars c;
    c.beta1 = a.beta1;
    c.beta2 = a.beta2;
    c.omb1 = a.omb1;
    c.omb2 = a.omb2;
    c.eps = a.eps;
    c.step_size = a.state->step_size;
    c.bc2_sqrt = a.state->bc2_sqrt;
    c.maximize = a.maximize != 0;

    const int64_t e0 = (item - first) * 4;  // < n: a slot has ceil(n / 4) items
    const int64_t left = n - e0;
    if (vec && left >= 4) {
        float4 p4 = *reinterpret_cast<const float4 *>(p + e0);
        const float4 g4 = *reinterpret_cast<const float4 *>(g + e0);
        float4 m4 = *reinterpret_cast<const float4 *>(m + e0);
        float4 v4 = *reinterpret_cast<const float4 *>(v + e0);
        adam_element(p4.x, g4.x, m4.x, v4.x, c);
        adam_element(p4.y, g4.y, m4.y, v4.y, c);
        adam_element(p4.z, g4.z, m4.z, v4.z, c);
        adam_element(p4.w, g4.w, m4.w, v4.w, c);
        *reinterpret_cast<float4 *>(m + e0) = m4;
        *reinterpret_cast<float4 *>(v + e0) = v4;
        *reinterpret_cast<float4 *>(p + e0) = p4;
    } else {
        const int cnt = left < 4 ? (int)left : 4;
        for (int j = 0; j < cnt; ++j) {
            float pj = p[e0 + j], mj = m[e0 + j], vj = v[e0 + j];
            adam_element(pj, g[e0 + j], mj, vj, c);
            m[e0 + j] = mj;
            v[e0 + j] = vj;
            p[e0 + j] = pj;
        }
    }
}

// ---- host side
int fail_slot(const char *fmt, int slot, long long value)
{
    char msg[256];
    snprintf(msg, sizeof(msg), fmt, slot, value);
    return marlnav_internal_fail(MARLNAV_EINVAL, msg);
}

int fail_real(const char *fmt, double value)
{
    char msg[256];
    snprintf(msg, sizeof(msg), fmt, value);
    return marlnav_internal_fail(MARLNAV_EINVAL, msg);
}

inline uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

int check_adam(const MarlnavAdamDims *d, const MarlnavAdamBuffers *b)
{
    if (!d) return marlnav_internal_fail(MARLNAV_EINVAL, "adam dims is NULL");
    if (d->num_tensors < 1 || d->num_tensors > kSlots)
        return fail_slot("adam: num_tensors=%d outside [1, %lld]", d->num_tensors, kSlots);
    if (d->maximize != 0 && d->maximize != 1)
        return fail_slot("adam: maximize=%d must be 0 or 1", d->maximize, 0);
    int64_t total = 0;
    for (int i = 0; i < d->num_tensors; ++i) {
        if (d->numel[i] < 1) return fail_slot("adam: numel[%d]=%lld < 1", i, d->numel[i]);
        if (d->numel[i] > kMaxElements - total)
            return fail_slot("adam: numel[%d]=%lld brings the table past 2^40 elements", i,
                             d->numel[i]);
        total += d->numel[i];
    }
    if (!(d->lr >= 0.0) || !__builtin_isfinite(d->lr))
        return fail_real("adam: lr=%g must be finite and >= 0", d->lr);
    if (!(d->beta1 >= 0.0 && d->beta1 < 1.0))
        return fail_real("adam: beta1=%g outside [0, 1)", d->beta1);
    if (!(d->beta2 >= 0.0 && d->beta2 < 1.0))
        return fail_real("adam: beta2=%g outside [0, 1)", d->beta2);
    if (!(d->eps >= 0.0) || !__builtin_isfinite(d->eps))
        return fail_real("adam: eps=%g must be finite and >= 0", d->eps);
    if (d->reserved != 0)
        return fail_real("adam: reserved=%.0f must be 0", (double)d->reserved);
    if (!b) return marlnav_internal_fail(MARLNAV_EINVAL, "adam buffers is NULL");
    for (int i = 0; i < d->num_tensors; ++i) {
        const void *ptr[4] = {b->param[i], b->grad[i], b->exp_avg[i], b->exp_avg_sq[i]};
        const char *null_fmt[4] = {"adam: buffer param[%d] is NULL", "adam: buffer grad[%d] is NULL",
                                   "adam: buffer exp_avg[%d] is NULL",
                                   "adam: buffer exp_avg_sq[%d] is NULL"};
        const char *align_fmt[4] = {"adam: buffer param[%d] must be 4-byte aligned",
                                    "adam: buffer grad[%d] must be 4-byte aligned",
                                    "adam: buffer exp_avg[%d] must be 4-byte aligned",
                                    "adam: buffer exp_avg_sq[%d] must be 4-byte aligned"};
        for (int k = 0; k < 4; ++k) {
            if (!ptr[k]) return fail_slot(null_fmt[k], i, 0);
            if (addr(ptr[k]) & 3u) return fail_slot(align_fmt[k], i, 0);
        }
    }
    if (!b->state) return marlnav_internal_fail(MARLNAV_EINVAL, "adam: buffer state is NULL");
    if (addr(b->state) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "adam: buffer state must be 8-byte aligned");
    return 0;
}

// checked arguments only
int enqueue_adam(const MarlnavAdamDims *d, const MarlnavAdamBuffers *b, hipStream_t s)
{
    AdamArgs a;
    int64_t items = 0;
    a.vec_mask = 0;
    for (int i = 0; i < kSlots; ++i) {
        const bool used = i < d->num_tensors;
        a.param[i] = used ? b->param[i] : nullptr;
        a.grad[i] = used ? b->grad[i] : nullptr;
        a.exp_avg[i] = used ? b->exp_avg[i] : nullptr;
        a.exp_avg_sq[i] = used ? b->exp_avg_sq[i] : nullptr;
        a.numel[i] = used ? d->numel[i] : 0;
        if (used) {
            items += (d->numel[i] + 3) / 4;
            if (((addr(b->param[i]) | addr(b->grad[i]) | addr(b->exp_avg[i]) |
                  addr(b->exp_avg_sq[i])) & 15u) == 0)
                a.vec_mask |= 1u << i;
        }
        a.item_end[i] = items;
    }
    AdamState *state = static_cast<AdamState *>(b->state);
    a.state = state;
    a.beta1 = d->beta1;
    a.beta2 = d->beta2;
    a.omb1 = 1.0 - d->beta1;
    a.omb2 = 1.0 - d->beta2;
    a.eps = d->eps;
    a.maximize = d->maximize;
    hipLaunchKernelGGL(adam_advance, dim3(1), dim3(64), 0, s, state, d->lr, d->beta1, d->beta2);
    // items <= 2^38 + 8: the grid fits 31 bits
    hipLaunchKernelGGL(adam_apply, dim3((unsigned)((items + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return marlnav_internal_fail(MARLNAV_ELAUNCH, hipGetErrorString(e));
    return 0;
}

// The Adam table of an update call must be the network's own: slot i is the
// i-th weight of `w`, its grad_ pointer and its size.
int check_table(const char *net, int count, const float *const *w, float *const *gw,
                const int64_t *size, const char *const *name, const MarlnavAdamDims *ad,
                const MarlnavAdamBuffers *ab)
{
    char msg[256];
    if (ad->num_tensors != count) {
        snprintf(msg, sizeof(msg), "adam table: num_tensors=%d, the %s has %d parameters",
                 ad->num_tensors, net, count);
        return marlnav_internal_fail(MARLNAV_EINVAL, msg);
    }
    for (int i = 0; i < count; ++i) {
        if (ab->param[i] != w[i]) {
            snprintf(msg, sizeof(msg), "adam table: param[%d] is not the ppo buffer %s", i, name[i]);
            return marlnav_internal_fail(MARLNAV_EINVAL, msg);
        }
        if (ab->grad[i] != gw[i]) {
            snprintf(msg, sizeof(msg), "adam table: grad[%d] is not the ppo buffer grad_%s", i,
                     name[i]);
            return marlnav_internal_fail(MARLNAV_EINVAL, msg);
        }
        if (ad->numel[i] != size[i]) {
            snprintf(msg, sizeof(msg), "adam table: numel[%d]=%lld, %s has %lld elements", i,
                     (long long)ad->numel[i], name[i], (long long)size[i]);
            return marlnav_internal_fail(MARLNAV_EINVAL, msg);
        }
    }
    return 0;
}

}  // namespace

extern "C" int64_t marlnav_adam_state_size(void) { return (int64_t)sizeof(AdamState); }

extern "C" int marlnav_adam_step(const MarlnavAdamDims *d, const MarlnavAdamBuffers *b,
                                 void *stream)
{
    const int rc = check_adam(d, b);
    if (rc) return rc;
    return enqueue_adam(d, b, (hipStream_t)stream);
}

extern "C" int marlnav_ppo_actor_update(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                        double epsilon, double ent_const,
                                        const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab,
                                        void *stream)
{
    // every check of both halves before the first launch: the ppo dims
    // (marlnav_ppo_work_size runs them), the Adam arguments, the table; the
    // gradient call then checks its own buffers before it launches
    if (marlnav_ppo_work_size(d) < 0) return MARLNAV_EINVAL;
    if (!b) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo buffers is NULL");
    int rc = check_adam(ad, ab);
    if (rc) return rc;
    const int64_t H = d->hidden_size, D = d->obs_dim;
    const float *const w[6] = {b->actor_fc1_w, b->actor_fc1_b, b->actor_mu_w,
                               b->actor_mu_b,  b->actor_std_w, b->actor_std_b};
    float *const gw[6] = {b->grad_actor_fc1_w, b->grad_actor_fc1_b, b->grad_actor_mu_w,
                          b->grad_actor_mu_b,  b->grad_actor_std_w, b->grad_actor_std_b};
    const int64_t size[6] = {H * D, H, 2 * H, 2, 2 * H, 2};
    const char *const name[6] = {"actor_fc1_w", "actor_fc1_b", "actor_mu_w",
                                 "actor_mu_b",  "actor_std_w", "actor_std_b"};
    rc = check_table("actor", 6, w, gw, size, name, ad, ab);
    if (rc) return rc;
    rc = marlnav_ppo_actor_grad(d, b, epsilon, ent_const, stream);
    if (rc) return rc;
    return enqueue_adam(ad, ab, (hipStream_t)stream);
}

extern "C" int marlnav_ppo_critic_update(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                         double epsilon, const MarlnavAdamDims *ad,
                                         const MarlnavAdamBuffers *ab, void *stream)
{
    if (marlnav_ppo_work_size(d) < 0) return MARLNAV_EINVAL;
    if (!b) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo buffers is NULL");
    int rc = check_adam(ad, ab);
    if (rc) return rc;
    const int64_t H = d->hidden_size, AD = (int64_t)d->num_agents * d->obs_dim;
    const float *const w[4] = {b->critic_fc1_w, b->critic_fc1_b, b->critic_fc2_w, b->critic_fc2_b};
    float *const gw[4] = {b->grad_critic_fc1_w, b->grad_critic_fc1_b, b->grad_critic_fc2_w,
                          b->grad_critic_fc2_b};
    const int64_t size[4] = {H * AD, H, H, 1};
    const char *const name[4] = {"critic_fc1_w", "critic_fc1_b", "critic_fc2_w", "critic_fc2_b"};
    rc = check_table("critic", 4, w, gw, size, name, ad, ab);
    if (rc) return rc;
    rc = marlnav_ppo_critic_grad(d, b, epsilon, stream);
    if (rc) return rc;
    return enqueue_adam(ad, ab, (hipStream_t)stream);
}
