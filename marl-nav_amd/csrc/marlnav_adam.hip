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
//
// Also here, for the training mode: marlnav_ppo_train_phase,
// a whole train_actor / train_critic enqueued by one call, whose updates hand
// the Adam step to marlnav_ppo.hip's finish kernels (adam_element.h is the
// shared element update) where that is faster and enqueue the two launches
// above elsewhere; and marlnav_params_snapshot_if, the reference's checkpoint
// rule as a copy launch and one bookkeeping thread. The `_mode` forms of the
// actor's calls carry the pairing of advantages to agent rows;
// the forms without it are calls of them with MARLNAV_ADVANTAGE_REFERENCE.
//
// The `_clipped` forms clip the gradient by its global L2 norm
// between the gradient launches and the update: three launches in place of
// the two. grad_sqsum writes one fp64 partial per block of adam_apply's items;
// adam_advance_clip (one block) reduces them, publishes the coefficient in
// AdamState.reserved, writes the norm and advances the count last;
// adam_apply<true> scales each gradient, stores it back and updates from the
// stored value. Datum by datum: .grad is written by the gradient launches
// and by adam_apply<true>, read by grad_sqsum and adam_apply<true> (each
// element by the one thread that rewrites it); the partials are written by
// grad_sqsum and read by adam_advance_clip; the state block is written by
// adam_advance_clip alone and read by adam_apply<true>. Stream order puts
// every read after its write, and no launch reads what another thread of it
// writes except through block_sum's barrier. The clipped phase does not use
// the unclipped phase's folded finish kernels; for an actor of up to 1024
// elements it takes marlnav_ppo.hip's in-block variant of actor_finish, which
// stores the same bits in two launches (marlnav_debug_clip_fold turns it off).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/marlnav.h"
#include "adam_element.h"

__attribute__((visibility("hidden"))) int marlnav_internal_fail(int code, const char *msg);

namespace {

#include "host_util.h"
#include "device_rng.h"  // Philox2x32-10 and the key mixing, for the minibatch permutations

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlots = MARLNAV_ADAM_MAX_TENSORS;
constexpr int64_t kMaxElements = (int64_t)1 << 40;  // all slots together

using marlnav_adam::AdamScalars;
using marlnav_adam::AdamState;
using marlnav_adam::adam_element;
using marlnav_adam::clip_coef;
using marlnav_adam::clipped_grad;

#include "block_sum.h"

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

// The kernels below take a trailing pack: empty, they are the kernels as they
// were; with one `const int64_t *` (the stop flag of the monitored actor
// phase) every thread first reads the flag, which an earlier
// launch wrote and no thread of these launches writes, and returns where it
// is set: the gated step of an update that raised the stop, or lies behind it,
// touches nothing.
template <class... G>
__device__ __forceinline__ bool gate_closed(G... flag)
{
    return ((*flag != 0) || ... || false);
}

template <class... G>
__global__ void __launch_bounds__(64) adam_advance(AdamState *s, double lr, double beta1,
                                                    double beta2, G... gate)
{
    if (gate_closed(gate...)) return;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    marlnav_adam::adam_advance_one(s, lr, beta1, beta2);
}

// kClip (the clipped step): each gradient is scaled by the
// coefficient that adam_advance_clip published, stored back into .grad, and
// the element is updated from that stored value. The unclipped instantiation
// is the kernel of marlnav_adam_step.
template <bool kClip, class... G>
__global__ void __launch_bounds__(kThreads) adam_apply(AdamArgs a, G... gate)
{
    if (gate_closed(gate...)) return;
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

    double coef = 1.0;  // kClip only
    if constexpr (kClip) coef = a.state->reserved;
    const int64_t e0 = (item - first) * 4;  // < n: a slot has ceil(n / 4) items
    const int64_t left = n - e0;
    if (vec && left >= 4) {
        float4 p4 = *reinterpret_cast<const float4 *>(p + e0);
        float4 g4 = *reinterpret_cast<const float4 *>(g + e0);
        float4 m4 = *reinterpret_cast<const float4 *>(m + e0);
        float4 v4 = *reinterpret_cast<const float4 *>(v + e0);
        if constexpr (kClip) {
            g4.x = clipped_grad(g4.x, coef);
            g4.y = clipped_grad(g4.y, coef);
            g4.z = clipped_grad(g4.z, coef);
            g4.w = clipped_grad(g4.w, coef);
            *reinterpret_cast<float4 *>(const_cast<float *>(g) + e0) = g4;
        }
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
            float gj = g[e0 + j];
            if constexpr (kClip) {
                gj = clipped_grad(gj, coef);
                const_cast<float *>(g)[e0 + j] = gj;
            }
            adam_element(pj, gj, mj, vj, c);
            m[e0 + j] = mj;
            v[e0 + j] = vj;
            p[e0 + j] = pj;
        }
    }
}

// The square sum of every gradient of the table, first stage:
// thread = item as adam_apply; a thread's fp64 sum of its <= 4 squares in
// element order (0 past the table's last item), then block_sum; block b's
// partial goes to partials[b]. Reads .grad only.
template <class... G>
__global__ void __launch_bounds__(kThreads) grad_sqsum(AdamArgs a, double *partials, G... gate)
{
    __shared__ double sh[kWaves];
    if (gate_closed(gate...)) return;  // uniform: ahead of block_sum's barriers
    const int64_t item = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double acc = 0.0;
    if (item < a.item_end[kSlots - 1]) {
        const float *g = a.grad[0];
        int64_t n = a.numel[0], first = 0;
        bool vec = a.vec_mask & 1u;
#pragma unroll
        for (int i = 1; i < kSlots; ++i)
            if (item >= a.item_end[i - 1]) {  // never true for an unused slot
                g = a.grad[i];
                n = a.numel[i];
                first = a.item_end[i - 1];
                vec = (a.vec_mask >> i) & 1u;
            }
        const int64_t e0 = (item - first) * 4;
        const int64_t left = n - e0;
        if (vec && left >= 4) {
            const float4 g4 = *reinterpret_cast<const float4 *>(g + e0);
            acc = (double)g4.x * (double)g4.x;
            acc += (double)g4.y * (double)g4.y;
            acc += (double)g4.z * (double)g4.z;
            acc += (double)g4.w * (double)g4.w;
        } else {
            const int cnt = left < 4 ? (int)left : 4;
            for (int j = 0; j < cnt; ++j) {
                const double gj = (double)g[e0 + j];
                acc += gj * gj;
            }
        }
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// Second stage and the count's advance, one block, in place of adam_advance:
// thread t sums partials[t], [t + 256], ... in that order, block_sum adds the
// 256 sums; thread 0 then publishes the coefficient in the state block,
// writes the norm and, last, advances the count (no other thread writes, and
// nothing written here is read in this launch except through block_sum's
// barrier).
template <class... G>
__global__ void __launch_bounds__(kThreads) adam_advance_clip(AdamState *s, double lr,
                                                              double beta1, double beta2,
                                                              const double *partials,
                                                              int64_t num_partials,
                                                              double max_norm, double *norm_out,
                                                              G... gate)
{
    __shared__ double sh[kWaves];
    if (gate_closed(gate...)) return;
    if (blockIdx.x != 0) return;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < num_partials; i += kThreads) acc += partials[i];
    const double total = block_sum(acc, sh);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(total);
    s->reserved = clip_coef(norm, max_norm);
    if (norm_out) *norm_out = norm;
    marlnav_adam::adam_advance_one(s, lr, beta1, beta2);
}

// ---- host side
inline uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

int check_adam_dims(const MarlnavAdamDims *d)
{
    if (!d) return marlnav_internal_fail(MARLNAV_EINVAL, "adam dims is NULL");
    if (d->num_tensors < 1 || d->num_tensors > kSlots)
        return failf(MARLNAV_EINVAL, "adam: num_tensors=%d outside [1, %d]", d->num_tensors, kSlots);
    if (d->maximize != 0 && d->maximize != 1)
        return failf(MARLNAV_EINVAL, "adam: maximize=%d must be 0 or 1", d->maximize);
    int64_t total = 0;
    for (int i = 0; i < d->num_tensors; ++i) {
        if (d->numel[i] < 1) return failf(MARLNAV_EINVAL, "adam: numel[%d]=%lld < 1", i, (long long)d->numel[i]);
        if (d->numel[i] > kMaxElements - total)
            return failf(MARLNAV_EINVAL, "adam: numel[%d]=%lld brings the table past 2^40 elements",
                         i, (long long)d->numel[i]);
        total += d->numel[i];
    }
    if (!(d->lr >= 0.0) || !__builtin_isfinite(d->lr))
        return failf(MARLNAV_EINVAL, "adam: lr=%g must be finite and >= 0", d->lr);
    if (!(d->beta1 >= 0.0 && d->beta1 < 1.0))
        return failf(MARLNAV_EINVAL, "adam: beta1=%g outside [0, 1)", d->beta1);
    if (!(d->beta2 >= 0.0 && d->beta2 < 1.0))
        return failf(MARLNAV_EINVAL, "adam: beta2=%g outside [0, 1)", d->beta2);
    if (!(d->eps >= 0.0) || !__builtin_isfinite(d->eps))
        return failf(MARLNAV_EINVAL, "adam: eps=%g must be finite and >= 0", d->eps);
    if (d->reserved != 0)
        return failf(MARLNAV_EINVAL, "adam: reserved=%lld must be 0", (long long)d->reserved);
    return 0;
}

int check_adam(const MarlnavAdamDims *d, const MarlnavAdamBuffers *b)
{
    const int rc = check_adam_dims(d);
    if (rc) return rc;
    if (!b) return marlnav_internal_fail(MARLNAV_EINVAL, "adam buffers is NULL");
    for (int i = 0; i < d->num_tensors; ++i) {
        const void *ptr[4] = {b->param[i], b->grad[i], b->exp_avg[i], b->exp_avg_sq[i]};
        const char *name[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
        for (int k = 0; k < 4; ++k) {
            if (!ptr[k]) return failf(MARLNAV_EINVAL, "adam: buffer %s[%d] is NULL", name[k], i);
            if (addr(ptr[k]) & 3u)
                return failf(MARLNAV_EINVAL, "adam: buffer %s[%d] must be 4-byte aligned", name[k], i);
        }
    }
    if (!b->state) return marlnav_internal_fail(MARLNAV_EINVAL, "adam: buffer state is NULL");
    if (addr(b->state) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "adam: buffer state must be 8-byte aligned");
    return 0;
}

// blocks of adam_apply / grad_sqsum over the table: ceil(items / 256)
int64_t table_blocks(const MarlnavAdamDims *d)
{
    int64_t items = 0;
    for (int i = 0; i < d->num_tensors; ++i) items += (d->numel[i] + 3) / 4;
    return (items + kThreads - 1) / kThreads;
}

// the clipped step's own arguments; norm_out is the call's norm_out / norm_log
struct ClipArgs {
    double max_norm;
    double *norm_work;
    double *norm_out;  // of the next step; NULL: not recorded
};

int check_clip(double max_norm, const void *norm_work, const void *norm_out, const char *out_name)
{
    if (!(max_norm > 0.0))  // a NaN is not greater
        return failf(MARLNAV_EINVAL, "clip: max_norm=%g must be > 0 (+inf: record the norm only)",
                     max_norm);
    if (!norm_work) return marlnav_internal_fail(MARLNAV_EINVAL, "clip: norm_work is NULL");
    if (addr(norm_work) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "clip: norm_work must be 8-byte aligned");
    if (addr(norm_out) & 7u)
        return failf(MARLNAV_EINVAL, "clip: %s must be 8-byte aligned", out_name);
    return 0;
}

// checked arguments only. clip NULL: the two launches of marlnav_adam_step;
// given: the three of marlnav_adam_step_clipped. gate: the same launches in
// their gated forms (the monitored actor phase).
int enqueue_adam(const MarlnavAdamDims *d, const MarlnavAdamBuffers *b, hipStream_t s,
                 const ClipArgs *clip = nullptr, const int64_t *gate = nullptr)
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
    // items <= 2^38 + 8: the grid fits 31 bits
    const dim3 grid((unsigned)((items + kThreads - 1) / kThreads));
    if (gate && clip) {
        hipLaunchKernelGGL(grad_sqsum, grid, dim3(kThreads), 0, s, a, clip->norm_work, gate);
        hipLaunchKernelGGL(adam_advance_clip, dim3(1), dim3(kThreads), 0, s, state, d->lr,
                           d->beta1, d->beta2, (const double *)clip->norm_work, (int64_t)grid.x,
                           clip->max_norm, clip->norm_out, gate);
        hipLaunchKernelGGL(adam_apply<true>, grid, dim3(kThreads), 0, s, a, gate);
        return launch_status();
    }
    if (gate) {
        hipLaunchKernelGGL(adam_advance, dim3(1), dim3(64), 0, s, state, d->lr, d->beta1,
                           d->beta2, gate);
        hipLaunchKernelGGL(adam_apply<false>, grid, dim3(kThreads), 0, s, a, gate);
        return launch_status();
    }
    if (clip) {
        hipLaunchKernelGGL(grad_sqsum<>, grid, dim3(kThreads), 0, s, a, clip->norm_work);
        hipLaunchKernelGGL(adam_advance_clip<>, dim3(1), dim3(kThreads), 0, s, state, d->lr,
                           d->beta1, d->beta2, (const double *)clip->norm_work, (int64_t)grid.x,
                           clip->max_norm, clip->norm_out);
        hipLaunchKernelGGL(adam_apply<true>, grid, dim3(kThreads), 0, s, a);
        return launch_status();
    }
    hipLaunchKernelGGL(adam_advance<>, dim3(1), dim3(64), 0, s, state, d->lr, d->beta1, d->beta2);
    hipLaunchKernelGGL(adam_apply<false>, grid, dim3(kThreads), 0, s, a);
    return launch_status();
}

// The Adam table of an update call must be the network's own: slot i is the
// i-th weight of `w`, its grad_ pointer and its size.
int check_table(const char *net, int count, const float *const *w, float *const *gw,
                const int64_t *size, const char *const *name, const MarlnavAdamDims *ad,
                const MarlnavAdamBuffers *ab)
{
    if (ad->num_tensors != count)
        return failf(MARLNAV_EINVAL, "adam table: num_tensors=%d, the %s has %d parameters",
                     ad->num_tensors, net, count);
    for (int i = 0; i < count; ++i) {
        if (ab->param[i] != w[i])
            return failf(MARLNAV_EINVAL, "adam table: param[%d] is not the ppo buffer %s", i,
                         name[i]);
        if (ab->grad[i] != gw[i])
            return failf(MARLNAV_EINVAL, "adam table: grad[%d] is not the ppo buffer grad_%s", i,
                         name[i]);
        if (ad->numel[i] != size[i])
            return failf(MARLNAV_EINVAL, "adam table: numel[%d]=%lld, %s has %lld elements", i,
                         (long long)ad->numel[i], name[i], (long long)size[i]);
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

extern "C" int64_t marlnav_grad_norm_work_size(const MarlnavAdamDims *d)
{
    const int rc = check_adam_dims(d);
    if (rc) return rc;
    return table_blocks(d);
}

extern "C" int marlnav_adam_step_clipped(const MarlnavAdamDims *d, const MarlnavAdamBuffers *b,
                                         double max_norm, double *norm_work, double *norm_out,
                                         void *stream)
{
    int rc = check_adam(d, b);
    if (rc) return rc;
    rc = check_clip(max_norm, norm_work, norm_out, "norm_out");
    if (rc) return rc;
    const ClipArgs clip = {max_norm, norm_work, norm_out};
    return enqueue_adam(d, b, (hipStream_t)stream, &clip);
}

namespace {

// clip NULL: marlnav_ppo_actor_update_mode; given: its _clipped form
int actor_update(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, double epsilon,
                 double ent_const, const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab,
                 int advantage_mode, const ClipArgs *clip, void *stream)
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
    if (clip) rc = check_clip(clip->max_norm, clip->norm_work, clip->norm_out, "norm_out");
    if (rc) return rc;
    rc = marlnav_ppo_actor_grad_mode(d, b, epsilon, ent_const, advantage_mode, stream);
    if (rc) return rc;
    return enqueue_adam(ad, ab, (hipStream_t)stream, clip);
}

int critic_update(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, double epsilon,
                  const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab, const ClipArgs *clip,
                  void *stream)
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
    if (clip) rc = check_clip(clip->max_norm, clip->norm_work, clip->norm_out, "norm_out");
    if (rc) return rc;
    rc = marlnav_ppo_critic_grad(d, b, epsilon, stream);
    if (rc) return rc;
    return enqueue_adam(ad, ab, (hipStream_t)stream, clip);
}

}  // namespace

extern "C" int marlnav_ppo_actor_update_mode(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                             double epsilon, double ent_const,
                                             const MarlnavAdamDims *ad,
                                             const MarlnavAdamBuffers *ab, int advantage_mode,
                                             void *stream)
{
    return actor_update(d, b, epsilon, ent_const, ad, ab, advantage_mode, nullptr, stream);
}

extern "C" int marlnav_ppo_actor_update_clipped(const MarlnavPpoDims *d,
                                                const MarlnavPpoBuffers *b, double epsilon,
                                                double ent_const, const MarlnavAdamDims *ad,
                                                const MarlnavAdamBuffers *ab, int advantage_mode,
                                                double max_norm, double *norm_work,
                                                double *norm_out, void *stream)
{
    const ClipArgs clip = {max_norm, norm_work, norm_out};
    return actor_update(d, b, epsilon, ent_const, ad, ab, advantage_mode, &clip, stream);
}

extern "C" int marlnav_ppo_actor_update(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                        double epsilon, double ent_const,
                                        const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab,
                                        void *stream)
{
    return marlnav_ppo_actor_update_mode(d, b, epsilon, ent_const, ad, ab,
                                         MARLNAV_ADVANTAGE_REFERENCE, stream);
}

extern "C" int marlnav_ppo_critic_update(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                         double epsilon, const MarlnavAdamDims *ad,
                                         const MarlnavAdamBuffers *ab, void *stream)
{
    return critic_update(d, b, epsilon, ad, ab, nullptr, stream);
}

extern "C" int marlnav_ppo_critic_update_clipped(const MarlnavPpoDims *d,
                                                 const MarlnavPpoBuffers *b, double epsilon,
                                                 const MarlnavAdamDims *ad,
                                                 const MarlnavAdamBuffers *ab, double max_norm,
                                                 double *norm_work, double *norm_out,
                                                 void *stream)
{
    const ClipArgs clip = {max_norm, norm_work, norm_out};
    return critic_update(d, b, epsilon, ad, ab, &clip, stream);
}

// =========================================================================
// one whole train_actor / train_critic as one call
// =========================================================================
__attribute__((visibility("hidden"))) int marlnav_internal_ppo_fold(
    int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, double epsilon,
    double ent_const, int advantage_mode, const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab,
    void *stream, int check_only);
__attribute__((visibility("hidden"))) int marlnav_internal_ppo_actor_clip_fold(
    const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, double epsilon, double ent_const,
    int advantage_mode, const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab, double max_norm,
    double *norm_out, void *stream);

namespace {

// whether the clipped phase folds the actor's clip and Adam step into
// actor_finish (marlnav_debug_clip_fold; the default is the measured decision
// of DESIGN.md §16)
int g_clip_fold = MARLNAV_CLIP_FOLD_DEFAULT;

// the (lo, hi) list against the buffer's steps
int check_bounds(const MarlnavPpoDims *d, const int64_t *bounds, int64_t num_batches)
{
    if (num_batches < 1)
        return failf(MARLNAV_EINVAL, "train: num_batches=%lld < 1", (long long)num_batches);
    if (!bounds) return marlnav_internal_fail(MARLNAV_EINVAL, "train: bounds is NULL");
    for (int64_t j = 0; j < num_batches; ++j) {
        const int64_t lo = bounds[2 * j], hi = bounds[2 * j + 1];
        if (lo < 0 || hi <= lo || hi > d->num_steps)
            return failf(MARLNAV_EINVAL,
                         "train: bounds[%lld]=(%lld, %lld) is not a non-empty range of the %lld "
                         "steps", (long long)j, (long long)lo, (long long)hi,
                         (long long)d->num_steps);
    }
    return 0;
}

// the structs of minibatch (lo, hi): dims of hi - lo steps, data pointers at step lo
void minibatch(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, int64_t lo, int64_t hi,
               double *loss, MarlnavPpoDims *md, MarlnavPpoBuffers *mb)
{
    *md = *d;
    md->num_steps = hi - lo;
    *mb = *b;
    const int64_t rows = lo * d->num_parallel, arows = rows * d->num_agents;
    mb->obs = b->obs + arows * d->obs_dim;
    if (b->actions) mb->actions = b->actions + arows * 2;
    if (b->log_probs) mb->log_probs = b->log_probs + arows;
    if (b->values) mb->values = b->values + rows;
    mb->returns = b->returns + rows;
    mb->loss = loss;
}

}  // namespace

namespace {

int64_t train_work_size(const MarlnavPpoDims *d, const int64_t *bounds, int64_t num_batches,
                        int64_t (*one)(const MarlnavPpoDims *))
{
    if (marlnav_ppo_work_size(d) < 0) return MARLNAV_EINVAL;
    const int rc = check_bounds(d, bounds, num_batches);
    if (rc) return rc;
    int64_t need = 0;
    for (int64_t j = 0; j < num_batches; ++j) {
        MarlnavPpoDims md = *d;
        md.num_steps = bounds[2 * j + 1] - bounds[2 * j];
        const int64_t w = one(&md);
        if (w < 0) return w;
        if (w > need) need = w;
    }
    return need;
}

}  // namespace

extern "C" int64_t marlnav_ppo_train_work_size(const MarlnavPpoDims *d, const int64_t *bounds,
                                               int64_t num_batches)
{
    return train_work_size(d, bounds, num_batches, marlnav_ppo_work_size);
}

extern "C" int64_t marlnav_ppo_train_diag_work_size(const MarlnavPpoDims *d,
                                                    const int64_t *bounds, int64_t num_batches)
{
    return train_work_size(d, bounds, num_batches, marlnav_ppo_diag_work_size);
}

namespace {

// every check of a phase call before its first launch; clip as for train_phase
int check_train_phase(int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                      const int64_t *bounds, int64_t num_batches, int64_t num_epochs,
                      double epsilon, double ent_const, const MarlnavAdamDims *ad,
                      const MarlnavAdamBuffers *ab, double *loss_log, int advantage_mode,
                      const ClipArgs *clip, void *stream)
{
    if (network != MARLNAV_NETWORK_ACTOR && network != MARLNAV_NETWORK_CRITIC)
        return failf(MARLNAV_EINVAL, "train: network=%d must be MARLNAV_NETWORK_ACTOR or _CRITIC", network);
    if (advantage_mode != MARLNAV_ADVANTAGE_REFERENCE && advantage_mode != MARLNAV_ADVANTAGE_ENV)
        return failf(MARLNAV_EINVAL, "train: advantage_mode=%d must be MARLNAV_ADVANTAGE_REFERENCE or _ENV",
                     advantage_mode);
    // the own-env pairing is the actor's: it reads no values
    const bool need_values =
        network == MARLNAV_NETWORK_CRITIC || advantage_mode == MARLNAV_ADVANTAGE_REFERENCE;
    if (marlnav_ppo_work_size(d) < 0) return MARLNAV_EINVAL;
    if (!b) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo buffers is NULL");
    if (num_epochs < 1) return failf(MARLNAV_EINVAL, "train: num_epochs=%lld < 1", (long long)num_epochs);
    int rc = check_bounds(d, bounds, num_batches);
    if (rc) return rc;
    if (!loss_log) return marlnav_internal_fail(MARLNAV_EINVAL, "train: loss_log is NULL");
    if (addr(loss_log) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "train: loss_log must be 8-byte aligned");
    rc = check_adam(ad, ab);
    if (rc) return rc;
    const int64_t H = d->hidden_size, D = d->obs_dim, AD = (int64_t)d->num_agents * D;
    if (network == MARLNAV_NETWORK_ACTOR) {
        const float *const w[6] = {b->actor_fc1_w, b->actor_fc1_b, b->actor_mu_w,
                                   b->actor_mu_b,  b->actor_std_w, b->actor_std_b};
        float *const gw[6] = {b->grad_actor_fc1_w, b->grad_actor_fc1_b, b->grad_actor_mu_w,
                              b->grad_actor_mu_b,  b->grad_actor_std_w, b->grad_actor_std_b};
        const int64_t size[6] = {H * D, H, 2 * H, 2, 2 * H, 2};
        const char *const name[6] = {"actor_fc1_w", "actor_fc1_b", "actor_mu_w",
                                     "actor_mu_b",  "actor_std_w", "actor_std_b"};
        rc = check_table("actor", 6, w, gw, size, name, ad, ab);
    } else {
        const float *const w[4] = {b->critic_fc1_w, b->critic_fc1_b, b->critic_fc2_w,
                                   b->critic_fc2_b};
        float *const gw[4] = {b->grad_critic_fc1_w, b->grad_critic_fc1_b, b->grad_critic_fc2_w,
                              b->grad_critic_fc2_b};
        const int64_t size[4] = {H * AD, H, H, 1};
        const char *const name[4] = {"critic_fc1_w", "critic_fc1_b", "critic_fc2_w",
                                     "critic_fc2_b"};
        rc = check_table("critic", 4, w, gw, size, name, ad, ab);
    }
    if (rc) return rc;
    if (clip) rc = check_clip(clip->max_norm, clip->norm_work, clip->norm_out, "norm_log");
    if (rc) return rc;
    if (!b->obs) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: buffer obs is NULL");
    if (need_values && !b->values)
        return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: buffer values is NULL");
    if (!b->returns) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: buffer returns is NULL");
    MarlnavPpoDims md;
    MarlnavPpoBuffers mb;
    for (int64_t j = 0; j < num_batches; ++j) {  // dims and buffers of every minibatch
        minibatch(d, b, bounds[2 * j], bounds[2 * j + 1], loss_log, &md, &mb);
        rc = marlnav_internal_ppo_fold(network, &md, &mb, epsilon, ent_const, advantage_mode, ad,
                                       ab, stream, 1);
        if (rc) return rc;
    }
    return 0;
}

// clip NULL: marlnav_ppo_train_phase_mode; given: its _clipped form, whose
// norm_out is the norm_log (update k writes [k]) or NULL
int train_phase(int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                const int64_t *bounds, int64_t num_batches, int64_t num_epochs, double epsilon,
                double ent_const, const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab,
                double *loss_log, int advantage_mode, const ClipArgs *clip, void *stream)
{
    int rc = check_train_phase(network, d, b, bounds, num_batches, num_epochs, epsilon, ent_const,
                               ad, ab, loss_log, advantage_mode, clip, stream);
    if (rc) return rc;
    MarlnavPpoDims md;
    MarlnavPpoBuffers mb;
    // ---- num_epochs x num_batches updates, epoch-major: two launches for the
    // actor, two or three for the critic, each with the Adam step inside (a
    // large actor keeps the four launches of marlnav_ppo_actor_update)
    int64_t k = 0;
    for (int64_t e = 0; e < num_epochs; ++e)
        for (int64_t j = 0; j < num_batches; ++j, ++k) {
            minibatch(d, b, bounds[2 * j], bounds[2 * j + 1], loss_log + k, &md, &mb);
            if (clip) {
                double *const norm_k = clip->norm_out ? clip->norm_out + k : nullptr;
                if (network == MARLNAV_NETWORK_ACTOR && g_clip_fold) {
                    // a small actor: norm, clip and update inside actor_finish
                    rc = marlnav_internal_ppo_actor_clip_fold(&md, &mb, epsilon, ent_const,
                                                              advantage_mode, ad, ab,
                                                              clip->max_norm, norm_k, stream);
                    if (rc < 0) return rc;
                    if (rc == 0) continue;
                }
                // the folded finish kernels of the unclipped phase update
                // elements before the norm exists: the gradient launches alone,
                // then the clipped step
                rc = network == MARLNAV_NETWORK_ACTOR
                         ? marlnav_ppo_actor_grad_mode(&md, &mb, epsilon, ent_const,
                                                       advantage_mode, stream)
                         : marlnav_ppo_critic_grad(&md, &mb, epsilon, stream);
                if (rc) return rc;
                const ClipArgs ck = {clip->max_norm, clip->norm_work, norm_k};
                rc = enqueue_adam(ad, ab, (hipStream_t)stream, &ck);
                if (rc) return rc;
                continue;
            }
            rc = marlnav_internal_ppo_fold(network, &md, &mb, epsilon, ent_const, advantage_mode,
                                           ad, ab, stream, 0);
            if (rc == 1) rc = enqueue_adam(ad, ab, (hipStream_t)stream);  // not folded
            if (rc) return rc;
        }
    return 0;
}

}  // namespace

extern "C" int marlnav_ppo_train_phase_mode(int network, const MarlnavPpoDims *d,
                                            const MarlnavPpoBuffers *b, const int64_t *bounds,
                                            int64_t num_batches, int64_t num_epochs,
                                            double epsilon, double ent_const,
                                            const MarlnavAdamDims *ad,
                                            const MarlnavAdamBuffers *ab, double *loss_log,
                                            int advantage_mode, void *stream)
{
    return train_phase(network, d, b, bounds, num_batches, num_epochs, epsilon, ent_const, ad, ab,
                       loss_log, advantage_mode, nullptr, stream);
}

extern "C" int marlnav_ppo_train_phase_clipped(int network, const MarlnavPpoDims *d,
                                               const MarlnavPpoBuffers *b, const int64_t *bounds,
                                               int64_t num_batches, int64_t num_epochs,
                                               double epsilon, double ent_const,
                                               const MarlnavAdamDims *ad,
                                               const MarlnavAdamBuffers *ab, double *loss_log,
                                               int advantage_mode, double max_norm,
                                               double *norm_work, double *norm_log, void *stream)
{
    const ClipArgs clip = {max_norm, norm_work, norm_log};
    return train_phase(network, d, b, bounds, num_batches, num_epochs, epsilon, ent_const, ad, ab,
                       loss_log, advantage_mode, &clip, stream);
}

extern "C" int marlnav_ppo_train_phase(int network, const MarlnavPpoDims *d,
                                       const MarlnavPpoBuffers *b, const int64_t *bounds,
                                       int64_t num_batches, int64_t num_epochs, double epsilon,
                                       double ent_const, const MarlnavAdamDims *ad,
                                       const MarlnavAdamBuffers *ab, double *loss_log,
                                       void *stream)
{
    return marlnav_ppo_train_phase_mode(network, d, b, bounds, num_batches, num_epochs, epsilon,
                                        ent_const, ad, ab, loss_log, MARLNAV_ADVANTAGE_REFERENCE,
                                        stream);
}

// =========================================================================
// the monitored actor phase
// =========================================================================
__attribute__((visibility("hidden"))) int marlnav_internal_ppo_actor_diag(
    const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, double epsilon, double ent_const,
    int advantage_mode, double *diag_row, int64_t *stop, double target_kl, int64_t k, void *stream);

extern "C" int marlnav_ppo_train_phase_monitored(
    int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, const int64_t *bounds,
    int64_t num_batches, int64_t num_epochs, double epsilon, double ent_const,
    const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab, double *loss_log, int advantage_mode,
    double max_norm, double *norm_work, double *norm_log, double target_kl, double *diag_log,
    int64_t *stop, void *stream)
{
    // ---- every check before the first launch
    if (network == MARLNAV_NETWORK_CRITIC)
        return marlnav_internal_fail(MARLNAV_EINVAL,
                                     "train: the monitored phase is the actor's; network is "
                                     "MARLNAV_NETWORK_CRITIC");
    const bool clipped = max_norm != MARLNAV_MAX_NORM_NONE;  // a NaN is refused by check_clip
    if (!clipped && (norm_work || norm_log))
        return marlnav_internal_fail(MARLNAV_EINVAL,
                                     "clip: norm_work and norm_log must be NULL with "
                                     "max_norm = MARLNAV_MAX_NORM_NONE");
    const ClipArgs clip = {max_norm, norm_work, norm_log};
    int rc = check_train_phase(network, d, b, bounds, num_batches, num_epochs, epsilon, ent_const,
                               ad, ab, loss_log, advantage_mode, clipped ? &clip : nullptr, stream);
    if (rc) return rc;
    if (!(target_kl > 0.0))  // a NaN is not greater
        return failf(MARLNAV_EINVAL, "train: target_kl=%g must be > 0 (+inf: monitor only)",
                     target_kl);
    if (!diag_log) return marlnav_internal_fail(MARLNAV_EINVAL, "train: diag_log is NULL");
    if (addr(diag_log) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "train: diag_log must be 8-byte aligned");
    if (!stop) return marlnav_internal_fail(MARLNAV_EINVAL, "train: stop is NULL");
    if (addr(stop) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "train: stop must be 8-byte aligned");
    // ---- num_epochs x num_batches updates: the diagnostic gradient launches,
    // whose finish publishes the flag, then the gated Adam launches (2, or 3
    // with a clip). Nothing is folded: an update that stops must not step.
    MarlnavPpoDims md;
    MarlnavPpoBuffers mb;
    int64_t k = 0;
    for (int64_t e = 0; e < num_epochs; ++e)
        for (int64_t j = 0; j < num_batches; ++j, ++k) {
            minibatch(d, b, bounds[2 * j], bounds[2 * j + 1], loss_log + k, &md, &mb);
            rc = marlnav_internal_ppo_actor_diag(&md, &mb, epsilon, ent_const, advantage_mode,
                                                 diag_log + MARLNAV_DIAG_ROW * k, stop, target_kl, k, stream);
            if (rc) return rc;
            const ClipArgs ck = {max_norm, norm_work, norm_log ? norm_log + k : nullptr};
            rc = enqueue_adam(ad, ab, (hipStream_t)stream, clipped ? &ck : nullptr, stop);
            if (rc) return rc;
        }
    return 0;
}

// =========================================================================
// shuffled minibatches
// =========================================================================
__attribute__((visibility("hidden"))) int marlnav_internal_ppo_grad_steps(
    int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, const int32_t *steps,
    double epsilon, double ent_const, int advantage_mode, double *diag_row, int64_t *stop,
    double target_kl, int64_t k, void *stream, int check_only);

namespace {

constexpr int64_t kPermMaxLen = 65535;     // L: a draw's block index stays below 2^15
constexpr int64_t kPermMaxEpochs = 65535;  // E: the epoch fills the counter word's high half
constexpr uint32_t kPermBlock = 0x5045524Du;  // "PERM": the key's block tag, + the network

// E uniform permutations of [0, L) in one launch of one block: thread e (then
// e + 256, ...) runs a Fisher-Yates over the identity in row e of the table.
//   c        the 64-bit call counter, read from *counter by every thread
//   key      native_key(m, kPermBlock + network, c), m = native_seed_mix(seed):
//            (uint32)m ^ fmix32((kPermBlock + network) * 0x9E3779B1
//                               + hi32(c) * 0x85EBCA77 + hi32(m))
//   block b  of epoch e: Philox2x32-10 of the counter (e << 16 | b, lo32(c))
//            under the key; b < 2^15 and e < 2^16, so no two (e, b) share a word
//   draws    position i = L - 1 down to 1 takes draw number n = L - 1 - i: word
//            n & 1 of block n >> 1; j = (uint64)word * (i + 1) >> 32 in [0, i];
//            row[i] and row[j] are swapped
// The multiply-shift picks each j with probability within 2^-32 of 1 / (i +
// 1): a bias of at most (i + 1) / 2^32 <= L / 2^32 per draw, below 1.6e-5 at
// the largest L = 65 535 the call accepts. Behind the block's barrier, when
// every thread holds c, thread 0 stores c + 1: a replayed graph draws anew,
// as the Adam step count advances. Plain vector loads and stores only, each
// row read and written by its one thread; no atomics.
__global__ void __launch_bounds__(kThreads) minibatch_permutations(int32_t *table, int L, int E,
                                                                    uint64_t m, uint32_t network,
                                                                    uint64_t *counter)
{
    const uint64_t c = *counter;
    __syncthreads();
    if (threadIdx.x == 0) *counter = c + 1;
    const uint32_t key = native_key(m, kPermBlock + network, c);
    for (int e = threadIdx.x; e < E; e += kThreads) {
        int32_t *__restrict__ row = table + (int64_t)e * L;
        for (int i = 0; i < L; ++i) row[i] = i;
        uint32_t w0 = 0, w1 = 0;
        for (int i = L - 1, n = 0; i >= 1; --i, ++n) {
            if ((n & 1) == 0) {
                w0 = ((uint32_t)e << 16) | (uint32_t)(n >> 1);
                w1 = (uint32_t)c;
                philox2x32_10(w0, w1, key);
            }
            const uint32_t word = (n & 1) ? w1 : w0;
            const int j = (int)(((uint64_t)word * (uint32_t)(i + 1)) >> 32);
            const int32_t a = row[i], bj = row[j];
            row[i] = bj;
            row[j] = a;
        }
    }
}

int check_permutations(int64_t L, int64_t E, int network, const void *counter, const void *table)
{
    if (L < 1 || L > kPermMaxLen)
        return failf(MARLNAV_EINVAL, "shuffle: %lld steps outside [1, %lld]", (long long)L,
                     (long long)kPermMaxLen);
    if (E < 1 || E > kPermMaxEpochs)
        return failf(MARLNAV_EINVAL, "shuffle: num_epochs=%lld outside [1, %lld]", (long long)E,
                     (long long)kPermMaxEpochs);
    if (network != MARLNAV_NETWORK_ACTOR && network != MARLNAV_NETWORK_CRITIC)
        return failf(MARLNAV_EINVAL, "shuffle: network=%d must be MARLNAV_NETWORK_ACTOR or _CRITIC",
                     network);
    if (!counter) return marlnav_internal_fail(MARLNAV_EINVAL, "shuffle: counter is NULL");
    if (addr(counter) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "shuffle: counter must be 8-byte aligned");
    if (!table) return marlnav_internal_fail(MARLNAV_EINVAL, "shuffle: table is NULL");
    if (addr(table) & 3u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "shuffle: table must be 4-byte aligned");
    return 0;
}

void enqueue_permutations(int64_t L, int64_t E, uint64_t seed, int network, uint64_t *counter,
                          int32_t *table, hipStream_t s)
{
    hipLaunchKernelGGL(minibatch_permutations, dim3(1), dim3(kThreads), 0, s, table, (int)L,
                       (int)E, native_seed_mix(seed), (uint32_t)network, counter);
}

// minibatch j of an epoch: entries [j bs, (j + 1) bs) of its permutation, the
// last one with the L % bs left over
inline int64_t shuffled_steps(int64_t L, int64_t bs, int64_t j)
{
    return j + 1 < L / bs ? bs : L - j * bs;
}

}  // namespace

extern "C" int marlnav_minibatch_permutations(int64_t L, int64_t E, uint64_t seed, int network,
                                              uint64_t *counter, int32_t *table, void *stream)
{
    const int rc = check_permutations(L, E, network, counter, table);
    if (rc) return rc;
    enqueue_permutations(L, E, seed, network, counter, table, (hipStream_t)stream);
    return launch_status();
}

extern "C" int64_t marlnav_ppo_train_shuffled_work_size(const MarlnavPpoDims *d,
                                                        int64_t batch_size, int diag)
{
    if (marlnav_ppo_work_size(d) < 0) return MARLNAV_EINVAL;
    const int64_t L = d->num_steps;
    if (batch_size < 1 || L / batch_size < 1)
        return failf(MARLNAV_EINVAL, "shuffle: batch_size=%lld gives no minibatch of %lld steps",
                     (long long)batch_size, (long long)L);
    int64_t need = 0;
    const int64_t B = L / batch_size;
    for (int64_t j = B > 1 ? B - 2 : 0; j < B; ++j) {  // the two sizes an epoch has
        MarlnavPpoDims md = *d;
        md.num_steps = shuffled_steps(L, batch_size, j);
        const int64_t w = diag ? marlnav_ppo_diag_work_size(&md) : marlnav_ppo_work_size(&md);
        if (w < 0) return w;
        if (w > need) need = w;
    }
    return need;
}

extern "C" int marlnav_ppo_train_phase_shuffled(
    int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, int64_t batch_size,
    int64_t num_epochs, double epsilon, double ent_const, const MarlnavAdamDims *ad,
    const MarlnavAdamBuffers *ab, double *loss_log, int advantage_mode, double max_norm,
    double *norm_work, double *norm_log, double target_kl, double *diag_log, int64_t *stop,
    uint64_t seed, uint64_t *counter, int32_t *table, void *stream)
{
    // ---- every check before the first launch
    const bool monitored = target_kl != 0.0 || diag_log || stop;
    if (monitored && network == MARLNAV_NETWORK_CRITIC)
        return marlnav_internal_fail(MARLNAV_EINVAL,
                                     "train: target_kl / diag_log / stop monitor the actor; "
                                     "network is MARLNAV_NETWORK_CRITIC");
    const bool clipped = max_norm != MARLNAV_MAX_NORM_NONE;  // a NaN is refused by check_clip
    if (!clipped && (norm_work || norm_log))
        return marlnav_internal_fail(MARLNAV_EINVAL,
                                     "clip: norm_work and norm_log must be NULL with "
                                     "max_norm = MARLNAV_MAX_NORM_NONE");
    if (marlnav_ppo_work_size(d) < 0) return MARLNAV_EINVAL;
    const int64_t L = d->num_steps;
    if (batch_size < 1 || L / batch_size < 1)
        return failf(MARLNAV_EINVAL, "shuffle: batch_size=%lld gives no minibatch of %lld steps",
                     (long long)batch_size, (long long)L);
    int rc = check_permutations(L, num_epochs, network, counter, table);
    if (rc) return rc;
    const int64_t B = L / batch_size;
    // the contiguous phase's checks, over the whole buffer as one range
    const int64_t whole[2] = {0, L};
    const ClipArgs clip = {max_norm, norm_work, norm_log};
    rc = check_train_phase(network, d, b, whole, 1, num_epochs, epsilon, ent_const, ad, ab,
                           loss_log, advantage_mode, clipped ? &clip : nullptr, stream);
    if (rc) return rc;
    if (monitored) {
        if (!(target_kl > 0.0))  // a NaN is not greater
            return failf(MARLNAV_EINVAL, "train: target_kl=%g must be > 0 (+inf: monitor only)",
                         target_kl);
        if (!diag_log) return marlnav_internal_fail(MARLNAV_EINVAL, "train: diag_log is NULL");
        if (addr(diag_log) & 7u)
            return marlnav_internal_fail(MARLNAV_EINVAL, "train: diag_log must be 8-byte aligned");
        if (!stop) return marlnav_internal_fail(MARLNAV_EINVAL, "train: stop is NULL");
        if (addr(stop) & 7u)
            return marlnav_internal_fail(MARLNAV_EINVAL, "train: stop must be 8-byte aligned");
    }
    MarlnavPpoDims md = *d;
    MarlnavPpoBuffers mb = *b;
    for (int64_t j = B > 1 ? B - 2 : 0; j < B; ++j) {  // dims of the two minibatch sizes
        md.num_steps = shuffled_steps(L, batch_size, j);
        rc = marlnav_internal_ppo_grad_steps(network, &md, &mb, table, epsilon, ent_const,
                                             advantage_mode, nullptr, nullptr, 0.0, 0, stream, 1);
        if (rc) return rc;
    }
    // ---- the permutations, then num_epochs x B updates, epoch-major: the gather
    // gradient launches and the Adam launches (clipped and gated where asked).
    // Nothing is folded: the finish kernels' folds have no gather variants.
    enqueue_permutations(L, num_epochs, seed, network, counter, table, (hipStream_t)stream);
    rc = launch_status();
    if (rc) return rc;
    int64_t k = 0;
    for (int64_t e = 0; e < num_epochs; ++e)
        for (int64_t j = 0; j < B; ++j, ++k) {
            md.num_steps = shuffled_steps(L, batch_size, j);
            mb.loss = loss_log + k;
            rc = marlnav_internal_ppo_grad_steps(
                network, &md, &mb, table + e * L + j * batch_size, epsilon, ent_const,
                advantage_mode, monitored ? diag_log + MARLNAV_DIAG_ROW * k : nullptr, stop,
                target_kl, k, stream, 0);
            if (rc) return rc;
            const ClipArgs ck = {max_norm, norm_work, norm_log ? norm_log + k : nullptr};
            rc = enqueue_adam(ad, ab, (hipStream_t)stream, clipped ? &ck : nullptr,
                              monitored ? stop : nullptr);
            if (rc) return rc;
        }
    return 0;
}

extern "C" int marlnav_debug_clip_fold(int on)
{
    const int before = g_clip_fold;
    if (on == 0 || on == 1) g_clip_fold = on;
    return before;
}

// =========================================================================
// the checkpoint rule of MAPPO.get_data on the device (models.py:127-129)
// =========================================================================
namespace {

constexpr int kSnapSlots = MARLNAV_SNAPSHOT_MAX_TENSORS;

struct SnapArgs {
    const float *src[kSnapSlots];
    float *dst[kSnapSlots];
    int64_t numel[kSnapSlots];
    int64_t item_end[kSnapSlots];  // items of slots 0..i; unused slots repeat the total
    const double *mean_rew;
    const double *max_rew;
    uint32_t vec_mask;  // bit i: both pointers of slot i are 16-byte aligned
};

// thread = item of 4 elements over all slots, as adam_apply; every thread
// reads the decision, which no thread of this launch writes
__global__ void __launch_bounds__(kThreads) snapshot_copy(SnapArgs a)
{
    const int64_t item = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (item >= a.item_end[kSnapSlots - 1]) return;
    if (!(*a.mean_rew > *a.max_rew)) return;  // a NaN mean copies nothing
    const float *src = a.src[0];
    float *dst = a.dst[0];
    int64_t n = a.numel[0], first = 0;
    bool vec = a.vec_mask & 1u;
#pragma unroll
    for (int i = 1; i < kSnapSlots; ++i)
        if (item >= a.item_end[i - 1]) {  // never true for an unused slot
            src = a.src[i];
            dst = a.dst[i];
            n = a.numel[i];
            first = a.item_end[i - 1];
            vec = (a.vec_mask >> i) & 1u;
        }
    const int64_t e0 = (item - first) * 4;  // < n: a slot has ceil(n / 4) items
    const int64_t left = n - e0;
    if (vec && left >= 4) {
        *reinterpret_cast<float4 *>(dst + e0) = *reinterpret_cast<const float4 *>(src + e0);
    } else {
        const int cnt = left < 4 ? (int)left : 4;
        for (int j = 0; j < cnt; ++j) dst[e0 + j] = src[e0 + j];
    }
}

// one thread, the launch after the copy: the save count, the repeat index of
// the save and, with track_best, the new maximum
__global__ void __launch_bounds__(64) snapshot_book(const double *mean_rew, double *max_rew,
                                                     int64_t *save_state, int64_t repeat_index,
                                                     int track_best)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double mean = *mean_rew;
    if (!(mean > *max_rew)) return;
    save_state[0] += 1;
    save_state[1] = repeat_index;
    if (track_best) *max_rew = mean;
}

}  // namespace

extern "C" int marlnav_params_snapshot_if(int num_tensors, const float *const *src,
                                          float *const *dst, const int64_t *numel,
                                          const double *mean_rew, double *max_rew,
                                          int64_t *save_state, int64_t repeat_index,
                                          int track_best, void *stream)
{
    if (num_tensors < 1 || num_tensors > kSnapSlots)
        return failf(MARLNAV_EINVAL, "snapshot: num_tensors=%d outside [1, %d]", num_tensors, kSnapSlots);
    if (!src) return marlnav_internal_fail(MARLNAV_EINVAL, "snapshot: src is NULL");
    if (!dst) return marlnav_internal_fail(MARLNAV_EINVAL, "snapshot: dst is NULL");
    if (!numel) return marlnav_internal_fail(MARLNAV_EINVAL, "snapshot: numel is NULL");
    int64_t total = 0;
    for (int i = 0; i < num_tensors; ++i) {
        if (numel[i] < 1) return failf(MARLNAV_EINVAL, "snapshot: numel[%d]=%lld < 1", i, (long long)numel[i]);
        if (numel[i] > kMaxElements - total)
            return failf(MARLNAV_EINVAL, "snapshot: numel[%d]=%lld brings the table past 2^40 elements",
                         i, (long long)numel[i]);
        total += numel[i];
        if (!src[i]) return failf(MARLNAV_EINVAL, "snapshot: src[%d] is NULL", i);
        if (!dst[i]) return failf(MARLNAV_EINVAL, "snapshot: dst[%d] is NULL", i);
        if (addr(src[i]) & 3u) return failf(MARLNAV_EINVAL, "snapshot: src[%d] must be 4-byte aligned", i);
        if (addr(dst[i]) & 3u) return failf(MARLNAV_EINVAL, "snapshot: dst[%d] must be 4-byte aligned", i);
    }
    if (!mean_rew) return marlnav_internal_fail(MARLNAV_EINVAL, "snapshot: mean_rew is NULL");
    if (!max_rew) return marlnav_internal_fail(MARLNAV_EINVAL, "snapshot: max_rew is NULL");
    if (!save_state) return marlnav_internal_fail(MARLNAV_EINVAL, "snapshot: save_state is NULL");
    if ((addr(mean_rew) | addr(max_rew) | addr(save_state)) & 7u)
        return marlnav_internal_fail(
            MARLNAV_EINVAL, "snapshot: mean_rew, max_rew and save_state must be 8-byte aligned");
    if (repeat_index < 0)
        return failf(MARLNAV_EINVAL, "snapshot: repeat_index=%lld < 0", (long long)repeat_index);
    if (track_best != 0 && track_best != 1)
        return failf(MARLNAV_EINVAL, "snapshot: track_best=%d must be 0 or 1", track_best);

    SnapArgs a;
    int64_t items = 0;
    a.vec_mask = 0;
    for (int i = 0; i < kSnapSlots; ++i) {
        const bool used = i < num_tensors;
        a.src[i] = used ? src[i] : nullptr;
        a.dst[i] = used ? dst[i] : nullptr;
        a.numel[i] = used ? numel[i] : 0;
        if (used) {
            items += (numel[i] + 3) / 4;
            if (((addr(src[i]) | addr(dst[i])) & 15u) == 0) a.vec_mask |= 1u << i;
        }
        a.item_end[i] = items;
    }
    a.mean_rew = mean_rew;
    a.max_rew = max_rew;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(snapshot_copy, dim3((unsigned)((items + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(snapshot_book, dim3(1), dim3(64), 0, s, mean_rew, max_rew, save_state,
                       repeat_index, track_best);
    return launch_status();
}
