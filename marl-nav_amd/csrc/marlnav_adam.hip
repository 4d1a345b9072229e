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
#include "host_util.h"
#include "ppo_update.h"

namespace {

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

// The Adam table of an update or phase call must be the network's own: slot i
// is the network's i-th weight, its grad_ pointer and its size.
int check_table(int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab)
{
    struct Slot {
        const float *w;
        float *gw;
        int64_t size;
        const char *name;
    };
#define SLOT(field, size) {b->field, b->grad_##field, size, #field}
    const int64_t H = d->hidden_size, D = d->obs_dim, AD = (int64_t)d->num_agents * D;
    const Slot actor[6] = {SLOT(actor_fc1_w, H * D), SLOT(actor_fc1_b, H),
                           SLOT(actor_mu_w, 2 * H),  SLOT(actor_mu_b, 2),
                           SLOT(actor_std_w, 2 * H), SLOT(actor_std_b, 2)};
    const Slot critic[4] = {SLOT(critic_fc1_w, H * AD), SLOT(critic_fc1_b, H),
                            SLOT(critic_fc2_w, H), SLOT(critic_fc2_b, 1)};
#undef SLOT
    const bool is_actor = network == MARLNAV_NETWORK_ACTOR;
    const Slot *slot = is_actor ? actor : critic;
    const int count = is_actor ? 6 : 4;
    if (ad->num_tensors != count)
        return failf(MARLNAV_EINVAL, "adam table: num_tensors=%d, the %s has %d parameters",
                     ad->num_tensors, is_actor ? "actor" : "critic", count);
    for (int i = 0; i < count; ++i) {
        if (ab->param[i] != slot[i].w)
            return failf(MARLNAV_EINVAL, "adam table: param[%d] is not the ppo buffer %s", i,
                         slot[i].name);
        if (ab->grad[i] != slot[i].gw)
            return failf(MARLNAV_EINVAL, "adam table: grad[%d] is not the ppo buffer grad_%s", i,
                         slot[i].name);
        if (ad->numel[i] != slot[i].size)
            return failf(MARLNAV_EINVAL, "adam table: numel[%d]=%lld, %s has %lld elements", i,
                         (long long)ad->numel[i], slot[i].name, (long long)slot[i].size);
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

// the update's gradient launches and, where they leave it owed, its Adam step
// (gated by the stop where the update is monitored); checked arguments only
int enqueue_update(const PpoUpdate &u, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                   hipStream_t s)
{
    bool adam_owed;
    const int rc = marlnav_internal_ppo_enqueue(&u, d, b, s, &adam_owed);
    if (rc || !adam_owed) return rc;
    return enqueue_adam(u.ad, u.ab, s, u.clip, u.diag_row ? u.stop : nullptr);
}

// a single-update entry's update: never folded, so the plain gradient
// launches, then the Adam step in launches of its own (clip NULL:
// marlnav_adam_step's; given: the clipped step's)
PpoUpdate single_update(int network, double epsilon, double ent_const, int advantage_mode,
                        const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab,
                        const ClipArgs *clip)
{
    PpoUpdate u = {};
    u.network = network;
    u.epsilon = epsilon;
    u.ent_const = ent_const;
    u.advantage_mode = advantage_mode;
    u.ad = ad;
    u.ab = ab;
    u.clip = clip;
    return u;
}

int run_update(const PpoUpdate &u, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
               void *stream)
{
    // every check of both halves before the first launch: the ppo dims
    // (marlnav_ppo_work_size runs them), the Adam arguments, the table, the
    // clip, then what the gradient call checks
    if (marlnav_ppo_work_size(d) < 0) return MARLNAV_EINVAL;
    if (!b) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo buffers is NULL");
    int rc = check_adam(u.ad, u.ab);
    if (rc) return rc;
    rc = check_table(u.network, d, b, u.ad, u.ab);
    if (rc) return rc;
    if (u.clip)
        rc = check_clip(u.clip->max_norm, u.clip->norm_work, u.clip->norm_out, "norm_out");
    if (rc) return rc;
    rc = marlnav_internal_ppo_validate(u.network, u.advantage_mode, d, b);
    if (rc) return rc;
    return enqueue_update(u, d, b, (hipStream_t)stream);
}

}  // namespace

extern "C" int marlnav_ppo_actor_update_mode(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                             double epsilon, double ent_const,
                                             const MarlnavAdamDims *ad,
                                             const MarlnavAdamBuffers *ab, int advantage_mode,
                                             void *stream)
{
    return run_update(single_update(MARLNAV_NETWORK_ACTOR, epsilon, ent_const, advantage_mode, ad,
                                    ab, nullptr), d, b, stream);
}

extern "C" int marlnav_ppo_actor_update_clipped(const MarlnavPpoDims *d,
                                                const MarlnavPpoBuffers *b, double epsilon,
                                                double ent_const, const MarlnavAdamDims *ad,
                                                const MarlnavAdamBuffers *ab, int advantage_mode,
                                                double max_norm, double *norm_work,
                                                double *norm_out, void *stream)
{
    const ClipArgs clip = {max_norm, norm_work, norm_out};
    return run_update(single_update(MARLNAV_NETWORK_ACTOR, epsilon, ent_const, advantage_mode, ad,
                                    ab, &clip), d, b, stream);
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
    return run_update(single_update(MARLNAV_NETWORK_CRITIC, epsilon, 0.0,
                                    MARLNAV_ADVANTAGE_REFERENCE, ad, ab, nullptr), d, b, stream);
}

extern "C" int marlnav_ppo_critic_update_clipped(const MarlnavPpoDims *d,
                                                 const MarlnavPpoBuffers *b, double epsilon,
                                                 const MarlnavAdamDims *ad,
                                                 const MarlnavAdamBuffers *ab, double max_norm,
                                                 double *norm_work, double *norm_out,
                                                 void *stream)
{
    const ClipArgs clip = {max_norm, norm_work, norm_out};
    return run_update(single_update(MARLNAV_NETWORK_CRITIC, epsilon, 0.0,
                                    MARLNAV_ADVANTAGE_REFERENCE, ad, ab, &clip), d, b, stream);
}

// =========================================================================
// the minibatch permutations of the shuffled phase
// =========================================================================
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

}  // namespace

extern "C" int marlnav_minibatch_permutations(int64_t L, int64_t E, uint64_t seed, int network,
                                              uint64_t *counter, int32_t *table, void *stream)
{
    const int rc = check_permutations(L, E, network, counter, table);
    if (rc) return rc;
    enqueue_permutations(L, E, seed, network, counter, table, (hipStream_t)stream);
    return launch_status();
}

// =========================================================================
// one whole train_actor / train_critic as one call (clipped
// §16, monitored §17, shuffled §18)
// =========================================================================
namespace {

// what a phase or work-size entry was given
struct Phase {
    int network;
    const MarlnavPpoDims *d;
    const MarlnavPpoBuffers *b;
    // the minibatch schedule. Contiguous: minibatch j is steps bounds[2 j] ..
    // bounds[2 j + 1] - 1. Shuffled: one launch first draws a permutation of
    // all num_steps steps per epoch into `table`; minibatch j of epoch e is
    // entries [j batch_size, (j + 1) batch_size) of row e, the last one with
    // the num_steps % batch_size left over
    bool shuffled;
    const int64_t *bounds;
    int64_t num_batches;
    int64_t batch_size;
    uint64_t seed;
    uint64_t *counter;
    int32_t *table;
    int64_t num_epochs;
    double epsilon, ent_const;
    int advantage_mode;
    const MarlnavAdamDims *ad;
    const MarlnavAdamBuffers *ab;
    double *loss_log;  // update k writes [k]
    bool clipped;
    ClipArgs clip;  // norm_out: the norm_log (update k writes [k]) or NULL
    bool monitored;
    double target_kl;
    double *diag_log;  // update k writes row k
    int64_t *stop;
};

inline int64_t num_minibatches(const Phase &p)
{
    return p.shuffled ? p.d->num_steps / p.batch_size : p.num_batches;
}

inline int64_t minibatch_steps(const Phase &p, int64_t j)
{
    if (!p.shuffled) return p.bounds[2 * j + 1] - p.bounds[2 * j];
    const int64_t L = p.d->num_steps, bs = p.batch_size;
    return j + 1 < L / bs ? bs : L - j * bs;
}

// minibatches [first_size(p), num_minibatches(p)) have every size the schedule
// has: a shuffled epoch has two
inline int64_t first_size(const Phase &p)
{
    const int64_t B = num_minibatches(p);
    return p.shuffled && B > 1 ? B - 2 : 0;
}

// the schedule against the buffer's steps (checked dims)
int check_schedule(const Phase &p)
{
    const int64_t L = p.d->num_steps;
    if (p.shuffled) {
        if (p.batch_size < 1 || L / p.batch_size < 1)
            return failf(MARLNAV_EINVAL,
                         "shuffle: batch_size=%lld gives no minibatch of %lld steps",
                         (long long)p.batch_size, (long long)L);
        return 0;
    }
    if (p.num_batches < 1)
        return failf(MARLNAV_EINVAL, "train: num_batches=%lld < 1", (long long)p.num_batches);
    if (!p.bounds) return marlnav_internal_fail(MARLNAV_EINVAL, "train: bounds is NULL");
    for (int64_t j = 0; j < p.num_batches; ++j) {
        const int64_t lo = p.bounds[2 * j], hi = p.bounds[2 * j + 1];
        if (lo < 0 || hi <= lo || hi > L)
            return failf(MARLNAV_EINVAL,
                         "train: bounds[%lld]=(%lld, %lld) is not a non-empty range of the %lld "
                         "steps", (long long)j, (long long)lo, (long long)hi, (long long)L);
    }
    return 0;
}

// the structs of minibatch j: dims of its steps, its loss cell; contiguous:
// the data pointers at its first step; shuffled: at step 0 of the storage and
// -> its entries of epoch e's permutation
const int32_t *minibatch(const Phase &p, int64_t e, int64_t j, double *loss, MarlnavPpoDims *md,
                         MarlnavPpoBuffers *mb)
{
    const MarlnavPpoDims *d = p.d;
    const MarlnavPpoBuffers *b = p.b;
    *md = *d;
    md->num_steps = minibatch_steps(p, j);
    *mb = *b;
    mb->loss = loss;
    if (p.shuffled) return p.table + e * d->num_steps + j * p.batch_size;
    const int64_t rows = p.bounds[2 * j] * d->num_parallel, arows = rows * d->num_agents;
    mb->obs = b->obs + arows * d->obs_dim;
    if (b->actions) mb->actions = b->actions + arows * 2;
    if (b->log_probs) mb->log_probs = b->log_probs + arows;
    if (b->values) mb->values = b->values + rows;
    mb->returns = b->returns + rows;
    return nullptr;
}

// the workspace of the schedule's largest minibatch (monitored: of the
// diagnostic variant), in doubles
int64_t phase_work_size(const Phase &p)
{
    if (marlnav_ppo_work_size(p.d) < 0) return MARLNAV_EINVAL;
    const int rc = check_schedule(p);
    if (rc) return rc;
    int64_t need = 0;
    MarlnavPpoDims md = *p.d;
    for (int64_t j = first_size(p); j < num_minibatches(p); ++j) {
        md.num_steps = minibatch_steps(p, j);
        const int64_t w =
            p.monitored ? marlnav_ppo_diag_work_size(&md) : marlnav_ppo_work_size(&md);
        if (w < 0) return w;
        if (w > need) need = w;
    }
    return need;
}

// every check of a phase call before its first launch
int check_phase(const Phase &p)
{
    const int network = p.network;
    if (p.monitored && network == MARLNAV_NETWORK_CRITIC)
        return marlnav_internal_fail(
            MARLNAV_EINVAL, p.shuffled ? "train: target_kl / diag_log / stop monitor the actor; "
                                         "network is MARLNAV_NETWORK_CRITIC"
                                       : "train: the monitored phase is the actor's; network is "
                                         "MARLNAV_NETWORK_CRITIC");
    if (!p.clipped && (p.clip.norm_work || p.clip.norm_out))
        return marlnav_internal_fail(MARLNAV_EINVAL,
                                     "clip: norm_work and norm_log must be NULL with "
                                     "max_norm = MARLNAV_MAX_NORM_NONE");
    int rc = 0;
    if (p.shuffled) {
        if (marlnav_ppo_work_size(p.d) < 0) return MARLNAV_EINVAL;
        rc = check_schedule(p);
        if (rc) return rc;
        rc = check_permutations(p.d->num_steps, p.num_epochs, network, p.counter, p.table);
        if (rc) return rc;
    }
    if (network != MARLNAV_NETWORK_ACTOR && network != MARLNAV_NETWORK_CRITIC)
        return failf(MARLNAV_EINVAL, "train: network=%d must be MARLNAV_NETWORK_ACTOR or _CRITIC", network);
    if (p.advantage_mode != MARLNAV_ADVANTAGE_REFERENCE && p.advantage_mode != MARLNAV_ADVANTAGE_ENV)
        return failf(MARLNAV_EINVAL, "train: advantage_mode=%d must be MARLNAV_ADVANTAGE_REFERENCE or _ENV",
                     p.advantage_mode);
    // the own-env pairing is the actor's: it reads no values
    const bool need_values =
        network == MARLNAV_NETWORK_CRITIC || p.advantage_mode == MARLNAV_ADVANTAGE_REFERENCE;
    if (marlnav_ppo_work_size(p.d) < 0) return MARLNAV_EINVAL;
    const MarlnavPpoBuffers *b = p.b;
    if (!b) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo buffers is NULL");
    if (p.num_epochs < 1)
        return failf(MARLNAV_EINVAL, "train: num_epochs=%lld < 1", (long long)p.num_epochs);
    if (!p.shuffled) rc = check_schedule(p);
    if (rc) return rc;
    if (!p.loss_log) return marlnav_internal_fail(MARLNAV_EINVAL, "train: loss_log is NULL");
    if (addr(p.loss_log) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "train: loss_log must be 8-byte aligned");
    rc = check_adam(p.ad, p.ab);
    if (rc) return rc;
    rc = check_table(network, p.d, b, p.ad, p.ab);
    if (rc) return rc;
    if (p.clipped) rc = check_clip(p.clip.max_norm, p.clip.norm_work, p.clip.norm_out, "norm_log");
    if (rc) return rc;
    if (!b->obs) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: buffer obs is NULL");
    if (need_values && !b->values)
        return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: buffer values is NULL");
    if (!b->returns) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: buffer returns is NULL");
    MarlnavPpoDims md;
    MarlnavPpoBuffers mb;
    for (int64_t j = first_size(p); j < num_minibatches(p); ++j) {  // dims and buffers
        minibatch(p, 0, j, p.loss_log, &md, &mb);
        rc = marlnav_internal_ppo_validate(network, p.advantage_mode, &md, &mb);
        if (rc) return rc;
    }
    if (!p.monitored) return 0;
    if (!(p.target_kl > 0.0))  // a NaN is not greater
        return failf(MARLNAV_EINVAL, "train: target_kl=%g must be > 0 (+inf: monitor only)",
                     p.target_kl);
    if (!p.diag_log) return marlnav_internal_fail(MARLNAV_EINVAL, "train: diag_log is NULL");
    if (addr(p.diag_log) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "train: diag_log must be 8-byte aligned");
    if (!p.stop) return marlnav_internal_fail(MARLNAV_EINVAL, "train: stop is NULL");
    if (addr(p.stop) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "train: stop must be 8-byte aligned");
    return 0;
}

// the phase: its checks, the permutations of a shuffled schedule, then
// num_epochs x num_minibatches updates, epoch-major. Which launches an update
// is, marlnav_ppo.hip decides ("The launch paths").
int run_phase(const Phase &p, void *stream)
{
    int rc = check_phase(p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (p.shuffled) {
        enqueue_permutations(p.d->num_steps, p.num_epochs, p.seed, p.network, p.counter, p.table,
                             s);
        rc = launch_status();
        if (rc) return rc;
    }
    PpoUpdate u = {};
    u.network = p.network;
    u.epsilon = p.epsilon;
    u.ent_const = p.ent_const;
    u.advantage_mode = p.advantage_mode;
    u.stop = p.stop;
    u.target_kl = p.target_kl;
    u.ad = p.ad;
    u.ab = p.ab;
    u.may_fold = true;
    ClipArgs clip = p.clip;
    if (p.clipped) u.clip = &clip;
    MarlnavPpoDims md;
    MarlnavPpoBuffers mb;
    const int64_t B = num_minibatches(p);
    for (int64_t e = 0, k = 0; e < p.num_epochs; ++e)
        for (int64_t j = 0; j < B; ++j, ++k) {
            u.steps = minibatch(p, e, j, p.loss_log + k, &md, &mb);
            u.k = k;
            if (p.monitored) u.diag_row = p.diag_log + MARLNAV_DIAG_ROW * k;
            if (p.clip.norm_out) clip.norm_out = p.clip.norm_out + k;
            rc = enqueue_update(u, &md, &mb, s);
            if (rc) return rc;
        }
    return 0;
}

Phase make_phase(int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                       const int64_t *bounds, int64_t num_batches, int64_t num_epochs,
                       double epsilon, double ent_const, const MarlnavAdamDims *ad,
                       const MarlnavAdamBuffers *ab, double *loss_log, int advantage_mode)
{
    Phase p = {};
    p.network = network;
    p.d = d;
    p.b = b;
    p.bounds = bounds;
    p.num_batches = num_batches;
    p.num_epochs = num_epochs;
    p.epsilon = epsilon;
    p.ent_const = ent_const;
    p.ad = ad;
    p.ab = ab;
    p.loss_log = loss_log;
    p.advantage_mode = advantage_mode;
    return p;
}

}  // namespace

extern "C" int64_t marlnav_ppo_train_work_size(const MarlnavPpoDims *d, const int64_t *bounds,
                                               int64_t num_batches)
{
    Phase p = {};
    p.d = d;
    p.bounds = bounds;
    p.num_batches = num_batches;
    return phase_work_size(p);
}

extern "C" int64_t marlnav_ppo_train_diag_work_size(const MarlnavPpoDims *d,
                                                    const int64_t *bounds, int64_t num_batches)
{
    Phase p = {};
    p.d = d;
    p.bounds = bounds;
    p.num_batches = num_batches;
    p.monitored = true;
    return phase_work_size(p);
}

extern "C" int64_t marlnav_ppo_train_shuffled_work_size(const MarlnavPpoDims *d,
                                                        int64_t batch_size, int diag)
{
    Phase p = {};
    p.d = d;
    p.shuffled = true;
    p.batch_size = batch_size;
    p.monitored = diag != 0;
    return phase_work_size(p);
}

extern "C" int marlnav_ppo_train_phase_mode(int network, const MarlnavPpoDims *d,
                                            const MarlnavPpoBuffers *b, const int64_t *bounds,
                                            int64_t num_batches, int64_t num_epochs,
                                            double epsilon, double ent_const,
                                            const MarlnavAdamDims *ad,
                                            const MarlnavAdamBuffers *ab, double *loss_log,
                                            int advantage_mode, void *stream)
{
    return run_phase(make_phase(network, d, b, bounds, num_batches, num_epochs, epsilon,
                                      ent_const, ad, ab, loss_log, advantage_mode), stream);
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
    Phase p = make_phase(network, d, b, bounds, num_batches, num_epochs, epsilon, ent_const,
                               ad, ab, loss_log, advantage_mode);
    p.clipped = true;
    p.clip = {max_norm, norm_work, norm_log};
    return run_phase(p, stream);
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

extern "C" int marlnav_ppo_train_phase_monitored(
    int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, const int64_t *bounds,
    int64_t num_batches, int64_t num_epochs, double epsilon, double ent_const,
    const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab, double *loss_log, int advantage_mode,
    double max_norm, double *norm_work, double *norm_log, double target_kl, double *diag_log,
    int64_t *stop, void *stream)
{
    Phase p = make_phase(network, d, b, bounds, num_batches, num_epochs, epsilon, ent_const,
                               ad, ab, loss_log, advantage_mode);
    p.clipped = max_norm != MARLNAV_MAX_NORM_NONE;  // a NaN is refused by check_clip
    p.clip = {max_norm, norm_work, norm_log};
    p.monitored = true;
    p.target_kl = target_kl;
    p.diag_log = diag_log;
    p.stop = stop;
    return run_phase(p, stream);
}

extern "C" int marlnav_ppo_train_phase_shuffled(
    int network, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, int64_t batch_size,
    int64_t num_epochs, double epsilon, double ent_const, const MarlnavAdamDims *ad,
    const MarlnavAdamBuffers *ab, double *loss_log, int advantage_mode, double max_norm,
    double *norm_work, double *norm_log, double target_kl, double *diag_log, int64_t *stop,
    uint64_t seed, uint64_t *counter, int32_t *table, void *stream)
{
    Phase p = make_phase(network, d, b, nullptr, 0, num_epochs, epsilon, ent_const, ad, ab,
                               loss_log, advantage_mode);
    p.shuffled = true;
    p.batch_size = batch_size;
    p.seed = seed;
    p.counter = counter;
    p.table = table;
    p.clipped = max_norm != MARLNAV_MAX_NORM_NONE;  // a NaN is refused by check_clip
    p.clip = {max_norm, norm_work, norm_log};
    p.monitored = target_kl != 0.0 || diag_log || stop;
    p.target_kl = target_kl;
    p.diag_log = diag_log;
    p.stop = stop;
    return run_phase(p, stream);
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
