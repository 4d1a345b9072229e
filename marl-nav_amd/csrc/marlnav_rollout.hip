// marlnav_rollout.hip - gfx950 kernels for the rollout side of the training
// loop that drives Env.step: MAPPO._process_rewards (marlnav/models.py:131-148)
// as a device scan instead of a Python loop of T x 3 small tensor ops.
//
// Layout: rewards (T, P) fp32 and done (T, P) bool as stacked step rows; one
// thread per env walks its column backwards (coalesced across the wave), in
// float64 as the reference accumulates (torch.zeros(P, dtype=float)). Mean
// and unbiased std are two-pass block reductions in a fixed order, so results
// are deterministic run to run.
//
// marlnav_gae_advantages: the GAE(lambda) scan of the opt-in advantage mode
// (DESIGN.md §15), the same one-thread-per-env backward walk with the critic's
// values and a bootstrap value beside the rewards, and the same reductions.
//
// marlnav_rollout_collect: the whole of MAPPO.get_data (models.py:106-125) as
// one host call that enqueues the existing observe / policy / step launches
// back to back, each step kernel writing its normalised observations straight
// into the next row of the stacked rollout storage. Two small kernels of its
// own: the ObsNormalizer of row 0 (the later rows come normalised out of the
// step kernels) and the merge of the terminated / truncated flag stacks.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/marlnav.h"

#include "host_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

#include "block_sum.h"

// G_t = done_t ? 0 : r_t + gamma * G_{t+1}  (models.py:133-137)
__global__ void __launch_bounds__(kThreads) returns_kernel(const float *__restrict__ rew,
                                                            const uint8_t *__restrict__ done,
                                                            int64_t T, int64_t P, double gamma,
                                                            double *__restrict__ ret,
                                                            double *__restrict__ partial)
{
    __shared__ double sh[kWaves];
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double s = 0.0;
    if (e < P) {
        double g = 0.0;
        for (int64_t t = T - 1; t >= 0; --t) {
            const int64_t i = t * P + e;
            g = done[i] ? 0.0 : (double)rew[i] + gamma * g;
            ret[i] = g;
            s += g;
        }
    }
    const double b = block_sum(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

// GAE(lambda): one thread per env walks its column backwards
// in fp64, as returns_kernel does. Selects, not products with a mask, so a
// non-finite value behind a done cannot leak. gl = gamma * lambda (host, fp64).
//   next  = t == T-1 ? last[p] : val[t+1][p]
//   delta = (r + gamma * (done ? 0 : next)) - v
//   A     = delta + gl * (done ? 0 : A_next)
//   vt    = A + v
__global__ void __launch_bounds__(kThreads) gae_kernel(const float *__restrict__ rew,
                                                        const uint8_t *__restrict__ done,
                                                        const float *__restrict__ val,
                                                        const float *__restrict__ last, int64_t T,
                                                        int64_t P, double gamma, double gl,
                                                        double *__restrict__ adv,
                                                        double *__restrict__ vt,
                                                        double *__restrict__ partial)
{
    __shared__ double sh[kWaves];
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double s = 0.0;
    if (e < P) {
        double a = 0.0;
        double next = (double)last[e];
        for (int64_t t = T - 1; t >= 0; --t) {
            const int64_t i = t * P + e;
            const bool d = done[i] != 0;
            const double v = (double)val[i];
            const double delta = ((double)rew[i] + gamma * (d ? 0.0 : next)) - v;
            a = delta + gl * (d ? 0.0 : a);
            adv[i] = a;
            vt[i] = a + v;
            s += a;
            next = v;
        }
    }
    const double b = block_sum(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

// sum of the block partials in index order -> out (one block)
__global__ void __launch_bounds__(kThreads) finish_kernel(const double *__restrict__ partial,
                                                           int64_t nb, int64_t n, int mode,
                                                           double *__restrict__ stats)
{
    __shared__ double sh[kWaves];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < nb; i += kThreads) s += partial[i];
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) {
        if (mode == 0)
            stats[0] = t / (double)n;                // mean
        else
            stats[1] = sqrt(t / (double)(n - 1));    // unbiased std
    }
}

__global__ void __launch_bounds__(kThreads) sqdev_kernel(const double *__restrict__ ret,
                                                          int64_t T, int64_t P,
                                                          const double *__restrict__ stats,
                                                          double *__restrict__ partial)
{
    __shared__ double sh[kWaves];
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const double mean = stats[0];
    double s = 0.0;
    if (e < P)
        for (int64_t t = T - 1; t >= 0; --t) {
            const double d = ret[t * P + e] - mean;
            s += d * d;
        }
    const double b = block_sum(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

// (G - mean) / (std + 1e-12)  (models.py:143-144)
__global__ void __launch_bounds__(kThreads) normalize_kernel(double *__restrict__ ret, int64_t T,
                                                              int64_t P,
                                                              const double *__restrict__ stats)
{
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= P) return;
    const double mean = stats[0], den = stats[1] + 1e-12;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t i = t * P + e;
        ret[i] = (ret[i] - mean) / den;
    }
}

int64_t blocks_for(int64_t P) { return (P + kThreads - 1) / kThreads; }

// ObsNormalizer (utils.py:519-532) of packed (P, A, D) observations: one IEEE
// subtraction and one IEEE division per element, the step kernels' fused
// normaliser (kernel_block.h) on row 0 of a rollout. One thread per element.
__global__ void __launch_bounds__(kThreads) obs_norm_kernel(const float *__restrict__ obs,
                                                             const float *__restrict__ mean,
                                                             const float *__restrict__ scale,
                                                             int64_t n, int D,
                                                             float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int k = (int)(i % D);
    out[i] = (obs[i] - mean[k]) / scale[k];
}

// bytes 0 / 1 of (a | b) != 0 for the four (eight) bytes of a word: every
// byte's bits are or-ed down into its bit 0
__device__ __forceinline__ uint32_t any_bits(uint32_t x)
{
    x |= x >> 4;
    x |= x >> 2;
    x |= x >> 1;
    return x & 0x01010101u;
}

// done[i] = (done[i] | trunc[i]) != 0 over n bytes (models.py:117 for a whole
// rollout). The first `head` bytes, up to done's 16-byte boundary, and the
// last n - head - 16 nvec one at a time, the nvec pieces between as 16-byte
// vectors; the host passes head = n (nvec = 0) when the two pointers are not
// equally placed within 16 bytes. One thread per piece or single byte.
__global__ void __launch_bounds__(kThreads) merge_flags_kernel(uint8_t *__restrict__ done,
                                                                const uint8_t *__restrict__ trunc,
                                                                int64_t n, int64_t head,
                                                                int64_t nvec)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g < nvec) {
        uint4 a = *reinterpret_cast<const uint4 *>(done + head + 16 * g);
        const uint4 b = *reinterpret_cast<const uint4 *>(trunc + head + 16 * g);
        a.x = any_bits(a.x | b.x);
        a.y = any_bits(a.y | b.y);
        a.z = any_bits(a.z | b.z);
        a.w = any_bits(a.w | b.w);
        *reinterpret_cast<uint4 *>(done + head + 16 * g) = a;
        return;
    }
    const int64_t k = g - nvec;                       // k-th single byte
    const int64_t i = k < head ? k : k + 16 * nvec;   // head bytes, then the tail
    if (i >= n) return;
    done[i] = (done[i] | trunc[i]) != 0;
}

}  // namespace

extern "C" {

int64_t marlnav_returns_work_size(int64_t P)
{
    return P < 1 ? -1 : 2 * blocks_for(P);
}

int marlnav_discounted_returns(const float *rewards, const uint8_t *done, int64_t T, int64_t P,
                               double gamma, double *returns, double *stats, double *work,
                               void *stream)
{
    if (T < 1 || P < 1) return marlnav_internal_fail(MARLNAV_EINVAL, "T and P must be >= 1");
    if (!rewards || !done || !returns || !stats || !work)
        return marlnav_internal_fail(MARLNAV_EINVAL, "a required returns buffer is NULL");
    const int64_t nb = blocks_for(P);
    if (nb > 0x7fffffff) return marlnav_internal_fail(MARLNAV_EINVAL, "P too large");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nb), blk(kThreads);
    hipLaunchKernelGGL(returns_kernel, grid, blk, 0, s, rewards, done, T, P, gamma, returns, work);
    hipLaunchKernelGGL(finish_kernel, dim3(1), blk, 0, s, work, nb, T * P, 0, stats);
    hipLaunchKernelGGL(sqdev_kernel, grid, blk, 0, s, returns, T, P, stats, work + nb);
    hipLaunchKernelGGL(finish_kernel, dim3(1), blk, 0, s, work + nb, nb, T * P, 1, stats);
    hipLaunchKernelGGL(normalize_kernel, grid, blk, 0, s, returns, T, P, stats);
    return launch_status();
}

int64_t marlnav_gae_work_size(int64_t P)
{
    return P < 1 ? -1 : 2 * blocks_for(P);
}

int marlnav_gae_advantages(const float *rewards, const uint8_t *done, const float *values,
                           const float *last_values, int64_t T, int64_t P, double gamma,
                           double lam, double *advantages, double *value_targets, double *stats,
                           double *work, void *stream)
{
    // ---- everything is checked before the first launch
#define MARLNAV_GAE_NEED(f) \
    if (!f) return failf(MARLNAV_EINVAL, "marlnav_gae_advantages: " #f " is NULL")
    MARLNAV_GAE_NEED(rewards);
    MARLNAV_GAE_NEED(done);
    MARLNAV_GAE_NEED(values);
    MARLNAV_GAE_NEED(last_values);
    MARLNAV_GAE_NEED(advantages);
    MARLNAV_GAE_NEED(value_targets);
    MARLNAV_GAE_NEED(stats);
    MARLNAV_GAE_NEED(work);
#undef MARLNAV_GAE_NEED
    if (T < 1) return failf(MARLNAV_EINVAL, "marlnav_gae_advantages: T=%lld < 1", (long long)T);
    if (P < 1) return failf(MARLNAV_EINVAL, "marlnav_gae_advantages: P=%lld < 1", (long long)P);
    if (T > ((int64_t)1 << 40) / P)
        return failf(MARLNAV_EINVAL, "marlnav_gae_advantages: T=%lld x P=%lld values are too many",
                     (long long)T, (long long)P);
    if (T * P < 2)
        return failf(MARLNAV_EINVAL, "marlnav_gae_advantages: T=%lld x P=%lld gives fewer than 2 "
                     "values (the unbiased std needs 2)", (long long)T, (long long)P);
    if (!(gamma >= 0.0 && gamma <= 1.0))  // a NaN fails both
        return failf(MARLNAV_EINVAL, "marlnav_gae_advantages: gamma=%g outside [0, 1]", gamma);
    if (!(lam >= 0.0 && lam <= 1.0))
        return failf(MARLNAV_EINVAL, "marlnav_gae_advantages: lam=%g outside [0, 1]", lam);
    const int64_t nb = blocks_for(P);
    if (nb > 0x7fffffff)
        return failf(MARLNAV_EINVAL, "marlnav_gae_advantages: P=%lld too large", (long long)P);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nb), blk(kThreads);
    const double gl = gamma * lam;
    hipLaunchKernelGGL(gae_kernel, grid, blk, 0, s, rewards, done, values, last_values, T, P,
                       gamma, gl, advantages, value_targets, work);
    // mean, unbiased std and the normalisation: the returns path's launches
    hipLaunchKernelGGL(finish_kernel, dim3(1), blk, 0, s, work, nb, T * P, 0, stats);
    hipLaunchKernelGGL(sqdev_kernel, grid, blk, 0, s, advantages, T, P, stats, work + nb);
    hipLaunchKernelGGL(finish_kernel, dim3(1), blk, 0, s, work + nb, nb, T * P, 1, stats);
    hipLaunchKernelGGL(normalize_kernel, grid, blk, 0, s, advantages, T, P, stats);
    return launch_status();
}

int marlnav_rollout_collect(const MarlnavDims *dims, const MarlnavParams *params,
                            const MarlnavStepBuffers *env, uint64_t env_step_idx0,
                            const MarlnavPolicyDims *pdims, const MarlnavPolicyBuffers *policy,
                            uint64_t policy_seed, uint64_t policy_step_idx0,
                            const MarlnavRolloutBuffers *rollout, int64_t T, double gamma,
                            void *stream)
{
    constexpr int64_t kMaxSteps = (int64_t)1 << 20;
    const char *who = "marlnav_rollout_collect";
    // ---- everything is checked before the first launch
    if (!dims || !params || !env || !pdims || !policy || !rollout)
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: %s is NULL",
                     !dims ? "dims" : !params ? "params" : !env ? "env" : !pdims ? "pdims"
                     : !policy ? "policy" : "rollout");
    if (T < 1 || T > kMaxSteps)
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: T=%lld outside [1, %lld]",
                     (long long)T, (long long)kMaxSteps);
    if (marlnav_counter_slots(dims) < 0) return MARLNAV_EINVAL;  // (the message names the field)
    const int64_t P = dims->num_parallel;
    const int A = dims->num_agents;
    const int D = 2 + 2 * dims->num_obstacles + 2 * (A - 1);
    if (pdims->num_agents != A)
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: policy num_agents=%d, env %d",
                     pdims->num_agents, A);
    if (pdims->obs_dim != D)
        return failf(MARLNAV_EINVAL,
                     "marlnav_rollout_collect: policy obs_dim=%d, the env's rows have "
                     "2 + 2*O + 2*(A-1) = %d", pdims->obs_dim, D);
    if (pdims->num_parallel != P)
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: policy num_parallel=%lld, env %lld",
                     (long long)pdims->num_parallel, (long long)P);
    if (pdims->env_offset != dims->env_offset || dims->env_offset < 0)
        return failf(MARLNAV_EINVAL,
                     "marlnav_rollout_collect: policy env_offset=%lld, env %lld (equal and >= 0)",
                     (long long)pdims->env_offset, (long long)dims->env_offset);
    if (pdims->hidden_size < 1 || pdims->hidden_size > kMaxHidden)
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: policy hidden_size=%d outside "
                     "[1, %d]", pdims->hidden_size, kMaxHidden);
    if (pdims->reserved != 0)
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: policy reserved=%d must be 0",
                     pdims->reserved);
    if (!(params->flags & MARLNAV_WRITE_OBS_NORM))
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: params->flags lacks "
                     "MARLNAV_WRITE_OBS_NORM (the policy reads the steps' normalised observations)");
    if (!(params->flags & MARLNAV_SCALE_ACTIONS))
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: params->flags lacks "
                     "MARLNAV_SCALE_ACTIONS (the steps read the policy-scale actions)");
    if (env->fresh_states)
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: fresh_states is given: re-init "
                     "from the reference's RNG needs the host every step (native re-init only)");
#define MARLNAV_NEED(s, f) \
    if (!(s)->f) return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: " #s "->" #f " is NULL")
    MARLNAV_NEED(env, states);
    MARLNAV_NEED(env, obstacles);
    MARLNAV_NEED(env, target);
    MARLNAV_NEED(env, step_num);
    MARLNAV_NEED(env, terminates);
    MARLNAV_NEED(env, formation);
    MARLNAV_NEED(env, obs);
    MARLNAV_NEED(env, obs_norm);
    MARLNAV_NEED(env, norm_mean);
    MARLNAV_NEED(env, norm_scale);
    MARLNAV_NEED(policy, actor_fc1_w);
    MARLNAV_NEED(policy, actor_fc1_b);
    MARLNAV_NEED(policy, actor_mu_w);
    MARLNAV_NEED(policy, actor_mu_b);
    MARLNAV_NEED(policy, actor_std_w);
    MARLNAV_NEED(policy, actor_std_b);
    MARLNAV_NEED(policy, critic_fc1_w);
    MARLNAV_NEED(policy, critic_fc1_b);
    MARLNAV_NEED(policy, critic_fc2_w);
    MARLNAV_NEED(policy, critic_fc2_b);
    MARLNAV_NEED(rollout, obs);
    MARLNAV_NEED(rollout, actions);
    MARLNAV_NEED(rollout, log_probs);
    MARLNAV_NEED(rollout, values);
    MARLNAV_NEED(rollout, rewards);
    MARLNAV_NEED(rollout, done);
    MARLNAV_NEED(rollout, truncated);
#undef MARLNAV_NEED
    const bool want_returns = rollout->returns || rollout->returns_stats || rollout->returns_work;
    if (want_returns && (!rollout->returns || !rollout->returns_stats || !rollout->returns_work))
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: rollout->returns, returns_stats "
                     "and returns_work must all be given or all be NULL");
    if (reinterpret_cast<uintptr_t>(rollout->actions) & 7u)
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: rollout->actions must be 8-byte "
                     "aligned");
    const int64_t row_obs = P * A * D;  // floats of one observation row
    const int64_t nflags = T * P;
    const size_t state_bytes = (size_t)P * A * 5 * sizeof(float);
    if (env->states_out && overlap(env->states, state_bytes, env->states_out, state_bytes))
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: env->states_out overlaps states");
    if (overlap(rollout->obs, (size_t)T * row_obs * sizeof(float), env->obs_norm,
                (size_t)row_obs * sizeof(float)))
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: rollout->obs overlaps "
                     "env->obs_norm (the last step's observations would land in the stack)");
    if (overlap(rollout->done, (size_t)nflags, rollout->truncated, (size_t)nflags))
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: rollout->truncated overlaps done");
    // the merge: 16-byte pieces where done and truncated are equally placed
    int64_t head = nflags, nvec = 0;
    {
        const uintptr_t d0 = reinterpret_cast<uintptr_t>(rollout->done);
        if (((d0 ^ reinterpret_cast<uintptr_t>(rollout->truncated)) & 15u) == 0) {
            head = (int64_t)((16 - (d0 & 15u)) & 15u);
            if (head > nflags) head = nflags;
            nvec = (nflags - head) / 16;
        }
    }
    const int64_t merge_blocks = blocks_for(nvec + (nflags - 16 * nvec));
    const int64_t norm_blocks = blocks_for(row_obs);
    if (merge_blocks > 0x7fffffff || norm_blocks > 0x7fffffff || P > ((int64_t)64 << 31) - 64)
        return failf(MARLNAV_EINVAL, "marlnav_rollout_collect: num_parallel=%lld (x T=%lld) too "
                     "large", (long long)P, (long long)T);

    // ---- row 0: the observations of the current state, normalised (models.py:110)
    hipStream_t s = (hipStream_t)stream;
    if (int rc = marlnav_observe(dims, params, env->states, env->obstacles, env->target, env->obs,
                                 stream))
        return fail_step(who, rc, 0, "marlnav_observe");
    hipLaunchKernelGGL(obs_norm_kernel, dim3((unsigned)norm_blocks), dim3(kThreads), 0, s, env->obs,
                       env->norm_mean, env->norm_scale, row_obs, D, rollout->obs);
    if (int rc = launch_status()) return fail_step(who, rc, 0, "normaliser");

    // ---- the steps (models.py:113-124)
    MarlnavPolicyBuffers pb = *policy;
    pb.eps_out = nullptr;
    MarlnavStepBuffers sb = *env;
    sb.fresh_states = sb.fresh_obstacles = sb.fresh_target = nullptr;
    for (int64_t t = 0; t < T; ++t) {
        pb.obs_norm = rollout->obs + t * row_obs;
        pb.eps = rollout->eps ? rollout->eps + t * P * A * 2 : nullptr;
        pb.actions = rollout->actions + t * P * A * 2;
        pb.log_probs = rollout->log_probs + t * P * A;
        pb.values = rollout->values + t * P;
        if (int rc = marlnav_policy_act(pdims, &pb, policy_seed, policy_step_idx0 + (uint64_t)t,
                                        stream))
            return fail_step(who, rc, t, "marlnav_policy_act");
        sb.actions = pb.actions;
        sb.reward = rollout->rewards + t * P;
        sb.terminated = rollout->done + t * P;
        sb.truncated = rollout->truncated + t * P;
        sb.obs_norm = t + 1 < T ? rollout->obs + (t + 1) * row_obs : env->obs_norm;
        if (int rc = marlnav_step(dims, params, &sb, env_step_idx0 + (uint64_t)t, stream))
            return fail_step(who, rc, t, "marlnav_step");
        if (sb.states_out) {  // the step wrote the new states there: current from here on
            float *cur = sb.states_out;
            sb.states_out = sb.states;
            sb.states = cur;
        }
    }

    // ---- done = terminated | truncated over the whole stack (models.py:117)
    hipLaunchKernelGGL(merge_flags_kernel, dim3((unsigned)merge_blocks), dim3(kThreads), 0, s,
                       rollout->done, rollout->truncated, nflags, head, nvec);
    if (launch_status())
        return failf(MARLNAV_ELAUNCH, "marlnav_rollout_collect: after step %lld, flag merge: %s",
                     (long long)(T - 1), marlnav_last_error());
    if (want_returns)
        if (int rc = marlnav_discounted_returns(rollout->rewards, rollout->done, T, P, gamma,
                                                rollout->returns, rollout->returns_stats,
                                                rollout->returns_work, stream))
            return fail_step(who, rc, T - 1, "marlnav_discounted_returns after it");
    return 0;
}

}  // extern "C"
