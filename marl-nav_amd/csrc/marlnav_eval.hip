// marlnav_eval.hip - gfx950 kernels for running a trained policy without
// training it: the reference's rendering loop (marlnav/animation.py:40-71,
// init_render :80-96) minus the drawing, plus the episode figures an
// evaluation reports.
//
// marlnav_actor_act: Actor.forward (models.py:27-36) and dist.loc or
// dist.sample() for all P*A agent rows in one launch. It is the actor third
// of policy_kernel (marlnav_policy.hip): the collapse
//   Weff = [Wmu; Wstd] W1 (4 x D), beff = [Wmu; Wstd] b1 + [bmu; bstd]
// recomputed per block from the live weight tensors (four waves each summing
// their quarter of the hidden units in groups of eight, the partials added in
// wave order) on policy_forward.h's LDS layout, then that header's row_chains
// (from beff, k ascending) and sample_action, so an action here has the bits
// marlnav_policy_act gives it. The collapse is policy_forward.h's written out
// in the kernel (measured: the comment there).
// What is gone is
// the critic (at 16 agents x 32 obstacles a 307 KB first layer streamed per
// 64 envs) and, in MEAN mode, everything after tanh. A block owns
// kRowsPerBlock consecutive agent rows whatever env they belong to; every
// output is a function of its own row.
//
// eval_init_kernel / eval_track_kernel / eval_summary_kernel: per-env episode
// returns and lengths accumulated after every step (thread = env, its own
// rewards in step order, fp64), an optional record of one env's states, and
// the totals over the envs by one block in a fixed order (no atomics).
//
// marlnav_rollout_evaluate chains them with the existing observe / step
// launches, as marlnav_rollout_collect (marlnav_rollout.hip) chains a rollout.
//
// Built with -ffp-contract=off: every FMA is explicit.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/marlnav.h"

#include "host_util.h"

namespace {

#include "policy_forward.h"

constexpr int kRowsPerBlock = kThreads;  // agent rows of a block: one per thread (measured
                                         // against 64, 128, 512, 1024: DESIGN.md §13)
static_assert(collapse_lds_floats(kMaxD) * sizeof(float) <= 64 * 1024, "LDS of the widest row");

struct ActorArgs {
    const float *obs_norm, *fc1_w, *fc1_b, *mu_w, *mu_b, *std_w, *std_b, *eps;
    float *actions, *eps_out;
    int64_t rows;      // P * A
    int64_t row_base;  // env_offset * A: global id of row 0
    int D, H;
    uint64_t seed;     // native_seed_mix(policy_seed)
    uint64_t step;
};

// D_T: compiled row length (0: run-time D, inputs read from memory as used)
template <int D_T, int MODE>
__global__ void __launch_bounds__(kThreads) actor_kernel(ActorArgs g)
{
    const int D = D_T ? D_T : g.D;
    const float *__restrict__ obs = g.obs_norm;

    // LDS, all in the dynamic region (the layout of policy_forward.h): Weff as
    // [k][4], the four waves' partial Weff, beff, its partials
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    float *s_w = s_dyn;
    float *s_wp = lds_wp(s_dyn, D);
    float *s_b = lds_b(s_dyn, D);
    float *s_bp = lds_bp(s_dyn, D);

    const int t = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(t >> 6);  // wave of the block
    const int lane = t & 63;
    const int H = g.H;
    int j0, j1;
    wave_share(H, q, j0, j1);

    // ---- the collapse: collapse_partials and collapse_sum (policy_forward.h)
    // written out, operation for operation. Called as functions they gave
    // actor_kernel<0, *> the same instructions in another order on 54 VGPRs
    // for 42, 0.06-0.08 us slower at 4 096 x 16 x 32 in every pass (9.99 / 10.78
    // against 9.94 / 10.70 us, mean / sample); written out the six kernels
    // compile to the code they had (DESIGN.md §13,
    // profiles/policy_share_bench.txt). tests/test_evaluate_gpu.py holds the two
    // to equal bits.
    {
        const float *__restrict__ w1 = g.fc1_w;
        const float *__restrict__ b1 = g.fc1_b;
        for (int idx = lane; idx < 4 * D + 4; idx += 64) {
            const bool bias = idx >= 4 * D;
            const int r = bias ? idx - 4 * D : idx / D;
            const int k = bias ? 0 : idx - r * D;
            const float *__restrict__ head = (r < 2 ? g.mu_w : g.std_w) + (r & 1) * H;
            const float *__restrict__ col = bias ? b1 : w1 + k;
            const int64_t stride = bias ? 1 : D;
            float acc = 0.0f;
            for (int j = j0; j < j1; j += 8) {
                float a[8], b[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int jj = j + i < j1 ? j + i : j1 - 1;  // a short last group repeats a unit
                    a[i] = head[jj];
                    b[i] = col[jj * stride];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (j + i < j1) acc = __builtin_fmaf(a[i], b[i], acc);
            }
            if (bias)
                s_bp[4 * q + r] = acc;
            else
                s_wp[q * 4 * D + 4 * k + r] = acc;
        }
    }
    __syncthreads();  // the waves' partial Weff and beff are in LDS

    // the partial sums, added in wave order
    for (int idx = t; idx < 4 * D; idx += kThreads) {
        float v = s_wp[idx];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += s_wp[w * 4 * D + idx];
        s_w[idx] = v;
    }
    if (t < 4) {
        float v = s_bp[t];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += s_bp[4 * w + t];
        s_b[t] = (t < 2 ? g.mu_b : g.std_b)[t & 1] + v;
    }
    __syncthreads();  // Weff and beff are in LDS

    // ---- one thread per agent row (MEAN never reads the two covariance
    // chains, so they are not formed)
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + t;
    const float4 be = *reinterpret_cast<const float4 *>(s_b);
    if (row < g.rows) {
        const float4 p = row_chains<D_T, MODE == MARLNAV_ACT_SAMPLE>(obs + row * D, D, be, s_w);
        const float mu0 = tanhf(p.x), mu1 = tanhf(p.y);
        if constexpr (MODE == MARLNAV_ACT_MEAN) {
            g.actions[2 * row] = mu0;  // dist.loc
            g.actions[2 * row + 1] = mu1;
        } else {
            float e0, e1;
            sample_action(g.eps, g.eps_out, g.actions, mu0, mu1, softplus_t(p.z), softplus_t(p.w),
                          row, g.seed, (uint64_t)(g.row_base + row), g.step, e0, e1);
        }
    }
}

using ActorFn = void (*)(ActorArgs);

struct ActorVariant {
    int D;
    ActorFn fn[2];  // by mode
};

// the generic path, then the compiled row lengths: 3 agents x 3 and x 8
// obstacles (the benchmark's)
const ActorVariant kGeneric = {
    0, {actor_kernel<0, MARLNAV_ACT_MEAN>, actor_kernel<0, MARLNAV_ACT_SAMPLE>}};
const ActorVariant kVariants[] = {
    {12, {actor_kernel<12, MARLNAV_ACT_MEAN>, actor_kernel<12, MARLNAV_ACT_SAMPLE>}},
    {22, {actor_kernel<22, MARLNAV_ACT_MEAN>, actor_kernel<22, MARLNAV_ACT_SAMPLE>}},
};

// ------------------------------------------------------------ the tracker
struct TrackArgs {
    MarlnavEvalBuffers b;
    const float *states;     // the buffer the step wrote (row 0: the current one)
    const float *obstacles;
    const float *target;
    const float *step_num;   // the start only
    int64_t P;
    int64_t row;             // trace row to write: 0 at the start, t + 1 after step t
    int A, S;
};

// the traced env's state into row g.row of the record, by the block's threads
__device__ __forceinline__ void trace_row(const TrackArgs &g)
{
    const int64_t e = g.b.trace_env;
    const int ns = g.A * 5, no = g.S * 2;
    for (int i = threadIdx.x; i < ns + no + 2; i += kThreads) {
        if (i < ns)
            g.b.trace_states[g.row * ns + i] = g.states[e * ns + i];
        else if (i < ns + no)
            g.b.trace_obstacles[g.row * no + (i - ns)] = g.obstacles[e * no + (i - ns)];
        else
            g.b.trace_target[g.row * 2 + (i - ns - no)] = g.target[e * 2 + (i - ns - no)];
    }
}

// blocks [0, ceil(P / kThreads)): thread = env; one further block when an
// env is traced
__global__ void __launch_bounds__(kThreads) eval_init_kernel(TrackArgs g)
{
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if ((int64_t)blockIdx.x * kThreads >= g.P) {
        trace_row(g);
        return;
    }
    if (p >= g.P) return;
    g.b.cur_return[p] = 0.0;
    g.b.cur_len[p] = 0;
    g.b.whole[p] = g.step_num[p] == 0.0f;
    g.b.ep_count[p] = 0;
    g.b.ret_sum[p] = 0.0;
    g.b.ret_sqsum[p] = 0.0;
    g.b.ret_min[p] = INFINITY;
    g.b.ret_max[p] = -INFINITY;
    g.b.len_sum[p] = 0;
    g.b.partial_count[p] = 0;
}

__global__ void __launch_bounds__(kThreads) eval_track_kernel(TrackArgs g)
{
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if ((int64_t)blockIdx.x * kThreads >= g.P) {
        trace_row(g);
        if (threadIdx.x == 0) {
            const int64_t e = g.b.trace_env, t = g.row - 1;
            g.b.trace_reward[t] = g.b.reward[e];
            g.b.trace_terminated[t] = g.b.terminated[e];
            g.b.trace_truncated[t] = g.b.truncated[e];
        }
        return;
    }
    if (p >= g.P) return;
    // what every env needs, loaded before the first use: one memory round trip
    const double cur = g.b.cur_return[p];
    const float rew = g.b.reward[p];
    const int32_t cur_len = g.b.cur_len[p];
    const bool done = (g.b.terminated[p] | g.b.truncated[p]) != 0;  // models.py:117
    const bool whole = g.b.whole[p] != 0;
    const double ret = cur + (double)rew;
    const int32_t len = cur_len + 1;
    if (done) {
        if (whole) {
            g.b.ep_count[p] += 1;
            g.b.ret_sum[p] += ret;
            const double sq = ret * ret;  // one product and one sum (-ffp-contract=off)
            g.b.ret_sqsum[p] += sq;
            g.b.len_sum[p] += len;
            if (ret < g.b.ret_min[p]) g.b.ret_min[p] = ret;
            if (ret > g.b.ret_max[p]) g.b.ret_max[p] = ret;
        } else {
            g.b.partial_count[p] += 1;
            g.b.whole[p] = 1;
        }
        g.b.cur_return[p] = 0.0;
        g.b.cur_len[p] = 0;
    } else {
        g.b.cur_return[p] = ret;
        g.b.cur_len[p] = len;
    }
}

// v of every thread folded by op down a fixed tree through LDS
template <int N, typename T, typename Op>
__device__ __forceinline__ T block_fold(T v, T *sh, Op op)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = N / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + off]);
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

// the totals over the envs: one block of kSummaryThreads (the loop is a chain
// of memory round trips: the more threads, the fewer trips), each thread its
// envs p = t, t + kSummaryThreads, ... in ascending order, then the fixed tree
constexpr int kSummaryThreads = 1024;

__global__ void __launch_bounds__(kSummaryThreads) eval_summary_kernel(MarlnavEvalBuffers b,
                                                                       int64_t P)
{
    __shared__ double sh_f[kSummaryThreads];
    __shared__ int64_t sh_i[kSummaryThreads];
    int64_t epi = 0, par = 0, len = 0;
    double sum = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t p = threadIdx.x; p < P; p += kSummaryThreads) {
        epi += b.ep_count[p];
        par += b.partial_count[p];
        len += b.len_sum[p];
        sum += b.ret_sum[p];
        sq += b.ret_sqsum[p];
        mn = b.ret_min[p] < mn ? b.ret_min[p] : mn;
        mx = b.ret_max[p] > mx ? b.ret_max[p] : mx;
    }
    auto addi = [](int64_t x, int64_t y) { return x + y; };
    auto addf = [](double x, double y) { return x + y; };
    epi = block_fold<kSummaryThreads>(epi, sh_i, addi);
    par = block_fold<kSummaryThreads>(par, sh_i, addi);
    len = block_fold<kSummaryThreads>(len, sh_i, addi);
    sum = block_fold<kSummaryThreads>(sum, sh_f, addf);
    sq = block_fold<kSummaryThreads>(sq, sh_f, addf);
    mn = block_fold<kSummaryThreads>(mn, sh_f, [](double x, double y) { return y < x ? y : x; });
    mx = block_fold<kSummaryThreads>(mx, sh_f, [](double x, double y) { return y > x ? y : x; });
    if (threadIdx.x == 0) {
        b.totals_i[0] = epi;
        b.totals_i[1] = par;
        b.totals_i[2] = len;
        b.totals_f[0] = sum;
        b.totals_f[1] = sq;
        b.totals_f[2] = mn;
        b.totals_f[3] = mx;
    }
}

// ObsNormalizer (utils.py:519-532) of packed (P, A, D) observations, as the
// rollout's row 0: one IEEE subtraction and one IEEE division per element
__global__ void __launch_bounds__(kThreads) eval_obs_norm_kernel(const float *__restrict__ obs,
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

// the shape checks of marlnav_policy_act and the actor's grid limit, for `who`
int check_policy_dims(const char *who, const MarlnavPolicyDims *d)
{
    if (int rc = check_policy_shape(who, d->num_parallel, d->num_agents, d->obs_dim,
                                    d->hidden_size))
        return rc;
    if (d->reserved != 0 || d->env_offset < 0)
        return failf(MARLNAV_EINVAL, "%s: reserved=%d must be 0 and env_offset=%lld >= 0", who,
                     d->reserved, (long long)d->env_offset);
    const int64_t nblk = (d->num_parallel * d->num_agents + kRowsPerBlock - 1) / kRowsPerBlock;
    if (nblk > 0x7fffffff)
        return failf(MARLNAV_EINVAL, "%s: num_parallel=%lld too large", who,
                     (long long)d->num_parallel);
    return 0;
}

int check_mode(const char *who, int mode)
{
    if (mode != MARLNAV_ACT_MEAN && mode != MARLNAV_ACT_SAMPLE)
        return failf(MARLNAV_EINVAL, "%s: mode=%d is neither MARLNAV_ACT_MEAN (0) nor "
                     "MARLNAV_ACT_SAMPLE (1)", who, mode);
    return 0;
}

// the one actor launch (everything checked by the caller)
int launch_actor(const MarlnavPolicyDims *d, const MarlnavPolicyBuffers *b, int mode,
                 uint64_t policy_seed, uint64_t step_idx, hipStream_t stream)
{
    ActorArgs a;
    a.obs_norm = b->obs_norm;
    a.fc1_w = b->actor_fc1_w, a.fc1_b = b->actor_fc1_b;
    a.mu_w = b->actor_mu_w, a.mu_b = b->actor_mu_b;
    a.std_w = b->actor_std_w, a.std_b = b->actor_std_b;
    a.eps = b->eps;
    a.actions = b->actions;
    a.eps_out = b->eps_out;
    a.rows = d->num_parallel * d->num_agents;
    a.row_base = d->env_offset * d->num_agents;
    a.D = d->obs_dim;
    a.H = d->hidden_size;
    a.seed = native_seed_mix(policy_seed);
    a.step = step_idx;
    const ActorVariant *v = &kGeneric;
    // the compiled row lengths load rows as 16- / 8-byte vectors
    if ((reinterpret_cast<uintptr_t>(b->obs_norm) & 15u) == 0)
        for (const ActorVariant &c : kVariants)
            if (c.D == a.D) v = &c;
    const int64_t nblk = (a.rows + kRowsPerBlock - 1) / kRowsPerBlock;
    const size_t lds = sizeof(float) * collapse_lds_floats(a.D);
    hipLaunchKernelGGL(v->fn[mode], dim3((unsigned)nblk), dim3(kThreads), lds, stream, a);
    return launch_status();
}

}  // namespace

extern "C" {

int marlnav_actor_act(const MarlnavPolicyDims *d, const MarlnavPolicyBuffers *b, int mode,
                      uint64_t policy_seed, uint64_t step_idx, void *stream)
{
    if (!d || !b) return marlnav_internal_fail(MARLNAV_EINVAL, "actor dims/buffers is NULL");
    if (int rc = check_mode("actor", mode)) return rc;
    if (int rc = check_policy_dims("actor", d)) return rc;
    if (!b->obs_norm || !b->actor_fc1_w || !b->actor_fc1_b || !b->actor_mu_w || !b->actor_mu_b ||
        !b->actor_std_w || !b->actor_std_b || !b->actions)
        return marlnav_internal_fail(MARLNAV_EINVAL, "a required actor buffer is NULL");
    return launch_actor(d, b, mode, policy_seed, step_idx, (hipStream_t)stream);
}

int marlnav_rollout_evaluate(const MarlnavDims *dims, const MarlnavParams *params,
                             const MarlnavStepBuffers *env, uint64_t env_step_idx0,
                             const MarlnavPolicyDims *pdims, const MarlnavPolicyBuffers *policy,
                             int mode, uint64_t policy_seed, uint64_t policy_step_idx0,
                             const MarlnavEvalBuffers *eval, int64_t T, void *stream)
{
    constexpr int64_t kMaxSteps = (int64_t)1 << 20;
    const char *who = "marlnav_rollout_evaluate";
    // ---- everything is checked before the first launch
    if (!dims || !params || !env || !pdims || !policy || !eval)
        return failf(MARLNAV_EINVAL, "%s: %s is NULL", who,
                     !dims ? "dims" : !params ? "params" : !env ? "env" : !pdims ? "pdims"
                     : !policy ? "policy" : "eval");
    if (int rc = check_mode(who, mode)) return rc;
    if (T < 1 || T > kMaxSteps)
        return failf(MARLNAV_EINVAL, "%s: T=%lld outside [1, %lld]", who, (long long)T,
                     (long long)kMaxSteps);
    if (marlnav_counter_slots(dims) < 0) return MARLNAV_EINVAL;  // (the message names the field)
    const int64_t P = dims->num_parallel;
    const int A = dims->num_agents, S = dims->obstacle_stride;
    const int D = 2 + 2 * dims->num_obstacles + 2 * (A - 1);
    if (pdims->num_agents != A)
        return failf(MARLNAV_EINVAL, "%s: policy num_agents=%d, env %d", who, pdims->num_agents, A);
    if (pdims->obs_dim != D)
        return failf(MARLNAV_EINVAL, "%s: policy obs_dim=%d, the env's rows have "
                     "2 + 2*O + 2*(A-1) = %d", who, pdims->obs_dim, D);
    if (pdims->num_parallel != P)
        return failf(MARLNAV_EINVAL, "%s: policy num_parallel=%lld, env %lld", who,
                     (long long)pdims->num_parallel, (long long)P);
    if (pdims->env_offset != dims->env_offset || dims->env_offset < 0)
        return failf(MARLNAV_EINVAL, "%s: policy env_offset=%lld, env %lld (equal and >= 0)", who,
                     (long long)pdims->env_offset, (long long)dims->env_offset);
    if (int rc = check_policy_dims(who, pdims)) return rc;
    if (!(params->flags & MARLNAV_WRITE_OBS_NORM))
        return failf(MARLNAV_EINVAL, "%s: params->flags lacks MARLNAV_WRITE_OBS_NORM (the actor "
                     "reads the steps' normalised observations)", who);
    if (!(params->flags & MARLNAV_SCALE_ACTIONS))
        return failf(MARLNAV_EINVAL, "%s: params->flags lacks MARLNAV_SCALE_ACTIONS (the steps "
                     "read the policy-scale actions)", who);
    if (env->fresh_states)
        return failf(MARLNAV_EINVAL, "%s: fresh_states is given: re-init from the reference's "
                     "RNG needs the host every step (native re-init only)", who);
#define MARLNAV_NEED(s, f) \
    if (!(s)->f) return failf(MARLNAV_EINVAL, "%s: " #s "->" #f " is NULL", who)
    MARLNAV_NEED(env, states);
    MARLNAV_NEED(env, obstacles);
    MARLNAV_NEED(env, target);
    MARLNAV_NEED(env, step_num);
    MARLNAV_NEED(env, terminates);
    MARLNAV_NEED(env, formation);
    MARLNAV_NEED(env, obs);
    MARLNAV_NEED(env, norm_mean);
    MARLNAV_NEED(env, norm_scale);
    MARLNAV_NEED(policy, actor_fc1_w);
    MARLNAV_NEED(policy, actor_fc1_b);
    MARLNAV_NEED(policy, actor_mu_w);
    MARLNAV_NEED(policy, actor_mu_b);
    MARLNAV_NEED(policy, actor_std_w);
    MARLNAV_NEED(policy, actor_std_b);
    MARLNAV_NEED(eval, obs_norm_a);
    MARLNAV_NEED(eval, obs_norm_b);
    MARLNAV_NEED(eval, actions);
    MARLNAV_NEED(eval, reward);
    MARLNAV_NEED(eval, terminated);
    MARLNAV_NEED(eval, truncated);
    MARLNAV_NEED(eval, cur_return);
    MARLNAV_NEED(eval, cur_len);
    MARLNAV_NEED(eval, whole);
    MARLNAV_NEED(eval, ep_count);
    MARLNAV_NEED(eval, ret_sum);
    MARLNAV_NEED(eval, ret_sqsum);
    MARLNAV_NEED(eval, ret_min);
    MARLNAV_NEED(eval, ret_max);
    MARLNAV_NEED(eval, len_sum);
    MARLNAV_NEED(eval, partial_count);
    MARLNAV_NEED(eval, totals_i);
    MARLNAV_NEED(eval, totals_f);
    if (eval->reserved != 0)
        return failf(MARLNAV_EINVAL, "%s: eval->reserved=%lld must be 0", who,
                     (long long)eval->reserved);
    if (eval->trace_env < -1 || eval->trace_env >= P)
        return failf(MARLNAV_EINVAL, "%s: eval->trace_env=%lld outside [-1, num_parallel=%lld)",
                     who, (long long)eval->trace_env, (long long)P);
    const bool trace = eval->trace_env >= 0;
    if (trace) {
        MARLNAV_NEED(eval, trace_states);
        MARLNAV_NEED(eval, trace_obstacles);
        MARLNAV_NEED(eval, trace_target);
        MARLNAV_NEED(eval, trace_reward);
        MARLNAV_NEED(eval, trace_terminated);
        MARLNAV_NEED(eval, trace_truncated);
    }
#undef MARLNAV_NEED
    if (reinterpret_cast<uintptr_t>(eval->actions) & 7u)
        return failf(MARLNAV_EINVAL, "%s: eval->actions must be 8-byte aligned", who);
    const int64_t row_obs = P * A * D;  // floats of one observation buffer
    const size_t obs_bytes = (size_t)row_obs * sizeof(float);
    const size_t state_bytes = (size_t)P * A * 5 * sizeof(float);
    if (env->states_out && overlap(env->states, state_bytes, env->states_out, state_bytes))
        return failf(MARLNAV_EINVAL, "%s: env->states_out overlaps states", who);
    if (overlap(eval->obs_norm_a, obs_bytes, eval->obs_norm_b, obs_bytes))
        return failf(MARLNAV_EINVAL, "%s: eval->obs_norm_b overlaps obs_norm_a (a step would "
                     "write the observations its actor launch read)", who);
    if (overlap(env->obs, obs_bytes, eval->obs_norm_a, obs_bytes) ||
        overlap(env->obs, obs_bytes, eval->obs_norm_b, obs_bytes))
        return failf(MARLNAV_EINVAL, "%s: eval->obs_norm_a / obs_norm_b overlaps env->obs", who);
    const int64_t env_blocks = (P + kThreads - 1) / kThreads;
    const int64_t norm_blocks = (row_obs + kThreads - 1) / kThreads;
    if (norm_blocks > 0x7fffffff || env_blocks + 1 > 0x7fffffff)
        return failf(MARLNAV_EINVAL, "%s: num_parallel=%lld too large", who, (long long)P);

    // ---- the observations of the current state, normalised (animation.py:42)
    hipStream_t s = (hipStream_t)stream;
    if (int rc = marlnav_observe(dims, params, env->states, env->obstacles, env->target, env->obs,
                                 stream))
        return fail_step(who, rc, 0, "marlnav_observe");
    hipLaunchKernelGGL(eval_obs_norm_kernel, dim3((unsigned)norm_blocks), dim3(kThreads), 0, s,
                       env->obs, env->norm_mean, env->norm_scale, row_obs, D, eval->obs_norm_a);
    if (int rc = launch_status()) return fail_step(who, rc, 0, "normaliser");

    // ---- the tracker's start and trace row 0
    TrackArgs ta;
    ta.b = *eval;
    ta.states = env->states;
    ta.obstacles = env->obstacles;
    ta.target = env->target;
    ta.step_num = env->step_num;
    ta.P = P;
    ta.row = 0;
    ta.A = A;
    ta.S = S;
    const dim3 track_grid((unsigned)(env_blocks + (trace ? 1 : 0)));
    hipLaunchKernelGGL(eval_init_kernel, track_grid, dim3(kThreads), 0, s, ta);
    if (int rc = launch_status()) return fail_step(who, rc, 0, "tracker start");

    // ---- the steps (animation.py:40-71)
    MarlnavPolicyBuffers pb = *policy;
    pb.eps = nullptr;
    pb.eps_out = nullptr;
    pb.actions = eval->actions;
    MarlnavStepBuffers sb = *env;
    sb.fresh_states = sb.fresh_obstacles = sb.fresh_target = nullptr;
    sb.actions = eval->actions;
    sb.reward = eval->reward;
    sb.terminated = eval->terminated;
    sb.truncated = eval->truncated;
    for (int64_t t = 0; t < T; ++t) {
        pb.obs_norm = (t & 1) ? eval->obs_norm_b : eval->obs_norm_a;
        if (int rc = launch_actor(pdims, &pb, mode, policy_seed, policy_step_idx0 + (uint64_t)t, s))
            return fail_step(who, rc, t, "marlnav_actor_act");
        sb.obs_norm = (t & 1) ? eval->obs_norm_a : eval->obs_norm_b;
        if (int rc = marlnav_step(dims, params, &sb, env_step_idx0 + (uint64_t)t, stream))
            return fail_step(who, rc, t, "marlnav_step");
        if (sb.states_out) {  // the step wrote the new states there: current from here on
            float *cur = sb.states_out;
            sb.states_out = sb.states;
            sb.states = cur;
        }
        ta.states = sb.states;
        ta.row = t + 1;
        hipLaunchKernelGGL(eval_track_kernel, track_grid, dim3(kThreads), 0, s, ta);
        if (int rc = launch_status()) return fail_step(who, rc, t, "tracker");
    }

    hipLaunchKernelGGL(eval_summary_kernel, dim3(1), dim3(kSummaryThreads), 0, s, *eval, P);
    if (int rc = launch_status()) return fail_step(who, rc, T - 1, "totals after it");
    return 0;
}

}  // extern "C"
