// marlnav_policy.hip - gfx950 kernel for the forward-only policy half of
// MAPPO.get_data (marlnav/models.py:113-120): Actor.forward (models.py:27-36),
// MultivariateNormal sample + log_prob, Critic.forward (models.py:51-56), for
// all P*A agent rows and P envs in one launch.
//
// What it computes (the reference's quirks are part of the contract):
//   h   = W1 x + b1                       no activation after fc1 (models.py:29)
//   mu  = tanh(Wmu h + bmu)               (models.py:30)
//   v   = softplus(Wstd h + bstd)         torch's: x > 20 ? x : log1p(exp(x))
//   v is the COVARIANCE diagonal of the MultivariateNormal (models.py:32-34),
//   so  action   = mu + sqrt(v) * eps
//       log_prob = -(eps0^2 + eps1^2)/2 - (log v0 + log v1)/2 - log(2 pi)
//   value = W2 relu(Wc flatten(x_env) + bc) + b2          (models.py:51-56)
//
// Layout. A block of 256 threads owns 64 consecutive envs.
//  * Collapse. fc1 has no activation, so the actor's two layers are one
//    affine map: Weff = [Wmu; Wstd] W1 (4 x D), beff = [Wmu; Wstd] b1 +
//    [bmu; bstd]. Every block recomputes it from the live weight tensors
//    (4 D dot products of length H) into LDS, so an in-place optimiser step
//    is seen by the next call; an actor row then costs 4 D FMAs instead of
//    H (D + 4). Each of the block's four waves sums a quarter of the hidden
//    units with its loads issued in groups of eight (the block's critical
//    path is memory latency, not FMAs); the four partials are added in wave
//    order.
//  * Critic. Thread (env e = t & 63, wave q = t >> 6) sums the hidden units
//    [q Hq, (q + 1) Hq), Hq = ceil(H / 4): the weight indices are
//    wave-uniform, so the weights arrive through the scalar cache as SGPR
//    operands of the FMAs (no LDS copy, which at 16 agents x 32 obstacles
//    would not fit: 1536 x 50 fp32), and the four waves of a block share one
//    env tile's rows in L1. The four partial sums are added in wave order.
//    Compiled shapes hold the env's A D inputs in VGPRs; the generic path
//    re-reads them per group of four hidden units.
//  * Actor. One thread per agent row of the block's envs: D x 4 FMAs against
//    the collapsed weights (LDS, one broadcast 16-byte read per feature).
// Every output element is a function of its own row / env only (fixed
// summation orders, no atomics), so results do not depend on P, on the
// block an env lands in, or on how envs are split across devices.
//
// Noise. eps given: the caller's normals (torch's generator reproduces the
// reference's stream). eps NULL: one Philox2x32-10 block (device_rng.h) per
// agent row, keyed by (policy_seed, kPolicyBlock, step_idx) with the GLOBAL
// row id (env_offset + e) A + a as the counter; Box-Muller on its two words.
// The re-init draws of the step kernels use block indices < 2^10 (obstacle
// j, then the noisy agents' 3 uniforms per agent), the policy uses 2^31:
// native_key() hashes blk * odd constant, a bijection, so under one seed and
// step the two domains never share a key.
//
// The collapse, the row chains, the sampling tail and the critic sum are the
// functions of policy_forward.h, which actor_kernel (marlnav_eval.hip) shares
// too (all but the collapse, written out there); policy_kernel and
// critic_values_kernel are their own thread-to-row mappings and barriers
// around them.
//
// Built with -ffp-contract=off: every FMA is explicit.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/marlnav.h"

#include "host_util.h"

namespace {

#include "policy_forward.h"

constexpr int kEnvsPerBlock = 64;
// dynamic LDS floats of a block: the collapse, then the critic partials
constexpr size_t lds_floats(int D) { return collapse_lds_floats(D) + kWaves * kEnvsPerBlock; }
static_assert(lds_floats(kMaxD) * sizeof(float) <= 64 * 1024, "LDS of the widest row");

struct PolicyArgs {
    MarlnavPolicyBuffers b;
    int64_t P, env_offset;
    int A, D, H;
    uint64_t seed;  // native_seed_mix(policy_seed)
    uint64_t step;
};

// A_T, D_T: compiled shape (0: run-time A, D; inputs read from memory as used)
template <int A_T, int D_T>
__global__ void __launch_bounds__(kThreads) policy_kernel(PolicyArgs g)
{
    static_assert((A_T != 0) == (D_T != 0), "a compiled shape fixes both");
    const int A = A_T ? A_T : g.A;
    const int D = D_T ? D_T : g.D;
    const int64_t P = g.P;
    const float *__restrict__ obs = g.b.obs_norm;

    // LDS, all in the dynamic region: the collapse, then the critic partials
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    float *s_part = lds_bp(s_dyn, D) + 4 * kWaves;

    const int t = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(t >> 6);  // wave of the block
    const int lane = t & 63;
    int j0, j1;
    wave_share(g.H, q, j0, j1);

    collapse_partials<D_T>(g.b.actor_fc1_w, g.b.actor_fc1_b, g.b.actor_mu_w, g.b.actor_std_w, D,
                           g.H, q, lane, j0, j1, s_dyn);
    // critic: wave q sums hidden units [j0, j1) for the block's 64 envs
    {
        const int64_t env_raw = (int64_t)blockIdx.x * kEnvsPerBlock + lane;
        const int64_t env = env_raw < P ? env_raw : P - 1;  // lanes past the end stay in bounds
        s_part[q * kEnvsPerBlock + lane] =
            critic_partial<A_T * D_T>(obs + env * (A * D), g.b.critic_fc1_w, g.b.critic_fc1_b,
                                      g.b.critic_fc2_w, A * D, j0, j1);
    }
    __syncthreads();  // the waves' partial Weff, beff and critic sums are in LDS

    collapse_sum(g.b.actor_mu_b, g.b.actor_std_b, D, t, s_dyn);
    if (t < kEnvsPerBlock) {
        const int64_t env = (int64_t)blockIdx.x * kEnvsPerBlock + t;
        if (env < P) g.b.values[env] = critic_total(s_part, kEnvsPerBlock, t, g.b.critic_fc2_b);
    }
    __syncthreads();  // Weff and beff are in LDS

    // ---- actor: one thread per agent row of the block's envs
    const int64_t row0 = (int64_t)blockIdx.x * kEnvsPerBlock * A;
    const int64_t rows_total = P * A;
    const int rows_block = kEnvsPerBlock * A;
    const float4 be = *reinterpret_cast<const float4 *>(lds_b(s_dyn, D));
    for (int r = t; r < rows_block; r += kThreads) {
        const int64_t row = row0 + r;
        if (row >= rows_total) break;
        const float4 p = row_chains<D_T, true>(obs + row * D, D, be, s_dyn);
        const float mu0 = tanhf(p.x), mu1 = tanhf(p.y);
        const float v0 = softplus_t(p.z), v1 = softplus_t(p.w);
        float e0, e1;
        sample_action(g.b.eps, g.b.eps_out, g.b.actions, mu0, mu1, v0, v1, row, g.seed,
                      (uint64_t)(g.env_offset * A + row), g.step, e0, e1);
        const float m = __builtin_fmaf(e1, e1, e0 * e0);
        const float ld = logf(v0) + logf(v1);
        g.b.log_probs[row] = __builtin_fmaf(-0.5f, m, __builtin_fmaf(-0.5f, ld, -kLog2Pi));
    }
}

// The critic of policy_kernel alone (marlnav_critic_values):
// the same blocks of 64 envs, the same wave shares of the hidden units and the
// same critic_partial / critic_total calls, so values[env] carries the bits
// policy_kernel stores for the same observations and weights. It is a kernel
// of its own, not a mode of policy_kernel. Reads no actor tensor and draws
// nothing.
template <int A_T, int D_T>
__global__ void __launch_bounds__(kThreads) critic_values_kernel(PolicyArgs g)
{
    const int AD = (A_T ? A_T : g.A) * (D_T ? D_T : g.D);
    const int64_t P = g.P;
    __shared__ float s_part[kWaves * kEnvsPerBlock];

    const int t = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(t >> 6);
    const int e = t & 63;
    int j0, j1;
    wave_share(g.H, q, j0, j1);

    const int64_t env_raw = (int64_t)blockIdx.x * kEnvsPerBlock + e;
    const int64_t env = env_raw < P ? env_raw : P - 1;  // lanes past the end stay in bounds
    s_part[q * kEnvsPerBlock + e] =
        critic_partial<A_T * D_T>(g.b.obs_norm + env * AD, g.b.critic_fc1_w, g.b.critic_fc1_b,
                                  g.b.critic_fc2_w, AD, j0, j1);
    __syncthreads();
    if (t < kEnvsPerBlock && env_raw < P)
        g.b.values[env_raw] = critic_total(s_part, kEnvsPerBlock, t, g.b.critic_fc2_b);
}

using PolicyFn = void (*)(PolicyArgs);

// compiled shapes: 3 agents x 3 and x 8 obstacles (the benchmark's), then the
// generic kernels
struct PolicyVariant {
    int A, D;
    PolicyFn act, values;
};
const PolicyVariant kVariants[] = {
    {3, 12, policy_kernel<3, 12>, critic_values_kernel<3, 12>},
    {3, 22, policy_kernel<3, 22>, critic_values_kernel<3, 22>},
};
const PolicyVariant kGeneric = {0, 0, policy_kernel<0, 0>, critic_values_kernel<0, 0>};

// the dims checks of both entry points; 0 or the failing code
int check_dims(const MarlnavPolicyDims *d, const MarlnavPolicyBuffers *b)
{
    if (!d || !b) return marlnav_internal_fail(MARLNAV_EINVAL, "policy dims/buffers is NULL");
    if (int rc = check_policy_shape("policy", d->num_parallel, d->num_agents, d->obs_dim,
                                    d->hidden_size))
        return rc;
    if (d->reserved != 0 || d->env_offset < 0)
        return failf(MARLNAV_EINVAL, "policy: reserved=%d must be 0 and env_offset=%lld >= 0",
                     d->reserved, (long long)d->env_offset);
    return 0;
}

// what a launch of either entry point needs (dims checked, buffers given)
struct PolicyLaunch {
    PolicyArgs args;
    const PolicyVariant *variant;
    dim3 grid;
};

// 0 and the launch filled in, or the failing code
int plan_launch(const MarlnavPolicyDims *d, const MarlnavPolicyBuffers *b, uint64_t seed,
                uint64_t step, PolicyLaunch &l)
{
    const int64_t nblk = (d->num_parallel + kEnvsPerBlock - 1) / kEnvsPerBlock;
    if (nblk > 0x7fffffff)
        return failf(MARLNAV_EINVAL, "policy: num_parallel=%lld too large",
                     (long long)d->num_parallel);
    l.args.b = *b;
    l.args.P = d->num_parallel;
    l.args.env_offset = d->env_offset;
    l.args.A = d->num_agents;
    l.args.D = d->obs_dim;
    l.args.H = d->hidden_size;
    l.args.seed = seed;
    l.args.step = step;
    l.grid = dim3((unsigned)nblk);
    l.variant = &kGeneric;
    // the compiled shapes load rows as 16- / 8-byte vectors
    if ((reinterpret_cast<uintptr_t>(b->obs_norm) & 15u) == 0)
        for (const PolicyVariant &v : kVariants)
            if (v.A == l.args.A && v.D == l.args.D) l.variant = &v;
    return 0;
}

}  // namespace

extern "C" int marlnav_policy_act(const MarlnavPolicyDims *d, const MarlnavPolicyBuffers *b,
                                  uint64_t policy_seed, uint64_t step_idx, void *stream)
{
    if (int rc = check_dims(d, b)) return rc;
    if (!b->obs_norm || !b->actor_fc1_w || !b->actor_fc1_b || !b->actor_mu_w || !b->actor_mu_b ||
        !b->actor_std_w || !b->actor_std_b || !b->critic_fc1_w || !b->critic_fc1_b ||
        !b->critic_fc2_w || !b->critic_fc2_b || !b->actions || !b->log_probs || !b->values)
        return marlnav_internal_fail(MARLNAV_EINVAL, "a required policy buffer is NULL");
    PolicyLaunch l;
    if (int rc = plan_launch(d, b, native_seed_mix(policy_seed), step_idx, l)) return rc;
    const size_t lds = sizeof(float) * lds_floats(l.args.D);
    hipLaunchKernelGGL(l.variant->act, l.grid, dim3(kThreads), lds, (hipStream_t)stream, l.args);
    return launch_status();
}

extern "C" int marlnav_critic_values(const MarlnavPolicyDims *d, const MarlnavPolicyBuffers *b,
                                     void *stream)
{
    if (int rc = check_dims(d, b)) return rc;
    if (!b->obs_norm || !b->critic_fc1_w || !b->critic_fc1_b || !b->critic_fc2_w ||
        !b->critic_fc2_b || !b->values)
        return marlnav_internal_fail(
            MARLNAV_EINVAL, "critic values: a required buffer (obs_norm, critic_*, values) is NULL");
    PolicyLaunch l;
    if (int rc = plan_launch(d, b, 0, 0, l)) return rc;
    hipLaunchKernelGGL(l.variant->values, l.grid, dim3(kThreads), 0, (hipStream_t)stream, l.args);
    return launch_status();
}
