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
// Built with -ffp-contract=off: every FMA below is explicit.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "../../include/marlnav.h"

__attribute__((visibility("hidden"))) int marlnav_internal_fail(int code, const char *msg);

namespace {

#include "device_rng.h"

constexpr int kThreads = 256;
constexpr int kEnvsPerBlock = 64;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxAgentsP = 64, kMaxObstP = 256, kMaxHidden = 512;
constexpr int kMaxD = 2 * kMaxAgentsP + 2 * kMaxObstP;  // 640
// dynamic LDS floats of a block: Weff and its kWaves partials (4 D each),
// beff and its partials, the critic partials
constexpr size_t lds_floats(int D)
{
    return (size_t)(1 + kWaves) * 4 * D + 4 + 4 * kWaves + kWaves * kEnvsPerBlock;
}
static_assert(lds_floats(kMaxD) * sizeof(float) <= 64 * 1024, "LDS of the widest row");
constexpr uint32_t kPolicyBlock = 0x80000000u;           // Philox block-index domain
constexpr float kLog2Pi = 1.8378770664093453f;

struct PolicyArgs {
    MarlnavPolicyBuffers b;
    int64_t P, env_offset;
    int A, D, H;
    uint64_t seed;  // native_seed_mix(policy_seed)
    uint64_t step;
};

// N consecutive floats at p into registers with the widest loads N allows
// (the caller guarantees p is 16-byte aligned when N % 4 == 0, 8-byte when
// N % 2 == 0: obs is 16-byte aligned and rows are N floats apart)
template <int N>
__device__ __forceinline__ void load_row(const float *__restrict__ p, float (&x)[N])
{
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
            const float4 v = reinterpret_cast<const float4 *>(p)[i];
            x[4 * i] = v.x, x[4 * i + 1] = v.y, x[4 * i + 2] = v.z, x[4 * i + 3] = v.w;
        }
    } else if constexpr (N % 2 == 0) {
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            const float2 v = reinterpret_cast<const float2 *>(p)[i];
            x[2 * i] = v.x, x[2 * i + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = p[i];
    }
}

__device__ __forceinline__ float relu_t(float a) { return a < 0.0f ? 0.0f : a; }  // NaN stays

// torch.nn.functional.softplus (beta 1, threshold 20)
__device__ __forceinline__ float softplus_t(float x) { return x > 20.0f ? x : log1pf(expf(x)); }

// two standard normals of global agent row gid at step s: Box-Muller on the
// two words of one Philox block, u1 in (0, 1], u2 in [0, 1) on the 24-bit grid
__device__ __forceinline__ void policy_normals(uint64_t seed, uint64_t gid, uint64_t s, float &z0,
                                               float &z1)
{
    uint32_t r0, r1;
    native_block(seed, kPolicyBlock, gid, s, r0, r1);
    const float u1 = (float)((r0 >> 8) + 1u) * 0x1.0p-24f;
    const float u2 = native_u24(r1);
    const float rad = sqrtf(-2.0f * logf(u1));
    // v_sin_f32 / v_cos_f32 take the angle in revolutions: no range reduction
    z0 = rad * __builtin_amdgcn_cosf(u2);
    z1 = rad * __builtin_amdgcn_sinf(u2);
}

// A_T, D_T: compiled shape (0: run-time A, D; inputs read from memory as used)
template <int A_T, int D_T>
__global__ void __launch_bounds__(kThreads) policy_kernel(PolicyArgs g)
{
    const int A = A_T ? A_T : g.A;
    const int D = D_T ? D_T : g.D;
    const int H = g.H;
    const int AD = A * D;
    const int64_t P = g.P;
    const float *__restrict__ obs = g.b.obs_norm;

    // LDS, all in the dynamic region (16-byte aligned base and offsets):
    // Weff as [k][4], the four waves' partial Weff, beff, its partials, the
    // critic partials
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    float *s_w = s_dyn;
    float *s_wp = s_w + 4 * D;
    float *s_b = s_wp + kWaves * 4 * D;
    float *s_bp = s_b + 4;
    float *s_part = s_bp + 4 * kWaves;

    const int t = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(t >> 6);  // wave of the block
    const int lane = t & 63;
    // wave q's share of the hidden units, in the collapse and in the critic
    const int Hq = (H + kWaves - 1) / kWaves;
    const int j0 = q * Hq, j1 = (j0 + Hq < H) ? j0 + Hq : H;

    // ---- collapse the actor: Weff[r][k] = sum_j head_r[j] W1[j][k], each
    // wave summing its hidden units (the loads of a group of 8 issued before
    // the first FMA: a rolled loop paid one memory round trip per unit)
    {
        const float *__restrict__ w1 = g.b.actor_fc1_w;
        const float *__restrict__ b1 = g.b.actor_fc1_b;
        // rows 0..4D-1: Weff[r][k] with r = idx / D, k = idx % D; then four
        // rows for beff's sums over fc1.bias (the same code with b1 for W1)
        for (int idx = lane; idx < 4 * D + 4; idx += 64) {
            const bool bias = idx >= 4 * D;
            const int r = bias ? idx - 4 * D : idx / D;
            const int k = bias ? 0 : idx - r * D;
            const float *__restrict__ head = (r < 2 ? g.b.actor_mu_w : g.b.actor_std_w) + (r & 1) * H;
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

    // ---- critic: wave q sums hidden units [j0, j1) for the block's 64 envs
    {
        const int e = lane;
        const int64_t env_raw = (int64_t)blockIdx.x * kEnvsPerBlock + e;
        const int64_t env = env_raw < P ? env_raw : P - 1;  // lanes past the end stay in bounds
        const float *__restrict__ xe = obs + env * AD;
        const float *__restrict__ wc = g.b.critic_fc1_w;
        const float *__restrict__ bc = g.b.critic_fc1_b;
        const float *__restrict__ w2 = g.b.critic_fc2_w;
        float part = 0.0f;
        if constexpr (A_T != 0 && D_T != 0) {
            float x[A_T * D_T];
            load_row<A_T * D_T>(xe, x);
            for (int j = j0; j < j1; j += 4) {
                float acc[4];
                const float *wr[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int jj = j + i < j1 ? j + i : j1 - 1;  // a short last group repeats a row
                    acc[i] = bc[jj];
                    wr[i] = wc + (int64_t)jj * (A_T * D_T);
                }
#pragma unroll
                for (int k = 0; k < A_T * D_T; ++k)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(wr[i][k], x[k], acc[i]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j + i < j1) part = __builtin_fmaf(w2[j + i], relu_t(acc[i]), part);
            }
        } else {
            for (int j = j0; j < j1; j += 4) {
                float acc[4];
                const float *wr[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int jj = j + i < j1 ? j + i : j1 - 1;
                    acc[i] = bc[jj];
                    wr[i] = wc + (int64_t)jj * AD;
                }
                for (int k = 0; k < AD; ++k) {
                    const float xv = xe[k];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(wr[i][k], xv, acc[i]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j + i < j1) part = __builtin_fmaf(w2[j + i], relu_t(acc[i]), part);
            }
        }
        s_part[q * kEnvsPerBlock + e] = part;
    }
    __syncthreads();  // the waves' partial Weff, beff and critic sums are in LDS

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
        s_b[t] = (t < 2 ? g.b.actor_mu_b : g.b.actor_std_b)[t & 1] + v;
    }
    if (t < kEnvsPerBlock) {
        const int64_t env = (int64_t)blockIdx.x * kEnvsPerBlock + t;
        if (env < P) {
            float v = s_part[t];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) v += s_part[w * kEnvsPerBlock + t];
            g.b.values[env] = v + g.b.critic_fc2_b[0];
        }
    }
    __syncthreads();  // Weff and beff are in LDS

    // ---- actor: one thread per agent row of the block's envs
    const int64_t row0 = (int64_t)blockIdx.x * kEnvsPerBlock * A;
    const int64_t rows_total = P * A;
    const int rows_block = kEnvsPerBlock * A;
    const float4 be = *reinterpret_cast<const float4 *>(s_b);
    for (int r = t; r < rows_block; r += kThreads) {
        const int64_t row = row0 + r;
        if (row >= rows_total) break;
        const float *__restrict__ xr = obs + row * D;
        float p0 = be.x, p1 = be.y, p2 = be.z, p3 = be.w;
        if constexpr (D_T != 0) {
            float x[D_T];
            load_row<D_T>(xr, x);
#pragma unroll
            for (int k = 0; k < D_T; ++k) {
                const float4 w = *reinterpret_cast<const float4 *>(s_w + 4 * k);
                p0 = __builtin_fmaf(w.x, x[k], p0);
                p1 = __builtin_fmaf(w.y, x[k], p1);
                p2 = __builtin_fmaf(w.z, x[k], p2);
                p3 = __builtin_fmaf(w.w, x[k], p3);
            }
        } else {
            for (int k = 0; k < D; ++k) {
                const float4 w = *reinterpret_cast<const float4 *>(s_w + 4 * k);
                const float xv = xr[k];
                p0 = __builtin_fmaf(w.x, xv, p0);
                p1 = __builtin_fmaf(w.y, xv, p1);
                p2 = __builtin_fmaf(w.z, xv, p2);
                p3 = __builtin_fmaf(w.w, xv, p3);
            }
        }
        const float mu0 = tanhf(p0), mu1 = tanhf(p1);
        const float v0 = softplus_t(p2), v1 = softplus_t(p3);
        float e0, e1;
        if (g.b.eps) {
            e0 = g.b.eps[2 * row];
            e1 = g.b.eps[2 * row + 1];
        } else {
            policy_normals(g.seed, (uint64_t)(g.env_offset * A + row), g.step, e0, e1);
        }
        if (g.b.eps_out) {
            g.b.eps_out[2 * row] = e0;
            g.b.eps_out[2 * row + 1] = e1;
        }
        // loc + scale_tril @ eps: the product and the sum round separately
        g.b.actions[2 * row] = mu0 + sqrtf(v0) * e0;
        g.b.actions[2 * row + 1] = mu1 + sqrtf(v1) * e1;
        const float m = __builtin_fmaf(e1, e1, e0 * e0);
        const float ld = logf(v0) + logf(v1);
        g.b.log_probs[row] = __builtin_fmaf(-0.5f, m, __builtin_fmaf(-0.5f, ld, -kLog2Pi));
    }
}

// The critic of policy_kernel alone (marlnav_critic_values):
// the same blocks of 64 envs, the same wave shares of the hidden units, the
// same FMA chains and the same wave-order sum, so values[env] carries the bits
// policy_kernel stores for the same observations and weights. It is a kernel
// of its own, not a mode of policy_kernel, and the critic sum is restated, not
// shared: a function called from both changed policy_kernel's compiled code,
// and the rollout's hot launch keeps its code. The bit
// identity is held by tests/test_gae_gpu.py. Reads no actor tensor and draws
// nothing.
template <int A_T, int D_T>
__global__ void __launch_bounds__(kThreads) critic_values_kernel(PolicyArgs g)
{
    const int AD = (A_T ? A_T : g.A) * (D_T ? D_T : g.D);
    const int H = g.H;
    const int64_t P = g.P;
    __shared__ float s_part[kWaves * kEnvsPerBlock];

    const int t = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(t >> 6);
    const int e = t & 63;
    const int Hq = (H + kWaves - 1) / kWaves;
    const int j0 = q * Hq, j1 = (j0 + Hq < H) ? j0 + Hq : H;

    const int64_t env_raw = (int64_t)blockIdx.x * kEnvsPerBlock + e;
    const int64_t env = env_raw < P ? env_raw : P - 1;  // lanes past the end stay in bounds
    const float *__restrict__ xe = g.b.obs_norm + env * AD;
    const float *__restrict__ wc = g.b.critic_fc1_w;
    const float *__restrict__ bc = g.b.critic_fc1_b;
    const float *__restrict__ w2 = g.b.critic_fc2_w;
    float part = 0.0f;
    if constexpr (A_T != 0 && D_T != 0) {
        float x[A_T * D_T];
        load_row<A_T * D_T>(xe, x);
        for (int j = j0; j < j1; j += 4) {
            float acc[4];
            const float *wr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int jj = j + i < j1 ? j + i : j1 - 1;  // a short last group repeats a row
                acc[i] = bc[jj];
                wr[i] = wc + (int64_t)jj * (A_T * D_T);
            }
#pragma unroll
            for (int k = 0; k < A_T * D_T; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(wr[i][k], x[k], acc[i]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (j + i < j1) part = __builtin_fmaf(w2[j + i], relu_t(acc[i]), part);
        }
    } else {
        for (int j = j0; j < j1; j += 4) {
            float acc[4];
            const float *wr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int jj = j + i < j1 ? j + i : j1 - 1;
                acc[i] = bc[jj];
                wr[i] = wc + (int64_t)jj * AD;
            }
            for (int k = 0; k < AD; ++k) {
                const float xv = xe[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(wr[i][k], xv, acc[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (j + i < j1) part = __builtin_fmaf(w2[j + i], relu_t(acc[i]), part);
        }
    }
    s_part[q * kEnvsPerBlock + e] = part;
    __syncthreads();
    if (t < kEnvsPerBlock && env_raw < P) {
        float v = s_part[t];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += s_part[w * kEnvsPerBlock + t];
        g.b.values[env_raw] = v + g.b.critic_fc2_b[0];
    }
}

using PolicyFn = void (*)(PolicyArgs);

struct PolicyVariant {
    int A, D;
    PolicyFn fn;
};

// compiled shapes: 3 agents x 3 and x 8 obstacles (the benchmark's)
const PolicyVariant kVariants[] = {
    {3, 12, policy_kernel<3, 12>},
    {3, 22, policy_kernel<3, 22>},
};
const PolicyVariant kCriticVariants[] = {
    {3, 12, critic_values_kernel<3, 12>},
    {3, 22, critic_values_kernel<3, 22>},
};

int failf(int code, const char *fmt, long long a, long long b, long long c)
{
    char msg[256];
    snprintf(msg, sizeof(msg), fmt, a, b, c);
    return marlnav_internal_fail(code, msg);
}

// the dims checks of both entry points; 0 or the failing code
int check_dims(const MarlnavPolicyDims *d, const MarlnavPolicyBuffers *b)
{
    if (!d || !b) return marlnav_internal_fail(MARLNAV_EINVAL, "policy dims/buffers is NULL");
    if (d->num_parallel < 1)
        return failf(MARLNAV_EINVAL, "policy: num_parallel=%lld < 1", d->num_parallel, 0, 0);
    if (d->num_agents < 2 || d->num_agents > kMaxAgentsP)
        return failf(MARLNAV_EINVAL, "policy: num_agents=%lld outside [2, %lld]", d->num_agents,
                     kMaxAgentsP, 0);
    if (d->hidden_size < 1 || d->hidden_size > kMaxHidden)
        return failf(MARLNAV_EINVAL, "policy: hidden_size=%lld outside [1, %lld]", d->hidden_size,
                     kMaxHidden, 0);
    {
        // D = 2 + 2 O + 2 (A - 1) for an observed obstacle count O in [1, 256]
        const int twoO = d->obs_dim - 2 * d->num_agents;
        if (twoO < 2 || (twoO & 1) || twoO > 2 * kMaxObstP)
            return failf(MARLNAV_EINVAL,
                         "policy: obs_dim=%lld is not 2 + 2*O + 2*(A-1) for num_agents=%lld and "
                         "an O in [1, %lld]",
                         d->obs_dim, d->num_agents, kMaxObstP);
    }
    if (d->reserved != 0 || d->env_offset < 0)
        return failf(MARLNAV_EINVAL, "policy: reserved=%lld must be 0 and env_offset=%lld >= 0",
                     d->reserved, d->env_offset, 0);
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
    const int64_t nblk = (d->num_parallel + kEnvsPerBlock - 1) / kEnvsPerBlock;
    if (nblk > 0x7fffffff)
        return failf(MARLNAV_EINVAL, "policy: num_parallel=%lld too large", d->num_parallel, 0, 0);

    PolicyArgs args;
    args.b = *b;
    args.P = d->num_parallel;
    args.env_offset = d->env_offset;
    args.A = d->num_agents;
    args.D = d->obs_dim;
    args.H = d->hidden_size;
    args.seed = native_seed_mix(policy_seed);
    args.step = step_idx;
    PolicyFn fn = policy_kernel<0, 0>;
    // the compiled shapes load rows as 16- / 8-byte vectors
    if ((reinterpret_cast<uintptr_t>(b->obs_norm) & 15u) == 0)
        for (const PolicyVariant &v : kVariants)
            if (v.A == args.A && v.D == args.D) fn = v.fn;
    const size_t lds = sizeof(float) * lds_floats(args.D);
    hipLaunchKernelGGL(fn, dim3((unsigned)nblk), dim3(kThreads), lds, (hipStream_t)stream, args);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return marlnav_internal_fail(MARLNAV_ELAUNCH, hipGetErrorString(e));
    return 0;
}

extern "C" int marlnav_critic_values(const MarlnavPolicyDims *d, const MarlnavPolicyBuffers *b,
                                     void *stream)
{
    if (int rc = check_dims(d, b)) return rc;
    if (!b->obs_norm || !b->critic_fc1_w || !b->critic_fc1_b || !b->critic_fc2_w ||
        !b->critic_fc2_b || !b->values)
        return marlnav_internal_fail(
            MARLNAV_EINVAL, "critic values: a required buffer (obs_norm, critic_*, values) is NULL");
    const int64_t nblk = (d->num_parallel + kEnvsPerBlock - 1) / kEnvsPerBlock;
    if (nblk > 0x7fffffff)
        return failf(MARLNAV_EINVAL, "policy: num_parallel=%lld too large", d->num_parallel, 0, 0);

    PolicyArgs args;
    args.b = *b;
    args.P = d->num_parallel;
    args.env_offset = d->env_offset;
    args.A = d->num_agents;
    args.D = d->obs_dim;
    args.H = d->hidden_size;
    args.seed = 0;
    args.step = 0;
    PolicyFn fn = critic_values_kernel<0, 0>;
    if ((reinterpret_cast<uintptr_t>(b->obs_norm) & 15u) == 0)
        for (const PolicyVariant &v : kCriticVariants)
            if (v.A == args.A && v.D == args.D) fn = v.fn;
    hipLaunchKernelGGL(fn, dim3((unsigned)nblk), dim3(kThreads), 0, (hipStream_t)stream, args);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return marlnav_internal_fail(MARLNAV_ELAUNCH, hipGetErrorString(e));
    return 0;
}
