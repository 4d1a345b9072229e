// policy_forward.h - the one definition of the policy's forward pass: the
// actor collapse, an agent row's FMA chains, the
// sampling tail and the critic's grouped hidden-unit sum. policy_kernel and
// critic_values_kernel (marlnav_policy.hip) are sequences of these calls
// around their own thread-to-row mappings and barriers; actor_kernel
// (marlnav_eval.hip) calls all but the collapse, which it has written out for
// a measured reason.
// marlnav_ppo.hip takes the limits, the block shape and relu_t; its forward
// pass keeps the hidden activations and stays its own. Included inside each
// translation unit's anonymous namespace, as device_rng.h is.
//
// Built with -ffp-contract=off: every FMA below is explicit.
#pragma once

#include "device_rng.h"
#include "policy_limits.h"

constexpr int kThreads = 256;  // the block of the policy, actor and PPO kernels
constexpr int kWaves = kThreads / 64;

constexpr uint32_t kPolicyBlock = 0x80000000u;           // Philox block-index domain
constexpr float kLog2Pi = 1.8378770664093453f;

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

// wave q's share [j0, j1) of the H hidden units, in the collapse and in the critic
__device__ __forceinline__ void wave_share(int H, int q, int &j0, int &j1)
{
    const int Hq = (H + kWaves - 1) / kWaves;
    j0 = q * Hq;
    j1 = (j0 + Hq < H) ? j0 + Hq : H;
}

// ---------------------------------------------------------------- collapse
// fc1 has no activation, so the actor's two layers are one affine map:
// Weff = [Wmu; Wstd] W1 (4 x D), beff = [Wmu; Wstd] b1 + [bmu; bstd]. A block
// recomputes it from the live weight tensors into LDS.

// The collapse's part of a block's dynamic LDS, from its 16-byte aligned
// base: Weff as [k][4], the kWaves waves' partial Weff (4 D each), beff, its
// partials. The functions below take the base and derive these pointers
// themselves: handed over ready-made (a struct of them, or one by one) every
// kernel compiled to another, slower prologue.
__device__ __forceinline__ float *lds_wp(float *lds, int D) { return lds + 4 * D; }
__device__ __forceinline__ float *lds_b(float *lds, int D) { return lds_wp(lds, D) + kWaves * 4 * D; }
__device__ __forceinline__ float *lds_bp(float *lds, int D) { return lds_b(lds, D) + 4; }
constexpr size_t collapse_lds_floats(int D) { return (size_t)(1 + kWaves) * 4 * D + 4 + 4 * kWaves; }

// Wave q's partial rows: Weff[r][k] = sum_j head_r[j] W1[j][k] over its hidden
// units [j0, j1), the loads of a group of 8 issued before the first FMA (a
// rolled loop paid one memory round trip per unit). The caller's
// __syncthreads() stands between this and collapse_sum. D_T: compiled row
// length (0: D_run), as in row_chains.
template <int D_T>
__device__ __forceinline__ void collapse_partials(const float *__restrict__ w1,
                                                  const float *__restrict__ b1, const float *mu_w,
                                                  const float *std_w, int D_run, int H, int q,
                                                  int lane, int j0, int j1, float *lds)
{
    const int D = D_T ? D_T : D_run;
    float *s_wp = lds_wp(lds, D), *s_bp = lds_bp(lds, D);
    // rows 0..4D-1: Weff[r][k] with r = idx / D, k = idx % D; then four
    // rows for beff's sums over fc1.bias (the same code with b1 for W1)
    for (int idx = lane; idx < 4 * D + 4; idx += 64) {
        const bool bias = idx >= 4 * D;
        const int r = bias ? idx - 4 * D : idx / D;
        const int k = bias ? 0 : idx - r * D;
        const float *__restrict__ head = (r < 2 ? mu_w : std_w) + (r & 1) * H;
        const float *__restrict__ col = bias ? b1 : w1 + k;
        const int64_t stride = bias ? 1 : D;
        float acc = 0.0f;
        for (int j = j0; j < j1; j += 8) {
            float u[8], v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int jj = j + i < j1 ? j + i : j1 - 1;  // a short last group repeats a unit
                u[i] = head[jj];
                v[i] = col[jj * stride];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (j + i < j1) acc = __builtin_fmaf(u[i], v[i], acc);
        }
        if (bias)
            s_bp[4 * q + r] = acc;
        else
            s_wp[q * 4 * D + 4 * k + r] = acc;
    }
}

// the partial sums, added in wave order, and the head biases; thread t of the block
__device__ __forceinline__ void collapse_sum(const float *mu_b, const float *std_b, int D, int t,
                                             float *lds)
{
    float *s_wp = lds_wp(lds, D), *s_bp = lds_bp(lds, D);
    for (int idx = t; idx < 4 * D; idx += kThreads) {
        float v = s_wp[idx];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += s_wp[w * 4 * D + idx];
        lds[idx] = v;
    }
    if (t < 4) {
        float v = s_bp[t];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += s_bp[4 * w + t];
        lds_b(lds, D)[t] = (t < 2 ? mu_b : std_b)[t & 1] + v;
    }
}

// --------------------------------------------------------------- agent row
// The FMA chains of the agent row at xr against the collapsed weights (LDS,
// one broadcast 16-byte read per feature): from be = beff, k ascending. x, y:
// the mean chains; z, w: the covariance chains, formed only with COV (else
// beff's). D_T: compiled row length (0: run-time D, inputs read from memory
// as used).
template <int D_T, bool COV>
__device__ __forceinline__ float4 row_chains(const float *__restrict__ xr, int D, float4 be,
                                             const float *s_w)
{
    float4 p = be;
    if constexpr (D_T != 0) {
        float x[D_T];
        load_row<D_T>(xr, x);
#pragma unroll
        for (int k = 0; k < D_T; ++k) {
            const float4 w = *reinterpret_cast<const float4 *>(s_w + 4 * k);
            p.x = __builtin_fmaf(w.x, x[k], p.x);
            p.y = __builtin_fmaf(w.y, x[k], p.y);
            if constexpr (COV) {
                p.z = __builtin_fmaf(w.z, x[k], p.z);
                p.w = __builtin_fmaf(w.w, x[k], p.w);
            }
        }
    } else {
        for (int k = 0; k < D; ++k) {
            const float4 w = *reinterpret_cast<const float4 *>(s_w + 4 * k);
            const float xv = xr[k];
            p.x = __builtin_fmaf(w.x, xv, p.x);
            p.y = __builtin_fmaf(w.y, xv, p.y);
            if constexpr (COV) {
                p.z = __builtin_fmaf(w.z, xv, p.z);
                p.w = __builtin_fmaf(w.w, xv, p.w);
            }
        }
    }
    return p;
}

// The sampling tail of agent row `row` (global id gid): eps given or drawn,
// eps_out when asked for, and loc + scale_tril @ eps with the product and the
// sum rounded separately. e0, e1: the normals used.
__device__ __forceinline__ void sample_action(const float *eps, float *eps_out, float *actions,
                                              float mu0, float mu1, float v0, float v1,
                                              int64_t row, uint64_t seed, uint64_t gid,
                                              uint64_t step, float &e0, float &e1)
{
    if (eps) {
        e0 = eps[2 * row];
        e1 = eps[2 * row + 1];
    } else {
        policy_normals(seed, gid, step, e0, e1);
    }
    if (eps_out) {
        eps_out[2 * row] = e0;
        eps_out[2 * row + 1] = e1;
    }
    actions[2 * row] = mu0 + sqrtf(v0) * e0;
    actions[2 * row + 1] = mu1 + sqrtf(v1) * e1;
}

// ------------------------------------------------------------------ critic
// One wave's partial of value = W2 relu(Wc x + bc) + b2 for the env whose A D
// inputs start at xe: the hidden units [j0, j1) in groups of four. The weight
// indices are wave-uniform, so the weights arrive through the scalar cache as
// SGPR operands of the FMAs. AD_T: compiled A D, the inputs held in VGPRs
// (0: run-time AD, re-read per group).
template <int AD_T>
__device__ __forceinline__ float critic_partial(const float *__restrict__ xe,
                                                const float *__restrict__ wc,
                                                const float *__restrict__ bc,
                                                const float *__restrict__ w2, int AD, int j0,
                                                int j1)
{
    float part = 0.0f;
    if constexpr (AD_T != 0) {
        float x[AD_T];
        load_row<AD_T>(xe, x);
        for (int j = j0; j < j1; j += 4) {
            float acc[4];
            const float *wr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int jj = j + i < j1 ? j + i : j1 - 1;  // a short last group repeats a row
                acc[i] = bc[jj];
                wr[i] = wc + (int64_t)jj * AD_T;
            }
#pragma unroll
            for (int k = 0; k < AD_T; ++k)
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
    return part;
}

// the value of a block's env e: the waves' partials (s_part[w * n + e], n envs
// per block) added in wave order, plus fc2.bias
__device__ __forceinline__ float critic_total(const float *s_part, int n, int e,
                                              const float *fc2_b)
{
    float v = s_part[e];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += s_part[w * n + e];
    return v + fc2_b[0];
}
