// marlnav_ppo.hip - gfx950 kernels for the update half of the training loop:
// MAPPO._actor_loss / _critic_loss (marlnav/models.py:270-316) of one
// minibatch together with the gradient of every parameter, i.e. what
// zero_grad() + loss.backward() leave in .grad (models.py:173-175, 193-195).
// No autograd graph, no MultivariateNormal (a batched Cholesky per row in the
// reference): the backward passes have closed forms.
//
// Shapes: T steps of P envs, N = T P env rows, M = N A agent rows in the
// rollout buffer's (t, p, a) order, D features per agent row, H hidden units.
//
// Actor. fc1 has no activation, so pre = Weff x + beff with Weff = [Wmu;
// Wstd] W1 (4 x D), as in marlnav_policy.hip. With g_i (4 values) the
// gradient of the loss with respect to pre of row i, every parameter gradient
// follows from S = sum_i g_i (x) [x_i, 1] = [S_x | s_1] (4 x (D + 1)):
//   d[Wmu; Wstd] = S_x W1^T + s_1 b1^T    d[bmu; bstd] = s_1
//   dW1 = [Wmu; Wstd]^T S_x               db1 = [Wmu; Wstd]^T s_1
// actor_pass: a block owns a contiguous range of rows and walks it in tiles
// of 256. Per tile, thread = row computes pre (4 D fp64 FMAs against Weff in
// LDS, rounded to fp32), the loss terms and g (fp32, to LDS); then thread =
// (column c of [x, 1], row slice) adds g_r x_rc over its rows of the tile into
// four fp64 accumulators (the products of two fp32 are exact in fp64). Block
// partials of S and of the two loss sums go to the workspace; actor_finish
// (one block) adds them in block order and runs the epilogue above in fp64.
//
// Critic. h = relu(Wc x + bc), nv = w2 h + b2, delta_n = dloss/dnv_n;
//   dWc = sum_n dh_n (x) x_n,  dh_nj = delta_n w2_j [h_nj > 0]   (H x A D)
//   dbc = sum_n dh_n    dW2 = sum_n delta_n h_n    db2 = sum_n delta_n
// critic_pass: grid = (row chunks, output tiles). A block walks its chunk in
// tiles of 64 rows. Forward as in marlnav_policy.hip (lane = row, wave q sums
// a quarter of the hidden units, weights through the scalar cache, fp32 FMA
// chains of 64 inputs added up in fp64); h of the
// block's own hidden units is kept in LDS, turned into dh once delta is
// known, and thread = (column k, unit slice) adds dh_rj x_rk over the tile's
// rows into JT fp64 accumulators (the ReLU prevents a collapse). Where the
// output needs several tiles the forward pass runs once, in a launch of its
// own on a finer row grid, and hands dh to the tiles' blocks through the
// workspace instead of being recomputed per tile. critic_finish adds the
// chunk partials per output element in chunk order.
//
// The kernels take a trailing argument pack. Empty, they are the kernels of
// marlnav_ppo_*_grad. With AdvArgs a pass kernel's last act is one thread
// advancing Adam's step count; with FoldArgs a finish kernel applies the Adam
// element update to every gradient element it has stored (the training
// phase call of marlnav_adam.hip). With DiagArgs the actor's two
// kernels also form the update's diagnostics and decide the target-KL stop
// (marlnav_ppo_actor_grad_diag, marlnav_ppo_train_phase_monitored, §17).
//
// Determinism: no atomics, every sum in a fixed order that depends on the
// dims only. Built with -ffp-contract=off: every FMA below is explicit.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/marlnav.h"
#include "adam_element.h"
#include "host_util.h"
#include "ppo_update.h"

namespace {

// the block shape, the policy's limits, kLog2Pi and relu_t; block_sum
#include "policy_forward.h"
#include "block_sum.h"

// ---- actor tiling
constexpr int kActorTile = kThreads;       // rows per tile
constexpr int kActorColsPerThread = 3;     // ceil((kMaxD + 1) / kThreads)
constexpr int64_t kActorMaxBlocks = 1024;
constexpr int64_t kActorMinRows = 1024;    // rows of a block, at least
static_assert(kActorColsPerThread * kThreads >= kMaxD + 1, "columns of the widest row");

// ---- critic tiling
constexpr int kCriticTile = 64;            // rows per tile (lane = row)
constexpr int kFwdChain = 64;              // inputs per fp32 FMA chain of the forward pass
constexpr int64_t kCriticTargetBlocks = 512;
constexpr int64_t kCriticMaxWork = 8 << 20;  // fp64 elements of chunk partials (64 MiB)
constexpr int64_t kCriticForwardBlocks = 1024;

struct PpoArgs {
    MarlnavPpoBuffers b;
    int64_t P, T, N, M;
    int A, D, H;
    int64_t rows_per_block;  // actor: rows of a block; critic: rows of a chunk
    int64_t nblocks;         // actor: blocks; critic: chunks
    // critic, forward pass shared through the workspace (else fw_part NULL):
    // rows and count of the kForward blocks, their unit-vector partials
    int64_t fw_rows, fw_blocks;
    double *fw_part;         // [fw_blocks][2 H + 2]: dbc, dW2, db2, loss sum
    float clip_lo, clip_hi, eps_f, ent_f;
};

// ---- the step gather (marlnav_ppo_*_grad_steps). A pass
// kernel instantiated with GatherArgs reads logical step slot s of the
// minibatch from physical step steps[s] of the storage, whose step 0 the data
// pointers address. Only the addresses of obs, actions, log_probs, values and
// returns change: the grid, the tiles, the workspace and every reduction order
// stay functions of the logical row, so the stored bits are those of the
// contiguous call on a storage gathered with index_select(0, steps). The
// instantiations with PpoArgs are the kernels as they were.
struct GatherArgs : PpoArgs {
    const int32_t *steps;  // [T], every entry a stored step (not checked here)
};

template <class ARGS>
struct is_gather {
    static constexpr bool value = false;
};
template <>
struct is_gather<GatherArgs> {
    static constexpr bool value = true;
};

// The physical rows of one tile. R rows make a step (P A agent rows, or P env
// rows); the tile starts at logical row `base` = slot0 R + off0, found with
// the one wave-uniform division the contiguous kernels already pay per tile.
// at(dlt), 0 <= dlt < TILE, is the physical row of logical row base + dlt.
// R >= TILE: the tile meets at most one step boundary, so the two table
// entries it can need are wave-uniform loads and a row costs an add, a compare
// and a select. R < TILE: the tile spans several steps; off0 + dlt < 2 TILE
// divides in 32 bits and the entry is a per-lane load from a table of a few
// cache lines. No row divides in 64 bits.
template <int TILE>
struct StepWalk {
    const int32_t *steps;
    int64_t R, slot0, off0;
    int64_t p0, p1;  // first physical row of the steps of slot0 and of slot0 + 1

    __device__ __forceinline__ void start(const int32_t *__restrict__ st, int64_t T, int64_t R_,
                                          int64_t base)
    {
        steps = st;
        R = R_;
        slot0 = base / R;
        off0 = base - slot0 * R;
        p0 = (int64_t)st[slot0] * R;
        p1 = (int64_t)st[slot0 + 1 < T ? slot0 + 1 : slot0] * R;
    }
    // R >= TILE: rows [0, run0()) of the tile are consecutive from physical row
    // first0(), the rest consecutive from first1() + dlt: a row loop split there
    // keeps the contiguous kernel's constant stride in each half
    __device__ __forceinline__ int64_t run0() const { return R - off0; }
    __device__ __forceinline__ int64_t first0() const { return p0 + off0; }
    __device__ __forceinline__ int64_t first1() const { return p1 + off0 - R; }
    __device__ __forceinline__ int64_t at(int dlt) const
    {
        if (R >= TILE) {
            const int64_t off = off0 + dlt;
            return off < R ? p0 + off : p1 + (off - R);
        }
        const uint32_t r = (uint32_t)R, o = (uint32_t)off0 + (uint32_t)dlt;
        const uint32_t q = o / r;
        return (int64_t)steps[slot0 + q] * R + (o - q * r);
    }
};

// ---- the Adam step folded into the finish kernels (marlnav_ppo_train_phase,
// DESIGN.md §14). AdvArgs: what one thread of the pass launch needs to advance
// the count and publish the step's scalars. FoldArgs: what the finish launch,
// which follows in stream order, needs to update every element it has just
// written to .grad. Slots in the network's declaration order (the actor's six,
// the critic's four).
using marlnav_adam::AdamScalars;
using marlnav_adam::AdamState;

struct AdvArgs {
    AdamState *state;
    double lr, beta1, beta2;
};

struct FoldArgs {
    float *param[6];
    float *exp_avg[6];
    float *exp_avg_sq[6];
    const AdamState *state;
    double beta1, beta2, omb1, omb2, eps;  // omb = 1 - beta
    int maximize;
};

__device__ __forceinline__ AdamScalars fold_scalars(const FoldArgs &f)
{
    AdamScalars c;
    c.beta1 = f.beta1;
    c.beta2 = f.beta2;
    c.omb1 = f.omb1;
    c.omb2 = f.omb2;
    c.eps = f.eps;
    c.step_size = f.state->step_size;
    c.bc2_sqrt = f.state->bc2_sqrt;
    c.maximize = f.maximize != 0;
    return c;
}

// element e of one slot, from the fp32 gradient this thread has stored
__device__ __forceinline__ void fold_element(const FoldArgs &f, int slot, int64_t e, float grad,
                                             const AdamScalars &c)
{
    float p = f.param[slot][e], m = f.exp_avg[slot][e], v = f.exp_avg_sq[slot][e];
    marlnav_adam::adam_element(p, grad, m, v, c);
    f.exp_avg[slot][e] = m;
    f.exp_avg_sq[slot][e] = v;
    f.param[slot][e] = p;
}

// The clipped update folded into actor_finish: FoldArgs plus
// the clip's own arguments. actor_pass takes the same AdvArgs as for FoldArgs.
struct ClipFoldArgs {
    FoldArgs f;
    double max_norm;
    double *norm_out;  // the norm before clipping, or NULL
};

// element e of one slot with the clip: the gradient scaled, stored back into
// .grad and the element updated from the stored value (adam_apply<true>)
__device__ __forceinline__ void clip_fold_element(const FoldArgs &f, int slot, int64_t e,
                                                  float *grad, double coef, const AdamScalars &c)
{
    const float gc = marlnav_adam::clipped_grad(grad[e], coef);
    grad[e] = gc;
    fold_element(f, slot, e, gc, c);
}

// The kernels below take the fold's arguments as a trailing pack: empty for
// the launches of marlnav_ppo_*_grad / _update, whose instantiations are the
// kernels as they were; one AdvArgs / FoldArgs for the folded ones.
template <class T>
__device__ __forceinline__ const T &only(const T &x)
{
    return x;
}

template <class... X>
struct is_clip_fold {
    static constexpr bool value = false;
};
template <>
struct is_clip_fold<ClipFoldArgs> {
    static constexpr bool value = true;
};
// 16 blocks of 256 items: far above what the 1024-element fold limit needs (2)
constexpr int kClipFoldMaxBlocks = 16;

// The diagnostic variant: actor_pass adds the k3 KL terms and
// the count of rows whose ratio left the clip range to its partial row (two
// more fp64 sums), actor_finish writes the update's row of five doubles
// [surrogate mean, entropy mean, approximate KL, clip fraction, status] and,
// where `stop` is given, decides the stop. stop[0] is the flag, stop[1] the
// update that raised it. Datum by datum: the flag is written by thread 0 of
// the first update's pass launch (the reset, which no thread of that update
// reads: `first`) and by thread 0 of a finish launch behind that block's
// barriers; it is read at the top of every later launch of the phase, the
// finish block's own reads ahead of its first barrier. Stream order covers
// the rest: no atomics, no host read.
struct DiagArgs {
    double *diag;      // the update's row of kDiagRow doubles
    int64_t *stop;     // {flag, stopped_at}, or NULL: no stop (status 0)
    double target_kl;  // +inf: monitor only
    int64_t k;         // the update's index in its phase call
    int first;         // the phase's first update: resets stop, reads no flag
};
constexpr int kDiagSums = 2;  // KL sum, outside count: columns behind the loss sums
constexpr int kDiagRow = 5;
constexpr int kDiagGroups = kThreads / kDiagSums;

template <class... X>
struct is_diag {
    static constexpr bool value = false;
};
template <>
struct is_diag<DiagArgs> {
    static constexpr bool value = true;
};

// p[0] + p[stride] + ... (n terms) in that order, the loads of eight terms
// issued before their adds (a rolled loop pays one memory round trip per term)
__device__ __forceinline__ double sum_strided(const double *__restrict__ p, int64_t n,
                                              int64_t stride)
{
    double a = 0.0;
    int64_t c = 0;
    for (; c + 8 <= n; c += 8) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[(c + i) * stride];
#pragma unroll
        for (int i = 0; i < 8; ++i) a += v[i];
    }
    for (; c < n; ++c) a += p[c * stride];
    return a;
}

// =========================================================================
// actor
// =========================================================================
// LDS: Weff [D][4] and beff [4] in fp64, g [256][4] in fp32, kWaves doubles
// of the block sums
constexpr size_t actor_lds_bytes(int D)
{
    return sizeof(double) * ((size_t)4 * D + 4) + sizeof(float) * 4 * kActorTile +
           sizeof(double) * kWaves;
}
static_assert(actor_lds_bytes(kMaxD) <= 64 * 1024, "LDS of the widest row");

// workspace of the actor: per block 4 (D + 1) sums of S ([r][c], c == D the
// ones column), then the surrogate sum and the entropy sum
__device__ __host__ inline int64_t actor_stride(int D) { return 4 * (int64_t)(D + 1) + 2; }

//
// PAIRING: which entry of the (t, p) vectors is the advantage of agent row i.
// kPairReference: returns[i mod N] - values[i mod N], the reference's
// repeat(num_agents). kPairEnv: returns[i / A], the row's own
// env, read as a ready fp64 advantage; values is not read.
enum { kPairReference = 0, kPairEnv = 1 };

template <int PAIRING, class ARGS, class... X>
__global__ void __launch_bounds__(kThreads) actor_pass(ARGS g, X... x)
{
    constexpr bool kDiag = is_diag<X...>::value;
    constexpr bool kGather = is_gather<ARGS>::value;
    if constexpr (kDiag) {
        // an update behind the stop costs its launches only (uniform per grid)
        const DiagArgs &dg = only(x...);
        if (dg.stop && !dg.first && dg.stop[0] != 0) return;
    }
    const int D = g.D, H = g.H;
    const int ncol = D + 1;
    extern __shared__ __attribute__((aligned(16))) double s_dyn_d[];
    double *s_w = s_dyn_d;              // Weff as [k][4]
    double *s_b = s_w + 4 * D;          // beff
    float *s_g = reinterpret_cast<float *>(s_b + 4);  // g of the tile's rows, [r][4]
    double *s_red = reinterpret_cast<double *>(s_g + 4 * kActorTile);

    const int t = threadIdx.x;
    // ---- collapse: Weff[r][k] = sum_j head_r[j] W1[j][k], beff likewise. In
    // fp64 (products of two fp32 are exact there), as is pre below: the new
    // log-prob is subtracted from the stored one, so the rounding of pre is
    // what the ratio's error is made of, and a row of 4 D FMAs is cheap
    // beside its tanh / exp / log
    for (int idx = t; idx < 4 * D + 4; idx += kThreads) {
        const bool bias = idx >= 4 * D;
        const int r = bias ? idx - 4 * D : idx / D;
        const int k = bias ? 0 : idx - r * D;
        const float *__restrict__ head = (r < 2 ? g.b.actor_mu_w : g.b.actor_std_w) + (r & 1) * H;
        const float *__restrict__ col = bias ? g.b.actor_fc1_b : g.b.actor_fc1_w + k;
        const int64_t stride = bias ? 1 : D;
        double acc = 0.0;
        for (int j = 0; j < H; j += 8) {  // the loads of a group before its FMAs
            float a[8], b[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int jj = j + i < H ? j + i : H - 1;
                a[i] = head[jj];
                b[i] = col[jj * stride];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (j + i < H) acc = __builtin_fma((double)a[i], (double)b[i], acc);
        }
        if (bias)
            s_b[r] = (double)(r < 2 ? g.b.actor_mu_b : g.b.actor_std_b)[r & 1] + acc;
        else
            s_w[4 * k + r] = acc;
    }
    __syncthreads();

    // phase-2 ownership: column(s) of [x, 1] and a slice of the tile's rows
    const int slices = ncol >= kThreads ? 1 : kThreads / ncol;
    const int us = ncol >= kThreads ? 0 : t / ncol;
    const int kk = ncol >= kThreads ? t : t - us * ncol;
    const bool own = us < slices;
    double acc[kActorColsPerThread][4];
#pragma unroll
    for (int i = 0; i < kActorColsPerThread; ++i)
        acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0;
    double sum_surr = 0.0, sum_ent = 0.0;
    double sum_kl = 0.0, sum_out = 0.0;  // kDiag only

    const int64_t M = g.M, N = g.N;
    const double inv_m = 1.0 / (double)M;
    const float ent_g = g.ent_f * 0.5f / (float)M;
    const int64_t row_lo = (int64_t)blockIdx.x * g.rows_per_block;
    const int64_t row_hi = row_lo + g.rows_per_block < M ? row_lo + g.rows_per_block : M;
    const double be0 = s_b[0], be1 = s_b[1], be2 = s_b[2], be3 = s_b[3];
    // GATHER: the tile's agent rows (wk), the env rows its advantages pair with
    // (wn) and, for the reference pairing's wrap past N, those from env row 0 (wz)
    StepWalk<kActorTile> wk, wn, wz;
    if constexpr (kGather && PAIRING == kPairReference) wz.start(g.steps, g.T, g.P, 0);

    for (int64_t tile = row_lo; tile < row_hi; tile += kActorTile) {
        // ---- phase 1: thread = row
        const int64_t row = tile + t;
        // wave-uniform: one scalar division per tile
        const int64_t tile_n = PAIRING == kPairEnv ? tile / g.A : tile % N;
        const int tile_a = PAIRING == kPairEnv ? (int)(tile - tile_n * g.A) : 0;
        if constexpr (kGather) {
            wk.start(g.steps, g.T, g.P * g.A, tile);
            wn.start(g.steps, g.T, g.P, tile_n);
        }
        float4 gr4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row < row_hi) {
            int64_t prow = row;  // the row in the storage
            if constexpr (kGather) prow = wk.at(t);
            const float *__restrict__ xr = g.b.obs + prow * D;
            double a0 = be0, a1 = be1, a2 = be2, a3 = be3;
            for (int k = 0; k < D; ++k) {
                const double2 wa = *reinterpret_cast<const double2 *>(s_w + 4 * k);
                const double2 wb = *reinterpret_cast<const double2 *>(s_w + 4 * k + 2);
                const double xv = (double)xr[k];
                a0 = __builtin_fma(wa.x, xv, a0);
                a1 = __builtin_fma(wa.y, xv, a1);
                a2 = __builtin_fma(wb.x, xv, a2);
                a3 = __builtin_fma(wb.y, xv, a3);
            }
            const float p0 = (float)a0, p1 = (float)a1, p2 = (float)a2, p3 = (float)a3;
            const float mu0 = tanhf(p0), mu1 = tanhf(p1);
            const float v0 = p2 > 20.0f ? p2 : log1pf(expf(p2));
            const float v1 = p3 > 20.0f ? p3 : log1pf(expf(p3));
            const float d0 = g.b.actions[2 * prow] - mu0, d1 = g.b.actions[2 * prow + 1] - mu1;
            const float iv0 = 1.0f / v0, iv1 = 1.0f / v1;
            const float q0 = d0 * d0 * iv0, q1 = d1 * d1 * iv1;
            const float ld = logf(v0) + logf(v1);
            const float lp = __builtin_fmaf(-0.5f, q0 + q1, __builtin_fmaf(-0.5f, ld, -kLog2Pi));
            const float ent = __builtin_fmaf(0.5f, ld, 1.0f + kLog2Pi);
            const float lr = lp - g.b.log_probs[prow];
            const float ratio = expf(lr);
            double adv;
            if constexpr (PAIRING == kPairEnv) {
                // row / A: the row's own env row, tile = tile_n A + tile_a
                if constexpr (kGather)
                    adv = g.b.returns[wn.at((tile_a + t) / g.A)];
                else
                    adv = g.b.returns[tile_n + (tile_a + t) / g.A];
            } else {
                // row mod N: the reference's repeat(num_agents), not the row's env
                int64_t n = tile_n + t;
                const bool wrapped = n >= N;
                if (wrapped) n = N >= kActorTile ? n - N : n % N;
                // GATHER: a wrapped n lies below kActorTile, counted from env row 0
                if constexpr (kGather) n = wrapped ? wz.at((int)n) : wn.at(t);
                adv = g.b.returns[n] - (double)g.b.values[n];
            }
            const float rc = ratio < g.clip_lo ? g.clip_lo : (ratio > g.clip_hi ? g.clip_hi : ratio);
            const double sa = (double)ratio * adv, sb = (double)rc * adv;
            sum_surr += sb < sa ? sb : sa;
            sum_ent += (double)ent;
            const bool inside = ratio >= g.clip_lo && ratio <= g.clip_hi;
            if constexpr (kDiag) {
                // k3, (r - 1) - log r, in fp64 from the fp32 ratio and log
                // ratio: in fp32 the subtraction cancels to nothing
                sum_kl += ((double)ratio - 1.0) - (double)lr;
                sum_out += inside ? 0.0 : 1.0;
            }
            const float g_ratio = (inside || sa < sb) ? (float)(adv * inv_m) : 0.0f;
            const float g_lp = g_ratio * ratio;
            const float g_mu0 = g_lp * (d0 * iv0), g_mu1 = g_lp * (d1 * iv1);
            const float g_v0 = __builtin_fmaf(g_lp, 0.5f * iv0 * (q0 - 1.0f), ent_g * iv0);
            const float g_v1 = __builtin_fmaf(g_lp, 0.5f * iv1 * (q1 - 1.0f), ent_g * iv1);
            const float sg0 = p2 > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-p2));
            const float sg1 = p3 > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-p3));
            gr4.x = g_mu0 * __builtin_fmaf(-mu0, mu0, 1.0f);
            gr4.y = g_mu1 * __builtin_fmaf(-mu1, mu1, 1.0f);
            gr4.z = g_v0 * sg0;
            gr4.w = g_v1 * sg1;
        }
        *reinterpret_cast<float4 *>(s_g + 4 * t) = gr4;  // rows past the end add zeros
        __syncthreads();

        // ---- phase 2: thread = (column, row slice); rows past the end hold g = 0
        if (own) {
            const int64_t left = row_hi - tile;
            const int nrows = left < kActorTile ? (int)left : kActorTile;
            if constexpr (kGather) {
                // row r of the tile at physical row `first` + r
                auto add_row = [&](int r, int64_t first) {
                    const float4 gv = *reinterpret_cast<const float4 *>(s_g + 4 * r);
                    const float *__restrict__ xr = g.b.obs + (first + r) * D;
    #pragma unroll
                    for (int i = 0; i < kActorColsPerThread; ++i) {
                        const int c = kk + i * kThreads;
                        if (c < ncol) {
                            const double xv = c < D ? (double)xr[c] : 1.0;
                            acc[i][0] = __builtin_fma((double)gv.x, xv, acc[i][0]);
                            acc[i][1] = __builtin_fma((double)gv.y, xv, acc[i][1]);
                            acc[i][2] = __builtin_fma((double)gv.z, xv, acc[i][2]);
                            acc[i][3] = __builtin_fma((double)gv.w, xv, acc[i][3]);
                        }
                    }
                };
                // the thread's rows in the same order, in two constant-stride
                // runs where the tile meets at most one step boundary
                int r = us;
                if (wk.R >= kActorTile) {
                    const int64_t run0 = wk.run0();
                    const int n0 = run0 < nrows ? (int)run0 : nrows;
                    const int64_t f0 = wk.first0(), f1 = wk.first1();
                    for (; r < n0; r += slices) add_row(r, f0);
                    for (; r < nrows; r += slices) add_row(r, f1);
                } else {
                    for (; r < nrows; r += slices) add_row(r, wk.at(r) - r);
                }
            } else {
                for (int r = us; r < nrows; r += slices) {
                    const float4 gv = *reinterpret_cast<const float4 *>(s_g + 4 * r);
                    const float *__restrict__ xr = g.b.obs + (tile + r) * D;
#pragma unroll
                    for (int i = 0; i < kActorColsPerThread; ++i) {
                        const int c = kk + i * kThreads;
                        if (c < ncol) {
                            const double xv = c < D ? (double)xr[c] : 1.0;
                            acc[i][0] = __builtin_fma((double)gv.x, xv, acc[i][0]);
                            acc[i][1] = __builtin_fma((double)gv.y, xv, acc[i][1]);
                            acc[i][2] = __builtin_fma((double)gv.z, xv, acc[i][2]);
                            acc[i][3] = __builtin_fma((double)gv.w, xv, acc[i][3]);
                        }
                    }
                }
            }
        }
        __syncthreads();  // s_g is rewritten by the next tile
    }

    // ---- block partials: the slices of a column added in slice order
    double *__restrict__ out =
        g.b.work + (int64_t)blockIdx.x * (actor_stride(D) + (kDiag ? kDiagSums : 0));
    if (slices == 1) {
        // 128 < ncol < 256: the threads t >= ncol own nothing (us == 1) and
        // must not store their zeros over the owners' columns
#pragma unroll
        for (int i = 0; i < kActorColsPerThread; ++i) {
            const int c = kk + i * kThreads;
            if (own && c < ncol)
#pragma unroll
                for (int r = 0; r < 4; ++r) out[r * ncol + c] = acc[i][r];
        }
    } else {
        // through LDS in rounds of 4 values per thread (reusing s_g as fp64:
        // 256 x 4 floats = 512 doubles = 2 values per thread and round)
        double *s_acc = reinterpret_cast<double *>(s_g);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            s_acc[2 * t] = acc[0][2 * half];
            s_acc[2 * t + 1] = acc[0][2 * half + 1];
            __syncthreads();
            if (t < ncol) {
                double a0 = 0.0, a1 = 0.0;
                for (int s = 0; s < slices; ++s) {
                    a0 += s_acc[2 * (s * ncol + t)];
                    a1 += s_acc[2 * (s * ncol + t) + 1];
                }
                out[(2 * half) * ncol + t] = a0;
                out[(2 * half + 1) * ncol + t] = a1;
            }
            __syncthreads();
        }
    }
    const double bs = block_sum(sum_surr, s_red);
    const double bent = block_sum(sum_ent, s_red);
    if (t == 0) {
        out[4 * ncol] = bs;
        out[4 * ncol + 1] = bent;
    }
    if constexpr (kDiag) {
        const double bkl = block_sum(sum_kl, s_red);
        const double bout = block_sum(sum_out, s_red);
        const DiagArgs &dg = only(x...);
        if (t == 0) {
            out[4 * ncol + 2] = bkl;
            out[4 * ncol + 3] = bout;
            if (dg.stop && dg.first && blockIdx.x == 0) {
                dg.stop[0] = 0;
                dg.stop[1] = -1;
            }
        }
    } else if constexpr (sizeof...(X) != 0) {
        // the count of the update this launch belongs to: one thread, read by
        // no thread of this launch, by every thread of the finish launch. Last
        // in the kernel, where nothing else is live: its pow() at the start
        // raised the critic pass from 88 to 111 VGPRs
        const AdvArgs &adv = only(x...);
        if (blockIdx.x == 0 && t == 0)
            marlnav_adam::adam_advance_one(adv.state, adv.lr, adv.beta1, adv.beta2);
    }
}

// one block: S and the loss sums added over the blocks in block order, then
// the epilogue. LDS: 4 (D + 1) + 2 doubles of totals, group partials before.
//
// ADAM: every thread then runs the Adam element update of the elements it has
// stored, from the stored fp32 values. The block barrier between the two
// halves puts every read of a parameter (the epilogue reads W1, b1 and the
// heads) before the first write of one.
template <class... X>
__global__ void __launch_bounds__(kThreads) actor_finish(PpoArgs g, X... x)
{
    constexpr bool kDiag = is_diag<X...>::value;
    const int D = g.D, H = g.H, ncol = D + 1;
    const int nS = 4 * ncol + 2;
    extern __shared__ __attribute__((aligned(16))) double s_fin[];
    double *s_S = s_fin;          // [r][c] totals, then the two loss sums
    double *s_grp = s_fin + nS;   // group partials [grp][nS] when nS < kThreads
    const int t = threadIdx.x;
    if constexpr (kDiag) {
        // behind the stop: the update's log cells say so and nothing else is
        // touched. Read ahead of the block's first barrier; thread 0's write
        // of the flag below is behind it.
        const DiagArgs &dg = only(x...);
        if (dg.stop && !dg.first && dg.stop[0] != 0) {
            if (t == 0) {
                const double nan = __builtin_nan("");
                g.b.loss[0] = nan;
                for (int i = 0; i < kDiagRow - 1; ++i) dg.diag[i] = nan;
                dg.diag[kDiagRow - 1] = 2.0;
            }
            return;
        }
    }
    const int64_t stride = actor_stride(D) + (kDiag ? kDiagSums : 0);
    const double *__restrict__ work = g.b.work;
    const int groups = nS >= kThreads ? 1 : kThreads / nS;
    if (groups == 1) {
        for (int c = t; c < nS; c += kThreads) s_S[c] = sum_strided(work + c, g.nblocks, stride);
    } else {
        const int grp = t / nS, c = t - grp * nS;
        if (grp < groups) {
            const int64_t n = grp < g.nblocks ? (g.nblocks - grp + groups - 1) / groups : 0;
            s_grp[grp * nS + c] = sum_strided(work + grp * stride + c, n, groups * stride);
        }
        __syncthreads();
        if (t < nS) {
            double a = 0.0;
            for (int q = 0; q < groups; ++q) a += s_grp[q * nS + t];
            s_S[t] = a;
        }
    }
    __syncthreads();

    if constexpr (kDiag) {
        // the two diagnostic columns, whatever D: thread = (column t & 1, group
        // t >> 1 of 128) adds its blocks grp, grp + 128, ... in that order,
        // block_sum adds a column's 128 group sums (the other column's
        // threads add zeros)
        const DiagArgs &dg = only(x...);
        double *s_red = s_fin + (size_t)nS * (1 + (groups > 1 ? groups : 0));
        const int c = t & 1, grp = t >> 1;
        const int64_t n =
            grp < g.nblocks ? (g.nblocks - grp + kDiagGroups - 1) / kDiagGroups : 0;
        const double part = sum_strided(work + grp * stride + nS + c, n, kDiagGroups * stride);
        const double tot_kl = block_sum(c == 0 ? part : 0.0, s_red);
        const double tot_out = block_sum(c == 1 ? part : 0.0, s_red);
        if (t == 0) {
            // the loss as below, the entropy's fp64 quotient kept for the row
            const double m = (double)g.M;
            const double clip_loss = s_S[4 * ncol] / m;
            const double ent_q = s_S[4 * ncol + 1] / m;
            const float ent_mean = (float)ent_q;
            g.b.loss[0] = clip_loss + (double)(g.ent_f * ent_mean);
            const double kl = tot_kl / m;
            // !(kl <= target): a NaN KL stops; target = +inf is monitor only
            const bool stop_now = dg.stop && dg.target_kl < __builtin_inf() && !(kl <= dg.target_kl);
            dg.diag[0] = clip_loss;
            dg.diag[1] = ent_q;
            dg.diag[2] = kl;
            dg.diag[3] = tot_out / m;
            dg.diag[4] = stop_now ? 1.0 : 0.0;
            if (stop_now) {
                dg.stop[0] = 1;
                dg.stop[1] = dg.k;
            }
        }
    } else if (t == 0) {
        // clip mean in fp64; entropy mean rounded to fp32 and scaled in fp32
        const double clip_loss = s_S[4 * ncol] / (double)g.M;
        const float ent_mean = (float)(s_S[4 * ncol + 1] / (double)g.M);
        g.b.loss[0] = clip_loss + (double)(g.ent_f * ent_mean);
    }
    const double *S[4] = {s_S, s_S + ncol, s_S + 2 * ncol, s_S + 3 * ncol};
    const float *__restrict__ w1 = g.b.actor_fc1_w;
    const float *__restrict__ b1 = g.b.actor_fc1_b;
    // d[Wmu; Wstd][r][j] = sum_k S_x[r][k] W1[j][k] + s_1[r] b1[j]
    for (int idx = t; idx < 4 * H; idx += kThreads) {
        const int r = idx / H, j = idx - r * H;
        double a = S[r][D] * (double)b1[j];
        for (int k = 0; k < D; ++k) a = __builtin_fma(S[r][k], (double)w1[(int64_t)j * D + k], a);
        (r < 2 ? g.b.grad_actor_mu_w : g.b.grad_actor_std_w)[(r & 1) * H + j] = (float)a;
    }
    if (t < 4) (t < 2 ? g.b.grad_actor_mu_b : g.b.grad_actor_std_b)[t & 1] = (float)S[t][D];
    // dW1[j][k] = sum_r head_r[j] S_x[r][k], db1[j] = sum_r head_r[j] s_1[r]
    for (int64_t idx = t; idx < (int64_t)H * ncol; idx += kThreads) {
        const int j = (int)(idx / ncol), c = (int)(idx - (int64_t)j * ncol);
        double a = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float hw = (r < 2 ? g.b.actor_mu_w : g.b.actor_std_w)[(r & 1) * H + j];
            a = __builtin_fma((double)hw, S[r][c], a);
        }
        if (c < D)
            g.b.grad_actor_fc1_w[(int64_t)j * D + c] = (float)a;
        else
            g.b.grad_actor_fc1_b[j] = (float)a;
    }
    if constexpr (sizeof...(X) != 0 && is_clip_fold<X...>::value) {
        // CLIP: every gradient is stored; behind the barrier the block re-reads
        // .grad in the canonical order of marlnav_adam.hip's grad_sqsum /
        // adam_advance_clip (items of 4 in table order, block_sum per 256
        // items, the partials summed by thread t = t, t + 256, ..., block_sum),
        // forms the coefficient, and updates from the scaled, stored gradient.
        // The totals in s_fin are dead by now: its head is the scratch.
        __syncthreads();
        const ClipFoldArgs &cf = only(x...);
        const FoldArgs &f = cf.f;
        float *const gp[6] = {g.b.grad_actor_fc1_w, g.b.grad_actor_fc1_b, g.b.grad_actor_mu_w,
                              g.b.grad_actor_mu_b,  g.b.grad_actor_std_w, g.b.grad_actor_std_b};
        const int n[6] = {H * D, H, 2 * H, 2, 2 * H, 2};
        int end[6], items = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            items += (n[i] + 3) / 4;
            end[i] = items;
        }
        double *sh = s_fin;                  // kWaves
        double *s_part = s_fin + kWaves;     // <= kClipFoldMaxBlocks partials
        double *s_coef = s_part + kClipFoldMaxBlocks;
        const int nb = (items + kThreads - 1) / kThreads;
        for (int blk = 0; blk < nb; ++blk) {
            const int item = blk * kThreads + t;
            double acc = 0.0;
            if (item < items) {
                int slot = 0;
#pragma unroll
                for (int i = 1; i < 6; ++i)
                    if (item >= end[i - 1]) slot = i;
                const int e0 = (item - (slot ? end[slot - 1] : 0)) * 4;
                const int left = n[slot] - e0;
                const int cnt = left < 4 ? left : 4;
                for (int j = 0; j < cnt; ++j) {
                    const double gj = (double)gp[slot][e0 + j];
                    acc += gj * gj;
                }
            }
            const double part = block_sum(acc, sh);
            if (t == 0) s_part[blk] = part;
        }
        __syncthreads();
        const double total = block_sum(t < nb ? 0.0 + s_part[t] : 0.0, sh);
        if (t == 0) {
            const double norm = sqrt(total);
            const double coef = marlnav_adam::clip_coef(norm, cf.max_norm);
            *s_coef = coef;
            const_cast<AdamState *>(f.state)->reserved = coef;  // as adam_advance_clip leaves it
            if (cf.norm_out) *cf.norm_out = norm;
        }
        __syncthreads();
        const double coef = *s_coef;
        const AdamScalars c = fold_scalars(f);
        for (int idx = t; idx < 4 * H; idx += kThreads) {
            const int r = idx / H, j = idx - r * H;
            clip_fold_element(f, r < 2 ? 2 : 4, (r & 1) * H + j, gp[r < 2 ? 2 : 4], coef, c);
        }
        if (t < 4) clip_fold_element(f, t < 2 ? 3 : 5, t & 1, gp[t < 2 ? 3 : 5], coef, c);
        for (int64_t idx = t; idx < (int64_t)H * ncol; idx += kThreads) {
            const int j = (int)(idx / ncol), cc = (int)(idx - (int64_t)j * ncol);
            if (cc < D)
                clip_fold_element(f, 0, (int64_t)j * D + cc, gp[0], coef, c);
            else
                clip_fold_element(f, 1, j, gp[1], coef, c);
        }
    } else if constexpr (sizeof...(X) != 0 && !kDiag) {
        __syncthreads();
        const FoldArgs &f = only(x...);
        const AdamScalars c = fold_scalars(f);
        // the same thread -> element maps as above; slots: fc1_w, fc1_b, mu_w,
        // mu_b, std_w, std_b
        for (int idx = t; idx < 4 * H; idx += kThreads) {
            const int r = idx / H, j = idx - r * H;
            const int64_t e = (r & 1) * H + j;
            fold_element(f, r < 2 ? 2 : 4, e,
                         (r < 2 ? g.b.grad_actor_mu_w : g.b.grad_actor_std_w)[e], c);
        }
        if (t < 4)
            fold_element(f, t < 2 ? 3 : 5, t & 1,
                         (t < 2 ? g.b.grad_actor_mu_b : g.b.grad_actor_std_b)[t & 1], c);
        for (int64_t idx = t; idx < (int64_t)H * ncol; idx += kThreads) {
            const int j = (int)(idx / ncol), cc = (int)(idx - (int64_t)j * ncol);
            if (cc < D)
                fold_element(f, 0, (int64_t)j * D + cc, g.b.grad_actor_fc1_w[(int64_t)j * D + cc],
                             c);
            else
                fold_element(f, 1, j, g.b.grad_actor_fc1_b[j], c);
        }
    }
}


// =========================================================================
// critic
// =========================================================================
// output tiling of one block: kc columns of A D (<= 256), `us_n` unit slices
// of JT hidden units each
struct CriticTiling {
    int kc;        // columns of a column tile
    int ncoltile;  // column tiles
    int us_n;      // unit slices of a block
    int ub;        // hidden units of a block = us_n * JT
    int nugroup;   // unit groups
    int jt;        // 8 or 64
};

inline CriticTiling critic_tiling(int AD, int H)
{
    CriticTiling c;
    c.kc = AD < kThreads ? AD : kThreads;
    c.ncoltile = (AD + c.kc - 1) / c.kc;
    c.us_n = kThreads / c.kc;
    // narrow rows: several unit slices of 8 share the block; wide rows: one
    // slice of 64 (fewer blocks that recompute the forward pass)
    c.jt = c.us_n >= 2 ? 8 : 64;
    c.ub = c.us_n * c.jt;
    if (c.ub > 64) {  // h of the block's units: at most 64 per row in LDS
        c.us_n = 64 / c.jt;
        c.ub = 64;
    }
    c.nugroup = (H + c.ub - 1) / c.ub;
    return c;
}

// per-chunk workspace: dWc [H][AD], dbc [H], dW2 [H], db2, loss sum
__device__ __host__ inline int64_t critic_stride(int AD, int H)
{
    return (int64_t)H * AD + 2 * (int64_t)H + 2;
}

constexpr int kHPad = 68;  // floats per row of the h tile: 64 units, rows 16-byte aligned
constexpr size_t kCriticLdsBytes =
    sizeof(float) * ((size_t)kCriticTile * kHPad + kWaves * kCriticTile + kCriticTile) +
    sizeof(double) * (kWaves + 2 * kThreads);

// MODE kFused: forward, delta, dh and the outer product in one block.
// MODE kForward: everything but the outer product; dh of the block's units
// goes to the workspace ([row][hp] fp32) for the kBackward blocks.
// MODE kBackward: the outer product alone, dh read back from the workspace.
enum { kFused = 0, kForward = 1, kBackward = 2 };

template <int JT, int MODE, class ARGS, class... X>
__global__ void __launch_bounds__(kThreads) critic_pass(ARGS g, CriticTiling ct, float *dhbuf,
                                                         int hp, int vec4, X... x)
{
    constexpr bool kGather = is_gather<ARGS>::value;
    const int A = g.A, D = g.D, H = g.H;
    const int AD = A * D;
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    float *s_h = s_dyn;                                // [row][kHPad]: h, then dh
    float *s_part = s_h + kCriticTile * kHPad;         // [wave][row]
    float *s_delta = s_part + kWaves * kCriticTile;    // [row]
    double *s_red = reinterpret_cast<double *>(s_delta + kCriticTile);
    double *s_vec = s_red + kWaves;                    // [2][256] unit-vector partials

    const int t = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lane = t & 63;
    const int Hq = (H + kWaves - 1) / kWaves;
    const int j0 = q * Hq, j1 = (j0 + Hq < H) ? j0 + Hq : H;

    const int coltile = blockIdx.y % ct.ncoltile, ugroup = blockIdx.y / ct.ncoltile;
    const int ubase = ugroup * ct.ub;                   // first hidden unit of this block
    const int col0 = coltile * ct.kc;
    // phase-2 ownership
    const int us = t / ct.kc, kk = t - us * ct.kc;
    const int col = col0 + kk;
    const bool own = us < ct.us_n && col < AD;
    const int uj0 = us * JT;                            // first own unit, relative to ubase
    double acc[JT];
#pragma unroll
    for (int i = 0; i < JT; ++i) acc[i] = 0.0;
    // unit vectors dbc, dW2: thread = (unit jj = t & 63, row quarter t >> 6)
    double a_bc = 0.0, a_w2 = 0.0, a_b2 = 0.0, a_loss = 0.0;
    const bool first = blockIdx.y == 0;

    const float *__restrict__ wc = g.b.critic_fc1_w;
    const float *__restrict__ bc = g.b.critic_fc1_b;
    const float *__restrict__ w2 = g.b.critic_fc2_w;
    const float b2 = g.b.critic_fc2_b[0];
    const int64_t N = g.N;
    const double inv_n = 1.0 / (double)N;
    const int64_t rows_blk = MODE == kForward ? g.fw_rows : g.rows_per_block;
    const int64_t row_lo = (int64_t)blockIdx.x * rows_blk;
    const int64_t row_hi = row_lo + rows_blk < N ? row_lo + rows_blk : N;

    StepWalk<kCriticTile> wk;  // GATHER: the tile's env rows in the storage
    for (int64_t tile = row_lo; tile < row_hi; tile += kCriticTile) {
        if constexpr (kGather) wk.start(g.steps, g.T, g.P, tile);
        if constexpr (MODE == kBackward) {
            // ---- dh of the tile's rows and the block's units, from the workspace
            for (int idx = t; idx < kCriticTile * ct.ub; idx += kThreads) {
                const int r = idx / ct.ub, jj = idx - r * ct.ub;
                const int64_t row = tile + r;
                const int j = ubase + jj;
                s_h[r * kHPad + jj] = (row < row_hi && j < hp) ? dhbuf[row * hp + j] : 0.0f;
            }
        } else {
            // ---- forward: wave q sums hidden units [j0, j1) for the tile's rows,
            // eight units at a time (AD is even: D is; rows are 8-byte aligned, and
            // 16-byte aligned where vec4 says so)
            {
                const int64_t row_raw = tile + lane;
                const int64_t row = row_raw < row_hi ? row_raw : row_hi - 1;  // stays in bounds
                int64_t prow = row;
                if constexpr (kGather) prow = wk.at((int)(row - tile));
                const float *__restrict__ xe = g.b.obs + prow * AD;
                float part = 0.0f;
                for (int j = j0; j < j1; j += 8) {
                    // fp32 FMA chains of kFwdChain inputs, added up in fp64:
                    // the rounding of a pre-activation does not grow with A D
                    double d8[8];
                    const float *wr[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int jj = j + i < j1 ? j + i : j1 - 1;  // a short last group repeats a unit
                        d8[i] = (double)bc[jj];
                        wr[i] = wc + (int64_t)jj * AD;
                    }
                    for (int k0 = 0; k0 < AD; k0 += kFwdChain) {
                        const int k1 = k0 + kFwdChain < AD ? k0 + kFwdChain : AD;
                        float a8[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) a8[i] = 0.0f;
                        if (vec4) {
                            for (int k = k0; k < k1; k += 4) {
                                const float4 xv = *reinterpret_cast<const float4 *>(xe + k);
#pragma unroll
                                for (int i = 0; i < 8; ++i) {
                                    a8[i] = __builtin_fmaf(wr[i][k], xv.x, a8[i]);
                                    a8[i] = __builtin_fmaf(wr[i][k + 1], xv.y, a8[i]);
                                    a8[i] = __builtin_fmaf(wr[i][k + 2], xv.z, a8[i]);
                                    a8[i] = __builtin_fmaf(wr[i][k + 3], xv.w, a8[i]);
                                }
                            }
                        } else {
                            for (int k = k0; k < k1; k += 2) {
                                const float2 xv = *reinterpret_cast<const float2 *>(xe + k);
#pragma unroll
                                for (int i = 0; i < 8; ++i) {
                                    a8[i] = __builtin_fmaf(wr[i][k], xv.x, a8[i]);
                                    a8[i] = __builtin_fmaf(wr[i][k + 1], xv.y, a8[i]);
                                }
                            }
                        }
#pragma unroll
                        for (int i = 0; i < 8; ++i) d8[i] += (double)a8[i];
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (j + i < j1) {
                            const float h = relu_t((float)d8[i]);
                            part = __builtin_fmaf(w2[j + i], h, part);
                            const int rel = j + i - ubase;
                            if (rel >= 0 && rel < ct.ub) s_h[lane * kHPad + rel] = h;
                        }
                }
                s_part[q * kCriticTile + lane] = part;
            }
            __syncthreads();
            // ---- delta of the tile's rows
            if (t < kCriticTile) {
                const int64_t row = tile + t;
                float delta = 0.0f;
                if (row < row_hi) {
                    float nv = s_part[t];
#pragma unroll
                    for (int w = 1; w < kWaves; ++w) nv += s_part[w * kCriticTile + t];
                    nv += b2;
                    int64_t prow = row;
                    if constexpr (kGather) prow = wk.at(t);
                    const double ret = g.b.returns[prow];
                    const float val = g.b.values[prow];
                    const float lo = val - g.eps_f, hi = val + g.eps_f;
                    const float cl = nv < lo ? lo : (nv > hi ? hi : nv);
                    const double e0 = (double)nv - ret, e1 = (double)cl - ret;
                    const double s0 = e0 * e0, s1 = e1 * e1;
                    a_loss += s1 > s0 ? s1 : s0;
                    const bool inside = nv >= lo && nv <= hi;
                    const double gd = 2.0 * e0 * inv_n;
                    // torch.maximum splits a tie; inside the clamp both halves arrive
                    delta = inside || s0 > s1 ? (float)gd : (s0 == s1 ? (float)(0.5 * gd) : 0.0f);
                    a_b2 += (double)delta;
                }
                s_delta[t] = delta;
            }
            __syncthreads();
            // ---- h -> dh in place, with the unit vectors' sums
            {
                const int jj = lane, rq = q;
                const int j = ubase + jj;
                const bool unit = jj < ct.ub && j < H;
                const float w2j = unit ? w2[j] : 0.0f;
                for (int r = rq * 16; r < rq * 16 + 16; ++r) {
                    const float dl = s_delta[r];
                    float dh = 0.0f;
                    if (unit && tile + r < row_hi) {  // padding rows repeat the last row
                        const float h = s_h[r * kHPad + jj];
                        a_w2 = __builtin_fma((double)dl, (double)h, a_w2);
                        dh = h > 0.0f ? dl * w2j : 0.0f;
                        a_bc += (double)dh;
                    }
                    if (jj < ct.ub) {
                        if constexpr (MODE == kForward) {
                            if (tile + r < row_hi) dhbuf[(tile + r) * hp + j] = dh;
                        } else {
                            s_h[r * kHPad + jj] = dh;  // units past H: zeros
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- outer product: thread = (column, unit slice)
        if (MODE != kForward && own) {
            const int64_t left = row_hi - tile;
            const int nrows = left < kCriticTile ? (int)left : kCriticTile;
            if constexpr (kGather) {
                // rows [r0, r1) of the tile, row r at physical row `first` + r
                auto add_rows = [&](int r0, int r1, int64_t first) {
                    const float *__restrict__ xc = g.b.obs + first * AD + col;
                    for (int r = r0; r < r1; ++r) {
                        const double xv = (double)xc[(int64_t)r * AD];
                        // uj0 is a multiple of JT >= 8 floats, the row pitch of 16 bytes
                        const float4 *__restrict__ dh =
                            reinterpret_cast<const float4 *>(s_h + r * kHPad + uj0);
    #pragma unroll
                        for (int i = 0; i < JT / 4; ++i) {
                            const float4 d4 = dh[i];
                            acc[4 * i] = __builtin_fma((double)d4.x, xv, acc[4 * i]);
                            acc[4 * i + 1] = __builtin_fma((double)d4.y, xv, acc[4 * i + 1]);
                            acc[4 * i + 2] = __builtin_fma((double)d4.z, xv, acc[4 * i + 2]);
                            acc[4 * i + 3] = __builtin_fma((double)d4.w, xv, acc[4 * i + 3]);
                        }
                    }
                };
                const bool one = wk.R >= kCriticTile;  // at most one step boundary
                const int64_t run0 = wk.run0();
                const int n0 = one && run0 < nrows ? (int)run0 : nrows;
                if (JT <= 8 && one) {
                    // two constant-stride runs
                    add_rows(0, n0, wk.first0());
                    add_rows(n0, nrows, wk.first1());
                } else {
                    // one copy of the loop (JT = 64: 64 accumulators per copy); r is
                    // block-uniform, so the choice of the base is scalar work
                    for (int r = 0; r < nrows; ++r)
                        add_rows(r, r + 1,
                                 one ? (r < n0 ? wk.first0() : wk.first1()) : wk.at(r) - r);
                }
            } else {
                const float *__restrict__ xc = g.b.obs + tile * AD + col;
                for (int r = 0; r < nrows; ++r) {
                    const double xv = (double)xc[(int64_t)r * AD];
                    // uj0 is a multiple of JT >= 8 floats, the row pitch of 16 bytes
                    const float4 *__restrict__ dh =
                        reinterpret_cast<const float4 *>(s_h + r * kHPad + uj0);
#pragma unroll
                    for (int i = 0; i < JT / 4; ++i) {
                        const float4 d4 = dh[i];
                        acc[4 * i] = __builtin_fma((double)d4.x, xv, acc[4 * i]);
                        acc[4 * i + 1] = __builtin_fma((double)d4.y, xv, acc[4 * i + 1]);
                        acc[4 * i + 2] = __builtin_fma((double)d4.z, xv, acc[4 * i + 2]);
                        acc[4 * i + 3] = __builtin_fma((double)d4.w, xv, acc[4 * i + 3]);
                    }
                }
            }
        }
        __syncthreads();  // s_h, s_part, s_delta are rewritten by the next tile
    }

    double *__restrict__ out = g.b.work + (int64_t)blockIdx.x * critic_stride(AD, H);
    if (MODE != kForward && own) {
#pragma unroll
        for (int i = 0; i < JT; ++i) {
            const int j = ubase + uj0 + i;
            if (j < H) out[(int64_t)j * AD + col] = acc[i];
        }
    }
    if constexpr (MODE == kBackward) return;
    double *__restrict__ vout = MODE == kForward
                                    ? g.fw_part + (int64_t)blockIdx.x * (2 * H + 2)
                                    : out + (int64_t)H * AD;
    // unit vectors (the blocks of column tile 0), row quarters in order
    if (coltile == 0) {
        s_vec[t] = a_bc;
        s_vec[kThreads + t] = a_w2;
        __syncthreads();
        if (t < ct.ub && ubase + t < H) {
            double vb = 0.0, vw = 0.0;
            for (int w = 0; w < kWaves; ++w) {
                vb += s_vec[w * 64 + t];
                vw += s_vec[kThreads + w * 64 + t];
            }
            vout[ubase + t] = vb;
            vout[H + ubase + t] = vw;
        }
        __syncthreads();
    }
    if (first) {  // uniform per block
        const double sb2 = block_sum(a_b2, s_red);
        const double sl = block_sum(a_loss, s_red);
        if (t == 0) {
            vout[2 * H] = sb2;
            vout[2 * H + 1] = sl;
        }
    }
    if constexpr (sizeof...(X) != 0) {
        // as in actor_pass: the first launch of the update advances the count
        const AdvArgs &adv = only(x...);
        if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0)
            marlnav_adam::adam_advance_one(adv.state, adv.lr, adv.beta1, adv.beta2);
    }
}

// thread = output element: its chunk partials added in chunk order. ADAM: the
// thread then updates that element of the parameter (critic_finish reads no
// parameter, so no thread of the launch reads what another writes).
template <class... X>
__global__ void __launch_bounds__(kThreads) critic_finish(PpoArgs g, X... x)
{
    const int H = g.H, AD = g.A * g.D;
    const int64_t stride = critic_stride(AD, H);
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= stride) return;
    const int64_t nW = (int64_t)H * AD;
    double a = 0.0;
    if (idx >= nW && g.fw_part) {  // the kForward blocks' partials
        a = sum_strided(g.fw_part + (idx - nW), g.fw_blocks, 2 * H + 2);
    } else {
        a = sum_strided(g.b.work + idx, g.nblocks, stride);
    }
    if (idx < nW)
        g.b.grad_critic_fc1_w[idx] = (float)a;
    else if (idx < nW + H)
        g.b.grad_critic_fc1_b[idx - nW] = (float)a;
    else if (idx < nW + 2 * H)
        g.b.grad_critic_fc2_w[idx - nW - H] = (float)a;
    else if (idx == nW + 2 * H)
        g.b.grad_critic_fc2_b[0] = (float)a;
    else
        g.b.loss[0] = a / (double)g.N;
    if constexpr (sizeof...(X) != 0) {
        if (idx > nW + 2 * H) return;  // the loss
        const FoldArgs &f = only(x...);
        const AdamScalars c = fold_scalars(f);
        const float gf = (float)a;     // the value stored above
        if (idx < nW)
            fold_element(f, 0, idx, gf, c);
        else if (idx < nW + H)
            fold_element(f, 1, idx - nW, gf, c);
        else if (idx < nW + 2 * H)
            fold_element(f, 2, idx - nW - H, gf, c);
        else
            fold_element(f, 3, 0, gf, c);
    }
}


// ---- host side
int check_dims(const MarlnavPpoDims *d)
{
    if (!d) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo dims is NULL");
    // (num_steps is reported after num_parallel and before the rest of the shape)
    if (d->num_parallel >= 1 && d->num_steps < 1)
        return failf(MARLNAV_EINVAL, "ppo: num_steps=%lld < 1", (long long)d->num_steps);
    if (int rc = check_policy_shape("ppo", d->num_parallel, d->num_agents, d->obs_dim,
                                    d->hidden_size))
        return rc;
    if (d->reserved != 0) return failf(MARLNAV_EINVAL, "ppo: reserved=%d must be 0", d->reserved);
    if (d->num_steps > ((int64_t)1 << 40) / d->num_parallel / d->num_agents)
        return failf(MARLNAV_EINVAL, "ppo: num_steps=%lld x num_parallel=%lld rows are too many",
                     (long long)d->num_steps, (long long)d->num_parallel);
    if (d->num_steps * d->num_parallel < 2)
        return failf(MARLNAV_EINVAL,
                     "ppo: num_steps=%lld x num_parallel=%lld gives fewer than 2 env rows",
                     (long long)d->num_steps, (long long)d->num_parallel);
    return 0;
}

void actor_grid(int64_t M, int64_t &rows_per_block, int64_t &nblocks)
{
    int64_t rows = (M + kActorMaxBlocks - 1) / kActorMaxBlocks;
    if (rows < kActorMinRows) rows = kActorMinRows;
    rows = (rows + kActorTile - 1) / kActorTile * kActorTile;
    rows_per_block = rows;
    nblocks = (M + rows - 1) / rows;
}

void critic_grid(int64_t N, int AD, int H, const CriticTiling &ct, int64_t &rows_per_chunk,
                 int64_t &nchunks)
{
    const int64_t per_y = (int64_t)ct.ncoltile * ct.nugroup;
    int64_t want = kCriticTargetBlocks / per_y;
    const int64_t fit = kCriticMaxWork / critic_stride(AD, H);
    if (want > fit) want = fit;
    if (want < 1) want = 1;
    const int64_t tiles = (N + kCriticTile - 1) / kCriticTile;
    const int64_t tiles_per_chunk = (tiles + want - 1) / want;
    rows_per_chunk = tiles_per_chunk * kCriticTile;
    nchunks = (N + rows_per_chunk - 1) / rows_per_chunk;
}

// The forward pass is shared through the workspace (kForward + kBackward
// launches) where the fused kernel would recompute it in several output
// tiles and dh of the whole minibatch ([N][hp] fp32) stays within bounds.
constexpr int64_t kCriticMaxDh = 32 << 20;  // floats (128 MiB)

inline int dh_pitch(int H) { return (H + 63) / 64 * 64; }

inline bool critic_split(int64_t N, int H, const CriticTiling &ct)
{
    return ct.ncoltile * ct.nugroup > 1 && N * dh_pitch(H) <= kCriticMaxDh;
}

// rows and count of the kForward blocks (finer than the chunks: they write
// 2 H + 2 partial sums each, not an H x A D tile)
inline void critic_forward_grid(int64_t N, int64_t &rows, int64_t &nblocks)
{
    rows = (N + kCriticForwardBlocks - 1) / kCriticForwardBlocks;
    rows = (rows + kCriticTile - 1) / kCriticTile * kCriticTile;
    nblocks = (N + rows - 1) / rows;
}

PpoArgs make_args(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b)
{
    PpoArgs a;
    a.b = *b;
    a.P = d->num_parallel;
    a.T = d->num_steps;
    a.N = a.T * a.P;
    a.A = d->num_agents;
    a.M = a.N * a.A;
    a.D = d->obs_dim;
    a.H = d->hidden_size;
    a.rows_per_block = a.nblocks = 0;
    a.fw_rows = a.fw_blocks = 0;
    a.fw_part = nullptr;
    a.clip_lo = a.clip_hi = a.eps_f = a.ent_f = 0.0f;
    return a;
}

#define PPO_NEED(field)                                                                   \
    if (!b->field) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: buffer " #field " is NULL")

}  // namespace

namespace {

// diag: the actor's partial rows carry the diagnostic variant's two columns
int64_t work_size(const MarlnavPpoDims *d, bool diag)
{
    const int rc = check_dims(d);
    if (rc) return rc;
    const int64_t N = d->num_steps * d->num_parallel, M = N * d->num_agents;
    int64_t rows, nb;
    actor_grid(M, rows, nb);
    const int64_t actor = nb * (actor_stride(d->obs_dim) + (diag ? kDiagSums : 0));
    const int AD = d->num_agents * d->obs_dim;
    const CriticTiling ct = critic_tiling(AD, d->hidden_size);
    critic_grid(N, AD, d->hidden_size, ct, rows, nb);
    int64_t critic = nb * critic_stride(AD, d->hidden_size);
    if (critic_split(N, d->hidden_size, ct)) {
        int64_t fr, fb;
        critic_forward_grid(N, fr, fb);
        critic += fb * (2 * d->hidden_size + 2) + (N * dh_pitch(d->hidden_size) + 1) / 2;
    }
    return actor > critic ? actor : critic;
}

}  // namespace

extern "C" int64_t marlnav_ppo_work_size(const MarlnavPpoDims *d) { return work_size(d, false); }

extern "C" int64_t marlnav_ppo_diag_work_size(const MarlnavPpoDims *d)
{
    return work_size(d, true);
}

namespace {

int check_mode(int advantage_mode)
{
    if (advantage_mode != MARLNAV_ADVANTAGE_REFERENCE && advantage_mode != MARLNAV_ADVANTAGE_ENV)
        return failf(MARLNAV_EINVAL,
                     "ppo: advantage_mode=%d must be MARLNAV_ADVANTAGE_REFERENCE or _ENV",
                     advantage_mode);
    return 0;
}

// values is read by the reference pairing only
int check_actor_bufs(const MarlnavPpoBuffers *b, int advantage_mode)
{
    if (!b) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo buffers is NULL");
    PPO_NEED(obs);
    PPO_NEED(actions);
    PPO_NEED(log_probs);
    if (advantage_mode == MARLNAV_ADVANTAGE_REFERENCE) PPO_NEED(values);
    PPO_NEED(returns);
    PPO_NEED(actor_fc1_w);
    PPO_NEED(actor_fc1_b);
    PPO_NEED(actor_mu_w);
    PPO_NEED(actor_mu_b);
    PPO_NEED(actor_std_w);
    PPO_NEED(actor_std_b);
    PPO_NEED(grad_actor_fc1_w);
    PPO_NEED(grad_actor_fc1_b);
    PPO_NEED(grad_actor_mu_w);
    PPO_NEED(grad_actor_mu_b);
    PPO_NEED(grad_actor_std_w);
    PPO_NEED(grad_actor_std_b);
    PPO_NEED(loss);
    PPO_NEED(work);
    return 0;
}

int check_critic_bufs(const MarlnavPpoBuffers *b)
{
    if (!b) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo buffers is NULL");
    PPO_NEED(obs);
    PPO_NEED(values);
    PPO_NEED(returns);
    PPO_NEED(critic_fc1_w);
    PPO_NEED(critic_fc1_b);
    PPO_NEED(critic_fc2_w);
    PPO_NEED(critic_fc2_b);
    PPO_NEED(grad_critic_fc1_w);
    PPO_NEED(grad_critic_fc1_b);
    PPO_NEED(grad_critic_fc2_w);
    PPO_NEED(grad_critic_fc2_b);
    PPO_NEED(loss);
    PPO_NEED(work);
    if (reinterpret_cast<uintptr_t>(b->obs) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: buffer obs must be 8-byte aligned");
    return 0;
}

int check_steps(const int32_t *steps)
{
    if (!steps) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: steps is NULL");
    if (reinterpret_cast<uintptr_t>(steps) & 3u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: steps must be 4-byte aligned");
    return 0;
}

// ---- which launches an update is ("The launch paths")
// whether the clipped phase folds the actor's clip and Adam step into
// actor_finish (marlnav_debug_clip_fold; the default is the measured decision
// of DESIGN.md §16)
int g_clip_fold = MARLNAV_CLIP_FOLD_DEFAULT;

// actor_finish is one block: its folded update walks the actor's elements
// 256 at a time, about 4 us per 1000 elements, against the 5 us the two
// launches of marlnav_adam_step cost. Measured: a gain of
// 1.3-2 us per update at 854 elements (3 x 3, H = 50), 0.5 us at 1354 (3 x 8),
// a loss of 14 us at 5054 (16 x 32). So the actor folds up to 1024 elements
// and keeps the separate Adam launches beyond. critic_finish is thread =
// element over many blocks; its fold gains 4-6 us per update up to 131 072
// env rows and loses 2-3 us at 524 288 (65536 x 3 x 3 of 8 steps), where the
// pass runs for 270 us and the separate Adam launches' dispatch hides behind
// it: the critic folds up to 2^17 env rows.
constexpr int64_t kActorFoldMaxElements = 1024;
constexpr int64_t kCriticFoldMaxRows = (int64_t)1 << 17;

// where the update's Adam step runs: in launches of its own (the caller's), in
// the finish launch, or, clipped, in actor_finish with the norm formed in-block
enum Fold { kNoFold, kFold, kClipFold };

Fold fold_of(const PpoUpdate &u, const MarlnavPpoDims *d)
{
    // the folds have no gather variants, and a monitored update that stops must
    // not step
    if (!u.ad || !u.may_fold || u.steps || u.diag_row) return kNoFold;
    if (u.network == MARLNAV_NETWORK_ACTOR) {
        const int64_t H = d->hidden_size, D = d->obs_dim;
        if (H * (D + 1) + 4 * H + 4 > kActorFoldMaxElements) return kNoFold;
        if (u.clip) return g_clip_fold ? kClipFold : kNoFold;
        return kFold;
    }
    // critic_finish updates elements before the norm exists
    if (u.clip || d->num_steps * d->num_parallel > kCriticFoldMaxRows) return kNoFold;
    return kFold;
}

void fold_args(const MarlnavAdamDims *ad, const MarlnavAdamBuffers *ab, AdvArgs *adv, FoldArgs *f)
{
    adv->state = static_cast<AdamState *>(ab->state);
    adv->lr = ad->lr;
    adv->beta1 = ad->beta1;
    adv->beta2 = ad->beta2;
    for (int i = 0; i < 6; ++i) {
        const bool used = i < ad->num_tensors;
        f->param[i] = used ? ab->param[i] : nullptr;
        f->exp_avg[i] = used ? ab->exp_avg[i] : nullptr;
        f->exp_avg_sq[i] = used ? ab->exp_avg_sq[i] : nullptr;
    }
    f->state = adv->state;
    f->beta1 = ad->beta1;
    f->beta2 = ad->beta2;
    f->omb1 = 1.0 - ad->beta1;
    f->omb2 = 1.0 - ad->beta2;
    f->eps = ad->eps;
    f->maximize = ad->maximize;
}

// checked arguments only: the two launches of the actor's update, the
// template packs chosen from the update and its fold
int enqueue_actor(const PpoUpdate &u, Fold fold, const MarlnavPpoDims *d,
                  const MarlnavPpoBuffers *b, hipStream_t s)
{
    PpoArgs a = make_args(d, b);
    actor_grid(a.M, a.rows_per_block, a.nblocks);
    // the reference's Python scalars 1 - margin, 1 + margin and ent_const meet
    // fp32 tensors: rounded to fp32 once
    a.clip_lo = (float)(1.0 - u.epsilon);
    a.clip_hi = (float)(1.0 + u.epsilon);
    a.ent_f = (float)u.ent_const;
    const int nS = 4 * (a.D + 1) + 2;
    const int groups = nS >= kThreads ? 1 : kThreads / nS;
    const size_t fin_lds = sizeof(double) * (size_t)nS * (1 + (groups > 1 ? groups : 0));
    const dim3 grid((unsigned)a.nblocks), blk(kThreads);
    const size_t lds = actor_lds_bytes(a.D);
    const bool env = u.advantage_mode == MARLNAV_ADVANTAGE_ENV;
    // the pass launch over `g` (PpoArgs, or GatherArgs: the gather variant) with
    // the trailing pack x
    auto pass = [&](const auto &g, auto... x) {
        if (env)
            hipLaunchKernelGGL((actor_pass<kPairEnv>), grid, blk, lds, s, g, x...);
        else
            hipLaunchKernelGGL((actor_pass<kPairReference>), grid, blk, lds, s, g, x...);
    };
    // the finish launches read the workspace alone: they take PpoArgs always
    auto finish = [&](size_t bytes, auto... x) {
        hipLaunchKernelGGL(actor_finish, dim3(1), dim3(kThreads), bytes, s, a, x...);
    };
    const size_t dg_lds = fin_lds + sizeof(double) * kWaves;
    const DiagArgs dg = {u.diag_row, u.stop, u.target_kl, u.k, u.k == 0 ? 1 : 0};
    AdvArgs adv;
    ClipFoldArgs c;
    if (fold != kNoFold) fold_args(u.ad, u.ab, &adv, &c.f);
    if (u.steps) {  // the gather variants
        GatherArgs ga;
        static_cast<PpoArgs &>(ga) = a;
        ga.steps = u.steps;
        if (u.diag_row) {
            pass(ga, dg);
            finish(dg_lds, dg);
        } else {
            pass(ga);
            finish(fin_lds);
        }
    } else if (u.diag_row) {  // the diagnostic variant
        pass(a, dg);
        finish(dg_lds, dg);
    } else if (fold == kClipFold) {  // norm, clip and update inside actor_finish
        c.max_norm = u.clip->max_norm;
        c.norm_out = u.clip->norm_out;
        pass(a, adv);
        finish(fin_lds, c);
    } else if (fold == kFold) {
        pass(a, adv);
        finish(fin_lds, c.f);
    } else {
        pass(a);
        finish(fin_lds);
    }
    return launch_status();
}

int enqueue_critic(const PpoUpdate &u, Fold fold, const MarlnavPpoDims *d,
                   const MarlnavPpoBuffers *b, hipStream_t s)
{
    PpoArgs a = make_args(d, b);
    const int AD = a.A * a.D;
    const CriticTiling ct = critic_tiling(AD, a.H);
    critic_grid(a.N, AD, a.H, ct, a.rows_per_block, a.nblocks);
    a.eps_f = (float)u.epsilon;  // values - epsilon: a Python scalar against an fp32 tensor
    const dim3 grid((unsigned)a.nblocks, (unsigned)(ct.ncoltile * ct.nugroup));
    // (with a gather too: every step starts a multiple of P A D floats after step 0)
    const int vec4 = AD % 4 == 0 && (reinterpret_cast<uintptr_t>(b->obs) & 15u) == 0;
    const bool split = critic_split(a.N, a.H, ct);
    CriticTiling fw = ct;
    float *dhbuf = nullptr;
    int hp = 0;
    dim3 fgrid(1);
    if (split) {
        // forward once per row: blocks of 64 hidden units, no output tile
        fw.kc = AD < kThreads ? AD : kThreads;
        fw.ncoltile = 1;
        fw.us_n = 1;
        fw.jt = 64;
        fw.ub = 64;
        fw.nugroup = (a.H + 63) / 64;
        hp = dh_pitch(a.H);
        critic_forward_grid(a.N, a.fw_rows, a.fw_blocks);
        a.fw_part = b->work + a.nblocks * critic_stride(AD, a.H);
        dhbuf = reinterpret_cast<float *>(a.fw_part + a.fw_blocks * (2 * a.H + 2));
        fgrid = dim3((unsigned)a.fw_blocks, (unsigned)fw.nugroup);
    }
    // the pass launches over `g` (PpoArgs, or GatherArgs: the gather variants);
    // x: empty, or the AdvArgs of a folded update for the update's first launch
    auto pass = [&](const auto &g, auto... x) {
        const dim3 blk(kThreads);
        if (split) {
            hipLaunchKernelGGL((critic_pass<1, kForward>), fgrid, blk, kCriticLdsBytes, s, g, fw,
                               dhbuf, hp, vec4, x...);
            if (ct.jt == 8)
                hipLaunchKernelGGL((critic_pass<8, kBackward>), grid, blk, kCriticLdsBytes, s, g,
                                   ct, dhbuf, hp, vec4);
            else
                hipLaunchKernelGGL((critic_pass<64, kBackward>), grid, blk, kCriticLdsBytes, s, g,
                                   ct, dhbuf, hp, vec4);
        } else if (ct.jt == 8) {
            hipLaunchKernelGGL((critic_pass<8, kFused>), grid, blk, kCriticLdsBytes, s, g, ct,
                               (float *)nullptr, 0, vec4, x...);
        } else {
            hipLaunchKernelGGL((critic_pass<64, kFused>), grid, blk, kCriticLdsBytes, s, g, ct,
                               (float *)nullptr, 0, vec4, x...);
        }
    };
    AdvArgs adv;
    FoldArgs f;
    if (fold == kFold) fold_args(u.ad, u.ab, &adv, &f);
    if (u.steps) {  // the gather variants
        GatherArgs ga;
        static_cast<PpoArgs &>(ga) = a;
        ga.steps = u.steps;
        pass(ga);
    } else if (fold == kFold) {
        pass(a, adv);
    } else {
        pass(a);
    }
    const int64_t nout = critic_stride(AD, a.H);
    const dim3 ogrid((unsigned)((nout + kThreads - 1) / kThreads));
    if (fold == kFold)
        hipLaunchKernelGGL(critic_finish, ogrid, dim3(kThreads), 0, s, a, f);
    else
        hipLaunchKernelGGL(critic_finish, ogrid, dim3(kThreads), 0, s, a);
    return launch_status();
}

// a gradient-only update: no optimiser, so nothing is folded and no step owed
PpoUpdate grad_only(int network, double epsilon, double ent_const, int advantage_mode,
                    const int32_t *steps, double *diag)
{
    PpoUpdate u = {};
    u.network = network;
    u.epsilon = epsilon;
    u.ent_const = ent_const;
    u.advantage_mode = advantage_mode;
    u.steps = steps;
    u.diag_row = diag;  // no stop: status 0
    u.target_kl = __builtin_inf();
    return u;
}

}  // namespace

int marlnav_internal_ppo_validate(int network, int advantage_mode, const MarlnavPpoDims *d,
                                  const MarlnavPpoBuffers *b)
{
    int rc = check_dims(d);
    if (rc) return rc;
    if (network != MARLNAV_NETWORK_ACTOR) return check_critic_bufs(b);
    rc = check_mode(advantage_mode);
    return rc ? rc : check_actor_bufs(b, advantage_mode);
}

int marlnav_internal_ppo_enqueue(const PpoUpdate *u, const MarlnavPpoDims *d,
                                 const MarlnavPpoBuffers *b, void *stream, bool *adam_owed)
{
    const Fold fold = fold_of(*u, d);
    *adam_owed = u->ad && fold == kNoFold;
    return u->network == MARLNAV_NETWORK_ACTOR
               ? enqueue_actor(*u, fold, d, b, (hipStream_t)stream)
               : enqueue_critic(*u, fold, d, b, (hipStream_t)stream);
}

extern "C" int marlnav_debug_clip_fold(int on)
{
    const int before = g_clip_fold;
    if (on == 0 || on == 1) g_clip_fold = on;
    return before;
}

namespace {

// a gradient-only entry behind its own checks
int enqueue_grad(const PpoUpdate &u, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                 void *stream)
{
    bool owed;
    return marlnav_internal_ppo_enqueue(&u, d, b, stream, &owed);
}

}  // namespace

extern "C" int marlnav_ppo_actor_grad_mode(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                           double epsilon, double ent_const, int advantage_mode,
                                           void *stream)
{
    const int rc = marlnav_internal_ppo_validate(MARLNAV_NETWORK_ACTOR, advantage_mode, d, b);
    if (rc) return rc;
    return enqueue_grad(grad_only(MARLNAV_NETWORK_ACTOR, epsilon, ent_const, advantage_mode,
                                  nullptr, nullptr), d, b, stream);
}

extern "C" int marlnav_ppo_actor_grad_diag(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                           double epsilon, double ent_const, int advantage_mode,
                                           double *diag, void *stream)
{
    const int rc = marlnav_internal_ppo_validate(MARLNAV_NETWORK_ACTOR, advantage_mode, d, b);
    if (rc) return rc;
    if (!diag) return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: diag is NULL");
    if (reinterpret_cast<uintptr_t>(diag) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: diag must be 8-byte aligned");
    return enqueue_grad(grad_only(MARLNAV_NETWORK_ACTOR, epsilon, ent_const, advantage_mode,
                                  nullptr, diag), d, b, stream);
}

// The gather forms: logical step slot s of the minibatch is
// step steps[s] of the storage whose step 0 the data pointers address.
extern "C" int marlnav_ppo_actor_grad_steps(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                            const int32_t *steps, double epsilon,
                                            double ent_const, int advantage_mode, double *diag,
                                            void *stream)
{
    int rc = marlnav_internal_ppo_validate(MARLNAV_NETWORK_ACTOR, advantage_mode, d, b);
    if (rc) return rc;
    rc = check_steps(steps);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(diag) & 7u)
        return marlnav_internal_fail(MARLNAV_EINVAL, "ppo: diag must be 8-byte aligned");
    return enqueue_grad(grad_only(MARLNAV_NETWORK_ACTOR, epsilon, ent_const, advantage_mode,
                                  steps, diag), d, b, stream);
}

extern "C" int marlnav_ppo_critic_grad_steps(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                             const int32_t *steps, double epsilon, void *stream)
{
    int rc = marlnav_internal_ppo_validate(MARLNAV_NETWORK_CRITIC, 0, d, b);
    if (rc) return rc;
    rc = check_steps(steps);
    if (rc) return rc;
    return enqueue_grad(grad_only(MARLNAV_NETWORK_CRITIC, epsilon, 0.0, 0, steps, nullptr), d, b,
                        stream);
}

extern "C" int marlnav_ppo_actor_grad(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                      double epsilon, double ent_const, void *stream)
{
    return marlnav_ppo_actor_grad_mode(d, b, epsilon, ent_const, MARLNAV_ADVANTAGE_REFERENCE,
                                       stream);
}

extern "C" int marlnav_ppo_critic_grad(const MarlnavPpoDims *d, const MarlnavPpoBuffers *b,
                                       double epsilon, void *stream)
{
    const int rc = marlnav_internal_ppo_validate(MARLNAV_NETWORK_CRITIC, 0, d, b);
    if (rc) return rc;
    return enqueue_grad(grad_only(MARLNAV_NETWORK_CRITIC, epsilon, 0.0, 0, nullptr, nullptr), d,
                        b, stream);
}
