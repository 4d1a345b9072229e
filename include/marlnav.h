/*
 * marlnav.h - C ABI of the MI355X (gfx950) environment-step library
 * (libmarlnav.so, built from marl-nav_amd/csrc/marlnav_step.hip,
 * marlnav_rollout.hip, marlnav_policy.hip, marlnav_ppo.hip,
 * marlnav_adam.hip and marlnav_eval.hip).
 *
 * The reference (JussiM01/MARL-nav) has no FFI: its boundary is the Python
 * class `Env` (marlnav/environment.py:8-286). Each entry point below replaces
 * one method of that class; the file:line it replaces is given per function.
 * The Python host mirror (marl-nav_amd/environment.py) binds these with
 * ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - Every pointer in MarlnavStepBuffers and every array argument is a DEVICE
 *    pointer (hipMalloc / torch caching allocator), contiguous, fp32 / uint8
 *    as documented. The library never allocates, frees or synchronises.
 *  - Every call enqueues its work on `stream` (a hipStream_t; NULL = the
 *    default stream) and returns immediately.
 *  - Return value: 0 on success, a negative MARLNAV_E* code otherwise; the
 *    message is available from marlnav_last_error() (thread-local).
 *  - Shapes: P = num_parallel, A = num_agents, O = observed obstacles,
 *    S = obstacle_stride (obstacles stored per env, >= O),
 *    D = 2 + 2*O + 2*(A-1) observation features per agent.
 *  - The observation buffer is packed (P, A, D) in the field order of the
 *    reference's `Observations` namedtuple (utils.py:13-15), which is also the
 *    concatenation order of `ObsNormalizer` (utils.py:531):
 *      [target_angle | target_distance | obstacles_angles[O] |
 *       obstacles_distances[O] | others_angles[A-1] | others_distances[A-1]]
 */
#ifndef MARLNAV_H
#define MARLNAV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MARLNAV_ABI_VERSION 5

/* error codes */
#define MARLNAV_OK 0
#define MARLNAV_EINVAL (-1)  /* bad dims / params / null pointer */
#define MARLNAV_ELAUNCH (-2) /* HIP launch error */
#define MARLNAV_EUNSUPPORTED (-3)

/* MarlnavParams.flags */
/* Finished envs take their fresh agent states from the post-move states of
 * this step instead of fresh_states: reproduces the aliasing of
 * MockInitializer (utils.py:310-319) on the reference's first step, where
 * Env.states IS the initializer's tensor and _move_agents mutates it. */
#define MARLNAV_FRESH_STATES_FROM_MOVED 0x1u
/* Native re-init draws agent noise (TriangleIntitializer with
 * noisy_ags=True, utils.py:381-388). The reference ships noisy_ags=False
 * (utils.py:25). */
#define MARLNAV_NOISY_AGENTS 0x2u
/* Also write the ObsNormalizer output (utils.py:519-532) to obs_norm. */
#define MARLNAV_WRITE_OBS_NORM 0x4u
/* Apply ActionScaler (utils.py:535-547) to the actions on load: the kernel
 * reads policy actions in [-1, 1] and scales them itself. */
#define MARLNAV_SCALE_ACTIONS 0x8u

typedef struct MarlnavDims {
    int64_t num_parallel;    /* P  (environment.py:15)                        */
    int32_t num_agents;      /* A  (environment.py:16), 2 <= A <= 64          */
    int32_t num_obstacles;   /* O  observed per agent (environment.py:17,148) */
    int32_t obstacle_stride; /* S  = obstacles.shape[1], O <= S <= 256        */
    int32_t reserved;        /* must be 0                                     */
    int64_t env_offset;      /* global id of env 0 of this shard (native RNG) */
} MarlnavDims;

typedef struct MarlnavParams {
    /* dynamics bounds, environment.py:32-35 */
    float min_speed, max_speed, min_accel, max_accel;
    /* truncation: truncated = step_num > trunc_after, with
     * trunc_after = episode_len - 1 (environment.py:97) */
    float trunc_after;
    /* reward weights, environment.py:48-53 */
    float risk_factor, distance_factor, heading_factor;
    float target_factor, soft_factor, bond_factor;
    /* geometric constants, environment.py:56-68 */
    float ob_risk_dist, ag_risk_dist, ob_coll_dist, ag_coll_dist;
    float agents_min_d, agents_max_d, max_at_prop_d, max_angle_diff;
    float target_radius, cap_distance, bond_sharpness, ideal_dist, init_dist;
    /* native re-init of obstacles, utils.py:344-347, 390-398:
     * x = obs_range_x * (u - 0.5) + obs_mean_x (same for y) */
    float obs_range_x, obs_mean_x, obs_range_y, obs_mean_y;
    /* native noisy agents (MARLNAV_NOISY_AGENTS), utils.py:370-388:
     * pos += ags_dist * noise_std * N(0,1); heading rotated by
     * angle_range * (u - 0.5) */
    float ags_dist, noise_std, angle_range;
    /* ActionScaler (MARLNAV_SCALE_ACTIONS): a' = scale[k]*a + mean[k] */
    float act_scale[2], act_mean[2];
    uint32_t flags;
    uint32_t reserved;
    uint64_t seed;           /* native RNG seed: all 64 bits enter the Philox2x32-10
                                keys through splitmix64 + fmix32 */
} MarlnavParams;

typedef struct MarlnavStepBuffers {
    /* environment state, updated in place (environment.py:28-30, 38-39) */
    float *states;           /* (P, A, 5): x, y, dir_x, dir_y, speed       */
    float *obstacles;        /* (P, S, 2)                                  */
    float *target;           /* (P, 1, 2)                                  */
    float *step_num;         /* (P,)                                       */
    uint8_t *terminates;     /* (P,) bool: reach-target delayed flag       */
    /* inputs */
    const float *actions;    /* (P, A, 2): angle, acceleration             */
    /* reference-RNG re-init candidates (the init sampler's output of this
     * step, environment.py:78). NULL => native Philox re-init. Only the rows
     * of finished envs are read. */
    const float *fresh_states;    /* (P, A, 5) */
    const float *fresh_obstacles; /* (P, S, 2) */
    const float *fresh_target;    /* (P, 1, 2) */
    /* native re-init template: A*5 agent states then 2 target coords */
    const float *formation;
    /* outputs */
    float *obs;              /* (P, A, D) packed Observations              */
    float *reward;           /* (P,)                                       */
    uint8_t *terminated;     /* (P,) bool                                  */
    uint8_t *truncated;      /* (P,) bool                                  */
    /* episode statistics accumulators: 3 rows (trunc, col, tar) of
     * marlnav_counter_slots() uint64 partial sums, added to in place */
    uint64_t *counters;
    /* optional fused ObsNormalizer (MARLNAV_WRITE_OBS_NORM) */
    float *obs_norm;         /* (P, A, D)                                  */
    const float *norm_mean;  /* (D,)                                       */
    const float *norm_scale; /* (D,)                                       */
    /* optional observation template of a native fresh env (NULL: computed
     * in full): marlnav_formation_obs() of `formation`. Finished envs whose
     * agent rows and target re-initialise to the formation exactly (every
     * old value finite) take their target and agent-agent pairs from it and
     * compute only the agent-obstacle pairs. */
    const float *formation_obs; /* (A, A, 2)                               */
    /* optional second state buffer (NULL: `states` is updated in place): the
     * step reads `states` and writes every env's new state row here, so the
     * launch never writes the lines it read (a host double-buffers the two,
     * as the reference rebinds `states` each step, environment.py:80).
     * Must not overlap `states`. The env-block and pair-split kernels write
     * it with 16-byte vector stores and are chosen only when it is 16-byte
     * aligned (as `states` must be for them); otherwise the step falls back
     * to the generic wave kernel. */
    float *states_out;       /* (P, A, 5)                                  */
} MarlnavStepBuffers;

/* Env.step(actions) - environment.py:92-107 (with _move_agents :113-137,
 * observations :139-180, _rews_and_terms :184-269, _reinit :76-90).
 * step_idx keys the native RNG (any value when fresh_* are given). */
int marlnav_step(const MarlnavDims *dims, const MarlnavParams *params,
                 const MarlnavStepBuffers *bufs, uint64_t step_idx,
                 void *stream);

/* Env.observations() - environment.py:139-180. obs: (P, A, D). params:
 * the env's parameters (only cap_distance, environment.py:65 / :172-177,
 * is read); NULL means the reference's default cap 0.1. */
int marlnav_observe(const MarlnavDims *dims, const MarlnavParams *params,
                    const float *states, const float *obstacles,
                    const float *target, float *obs, void *stream);

/* Native TriangleIntitializer.__call__ for every env (utils.py:375-398), as
 * used by Env.__init__ (environment.py:26-30): writes states/obstacles/target
 * from the formation template and the Philox stream at step_idx. */
int marlnav_reinit_all(const MarlnavDims *dims, const MarlnavParams *params,
                       const float *formation, float *states,
                       float *obstacles, float *target, uint64_t step_idx,
                       void *stream);

/* Observation template of the native re-init's fresh env (the
 * TriangleIntitializer formation, utils.py:350-368, observed as in
 * environment.py:139-166): out[(a*A + m)*2 + {0, 1}] = (bearing before the
 * cap of environment.py:172-177, distance) of agent a to pair m, m = 0 the
 * target, m >= 1 the other agents in ascending order skipping a. The same
 * fp32 arithmetic as the step kernels' observation. formation: 5A + 2
 * floats (as MarlnavStepBuffers.formation); out: 2*A*A floats. */
int marlnav_formation_obs(const MarlnavDims *dims, const float *formation, float *out,
                          void *stream);

/* Number of uint64 partial-sum slots per counter row for these dims. */
int64_t marlnav_counter_slots(const MarlnavDims *dims);

/* Sum the counter slots: out3[0..2] = (num_trunc, num_col, num_tar)
 * (environment.py:43-45, 98, 210-211). out3 is a device pointer. */
int marlnav_counters_total(const MarlnavDims *dims, const uint64_t *counters,
                           uint64_t *out3, void *stream);

/* MAPPO._process_rewards (models.py:131-148) on the device. Discounted
 * returns of a rollout of T steps, G_t = done_t ? 0 : r_t + gamma * G_{t+1}
 * (G_T = 0), in float64 like the reference (its accumulator is
 * torch.zeros(P, dtype=float), models.py:133), then normalized in place,
 * returns = (G - mean) / (std + 1e-12) with the unbiased std over all T*P
 * values (torch.std_mean, models.py:140-144).
 *   rewards (T, P) fp32, done (T, P) uint8 (bool), returns (T, P) fp64 out,
 *   stats: 2 fp64 out (mean, std), work: marlnav_returns_work_size(P) fp64.
 * All device pointers; enqueued on stream. */
int64_t marlnav_returns_work_size(int64_t num_parallel);
int marlnav_discounted_returns(const float *rewards, const uint8_t *done, int64_t T,
                               int64_t P, double gamma, double *returns, double *stats,
                               double *work, void *stream);

/* GAE(lambda) advantages of a rollout of T steps (not in the
 * reference, whose estimator is the normalised return above). One thread per
 * env walks its column backwards in fp64 in this operation order, with
 * gl = gamma * lam formed once on the host in fp64 and A_next = 0 at t = T-1:
 *   next  = t == T-1 ? (double)last_values[p] : (double)values[t+1][p]
 *   delta = ((double)r + gamma * (done ? 0.0 : next)) - (double)v
 *   A     = delta + gl * (done ? 0.0 : A_next)
 *   value_targets[t][p] = A + (double)v
 * The two `done ? 0.0 : x` are selects, so a non-finite value behind a done
 * does not reach any output. Then advantages = (A - mean) / (std + 1e-12)
 * with the mean and the unbiased std over all T*P raw advantages, by the
 * fixed-order two-pass reductions of marlnav_discounted_returns;
 * value_targets stay in reward units (not normalised).
 *   rewards, values (T, P) fp32; done (T, P) uint8, the merged terminated |
 *   truncated flag of the rollout: a truncated episode counts as ended and
 *   gets no bootstrap (its final observation is overwritten by the in-kernel
 *   re-init); last_values (P,) fp32, the critic's value of the observation
 *   after step T-1; advantages, value_targets (T, P) fp64 out; stats: 2 fp64
 *   out (mean, std of the raw advantages); work:
 *   marlnav_gae_work_size(P) fp64.
 * Everything is validated before the first launch (MARLNAV_EINVAL, the
 * message names the field): NULL pointers, T >= 1, T*P >= 2, gamma and lam
 * finite and in [0, 1]. No synchronisation, no atomics: equal inputs give
 * equal bits. */
int64_t marlnav_gae_work_size(int64_t num_parallel);
int marlnav_gae_advantages(const float *rewards, const uint8_t *done, const float *values,
                           const float *last_values, int64_t T, int64_t P, double gamma,
                           double lam, double *advantages, double *value_targets, double *stats,
                           double *work, void *stream);

/* Shapes of one policy call. D is the env's observation row length,
 * D = 2 + 2*O + 2*(A-1) for an observed obstacle count O in [1, 256]; H is
 * the hidden size of both networks (models.py:69-70, `hidden_size`). */
typedef struct MarlnavPolicyDims {
    int64_t num_parallel;    /* P  envs in this call                          */
    int32_t num_agents;      /* A  2 <= A <= 64                               */
    int32_t obs_dim;         /* D  features per agent row                     */
    int32_t hidden_size;     /* H  1 <= H <= 512                              */
    int32_t reserved;        /* must be 0                                     */
    int64_t env_offset;      /* global id of env 0 of this shard (native RNG) */
} MarlnavPolicyDims;

/* Device pointers of one policy call, fp32, contiguous. The ten weight and
 * bias pointers are the LIVE parameter tensors in nn.Linear's own layout
 * (weight (out, in) row-major): nothing is cached between calls. */
typedef struct MarlnavPolicyBuffers {
    const float *obs_norm;     /* (P, A, D) normalised observations           */
    /* Actor (models.py:20-25) */
    const float *actor_fc1_w;  /* (H, D)                                      */
    const float *actor_fc1_b;  /* (H,)                                        */
    const float *actor_mu_w;   /* (2, H)                                      */
    const float *actor_mu_b;   /* (2,)                                        */
    const float *actor_std_w;  /* (2, H)                                      */
    const float *actor_std_b;  /* (2,)                                        */
    /* Critic (models.py:45-49) */
    const float *critic_fc1_w; /* (H, A*D)                                    */
    const float *critic_fc1_b; /* (H,)                                        */
    const float *critic_fc2_w; /* (1, H)                                      */
    const float *critic_fc2_b; /* (1,)                                        */
    /* standard normals of dist.sample() (models.py:114), (P*A, 2); NULL:
     * drawn by the kernel from the native Philox stream */
    const float *eps;
    /* outputs */
    float *actions;            /* (P, A, 2) policy scale (before ActionScaler) */
    float *log_probs;          /* (P*A,)                                      */
    float *values;             /* (P, 1)                                      */
    float *eps_out;            /* optional (P*A, 2): the normals used         */
} MarlnavPolicyBuffers;

/* The forward-only policy work of one MAPPO.get_data step (models.py:113-120)
 * in one launch: Actor.forward (models.py:27-36: fc1 WITHOUT an activation,
 * mu = tanh(fc_mu), softplus(fc_std) used as the COVARIANCE diagonal of the
 * MultivariateNormal), dist.sample() (:114) as mu + sqrt(v) * eps,
 * dist.log_prob (:115) and Critic.forward (models.py:51-56, :120).
 * eps NULL: the kernel draws the normals, keyed by (policy_seed, step_idx,
 * global agent row (env_offset + e) * A + a), in a Philox block-index domain
 * disjoint from the re-init draws of the same seed; the result does not
 * depend on how envs are split into calls. With eps given, policy_seed and
 * step_idx are not used. */
int marlnav_policy_act(const MarlnavPolicyDims *dims, const MarlnavPolicyBuffers *bufs,
                       uint64_t policy_seed, uint64_t step_idx, void *stream);

/* The critic half of marlnav_policy_act alone: Critic.forward (models.py:
 * 51-56) of (P, A, D) normalised observations into values (P, 1), bit-identical
 * to the values marlnav_policy_act writes for the same observations and
 * weights (the bootstrap value of marlnav_gae_advantages). One launch. Reads
 * obs_norm and the four critic tensors (live); the six actor pointers, eps,
 * actions, log_probs and eps_out are ignored and may be NULL. Draws no random
 * number. */
int marlnav_critic_values(const MarlnavPolicyDims *dims, const MarlnavPolicyBuffers *bufs,
                          void *stream);

/* Device pointers of one rollout of T steps of P envs: the stacked storage of
 * the six entries MAPPO.get_data keeps per step (models.py:120), row t of each
 * being step t, plus what the call needs beside them. Contiguous; fp32 unless
 * noted. Rows may start at any offset the entry's own type allows (a row of
 * `actions` is always 8-byte aligned, as marlnav_step needs; where a row of
 * `actions` is not 16-byte aligned that step runs the env-block or the
 * generic wave kernel, which read it in 8-byte pairs, and where a row of
 * `obs` is not, that policy launch loads narrower: both bit-identical to
 * the aligned paths). */
typedef struct MarlnavRolloutBuffers {
    float *obs;                /* (T, P, A, D) normalised observations the policy
                                  read at step t (models.py:110, :113, :124)     */
    float *actions;            /* (T, P, A, 2) policy-scale actions (models.py:114) */
    float *log_probs;          /* (T, P*A)     (models.py:115)                   */
    float *values;             /* (T, P)       (models.py:120)                   */
    float *rewards;            /* (T, P)       (models.py:116)                   */
    uint8_t *done;             /* (T, P) bool: terminated | truncated (models.py:117);
                                  holds `terminated` until the merge at the end  */
    uint8_t *truncated;        /* (T, P) scratch: the steps' `truncated` flags   */
    /* optional standard normals of dist.sample() (models.py:114), row t for
     * step t; NULL: drawn by the policy kernel at policy_step_idx0 + t */
    const float *eps;          /* (T, P*A, 2)                                    */
    /* optional MAPPO._process_rewards (models.py:131-148) over rewards and done
     * with `gamma`, as marlnav_discounted_returns: all three given or all NULL */
    double *returns;           /* (T, P) fp64 out                                */
    double *returns_stats;     /* 2 fp64 out (mean, std)                         */
    double *returns_work;      /* marlnav_returns_work_size(P) fp64 scratch      */
} MarlnavRolloutBuffers;

/* MAPPO.get_data (models.py:106-125) for T steps of one env shard and, with
 * the returns pointers, _process_rewards (:131-148), enqueued on `stream` by
 * one call with no host work between the launches:
 *   marlnav_observe of the current state into env->obs, and its normalised
 *     form (obs - norm_mean[k]) / norm_scale[k] (one IEEE subtraction and one
 *     IEEE division, as the step kernels' fused ObsNormalizer) into obs row 0
 *     (models.py:110);
 *   for t = 0 .. T-1 what marlnav_policy_act enqueues on obs row t, writing
 *     actions / log_probs / values row t (eps row t, or the kernel's stream at
 *     policy_step_idx0 + t), then what marlnav_step enqueues at step index
 *     env_step_idx0 + t with actions row t, reward = rewards row t,
 *     terminated = done row t, truncated = truncated row t and obs_norm =
 *     obs row t + 1, the last step's being env->obs_norm (models.py:113-124);
 *   done[i] = (done[i] | truncated[i]) != 0 over the T*P flags (models.py:117);
 *   what marlnav_discounted_returns enqueues, when asked for.
 * env: the table of a marlnav_step call with native re-init (fresh_states
 *   NULL) and both MARLNAV_WRITE_OBS_NORM and MARLNAV_SCALE_ACTIONS set in
 *   params->flags; its actions, reward, terminated and truncated fields are
 *   ignored, obs (raw observations, overwritten every step) and obs_norm (the
 *   observations after the last step; must not overlap rollout->obs) are used.
 *   With states_out given the two state buffers swap roles every step, so the
 *   current states are in `states` after an even T and in `states_out` after
 *   an odd one; without it every step runs in place.
 * policy: the weights are read live at every step; obs_norm, eps, actions,
 *   log_probs, values and eps_out are ignored. pdims must describe the same
 *   shard: num_parallel, num_agents and env_offset of dims, obs_dim = D.
 * Everything is validated before the first launch (MARLNAV_EINVAL, the
 * message names the field). A failing launch ends the call at once with its
 * code; the message names the step, and nothing further is enqueued. */
int marlnav_rollout_collect(const MarlnavDims *dims, const MarlnavParams *params,
                            const MarlnavStepBuffers *env, uint64_t env_step_idx0,
                            const MarlnavPolicyDims *pdims, const MarlnavPolicyBuffers *policy,
                            uint64_t policy_seed, uint64_t policy_step_idx0,
                            const MarlnavRolloutBuffers *rollout, int64_t T, double gamma,
                            void *stream);

/* marlnav_actor_act modes */
#define MARLNAV_ACT_MEAN   0  /* actions = dist.loc (animation.py:48)      */
#define MARLNAV_ACT_SAMPLE 1  /* actions = dist.sample() (animation.py:46) */

/* The actor half of marlnav_policy_act alone, as the reference's rendering
 * path runs it (animation.py:40-50 with init_render :80-96, which loads only
 * the actor's weights): Actor.forward (models.py:27-36) and then dist.loc
 * (MARLNAV_ACT_MEAN: actions = tanh(fc_mu(fc1(x))), nothing else evaluated) or
 * dist.sample() (MARLNAV_ACT_SAMPLE: mu + sqrt(v) * eps, bit-identical to
 * marlnav_policy_act's actions for the same eps, or the same (policy_seed,
 * step_idx, env_offset) with eps NULL). One launch.
 * Reads obs_norm, the six actor tensors (live, nothing cached) and, in SAMPLE
 * mode, eps; writes actions and, when given, eps_out (SAMPLE mode only). The
 * four critic pointers, log_probs and values are ignored and may be NULL.
 * Every action is a function of its own row only: the result does not depend
 * on P, on the block a row lands in or on how envs are split into calls. */
int marlnav_actor_act(const MarlnavPolicyDims *dims, const MarlnavPolicyBuffers *bufs,
                      int mode, uint64_t policy_seed, uint64_t step_idx, void *stream);

/* Device pointers of one evaluation of T steps of P envs
 * (marlnav_rollout_evaluate). Contiguous; everything is written by the call,
 * nothing needs initialising. */
typedef struct MarlnavEvalBuffers {
    /* scratch the steps run through */
    float *obs_norm_a;         /* (P, A, D) normalised observations, even steps  */
    float *obs_norm_b;         /* (P, A, D) odd steps (the two alternate)        */
    float *actions;            /* (P, A, 2) policy-scale actions, 8-byte aligned */
    float *reward;             /* (P,)  the last step's (environment.py:100)     */
    uint8_t *terminated;       /* (P,)  bool, the last step's                    */
    uint8_t *truncated;        /* (P,)  bool, the last step's                    */
    /* per-env episode state: the episode under way at the end of the call */
    double *cur_return;        /* (P,)  sum of its rewards so far                */
    int32_t *cur_len;          /* (P,)  its steps so far                         */
    uint8_t *whole;            /* (P,)  it started inside the call (or the env
                                  entered the call with step_num == 0)          */
    /* per-env results over the episodes that ended inside the call and were
     * whole; an env that entered the call mid-episode closes a partial one */
    int32_t *ep_count;         /* (P,)                                           */
    double *ret_sum;           /* (P,)  sum of the episode returns               */
    double *ret_sqsum;         /* (P,)  sum of their squares                     */
    double *ret_min;           /* (P,)  +inf without an episode                  */
    double *ret_max;           /* (P,)  -inf without an episode                  */
    int64_t *len_sum;          /* (P,)  sum of the episode lengths               */
    int32_t *partial_count;    /* (P,)  0 or 1                                   */
    /* totals over the envs (one block, fixed order) */
    int64_t *totals_i;         /* 3: episodes, partials, len_sum                 */
    double *totals_f;          /* 4: ret_sum, ret_sqsum, min, max                */
    /* optional record of env trace_env (all NULL when trace_env < 0): row 0
     * the state before the first step (Animation.__init__), row t + 1 the
     * state after step t, finished envs showing their fresh state */
    float *trace_states;       /* (T+1, A, 5)                                    */
    float *trace_obstacles;    /* (T+1, S, 2)                                    */
    float *trace_target;       /* (T+1, 2)                                       */
    float *trace_reward;       /* (T,)                                           */
    uint8_t *trace_terminated; /* (T,)  bool                                     */
    uint8_t *trace_truncated;  /* (T,)  bool                                     */
    int64_t trace_env;         /* local env index in [0, P), or -1: no trace     */
    int64_t reserved;          /* must be 0                                      */
} MarlnavEvalBuffers;

/* The reference's policy rendering loop (animation.py:40-71: normalise the
 * observations, Actor.forward, dist.loc or dist.sample(), ActionScaler,
 * Env.step) for T steps of one env shard without the drawing, with the
 * episode figures an evaluation reports, enqueued on `stream` by one call
 * with no host work between the launches:
 *   marlnav_observe of the current state into env->obs and its normalised
 *     form into obs_norm_a (as marlnav_rollout_collect's row 0);
 *   the tracker's start: every per-env array zero, ret_min = +inf, ret_max =
 *     -inf, whole[p] = (step_num[p] == 0); trace row 0;
 *   for t = 0 .. T-1 what marlnav_actor_act enqueues in `mode` (SAMPLE: the
 *     kernel's own normals at policy_step_idx0 + t) from the observations of
 *     step t into `actions`, what marlnav_step enqueues at env_step_idx0 + t,
 *     writing the other obs_norm buffer, then the tracker:
 *       cur_return += (double)reward[p]; cur_len += 1;
 *       if terminated[p] | truncated[p]  (the `done` of models.py:117):
 *         whole[p] ? (ep_count += 1, ret_sum += cur_return,
 *                     ret_sqsum += cur_return * cur_return (one product and
 *                     one sum, rounded separately), len_sum += cur_len,
 *                     min / max updated)
 *                  : partial_count += 1;
 *         cur_return = 0, cur_len = 0, whole = 1
 *     and trace row t + 1, read from the state buffer that step wrote;
 *   the totals. With no whole episode totals_f[2..3] stay +inf / -inf.
 * Every per-env number is a function of its own env's rewards in step order.
 * env, policy, pdims: as for marlnav_rollout_collect (native re-init, both
 *   MARLNAV_WRITE_OBS_NORM and MARLNAV_SCALE_ACTIONS, the state buffers
 *   swapping per step with states_out); env->obs_norm is not used, and of
 *   `policy` only the six actor tensors are read.
 * Everything is validated before the first launch (MARLNAV_EINVAL, the
 * message names the field). A failing launch ends the call at once. */
int marlnav_rollout_evaluate(const MarlnavDims *dims, const MarlnavParams *params,
                             const MarlnavStepBuffers *env, uint64_t env_step_idx0,
                             const MarlnavPolicyDims *pdims, const MarlnavPolicyBuffers *policy,
                             int mode, uint64_t policy_seed, uint64_t policy_step_idx0,
                             const MarlnavEvalBuffers *eval, int64_t T, void *stream);

/* Shapes of one PPO minibatch: rows lo..hi of a stacked rollout, T = hi - lo
 * steps of P envs. N = T*P env rows, M = N*A agent rows in (t, p, a) order. */
typedef struct MarlnavPpoDims {
    int64_t num_parallel;    /* P  envs per step                              */
    int64_t num_steps;       /* T  steps in the minibatch, >= 1, T*P >= 2     */
    int32_t num_agents;      /* A  2 <= A <= 64                               */
    int32_t obs_dim;         /* D  features per agent row                     */
    int32_t hidden_size;     /* H  1 <= H <= 512                              */
    int32_t reserved;        /* must be 0                                     */
} MarlnavPpoDims;

/* Device pointers of one PPO call, contiguous; fp32 unless noted. The data
 * pointers address step `lo` of the stacked rollout storage; the ten weight
 * pointers are the LIVE parameter tensors (nn.Linear layout), the ten
 * gradient pointers their fp32 .grad tensors of the same shapes, which the
 * call OVERWRITES (zero_grad() + backward()). */
typedef struct MarlnavPpoBuffers {
    const float *obs;          /* (T, P, A, D) normalised observations        */
    const float *actions;      /* (T, P, A, 2) policy-scale actions           */
    const float *log_probs;    /* (T, P*A) log-probs at collection time       */
    const float *values;       /* (T, P) critic values at collection time     */
    const double *returns;     /* (T, P) fp64 normalised returns              */
    const float *actor_fc1_w;  /* weights as in MarlnavPolicyBuffers          */
    const float *actor_fc1_b;
    const float *actor_mu_w;
    const float *actor_mu_b;
    const float *actor_std_w;
    const float *actor_std_b;
    const float *critic_fc1_w;
    const float *critic_fc1_b;
    const float *critic_fc2_w;
    const float *critic_fc2_b;
    float *grad_actor_fc1_w;   /* gradients, the shapes of the weights        */
    float *grad_actor_fc1_b;
    float *grad_actor_mu_w;
    float *grad_actor_mu_b;
    float *grad_actor_std_w;
    float *grad_actor_std_b;
    float *grad_critic_fc1_w;
    float *grad_critic_fc1_b;
    float *grad_critic_fc2_w;
    float *grad_critic_fc2_b;
    double *loss;              /* 1 fp64 out                                  */
    double *work;              /* marlnav_ppo_work_size(dims) fp64 scratch    */
} MarlnavPpoBuffers;

/* fp64 elements of MarlnavPpoBuffers.work for these dims (enough for either
 * call); negative on bad dims. */
int64_t marlnav_ppo_work_size(const MarlnavPpoDims *dims);

/* MAPPO._actor_loss (models.py:270-299) of one minibatch and the gradient of
 * every actor parameter, as zero_grad() + loss.backward() leave them
 * (models.py:173-175). Quirks kept: softplus(fc_std) is the covariance
 * diagonal; the advantage of agent row i is returns[i mod N] - values[i mod N]
 * (the reference's repeat(num_agents) on the (t, p) vectors), in fp64; the
 * clip bounds 1 -+ epsilon and ent_const act as fp32 scalars on fp32 tensors;
 * the clipped mean is summed in fp64. Reads obs, actions, log_probs, values,
 * returns, the six actor weights; writes the six actor gradients and loss.
 * Fixed reduction order, no atomics: equal inputs give equal bits. */
int marlnav_ppo_actor_grad(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                           double epsilon, double ent_const, void *stream);

/* MAPPO._critic_loss (models.py:301-316) of one minibatch and the gradient of
 * every critic parameter (models.py:193-195). Reads obs, values, returns, the
 * four critic weights; writes the four critic gradients and loss. */
int marlnav_ppo_critic_grad(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                            double epsilon, void *stream);

/* One Adam step over up to MARLNAV_ADAM_MAX_TENSORS parameter tensors of one
 * network: torch.optim.Adam (models.py:71-74) with weight_decay = 0 and
 * amsgrad = False. */
#define MARLNAV_ADAM_MAX_TENSORS 8

typedef struct MarlnavAdamDims {
    int32_t num_tensors;     /* used slots, 1..MARLNAV_ADAM_MAX_TENSORS       */
    int32_t maximize;        /* 0: descend, 1: ascend (the actor's optimiser) */
    int64_t numel[MARLNAV_ADAM_MAX_TENSORS]; /* elements per used slot, >= 1  */
    double lr, beta1, beta2, eps; /* lr >= 0, betas in [0, 1), eps >= 0       */
    int64_t reserved;        /* must be 0                                     */
} MarlnavAdamDims;

/* Device pointers of one Adam step, fp32, contiguous, numel[i] elements each;
 * any 4-byte alignment (a slot whose four pointers are all 16-byte aligned
 * takes the vector path). The slots must not overlap. */
typedef struct MarlnavAdamBuffers {
    float *param[MARLNAV_ADAM_MAX_TENSORS];       /* updated in place         */
    /* read only, except by the `_clipped` calls below, which WRITE the
     * clipped gradient back through these pointers */
    const float *grad[MARLNAV_ADAM_MAX_TENSORS];
    float *exp_avg[MARLNAV_ADAM_MAX_TENSORS];     /* first moment, in place   */
    float *exp_avg_sq[MARLNAV_ADAM_MAX_TENSORS];  /* second moment, in place  */
    /* marlnav_adam_state_size() bytes, 8-byte aligned: the int64 step count
     * (the first 8 bytes; all zero = no step taken yet) and the step's
     * scalars derived from it. Owned by the library between calls. */
    void *state;
} MarlnavAdamBuffers;

/* Bytes of MarlnavAdamBuffers.state. */
int64_t marlnav_adam_state_size(void);

/* One optimiser step. With k the count in `state` after this call's
 * increment and g = maximize ? -grad : grad:
 *   m = beta1 m + (1 - beta1) g         v = beta2 v + (1 - beta2) g^2
 *   p -= lr / (1 - beta1^k) * m / (sqrt(v) / sqrt(1 - beta2^k) + eps)
 * The bias corrections are evaluated in fp64 from the device count; every
 * element is updated in fp64 and m, v, p are rounded to fp32 once on the
 * store. Two launches on `stream`: one thread advances the count and
 * publishes the step's scalars, then thread = 4 elements over all slots. No
 * synchronisation, no host copy of the count (a captured graph replays
 * correctly), no atomics: equal inputs give equal bits. lr, the betas, eps
 * and maximize travel as launch arguments: a captured graph keeps the values
 * of capture time. */
int marlnav_adam_step(const MarlnavAdamDims *dims, const MarlnavAdamBuffers *bufs,
                      void *stream);

/* One minibatch update in one call: what marlnav_ppo_actor_grad /
 * marlnav_ppo_critic_grad enqueue, then marlnav_adam_step over that network's
 * tensors, all on `stream`. The Adam table must be that network's: param[i],
 * grad[i] and numel[i] equal the weights, the grad_ pointers and the sizes of
 * `bufs` in declaration order (six slots for the actor, four for the critic);
 * anything else is MARLNAV_EINVAL before any launch. */
int marlnav_ppo_actor_update(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                             double epsilon, double ent_const,
                             const MarlnavAdamDims *adam_dims,
                             const MarlnavAdamBuffers *adam_bufs, void *stream);
int marlnav_ppo_critic_update(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                              double epsilon, const MarlnavAdamDims *adam_dims,
                              const MarlnavAdamBuffers *adam_bufs, void *stream);

/* One whole MAPPO.train_actor / train_critic (models.py:160-198) in one call:
 * num_epochs x num_batches minibatch updates enqueued back to back on
 * `stream`, epoch-major, with no synchronisation and no allocation.
 *   network     MARLNAV_NETWORK_ACTOR or MARLNAV_NETWORK_CRITIC
 *   dims        P, A, D, H of the rollout buffer; num_steps = its stored steps
 *   bufs        as for marlnav_ppo_*_update, the data pointers addressing
 *               step 0 of the stacked storage; `loss` is not used; `work` has
 *               marlnav_ppo_train_work_size(dims, bounds, num_batches) doubles
 *   bounds      host array of num_batches (lo, hi) pairs: minibatch j is
 *               steps lo..hi-1, 0 <= lo < hi <= num_steps
 *   adam        the network's own table, checked as marlnav_ppo_*_update does
 *   loss_log    device, num_epochs * num_batches doubles: update k (epoch e,
 *               batch j: k = e * num_batches + j) writes its loss to [k]
 * Update k stores what marlnav_ppo_*_update on steps lo..hi stores, bit for
 * bit: loss, every .grad, parameters, both moments, the step count. Where it
 * was measured to be faster (an actor of up to 1024 elements, a critic
 * minibatch of up to 2^17 env rows) it takes fewer launches: one thread of the
 * gradient pass advances the count and publishes the step's scalars, and the
 * finish launch, which follows in stream order, applies the Adam element
 * update to each element as it stores its gradient (2 launches for the actor,
 * 2-3 for the critic); elsewhere it enqueues the launches of
 * marlnav_ppo_*_update. ent_const is ignored for the critic. Everything is
 * validated before the first launch (MARLNAV_EINVAL, the message names the
 * field). */
#define MARLNAV_NETWORK_ACTOR 0
#define MARLNAV_NETWORK_CRITIC 1
int marlnav_ppo_train_phase(int network, const MarlnavPpoDims *dims,
                            const MarlnavPpoBuffers *bufs, const int64_t *bounds,
                            int64_t num_batches, int64_t num_epochs, double epsilon,
                            double ent_const, const MarlnavAdamDims *adam_dims,
                            const MarlnavAdamBuffers *adam_bufs, double *loss_log, void *stream);

/* The three actor-side calls above with the pairing of advantages to agent
 * rows as an argument.
 *   MARLNAV_ADVANTAGE_REFERENCE  the advantage of agent row i is
 *     returns[i mod N] - values[i mod N]: each call stores exactly what its
 *     counterpart without `_mode` stores.
 *   MARLNAV_ADVANTAGE_ENV  the advantage of agent row i is returns[i / A], the
 *     row's own (t, p), read as a ready fp64 advantage (the normalised
 *     `advantages` of marlnav_gae_advantages). `values` is not read by the
 *     actor and may be NULL. Everything else about the loss and the gradients
 *     is unchanged, and so are the folded-Adam variants and their two limits.
 * The critic has no pairing: marlnav_ppo_train_phase_mode with
 * MARLNAV_NETWORK_CRITIC validates advantage_mode and is otherwise
 * marlnav_ppo_train_phase (in the GAE mode its `returns` pointer addresses
 * the value_targets). Any other advantage_mode is MARLNAV_EINVAL before any
 * launch. */
#define MARLNAV_ADVANTAGE_REFERENCE 0
#define MARLNAV_ADVANTAGE_ENV 1
int marlnav_ppo_actor_grad_mode(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                                double epsilon, double ent_const, int advantage_mode,
                                void *stream);
int marlnav_ppo_actor_update_mode(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                                  double epsilon, double ent_const,
                                  const MarlnavAdamDims *adam_dims,
                                  const MarlnavAdamBuffers *adam_bufs, int advantage_mode,
                                  void *stream);
int marlnav_ppo_train_phase_mode(int network, const MarlnavPpoDims *dims,
                                 const MarlnavPpoBuffers *bufs, const int64_t *bounds,
                                 int64_t num_batches, int64_t num_epochs, double epsilon,
                                 double ent_const, const MarlnavAdamDims *adam_dims,
                                 const MarlnavAdamBuffers *adam_bufs, double *loss_log,
                                 int advantage_mode, void *stream);

/* fp64 elements of `work` that cover the largest minibatch of the list;
 * negative on bad dims or bounds. */
int64_t marlnav_ppo_train_work_size(const MarlnavPpoDims *dims, const int64_t *bounds,
                                    int64_t num_batches);

/* Global-norm gradient clipping inside the update: what
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) does between
 * backward() and optimizer.step(), with error_if_nonfinite=False. For one
 * network's Adam table and max_norm:
 *   S    = sum over all slots, all elements of (double)g^2   fp64, fixed order
 *   norm = sqrt(S)
 *   coef = min(1.0, max_norm / (norm + 1e-6))                fp64; torch's formula
 *   g'   = (float)((double)g * coef)                         stored back into .grad
 *   Adam = the element update of marlnav_adam_step from the stored, rounded g'
 * .grad holds the clipped gradient afterwards: these calls WRITE through
 * MarlnavAdamBuffers.grad although it is declared const float *. coef == 1.0
 * (a norm below max_norm - 1e-6, a zero gradient, max_norm = +inf) leaves
 * every bit of .grad, the parameters, the moments and the count equal to the
 * unclipped call's. max_norm must be > 0 and not NaN; +inf is allowed and
 * means "record the norm, clip nothing". A non-finite gradient gives a
 * non-finite norm and coefficient and poisons the step, as clip_grad_norm_'s
 * default does; nothing special-cases it.
 *
 * Reduction order, fixed, no atomics, equal inputs give equal bits: the
 * table's elements are cut into items of 4 in table order as for
 * marlnav_adam_step; a thread forms the fp64 sum of its item's <= 4 squares
 * in element order; blocks of 256 consecutive items are summed wave by wave
 * (a fixed shuffle tree, the four waves in order) into one partial per block,
 * stored to norm_work in block order; the second stage is one block of 256
 * threads, thread t summing partials t, t + 256, ... in that order, then the
 * same block sum. The order does not depend on the launch path or on the
 * slots' alignment.
 *
 * Three launches on `stream` after the gradient launches: the square sums;
 * one block that reduces the partials, publishes coef in the state block
 * (its last 8 bytes, which marlnav_adam_step never reads), writes *norm_out
 * and then advances the count; the element update. max_norm travels as a
 * launch argument: a captured graph keeps the value of capture time.
 *   norm_work  device, marlnav_grad_norm_work_size(dims) doubles, 8-byte
 *              aligned, owned by the call while it runs on the stream
 *   norm_out   device double, 8-byte aligned, or NULL: the norm BEFORE clipping
 *   norm_log   (train phase) device, num_epochs * num_batches doubles or NULL:
 *              update k writes [k]
 * Each call makes every check of its unclipped counterpart
 * (marlnav_adam_step, marlnav_ppo_actor_update_mode,
 * marlnav_ppo_critic_update, marlnav_ppo_train_phase_mode) and those of
 * max_norm, norm_work and norm_out / norm_log before the first launch
 * (MARLNAV_EINVAL, the message names the field). The clipped phase never
 * takes the unclipped phase's folded finish launches (those kernels update
 * elements before the norm exists): an update is the gradient launches of
 * marlnav_ppo_*_grad and the three above, except for an actor of up to 1024
 * elements, whose one-block finish launch forms the norm in the same order
 * and updates behind a block barrier (marlnav_debug_clip_fold below). Either
 * way it stores what marlnav_ppo_*_update_clipped on the same steps stores,
 * bit for bit. */
int64_t marlnav_grad_norm_work_size(const MarlnavAdamDims *dims); /* < 0: bad dims */
int marlnav_adam_step_clipped(const MarlnavAdamDims *dims, const MarlnavAdamBuffers *bufs,
                              double max_norm, double *norm_work, double *norm_out,
                              void *stream);
int marlnav_ppo_actor_update_clipped(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                                     double epsilon, double ent_const,
                                     const MarlnavAdamDims *adam_dims,
                                     const MarlnavAdamBuffers *adam_bufs, int advantage_mode,
                                     double max_norm, double *norm_work, double *norm_out,
                                     void *stream);
int marlnav_ppo_critic_update_clipped(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                                      double epsilon, const MarlnavAdamDims *adam_dims,
                                      const MarlnavAdamBuffers *adam_bufs, double max_norm,
                                      double *norm_work, double *norm_out, void *stream);
int marlnav_ppo_train_phase_clipped(int network, const MarlnavPpoDims *dims,
                                    const MarlnavPpoBuffers *bufs, const int64_t *bounds,
                                    int64_t num_batches, int64_t num_epochs, double epsilon,
                                    double ent_const, const MarlnavAdamDims *adam_dims,
                                    const MarlnavAdamBuffers *adam_bufs, double *loss_log,
                                    int advantage_mode, double max_norm, double *norm_work,
                                    double *norm_log, void *stream);

/* Testing and measurement hook (not part of the reference's interface):
 * whether marlnav_ppo_train_phase_clipped takes the in-block fold for an actor
 * of up to 1024 elements: actor_finish, one block, re-reads
 * the gradients it has stored in the reduction order above, forms the norm
 * and the coefficient in-block and then updates, two launches per update in
 * place of five, with the same stored bits. Process-wide; 0 or 1 sets it, any
 * other value only queries; returns the previous setting. The default,
 * MARLNAV_CLIP_FOLD_DEFAULT, is the measured decision: on (1.1-2.4 us per
 * update below the five launches at 854 elements, more than the spread of
 * the repetitions, in both runs of scripts/clip_bench.py). */
#define MARLNAV_CLIP_FOLD_DEFAULT 1
int marlnav_debug_clip_fold(int on);

/* Actor diagnostics and the target-KL stop, on the device.
 * The diagnostic form of the actor's gradient launches adds two fp64 sums to
 * the pass (through the reduction that carries the loss sums) and writes one
 * row of MARLNAV_DIAG_ROW doubles per update:
 *   [0] surrogate_mean  the clipped-surrogate mean (the loss's first term)
 *   [1] entropy_mean    the entropy's fp64 mean;
 *                       loss == [0] + (double)((float)ent_const * (float)[1])
 *   [2] approx_kl       mean of ((double)ratio - 1.0) - (double)lr per row, the
 *                       k3 estimator (r - 1) - log r with lr the fp32
 *                       new_log_prob - log_prob whose expf is the fp32 ratio
 *   [3] clip_frac       the fraction of rows with ratio outside the fp32 bounds
 *                       [1 - epsilon, 1 + epsilon] (a NaN ratio is outside)
 *   [4] status          0.0 applied, 1.0 the update that raised the stop,
 *                       2.0 an update behind the stop
 * loss and every .grad element carry the bits of the plain call: the new
 * accumulators touch none of the existing ones. The pass's partial rows are two
 * doubles longer: `work` has marlnav_ppo_diag_work_size(dims) doubles, for the
 * phase marlnav_ppo_train_diag_work_size(dims, bounds, num_batches) (never
 * less than the plain queries' values; negative on bad arguments).
 *
 * marlnav_ppo_actor_grad_diag: marlnav_ppo_actor_grad_mode plus `diag` (device,
 * 8-byte aligned). No stop: status is 0.
 *
 * marlnav_ppo_train_phase_monitored: the actor's marlnav_ppo_train_phase_mode /
 * _clipped with the row of every update in diag_log and the stop.
 *   network    MARLNAV_NETWORK_ACTOR; the critic is refused
 *   max_norm   as for _clipped, or MARLNAV_MAX_NORM_NONE: no clip, the two
 *              launches of marlnav_adam_step; norm_work and norm_log NULL then
 *   target_kl  > 0; +inf: monitor only, no update ever stops (status 0 always)
 *   diag_log   device, num_epochs * num_batches rows, update k writes row k
 *   stop       device, 2 int64: {flag, stopped_at}. The call's first launch
 *              resets it to {0, -1}; whatever it held before is ignored
 * In the finish launch of update k one thread evaluates !(approx_kl <=
 * target_kl), so a NaN KL stops. The comparison is with target_kl itself:
 * a caller who wants Stable-Baselines3's rule passes 1.5 x its target. The
 * stop sits before the optimiser step, as there:
 *   status 0  loss, row and .grad stored; the Adam step (clipped where asked)
 *             applied. Bit for bit the plain phase's update.
 *   status 1  loss, row and .grad stored; stop = {1, k}; NO Adam step:
 *             parameters, moments, count, step scalars, the clip's coefficient
 *             cell and norm_log[k] stay as they were
 *   status 2  every later update of the call: loss_log[k] and row k are NaN but
 *             for status; .grad, parameters, moments, count, norm_log[k] stay
 * Every launch of an update behind the stop reads the flag, which an earlier
 * launch wrote, and returns: such an update costs its launches, not work. No
 * atomics and no host read; a captured graph replays the decision. An update
 * is the two gradient launches and the gated forms of marlnav_adam_step's two
 * (or _clipped's three); nothing is folded. Everything is validated before the
 * first launch (MARLNAV_EINVAL, the message names the field). */
#define MARLNAV_DIAG_ROW 5
#define MARLNAV_MAX_NORM_NONE 0.0
int64_t marlnav_ppo_diag_work_size(const MarlnavPpoDims *dims);
int64_t marlnav_ppo_train_diag_work_size(const MarlnavPpoDims *dims, const int64_t *bounds,
                                         int64_t num_batches);
int marlnav_ppo_actor_grad_diag(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                                double epsilon, double ent_const, int advantage_mode,
                                double *diag, void *stream);
int marlnav_ppo_train_phase_monitored(int network, const MarlnavPpoDims *dims,
                                      const MarlnavPpoBuffers *bufs, const int64_t *bounds,
                                      int64_t num_batches, int64_t num_epochs, double epsilon,
                                      double ent_const, const MarlnavAdamDims *adam_dims,
                                      const MarlnavAdamBuffers *adam_bufs, double *loss_log,
                                      int advantage_mode, double max_norm, double *norm_work,
                                      double *norm_log, double target_kl, double *diag_log,
                                      int64_t *stop, void *stream);

/* Shuffled minibatches: the gradient launches over a list of
 * steps, an on-device permutation generator, and a training phase that draws
 * a fresh permutation of all stored steps per epoch. Additions only; the
 * calls above and their kernels are untouched.
 *
 * marlnav_ppo_actor_grad_steps / marlnav_ppo_critic_grad_steps: the gradient
 * calls above over the minibatch whose logical step slot s is step steps[s] of
 * the storage.
 *   dims->num_steps  T, the steps of the minibatch (the table's entries)
 *   bufs             obs, actions, log_probs, values and returns address step 0
 *                    of the storage; everything else as for the plain calls
 *   steps            device, T int32, 4-byte aligned. Every entry must lie in
 *                    [0, stored steps): the library cannot check a device table
 *                    without a synchronisation and does not. Duplicates are fine
 *   diag             NULL, or as for marlnav_ppo_actor_grad_diag (`work` then has
 *                    marlnav_ppo_diag_work_size(dims) doubles)
 * Logical row (slot, p, a) is the agent row of step steps[slot]; the means,
 * both pairings, the tiles and every reduction order are those of the plain
 * call over the logical order. So the call stores, bit for bit, what the plain
 * call stores on a storage gathered with index_select(0, steps).
 *
 * marlnav_minibatch_permutations: one launch that writes E permutations of
 * [0, L) into table (device, E x L int32), 1 <= L <= 65535, 1 <= E <= 65535.
 *   seed     enters through its splitmix64 finalisation m, as the step's seed
 *   network  MARLNAV_NETWORK_*: the two networks draw different permutations
 *   counter  device, one uint64, 8-byte aligned: the call counter c. Every
 *            thread reads it; behind a block barrier one thread stores c + 1. A
 *            captured graph therefore draws new permutations at every replay
 * Row e is a Fisher-Yates over the identity: for i = L - 1 down to 1, draw
 * number n = L - 1 - i is word n & 1 of Philox2x32-10 with the counter words
 * (e << 16 | n >> 1, lo32(c)) under the key
 *   (uint32)m ^ fmix32((0x5045524D + network) * 0x9E3779B1 + hi32(c) * 0x85EBCA77
 *                      + hi32(m))
 * (fmix32: murmur3's finaliser), j = (uint64)word * (i + 1) >> 32, and row[i],
 * row[j] are swapped. The multiply-shift is biased by at most L / 2^32 per
 * draw (1.6e-5 at L = 65535, which is why a longer buffer is refused).
 * tests/shuffle_ref.py restates it.
 *
 * marlnav_ppo_train_phase_shuffled: one train_actor / train_critic with fresh
 * minibatches per epoch. dims and bufs describe the whole buffer of L =
 * dims->num_steps stored steps. Epoch e uses row e of the table; minibatch j <
 * L / batch_size of it is entries [j batch_size, (j + 1) batch_size), the last
 * one extended by the L % batch_size left over: every stored step is used
 * exactly once per epoch. num_epochs * (L / batch_size) updates, logged as by
 * the other phase calls.
 *   max_norm, norm_work, norm_log   as for _monitored (MARLNAV_MAX_NORM_NONE: off)
 *   target_kl, diag_log, stop       0, NULL, NULL: off, and the critic is
 *                                   allowed; else as for _monitored (actor only)
 *   seed, counter, table            as for marlnav_minibatch_permutations; table
 *                                   has num_epochs x L entries and holds the
 *                                   phase's permutations afterwards
 *   work    marlnav_ppo_train_shuffled_work_size(dims, batch_size, diag != 0)
 * Every check is made before the first launch; then the permutation launch
 * and the updates are enqueued. An update is the gather gradient launches and
 * marlnav_adam_step's launches (the clipped three with max_norm, the gated
 * forms with the monitor): this phase has no folded finish variants. */
int marlnav_ppo_actor_grad_steps(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                                 const int32_t *steps, double epsilon, double ent_const,
                                 int advantage_mode, double *diag, void *stream);
int marlnav_ppo_critic_grad_steps(const MarlnavPpoDims *dims, const MarlnavPpoBuffers *bufs,
                                  const int32_t *steps, double epsilon, void *stream);
int marlnav_minibatch_permutations(int64_t L, int64_t E, uint64_t seed, int network,
                                   uint64_t *counter, int32_t *table, void *stream);
int64_t marlnav_ppo_train_shuffled_work_size(const MarlnavPpoDims *dims, int64_t batch_size,
                                             int diag);
int marlnav_ppo_train_phase_shuffled(int network, const MarlnavPpoDims *dims,
                                     const MarlnavPpoBuffers *bufs, int64_t batch_size,
                                     int64_t num_epochs, double epsilon, double ent_const,
                                     const MarlnavAdamDims *adam_dims,
                                     const MarlnavAdamBuffers *adam_bufs, double *loss_log,
                                     int advantage_mode, double max_norm, double *norm_work,
                                     double *norm_log, double target_kl, double *diag_log,
                                     int64_t *stop, uint64_t seed, uint64_t *counter,
                                     int32_t *table, void *stream);

/* The checkpoint rule of MAPPO.get_data (models.py:127-129) on the device: if
 * *mean_rew > *max_rew (fp64; a NaN mean is not greater), copy src[i] to
 * dst[i] (numel[i] fp32 elements, any 4-byte alignment, i < num_tensors <=
 * MARLNAV_SNAPSHOT_MAX_TENSORS), add 1 to save_state[0], set save_state[1] =
 * repeat_index and, with track_best = 1, *max_rew = *mean_rew. The reference
 * never updates its maximum (track_best = 0: every rollout with a non-NaN
 * mean saves). src, dst, numel are host arrays; mean_rew, max_rew and
 * save_state (2 int64) are device pointers, 8-byte aligned. Two launches: the
 * copy, then one bookkeeping thread, so no block reads a decision written in
 * its own launch. */
#define MARLNAV_SNAPSHOT_MAX_TENSORS 10
int marlnav_params_snapshot_if(int num_tensors, const float *const *src, float *const *dst,
                               const int64_t *numel, const double *mean_rew, double *max_rew,
                               int64_t *save_state, int64_t repeat_index, int track_best,
                               void *stream);

/* Testing hook (not part of the reference's interface): restrict the step /
 * observe kernel selection to one family, process-wide. 0 = automatic (the
 * default); a family that does not support the call's shape or buffer
 * alignment falls back to the generic wave kernel. Returns the previous
 * setting. */
#define MARLNAV_FAMILY_AUTO 0
#define MARLNAV_FAMILY_BLOCK 1 /* env-block kernel (compiled shapes)          */
#define MARLNAV_FAMILY_SPLIT 2 /* pair-split kernel (compiled shapes)         */
/* 3 was the wave-tile family of ABI 1 (retired in ABI 2) */
#define MARLNAV_FAMILY_WAVE 4  /* generic wave kernel (any shape)             */
int marlnav_debug_force_family(int family);

/* Family (MARLNAV_FAMILY_*) the last marlnav_step / marlnav_observe call on
 * this thread launched. */
int marlnav_debug_last_family(void);

/* Testing hook (not part of the reference's interface): the env-block step
 * kernel also exists with its launch-invariant choices compiled in (every
 * block full, native non-noisy re-init from a formation, no fused normaliser,
 * no action scaler, default bond parameters, counters present), and
 * marlnav_step launches that instantiation exactly when all of them hold.
 * This restricts the choice, process-wide: AUTO (the default); GENERAL: never
 * the specialised instantiation; FIXED_NO_DRAW: the specialised one whenever
 * eligible, without the draw wave that grids of at most one block per
 * compute unit otherwise add. Returns the previous setting, MARLNAV_EINVAL
 * for an unknown mode. */
#define MARLNAV_BLOCK_TRAITS_AUTO 0
#define MARLNAV_BLOCK_TRAITS_GENERAL 1
#define MARLNAV_BLOCK_TRAITS_FIXED_NO_DRAW 2
int marlnav_debug_force_block_traits(int mode);

/* What the last marlnav_step call on this thread launched: GENERAL (also for
 * the other kernel families), FIXED (the specialised env-block step) or
 * FIXED_DRAW (the same with the draw wave). */
#define MARLNAV_BLOCK_RAN_GENERAL 0
#define MARLNAV_BLOCK_RAN_FIXED 1
#define MARLNAV_BLOCK_RAN_FIXED_DRAW 2
int marlnav_debug_last_block_traits(void);

/* Testing hook (not part of the reference's interface): the step kernels'
 * bearing acos (environment.py:286) of the n consecutive fp32 bit patterns
 * from `first`, into the device array out[n] (tests/golden/acos_dev_check.py
 * compares it with the oracle's restatement over every fp32 in [-1, 1]). */
int marlnav_debug_acos_range(uint32_t first, int64_t n, float *out, void *stream);

/* Testing hook (not part of the reference's interface): the step kernels'
 * short fp32 division sequences (one Newton step, one residual correction:
 * the normalisation's two quotients, the reward terms' divisions by a
 * parameter, the bond term's reciprocal) against IEEE division, for the nd
 * divisor significands d_first + k * d_stride in [1, 2) and every dividend
 * significand; adds the mismatch counts to the device array out[3]
 * (quotients, parameter divisions, reciprocals). All-zero over the 2^23
 * divisors is the exhaustive proof (scripts/probes/div_exhaustive.hip). */
int marlnav_debug_fastdiv_check(uint32_t d_first, uint32_t d_stride, uint32_t nd, uint64_t *out,
                                void *stream);

/* Message of the last failing call on this thread. */
const char *marlnav_last_error(void);

/* MARLNAV_ABI_VERSION of the built library. */
int marlnav_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* MARLNAV_H */
