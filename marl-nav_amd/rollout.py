"""Device-side rollout helpers for the training loop that drives Env.step
(SURVEY.md §8(f) row 3): MAPPO._process_rewards (marlnav/models.py:131-148)
as one HIP scan instead of a Python loop of T x 3 small tensor ops.

* ``discounted_returns(rewards, done, gamma)`` - stacked (T, P) rollout ->
  normalized float64 returns, mean, std (libmarlnav.so
  ``marlnav_discounted_returns``).
* ``process_rewards(buffer, gamma)`` - the reference's list buffer
  (``[obs, actions, log_probs, values, rewards, done]`` per step) updated in
  place exactly as ``MAPPO._process_rewards`` does; returns the mean.
* ``mappo_process_rewards(mappo)`` - drop-in body for the method (logs and
  prints like the reference).
* ``RolloutBuffer`` - preallocated stacked device storage for those six
  entries, so no per-step Python list growth and no stacking before the scan.
* ``FusedPolicy(actor, critic)`` - the forward-only policy work of
  ``MAPPO.get_data`` (models.py:113-120: ``Actor.forward``, the
  ``MultivariateNormal``'s ``sample`` and ``log_prob``, ``Critic.forward``) as
  one launch of libmarlnav.so ``marlnav_policy_act`` on the modules' live
  parameter tensors.
* ``gae_advantages(rewards, done, values, last_values, gamma, lam)`` - the
  opt-in GAE(lambda) estimator (libmarlnav.so ``marlnav_gae_advantages``,
  DESIGN.md §15), ``RolloutBuffer.process_gae``, ``FusedPolicy.values`` (the
  bootstrap value) and ``FusedPPO(..., advantage='gae')``; ``collect`` /
  ``collect_fused`` take ``gae_lambda``.
* ``collect(env, policy, buffer)`` - the ``get_data`` loop (models.py:106-125)
  around ``Env.step`` with no ``torch.nn`` / ``torch.distributions`` call in it.
* ``collect_fused(env, policy, buffer)`` - the same rollout enqueued by one C
  call (libmarlnav.so ``marlnav_rollout_collect``): the step kernels write
  their normalised observations straight into the buffer's rows.
* ``FusedPPO(actor, critic, epsilon, ent_const)`` - ``MAPPO._actor_loss`` /
  ``_critic_loss`` (models.py:270-316) of one minibatch with the gradient of
  every parameter written to ``.grad`` (libmarlnav.so
  ``marlnav_ppo_actor_grad`` / ``marlnav_ppo_critic_grad``), and
  ``train_actor`` / ``train_critic`` / ``minibatch_bounds``, the loops of
  models.py:160-198 around them and the caller's ``torch.optim`` optimiser.
* ``FusedAdam(params, lr, betas, eps, maximize)`` - ``torch.optim.Adam`` as
  the reference constructs it (models.py:71-74) in one launch over all of a
  network's parameters with the step count on the device (libmarlnav.so
  ``marlnav_adam_step``). Given one, ``train_actor`` / ``train_critic`` issue a
  whole minibatch update (loss, gradients, Adam) as one C call
  (``FusedPPO.actor_update`` / ``critic_update``), and an epoch of them can be
  captured in a graph and replayed.

Numerics: float64 like the reference (its accumulator is
``torch.zeros(P, dtype=float)``); the returns recursion is evaluated in the
same order; mean and unbiased std are fixed-order two-pass reductions (torch
uses a Welford reduction), so they agree with the reference to ~1e-15
relative, not bit for bit.
"""
import ctypes

import torch

from . import abi

_F64 = torch.float64


def _stream(device):
    return torch._C._cuda_getCurrentRawStream(device.index)


def discounted_returns(rewards, done, gamma):
    """rewards (T, P) float32, done (T, P) bool, on one HIP device. Returns
    (returns (T, P) float64 normalized, mean 0-d float64, std 0-d float64)."""
    if rewards.dim() != 2 or done.shape != rewards.shape:
        raise ValueError(f"rewards and done must be (T, P); got {tuple(rewards.shape)}, "
                         f"{tuple(done.shape)}")
    dev = rewards.device
    if dev.type != "cuda":
        raise RuntimeError("discounted_returns runs on a HIP device (no CPU fallback)")
    lib = abi.load_library()
    rew = rewards.to(torch.float32).contiguous()
    dn = done.to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8)
    T, P = rew.shape
    out = torch.empty(T, P, dtype=_F64, device=dev)
    stats = torch.empty(2, dtype=_F64, device=dev)
    work = torch.empty(int(lib.marlnav_returns_work_size(P)), dtype=_F64, device=dev)
    abi.check(lib.marlnav_discounted_returns(
        rew.data_ptr(), dn.data_ptr(), T, P, ctypes.c_double(float(gamma)), out.data_ptr(),
        stats.data_ptr(), work.data_ptr(), _stream(dev)), lib)
    return out, stats[0], stats[1]


def gae_advantages(rewards, done, values, last_values, gamma, lam):
    """GAE(lambda) of a stacked rollout (libmarlnav.so ``marlnav_gae_advantages``,
    DESIGN.md §15). rewards (T, P) float32, done (T, P) bool (terminated |
    truncated: a truncated episode counts as ended and gets no bootstrap),
    values (T, P) or (T, P, 1) float32 as collected, last_values (P,) or
    (P, 1) float32: the critic's value of the observation after the last step.
    Returns (advantages (T, P) float64 normalised over all T*P, value_targets
    (T, P) float64 in reward units, mean and unbiased std of the raw
    advantages as 0-d float64). Nothing synchronises."""
    if rewards.dim() != 2 or done.shape != rewards.shape:
        raise ValueError(f"rewards and done must be (T, P); got {tuple(rewards.shape)}, "
                         f"{tuple(done.shape)}")
    dev = rewards.device
    if dev.type != "cuda":
        raise RuntimeError("gae_advantages runs on a HIP device (no CPU fallback)")
    T, P = rewards.shape
    if values.numel() != T * P or values.shape[:2] != rewards.shape:
        raise ValueError(f"values must be (T, P) or (T, P, 1); got {tuple(values.shape)}")
    if last_values.numel() != P:
        raise ValueError(f"last_values must be (P,) or (P, 1); got {tuple(last_values.shape)}")
    lib = abi.load_library()
    rew = rewards.to(torch.float32).contiguous()
    dn = done.to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8)
    val = values.to(device=dev, dtype=torch.float32).contiguous()
    last = last_values.to(device=dev, dtype=torch.float32).contiguous()
    adv = torch.empty(T, P, dtype=_F64, device=dev)
    vt = torch.empty(T, P, dtype=_F64, device=dev)
    stats = torch.empty(2, dtype=_F64, device=dev)
    work = torch.empty(int(lib.marlnav_gae_work_size(P)), dtype=_F64, device=dev)
    abi.check(lib.marlnav_gae_advantages(
        rew.data_ptr(), dn.data_ptr(), val.data_ptr(), last.data_ptr(), T, P,
        ctypes.c_double(float(gamma)), ctypes.c_double(float(lam)), adv.data_ptr(), vt.data_ptr(),
        stats.data_ptr(), work.data_ptr(), _stream(dev)), lib)
    return adv, vt, stats[0], stats[1]


def process_rewards(buffer, gamma):
    """models.py:131-148 on the reference's list buffer: every entry's reward
    slot (index -2) becomes its normalized float64 return. Returns the mean
    (0-d tensor, as the reference's ``mean_rew``)."""
    rew = torch.stack([e[-2] for e in buffer])
    done = torch.stack([e[-1] for e in buffer])
    ret, mean, _ = discounted_returns(rew, done, gamma)
    for i, e in enumerate(buffer):
        e[-2] = ret[i]
    return mean


def mappo_process_rewards(mappo):
    """Drop-in body of MAPPO._process_rewards (models.py:131-148) for a MAPPO
    instance (reads buffer, gamma; sets _mean_rew, logs and prints like the
    reference)."""
    mean = process_rewards(mappo.buffer, mappo.gamma)
    mappo._mean_rew = mean
    print('MEAN_REW', mean.item())
    mappo._logs['mean_rews'] += [mean.item()]


class RolloutBuffer(object):
    """Stacked device storage for ``buffer_len`` steps of the six rollout
    entries MAPPO.get_data keeps per step (models.py:120): obs, actions,
    log_probs, values, rewards, done. Storage is allocated on the first
    ``add`` from the shapes and dtypes given."""

    VALUES, REWARDS, DONE = 3, 4, 5

    def __init__(self, buffer_len):
        self.buffer_len = int(buffer_len)
        self._store = None
        self._n = 0
        self.returns = None
        self.advantages = self.value_targets = None    # process_gae

    def __len__(self):
        return self._n

    def add(self, obs, actions, log_probs, values, rewards, done):
        items = (obs, actions, log_probs, values, rewards, done)
        if self._n >= self.buffer_len:
            raise IndexError(f"rollout buffer full ({self.buffer_len} steps)")
        if self._store is None:
            self._store = [torch.empty((self.buffer_len,) + tuple(x.shape), dtype=x.dtype,
                                       device=x.device) for x in items]
        for s, x in zip(self._store, items):
            s[self._n].copy_(x)
        self._n += 1

    def clear(self):
        self._n = 0
        self.returns = None
        self.advantages = self.value_targets = None

    def reserve(self, num_parallel, num_agents, obs_dim, device):
        """Allocate the storage for MAPPO.get_data's entry shapes (models.py:
        113-121) without an ``add``: obs (P, A, D), actions (P, A, 2),
        log_probs (P*A,), values (P, 1), rewards (P,), done (P,) bool. Keeps
        storage that already has these shapes on ``device``."""
        P, A, D = int(num_parallel), int(num_agents), int(obs_dim)
        shapes = ((P, A, D), (P, A, 2), (P * A,), (P, 1), (P,), (P,))
        dtypes = (torch.float32,) * 5 + (torch.bool,)
        device = torch.device(device)
        if self._store is not None and all(
                tuple(s.shape[1:]) == sh and s.dtype == dt and s.device == device
                for s, sh, dt in zip(self._store, shapes, dtypes)):
            return
        self._store = [torch.empty((self.buffer_len,) + sh, dtype=dt, device=device)
                       for sh, dt in zip(shapes, dtypes)]
        self.clear()

    def row(self, t):
        """The six storage rows of step ``t`` (views a producer writes in
        place, in ``add``'s order); ``commit`` then makes them stored steps."""
        if self._store is None:
            raise RuntimeError("rollout buffer has no storage yet: reserve() or add() first")
        if not 0 <= t < self.buffer_len:
            raise IndexError(f"step {t} outside the rollout buffer ({self.buffer_len} steps)")
        return tuple(s[t] for s in self._store)

    def commit(self, n):
        """Declare steps 0..n-1 stored (written through ``row``)."""
        if not 0 <= n <= self.buffer_len:
            raise IndexError(f"{n} steps do not fit the rollout buffer ({self.buffer_len})")
        self._n = int(n)
        self.returns = None
        self.advantages = self.value_targets = None

    def stacked(self, k):
        """Entry k (0..5) of every stored step, stacked: (n, ...)."""
        return self._store[k][:self._n]

    def process_rewards(self, gamma):
        """models.py:131-148 over the stored steps; the normalized float64
        returns replace the rewards in ``entries()``. Returns the mean."""
        ret, mean, _ = discounted_returns(self.stacked(self.REWARDS), self.stacked(self.DONE),
                                          gamma)
        self.returns = ret
        return mean

    def process_gae(self, gamma, lam, last_values):
        """``gae_advantages`` over the stored steps with ``last_values`` (P,)
        or (P, 1), the critic's value of the observation after the last one:
        sets ``advantages`` (normalised) and ``value_targets`` (reward units),
        both (n, P) float64; ``returns`` is left alone. Returns the mean of
        the raw advantages."""
        adv, vt, mean, _ = gae_advantages(self.stacked(self.REWARDS), self.stacked(self.DONE),
                                          self.stacked(self.VALUES), last_values, gamma, lam)
        self.advantages, self.value_targets = adv, vt
        return mean

    def entries(self):
        """The reference's list form: ``[[obs, actions, log_probs, values,
        reward_or_return, done], ...]`` as views of the stored steps."""
        out = []
        for t in range(self._n):
            e = [s[t] for s in self._store]
            if self.returns is not None:
                e[self.REWARDS] = self.returns[t]
            out.append(e)
        return out


_POLICY_PARAMS = (("actor_fc1_w", "actor", "fc1", "weight"), ("actor_fc1_b", "actor", "fc1", "bias"),
                  ("actor_mu_w", "actor", "fc_mu", "weight"), ("actor_mu_b", "actor", "fc_mu", "bias"),
                  ("actor_std_w", "actor", "fc_std", "weight"),
                  ("actor_std_b", "actor", "fc_std", "bias"),
                  ("critic_fc1_w", "critic", "fc1", "weight"),
                  ("critic_fc1_b", "critic", "fc1", "bias"),
                  ("critic_fc2_w", "critic", "fc2", "weight"),
                  ("critic_fc2_b", "critic", "fc2", "bias"))


def _module_params(actor, critic, who):
    """The ten live parameter tensors of ``actor`` / ``critic`` as
    ``[(field, tensor)]`` in ``_POLICY_PARAMS`` order, checked once (fp32,
    one HIP device, contiguous, the reference's shapes); -> (params, device,
    H, D, A)."""
    mods = {"actor": actor, "critic": critic}
    params = [(f, getattr(getattr(mods[m], layer), attr)) for f, m, layer, attr in _POLICY_PARAMS]
    p = dict(params)
    dev = p["actor_fc1_w"].device
    if dev.type != "cuda":
        raise RuntimeError(f"{who} runs on a HIP device (no CPU fallback); "
                           f"the actor's parameters are on {dev}")
    for f, t in params:
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{f}: need a contiguous float32 tensor on {dev}, got "
                             f"{t.dtype} on {t.device}, contiguous={t.is_contiguous()}")
    if p["actor_fc1_w"].dim() != 2:
        raise ValueError("actor.fc1.weight must be (H, D)")
    H, D = p["actor_fc1_w"].shape
    AD = p["critic_fc1_w"].shape[1] if p["critic_fc1_w"].dim() == 2 else -1
    want = {"actor_fc1_w": (H, D), "actor_fc1_b": (H,), "actor_mu_w": (2, H),
            "actor_mu_b": (2,), "actor_std_w": (2, H), "actor_std_b": (2,),
            "critic_fc1_w": (H, AD), "critic_fc1_b": (H,), "critic_fc2_w": (1, H),
            "critic_fc2_b": (1,)}
    for f, t in params:
        if tuple(t.shape) != want[f]:
            raise ValueError(f"{f}: shape {tuple(t.shape)}, expected {want[f]} "
                             "(one hidden size for both networks, models.py:69-70)")
    if AD < 2 * D or AD % D:
        raise ValueError(f"critic.fc1 takes {AD} inputs, not a multiple (>= 2) of the "
                         f"actor's {D}")
    return params, dev, int(H), int(D), int(AD // D)


class FusedPolicy(object):
    """``Actor`` + ``Critic`` (models.py:14-56) evaluated forward-only by one
    HIP launch per call (include/marlnav.h ``marlnav_policy_act``).

    ``actor`` / ``critic`` are any modules with the reference's attribute
    names (``fc1``, ``fc_mu``, ``fc_std`` / ``fc1``, ``fc2``) and shapes.
    Shapes, dtype (fp32), device and contiguity are checked here, once; the
    kernel reads the parameter tensors themselves on every call (no copy is
    kept), so an in-place optimiser step is seen by the next ``act``.

    ``seed`` keys the kernel's own normals (``act`` without ``eps``);
    ``env_offset`` is the global id of env 0 of this shard, so sharded runs
    draw what the unsharded run draws for the same envs."""

    def __init__(self, actor, critic, seed=0, env_offset=0):
        self.actor, self.critic = actor, critic
        self._params, self.device, H, D, A = _module_params(actor, critic, "FusedPolicy")
        self.hidden_size, self.obs_dim, self.num_agents = H, D, A
        self.seed = int(seed) & (2 ** 64 - 1)
        self.step_idx = 0          # next step index of the kernel's own normals
        self._lib = abi.load_library()
        self._dims = abi.MarlnavPolicyDims(num_agents=self.num_agents, obs_dim=self.obs_dim,
                                           hidden_size=self.hidden_size,
                                           env_offset=int(env_offset))
        self._bufs = abi.MarlnavPolicyBuffers()

    def _check(self, t, shape, what):
        if (t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != shape
                or not t.is_contiguous()):
            raise ValueError(f"{what}: need a contiguous float32 {shape} tensor on "
                             f"{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t.data_ptr()

    def act(self, obs_norm, eps=None, step_idx=None, out=None, eps_out=None):
        """obs_norm (P, A, D) normalised observations -> (actions (P, A, 2) in
        policy scale, log_probs (P*A,), values (P, 1)) as models.py:113-120
        computes them. ``eps`` (P*A, 2): the standard normals to use (e.g.
        ``torch.empty(P*A, 2).normal_()``, which is the reference's stream);
        None: the kernel draws them for ``(seed, step_idx)`` (``step_idx``
        None: this policy's running counter, which then advances). ``out``: a
        triple of tensors to write into; ``eps_out`` (P*A, 2) receives the
        normals used. One launch on the current stream, no synchronisation."""
        if obs_norm.dim() != 3:
            raise ValueError(f"obs_norm must be (P, A, D), got {tuple(obs_norm.shape)}")
        P, A, D = int(obs_norm.shape[0]), self.num_agents, self.obs_dim
        b, d = self._bufs, self._dims
        b.obs_norm = self._check(obs_norm, (P, A, D), "obs_norm")
        if out is None:
            out = (torch.empty(P, A, 2, device=self.device),
                   torch.empty(P * A, device=self.device),
                   torch.empty(P, 1, device=self.device))
        actions, log_probs, values = out
        b.actions = self._check(actions, (P, A, 2), "out[0] (actions)")
        b.log_probs = self._check(log_probs, (P * A,), "out[1] (log_probs)")
        b.values = self._check(values, (P, 1), "out[2] (values)")
        b.eps = None if eps is None else self._check(eps, (P * A, 2), "eps")
        b.eps_out = None if eps_out is None else self._check(eps_out, (P * A, 2), "eps_out")
        for f, t in self._params:
            setattr(b, f, t.data_ptr())
        if step_idx is None:
            step_idx = self.step_idx
            if eps is None:
                self.step_idx += 1
        d.num_parallel = P
        abi.check(self._lib.marlnav_policy_act(ctypes.byref(d), ctypes.byref(b), self.seed,
                                               int(step_idx), _stream(self.device)), self._lib)
        return actions, log_probs, values

    def values(self, obs_norm, out=None):
        """obs_norm (P, A, D) normalised observations -> values (P, 1): the
        critic alone (libmarlnav.so ``marlnav_critic_values``), bit-identical
        to ``act(obs_norm, ...)[2]``. Reads no actor weight, draws no random
        number and leaves ``step_idx`` alone. ``out``: a (P, 1) tensor to write
        into. One launch on the current stream, no synchronisation."""
        if obs_norm.dim() != 3:
            raise ValueError(f"obs_norm must be (P, A, D), got {tuple(obs_norm.shape)}")
        P, A, D = int(obs_norm.shape[0]), self.num_agents, self.obs_dim
        b, d = self._bufs, self._dims
        b.obs_norm = self._check(obs_norm, (P, A, D), "obs_norm")
        if out is None:
            out = torch.empty(P, 1, device=self.device)
        b.values = self._check(out, (P, 1), "out (values)")
        for f, t in self._params:
            setattr(b, f, t.data_ptr())
        d.num_parallel = P
        abi.check(self._lib.marlnav_critic_values(ctypes.byref(d), ctypes.byref(b),
                                                  _stream(self.device)), self._lib)
        return out


def _check_lambda(gae_lambda):
    lam = float(gae_lambda)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"gae_lambda={gae_lambda} must be in [0, 1]")
    return lam


def collect(env, policy, buffer, eps_source=None, gamma=0.9, gae_lambda=None):
    """MAPPO.get_data's loop (models.py:106-125) for ``buffer.buffer_len``
    steps: the initial normalised observations, then per step ``policy.act``
    straight into the buffer's row, ``env.step`` on those actions (the env's
    attached ObsNormalizer and ActionScaler do the normalising and the
    up-scaling inside the step kernel), ``done = terminated | truncated``;
    after the loop ``_process_rewards`` (``buffer.process_rewards(gamma)``;
    0.9 is the reference's default) and ``_update_epi_stats`` (the env's
    episode counters are read and zeroed). Prints and file saving stay with
    the caller.

    ``eps_source(t)``: the (P*A, 2) standard normals of step ``t`` (None: the
    kernel's own stream). Returns ``(mean_rew, {'trunc', 'col', 'tar'})``.

    ``gae_lambda`` (None: the reference's estimator alone): also
    ``policy.values`` of the normalised observations the env holds after the
    last step and ``buffer.process_gae(gamma, gae_lambda, ...)`` (DESIGN.md
    §15). The returns and ``mean_rew`` are computed either way."""
    lam = None if gae_lambda is None else _check_lambda(gae_lambda)
    nrm = env._normalizer
    if nrm is None or env._action_scaler is None:
        raise RuntimeError("collect needs env.attach_normalizer(...) and "
                           "env.attach_action_scaler(...): the policy reads normalised "
                           "observations and the env takes policy-scale actions")
    P, A, D = env._obs_shape
    if (A, D) != (policy.num_agents, policy.obs_dim):
        raise ValueError(f"policy is built for {policy.num_agents} agents x {policy.obs_dim} "
                         f"features, the env has {A} x {D}")
    T = buffer.buffer_len
    buffer.reserve(P, A, D, env.device)
    buffer.clear()
    obs_n = nrm(env.observations())        # models.py:110
    for t in range(T):
        o, actions, log_probs, values, rewards, done = buffer.row(t)
        o.copy_(obs_n)
        policy.act(obs_n, eps=None if eps_source is None else eps_source(t),
                   out=(actions, log_probs, values))
        obs, rew, terminated, truncated = env.step(actions)
        torch.logical_or(terminated, truncated, out=done)
        rewards.copy_(rew)
        obs_n = nrm(obs)
    buffer.commit(T)
    mean = buffer.process_rewards(gamma)
    if lam is not None:
        buffer.process_gae(gamma, lam, policy.values(obs_n.contiguous()))
    trunc, col, tar = env._counter_totals()                # one read of the three counters
    stats = {"trunc": trunc, "col": col, "tar": tar}
    env._num_trunc = env._num_col = env._num_tar = 0      # models.py:153-158
    return mean, stats


def collect_fused(env, policy, buffer, eps=None, gamma=0.9, gae_lambda=None):
    """``collect`` as ONE C call (libmarlnav.so ``marlnav_rollout_collect``):
    the initial observations and their normalisation, then for each of the
    ``buffer.buffer_len`` steps the policy launch and the step launch, the
    merge ``done = terminated | truncated`` over the whole stack and the
    returns scan are enqueued back to back on the current stream, with no
    Python, no ``torch`` launch and no copy between them. Every step kernel
    writes its normalised observations straight into the buffer's next row,
    where the next policy launch reads them. The buffer, ``buffer.returns``,
    the env and the policy end exactly as ``collect`` leaves them, bit for
    bit (the same kernels on the same bits); returns the same
    ``(mean_rew, {'trunc', 'col', 'tar'})``.

    ``eps``: None for the policy kernel's own stream (``policy.step_idx``
    then advances by the number of steps), or a ``(T, P*A, 2)`` float32
    tensor of standard normals, row ``t`` for step ``t``.

    ``gae_lambda`` (None: the reference's estimator alone): three calls follow
    the rollout call on the same stream with no synchronisation, as in
    ``collect``: the normalised observations the env holds after the last
    step (what the next rollout's row 0 will be), ``policy.values`` of them
    and ``buffer.process_gae``.

    Tensors the caller still holds from before the call (``env.states``,
    ``obstacles``, ``target``, ``_step_num``, ``_terminates``) are not
    written: the env moves to copies first, and the held ones keep their
    pre-call values.

    Raises RuntimeError, before anything is launched, for what only the
    per-step loop of ``collect`` can do: an env in reference-RNG mode or with
    a user-assigned init sampler (the host draws every step), no attached
    normaliser or action scaler, parameters that cannot be synced; and under
    stream capture unless ``env.allow_graph_capture`` is set (then the
    episode counters are left alone and the stats are None: reading them
    would synchronise)."""
    mean, capturing = _collect_fused_enqueue(env, policy, buffer, eps, gamma, gae_lambda)
    if capturing:
        return mean, None
    trunc, col, tar = env._counter_totals()                # one read of the three counters
    env._num_trunc = env._num_col = env._num_tar = 0      # models.py:153-158
    return mean, {"trunc": trunc, "col": col, "tar": tar}


def _collect_fused_enqueue(env, policy, buffer, eps=None, gamma=0.9, gae_lambda=None):
    """``collect_fused`` up to the episode counters, which are left alone:
    every check, the one C call and the host-side bookkeeping, with nothing
    that synchronises. -> (mean_rew, capturing)."""
    who = "collect_fused"
    lam = None if gae_lambda is None else _check_lambda(gae_lambda)
    if env._rng != 'native' or env._init_sampler is not env._default_init_sampler:
        raise RuntimeError(f"{who} needs an env in native-RNG mode with its default init "
                           "sampler: a reference-RNG or user-assigned sampler is called on the "
                           "host every step; use collect() for such an env")
    if env._normalizer is None or env._action_scaler is None:
        raise RuntimeError(f"{who} needs env.attach_normalizer(...) and "
                           "env.attach_action_scaler(...), as collect() does: the policy reads "
                           "normalised observations and the env takes policy-scale actions")
    dev = env.device
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing and not env.allow_graph_capture:
        raise RuntimeError(f"{who} under stream capture replays the steps' re-init draws on "
                           "every graph replay; set env.allow_graph_capture = True to accept "
                           "that (timing runs), or use collect() outside the capture")
    P, A, D = env._obs_shape
    if (A, D) != (policy.num_agents, policy.obs_dim):
        raise ValueError(f"policy is built for {policy.num_agents} agents x {policy.obs_dim} "
                         f"features, the env has {A} x {D}")
    if policy.device != dev:
        raise ValueError(f"the policy is on {policy.device}, the env on {dev}")
    T = buffer.buffer_len
    if eps is not None and (eps.dtype != torch.float32 or eps.device != dev
                            or tuple(eps.shape) != (T, P * A, 2) or not eps.is_contiguous()):
        raise ValueError(f"eps: need a contiguous float32 {(T, P * A, 2)} tensor on {dev}, got "
                         f"{eps.dtype} {tuple(eps.shape)} on {eps.device}")
    env._sync_params()
    if any(env._engine.shared_state()):
        env._unshare_state(multi_step=True)
    if not env._engine.fast_ok:
        raise RuntimeError(f"{who}: the env's parameters are not in sync with its engine and "
                           "could not be synced; use collect()")
    lib = abi.load_library()
    buffer.reserve(P, A, D, dev)
    buffer.clear()
    r = abi.MarlnavRolloutBuffers()
    for name, s in zip(abi.ROLLOUT_BUFFER_FIELDS, buffer._store):
        setattr(r, name, s.data_ptr())
    truncated = torch.empty(T, P, dtype=torch.uint8, device=dev)
    returns = torch.empty(T, P, dtype=_F64, device=dev)
    stats = torch.empty(2, dtype=_F64, device=dev)
    work = torch.empty(int(lib.marlnav_returns_work_size(P)), dtype=_F64, device=dev)
    # the env's own observation outputs: the raw rows of every step and the
    # normalised ones of the last step (the earlier ones land in the buffer)
    raw, last = env._new_obs(), env._new_obs()
    r.truncated, r.eps = truncated.data_ptr(), None if eps is None else eps.data_ptr()
    r.returns, r.returns_stats, r.returns_work = returns.data_ptr(), stats.data_ptr(), work.data_ptr()
    pd, pb = policy._dims, policy._bufs
    for f, t in policy._params:
        setattr(pb, f, t.data_ptr())
    pd.num_parallel = P
    env._engine.rollout(abi.fn_addr(lib.marlnav_rollout_collect), bytes(pd), bytes(pb), bytes(r),
                        raw.data_ptr(), last.data_ptr(), T, policy.seed, policy.step_idx,
                        float(gamma))
    del truncated, work, raw           # stream-ordered: reused after the kernels
    if eps is None:
        policy.step_idx += T
    buffer.commit(T)
    buffer.returns = returns
    if lam is not None:                # `last`: the observations after step T - 1, normalised
        buffer.process_gae(gamma, lam, policy.values(last))
    del last
    env._reinit_mask = torch.where(buffer.stacked(buffer.DONE)[T - 1], 1, 0)   # environment.py:102
    return stats[0], capturing


def minibatch_bounds(buffer_len, batch_size):
    """The minibatch slices of MAPPO.train_actor / train_critic (models.py:
    165-172) as ``[(lo, hi)]`` step ranges: ``buffer_len // batch_size`` of
    them, ``[start : start + batch_size]`` while ``start + batch_size <
    buffer_len``, else ``[start : -1]`` - the last batch loses the buffer's
    final step. An empty slice (where the reference's ``torch.cat`` raises) is
    a ValueError."""
    buffer_len, batch_size = int(buffer_len), int(batch_size)
    if batch_size < 1 or buffer_len < 1:
        raise ValueError(f"buffer_len={buffer_len} and batch_size={batch_size} must be >= 1")
    out = []
    for j in range(buffer_len // batch_size):
        lo = j * batch_size
        hi = lo + batch_size if lo + batch_size < buffer_len else buffer_len - 1
        if hi <= lo:
            raise ValueError(f"minibatch {j} of buffer_len={buffer_len}, batch_size={batch_size} "
                             f"is the empty slice [{lo}:-1]")
        out.append((lo, hi))
    return out


def shuffled_minibatch_sizes(buffer_len, batch_size):
    """The step counts of one epoch's minibatches in the shuffled mode
    (DESIGN.md §18): ``buffer_len // batch_size`` minibatches of
    ``batch_size`` steps of the epoch's permutation, the last one extended by
    the ``buffer_len % batch_size`` left over, so the sizes sum to
    ``buffer_len`` and every stored step is used once per epoch. No minibatch
    (``batch_size > buffer_len``) is a ValueError."""
    buffer_len, batch_size = int(buffer_len), int(batch_size)
    if batch_size < 1 or buffer_len < 1:
        raise ValueError(f"buffer_len={buffer_len} and batch_size={batch_size} must be >= 1")
    n = buffer_len // batch_size
    if n == 0:
        raise ValueError(f"batch_size={batch_size} is greater than the {buffer_len} stored "
                         "steps: no minibatch")
    return [batch_size] * (n - 1) + [buffer_len - (n - 1) * batch_size]


def shuffled_minibatches(perm, batch_size):
    """One epoch's minibatches as lists of steps: ``perm`` (a sequence of
    ``buffer_len`` steps) cut by ``shuffled_minibatch_sizes``."""
    perm = [int(x) for x in perm]
    out, at = [], 0
    for n in shuffled_minibatch_sizes(len(perm), batch_size):
        out.append(perm[at:at + n])
        at += n
    return out


def check_shuffle_len(buffer_len, num_epochs=1):
    """ValueError unless the on-device permutation generator takes a buffer
    of ``buffer_len`` steps over ``num_epochs`` epochs (both at most 65 535:
    ``marlnav_minibatch_permutations``)."""
    if not 1 <= int(buffer_len) <= abi.SHUFFLE_MAX_STEPS:
        raise ValueError(f"shuffled minibatches take 1..{abi.SHUFFLE_MAX_STEPS} stored steps, "
                         f"got {buffer_len}")
    if not 1 <= int(num_epochs) <= abi.SHUFFLE_MAX_STEPS:
        raise ValueError(f"shuffled minibatches take 1..{abi.SHUFFLE_MAX_STEPS} epochs, "
                         f"got {num_epochs}")


def check_steps(steps, stored):
    """A minibatch's step list as a list of ints: a non-empty HOST sequence or
    CPU integer tensor with every entry in ``[0, stored)`` (duplicates are
    allowed); anything else is a ValueError. A device tensor is refused: its
    entries would reach the kernels unchecked."""
    if torch.is_tensor(steps):
        if steps.device.type != 'cpu':
            raise ValueError("steps: need a host sequence or a CPU integer tensor, got a tensor "
                             f"on {steps.device}; device-side step tables are drawn and used by "
                             "training.train_phase(shuffle=...) only")
        if steps.dtype.is_floating_point or steps.dtype == torch.bool or steps.dim() != 1:
            raise ValueError(f"steps: need a 1-d integer tensor, got {steps.dtype} "
                             f"{tuple(steps.shape)}")
        steps = steps.tolist()
    out = []
    for x in steps:
        if isinstance(x, bool) or int(x) != x:
            raise ValueError(f"steps: {x!r} is not an integer")
        out.append(int(x))
    if not out:
        raise ValueError("steps is empty: a minibatch needs at least one step")
    for x in out:
        if not 0 <= x < stored:
            raise ValueError(f"steps: {x} is outside the {stored} stored steps [0, {stored})")
    return out


class FusedPPO(object):
    """``MAPPO._actor_loss`` / ``_critic_loss`` (models.py:270-316) of one
    minibatch with ``zero_grad()`` + ``backward()`` (models.py:173-175,
    193-195), by libmarlnav.so ``marlnav_ppo_actor_grad`` /
    ``marlnav_ppo_critic_grad``: no autograd graph and no
    ``MultivariateNormal``. The kernels read steps ``lo..hi`` of a
    ``RolloutBuffer``'s stacked storage in place and the modules' live
    parameter tensors, and OVERWRITE the parameters' ``.grad`` (allocated here
    where None), so a ``torch.optim`` optimiser's ``step()`` follows directly.

    ``actor`` / ``critic``: checked as ``FusedPolicy`` checks them. ``epsilon``
    and ``ent_const`` are the reference's Python scalars.

    Single device: the losses are means over the whole minibatch and the
    advantage of agent row ``i`` is that of env row ``i mod (T*P)`` (the
    reference's ``repeat(num_agents)``, kept), which pairs rows across env
    shards; training over ``shard``-split envs needs an all-reduce of the
    gradients and a cross-shard reading of that pairing, neither of which is
    here.

    ``advantage='gae'`` (the default ``'reference'`` is the
    above, bit for bit): the actor reads ``buffer.advantages`` as the ready
    advantage of each agent row's OWN env row (``i // A``), the critic is
    trained towards ``buffer.value_targets``; both come from
    ``buffer.process_gae`` (``collect(..., gae_lambda=...)``). The own-env
    pairing removes the cross-shard reading; the all-reduce is still missing."""

    def __init__(self, actor, critic, epsilon, ent_const, advantage='reference'):
        if advantage not in ('reference', 'gae'):
            raise ValueError(f"advantage must be 'reference' or 'gae', got {advantage!r}")
        self.advantage = advantage
        self._mode = abi.ADVANTAGE_ENV if advantage == 'gae' else abi.ADVANTAGE_REFERENCE
        self.actor, self.critic = actor, critic
        self._params, self.device, H, D, A = _module_params(actor, critic, "FusedPPO")
        self.hidden_size, self.obs_dim, self.num_agents = H, D, A
        self.epsilon, self.ent_const = float(epsilon), float(ent_const)
        self._lib = abi.load_library()
        self._dims = abi.MarlnavPpoDims(num_agents=A, obs_dim=D, hidden_size=H)
        self._bufs = abi.MarlnavPpoBuffers()
        self._work = None
        self.last_diag = self.last_stop = None     # of the last monitored train_phase
        # train_phase(shuffle=...): per network the call counter cell and the last table
        self._shuffle_counter, self.last_steps = {}, {}
        for f, t in self._params:
            if t.grad is None:
                t.grad = torch.zeros_like(t)

    def _require(self, buffer):
        """Refuse a buffer that lacks what this mode trains on."""
        if self.advantage == 'gae':
            if buffer.advantages is None or buffer.value_targets is None:
                raise RuntimeError("the rollout buffer has no GAE advantages yet: call "
                                   "buffer.process_gae(gamma, lam, last_values) (or collect(..., "
                                   "gae_lambda=...)) before training")
        elif buffer.returns is None:
            raise RuntimeError("the rollout buffer has no returns yet: call "
                               "buffer.process_rewards(gamma) (or collect()) before training")

    def _bind(self, buffer, lo, hi, network='actor', diag=False):
        """Point the call's structs at steps lo..hi of the buffer; -> loss.
        The ``returns`` pointer: the normalised returns, or in the GAE mode
        the advantages (``network='actor'``) / the value targets
        (``'critic'``). ``diag``: the workspace of the diagnostic variant."""
        self._require(buffer)
        if self.advantage == 'gae':
            target = buffer.advantages if network == 'actor' else buffer.value_targets
        else:
            target = buffer.returns
        n = len(buffer)
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= n:
            raise ValueError(f"steps [{lo}:{hi}] are not a non-empty range of the {n} stored steps")
        obs, actions, log_probs, values = (buffer.stacked(k) for k in range(4))
        P, A, D = int(obs.shape[1]), self.num_agents, self.obs_dim
        T = hi - lo
        b, d = self._bufs, self._dims
        for name, t, shape, dtype in (("obs", obs, (n, P, A, D), torch.float32),
                                      ("actions", actions, (n, P, A, 2), torch.float32),
                                      ("log_probs", log_probs, (n, P * A), torch.float32),
                                      ("values", values, (n, P, 1), torch.float32),
                                      ("returns", target, (n, P), _F64)):
            if (tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device
                    or not t.is_contiguous()):
                raise ValueError(f"buffer {name}: need a contiguous {dtype} {shape} tensor on "
                                 f"{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
            setattr(b, name, t[lo].data_ptr())
        for f, t in self._params:
            g = t.grad
            if g is None:          # zero_grad(set_to_none=True) between calls
                g = t.grad = torch.zeros_like(t)
            if g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous() \
                    or g.shape != t.shape:
                raise ValueError(f"{f}.grad: need a contiguous float32 tensor like the parameter")
            setattr(b, f, t.data_ptr())
            setattr(b, "grad_" + f, g.data_ptr())
        d.num_parallel, d.num_steps = P, T
        self._grow_work(diag)
        loss = torch.empty((), dtype=_F64, device=self.device)
        b.loss = loss.data_ptr()
        return loss

    def _grow_work(self, diag=False, need=None):
        """Bind a workspace of ``need`` doubles (the answer of a phase's
        work-size call; None: what one update of the bound dims needs, with
        ``diag`` the diagnostic variant's), grown where it is too small."""
        if need is None:
            size = self._lib.marlnav_ppo_diag_work_size if diag else self._lib.marlnav_ppo_work_size
            need = size(ctypes.byref(self._dims))
        need = int(need)
        if need < 0:
            abi.check(need, self._lib)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=_F64, device=self.device)
        self._bufs.work = self._work.data_ptr()

    def actor_loss_grad(self, buffer, lo, hi, diag_out=None):
        """Actor loss (0-d float64 device tensor) of steps ``lo..hi`` of
        ``buffer``; the six actor parameters' ``.grad`` are overwritten. Two
        launches on the current stream, no synchronisation.

        ``diag_out`` (None: the above): a contiguous float64 device tensor of
        5 elements that receives the update's diagnostics (DESIGN.md §17,
        ``marlnav_ppo_actor_grad_diag``): the surrogate mean, the entropy
        mean, the approximate KL divergence from the rollout policy (the k3
        estimator, mean of ``(ratio - 1) - log ratio``), the fraction of rows
        whose ratio left ``[1 - epsilon, 1 + epsilon]`` and a status that is
        0 here. Loss and ``.grad`` carry the bits they carry without it. Also
        bound as ``actor_grad``."""
        if diag_out is not None:
            check_diag_out(diag_out, self.device)
            loss = self._bind(buffer, lo, hi, diag=True)
            abi.check(self._lib.marlnav_ppo_actor_grad_diag(
                ctypes.byref(self._dims), ctypes.byref(self._bufs), self.epsilon, self.ent_const,
                self._mode, diag_out.data_ptr(), _stream(self.device)), self._lib)
            return loss
        loss = self._bind(buffer, lo, hi)
        abi.check(self._lib.marlnav_ppo_actor_grad_mode(
            ctypes.byref(self._dims), ctypes.byref(self._bufs), self.epsilon, self.ent_const,
            self._mode, _stream(self.device)), self._lib)
        return loss

    actor_grad = actor_loss_grad

    def critic_loss_grad(self, buffer, lo, hi):
        """Critic loss (0-d float64 device tensor) of steps ``lo..hi``; the
        four critic parameters' ``.grad`` are overwritten."""
        loss = self._bind(buffer, lo, hi, 'critic')
        abi.check(self._lib.marlnav_ppo_critic_grad(
            ctypes.byref(self._dims), ctypes.byref(self._bufs), self.epsilon,
            _stream(self.device)), self._lib)
        return loss

    def _bind_steps(self, buffer, steps, network='actor', diag=False):
        """``_bind`` for a minibatch given as a list of steps: the data
        pointers at step 0 of the storage, ``num_steps`` the length of the
        list, the list uploaded as an int32 device table; -> (loss, table)."""
        steps = check_steps(steps, len(buffer))
        loss = self._bind(buffer, 0, len(buffer), network, diag)
        self._dims.num_steps = len(steps)
        self._grow_work(diag)
        table = torch.tensor(steps, dtype=torch.int32).to(self.device)
        return loss, table

    def actor_loss_grad_steps(self, buffer, steps, diag_out=None):
        """``actor_loss_grad`` of the minibatch whose steps are ``steps`` in
        that order (``marlnav_ppo_actor_grad_steps``): logical
        row ``(slot, p, a)`` is the agent row of step ``steps[slot]``. Bit for
        bit ``actor_loss_grad(gathered, 0, len(steps))`` on a buffer whose
        storage was gathered with ``index_select(0, steps)``; the kernels
        gather by address and copy nothing.

        ``steps``: a host sequence or CPU integer tensor, non-empty, every
        entry in ``[0, len(buffer))``, duplicates allowed; checked here and
        uploaded as int32 (a host-to-device copy: not for graph capture). A
        device tensor is a ValueError: ``training.train_phase(shuffle=...)``
        is the path whose tables never leave the device."""
        if diag_out is not None:
            check_diag_out(diag_out, self.device)
        loss, table = self._bind_steps(buffer, steps, 'actor', diag=diag_out is not None)
        abi.check(self._lib.marlnav_ppo_actor_grad_steps(
            ctypes.byref(self._dims), ctypes.byref(self._bufs), table.data_ptr(), self.epsilon,
            self.ent_const, self._mode, None if diag_out is None else diag_out.data_ptr(),
            _stream(self.device)), self._lib)
        return loss

    def critic_loss_grad_steps(self, buffer, steps):
        """``critic_loss_grad`` of the minibatch ``steps``
        (``marlnav_ppo_critic_grad_steps``), as ``actor_loss_grad_steps``."""
        loss, table = self._bind_steps(buffer, steps, 'critic')
        abi.check(self._lib.marlnav_ppo_critic_grad_steps(
            ctypes.byref(self._dims), ctypes.byref(self._bufs), table.data_ptr(), self.epsilon,
            _stream(self.device)), self._lib)
        return loss

    def actor_update_steps(self, buffer, steps, adam, max_grad_norm=None, norm_out=None):
        """``actor_loss_grad_steps(buffer, steps)`` then
        ``adam.step(max_grad_norm, norm_out)``: the unfolded update that
        ``train_phase(shuffle=...)`` enqueues per minibatch. ``adam``: a
        ``FusedAdam`` over exactly the six actor parameters in order.
        Returns the loss."""
        return self._update_steps("actor", buffer, steps, adam, max_grad_norm, norm_out)

    def critic_update_steps(self, buffer, steps, adam, max_grad_norm=None, norm_out=None):
        """As ``actor_update_steps``, for the critic."""
        return self._update_steps("critic", buffer, steps, adam, max_grad_norm, norm_out)

    def _update_steps(self, network, buffer, steps, adam, max_grad_norm, norm_out):
        if not (isinstance(adam, FusedAdam) and adam.covers(self._network_params(network))):
            raise ValueError(f"adam: need a FusedAdam over exactly the {network}'s parameters in "
                             "order")
        loss = getattr(self, network + "_loss_grad_steps")(buffer, steps)
        adam.step(max_grad_norm=max_grad_norm, norm_out=norm_out)
        return loss

    def _network_params(self, which):
        """The parameter tensors of 'actor' / 'critic' in ``_POLICY_PARAMS``
        order."""
        return [t for f, t in self._params if f.startswith(which)]

    def actor_update(self, buffer, lo, hi, adam, max_grad_norm=None, norm_out=None):
        """``actor_loss_grad(buffer, lo, hi)`` then ``adam.step()`` as ONE C
        call (``marlnav_ppo_actor_update``): four launches on the current
        stream with no host work between them, bit-identical to the two
        calls. ``adam``: a ``FusedAdam`` over exactly the six actor
        parameters in ``_POLICY_PARAMS`` order (the library refuses any other
        table). Returns the loss (0-d float64 device tensor).

        ``max_grad_norm`` (None: the above, bit for bit): the gradient is
        clipped by its global L2 norm before the step, as
        ``adam.step(max_grad_norm=..., norm_out=...)`` does it
        (``marlnav_ppo_actor_update_clipped``, five launches)."""
        return self._update("actor", buffer, lo, hi, adam, max_grad_norm, norm_out)

    def critic_update(self, buffer, lo, hi, adam, max_grad_norm=None, norm_out=None):
        """``critic_loss_grad`` then ``adam.step()`` as one C call
        (``marlnav_ppo_critic_update``); ``adam`` over the four critic
        parameters. As ``actor_update``, ``max_grad_norm`` included
        (``marlnav_ppo_critic_update_clipped``)."""
        return self._update("critic", buffer, lo, hi, adam, max_grad_norm, norm_out)

    def _update(self, network, buffer, lo, hi, adam, max_grad_norm, norm_out):
        """``actor_update`` / ``critic_update``: the network's one-call update,
        its ``_clipped`` form with ``max_grad_norm``; the critic's take no
        ``ent_const`` and no advantage mode."""
        loss = self._bind(buffer, lo, hi, network)
        ad, ab = adam._bind()
        clip = adam._clip_args(max_grad_norm, norm_out)
        actor = network == "actor"
        entry = f"marlnav_ppo_{network}_update_clipped"
        if max_grad_norm is None:
            entry = "marlnav_ppo_actor_update_mode" if actor else "marlnav_ppo_critic_update"
            clip = ()
        abi.check(getattr(self._lib, entry)(
            ctypes.byref(self._dims), ctypes.byref(self._bufs), self.epsilon,
            *((self.ent_const,) if actor else ()), ctypes.byref(ad), ctypes.byref(ab),
            *((self._mode,) if actor else ()), *clip, _stream(self.device)), self._lib)
        return loss


class FusedAdam(object):
    """``torch.optim.Adam`` with ``weight_decay=0`` and ``amsgrad=False`` (how
    the reference constructs it, models.py:71-74) over up to 8 contiguous fp32
    parameters on one HIP device, as one call of libmarlnav.so
    ``marlnav_adam_step``: one launch advances the step count, which lives on
    the device, the next updates every element of every parameter. Nothing
    synchronises and the host keeps no count, so steps can be captured in a
    graph and replayed.

    ``exp_avg`` and ``exp_avg_sq`` of all parameters are views of one flat
    fp32 allocation (each segment padded to 16 bytes), created zeroed here and
    never reallocated: ``load_state_dict`` copies into them in place, so the
    pointers a captured graph holds stay valid. ``.grad`` is allocated
    (zeros) where it is None.

    ``param_groups`` is a one-entry list of dicts as ``torch.optim`` keeps it;
    ``lr``, ``betas``, ``eps`` and ``maximize`` are read from it at every call
    and travel as launch arguments, so a captured graph keeps the values of
    capture time (change them, then capture again).

    ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam``'s
    format, so a checkpoint moves between the two in either direction.

    ``step(max_grad_norm=G)`` clips the gradient by its global L2 norm over
    all parameters first, as
    ``torch.nn.utils.clip_grad_norm_(params, G)`` before ``step()`` does. The
    scratch of the norm's partial sums is allocated at the first such call
    and never again, so a captured graph's pointer stays valid."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, maximize=False,
                 weight_decay=0, amsgrad=False):
        if weight_decay != 0:
            raise ValueError(f"FusedAdam: weight_decay={weight_decay} is unsupported "
                             "(the reference's Adam has none)")
        if amsgrad:
            raise ValueError("FusedAdam: amsgrad=True is unsupported")
        params = list(params)
        if not 1 <= len(params) <= abi.ADAM_MAX_TENSORS:
            raise ValueError(f"FusedAdam takes 1..{abi.ADAM_MAX_TENSORS} parameter tensors, "
                             f"got {len(params)}")
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FusedAdam runs on a HIP device (no CPU fallback); "
                               f"the parameters are on {dev}")
        for i, p in enumerate(params):
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous() \
                    or p.numel() < 1:
                raise ValueError(f"params[{i}]: need a non-empty contiguous float32 tensor on "
                                 f"{dev}, got {p.dtype} {tuple(p.shape)} on {p.device}, "
                                 f"contiguous={p.is_contiguous()}")
        self.device = dev
        self.param_groups = [{"params": params, "lr": lr, "betas": tuple(betas), "eps": eps,
                              "maximize": bool(maximize), "weight_decay": 0, "amsgrad": False}]
        self._hyper()                       # refuses bad values now rather than at step()
        self._lib = abi.load_library()
        offs, at = [], 0
        for p in params:
            offs.append(at)
            at += (p.numel() + 3) // 4 * 4  # segments start on 16 bytes
        self._flat = torch.zeros(2 * at, dtype=torch.float32, device=dev)
        self.exp_avg = [self._flat[o:o + p.numel()].view(p.shape) for o, p in zip(offs, params)]
        self.exp_avg_sq = [self._flat[at + o:at + o + p.numel()].view(p.shape)
                           for o, p in zip(offs, params)]
        nstate = int(self._lib.marlnav_adam_state_size())
        self._state = torch.zeros((nstate + 7) // 8, dtype=torch.int64, device=dev)
        self._dims = abi.MarlnavAdamDims(num_tensors=len(params))
        self._bufs = abi.MarlnavAdamBuffers(state=self._state.data_ptr())
        self._norm_work = None              # the clipped step's scratch, at first use
        for i, p in enumerate(params):
            self._dims.numel[i] = p.numel()
            self._bufs.exp_avg[i] = self.exp_avg[i].data_ptr()
            self._bufs.exp_avg_sq[i] = self.exp_avg_sq[i].data_ptr()
            if p.grad is None:
                p.grad = torch.zeros_like(p)

    @property
    def params(self):
        return self.param_groups[0]["params"]

    def _hyper(self):
        g = self.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False):
            raise ValueError("FusedAdam: weight_decay and amsgrad are unsupported")
        lr, (b1, b2), eps = float(g["lr"]), g["betas"], float(g["eps"])
        if not 0.0 <= lr < float("inf"):
            raise ValueError(f"FusedAdam: lr={lr} must be finite and >= 0")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"FusedAdam: betas={g['betas']} outside [0, 1)")
        if not 0.0 <= eps < float("inf"):
            raise ValueError(f"FusedAdam: eps={eps} must be finite and >= 0")
        return lr, float(b1), float(b2), eps, 1 if g["maximize"] else 0

    def _bind(self):
        """The call's structs from the live tensors and ``param_groups``."""
        d, b = self._dims, self._bufs
        d.lr, d.beta1, d.beta2, d.eps, d.maximize = self._hyper()
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                raise RuntimeError(f"FusedAdam: params[{i}].grad is None (zero_grad("
                                   "set_to_none=True) with no gradient written since)")
            if g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous() \
                    or g.shape != p.shape:
                raise ValueError(f"params[{i}].grad: need a contiguous float32 tensor like the "
                                 "parameter")
            b.param[i] = p.data_ptr()
            b.grad[i] = g.data_ptr()
        return d, b

    def _clip_args(self, max_grad_norm, norm_out, count=1, what="norm_out"):
        """-> (max_norm, norm_work pointer, norm_out pointer or None) of a
        clipped call; the scratch is allocated at the first one. ``norm_out``:
        None or a contiguous float64 tensor of ``count`` elements on the
        device. The value is checked here and again by the library.
        ``max_grad_norm`` None, no clip: ``(abi.MAX_NORM_NONE, None, None)``,
        and a ``norm_out`` is a ValueError."""
        if max_grad_norm is None:
            if norm_out is not None:
                raise ValueError(f"{what} needs max_grad_norm (inf records the "
                                 f"norm{'s' if count != 1 else ''} only)")
            return abi.MAX_NORM_NONE, None, None
        g = check_max_grad_norm(max_grad_norm)
        if self._norm_work is None:
            need = int(self._lib.marlnav_grad_norm_work_size(ctypes.byref(self._dims)))
            if need < 0:
                abi.check(need, self._lib)
            self._norm_work = torch.empty(need, dtype=_F64, device=self.device)
        out = None
        if norm_out is not None:
            if (not torch.is_tensor(norm_out) or norm_out.dtype != _F64
                    or norm_out.device != self.device or norm_out.numel() != count
                    or not norm_out.is_contiguous()):
                raise ValueError(f"{what}: need a contiguous float64 tensor of {count} "
                                 f"element(s) on {self.device}")
            out = norm_out.data_ptr()
        return g, self._norm_work.data_ptr(), out

    def step(self, max_grad_norm=None, norm_out=None):
        """One Adam step of every parameter from its ``.grad``: one
        ``marlnav_adam_step`` (two launches) on the current stream.

        ``max_grad_norm`` (None: the above, bit for bit): ``.grad`` is first
        scaled by ``min(1, max_grad_norm / (norm + 1e-6))``, ``norm`` the L2
        norm over all parameters in fp64, and stays scaled afterwards, as
        after ``clip_grad_norm_``; the norm before clipping goes to
        ``norm_out`` (a float64 device tensor of one element) where given.
        ``float('inf')`` records the norm and clips nothing. One
        ``marlnav_adam_step_clipped`` (three launches), nothing synchronises;
        the value travels as a launch argument, so a captured graph keeps it."""
        d, b = self._bind()
        g, work, out = self._clip_args(max_grad_norm, norm_out)
        if max_grad_norm is None:
            abi.check(self._lib.marlnav_adam_step(ctypes.byref(d), ctypes.byref(b),
                                                  _stream(self.device)), self._lib)
            return
        abi.check(self._lib.marlnav_adam_step_clipped(ctypes.byref(d), ctypes.byref(b), g, work,
                                                      out, _stream(self.device)), self._lib)

    def zero_grad(self, set_to_none=False):
        """Zero the gradients in place (the default here, unlike torch's: the
        fused gradient kernels overwrite ``.grad``, and a graph keeps its
        pointer); ``set_to_none=True`` drops them instead."""
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def covers(self, tensors):
        """True when the parameters are exactly ``tensors``, in that order."""
        mine = self.params
        return len(mine) == len(tensors) and all(a is b for a, b in zip(mine, tensors))

    def step_count(self):
        """The device's step count (synchronises)."""
        return int(self._state[0].item())

    def state_dict(self):
        """``torch.optim.Adam``'s format: ``state[i]`` = ``step`` (0-d float32,
        on the CPU as Adam keeps it), ``exp_avg``, ``exp_avg_sq`` (copies);
        ``param_groups`` with Adam's keys. ``torch.optim.Adam`` over the same
        parameters loads it. Synchronises."""
        k = self.step_count()
        state = {i: {"step": torch.tensor(float(k), dtype=torch.float32),
                     "exp_avg": self.exp_avg[i].clone(), "exp_avg_sq": self.exp_avg_sq[i].clone()}
                 for i in range(len(self.params))} if k else {}
        g = self.param_groups[0]
        group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": 0,
                 "amsgrad": False, "maximize": bool(g["maximize"]), "foreach": None,
                 "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": False, "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict):
        """Load a ``state_dict()`` of this class or of a ``torch.optim.Adam``
        over the same parameters: one group, no weight decay, no amsgrad, one
        ``step`` for all parameters (anything else is a ValueError). Moments
        and count are copied IN PLACE into the existing storage; ``lr``,
        ``betas``, ``eps`` and ``maximize`` are taken from the group."""
        groups, state = state_dict["param_groups"], state_dict["state"]
        n = len(self.params)
        if len(groups) != 1 or len(groups[0]["params"]) != n:
            raise ValueError(f"FusedAdam: need one parameter group of {n} parameters")
        g = groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False):
            raise ValueError("FusedAdam: a state with weight_decay or amsgrad is unsupported")
        ids = list(g["params"])
        have = [i for i in ids if i in state and len(state[i])]
        if have and len(have) != n:
            raise ValueError("FusedAdam: the state covers some parameters only; their step "
                             "counts differ")
        steps = [float(state[i]["step"]) for i in have]
        if any(s != steps[0] for s in steps):
            raise ValueError(f"FusedAdam: the parameters' step counts differ ({steps}); one "
                             "count serves all")
        k = steps[0] if steps else 0.0
        if k < 0 or k != int(k):
            raise ValueError(f"FusedAdam: step={k} is not a whole number >= 0")
        for j, i in enumerate(have):
            for name, dst in (("exp_avg", self.exp_avg[j]), ("exp_avg_sq", self.exp_avg_sq[j])):
                src = state[i][name]
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError(f"FusedAdam: state[{i}].{name} has shape "
                                     f"{tuple(src.shape)}, the parameter {tuple(dst.shape)}")
        for j, i in enumerate(have):
            self.exp_avg[j].copy_(state[i]["exp_avg"])
            self.exp_avg_sq[j].copy_(state[i]["exp_avg_sq"])
        if not have:
            self._flat.zero_()
        self._state.zero_()
        self._state[0] = int(k)
        mine = self.param_groups[0]
        mine.update(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"],
                    maximize=bool(g.get("maximize", False)))
        self._hyper()


def check_max_grad_norm(max_grad_norm):
    """``max_grad_norm`` as a float: > 0 and not NaN (``inf`` records the norm
    and clips nothing); anything else is a ValueError."""
    g = float(max_grad_norm)
    if not g > 0.0:
        raise ValueError(f"max_grad_norm={max_grad_norm} must be > 0 (inf: record the norm only)")
    return g


def check_target_kl(target_kl):
    """``target_kl`` as a float; ValueError unless it is > 0 (``inf``
    monitors only), as ``marlnav_ppo_train_phase_monitored`` demands."""
    k = float(target_kl)
    if not k > 0.0:     # a NaN is not greater
        raise ValueError(f"target_kl={target_kl!r} must be > 0 (inf: monitor only)")
    return k


def check_diag_out(diag_out, device, rows=1, what="diag_out"):
    """ValueError unless ``diag_out`` is a contiguous float64 tensor of
    ``rows`` x 5 elements on ``device``."""
    n = rows * abi.DIAG_ROW
    if (not torch.is_tensor(diag_out) or diag_out.dtype != _F64 or diag_out.device != device
            or diag_out.numel() != n or not diag_out.is_contiguous()):
        raise ValueError(f"{what}: need a contiguous float64 tensor of {n} elements on {device}")


def _train_steps(ppo, update_steps, network, buffer, optimizer, num_epochs, batch_size, log,
                 max_grad_norm, norm_log, steps_table):
    """The shuffled mode's host loop: row e of ``steps_table`` is epoch e's
    permutation, cut by ``shuffled_minibatches``; one ``*_update_steps`` per
    minibatch."""
    ppo._require(buffer)
    if torch.is_tensor(steps_table):
        if steps_table.device.type != 'cpu':
            raise ValueError("steps_table: need a host (E, L) array, got a tensor on "
                             f"{steps_table.device} (copy ppo.last_steps[...] to the host)")
        steps_table = steps_table.tolist()
    rows = [list(r) for r in steps_table]
    if len(rows) != int(num_epochs) or any(len(r) != len(buffer) for r in rows):
        raise ValueError(f"steps_table: need {int(num_epochs)} rows of {len(buffer)} steps")
    if not (isinstance(optimizer, FusedAdam) and optimizer.covers(network)):
        raise ValueError("steps_table needs a FusedAdam over exactly this network's parameters "
                         "in order")
    _check_norm_log(max_grad_norm, norm_log)
    _run_updates(ppo, [steps for perm in rows for steps in shuffled_minibatches(perm, batch_size)],
                 lambda steps, norm: update_steps(buffer, steps, optimizer,
                                                  max_grad_norm=max_grad_norm, norm_out=norm),
                 log, norm_log)


def _check_norm_log(max_grad_norm, norm_log):
    if max_grad_norm is not None:
        check_max_grad_norm(max_grad_norm)
    elif norm_log is not None:
        raise ValueError("norm_log needs max_grad_norm (inf records the norms only)")


def _run_updates(ppo, minibatches, update, log, norm_log):
    """What both host loops do per minibatch: ``update(minibatch, norm)`` ->
    loss, ``norm`` the update's cell of one allocation (appended to the list
    ``norm_log``) or None where the norms are not logged; the loss, left on
    the device, is appended to ``log``."""
    cells = None
    if norm_log is not None:                # one allocation, an element per update
        cells = torch.empty(len(minibatches), dtype=_F64, device=ppo.device)
    for k, minibatch in enumerate(minibatches):
        norm = None
        if cells is not None:
            norm = cells[k]
            norm_log.append(norm)
        loss = update(minibatch, norm)
        if log is not None:
            log.append(loss)


def _train(ppo, loss_grad, update, network, buffer, optimizer, num_epochs, batch_size, log,
           max_grad_norm=None, norm_log=None):
    ppo._require(buffer)
    bounds = minibatch_bounds(len(buffer), batch_size)
    # a FusedAdam over exactly this network's parameters: one C call per
    # minibatch; any other optimiser: the two calls
    one_call = isinstance(optimizer, FusedAdam) and optimizer.covers(network)
    _check_norm_log(max_grad_norm, norm_log)
    if max_grad_norm is not None and not one_call:
        raise ValueError("max_grad_norm needs a FusedAdam over exactly this network's "
                         "parameters in order: the clipping is part of its step (clip any "
                         "other optimiser's gradients yourself between loss_grad and step)")

    def one(lo_hi, norm):
        if one_call:
            return update(buffer, *lo_hi, optimizer, max_grad_norm=max_grad_norm, norm_out=norm)
        loss = loss_grad(buffer, *lo_hi)
        optimizer.step()
        return loss

    _run_updates(ppo, bounds * int(num_epochs), one, log, norm_log)


def train_actor(ppo, buffer, optimizer, num_epochs, batch_size, log=None, max_grad_norm=None,
                norm_log=None, steps_table=None):
    """MAPPO.train_actor (models.py:160-178): per epoch and minibatch
    (``minibatch_bounds``) the fused loss and gradients, ``optimizer.step()``,
    then ``log.append(loss)`` with the loss left on the device. ``optimizer``
    is the caller's (the reference's: ``Adam(actor.parameters(), lr,
    maximize=True)``). Nothing is printed and nothing synchronises.

    With a ``FusedAdam`` over exactly the actor's six parameters in
    ``_POLICY_PARAMS`` order (``FusedAdam(actor.parameters(), ...)`` of the
    reference's module) the two calls of a minibatch become the one call
    ``ppo.actor_update``, with equal bits, and a whole epoch can be captured
    in a graph.

    ``max_grad_norm`` (None: the above): every update clips its gradient by
    the global L2 norm first (``ppo.actor_update(..., max_grad_norm=...)``,
    DESIGN.md §16) and, with a list ``norm_log``, appends the norm before
    clipping (0-d float64 device tensor). This needs that ``FusedAdam``: with
    any other optimiser it is a ValueError.

    ``steps_table`` (None: the above): a host ``(num_epochs, len(buffer))``
    array of steps, row e the permutation of epoch e. The
    epochs then run over the minibatches of ``shuffled_minibatches(row,
    batch_size)``, one ``ppo.actor_update_steps`` each, and use every stored
    step once per epoch: the host loop that ``training.train_phase(...,
    shuffle=seed)`` equals bit for bit when given its
    ``ppo.last_steps['actor']``. Needs that ``FusedAdam`` too."""
    if steps_table is not None:
        return _train_steps(ppo, ppo.actor_update_steps, ppo._network_params("actor"), buffer,
                            optimizer, num_epochs, batch_size, log, max_grad_norm, norm_log,
                            steps_table)
    _train(ppo, ppo.actor_loss_grad, ppo.actor_update, ppo._network_params("actor"), buffer,
           optimizer, num_epochs, batch_size, log, max_grad_norm, norm_log)


def train_critic(ppo, buffer, optimizer, num_epochs, batch_size, log=None, max_grad_norm=None,
                 norm_log=None, steps_table=None):
    """MAPPO.train_critic (models.py:180-198), as ``train_actor``
    (``steps_table`` included: ``ppo.critic_update_steps``)."""
    if steps_table is not None:
        return _train_steps(ppo, ppo.critic_update_steps, ppo._network_params("critic"), buffer,
                            optimizer, num_epochs, batch_size, log, max_grad_norm, norm_log,
                            steps_table)
    _train(ppo, ppo.critic_loss_grad, ppo.critic_update, ppo._network_params("critic"), buffer,
           optimizer, num_epochs, batch_size, log, max_grad_norm, norm_log)
