"""Running a trained policy on the device without training it: the reference's
rendering path (marlnav/animation.py:40-71, ``init_render`` :80-96) minus the
drawing, plus the episode figures an evaluation reports.

* ``FusedActor(actor)`` - ``Actor.forward`` (models.py:27-36) and ``dist.loc``
  or ``dist.sample()`` as one launch of libmarlnav.so ``marlnav_actor_act``:
  the actor third of ``FusedPolicy``'s kernel, without the critic, the
  log-probabilities and (for the mean action) the covariance.
  ``FusedActor.from_state_dict`` takes the reference's ``*_actor.pt``.
* ``evaluate(env, actor, num_steps)`` - ``num_steps`` steps of the env under
  the actor as ONE C call (``marlnav_rollout_evaluate``): no rollout buffer is
  written; per-env episode returns and lengths are accumulated on the device
  after every step, and one env's trajectory can be recorded for drawing.
* ``EvalResult`` - what ``evaluate`` returns.
"""
import ctypes
import math
from types import SimpleNamespace

import torch

from . import abi
from .rollout import _POLICY_PARAMS, FusedPolicy, _stream

_ACTOR_PARAMS = tuple((f, layer, attr) for f, m, layer, attr in _POLICY_PARAMS if m == "actor")
_MODES = {"mean": abi.ACT_MEAN, "sample": abi.ACT_SAMPLE}
# the reference's Actor.state_dict() (models.py:20-25), in _ACTOR_PARAMS order
STATE_DICT_KEYS = tuple(f"{layer}.{attr}" for _, layer, attr in _ACTOR_PARAMS)


def _actor_params(actor, who):
    """The six live parameter tensors of ``actor`` as ``[(field, tensor)]``,
    checked once as ``rollout._module_params`` checks them (fp32, one HIP
    device, contiguous, the reference's shapes); -> (params, device, H, D)."""
    params = [(f, getattr(getattr(actor, layer), attr)) for f, layer, attr in _ACTOR_PARAMS]
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
    want = {"actor_fc1_w": (H, D), "actor_fc1_b": (H,), "actor_mu_w": (2, H),
            "actor_mu_b": (2,), "actor_std_w": (2, H), "actor_std_b": (2,)}
    for f, t in params:
        if tuple(t.shape) != want[f]:
            raise ValueError(f"{f}: shape {tuple(t.shape)}, expected {want[f]}")
    return params, dev, int(H), int(D)


def _mode(mode):
    if mode not in _MODES:
        raise ValueError(f"mode must be 'mean' (dist.loc) or 'sample' (dist.sample()), got {mode!r}")
    return _MODES[mode]


class FusedActor(object):
    """``Actor`` (models.py:14-36) evaluated forward-only by one HIP launch
    per call (include/marlnav.h ``marlnav_actor_act``), as the reference's
    renderer uses it (animation.py:43-48): ``mode='mean'`` gives ``dist.loc``,
    ``mode='sample'`` gives ``dist.sample()`` with the bits ``FusedPolicy.act``
    gives the same seed, step index and env offset (or the same ``eps``).

    ``actor`` is any object with the reference's attribute names (``fc1``,
    ``fc_mu``, ``fc_std``) and shapes, checked here once; the kernel reads the
    parameter tensors themselves on every call. The number of agents is taken
    from the observations of each call."""

    def __init__(self, actor, seed=0, env_offset=0):
        self.actor = actor
        self._params, self.device, H, D = _actor_params(actor, "FusedActor")
        self.hidden_size, self.obs_dim = H, D
        self.seed = int(seed) & (2 ** 64 - 1)
        self.step_idx = 0          # next step index of the kernel's own normals
        self._lib = abi.load_library()
        self._dims = abi.MarlnavPolicyDims(obs_dim=D, hidden_size=H, env_offset=int(env_offset))
        self._bufs = abi.MarlnavPolicyBuffers()

    @classmethod
    def from_state_dict(cls, state_dict, device, seed=0, env_offset=0):
        """From the reference's ``*_actor.pt`` contents (``torch.load(file,
        weights_only=True)``, animation.py:87-88): exactly the keys
        ``fc1.weight``, ``fc1.bias``, ``fc_mu.weight``, ``fc_mu.bias``,
        ``fc_std.weight``, ``fc_std.bias`` with the reference's shapes, copied
        to ``device`` as float32."""
        keys = set(state_dict.keys())
        if keys != set(STATE_DICT_KEYS):
            raise ValueError(f"an actor state dict has the keys {sorted(STATE_DICT_KEYS)}; "
                             f"missing {sorted(set(STATE_DICT_KEYS) - keys)}, "
                             f"unexpected {sorted(keys - set(STATE_DICT_KEYS))}")
        w1 = state_dict["fc1.weight"]
        if not isinstance(w1, torch.Tensor) or w1.dim() != 2:
            raise ValueError("fc1.weight must be a (H, D) tensor")
        H = int(w1.shape[0])
        want = {"fc1.weight": tuple(w1.shape), "fc1.bias": (H,), "fc_mu.weight": (2, H),
                "fc_mu.bias": (2,), "fc_std.weight": (2, H), "fc_std.bias": (2,)}
        for k in STATE_DICT_KEYS:
            t = state_dict[k]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != want[k]:
                got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"{k}: shape {got}, expected {want[k]}")
        layers = {}
        for k in STATE_DICT_KEYS:
            layer, attr = k.split(".")
            t = state_dict[k].detach().to(device=device, dtype=torch.float32).contiguous()
            setattr(layers.setdefault(layer, SimpleNamespace()), attr, t)
        return cls(SimpleNamespace(**layers), seed=seed, env_offset=env_offset)

    def _check(self, t, shape, what):
        if (t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != shape
                or not t.is_contiguous()):
            raise ValueError(f"{what}: need a contiguous float32 {shape} tensor on "
                             f"{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t.data_ptr()

    def act(self, obs_norm, mode='mean', eps=None, step_idx=None, out=None, eps_out=None):
        """obs_norm (P, A, D) normalised observations -> actions (P, A, 2) in
        policy scale. ``mode='mean'``: ``dist.loc`` (animation.py:48);
        ``eps`` / ``eps_out`` do not apply. ``mode='sample'``: ``dist.sample()``
        (:46) with the standard normals ``eps`` (P*A, 2), or the kernel's own
        for ``(seed, step_idx)`` (``step_idx`` None: this actor's running
        counter, which then advances); ``eps_out`` receives the normals used.
        ``out``: the tensor to write into. One launch on the current stream,
        no synchronisation."""
        m = _mode(mode)
        if obs_norm.dim() != 3:
            raise ValueError(f"obs_norm must be (P, A, D), got {tuple(obs_norm.shape)}")
        P, A, D = int(obs_norm.shape[0]), int(obs_norm.shape[1]), self.obs_dim
        if m == abi.ACT_MEAN and (eps is not None or eps_out is not None):
            raise ValueError("mode='mean' draws nothing: eps and eps_out apply to mode='sample'")
        b, d = self._bufs, self._dims
        b.obs_norm = self._check(obs_norm, (P, A, D), "obs_norm")
        if out is None:
            out = torch.empty(P, A, 2, device=self.device)
        b.actions = self._check(out, (P, A, 2), "out (actions)")
        b.eps = None if eps is None else self._check(eps, (P * A, 2), "eps")
        b.eps_out = None if eps_out is None else self._check(eps_out, (P * A, 2), "eps_out")
        for f, t in self._params:
            setattr(b, f, t.data_ptr())
        if step_idx is None:
            step_idx = self.step_idx
            if m == abi.ACT_SAMPLE and eps is None:
                self.step_idx += 1
        d.num_parallel, d.num_agents = P, A
        abi.check(self._lib.marlnav_actor_act(ctypes.byref(d), ctypes.byref(b), m, self.seed,
                                              int(step_idx), _stream(self.device)), self._lib)
        return out


class EvalResult(object):
    """What ``evaluate`` returns. The per-env device tensors (each (P,)):
    ``ep_count``, ``ret_sum``, ``ret_sqsum``, ``ret_min``, ``ret_max``,
    ``len_sum``, ``partial_count`` over the whole episodes that ended inside
    the call, and ``cur_return``, ``cur_len``, ``whole`` of the episode still
    under way; ``totals_i`` (episodes, partials, len_sum) and ``totals_f``
    (ret_sum, ret_sqsum, min, max), the device's totals over the envs.

    ``episodes``, ``partial_episodes``, ``mean_return``, ``std_return``
    (unbiased), ``min_return``, ``max_return`` and ``mean_length`` are formed
    on the host from the totals when first read (one synchronising copy).
    With no whole episode the means are NaN and min / max stay +-inf; with
    one, the std is NaN.

    ``endings``: ``{'trunc', 'col', 'tar'}``, how many episodes ended each way
    during the call (the env's counters after minus before; they are not
    zeroed); None under stream capture. ``trace``: None, or the traced env's
    ``states`` (T+1, A, 5), ``obstacles`` (T+1, S, 2), ``target`` (T+1, 2),
    row 0 before the first step, and ``reward``, ``terminated``, ``truncated``
    (T,)."""

    SCALARS = ("episodes", "partial_episodes", "mean_return", "std_return", "min_return",
               "max_return", "mean_length")

    def __init__(self, num_steps, mode, per_env, totals_i, totals_f, endings, trace):
        self.num_steps, self.mode = num_steps, mode
        for name, t in per_env.items():
            setattr(self, name, t)
        self.totals_i, self.totals_f = totals_i, totals_f
        self.endings, self.trace = endings, trace
        self._host = None

    def _totals(self):
        if self._host is None:
            n, partials, len_sum = (int(v) for v in self.totals_i.tolist())
            s, sq, mn, mx = self.totals_f.tolist()
            self._host = summary_stats(n, partials, len_sum, s, sq, mn, mx)
        return self._host

    def __getattr__(self, name):
        if name in EvalResult.SCALARS:
            return self._totals()[name]
        raise AttributeError(name)

    def as_dict(self):
        """The scalars, ``num_steps``, ``mode`` and ``endings`` (JSON-ready)."""
        d = {"num_steps": self.num_steps, "mode": self.mode}
        d.update(self._totals())
        d["endings"] = self.endings
        return d


def summary_stats(episodes, partials, len_sum, ret_sum, ret_sqsum, ret_min, ret_max):
    """The host's part of the summary: mean, unbiased std and mean length from
    the device's totals."""
    n = int(episodes)
    mean = ret_sum / n if n else math.nan
    std = math.sqrt(max(ret_sqsum - ret_sum * ret_sum / n, 0.0) / (n - 1)) if n > 1 else math.nan
    return {"episodes": n, "partial_episodes": int(partials), "mean_return": mean,
            "std_return": std, "min_return": ret_min, "max_return": ret_max,
            "mean_length": len_sum / n if n else math.nan}


def evaluate(env, actor, num_steps, mode='mean', trace_env=None):
    """``num_steps`` steps of ``env`` under ``actor`` as ONE C call (libmarlnav.so
    ``marlnav_rollout_evaluate``): what the reference's renderer does per frame
    (animation.py:40-50: normalise the observations, ``Actor.forward``,
    ``dist.loc`` for ``mode='mean'`` or ``dist.sample()`` for ``'sample'``,
    ``ActionScaler``, ``Env.step``), with the actor launch, the step launch and
    a small tracker launch per step enqueued back to back on the current
    stream. Nothing of a rollout buffer is written. Returns an ``EvalResult``.

    ``actor``: a ``FusedActor``, or a ``FusedPolicy`` whose actor tensors, seed
    and ``step_idx`` are used; in sample mode its ``step_idx`` advances by
    ``num_steps``. ``trace_env``: the local index of an env whose states,
    obstacles and target are recorded after every step (``EvalResult.trace``).

    The env is not reset (``reset()`` only marks the envs): an env that enters
    the call inside an episode (``_step_num != 0``) closes a *partial* episode
    first, which is counted apart and enters no return figure. The env ends
    exactly as ``num_steps`` calls of ``env.step`` on those actions leave it
    (states, step index, ``_reinit_mask``); tensors the caller still holds from
    before the call are not written, as in ``collect_fused``, and the same
    things are refused before anything is launched: an env in reference-RNG
    mode or with a user-assigned init sampler, no attached normaliser or action
    scaler, and stream capture unless ``env.allow_graph_capture`` is set."""
    who = "evaluate"
    m = _mode(mode)
    T = int(num_steps)
    if T < 1:
        raise ValueError(f"num_steps={num_steps} must be >= 1")
    if not isinstance(actor, (FusedActor, FusedPolicy)):
        raise TypeError(f"{who} takes a FusedActor or a FusedPolicy, got {type(actor).__name__}")
    if env._rng != 'native' or env._init_sampler is not env._default_init_sampler:
        raise RuntimeError(f"{who} needs an env in native-RNG mode with its default init "
                           "sampler: a reference-RNG or user-assigned sampler is called on the "
                           "host every step; step such an env in a loop around actor.act()")
    if env._normalizer is None or env._action_scaler is None:
        raise RuntimeError(f"{who} needs env.attach_normalizer(...) and "
                           "env.attach_action_scaler(...): the actor reads normalised "
                           "observations and the env takes policy-scale actions")
    dev = env.device
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing and not env.allow_graph_capture:
        raise RuntimeError(f"{who} under stream capture replays the steps' re-init draws on "
                           "every graph replay; set env.allow_graph_capture = True to accept "
                           "that (timing runs)")
    P, A, D = env._obs_shape
    if D != actor.obs_dim or (isinstance(actor, FusedPolicy) and A != actor.num_agents):
        raise ValueError(f"the actor is built for rows of {actor.obs_dim} features"
                         + (f" and {actor.num_agents} agents" if isinstance(actor, FusedPolicy)
                            else "") + f", the env has {A} agents x {D}")
    if actor.device != dev:
        raise ValueError(f"the actor is on {actor.device}, the env on {dev}")
    if trace_env is not None and not 0 <= int(trace_env) < P:
        raise ValueError(f"trace_env={trace_env} outside [0, {P})")
    env._sync_params()
    if any(env._engine.shared_state()):
        env._unshare_state(multi_step=True)
    if not env._engine.fast_ok:
        raise RuntimeError(f"{who}: the env's parameters are not in sync with its engine and "
                           "could not be synced")
    lib = abi.load_library()
    S = int(env._obstacles.shape[1])
    e = abi.MarlnavEvalBuffers(trace_env=-1 if trace_env is None else int(trace_env))
    raw, norm_a, norm_b = env._new_obs(), env._new_obs(), env._new_obs()
    actions = torch.empty(P, A, 2, device=dev)
    reward = torch.empty(P, device=dev)
    flags = torch.empty(2, P, dtype=torch.bool, device=dev)
    e.obs_norm_a, e.obs_norm_b, e.actions = norm_a.data_ptr(), norm_b.data_ptr(), actions.data_ptr()
    e.reward, e.terminated, e.truncated = reward.data_ptr(), flags[0].data_ptr(), flags[1].data_ptr()
    per_env = {}
    for name, dtype in abi.EVAL_ENV_FIELDS:
        per_env[name] = torch.empty(P, dtype=getattr(torch, dtype), device=dev)
        setattr(e, name, per_env[name].data_ptr())
    totals_i = torch.empty(3, dtype=torch.int64, device=dev)
    totals_f = torch.empty(4, dtype=torch.float64, device=dev)
    e.totals_i, e.totals_f = totals_i.data_ptr(), totals_f.data_ptr()
    trace = None
    if trace_env is not None:
        trace = {"states": torch.empty(T + 1, A, 5, device=dev),
                 "obstacles": torch.empty(T + 1, S, 2, device=dev),
                 "target": torch.empty(T + 1, 2, device=dev),
                 "reward": torch.empty(T, device=dev),
                 "terminated": torch.empty(T, dtype=torch.bool, device=dev),
                 "truncated": torch.empty(T, dtype=torch.bool, device=dev)}
        for name, t in trace.items():
            setattr(e, "trace_" + name, t.data_ptr())
    pd = abi.MarlnavPolicyDims(num_parallel=P, num_agents=A, obs_dim=D,
                               hidden_size=actor.hidden_size, env_offset=actor._dims.env_offset)
    pb = abi.MarlnavPolicyBuffers()
    for f, t in actor._params[:len(_ACTOR_PARAMS)]:
        setattr(pb, f, t.data_ptr())
    before = None
    if not capturing:
        # the three episode counters before the call, left on the device
        before = torch.empty(3, dtype=torch.int64, device=dev)
        abi.check(lib.marlnav_counters_total(ctypes.byref(env._dims), env._counters.data_ptr(),
                                             before.data_ptr(), _stream(dev)), lib)
    env._engine.evaluate(abi.fn_addr(lib.marlnav_rollout_evaluate), bytes(pd), bytes(pb), bytes(e),
                         raw.data_ptr(), T, m, actor.seed, actor.step_idx)
    del raw, norm_a, norm_b, actions, reward     # stream-ordered: reused after the kernels
    if m == abi.ACT_SAMPLE:
        actor.step_idx += T
    env._reinit_mask = torch.where(torch.logical_or(flags[0], flags[1]), 1, 0)  # environment.py:102
    per_env["whole"] = per_env["whole"].view(torch.bool)
    endings = None
    if not capturing:
        after = env._counter_totals()                     # the call's one synchronisation
        endings = dict(zip(("trunc", "col", "tar"),
                           (a - b for a, b in zip(after, before.tolist()))))
    return EvalResult(T, mode, per_env, totals_i, totals_f, endings, trace)
