"""A plain torch restatement of the update half of the training loop
(marlnav/models.py:160-198, 270-316): the actor and critic losses of one
minibatch through tensor ops and autograd in whatever dtype the weights have,
the minibatch slicing rule, the loader of fixture F7-ppo
(tests/golden/ppo_f7.npz, written by tests/golden/make_ppo_golden.py from the
reference's own ``_actor_loss`` / ``_critic_loss``) and the parity measure
both PPO test files use. No torch.nn module and no torch.distributions.

The quirks restated (they are the contract of include/marlnav.h
``marlnav_ppo_actor_grad`` / ``marlnav_ppo_critic_grad``):

* no activation after the actor's fc1; softplus(fc_std) (threshold 20) is the
  COVARIANCE diagonal v, so log_prob = -sum (a - mu)^2 / v / 2 - sum log v / 2
  - log 2 pi and entropy = 1 + log 2 pi + sum log v / 2;
* the advantage of agent row i (rows in (t, p, a) order) is ret[i mod N] -
  val[i mod N], N = T P: ``repeat(num_agents)`` on the (t, p) vectors, not the
  row's own env i // A;
* the returns are float64, so the clipped surrogate and the critic's squares
  are float64 while the ratio, the entropy and the clamp stay in the weights'
  dtype; the bounds 1 -+ epsilon, values -+ epsilon and ent_const are Python
  scalars;
* the last minibatch is ``buffer[start:-1]``.
"""
import json
import math
import os

import numpy as np
import torch

from policy_ref import ACTOR_KEYS, CRITIC_KEYS, FACTOR  # noqa: F401  (the project's 4)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAM_KEYS = tuple("actor." + k for k in ACTOR_KEYS) + tuple("critic." + k for k in CRITIC_KEYS)
ACTOR_PARAMS = PARAM_KEYS[:6]
CRITIC_PARAMS = PARAM_KEYS[6:]
DATA_KEYS = ("obs", "actions", "log_probs", "values", "returns")


def actor_terms(w, obs, actions):
    """The new log-prob and the entropy of every agent row, (M,) each, of the
    diagonal normal the actor puts out for obs (T, P, A, D) at actions
    (T, P, A, 2)."""
    T, P, A, D = obs.shape
    M = T * P * A
    x = obs.reshape(M, D)
    h = x @ w["actor.fc1.weight"].T + w["actor.fc1.bias"]
    mu = torch.tanh(h @ w["actor.fc_mu.weight"].T + w["actor.fc_mu.bias"])
    pre = h @ w["actor.fc_std.weight"].T + w["actor.fc_std.bias"]
    v = torch.where(pre > 20, pre, torch.log1p(torch.exp(torch.clamp(pre, max=20.0))))
    d = actions.reshape(M, 2) - mu
    half_log_det = 0.5 * torch.log(v).sum(-1)
    new_lp = -0.5 * (d * d / v).sum(-1) - half_log_det - math.log(2 * math.pi)
    entropy = 1.0 + math.log(2 * math.pi) + half_log_det
    return new_lp, entropy


def clipped_surrogate(new_lp, entropy, log_probs, values, returns, A, epsilon, ent_const,
                      advantage_of_own_env=False):
    """The actor loss from the rows' new log-probs and entropies (M,), the
    stored log_probs (T, P*A), values (T, P, 1) and returns (T, P).
    ``advantage_of_own_env``: the WRONG pairing (row i with env i // A), kept
    so a test can show the fixture tells them apart."""
    N = returns.numel()
    M = N * A
    adv = returns.reshape(N) - values.reshape(N)
    adv = adv.repeat_interleave(A) if advantage_of_own_env else adv.repeat(A)
    ratio = torch.exp(new_lp - log_probs.reshape(M))
    clip_loss = torch.mean(torch.minimum(ratio * adv,
                                         torch.clamp(ratio, 1 - epsilon, 1 + epsilon) * adv))
    return clip_loss + ent_const * torch.mean(entropy)


def actor_loss(w, obs, actions, log_probs, values, returns, epsilon, ent_const,
               advantage_of_own_env=False):
    """w: {'actor.fc1.weight': ...}; obs (T, P, A, D), actions (T, P, A, 2),
    log_probs (T, P*A), values (T, P, 1), returns (T, P). -> 0-d loss."""
    new_lp, entropy = actor_terms(w, obs, actions)
    return clipped_surrogate(new_lp, entropy, log_probs, values, returns, obs.shape[2], epsilon,
                             ent_const, advantage_of_own_env)


def critic_loss(w, obs, values, returns, epsilon):
    """-> 0-d loss; shapes as in ``actor_loss``."""
    T, P, A, D = obs.shape
    N = T * P
    h = torch.relu(obs.reshape(N, A * D) @ w["critic.fc1.weight"].T + w["critic.fc1.bias"])
    nv = (h @ w["critic.fc2.weight"].T + w["critic.fc2.bias"]).reshape(N)
    val, ret = values.reshape(N), returns.reshape(N)
    diff = (nv - ret) ** 2
    clamped = torch.clamp(nv, min=val - epsilon, max=val + epsilon)
    return torch.mean(torch.maximum(diff, (clamped - ret) ** 2))


def loss_and_grads(which, w, data, epsilon, ent_const, **kw):
    """``which`` 'actor' | 'critic'; w: the ten weights (leaf copies are made
    here); data: dict of DATA_KEYS tensors. -> (loss, {key: grad}) detached."""
    keys = ACTOR_PARAMS if which == "actor" else CRITIC_PARAMS
    leaf = {k: w[k].detach().clone().requires_grad_(True) for k in keys}
    if which == "actor":
        loss = actor_loss(leaf, data["obs"], data["actions"], data["log_probs"], data["values"],
                          data["returns"], epsilon, ent_const, **kw)
    else:
        loss = critic_loss(leaf, data["obs"], data["values"], data["returns"], epsilon)
    grads = torch.autograd.grad(loss, [leaf[k] for k in keys])
    return loss.detach(), dict(zip(keys, (g.detach() for g in grads)))


def list_minibatches(buffer, batch_size):
    """models.py:165-172 on a Python list: the slices the loops train on."""
    n, out = len(buffer), []
    for j in range(n // batch_size):
        start = j * batch_size
        end = start + batch_size if start + batch_size < n else -1
        out.append(buffer[start:end])
    return out


# ------------------------------------------------------------------ launch plan
# The host side of csrc/marlnav_ppo.hip restated: which kernels a minibatch of
# T x P env rows of A agents, O obstacles and H hidden units launches, and on
# what grid. tests/test_ppo_cpu.py holds it to marlnav_ppo_work_size and pins
# every named shape of the GPU tests to the path it is there for.
THREADS = 256
ACTOR_TILE, ACTOR_MAX_BLOCKS, ACTOR_MIN_ROWS = 256, 1024, 1024
CRITIC_TILE, CRITIC_TARGET_BLOCKS, CRITIC_FORWARD_BLOCKS = 64, 512, 1024
CRITIC_MAX_WORK = 8 << 20       # fp64 elements of chunk partials
CRITIC_MAX_DH = 32 << 20        # floats of dh shared through the workspace


def _cdiv(a, b):
    return -(-a // b)


def launch_plan(T, P, A, O, H):
    """-> {'critic': {...}, 'actor': {...}, 'work_size': doubles}.

    critic: kernel ('fused8' | 'fused64' | 'split8' | 'split64'; a split one
    is critic_pass<1, kForward> then critic_pass<8 | 64, kBackward>),
    col_tiles, last_tile_cols, unit_slices, units_per_block, unit_groups,
    forward_groups (unit groups of the kForward launch, 0 when fused),
    forward_blocks, chunks, tiles_per_chunk, last_tile_rows, vec4 (what the
    row width allows; the launch also wants obs 16-byte aligned).
    actor: blocks, tiles_per_block, slices, col_rounds, finish_groups."""
    D = 2 + 2 * O + 2 * (A - 1)
    AD, N = A * D, T * P
    M = N * A
    # actor_grid, the phase-2 ownership of actor_pass, the groups of actor_finish
    rows = max(_cdiv(M, ACTOR_MAX_BLOCKS), ACTOR_MIN_ROWS)
    rows = _cdiv(rows, ACTOR_TILE) * ACTOR_TILE
    ncol = D + 1
    nS = 4 * ncol + 2
    actor = {"blocks": _cdiv(M, rows), "tiles_per_block": rows // ACTOR_TILE,
             "slices": 1 if ncol >= THREADS else THREADS // ncol,
             "col_rounds": _cdiv(ncol, THREADS),
             "finish_groups": 1 if nS >= THREADS else THREADS // nS}
    actor_work = actor["blocks"] * nS
    # critic_tiling
    kc = min(AD, THREADS)
    col_tiles = _cdiv(AD, kc)
    us_n = THREADS // kc
    jt = 8 if us_n >= 2 else 64
    ub = us_n * jt
    if ub > 64:
        us_n, ub = 64 // jt, 64
    unit_groups = _cdiv(H, ub)
    # critic_grid
    stride = H * AD + 2 * H + 2
    want = max(min(CRITIC_TARGET_BLOCKS // (col_tiles * unit_groups), CRITIC_MAX_WORK // stride), 1)
    tiles = _cdiv(N, CRITIC_TILE)
    tiles_per_chunk = _cdiv(tiles, want)
    chunks = _cdiv(N, tiles_per_chunk * CRITIC_TILE)
    critic_work = chunks * stride
    # critic_split, critic_forward_grid, dh_pitch
    pitch = _cdiv(H, 64) * 64
    split = col_tiles * unit_groups > 1 and N * pitch <= CRITIC_MAX_DH
    forward_blocks = 0
    if split:
        frows = _cdiv(_cdiv(N, CRITIC_FORWARD_BLOCKS), CRITIC_TILE) * CRITIC_TILE
        forward_blocks = _cdiv(N, frows)
        critic_work += forward_blocks * (2 * H + 2) + (N * pitch + 1) // 2
    critic = {"kernel": ("split" if split else "fused") + str(jt),
              "col_tiles": col_tiles, "last_tile_cols": AD - (col_tiles - 1) * kc,
              "unit_slices": us_n, "units_per_block": ub, "unit_groups": unit_groups,
              "forward_groups": _cdiv(H, 64) if split else 0, "forward_blocks": forward_blocks,
              "chunks": chunks, "tiles_per_chunk": tiles_per_chunk,
              "last_tile_rows": N - (tiles - 1) * CRITIC_TILE, "vec4": AD % 4 == 0}
    return {"critic": critic, "actor": actor, "work_size": max(actor_work, critic_work)}


def launch_path(T, P, A, O, H):
    """What the CPU tests pin per named shape: (critic kernel, column tiles,
    unit groups, tiles per chunk, actor slices, actor column rounds)."""
    p = launch_plan(T, P, A, O, H)
    c, a = p["critic"], p["actor"]
    return (c["kernel"], c["col_tiles"], c["unit_groups"], c["tiles_per_chunk"], a["slices"],
            a["col_rounds"])


# ------------------------------------------------------------------ fixture F7
_cache = {}


def manifest():
    if "manifest" not in _cache:
        with open(os.path.join(GOLDEN, "ppo_MANIFEST.json")) as fh:
            _cache["manifest"] = json.load(fh)
    return _cache["manifest"]


def case_names():
    return list(manifest()["cases"])


def load_case(name):
    """-> dict: T, P, A, O, H, D, epsilon, ent_const, the DATA_KEYS arrays,
    'w' (the perturbed fp32 weights), 'g32' / 'g64' (the reference's
    gradients per PARAM_KEYS), 'loss32' / 'loss64' ({'actor', 'critic'})."""
    if ("case", name) in _cache:
        return _cache[("case", name)]
    if "npz" not in _cache:
        _cache["npz"] = np.load(os.path.join(GOLDEN, "ppo_f7.npz"))
    z, info, arr = _cache["npz"], manifest()["cases"][name], {}
    for kind in ("f32", "f64"):
        blob, at = z[f"{name}.{kind}"], 0
        for key, shape in info["layout"][kind]:
            n = int(np.prod(shape))
            arr[key] = blob[at:at + n].reshape(shape)
            at += n
        assert at == blob.size
    c = {k: info[k] for k in ("T", "P", "A", "O", "H", "D")}
    c.update(name=name, epsilon=manifest()["epsilon"], ent_const=manifest()["ent_const"])
    for k in DATA_KEYS:
        c[k] = arr[k]
    c["w"] = {k: arr["w." + k] for k in PARAM_KEYS}
    c["g32"] = {k: arr["g32." + k] for k in PARAM_KEYS}
    c["g64"] = {k: arr["g64." + k] for k in PARAM_KEYS}
    c["loss32"] = {n: float(arr["loss32." + n][0]) for n in ("actor", "critic")}
    c["loss64"] = {n: float(arr["loss64." + n][0]) for n in ("actor", "critic")}
    _cache[("case", name)] = c
    return c


def tensors(c, device="cpu", dtype=torch.float32):
    """(w, data) of a loaded case as tensors; the returns stay float64."""
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)
    w = {k: t(v, dtype) for k, v in c["w"].items()}
    data = {k: t(c[k], torch.float64 if k == "returns" else dtype) for k in DATA_KEYS}
    return w, data


class Pooled(object):
    """Per parameter tensor (and per loss), pooled over the cases added: the
    largest |g - g64| / max|g64| of the reference side and of a candidate."""

    def __init__(self):
        self.ref, self.got = {}, {}

    @staticmethod
    def _measure(g, g64):
        g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
        assert g.size == g64.size and np.isfinite(g).all()
        scale = float(np.abs(g64).max())
        return float(np.abs(g.reshape(g64.shape) - g64).max()) / scale if scale else 0.0

    def add(self, key, got, ref32, truth64):
        self.got[key] = max(self.got.get(key, 0.0), self._measure(got, truth64))
        self.ref[key] = max(self.ref.get(key, 0.0), self._measure(ref32, truth64))

    def lines(self, who="kernel"):
        return [f"{k:22s} reference {self.ref[k]:.3e}  {who} {self.got[k]:.3e}  ratio "
                f"{self.got[k] / self.ref[k] if self.ref[k] else float('inf'):.2f}"
                for k in self.got]

    def failures(self):
        return [(k, self.got[k], self.ref[k]) for k in self.got
                if not self.got[k] <= FACTOR * self.ref[k]]
