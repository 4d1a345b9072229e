"""A plain torch restatement of the policy half of MAPPO.get_data
(marlnav/models.py:113-120: Actor.forward :27-36, the MultivariateNormal's
sample and log_prob, Critic.forward :51-56), the loader of fixture F6-policy
(tests/golden/policy_f6.npz, written by tests/golden/make_policy_golden.py
from the reference's modules) and the parity criterion both policy test files
use. No torch.nn module and no torch.distributions here: the formulas are
spelled out, quirks included -

* no activation after the actor's fc1;
* softplus(fc_std) is torch's (x itself when x > 20, else log1p(exp(x))) and
  is the COVARIANCE diagonal, so the standard deviation is its square root;
* log_prob = -(eps0^2 + eps1^2)/2 - (log v0 + log v1)/2 - log(2 pi).

Below the fixture's part: the generated shapes beyond the fixture's reach
(``SHAPES``, ``make_case``, ``generated``) with their per-shape criterion
(``check_shape``), the kernel's own formulation in torch (``collapsed_ref``,
CPU only), and a numpy restatement of the kernel's own normals
(``native_normals``).
"""
import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("actions", "log_probs", "values")
GROUPS = ("default", "sat")
# the kernel's (or a restatement's) largest fp32 error against the fp64
# values may be FACTOR times the reference's own largest fp32 error, per
# output kind and weight group, pooled over all cases
FACTOR = 4.0

ACTOR_KEYS = ("fc1.weight", "fc1.bias", "fc_mu.weight", "fc_mu.bias", "fc_std.weight",
              "fc_std.bias")
CRITIC_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def policy_ref(w, obs, eps, variance_is_std=False):
    """w: {'actor.fc1.weight': ..., 'critic.fc2.bias': ...} tensors in
    nn.Linear's layout; obs (P, A, D); eps (P*A, 2); all of one dtype and
    device. Returns (actions (P, A, 2), log_probs (P*A,), values (P, 1)).
    ``variance_is_std``: the WRONG reading (softplus output used as the
    standard deviation), kept so a test can show the fixture tells them apart."""
    P, A, D = obs.shape
    x = obs.reshape(P * A, D)
    h = x @ w["actor.fc1.weight"].T + w["actor.fc1.bias"]
    mu = torch.tanh(h @ w["actor.fc_mu.weight"].T + w["actor.fc_mu.bias"])
    pre = h @ w["actor.fc_std.weight"].T + w["actor.fc_std.bias"]
    v = torch.where(pre > 20, pre, torch.log1p(torch.exp(pre)))
    if variance_is_std:
        std, log_det_half = v, torch.log(v).sum(-1)
    else:
        std, log_det_half = torch.sqrt(v), 0.5 * torch.log(v).sum(-1)
    actions = mu + std * eps
    log_probs = -0.5 * (eps * eps).sum(-1) - log_det_half - math.log(2 * math.pi)
    hc = torch.relu(obs.reshape(P, A * D) @ w["critic.fc1.weight"].T + w["critic.fc1.bias"])
    values = hc @ w["critic.fc2.weight"].T + w["critic.fc2.bias"]
    return actions.reshape(P, A, 2), log_probs, values


_cache = {}


def manifest():
    if "manifest" not in _cache:
        with open(os.path.join(GOLDEN, "policy_MANIFEST.json")) as fh:
            _cache["manifest"] = json.load(fh)
    return _cache["manifest"]


def case_names():
    return list(manifest()["cases"])


def _arrays(name):
    """Every stored array of one case, unpacked (keys as the generator named
    them: 'obs', 'default.actions64', 'sat.actor.fc_mu.weight', ...)."""
    if ("arrays", name) in _cache:
        return _cache[("arrays", name)]
    if "npz" not in _cache:
        _cache["npz"] = np.load(os.path.join(GOLDEN, "policy_f6.npz"))
    z, info, out = _cache["npz"], manifest()["cases"][name], {}
    for kind in ("f32", "f64"):
        blob, at = z[f"{name}.{kind}"], 0
        for key, shape in info["layout"][kind]:
            n = int(np.prod(shape))
            out[key] = blob[at:at + n].reshape(shape)
            at += n
        assert at == blob.size
    for k in z.files:
        if k.startswith(name + ".") and ".q" in k:          # int8 k of value k * 2^-bits
            key, bits = k[len(name) + 1:].rsplit(".q", 1)
            out[key] = (z[k].astype(np.float32) * np.float32(2.0 ** -int(bits)))
    _cache[("arrays", name)] = out
    return out


def load_case(name, group):
    """-> dict: P, A, O, H, D, obs, eps, w (fp32 weights of the group), and
    the reference's fp32 / fp64 outputs under KINDS / KINDS + '64' (numpy)."""
    info = manifest()["cases"][name]
    own, base = _arrays(name), _arrays(info["weights_from"])
    w = {}
    for pre, keys in (("actor.", ACTOR_KEYS), ("critic.", CRITIC_KEYS)):
        for k in keys:
            sat = own.get(f"sat.{pre}{k}") if group == "sat" else None
            w[pre + k] = sat if sat is not None else base[f"default.{pre}{k}"]
    c = {k: info[k] for k in ("P", "A", "O", "H", "D")}
    c.update(name=name, group=group, obs=own["obs"], eps=own["eps"], w=w)
    for k in KINDS:
        c[k] = own[f"{group}.{k}"]
        c[k + "64"] = own[f"{group}.{k}64"]
    return c


def tensors(c, device="cpu", dtype=torch.float32):
    """(w, obs, eps) of a loaded case as tensors."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    return {k: t(v) for k, v in c["w"].items()}, t(c["obs"]), t(c["eps"])


class Pooled(object):
    """Largest absolute fp32 error against the fp64 values per (kind, group),
    pooled over the cases added, for the reference and for a candidate."""

    def __init__(self):
        self.ref = {(k, g): 0.0 for k in KINDS for g in GROUPS}
        self.got = dict(self.ref)
        self.seen = set()

    def add(self, c, outputs):
        """outputs: the candidate's (actions, log_probs, values) for case c."""
        for k, o in zip(KINDS, outputs):
            o = np.asarray(o, np.float64).reshape(c[k + "64"].shape)
            assert np.isfinite(o).all(), (c["name"], c["group"], k)
            key = (k, c["group"])
            self.seen.add(key)
            self.got[key] = max(self.got[key], float(np.abs(o - c[k + "64"]).max()))
            self.ref[key] = max(self.ref[key],
                                float(np.abs(c[k].astype(np.float64) - c[k + "64"]).max()))

    def lines(self, who="kernel"):
        return [f"{k:9s} {g:7s} reference max|err| {self.ref[k, g]:.3e}  {who} {self.got[k, g]:.3e}"
                f"  ratio {self.got[k, g] / self.ref[k, g] if self.ref[k, g] else float('inf'):.2f}"
                for k in KINDS for g in GROUPS if (k, g) in self.seen]

    def failures(self):
        return [(k, g, self.got[k, g], self.ref[k, g]) for k in KINDS for g in GROUPS
                if (k, g) in self.seen and not self.got[k, g] <= FACTOR * self.ref[k, g]]


# ------------------------------------------------------------- generated shapes
# (P, A, O, H), each the smallest that reaches its path of marlnav_policy.hip
# (blocks of 64 envs and 256 threads; Hq = ceil(H / 4) hidden units per wave,
# summed in groups of 8 in the collapse and of 4 in the critic; compiled
# variants at A3 O3 and A3 O8, the generic path elsewhere)
SHAPES = (
    [(130, 16, 32, 50),       # generic, 3 blocks, 4 trips of the actor's row loop, last block 2 envs
     (65, 64, 256, 5),        # the limits A = 64, O = 256: D = 640, AD = 40 960; a wave with no unit
     (3, 64, 256, 512),       # the limits with H = 512 as well
     (129, 3, 8, 67),         # compiled A3 O8, 3 blocks, last block 1 env
     (130, 2, 1, 50)]         # generic at the smallest row, D = 6
    # Hq = 1, 1, 1, 1, 2, 2, 2, 3, 8, 8, 9, 128: every remainder of the groups
    # of 4 and 8, and waves with an empty share (H = 1, 2, 3, 5, 9), compiled
    + [(70, 3, 3, H) for H in (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 512)]
    + [(70, 2, 1, H) for H in (1, 5, 9, 512)]             # the same edges on the generic path
    + [(64, 3, 3, 50), (128, 3, 3, 50), (1, 16, 32, 50)])  # no partial block; a single env
SEED = 7
# an fp32 result cannot be asked below half an ulp at the largest entry of
# its kind: the reference side's figure counts as at least FLOOR * max|x64|
FLOOR = 2.0 ** -24


def make_case(P, A, O, H, seed):
    """(w, obs, eps) of a seeded case, built as test_ppo_gpu.make_case builds
    its weights: nn.Linear-style uniform weights U(-1, 1) / sqrt(fan_in), obs
    uniform in [-1, 1), eps standard normal, one seeded generator. fp32, CPU."""
    D = 2 + 2 * O + 2 * (A - 1)
    gen = torch.Generator().manual_seed(seed)
    uni = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    lin = lambda o, i: (uni(o, i) / i ** 0.5, uni(o) / i ** 0.5)
    w = {}
    for pre, o, i in (("actor.fc1", H, D), ("actor.fc_mu", 2, H), ("actor.fc_std", 2, H),
                      ("critic.fc1", H, A * D), ("critic.fc2", 1, H)):
        w[pre + ".weight"], w[pre + ".bias"] = lin(o, i)
    obs = uni(P, A, D)
    eps = torch.randn(P * A, 2, generator=gen)
    return w, obs, eps


def collapsed_ref(w, obs, eps, drop_collapse=0, drop_critic=0):
    """The kernel's formulation in torch: Weff = [Wmu; Wstd] @ W1, beff =
    [Wmu; Wstd] @ b1 + [bmu; bstd], the agent rows against Weff; the critic as
    policy_ref's. ``drop_collapse`` / ``drop_critic``: WRONG on purpose, the
    last that many hidden units left out of the collapse / of the critic (for
    the tests that show the criterion refuses it)."""
    P, A, D = obs.shape
    H = w["actor.fc1.weight"].shape[0]
    ha, hc = H - drop_collapse, H - drop_critic
    heads = torch.cat([w["actor.fc_mu.weight"], w["actor.fc_std.weight"]])[:, :ha]      # (4, H)
    weff = heads @ w["actor.fc1.weight"][:ha]
    beff = heads @ w["actor.fc1.bias"][:ha] + torch.cat([w["actor.fc_mu.bias"],
                                                         w["actor.fc_std.bias"]])
    pre = obs.reshape(P * A, D) @ weff.T + beff
    mu = torch.tanh(pre[:, :2])
    v = torch.where(pre[:, 2:] > 20, pre[:, 2:], torch.log1p(torch.exp(pre[:, 2:])))
    actions = mu + torch.sqrt(v) * eps
    log_probs = -0.5 * (eps * eps).sum(-1) - 0.5 * torch.log(v).sum(-1) - math.log(2 * math.pi)
    hid = torch.relu(obs.reshape(P, A * D) @ w["critic.fc1.weight"][:hc].T
                     + w["critic.fc1.bias"][:hc])
    values = hid @ w["critic.fc2.weight"][:, :hc].T + w["critic.fc2.bias"]
    return actions.reshape(P, A, 2), log_probs, values


_generated = {}


def generated(P, A, O, H, seed=SEED):
    """-> namespace of ``make_case``'s (w, obs, eps) with ``c64`` (policy_ref
    in fp64, the truth) and ``ref32`` (policy_ref in fp32: the reference side),
    all on the CPU, computed once per shape and shared: leave them unchanged."""
    key = (P, A, O, H, seed)
    if key not in _generated:
        from types import SimpleNamespace
        w, obs, eps = make_case(P, A, O, H, seed)
        with torch.no_grad():
            ref32 = policy_ref(w, obs, eps)
            c64 = policy_ref({k: v.double() for k, v in w.items()}, obs.double(), eps.double())
        _generated[key] = SimpleNamespace(shape=(P, A, O, H), w=w, obs=obs, eps=eps, c64=c64,
                                          ref32=ref32)
    return _generated[key]


def _np64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, np.float64)


class ShapeCheck(object):
    """The criterion on ONE shape: per output kind the candidate's largest
    absolute error against the fp64 values must not exceed FACTOR x
    max(the reference side's, FLOOR x max|x64| of that kind). A candidate
    with a non-finite entry fails its kind."""

    def __init__(self, c64, ref32, got):
        self.rows = {}
        for k, t, r, g in zip(KINDS, c64, ref32, got):
            t, r = _np64(t), _np64(r)
            g = _np64(g).reshape(t.shape)
            err = float(np.abs(g - t).max()) if np.isfinite(g).all() else float("inf")
            self.rows[k] = (float(np.abs(r - t).max()), FLOOR * float(np.abs(t).max()), err)

    def ratio(self, k):
        ref, floor, got = self.rows[k]
        return got / max(ref, floor)

    def lines(self, who="kernel"):
        return [f"{k:9s} reference max|err| {ref:.3e}  floor {floor:.3e}  {who} {got:.3e}"
                f"  ratio {self.ratio(k):.2f}" for k, (ref, floor, got) in self.rows.items()]

    def failures(self):
        return [(k,) + self.rows[k] for k in KINDS if not self.ratio(k) <= FACTOR]


def check_shape(c64, ref32, got):
    """-> ShapeCheck; ``.failures()`` is empty when ``got`` meets the criterion."""
    return ShapeCheck(c64, ref32, got)


# ----------------------------------------------- the native normals on the host
# device_rng.h restated with numpy: Philox2x32-10 under native_key(mixed seed,
# block 2^31, step), counter (lo32(gid), lo32(step) ^ hi32(gid) * 0x85EBCA77),
# gid = env_offset * A + row; then Box-Muller on the two words in float64.
POLICY_BLOCK = 0x80000000
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def seed_mix(seed):
    """splitmix64's finaliser of the caller's seed (native_seed_mix)."""
    z = (seed + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def native_key(mixed, blk, step):
    return (mixed & _M32) ^ _fmix32((blk * 0x9E3779B1 + (step >> 32) * 0x85EBCA77
                                     + (mixed >> 32)) & _M32)


def philox2x32_10(c0, c1, key):
    """Philox2x32-10 of uint32 counter arrays (c0, c1) under one 32-bit key."""
    c0, c1 = np.asarray(c0, np.uint64), np.asarray(c1, np.uint64)
    k = int(key)
    for _ in range(10):
        p = c0 * np.uint64(0xD256D193)                    # < 2^64: no wrap
        c0, c1 = (p >> np.uint64(32)) ^ np.uint64(k) ^ c1, p & np.uint64(_M32)
        k = (k + 0x9E3779B9) & _M32
    return c0.astype(np.uint32), c1.astype(np.uint32)


def native_words(seed, step, env_offset, rows, A):
    """The two Philox words of agent rows 0..rows-1 of a shard whose env 0 is
    global env ``env_offset``: uint32 arrays (r0, r1)."""
    gid = [(env_offset * A + r) & _M64 for r in range(rows)]
    c0 = np.array([g & _M32 for g in gid], np.uint64)
    c1 = np.array([(step & _M32) ^ (((g >> 32) * 0x85EBCA77) & _M32) for g in gid], np.uint64)
    return philox2x32_10(c0, c1, native_key(seed_mix(seed & _M64), POLICY_BLOCK, step & _M64))


def native_normals(seed, step, env_offset, rows, A):
    """(rows, 2) float64: Box-Muller on ``native_words``, u1 = ((r0 >> 8) + 1)
    2^-24 in (0, 1], u2 = (r1 >> 8) 2^-24 in [0, 1), z = sqrt(-2 ln u1) (cos,
    sin)(2 pi u2)."""
    r0, r1 = native_words(seed, step, env_offset, rows, A)
    u1 = ((r0 >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (r1 >> 8).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)], 1)
