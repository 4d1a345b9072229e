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
