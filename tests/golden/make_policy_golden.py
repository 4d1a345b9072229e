"""Generate tests/golden/policy_f6.npz and policy_MANIFEST.json: the
reference's ``Actor`` and ``Critic`` (marlnav/models.py:14-56), imported
unmodified, evaluated as ``MAPPO.get_data`` evaluates them per step
(models.py:113-120) on seeded inputs. Numbers only are stored.

Per case ``(P, A, O, H)`` and weight group:

* the state dicts (``default``: the modules' own orthogonal initialisation;
  ``sat``: the same modules with the two heads mapped affinely so that the
  ``fc_mu`` pre-activations span [-10, 10] and the ``fc_std`` pre-activations
  span [-30, 30], i.e. both sides of softplus's threshold 20 and below -20;
  the ``sat`` group stores the heads only, the rest is the ``default``'s);
* ``obs``: the normalised observations, uniform in [-1, 1];
* ``eps``: ``torch.empty(P*A, 2).normal_()`` after ``torch.manual_seed(seed)``,
  the normals ``dist.sample()`` consumes after the same seed;
* ``actions`` / ``log_probs`` / ``values``: the reference's fp32 outputs
  (``dist.sample()`` after that seed, ``dist.log_prob`` of it, the critic);
* ``actions64`` / ``log_probs64`` / ``values64``: the same from ``.double()``
  copies of the same modules on the same ``eps`` (loc + scale_tril @ eps).

Cases of one (A, O, H) share one pair of modules (one seed), so the
``default`` weights are stored with the first of them (``weights_from`` in the
manifest). To keep the archive small (each array of an .npz costs ~300 bytes
of headers) a case's float32 arrays are concatenated into one vector
``<case>.f32`` and its float64 arrays into ``<case>.f64``; the manifest's
``layout`` lists (key, shape) in order. tests/policy_ref.py ``load_case``
undoes both.

A weight tensor of more than 16384 elements (the critic's first layer at 16
agents x 32 obstacles) is first rounded to the grid k * 2^-10 and stored as
int8 k (key suffix ``.q10``); the module computes with the rounded weights,
so the stored numbers are exactly the ones the outputs were computed from.

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_policy_golden.py
"""
import copy
import json
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MARLNAV_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from marlnav.models import Actor, Critic  # noqa: E402

CASES = ((1, 3, 3, 50), (5, 3, 3, 50), (67, 3, 3, 50), (9, 2, 1, 1), (33, 3, 8, 67),
         (3, 16, 32, 50))
GROUPS = ("default", "sat")
Q_ELEMS, Q_BITS = 16384, 10
MU_SPAN, STD_SPAN = 10.0, 30.0
FP32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


def case_name(P, A, O, H):
    return f"p{P}a{A}o{O}h{H}"


def quantize_(w):
    """Round w in place to the grid k * 2^-Q_BITS, |k| <= 127; returns k."""
    k = torch.round(w * 2.0 ** Q_BITS)
    assert float(k.abs().max()) <= 127, "weight outside the int8 grid"
    w.copy_(k * 2.0 ** -Q_BITS)
    return k.to(torch.int8)


def span_head_(lin, h, lo, hi):
    """Map the head affinely (weight scaled, bias shifted) so that its
    pre-activations over the rows h span [lo, hi]."""
    pre = lin(h)
    mn, mx = float(pre.min()), float(pre.max())
    assert mx > mn
    a = (hi - lo) / (mx - mn)
    lin.weight.mul_(a)
    lin.bias.mul_(a).add_(lo - a * mn)


@torch.no_grad()
def evaluate(actor, critic, obs, eps, seed):
    """models.py:113-120 with the reference's own calls, fp32, then the same
    arithmetic from .double() copies on the same normals."""
    torch.manual_seed(seed)
    dist = actor(obs)
    actions = dist.sample()
    log_probs = dist.log_prob(actions)
    values = critic(obs)
    # the recorded eps is what sample() consumed
    restated = dist.loc + (dist.scale_tril @ eps[..., None])[..., 0]
    assert float((restated - actions).abs().max()) <= 1e-6, "eps is not sample()'s stream"
    var = dist.covariance_matrix.diagonal(dim1=-2, dim2=-1)
    assert bool((var >= FP32_MIN_NORMAL).all()) and bool(torch.isfinite(var).all()), \
        "a variance is not a positive normal fp32"
    actor64, critic64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    dist64 = actor64(obs.double())
    actions64 = dist64.loc + (dist64.scale_tril @ eps.double()[..., None])[..., 0]
    return {"actions": actions, "log_probs": log_probs, "values": values,
            "actions64": actions64, "log_probs64": dist64.log_prob(actions64),
            "values64": critic64(obs.double())}


@torch.no_grad()
def make_case(idx, P, A, O, H):
    D = 2 + 2 * O + 2 * (A - 1)
    name = case_name(P, A, O, H)
    seed = 1000 + idx
    first = [i for i, c in enumerate(CASES) if c[1:] == (A, O, H)][0]
    torch.manual_seed(1000 + first)          # one pair of modules per (A, O, H)
    actor, critic = Actor(D, H), Critic(A * D, H)
    rec, info = {}, {"P": P, "A": A, "O": O, "H": H, "D": D, "seed": seed, "groups": {},
                     "weights_from": case_name(*CASES[first])}
    qkeys = {}
    for mod, pre in ((actor, "actor."), (critic, "critic.")):
        for k, v in mod.state_dict().items():
            if v.numel() > Q_ELEMS:
                qkeys[pre + k] = quantize_(v)        # state_dict tensors alias the parameters
    gen = torch.Generator().manual_seed(seed + 500)
    obs = torch.rand(P, A, D, generator=gen) * 2.0 - 1.0
    torch.manual_seed(seed + 700)
    eps = torch.empty(P * A, 2).normal_()
    rec["obs"] = obs.numpy()
    rec["eps"] = eps.numpy()
    for group in GROUPS:
        if group == "sat":
            h = actor.fc1(obs.reshape(-1, D))
            span_head_(actor.fc_mu, h, -MU_SPAN, MU_SPAN)
            span_head_(actor.fc_std, h, -STD_SPAN, STD_SPAN)
        h = actor.fc1(obs.reshape(-1, D))
        pmu, pstd = actor.fc_mu(h), actor.fc_std(h)
        rng = {"mu_pre": [float(pmu.min()), float(pmu.max())],
               "std_pre": [float(pstd.min()), float(pstd.max())]}
        if group == "sat":
            assert rng["mu_pre"][0] < -8 and rng["mu_pre"][1] > 8, rng
            assert rng["std_pre"][0] < -20 and rng["std_pre"][1] > 20, rng
            assert bool(((pstd > -20) & (pstd < 20)).any()) or P * A < 4, rng
        out = evaluate(actor, critic, obs, eps, seed + 700)
        var = torch.nn.functional.softplus(pstd)
        rng["variance"] = [float(var.min()), float(var.max())]
        info["groups"][group] = rng
        for k, v in out.items():
            rec[f"{group}.{k}"] = v.numpy()
        for mod, pre in ((actor, "actor."), (critic, "critic.")):
            for k, v in mod.state_dict().items():
                if group == "sat" and not k.startswith(("fc_mu", "fc_std")):
                    continue
                if group == "default" and first != idx:
                    continue
                if pre + k in qkeys:
                    rec[f"{group}.{pre}{k}.q{Q_BITS}"] = qkeys[pre + k].numpy()
                else:
                    rec[f"{group}.{pre}{k}"] = v.numpy().copy()
    return name, rec, info


def pack(name, rec, info):
    """One float32 and one float64 vector per case (+ the int8 arrays)."""
    out, layout = {}, {"f32": [], "f64": []}
    for k, v in rec.items():
        if v.dtype == np.int8:
            out[f"{name}.{k}"] = v
            continue
        kind = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}[v.dtype]
        layout[kind].append([k, list(v.shape)])
    for kind in ("f32", "f64"):
        out[f"{name}.{kind}"] = np.concatenate([rec[k].ravel() for k, _ in layout[kind]])
    info["layout"] = layout
    return out


def main():
    rec, cases = {}, {}
    for idx, c in enumerate(CASES):
        name, r, info = make_case(idx, *c)
        rec.update(pack(name, r, info))
        cases[name] = info
    path = os.path.join(HERE, "policy_f6.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    manifest = {"file": "policy_f6.npz", "bytes": size, "torch": torch.__version__,
                "generator": "tests/golden/make_policy_golden.py",
                "reference": "marlnav/models.py Actor, Critic (models.py:14-56), unmodified",
                "quantized": f"weights of more than {Q_ELEMS} elements: int8 k, value k * 2^-{Q_BITS}",
                "cases": cases}
    with open(os.path.join(HERE, "policy_MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(path, size, "bytes")
    for n, i in cases.items():
        print(n, json.dumps(i["groups"]))
    print(len(rec), "arrays")


if __name__ == "__main__":
    main()
