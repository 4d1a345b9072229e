"""Generate tests/golden/ppo_f7.npz and ppo_MANIFEST.json: the reference's
``MAPPO._actor_loss`` / ``_critic_loss`` (marlnav/models.py:270-316) with
``backward()``, on its own ``Actor`` and ``Critic`` (models.py:14-56), all
imported unmodified. The ``MAPPO`` instance comes from ``MAPPO.__new__`` and
gets only ``num_agents``, ``num_parallel``, ``action_size``, ``actor``,
``critic``, ``epsilon``, ``ent_const``. Numbers only are stored.

Per case ``(T, P, A, O, H)``:

* a buffer as ``get_data`` builds it (models.py:113-121): per step obs uniform
  in [-1, 1], ``dist.sample()``, ``dist.log_prob`` of it, the critic's values,
  and float64 standard-normal returns in the reward slot;
* every parameter then moves by 2% of its mean magnitude (times a standard
  normal), so the new log-probs and values differ from the stored ones;
* ``w.*``: the perturbed fp32 weights; ``loss32.*`` / ``g32.*``: the
  reference's fp32 losses and gradients; ``loss64.*`` / ``g64.*``: the same
  from ``.double()`` copies of the modules and of the buffer.

The generator asserts what the tests rest on:

* no row lies within 1e-4 (relative) of a decision boundary - the ratio
  against 1 -+ epsilon, the two surrogates against each other when outside,
  the new value against values -+ epsilon, the two squares when outside, a
  critic pre-activation against 0 on the scale of its row's largest - so the
  fp32 and fp64 evaluations take the same branches (per case; the case's seed
  is advanced until it holds);
* every branch (inside the clip, outside and passing, outside and blocked,
  for both losses) holds at least 5% of the pooled rows (a case of two env
  rows cannot populate three branches on its own; the per-case counts are in
  the manifest);
* per parameter tensor the reference's pooled fp32 gradient error,
  max|g32 - g64| / max|g64|, is at least 2^-24.

The arrays of a case are packed as in make_policy_golden.py: one float32 and
one float64 vector, the manifest's ``layout`` listing (key, shape) in order.

Run:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_ppo_golden.py
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

from marlnav.models import MAPPO, Actor, Critic  # noqa: E402

CASES = ((2, 1, 3, 3, 50), (2, 5, 3, 3, 50), (3, 67, 3, 3, 50), (2, 9, 2, 1, 1), (2, 33, 3, 8, 67))
EPSILON, ENT_CONST = 0.01, 0.001       # the CLI defaults
PERTURB, NEAR, MIN_SHARE = 0.02, 1e-4, 0.05
BRANCHES = ("inside", "passing", "blocked")


def case_name(T, P, A, O, H):
    return f"t{T}p{P}a{A}o{O}h{H}"


def make_mappo(actor, critic, P, A):
    m = MAPPO.__new__(MAPPO)
    m.num_agents, m.num_parallel, m.action_size = A, P, 2
    m.actor, m.critic = actor, critic
    m.epsilon, m.ent_const = EPSILON, ENT_CONST
    return m


def loss_grads(mappo, buffer):
    out = {}
    for which, mod, fn in (("actor", mappo.actor, mappo._actor_loss),
                           ("critic", mappo.critic, mappo._critic_loss)):
        mod.zero_grad()
        loss = fn(buffer)
        loss.backward()
        out[which] = (loss.detach().clone(),
                      {f"{which}.{k}": p.grad.detach().clone()
                       for k, p in mod.named_parameters()})
    return out


def rel_gap(a, b):
    return (a - b).abs() / torch.maximum(a.abs(), b.abs()).clamp_min(1e-300)


@torch.no_grad()
def branches(actor64, critic64, buffer64, A):
    """Branch of every row in the fp64 evaluation and the smallest relative
    distance to a decision boundary. -> ({loss: {branch: count}}, gap)."""
    obs = torch.cat([e[0] for e in buffer64])
    actions = torch.cat([e[1] for e in buffer64]).reshape(-1, 2)
    lp_old = torch.cat([e[2] for e in buffer64])
    val = torch.cat([e[3] for e in buffer64]).squeeze(-1)
    ret = torch.cat([e[4] for e in buffer64])
    ratio = torch.exp(actor64(obs).log_prob(actions) - lp_old)
    adv = (ret - val).repeat(A)
    lo, hi = 1 - EPSILON, 1 + EPSILON
    sa, sb = ratio * adv, torch.clip(ratio, lo, hi) * adv
    inside = (ratio >= lo) & (ratio <= hi)
    counts = {"actor": {"inside": int(inside.sum()), "passing": int((~inside & (sa < sb)).sum()),
                        "blocked": int((~inside & ~(sa < sb)).sum())}}
    gaps = [rel_gap(ratio, torch.full_like(ratio, lo)).min(),
            rel_gap(ratio, torch.full_like(ratio, hi)).min()]
    if bool((~inside).any()):
        gaps.append(rel_gap(sa, sb)[~inside].min())
    pre = critic64.fc1(critic64.flatten(obs))
    nv = critic64.fc2(torch.relu(pre)).squeeze(-1)
    s0 = (nv - ret) ** 2
    s1 = (torch.clamp(nv, min=val - EPSILON, max=val + EPSILON) - ret) ** 2
    inside = (nv >= val - EPSILON) & (nv <= val + EPSILON)
    counts["critic"] = {"inside": int(inside.sum()), "passing": int((~inside & (s0 > s1)).sum()),
                        "blocked": int((~inside & ~(s0 > s1)).sum())}
    gaps += [rel_gap(nv, val - EPSILON).min(), rel_gap(nv, val + EPSILON).min(),
             (pre.abs() / pre.abs().max(dim=1, keepdim=True).values).min()]
    if bool((~inside).any()):
        gaps.append(rel_gap(s0, s1)[~inside].min())
    return counts, float(torch.stack(gaps).min())


def make_case(seed, T, P, A, O, H):
    D = 2 + 2 * O + 2 * (A - 1)
    torch.manual_seed(seed)
    actor, critic = Actor(D, H), Critic(A * D, H)
    mappo = make_mappo(actor, critic, P, A)
    buffer = []
    with torch.no_grad():
        for _ in range(T):
            obs = torch.rand(P, A, D) * 2.0 - 1.0
            dist = actor(obs)
            actions = dist.sample()
            log_probs = dist.log_prob(actions)
            actions = actions.view(-1, A, 2)
            values = critic(obs)
            returns = torch.randn(P, dtype=torch.float64)
            buffer.append([obs, actions, log_probs, values, returns, torch.zeros(P, dtype=torch.bool)])
        for mod in (actor, critic):
            for p in mod.parameters():
                p.add_(PERTURB * p.abs().mean() * torch.randn_like(p))
    out32 = loss_grads(mappo, buffer)
    actor64, critic64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    buffer64 = [[x.double() if x.is_floating_point() else x for x in e] for e in buffer]
    out64 = loss_grads(make_mappo(actor64, critic64, P, A), buffer64)
    counts, gap = branches(actor64, critic64, buffer64, A)

    rec = {"obs": torch.stack([e[0] for e in buffer]), "actions": torch.stack([e[1] for e in buffer]),
           "log_probs": torch.stack([e[2] for e in buffer]),
           "values": torch.stack([e[3] for e in buffer]),
           "returns": torch.stack([e[4] for e in buffer])}
    for pre, mod in (("actor.", actor), ("critic.", critic)):
        for k, p in mod.named_parameters():
            rec["w." + pre + k] = p.detach()
    for which in ("actor", "critic"):
        rec["loss32." + which] = out32[which][0].reshape(1).float()
        rec["loss64." + which] = out64[which][0].reshape(1)
        for k, g in out32[which][1].items():
            assert g.dtype == torch.float32
            rec["g32." + k] = g
        for k, g in out64[which][1].items():
            assert g.dtype == torch.float64
            rec["g64." + k] = g
    rec = {k: v.numpy().copy() for k, v in rec.items()}
    info = {"T": T, "P": P, "A": A, "O": O, "H": H, "D": D, "seed": seed, "branches": counts,
            "min_boundary_gap": gap,
            "loss32": {w: float(out32[w][0]) for w in out32},
            "loss64": {w: float(out64[w][0]) for w in out64}}
    return rec, info


def pack(name, rec, info):
    out, layout = {}, {"f32": [], "f64": []}
    for k, v in rec.items():
        kind = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}[v.dtype]
        layout[kind].append([k, list(v.shape)])
    for kind in ("f32", "f64"):
        out[f"{name}.{kind}"] = np.concatenate([rec[k].ravel() for k, _ in layout[kind]])
    info["layout"] = layout
    return out


def main():
    packed, cases, recs = {}, {}, {}
    for idx, c in enumerate(CASES):
        for attempt in range(500):
            rec, info = make_case(7000 + 1000 * idx + attempt, *c)
            if info["min_boundary_gap"] > NEAR:
                break
        else:
            raise AssertionError(f"no seed keeps case {c} away from the decision boundaries")
        name = case_name(*c)
        recs[name], cases[name] = rec, info
        packed.update(pack(name, rec, info))
    pooled = {}
    for which in ("actor", "critic"):
        total = sum(sum(i["branches"][which].values()) for i in cases.values())
        pooled[which] = {b: sum(i["branches"][which][b] for i in cases.values()) / total
                         for b in BRANCHES}
        for b in BRANCHES:
            assert pooled[which][b] >= MIN_SHARE, (which, b, pooled[which])
    ref_err = {}
    for k in [k[4:] for k in next(iter(recs.values())) if k.startswith("g32.")]:
        e = max(float(np.abs(r["g32." + k] - r["g64." + k]).max() / np.abs(r["g64." + k]).max())
                for r in recs.values())
        assert e >= 2.0 ** -24, (k, e)
        ref_err[k] = e
    path = os.path.join(HERE, "ppo_f7.npz")
    np.savez_compressed(path, **packed)
    size = os.path.getsize(path)
    assert size < 1024 * 1024, size
    manifest = {"file": "ppo_f7.npz", "bytes": size, "torch": torch.__version__,
                "generator": "tests/golden/make_ppo_golden.py",
                "reference": "marlnav/models.py MAPPO._actor_loss, _critic_loss (models.py:270-316) "
                             "on Actor, Critic (models.py:14-56), unmodified",
                "epsilon": EPSILON, "ent_const": ENT_CONST, "perturbation": PERTURB,
                "pooled_branch_shares": pooled, "reference_fp32_gradient_error": ref_err,
                "cases": cases}
    with open(os.path.join(HERE, "ppo_MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(path, size, "bytes")
    for n, i in cases.items():
        print(n, "seed", i["seed"], "gap", i["min_boundary_gap"], json.dumps(i["branches"]))
    print("pooled", json.dumps(pooled))
    print("reference fp32 gradient error", json.dumps(ref_err))


if __name__ == "__main__":
    main()
