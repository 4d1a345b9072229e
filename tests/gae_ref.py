"""A float64 torch restatement of the GAE(lambda) advantage mode (DESIGN.md
§15; include/marlnav.h ``marlnav_gae_advantages`` and the
``MARLNAV_ADVANTAGE_ENV`` pairing of ``marlnav_ppo_actor_grad_mode``).

``gae`` is the scan in the contract's operation order, one tensor op per
operation over all envs of a step (so every env sees exactly the scalar
sequence below), with selects where the contract has selects:

    next  = t == T-1 ? last_values[p] : values[t+1][p]
    delta = (r + gamma * (done ? 0 : next)) - v
    A     = delta + gl * (done ? 0 : A_next)        gl = gamma * lam, A_T = 0
    value_targets[t][p] = A + v

then ``advantages = (A - mean) / (std + 1e-12)`` with the unbiased std over
all T*P raw advantages; the value targets stay in reward units.

``actor_loss_own_env`` is the actor loss of tests/ppo_ref.py with the one
change of the mode: the advantage of agent row i (rows in (t, p, a) order) is
``advantages[i // A]``, the row's own (t, p), taken as a ready advantage (no
values are subtracted). Everything else is ppo_ref's, imported.
"""
import torch

import ppo_ref as pp

F64 = torch.float64


def gae(rewards, done, values, last_values, gamma, lam):
    """rewards (T, P), done (T, P) bool, values (T, P) or (T, P, 1),
    last_values (P,) or (P, 1), any float dtype (fp32 inputs are widened
    exactly) -> dict of float64: raw (T, P), value_targets (T, P),
    advantages (T, P) normalised, mean, std (0-d)."""
    T, P = rewards.shape
    r, v = rewards.to(F64), values.reshape(T, P).to(F64)
    last = last_values.reshape(P).to(F64)
    d = done.reshape(T, P).bool()
    gamma, gl = float(gamma), float(gamma) * float(lam)
    zero = torch.zeros(P, dtype=F64)
    raw = torch.empty(T, P, dtype=F64)
    a = zero.clone()
    for t in range(T - 1, -1, -1):
        nxt = last if t == T - 1 else v[t + 1]
        delta = (r[t] + gamma * torch.where(d[t], zero, nxt)) - v[t]
        a = delta + gl * torch.where(d[t], zero, a)
        raw[t] = a
    mean = raw.sum() / (T * P)
    std = torch.sqrt(((raw - mean) ** 2).sum() / (T * P - 1))
    return {"raw": raw, "value_targets": raw + v, "advantages": (raw - mean) / (std + 1e-12),
            "mean": mean, "std": std}


def actor_loss_own_env(w, obs, actions, log_probs, advantages, epsilon, ent_const):
    """w: {'actor.fc1.weight': ...}; obs (T, P, A, D), actions (T, P, A, 2),
    log_probs (T, P*A), advantages (T, P) float64. -> 0-d loss."""
    new_lp, entropy = pp.actor_terms(w, obs, actions)
    A = obs.shape[2]
    M = advantages.numel() * A
    adv = advantages.reshape(-1).repeat_interleave(A)       # row i -> env row i // A
    ratio = torch.exp(new_lp - log_probs.reshape(M))
    clip_loss = torch.mean(torch.minimum(ratio * adv,
                                         torch.clamp(ratio, 1 - epsilon, 1 + epsilon) * adv))
    return clip_loss + ent_const * torch.mean(entropy)


def actor_loss_and_grads(w, data, advantages, epsilon, ent_const):
    """As ``ppo_ref.loss_and_grads('actor', ...)`` for the own-env pairing:
    -> (loss, {key: grad}) detached, in the dtype of w."""
    leaf = {k: w[k].detach().clone().requires_grad_(True) for k in pp.ACTOR_PARAMS}
    loss = actor_loss_own_env(leaf, data["obs"], data["actions"], data["log_probs"], advantages,
                              epsilon, ent_const)
    grads = torch.autograd.grad(loss, [leaf[k] for k in pp.ACTOR_PARAMS])
    return loss.detach(), dict(zip(pp.ACTOR_PARAMS, (g.detach() for g in grads)))
