"""A plain torch restatement of the actor phase's diagnostics and of the
target-KL stop (include/marlnav.h ``marlnav_ppo_actor_grad_diag``
/ ``marlnav_ppo_train_phase_monitored``), on top of ``ppo_ref.actor_terms``, in
whatever dtype the weights have:

    logr      = new_lp - log_probs
    ratio     = exp(logr)
    approx_kl = mean((ratio - 1) - logr)                  the k3 estimator
    clip_frac = mean((ratio < 1 - eps) | (ratio > 1 + eps))
    surrogate = mean(min(ratio adv, clamp(ratio, 1 - eps, 1 + eps) adv))
    entropy   = mean(entropy of the row's normal)

``own_env``: the pairing of advantages to agent rows. False: the reference's
``(returns - values).repeat(A)``; True (the GAE mode):
``returns`` holds ready advantages and row i reads that of its own env i // A.

``stop_rule`` restates the decision on a list of KLs: update k stops the phase
when ``not (kl[k] <= target)``, so a NaN stops; the update that stops has status
1 and takes no optimiser step, every later one status 2; ``target = inf``
monitors only and never stops, a NaN included."""
import math

import torch

import ppo_ref as pp

KEYS = ("surrogate_mean", "entropy_mean", "approx_kl", "clip_frac")
ROW = KEYS + ("status",)


def diagnostics(w, data, epsilon, own_env=False):
    """w: the actor's weights by ppo_ref's keys; data: dict of ppo_ref.DATA_KEYS
    tensors (returns float64). -> dict of KEYS as Python floats, plus
    'outside' (the count behind clip_frac) and 'ratio' (M,) for the callers
    that check how far the rows are from the clip bounds."""
    with torch.no_grad():
        new_lp, entropy = pp.actor_terms(w, data["obs"], data["actions"])
        A = data["obs"].shape[2]
        N = data["returns"].numel()
        M = N * A
        logr = new_lp - data["log_probs"].reshape(M)
        ratio = torch.exp(logr)
        if own_env:
            adv = data["returns"].reshape(N).repeat_interleave(A)
        else:
            adv = (data["returns"].reshape(N) - data["values"].reshape(N)).repeat(A)
        outside = (ratio < 1 - epsilon) | (ratio > 1 + epsilon)
        surr = torch.mean(torch.minimum(ratio * adv,
                                        torch.clamp(ratio, 1 - epsilon, 1 + epsilon) * adv))
        return {"surrogate_mean": float(surr), "entropy_mean": float(torch.mean(entropy)),
                "approx_kl": float(torch.mean((ratio - 1) - logr)),
                "clip_frac": float(outside.sum()) / M, "outside": int(outside.sum()),
                "ratio": ratio}


def ratio_gap(ratio, epsilon):
    """The smallest relative distance of a row's ratio to 1 - eps or 1 + eps."""
    r = ratio.double()
    return min(float(((r - b).abs() / torch.clamp(r.abs(), min=b)).min())
               for b in (1 - epsilon, 1 + epsilon))


def stop_rule(kls, target):
    """-> (status per update, stopped_at or -1)."""
    status, stopped_at = [], -1
    for k, kl in enumerate(kls):
        if stopped_at >= 0:
            status.append(2)
        elif target < math.inf and not kl <= target:
            status.append(1)
            stopped_at = k
        else:
            status.append(0)
    return status, stopped_at
