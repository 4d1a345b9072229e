"""Time of one PPO minibatch update (loss, gradients, optimiser step) of the
actor and of the critic on one GPU, four arms:

* ``onecall``: ``FusedPPO.actor_update`` / ``critic_update`` with a
  ``FusedAdam``: loss, gradients and the Adam step as one C call
  (libmarlnav.so ``marlnav_ppo_actor_update`` / ``marlnav_ppo_critic_update``),
  no host work between its launches;
* ``fused``: ``FusedPPO.actor_loss_grad`` / ``critic_loss_grad`` (two launches
  each, libmarlnav.so ``marlnav_ppo_actor_grad`` / ``marlnav_ppo_critic_grad``)
  on the RolloutBuffer's stacked storage, then ``optimizer.step()``;
* ``torch``: the written-out torch path (tests/ppo_ref.py: tensor ops and
  autograd) on the same device and the same stacked slices, with
  ``zero_grad()``, ``backward()`` and the same optimiser;
* ``mvn``: the reference's formulation of the actor (``vmap(torch.diag)`` into
  a ``MultivariateNormal``, its ``log_prob`` and ``entropy`` fed to ppo_ref's
  surrogate) on the ``torch.cat`` of a list buffer, at ``--mvn-envs`` envs per step where the shape
  has more (the batched Cholesky of every row and its backward do not finish
  in a useful time beyond that).

Adam as the reference constructs it (lr 3e-4; ``maximize=True`` for the
actor). Device events around ``--iters`` updates, after a warm-up, the arms
alternating ``--reps`` times; medians per update.

Also each fused call alone (a hipGraph of ``--chain`` calls replayed under
events, so the host's enqueue rate is not what is measured) next to its byte
and FMA counts: bytes are the minibatch read once plus the workspace written
and read back; the byte bound is at 6.3 TB/s achievable HBM. The Adam call
alone likewise (``FusedAdam.step``; bytes: param, grad and the two moments
read, param and the moments written back, seven fp32 streams of numel), and
one epoch of ``train_actor`` + ``train_critic`` with ``FusedAdam`` (the
minibatches of ``minibatch_bounds(steps, --epoch-batch)``) captured in a graph
and replayed, against the same epoch issued eagerly.

    python scripts/ppo_bench.py [--shapes 65536x3x3,16384x3x3,1024x3x8,4096x16x32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
from torch import nn  # noqa: E402
from torch.distributions import MultivariateNormal  # noqa: E402

PEAK_BYTES_PER_S = 6.3e12
EPSILON, ENT_CONST, LR = 0.01, 0.001, 3e-4


class Actor(nn.Module):
    """The reference's actor (as in scripts/policy_bench.py)."""

    def __init__(self, D, H):
        super().__init__()
        self.fc1, self.fc_mu, self.fc_std = nn.Linear(D, H), nn.Linear(H, 2), nn.Linear(H, 2)
        for m in (self.fc1, self.fc_mu, self.fc_std):
            nn.init.orthogonal_(m.weight)

    def forward(self, x):
        x = self.fc1(x.flatten(0, 1))
        mu = torch.tanh(self.fc_mu(x))
        var = nn.functional.softplus(self.fc_std(x))
        return MultivariateNormal(mu, torch.vmap(torch.diag)(var))


class Critic(nn.Module):
    def __init__(self, AD, H):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(AD, H), nn.Linear(H, 1)
        for m in (self.fc1, self.fc2):
            nn.init.orthogonal_(m.weight)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x.flatten(1))))


def cat_entries(entries):
    """The reference's list buffer as the stacked tensors ppo_ref takes:
    ``torch.cat`` per entry kind, as models.py:273-277 does per minibatch."""
    T = len(entries)
    return [torch.cat([e[k] for e in entries]).unflatten(0, (T, -1)) for k in range(5)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def graph_time(fn, chain, replays, iters=1):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(chain):
            fn()
    g.replay()
    ts = sorted(timed(g.replay, iters) / chain for _ in range(replays))
    return ts[len(ts) // 2]


def cdiv(a, b):
    return -(-a // b)


def actor_blocks(M):
    """Blocks of marlnav_ppo.hip's actor grid."""
    return cdiv(M, max(1024, cdiv(cdiv(M, 1024), 256) * 256))


def critic_blocks(N, AD, H):
    """(row chunks, forward passes per row) of marlnav_ppo.hip's critic grid."""
    kc = min(AD, 256)
    ncol, us = cdiv(AD, kc), 256 // kc
    jt = 8 if us >= 2 else 64
    ub = min(us * jt, 64)
    ngrp = cdiv(H, ub)
    stride = H * AD + 2 * H + 2
    want = max(1, min(512 // (ncol * ngrp), (8 << 20) // stride))
    rows = cdiv(cdiv(N, 64), want) * 64
    # several output tiles: the forward pass runs once, dh goes through the workspace
    split = ncol * ngrp > 1 and N * cdiv(H, 64) * 64 <= 32 << 20
    return cdiv(N, rows), (1 if split else ncol * ngrp), split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x3x3,16384x3x3,1024x3x8,4096x16x32")
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--steps", type=int, default=8, help="steps per minibatch")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--mvn-envs", type=int, default=1024)
    ap.add_argument("--epoch-batch", type=int, default=2,
                    help="steps per minibatch of the captured epoch")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppo_bench.py needs a HIP device")
    import marlnav_amd as pkg
    import ppo_ref as pp
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; minibatch of "
          f"{a.steps} steps, H={a.hidden}, Adam; {a.iters} updates per timing, {a.reps} "
          f"alternating reps, medians", flush=True)
    for shape in a.shapes.split(","):
        P, A, O = (int(x) for x in shape.split("x"))
        D, H, T = 2 + 2 * O + 2 * (A - 1), a.hidden, a.steps
        N, M, AD = T * P, T * P * A, A * D
        torch.manual_seed(0)
        actor, critic = Actor(D, H).to(dev), Critic(AD, H).to(dev)
        # a buffer as collect() leaves it, then the weights moved so that the
        # ratios spread around the clip
        policy = pkg.FusedPolicy(actor, critic, seed=1)
        buf = pkg.RolloutBuffer(T)
        buf.reserve(P, A, D, dev)
        for t in range(T):
            o, act, lp, val, rew, done = buf.row(t)
            o.uniform_(-1.0, 1.0)
            policy.act(o, out=(act, lp, val))
            rew.zero_()
            done.zero_()
        buf.commit(T)
        buf.returns = torch.randn(T, P, dtype=torch.float64, device=dev)
        with torch.no_grad():
            for p in list(actor.parameters()) + list(critic.parameters()):
                p.add_(0.02 * p.abs().mean() * torch.randn_like(p))
        start = {id(p): p.detach().clone() for m in (actor, critic) for p in m.parameters()}
        ppo = pkg.FusedPPO(actor, critic, EPSILON, ENT_CONST)
        opt_a = torch.optim.Adam(actor.parameters(), lr=LR, maximize=True)
        opt_c = torch.optim.Adam(critic.parameters(), lr=LR, maximize=False)
        # the one-call arm's optimisers: their own moments over the same parameters
        adam_a = pkg.FusedAdam(actor.parameters(), lr=LR, maximize=True)
        adam_c = pkg.FusedAdam(critic.parameters(), lr=LR, maximize=False)
        names = {"actor": (actor, ("fc1", "fc_mu", "fc_std")), "critic": (critic, ("fc1", "fc2"))}

        def weights(which):
            mod, layers = names[which]
            return {f"{which}.{l}.{x}": getattr(getattr(mod, l), x) for l in layers
                    for x in ("weight", "bias")}

        data = {k: buf.stacked(i) for i, k in enumerate(("obs", "actions", "log_probs", "values"))}
        data["returns"] = buf.returns

        def fused_actor():
            ppo.actor_loss_grad(buf, 0, T)
            opt_a.step()

        def fused_critic():
            ppo.critic_loss_grad(buf, 0, T)
            opt_c.step()

        def onecall_actor():
            ppo.actor_update(buf, 0, T, adam_a)

        def onecall_critic():
            ppo.critic_update(buf, 0, T, adam_c)

        def torch_actor():
            opt_a.zero_grad()
            pp.actor_loss(weights("actor"), data["obs"], data["actions"], data["log_probs"],
                          data["values"], data["returns"], EPSILON, ENT_CONST).backward()
            opt_a.step()

        def torch_critic():
            opt_c.zero_grad()
            pp.critic_loss(weights("critic"), data["obs"], data["values"], data["returns"],
                           EPSILON).backward()
            opt_c.step()

        Pm = min(P, a.mvn_envs)
        entries = [[s[t][:Pm * A] if k == 2 else s[t][:Pm] for k, s in
                    enumerate([buf.stacked(i) for i in range(4)] + [buf.returns])]
                   for t in range(T)]

        def mvn_actor():
            # ppo_ref's surrogate on the MultivariateNormal's log_prob / entropy
            opt_a.zero_grad()
            obs, actions, lps, vals, rets = cat_entries(entries)
            dist = actor(obs.flatten(0, 1))
            pp.clipped_surrogate(dist.log_prob(actions.reshape(-1, 2)), dist.entropy(), lps, vals,
                                 rets, A, EPSILON, ENT_CONST).backward()
            opt_a.step()

        def mvn_critic():
            # no distribution in the critic: the torch arm after the list's cat
            opt_c.zero_grad()
            obs, _, _, vals, rets = cat_entries(entries)
            pp.critic_loss(weights("critic"), obs, vals, rets, EPSILON).backward()
            opt_c.step()

        arms = {"onecall": (onecall_actor, onecall_critic), "fused": (fused_actor, fused_critic),
                "torch": (torch_actor, torch_critic), "mvn": (mvn_actor, mvn_critic)}
        for fa, fc in arms.values():
            for _ in range(2):
                fa()
                fc()
        times = {k: ([], []) for k in arms}
        for _ in range(a.reps):
            for k, (fa, fc) in arms.items():
                times[k][0].append(timed(fa, a.iters))
                times[k][1].append(timed(fc, a.iters))
        med = {k: [sorted(v)[len(v) // 2] for v in ts] for k, ts in times.items()}
        for m in (actor, critic):
            for p in m.parameters():
                assert bool(torch.isfinite(p).all())
                assert not torch.equal(p, start[id(p)])

        assert adam_a.step_count() == adam_c.step_count() == 2 + a.reps * a.iters

        k_actor = graph_time(lambda: ppo.actor_loss_grad(buf, 0, T), a.chain, 7)
        k_critic = graph_time(lambda: ppo.critic_loss_grad(buf, 0, T), a.chain, 7)
        a_blocks = actor_blocks(M)
        a_bytes = 4 * M * (D + 3) + 12 * N + 2 * 8 * a_blocks * (4 * (D + 1) + 2) \
            + 2 * 4 * (H * D + 5 * H + 4)
        a_fma64 = M * (4 * D + 4 * (D + 1))
        chunks, fwd, split = critic_blocks(N, AD, H)
        c_bytes = 4 * N * AD + 12 * N + 2 * 8 * chunks * (H * AD + 2 * H + 2) \
            + 2 * 4 * (H * AD + 2 * H + 1) + (2 * 4 * N * cdiv(H, 64) * 64 if split else 0)
        c_fma32, c_fma64 = N * (H * AD + H) * fwd, N * H * AD
        # the Adam call alone, and one epoch eager against its graph
        k_adam_a = graph_time(adam_a.step, a.chain, 7)
        k_adam_c = graph_time(adam_c.step, a.chain, 7)
        n_a = sum(p.numel() for p in actor.parameters())
        n_c = sum(p.numel() for p in critic.parameters())
        bounds = pkg.minibatch_bounds(T, a.epoch_batch)

        def epoch():
            pkg.train_actor(ppo, buf, adam_a, 1, a.epoch_batch)
            pkg.train_critic(ppo, buf, adam_c, 1, a.epoch_batch)

        epoch()
        eager = sorted(timed(epoch, a.iters) for _ in range(a.reps))[a.reps // 2]
        count = adam_a.step_count()
        replayed = graph_time(epoch, 1, a.reps, iters=a.iters)
        # 3 warm-up epochs, then 1 + reps * iters replays: the count followed them
        assert adam_a.step_count() == count + (4 + a.reps * a.iters) * len(bounds)
        rec = {"shape": shape, "hidden": H, "steps": T, "agent_rows": M, "env_rows": N,
               "actor_us": {k: round(v[0], 1) for k, v in med.items()},
               "critic_us": {k: round(v[1], 1) for k, v in med.items()},
               "mvn_envs": Pm,
               "actor_onecall_vs_fused": round(med["fused"][0] / med["onecall"][0], 2),
               "critic_onecall_vs_fused": round(med["fused"][1] / med["onecall"][1], 2),
               "actor_speedup_vs_torch": round(med["torch"][0] / med["fused"][0], 2),
               "critic_speedup_vs_torch": round(med["torch"][1] / med["fused"][1], 2),
               "adam_actor_call_us": round(k_adam_a, 1), "adam_actor_bytes": 28 * n_a,
               "adam_critic_call_us": round(k_adam_c, 1), "adam_critic_bytes": 28 * n_c,
               "adam_actor_share_of_byte_bound":
                   round(28 * n_a / PEAK_BYTES_PER_S * 1e6 / k_adam_a, 5),
               "adam_critic_share_of_byte_bound":
                   round(28 * n_c / PEAK_BYTES_PER_S * 1e6 / k_adam_c, 5),
               "epoch_minibatches": len(bounds), "epoch_eager_us": round(eager, 1),
               "epoch_graph_us": round(replayed, 1),
               "reps": {k: [[round(x, 1) for x in v] for v in ts] for k, ts in times.items()},
               "actor_call_us": round(k_actor, 1), "actor_bytes": a_bytes,
               "actor_fma_fp64": a_fma64, "actor_blocks": a_blocks,
               "actor_share_of_byte_bound": round(a_bytes / PEAK_BYTES_PER_S * 1e6 / k_actor, 3),
               "critic_call_us": round(k_critic, 1), "critic_bytes": c_bytes,
               "critic_fma_fp32": c_fma32, "critic_fma_fp64": c_fma64,
               "critic_chunks": chunks, "critic_forward_passes": fwd,
               "critic_share_of_byte_bound": round(c_bytes / PEAK_BYTES_PER_S * 1e6 / k_critic, 3)}
        print(json.dumps(rec), flush=True)
        del buf, data, entries, ppo, policy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
