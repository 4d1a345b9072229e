"""Per-step time of the rollout loop around Env.step, fused against torch
modules, on one GPU:

* ``fused``: ``rollout.collect`` (one ``marlnav_policy_act`` launch per step
  for actor, sample, log-prob and critic, written into the RolloutBuffer);
* ``torch``: the same loop as MAPPO.get_data writes it (models.py:106-125)
  with ``torch.nn`` modules and ``torch.distributions.MultivariateNormal`` on
  the GPU and a Python list buffer, then ``rollout.process_rewards``.

Both drive the same Env with the fused ObsNormalizer / ActionScaler and end
with the returns scan and the episode counters. Timed with device events over
one rollout of ``--steps`` steps (>= 200) after a warm-up rollout, the two
arms alternating ``--reps`` times.

Also the policy kernel alone: a hipGraph of ``--chain`` back-to-back launches
replayed under events (so the host's enqueue rate is not what is measured),
per launch, next to the least time its FMA and byte counts allow (peaks:
157.3 TFLOP/s fp32 vector, 6.3 TB/s achievable HBM).

    python scripts/policy_bench.py [--shapes 65536x3x3,16384x3x3,1024x3x8] [--hidden 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402
from torch.distributions import MultivariateNormal  # noqa: E402

PEAK_FMA_PER_S = 157.3e12 / 2
PEAK_BYTES_PER_S = 6.3e12


class Actor(nn.Module):
    """The reference's actor: fc1 without activation, tanh mean head,
    softplus head used as the covariance diagonal."""

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


@torch.no_grad()
def torch_loop(pkg, env, nrm, actor, critic, T, A, gamma):
    buffer = []
    obs = nrm(env.observations())
    for _ in range(T):
        dist = actor(obs)
        actions = dist.sample()
        log_probs = dist.log_prob(actions)
        actions = actions.view(-1, A, 2)
        new_obs, rewards, terminated, truncated = env.step(actions)
        done = torch.logical_or(terminated, truncated)
        values = critic(obs)
        buffer += [[obs, actions, log_probs, values, rewards, done]]
        obs = nrm(new_obs)
    mean = pkg.rollout.process_rewards(buffer, gamma)
    stats = env._counter_totals()
    env._num_trunc = env._num_col = env._num_tar = 0
    return mean, stats


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3   # us


def kernel_alone(policy, obs, chain, replays):
    P, A = obs.shape[0], policy.num_agents
    out = (torch.empty(P, A, 2, device=obs.device), torch.empty(P * A, device=obs.device),
           torch.empty(P, 1, device=obs.device))
    for s in range(3):
        policy.act(obs, step_idx=s, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for s in range(chain):
            policy.act(obs, step_idx=s, out=out)
    g.replay()
    ts = sorted(timed(g.replay) / chain for _ in range(replays))
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x3x3,16384x3x3,1024x3x8")
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chain", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_bench.py needs a HIP device")
    import marlnav_amd as pkg
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; "
          f"{a.steps} steps per rollout, {a.reps} alternating reps, H={a.hidden}")
    for shape in a.shapes.split(","):
        P, A, O = (int(x) for x in shape.split("x"))
        D, H, T = 2 + 2 * O + 2 * (A - 1), a.hidden, a.steps
        args = pkg.default_args(num_parallel=P, num_agents=A, num_obstacles=O)
        nrm = pkg.ObsNormalizer(pkg.set_normalizer_params(args, dev))
        scl = pkg.ActionScaler(pkg.set_scaler_params(args, dev))
        torch.manual_seed(0)
        actor, critic = Actor(D, H).to(dev), Critic(A * D, H).to(dev)
        policy = pkg.FusedPolicy(actor, critic, seed=1)
        buf = pkg.RolloutBuffer(T)

        def new_env():
            params = pkg.set_env_params(args, dev)
            params.update(rng="native", seed=20251003)
            env = pkg.Env(params)
            env.attach_normalizer(nrm)
            env.attach_action_scaler(scl)
            return env

        arms = {"fused": lambda e: pkg.collect(e, policy, buf, gamma=args.gamma),
                "torch": lambda e: torch_loop(pkg, e, nrm, actor, critic, T, A, args.gamma)}
        envs = {k: new_env() for k in arms}
        for k, fn in arms.items():            # warm-up rollout of each arm
            fn(envs[k])
        per_step = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                per_step[k].append(timed(lambda: fn(envs[k])) / T)
        med = {k: sorted(v)[len(v) // 2] for k, v in per_step.items()}
        obs = nrm(envs["fused"].observations())
        k_med, k_min = kernel_alone(policy, obs, a.chain, 9)
        nblk = (P + 63) // 64
        fma = P * (H * A * D + H) + P * A * 4 * D + nblk * (4 * D * H + 4 * H)
        fma_uncollapsed = P * (H * A * D + H) + P * A * (H * D + 4 * H)
        nbytes = 4 * (P * A * D + P * A * 3 + P) + 4 * (H * D + 5 * H + 4 + H * A * D + H + 1)
        floor_us = max(fma / PEAK_FMA_PER_S, nbytes / PEAK_BYTES_PER_S) * 1e6
        rec = {"shape": shape, "hidden": H, "steps": T,
               "fused_us_per_step": round(med["fused"], 2),
               "torch_us_per_step": round(med["torch"], 2),
               "speedup": round(med["torch"] / med["fused"], 2),
               "fused_reps": [round(x, 2) for x in per_step["fused"]],
               "torch_reps": [round(x, 2) for x in per_step["torch"]],
               "policy_kernel_us": round(k_med, 2), "policy_kernel_us_min": round(k_min, 2),
               "kernel_fma": fma, "kernel_fma_uncollapsed": fma_uncollapsed,
               "kernel_bytes": nbytes, "kernel_floor_us": round(floor_us, 3),
               "kernel_floor_bound": "fma" if fma / PEAK_FMA_PER_S > nbytes / PEAK_BYTES_PER_S
               else "bytes",
               "kernel_gfma_per_s": round(fma / k_med / 1e3, 1),
               "kernel_gbytes_per_s": round(nbytes / k_med / 1e3, 1),
               "kernel_share_of_floor": round(floor_us / k_med, 3)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
