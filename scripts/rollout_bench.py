"""Per-step time of a whole rollout, one C call against the Python loop, on
one GPU:

* ``fused``: ``rollout.collect_fused`` (``marlnav_rollout_collect``: the
  policy and step launches of every step, the flag merge and the returns scan
  enqueued by one call; the step kernels write their normalised observations
  into the buffer's rows);
* ``loop``: ``rollout.collect`` (per step an observation copy, the policy
  launch through ctypes, ``env.step`` through the host engine, a
  ``logical_or`` and a reward copy).

Both arms drive their own identically seeded Env and FusedPolicy over the
same weights and fill their own RolloutBuffer. The first (warm-up) rollout of
each arm doubles as the check that the two buffers and the returns are equal
bit for bit at the size timed. Then device events around one rollout of
``--steps`` steps (>= 200), the two arms alternating ``--reps`` times (>= 3);
the returns scan and the read of the episode counters are inside the window
of both.

    python scripts/rollout_bench.py [--shapes 65536x3x3,16384x3x3,1024x3x8] [--hidden 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402

ENTRIES = ("obs", "actions", "log_probs", "values", "rewards", "done")


def modules(D, AD, H, dev):
    """Modules with the reference's attribute names and shapes."""
    torch.manual_seed(0)
    actor, critic = nn.Module(), nn.Module()
    actor.fc1, actor.fc_mu, actor.fc_std = nn.Linear(D, H), nn.Linear(H, 2), nn.Linear(H, 2)
    critic.fc1, critic.fc2 = nn.Linear(AD, H), nn.Linear(H, 1)
    for m in (actor.fc1, actor.fc_mu, actor.fc_std, critic.fc1, critic.fc2):
        nn.init.orthogonal_(m.weight)
    return actor.to(dev), critic.to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3   # us


def same_bits(a, b):
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    as_int = torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(a.view(as_int), b.view(as_int))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x3x3,16384x3x3,1024x3x8")
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bench.py needs a HIP device")
    if a.steps < 200 or a.reps < 3:
        raise SystemExit("rollout_bench.py times >= 200 steps per rollout and >= 3 alternating reps")
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
        actor, critic = modules(D, A * D, H, dev)

        def new_env():
            params = pkg.set_env_params(args, dev)
            params.update(rng="native", seed=20251003)
            env = pkg.Env(params)
            env.attach_normalizer(nrm)
            env.attach_action_scaler(scl)
            return env

        calls = {"fused": pkg.collect_fused, "loop": pkg.collect}
        envs = {k: new_env() for k in calls}
        policies = {k: pkg.FusedPolicy(actor, critic, seed=1) for k in calls}
        bufs = {k: pkg.RolloutBuffer(T) for k in calls}
        run = lambda k: calls[k](envs[k], policies[k], bufs[k], gamma=args.gamma)
        # warm-up rollout of each arm, equally seeded: equal bits at this size
        outs = {k: run(k) for k in calls}
        torch.cuda.synchronize()
        differ = [n for i, n in enumerate(ENTRIES)
                  if not same_bits(bufs["fused"].stacked(i), bufs["loop"].stacked(i))]
        if not same_bits(bufs["fused"].returns, bufs["loop"].returns):
            differ.append("returns")
        if float(outs["fused"][0]) != float(outs["loop"][0]) or outs["fused"][1] != outs["loop"][1]:
            differ.append("mean/stats")
        if not torch.equal(envs["fused"].states, envs["loop"].states):
            differ.append("states")
        episodes_ended = bool(bufs["fused"].stacked(5).any())
        per_step = {k: [] for k in calls}
        for _ in range(a.reps):
            for k in calls:
                per_step[k].append(timed(lambda: run(k)) / T)
        med = {k: sorted(v)[len(v) // 2] for k, v in per_step.items()}
        rec = {"shape": shape, "hidden": H, "steps": T,
               "fused_us_per_step": round(med["fused"], 2),
               "loop_us_per_step": round(med["loop"], 2),
               "speedup": round(med["loop"] / med["fused"], 2),
               "fused_reps": [round(x, 2) for x in per_step["fused"]],
               "loop_reps": [round(x, 2) for x in per_step["loop"]],
               "bit_equal": not differ, "differ": differ, "episodes_ended": episodes_ended}
        print(json.dumps(rec), flush=True)
        if differ:
            raise SystemExit(f"{shape}: the two arms differ in {differ}")
        del envs, policies, bufs, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
