"""Per-step time of an evaluation, one C call against the per-step loop, on
one GPU:

* ``fused``: ``marlnav_amd.evaluate`` (``marlnav_rollout_evaluate``: the actor
  launch, the step launch and the tracker launch of every step and the totals
  enqueued by one call), mean actions;
* ``loop``: what there was before it: per step ``FusedPolicy.act`` with zero
  ``eps`` (actor, log-prob and critic in one launch), ``env.step`` through the
  host engine, and the tracker's rule as torch fp64 tensor ops
  (tests/eval_ref.py).

Both arms drive their own identically seeded Env over the same weights. The
first (warm-up) evaluation of each arm doubles as the check that every per-env
figure and the env states are equal bit for bit at the size timed. Then device
events around one evaluation of ``--steps`` steps (>= 200), the two arms
alternating ``--reps`` times (>= 3); the read of the episode counters and of
the totals is inside the window of both.

Also the actor kernel alone against the policy kernel alone: for each a
hipGraph of ``--chain`` back-to-back launches replayed under events (so the
host's enqueue rate is not what is measured), per launch.

    python scripts/eval_bench.py [--shapes 65536x3x3,16384x3x3,1024x3x8,4096x16x32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
from torch import nn  # noqa: E402

import eval_ref  # noqa: E402


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


def loop(env, policy, T, zeros):
    """The per-step loop; returns the tracker and its totals (read back, as
    ``evaluate``'s are) and the episode endings."""
    before = env._counter_totals()
    tracker = eval_ref.EpisodeTracker(env._step_num.clone())
    obs_n = env._normalizer(env.observations())
    for _ in range(T):
        actions = policy.act(obs_n, eps=zeros)[0]
        obs, rew, term, trunc = env.step(actions)
        tracker.step(rew, term, trunc)
        obs_n = env._normalizer(obs)
    totals = tracker.totals()
    endings = [a - b for a, b in zip(env._counter_totals(), before)]
    return tracker, totals, endings


def fused(pkg, env, actor, T):
    res = pkg.evaluate(env, actor, T, mode='mean')
    res.episodes                       # the totals' read-back
    return res


def kernel_alone(launch, chain, replays):
    for s in range(3):
        launch(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for s in range(chain):
            launch(s)
    g.replay()
    ts = sorted(timed(g.replay) / chain for _ in range(replays))
    return round(ts[len(ts) // 2], 2), round(ts[0], 2), round(ts[-1], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x3x3,16384x3x3,1024x3x8,4096x16x32")
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chain", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py needs a HIP device")
    if a.steps < 200 or a.reps < 3:
        raise SystemExit("eval_bench.py times >= 200 steps per evaluation and >= 3 alternating reps")
    import marlnav_amd as pkg
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; "
          f"{a.steps} steps per evaluation, {a.reps} alternating reps, H={a.hidden}")
    for shape in a.shapes.split(","):
        P, A, O = (int(x) for x in shape.split("x"))
        D, H, T = 2 + 2 * O + 2 * (A - 1), a.hidden, a.steps
        args = pkg.default_args(num_parallel=P, num_agents=A, num_obstacles=O)
        nrm = pkg.ObsNormalizer(pkg.set_normalizer_params(args, dev))
        scl = pkg.ActionScaler(pkg.set_scaler_params(args, dev))
        actor_mod, critic_mod = modules(D, A * D, H, dev)

        def new_env():
            params = pkg.set_env_params(args, dev)
            params.update(rng="native", seed=20251003)
            env = pkg.Env(params)
            env.attach_normalizer(nrm)
            env.attach_action_scaler(scl)
            return env

        envs = {"fused": new_env(), "loop": new_env()}
        actor = pkg.FusedActor(actor_mod, seed=1)
        policy = pkg.FusedPolicy(actor_mod, critic_mod, seed=1)
        zeros = torch.zeros(P * A, 2, device=dev)
        arms = {"fused": lambda: fused(pkg, envs["fused"], actor, T),
                "loop": lambda: loop(envs["loop"], policy, T, zeros)}
        # warm-up evaluation of each arm, equally seeded: equal bits at this size
        res = arms["fused"]()
        tracker, totals, endings = arms["loop"]()
        torch.cuda.synchronize()
        differ = [n for n in eval_ref.PER_ENV
                  if not torch.equal(getattr(res, n), getattr(tracker, n))]
        if [res.endings[k] for k in ("trunc", "col", "tar")] != endings:
            differ.append("endings")
        if (res.episodes, res.partial_episodes) != totals[0][:2]:
            differ.append("totals")
        if not torch.equal(envs["fused"].states, envs["loop"].states):
            differ.append("states")
        per_step = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                per_step[k].append(timed(fn) / T)
        med = {k: sorted(v)[len(v) // 2] for k, v in per_step.items()}
        obs = nrm(envs["fused"].observations())
        out_a = torch.empty(P, A, 2, device=dev)
        out_p = (out_a, torch.empty(P * A, device=dev), torch.empty(P, 1, device=dev))
        alone = {
            "actor_mean": kernel_alone(lambda s: actor.act(obs, out=out_a), a.chain, 9),
            "actor_sample": kernel_alone(
                lambda s: actor.act(obs, mode='sample', step_idx=s, out=out_a), a.chain, 9),
            "policy": kernel_alone(lambda s: policy.act(obs, step_idx=s, out=out_p), a.chain, 9)}
        rec = {"shape": shape, "hidden": H, "steps": T,
               "fused_us_per_step": round(med["fused"], 2),
               "loop_us_per_step": round(med["loop"], 2),
               "speedup": round(med["loop"] / med["fused"], 2),
               "fused_reps": [round(x, 2) for x in per_step["fused"]],
               "loop_reps": [round(x, 2) for x in per_step["loop"]],
               "kernel_us_med_min_max": alone,
               "bit_equal": not differ, "differ": differ, "episodes": res.episodes,
               "partial_episodes": res.partial_episodes}
        print(json.dumps(rec), flush=True)
        if differ:
            raise SystemExit(f"{shape}: the two arms differ in {differ}")
        del envs, res, tracker
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
