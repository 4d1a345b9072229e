"""Cost of the GAE(lambda) advantage mode on one GPU, each
figure against the yardstick that already exists, both arms in the same
process:

* the GAE tail of a rollout, ``FusedPolicy.values`` of the observations after
  the last step plus ``rollout.gae_advantages`` (one launch and five), against
  ``rollout.discounted_returns`` (five launches) at the same ``T x P``;
* one actor minibatch update (``FusedPPO.actor_update``, loss, gradients and
  Adam as one C call) with ``advantage='gae'`` (own-env pairing) against
  ``advantage='reference'`` on the same rollout, each arm with its own copy of
  the weights.

Setup: H = 50, ``buffer_len`` 16, ``batch_size`` 8. Device events around
``--iters`` calls after a warm-up, the arms alternating ``--reps`` times;
medians and the spread (min .. max) of the repetitions, in us per call. Each
arm is timed issued eagerly (the host's allocations and enqueue rate are part
of it) and as a captured graph replayed (device time alone).
profiles/gae_bench.txt holds two runs.

    python scripts/gae_bench.py [--shapes 65536x3x3,16384x3x3,1024x3x8,4096x16x32]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from train_bench import captured, med_spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x3x3,16384x3x3,1024x3x8,4096x16x32")
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--buffer-len", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gae_bench.py needs a HIP device")
    import marlnav_amd as pkg
    dev = "cuda"
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; H={a.hidden}, "
          f"buffer_len {a.buffer_len}, batch_size {a.batch}, lambda {a.gae_lambda}; {a.iters} "
          f"calls per timing, {a.reps} alternating reps, medians [min, max], us", flush=True)
    for shape in a.shapes.split(","):
        P, A, O = (int(x) for x in shape.split("x"))
        args = pkg.default_args(num_parallel=P, num_agents=A, num_obstacles=O,
                                hidden_size=a.hidden, buffer_len=a.buffer_len, batch_size=a.batch,
                                num_epochs=1, learning_rate=3e-4, num_total=a.buffer_len * P)
        args.gae_lambda = a.gae_lambda
        params = pkg.set_env_params(args, dev)
        params["rng"], params["seed"] = "native", 17
        torch.manual_seed(0)
        m = pkg.MAPPO(pkg.set_model_params(args, dev), pkg.Env(params), seed=1)
        m.get_data()
        buf, policy = m.buffer, m.policy
        rewards, done, values = buf.stacked(buf.REWARDS), buf.stacked(buf.DONE), buf.stacked(buf.VALUES)
        last_obs = buf.stacked(0)[-1].clone()     # any (P, A, D) normalised observations
        last_values = torch.empty(P, 1, device=dev)

        def tail():
            policy.values(last_obs, out=last_values)
            pkg.rollout.gae_advantages(rewards, done, values, last_values, args.gamma,
                                       a.gae_lambda)

        def returns():
            pkg.rollout.discounted_returns(rewards, done, args.gamma)

        ppo, adam = {}, {}
        for mode in ("reference", "gae"):
            actor, critic = copy.deepcopy(m.actor), copy.deepcopy(m.critic)
            ppo[mode] = pkg.FusedPPO(actor, critic, args.epsilon, args.ent_const, advantage=mode)
            adam[mode] = pkg.FusedAdam(actor.parameters(), lr=args.learning_rate, maximize=True)
        arms = {"gae_tail": tail, "returns": returns,
                "actor_update_env": lambda: ppo["gae"].actor_update(buf, 0, a.batch, adam["gae"]),
                "actor_update_reference":
                    lambda: ppo["reference"].actor_update(buf, 0, a.batch, adam["reference"])}
        for fn in arms.values():              # warm-up: workspaces, code objects
            fn()
        torch.cuda.synchronize()
        replay = {k: captured(fn) for k, fn in arms.items()}
        times = {(k, how): [] for k in arms for how in ("eager", "graph")}
        for _ in range(a.reps):
            for k in arms:
                times[(k, "eager")].append(timed(arms[k], a.iters))
                times[(k, "graph")].append(timed(replay[k], a.iters))
        for mode in ppo:
            for p in ppo[mode].actor.parameters():
                assert bool(torch.isfinite(p).all())
        rec = {"shape": shape, "hidden": a.hidden, "T": a.buffer_len, "batch": a.batch}
        for (k, how), ts in times.items():
            rec[f"{k}_{how}_us"], rec[f"{k}_{how}_spread"] = med_spread(ts)
        print(json.dumps(rec), flush=True)
        del m, buf, ppo, adam, replay
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
