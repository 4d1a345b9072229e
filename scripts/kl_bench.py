"""What the actor's diagnostics and the target-KL stop cost per update
(DESIGN.md §17), three arms in the same process on the same rollout buffer:

* ``plain``: ``MAPPO.train_actor()`` as it is without the options: one
  ``marlnav_ppo_train_phase`` call, the Adam step folded into the finish
  launch where §14 folds it;
* ``monitored``: the same trainer built with ``log_diagnostics``
  (``target_kl = inf``): one ``marlnav_ppo_train_phase_monitored`` call, every
  update the diagnostic gradient launches and the gated Adam launches;
* ``stopped``: the same with a target below any KL, after a warm-up that has
  moved the policy away from the rollout's: the phase stops at its first
  update, so its other updates are skipped. (phase - one monitored update) /
  (updates - 1) is the cost of a skipped update, which is launches only.

Method of scripts/train_bench.py and scripts/clip_bench.py: H = 50,
``buffer_len`` 16, ``batch_size`` 8, 4 epochs (8 updates per phase), device
events around ``--iters`` phases after a warm-up, the arms alternating
``--reps`` times; medians and the spread (min .. max) of the repetitions, in
us per update, issued eagerly and as a captured graph replayed. Run it twice.

    python scripts/kl_bench.py [--shapes 65536x3x3,16384x3x3,1024x3x8,4096x16x32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from train_bench import captured, med_spread, timed  # noqa: E402


def build(pkg, P, A, O, a, dev, **options):
    args = pkg.default_args(num_parallel=P, num_agents=A, num_obstacles=O, hidden_size=a.hidden,
                            buffer_len=a.buffer_len, batch_size=a.batch, num_epochs=a.epochs,
                            learning_rate=3e-4, num_total=a.buffer_len * P)
    for k, v in options.items():
        setattr(args, k, v)
    params = pkg.set_env_params(args, dev)
    params["rng"], params["seed"] = "native", 17
    torch.manual_seed(0)
    return pkg.MAPPO(pkg.set_model_params(args, dev), pkg.Env(params), seed=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x3x3,16384x3x3,1024x3x8,4096x16x32")
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--buffer-len", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kl_bench.py needs a HIP device")
    import marlnav_amd as pkg
    dev = "cuda"
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; H={a.hidden}, "
          f"buffer_len {a.buffer_len}, batch_size {a.batch}, {a.epochs} epochs; the actor phase; "
          f"{a.iters} phases per timing, {a.reps} alternating reps, medians [min, max], us per "
          f"update (stopped: us per phase)", flush=True)
    for shape in a.shapes.split(","):
        P, A, O = (int(x) for x in shape.split("x"))
        plain = build(pkg, P, A, O, a, dev)
        mon = build(pkg, P, A, O, a, dev, log_diagnostics=True)
        stop = build(pkg, P, A, O, a, dev, target_kl=1e300)
        for m in (plain, mon, stop):
            m.get_data()                      # the same seeds: the same rollout
        updates = a.epochs * len(pkg.minibatch_bounds(a.buffer_len, a.batch))
        arms = {"plain": plain.train_actor, "monitored": mon.train_actor,
                "stopped": stop.train_actor}
        for fn in arms.values():              # warm-up: workspaces, code objects; the policy moves
            fn()
        stop.target_kl = 1e-300               # read when the launches are enqueued or captured
        arms["stopped"]()
        torch.cuda.synchronize()
        replay = {k: captured(fn) for k, fn in arms.items()}
        times = {(k, how): [] for k in arms for how in ("eager", "graph")}
        for _ in range(a.reps):
            for k in arms:
                for how, fn in (("eager", arms[k]), ("graph", replay[k])):
                    t = timed(fn, a.iters)
                    times[(k, how)].append(t if k == "stopped" else t / updates)
        logs = {k: m.logs() for k, m in (("monitored", mon), ("stopped", stop))}
        assert logs["stopped"]["actor_stopped_at"] == [0], logs["stopped"]["actor_stopped_at"]
        assert logs["stopped"]["actor_status"] == [1] + [2] * (updates - 1)
        assert logs["monitored"]["actor_stopped_at"] == [-1]
        for m in (plain, mon, stop):
            for p in m.actor.parameters():
                assert bool(torch.isfinite(p).all())
        rec = {"shape": shape, "hidden": a.hidden, "updates": updates,
               "actor_elements": sum(p.numel() for p in plain.actor.parameters()),
               "last_approx_kl": logs["monitored"]["actor_approx_kl"][-1],
               "last_clip_frac": logs["monitored"]["actor_clip_frac"][-1]}
        for (k, how), ts in times.items():
            unit = "phase_us" if k == "stopped" else "us"
            rec[f"{k}_{how}_{unit}"], rec[f"{k}_{how}_spread"] = med_spread(ts)
        for how in ("eager", "graph"):
            rec[f"monitor_cost_{how}_us"] = round(rec[f"monitored_{how}_us"]
                                                  - rec[f"plain_{how}_us"], 2)
            rec[f"skipped_update_{how}_us"] = round(
                (rec[f"stopped_{how}_phase_us"] - rec[f"monitored_{how}_us"]) / (updates - 1), 2)
        print(json.dumps(rec), flush=True)
        del plain, mon, stop, replay, arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
