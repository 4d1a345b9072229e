"""Time of the training phases of one rollout on one GPU, two arms in the same
process:

* ``phase``: ``MAPPO.train_actor()`` + ``MAPPO.train_critic()``: one
  ``marlnav_ppo_train_phase`` call per network, every update two launches for
  the actor and two or three for the critic, the Adam step folded into the
  finish launch;
* ``loops``: ``rollout.train_actor`` + ``rollout.train_critic`` with a
  ``FusedAdam``: one ``marlnav_ppo_*_update`` call per minibatch, four or five
  launches each (§11), on the same buffer with its own copy of the weights.

Setup: H = 50, ``buffer_len`` 16, ``batch_size`` 8, 4 epochs (8 updates per
network and phase). Device events around ``--iters`` phases after a warm-up,
the arms alternating ``--reps`` times; medians and the spread (min .. max) of
the repetitions, in us per update. Each arm is timed twice: issued eagerly
(the host's enqueue rate is part of it: one C call per phase against one per
update) and as a captured graph replayed (device time alone, which is where
the fold itself shows). Also us per ``MAPPO.repeat()`` against
``collect_fused`` + the existing loops.

``--profile``: no timing; one phase of each arm and nothing else after the
rollout, for a kernel trace that counts the launches per update.

    python scripts/train_bench.py [--shapes 65536x3x3,16384x3x3,1024x3x8,4096x16x32]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def med_spread(xs):
    s = sorted(xs)
    return round(s[len(s) // 2], 2), [round(s[0], 2), round(s[-1], 2)]


def build(pkg, P, A, O, a, dev):
    args = pkg.default_args(num_parallel=P, num_agents=A, num_obstacles=O, hidden_size=a.hidden,
                            buffer_len=a.buffer_len, batch_size=a.batch, num_epochs=a.epochs,
                            learning_rate=3e-4, num_total=a.buffer_len * P)
    params = pkg.set_env_params(args, dev)
    params["rng"], params["seed"] = "native", 17
    torch.manual_seed(0)
    return pkg.MAPPO(pkg.set_model_params(args, dev), pkg.Env(params), seed=1), args


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x3x3,16384x3x3,1024x3x8,4096x16x32")
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--buffer-len", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_bench.py needs a HIP device")
    import marlnav_amd as pkg
    dev = "cuda"
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; H={a.hidden}, "
          f"buffer_len {a.buffer_len}, batch_size {a.batch}, {a.epochs} epochs; {a.iters} "
          f"phases per timing, {a.reps} alternating reps, medians [min, max], us", flush=True)
    for shape in a.shapes.split(","):
        P, A, O = (int(x) for x in shape.split("x"))
        m, args = build(pkg, P, A, O, a, dev)
        m.get_data()
        buf = m.buffer
        updates = a.epochs * len(pkg.minibatch_bounds(a.buffer_len, a.batch))
        # the loops arm: its own weights (a copy) and optimisers over the same buffer
        actor, critic = copy.deepcopy(m.actor), copy.deepcopy(m.critic)
        ppo = pkg.FusedPPO(actor, critic, args.epsilon, args.ent_const)
        adam_a = pkg.FusedAdam(actor.parameters(), lr=args.learning_rate, maximize=True)
        adam_c = pkg.FusedAdam(critic.parameters(), lr=args.learning_rate, maximize=False)
        arms = {
            "phase": (m.train_actor, m.train_critic),
            "loops": (lambda: pkg.train_actor(ppo, buf, adam_a, a.epochs, a.batch),
                      lambda: pkg.train_critic(ppo, buf, adam_c, a.epochs, a.batch)),
        }
        for fa, fc in arms.values():        # warm-up: workspaces, code objects
            fa()                            # (with --profile: the one phase that is traced)
            fc()
        torch.cuda.synchronize()
        if a.profile:
            print(json.dumps({"shape": shape, "profile": True, "updates_per_network": updates,
                              "phases_per_arm": 1}), flush=True)
            continue
        replay = {k: (captured(fa), captured(fc)) for k, (fa, fc) in arms.items()}
        times = {(k, how): ([], []) for k in arms for how in ("eager", "graph")}
        for _ in range(a.reps):
            for k in arms:
                for how, (fa, fc) in (("eager", arms[k]), ("graph", replay[k])):
                    times[(k, how)][0].append(timed(fa, a.iters) / updates)
                    times[(k, how)][1].append(timed(fc, a.iters) / updates)
        for mod in (m.actor, m.critic, actor, critic):
            for p in mod.parameters():
                assert bool(torch.isfinite(p).all())
        # a whole repeat: rollout, actor phase, critic phase
        m2, _ = build(pkg, P, A, O, a, dev)
        env2 = m2.env                         # an env with normaliser and scaler attached
        pol2 = pkg.FusedPolicy(actor, critic, seed=1)
        buf2 = pkg.RolloutBuffer(a.buffer_len)

        def hand():
            pkg.collect_fused(env2, pol2, buf2, gamma=args.gamma)
            pkg.train_actor(ppo, buf2, adam_a, a.epochs, a.batch)
            pkg.train_critic(ppo, buf2, adam_c, a.epochs, a.batch)

        m.repeat()
        hand()
        rep = {"repeat": [], "hand": []}
        for _ in range(a.reps):
            rep["repeat"].append(timed(m.repeat, 1))
            rep["hand"].append(timed(hand, 1))
        rec = {"shape": shape, "hidden": a.hidden, "updates_per_network": updates}
        for (k, how), (ta, tc) in times.items():
            rec[f"actor_{k}_{how}_us"], rec[f"actor_{k}_{how}_spread"] = med_spread(ta)
            rec[f"critic_{k}_{how}_us"], rec[f"critic_{k}_{how}_spread"] = med_spread(tc)
        rec["repeat_us"], rec["repeat_spread"] = med_spread(rep["repeat"])
        rec["collect_fused_plus_loops_us"], rec["collect_fused_plus_loops_spread"] = \
            med_spread(rep["hand"])
        print(json.dumps(rec), flush=True)
        del m, m2, buf, buf2, ppo, replay
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
