"""What global-norm gradient clipping costs per update, three
arms in the same process on the same rollout buffer:

* ``unclipped``: ``MAPPO.train_actor()`` + ``MAPPO.train_critic()`` as they
  are without ``max_grad_norm``: one ``marlnav_ppo_train_phase`` call per
  network, the Adam step folded into the finish launch where §14 folds it;
* ``clipped``: the same trainer built with ``max_grad_norm``: one
  ``marlnav_ppo_train_phase_clipped`` call per network, with
  ``marlnav_debug_clip_fold(0)``: every update the unfolded gradient launches
  and the clipped step's three;
* ``clipped_fold`` (actors of up to 1 024 elements): the same with
  ``marlnav_debug_clip_fold(1)``, the default: the actor's norm, clip and Adam
  step inside ``actor_finish``, two launches per update.

Method of scripts/train_bench.py: H = 50, ``buffer_len`` 16, ``batch_size`` 8,
4 epochs (8 updates per network and phase), device events around ``--iters``
phases after a warm-up, the arms alternating ``--reps`` times; medians and the
spread (min .. max) of the repetitions, in us per update, issued eagerly and as
a captured graph replayed. Run it twice.

    python scripts/clip_bench.py [--shapes 65536x3x3,16384x3x3,1024x3x8,4096x16x32]
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


def build(pkg, P, A, O, a, dev, max_grad_norm):
    args = pkg.default_args(num_parallel=P, num_agents=A, num_obstacles=O, hidden_size=a.hidden,
                            buffer_len=a.buffer_len, batch_size=a.batch, num_epochs=a.epochs,
                            learning_rate=3e-4, num_total=a.buffer_len * P)
    args.max_grad_norm = max_grad_norm
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
    ap.add_argument("--max-grad-norm", type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench.py needs a HIP device")
    import marlnav_amd as pkg
    dev = "cuda"
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; H={a.hidden}, "
          f"buffer_len {a.buffer_len}, batch_size {a.batch}, {a.epochs} epochs, max_grad_norm "
          f"{a.max_grad_norm}; {a.iters} phases per timing, {a.reps} alternating reps, medians "
          f"[min, max], us per update", flush=True)
    for shape in a.shapes.split(","):
        P, A, O = (int(x) for x in shape.split("x"))
        plain = build(pkg, P, A, O, a, dev, None)
        clip = build(pkg, P, A, O, a, dev, a.max_grad_norm)
        plain.get_data()
        clip.get_data()                       # the same seeds: the same rollout
        updates = a.epochs * len(pkg.minibatch_bounds(a.buffer_len, a.batch))
        lib = pkg.abi.load_library()

        def hooked(fold, fn):
            # the hook is read when the launches are enqueued: eagerly, or at capture
            def run():
                before = lib.marlnav_debug_clip_fold(fold)
                try:
                    fn()
                finally:
                    lib.marlnav_debug_clip_fold(before)
            return run

        arms = {"unclipped": (plain.train_actor, plain.train_critic),
                "clipped": (hooked(0, clip.train_actor), clip.train_critic)}
        folds = sum(p.numel() for p in clip.actor.parameters()) <= 1024
        if folds:
            arms["clipped_fold"] = (hooked(1, clip.train_actor), clip.train_critic)
        for fa, fc in arms.values():          # warm-up: workspaces, code objects
            fa()
            fc()
        torch.cuda.synchronize()
        replay = {k: (captured(fa), captured(fc)) for k, (fa, fc) in arms.items()}
        times = {(k, how): ([], []) for k in arms for how in ("eager", "graph")}
        for _ in range(a.reps):
            for k in arms:
                for how, (fa, fc) in (("eager", arms[k]), ("graph", replay[k])):
                    times[(k, how)][0].append(timed(fa, a.iters) / updates)
                    times[(k, how)][1].append(timed(fc, a.iters) / updates)
        for m in (plain, clip):
            for mod in (m.actor, m.critic):
                for p in mod.parameters():
                    assert bool(torch.isfinite(p).all())
        norms = clip.logs()
        rec = {"shape": shape, "hidden": a.hidden, "updates_per_network": updates,
               "actor_elements": sum(p.numel() for p in clip.actor.parameters()),
               "critic_elements": sum(p.numel() for p in clip.critic.parameters()),
               "last_actor_grad_norm": norms["actor_grad_norm"][-1],
               "last_critic_grad_norm": norms["critic_grad_norm"][-1]}
        for (k, how), (ta, tc) in times.items():
            rec[f"actor_{k}_{how}_us"], rec[f"actor_{k}_{how}_spread"] = med_spread(ta)
            rec[f"critic_{k}_{how}_us"], rec[f"critic_{k}_{how}_spread"] = med_spread(tc)
        if folds:
            rec["actor_fold_gain_graph_us"] = round(rec["actor_clipped_graph_us"]
                                                    - rec["actor_clipped_fold_graph_us"], 2)
            for k in [k for k in rec if k.startswith("critic_clipped_fold")]:
                del rec[k]                    # the critic has no fold: the clipped arm again
        # what the option costs: the clipped phase as it runs by default (the
        # fold where the actor has one) against the unclipped phase
        best = "clipped_fold" if folds else "clipped"
        rec["actor_cost_graph_us"] = round(rec[f"actor_{best}_graph_us"]
                                           - rec["actor_unclipped_graph_us"], 2)
        rec["critic_cost_graph_us"] = round(rec["critic_clipped_graph_us"]
                                            - rec["critic_unclipped_graph_us"], 2)
        print(json.dumps(rec), flush=True)
        del plain, clip, replay, arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
