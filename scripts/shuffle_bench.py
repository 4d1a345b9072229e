"""What the shuffled minibatches cost per update, three arms per
network in the same process on the same rollout buffer:

* ``shuffled``: ``MAPPO.train_actor()`` / ``train_critic()`` of a trainer built
  with ``shuffle_minibatches``: one ``marlnav_ppo_train_phase_shuffled`` call,
  the permutation launch, then per update the gather gradient launches and the
  Adam launches (nothing folded);
* ``contiguous``: the same unfolded launches on contiguous slices of the same
  size, ``FusedPPO.actor_loss_grad(buffer, lo, lo + batch)`` and
  ``FusedAdam.step()`` over ``[0, batch), [batch, 2 batch), ...`` for as many
  epochs: shuffled - contiguous is the gather (and 1 / updates of the
  permutation launch);
* ``default``: the shipped phase without the option, one
  ``marlnav_ppo_train_phase`` call with the Adam step folded where §14 folds
  it. Its last slice of an epoch is one step short (the reference's
  ``[start:-1]``), so it also reads 1 / buffer_len fewer rows: shuffled -
  default is what the lost fold, the gather and the extra step cost together.

And ``permutations``: the permutation launch alone (``buffer_len`` steps,
``epochs`` rows), per launch.

Method of scripts/kl_bench.py: H = 50, ``buffer_len`` 16, ``batch_size`` 8, 4
epochs (8 updates per phase), device events around ``--iters`` replays of a
captured graph, the arms alternating ``--reps`` times; medians and the spread
(min .. max) of the repetitions, in us per update. Run it twice.

    python scripts/shuffle_bench.py [--shapes 65536x3x3,16384x3x3,1024x3x8,4096x16x32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from kl_bench import build  # noqa: E402
from train_bench import captured, med_spread, timed  # noqa: E402


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
        raise SystemExit("shuffle_bench.py needs a HIP device")
    import marlnav_amd as pkg
    dev = "cuda"
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; H={a.hidden}, "
          f"buffer_len {a.buffer_len}, batch_size {a.batch}, {a.epochs} epochs; replayed graphs; "
          f"{a.iters} phases per timing, {a.reps} alternating reps, medians [min, max], us per "
          f"update (permutations: us per launch)", flush=True)
    sizes = pkg.shuffled_minibatch_sizes(a.buffer_len, a.batch)
    updates = a.epochs * len(sizes)
    for shape in a.shapes.split(","):
        P, A, O = (int(x) for x in shape.split("x"))
        plain = build(pkg, P, A, O, a, dev)
        shuf = build(pkg, P, A, O, a, dev, shuffle_minibatches=True)
        for m in (plain, shuf):
            m.get_data()                      # the same seeds: the same rollout

        def contiguous(m, grad, adam):
            def run():
                for _ in range(a.epochs):
                    for j in range(len(sizes)):
                        grad(m.buffer, j * a.batch, (j + 1) * a.batch)
                        adam.step()
            return run

        lib = pkg.abi.load_library()
        cell = torch.zeros(1, dtype=torch.int64, device=dev)
        table = torch.zeros(a.epochs, a.buffer_len, dtype=torch.int32, device=dev)

        def permutations():
            pkg.abi.check(lib.marlnav_minibatch_permutations(
                a.buffer_len, a.epochs, 1, 0, cell.data_ptr(), table.data_ptr(),
                torch.cuda.current_stream().cuda_stream), lib)

        arms = {
            ("actor", "shuffled"): shuf.train_actor,
            ("actor", "contiguous"): contiguous(plain, plain.ppo.actor_loss_grad,
                                                plain.actor_optimizer),
            ("actor", "default"): plain.train_actor,
            ("critic", "shuffled"): shuf.train_critic,
            ("critic", "contiguous"): contiguous(plain, plain.ppo.critic_loss_grad,
                                                 plain.critic_optimizer),
            ("critic", "default"): plain.train_critic,
            ("table", "permutations"): permutations,
        }
        # Every arm once before the first capture, the whole-buffer phases first:
        # FusedPPO reallocates its workspace when a call needs a larger one, and
        # a graph captured before that would keep the pointer of the freed one
        # (the 8-step calls of `contiguous` need less than a 16-step phase).
        for k in sorted(arms, key=lambda k: k[1] == "contiguous"):
            arms[k]()
        torch.cuda.synchronize()
        work = {id(m): m.ppo._work.data_ptr() for m in (plain, shuf)}
        replay = {k: captured(fn) for k, fn in arms.items()}
        assert work == {id(m): m.ppo._work.data_ptr() for m in (plain, shuf)}
        times = {k: [] for k in arms}
        for _ in range(a.reps):
            for k in arms:
                t = timed(replay[k], a.iters)
                times[k].append(t if k[0] == "table" else t / updates)
        for m in (plain, shuf):
            for p in list(m.actor.parameters()) + list(m.critic.parameters()):
                assert bool(torch.isfinite(p).all())
        last = shuf.ppo.last_steps["actor"]
        assert bool((last.sort(dim=1).values == torch.arange(a.buffer_len, device=dev)).all())
        rec = {"shape": shape, "hidden": a.hidden, "updates": updates,
               "actor_elements": sum(p.numel() for p in plain.actor.parameters())}
        for (net, arm), ts in times.items():
            name = arm if net == "table" else f"{net}_{arm}"
            rec[name + "_us"], rec[name + "_spread"] = med_spread(ts)
        for net in ("actor", "critic"):
            rec[f"{net}_gather_us"] = round(rec[f"{net}_shuffled_us"]
                                            - rec[f"{net}_contiguous_us"], 2)
            rec[f"{net}_over_default_us"] = round(rec[f"{net}_shuffled_us"]
                                                  - rec[f"{net}_default_us"], 2)
        print(json.dumps(rec), flush=True)
        del plain, shuf, replay, arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
