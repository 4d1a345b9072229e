"""Command line of marlnav_amd, mirroring the reference's
``python -m marlnav`` (marlnav/__main__.py): same arguments and defaults.

Implemented modes: the reward check (``-rc``, utils.py:579-666 via
__main__.py:36-42) on the HIP environment step, and the two marlnav_amd-only
flags below. Without a mode flag (the reference's training default) and with
``-re`` the command says what to use and returns 2: the reference's own MAPPO
and animation take ``marlnav_amd.Env`` as their environment.

    python -m marlnav_amd -rc -se 0            # config-1 reward check
    python -m marlnav_amd -rc -sn 0 -ms 400    # mock scenario 0

``--evaluate`` (marlnav_amd only) runs a trained actor on the device for
``-ms`` steps (``marlnav_amd.evaluate``): what ``-re -sa policy -w FILE`` does
per frame in the reference (animation.py:40-71), without the window, and
prints the episode figures as one JSON line.

    python -m marlnav_amd --evaluate -w weights/X_actor.pt -np 4096 -ms 1000

``--train`` (marlnav_amd only) is the reference's default mode (__main__.py:
16-28) on the device (``marlnav_amd.MAPPO``): ``num_total // (buffer_len *
num_parallel)`` repeats of rollout, actor phase and critic phase, then the
reference's weight files, CSVs, params file and figures, and one JSON line.

    python -m marlnav_amd --train -np 4096 -bl 16 -bs 8 -ne 4 -nt 1048576

``--gae-lambda L`` with ``--train`` selects the GAE(lambda) advantage mode
 instead of the reference's normalised returns.

    python -m marlnav_amd --train --gae-lambda 0.95 -np 4096 -bl 16 -bs 8 -ne 4 -nt 1048576

``--max-grad-norm G`` with ``--train`` clips every update's gradient by its
global L2 norm and adds the two ``_gnorm.csv`` logs; it
composes with ``--gae-lambda``.

    python -m marlnav_amd --train --max-grad-norm 0.5 -np 4096 -bl 16 -bs 8 -ne 4 -nt 1048576

``--target-kl K`` with ``--train`` abandons the remaining actor updates of a
rollout once an update's approximate KL divergence from the rollout policy
exceeds K (decided on the device, before that update's
optimiser step; Stable-Baselines3 compares with 1.5 K, so pass 1.5 times its
value for its rule). ``--log-diagnostics`` records every actor update's
approximate KL, clip fraction, entropy and surrogate without stopping. Either
adds ``_act_kl.csv``, ``_act_clipfrac.csv``, ``_act_entropy.csv``,
``_act_stop.csv`` and the figure ``_act_kl.png``; both compose with
``--gae-lambda`` and ``--max-grad-norm``.

    python -m marlnav_amd --train --target-kl 0.02 -np 4096 -bl 16 -bs 8 -ne 4 -nt 1048576

``--shuffle-minibatches`` with ``--train`` draws a fresh random permutation of
all ``buffer_len`` stored steps per epoch, on the device, and cuts the
minibatches from it, the buffer's final step included; the
default walks the reference's fixed contiguous slices. Keyed by ``-se``; it
composes with every option above and is refused without ``--train``.

    python -m marlnav_amd --train --shuffle-minibatches -np 4096 -bl 16 -bs 8 -ne 4 -nt 1048576
"""
import argparse
import sys


def build_parser():
    """The reference's arguments (marlnav/__main__.py:49-132)."""
    p = argparse.ArgumentParser(prog="python -m marlnav_amd",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    a = p.add_argument
    a('-se', '--seed', type=int, help='value of the random seed (optional, default is None).')
    a('-mx', '--max_x_value', type=float, default=1500.0)
    a('-my', '--max_y_value', type=float, default=750.0)
    a('-fx', '--fig_size_x', type=float, default=10.0)
    a('-fy', '--fig_size_y', type=float, default=5.0)
    a('-pi', '--parallel_index', type=int, default=0)
    a('-ai', '--agent_index', type=int, default=0)
    a('-in', '--interval', type=int, default=10)
    a('-ra', '--random', action='store_true')
    a('-w', '--weights_file', type=str)
    a('-np', '--num_parallel', type=int, default=2)
    a('-na', '--num_agents', type=int, default=3)
    a('-no', '--num_obstacles', type=int, default=3)
    a('-ms', '--max_step', type=int, default=1000)
    a('-el', '--episode_len', type=int, default=200)
    a('-mis', '--min_speed', type=float, default=3.)
    a('-mas', '--max_speed', type=float, default=10.)
    a('-mia', '--min_accel', type=float, default=-0.5)
    a('-maa', '--max_accel', type=float, default=0.5)
    a('-rf', '--risk_factor', type=float, default=0.)
    a('-df', '--distance_factor', type=float, default=0.)
    a('-hf', '--heading_factor', type=float, default=500.)
    a('-tf', '--target_factor', type=float, default=500.)
    a('-sf', '--soft_factor', type=float, default=500.)
    a('-bf', '--bond_factor', type=float, default=10.)
    a('-hs', '--hidden_size', type=int, default=50)
    a('-lr', '--learning_rate', type=float, default=0.001)
    a('-ec', '--ent_const', type=float, default=0.001)
    a('-ep', '--epsilon', type=float, default=0.01)
    a('-g', '--gamma', type=float, default=0.9)
    a('-nt', '--num_total', type=int, default=1000000)
    a('-bl', '--buffer_len', type=int, default=1000)
    a('-ne', '--num_epochs', type=int, default=50)
    a('-bs', '--batch_size', type=int, default=1000)
    a('-re', '--rendering', action='store_true')
    a('-sa', '--sampling_style', type=str, default='sampler')
    a('-rc', '--reward_check', action='store_true')
    a('-sn', '--sampler_num', type=int, default=-1)
    # marlnav_amd only
    a('--rng', choices=('reference', 'native'), default='reference',
      help='re-init randomness: the reference torch RNG stream (bit-compatible '
           'with python -m marlnav) or the in-kernel Philox stream')
    a('--init-noise-device', choices=('auto', 'cpu'), default='auto',
      help="generator of the initializer's agent-noise draw: 'auto' = the env device, as "
           "the reference does on a GPU machine; 'cpu' = as on a CPU-only machine (the "
           "reference's CPU run, BASELINE configs[0])")
    a('--evaluate', action='store_true',
      help='run the actor of -w FILE for -ms steps on the device and print the episode '
           'figures as one JSON line; -ra samples actions (default: the mean action), -pi '
           'is the traced env of --trace-out and of the figure')
    a('--trace-out', metavar='FILE.npz',
      help='with --evaluate: save the traced env\'s states, obstacles, target, rewards and '
           'flags of every step')
    a('--train', action='store_true',
      help='train on the device with the model arguments above (-hs -lr -ec -ep -g -nt -bl '
           '-ne -bs) and write weights/, logs/ and plots/ under --out-dir; prints one JSON '
           'line')
    a('--track-best', action='store_true',
      help='with --train: keep the weights of the rollout with the highest mean reward (the '
           'reference never raises its maximum and so keeps the weights from before the '
           'last repeat\'s training, which is the default here too)')
    a('--save-every', type=int, default=0, metavar='N',
      help='with --train: also write the weight files after every N repeats')
    a('--gae-lambda', type=float, default=None, metavar='LAMBDA',
      help='with --train: GAE(lambda) advantages in [0, 1] with own-env pairing, the terminal '
           'reward kept and a bootstrap value (default: the reference\'s normalised returns)')
    a('--max-grad-norm', type=float, default=None, metavar='G',
      help='with --train: clip every update\'s gradient to the global L2 norm G > 0, as '
           'clip_grad_norm_ does (default: no clipping)')
    a('--target-kl', type=float, default=None, metavar='K',
      help='with --train: stop a rollout\'s actor updates once the approximate KL divergence '
           'from the rollout policy exceeds K > 0 (default: no stop)')
    a('--log-diagnostics', action='store_true',
      help='with --train: log every actor update\'s approximate KL, clip fraction, entropy '
           'and surrogate')
    a('--shuffle-minibatches', action='store_true',
      help='with --train: a fresh random permutation of all stored steps per epoch, cut into '
           'the minibatches (default: the reference\'s fixed contiguous slices, which never '
           'train on the buffer\'s final step)')
    a('--out-dir', default='.', help='with --train: where weights/, logs/ and plots/ go')
    a('--plot-dir', default='plots', help='directory of the saved figures')
    a('--no-plots', action='store_true', help='skip the figures, print the series')
    return p


def main(argv=None):
    import importlib

    import torch
    pkg = importlib.import_module("marl-nav_amd")
    args = build_parser().parse_args(argv)
    if args.shuffle_minibatches and not args.train:
        print("--shuffle-minibatches is an option of --train (marlnav_amd.MAPPO)", file=sys.stderr)
        return 2
    if args.evaluate:
        return _evaluate(pkg, args)
    if args.train:
        return _train(pkg, args)
    if not args.reward_check:
        mode = 'rendering' if args.rendering else 'training'
        print(f"marlnav_amd implements the environment step; {mode} is the reference's "
              "own code (MAPPO / animation): run it with marlnav_amd.Env as its "
              "environment (INTEGRATION.md). Use -rc for the reward check, --evaluate to run "
              "a trained actor without the window, --train for the device training mode "
              "(marlnav_amd.MAPPO).",
              file=sys.stderr)
        return 2
    if not torch.cuda.is_available():
        print("marlnav_amd needs a HIP device (no CPU fallback)", file=sys.stderr)
        return 1
    device = 'cuda'
    if args.seed is not None:
        pkg.set_all_seeds(args.seed)          # __main__.py:137-138
    env_params = pkg.set_env_params(args, device)
    env_params['rng'] = args.rng
    if args.init_noise_device == 'cpu':
        env_params['init'] = dict(env_params['init'], noise_device='cpu')
    anim = pkg.utils.set_animation_params(args, device)
    env = pkg.Env(env_params)
    series = pkg.utils.check_rews(env, anim['max_step'], anim['parallel_index'],
                                  anim['agent_index'], plot_dir=args.plot_dir,
                                  plot=not args.no_plots)
    if args.no_plots:
        for k, v in series.items():
            print(k, " ".join(f"{x:.9g}" for x in v))
    else:
        print(f"saved figures under {args.plot_dir}/")
    return 0


def _evaluate(pkg, args):
    """``--evaluate``: init_render's policy branch (animation.py:80-96) and
    Animation.update's loop (:40-71) for ``-ms`` steps, as one call."""
    import json

    import torch
    if not torch.cuda.is_available():
        print("marlnav_amd needs a HIP device (no CPU fallback)", file=sys.stderr)
        return 1
    if not args.weights_file:
        print("--evaluate needs the actor's weights: -w FILE (the reference's *_actor.pt)",
              file=sys.stderr)
        return 2
    device = 'cuda'
    if args.seed is not None:
        pkg.set_all_seeds(args.seed)
    env_params = pkg.set_env_params(args, device)
    env_params['rng'] = 'native'           # the host is not in the loop: in-kernel re-init
    if args.seed is not None:
        env_params['seed'] = args.seed
    env = pkg.Env(env_params)
    env.attach_normalizer(pkg.ObsNormalizer(pkg.set_normalizer_params(args, device)))
    env.attach_action_scaler(pkg.ActionScaler(pkg.set_scaler_params(args, device)))
    actor = pkg.FusedActor.from_state_dict(
        torch.load(args.weights_file, map_location='cpu', weights_only=True), device,
        seed=args.seed or 0)
    want_trace = bool(args.trace_out) or not args.no_plots
    res = pkg.evaluate(env, actor, args.max_step, mode='sample' if args.random else 'mean',
                       trace_env=args.parallel_index if want_trace else None)
    print(json.dumps(res.as_dict()))
    if res.trace is None:
        return 0
    trace = {k: v.cpu().numpy() for k, v in res.trace.items()}
    if args.trace_out:
        import numpy as np
        np.savez(args.trace_out, **trace)
    if not args.no_plots:
        _plot_trace(trace, args)
    return 0


def _train(pkg, args):
    """``--train``: main()'s training branch (__main__.py:16-28)."""
    import json

    import torch
    if not torch.cuda.is_available():
        print("marlnav_amd needs a HIP device (no CPU fallback)", file=sys.stderr)
        return 1
    device = 'cuda'
    if args.seed is not None:
        pkg.set_all_seeds(args.seed)
    try:
        if args.gae_lambda is not None:
            pkg.rollout._check_lambda(args.gae_lambda)
        model_params = pkg.set_model_params(args, device)
    except ValueError as e:
        print(f"--train: {e}", file=sys.stderr)
        return 2
    env_params = pkg.set_env_params(args, device)
    env_params['rng'] = 'native'           # the host is not in the loop: in-kernel re-init
    if args.seed is not None:
        env_params['seed'] = args.seed
    env = pkg.Env(env_params)
    mappo = pkg.MAPPO(model_params, env, seed=args.seed or 0, track_best=args.track_best,
                      out_dir=args.out_dir)
    repeats = args.num_total // (args.buffer_len * args.num_parallel)
    weights = mappo.run(repeats, save_every=args.save_every or None)
    full = {'env': env_params, 'model': model_params,
            'animation': pkg.utils.set_animation_params(args, device)}
    files = mappo.save_stats(full, plot=not args.no_plots)
    logs = mappo._logs
    print(json.dumps({"repeats": repeats,
                      "last_mean_rew": logs['mean_rews'][-1] if logs['mean_rews'] else None,
                      "saves": mappo.save_count()[0],
                      "weights": list(weights) if weights else [], "files": files}))
    return 0


def _plot_trace(trace, args):
    """One static figure of the traced env: every agent's path, the obstacles
    and the target (the reference animates the same scatter, animation.py:
    14-38), saved as check_rews saves its figures."""
    import os
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        return
    fig, ax = plt.subplots(figsize=(args.fig_size_x, args.fig_size_y))
    st = trace["states"]
    for a in range(st.shape[1]):
        ax.plot(st[:, a, 0], st[:, a, 1], lw=0.8, label=f"agent {a}")
    ax.scatter(trace["obstacles"][:, :, 0], trace["obstacles"][:, :, 1], s=12, c='k',
               label="obstacles")
    ax.scatter(trace["target"][:, 0], trace["target"][:, 1], s=40, c='r', marker='*',
               label="target")
    ax.set_xlim(0, args.max_x_value)
    ax.set_ylim(0, args.max_y_value)
    ax.legend(loc='upper right', fontsize=7)
    os.makedirs(args.plot_dir, exist_ok=True)
    fig.savefig(os.path.join(args.plot_dir, f"evaluate_env_{args.parallel_index}.png"))
    plt.close(fig)


if __name__ == "__main__":
    sys.exit(main())
