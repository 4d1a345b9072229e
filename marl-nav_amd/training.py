"""The training mode: the reference's ``MAPPO`` (marlnav/models.py:59-316)
and its loop (marlnav/__main__.py:23-27) with every phase enqueued on the
device by one C call and nothing read back until the logs are asked for
(DESIGN.md §14).

* ``Actor(input_size, hidden_size)`` / ``Critic(input_size, hidden_size)`` -
  the reference's modules (models.py:14-56) written from their contract: the
  attribute names, shapes and orthogonal weight init, so ``state_dict()``s move
  to and from the reference's modules and ``FusedActor.from_state_dict``.
* ``MAPPO(params, env)`` - the reference class's surface. ``get_data()`` is
  ``collect_fused`` plus the mean-reward and episode-counter logs and the
  checkpoint rule (libmarlnav.so ``marlnav_params_snapshot_if``), all on the
  device; ``train_actor()`` / ``train_critic()`` are one
  ``marlnav_ppo_train_phase`` call each; ``repeat()`` is the three in the
  reference's order with no host synchronisation from entry to return.
* ``train_phase(ppo, buffer, adam, network, num_epochs, batch_size)`` - the
  phase call alone, over any ``FusedPPO`` / ``RolloutBuffer`` / ``FusedAdam``.
* ``write_stats(logs, full_params, out_dir, stamp)`` - ``MAPPO.save_stats``
  (models.py:200-268) on a ``_logs`` dict: the four CSVs, ``_params.json`` and
  the four figures under the reference's file names.
"""
import csv
import ctypes
import json
import os
from datetime import datetime

import torch
from torch import nn

from . import abi, rollout
from .rollout import (FusedAdam, FusedPolicy, FusedPPO, RolloutBuffer, minibatch_bounds,
                      shuffled_minibatch_sizes)
from .utils import ActionScaler, ObsNormalizer

_F64 = torch.float64
ACTOR_KEYS = ("fc1.weight", "fc1.bias", "fc_mu.weight", "fc_mu.bias", "fc_std.weight",
              "fc_std.bias")
CRITIC_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


class Actor(nn.Module):
    """models.py:14-36: ``fc1`` (no activation), then ``tanh(fc_mu)`` as the
    mean and ``softplus(fc_std)`` as the covariance diagonal of a
    ``MultivariateNormal`` over the flattened agent rows."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.fc1 = nn.Linear(input_size, hidden_size)
        self.fc_mu = nn.Linear(hidden_size, 2)
        self.fc_std = nn.Linear(hidden_size, 2)
        for m in (self.fc1, self.fc_mu, self.fc_std):
            nn.init.orthogonal_(m.weight)

    def forward(self, x):
        x = self.fc1(x.flatten(0, 1))
        mu = torch.tanh(self.fc_mu(x))
        var = nn.functional.softplus(self.fc_std(x))
        return torch.distributions.MultivariateNormal(mu, torch.diag_embed(var))


class Critic(nn.Module):
    """models.py:39-56: ``fc2(relu(fc1(x)))`` over the env's flattened rows."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.fc1 = nn.Linear(input_size, hidden_size)
        self.fc2 = nn.Linear(hidden_size, 1)
        for m in (self.fc1, self.fc2):
            nn.init.orthogonal_(m.weight)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x.flatten(1))))


def _empty_logs():
    return {'epi_stats': {'trunc': [], 'col': [], 'tar': []}, 'mean_rews': [], 'actor': [],
            'critic': []}


def stats_paths(out_dir, stamp):
    """The reference's file names (models.py:84-92, 202-222) under
    ``out_dir``: -> dict of the two weight files, the four figures, the four
    CSVs and the params file."""
    w, p, l = (os.path.join(out_dir, d) for d in ('weights', 'plots', 'logs'))
    return {'actor': os.path.join(w, stamp + '_actor.pt'),
            'critic': os.path.join(w, stamp + '_critic.pt'),
            'rew_plot': os.path.join(p, stamp + '_mean_rews.png'),
            'act_plot': os.path.join(p, stamp + '_act_loss.png'),
            'cri_plot': os.path.join(p, stamp + '_cri_loss.png'),
            'epi_plot': os.path.join(p, stamp + '_epi_stats.png'),
            'params': os.path.join(l, stamp + '_params.json'),
            'rew_log': os.path.join(l, stamp + '_mean_rews.csv'),
            'act_log': os.path.join(l, stamp + '_act_loss.csv'),
            'cri_log': os.path.join(l, stamp + '_cri_loss.csv'),
            'epi_log': os.path.join(l, stamp + '_epi_stats.csv'),
            'act_gnorm_log': os.path.join(l, stamp + '_act_gnorm.csv'),
            'cri_gnorm_log': os.path.join(l, stamp + '_cri_gnorm.csv'),
            'act_kl_log': os.path.join(l, stamp + '_act_kl.csv'),
            'act_clipfrac_log': os.path.join(l, stamp + '_act_clipfrac.csv'),
            'act_entropy_log': os.path.join(l, stamp + '_act_entropy.csv'),
            'act_stop_log': os.path.join(l, stamp + '_act_stop.csv'),
            'act_kl_plot': os.path.join(p, stamp + '_act_kl.png')}


def write_stats(logs, full_params, out_dir, stamp, plot=True):
    """``MAPPO.save_stats`` (models.py:200-268) for a ``_logs`` dict of Python
    numbers: ``logs/<stamp>_params.json`` (indent 4, sorted keys; what json
    cannot write goes through ``str``), the three one-column CSVs (header
    ``Value``) and ``_epi_stats.csv`` (``Truncated, Collisions, Target
    reached``), and with ``plot`` the four figures under ``plots/``. Where
    ``logs`` has ``actor_grad_norm`` / ``critic_grad_norm`` (a run with
    ``max_grad_norm``) also ``_act_gnorm.csv`` /
    ``_cri_gnorm.csv``, one-column like the losses; a ``logs`` without them
    writes exactly the reference's files. Where ``logs`` has the actor's
    diagnostics (``actor_approx_kl`` ..., a run with ``target_kl`` or
    ``log_diagnostics``) also ``_act_kl.csv``,
    ``_act_clipfrac.csv``, ``_act_entropy.csv`` (one-column, one row per
    update), ``_act_stop.csv`` (header ``Stopped at``, one row per rollout, -1
    where the phase ran to its end) and with ``plot`` the figure
    ``_act_kl.png``; the NaN of an update behind a stop is written as it is.
    Returns the paths written."""
    paths = stats_paths(out_dir, stamp)
    os.makedirs(os.path.dirname(paths['params']), exist_ok=True)
    with open(paths['params'], 'w') as f:
        json.dump(full_params, f, indent=4, sort_keys=True, default=str)
    for key, name in (('mean_rews', 'rew_log'), ('actor', 'act_log'), ('critic', 'cri_log')):
        with open(paths[name], 'w', newline='') as f:
            writer = csv.writer(f)
            writer.writerow(['Value'])
            writer.writerows([[num] for num in logs[key]])
    epi = logs['epi_stats']
    with open(paths['epi_log'], 'w', newline='') as f:
        writer = csv.writer(f)
        writer.writerow(['Truncated', 'Collisions', 'Target reached'])
        writer.writerows([[epi['trunc'][i], epi['col'][i], epi['tar'][i]]
                          for i in range(len(epi['trunc']))])
    written = [paths[k] for k in ('params', 'rew_log', 'act_log', 'cri_log', 'epi_log')]
    for key, name in (('actor_grad_norm', 'act_gnorm_log'),
                      ('critic_grad_norm', 'cri_gnorm_log')):
        if key in logs:
            with open(paths[name], 'w', newline='') as f:
                writer = csv.writer(f)
                writer.writerow(['Value'])
                writer.writerows([[num] for num in logs[key]])
            written.append(paths[name])
    diag = 'actor_approx_kl' in logs
    if diag:
        for key, name, head in (('actor_approx_kl', 'act_kl_log', 'Value'),
                                ('actor_clip_frac', 'act_clipfrac_log', 'Value'),
                                ('actor_entropy', 'act_entropy_log', 'Value'),
                                ('actor_stopped_at', 'act_stop_log', 'Stopped at')):
            with open(paths[name], 'w', newline='') as f:
                writer = csv.writer(f)
                writer.writerow([head])
                writer.writerows([[num] for num in logs[key]])
            written.append(paths[name])
    if not plot:
        return written
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    os.makedirs(os.path.dirname(paths['rew_plot']), exist_ok=True)
    for key, xlabel, title, name in (('mean_rews', 'rollot_num', 'Mean Rewards', 'rew_plot'),
                                     ('actor', 'batch_num', 'Actor Losses', 'act_plot'),
                                     ('critic', 'batch_num', 'Critic Losses', 'cri_plot')):
        fig, ax = plt.subplots(1, 1)
        ax.set(xlabel=xlabel, ylabel='value')
        ax.plot(logs[key])
        fig.suptitle(title)
        fig.savefig(paths[name])
        plt.close(fig)
    fig, ax = plt.subplots(1, 1)
    ax.set(xlabel='rollout', ylabel='value')
    ax.plot(epi['trunc'], color='blue', label='truncated')
    ax.plot(epi['col'], color='red', label='collisions')
    ax.plot(epi['tar'], color='green', label='target reached')
    ax.legend()
    fig.suptitle('Episode endings')
    fig.savefig(paths['epi_plot'])
    plt.close(fig)
    written += [paths[k] for k in ('rew_plot', 'act_plot', 'cri_plot', 'epi_plot')]
    if diag:
        fig, ax = plt.subplots(1, 1)
        ax.set(xlabel='batch_num', ylabel='value')
        ax.plot(logs['actor_approx_kl'])
        fig.suptitle('Actor approximate KL')
        fig.savefig(paths['act_kl_plot'])
        plt.close(fig)
        written.append(paths['act_kl_plot'])
    return written


def train_phase(ppo, buffer, adam, network, num_epochs, batch_size, out=None, max_grad_norm=None,
                norm_out=None, target_kl=None, diag_out=None, stop_out=None, shuffle=None):
    """One whole ``train_actor`` (``network='actor'``) or ``train_critic``
    (``'critic'``) of the reference (models.py:160-198) over ``buffer`` as ONE
    C call, libmarlnav.so ``marlnav_ppo_train_phase``: ``num_epochs`` times
    the minibatches of ``minibatch_bounds(len(buffer), batch_size)``, an
    update's Adam step folded into the gradient kernels' finish launch where
    that was measured to be faster.
    Bit for bit what ``rollout.train_actor`` / ``train_critic`` leave with the
    same ``FusedAdam``: losses, ``.grad``, parameters, moments, step count.

    ``ppo``: a ``FusedPPO``; ``adam``: a ``FusedAdam`` over exactly that
    network's parameters in ``_POLICY_PARAMS`` order (the library refuses any
    other table). ``out``: a contiguous float64 device tensor of
    ``num_epochs * len(bounds)`` elements for the losses in update order
    (allocated where None); returned. Nothing synchronises.

    ``max_grad_norm`` (None: the above, bit for bit): every update clips its
    gradient by the global L2 norm before its Adam step, one
    ``marlnav_ppo_train_phase_clipped``: each update is the gradient launches
    and the clipped step's three (an actor of up to 1024 elements: two
    launches, the norm formed inside the finish launch) and stores the bits of
    ``ppo.actor_update(..., max_grad_norm=...)`` / ``critic_update``.
    ``norm_out``: None or a contiguous float64 device tensor like ``out`` for
    the norms before clipping, in update order.

    ``target_kl`` / ``diag_out`` (both None: the above, bit for bit), the
    actor only (one ``marlnav_ppo_train_phase_monitored``):
    every update writes a row of 5 doubles, ``[surrogate mean, entropy mean,
    approximate KL, clip fraction, status]``, to ``diag_out`` (a contiguous
    float64 device tensor of ``num_epochs * len(bounds)`` rows, allocated
    where None) and the first update whose approximate KL exceeds
    ``target_kl`` (or is NaN) abandons the phase on the device: that update
    (status 1) stores its loss, row and ``.grad`` and takes no Adam step, the
    updates behind it (status 2) cost their launches only and log NaN.
    ``stop_out``: a contiguous int64 device tensor of 2 elements (allocated
    where None) that receives ``[flag, stopped_at]``, reset by the call's
    first launch; ``stopped_at`` is -1 where the phase ran to its end. The
    comparison is with ``target_kl`` itself: for Stable-Baselines3's rule pass
    1.5 times its value. ``diag_out`` alone monitors only (``target_kl =
    inf``): no update stops, and losses, ``.grad``, parameters, moments and
    the count carry the bits of the unmonitored call. Composes with
    ``max_grad_norm`` and both advantage modes. The rows and the cell are kept
    as ``ppo.last_diag`` / ``ppo.last_stop``. ``network='critic'`` with any of
    the three is a ValueError.

    ``shuffle`` (None: the above, bit for bit): an int seed selects the
    shuffled mode (one ``marlnav_ppo_train_phase_shuffled``).
    One launch draws a fresh uniform permutation of ALL ``len(buffer)`` stored
    steps per epoch, on the device; minibatch j of an epoch is entries ``[j
    batch_size, (j + 1) batch_size)`` of its permutation, the last one extended
    by the ``len(buffer) % batch_size`` left over
    (``rollout.shuffled_minibatch_sizes``), so every stored step, the final one
    included, is used exactly once per epoch. The number of updates and every
    log's layout stay as they are. The kernels gather the steps by address and
    copy nothing; an update is the gradient launches and ``FusedAdam.step``'s
    (this mode has no folded finish launches). The permutations are keyed by
    the seed, the network, the epoch and a call counter that lives on the
    device (one cell per network on ``ppo``, created zero at first use and
    advanced by the launch), so a captured graph draws new permutations at
    every replay. The table of the last call, ``(num_epochs, len(buffer))``
    int32 on the device, is ``ppo.last_steps['actor' | 'critic']``: with it
    ``rollout.train_actor`` / ``train_critic(..., steps_table=...)`` repeat
    the phase bit for bit. Composes with ``max_grad_norm``, ``target_kl`` /
    ``diag_out`` and both advantage modes. At most 65 535 stored steps and
    epochs."""
    nets = {'actor': abi.NETWORK_ACTOR, 'critic': abi.NETWORK_CRITIC,
            abi.NETWORK_ACTOR: abi.NETWORK_ACTOR, abi.NETWORK_CRITIC: abi.NETWORK_CRITIC}
    if network not in nets:
        raise ValueError(f"network must be 'actor' or 'critic', got {network!r}")
    monitored = target_kl is not None or diag_out is not None or stop_out is not None
    if monitored:
        if nets[network] != abi.NETWORK_ACTOR:
            raise ValueError("target_kl / diag_out / stop_out monitor the actor phase: "
                             "network='critic' has no diagnostics")
        target_kl = float('inf') if target_kl is None else rollout.check_target_kl(target_kl)
    ppo._require(buffer)
    lib, dev = ppo._lib, ppo.device
    if shuffle is not None:
        if isinstance(shuffle, bool) or not isinstance(shuffle, int):
            raise ValueError(f"shuffle: need an int seed or None, got {shuffle!r}")
        bounds = shuffled_minibatch_sizes(len(buffer), batch_size)
        rollout.check_shuffle_len(len(buffer), num_epochs)
    else:
        bounds = minibatch_bounds(len(buffer), batch_size)
    B, E = len(bounds), int(num_epochs)
    if B < 1:
        raise ValueError(f"batch_size={batch_size} is greater than the {len(buffer)} stored "
                         "steps: no minibatch")
    if E < 1:
        raise ValueError(f"num_epochs={num_epochs} must be >= 1")
    if out is None:
        out = torch.empty(E * B, dtype=_F64, device=dev)
    if (out.dtype != _F64 or out.device != dev or out.numel() != E * B
            or not out.is_contiguous()):
        raise ValueError(f"out: need a contiguous float64 tensor of {E * B} elements on {dev}")
    if monitored:
        if diag_out is None:
            diag_out = torch.empty(E * B, abi.DIAG_ROW, dtype=_F64, device=dev)
        rollout.check_diag_out(diag_out, dev, rows=E * B)
        if stop_out is None:
            stop_out = torch.empty(2, dtype=torch.int64, device=dev)
        if (not torch.is_tensor(stop_out) or stop_out.dtype != torch.int64
                or stop_out.device != dev or stop_out.numel() != 2
                or not stop_out.is_contiguous()):
            raise ValueError(f"stop_out: need a contiguous int64 tensor of 2 elements on {dev}")
    # step 0 of the storage, dims of the whole buffer
    name = 'actor' if nets[network] == abi.NETWORK_ACTOR else 'critic'
    ppo._bind(buffer, 0, len(buffer), name)
    d, b = ppo._dims, ppo._bufs
    if shuffle is not None:
        schedule = (int(batch_size), E)
        need = lib.marlnav_ppo_train_shuffled_work_size(ctypes.byref(d), int(batch_size),
                                                        1 if monitored else 0)
    else:
        schedule = ((ctypes.c_int64 * (2 * B))(*[x for lo_hi in bounds for x in lo_hi]), B, E)
        size = (lib.marlnav_ppo_train_diag_work_size if monitored
                else lib.marlnav_ppo_train_work_size)
        need = size(ctypes.byref(d), *schedule[:2])
    ppo._grow_work(need=need)
    if shuffle is not None:
        # the call counter and the table live on ppo: a captured graph keeps their pointers
        L = int(d.num_steps)
        if name not in ppo._shuffle_counter:
            ppo._shuffle_counter[name] = torch.zeros(1, dtype=torch.int64, device=dev)
        table = ppo.last_steps.get(name)
        if table is None or tuple(table.shape) != (E, L):
            table = torch.zeros(E, L, dtype=torch.int32, device=dev)
        ppo.last_steps[name] = table
        draw = (shuffle & 0xFFFFFFFFFFFFFFFF, ppo._shuffle_counter[name].data_ptr(),
                table.data_ptr())
    ad, ab = adam._bind()
    clip = adam._clip_args(max_grad_norm, norm_out, count=E * B)
    monitor = ((target_kl, diag_out.data_ptr(), stop_out.data_ptr()) if monitored
               else (0.0, None, None))
    head = (nets[network], ctypes.byref(d), ctypes.byref(b), *schedule, ppo.epsilon,
            ppo.ent_const, ctypes.byref(ad), ctypes.byref(ab), out.data_ptr(), ppo._mode)
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    if shuffle is not None:
        rc = lib.marlnav_ppo_train_phase_shuffled(*head, *clip, *monitor, *draw, stream)
    elif monitored:
        rc = lib.marlnav_ppo_train_phase_monitored(*head, *clip, *monitor, stream)
    elif max_grad_norm is not None:
        rc = lib.marlnav_ppo_train_phase_clipped(*head, *clip, stream)
    else:
        rc = lib.marlnav_ppo_train_phase_mode(*head, stream)
    abi.check(rc, lib)
    if monitored:
        ppo.last_diag, ppo.last_stop = diag_out, stop_out
    return out


class MAPPO(object):
    """The reference's ``MAPPO(params, env)`` (models.py:59-104) on the
    device. ``params`` is ``utils.set_model_params``'s dict; ``env`` a
    ``marlnav_amd.Env`` in native-RNG mode with its default init sampler.
    Refused at construction, as ``collect_fused`` refuses them at its call: a
    reference-RNG env or one with a user-assigned sampler, and an env with no
    normaliser / action scaler where ``params`` has none to attach
    (``params['normalizer']`` / ``params['scaler']`` are attached to an env
    that has none, as ``--evaluate`` does).

    ``params['gae_lambda']`` (absent or None: the reference's estimator, bit
    for bit) selects the GAE(lambda) advantage mode of DESIGN.md §15: every
    rollout is followed by the bootstrap value and the GAE scan, the actor
    trains on own-env advantages and the critic towards the value targets.
    The mean-reward log and the checkpoint rule still read the reference's
    returns, so they mean the same in both modes. A value outside [0, 1] is a
    ValueError.

    ``params['max_grad_norm']`` (absent or None: no clipping, today's
    behaviour bit for bit) clips every update's gradient by its global L2
    norm in both phases; the device logs then keep each
    update's norm before clipping and ``logs()`` gains ``actor_grad_norm`` /
    ``critic_grad_norm``. A value that is not > 0 is a ValueError.

    ``params['target_kl']`` (absent or None: today's behaviour) abandons the
    remaining actor updates of a rollout once an update's approximate KL
    divergence from the rollout policy exceeds it (decided on
    the device, ``repeat()`` still does not synchronise); the comparison is
    with the value itself, so pass 1.5 times Stable-Baselines3's ``target_kl``
    for its rule. A value that is not > 0 is a ValueError.
    ``params['log_diagnostics']`` (a bool) records the diagnostics without a
    stop. With either, ``logs()`` gains ``actor_approx_kl``,
    ``actor_clip_frac``, ``actor_entropy``, ``actor_surrogate`` and
    ``actor_status`` (one per update, laid out as the losses) and
    ``actor_stopped_at`` (one int per rollout, -1 where the phase ran to its
    end); the loss of an update behind a stop is NaN.

    ``params['shuffle_minibatches']`` (a bool; absent or False: today's
    behaviour bit for bit) trains both phases on fresh random minibatches
    (DESIGN.md §18): per epoch a new uniform permutation of all ``buffer_len``
    stored steps, drawn on the device and keyed by ``seed``, is cut into the
    ``buffer_len // batch_size`` minibatches, the last one taking the steps
    left over, so the buffer's final step, which the reference's slices drop,
    is trained on. The logs keep their layout; ``repeat()`` still does not
    synchronise. The last tables are ``self.ppo.last_steps``.

    ``seed`` keys the policy kernel's normals (``FusedPolicy``); the modules'
    initial weights come from torch's global generator, as the reference's do.

    The checkpoint rule and its quirk. The reference saves both state dicts
    after a rollout whose mean reward exceeds ``_max_rew`` (models.py:127-129)
    and never updates ``_max_rew`` from ``-inf``: it saves after EVERY rollout
    whose mean is not NaN, and since the save happens in ``get_data``, before
    that repeat's training, the files left by a run hold the weights from
    before the last repeat's training. ``track_best=False`` (the default)
    reproduces exactly that; ``track_best=True`` keeps the maximum, so the
    files hold the weights that produced the best rollout. Here the save is a
    device-side copy into a snapshot allocation (``marlnav_params_snapshot_if``)
    and ``save_weights()`` writes that snapshot to the reference's two files.

    ``out_dir``: where ``weights/``, ``plots/`` and ``logs/`` are created
    (the reference uses the working directory), at the first write."""

    def __init__(self, params, env, seed=0, track_best=False, out_dir='.'):
        who = "MAPPO"
        # the advantage mode, before anything touches the env
        self.gae_lambda = params.get('gae_lambda')
        if self.gae_lambda is not None:
            self.gae_lambda = rollout._check_lambda(self.gae_lambda)
        self.max_grad_norm = params.get('max_grad_norm')
        if self.max_grad_norm is not None:
            self.max_grad_norm = rollout.check_max_grad_norm(self.max_grad_norm)
        self.target_kl = params.get('target_kl')
        if self.target_kl is not None:
            self.target_kl = rollout.check_target_kl(self.target_kl)
        self.log_diagnostics = bool(params.get('log_diagnostics'))
        self._monitored = self.target_kl is not None or self.log_diagnostics
        self.shuffle_minibatches = bool(params.get('shuffle_minibatches'))
        self._seed = int(seed)
        if env._rng != 'native' or env._init_sampler is not env._default_init_sampler:
            raise RuntimeError(f"{who} needs an env in native-RNG mode with its default init "
                               "sampler: a reference-RNG or user-assigned sampler is called on "
                               "the host every step")
        if env._normalizer is None and params.get('normalizer') is not None:
            env.attach_normalizer(ObsNormalizer(params['normalizer']))
        if env._action_scaler is None and params.get('scaler') is not None:
            env.attach_action_scaler(ActionScaler(params['scaler']))
        if env._normalizer is None or env._action_scaler is None:
            raise RuntimeError(f"{who} needs an observation normaliser and an action scaler: "
                               "params['normalizer'] / params['scaler'], or "
                               "env.attach_normalizer(...) / env.attach_action_scaler(...)")
        # the env's C parameters now (the action scaler's two tensors are read
        # back once): the first repeat() then has nothing left that synchronises
        env._sync_params()
        self.num_agents = params['num_agents']
        self.num_parallel = params['num_parallel']
        self.action_size = params['action_size']
        self.device = torch.device(env.device)
        if self.device.type != 'cuda':
            raise RuntimeError(f"{who} runs on a HIP device (no CPU fallback); the env is on "
                               f"{self.device}")
        self.env = env
        self.actor = Actor(**params['actor']).to(self.device)
        self.critic = Critic(**params['critic']).to(self.device)
        self.actor_optimizer = FusedAdam(self.actor.parameters(), lr=params['lr'], maximize=True)
        self.critic_optimizer = FusedAdam(self.critic.parameters(), lr=params['lr'],
                                          maximize=False)
        self.ent_const = params['ent_const']
        self.epsilon = params['epsilon']
        self.gamma = params['gamma']
        self.buffer_len = int(params['buffer_len'])
        self.num_epochs = int(params['num_epochs'])
        self.batch_size = int(params['batch_size'])
        if self.num_epochs < 1:
            raise ValueError(f"num_epochs={self.num_epochs} must be >= 1")
        if self.shuffle_minibatches:    # as many updates; every stored step in some minibatch
            self._bounds = shuffled_minibatch_sizes(self.buffer_len, self.batch_size)
            rollout.check_shuffle_len(self.buffer_len, self.num_epochs)
        else:
            self._bounds = minibatch_bounds(self.buffer_len, self.batch_size)
        if not self._bounds:
            raise ValueError(f"batch_size={self.batch_size} is greater than "
                             f"buffer_len={self.buffer_len}: no minibatch")
        self.buffer = RolloutBuffer(self.buffer_len)
        self.policy = FusedPolicy(self.actor, self.critic, seed=seed)
        self.ppo = FusedPPO(self.actor, self.critic, self.epsilon, self.ent_const,
                            advantage='reference' if self.gae_lambda is None else 'gae')
        self.track_best = bool(track_best)
        self.out_dir = out_dir
        self._time = datetime.now().strftime('%Y%m%d%H%M%S')
        paths = stats_paths(out_dir, self._time)
        self._actor_path, self._critic_path = paths['actor'], paths['critic']
        self._lib = abi.load_library()
        dev = self.device
        self._mean_rew = None
        self._max_rew = torch.full((1,), float('-inf'), dtype=_F64, device=dev)
        self._save_state = torch.tensor([0, -1], dtype=torch.int64, device=dev)
        # the snapshot of the ten parameters: one flat allocation, segments on 16 bytes
        self._live = [t for _, t in self.policy._params]
        offs, at = [], 0
        for t in self._live:
            offs.append(at)
            at += (t.numel() + 3) // 4 * 4
        self._snap_flat = torch.zeros(at, dtype=torch.float32, device=dev)
        self._snapshot = [self._snap_flat[o:o + t.numel()].view(t.shape)
                          for o, t in zip(offs, self._live)]
        n = len(self._live)
        self._snap_src = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self._live])
        self._snap_dst = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self._snapshot])
        self._snap_numel = (ctypes.c_int64 * n)(*[t.numel() for t in self._live])
        self._r = 0                         # rollouts collected
        total = params.get('num_total')
        self._cap = 0
        self._mean_log = self._epi_log = self._actor_log = self._critic_log = None
        self._actor_norm_log = self._critic_norm_log = None    # with max_grad_norm only
        self._diag_log = self._stop_log = None    # with target_kl / log_diagnostics only
        self._reserve(max(1, int(total) // (self.buffer_len * self.num_parallel)) if total else 1)
        self._logs = _empty_logs()

    # ------------------------------------------------------------- the logs
    def _reserve(self, repeats):
        """Device logs for ``repeats`` rollouts: rows are kept when they grow
        (a device copy, nothing synchronises)."""
        if repeats <= self._cap:
            return
        cap = max(repeats, 2 * self._cap)
        U = self.num_epochs * len(self._bounds)
        new = (torch.zeros(cap, dtype=_F64, device=self.device),
               torch.zeros(cap, 3, dtype=torch.int64, device=self.device),
               torch.zeros(cap, U, dtype=_F64, device=self.device),
               torch.zeros(cap, U, dtype=_F64, device=self.device))
        old = (self._mean_log, self._epi_log, self._actor_log, self._critic_log)
        if self.max_grad_norm is not None:
            new += (torch.zeros(cap, U, dtype=_F64, device=self.device),
                    torch.zeros(cap, U, dtype=_F64, device=self.device))
            old += (self._actor_norm_log, self._critic_norm_log)
        if self._monitored:
            new += (torch.zeros(cap, U, abi.DIAG_ROW, dtype=_F64, device=self.device),
                    torch.zeros(cap, 2, dtype=torch.int64, device=self.device))
            new[-1][:, 1] = -1      # a rollout that was not trained on never stopped
            old += (self._diag_log, self._stop_log)
        if self._cap:
            for n, o in zip(new, old):
                n[:self._cap].copy_(o)
        self._mean_log, self._epi_log, self._actor_log, self._critic_log = new[:4]
        if self.max_grad_norm is not None:
            self._actor_norm_log, self._critic_norm_log = new[4:6]
        if self._monitored:
            self._diag_log, self._stop_log = new[-2:]
        self._cap = cap

    def logs(self):
        """The reference's ``_logs`` layout (models.py:95-104) with Python
        numbers, for the rollouts collected so far: ``epi_stats`` (``trunc`` /
        ``col`` / ``tar``, one int per rollout), ``mean_rews`` (one float per
        rollout), ``actor`` / ``critic`` (one loss per update, in order; a
        rollout that was not trained on contributes zeros); with
        ``max_grad_norm`` also ``actor_grad_norm`` / ``critic_grad_norm``, each
        update's gradient norm before clipping, laid out as the losses; with
        ``target_kl`` / ``log_diagnostics`` also ``actor_surrogate``,
        ``actor_entropy``, ``actor_approx_kl``, ``actor_clip_frac`` and
        ``actor_status`` (0 applied, 1 the update that raised the stop, 2
        behind it), laid out as the losses, and ``actor_stopped_at``, one int
        per rollout (-1: the phase ran to its end).
        Synchronises once:
        the device logs travel as one float64 tensor (the counters are exact
        below 2^53). Also kept as ``self._logs``."""
        r = self._r
        U = self._actor_log.shape[1]
        clip = self.max_grad_norm is not None
        norms = [self._actor_norm_log[:r].flatten(),
                 self._critic_norm_log[:r].flatten()] if clip else []
        mon = self._monitored
        diag = [self._diag_log[:r].flatten(), self._stop_log[:r].to(_F64).flatten()] if mon else []
        flat = torch.cat([self._mean_log[:r], self._epi_log[:r].to(_F64).flatten(),
                          self._actor_log[:r].flatten(), self._critic_log[:r].flatten(),
                          self._save_state.to(_F64)] + norms + diag).cpu()
        mean, epi, act, cri, save, *rest = torch.split(
            flat, [r, 3 * r, r * U, r * U, 2] + [r * U] * len(norms)
            + ([r * U * abi.DIAG_ROW, 2 * r] if mon else []))
        norms = rest[:len(norms)]
        epi = epi.view(r, 3).to(torch.int64).tolist()
        self._saves = (int(save[0]), int(save[1]))
        self._logs = {'epi_stats': {'trunc': [e[0] for e in epi], 'col': [e[1] for e in epi],
                                    'tar': [e[2] for e in epi]},
                      'mean_rews': mean.tolist(), 'actor': act.tolist(), 'critic': cri.tolist()}
        if clip:
            self._logs['actor_grad_norm'] = norms[0].tolist()
            self._logs['critic_grad_norm'] = norms[1].tolist()
        if mon:
            rows = rest[-2].view(r * U, abi.DIAG_ROW)
            for i, key in enumerate(('actor_surrogate', 'actor_entropy', 'actor_approx_kl',
                                     'actor_clip_frac')):
                self._logs[key] = rows[:, i].tolist()
            self._logs['actor_status'] = [int(x) for x in rows[:, 4].tolist()]
            self._logs['actor_stopped_at'] = [int(x) for x in rest[-1].view(r, 2)[:, 1].tolist()]
        return self._logs

    def save_count(self):
        """(number of snapshots taken, repeat index of the last one or -1).
        Synchronises."""
        s = self._save_state.tolist()
        return int(s[0]), int(s[1])

    # ----------------------------------------------------------- the phases
    def _stream(self):
        return torch._C._cuda_getCurrentRawStream(self.device.index)

    def get_data(self):
        """models.py:106-129: one rollout of ``buffer_len`` steps into
        ``buffer`` (``collect_fused``'s one C call), its mean reward into row
        r of the device log, the three episode counters' totals into row r of
        theirs and the counters zeroed (models.py:151-158), then the
        checkpoint rule (the class docstring). Nothing synchronises and
        nothing is printed."""
        r = self._r
        self._reserve(r + 1)
        env, lib = self.env, self._lib
        mean, _ = rollout._collect_fused_enqueue(env, self.policy, self.buffer, gamma=self.gamma,
                                                 gae_lambda=self.gae_lambda)
        self._mean_rew = mean
        self._mean_log[r].copy_(mean)
        abi.check(lib.marlnav_counters_total(ctypes.byref(env._dims), env._counters.data_ptr(),
                                             self._epi_log[r].data_ptr(), self._stream()), lib)
        env._counters.zero_()
        abi.check(lib.marlnav_params_snapshot_if(
            len(self._live), self._snap_src, self._snap_dst, self._snap_numel,
            self._mean_log[r].data_ptr(), self._max_rew.data_ptr(), self._save_state.data_ptr(),
            r, 1 if self.track_best else 0, self._stream()), lib)
        self._r = r + 1

    def _phase(self, network, adam, log, norm_log):
        if self._r < 1:
            raise RuntimeError("no rollout to train on yet: call get_data() first")
        r = self._r - 1
        monitor = {}
        if self._monitored and network == abi.NETWORK_ACTOR:
            monitor = dict(target_kl=self.target_kl, diag_out=self._diag_log[r],
                           stop_out=self._stop_log[r])
        train_phase(self.ppo, self.buffer, adam, network, self.num_epochs, self.batch_size,
                    out=log[r], max_grad_norm=self.max_grad_norm,
                    norm_out=None if norm_log is None else norm_log[r],
                    shuffle=self._seed if self.shuffle_minibatches else None, **monitor)

    def train_actor(self):
        """models.py:160-178 for the last rollout as ONE C call
        (``marlnav_ppo_train_phase``): ``num_epochs`` times the minibatches of
        ``minibatch_bounds(buffer_len, batch_size)``, each update's loss into
        the device log. Nothing is printed and nothing synchronises."""
        self._phase(abi.NETWORK_ACTOR, self.actor_optimizer, self._actor_log,
                    self._actor_norm_log)

    def train_critic(self):
        """models.py:180-198, as ``train_actor``."""
        self._phase(abi.NETWORK_CRITIC, self.critic_optimizer, self._critic_log,
                    self._critic_norm_log)

    def repeat(self):
        """One pass of the reference's loop body (__main__.py:25-27):
        ``get_data``, ``train_actor``, ``train_critic``; no host
        synchronisation from entry to return."""
        self.get_data()
        self.train_actor()
        self.train_critic()

    def run(self, num_repeats, save_every=None):
        """``num_repeats`` repeats; ``save_weights()`` at the end and, with
        ``save_every=N``, after every N-th repeat. Returns the two paths (or
        None where no snapshot was ever taken)."""
        num_repeats = int(num_repeats)
        self._reserve(self._r + num_repeats)
        for i in range(num_repeats):
            self.repeat()
            if save_every and (i + 1) % int(save_every) == 0 and i + 1 < num_repeats:
                self.save_weights()
        return self.save_weights()

    # ------------------------------------------------------------ the files
    def snapshot_state_dicts(self):
        """The snapshot as the two state dicts with the reference's keys (CPU
        copies)."""
        cpu = [t.detach().cpu().clone() for t in self._snapshot]
        return dict(zip(ACTOR_KEYS, cpu[:6])), dict(zip(CRITIC_KEYS, cpu[6:]))

    def save_weights(self):
        """Write the snapshot as ``weights/<time>_actor.pt`` and
        ``_critic.pt`` (state dicts with the reference's keys, as models.py:
        128-129 saves them) -> (actor path, critic path); None, with nothing
        written, where no snapshot was taken yet (the reference has no files
        then either). With ``track_best=False`` the files hold the weights
        from BEFORE the last repeat's training, as the reference's do at the
        same moment (the class docstring). Synchronises."""
        if self.save_count()[0] < 1:
            return None
        actor, critic = self.snapshot_state_dicts()
        os.makedirs(os.path.dirname(self._actor_path), exist_ok=True)
        torch.save(actor, self._actor_path)
        torch.save(critic, self._critic_path)
        return self._actor_path, self._critic_path

    def save_stats(self, full_params, plot=True):
        """models.py:200-268: ``write_stats`` of ``logs()``."""
        return write_stats(self.logs(), full_params, self.out_dir, self._time, plot=plot)
