"""The device training mode on the GPU: ``marlnav_ppo_train_phase`` (through
``training.train_phase`` and ``MAPPO.train_actor`` / ``train_critic``),
``marlnav_params_snapshot_if`` and the ``MAPPO`` trainer with ``--train``.

Every comparison is for equal bits, derived and not measured: the phase call
launches the gradient kernels of ``marlnav_ppo_*_update`` (fixed reduction
orders, no atomics) and its folded finish kernels restate ``adam_apply``'s
element update through the one shared definition (csrc/adam_element.h), from
the fp32 gradient they have just stored; the snapshot is a copy; the trainer
enqueues what the hand-assembled loop enqueues. So no tolerance appears below.

The shape cases run the whole-buffer call at function level
(``training.train_phase``, which is all ``MAPPO.train_actor`` calls); the
3 x 3 cases and every bounds case also go through a ``MAPPO`` object."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import ppo_ref as pp
import test_adam_gpu as tad
import test_ppo_gpu as tg
import test_rollout_gpu as tr
from conftest import cli_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = tad.LR
SENTINEL = tad.SENTINEL


def bits64(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def losses(t):
    return tg.np_(t).reshape(-1).copy()


# one case per shape, computed once and shared (T + 1 steps, so that the one
# minibatch of batch_size T is T x P rows: the last batch loses the final step)
_cases = {}


def case(T, P, A, O, H, seed):
    key = (T, P, A, O, H, seed)
    if key not in _cases:
        _cases[key] = tg.make_case(T, P, A, O, H, seed)
    return _cases[key]


def run_loops(pkg, w, data, epochs, batch, maximize=(True, False)):
    """The existing path: rollout.train_actor / train_critic with FusedAdam."""
    ppo, buf, par, adams = setup(pkg, w, data, maximize)
    logs = {"actor": [], "critic": []}
    pkg.train_actor(ppo, buf, adams["actor"], epochs, batch, log=logs["actor"])
    pkg.train_critic(ppo, buf, adams["critic"], epochs, batch, log=logs["critic"])
    out = {k: np.array([float(x) for x in v]) for k, v in logs.items()}
    return out, tad.full_state(par, adams)


def setup(pkg, w, data, maximize=(True, False)):
    ppo, buf, par = tg.fused(pkg, w, data)
    adams = {"actor": tad.fused_adam(pkg, [par[k] for k in pp.ACTOR_PARAMS], maximize[0]),
             "critic": tad.fused_adam(pkg, [par[k] for k in pp.CRITIC_PARAMS], maximize[1])}
    return ppo, buf, par, adams


def run_phase(pkg, w, data, epochs, batch, maximize=(True, False)):
    """The new path at function level: one C call per network."""
    ppo, buf, par, adams = setup(pkg, w, data, maximize)
    out = {k: losses(pkg.training.train_phase(ppo, buf, adams[k], k, epochs, batch))
           for k in ("actor", "critic")}
    return out, tad.full_state(par, adams)


def make_mappo(pkg, P, A, O, H, buffer_len, batch_size, epochs, repeats=2, seed=21,
               weight_seed=11, **kw):
    """A MAPPO over test_rollout_gpu's staggered env (episodes of 2 steps)."""
    args = cli_args(num_parallel=P, num_agents=A, num_obstacles=O, episode_len=2,
                    risk_factor=2.0, distance_factor=3.0, hidden_size=H, buffer_len=buffer_len,
                    batch_size=batch_size, num_epochs=epochs, learning_rate=LR,
                    num_total=repeats * buffer_len * P)
    env = tr.make_env(pkg, P, A, O, seed=seed, normalizer=False, scaler=False)
    torch.manual_seed(weight_seed)
    return pkg.MAPPO(pkg.set_model_params(args, DEV), env, seed=5, **kw), args


def run_mappo_phase(pkg, w, data, epochs, batch, P, A, O, H):
    """The new path through a MAPPO object: its modules take the case's
    weights in place, its buffer is the case's."""
    m, _ = make_mappo(pkg, P, A, O, H, data["returns"].shape[0], batch, epochs)
    mods = {"actor": m.actor, "critic": m.critic}
    par = {}
    with torch.no_grad():
        for k, v in w.items():
            net, layer, attr = k.split(".")
            p = getattr(getattr(mods[net], layer), attr)
            p.copy_(v.to(DEV))
            par[k] = p
    m.buffer = tg.buffer_of(pkg, data)
    m._r = 1                                  # as after one get_data()
    m.train_actor()
    m.train_critic()
    logs = m.logs()
    out = {k: np.array(logs[k]) for k in ("actor", "critic")}
    adams = {"actor": m.actor_optimizer, "critic": m.critic_optimizer}
    return out, tad.full_state(par, adams)


def assert_runs_equal(a, b, what):
    (la, sa), (lb, sb) = a, b
    for k in ("actor", "critic"):
        assert la[k].shape == lb[k].shape and la[k].size > 0, (what, k)
        assert np.array_equal(bits64(la[k]), bits64(lb[k])), (what, k, la[k], lb[k])
        assert np.isfinite(la[k]).all(), (what, k)
    tad.assert_same_bits(sa, sb)


# ------------------------------------------------ 1. the phase call, every path
# T x P of A x O with H (§10's paths), seed
PHASE_SHAPES = {
    "tiny": (2, 3, 3, 3, 50, 7),
    "fold_last": (2, 3, 3, 3, 60, 8),       # 1024 actor elements: the largest folded actor
    "fold_first_out": (2, 3, 3, 3, 61, 9),  # 1041: the actor keeps its own Adam launches
    "chunks": (4, 700, 3, 3, 50, 1621),     # 9 actor blocks, 44 critic chunks
    "wide": (2, 3, 16, 32, 7, 101),         # six column tiles, the critic's own forward launch
    "mid_row": (2, 16, 16, 48, 5, 303),
    "long_row": (2, 64, 2, 127, 3, 404),    # D + 1 > 256
    "fused64": (2, 40, 4, 13, 50, 2),       # critic_pass<64, kFused> with the count's advance
    "unit_groups64": (2, 40, 2, 31, 65, 1),  # folded critic_finish behind 2 forward unit groups
}
# the path of each, as test_ppo_gpu.PATHS (pinned by tests/test_ppo_cpu.py)
PHASE_PATHS = {
    "tiny": ("fused8", 1, 1, 1, 19, 1),
    "fold_last": ("split8", 1, 2, 1, 19, 1),
    "fold_first_out": ("split8", 1, 2, 1, 19, 1),
    "chunks": ("fused8", 1, 1, 1, 19, 1),
    "wide": ("split64", 6, 1, 1, 2, 1),
    "mid_row": ("split64", 8, 1, 1, 1, 1),
    "long_row": ("split64", 3, 1, 1, 1, 2),
    "fused64": ("fused64", 1, 1, 1, 7, 1),
    "unit_groups64": ("split64", 1, 2, 1, 3, 1),
}


@pytest.mark.parametrize("name", sorted(PHASE_SHAPES))
def test_phase_equals_the_existing_loops(pkg, name):
    T, P, A, O, H, seed = PHASE_SHAPES[name]
    w, data = case(T + 1, P, A, O, H, seed)
    assert pkg.minibatch_bounds(T + 1, T) == [(0, T)]
    epochs = 2
    want = run_loops(pkg, w, data, epochs, T)
    got = run_phase(pkg, w, data, epochs, T)
    assert_runs_equal(got, want, name)
    assert want[1]["actor count"] == want[1]["critic count"] == epochs
    for k in w:
        assert not np.array_equal(got[1][k], w[k].numpy()), f"{name}: {k} did not move"
    if (A, O) == (3, 3):
        assert_runs_equal(run_mappo_phase(pkg, w, data, epochs, T, P, A, O, H), want,
                          name + " through MAPPO")


def device_case(pkg, T, P, A, O, H, seed):
    """A case too large for policy_ref on the CPU: observations drawn on the
    device, old actions, log-probs and values from the policy kernel, then
    every parameter moved by 2% of its mean magnitude (as make_case does)."""
    w, _ = tg.make_case(1, 2, A, O, H, seed)
    actor, critic, _ = tg.modules(w)
    D = 2 + 2 * O + 2 * (A - 1)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    obs = torch.rand(T, P, A, D, device=DEV, generator=gen) * 2 - 1
    policy = pkg.FusedPolicy(actor, critic, seed=seed)
    old = [policy.act(obs[t]) for t in range(T)]
    data = {"obs": obs, "actions": torch.stack([o[0] for o in old]),
            "log_probs": torch.stack([o[1] for o in old]),
            "values": torch.stack([o[2] for o in old]),
            "returns": torch.randn(T, P, dtype=torch.float64, device=DEV, generator=gen)}
    cpu = torch.Generator().manual_seed(seed)
    w = {k: v + 0.02 * v.abs().mean() * torch.randn(v.shape, generator=cpu) for k, v in w.items()}
    return w, data


@pytest.mark.parametrize("P", [1 << 17, (1 << 17) + 1])
def test_phase_on_both_sides_of_the_critic_fold_limit(pkg, P):
    """One step of 2^17 envs is the largest minibatch whose critic update is
    folded; one env more and the critic keeps its own Adam launches."""
    w, data = device_case(pkg, 2, P, 3, 3, 5, 31)
    assert pkg.minibatch_bounds(2, 2) == [(0, 1)]
    want = run_loops(pkg, w, data, 2, 2)
    assert_runs_equal(run_phase(pkg, w, data, 2, 2), want, str(P))
    assert want[1]["critic count"] == 2


@pytest.mark.parametrize("buffer_len,batch_size", [(7, 3), (6, 3), (4, 4), (8, 2)])
def test_phase_bounds_lose_the_final_step_where_the_reference_does(pkg, buffer_len, batch_size):
    bounds = pkg.minibatch_bounds(buffer_len, batch_size)
    assert bounds == {(7, 3): [(0, 3), (3, 6)], (6, 3): [(0, 3), (3, 5)], (4, 4): [(0, 3)],
                      (8, 2): [(0, 2), (2, 4), (4, 6), (6, 7)]}[(buffer_len, batch_size)]
    P, A, O, H = 3, 3, 3, 50
    w, data = case(buffer_len, P, A, O, H, 77)
    want = run_loops(pkg, w, data, 2, batch_size)
    assert want[0]["actor"].size == 2 * len(bounds)
    assert_runs_equal(run_phase(pkg, w, data, 2, batch_size), want, "function")
    assert_runs_equal(run_mappo_phase(pkg, w, data, 2, batch_size, P, A, O, H), want, "MAPPO")


# --------------------------------------------- 2. the folded update at its edges
H5 = (2, 3, 3, 3, 5, 55)                # tensors of 1, 2, 5, 10, 60 and 180 elements


@pytest.mark.parametrize("maximize", [(True, False), (False, True)])
def test_two_consecutive_folded_updates_with_short_tensors(pkg, maximize):
    """Two updates in one call: the second runs on k = 2's bias corrections.
    H = 5: every tensor is shorter than a block, most shorter than a wave."""
    T, P, A, O, H, seed = H5
    w, data = case(T + 1, P, A, O, H, seed)
    sizes = sorted({v.numel() for v in w.values()})
    assert sizes == [1, 2, 5, 10, 60, 180]
    want = run_loops(pkg, w, data, 2, T, maximize)
    got = run_phase(pkg, w, data, 2, T, maximize)
    assert_runs_equal(got, want, str(maximize))
    assert got[1]["actor count"] == 2 and got[1]["critic count"] == 2
    # the other sign of the gradient: the parameters moved the other way
    other = run_phase(pkg, w, data, 2, T, (not maximize[0], not maximize[1]))
    for k in w:
        assert not np.array_equal(other[1][k], got[1][k]), k


def raw_phase(pkg, which, w, data, epochs, offset, maximize):
    """``marlnav_ppo_train_phase`` through ctypes with every parameter, grad
    and moment tensor of the network a view at ``offset`` elements inside a
    sentinel-filled buffer (test_adam_gpu.py's method). -> (losses, {name:
    (param, grad, exp_avg, exp_avg_sq)} as numpy, count, buffers)."""
    abi = pkg.abi
    lib = abi.load_library()
    T, P = data["returns"].shape
    A, D = data["obs"].shape[2:]
    names = pp.ACTOR_PARAMS if which == "actor" else pp.CRITIC_PARAMS
    H = w["actor.fc1.weight"].shape[0]
    d = abi.MarlnavPpoDims(num_parallel=P, num_steps=T, num_agents=A, obs_dim=D, hidden_size=H)
    b = abi.MarlnavPpoBuffers()
    dev = {k: v.to(DEV).contiguous() for k, v in data.items()}
    for f in abi.PPO_DATA_FIELDS:
        setattr(b, f, dev[f].data_ptr())
    ad = abi.MarlnavAdamDims(num_tensors=len(names), maximize=int(maximize), lr=LR,
                             beta1=tad.BETAS[0], beta2=tad.BETAS[1], eps=tad.EPS)
    state = torch.zeros(int(lib.marlnav_adam_state_size()) // 8, dtype=torch.int64, device=DEV)
    ab = abi.MarlnavAdamBuffers(state=state.data_ptr())
    quads, bufs = {}, []
    fields = [f for f in abi.POLICY_WEIGHT_FIELDS if f.startswith(which)]
    for i, (k, f) in enumerate(zip(names, fields)):
        quad = []
        for src in (w[k], torch.zeros_like(w[k]), torch.zeros_like(w[k]), torch.zeros_like(w[k])):
            view, buf = tad.sentinel_view(src, offset=offset)
            assert (view.data_ptr() % 16 != 0) == (offset % 4 != 0)
            quad.append(view)
            bufs.append((view, buf))
        quads[k] = quad
        ad.numel[i] = w[k].numel()
        for af, t in zip(abi.ADAM_POINTER_FIELDS, quad):
            getattr(ab, af)[i] = t.data_ptr()
        setattr(b, f, quad[0].data_ptr())
        setattr(b, "grad_" + f, quad[1].data_ptr())
    bounds = pkg.minibatch_bounds(T, T - 1)
    arr = (ctypes.c_int64 * (2 * len(bounds)))(*[x for p in bounds for x in p])
    need = lib.marlnav_ppo_train_work_size(ctypes.byref(d), arr, len(bounds))
    assert need > 0
    work = torch.empty(need, dtype=torch.float64, device=DEV)
    b.work = work.data_ptr()
    log = torch.full((epochs * len(bounds),), math.nan, dtype=torch.float64, device=DEV)
    abi.check(lib.marlnav_ppo_train_phase(
        0 if which == "actor" else 1, ctypes.byref(d), ctypes.byref(b), arr, len(bounds), epochs,
        tg.EPSILON, tg.ENT_CONST, ctypes.byref(ad), ctypes.byref(ab), log.data_ptr(),
        torch.cuda.current_stream().cuda_stream), lib)
    torch.cuda.synchronize()
    out = {k: tuple(tg.np_(t).copy() for t in q) for k, q in quads.items()}
    return losses(log), out, int(state[0]), bufs


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_offset_tensors_stay_in_bounds_and_match_the_aligned_run(pkg, which):
    T, P, A, O, H, seed = H5
    w, data = case(T + 1, P, A, O, H, seed)
    maximize = which == "actor"
    l0, aligned, n0, bufs0 = raw_phase(pkg, which, w, data, 2, 4, maximize)
    l1, shifted, n1, bufs1 = raw_phase(pkg, which, w, data, 2, 1, maximize)
    assert n0 == n1 == 2
    assert np.array_equal(bits64(l0), bits64(l1)) and np.isfinite(l0).all()
    for view, buf in bufs0 + bufs1:
        off = view.storage_offset()
        outside = torch.cat([buf[:off], buf[off + view.numel():]])
        assert bool((outside == SENTINEL).all()), "a sentinel was overwritten"
    for k in aligned:
        for j, what in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):
            assert np.array_equal(tad.bits(aligned[k][j]), tad.bits(shifted[k][j])), (k, what)
        assert not np.array_equal(aligned[k][0], w[k].numpy().reshape(-1)), k
    # and the aligned raw run is the existing path's
    want = run_loops(pkg, w, data, 2, T)
    assert np.array_equal(bits64(l0), bits64(want[0][which]))
    for k in aligned:
        assert np.array_equal(tad.bits(aligned[k][0]), tad.bits(want[1][k].reshape(-1))), k
        assert np.array_equal(tad.bits(aligned[k][1]), tad.bits(want[1]["grad " + k].reshape(-1))), k


def test_a_zero_gradient_moves_nothing(pkg):
    """Actor: advantages 0 (returns == values) and ent_const 0. Critic: a dead
    first layer, so the new value is fc2's bias, which values and returns
    equal. Every gradient element is then +-0: p keeps its bits, m and v stay
    0, and the count still advances."""
    T, P, A, O, H, seed = H5
    w, data = case(T + 1, P, A, O, H, seed)
    w, data = dict(w), dict(data)
    w["critic.fc1.weight"] = torch.zeros_like(w["critic.fc1.weight"])
    w["critic.fc1.bias"] = torch.zeros_like(w["critic.fc1.bias"])
    data["values"] = torch.full_like(data["values"], float(w["critic.fc2.bias"][0]))
    data["returns"] = data["values"].reshape(data["returns"].shape).double()
    actor, critic, par = tg.modules(w)
    ppo = pkg.FusedPPO(actor, critic, tg.EPSILON, 0.0)
    buf = tg.buffer_of(pkg, data)
    adams = {"actor": tad.fused_adam(pkg, [par[k] for k in pp.ACTOR_PARAMS], True),
             "critic": tad.fused_adam(pkg, [par[k] for k in pp.CRITIC_PARAMS], False)}
    for k in ("actor", "critic"):
        pkg.training.train_phase(ppo, buf, adams[k], k, 2, T)
    state = tad.full_state(par, adams)
    for k, v in w.items():
        assert not np.any(state["grad " + k]), k
        assert np.array_equal(tad.bits(state[k]), tad.bits(v.numpy())), k
    for k, v in state.items():
        if "exp_avg" in k:
            assert not np.any(v), k
    assert state["actor count"] == 2 and state["critic count"] == 2


def test_a_captured_phase_replays_as_the_eager_phases(pkg):
    T, P, A, O, H, seed = PHASE_SHAPES["tiny"]
    w, data = case(T + 1, P, A, O, H, seed)

    def phases(s, out):
        ppo, buf, par, adams = s
        for k in ("actor", "critic"):
            pkg.training.train_phase(ppo, buf, adams[k], k, 1, T, out=out[k])

    new_out = lambda: {k: torch.zeros(1, dtype=torch.float64, device=DEV)
                       for k in ("actor", "critic")}
    eager, eager_out = setup(pkg, w, data), new_out()
    for _ in range(2):
        phases(eager, eager_out)
    cap, cap_out = setup(pkg, w, data), new_out()
    ppo, buf, par, adams = cap
    start = {k: p.detach().clone() for k, p in par.items()}
    start_sd = {k: a.state_dict() for k, a in adams.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        phases(cap, cap_out)                         # warm-up: workspace, code objects
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for k, p in par.items():
            p.copy_(start[k])
    for k, a in adams.items():
        a.load_state_dict(start_sd[k])
        assert a.step_count() == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        phases(cap, cap_out)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a in list(adams.values()) + list(eager[3].values()):
        assert a.step_count() == 2
    tad.assert_same_bits(tad.full_state(cap[2], cap[3]), tad.full_state(eager[2], eager[3]))
    for k in cap_out:
        assert np.array_equal(bits64(losses(cap_out[k])), bits64(losses(eager_out[k]))), k


# ------------------------------------------------------------- 3. the snapshot
SNAP_SHAPES = [(5, 12), (5,), (2, 5), (2,), (2, 5), (2,), (5, 36), (5,), (1, 5), (1,)]


@pytest.mark.parametrize("offset", [4, 1])
@pytest.mark.parametrize("track_best", [0, 1])
def test_snapshot_copies_only_above_the_maximum(pkg, offset, track_best):
    lib = pkg.abi.load_library()
    gen = torch.Generator().manual_seed(9)
    n = len(SNAP_SHAPES)
    src = [tad.sentinel_view(torch.randn(*s, generator=gen), offset=offset) for s in SNAP_SHAPES]
    dst = [tad.sentinel_view(torch.full(s, -7.0), offset=offset) for s in SNAP_SHAPES]
    P = ctypes.c_void_p
    c_src = (P * n)(*[v.data_ptr() for v, _ in src])
    c_dst = (P * n)(*[v.data_ptr() for v, _ in dst])
    c_numel = (ctypes.c_int64 * n)(*[v.numel() for v, _ in src])
    mean = torch.zeros(1, dtype=torch.float64, device=DEV)
    best = torch.full((1,), 1.5, dtype=torch.float64, device=DEV)
    state = torch.tensor([0, -1], dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(value, repeat):
        mean.fill_(value)
        pkg.abi.check(lib.marlnav_params_snapshot_if(
            n, c_src, c_dst, c_numel, mean.data_ptr(), best.data_ptr(), state.data_ptr(), repeat,
            track_best, stream), lib)
        torch.cuda.synchronize()
        return [int(x) for x in state.tolist()], float(best)

    untouched = lambda: all(bool((v == -7.0).all()) for v, _ in dst)
    copied = lambda: all(np.array_equal(tad.bits(tg.np_(d)), tad.bits(tg.np_(s)))
                         for (d, _), (s, _) in zip(dst, src))
    assert call(1.0, 3) == ([0, -1], 1.5) and untouched()            # below
    assert call(1.5, 4) == ([0, -1], 1.5) and untouched()            # equal
    assert call(math.nan, 5) == ([0, -1], 1.5) and untouched()       # NaN: not greater
    assert call(2.0, 6) == ([1, 6], 2.0 if track_best else 1.5) and copied()   # above
    for v, _ in src:
        v.add_(1.0)
    # the same mean again: above the reference's never-raised maximum, not above a tracked one
    if track_best:
        assert call(2.0, 7) == ([1, 6], 2.0) and not copied()
    else:
        assert call(2.0, 7) == ([2, 7], 1.5) and copied()
    assert call(-math.inf, 8)[0] == ([1, 6] if track_best else [2, 7])
    for view, buf in src + dst:
        off = view.storage_offset()
        assert off == offset
        outside = torch.cat([buf[:off], buf[off + view.numel():]])
        assert bool((outside == SENTINEL).all()), "a sentinel was overwritten"


# -------------------------------------------------------------- 4. the trainer
def hand_loop(pkg, args, P, A, O, H, seed=21, weight_seed=11):
    """What INTEGRATION.md had a caller assemble: collect_fused, train_actor,
    train_critic with two FusedAdams, on an identically built env."""
    env = tr.make_env(pkg, P, A, O, seed=seed)
    D = 2 + 2 * O + 2 * (A - 1)
    torch.manual_seed(weight_seed)
    actor, critic = pkg.Actor(D, H).to(DEV), pkg.Critic(A * D, H).to(DEV)
    s = {"env": env, "actor": actor, "critic": critic,
         "policy": pkg.FusedPolicy(actor, critic, seed=5),
         "buffer": pkg.RolloutBuffer(args.buffer_len),
         "ppo": pkg.FusedPPO(actor, critic, args.epsilon, args.ent_const),
         "adam_a": pkg.FusedAdam(actor.parameters(), lr=args.learning_rate, maximize=True),
         "adam_c": pkg.FusedAdam(critic.parameters(), lr=args.learning_rate, maximize=False),
         "logs": {"actor": [], "critic": [], "mean_rews": [], "epi": []}, "args": args}
    return s


def hand_repeat(pkg, s):
    a = s["args"]
    mean, stats = pkg.collect_fused(s["env"], s["policy"], s["buffer"], gamma=a.gamma)
    s["logs"]["mean_rews"].append(float(mean))
    s["logs"]["epi"].append(stats)
    pkg.train_actor(s["ppo"], s["buffer"], s["adam_a"], a.num_epochs, a.batch_size,
                    log=s["logs"]["actor"])
    pkg.train_critic(s["ppo"], s["buffer"], s["adam_c"], a.num_epochs, a.batch_size,
                     log=s["logs"]["critic"])


def trainer_state(actor, critic, adam_a, adam_c):
    par = {"actor." + k: v for k, v in actor.named_parameters()}
    par.update({"critic." + k: v for k, v in critic.named_parameters()})
    return tad.full_state(par, {"actor": adam_a, "critic": adam_c})


def assert_trainer_equals_loop(m, s, repeats_done):
    for k, name in enumerate(tr.ENTRIES):
        tr.assert_same(m.buffer.stacked(k), s["buffer"].stacked(k), name)
    np.testing.assert_array_equal(tg.np_(m.buffer.returns), tg.np_(s["buffer"].returns))
    tad.assert_same_bits(trainer_state(m.actor, m.critic, m.actor_optimizer, m.critic_optimizer),
                         trainer_state(s["actor"], s["critic"], s["adam_a"], s["adam_c"]))
    for name in tr.ENV_STATE:
        tr.assert_same(getattr(m.env, name), getattr(s["env"], name), name)
    assert m.env._step_idx == s["env"]._step_idx
    assert m.policy.step_idx == s["policy"].step_idx == repeats_done * m.buffer_len
    assert (m.env._num_trunc, m.env._num_col, m.env._num_tar) == (0, 0, 0)
    logs, want = m.logs(), s["logs"]
    assert np.array_equal(bits64(logs["mean_rews"]), bits64(want["mean_rews"]))
    for k in ("actor", "critic"):
        assert len(logs[k]) == len(want[k]) > 0
        assert np.array_equal(bits64(logs[k]), bits64([float(x) for x in want[k]])), k
    for k in ("trunc", "col", "tar"):
        assert logs["epi_stats"][k] == [e[k] for e in want["epi"]], k
        assert all(isinstance(x, int) for x in logs["epi_stats"][k])
    assert sum(sum(logs["epi_stats"][k]) for k in ("trunc", "col", "tar")) > 0


@pytest.mark.parametrize("P,A,O,H", [(96, 3, 3, 50), (8, 3, 8, 5)])
def test_trainer_equals_the_hand_assembled_loop(pkg, tmp_path, P, A, O, H):
    m, args = make_mappo(pkg, P, A, O, H, 6, 3, 2, out_dir=str(tmp_path))
    s = hand_loop(pkg, args, P, A, O, H)
    assert isinstance(m.actor_optimizer, pkg.FusedAdam) and isinstance(m.buffer, pkg.RolloutBuffer)
    assert m.actor_optimizer.param_groups[0]["maximize"] is True
    assert m.critic_optimizer.param_groups[0]["maximize"] is False
    for r in range(2):
        m.repeat()
        hand_repeat(pkg, s)
        assert_trainer_equals_loop(m, s, r + 1)
    logs = m.logs()
    assert m.save_count() == (2, 1) and m._logs is logs
    # run(2) is two repeats and the files
    m2, _ = make_mappo(pkg, P, A, O, H, 6, 3, 2, out_dir=str(tmp_path / "second"))
    paths = m2.run(2)
    tad.assert_same_bits(
        trainer_state(m2.actor, m2.critic, m2.actor_optimizer, m2.critic_optimizer),
        trainer_state(m.actor, m.critic, m.actor_optimizer, m.critic_optimizer))
    assert [os.path.relpath(p, tmp_path / "second") for p in paths] == [
        os.path.join("weights", m2._time + "_actor.pt"),
        os.path.join("weights", m2._time + "_critic.pt")]


def test_saved_weights_are_those_from_before_the_last_training(pkg, tmp_path):
    P, A, O, H = 96, 3, 3, 50
    m, args = make_mappo(pkg, P, A, O, H, 6, 3, 2, out_dir=str(tmp_path / "ref"))
    best, _ = make_mappo(pkg, P, A, O, H, 6, 3, 2, out_dir=str(tmp_path / "best"),
                         track_best=True)
    assert m.save_weights() is None and not (tmp_path / "ref").exists()
    stages = [{k: v.detach().cpu().clone() for k, v in m.actor.state_dict().items()}]
    critics = [{k: v.detach().cpu().clone() for k, v in m.critic.state_dict().items()}]
    for _ in range(2):
        m.repeat()
        best.repeat()
        stages.append({k: v.detach().cpu().clone() for k, v in m.actor.state_dict().items()})
        critics.append({k: v.detach().cpu().clone() for k, v in m.critic.state_dict().items()})
    actor_path, critic_path = m.save_weights()
    sd = torch.load(actor_path, map_location="cpu", weights_only=True)
    assert tuple(sd) == pkg.training.ACTOR_KEYS
    # the reference's quirk: saved in get_data of repeat 2, before its training
    for k in sd:
        assert torch.equal(sd[k], stages[1][k]), k
        assert not torch.equal(sd[k], stages[2][k]), k
    sc = torch.load(critic_path, map_location="cpu", weights_only=True)
    assert tuple(sc) == pkg.training.CRITIC_KEYS
    for k in sc:
        assert torch.equal(sc[k], critics[1][k]), k
    # track_best: the weights that produced the rollout with the larger mean
    means = best.logs()["mean_rews"]
    assert means == m.logs()["mean_rews"] and means[0] != means[1]
    winner = 1 if means[1] > means[0] else 0
    assert best.save_count() == (1 + winner, winner)
    sb = torch.load(best.save_weights()[0], map_location="cpu", weights_only=True)
    for k in sb:
        assert torch.equal(sb[k], stages[winner][k]), k
    # the file is an actor the evaluation takes
    fused = pkg.FusedActor.from_state_dict(sd, DEV, seed=3)
    res = pkg.evaluate(m.env, fused, 4)
    assert res.as_dict()["num_steps"] == 4


def test_repeat_does_not_synchronise(pkg, tmp_path):
    m, _ = make_mappo(pkg, 96, 3, 3, 50, 6, 3, 2, out_dir=str(tmp_path))
    probe = torch.ones(1, device=DEV)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                       # the mode bites on this build
        m.repeat()
        m.repeat()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    logs = m.logs()
    assert len(logs["mean_rews"]) == 2 and len(logs["actor"]) == 2 * 2 * 2
    assert all(math.isfinite(x) for x in logs["mean_rews"] + logs["actor"] + logs["critic"])


def test_mappo_refuses_what_collect_fused_refuses(pkg):
    args = cli_args(num_parallel=4, buffer_len=4, batch_size=2, num_epochs=1, num_total=16)
    params = pkg.set_env_params(args, DEV)
    params["rng"] = "reference"
    env = pkg.Env(params)
    with pytest.raises(RuntimeError, match="native-RNG"):
        pkg.MAPPO(pkg.set_model_params(args, DEV), env)
    params = pkg.set_env_params(args, DEV)
    params["rng"], params["seed"] = "native", 1
    model = pkg.set_model_params(args, DEV)
    model["normalizer"] = None
    with pytest.raises(RuntimeError, match="normaliser"):
        pkg.MAPPO(model, pkg.Env(params))
    m = pkg.MAPPO(pkg.set_model_params(args, DEV), pkg.Env(params))
    assert m.env._normalizer is not None and m.env._action_scaler is not None
    with pytest.raises(RuntimeError, match="get_data"):
        m.train_actor()


def test_cli_train_runs_and_writes_the_files(pkg, tmp_path, capsys):
    rc = pkg.cli.main(["--train", "-se", "3", "-np", "8", "-bl", "4", "-bs", "2", "-ne", "2", "-nt",
                       "64", "-el", "3", "--no-plots", "--out-dir", str(tmp_path)])
    assert rc == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["repeats"] == 2 and res["saves"] == 2 and math.isfinite(res["last_mean_rew"])
    assert len(res["weights"]) == 2 and len(res["files"]) == 5
    for f in res["weights"] + res["files"]:
        assert os.path.commonpath([f, str(tmp_path)]) == str(tmp_path) and os.path.getsize(f) > 0
    sd = torch.load(res["weights"][0], map_location="cpu", weights_only=True)
    assert tuple(sd) == pkg.training.ACTOR_KEYS and sd["fc1.weight"].shape == (50, 12)
    rows = open([f for f in res["files"] if f.endswith("_act_loss.csv")][0]).read().split()
    assert rows[0] == "Value" and len(rows) == 1 + 2 * 2 * 2
    assert not (tmp_path / "plots").exists()
