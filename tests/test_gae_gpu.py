"""The GAE(lambda) advantage mode on the GPU against
tests/gae_ref.py: the scan (``marlnav_gae_advantages``), the bootstrap value
(``marlnav_critic_values``), the own-env pairing of the actor update
(``marlnav_ppo_*_mode`` with ``MARLNAV_ADVANTAGE_ENV``), the one-call paths in
that mode and the trainer with ``gae_lambda``.

The actor's parity criterion is §10's (tests/test_ppo_gpu.py): per tensor the
kernel's largest |g - g64| / max|g64| within ``FACTOR`` (4) times that of the
fp32 evaluation of gae_ref on the CPU, the reference side of a gradient
counting as at least 2^-24, the loss without a floor. The cases are
test_ppo_gpu's ``make_case`` with the float64 standard-normal ``returns`` read
as ready advantages; the ratio does not depend on the advantage, so
``boundary_margins`` of that file holds every row away from the clip bounds
as it does there (asserted in ``own_env_case``). A loss has no floor in the
criterion, so, as in test_ppo_gpu, a seed is usable only where the fp32
reference's loss error does not land, by cancellation over the rows, below
the rounding level of the values every fp32 evaluation stores (test_ppo_gpu
``loss_rounding_levels``, with the own-env advantage). The CPU's fp32
evaluation differs between hosts, so both conditions were measured, for the
reference alone, on a host without and on a host with a GPU: the seeds below
keep the margins with a factor 2 to spare on both (CHUNKS: test_ppo_gpu's
seed, whose margin of 8400 rows holds without that factor) and have, on the
host with the GPU, where the comparison is made, a reference loss error of
1.0 to 4.4 times that level. The figures are
printed past pytest's capture and appended to the file named by
MARLNAV_GAE_PARITY_OUT, which is how profiles/gae_parity.txt was written."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import gae_ref as gr
import ppo_ref as pp
import test_adam_gpu as tad
import test_ppo_gpu as tg
import test_rollout_gpu as tr
import test_train_gpu as tt
from conftest import cli_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPSILON, ENT_CONST = tg.EPSILON, tg.ENT_CONST
np_ = tg.np_


def bits64(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


# ------------------------------------------------------------------ 1. the scan
SCAN_SHAPES = [(1, 2), (5, 257), (16, 1025), (3, 256)]
_scan = {}


def scan_inputs(T, P):
    """Seeded inputs, shared: done at 5% plus column 0 all done, column 1
    never done and a done in the last row."""
    if (T, P) not in _scan:
        g = torch.Generator().manual_seed(1000 * T + P)
        rewards, values = torch.randn(T, P, generator=g), torch.randn(T, P, 1, generator=g)
        last = torch.randn(P, 1, generator=g)
        done = torch.rand(T, P, generator=g) < 0.05
        done[:, 0], done[:, 1] = True, False
        done[T - 1, P - 1 if P > 2 else 0] = True
        _scan[(T, P)] = (rewards, done, values, last)
    return _scan[(T, P)]


def run_scan(pkg, rewards, done, values, last, gamma, lam):
    out = pkg.rollout.gae_advantages(rewards.to(DEV), done.to(DEV), values.to(DEV), last.to(DEV),
                                     gamma, lam)
    return [np_(x) for x in out]


@pytest.mark.parametrize("gamma", [0.9, 1.0])
@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("T,P", SCAN_SHAPES)
def test_scan_equals_gae_ref(pkg, T, P, lam, gamma):
    rewards, done, values, last = scan_inputs(T, P)
    want = gr.gae(rewards, done, values, last, gamma, lam)
    adv, vt, mean, std = run_scan(pkg, rewards, done, values, last, gamma, lam)
    assert adv.dtype == vt.dtype == np.float64 and adv.shape == vt.shape == (T, P)
    v64 = values.reshape(T, P).double().numpy()
    tight = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(vt - v64, want["raw"].numpy(), **tight)
    np.testing.assert_allclose(vt, want["value_targets"].numpy(), **tight)
    np.testing.assert_allclose(mean, float(want["mean"]), **tight)
    np.testing.assert_allclose(std, float(want["std"]), **tight)
    np.testing.assert_allclose(adv, want["advantages"].numpy(), rtol=1e-10, atol=1e-10)
    # two calls on equal inputs: equal bits
    again = run_scan(pkg, rewards, done, values, last, gamma, lam)
    for a, b in zip((adv, vt, mean, std), again):
        assert np.array_equal(bits64(a), bits64(b))
    # a masked bootstrap value set to inf reaches no output (column 0 is done
    # throughout), and changes none
    last_inf = last.clone()
    last_inf[0] = math.inf
    masked = run_scan(pkg, rewards, done, values, last_inf, gamma, lam)
    for a, b in zip((adv, vt, mean, std), masked):
        assert np.isfinite(b).all() and np.array_equal(bits64(a), bits64(b))


@pytest.mark.parametrize("T,P", SCAN_SHAPES)
def test_scan_with_no_critic_is_the_returns_scan(pkg, T, P):
    """values = 0, last_values = 0, lambda = 1 and no done: the raw advantages
    are the discounted returns, so the normalised ones are
    ``discounted_returns``' to its own tolerance."""
    rewards = scan_inputs(T, P)[0].to(DEV)
    none = torch.zeros(T, P, dtype=torch.bool, device=DEV)
    adv, vt, mean, std = pkg.rollout.gae_advantages(
        rewards, none, torch.zeros(T, P, device=DEV), torch.zeros(P, device=DEV), 0.9, 1.0)
    ret, rmean, rstd = pkg.rollout.discounted_returns(rewards, none, 0.9)
    np.testing.assert_allclose(np_(adv), np_(ret), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(float(mean), float(rmean), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(float(std), float(rstd), rtol=1e-12, atol=1e-12)


def test_buffer_process_gae_sets_both_and_leaves_the_returns(pkg):
    T, P = 5, 257
    rewards, done, values, last = (x.to(DEV) for x in scan_inputs(T, P))
    buf = pkg.RolloutBuffer(T)
    for t in range(T):
        buf.add(torch.zeros(P, 3, 12, device=DEV), torch.zeros(P, 3, 2, device=DEV),
                torch.zeros(P * 3, device=DEV), values[t], rewards[t], done[t])
    buf.process_rewards(0.9)
    ret = buf.returns
    mean = buf.process_gae(0.9, 0.95, last)
    adv, vt, m, _ = pkg.rollout.gae_advantages(rewards, done, values, last, 0.9, 0.95)
    assert torch.equal(buf.advantages, adv) and torch.equal(buf.value_targets, vt)
    assert float(mean) == float(m) and buf.returns is ret
    buf.clear()
    assert buf.advantages is None and buf.value_targets is None


# ---------------------------------------------------------------- 2. bootstrap
@pytest.mark.parametrize("offset_floats", [0, 2])
@pytest.mark.parametrize("H", [5, 50])
@pytest.mark.parametrize("P,A,O", [(5, 3, 3), (70, 3, 8), (3, 16, 32)])
def test_values_equal_the_policy_launchs_values(pkg, P, A, O, H, offset_floats):
    policy = tr.make_policy(pkg, A, O, H)
    D = policy.obs_dim
    n = P * A * D
    g = torch.Generator().manual_seed(P + H)
    flat = (torch.rand(n + 4, generator=g) * 2 - 1).to(DEV)
    zeros = torch.zeros(P * A, 2, device=DEV)
    # rows at offset_floats (0: 16-byte aligned, the compiled shapes' kernels;
    # 2: 8-byte only, the generic kernel at a compiled shape too) and the same
    # 4 bytes further on (the generic kernel, scalar loads alone)
    for off in (offset_floats, offset_floats + 1):
        x = flat[off:off + n].view(P, A, D)
        assert x.is_contiguous() and x.data_ptr() % 16 == 4 * off
        policy.step_idx = 7
        want = policy.act(x, eps=zeros)[2]
        got = policy.values(x)
        assert got.shape == (P, 1) and got.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert policy.step_idx == 7
        out = torch.full((P, 1), 3.0, device=DEV)
        assert policy.values(x, out=out) is out and torch.equal(out, want)
    # the kernel's own normals are drawn by act alone: values() between two
    # draws does not move the stream
    a = policy.act(x)[0].clone()
    policy.step_idx = 7
    policy.values(x)
    assert torch.equal(policy.act(x)[0], a)


# ------------------------------------------------- 3. own-env actor gradients
# T x P of A x O with H, seed (module docstring)
TINY = (2, 3, 3, 3, 50, 1)           # less than one tile
RAGGED = (1, 300, 2, 3, 50, 5)       # 600 rows: a ragged third tile
CHUNKS = (4, 700, 3, 3, 50, 1621)    # 9 blocks of 1024 rows: ranges no multiple of A = 3
WIDE = (2, 3, 16, 32, 50, 1)         # 4954 actor elements: past the folded Adam's 1024
OWN_ENV_SHAPES = {"tiny": TINY, "ragged": RAGGED, "chunks": CHUNKS, "wide": WIDE}
_own = {}


def own_env_case(T, P, A, O, H, seed):
    """(w, data, truth64, ref32) of test_ppo_gpu.make_case, its ``returns``
    read as ready advantages; every row keeps its margin from the clip
    bounds."""
    key = (T, P, A, O, H, seed)
    if key not in _own:
        w, data = tg.make_case(T, P, A, O, H, seed)
        for what, gap, dev in tg.boundary_margins(w, data, ("actor",)):
            assert gap >= tg.GAPS[what] and gap >= tg.MARGIN * dev, (what, gap, dev)
        w64 = {k: v.double() for k, v in w.items()}
        d64 = {k: v.double() for k, v in data.items()}
        truth = gr.actor_loss_and_grads(w64, d64, d64["returns"], EPSILON, ENT_CONST)
        ref = gr.actor_loss_and_grads(w, data, data["returns"], EPSILON, ENT_CONST)
        _own[key] = (w, data, truth, ref)
    return _own[key]


def gae_buffer(pkg, data, value_targets=None):
    """test_ppo_gpu's buffer with ``returns`` moved to ``advantages``."""
    buf = tg.buffer_of(pkg, data)
    buf.advantages, buf.returns = buf.returns, None
    vt = data["values"].reshape(buf.advantages.shape).double() if value_targets is None \
        else value_targets
    buf.value_targets = vt.to(DEV)
    return buf


def fused_gae(pkg, w, data, value_targets=None):
    actor, critic, par = tg.modules(w)
    ppo = pkg.FusedPPO(actor, critic, EPSILON, ENT_CONST, advantage="gae")
    return ppo, gae_buffer(pkg, data, value_targets), par


def actor_grads(ppo, buf, par):
    loss = float(ppo.actor_loss_grad(buf, 0, len(buf)))
    return loss, {k: np_(par[k].grad).copy() for k in pp.ACTOR_PARAMS}


def report(capsys, title, pooled):
    text = "\n".join([f"{title} (largest |x - x64| / max|x64|, bound {pp.FACTOR:g} x reference)"]
                     + ["  " + line for line in pooled.lines()])
    with capsys.disabled():
        print("\n" + text)
    out = os.environ.get("MARLNAV_GAE_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(text + "\n")


@pytest.mark.parametrize("name", list(OWN_ENV_SHAPES))
def test_own_env_actor_parity(pkg, capsys, name):
    shape = OWN_ENV_SHAPES[name]
    w, data, truth, ref = own_env_case(*shape)
    if name == "wide":
        assert sum(w[k].numel() for k in pp.ACTOR_PARAMS) > 1024
    ppo, buf, par = fused_gae(pkg, w, data)
    loss, grads = actor_grads(ppo, buf, par)
    pooled = pp.Pooled()
    pooled.add("actor loss", loss, float(ref[0]), float(truth[0]))
    for k, g64 in truth[1].items():
        pooled.add(k, grads[k], ref[1][k].numpy(), g64.numpy())
    report(capsys, f"own-env actor, (T, P, A, O, H) = {shape[:5]}:", pooled)
    floor = lambda k: 0.0 if k.endswith("loss") else 2.0 ** -24
    bad = [(k, pooled.got[k], pooled.ref[k]) for k in pooled.got
           if not pooled.got[k] <= pp.FACTOR * max(pooled.ref[k], floor(k))]
    assert not bad, bad
    # the actor reads no values in this mode: equal bits with other values stored
    buf.stacked(buf.VALUES).add_(1.0)
    loss2, grads2 = actor_grads(ppo, buf, par)
    assert loss2 == loss and all(np.array_equal(grads2[k], grads[k]) for k in grads)


def test_the_pairing_really_changed(pkg):
    """On the same arrays (values zero, so both modes read the same
    advantages and only pair them differently) the own-env gradients are more
    than 100 x the fp32 error away from the reference pairing's."""
    w, data, truth, ref = own_env_case(*TINY)
    data = dict(data, values=torch.zeros_like(data["values"]))
    ppo1, buf1, par1 = fused_gae(pkg, w, data)
    _, g1 = actor_grads(ppo1, buf1, par1)
    ppo0, buf0, par0 = tg.fused(pkg, w, data)
    _, g0 = actor_grads(ppo0, buf0, par0)
    for k, g64 in truth[1].items():
        scale = float(g64.abs().max())
        err32 = max(float((ref[1][k].double() - g64).abs().max()) / scale, 2.0 ** -24)
        moved = float(np.abs(g1[k].astype(np.float64) - g0[k]).max()) / scale
        assert moved > 100 * err32, (k, moved, err32)
    # and mode 0 holds the reference pairing's truth, mode 1 does not
    t0 = pp.loss_and_grads("actor", {k: v.double() for k, v in w.items()},
                           {k: v.double() for k, v in data.items()}, EPSILON, ENT_CONST)[1]
    for k in g0:
        np.testing.assert_allclose(g0[k], t0[k].numpy(), rtol=1e-3, atol=1e-6 * float(t0[k].abs().max()))


def old_calls(pkg, ppo, buf, adam, lo, hi, bounds=None, epochs=1):
    """The three entry points from before the mode argument, called through
    the structs ``ppo`` binds: grad, update, or (with bounds) the phase."""
    lib = pkg.abi.load_library()
    stream = torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
    loss = ppo._bind(buf, lo, hi)
    d, b = ctypes.byref(ppo._dims), ctypes.byref(ppo._bufs)
    if adam is None:
        pkg.abi.check(lib.marlnav_ppo_actor_grad(d, b, ppo.epsilon, ppo.ent_const, stream), lib)
        return loss
    ad, ab = adam._bind()
    if bounds is None:
        pkg.abi.check(lib.marlnav_ppo_actor_update(d, b, ppo.epsilon, ppo.ent_const,
                                                   ctypes.byref(ad), ctypes.byref(ab), stream), lib)
        return loss
    B = len(bounds)
    arr = (ctypes.c_int64 * (2 * B))(*[x for p in bounds for x in p])
    out = torch.empty(epochs * B, dtype=torch.float64, device=DEV)
    need = int(lib.marlnav_ppo_train_work_size(d, arr, B))
    if ppo._work.numel() < need:
        ppo._work = torch.empty(need, dtype=torch.float64, device=DEV)
        ppo._bufs.work = ppo._work.data_ptr()
    pkg.abi.check(lib.marlnav_ppo_train_phase(0, d, b, arr, B, epochs, ppo.epsilon, ppo.ent_const,
                                              ctypes.byref(ad), ctypes.byref(ab), out.data_ptr(),
                                              stream), lib)
    return out


@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_mode_zero_through_the_new_calls_is_the_old_calls(pkg, name):
    T, P, A, O, H, seed = OWN_ENV_SHAPES[name]
    w, data = tg.make_case(T + 1, P, A, O, H, seed)
    bounds = pkg.minibatch_bounds(T + 1, T)

    def run(old):
        ppo, buf, par, adams = tad.ppo_setup(pkg, w, data)
        assert ppo._mode == pkg.abi.ADVANTAGE_REFERENCE
        adam = adams["actor"]
        out = []
        if old:
            out.append(float(old_calls(pkg, ppo, buf, None, 0, T)))
            out.append(float(old_calls(pkg, ppo, buf, adam, 0, T)))
            out += np_(old_calls(pkg, ppo, buf, adam, 0, T + 1, bounds, 2)).tolist()
        else:
            out.append(float(ppo.actor_loss_grad(buf, 0, T)))
            out.append(float(ppo.actor_update(buf, 0, T, adam)))
            out += np_(pkg.training.train_phase(ppo, buf, adam, "actor", 2, T)).tolist()
        return np.array(out), tad.full_state(par, adams)

    (lo, so), (ln, sn) = run(True), run(False)
    assert np.array_equal(bits64(lo), bits64(ln)) and np.isfinite(lo).all()
    tad.assert_same_bits(so, sn)
    assert so["actor count"] == 3


# ------------------------------------------------------------ 4. one-call paths
def gae_setup(pkg, w, data):
    g = torch.Generator().manual_seed(77)
    vt = data["values"].reshape(data["returns"].shape).double() + \
        0.05 * torch.randn(data["returns"].shape, generator=g, dtype=torch.float64)
    ppo, buf, par = fused_gae(pkg, w, data, vt)
    adams = {"actor": tad.fused_adam(pkg, [par[k] for k in pp.ACTOR_PARAMS], True),
             "critic": tad.fused_adam(pkg, [par[k] for k in pp.CRITIC_PARAMS], False)}
    return ppo, buf, par, adams


def test_gae_actor_update_equals_grad_then_adam(pkg):
    for shape in (TINY, WIDE):
        w, data = own_env_case(*shape)[:2]
        T = shape[0]
        two, one = gae_setup(pkg, w, data), gae_setup(pkg, w, data)
        for _ in range(2):
            ppo, buf, par, adams = two
            l2 = ppo.actor_loss_grad(buf, 0, T)
            adams["actor"].step()
            c2 = ppo.critic_loss_grad(buf, 0, T)
            adams["critic"].step()
            ppo, buf, par, adams = one
            l1 = ppo.actor_update(buf, 0, T, adams["actor"])
            c1 = ppo.critic_update(buf, 0, T, adams["critic"])
            assert float(l1) == float(l2) and float(c1) == float(c2)
            tad.assert_same_bits(tad.full_state(one[2], one[3]), tad.full_state(two[2], two[3]))
        assert one[3]["actor"].step_count() == 2 and one[3]["critic"].step_count() == 2
        for k, p in one[2].items():
            assert not np.array_equal(np_(p), w[k].numpy()), f"{k} did not move"


def test_gae_critic_is_trained_towards_the_value_targets(pkg):
    """The critic kernel is unchanged: its loss in the GAE mode is the
    reference-mode loss of a buffer whose returns are the value targets."""
    w, data = own_env_case(*TINY)[:2]
    ppo, buf, par, _ = gae_setup(pkg, w, data)
    got = float(ppo.critic_loss_grad(buf, 0, len(buf)))
    grads = {k: np_(par[k].grad).copy() for k in pp.CRITIC_PARAMS}
    ppo0, buf0, par0 = tg.fused(pkg, w, dict(data, returns=buf.value_targets.cpu()))
    want = float(ppo0.critic_loss_grad(buf0, 0, len(buf0)))
    assert got == want
    for k in grads:
        assert np.array_equal(grads[k], np_(par0[k].grad))


# P x A x O (H = 50), the networks checked: 16 x 3 x 3 folds both Adam steps
# into the finish launches, 6 x 16 x 32 has more than 1024 actor elements
PHASES = {"folded": (16, 3, 3, 7, ("actor", "critic")), "unfolded": (6, 16, 32, 101, ("actor",))}


@pytest.mark.parametrize("name", sorted(PHASES))
def test_gae_phase_equals_the_loops_of_updates(pkg, name):
    P, A, O, seed, nets = PHASES[name]
    w, data = tt.case(5, P, A, O, 50, seed)
    epochs, batch = 2, 2
    assert pkg.minibatch_bounds(5, batch) == [(0, 2), (2, 4)]
    ppo, buf, par, adams = gae_setup(pkg, w, data)
    logs = {"actor": [], "critic": []}
    train = {"actor": pkg.train_actor, "critic": pkg.train_critic}
    for net in nets:
        train[net](ppo, buf, adams[net], epochs, batch, log=logs[net])
    want = tad.full_state(par, adams)
    ppo, buf, par, adams = gae_setup(pkg, w, data)
    for net in nets:
        got = np_(pkg.training.train_phase(ppo, buf, adams[net], net, epochs, batch))
        loop = np.array([float(x) for x in logs[net]])
        assert got.shape == (4,) and np.isfinite(got).all()
        assert np.array_equal(bits64(got), bits64(loop)), (net, got, loop)
    have = tad.full_state(par, adams)
    tad.assert_same_bits(have, want)
    for net in nets:
        assert have[net + " count"] == 4
        for k in (pp.ACTOR_PARAMS if net == "actor" else pp.CRITIC_PARAMS):
            assert not np.array_equal(have[k], w[k].numpy()), f"{k} did not move"


def test_gae_training_refuses_a_buffer_without_advantages(pkg):
    w, data = own_env_case(*TINY)[:2]
    ppo, buf, par, adams = gae_setup(pkg, w, data)
    buf.advantages = None
    for call in (lambda: ppo.actor_loss_grad(buf, 0, 2), lambda: ppo.critic_loss_grad(buf, 0, 2),
                 lambda: ppo.actor_update(buf, 0, 2, adams["actor"]),
                 lambda: pkg.train_actor(ppo, buf, adams["actor"], 1, 1),
                 lambda: pkg.training.train_phase(ppo, buf, adams["critic"], "critic", 1, 1)):
        with pytest.raises(RuntimeError, match="process_gae"):
            call()


# -------------------------------------------------------------- 5. the trainer
P5, A5, O5, H5, BL, BS, NE, LAM = 64, 3, 3, 50, 4, 2, 2, 0.95


def make_mappo(pkg, out_dir, gae_lambda=LAM):
    args = cli_args(num_parallel=P5, num_agents=A5, num_obstacles=O5, episode_len=2,
                    risk_factor=2.0, distance_factor=3.0, hidden_size=H5, buffer_len=BL,
                    batch_size=BS, num_epochs=NE, learning_rate=tt.LR, num_total=2 * BL * P5)
    args.gae_lambda = gae_lambda
    env = tr.make_env(pkg, P5, A5, O5, seed=21, normalizer=False, scaler=False)
    torch.manual_seed(11)
    params = pkg.set_model_params(args, DEV)
    assert ("gae_lambda" in params) == (gae_lambda is not None)
    return pkg.MAPPO(params, env, seed=5, out_dir=str(out_dir)), args


def test_trainer_in_gae_mode_equals_the_hand_assembled_sequence(pkg, tmp_path):
    m, args = make_mappo(pkg, tmp_path / "gae")
    assert m.gae_lambda == LAM and m.ppo.advantage == "gae"
    s = tt.hand_loop(pkg, args, P5, A5, O5, H5)
    s["ppo"] = pkg.FusedPPO(s["actor"], s["critic"], args.epsilon, args.ent_const, advantage="gae")
    before = torch.cuda.get_sync_debug_mode()
    for r in range(2):
        torch.cuda.set_sync_debug_mode("error")
        try:
            m.repeat()
        finally:
            torch.cuda.set_sync_debug_mode(before)
        mean, stats = pkg.collect_fused(s["env"], s["policy"], s["buffer"], gamma=args.gamma,
                                        gae_lambda=LAM)
        s["logs"]["mean_rews"].append(float(mean))
        s["logs"]["epi"].append(stats)
        pkg.train_actor(s["ppo"], s["buffer"], s["adam_a"], NE, BS, log=s["logs"]["actor"])
        pkg.train_critic(s["ppo"], s["buffer"], s["adam_c"], NE, BS, log=s["logs"]["critic"])
        for k in ("advantages", "value_targets"):
            a, b = getattr(m.buffer, k), getattr(s["buffer"], k)
            assert a.shape == (BL, P5) and a.dtype == torch.float64 and torch.equal(a, b), k
            assert bool(torch.isfinite(a).all())
        tt.assert_trainer_equals_loop(m, s, r + 1)
    # the bootstrap is the critic's value of what the env holds after the last
    # step; the estimator is gae_ref's on the stored rollout
    buf = s["buffer"]
    want = gr.gae(buf.stacked(4).cpu(), buf.stacked(5).cpu(), buf.stacked(3).cpu(),
                  torch.zeros(P5), args.gamma, LAM)
    done_last = buf.stacked(5)[BL - 1].cpu()
    got_raw = buf.value_targets.cpu() - buf.stacked(3).cpu().reshape(BL, P5).double()
    np.testing.assert_allclose(got_raw[:, done_last].numpy(), want["raw"][:, done_last].numpy(),
                               rtol=1e-12, atol=1e-12)      # envs whose bootstrap is masked
    assert bool(done_last.any()) and not bool(done_last.all())

    # run(2) is the two repeats and the files; the first rollout is collected
    # before any training, so its mean reward is the reference mode's
    m2, _ = make_mappo(pkg, tmp_path / "gae2")
    paths = m2.run(2)
    assert paths is not None and all(os.path.exists(p) for p in paths)
    tad.assert_same_bits(
        tt.trainer_state(m2.actor, m2.critic, m2.actor_optimizer, m2.critic_optimizer),
        tt.trainer_state(m.actor, m.critic, m.actor_optimizer, m.critic_optimizer))
    ref, _ = make_mappo(pkg, tmp_path / "ref", gae_lambda=None)
    assert ref.gae_lambda is None and ref.ppo.advantage == "reference"
    ref.run(2)
    assert ref.buffer.advantages is None and ref.buffer.value_targets is None
    lg, lr = m2.logs(), ref.logs()
    assert np.array_equal(bits64(lg["mean_rews"][:1]), bits64(lr["mean_rews"][:1]))
    assert lg["actor"] != lr["actor"]                # the estimators differ
    assert all(math.isfinite(x) for x in lg["mean_rews"] + lg["actor"] + lg["critic"])


def test_collect_and_collect_fused_agree_in_gae_mode(pkg):
    P, A, O, H, T = 70, 3, 3, 50, 5
    out = []
    for fn in (pkg.collect, pkg.collect_fused):
        env = tr.make_env(pkg, P, A, O)
        policy = tr.make_policy(pkg, A, O, H)
        buf = pkg.RolloutBuffer(T)
        fn(env, policy, buf, gamma=0.9, gae_lambda=0.95)
        assert policy.step_idx == T
        out.append((buf.advantages, buf.value_targets, buf.returns))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_cli_train_with_gae_lambda_writes_the_files(pkg, tmp_path, capsys):
    import json
    argv = ["--train", "-se", "3", "-np", "8", "-bl", "4", "-bs", "2", "-ne", "2", "-nt", "64",
            "-el", "3", "--no-plots"]
    assert pkg.cli.main(argv + ["--gae-lambda", "0.95", "--out-dir", str(tmp_path / "gae")]) == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["repeats"] == 2 and res["saves"] == 2 and math.isfinite(res["last_mean_rew"])
    assert len(res["weights"]) == 2 and len(res["files"]) == 5
    for f in res["weights"] + res["files"]:
        assert os.path.getsize(f) > 0
    params = json.load(open([f for f in res["files"] if f.endswith("_params.json")][0]))
    assert params["model"]["gae_lambda"] == 0.95
    # without the flag: the params file has no such key, and other losses
    assert pkg.cli.main(argv + ["--out-dir", str(tmp_path / "ref")]) == 0
    ref = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert "gae_lambda" not in json.load(
        open([f for f in ref["files"] if f.endswith("_params.json")][0]))["model"]
    rows = lambda r: open([f for f in r["files"] if f.endswith("_act_loss.csv")][0]).read().split()
    assert len(rows(res)) == len(rows(ref)) == 1 + 2 * 2 * 2 and rows(res) != rows(ref)
    assert pkg.cli.main(argv + ["--gae-lambda", "1.5", "--out-dir", str(tmp_path / "bad")]) == 2
    assert "gae_lambda" in capsys.readouterr().err and not (tmp_path / "bad").exists()
