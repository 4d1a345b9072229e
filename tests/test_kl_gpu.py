"""The actor phase's diagnostics and target-KL stop on the GPU:
``marlnav_ppo_actor_grad_diag`` through ``FusedPPO.actor_loss_grad(diag_out=)``,
``marlnav_ppo_train_phase_monitored`` through ``training.train_phase(target_kl=,
diag_out=, stop_out=)`` and ``MAPPO`` with ``params['target_kl']`` /
``params['log_diagnostics']``.

Parity: truth is tests/kl_ref.py in float64 on the CPU, the reference side
the same in float32, under the project's criterion (``ppo_ref.Pooled``,
``FACTOR`` 4, floor 2^-24 as in tests/test_clip_gpu.py) pooled per quantity
over every case of fixture F7-ppo and the four generated shapes, per pairing;
the clip fraction must be the float64 count exactly, which the cases allow: no
row's float64 ratio lies within ``GAPS['ratio']`` of 1 -+ epsilon (asserted
here, and on the CPU by tests/test_kl_cpu.py). The figures are printed past
pytest's capture and appended to the file named by MARLNAV_KL_PARITY_OUT, which
is how profiles/kl_parity.txt was written.

Everything else is for equal bits, derived and not measured: the diagnostic
kernels add accumulators and touch none of the existing ones, the finish
launch sums the existing columns in the existing order, the gated Adam
launches are the ungated ones behind one read of the flag, and a phase that
stops at update j has run the kernels of the unstopped phase on the same bits
up to j.

Shapes (T, P, A, O, H, seed), the path of each pinned by tests/test_kl_cpu.py
through ``ppo_ref.launch_plan`` as (actor blocks, finish groups, row slices,
column rounds):

  tiny      2  3    3   3    50   one block, one partial tile of 18 rows
  chunks    4  700  3   3    50   9 blocks, the last partial; finish by groups
  mid_row   2  16   16  48   50   D + 1 = 129: idle phase-2 threads
  long_row  2  64   2   127  8    D + 1 = 259: 2 column rounds, finish without groups
  small     5  3    3   3    50   854 actor elements (folded when unmonitored)
  large     5  5    16  32   16   1620 (never folded); minibatches of 2 steps
  capture   3  67   3   3    50   one minibatch of 2 steps"""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import kl_ref as kr
import ppo_ref as pp
import test_adam_gpu as tad
import test_clip_gpu as tc
import test_ppo_gpu as tg
import test_train_gpu as tt
from conftest import cli_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
EPSILON, ENT_CONST = tg.EPSILON, tg.ENT_CONST
SENTINEL = tad.SENTINEL
MODES = ("reference", "gae")
MAX_NORMS = (None, tc.PATH_MAX_NORM)

DIAG_SHAPES = {"tiny": (2, 3, 3, 3, 50, 7), "chunks": tg.CHUNKS, "mid_row": tg.MID_ROW,
               "long_row": tg.LONG_ROW}
# a learning rate of test_adam_gpu's 3e-4 and these seeds give, on the CPU in
# float64, a KL sequence over 3 epochs x 2 minibatches whose first record
# update is j = 2 (4 for the clipped own-env pairing of `small`), 4% to 90%
# above the earlier ones
STOP_SHAPES = {"small": (5, 3, 3, 3, 50, 3), "large": (5, 5, 16, 32, 16, 2)}
OTHER_SHAPES = {"small minibatch": (2, 3, 3, 3, 50, 3), "large minibatch": (2, 5, 16, 32, 16, 2),
                "capture": (2, 67, 3, 3, 50, 404)}
ACTOR_PLANS = {"tiny": (1, 4, 19, 1), "chunks": (9, 4, 19, 1), "mid_row": (1, 1, 1, 1),
               "long_row": (1, 1, 1, 2), "small": (1, 4, 19, 1), "large": (1, 1, 2, 1),
               "small minibatch": (1, 4, 19, 1), "large minibatch": (1, 1, 2, 1),
               "capture": (1, 4, 19, 1)}
STOP_EPOCHS, STOP_BATCH = 3, 2


def cells(n, dtype=F64, fill=0.0):
    return torch.full((n,), fill, dtype=dtype, device=DEV)


# ------------------------------------------------------------------ 1. parity
_cases, _refs = {}, {}


def diag_case(name):
    """(w, data) of a generated shape or of a fixture case, float32 on the CPU."""
    if name not in _cases:
        if name in DIAG_SHAPES:
            _cases[name] = tg.make_case(*DIAG_SHAPES[name])
        else:
            _cases[name] = pp.tensors(pp.load_case(name))
    return _cases[name]


def case_epsilon(name):
    return EPSILON if name in DIAG_SHAPES else pp.load_case(name)["epsilon"]


def references(name, mode):
    """(truth in float64, reference side in float32) of kl_ref, once per case."""
    if (name, mode) not in _refs:
        w, data = diag_case(name)
        w64 = {k: v.double() for k, v in w.items()}
        d64 = {k: v.double() for k, v in data.items()}
        own, eps = mode == "gae", case_epsilon(name)
        _refs[(name, mode)] = (kr.diagnostics(w64, d64, eps, own), kr.diagnostics(w, data, eps, own))
    return _refs[(name, mode)]


def guarded_grads(par):
    """Every actor .grad becomes a view inside a sentinel-filled buffer."""
    guards = []
    for k in pp.ACTOR_PARAMS:
        view, whole = tad.sentinel_view(torch.zeros(par[k].numel()), offset=4)
        par[k].grad = view.view(par[k].shape)
        guards.append((view, whole))
    return guards


def assert_guards(guards):
    for view, whole in guards:
        off = view.storage_offset()
        outside = torch.cat([whole[:off], whole[off + view.numel():]])
        assert bool((outside == SENTINEL).all()), "a sentinel was overwritten"


def run_diag(pkg, w, data, mode, epsilon=EPSILON):
    """``actor_loss_grad(diag_out=)`` over the whole case between sentinels in
    the row, behind the workspace and around every .grad; -> (loss, row,
    grads) and the same from the plain call on other allocations."""
    lib = pkg.abi.load_library()
    T = data["returns"].shape[0]
    ppo, buf, par, _ = tc.setup(pkg, w, data, mode)
    ppo.epsilon = float(epsilon)
    guards = guarded_grads(par)
    ppo._bind(buf, 0, T)
    need = int(lib.marlnav_ppo_diag_work_size(ctypes.byref(ppo._dims)))
    assert need >= int(lib.marlnav_ppo_work_size(ctypes.byref(ppo._dims))) > 0
    work = ppo._work = cells(need + 16, fill=SENTINEL)
    cell = cells(1 + 5 + 2, fill=SENTINEL)
    loss = ppo.actor_grad(buf, 0, T, diag_out=cell[1:6])
    torch.cuda.synchronize()
    assert ppo._work is work and bool((work[need:] == SENTINEL).all())
    assert float(cell[0]) == SENTINEL and bool((cell[6:] == SENTINEL).all())
    assert_guards(guards)
    got = (float(loss), tg.np_(cell[1:6]).copy(),
           {k: tg.np_(par[k].grad).copy() for k in pp.ACTOR_PARAMS})
    ppo2, buf2, par2, _ = tc.setup(pkg, w, data, mode)
    ppo2.epsilon = float(epsilon)
    loss2 = float(ppo2.actor_loss_grad(buf2, 0, T))
    return got, (loss2, {k: tg.np_(par2[k].grad).copy() for k in pp.ACTOR_PARAMS})


def loss_of_row(row, ent_const=ENT_CONST):
    """surrogate_mean + (double)(ent_f * (float)entropy_mean), as the kernel forms it."""
    return float(np.float64(row[0]) + np.float64(np.float32(ent_const) * np.float32(row[1])))


def report(capsys, title, pooled, extra):
    text = "\n".join([f"{title} (largest |x - x64| / |x64| over the cases, bound "
                      f"{pp.FACTOR:g} x max(reference, 2^-24))"]
                     + ["  " + line for line in pooled.lines()] + ["  " + extra])
    with capsys.disabled():
        print("\n" + text)
    out = os.environ.get("MARLNAV_KL_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(text + "\n")


@pytest.mark.parametrize("mode", MODES)
def test_diagnostics_parity_and_monitoring_changes_nothing(pkg, capsys, mode):
    pooled, counts = pp.Pooled(), []
    for name in pp.case_names() + list(DIAG_SHAPES):
        w, data = diag_case(name)
        eps = case_epsilon(name)
        truth, ref = references(name, mode)
        # the exact comparison of the clip fraction needs every row off the bounds
        gap = kr.ratio_gap(truth["ratio"], eps)
        assert gap >= tg.GAPS["ratio"], (name, gap)
        (loss, row, grads), (loss2, grads2) = run_diag(pkg, w, data, mode, eps)
        print(name, mode, dict(zip(kr.ROW, row)), "gap %.2e" % gap)
        for k in ("approx_kl", "surrogate_mean", "entropy_mean"):
            pooled.add(k, row[kr.ROW.index(k)], ref[k], truth[k])
        M = truth["ratio"].numel()
        assert row[3] == truth["outside"] / M, (name, row[3] * M, truth["outside"])
        assert row[4] == 0.0
        counts.append(f"{truth['outside']}/{M}")
        # monitoring changes nothing: loss and every .grad bit for bit
        assert tt.bits64(loss) == tt.bits64(loss2), (name, loss, loss2)
        for k in grads:
            assert np.array_equal(tad.bits(grads[k]), tad.bits(grads2[k])), (name, k)
        assert tt.bits64(loss) == tt.bits64(loss_of_row(row)), (name, loss, loss_of_row(row))
    report(capsys, f"actor diagnostics, {mode} pairing, {len(counts)} cases:", pooled,
           "clip fraction equal to the float64 count in every case: " + " ".join(counts))
    bad = [(k, pooled.got[k], pooled.ref[k]) for k in pooled.got
           if not pooled.got[k] <= pp.FACTOR * max(pooled.ref[k], 2.0 ** -24)]
    assert not bad, bad


# ------------------------------------------------ 2. monitoring changes nothing
def stop_case(name):
    return tt.case(*STOP_SHAPES[name])


def phase(pkg, s, **kw):
    """The actor phase of 3 epochs x 2 minibatches over setup ``s``; -> losses."""
    ppo, buf, par, adams = s
    return tt.losses(pkg.training.train_phase(ppo, buf, adams["actor"], "actor", STOP_EPOCHS,
                                              STOP_BATCH, **kw))


def actor_state(s):
    """Parameters, .grad, moments and count of the actor, and its whole state
    block (count, step scalars, the clip's coefficient cell)."""
    ppo, buf, par, adams = s
    actor = {k: par[k] for k in pp.ACTOR_PARAMS}
    return tad.full_state(actor, {"actor": adams["actor"]}), tg.np_(adams["actor"]._state).copy()


@pytest.mark.parametrize("max_norm", MAX_NORMS, ids=["plain", "clipped"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(STOP_SHAPES))
def test_the_monitored_phase_stores_the_unmonitored_bits(pkg, name, mode, max_norm):
    w, data = stop_case(name)
    assert pkg.minibatch_bounds(5, STOP_BATCH) == [(0, 2), (2, 4)]
    U = STOP_EPOCHS * 2
    plain, mon = tc.setup(pkg, w, data, mode), tc.setup(pkg, w, data, mode)
    kw = {} if max_norm is None else {"max_grad_norm": max_norm}
    norms_p, norms_m = (cells(U), cells(U)) if max_norm else (None, None)
    lp = phase(pkg, plain, norm_out=norms_p, **kw)
    diag, stop = cells(U * 5, fill=SENTINEL).view(U, 5), cells(2, torch.int64, 7)
    lm = phase(pkg, mon, norm_out=norms_m, diag_out=diag, stop_out=stop, **kw)
    assert np.array_equal(tt.bits64(lm), tt.bits64(lp)) and np.isfinite(lp).all()
    (sp, bp), (sm, bm) = actor_state(plain), actor_state(mon)
    tad.assert_same_bits(sm, sp)
    assert np.array_equal(bm, bp) and sp["actor count"] == U
    if max_norm:
        assert np.array_equal(tt.bits64(tt.losses(norms_m)), tt.bits64(tt.losses(norms_p)))
        assert (tt.losses(norms_p) > max_norm).all()            # every update is clipped
    rows = tg.np_(diag)
    assert stop.tolist() == [0, -1] and (rows[:, 4] == 0.0).all()
    assert np.isfinite(rows).all() and (rows[1:, 2] > 0).all() and (rows[:, 3] > 0).all()
    for k in range(U):
        assert tt.bits64(lm[k]) == tt.bits64(loss_of_row(rows[k])), k
    assert mon[0].last_diag is diag and mon[0].last_stop is stop
    for k in w:
        if k.startswith("actor"):
            assert not np.array_equal(sm[k], w[k].numpy()), f"{k} did not move"


# ---------------------------------------------------------------- 3. the stop
def run_stop(pkg, w, data, mode, max_norm, target):
    s = tc.setup(pkg, w, data, mode)
    U = STOP_EPOCHS * 2
    kw = {} if max_norm is None else {"max_grad_norm": max_norm, "norm_out": cells(U, fill=-1.0)}
    diag, stop = cells(U * 5, fill=SENTINEL).view(U, 5), cells(2, torch.int64, 7)
    losses = phase(pkg, s, target_kl=target, diag_out=diag, stop_out=stop, **kw)
    norms = tt.losses(kw["norm_out"]) if max_norm else None
    return s, losses, tg.np_(diag).copy(), [int(x) for x in stop.tolist()], norms


@pytest.mark.parametrize("max_norm", MAX_NORMS, ids=["plain", "clipped"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(STOP_SHAPES))
def test_the_stop(pkg, name, mode, max_norm):
    w, data = stop_case(name)
    bounds = pkg.minibatch_bounds(5, STOP_BATCH)
    U, B = STOP_EPOCHS * len(bounds), len(bounds)
    _, l0, d0, stop0, n0 = run_stop(pkg, w, data, mode, max_norm, math.inf)
    kl = d0[:, 2]
    assert stop0 == [0, -1] and (d0[:, 4] == 0.0).all() and np.isfinite(d0).all()
    record = [j for j in range(1, U) if kl[j] > kl[:j].max()]
    assert record, kl                      # (chosen on the CPU: STOP_SHAPES)
    j = record[0]
    target = math.sqrt(kl[:j].max() * kl[j])
    assert kl[:j].max() < target < kl[j]
    print(name, mode, max_norm, "kl", kl, "j", j, "target", target)
    assert kr.stop_rule(list(kl), target) == ([0] * j + [1] + [2] * (U - j - 1), j)

    s, l1, d1, stop1, n1 = run_stop(pkg, w, data, mode, max_norm, target)
    assert stop1 == [1, j]
    assert d1[:, 4].tolist() == [0.0] * j + [1.0] + [2.0] * (U - j - 1)
    assert np.array_equal(tt.bits64(l1[:j + 1]), tt.bits64(l0[:j + 1]))
    assert np.array_equal(tt.bits64(d1[:j + 1, :4]), tt.bits64(d0[:j + 1, :4]))
    assert np.isnan(l1[j + 1:]).all() and l1[j + 1:].size == U - j - 1 > 0
    assert np.isnan(d1[j + 1:, :4]).all()
    if max_norm:
        # the norms of the applied updates; the cells of the others stay untouched
        assert np.array_equal(tt.bits64(n1[:j]), tt.bits64(n0[:j])) and (n1[j:] == -1.0).all()
    # a third run of exactly j updates through actor_update
    third = tc.setup(pkg, w, data, mode)
    ppo3, buf3, par3, adams3 = third
    for k in range(j):
        lo, hi = bounds[k % B]
        lk = ppo3.actor_update(buf3, lo, hi, adams3["actor"], max_grad_norm=max_norm)
        assert tt.bits64(float(lk)) == tt.bits64(l1[k]), k
    (s1, b1), (s3, b3) = actor_state(s), actor_state(third)
    assert s1["actor count"] == j
    not_grad = lambda d: {k: v for k, v in d.items() if not k.startswith("grad ")}
    tad.assert_same_bits(not_grad(s1), not_grad(s3))
    assert np.array_equal(b1, b3)               # count, step scalars, the coefficient cell
    # .grad is the gradient of minibatch j mod B at those parameters, unclipped
    lo, hi = bounds[j % B]
    lj = ppo3.actor_loss_grad(buf3, lo, hi)
    assert tt.bits64(float(lj)) == tt.bits64(l1[j])
    for k in pp.ACTOR_PARAMS:
        assert np.array_equal(tad.bits(s1["grad " + k]), tad.bits(tg.np_(par3[k].grad))), k


@pytest.mark.parametrize("mode", MODES)
def test_a_stop_at_the_first_update_leaves_the_entry_state(pkg, mode):
    w, data = stop_case("small")
    U = STOP_EPOCHS * 2
    fresh = actor_state(tc.setup(pkg, w, data, mode))
    _, _, d0, _, _ = run_stop(pkg, w, data, mode, None, math.inf)
    for what in ("target below kl[0]", "nan", "clipped"):
        data1 = data
        if what == "nan":
            # a row of the first minibatch that is well inside the clip range
            mb = {k: v[0:2].double() for k, v in data.items()}
            ratio = kr.diagnostics({k: v.double() for k, v in w.items()}, mb, EPSILON)["ratio"]
            i = int(torch.nonzero((ratio - 1).abs() < 0.5 * EPSILON)[0])
            data1 = dict(data, log_probs=data["log_probs"].clone())
            data1["log_probs"].view(-1)[i] = math.nan
        max_norm = tc.PATH_MAX_NORM if what == "clipped" else None
        target = 0.5 * d0[0, 2] if what != "nan" else 1e300
        s, l1, d1, stop1, n1 = run_stop(pkg, w, data1, mode, max_norm, target)
        assert stop1 == [1, 0], what
        assert d1[:, 4].tolist() == [1.0] + [2.0] * (U - 1), what
        assert np.isnan(l1[1:]).all() and np.isnan(d1[1:, :4]).all(), what
        state, block = actor_state(s)
        assert state["actor count"] == 0 and not block.any(), what
        for k, v in state.items():
            if not k.startswith("grad "):
                assert np.array_equal(tad.bits(v), tad.bits(fresh[0][k])), (what, k)
        if what == "nan":
            assert math.isnan(d1[0, 2]) and math.isnan(l1[0])
            assert d1[0, 3] > d0[0, 3]          # the NaN ratio counts as outside
        else:
            assert np.array_equal(tt.bits64(d1[0, :4]), tt.bits64(d0[0, :4])), what
            assert any(s1.any() for k, s1 in state.items() if k.startswith("grad actor"))
        if max_norm:
            assert (n1 == -1.0).all()
        # monitor only never stops, a NaN KL included
        if what == "nan":
            s, l2, d2, stop2, _ = run_stop(pkg, w, data1, mode, None, math.inf)
            assert stop2 == [0, -1] and (d2[:, 4] == 0.0).all()
            assert actor_state(s)[0]["actor count"] == U


def test_a_second_call_on_the_same_cell_starts_with_a_clean_flag(pkg):
    w, data = stop_case("small")
    s = tc.setup(pkg, w, data, "reference")
    U = STOP_EPOCHS * 2
    diag, stop = cells(U * 5).view(U, 5), cells(2, torch.int64, 7)
    phase(pkg, s, target_kl=1e-300, diag_out=diag, stop_out=stop)
    assert stop.tolist() == [1, 0] and actor_state(s)[0]["actor count"] == 0
    l2 = phase(pkg, s, target_kl=1e300, diag_out=diag, stop_out=stop)
    assert stop.tolist() == [0, -1] and np.isfinite(l2).all()
    assert (tg.np_(diag)[:, 4] == 0.0).all() and actor_state(s)[0]["actor count"] == U
    # and it is the unmonitored phase from the same start
    plain = tc.setup(pkg, w, data, "reference")
    lp = phase(pkg, plain)
    assert np.array_equal(tt.bits64(l2), tt.bits64(lp))
    tad.assert_same_bits(actor_state(s)[0], actor_state(plain)[0])


# ------------------------------------------------------ 4. no sync, and capture
def test_a_captured_monitored_phase_replays_as_the_eager_phases(pkg):
    T, P, A, O, H, seed = OTHER_SHAPES["capture"]
    w, data = tt.case(T + 1, P, A, O, H, seed)
    assert pkg.minibatch_bounds(T + 1, T) == [(0, T)]
    U, replays = 5, 2
    # a target under the first record KL of the first phase, update j: the
    # second phase starts at the parameters that update was evaluated at, on
    # the same minibatch, and so stops at its first update
    probe = tc.setup(pkg, w, data, "reference")
    pd = cells(U * 5).view(U, 5)
    pkg.training.train_phase(probe[0], probe[1], probe[3]["actor"], "actor", U, T, diag_out=pd)
    kl = tg.np_(pd)[:, 2]
    record = [j for j in range(1, U) if kl[j] > kl[:j].max()]
    assert record, kl
    j = record[0]
    target = math.sqrt(kl[:j].max() * kl[j])

    def run(s, out):
        ppo, buf, par, adams = s
        pkg.training.train_phase(ppo, buf, adams["actor"], "actor", U, T, out=out["loss"],
                                 target_kl=target, diag_out=out["diag"], stop_out=out["stop"])

    new_out = lambda: {"loss": cells(U), "diag": cells(U * 5).view(U, 5),
                       "stop": cells(2, torch.int64, 7)}
    eager, eager_out = tc.setup(pkg, w, data, "reference"), new_out()
    stops = []
    for _ in range(replays):
        run(eager, eager_out)
        stops.append(eager_out["stop"].tolist())
    assert stops == [[1, j], [1, 0]], stops
    cap, cap_out = tc.setup(pkg, w, data, "reference"), new_out()
    ppo, buf, par, adams = cap
    start = {k: p.detach().clone() for k, p in par.items()}
    start_sd = adams["actor"].state_dict()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(cap, cap_out)                            # warm-up: workspace, code objects
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for k, p in par.items():
            p.copy_(start[k])
    adams["actor"].load_state_dict(start_sd)
    assert adams["actor"].step_count() == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(cap, cap_out)
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()
    tad.assert_same_bits(actor_state(cap)[0], actor_state(eager)[0])
    assert np.array_equal(actor_state(cap)[1], actor_state(eager)[1])
    assert actor_state(cap)[0]["actor count"] == j
    for k in cap_out:
        a, b = tg.np_(cap_out[k]).astype(np.float64), tg.np_(eager_out[k]).astype(np.float64)
        assert np.array_equal(tt.bits64(a), tt.bits64(b)), k


# ------------------------------------------------------------- 5. MAPPO, CLI
P5, A5, O5, H5, BL, BS, NE = 67, 3, 3, 50, 4, 2, 2


def make_mappo(pkg, out_dir, target_kl=None, log_diagnostics=False, max_grad_norm=None):
    import test_rollout_gpu as tr
    args = cli_args(num_parallel=P5, num_agents=A5, num_obstacles=O5, episode_len=2,
                    risk_factor=2.0, distance_factor=3.0, hidden_size=H5, buffer_len=BL,
                    batch_size=BS, num_epochs=NE, learning_rate=tt.LR, num_total=2 * BL * P5)
    args.target_kl, args.log_diagnostics, args.max_grad_norm = (target_kl, log_diagnostics,
                                                               max_grad_norm)
    env = tr.make_env(pkg, P5, A5, O5, seed=21, normalizer=False, scaler=False)
    torch.manual_seed(11)
    params = pkg.set_model_params(args, DEV)
    assert ("target_kl" in params) == (target_kl is not None)
    assert ("log_diagnostics" in params) == bool(log_diagnostics)
    return pkg.MAPPO(params, env, seed=5, out_dir=str(out_dir)), args


NEW_KEYS = ("actor_approx_kl", "actor_clip_frac", "actor_entropy", "actor_surrogate",
            "actor_status", "actor_stopped_at")


def test_trainer_with_a_target_equals_the_hand_assembled_loop(pkg, tmp_path):
    U = NE * len(pkg.minibatch_bounds(BL, BS))
    # the KLs of the two rollouts' updates, monitor only, to place the target
    m0, _ = make_mappo(pkg, tmp_path / "monitor", log_diagnostics=True)
    assert m0.target_kl is None and m0._monitored
    m0.run(2)
    logs0 = m0.logs()
    assert logs0["actor_status"] == [0] * (2 * U) and logs0["actor_stopped_at"] == [-1, -1]
    later = sorted(x for i, x in enumerate(logs0["actor_approx_kl"]) if i % U)
    assert len(later) == 2 * (U - 1) and later[0] > 0 and later[-1] > 1.5 * later[0], later
    target = math.sqrt(later[0] * later[-1])

    m, args = make_mappo(pkg, tmp_path / "kl", target_kl=target, log_diagnostics=True)
    assert m.target_kl == target and m._diag_log.shape[1:] == (U, 5)
    s = tt.hand_loop(pkg, args, P5, A5, O5, H5)
    rows, stops = [], []
    before = torch.cuda.get_sync_debug_mode()
    for r in range(2):
        torch.cuda.set_sync_debug_mode("error")
        try:
            m.repeat()
        finally:
            torch.cuda.set_sync_debug_mode(before)
        mean, stats = pkg.collect_fused(s["env"], s["policy"], s["buffer"], gamma=args.gamma)
        s["logs"]["mean_rews"].append(float(mean))
        s["logs"]["epi"].append(stats)
        diag, stop = cells(U * 5).view(U, 5), cells(2, torch.int64, 7)
        loss = pkg.training.train_phase(s["ppo"], s["buffer"], s["adam_a"], "actor", NE, BS,
                                        target_kl=target, diag_out=diag, stop_out=stop)
        s["logs"]["actor"] += tt.losses(loss).tolist()
        rows.append(tg.np_(diag).copy())
        stops.append(int(stop[1]))
        pkg.train_critic(s["ppo"], s["buffer"], s["adam_c"], NE, BS, log=s["logs"]["critic"])
        tt.assert_trainer_equals_loop(m, s, r + 1)
    logs = m.logs()
    want = np.concatenate(rows)
    assert sorted(logs) == sorted(("actor", "critic", "epi_stats", "mean_rews") + NEW_KEYS)
    for i, key in enumerate(("actor_surrogate", "actor_entropy", "actor_approx_kl",
                             "actor_clip_frac")):
        assert len(logs[key]) == 2 * U == len(logs["actor"])
        assert np.array_equal(tt.bits64(logs[key]), tt.bits64(want[:, i])), key
    assert logs["actor_status"] == [int(x) for x in want[:, 4]]
    assert all(isinstance(x, int) for x in logs["actor_status"] + logs["actor_stopped_at"])
    assert logs["actor_stopped_at"] == stops and len(stops) == 2
    print(target, logs["actor_approx_kl"], logs["actor_status"], stops)
    # the target lies inside the KLs seen: something was applied, something stopped
    assert 0 in logs["actor_status"] and 1 in logs["actor_status"] and max(stops) >= 1
    for r in range(2):
        st = logs["actor_status"][r * U:(r + 1) * U]
        assert re.fullmatch("0*(12*)?", "".join(map(str, st))), st
        assert all(math.isnan(logs["actor"][r * U + k]) == (st[k] == 2) for k in range(U))
    # run(2) is the two repeats; save_stats leaves the four extra CSVs
    m2, _ = make_mappo(pkg, tmp_path / "kl2", target_kl=target, log_diagnostics=True)
    m2.run(2)
    tad.assert_same_bits(
        tt.trainer_state(m2.actor, m2.critic, m2.actor_optimizer, m2.critic_optimizer),
        tt.trainer_state(m.actor, m.critic, m.actor_optimizer, m.critic_optimizer))
    files = m2.save_stats({"model": "x"}, plot=False)
    assert len(files) == 9
    assert sorted(f[len(m2._time):] for f in os.listdir(tmp_path / "kl2" / "logs")) == [
        "_act_clipfrac.csv", "_act_entropy.csv", "_act_kl.csv", "_act_loss.csv", "_act_stop.csv",
        "_cri_loss.csv", "_epi_stats.csv", "_mean_rews.csv", "_params.json"]


def test_repeat_with_a_target_and_a_clip_does_not_synchronise(pkg, tmp_path):
    m, _ = make_mappo(pkg, tmp_path, target_kl=1e-5, max_grad_norm=0.5)
    assert not m.log_diagnostics and m._monitored
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
    U = NE * 2
    assert len(logs["actor_approx_kl"]) == 2 * U == len(logs["actor_grad_norm"])
    assert len(logs["actor_stopped_at"]) == 2 and set(logs["actor_status"]) <= {0, 1, 2}
    assert all(math.isfinite(x) for x in logs["mean_rews"] + logs["critic"])
    for k, st in enumerate(logs["actor_status"]):
        assert math.isnan(logs["actor"][k]) == (st == 2), (k, st)


def test_cli_train_with_the_flags_writes_the_new_files(pkg, tmp_path, capsys):
    base = ["--train", "-se", "3", "-np", "8", "-bl", "4", "-bs", "2", "-ne", "2", "-nt", "64",
            "-el", "3", "--no-plots"]
    rc = pkg.cli.main(base + ["--target-kl", "0.02", "--log-diagnostics", "--out-dir",
                              str(tmp_path / "kl")])
    assert rc == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["repeats"] == 2 and len(res["files"]) == 9
    U = 2 * 2
    for tail, head, n in (("_act_kl.csv", "Value", 2 * U), ("_act_clipfrac.csv", "Value", 2 * U),
                          ("_act_entropy.csv", "Value", 2 * U), ("_act_stop.csv", "Stopped", 2)):
        rows = open([f for f in res["files"] if f.endswith(tail)][0]).read().split("\n")
        rows = [r.strip() for r in rows if r.strip()]
        assert rows[0].startswith(head) and len(rows) == 1 + n, (tail, rows)
    assert open([f for f in res["files"] if f.endswith("_act_stop.csv")][0]).read().split(
        "\n")[0].strip() == "Stopped at"
    # without the flags: exactly today's set
    rc = pkg.cli.main(base + ["--out-dir", str(tmp_path / "plain")])
    assert rc == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert len(json.loads(line)["files"]) == 5
    assert len(os.listdir(tmp_path / "plain" / "logs")) == 5
    assert pkg.cli.main(base + ["--target-kl", "0", "--out-dir", str(tmp_path / "bad")]) == 2
    assert "target_kl" in capsys.readouterr().err
