"""The actor phase's diagnostics and target-KL stop without a GPU (DESIGN.md
§17; include/marlnav.h ``marlnav_ppo_actor_grad_diag``,
``marlnav_ppo_train_phase_monitored`` and the two diagnostic work-size queries;
``--target-kl`` / ``--log-diagnostics``): the library exports the entry points
and refuses bad arguments before any launch, tests/kl_ref.py is consistent
with itself, the Python layers refuse what the library refuses, ``write_stats``
adds its files only where the keys exist, and every shape of
tests/test_kl_gpu.py is pinned to the launch path it is there for."""
import csv
import ctypes
import inspect
import math
import os
import subprocess

import pytest
import torch

import kl_ref as kr
import ppo_ref as pp
import test_adam_cpu as ta
import test_kl_gpu as tk
import test_ppo_cpu as tpc
import test_ppo_gpu as tg
import test_train_cpu as tt

FAKE = ta.FAKE
SYMBOLS = ("marlnav_ppo_actor_grad_diag", "marlnav_ppo_train_phase_monitored",
           "marlnav_ppo_diag_work_size", "marlnav_ppo_train_diag_work_size")
DIAG, STOP = FAKE * 500, FAKE * 501


def _ref(x):
    return None if x is None else ctypes.byref(x)


def test_library_exports_the_diagnostic_entry_points(pkg):
    lib = pkg.abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert s in pkg.abi.EXPORTS and hasattr(lib, s)
        assert f" T {s}" in out
    assert "marlnav_internal" not in out
    assert pkg.abi.ABI_VERSION == 5 and lib.marlnav_abi_version() == 5
    header = open(ta.HEADER).read()
    assert int(header.split("#define MARLNAV_DIAG_ROW")[1].split()[0]) == pkg.abi.DIAG_ROW == 5
    assert float(header.split("#define MARLNAV_MAX_NORM_NONE")[1].split()[0]) == \
        pkg.abi.MAX_NORM_NONE == 0.0
    assert len(kr.ROW) == pkg.abi.DIAG_ROW


# ------------------------------------------------------------- the work sizes
def _dims(pkg, T, P, A, O, H):
    return pkg.abi.MarlnavPpoDims(num_parallel=P, num_steps=T, num_agents=A,
                                  obs_dim=2 + 2 * O + 2 * (A - 1), hidden_size=H)


def test_the_diagnostic_work_size_adds_two_columns_to_the_actor_rows(pkg):
    lib = pkg.abi.load_library()
    shapes = [s[:5] for s in tg.SHAPES.values()] + [s[:5] for s in tk.DIAG_SHAPES.values()]
    # test_ppo_cpu's sweep: the narrow critics among it are smaller than the actor's rows
    shapes += [(1, N, A, O, H) for A, O in tpc.SWEEP_AD.values() for H in tpc.SWEEP_H
               for N in tpc.SWEEP_N]
    grew = 0
    for s in shapes:
        plan = pp.launch_plan(*s)
        D = 2 + 2 * s[3] + 2 * (s[2] - 1)
        actor = plan["actor"]["blocks"] * (4 * (D + 1) + 2 + 2)
        d = _dims(pkg, *s)
        plain = lib.marlnav_ppo_work_size(ctypes.byref(d))
        assert plain == plan["work_size"]
        got = lib.marlnav_ppo_diag_work_size(ctypes.byref(d))
        assert got == max(plain, actor) >= plain, s
        grew += got > plain
    assert grew >= 1
    assert lib.marlnav_ppo_diag_work_size(None) < 0
    d = _dims(pkg, 2, 3, 3, 3, 513)
    assert lib.marlnav_ppo_diag_work_size(ctypes.byref(d)) < 0
    assert b"hidden_size" in lib.marlnav_last_error()
    # the phase's query: the largest minibatch, the plain query's refusals
    a = tt._good_phase(pkg, "actor", steps=9, pairs=((0, 2), (2, 9), (3, 4)))
    d = a["d"]
    d.num_parallel = 700
    got = lib.marlnav_ppo_train_diag_work_size(ctypes.byref(d), a["bounds"], a["B"])
    each = [lib.marlnav_ppo_diag_work_size(ctypes.byref(_dims(pkg, T, 700, 3, 3, 50)))
            for T in (2, 7, 1)]
    assert got == max(each) >= lib.marlnav_ppo_train_work_size(ctypes.byref(d), a["bounds"], a["B"])
    arr, B = tt._bounds(((0, 10),))
    assert lib.marlnav_ppo_train_diag_work_size(ctypes.byref(d), arr, B) == -1
    assert b"bounds[0]" in lib.marlnav_last_error()
    assert lib.marlnav_ppo_train_diag_work_size(ctypes.byref(d), None, 1) == -1
    assert lib.marlnav_ppo_train_diag_work_size(None, arr, 1) == -1


# ------------------------------------------------------------- the two calls
def _grad_diag(pkg, d, b, diag=DIAG, mode=0):
    lib = pkg.abi.load_library()
    rc = lib.marlnav_ppo_actor_grad_diag(_ref(d), _ref(b), 0.01, 0.001, mode, diag, None)
    return rc, lib.marlnav_last_error()


def _phase(pkg, a, max_norm=0.0, work=None, norm_log=None, target_kl=0.02, diag=DIAG, stop=STOP,
           mode=0):
    lib = pkg.abi.load_library()
    rc = lib.marlnav_ppo_train_phase_monitored(
        a["network"], _ref(a["d"]), _ref(a["b"]), a["bounds"], a["B"], a["E"], 0.01, 0.001,
        _ref(a["ad"]), _ref(a["ab"]), a["log"], mode, max_norm, work, norm_log, target_kl, diag,
        stop, None)
    return rc, lib.marlnav_last_error()


def test_grad_diag_refuses_what_the_plain_call_refuses_and_a_bad_diag(pkg):
    d, b, _, _, _ = ta._good_update(pkg, "actor")
    rc, msg = _grad_diag(pkg, d, b, diag=None)
    assert rc == -1 and b"diag" in msg and b"NULL" in msg
    rc, msg = _grad_diag(pkg, d, b, diag=DIAG + 4)
    assert rc == -1 and b"diag" in msg and b"aligned" in msg
    rc, msg = _grad_diag(pkg, d, b, mode=2)
    assert rc == -1 and b"advantage_mode" in msg
    assert _grad_diag(pkg, None, b)[0] == -1 and _grad_diag(pkg, d, None)[0] == -1
    for field in ("obs", "actions", "log_probs", "values", "returns", "work", "loss",
                  "grad_actor_mu_w"):
        d, b, _, _, _ = ta._good_update(pkg, "actor")
        setattr(b, field, None)
        rc, msg = _grad_diag(pkg, d, b)
        assert rc == -1 and field.encode() in msg and b"NULL" in msg, (field, msg)
    d, b, _, _, _ = ta._good_update(pkg, "actor")
    b.values = None                         # the own-env pairing reads no values
    rc, msg = _grad_diag(pkg, d, b, diag=None, mode=1)
    assert rc == -1 and b"diag" in msg
    d.hidden_size = 513
    rc, msg = _grad_diag(pkg, d, b)
    assert rc == -1 and b"hidden_size" in msg


@pytest.mark.parametrize("bad", [0.0, -0.0, -0.5, -math.inf, math.nan])
def test_a_bad_target_kl_is_refused_with_its_name(pkg, bad):
    rc, msg = _phase(pkg, tt._good_phase(pkg, "actor"), target_kl=bad)
    assert rc == -1 and b"target_kl" in msg, msg
    with pytest.raises(RuntimeError, match="target_kl"):
        pkg.abi.check(rc)


def test_the_monitored_phase_names_what_it_refuses(pkg):
    good = lambda: tt._good_phase(pkg, "actor")
    rc, msg = _phase(pkg, tt._good_phase(pkg, "critic"))
    assert rc == -1 and b"MARLNAV_NETWORK_CRITIC" in msg and b"actor" in msg, msg
    a = good()
    a["network"] = 2
    rc, msg = _phase(pkg, a)
    assert rc == -1 and b"network" in msg
    for kw, words in (({"diag": None}, (b"diag_log", b"NULL")),
                      ({"diag": DIAG + 4}, (b"diag_log", b"aligned")),
                      ({"stop": None}, (b"stop", b"NULL")),
                      ({"stop": STOP + 4}, (b"stop", b"aligned")),
                      ({"mode": 2}, (b"advantage_mode",)),
                      # the clip's conventions: a value that is neither the no-clip one nor > 0
                      ({"max_norm": -1.0, "work": FAKE * 400}, (b"max_norm",)),
                      ({"max_norm": math.nan, "work": FAKE * 400}, (b"max_norm",)),
                      ({"max_norm": 0.5}, (b"norm_work", b"NULL")),
                      ({"max_norm": 0.5, "work": FAKE * 400 + 4}, (b"norm_work", b"aligned")),
                      ({"max_norm": 0.5, "work": FAKE * 400, "norm_log": FAKE * 401 + 4},
                       (b"norm_log", b"aligned")),
                      ({"work": FAKE * 400}, (b"MARLNAV_MAX_NORM_NONE",)),
                      ({"norm_log": FAKE * 401}, (b"MARLNAV_MAX_NORM_NONE",))):
        rc, msg = _phase(pkg, good(), **kw)
        assert rc == -1, (kw, msg)
        for word in words:
            assert word in msg, (kw, msg)
    # and its counterpart's checks
    a = good()
    a["log"] = None
    rc, msg = _phase(pkg, a)
    assert rc == -1 and b"loss_log" in msg and b"NULL" in msg
    a = good()
    a["log"] = FAKE + 4
    rc, msg = _phase(pkg, a)
    assert rc == -1 and b"loss_log" in msg and b"aligned" in msg
    a = tt._good_phase(pkg, "actor", pairs=((0, 3), (3, 3)))
    rc, msg = _phase(pkg, a)
    assert rc == -1 and b"bounds[1]" in msg
    a = good()
    a["E"] = 0
    rc, msg = _phase(pkg, a)
    assert rc == -1 and b"num_epochs" in msg
    a = good()
    o = tt._good_phase(pkg, "critic")
    a["ad"], a["ab"] = o["ad"], o["ab"]
    rc, msg = _phase(pkg, a)
    assert rc == -1 and b"adam table" in msg
    for field in ("obs", "actions", "log_probs", "values", "returns", "work"):
        a = good()
        setattr(a["b"], field, None)
        rc, msg = _phase(pkg, a, target_kl=math.inf)      # +inf: monitor only, a valid target
        assert rc == -1 and field.encode() in msg and b"NULL" in msg, (field, msg)


# ------------------------------------------------------------------- kl_ref
def test_the_reference_is_consistent_with_itself():
    """approx_kl >= 0 in float64 (x - 1 - log x >= 0) and exactly 0 for the
    rollout's own policy; the clip fraction counts what it says; the loss is
    the surrogate plus the weighted entropy, in both pairings."""
    for shape in ((2, 3, 3, 3, 50, 7), (2, 5, 16, 32, 16, 2)):
        w, data = tg.make_case(*shape)
        w64 = {k: v.double() for k, v in w.items()}
        d64 = {k: v.double() for k, v in data.items()}
        for own in (False, True):
            t = kr.diagnostics(w64, d64, tg.EPSILON, own)
            assert t["approx_kl"] > 0.0 and 0 < t["outside"] < t["ratio"].numel()
            assert t["clip_frac"] == t["outside"] / t["ratio"].numel()
            assert t["outside"] == int(((t["ratio"] - 1).abs() > tg.EPSILON).sum())
            assert (((t["ratio"] - 1) - torch.log(t["ratio"])) >= 0).all()
            if not own:
                loss = pp.actor_loss(w64, d64["obs"], d64["actions"], d64["log_probs"],
                                     d64["values"], d64["returns"], tg.EPSILON, tg.ENT_CONST)
                want = t["surrogate_mean"] + tg.ENT_CONST * t["entropy_mean"]
                assert abs(float(loss) - want) <= 1e-15 * abs(want)
        # the policy that produced the log-probs: every ratio is exactly 1
        new_lp, _ = pp.actor_terms(w64, d64["obs"], d64["actions"])
        same = dict(d64, log_probs=new_lp.reshape(d64["log_probs"].shape))
        t = kr.diagnostics(w64, same, tg.EPSILON)
        assert t["approx_kl"] == 0.0 and t["outside"] == 0 and t["clip_frac"] == 0.0
        # the two pairings share everything but the surrogate
        a, b = kr.diagnostics(w64, d64, tg.EPSILON, False), kr.diagnostics(w64, d64, tg.EPSILON, True)
        assert all(a[k] == b[k] for k in ("entropy_mean", "approx_kl", "clip_frac"))
        assert a["surrogate_mean"] != b["surrogate_mean"]


def test_the_stop_rule_on_hand_made_lists():
    inf, nan = math.inf, math.nan
    assert kr.stop_rule([1.0, 2.0, 3.0], 2.5) == ([0, 0, 1], 2)
    assert kr.stop_rule([1.0, 3.0, 0.5, 9.0], 2.5) == ([0, 1, 2, 2], 1)
    assert kr.stop_rule([3.0, 1.0], 2.5) == ([1, 2], 0)
    assert kr.stop_rule([2.5, 2.5], 2.5) == ([0, 0], -1)           # > target, not >=
    assert kr.stop_rule([1.0, 2.0], 5.0) == ([0, 0], -1)
    assert kr.stop_rule([1.0, nan, 1.0], 5.0) == ([0, 1, 2], 1)    # a NaN is not <= target
    assert kr.stop_rule([nan], 5.0) == ([1], 0)
    assert kr.stop_rule([1.0, inf], 1e300) == ([0, 1], 1)
    assert kr.stop_rule([1.0, inf, nan], inf) == ([0, 0, 0], -1)   # monitor only: never
    assert kr.stop_rule([], 1.0) == ([], -1)


# -------------------------------------------------- params, CLI, the trainer
def test_set_model_params_adds_the_keys_only_when_given(pkg):
    args = pkg.default_args(num_parallel=4, buffer_len=10, batch_size=5, num_total=400)
    base = pkg.set_model_params(args, "cuda")
    assert "target_kl" not in base and "log_diagnostics" not in base
    args.target_kl, args.log_diagnostics = None, False
    assert pkg.set_model_params(args, "cuda") == base
    parsed = pkg.cli.build_parser().parse_args(["--train", "-np", "4", "-bl", "10", "-bs", "5",
                                                "-nt", "400"])
    assert parsed.target_kl is None and parsed.log_diagnostics is False
    assert pkg.set_model_params(parsed, "cuda") == base
    args.target_kl = 0.02
    assert pkg.set_model_params(args, "cuda") == dict(base, target_kl=0.02)
    args.log_diagnostics = True
    args.max_grad_norm, args.gae_lambda = 0.5, 0.95            # the options compose
    assert pkg.set_model_params(args, "cuda") == dict(base, target_kl=0.02, log_diagnostics=True,
                                                      max_grad_norm=0.5, gae_lambda=0.95)
    args.target_kl = None
    assert pkg.set_model_params(args, "cuda") == dict(base, log_diagnostics=True,
                                                      max_grad_norm=0.5, gae_lambda=0.95)
    for bad in (0.0, -1.0, math.nan):
        args.target_kl = bad
        with pytest.raises(ValueError, match="target_kl"):
            pkg.set_model_params(args, "cuda")


def test_cli_parses_and_validates_the_flags(pkg, capsys):
    cli = pkg.cli
    args = cli.build_parser().parse_args(["--train", "--target-kl", "0.02", "--log-diagnostics",
                                          "--max-grad-norm", "0.5"])
    assert args.train and args.target_kl == 0.02 and args.log_diagnostics
    assert args.max_grad_norm == 0.5
    assert "--target-kl" in cli.__doc__ and "--log-diagnostics" in cli.__doc__
    if not torch.cuda.is_available():
        assert cli.main(["--train", "--target-kl", "0.02"]) == 1
        assert "HIP device" in capsys.readouterr().err


@pytest.mark.parametrize("bad", [0.0, -2.0, math.nan])
def test_mappo_and_the_phase_refuse_a_bad_target_kl(pkg, bad):
    with pytest.raises(ValueError, match="target_kl"):
        pkg.MAPPO({"target_kl": bad}, None)
    with pytest.raises(ValueError, match="target_kl"):
        pkg.rollout.check_target_kl(bad)
    with pytest.raises(ValueError, match="target_kl"):
        pkg.training.train_phase(None, None, None, "actor", 1, 1, target_kl=bad)
    assert pkg.rollout.check_target_kl(math.inf) == math.inf
    assert pkg.rollout.check_target_kl(0.02) == 0.02


def test_the_critic_has_no_diagnostics(pkg):
    for kw in ({"target_kl": 0.02}, {"diag_out": torch.zeros(5, dtype=torch.float64)},
               {"stop_out": torch.zeros(2, dtype=torch.int64)}):
        for critic in ("critic", pkg.abi.NETWORK_CRITIC):
            with pytest.raises(ValueError, match="critic"):
                pkg.training.train_phase(None, None, None, critic, 1, 1, **kw)


def test_a_bad_diag_out_is_refused(pkg):
    cpu = torch.device("cpu")
    check = pkg.rollout.check_diag_out
    check(torch.zeros(5, dtype=torch.float64), cpu)
    check(torch.zeros(3, 5, dtype=torch.float64), cpu, rows=3)
    for bad in (torch.zeros(5), torch.zeros(4, dtype=torch.float64),
                torch.zeros(6, dtype=torch.float64), torch.zeros(10, dtype=torch.float64)[::2],
                [0.0] * 5, None):
        with pytest.raises(ValueError, match="diag_out"):
            check(bad, cpu)
    with pytest.raises(ValueError, match="15 elements"):
        check(torch.zeros(5, dtype=torch.float64), cpu, rows=3)
    with pytest.raises(ValueError, match="diag_out"):
        check(torch.zeros(5, dtype=torch.float64), torch.device("meta"))


def test_the_python_keywords_exist(pkg):
    p = inspect.signature(pkg.training.train_phase).parameters
    assert all(p[k].default is None for k in ("target_kl", "diag_out", "stop_out"))
    for f in (pkg.FusedPPO.actor_loss_grad, pkg.FusedPPO.actor_grad):
        assert inspect.signature(f).parameters["diag_out"].default is None
    assert "1.5" in pkg.training.train_phase.__doc__ and "1.5" in pkg.MAPPO.__doc__


# --------------------------------------------------------------------- stats
def test_write_stats_writes_the_diagnostics_only_when_they_exist(pkg, tmp_path):
    logs = {"epi_stats": {"trunc": [1, 0], "col": [2, 3], "tar": [0, 4]},
            "mean_rews": [-1.5, -1.25], "actor": [0.1, 0.2, math.nan, math.nan],
            "critic": [1.0, 0.5, 0.25, 0.125]}
    plain = pkg.training.write_stats(logs, {"a": 1}, str(tmp_path / "plain"), "S", plot=False)
    today = ["S_act_loss.csv", "S_cri_loss.csv", "S_epi_stats.csv", "S_mean_rews.csv",
             "S_params.json"]
    assert sorted(os.listdir(tmp_path / "plain" / "logs")) == today
    assert [os.path.basename(f) for f in plain] == [
        "S_params.json", "S_mean_rews.csv", "S_act_loss.csv", "S_cri_loss.csv", "S_epi_stats.csv"]
    full = dict(logs, actor_approx_kl=[1e-5, 3e-4, math.nan, math.nan],
                actor_clip_frac=[0.0, 0.25, math.nan, math.nan],
                actor_entropy=[2.5, 2.25, math.nan, math.nan],
                actor_surrogate=[0.5, 0.75, math.nan, math.nan], actor_status=[0, 1, 2, 2],
                actor_stopped_at=[1, -1])
    files = pkg.training.write_stats(full, {"a": 1}, str(tmp_path / "kl"), "S", plot=False)
    assert files[:5] == [p.replace("plain", "kl") for p in plain] and len(files) == 9
    assert sorted(os.listdir(tmp_path / "kl" / "logs")) == sorted(
        today + ["S_act_kl.csv", "S_act_clipfrac.csv", "S_act_entropy.csv", "S_act_stop.csv"])
    rows = lambda name: [r[0] for r in csv.reader(open(tmp_path / "kl" / "logs" / name,
                                                       newline=""))]
    assert rows("S_act_kl.csv") == ["Value", "1e-05", "0.0003", "nan", "nan"]
    assert rows("S_act_clipfrac.csv") == ["Value", "0.0", "0.25", "nan", "nan"]
    assert rows("S_act_entropy.csv") == ["Value", "2.5", "2.25", "nan", "nan"]
    assert rows("S_act_stop.csv") == ["Stopped at", "1", "-1"]
    assert rows("S_act_loss.csv") == ["Value", "0.1", "0.2", "nan", "nan"]
    # the two extras compose; the figures: today's four, and one more with the keys
    both = dict(full, actor_grad_norm=[3.0, 2.5, 0.0, 0.0], critic_grad_norm=[9.0, 8.0, 7.0, 6.0])
    files = pkg.training.write_stats(both, {"a": 1}, str(tmp_path / "both"), "S", plot=True)
    assert len(files) == 5 + 2 + 4 + 4 + 1
    assert [os.path.basename(f) for f in files[-5:]] == [
        "S_mean_rews.png", "S_act_loss.png", "S_cri_loss.png", "S_epi_stats.png", "S_act_kl.png"]
    assert all(os.path.getsize(f) > 0 for f in files)
    files = pkg.training.write_stats(logs, {"a": 1}, str(tmp_path / "plain"), "S", plot=True)
    assert sorted(os.listdir(tmp_path / "plain" / "plots")) == [
        "S_act_loss.png", "S_cri_loss.png", "S_epi_stats.png", "S_mean_rews.png"]
    assert len(files) == 9


# ------------------------------------------------------------- launch paths
def test_every_shape_of_the_gpu_tests_takes_the_path_it_is_there_for():
    plans = {}
    for table in (tk.DIAG_SHAPES, tk.STOP_SHAPES, tk.OTHER_SHAPES):
        for name, shape in table.items():
            a = pp.launch_plan(*shape[:5])["actor"]
            plans[name] = (a["blocks"], a["finish_groups"], a["slices"], a["col_rounds"])
    assert plans == tk.ACTOR_PLANS, plans
    # one block with one partial tile; 9 blocks, the last partial, finish by
    # groups; idle phase-2 threads; several columns per thread, no groups
    T, P, A = tk.DIAG_SHAPES["tiny"][:3]
    assert T * P * A == 18
    T, P, A = tk.DIAG_SHAPES["chunks"][:3]
    assert T * P * A == 8 * 1024 + 208
    assert tk.ACTOR_PLANS["mid_row"][2:] == (1, 1) and tk.ACTOR_PLANS["long_row"][2:] == (1, 2)
    # the stop's two actors lie on either side of the fold limit of the
    # unmonitored phase
    sizes = {}
    for name, (T, P, A, O, H, _) in tk.STOP_SHAPES.items():
        D = 2 + 2 * O + 2 * (A - 1)
        sizes[name] = H * (D + 1) + 4 * H + 4
    assert sizes == {"small": 854, "large": 1620}


@pytest.mark.parametrize("name", list(tk.DIAG_SHAPES))
def test_no_row_of_a_parity_case_lies_at_a_clip_bound(name):
    """The clip fraction is compared exactly: the seeds beside the shapes keep
    every row's float64 ratio GAPS['ratio'] away from 1 -+ epsilon, and the
    float32 evaluation on this host counts the same rows."""
    w, data = tk.diag_case(name)
    truth, ref = tk.references(name, "reference")
    assert kr.ratio_gap(truth["ratio"], tg.EPSILON) >= tg.GAPS["ratio"]
    assert truth["outside"] == ref["outside"] > 0
