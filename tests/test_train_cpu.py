"""The device training mode without a GPU (include/marlnav.h
``marlnav_ppo_train_phase``, ``marlnav_ppo_train_work_size``,
``marlnav_params_snapshot_if``; marl-nav_amd/training.py; ``--train``): the
library exports the entry points under the unchanged ABI version, every
validation fails before any HIP call and names the field, ``set_model_params``
keeps the reference's layout and validations, the modules' state dicts are what
the fused classes expect, the CLI returns 1 without a device, and the stats
files carry the reference's names and headers."""
import csv
import ctypes
import json
import math
import os
import subprocess

import pytest
import torch

import test_adam_cpu as ta

FAKE = ta.FAKE
SYMBOLS = ("marlnav_ppo_train_phase", "marlnav_ppo_train_work_size", "marlnav_params_snapshot_if")


def test_library_exports_the_training_entry_points(pkg):
    lib = pkg.abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert s in pkg.abi.EXPORTS and hasattr(lib, s)
        assert f" T {s}" in out
    assert "marlnav_internal" not in out            # the fold's hand-over stays inside
    assert pkg.abi.ABI_VERSION == 5 and lib.marlnav_abi_version() == 5
    assert (pkg.abi.NETWORK_ACTOR, pkg.abi.NETWORK_CRITIC) == (0, 1)
    assert pkg.abi.SNAPSHOT_MAX_TENSORS == 10
    for name in ("MAPPO", "Actor", "Critic", "set_model_params", "training"):
        assert name in pkg.__all__ and hasattr(pkg, name)


# ------------------------------------------------------------- the phase call
def _bounds(pairs):
    flat = [x for p in pairs for x in p]
    return (ctypes.c_int64 * max(1, len(flat)))(*flat), len(pairs)


def _good_phase(pkg, which, steps=6, pairs=((0, 3), (3, 5))):
    d, b, ad, ab, fields = ta._good_update(pkg, which)
    d.num_steps = steps
    arr, B = _bounds(pairs)
    return {"network": 0 if which == "actor" else 1, "d": d, "b": b, "bounds": arr, "B": B,
            "E": 2, "ad": ad, "ab": ab, "log": FAKE * 300}


def _phase(pkg, a):
    lib = pkg.abi.load_library()
    ref = lambda x: None if x is None else ctypes.byref(x)
    rc = lib.marlnav_ppo_train_phase(a["network"], ref(a["d"]), ref(a["b"]), a["bounds"], a["B"],
                                     a["E"], 0.01, 0.001, ref(a["ad"]), ref(a["ab"]), a["log"],
                                     None)
    return rc, lib.marlnav_last_error()


def _refused(pkg, a, *words):
    rc, msg = _phase(pkg, a)
    assert rc == -1, (rc, msg)
    for w in words:
        assert w in msg, (msg, w)
    with pytest.raises(RuntimeError):
        pkg.abi.check(rc)


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_phase_refuses_bad_bounds_counts_and_log(pkg, which):
    a = _good_phase(pkg, which)
    a["network"] = 2
    _refused(pkg, a, b"network")
    for pairs, word in ((((0, 3), (3, 3)), b"bounds[1]"),      # empty
                        (((0, 3), (4, 3)), b"bounds[1]"),      # reversed
                        (((-1, 3),), b"bounds[0]"),            # below the buffer
                        (((0, 3), (3, 5), (5, 7)), b"bounds[2]")):   # past its 6 steps
        a = _good_phase(pkg, which, pairs=pairs)
        _refused(pkg, a, word)
    a = _good_phase(pkg, which)
    a["B"] = 0
    _refused(pkg, a, b"num_batches")
    a = _good_phase(pkg, which)
    a["bounds"] = None
    _refused(pkg, a, b"bounds", b"NULL")
    for E in (0, -3):
        a = _good_phase(pkg, which)
        a["E"] = E
        _refused(pkg, a, b"num_epochs")
    a = _good_phase(pkg, which)
    a["log"] = None
    _refused(pkg, a, b"loss_log", b"NULL")
    a = _good_phase(pkg, which)
    a["log"] = FAKE + 4
    _refused(pkg, a, b"loss_log", b"aligned")


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_phase_refuses_a_foreign_adam_table(pkg, which):
    other = "critic" if which == "actor" else "actor"
    a = _good_phase(pkg, which)
    o = _good_phase(pkg, other)
    a["ad"], a["ab"] = o["ad"], o["ab"]
    _refused(pkg, a, b"adam table")
    a = _good_phase(pkg, which)
    a["ab"].param[1] = FAKE * 9
    _refused(pkg, a, b"adam table", b"param[1]")
    a = _good_phase(pkg, which)
    a["ab"].grad[0] = FAKE * 9
    _refused(pkg, a, b"adam table", b"grad[0]")
    a = _good_phase(pkg, which)
    a["ad"].numel[2] += 1
    _refused(pkg, a, b"adam table", b"numel[2]")


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_phase_validates_dims_adam_and_buffers_before_any_launch(pkg, which):
    a = _good_phase(pkg, which)
    a["d"].hidden_size = 513
    _refused(pkg, a, b"hidden_size")
    a = _good_phase(pkg, which)
    a["d"] = None
    _refused(pkg, a, b"dims")
    a = _good_phase(pkg, which)
    a["b"] = None
    _refused(pkg, a, b"buffers")
    a = _good_phase(pkg, which)
    a["ad"].beta2 = 1.0
    _refused(pkg, a, b"beta2")
    a = _good_phase(pkg, which)
    a["ab"].state = None
    _refused(pkg, a, b"state")
    a = _good_phase(pkg, which)
    a["ad"] = None
    _refused(pkg, a)
    for field in ("obs", "values", "returns", "work") + (("actions", "log_probs")
                                                        if which == "actor" else ()):
        a = _good_phase(pkg, which)
        setattr(a["b"], field, None)
        _refused(pkg, a, field.encode(), b"NULL")
    # a minibatch of one env row (T * P < 2) is refused as the update calls refuse it
    a = _good_phase(pkg, which, pairs=((0, 1), (1, 5)))
    a["d"].num_parallel = 1
    _refused(pkg, a, b"fewer than 2 env rows")


def test_train_work_size_covers_the_largest_minibatch(pkg):
    lib = pkg.abi.load_library()
    a = _good_phase(pkg, "critic", steps=9, pairs=((0, 2), (2, 9), (3, 4)))
    d = a["d"]
    d.num_parallel = 700
    got = lib.marlnav_ppo_train_work_size(ctypes.byref(d), a["bounds"], a["B"])
    each = []
    for T in (2, 7, 1):
        one = pkg.abi.MarlnavPpoDims(num_parallel=700, num_steps=T, num_agents=3, obs_dim=12,
                                     hidden_size=50)
        each.append(lib.marlnav_ppo_work_size(ctypes.byref(one)))
    assert got == max(each) > 0
    arr, B = _bounds(((0, 10),))
    assert lib.marlnav_ppo_train_work_size(ctypes.byref(d), arr, B) == -1
    assert b"bounds[0]" in lib.marlnav_last_error()
    assert lib.marlnav_ppo_train_work_size(ctypes.byref(d), None, 1) == -1
    assert lib.marlnav_ppo_train_work_size(None, arr, 1) == -1


# --------------------------------------------------------------- the snapshot
def _good_snapshot(n=10):
    P = ctypes.c_void_p
    return {"n": n, "src": (P * 10)(*[FAKE * (2 + i) for i in range(10)]),
            "dst": (P * 10)(*[FAKE * (40 + i) for i in range(10)]),
            "numel": (ctypes.c_int64 * 10)(*range(1, 11)), "mean": FAKE * 80, "max": FAKE * 81,
            "state": FAKE * 82, "repeat": 0, "track": 0}


def _snapshot(pkg, a):
    lib = pkg.abi.load_library()
    rc = lib.marlnav_params_snapshot_if(a["n"], a["src"], a["dst"], a["numel"], a["mean"],
                                        a["max"], a["state"], a["repeat"], a["track"], None)
    return rc, lib.marlnav_last_error()


def test_snapshot_validation_names_the_field(pkg):
    def refused(word, **change):
        a = _good_snapshot()
        for k, v in change.items():
            if isinstance(v, tuple):
                a[k][v[0]] = v[1]
            else:
                a[k] = v
        rc, msg = _snapshot(pkg, a)
        assert rc == -1 and word in msg, (rc, msg, word)

    refused(b"num_tensors", n=0)
    refused(b"num_tensors", n=11)
    refused(b"src is NULL", src=None)
    refused(b"dst is NULL", dst=None)
    refused(b"numel is NULL", numel=None)
    refused(b"numel[3]", numel=(3, 0))
    refused(b"src[9] is NULL", src=(9, None))
    refused(b"dst[0] is NULL", dst=(0, None))
    refused(b"src[2] must be 4-byte aligned", src=(2, FAKE + 2))
    refused(b"dst[4] must be 4-byte aligned", dst=(4, FAKE + 1))
    refused(b"mean_rew is NULL", mean=None)
    refused(b"max_rew is NULL", max=None)
    refused(b"save_state is NULL", state=None)
    refused(b"8-byte aligned", mean=FAKE + 4)
    refused(b"8-byte aligned", state=FAKE + 4)
    refused(b"repeat_index", repeat=-1)
    refused(b"track_best", track=2)
    # slots past num_tensors are not read
    a = _good_snapshot(n=4)
    a["src"][7] = None
    a["numel"][5] = -1
    a["dst"][1] = None
    rc, msg = _snapshot(pkg, a)
    assert rc == -1 and b"dst[1]" in msg, msg


# ---------------------------------------------------------- set_model_params
def test_set_model_params_layout_and_validations(pkg):
    args = pkg.default_args(num_parallel=4, buffer_len=10, batch_size=5, num_total=400,
                            num_epochs=3, hidden_size=7)
    p = pkg.set_model_params(args, "cuda")
    assert set(p) == {"actor", "critic", "num_agents", "device", "lr", "ent_const", "epsilon",
                      "gamma", "num_total", "num_parallel", "buffer_len", "num_epochs",
                      "batch_size", "action_size", "normalizer", "scaler"}
    assert p["actor"] == {"input_size": 12, "hidden_size": 7}           # 3 x 3: the reference's 12
    assert p["critic"] == {"input_size": 36, "hidden_size": 7}
    assert (p["lr"], p["ent_const"], p["epsilon"], p["gamma"]) == (0.001, 0.001, 0.01, 0.9)
    assert (p["num_total"], p["buffer_len"], p["num_epochs"], p["batch_size"]) == (400, 10, 3, 5)
    assert p["action_size"] == 2 and p["device"] == "cuda" and p["num_agents"] == 3
    assert p["normalizer"] == pkg.set_normalizer_params(args, "cuda")
    assert p["scaler"] == pkg.set_scaler_params(args, "cuda")
    # the observation size follows the shape: 2 + 2 O + 2 (A - 1)
    for A, O in ((3, 8), (16, 32), (2, 127)):
        args = pkg.default_args(num_agents=A, num_obstacles=O, num_parallel=2, buffer_len=5,
                                batch_size=5, num_total=10)
        p = pkg.set_model_params(args, "cuda")
        D = 2 + 2 * O + 2 * (A - 1)
        assert p["actor"]["input_size"] == D and p["critic"]["input_size"] == A * D
    with pytest.raises(ValueError, match="batch_size can't be greater than buffer_len"):
        pkg.set_model_params(pkg.default_args(buffer_len=4, batch_size=5, num_parallel=1,
                                              num_total=4), "cuda")
    with pytest.raises(ValueError, match="divisible"):
        pkg.set_model_params(pkg.default_args(buffer_len=4, batch_size=2, num_parallel=3,
                                              num_total=100), "cuda")


# ------------------------------------------------------------------- modules
@pytest.mark.parametrize("A,O,H", [(3, 3, 50), (16, 32, 7), (2, 127, 3)])
def test_module_state_dicts_are_what_the_fused_classes_expect(pkg, A, O, H):
    D = 2 + 2 * O + 2 * (A - 1)
    torch.manual_seed(3)
    actor, critic = pkg.Actor(D, H), pkg.Critic(A * D, H)
    sa, sc = actor.state_dict(), critic.state_dict()
    assert tuple(sa) == pkg.evaluation.STATE_DICT_KEYS == pkg.training.ACTOR_KEYS
    assert tuple(sc) == pkg.training.CRITIC_KEYS
    want = {"fc1.weight": (H, D), "fc1.bias": (H,), "fc_mu.weight": (2, H), "fc_mu.bias": (2,),
            "fc_std.weight": (2, H), "fc_std.bias": (2,)}
    assert {k: tuple(v.shape) for k, v in sa.items()} == want
    assert {k: tuple(v.shape) for k, v in sc.items()} == {
        "fc1.weight": (H, A * D), "fc1.bias": (H,), "fc2.weight": (1, H), "fc2.bias": (1,)}
    # parameters() in the order of the C tables (rollout._POLICY_PARAMS)
    order = [getattr(getattr({"actor": actor, "critic": critic}[m], layer), attr)
             for _, m, layer, attr in pkg.rollout._POLICY_PARAMS]
    assert all(a is b for a, b in zip(order, list(actor.parameters()) + list(critic.parameters())))
    # and the fused classes refuse them only for being on the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.rollout._module_params(actor, critic, "test")
    # orthogonal init: the smaller side of every weight is orthonormal
    for w in (actor.fc1.weight, actor.fc_mu.weight, actor.fc_std.weight, critic.fc1.weight,
              critic.fc2.weight):
        w = w.detach().double()
        g = w @ w.T if w.shape[0] <= w.shape[1] else w.T @ w
        assert torch.allclose(g, torch.eye(g.shape[0], dtype=torch.float64), atol=1e-5)
    # the forward passes of DESIGN.md §9
    x = torch.rand(5, A, D) * 2 - 1
    dist = actor(x)
    h = x.flatten(0, 1) @ actor.fc1.weight.T + actor.fc1.bias
    assert torch.allclose(dist.loc, torch.tanh(h @ actor.fc_mu.weight.T + actor.fc_mu.bias))
    var = torch.nn.functional.softplus(h @ actor.fc_std.weight.T + actor.fc_std.bias)
    assert torch.allclose(torch.diagonal(dist.covariance_matrix, dim1=1, dim2=2), var)
    assert critic(x).shape == (5, 1)


def test_actor_state_dict_loads_where_the_reference_keys_are_checked(pkg):
    """FusedActor.from_state_dict checks keys and shapes before it needs the
    device: a dict of this Actor gets past them (to the device refusal), one
    with a missing key does not."""
    sd = pkg.Actor(12, 5).state_dict()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.FusedActor.from_state_dict(sd, "cpu")
    bad = dict(sd)
    del bad["fc_std.bias"]
    with pytest.raises(ValueError, match="fc_std.bias"):
        pkg.FusedActor.from_state_dict(bad, "cpu")


# ----------------------------------------------------------------------- CLI
def test_cli_train_needs_a_device_and_the_other_modes_stay(pkg, capsys):
    cli = pkg.cli
    args = cli.build_parser().parse_args(["--train", "--track-best", "--save-every", "3",
                                          "--no-plots", "--out-dir", "x"])
    assert args.train and args.track_best and args.save_every == 3 and args.no_plots
    assert args.out_dir == "x"
    assert not cli.build_parser().parse_args([]).train
    if torch.cuda.is_available():
        return                      # with a device --train trains: tests/test_train_gpu.py
    assert cli.main(["--train"]) == 1
    assert "HIP device" in capsys.readouterr().err
    assert cli.main([]) == 2 and cli.main(["-re"]) == 2


# --------------------------------------------------------------------- stats
def test_write_stats_file_names_and_headers(pkg, tmp_path):
    logs = {"epi_stats": {"trunc": [4, 0], "col": [1, 2], "tar": [0, 7]},
            "mean_rews": [-1.5, 0.25], "actor": [0.5, 0.25, 0.125, 1.0],
            "critic": [2.0, 1.0, 0.5, 0.25]}
    full = {"model": {"lr": 0.001, "device": "cuda"}, "env": {"num_parallel": 2,
                                                             "init": {"x": math.pi}}}
    stamp = "20260102030405"
    files = pkg.training.write_stats(logs, full, str(tmp_path), stamp, plot=False)
    names = sorted(os.path.relpath(f, tmp_path) for f in files)
    assert names == sorted(os.path.join("logs", stamp + s) for s in (
        "_params.json", "_mean_rews.csv", "_act_loss.csv", "_cri_loss.csv", "_epi_stats.csv"))
    assert not (tmp_path / "plots").exists()
    rows = lambda name: list(csv.reader(open(tmp_path / "logs" / (stamp + name), newline="")))
    assert rows("_mean_rews.csv") == [["Value"], ["-1.5"], ["0.25"]]
    assert rows("_act_loss.csv") == [["Value"], ["0.5"], ["0.25"], ["0.125"], ["1.0"]]
    assert rows("_cri_loss.csv") == [["Value"], ["2.0"], ["1.0"], ["0.5"], ["0.25"]]
    assert rows("_epi_stats.csv") == [["Truncated", "Collisions", "Target reached"],
                                      ["4", "1", "0"], ["0", "2", "7"]]
    text = (tmp_path / "logs" / (stamp + "_params.json")).read_text()
    assert json.loads(text) == full
    assert text == json.dumps(full, indent=4, sort_keys=True)
    # the figures, under the reference's names
    files = pkg.training.write_stats(logs, full, str(tmp_path), stamp, plot=True)
    plots = sorted(os.path.basename(f) for f in files if f.endswith(".png"))
    assert plots == sorted(stamp + s for s in ("_mean_rews.png", "_act_loss.png",
                                               "_cri_loss.png", "_epi_stats.png"))
    for f in files:
        assert os.path.getsize(f) > 0
    paths = pkg.training.stats_paths(str(tmp_path), stamp)
    assert os.path.relpath(paths["actor"], tmp_path) == os.path.join("weights",
                                                                     stamp + "_actor.pt")
    assert os.path.relpath(paths["critic"], tmp_path) == os.path.join("weights",
                                                                      stamp + "_critic.pt")
