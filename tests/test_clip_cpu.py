"""Global-norm gradient clipping in the device update, without a GPU
(include/marlnav.h ``marlnav_grad_norm_work_size``,
``marlnav_adam_step_clipped``, ``marlnav_ppo_*_update_clipped``,
``marlnav_ppo_train_phase_clipped``; ``--max-grad-norm``): the library exports
the new entry points under the unchanged ABI version and state size, every
refusal comes before any HIP call and names the field, tests/clip_ref.py
agrees with an independent per-thread loop, ``set_model_params`` is the dict of
before without the flag, and ``write_stats`` writes the two norm CSVs only for
a run that has them.

Nothing here gets past validation: the pointers are fake, and a call that
passed every check would launch on them. ``+inf`` is shown to be accepted by
the refusal of a field that is checked after ``max_norm``."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import clip_ref as cr
import test_adam_cpu as ta
import test_train_cpu as tt

FAKE = ta.FAKE
SYMBOLS = ("marlnav_grad_norm_work_size", "marlnav_adam_step_clipped",
           "marlnav_ppo_actor_update_clipped", "marlnav_ppo_critic_update_clipped",
           "marlnav_ppo_train_phase_clipped")
WORK, OUT = FAKE * 400, FAKE * 401


def _ref(x):
    return None if x is None else ctypes.byref(x)


def test_library_exports_the_clipped_entry_points(pkg):
    lib = pkg.abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert s in pkg.abi.EXPORTS and hasattr(lib, s)
        assert f" T {s}" in out
    assert pkg.abi.ABI_VERSION == 5 and lib.marlnav_abi_version() == 5
    # the coefficient travels in the state block's spare 8 bytes: no new size,
    # so every checkpoint and every FusedAdam allocation stays as it is
    assert lib.marlnav_adam_state_size() == 32


def test_work_size_is_one_partial_per_block_of_256_items(pkg):
    lib = pkg.abi.load_library()
    for sizes, want in (((1,), 1), ((1023,), 1), ((1024,), 1), ((1025,), 2),
                        ((262144,), 256), ((262145,), 257),
                        ((1, 3, 4, 5, 255, 257, 1024, 70001), 70),   # 17 891 items
                        ((600, 50, 100, 2, 100, 2), 1)):
        d, _ = ta._good_adam(pkg, sizes)
        items = sum((n + 3) // 4 for n in sizes)
        assert want == (items + 255) // 256
        assert lib.marlnav_grad_norm_work_size(ctypes.byref(d)) == want, sizes
    assert lib.marlnav_grad_norm_work_size(None) < 0
    d, _ = ta._good_adam(pkg)
    d.numel[1] = 0
    assert lib.marlnav_grad_norm_work_size(ctypes.byref(d)) < 0
    assert b"numel[1]" in lib.marlnav_last_error()
    d, _ = ta._good_adam(pkg)
    d.num_tensors = 9
    assert lib.marlnav_grad_norm_work_size(ctypes.byref(d)) < 0
    assert b"num_tensors" in lib.marlnav_last_error()


# ------------------------------------------------------------ the four calls
def _step(pkg, d, b, max_norm=0.5, work=WORK, out=OUT):
    lib = pkg.abi.load_library()
    rc = lib.marlnav_adam_step_clipped(_ref(d), _ref(b), max_norm, work, out, None)
    return rc, lib.marlnav_last_error()


def _update(pkg, which, d, b, ad, ab, max_norm=0.5, work=WORK, out=OUT):
    lib = pkg.abi.load_library()
    if which == "actor":
        rc = lib.marlnav_ppo_actor_update_clipped(_ref(d), _ref(b), 0.01, 0.001, _ref(ad),
                                                  _ref(ab), 0, max_norm, work, out, None)
    else:
        rc = lib.marlnav_ppo_critic_update_clipped(_ref(d), _ref(b), 0.01, _ref(ad), _ref(ab),
                                                   max_norm, work, out, None)
    return rc, lib.marlnav_last_error()


def _phase(pkg, a, max_norm=0.5, work=WORK, log=OUT, mode=0):
    lib = pkg.abi.load_library()
    rc = lib.marlnav_ppo_train_phase_clipped(
        a["network"], _ref(a["d"]), _ref(a["b"]), a["bounds"], a["B"], a["E"], 0.01, 0.001,
        _ref(a["ad"]), _ref(a["ab"]), a["log"], mode, max_norm, work, log, None)
    return rc, lib.marlnav_last_error()


def _calls(pkg):
    """(name, call(**clip arguments) -> (rc, message), name of the norm
    output) for the clipped step, both updates and both phases, each with
    arguments that pass every other check."""
    d, b = ta._good_adam(pkg)
    yield "step", lambda **kw: _step(pkg, d, b, **kw), "out", b"norm_out"
    for which in ("actor", "critic"):
        u = ta._good_update(pkg, which)[:4]
        yield which + " update", (lambda u=u, which=which, **kw: _update(pkg, which, *u, **kw)), \
            "out", b"norm_out"
        a = tt._good_phase(pkg, which)
        yield which + " phase", (lambda a=a, **kw: _phase(pkg, a, **kw)), "log", b"norm_log"


@pytest.mark.parametrize("bad", [0.0, -0.0, -0.5, -math.inf, math.nan])
def test_a_bad_max_norm_is_refused_with_its_name(pkg, bad):
    for name, call, _, _ in _calls(pkg):
        rc, msg = call(max_norm=bad)
        assert rc == -1 and b"max_norm" in msg, (name, rc, msg)
        with pytest.raises(RuntimeError, match="max_norm"):
            pkg.abi.check(rc)


def test_norm_pointers_are_checked_with_their_names(pkg):
    for name, call, out_kw, out_name in _calls(pkg):
        rc, msg = call(work=None)
        assert rc == -1 and b"norm_work" in msg and b"NULL" in msg, (name, msg)
        rc, msg = call(work=WORK + 4)
        assert rc == -1 and b"norm_work" in msg and b"aligned" in msg, (name, msg)
        rc, msg = call(**{out_kw: OUT + 4})
        assert rc == -1 and out_name in msg and b"aligned" in msg, (name, msg)


def test_infinity_and_a_null_norm_output_pass_the_clip_checks(pkg):
    """+inf means "record the norm, clip nothing" and norm_out / norm_log may
    be NULL: with either, the refusal is that of a field checked later."""
    for name, call, out_kw, out_name in _calls(pkg):
        rc, msg = call(max_norm=math.inf, **{out_kw: OUT + 4})
        assert rc == -1 and out_name in msg and b"max_norm" not in msg, (name, msg)
    # the gradient half checks its data pointers after the clip arguments
    for which in ("actor", "critic"):
        d, b, ad, ab, _ = ta._good_update(pkg, which)
        b.returns = None
        for kw in ({"max_norm": math.inf}, {"out": None}, {"max_norm": 1e30}):
            rc, msg = _update(pkg, which, d, b, ad, ab, **kw)
            assert rc == -1 and b"returns" in msg and b"NULL" in msg, (which, kw, msg)
        a = tt._good_phase(pkg, which)
        a["b"].obs = None
        rc, msg = _phase(pkg, a, max_norm=math.inf, log=None)
        assert rc == -1 and b"obs" in msg and b"NULL" in msg, (which, msg)


def test_the_clipped_calls_make_their_counterparts_checks(pkg):
    # the Adam step's
    d, b = ta._good_adam(pkg)
    d.beta2 = 1.0
    rc, msg = _step(pkg, d, b)
    assert rc == -1 and b"beta2" in msg
    d, b = ta._good_adam(pkg)
    b.grad[3] = None
    rc, msg = _step(pkg, d, b)
    assert rc == -1 and b"grad[3] is NULL" in msg
    assert _step(pkg, None, b)[0] == -1 and _step(pkg, d, None)[0] == -1
    for which in ("actor", "critic"):
        other = "critic" if which == "actor" else "actor"
        # a table that is not the network's
        d, b, _, _, _ = ta._good_update(pkg, which)
        _, _, ad, ab, _ = ta._good_update(pkg, other)
        rc, msg = _update(pkg, which, d, b, ad, ab)
        assert rc == -1 and b"adam table" in msg, msg
        d, b, ad, ab, fields = ta._good_update(pkg, which)
        ab.grad[1] = FAKE * 9
        rc, msg = _update(pkg, which, d, b, ad, ab)
        assert rc == -1 and b"adam table" in msg and b"grad[1]" in msg, msg
        d, b, ad, ab, _ = ta._good_update(pkg, which)
        d.hidden_size = 513
        rc, msg = _update(pkg, which, d, b, ad, ab)
        assert rc == -1 and b"hidden_size" in msg, msg
        # the phase's
        a = tt._good_phase(pkg, which)
        o = tt._good_phase(pkg, other)
        a["ad"], a["ab"] = o["ad"], o["ab"]
        rc, msg = _phase(pkg, a)
        assert rc == -1 and b"adam table" in msg, msg
        a = tt._good_phase(pkg, which, pairs=((0, 3), (3, 3)))
        rc, msg = _phase(pkg, a)
        assert rc == -1 and b"bounds[1]" in msg, msg
        a = tt._good_phase(pkg, which)
        a["log"] = None
        rc, msg = _phase(pkg, a)
        assert rc == -1 and b"loss_log" in msg, msg
        a = tt._good_phase(pkg, which)
        rc, msg = _phase(pkg, a, mode=2)
        assert rc == -1 and b"advantage_mode" in msg, msg
    d, b, ad, ab, _ = ta._good_update(pkg, "actor")
    lib = pkg.abi.load_library()
    rc = lib.marlnav_ppo_actor_update_clipped(_ref(d), _ref(b), 0.01, 0.001, _ref(ad), _ref(ab), 7,
                                              0.5, WORK, OUT, None)
    assert rc == -1 and b"advantage_mode" in lib.marlnav_last_error()


# ------------------------------------------------------------------ clip_ref
def _thread_loop_norm(slots):
    """The reduction written as the threads run it, one Python float at a
    time: an independent check of clip_ref's array form."""
    items = []
    for g in slots:
        x = [float(v) for v in np.asarray(g, np.float32).reshape(-1)]
        for e0 in range(0, len(x), 4):
            acc = 0.0
            for v in x[e0:e0 + 4]:
                acc += v * v
            items.append(acc)

    def block(vals):                      # 256 values, one per thread
        waves = []
        for w in range(4):
            v = list(vals[64 * w:64 * w + 64])
            off = 32
            while off:
                v = [v[i] + (v[i + off] if i + off < 64 else v[i]) for i in range(64)]
                off //= 2
            waves.append(v[0])
        t = 0.0
        for w in waves:
            t += w
        return t

    items += [0.0] * (-len(items) % 256)
    partials = [block(items[i:i + 256]) for i in range(0, len(items), 256)]
    acc = [0.0] * 256
    for i, p in enumerate(partials):
        acc[i % 256] += p
    return math.sqrt(block(acc)), len(partials)


@pytest.mark.parametrize("sizes", [(1,), (3,), (1023,), (1024,), (1025,), (5, 255, 257, 1024, 2049),
                                   (262145,)])
def test_clip_ref_is_the_per_thread_loop(sizes):
    gen = np.random.default_rng(sum(sizes))
    slots = [(gen.standard_normal(n) * 10.0 ** gen.integers(-3, 2)).astype(np.float32)
             for n in sizes]
    want, blocks = _thread_loop_norm(slots)
    assert cr.block_partials(slots).size == blocks
    # the partition is the library's: one partial per block of its scratch
    import marlnav_amd as pkg
    d, _ = ta._good_adam(pkg, sizes)
    assert pkg.abi.load_library().marlnav_grad_norm_work_size(ctypes.byref(d)) == blocks
    assert cr.norm(slots) == want
    exact = math.sqrt(math.fsum(float(v) ** 2 for g in slots for v in g))
    assert abs(want - exact) <= 1e-13 * exact


def test_clip_ref_coefficient_and_stored_gradient(pkg):
    """The helper's coefficient over the values the library's validation
    (``check_max_grad_norm``, as ``marlnav_*_clipped``) lets through."""
    for ok in (0.5, 1e30, math.inf):
        assert pkg.rollout.check_max_grad_norm(ok) == ok
    assert cr.coef(2.0, 0.5) == 0.5 / (2.0 + 1e-6)
    assert cr.coef(0.4, 0.5) == 1.0 and cr.coef(0.0, 0.5) == 1.0
    assert cr.coef(0.5, 0.5) < 1.0            # torch's 1e-6: a norm AT max_norm is scaled
    assert cr.coef(1e300, math.inf) == 1.0
    assert math.isnan(cr.coef(math.nan, 0.5)) and math.isnan(cr.coef(math.inf, math.inf))
    g = np.array([1.5, -0.0, 2.0 ** -130, -7.25], np.float32)
    assert np.array_equal(cr.clipped(g, 1.0).view(np.uint32), g.view(np.uint32))
    assert np.array_equal(cr.clipped(g, 0.5), np.array([0.75, -0.0, 2.0 ** -131, -3.625], np.float32))


# ------------------------------------------------------- params, CLI, trainer
def test_set_model_params_adds_max_grad_norm_only_when_given(pkg):
    args = pkg.default_args(num_parallel=4, buffer_len=10, batch_size=5, num_total=400)
    base = pkg.set_model_params(args, "cuda")
    assert "max_grad_norm" not in base
    args.max_grad_norm = None
    assert pkg.set_model_params(args, "cuda") == base
    parsed = pkg.cli.build_parser().parse_args(["--train", "-np", "4", "-bl", "10", "-bs", "5",
                                                "-nt", "400"])
    assert parsed.max_grad_norm is None and pkg.set_model_params(parsed, "cuda") == base
    args.max_grad_norm = 0.5
    assert pkg.set_model_params(args, "cuda") == dict(base, max_grad_norm=0.5)
    args.gae_lambda = 0.95                     # the two options compose
    assert pkg.set_model_params(args, "cuda") == dict(base, max_grad_norm=0.5, gae_lambda=0.95)
    args.max_grad_norm = math.inf
    assert pkg.set_model_params(args, "cuda")["max_grad_norm"] == math.inf
    for bad in (0.0, -1.0, math.nan):
        args.max_grad_norm = bad
        with pytest.raises(ValueError, match="max_grad_norm"):
            pkg.set_model_params(args, "cuda")


def test_cli_parses_and_validates_max_grad_norm(pkg, capsys):
    cli = pkg.cli
    args = cli.build_parser().parse_args(["--train", "--max-grad-norm", "0.5", "--gae-lambda",
                                          "0.9"])
    assert args.train and args.max_grad_norm == 0.5 and args.gae_lambda == 0.9
    assert cli.build_parser().parse_args(["--train"]).max_grad_norm is None
    if not torch.cuda.is_available():
        assert cli.main(["--train", "--max-grad-norm", "0.5"]) == 1
        assert "HIP device" in capsys.readouterr().err


@pytest.mark.parametrize("bad", [0.0, -2.0, math.nan])
def test_mappo_and_the_loops_refuse_a_bad_max_grad_norm(pkg, bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        pkg.MAPPO({"max_grad_norm": bad}, None)
    with pytest.raises(ValueError, match="max_grad_norm"):
        pkg.rollout.check_max_grad_norm(bad)
    assert pkg.rollout.check_max_grad_norm(math.inf) == math.inf


def test_write_stats_writes_the_norm_logs_only_when_they_exist(pkg, tmp_path):
    logs = {"epi_stats": {"trunc": [1, 0], "col": [2, 3], "tar": [0, 4]},
            "mean_rews": [-1.5, -1.25], "actor": [0.1, 0.2, 0.3, 0.4],
            "critic": [1.0, 0.5, 0.25, 0.125]}
    plain = pkg.training.write_stats(logs, {"a": 1}, str(tmp_path / "plain"), "S", plot=False)
    assert sorted(os.listdir(tmp_path / "plain" / "logs")) == [
        "S_act_loss.csv", "S_cri_loss.csv", "S_epi_stats.csv", "S_mean_rews.csv", "S_params.json"]
    assert len(plain) == 5
    clipped = dict(logs, actor_grad_norm=[3.0, 2.5, 2.0, 1.5], critic_grad_norm=[9.0, 8.0, 7.0, 6.0])
    files = pkg.training.write_stats(clipped, {"a": 1}, str(tmp_path / "clip"), "S", plot=False)
    assert files[:5] == [p.replace("plain", "clip") for p in plain] and len(files) == 7
    assert sorted(os.listdir(tmp_path / "clip" / "logs")) == [
        "S_act_gnorm.csv", "S_act_loss.csv", "S_cri_gnorm.csv", "S_cri_loss.csv",
        "S_epi_stats.csv", "S_mean_rews.csv", "S_params.json"]
    rows = open(tmp_path / "clip" / "logs" / "S_act_gnorm.csv").read().split()
    assert rows == ["Value", "3.0", "2.5", "2.0", "1.5"]
    rows = open(tmp_path / "clip" / "logs" / "S_cri_gnorm.csv").read().split()
    assert rows == ["Value", "9.0", "8.0", "7.0", "6.0"]
    for name in ("S_act_loss.csv", "S_params.json"):
        assert open(tmp_path / "clip" / "logs" / name).read() == \
            open(tmp_path / "plain" / "logs" / name).read()


def test_the_fold_hook_defaults_to_the_measured_decision(pkg):
    lib = pkg.abi.load_library()
    assert "marlnav_debug_clip_fold" in pkg.abi.EXPORTS
    header = open(ta.HEADER).read()
    default = int(header.split("#define MARLNAV_CLIP_FOLD_DEFAULT")[1].split()[0])
    assert default in (0, 1)
    assert lib.marlnav_debug_clip_fold(-1) == default        # any other value only queries
    assert lib.marlnav_debug_clip_fold(7) == default
    assert lib.marlnav_debug_clip_fold(1 - default) == default
    assert lib.marlnav_debug_clip_fold(default) == 1 - default
    assert lib.marlnav_debug_clip_fold(-1) == default


def test_the_python_keywords_exist(pkg):
    import inspect
    for f in (pkg.FusedAdam.step, pkg.FusedPPO.actor_update, pkg.FusedPPO.critic_update):
        p = inspect.signature(f).parameters
        assert p["max_grad_norm"].default is None and p["norm_out"].default is None, f
    for f in (pkg.train_actor, pkg.train_critic):
        p = inspect.signature(f).parameters
        assert p["max_grad_norm"].default is None and p["norm_log"].default is None, f
    p = inspect.signature(pkg.training.train_phase).parameters
    assert p["max_grad_norm"].default is None and p["norm_out"].default is None
