"""The GAE(lambda) advantage mode without a GPU (include/
marlnav.h ``marlnav_gae_advantages``, ``marlnav_critic_values``, the three
``marlnav_ppo_*_mode`` calls; ``--gae-lambda``): the library exports the new
entry points under the unchanged ABI version, every refusal comes before any
HIP call and names the field, tests/gae_ref.py agrees with an independent
per-env loop and with three closed forms, ``set_model_params`` is the dict of
before without the flag, and ``MAPPO`` refuses a lambda outside [0, 1]."""
import ctypes
import math
import subprocess

import pytest
import torch

import gae_ref as gr
import test_adam_cpu as ta
import test_train_cpu as tt

FAKE = ta.FAKE
SYMBOLS = ("marlnav_gae_work_size", "marlnav_gae_advantages", "marlnav_critic_values",
           "marlnav_ppo_actor_grad_mode", "marlnav_ppo_actor_update_mode",
           "marlnav_ppo_train_phase_mode")


def test_library_exports_the_gae_entry_points(pkg):
    lib = pkg.abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    import test_abi
    declared = test_abi.declared_functions()
    for s in SYMBOLS:
        assert s in pkg.abi.EXPORTS and hasattr(lib, s) and s in declared
        assert f" T {s}" in out
    assert pkg.abi.ABI_VERSION == 5 and lib.marlnav_abi_version() == 5
    assert (pkg.abi.ADVANTAGE_REFERENCE, pkg.abi.ADVANTAGE_ENV) == (0, 1)
    for P, want in ((1, 2), (256, 2), (257, 4), (1025, 10)):
        assert lib.marlnav_gae_work_size(P) == want == lib.marlnav_returns_work_size(P)
    assert lib.marlnav_gae_work_size(0) == -1


# ------------------------------------------------------------------- the scan
GAE_POINTERS = ("rewards", "done", "values", "last_values", "advantages", "value_targets", "stats",
                "work")


def _gae(pkg, T=4, P=3, gamma=0.9, lam=0.95, **null):
    lib = pkg.abi.load_library()
    p = {n: None if null.get(n) else FAKE * (2 + i) for i, n in enumerate(GAE_POINTERS)}
    rc = lib.marlnav_gae_advantages(p["rewards"], p["done"], p["values"], p["last_values"], T, P,
                                    gamma, lam, p["advantages"], p["value_targets"], p["stats"],
                                    p["work"], None)
    return rc, lib.marlnav_last_error()


@pytest.mark.parametrize("name", GAE_POINTERS)
def test_scan_refuses_a_null_pointer_by_name(pkg, name):
    rc, msg = _gae(pkg, **{name: True})
    assert rc == -1 and name.encode() in msg and b"NULL" in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="NULL"):
        pkg.abi.check(rc)


@pytest.mark.parametrize("kw,word", [
    ({"lam": 1.5}, b"lam"), ({"lam": -0.1}, b"lam"), ({"lam": math.nan}, b"lam"),
    ({"lam": math.inf}, b"lam"),
    ({"gamma": math.nan}, b"gamma"), ({"gamma": 1.01}, b"gamma"), ({"gamma": -1e-9}, b"gamma"),
    ({"gamma": math.inf}, b"gamma"),
    ({"T": 0}, b"T=0"), ({"T": -2}, b"T="), ({"P": 0}, b"P=0"),
    ({"T": 1, "P": 1}, b"fewer than 2")])
def test_scan_refuses_bad_sizes_and_factors(pkg, kw, word):
    rc, msg = _gae(pkg, **kw)
    assert rc == -1 and word in msg, (rc, msg)


# ------------------------------------------------------------------ bootstrap
def test_critic_values_refusals(pkg):
    abi = pkg.abi
    lib = abi.load_library()

    def call(d, b):
        rc = lib.marlnav_critic_values(None if d is None else ctypes.byref(d),
                                       None if b is None else ctypes.byref(b), None)
        return rc, lib.marlnav_last_error()

    def good():
        d = abi.MarlnavPolicyDims(num_parallel=5, num_agents=3, obs_dim=12, hidden_size=50)
        b = abi.MarlnavPolicyBuffers()
        for f in abi.CRITIC_VALUES_REQUIRED:       # the actor side stays NULL
            setattr(b, f, FAKE)
        return d, b

    assert abi.CRITIC_VALUES_REQUIRED == ("obs_norm", "critic_fc1_w", "critic_fc1_b",
                                          "critic_fc2_w", "critic_fc2_b", "values")
    d, b = good()
    assert call(None, b)[0] == -1 and call(d, None)[0] == -1
    for f in abi.CRITIC_VALUES_REQUIRED:
        d, b = good()
        setattr(b, f, None)
        rc, msg = call(d, b)
        assert rc == -1 and b"NULL" in msg, (f, rc, msg)
    for field, value, word in (("num_parallel", 0, b"num_parallel"), ("num_agents", 1, b"num_agents"),
                               ("hidden_size", 513, b"hidden_size"), ("obs_dim", 13, b"obs_dim"),
                               ("reserved", 1, b"reserved")):
        d, b = good()
        setattr(d, field, value)
        rc, msg = call(d, b)
        assert rc == -1 and word in msg, (field, rc, msg)


# ---------------------------------------------------------------- the pairing
def _ref(x):
    return None if x is None else ctypes.byref(x)


def test_mode_calls_refuse_a_bad_mode_and_need_no_values_in_env_mode(pkg):
    lib = pkg.abi.load_library()
    for mode in (2, -1):
        d, b, ad, ab, _ = ta._good_update(pkg, "actor")
        assert lib.marlnav_ppo_actor_grad_mode(_ref(d), _ref(b), 0.01, 0.001, mode, None) == -1
        assert b"advantage_mode" in lib.marlnav_last_error()
        assert lib.marlnav_ppo_actor_update_mode(_ref(d), _ref(b), 0.01, 0.001, _ref(ad), _ref(ab),
                                                 mode, None) == -1
        assert b"advantage_mode" in lib.marlnav_last_error()
        for which in ("actor", "critic"):
            a = tt._good_phase(pkg, which)
            rc = lib.marlnav_ppo_train_phase_mode(
                a["network"], _ref(a["d"]), _ref(a["b"]), a["bounds"], a["B"], a["E"], 0.01, 0.001,
                _ref(a["ad"]), _ref(a["ab"]), a["log"], mode, None)
            assert rc == -1 and b"advantage_mode" in lib.marlnav_last_error()
    # values: required by the reference pairing, not looked at by the own-env
    # one (the next missing buffer is named instead)
    for mode, word in ((0, b"values"), (1, b"work")):
        d, b, ad, ab, _ = ta._good_update(pkg, "actor")
        b.values, b.work = None, None
        assert lib.marlnav_ppo_actor_grad_mode(_ref(d), _ref(b), 0.01, 0.001, mode, None) == -1
        assert word in lib.marlnav_last_error(), (mode, lib.marlnav_last_error())
        assert lib.marlnav_ppo_actor_update_mode(_ref(d), _ref(b), 0.01, 0.001, _ref(ad), _ref(ab),
                                                 mode, None) == -1
        assert word in lib.marlnav_last_error(), (mode, lib.marlnav_last_error())
        a = tt._good_phase(pkg, "actor")
        a["b"].values, a["b"].work = None, None
        rc = lib.marlnav_ppo_train_phase_mode(
            0, _ref(a["d"]), _ref(a["b"]), a["bounds"], a["B"], a["E"], 0.01, 0.001, _ref(a["ad"]),
            _ref(a["ab"]), a["log"], mode, None)
        assert rc == -1 and word in lib.marlnav_last_error(), (mode, lib.marlnav_last_error())
    # the critic reads values in either mode
    a = tt._good_phase(pkg, "critic")
    a["b"].values = None
    rc = lib.marlnav_ppo_train_phase_mode(
        1, _ref(a["d"]), _ref(a["b"]), a["bounds"], a["B"], a["E"], 0.01, 0.001, _ref(a["ad"]),
        _ref(a["ab"]), a["log"], 1, None)
    assert rc == -1 and b"values" in lib.marlnav_last_error()
    # every other refusal of the existing calls is the mode calls' too
    for mode in (0, 1):
        d, b, ad, ab, _ = ta._good_update(pkg, "actor")
        d.hidden_size = 513
        assert lib.marlnav_ppo_actor_grad_mode(_ref(d), _ref(b), 0.01, 0.001, mode, None) == -1
        assert b"hidden_size" in lib.marlnav_last_error()
        d, b, ad, ab, _ = ta._good_update(pkg, "actor")
        ab.param[1] = FAKE * 9
        assert lib.marlnav_ppo_actor_update_mode(_ref(d), _ref(b), 0.01, 0.001, _ref(ad), _ref(ab),
                                                 mode, None) == -1
        assert b"adam table" in lib.marlnav_last_error()


# ------------------------------------------------------------------- gae_ref
def _loop(rewards, done, values, last, gamma, lam):
    """Per env, in Python floats: the textbook recursion with a 0 / 1 mask
    written as branches."""
    T, P = rewards.shape
    raw = [[0.0] * P for _ in range(T)]
    for p in range(P):
        a_next = 0.0
        for t in reversed(range(T)):
            r, v = float(rewards[t, p]), float(values[t, p])
            nxt = float(last[p]) if t == T - 1 else float(values[t + 1, p])
            if bool(done[t, p]):
                a = r - v
            else:
                a = (r + gamma * nxt) - v + gamma * lam * a_next
            raw[t][p] = a_next = a
    return torch.tensor(raw, dtype=torch.float64)


@pytest.mark.parametrize("gamma,lam", [(0.9, 0.95), (1.0, 1.0), (0.9, 0.0), (0.5, 0.3)])
def test_gae_ref_against_a_per_env_loop(gamma, lam):
    g = torch.Generator().manual_seed(11)
    T, P = 7, 9
    rewards, values = torch.randn(T, P, generator=g), torch.randn(T, P, generator=g)
    last = torch.randn(P, generator=g)
    done = torch.rand(T, P, generator=g) < 0.2
    done[:, 0], done[:, 1], done[T - 1, 2] = True, False, True
    got = gr.gae(rewards, done, values.unsqueeze(-1), last.unsqueeze(-1), gamma, lam)
    raw = _loop(rewards, done, values, last, gamma, lam)
    torch.testing.assert_close(got["raw"], raw, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(got["value_targets"], raw + values.double(), rtol=1e-13, atol=1e-13)
    mean, std = raw.mean(), raw.std(unbiased=True)
    torch.testing.assert_close(got["mean"], mean, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(got["std"], std, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(got["advantages"], (raw - mean) / (std + 1e-12), rtol=1e-12,
                               atol=1e-12)
    # a value behind a done is selected away, not multiplied by zero
    last2 = last.clone()
    last2[0] = math.inf                      # column 0 is done everywhere
    last2[2] = math.nan                      # done in the last row
    again = gr.gae(rewards, done, values, last2, gamma, lam)
    for k in ("raw", "value_targets", "advantages"):
        assert torch.equal(again[k], got[k]), k


def test_gae_ref_closed_forms():
    T, P, gamma = 4, 3, 0.9
    g = torch.Generator().manual_seed(5)
    r, v = torch.randn(T, P, generator=g).double(), torch.randn(T, P, generator=g).double()
    last = torch.randn(P, generator=g).double()
    none = torch.zeros(T, P, dtype=torch.bool)
    # lambda = 0: A_t = delta_t
    got = gr.gae(r, none, v, last, gamma, 0.0)
    nxt = torch.cat([v[1:], last[None]])
    torch.testing.assert_close(got["raw"], r + gamma * nxt - v, rtol=1e-14, atol=1e-14)
    # lambda = 1, no done, V = 0, last = 0: A_t = sum_k gamma^k r_{t+k}
    got = gr.gae(r, none, torch.zeros(T, P), torch.zeros(P), gamma, 1.0)
    want = torch.stack([sum(gamma ** k * r[t + k] for k in range(T - t)) for t in range(T)])
    torch.testing.assert_close(got["raw"], want, rtol=1e-14, atol=1e-14)
    torch.testing.assert_close(got["value_targets"], want, rtol=1e-14, atol=1e-14)
    # a done at t cuts the bootstrap and the tail, and keeps r_t
    done = none.clone()
    done[1, 0] = done[3, 1] = True
    got = gr.gae(r, done, v, last, gamma, 0.95)
    full = gr.gae(r, none, v, last, gamma, 0.95)
    assert got["raw"][1, 0] == r[1, 0] - v[1, 0]
    assert got["raw"][3, 1] == r[3, 1] - v[3, 1]
    d0 = (r[0, 0] + gamma * v[1, 0]) - v[0, 0]
    torch.testing.assert_close(got["raw"][0, 0], d0 + gamma * 0.95 * (r[1, 0] - v[1, 0]),
                               rtol=1e-14, atol=1e-14)
    assert torch.equal(got["raw"][2:, 0], full["raw"][2:, 0])      # after the cut: untouched
    assert torch.equal(got["raw"][:, 2], full["raw"][:, 2])        # another env: untouched
    assert got["value_targets"][1, 0] == (r[1, 0] - v[1, 0]) + v[1, 0]


def test_own_env_loss_pairs_each_row_with_its_env():
    """With a single agent row per env differing, only that env's advantage
    matters; the pairing is ppo_ref's ``advantage_of_own_env`` with values 0."""
    import ppo_ref as pp
    c = pp.load_case(pp.case_names()[0])
    w, data = pp.tensors(c, dtype=torch.float64)
    adv = data["returns"]
    got = gr.actor_loss_own_env(w, data["obs"], data["actions"], data["log_probs"], adv, 0.01, 0.001)
    want = pp.actor_loss(w, data["obs"], data["actions"], data["log_probs"],
                         torch.zeros_like(data["values"]), adv, 0.01, 0.001,
                         advantage_of_own_env=True)
    assert float(got) == float(want)
    other = pp.actor_loss(w, data["obs"], data["actions"], data["log_probs"],
                          torch.zeros_like(data["values"]), adv, 0.01, 0.001)
    assert float(got) != float(other)


# ------------------------------------------------------- params, CLI, trainer
def test_set_model_params_adds_gae_lambda_only_when_given(pkg):
    args = pkg.default_args(num_parallel=4, buffer_len=10, batch_size=5, num_total=400)
    base = pkg.set_model_params(args, "cuda")
    assert "gae_lambda" not in base
    args.gae_lambda = None
    assert pkg.set_model_params(args, "cuda") == base
    parsed = pkg.cli.build_parser().parse_args(["--train", "-np", "4", "-bl", "10", "-bs", "5",
                                                "-nt", "400"])
    assert parsed.gae_lambda is None and pkg.set_model_params(parsed, "cuda") == base
    args.gae_lambda = 0.95
    with_flag = pkg.set_model_params(args, "cuda")
    assert with_flag == dict(base, gae_lambda=0.95)


def test_cli_parses_gae_lambda(pkg, capsys):
    cli = pkg.cli
    args = cli.build_parser().parse_args(["--train", "--gae-lambda", "0.95"])
    assert args.train and args.gae_lambda == 0.95
    assert cli.build_parser().parse_args(["--train"]).gae_lambda is None
    if not torch.cuda.is_available():
        assert cli.main(["--train", "--gae-lambda", "0.95"]) == 1
        assert "HIP device" in capsys.readouterr().err


@pytest.mark.parametrize("lam", [1.5, -0.01, math.nan, math.inf])
def test_mappo_and_collect_refuse_a_lambda_outside_the_unit_interval(pkg, lam):
    with pytest.raises(ValueError, match="gae_lambda"):
        pkg.MAPPO({"gae_lambda": lam}, None)
    with pytest.raises(ValueError, match="gae_lambda"):
        pkg.collect(None, None, None, gae_lambda=lam)
    with pytest.raises(ValueError, match="gae_lambda"):
        pkg.collect_fused(None, None, None, gae_lambda=lam)


def test_buffer_drops_the_gae_results_with_the_returns(pkg):
    buf = pkg.RolloutBuffer(3)
    assert buf.advantages is None and buf.value_targets is None
    buf.reserve(2, 3, 12, "cpu")
    for drop in (buf.clear, lambda: buf.commit(3)):
        buf.returns = buf.advantages = buf.value_targets = torch.zeros(3, 2, dtype=torch.float64)
        drop()
        assert buf.returns is None and buf.advantages is None and buf.value_targets is None
    with pytest.raises(ValueError, match="advantage"):
        pkg.FusedPPO(None, None, 0.01, 0.001, advantage="td")
    for name in ("gae_advantages",):
        assert hasattr(pkg.rollout, name)
