"""Actor-only evaluation (include/marlnav.h ``marlnav_actor_act`` /
``marlnav_rollout_evaluate``, marl-nav_amd/evaluation.py) without a GPU: the
new struct matches its ctypes mirror, the library exports the entry points
under the unchanged ABI version, every validation case fails with
MARLNAV_EINVAL and its field named before any HIP call (the pointers below are
never dereferenced), the tracker's rule gives hand-computed figures, and the
Python layer refuses what it must."""
import ctypes
import importlib
import math
import os
import subprocess

import pytest
import torch

import eval_ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "marlnav.h")


# ---------------------------------------------------------------- the C ABI
def test_eval_struct_layout_matches_header(pkg, tmp_path):
    cls = pkg.abi.MarlnavEvalBuffers
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
             'int main(void) {',
             f'printf("size %zu\\n", sizeof({cls.__name__}));',
             'printf("mean %d\\n", MARLNAV_ACT_MEAN);',
             'printf("sample %d\\n", MARLNAV_ACT_SAMPLE);']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cls.__name__}, {fname}));')
    lines.append("return 0; }")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(c), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        field, val = line.split()
        got[field] = int(val)
    assert got.pop("mean") == pkg.abi.ACT_MEAN == 0
    assert got.pop("sample") == pkg.abi.ACT_SAMPLE == 1
    assert got["size"] == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname
    assert [f for f, _ in cls._fields_] == [
        "obs_norm_a", "obs_norm_b", "actions", "reward", "terminated", "truncated",
        "cur_return", "cur_len", "whole", "ep_count", "ret_sum", "ret_sqsum", "ret_min",
        "ret_max", "len_sum", "partial_count", "totals_i", "totals_f", "trace_states",
        "trace_obstacles", "trace_target", "trace_reward", "trace_terminated",
        "trace_truncated", "trace_env", "reserved"]
    assert len(got) == 1 + len(cls._fields_)


def test_library_exports_the_eval_entry_points(pkg):
    lib = pkg.abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for symbol in ("marlnav_actor_act", "marlnav_rollout_evaluate"):
        assert symbol in pkg.abi.EXPORTS and hasattr(lib, symbol)
        assert f" T {symbol}" in out
    assert pkg.abi.ABI_VERSION == 5 and lib.marlnav_abi_version() == 5
    for name in ("FusedActor", "EvalResult", "evaluate"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert hasattr(pkg.abi.load_host().Engine, "evaluate")


class ActorCall(object):
    """A marlnav_actor_act call that passes every check (fake pointers)."""

    def __init__(self, pkg):
        abi = pkg.abi
        self.lib = abi.load_library()
        self.dims = abi.MarlnavPolicyDims(num_parallel=8, num_agents=3, obs_dim=12,
                                          hidden_size=50, env_offset=16)
        self.bufs = abi.MarlnavPolicyBuffers()
        at = 0x10000000
        for f in abi.ACTOR_REQUIRED_FIELDS:
            setattr(self.bufs, f, at)
            at += 0x100000
        self.mode = abi.ACT_MEAN
        self.null = set()

    def __call__(self):
        ref = lambda name: None if name in self.null else ctypes.byref(getattr(self, name))
        rc = self.lib.marlnav_actor_act(ref("dims"), ref("bufs"), self.mode, 0, 0, None)
        return rc, self.lib.marlnav_last_error()


class EvalCall(object):
    """A marlnav_rollout_evaluate call that passes every check: 8 envs x 3
    agents x 3 obstacles (D = 12), 4 steps, env 7 traced, distinct fake
    pointers far apart."""

    def __init__(self, pkg):
        abi = pkg.abi
        self.lib = abi.load_library()
        self.dims = abi.MarlnavDims(num_parallel=8, num_agents=3, num_obstacles=3,
                                    obstacle_stride=3, env_offset=16)
        self.params = abi.MarlnavParams(flags=abi.WRITE_OBS_NORM | abi.SCALE_ACTIONS)
        self.env = abi.MarlnavStepBuffers()
        at = 0x10000000
        for f in abi.STEP_BUFFER_FIELDS:
            if not f.startswith("fresh_"):
                setattr(self.env, f, at)
                at += 0x100000
        self.pdims = abi.MarlnavPolicyDims(num_parallel=8, num_agents=3, obs_dim=12,
                                           hidden_size=50, env_offset=16)
        self.policy = abi.MarlnavPolicyBuffers()
        for f in abi.POLICY_WEIGHT_FIELDS[:6]:
            setattr(self.policy, f, at)
            at += 0x100000
        self.eval = abi.MarlnavEvalBuffers(trace_env=7)
        for f in abi.EVAL_POINTER_FIELDS:
            setattr(self.eval, f, at)
            at += 0x100000
        self.mode = abi.ACT_SAMPLE
        self.T = 4
        self.null = set()

    def __call__(self):
        ref = lambda name: None if name in self.null else ctypes.byref(getattr(self, name))
        rc = self.lib.marlnav_rollout_evaluate(
            ref("dims"), ref("params"), ref("env"), 1, ref("pdims"), ref("policy"), self.mode,
            0, 0, ref("eval"), self.T, None)
        return rc, self.lib.marlnav_last_error()

    def reaches_the_last_check(self):
        """Everything before it passed: the overlap of the two observation
        buffers is the last check there is."""
        self.eval.obs_norm_b = self.eval.obs_norm_a
        refused(self, "obs_norm_b", "overlaps")


def refused(call, *words):
    rc, msg = call()
    assert rc == -1, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_actor_refusals(pkg):
    for which in ("dims", "bufs"):
        c = ActorCall(pkg)
        c.null.add(which)
        refused(c, "NULL")
    for mode in (-1, 2, 7):
        c = ActorCall(pkg)
        c.mode = mode
        refused(c, f"mode={mode}")
    for f in pkg.abi.ACTOR_REQUIRED_FIELDS:
        c = ActorCall(pkg)
        setattr(c.bufs, f, None)
        refused(c, "NULL")
    for field, value in (("num_parallel", 0), ("num_agents", 1), ("num_agents", 65),
                         ("obs_dim", 13), ("obs_dim", 6), ("hidden_size", 0),
                         ("hidden_size", 513), ("reserved", 1), ("env_offset", -1)):
        c = ActorCall(pkg)
        setattr(c.dims, field, value)
        refused(c, field)


@pytest.mark.parametrize("which", ["dims", "params", "env", "pdims", "policy", "eval"])
def test_evaluate_null_structs_are_refused(pkg, which):
    c = EvalCall(pkg)
    c.null.add(which)
    refused(c, which, "NULL")


@pytest.mark.parametrize("mode", [-1, 2])
def test_evaluate_bad_mode_is_refused(pkg, mode):
    c = EvalCall(pkg)
    c.mode = mode
    refused(c, f"mode={mode}", "MARLNAV_ACT_MEAN")


@pytest.mark.parametrize("T", [0, -3])
def test_evaluate_needs_a_step(pkg, T):
    c = EvalCall(pkg)
    c.T = T
    refused(c, "T=")


@pytest.mark.parametrize("trace_env", [8, 9, -2])
def test_evaluate_trace_env_must_be_an_env(pkg, trace_env):
    c = EvalCall(pkg)
    c.eval.trace_env = trace_env
    refused(c, f"trace_env={trace_env}", "num_parallel=8")


def test_evaluate_overlapping_observation_buffers_are_refused(pkg):
    row = 8 * 3 * 12 * 4                       # bytes of one observation buffer
    for delta in (0, 4, row - 4, -(row - 4)):
        c = EvalCall(pkg)
        c.eval.obs_norm_b = c.eval.obs_norm_a + delta
        refused(c, "obs_norm_b", "overlaps")
    for which in ("obs_norm_a", "obs_norm_b"):
        c = EvalCall(pkg)
        setattr(c.eval, which, c.env.obs + row - 4)
        refused(c, "env->obs", "overlaps")
    c = EvalCall(pkg)
    c.env.states_out = c.env.states + 16
    refused(c, "states_out", "overlaps")
    c = EvalCall(pkg)
    c.eval.actions += 4
    refused(c, "actions", "8-byte")


def test_evaluate_needs_both_fused_flags(pkg):
    abi = pkg.abi
    c = EvalCall(pkg)
    c.params.flags = abi.SCALE_ACTIONS
    refused(c, "MARLNAV_WRITE_OBS_NORM")
    c.params.flags = abi.WRITE_OBS_NORM
    refused(c, "MARLNAV_SCALE_ACTIONS")


def test_evaluate_reserved_fields_must_be_zero(pkg):
    c = EvalCall(pkg)
    c.eval.reserved = 1
    refused(c, "eval->reserved=1")
    c = EvalCall(pkg)
    c.pdims.reserved = 1
    refused(c, "reserved=1")


def test_evaluate_null_pointers_are_refused(pkg):
    abi = pkg.abi
    for struct, fields in (("env", abi.EVAL_ENV_REQUIRED),
                           ("policy", abi.POLICY_WEIGHT_FIELDS[:6]),
                           ("eval", abi.EVAL_POINTER_FIELDS)):
        for f in fields:
            c = EvalCall(pkg)
            setattr(getattr(c, struct), f, None)
            refused(c, f"{struct}->{f}", "NULL")
    # what the call ignores may be NULL: the critic, the policy's per-call
    # fields, the env's per-step fields and, without a traced env, the trace
    c = EvalCall(pkg)
    for f in ("actions", "reward", "terminated", "truncated", "counters", "formation_obs",
              "states_out", "obs_norm"):
        setattr(c.env, f, None)
    for f in abi.POLICY_BUFFER_FIELDS:
        if f not in abi.POLICY_WEIGHT_FIELDS[:6]:
            assert not getattr(c.policy, f)
    c.eval.trace_env = -1
    for f in abi.EVAL_TRACE_FIELDS:
        setattr(c.eval, f, None)
    c.reaches_the_last_check()


@pytest.mark.parametrize("field,value,word", [
    ("num_agents", 4, "num_agents"), ("obs_dim", 14, "obs_dim"),
    ("num_parallel", 7, "num_parallel"), ("env_offset", 0, "env_offset"),
    ("hidden_size", 0, "hidden_size"), ("hidden_size", 513, "hidden_size")])
def test_evaluate_policy_dims_must_match_the_env(pkg, field, value, word):
    c = EvalCall(pkg)
    setattr(c.pdims, field, value)
    refused(c, word)


def test_evaluate_refuses_reference_rng_candidates(pkg):
    c = EvalCall(pkg)
    c.env.fresh_states = c.env.fresh_obstacles = c.env.fresh_target = 0x7000000
    refused(c, "fresh_states")


# --------------------------------------------------------- the tracker's rule
def test_tracker_rule_on_a_hand_written_table():
    """3 envs, 5 steps. Env 0 starts at an episode's first step, env 1 and 2
    inside one. Rewards are exact in binary, so every sum below is exact.

    env 0: done after steps 1 and 3 -> whole episodes (1 + 2 = 3, length 2),
           (0.5 - 4 = -3.5, length 2); step 4 leaves 8 under way.
    env 1: done after step 0 -> a partial one; then done after step 4 ->
           whole (2 + 2 + 2 + 2 = 8, length 4).
    env 2: never done: nothing closes, 5 steps under way, still not whole."""
    F, T_ = False, True
    reward = torch.tensor([[1.0, 7.0, 0.25], [2.0, 2.0, 0.25], [0.5, 2.0, 0.25],
                           [-4.0, 2.0, 0.25], [8.0, 2.0, 0.25]], dtype=torch.float32)
    term = torch.tensor([[F, T_, F], [F, F, F], [F, F, F], [T_, F, F], [F, F, F]])
    trunc = torch.tensor([[F, F, F], [T_, F, F], [F, F, F], [T_, F, F], [F, T_, F]])
    tr = eval_ref.EpisodeTracker(torch.tensor([0.0, 3.0, 1.0]))
    assert tr.whole.tolist() == [True, False, False]
    for t in range(5):
        tr.step(reward[t], term[t], trunc[t])
    assert tr.ep_count.tolist() == [2, 1, 0]
    assert tr.partial_count.tolist() == [0, 1, 0]
    assert tr.ret_sum.tolist() == [-0.5, 8.0, 0.0]
    assert tr.ret_sqsum.tolist() == [9.0 + 12.25, 64.0, 0.0]
    assert tr.len_sum.tolist() == [4, 4, 0]
    assert tr.ret_min.tolist() == [-3.5, 8.0, math.inf]
    assert tr.ret_max.tolist() == [3.0, 8.0, -math.inf]
    assert tr.cur_return.tolist() == [8.0, 0.0, 1.25]
    assert tr.cur_len.tolist() == [1, 0, 5]
    assert tr.whole.tolist() == [True, True, False]
    assert tr.ret_sum.dtype == torch.float64 and tr.len_sum.dtype == torch.int64
    ints, floats = tr.totals()
    assert ints == (3, 1, 8) and floats == (7.5, 85.25, -3.5, 8.0)
    ev = importlib.import_module("marl-nav_amd.evaluation")
    s = ev.summary_stats(*ints, *floats)
    assert s["episodes"] == 3 and s["partial_episodes"] == 1
    assert s["mean_return"] == 2.5 and s["mean_length"] == 8 / 3
    # unbiased: ((3 - 2.5)^2 + (-3.5 - 2.5)^2 + (8 - 2.5)^2) / 2 = 33.25
    assert s["std_return"] == pytest.approx(math.sqrt(33.25), rel=1e-15)
    assert (s["min_return"], s["max_return"]) == (-3.5, 8.0)
    none = ev.summary_stats(0, 2, 0, 0.0, 0.0, math.inf, -math.inf)
    assert math.isnan(none["mean_return"]) and math.isnan(none["std_return"])
    assert math.isnan(none["mean_length"])
    assert (none["min_return"], none["max_return"]) == (math.inf, -math.inf)
    assert math.isnan(ev.summary_stats(1, 0, 2, 3.0, 9.0, 3.0, 3.0)["std_return"])


# ------------------------------------------------------------ the Python layer
def state_dict(H=50, D=12):
    g = torch.Generator().manual_seed(0)
    return {"fc1.weight": torch.randn(H, D, generator=g), "fc1.bias": torch.randn(H, generator=g),
            "fc_mu.weight": torch.randn(2, H, generator=g), "fc_mu.bias": torch.randn(2, generator=g),
            "fc_std.weight": torch.randn(2, H, generator=g),
            "fc_std.bias": torch.randn(2, generator=g)}


def test_fused_actor_refuses_cpu_tensors(pkg):
    from types import SimpleNamespace as NS
    sd = state_dict()
    lin = lambda p: NS(weight=sd[p + ".weight"], bias=sd[p + ".bias"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.FusedActor(NS(fc1=lin("fc1"), fc_mu=lin("fc_mu"), fc_std=lin("fc_std")))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.FusedActor.from_state_dict(sd, "cpu")
    with pytest.raises(AttributeError):
        pkg.FusedActor(NS(fc1=lin("fc1"), fc_mu=lin("fc_mu")))     # no fc_std


def test_from_state_dict_rejects_wrong_keys_and_shapes(pkg):
    sd = state_dict()
    missing = {k: v for k, v in sd.items() if k != "fc_std.bias"}
    with pytest.raises(ValueError, match=r"missing \['fc_std.bias'\]"):
        pkg.FusedActor.from_state_dict(missing, "cpu")
    extra = dict(sd, **{"fc2.weight": torch.zeros(1, 50)})        # a critic's file
    with pytest.raises(ValueError, match=r"unexpected \['fc2.weight'\]"):
        pkg.FusedActor.from_state_dict(extra, "cpu")
    for key, shape in (("fc1.bias", (49,)), ("fc_mu.weight", (2, 49)), ("fc_mu.weight", (3, 50)),
                       ("fc_mu.bias", (3,)), ("fc_std.weight", (50, 2)), ("fc_std.bias", (1,)),
                       ("fc1.weight", (50,))):
        bad = dict(sd, **{key: torch.zeros(shape)})
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            pkg.FusedActor.from_state_dict(bad, "cpu")


def test_cli_evaluate_without_a_device_returns_1(pkg, capsys, monkeypatch):
    cli = importlib.import_module("marl-nav_amd.cli")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert cli.main(["--evaluate"]) == 1
    assert "HIP device" in capsys.readouterr().err
    assert cli.main([]) == 2 and cli.main(["-re"]) == 2


def test_parser_keeps_every_reference_default(pkg):
    cli = importlib.import_module("marl-nav_amd.cli")
    args = vars(cli.build_parser().parse_args([]))
    ref = vars(pkg.default_args())
    for k, v in ref.items():
        assert args[k] == v, k
    assert args["evaluate"] is False and args["trace_out"] is None
    got = cli.build_parser().parse_args(["--evaluate", "-w", "a.pt", "-ra", "-ms", "7", "-pi", "3",
                                         "--trace-out", "t.npz"])
    assert (got.evaluate, got.weights_file, got.random, got.max_step, got.parallel_index,
            got.trace_out) == (True, "a.pt", True, 7, 3, "t.npz")
