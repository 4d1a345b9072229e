"""The one-call rollout (include/marlnav.h ``marlnav_rollout_collect``)
without a GPU: the new struct matches its ctypes mirror, the library exports
the entry point under the unchanged ABI version, and every validation case
fails with MARLNAV_EINVAL and its field named before any HIP call (the
pointers below are never dereferenced)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "marlnav.h")
SYMBOL = "marlnav_rollout_collect"


def test_rollout_struct_layout_matches_header(pkg, tmp_path):
    abi = pkg.abi
    cls = abi.MarlnavRolloutBuffers
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
             'int main(void) {',
             f'printf("size %zu\\n", sizeof({cls.__name__}));']
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
    assert got["size"] == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname
    assert [f for f, _ in cls._fields_] == [
        "obs", "actions", "log_probs", "values", "rewards", "done", "truncated", "eps",
        "returns", "returns_stats", "returns_work"]
    assert len(got) == 1 + len(cls._fields_)


def test_library_exports_the_rollout_entry_point(pkg):
    lib = pkg.abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert SYMBOL in pkg.abi.EXPORTS and hasattr(lib, SYMBOL)
    assert f" T {SYMBOL}" in out
    assert pkg.abi.ABI_VERSION == 5 and lib.marlnav_abi_version() == 5
    assert "collect_fused" in pkg.__all__ and callable(pkg.collect_fused)


class Call(object):
    """A call that passes every check: 8 envs x 3 agents x 3 obstacles
    (D = 12), 4 steps, distinct fake pointers far apart."""

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
        for f in abi.POLICY_WEIGHT_FIELDS:
            setattr(self.policy, f, at)
            at += 0x100000
        self.rollout = abi.MarlnavRolloutBuffers()
        for f in abi.ROLLOUT_BUFFER_FIELDS:
            setattr(self.rollout, f, at)
            at += 0x100000
        self.T = 4
        self.null = set()

    def __call__(self):
        ref = lambda name: None if name in self.null else ctypes.byref(getattr(self, name))
        rc = self.lib.marlnav_rollout_collect(
            ref("dims"), ref("params"), ref("env"), 1, ref("pdims"), ref("policy"), 0, 0,
            ref("rollout"), self.T, 0.9, None)
        return rc, self.lib.marlnav_last_error()


def refused(call, *words):
    rc, msg = call()
    assert rc == -1, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


@pytest.mark.parametrize("T", [0, -3])
def test_rollout_needs_a_step(pkg, T):
    c = Call(pkg)
    c.T = T
    refused(c, "T=")


@pytest.mark.parametrize("which", ["dims", "params", "env", "pdims", "policy", "rollout"])
def test_rollout_null_structs_are_refused(pkg, which):
    c = Call(pkg)
    c.null.add(which)
    refused(c, which, "NULL")


def test_rollout_null_pointers_are_refused(pkg):
    abi = pkg.abi
    for struct, fields in (("env", abi.ROLLOUT_ENV_REQUIRED),
                           ("policy", abi.POLICY_WEIGHT_FIELDS),
                           ("rollout", abi.ROLLOUT_REQUIRED_FIELDS)):
        for f in fields:
            c = Call(pkg)
            setattr(getattr(c, struct), f, None)
            refused(c, f"{struct}->{f}", "NULL")
    # the ignored per-step fields and the optional ones may be NULL: with all
    # of them NULL the call still reaches the check of a later field
    c = Call(pkg)
    for f in ("actions", "reward", "terminated", "truncated", "counters", "formation_obs",
              "states_out"):
        setattr(c.env, f, None)
    for f in ("obs_norm", "eps", "actions", "log_probs", "values", "eps_out"):
        setattr(c.policy, f, None)
    for f in ("eps", "returns", "returns_stats", "returns_work"):
        setattr(c.rollout, f, None)
    c.rollout.truncated = c.rollout.done       # the last check there is
    refused(c, "truncated", "overlaps")


@pytest.mark.parametrize("missing", ["returns", "returns_stats", "returns_work"])
def test_rollout_returns_pointers_come_together(pkg, missing):
    c = Call(pkg)
    setattr(c.rollout, missing, None)
    refused(c, "returns", "returns_stats", "returns_work")


@pytest.mark.parametrize("field,value,word", [
    ("num_agents", 4, "num_agents"), ("obs_dim", 14, "obs_dim"), ("obs_dim", 10, "obs_dim"),
    ("num_parallel", 7, "num_parallel"), ("env_offset", 0, "env_offset"),
    ("hidden_size", 0, "hidden_size"), ("hidden_size", 513, "hidden_size"),
    ("reserved", 1, "reserved")])
def test_rollout_policy_dims_must_match_the_env(pkg, field, value, word):
    c = Call(pkg)
    setattr(c.pdims, field, value)
    refused(c, word)


@pytest.mark.parametrize("field,value,word", [
    ("num_parallel", 0, "num_parallel"), ("num_agents", 1, "num_agents"),
    ("num_obstacles", 4, "num_obstacles")])
def test_rollout_bad_env_dims_are_refused(pkg, field, value, word):
    c = Call(pkg)
    setattr(c.dims, field, value)
    refused(c, word)


def test_rollout_obs_dim_follows_the_observed_obstacles(pkg):
    """D = 2 + 2*O + 2*(A-1) with O the observed count, not the stride."""
    c = Call(pkg)
    c.dims.num_obstacles, c.dims.obstacle_stride = 2, 3
    refused(c, "obs_dim")
    c.pdims.obs_dim = 10
    c.rollout.truncated = c.rollout.done
    refused(c, "truncated")


def test_rollout_needs_both_fused_flags(pkg):
    abi = pkg.abi
    c = Call(pkg)
    c.params.flags = abi.SCALE_ACTIONS
    refused(c, "MARLNAV_WRITE_OBS_NORM")
    c.params.flags = abi.WRITE_OBS_NORM
    refused(c, "MARLNAV_SCALE_ACTIONS")
    c.params.flags = 0
    refused(c, "MARLNAV_")


def test_rollout_refuses_reference_rng_candidates(pkg):
    c = Call(pkg)
    c.env.fresh_states = c.env.fresh_obstacles = c.env.fresh_target = 0x7000000
    refused(c, "fresh_states")


def test_rollout_refuses_a_stack_over_the_envs_own_obs_norm(pkg):
    row = 8 * 3 * 12 * 4                       # bytes of one observation row
    base = Call(pkg).rollout.obs
    for at in (base, base + row, base + 4 * row - 4, base - row + 4):
        c = Call(pkg)
        c.env.obs_norm = at
        refused(c, "obs_norm", "overlaps")
    for at in (base + 4 * row, base - row):    # adjacent, not overlapping
        c = Call(pkg)
        c.env.obs_norm = at
        c.rollout.truncated = c.rollout.done
        refused(c, "truncated")


def test_rollout_other_pointer_checks(pkg):
    c = Call(pkg)
    c.rollout.actions += 4
    refused(c, "actions", "8-byte")
    c = Call(pkg)
    c.env.states_out = c.env.states + 16
    refused(c, "states_out", "overlaps")
    c = Call(pkg)
    c.rollout.truncated = c.rollout.done + 8 * 4 - 1
    refused(c, "truncated", "overlaps")


def test_collect_fused_checks_run_through_abi_check(pkg):
    c = Call(pkg)
    c.T = 0
    rc, _ = c()
    with pytest.raises(RuntimeError, match="T=0"):
        pkg.abi.check(rc)
