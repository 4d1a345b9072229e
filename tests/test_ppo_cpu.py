"""The fused PPO update (include/marlnav.h ``marlnav_ppo_actor_grad`` /
``marlnav_ppo_critic_grad``) without a GPU: the two new structs match their
ctypes mirrors, the library exports the three entry points, argument
validation fails loudly before any HIP call, and fixture F7-ppo pins the
formulas and the reference's quirks (tests/ppo_ref.py) independently of the
kernels. The host side's launch plan, restated as ppo_ref.launch_plan, is held
to marlnav_ppo_work_size, every named shape of the GPU tests is pinned to the
launch path it is there for, and the generated cases' seeds are checked
against their boundary margins."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import ppo_ref as pp
import test_ppo_gpu as tg
import test_train_gpu as tt
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "marlnav.h")
SYMBOLS = ("marlnav_ppo_work_size", "marlnav_ppo_actor_grad", "marlnav_ppo_critic_grad")


def test_ppo_struct_layout_matches_header(pkg, tmp_path):
    abi = pkg.abi
    classes = (abi.MarlnavPpoDims, abi.MarlnavPpoBuffers)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
             'int main(void) {']
    for cls in classes:
        lines.append(f'printf("{cls.__name__} size %zu\\n", sizeof({cls.__name__}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cls.__name__} {fname} %zu\\n", '
                         f'offsetof({cls.__name__}, {fname}));')
    lines.append("return 0; }")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(c), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True,
                               check=True).stdout.splitlines():
        cls, field, val = line.split()
        got[(cls, field)] = int(val)
    for cls in classes:
        assert got[(cls.__name__, "size")] == ctypes.sizeof(cls), cls.__name__
        for fname, _ in cls._fields_:
            assert got[(cls.__name__, fname)] == getattr(cls, fname).offset, (cls, fname)
    assert [f for f, _ in abi.MarlnavPpoDims._fields_] == [
        "num_parallel", "num_steps", "num_agents", "obs_dim", "hidden_size", "reserved"]
    assert len(abi.MarlnavPpoBuffers._fields_) == 5 + 10 + 10 + 2


def test_library_exports_the_ppo_entry_points(pkg):
    lib = pkg.abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert s in pkg.abi.EXPORTS and hasattr(lib, s)
        assert f" T {s}" in out
    assert pkg.abi.ABI_VERSION == 5 and lib.marlnav_abi_version() == 5


def _good(pkg):
    """Dims and buffers that pass every check (the pointers are never
    dereferenced: each call below fails validation, which runs first)."""
    abi = pkg.abi
    d = abi.MarlnavPpoDims(num_parallel=8, num_steps=2, num_agents=3, obs_dim=12, hidden_size=50)
    b = abi.MarlnavPpoBuffers()
    for f in abi.PPO_BUFFER_FIELDS:
        setattr(b, f, 0x1000)
    return d, b


def _calls(pkg):
    lib = pkg.abi.load_library()
    return (("actor", pkg.abi.PPO_ACTOR_REQUIRED,
             lambda d, b: lib.marlnav_ppo_actor_grad(d, b, 0.01, 0.001, None)),
            ("critic", pkg.abi.PPO_CRITIC_REQUIRED,
             lambda d, b: lib.marlnav_ppo_critic_grad(d, b, 0.01, None)))


@pytest.mark.parametrize("field,value,word", [
    ("hidden_size", 0, b"hidden_size"), ("hidden_size", 513, b"hidden_size"),
    ("num_agents", 1, b"num_agents"), ("num_agents", 65, b"num_agents"),
    ("obs_dim", 13, b"obs_dim"), ("obs_dim", 6, b"obs_dim"), ("obs_dim", 4, b"obs_dim"),
    ("num_parallel", 0, b"num_parallel"), ("num_steps", 0, b"num_steps"),
    ("reserved", 1, b"reserved")])
def test_ppo_bad_dims_are_refused(pkg, field, value, word):
    lib = pkg.abi.load_library()
    for _, _, call in _calls(pkg):
        d, b = _good(pkg)
        setattr(d, field, value)
        rc = call(ctypes.byref(d), ctypes.byref(b))
        msg = lib.marlnav_last_error()
        assert rc == -1 and word in msg, (rc, msg)
        with pytest.raises(RuntimeError, match=word.decode()):
            pkg.abi.check(rc)
    d, _ = _good(pkg)
    setattr(d, field, value)
    assert lib.marlnav_ppo_work_size(ctypes.byref(d)) == -1
    assert word in lib.marlnav_last_error()


def test_ppo_needs_two_env_rows(pkg):
    lib = pkg.abi.load_library()
    for _, _, call in _calls(pkg):
        d, b = _good(pkg)
        d.num_parallel, d.num_steps = 1, 1
        assert call(ctypes.byref(d), ctypes.byref(b)) == -1
        msg = lib.marlnav_last_error()
        assert b"num_steps" in msg and b"num_parallel" in msg, msg
    d, _ = _good(pkg)
    d.num_parallel, d.num_steps = 1, 2
    assert lib.marlnav_ppo_work_size(ctypes.byref(d)) > 0


def test_ppo_null_pointers_are_refused(pkg):
    lib = pkg.abi.load_library()
    abi = pkg.abi
    assert len(abi.PPO_ACTOR_REQUIRED) == 5 + 6 + 6 + 2
    assert len(abi.PPO_CRITIC_REQUIRED) == 3 + 4 + 4 + 2
    for which, required, call in _calls(pkg):
        d, b = _good(pkg)
        assert call(None, ctypes.byref(b)) == -1
        assert call(ctypes.byref(d), None) == -1
        for f in required:
            d, b = _good(pkg)
            setattr(b, f, None)
            rc = call(ctypes.byref(d), ctypes.byref(b))
            msg = lib.marlnav_last_error()
            assert rc == -1 and b"NULL" in msg and f.encode() in msg, (which, f, rc, msg)
        # the other network's pointers (and what this loss does not read) are
        # not required: with all of them NULL the call gets past validation of
        # every field it names, which only a later required NULL would stop
        d, b = _good(pkg)
        for f in abi.PPO_BUFFER_FIELDS:
            if f not in required:
                setattr(b, f, None)
        setattr(b, required[-1], None)
        rc = call(ctypes.byref(d), ctypes.byref(b))
        msg = lib.marlnav_last_error()
        assert rc == -1 and required[-1].encode() in msg, (which, msg)


def test_fused_ppo_refuses_cpu_modules(pkg):
    from types import SimpleNamespace as NS
    lin = lambda o, i: NS(weight=torch.zeros(o, i), bias=torch.zeros(o))
    actor = NS(fc1=lin(50, 12), fc_mu=lin(2, 50), fc_std=lin(2, 50))
    critic = NS(fc1=lin(50, 36), fc2=lin(1, 50))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.FusedPPO(actor, critic, 0.01, 0.001)


# --------------------------------------------------------------- fixture F7-ppo
def test_fixture_covers_the_issue_cases():
    m = pp.manifest()
    got = {(c["T"], c["P"], c["A"], c["O"], c["H"]) for c in m["cases"].values()}
    assert got == {(2, 1, 3, 3, 50), (2, 5, 3, 3, 50), (3, 67, 3, 3, 50), (2, 9, 2, 1, 1),
                   (2, 33, 3, 8, 67)}
    assert (m["epsilon"], m["ent_const"]) == (0.01, 0.001)
    assert os.path.getsize(os.path.join(pp.GOLDEN, "ppo_f7.npz")) < 1024 * 1024
    for which in ("actor", "critic"):
        for branch, share in m["pooled_branch_shares"][which].items():
            assert share >= 0.05, (which, branch, share)
    for c in m["cases"].values():
        assert c["min_boundary_gap"] > 1e-4
    for k, e in m["reference_fp32_gradient_error"].items():
        assert e >= 2.0 ** -24, (k, e)


def _fixture_check(rtol, **kw):
    """ppo_ref in fp64 against the fixture's fp64 losses and gradients:
    -> [(case, what, relative error)] beyond rtol."""
    bad = []
    for name in pp.case_names():
        c = pp.load_case(name)
        w, data = pp.tensors(c, dtype=torch.float64)
        for which in ("actor", "critic"):
            loss, grads = pp.loss_and_grads(which, w, data, c["epsilon"], c["ent_const"],
                                            **(kw if which == "actor" else {}))
            want = c["loss64"][which]
            err = abs(float(loss) - want) / abs(want)
            if not err <= rtol:
                bad.append((name, which + " loss", err))
            for k, g in grads.items():
                g64 = c["g64"][k]
                err = float(np.abs(g.numpy().reshape(g64.shape) - g64).max() / np.abs(g64).max())
                if not err <= rtol:
                    bad.append((name, k, err))
    return bad


def test_restated_formulas_reproduce_the_reference():
    assert not _fixture_check(1e-12)
    # and in fp32 the restatement meets the criterion the kernels are held to
    pooled = pp.Pooled()
    for name in pp.case_names():
        c = pp.load_case(name)
        w, data = pp.tensors(c)
        for which in ("actor", "critic"):
            loss, grads = pp.loss_and_grads(which, w, data, c["epsilon"], c["ent_const"])
            pooled.add(which + " loss", float(loss), c["loss32"][which], c["loss64"][which])
            for k, g in grads.items():
                pooled.add(k, g.numpy(), c["g32"][k], c["g64"][k])
    print("\n".join(pooled.lines("ppo_ref(cpu fp32)")))
    assert not pooled.failures(), pooled.failures()


def test_fixture_rejects_the_advantage_of_the_rows_own_env():
    """With row i paired to env i // A instead of i mod N the restatement
    must miss the fixture: it pins the reference's repeat(num_agents)."""
    bad = _fixture_check(1e-12, advantage_of_own_env=True)
    missed = {(name, what) for name, what, _ in bad}
    for name in pp.case_names():
        assert (name, "actor loss") in missed, name
        assert (name, "actor.fc1.weight") in missed, name
    assert all(what.startswith("actor") for _, what in missed)


def test_minibatch_bounds_are_the_reference_slices(pkg):
    for n in range(1, 13):
        steps = list(range(n))
        for bs in range(1, n + 1):
            want = pp.list_minibatches(steps, bs)
            if any(len(s) == 0 for s in want):
                with pytest.raises(ValueError, match="empty"):
                    pkg.minibatch_bounds(n, bs)
                continue
            got = pkg.minibatch_bounds(n, bs)
            assert [steps[lo:hi] for lo, hi in got] == want, (n, bs)
            assert all(0 <= lo < hi <= n for lo, hi in got)


# ------------------------------------------------------------------ launch plan
def _named_shapes():
    """Every (T, P, A, O, H) the GPU tests launch under a name, with the path
    written beside it."""
    named = [("ppo " + n, s[:5], tg.PATHS[n]) for n, s in tg.SHAPES.items()]
    named += [("phase " + n, s[:5], tt.PHASE_PATHS[n]) for n, s in tt.PHASE_SHAPES.items()]
    for n, (A, O, H, _) in tg.TILE_LOOP.items():
        both, one = tg.TILE_LOOP_PATHS[n]
        named.append(("tile loop " + n, (2, tg.TILE_LOOP_P, A, O, H), both))
        named.append(("tile loop step " + n, (1, tg.TILE_LOOP_P, A, O, H), one))
    return named


def _work_size(pkg, T, P, A, O, H):
    d = pkg.abi.MarlnavPpoDims(num_parallel=P, num_steps=T, num_agents=A,
                               obs_dim=2 + 2 * O + 2 * (A - 1), hidden_size=H)
    return int(pkg.abi.load_library().marlnav_ppo_work_size(ctypes.byref(d)))


# A D -> (A, O) of the sweep: up to, at and past one block's 128 and 256
# columns, rows that are no multiple of 4 (30, 66, 130, 258), the widest
SWEEP_AD = {12: (2, 1), 28: (2, 5), 30: (3, 2), 64: (2, 14), 66: (3, 8), 128: (2, 30),
            130: (5, 8), 132: (2, 31), 256: (2, 62), 258: (3, 40), 516: (2, 127),
            40960: (64, 256)}
SWEEP_H = (1, 8, 16, 17, 56, 57, 64, 65, 512)
SWEEP_N = (2, 64, 65, 32768, 32769)


def test_launch_plan_agrees_with_the_library_on_the_work_size(pkg):
    shapes = [s for _, s, _ in _named_shapes()]
    for AD, (A, O) in SWEEP_AD.items():
        assert A * (2 + 2 * O + 2 * (A - 1)) == AD
        shapes += [(1, N, A, O, H) for H in SWEEP_H for N in SWEEP_N]
    assert len(shapes) > 12 * 9 * 5
    kernels = set()
    for s in shapes:
        plan = pp.launch_plan(*s)
        assert plan["work_size"] == _work_size(pkg, *s), s
        kernels.add(plan["critic"]["kernel"])
    assert kernels == {"fused8", "fused64", "split8", "split64"}


def test_every_named_shape_takes_the_path_it_is_there_for():
    named = _named_shapes()
    for name, shape, path in named:
        assert pp.launch_path(*shape) == path, (name, shape, pp.launch_path(*shape))
    plan = {name: pp.launch_plan(*shape) for name, shape, _ in named}
    crit = lambda n, *keys: tuple(plan[n]["critic"][k] for k in keys)
    act = lambda n, *keys: tuple(plan[n]["actor"][k] for k in keys)
    # what the path tuple does not show
    assert crit("ppo chunks", "chunks") == (44,) and act("ppo chunks", "blocks") == (9,)
    assert crit("ppo long_row", "last_tile_cols") == (4,)
    assert crit("ppo fused64", "chunks", "last_tile_rows") == (2, 16)
    assert crit("ppo fused64_full", "last_tile_cols", "units_per_block") == (256, 64)
    assert crit("ppo unit_groups64", "units_per_block", "forward_groups") == (64, 2)
    assert crit("ppo slice_cap", "unit_slices", "units_per_block") == (8, 64)
    assert crit("ppo two_slices", "unit_slices", "units_per_block") == (2, 16)
    assert crit("ppo h_max", "unit_slices", "units_per_block", "forward_groups") == (7, 56, 8)
    assert crit("ppo cols255", "last_tile_cols") == (252,)
    assert crit("ppo cols257", "last_tile_cols") == (256,)
    assert crit("ppo two_tiles", "chunks", "last_tile_rows") == (1, 6)
    assert crit("tile loop fused8", "chunks", "last_tile_rows") == (257, 32)
    assert crit("tile loop fused64", "chunks", "last_tile_rows") == (257, 32)
    assert crit("tile loop step fused64", "chunks") == (257,)
    # between them the shapes reach every critic kernel, a second tile of a
    # chunk in a fused and in a split kernel, several unit groups behind both
    # backward kernels, every column regime of the actor and 2..7 row slices
    paths = {p for _, _, p in named}
    assert {p[0] for p in paths} == {"fused8", "fused64", "split8", "split64"}
    assert {(p[0], p[3]) for p in paths} >= {("fused8", 2), ("fused64", 2), ("split64", 2)}
    assert {p[0] for p in paths if p[2] > 1} == {"split8", "split64"}
    assert {p[5] for p in paths} == {1, 2, 3}
    assert {p[4] for p in paths} >= {1, 2, 3, 7}


@pytest.mark.parametrize("name", list(tg.SHAPES))
def test_generated_cases_keep_their_margins(name):
    """``generated`` asserts the GAPS / MARGIN conditions of its case (and
    that the fp32 and fp64 evaluations take the same branches) on the CPU:
    the seeds written beside the shapes are valid before any GPU runs."""
    which = tg.WHICH.get(name, tg.BOTH)
    w, data, truth, ref = tg.generated(*tg.SHAPES[name], which=which)
    assert set(truth) == set(ref) == set(which)
    # what the seeds were picked on (tg.SHAPES), printed: the reference's fp32
    # loss error on this host beside the rounding level of its stored values
    levels = tg.loss_rounding_levels(w, data, which)
    for net in which:
        l64, l32 = float(truth[net][0]), float(ref[net][0])
        assert np.isfinite(l64) and np.isfinite(levels[net]) and levels[net] > 0
        print(f"{name} {net} loss: reference {abs(l32 - l64) / abs(l64):.3e}  "
              f"rounding level {levels[net]:.3e}")
