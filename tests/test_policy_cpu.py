"""The fused policy step (include/marlnav.h ``marlnav_policy_act``) without a
GPU: the two new structs match their ctypes mirrors, the library exports the
entry point, argument validation fails loudly before any HIP call, and the
fixture F6-policy pins the formulas (tests/policy_ref.py) independently of
the kernel; the per-shape criterion of the generated shapes admits a correct
fp32 evaluation in the kernel's formulation and refuses subtly wrong ones; the
host restatement of the kernel's normals is the oracle's Philox and is normal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import policy_ref as pr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "marlnav.h")


def test_policy_struct_layout_matches_header(pkg, tmp_path):
    abi = pkg.abi
    classes = (abi.MarlnavPolicyDims, abi.MarlnavPolicyBuffers)
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
    assert abi.ABI_VERSION == 5


def test_library_exports_policy_act(pkg):
    lib = pkg.abi.load_library()
    assert "marlnav_policy_act" in pkg.abi.EXPORTS and hasattr(lib, "marlnav_policy_act")
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert " T marlnav_policy_act" in out
    assert lib.marlnav_abi_version() == 5


def _call(pkg, dims, bufs):
    lib = pkg.abi.load_library()
    rc = lib.marlnav_policy_act(ctypes.byref(dims), ctypes.byref(bufs), 1, 2, None)
    return rc, lib.marlnav_last_error()


def _good(pkg):
    """Dims and buffers that pass every check (the pointers are never
    dereferenced: each call below fails validation, which runs first)."""
    abi = pkg.abi
    d = abi.MarlnavPolicyDims(num_parallel=8, num_agents=3, obs_dim=12, hidden_size=50)
    b = abi.MarlnavPolicyBuffers()
    for f in abi.POLICY_REQUIRED_FIELDS:
        setattr(b, f, 0x1000)
    return d, b


@pytest.mark.parametrize("field,value,word", [
    ("hidden_size", 0, b"hidden_size"), ("hidden_size", 513, b"hidden_size"),
    ("num_agents", 1, b"num_agents"), ("num_agents", 65, b"num_agents"),
    ("obs_dim", 13, b"obs_dim"),      # odd: no O gives 2 + 2 O + 2 (A - 1) = 13
    ("obs_dim", 6, b"obs_dim"),       # O = 0
    ("obs_dim", 4, b"obs_dim"),       # right for A = 2 (O = 0 aside), too short for A = 3
    ("num_parallel", 0, b"num_parallel"), ("env_offset", -1, b"env_offset"),
    ("reserved", 1, b"reserved")])
def test_policy_bad_dims_are_refused(pkg, field, value, word):
    d, b = _good(pkg)
    setattr(d, field, value)
    rc, msg = _call(pkg, d, b)
    assert rc == -1 and word in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=word.decode()):
        pkg.abi.check(rc)


def test_policy_null_pointers_are_refused(pkg):
    lib = pkg.abi.load_library()
    d, b = _good(pkg)
    assert lib.marlnav_policy_act(None, ctypes.byref(b), 0, 0, None) == -1
    assert lib.marlnav_policy_act(ctypes.byref(d), None, 0, 0, None) == -1
    assert len(pkg.abi.POLICY_REQUIRED_FIELDS) == 14
    for f in pkg.abi.POLICY_REQUIRED_FIELDS:
        d, b = _good(pkg)
        setattr(b, f, None)
        rc, msg = _call(pkg, d, b)
        assert rc == -1 and b"NULL" in msg, (f, rc, msg)


def test_fused_policy_refuses_cpu_modules(pkg):
    import torch
    from types import SimpleNamespace as NS
    lin = lambda o, i: NS(weight=torch.zeros(o, i), bias=torch.zeros(o))
    actor = NS(fc1=lin(50, 12), fc_mu=lin(2, 50), fc_std=lin(2, 50))
    critic = NS(fc1=lin(50, 36), fc2=lin(1, 50))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.FusedPolicy(actor, critic)


# ------------------------------------------------------------ fixture F6-policy
def test_fixture_covers_the_issue_cases():
    cases = pr.manifest()["cases"]
    got = {(c["P"], c["A"], c["O"], c["H"]) for c in cases.values()}
    assert got == {(1, 3, 3, 50), (5, 3, 3, 50), (67, 3, 3, 50), (9, 2, 1, 1), (33, 3, 8, 67),
                   (3, 16, 32, 50)}
    assert os.path.getsize(os.path.join(pr.GOLDEN, "policy_f6.npz")) < 200 * 1024
    tiny = float(np.finfo(np.float32).tiny)
    for c in cases.values():
        sat = c["groups"]["sat"]
        assert sat["mu_pre"][0] < -8 and sat["mu_pre"][1] > 8
        assert sat["std_pre"][0] < -20 and sat["std_pre"][1] > 20
        for g in c["groups"].values():
            assert g["variance"][0] >= tiny


def _restated(variance_is_std=False):
    import torch
    pooled = pr.Pooled()
    for name in pr.case_names():
        for group in pr.GROUPS:
            c = pr.load_case(name, group)
            w, obs, eps = pr.tensors(c)
            assert obs.shape == (c["P"], c["A"], c["D"]) and float(obs.abs().max()) <= 1.0
            with torch.no_grad():
                out = pr.policy_ref(w, obs, eps, variance_is_std=variance_is_std)
            pooled.add(c, [o.numpy() for o in out])
    return pooled


def test_restated_formulas_reproduce_the_reference():
    """policy_ref in fp32 on the CPU against the reference's fp32 outputs,
    under the criterion the kernel is held to (both measured against the
    fp64 values, pooled per output kind and weight group)."""
    pooled = _restated()
    print("\n".join(pooled.lines("policy_ref(cpu fp32)")))
    assert not pooled.failures(), pooled.failures()
    # and in fp64 it IS the fixture's fp64 evaluation, to that one's own
    # rounding: its log_prob recovers eps as (a - mu) / sqrt(v) with sqrt(v)
    # down to 3e-7 (sat), i.e. to 2^-53 / 3e-7 = 4e-10 of |a| <= 1
    import torch
    for name in pr.case_names():
        for group in pr.GROUPS:
            c = pr.load_case(name, group)
            w, obs, eps = pr.tensors(c, dtype=torch.float64)
            for k, o in zip(pr.KINDS, pr.policy_ref(w, obs, eps)):
                np.testing.assert_allclose(o.numpy().reshape(c[k + "64"].shape), c[k + "64"],
                                           rtol=1e-9, atol=1e-9, err_msg=f"{name} {group} {k}")


def test_fixture_rejects_variance_read_as_std():
    """The restatement with softplus's output used as the standard deviation
    must miss the criterion: the fixture discriminates covariance from std."""
    bad = {(k, g) for k, g, _, _ in _restated(variance_is_std=True).failures()}
    assert ("actions", "default") in bad and ("log_probs", "default") in bad, bad
    assert ("actions", "sat") in bad, bad


# ------------------------------------------------------------- generated shapes
def test_shape_list_reaches_every_split_of_the_hidden_units():
    """The list holds what tests/test_policy_gpu.py relies on it for."""
    shapes = pr.SHAPES
    assert len(set(shapes)) == len(shapes) == 24
    hq = {(H + 3) // 4 for _, _, _, H in shapes}
    assert {q % 4 for q in hq} == {0, 1, 2, 3} and {q % 8 for q in hq} >= {0, 1, 2, 3}
    assert any(3 * ((H + 3) // 4) >= H for _, _, _, H in shapes)       # a wave with no unit
    assert max(64 * A for _, A, _, _ in shapes if A == 16) > 3 * 256   # 4 trips of the row loop
    assert (65, 64, 256, 5) in shapes and (3, 64, 256, 512) in shapes  # D = 640, H = 512


def test_criterion_admits_the_collapsed_formulation_on_every_shape():
    """``collapsed_ref`` (the kernel's formulation: the actor's two layers as
    one affine map) in fp32 on the CPU against fp64, per shape: a correct
    kernel with another summation order than the reference's meets the
    criterion with room. Worst ratio measured: see the printed lines."""
    import torch
    worst = 0.0
    for shape in pr.SHAPES:
        c = pr.generated(*shape)
        with torch.no_grad():
            chk = pr.check_shape(c.c64, c.ref32, pr.collapsed_ref(c.w, c.obs, c.eps))
        print(f"(P, A, O, H) = {shape}:")
        print("\n".join("  " + line for line in chk.lines("collapsed_ref(cpu fp32)")))
        worst = max([worst] + [chk.ratio(k) for k in pr.KINDS])
        assert not chk.failures(), (shape, chk.failures())
    print(f"worst ratio over {len(pr.SHAPES)} shapes: {worst:.2f} (bound {pr.FACTOR:g})")


def _mutants(c):
    """fp32 candidates that are each wrong in one way a kernel could be, on the
    generated case ``c``: name -> (outputs, the kinds it must fail)."""
    import torch
    P, A, O, H = c.shape
    w, obs, eps = c.w, c.obs, c.eps
    out = {}
    with torch.no_grad():
        out["collapse drops the last hidden unit"] = (
            pr.collapsed_ref(w, obs, eps, drop_collapse=1), ("actions", "log_probs"))
        out["critic drops the last hidden unit"] = (
            pr.collapsed_ref(w, obs, eps, drop_critic=1), ("values",))
        shifted = obs.clone()
        shifted[63] = obs[64]                      # the critic of env 63 reads env 64's rows
        good = pr.collapsed_ref(w, obs, eps)
        out["critic of env 63 fed env 64's row"] = (
            (good[0], good[1], pr.collapsed_ref(w, shifted, eps)[2]), ("values",))
        if 64 * A > 256:                           # the block's row loop has a second trip
            wrapped = obs.clone().reshape(P * A, -1)
            wrapped[256] = wrapped[0]              # row 256 of block 0 reads row 0's obs
            bad = pr.collapsed_ref(w, wrapped.reshape(obs.shape), eps)
            out["actor row 256 fed row 0's obs"] = ((bad[0], bad[1], good[2]),
                                                    ("actions", "log_probs"))
        out["variance read as std"] = (pr.policy_ref(w, obs, eps, variance_is_std=True),
                                       ("actions", "log_probs"))
    return out


@pytest.mark.parametrize("shape", [(70, 3, 3, 512), (130, 16, 32, 50)])
def test_criterion_refuses_a_subtly_wrong_kernel(shape):
    """Each candidate of ``_mutants`` misses the criterion in the kinds its
    defect touches and meets it in the others. A block of 3-agent envs has
    192 agent rows, one trip of the actor's row loop: the row-256 candidate
    exists at 16 agents only, where the loop makes 4 trips."""
    c = pr.generated(*shape)
    mutants = _mutants(c)
    assert len(mutants) == (5 if shape[1] == 16 else 4)
    for name, (got, kinds) in mutants.items():
        chk = pr.check_shape(c.c64, c.ref32, got)
        print(f"{shape} {name}:")
        print("\n".join("  " + line for line in chk.lines("candidate")))
        assert {f[0] for f in chk.failures()} == set(kinds), (shape, name, chk.failures())


# ---------------------------------------------------------------- native normals
def test_host_philox_is_the_oracles():
    """policy_ref's numpy Philox2x32-10 and key against oracle.philox and
    oracle.native_key (the C restatement of device_rng.h, itself pinned to
    Random123's known-answer vectors by tests/test_oracle_golden.py)."""
    import oracle as orc
    for seed, step in ((11, 5), (11 + 2 ** 32, 5 + 2 ** 32), (2 ** 64 - 1, 2 ** 63 + 9)):
        mixed = pr.seed_mix(seed)                  # the oracle mixes the seed itself
        for blk in (0, 3, pr.POLICY_BLOCK):
            assert pr.native_key(mixed, blk, step) == orc.native_key(seed, blk, step)
    ctr = np.array([[0, 0], [1, 2], [0xFFFFFFFF, 0xFFFFFFFF], [0x243F6A88, 0x85A308D3]], np.uint32)
    for key in (0, 0xFFFFFFFF, 0x13198A2E):
        got = np.stack(pr.philox2x32_10(ctr[:, 0], ctr[:, 1], key), 1)
        for row, want in zip(got, (orc.philox(c, key) for c in ctr)):
            np.testing.assert_array_equal(row, want)
    # the counter of a global row id past 2^32 carries its high word
    off, A = 2 ** 32 // 3 - 100, 3
    r0, r1 = pr.native_words(11, 5, off, 400, A)
    key = orc.native_key(11, pr.POLICY_BLOCK, 5)
    for row in (0, 300, 301, 399):
        gid = off * A + row
        want = orc.philox([gid & 0xFFFFFFFF, 5 ^ ((gid >> 32) * 0x85EBCA77 & 0xFFFFFFFF)], key)
        assert (int(r0[row]), int(r1[row])) == (int(want[0]), int(want[1])), row
    assert off * A + 300 < 2 ** 32 <= off * A + 301


def test_host_normals_have_the_standard_normal_law():
    """The checks of test_native_normals_have_the_standard_normal_law
    (tests/test_policy_gpu.py) on the host restatement, 12 288 rows of (seed
    11, step 5): what the kernel's eps_out is compared with is itself normal."""
    import rng_stats
    import torch
    from scipy import stats
    eps = pr.native_normals(11, 5, 0, 4096 * 3, 3)
    assert eps.shape == (12288, 2) and np.isfinite(eps).all()
    n = eps.shape[0]
    for comp in range(2):
        z = eps[:, comp]
        assert abs(z.mean()) < 6 / np.sqrt(n), (comp, z.mean())
        assert abs(z.var() - 1.0) < 6 * np.sqrt(2.0 / n), (comp, z.var())
        ks = stats.kstest(z, "norm")
        assert ks.pvalue > rng_stats.P_MIN, (comp, ks)
    rng_stats.check_uncorrelated(eps[:, 0], eps[:, 1], "host eps components")
    rng_stats.check_uncorrelated(eps[:-1, 0], eps[1:, 0], "host eps row r, r+1")
    ref = torch.randn(n, 2, generator=torch.Generator().manual_seed(7)).numpy()
    rng_stats.check_same_law(eps, ref, "host eps vs torch.randn")
