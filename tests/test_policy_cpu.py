"""The fused policy step (include/marlnav.h ``marlnav_policy_act``) without a
GPU: the two new structs match their ctypes mirrors, the library exports the
entry point, argument validation fails loudly before any HIP call, and the
fixture F6-policy pins the formulas (tests/policy_ref.py) independently of
the kernel."""
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
