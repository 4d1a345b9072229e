"""The fused Adam step (include/marlnav.h ``marlnav_adam_step``,
``marlnav_ppo_actor_update`` / ``marlnav_ppo_critic_update``) without a GPU:
the two new structs match their ctypes mirrors, the library exports the four
entry points under the unchanged ABI version, argument validation fails loudly
before any HIP call and names the offending field, the update calls refuse an
Adam table that is not the network's, and ``FusedAdam`` refuses what it does
not support."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "marlnav.h")
SYMBOLS = ("marlnav_adam_state_size", "marlnav_adam_step", "marlnav_ppo_actor_update",
           "marlnav_ppo_critic_update")
FAKE = 0x1000          # non-null, 16-byte aligned, never dereferenced


def test_adam_struct_layout_matches_header(pkg, tmp_path):
    abi = pkg.abi
    classes = (abi.MarlnavAdamDims, abi.MarlnavAdamBuffers)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
             'int main(void) {']
    for cls in classes:
        lines.append(f'printf("{cls.__name__} size %zu\\n", sizeof({cls.__name__}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cls.__name__} {fname} %zu\\n", '
                         f'offsetof({cls.__name__}, {fname}));')
    lines.append('printf("max tensors %d\\n", MARLNAV_ADAM_MAX_TENSORS);')
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
    assert got[("max", "tensors")] == abi.ADAM_MAX_TENSORS == 8
    for cls in classes:
        assert got[(cls.__name__, "size")] == ctypes.sizeof(cls), cls.__name__
        for fname, _ in cls._fields_:
            assert got[(cls.__name__, fname)] == getattr(cls, fname).offset, (cls, fname)
    assert [f for f, _ in abi.MarlnavAdamDims._fields_] == [
        "num_tensors", "maximize", "numel", "lr", "beta1", "beta2", "eps", "reserved"]
    assert [f for f, _ in abi.MarlnavAdamBuffers._fields_] == [
        "param", "grad", "exp_avg", "exp_avg_sq", "state"]


def test_library_exports_the_adam_entry_points(pkg):
    lib = pkg.abi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.abi.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert s in pkg.abi.EXPORTS and hasattr(lib, s)
        assert f" T {s}" in out
    assert pkg.abi.ABI_VERSION == 5 and lib.marlnav_abi_version() == 5
    size = lib.marlnav_adam_state_size()
    assert size >= 8 and size % 8 == 0      # the int64 count and fp64 scalars


def _good_adam(pkg, sizes=(600, 50, 100, 2, 100, 2)):
    """Adam dims and buffers that pass every check; slot i's param / grad
    pointers are distinct fake addresses (never dereferenced)."""
    abi = pkg.abi
    d = abi.MarlnavAdamDims(num_tensors=len(sizes), maximize=0, lr=3e-4, beta1=0.9, beta2=0.999,
                            eps=1e-8)
    b = abi.MarlnavAdamBuffers(state=FAKE)
    for i, n in enumerate(sizes):
        d.numel[i] = n
        b.param[i] = FAKE * (2 + i)
        b.grad[i] = FAKE * (32 + i)
        b.exp_avg[i] = FAKE * (64 + i)
        b.exp_avg_sq[i] = FAKE * (96 + i)
    return d, b


def _refused(pkg, d, b, word):
    lib = pkg.abi.load_library()
    rc = lib.marlnav_adam_step(ctypes.byref(d) if d is not None else None,
                               ctypes.byref(b) if b is not None else None, None)
    msg = lib.marlnav_last_error()
    assert rc == -1 and word in msg, (rc, msg, word)
    with pytest.raises(RuntimeError, match=word.decode().replace("[", r"\[").replace("]", r"\]")):
        pkg.abi.check(rc)


@pytest.mark.parametrize("field,value,word", [
    ("num_tensors", 0, b"num_tensors"), ("num_tensors", 9, b"num_tensors"),
    ("num_tensors", -1, b"num_tensors"),
    ("maximize", 2, b"maximize"), ("maximize", -1, b"maximize"),
    ("lr", -1e-3, b"lr"), ("lr", math.inf, b"lr"), ("lr", math.nan, b"lr"),
    ("beta1", -0.1, b"beta1"), ("beta1", 1.0, b"beta1"), ("beta1", math.nan, b"beta1"),
    ("beta2", -0.1, b"beta2"), ("beta2", 1.0, b"beta2"), ("beta2", 1.5, b"beta2"),
    ("eps", -1e-8, b"eps"), ("eps", math.inf, b"eps"), ("eps", math.nan, b"eps"),
    ("reserved", 1, b"reserved")])
def test_adam_bad_dims_are_refused(pkg, field, value, word):
    d, b = _good_adam(pkg)
    setattr(d, field, value)
    _refused(pkg, d, b, word)


@pytest.mark.parametrize("slot,value", [(0, 0), (5, 0), (3, -4)])
def test_adam_numel_below_one_is_refused(pkg, slot, value):
    d, b = _good_adam(pkg)
    d.numel[slot] = value
    _refused(pkg, d, b, f"numel[{slot}]".encode())


def test_adam_unused_slots_are_not_read(pkg):
    """Slots past num_tensors may hold anything: validation gets past them to
    the one bad field of a used slot."""
    d, b = _good_adam(pkg, sizes=(7, 3))
    d.numel[2] = -1
    b.param[2] = None
    b.grad[1] = None
    _refused(pkg, d, b, b"grad[1]")


def test_adam_null_pointers_are_refused(pkg):
    d, b = _good_adam(pkg)
    _refused(pkg, None, b, b"dims")
    _refused(pkg, d, None, b"buffers")
    for f in pkg.abi.ADAM_POINTER_FIELDS:
        for slot in (0, 5):
            d, b = _good_adam(pkg)
            getattr(b, f)[slot] = None
            _refused(pkg, d, b, f"{f}[{slot}] is NULL".encode())
    d, b = _good_adam(pkg)
    b.state = None
    _refused(pkg, d, b, b"state is NULL")
    d, b = _good_adam(pkg)
    b.state = FAKE + 4
    _refused(pkg, d, b, b"state")
    d, b = _good_adam(pkg)
    b.param[1] = FAKE + 2
    _refused(pkg, d, b, b"param[1]")


# ----------------------------------------------------------- the update calls
ACTOR_SIZES = lambda H, D: (H * D, H, 2 * H, 2, 2 * H, 2)
CRITIC_SIZES = lambda H, A, D: (H * A * D, H, H, 1)


def _good_update(pkg, which):
    """PPO dims / buffers as test_ppo_cpu.py builds them (every pointer the
    same fake address would make any table match, so the weights and
    gradients get distinct ones) and the matching Adam table."""
    abi = pkg.abi
    H, A, D = 50, 3, 12
    d = abi.MarlnavPpoDims(num_parallel=8, num_steps=2, num_agents=A, obs_dim=D, hidden_size=H)
    b = abi.MarlnavPpoBuffers()
    for k, f in enumerate(abi.PPO_BUFFER_FIELDS):
        setattr(b, f, FAKE * (200 + k))
    fields = [f for f in abi.POLICY_WEIGHT_FIELDS if f.startswith(which)]
    sizes = ACTOR_SIZES(H, D) if which == "actor" else CRITIC_SIZES(H, A, D)
    ad, ab = _good_adam(pkg, sizes)
    for i, f in enumerate(fields):
        ab.param[i] = getattr(b, f)
        ab.grad[i] = getattr(b, "grad_" + f)
    return d, b, ad, ab, fields


def _update(pkg, which, d, b, ad, ab):
    lib = pkg.abi.load_library()
    ref = lambda x: None if x is None else ctypes.byref(x)
    if which == "actor":
        rc = lib.marlnav_ppo_actor_update(ref(d), ref(b), 0.01, 0.001, ref(ad), ref(ab), None)
    else:
        rc = lib.marlnav_ppo_critic_update(ref(d), ref(b), 0.01, ref(ad), ref(ab), None)
    return rc, lib.marlnav_last_error()


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_update_refuses_a_mismatched_adam_table(pkg, which):
    n = 6 if which == "actor" else 4
    # one slot too few / too many
    for count in (n - 1, n + 1):
        d, b, ad, ab, _ = _good_update(pkg, which)
        ad.num_tensors = count
        if count > n:
            ad.numel[n] = 1
            for f in pkg.abi.ADAM_POINTER_FIELDS:
                getattr(ab, f)[n] = FAKE * 7
        rc, msg = _update(pkg, which, d, b, ad, ab)
        assert rc == -1 and b"num_tensors" in msg and which.encode() in msg, (rc, msg)
    for slot in range(n):
        # a parameter pointer that is not the network's weight
        d, b, ad, ab, fields = _good_update(pkg, which)
        ab.param[slot] = FAKE * 9
        rc, msg = _update(pkg, which, d, b, ad, ab)
        assert rc == -1 and f"param[{slot}]".encode() in msg and fields[slot].encode() in msg, msg
        # a gradient pointer that is not that weight's .grad
        d, b, ad, ab, fields = _good_update(pkg, which)
        ab.grad[slot] = FAKE * 9
        rc, msg = _update(pkg, which, d, b, ad, ab)
        assert rc == -1 and f"grad[{slot}]".encode() in msg and fields[slot].encode() in msg, msg
        # a size that is not the weight's
        d, b, ad, ab, fields = _good_update(pkg, which)
        ad.numel[slot] += 1
        rc, msg = _update(pkg, which, d, b, ad, ab)
        assert rc == -1 and f"numel[{slot}]".encode() in msg, msg
    # two slots swapped: the right tensors in the wrong order
    d, b, ad, ab, _ = _good_update(pkg, which)
    for f in ("param", "grad"):
        arr = getattr(ab, f)
        arr[0], arr[1] = arr[1], arr[0]
    ad.numel[0], ad.numel[1] = ad.numel[1], ad.numel[0]
    rc, msg = _update(pkg, which, d, b, ad, ab)
    assert rc == -1 and b"param[0]" in msg, msg
    # the other network's table
    other = "critic" if which == "actor" else "actor"
    d, b, _, _, _ = _good_update(pkg, which)
    _, _, ad, ab, _ = _good_update(pkg, other)
    rc, msg = _update(pkg, which, d, b, ad, ab)
    assert rc == -1 and b"adam table" in msg, msg


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_update_validates_both_halves_before_any_launch(pkg, which):
    # the Adam half's own refusals
    d, b, ad, ab, _ = _good_update(pkg, which)
    ad.beta2 = 1.0
    rc, msg = _update(pkg, which, d, b, ad, ab)
    assert rc == -1 and b"beta2" in msg, msg
    d, b, ad, ab, _ = _good_update(pkg, which)
    ab.state = None
    rc, msg = _update(pkg, which, d, b, ad, ab)
    assert rc == -1 and b"state" in msg, msg
    d, b, ad, ab, _ = _good_update(pkg, which)
    assert _update(pkg, which, d, b, None, ab)[0] == -1
    assert _update(pkg, which, d, b, ad, None)[0] == -1
    # the PPO half's: bad dims, NULL structs, a NULL data pointer (checked by
    # the gradient call, which runs its checks before it launches)
    d, b, ad, ab, _ = _good_update(pkg, which)
    d.hidden_size = 513
    rc, msg = _update(pkg, which, d, b, ad, ab)
    assert rc == -1 and b"hidden_size" in msg, msg
    d, b, ad, ab, _ = _good_update(pkg, which)
    assert _update(pkg, which, None, b, ad, ab)[0] == -1
    assert _update(pkg, which, d, None, ad, ab)[0] == -1
    d, b, ad, ab, _ = _good_update(pkg, which)
    b.returns = None
    rc, msg = _update(pkg, which, d, b, ad, ab)
    assert rc == -1 and b"returns" in msg and b"NULL" in msg, msg


# ------------------------------------------------------------------ FusedAdam
def test_fused_adam_is_exported(pkg):
    assert "FusedAdam" in pkg.__all__ and pkg.FusedAdam is pkg.rollout.FusedAdam


def test_fused_adam_refuses_cpu_parameters(pkg):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.FusedAdam([torch.zeros(3, 4), torch.zeros(4)])


def test_fused_adam_refuses_weight_decay_and_amsgrad(pkg):
    p = [torch.zeros(3)]
    with pytest.raises(ValueError, match="weight_decay.*unsupported"):
        pkg.FusedAdam(p, weight_decay=1e-2)
    with pytest.raises(ValueError, match="amsgrad.*unsupported"):
        pkg.FusedAdam(p, amsgrad=True)


def test_fused_adam_refuses_too_many_tensors(pkg):
    with pytest.raises(ValueError, match="1..8"):
        pkg.FusedAdam([torch.zeros(2) for _ in range(9)])
    with pytest.raises(ValueError, match="1..8"):
        pkg.FusedAdam([])
