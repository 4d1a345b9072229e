"""The fixed env-block instantiations' staging prologue (csrc/kernel_block.h
BlockFixed::prologue: the own-action load from an SGPR base and a 32-bit lane
offset, LDS-address-space staging destinations, partial spans under a literal
exec mask, a constant wait count per wave, the stage-time draw keyed by the
wave index, and the reward terms' short divisions compiled in): every output
and every state buffer equal to the oracle's, rtol 0."""
import ctypes

import numpy as np
import pytest
import torch

import oracle as orc
from test_block_traits import (AUTO, GENERAL, NO_DRAW, RAN_FIXED, RAN_FIXED_DRAW, RAN_GENERAL,
                               STEPS, actions_for, assert_equals_oracle, env_outputs, make_env,
                               np_, oracle_native, run_native)

DEV = "cuda"
FAMILY_BLOCK = 1  # MARLNAV_FAMILY_BLOCK
EP = 3  # every env truncates at steps 3, 6, 9, 12: the formation span and the draws feed outputs

# (P, A, O, mode, what runs): one block; 384x3x3, the smallest launch with
# written-through outputs (BlockFixed<true>); 128x3x8 and, above the 64 KB
# written-through threshold, 256x3x8 (no draw-wave twin at O = 8). Auto mode
# takes the draw-wave twin at grids of at most a block per CU.
INSTANCES = [
    (64, 3, 3, AUTO, RAN_FIXED_DRAW), (64, 3, 3, NO_DRAW, RAN_FIXED),
    (384, 3, 3, AUTO, RAN_FIXED_DRAW), (384, 3, 3, NO_DRAW, RAN_FIXED),
    (128, 3, 8, AUTO, RAN_FIXED), (256, 3, 8, AUTO, RAN_FIXED),
]


@pytest.mark.gpu
@pytest.mark.parametrize("P,A,O,mode,ran", INSTANCES)
def test_each_fixed_instantiation_equals_oracle(pkg, P, A, O, mode, ran):
    """12 steps, episode_len 3: every env is re-initialised four times from
    the staged formation and the stage-time draws."""
    outs, got_ran = run_native(pkg, P, A, O, EP, mode)
    assert got_ran == {ran}
    exp = oracle_native(pkg, P, A, O, EP)
    for k in range(STEPS):
        assert_equals_oracle(outs[k], exp[k], A, O, f"P{P} A{A} O{O} mode{mode} step {k + 1}")
    assert outs[-1]["counters"][0] == 4 * P


def _abi_buffers(pkg, env, P, A, O):
    """Device buffers of a step through the C ABI, initialised from `env`."""
    lib = pkg.abi.load_library()
    D = 2 + 2 * O + 2 * (A - 1)
    t = {"states": env.states.clone(), "obstacles": env.obstacles.clone(),
         "target": env.target.clone(), "step_num": torch.zeros(P, device=DEV),
         "terminates": torch.zeros(P, dtype=torch.uint8, device=DEV),
         "formation": env._formation.clone(),
         "obs": torch.empty(P, A, D, device=DEV), "reward": torch.empty(P, device=DEV),
         "terminated": torch.empty(P, dtype=torch.uint8, device=DEV),
         "truncated": torch.empty(P, dtype=torch.uint8, device=DEV),
         "counters": torch.zeros(3 * lib.marlnav_counter_slots(ctypes.byref(env._dims)),
                                 dtype=torch.int64, device=DEV)}
    b = pkg.abi.MarlnavStepBuffers()
    for name, x in t.items():
        setattr(b, name, x.data_ptr())
    return t, b


def _abi_outputs(t):
    got = {n: t[n].cpu().numpy() for n in ("reward", "states", "obstacles", "target", "step_num",
                                           "obs")}
    got.update({n: t[n].cpu().numpy().astype(bool)
                for n in ("terminated", "truncated", "terminates")})
    got["counters"] = t["counters"].view(3, -1).sum(1).cpu().numpy()
    return got


# the fixed (3,3) kernels; then every other way the env-block family reads
# actions: (3,8) fixed (two dword LDS-DMA loads per lane), the general kernel
# (64-bit lane addresses), and a partial last block (scalar reads)
OFFSET_CASES = [(384, 3, 3, AUTO, RAN_FIXED_DRAW), (384, 3, 3, NO_DRAW, RAN_FIXED),
                (128, 3, 8, AUTO, RAN_FIXED), (384, 3, 3, GENERAL, RAN_GENERAL),
                (64 * 5 + 7, 3, 3, AUTO, RAN_GENERAL)]


@pytest.mark.gpu
@pytest.mark.parametrize("P,A,O,mode,ran", OFFSET_CASES)
def test_actions_eight_bytes_into_their_storage_and_env_offset(pkg, P, A, O, mode, ran):
    """The actions as a view that starts 8 bytes into its storage (8-byte, not
    16-byte aligned: the lane pitch of the action load) and a non-zero
    env_offset (the Philox key's env id), through the C ABI: the Env would
    copy such a view to an aligned buffer."""
    off = 1000003
    abi = pkg.abi
    lib = abi.load_library()
    prev = lib.marlnav_debug_force_block_traits(mode)
    prev_family = lib.marlnav_debug_force_family(FAMILY_BLOCK)
    try:
        env = make_env(pkg, P, A, O, episode_len=EP, seed=99)
        env._sync_params()
        dm, pr, form = env._dims, env._cparams, np_(env._formation)
        dm.env_offset = off  # (this env is never stepped: only its dims, params and formation)
        st, ob, tg = orc.reinit_all(dm, pr, form, 0)
        t, b = _abi_buffers(pkg, env, P, A, O)
        for name, x in (("states", st), ("obstacles", ob), ("target", tg)):
            t[name].copy_(torch.from_numpy(x).view(t[name].shape))
        big = torch.full((2 + P * A * 2 + 64,), float("nan"), device=DEV)
        view = big[2:2 + P * A * 2].view(P, A, 2)
        assert view.data_ptr() % 16 == 8
        b.actions = view.data_ptr()
        sn, te = np.zeros(P, np.float32), np.zeros(P, np.bool_)
        tot = np.zeros(3, np.int64)
        for k, acts in enumerate(actions_for(P, A, STEPS)):
            exp = orc.step(dm, pr, st, ob, tg, sn, te, acts.numpy(), formation=form,
                           step_idx=k + 1)
            view.copy_(acts)
            torch.cuda.synchronize()
            abi.check(lib.marlnav_step(ctypes.byref(dm), ctypes.byref(pr), ctypes.byref(b), k + 1,
                                       None), lib)
            torch.cuda.synchronize()
            assert lib.marlnav_debug_last_family() == FAMILY_BLOCK
            assert lib.marlnav_debug_last_block_traits() == ran
            tot = tot + exp["counters"]
            exp["counters"] = tot
            assert_equals_oracle(_abi_outputs(t), exp, A, O,
                                 f"offset view P{P} O{O} mode{mode} step {k + 1}")
            st, ob, tg, sn, te = (exp[x] for x in ("states", "obstacles", "target", "step_num",
                                                   "terminates"))
        assert torch.isnan(big[:2]).all() and torch.isnan(big[2 + P * A * 2:]).all()
        assert tot[0] == 4 * P
    finally:
        lib.marlnav_debug_force_family(prev_family)
        lib.marlnav_debug_force_block_traits(prev)


def _run_against_oracle(pkg, env, actions, ran, where, lib):
    """Step `env` through `actions`; every output against the oracle started
    from the env's own buffers."""
    P, A = env.num_parallel, env.num_agents
    O = env.obstacles.shape[1]
    env._sync_params()
    dm, pr, form = env._dims, env._cparams, np_(env._formation)
    st, ob, tg = (np_(x).copy() for x in (env.states, env.obstacles, env.target))
    sn, te = np.zeros(P, np.float32), np.zeros(P, np.bool_)
    tot = np.zeros(3, np.int64)
    for k, acts in enumerate(actions):
        exp = orc.step(dm, pr, st, ob, tg, sn, te, acts.numpy(), formation=form, step_idx=k + 1)
        res = env.step(acts.to(DEV))
        assert lib.marlnav_debug_last_family() == FAMILY_BLOCK
        assert lib.marlnav_debug_last_block_traits() == ran, where
        tot = tot + exp["counters"]
        exp["counters"] = tot
        assert_equals_oracle(env_outputs(env, *res), exp, A, O, f"{where} step {k + 1}")
        st, ob, tg, sn, te = (exp[x] for x in ("states", "obstacles", "target", "step_num",
                                               "terminates"))
    return tot


@pytest.mark.gpu
@pytest.mark.parametrize("mode,ran", [(AUTO, RAN_FIXED_DRAW), (NO_DRAW, RAN_FIXED)])
def test_every_lane_moves_its_own_agent(pkg, mode, ran):
    """Lane l of wave w gets the action (env * A + agent) * 2^-12 in both
    components (below 0.29: inside [-pi, pi] and [min_accel, max_accel], so
    nothing clamps): a wrong lane offset moves the wrong agent, and the
    states say which."""
    P, A, O = 384, 3, 3
    lib = pkg.abi.load_library()
    prev = lib.marlnav_debug_force_block_traits(mode)
    try:
        env = make_env(pkg, P, A, O, episode_len=EP, seed=99)
        ids = (torch.arange(P * A, dtype=torch.float32) * 2.0 ** -12).view(P, A, 1)
        acts = ids.expand(P, A, 2).contiguous()
        assert float(acts.max()) < 0.5
        _run_against_oracle(pkg, env, [acts] * 4, ran, f"lane ids mode{mode}", lib)
    finally:
        lib.marlnav_debug_force_block_traits(prev)


@pytest.mark.gpu
def test_reward_parameters_outside_the_short_divisions_take_the_general_kernel(pkg):
    """init_dist = 2^-25 fails terms_fast_params: the fixed instantiations
    compile only the short reward-term divisions, so the launch takes the
    general kernel (and equals the oracle); the defaults take the fixed one."""
    P, A, O = 384, 3, 3
    lib = pkg.abi.load_library()
    prev = lib.marlnav_debug_force_block_traits(AUTO)
    try:
        env = make_env(pkg, P, A, O, episode_len=EP, seed=99)
        env._init_dist = 2.0 ** -25
        tot = _run_against_oracle(pkg, env, actions_for(P, A, 6), RAN_GENERAL, "init_dist 2^-25",
                                  lib)
        assert tot[0] == 2 * P
        env = make_env(pkg, P, A, O, episode_len=EP, seed=99)
        tot = _run_against_oracle(pkg, env, actions_for(P, A, 6), RAN_FIXED_DRAW, "defaults", lib)
        assert tot[0] == 2 * P
    finally:
        lib.marlnav_debug_force_block_traits(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,ran", [(AUTO, RAN_FIXED_DRAW), (NO_DRAW, RAN_FIXED)])
def test_non_finite_coordinate_in_one_block(pkg, mode, ran):
    """One NaN coordinate in block 2 of 6: that block takes the IEEE arm of
    the fixed kernel, next to the compiled-in reward terms of the others."""
    P, A, O = 384, 3, 3
    lib = pkg.abi.load_library()
    prev = lib.marlnav_debug_force_block_traits(mode)
    try:
        env = make_env(pkg, P, A, O, episode_len=50, seed=9)
        st = env.states.cpu().clone()
        st[2 * 64 + 5, 1, 0] = float("nan")
        env.states = st
        _run_against_oracle(pkg, env, actions_for(P, A, 3), ran, f"non-finite mode{mode}", lib)
    finally:
        lib.marlnav_debug_force_block_traits(prev)
