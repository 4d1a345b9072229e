"""The env-block step's stage phase (csrc/kernel_block.h: the staging spans
by LDS-DMA spread over the block's waves; where kBlockWaveStage says so, each
wave's own actions by one register load and its spans issued behind one
branch on the wave index): every output and every state buffer equal to the
oracle's, rtol 0, at the four compiled shapes, on one full block, two (the
draw-wave twin where the shape has one) and a partial grid, in the three
block-trait modes; with the actions at an offset inside a larger allocation;
and with a buffer alignment that keeps the launch out of the block family."""
import ctypes

import pytest
import torch

from test_block_traits import (AUTO, GENERAL, NO_DRAW, RAN_FIXED, RAN_FIXED_DRAW, RAN_GENERAL,
                               STEPS, actions_for, assert_equals_oracle, env_outputs, make_env,
                               oracle_native, run_native)

DEV = "cuda"
FAMILY_BLOCK, FAMILY_WAVE = 1, 4  # MARLNAV_FAMILY_*
EP = 3  # every env truncates at steps 3, 6, 9, 12: the re-init reads the staged formation
SHAPES = [(3, 3), (3, 8), (3, 1), (2, 1)]  # kBlockVariants
# one full block, two, and five full blocks with a partial sixth
PS = [64, 128, 64 * 5 + 7]
HAS_FIXED = {(3, 3), (3, 8)}  # the shapes with BlockFixed instantiations


def expected_ran(P, A, O, mode):
    """What marlnav_step's selection rule launches: the specialised
    instantiation only on full grids of the shapes that have one, with the
    draw wave (O <= 3) unless the mode forbids it."""
    if mode == GENERAL or (A, O) not in HAS_FIXED or P % 64:
        return RAN_GENERAL
    return RAN_FIXED_DRAW if (mode == AUTO and O <= 3) else RAN_FIXED


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [AUTO, GENERAL, NO_DRAW])
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("A,O", SHAPES)
def test_staged_step_equals_oracle(pkg, A, O, P, mode):
    """12 steps with episode_len 3 with the env-block family forced (run_native
    forces it and asserts it on every step; the partial grid runs the general
    instantiation's partial-block path): outputs, states, obstacles, target,
    step_num, terminates and counters against the oracle, rtol 0. What an
    unforced partial grid launches: test_partial_grid_family_unforced."""
    outs, ran = run_native(pkg, P, A, O, EP, mode)
    assert ran == {expected_ran(P, A, O, mode)}
    exp = oracle_native(pkg, P, A, O, EP)
    for k in range(STEPS):
        assert_equals_oracle(outs[k], exp[k], A, O, f"P{P} A{A} O{O} mode{mode} step {k + 1}")
    assert outs[-1]["counters"][0] == 4 * P  # every env truncated four times


# what marlnav_step launches for 64 * 5 + 7 envs with no family forced: the
# env-block kernel, except at A3/O8, which the split rule keeps below ~11 700
# envs (the family table)
FAMILY_SPLIT = 2
PARTIAL_FAMILY = {(3, 3): FAMILY_BLOCK, (3, 8): FAMILY_SPLIT, (3, 1): FAMILY_BLOCK,
                  (2, 1): FAMILY_BLOCK}


@pytest.mark.gpu
@pytest.mark.parametrize("A,O", SHAPES)
def test_partial_grid_family_unforced(pkg, A, O):
    """No family forced: the partial grid takes the family it took before the
    stage phase changed (and, where that is the env-block kernel, its general
    instantiation), and equals the oracle."""
    P = PS[-1]
    lib = pkg.abi.load_library()
    prev = lib.marlnav_debug_force_block_traits(AUTO)
    prev_family = lib.marlnav_debug_force_family(0)  # MARLNAV_FAMILY_AUTO
    try:
        env = make_env(pkg, P, A, O, episode_len=EP, seed=99)
        exp = oracle_native(pkg, P, A, O, EP)
        for k, acts in enumerate(actions_for(P, A, STEPS)):
            res = env.step(acts.to(DEV))
            assert lib.marlnav_debug_last_family() == PARTIAL_FAMILY[(A, O)]
            assert lib.marlnav_debug_last_block_traits() == RAN_GENERAL
            assert_equals_oracle(env_outputs(env, *res), exp[k], A, O,
                                 f"unforced P{P} A{A} O{O} step {k + 1}")
    finally:
        lib.marlnav_debug_force_family(prev_family)
        lib.marlnav_debug_force_block_traits(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("A,O", [(3, 3), (2, 1)])
def test_actions_at_an_offset_inside_a_larger_allocation(pkg, A, O):
    """The actions at a 16-byte aligned offset that is no multiple of 1 KiB
    (nor of the 8-byte lane pitch times 64) inside a larger buffer: lane l of
    wave w reads its own (angle, accel) pair from there."""
    P = 128
    lib = pkg.abi.load_library()
    prev = lib.marlnav_debug_force_block_traits(AUTO)
    prev_family = lib.marlnav_debug_force_family(FAMILY_BLOCK)
    try:
        env = make_env(pkg, P, A, O, episode_len=EP, seed=99)
        exp = oracle_native(pkg, P, A, O, EP)
        off = 4 * 13  # floats: 208 bytes
        big = torch.full((off + P * A * 2 + 1024,), float("nan"), device=DEV)
        view = big[off:off + P * A * 2].view(P, A, 2)
        assert view.data_ptr() % 16 == 0 and view.data_ptr() % 1024 != 0
        for k, acts in enumerate(actions_for(P, A, STEPS)):
            view.copy_(acts)
            res = env.step(view)
            assert lib.marlnav_debug_last_family() == FAMILY_BLOCK
            assert lib.marlnav_debug_last_block_traits() == expected_ran(P, A, O, AUTO)
            assert_equals_oracle(env_outputs(env, *res), exp[k], A, O,
                                 f"offset actions A{A} O{O} step {k + 1}")
        assert torch.isnan(big[:off]).all() and torch.isnan(big[off + P * A * 2:]).all()
    finally:
        lib.marlnav_debug_force_family(prev_family)
        lib.marlnav_debug_force_block_traits(prev)


@pytest.mark.gpu
def test_unaligned_obstacles_leave_the_block_family(pkg):
    """Obstacles at a view 4 bytes off 16-byte alignment (through the C ABI:
    the Env only ever passes its own, aligned, buffers): the staging pieces
    need 16-byte aligned spans, so the launch leaves the env-block family for
    the generic wave kernel, also when the block family is forced, and still
    equals the oracle."""
    P, A, O = 128, 3, 3
    D = 2 + 2 * O + 2 * (A - 1)
    abi = pkg.abi
    lib = abi.load_library()
    prev_family = lib.marlnav_debug_force_family(FAMILY_BLOCK)
    try:
        env = make_env(pkg, P, A, O, episode_len=EP, seed=99)
        env._sync_params()
        exp = oracle_native(pkg, P, A, O, EP)
        big = torch.zeros(P * O * 2 + 1, device=DEV)
        obst = big[1:].view(P, O, 2)
        obst.copy_(env.obstacles)
        assert obst.data_ptr() % 16 == 4
        t = {"states": env.states.clone(), "obstacles": obst, "target": env.target.clone(),
             "step_num": torch.zeros(P, device=DEV),
             "terminates": torch.zeros(P, dtype=torch.uint8, device=DEV),
             "formation": env._formation.clone(),
             "obs": torch.empty(P, A, D, device=DEV), "reward": torch.empty(P, device=DEV),
             "terminated": torch.empty(P, dtype=torch.uint8, device=DEV),
             "truncated": torch.empty(P, dtype=torch.uint8, device=DEV),
             "counters": torch.zeros(3 * lib.marlnav_counter_slots(ctypes.byref(env._dims)),
                                     dtype=torch.int64, device=DEV)}
        b = abi.MarlnavStepBuffers()
        for name, x in t.items():
            setattr(b, name, x.data_ptr())
        for k, acts in enumerate(actions_for(P, A, STEPS)):
            a = acts.to(DEV).contiguous()
            b.actions = a.data_ptr()
            torch.cuda.synchronize()
            abi.check(lib.marlnav_step(ctypes.byref(env._dims), ctypes.byref(env._cparams),
                                       ctypes.byref(b), k + 1, None), lib)
            torch.cuda.synchronize()
            assert lib.marlnav_debug_last_family() == FAMILY_WAVE
            got = {n: t[n].cpu().numpy() for n in ("reward", "states", "obstacles", "target",
                                                   "step_num")}
            got.update({n: t[n].cpu().numpy().astype(bool)
                        for n in ("terminated", "truncated", "terminates")})
            got["obs"] = t["obs"].cpu().numpy()
            # (3, slots) per-slot partial counts, accumulated over the steps
            got["counters"] = t["counters"].view(3, -1).sum(1).cpu().numpy()
            assert_equals_oracle(got, exp[k], A, O, f"unaligned obstacles step {k + 1}")
    finally:
        lib.marlnav_debug_force_family(prev_family)
