"""The env-block step with its launch-invariant choices compiled in
(BlockFixed, csrc/kernel_block.h): bit for bit the general instantiation and
the oracle on every output, launched exactly when the host's selection rule
holds (marlnav_step), and the testing hook that restricts the choice."""
import numpy as np
import pytest
import torch

from conftest import OBS_FIELDS, assert_obs_close, cli_args

import oracle as orc

DEV = "cuda"
AUTO, GENERAL, NO_DRAW = 0, 1, 2              # MARLNAV_BLOCK_TRAITS_*
RAN_GENERAL, RAN_FIXED, RAN_FIXED_DRAW = 0, 1, 2  # MARLNAV_BLOCK_RAN_*
STEPS = 12
OUTPUTS = ("obs", "reward", "terminated", "truncated", "states", "obstacles", "target",
           "step_num", "terminates", "counters")


def np_(t):
    return t.detach().cpu().numpy()


def make_env(pkg, P, A, O, episode_len=200, rng="native", seed=1234, **init_over):
    args = cli_args(num_parallel=P, num_agents=A, num_obstacles=O, episode_len=episode_len,
                    sampler_num=-1, max_step=1000)
    params = pkg.set_env_params(args, DEV)
    params["init"] = dict(params["init"], **init_over)
    if params["sampler"] is not None:
        params["sampler"] = dict(params["sampler"])
    params["rng"] = rng
    params["seed"] = seed
    return pkg.Env(params)


def actions_for(P, A, steps):
    g = torch.Generator().manual_seed(1000 * P + A)
    return [torch.stack([(torch.rand(P, A, generator=g) - 0.5) * 0.8,
                         (torch.rand(P, A, generator=g) - 0.5) * 1.2], 2) for _ in range(steps)]


def env_outputs(env, obs, rew, term, trunc):
    got = {"obs": obs._packed, "reward": rew, "terminated": term, "truncated": trunc,
           "states": env.states, "obstacles": env.obstacles, "target": env.target,
           "step_num": env._step_num, "terminates": env._terminates}
    out = {k: np_(v).copy() for k, v in got.items()}
    out["counters"] = np.array([env._num_trunc, env._num_col, env._num_tar], np.int64)
    return out


def run_native(pkg, P, A, O, ep, mode, steps=STEPS):
    """`steps` steps of a fresh native env under the hook's `mode`: every
    output of every step, and what each step launched. The env-block family
    is forced: 320x3x8 is a size the host otherwise gives the split kernel."""
    lib = pkg.abi.load_library()
    prev = lib.marlnav_debug_force_block_traits(mode)
    prev_family = lib.marlnav_debug_force_family(1)  # MARLNAV_FAMILY_BLOCK
    try:
        env = make_env(pkg, P, A, O, episode_len=ep, seed=99)
        outs, ran = [], set()
        for acts in actions_for(P, A, steps):
            res = env.step(acts.to(DEV))
            assert lib.marlnav_debug_last_family() == 1
            ran.add(lib.marlnav_debug_last_block_traits())
            outs.append(env_outputs(env, *res))
        return outs, ran
    finally:
        lib.marlnav_debug_force_family(prev_family)
        lib.marlnav_debug_force_block_traits(prev)


_ORACLE = {}


def oracle_native(pkg, P, A, O, ep, steps=STEPS):
    """The oracle's trajectory for run_native's seeds and actions (computed
    once per shape and episode length; the tests only read it)."""
    key = (P, A, O, ep, steps)
    if key not in _ORACLE:
        env = make_env(pkg, P, A, O, episode_len=ep, seed=99)
        env._sync_params()
        dm, pr = env._dims, env._cparams
        form = np_(env._formation)
        st, ob, tg = orc.reinit_all(dm, pr, form, 0)
        sn, te = np.zeros(P, np.float32), np.zeros(P, np.bool_)
        tot, outs = np.zeros(3, np.int64), []
        for k, acts in enumerate(actions_for(P, A, steps)):
            exp = orc.step(dm, pr, st, ob, tg, sn, te, acts.numpy(), formation=form,
                           step_idx=k + 1)
            tot = tot + exp["counters"]
            exp["counters"] = tot
            outs.append(exp)
            st, ob, tg, sn, te = (exp[x] for x in ("states", "obstacles", "target", "step_num",
                                                   "terminates"))
        _ORACLE[key] = outs
    return _ORACLE[key]


def assert_equals_oracle(got, exp, A, O, where):
    for name in OUTPUTS:
        if name == "obs":
            continue
        np.testing.assert_array_equal(got[name].reshape(exp[name].shape), exp[name],
                                      where + " " + name)
    fg, fo = orc.split_obs(got["obs"], A, O), orc.split_obs(exp["obs"], A, O)
    assert_obs_close(fg, dict(zip(OBS_FIELDS, fo)), prefix="", exact=True, where=where)


# 64 (one block), 192 (three) and 320x3x8 (five); 384x3x3 is the smallest
# multiple of 64 whose launch writes 64 KiB, where the host turns on
# written-through outputs: the BlockFixed<true> code of the headline size
SHAPES = [(64, 3, 3), (192, 3, 3), (320, 3, 8), (384, 3, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("ep", [200, 3])
@pytest.mark.parametrize("mode", [AUTO, NO_DRAW])
@pytest.mark.parametrize("P,A,O", SHAPES)
def test_fixed_equals_general_and_oracle(pkg, P, A, O, mode, ep):
    """Same seeds and actions, 12 steps: the specialised instantiation (with
    the draw wave in auto mode where the shape has one, without it in the
    no-draw mode) against the forced general one, rtol 0 on every output, and
    against the oracle. ep = 3: every env truncates and re-initialises inside
    the run (steps 3, 6, 9, 12)."""
    fixed, ran_fixed = run_native(pkg, P, A, O, ep, mode)
    general, ran_general = run_native(pkg, P, A, O, ep, GENERAL)
    assert ran_general == {RAN_GENERAL}
    assert ran_fixed == {RAN_FIXED_DRAW if (mode == AUTO and O <= 3) else RAN_FIXED}
    exp = oracle_native(pkg, P, A, O, ep)
    for k in range(STEPS):
        where = f"P{P} A{A} O{O} ep{ep} mode{mode} step {k + 1}"
        for name in OUTPUTS:
            np.testing.assert_array_equal(fixed[k][name], general[k][name], where + " " + name)
        assert_equals_oracle(fixed[k], exp[k], A, O, where)
    if ep == 3:
        assert fixed[-1]["counters"][0] == 4 * P  # every env truncated four times


@pytest.mark.gpu
def test_fixed_non_finite_block_matches_oracle(pkg):
    """A block with non-finite coordinates takes the IEEE pair math in the
    specialised instantiation as in the general one."""
    P, A, O = 128, 3, 3
    lib = pkg.abi.load_library()
    res = {}
    for mode in (NO_DRAW, AUTO, GENERAL):
        prev = lib.marlnav_debug_force_block_traits(mode)
        try:
            env = make_env(pkg, P, A, O, episode_len=50, seed=9)
            st = env.states.cpu().clone()
            st[3, 0, 0] = float("nan")
            st[70, 1, 2:4] = torch.tensor([float("inf"), 0.0])
            env.states = st
            env._sync_params()
            dm, pr, form = env._dims, env._cparams, np_(env._formation)
            s, o, t = st.numpy(), np_(env.obstacles).copy(), np_(env.target).copy()
            sn, te = np.zeros(P, np.float32), np.zeros(P, np.bool_)
            for k, acts in enumerate(actions_for(P, A, 3)):
                exp = orc.step(dm, pr, s, o, t, sn, te, acts.numpy(), formation=form,
                               step_idx=k + 1)
                obs, rew, term, trunc = env.step(acts.to(DEV))
                res.setdefault(k, []).append(np_(obs._packed).copy())
                where = f"mode{mode} step {k + 1}"
                np.testing.assert_array_equal(np_(env.states), exp["states"], where)
                np.testing.assert_array_equal(np_(rew), exp["reward"], where)
                np.testing.assert_array_equal(np_(term), exp["terminated"], where)
                np.testing.assert_array_equal(np_(env.obstacles), exp["obstacles"], where)
                s, o, t, sn, te = (exp[x] for x in ("states", "obstacles", "target", "step_num",
                                                    "terminates"))
            assert lib.marlnav_debug_last_block_traits() == {
                NO_DRAW: RAN_FIXED, AUTO: RAN_FIXED_DRAW, GENERAL: RAN_GENERAL}[mode]
        finally:
            lib.marlnav_debug_force_block_traits(prev)
    for k, (a, b, c) in res.items():
        np.testing.assert_array_equal(a, c, f"obs step {k + 1}")  # (NaN for NaN)
        np.testing.assert_array_equal(b, c, f"obs step {k + 1}")


def _setup_partial(pkg, env):
    return {}


def _setup_normalizer(pkg, env):
    args = cli_args(num_parallel=env.num_parallel, num_obstacles=3)
    env.attach_normalizer(pkg.ObsNormalizer(pkg.set_normalizer_params(args, DEV)))
    return {}


def _setup_scaler(pkg, env):
    args = cli_args(num_parallel=env.num_parallel, num_obstacles=3)
    env.attach_action_scaler(pkg.ActionScaler(pkg.set_scaler_params(args, DEV)))
    return {}


def _setup_bond(pkg, env):
    env._bond_sharpness = 0.05
    return {}


def _setup_reference(pkg, env):
    P, A, O = env.num_parallel, env.num_agents, 3
    g = torch.Generator().manual_seed(5)
    fresh = ((torch.rand(P, A, 5, generator=g) - 0.5) * 4, (torch.rand(P, O, 2, generator=g) - 0.5) * 40,
             (torch.rand(P, 1, 2, generator=g) - 0.5) * 40)
    env._init_sampler = lambda: fresh
    return {"fresh": tuple(x.numpy() for x in fresh)}


RULE_CASES = {
    "partial_last_block": (100, "native", _setup_partial),
    "fused_normaliser": (128, "native", _setup_normalizer),
    "action_scaler": (128, "native", _setup_scaler),
    "bond_sharpness": (128, "native", _setup_bond),
    "rng_reference": (128, "reference", _setup_reference),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(RULE_CASES))
def test_selection_rule_keeps_the_general_kernel(pkg, case):
    """Anything the specialised pack compiles out sends the launch to the
    general instantiation (auto mode), which still equals the oracle."""
    P, rng, setup = RULE_CASES[case]
    A, O = 3, 3
    lib = pkg.abi.load_library()
    prev = lib.marlnav_debug_force_block_traits(AUTO)
    try:
        extra = dict(noise_device="cpu") if rng == "reference" else {}
        env = make_env(pkg, P, A, O, episode_len=3, rng=rng, seed=99, **extra)
        step_kw = setup(pkg, env)
        env._sync_params()
        dm, pr = env._dims, env._cparams
        if rng == "native":
            step_kw["formation"] = np_(env._formation)
        st, ob, tg = (np_(x).copy() for x in (env.states, env.obstacles, env.target))
        sn, te = np.zeros(P, np.float32), np.zeros(P, np.bool_)
        tot = np.zeros(3, np.int64)
        for k, acts in enumerate(actions_for(P, A, 6)):
            exp = orc.step(dm, pr, st, ob, tg, sn, te, acts.numpy(), step_idx=k + 1, **step_kw)
            res = env.step(acts.to(DEV))
            assert lib.marlnav_debug_last_family() == 1  # MARLNAV_FAMILY_BLOCK
            assert lib.marlnav_debug_last_block_traits() == RAN_GENERAL, case
            tot = tot + exp["counters"]
            exp["counters"] = tot
            assert_equals_oracle(env_outputs(env, *res), exp, A, O, f"{case} step {k + 1}")
            st, ob, tg, sn, te = (exp[x] for x in ("states", "obstacles", "target", "step_num",
                                                   "terminates"))
        assert tot[0] >= P  # every env truncated and was re-initialised inside the run
    finally:
        lib.marlnav_debug_force_block_traits(prev)


@pytest.mark.gpu
def test_selection_rule_takes_the_fixed_kernel_by_default(pkg):
    """P = 128, every default: the specialised instantiation (two blocks: with
    the draw wave), and the general one only when forced."""
    lib = pkg.abi.load_library()
    prev = lib.marlnav_debug_force_block_traits(AUTO)
    try:
        env = make_env(pkg, 128, 3, 3)
        env.step(torch.zeros(128, 3, 2, device=DEV))
        assert lib.marlnav_debug_last_block_traits() == RAN_FIXED_DRAW
        lib.marlnav_debug_force_block_traits(NO_DRAW)
        env.step(torch.zeros(128, 3, 2, device=DEV))
        assert lib.marlnav_debug_last_block_traits() == RAN_FIXED
        lib.marlnav_debug_force_block_traits(GENERAL)
        env.step(torch.zeros(128, 3, 2, device=DEV))
        assert lib.marlnav_debug_last_block_traits() == RAN_GENERAL
    finally:
        lib.marlnav_debug_force_block_traits(prev)


def test_hook_rejects_unknown_modes_and_round_trips(pkg):
    """CPU only: needs nothing but the loaded library."""
    try:
        lib = pkg.abi.load_library()
    except (RuntimeError, OSError) as e:
        pytest.skip(f"libmarlnav.so does not load: {e}")
    first = lib.marlnav_debug_force_block_traits(AUTO)
    try:
        for bad in (-1, 3, 99):
            assert lib.marlnav_debug_force_block_traits(bad) == -1  # MARLNAV_EINVAL
            assert b"block traits" in lib.marlnav_last_error()
            assert lib.marlnav_debug_force_block_traits(AUTO) == AUTO  # (left unchanged)
        assert lib.marlnav_debug_force_block_traits(GENERAL) == AUTO
        assert lib.marlnav_debug_force_block_traits(NO_DRAW) == GENERAL
        assert lib.marlnav_debug_force_block_traits(AUTO) == NO_DRAW
        assert lib.marlnav_debug_last_block_traits() in (RAN_GENERAL, RAN_FIXED, RAN_FIXED_DRAW)
    finally:
        lib.marlnav_debug_force_block_traits(first)
