"""The one-call rollout on the GPU: ``collect_fused`` (libmarlnav.so
``marlnav_rollout_collect``) against ``collect`` on an identically built
second env and policy.

Zero tolerance, derived and not measured: both sides run the same policy,
step and returns kernels on the same bits (the step families are bit-identical
to each other, the policy kernel's load widths do not change its arithmetic),
the new row-0 normaliser does the torch normaliser's one IEEE subtraction and
one IEEE division, and the flag merge is exact. So every comparison below is
for equal bits."""
import warnings
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from conftest import assert_bits_equal, cli_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAMMA = 0.9

# (P, A, O, H, T), each the smallest that reaches its path
SHAPES = [
    (2, 3, 3, 50, 3),     # the reference's default, tiny grid
    (67, 3, 3, 50, 5),    # block family, partial second block; odd P: action rows at odd t are
                          # 8-byte aligned only, done rows start at odd bytes, 335 flag bytes
    (347, 3, 3, 7, 4),    # first odd P whose step writes >= 64 KiB (written-through stores
                          # into buffer rows); odd H
    (129, 3, 8, 50, 3),   # block family at A3 O8
    (5, 16, 32, 16, 3),   # split family at A16 O32
    (130, 2, 1, 50, 4),   # block family at A2 O1
]


def np_(t):
    return t.detach().cpu().numpy()


def make_env(pkg, P, A, O, seed=21, normalizer=True, scaler=True, first=0, **extra):
    """An env with ``episode_len=2`` whose env i has run ``(first + i) % 3``
    steps: envs finish at different steps, finished and kept ones share
    blocks."""
    args = cli_args(num_parallel=P, num_agents=A, num_obstacles=O, episode_len=2,
                    risk_factor=2.0, distance_factor=3.0)
    params = pkg.set_env_params(args, DEV)
    params["rng"], params["seed"] = "native", seed
    params.update(extra)
    env = pkg.Env(params)
    if normalizer:
        env.attach_normalizer(pkg.ObsNormalizer(pkg.set_normalizer_params(args, DEV)))
    if scaler:
        env.attach_action_scaler(pkg.ActionScaler(pkg.set_scaler_params(args, DEV)))
    env._step_num = (torch.arange(P) + first) % 3
    return env


def make_policy(pkg, A, O, H, seed=5, **kw):
    """A FusedPolicy over seeded random weights of the reference's shapes."""
    D = 2 + 2 * O + 2 * (A - 1)
    g = torch.Generator().manual_seed(1234)
    lin = lambda o, i: NS(weight=(torch.randn(o, i, generator=g) / i ** 0.5).to(DEV),
                          bias=(0.1 * torch.randn(o, generator=g)).to(DEV))
    actor = NS(fc1=lin(H, D), fc_mu=lin(2, H), fc_std=lin(2, H))
    critic = NS(fc1=lin(H, A * D), fc2=lin(1, H))
    return pkg.FusedPolicy(actor, critic, seed=seed, **kw)


def assert_same(a, b, what):
    a, b = np_(a), np_(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if a.dtype == np.float32:
        assert_bits_equal(a, b, what)
    else:
        np.testing.assert_array_equal(a, b, what)


ENTRIES = ("obs", "actions", "log_probs", "values", "rewards", "done")
ENV_STATE = ("states", "obstacles", "target", "_step_num", "_terminates", "_reinit_mask")


def assert_rollouts_equal(fused, loop, T):
    """(env, policy, buffer, (mean, stats)) of the fused call and of the
    loop: everything the issue lists, then one further env.step on both."""
    (env_f, pol_f, buf_f, out_f), (env_l, pol_l, buf_l, out_l) = fused, loop
    assert len(buf_f) == len(buf_l) == T
    for k, name in enumerate(ENTRIES):
        assert_same(buf_f.stacked(k), buf_l.stacked(k), name)
    done = np_(buf_f.stacked(5))
    assert done.dtype == np.bool_ and done.any() and not done.all(), \
        "done must hold both values: no case passes without an episode ending"
    assert set(np.unique(np_(buf_f.stacked(5).view(torch.uint8)))) == {0, 1}
    np.testing.assert_array_equal(np_(buf_f.returns), np_(buf_l.returns))
    assert buf_f.returns.dtype == torch.float64
    assert float(out_f[0]) == float(out_l[0])
    assert out_f[1] == out_l[1] and sum(out_f[1].values()) > 0
    for name in ENV_STATE:
        assert_same(getattr(env_f, name), getattr(env_l, name), name)
    assert env_f._step_idx == env_l._step_idx
    assert env_f._engine.steps_done == env_l._engine.steps_done
    assert pol_f.step_idx == pol_l.step_idx
    assert (env_f._num_trunc, env_f._num_col, env_f._num_tar) == (0, 0, 0)
    acts = buf_l.stacked(1)[T - 1].clone()
    nxt_f, nxt_l = env_f.step(acts), env_l.step(acts.clone())
    assert_same(nxt_f[0]._packed, nxt_l[0]._packed, "next obs")
    assert_same(env_f._normalizer(nxt_f[0]), env_l._normalizer(nxt_l[0]), "next obs_norm")
    for k, name in ((1, "reward"), (2, "terminated"), (3, "truncated")):
        assert_same(nxt_f[k], nxt_l[k], "next " + name)
    for name in ENV_STATE:
        assert_same(getattr(env_f, name), getattr(env_l, name), "next " + name)


def run_pair(pkg, P, A, O, H, T, eps=None, **extra):
    fused_env, loop_env = make_env(pkg, P, A, O, **extra), make_env(pkg, P, A, O, **extra)
    fused_pol, loop_pol = make_policy(pkg, A, O, H), make_policy(pkg, A, O, H)
    fused_buf, loop_buf = pkg.RolloutBuffer(T), pkg.RolloutBuffer(T)
    out_f = pkg.collect_fused(fused_env, fused_pol, fused_buf, eps=eps, gamma=GAMMA)
    out_l = pkg.collect(loop_env, loop_pol, loop_buf, gamma=GAMMA,
                        eps_source=None if eps is None else (lambda t: eps[t]))
    fused = (fused_env, fused_pol, fused_buf, out_f)
    loop = (loop_env, loop_pol, loop_buf, out_l)
    assert_rollouts_equal(fused, loop, T)
    return fused, loop


@pytest.mark.parametrize("P,A,O,H,T", SHAPES)
def test_collect_fused_equals_collect(pkg, P, A, O, H, T):
    (env, pol, _, _), _ = run_pair(pkg, P, A, O, H, T)
    assert pol.step_idx == T and env._step_idx == 1 + T + 1   # T steps and the further one


def test_collect_fused_double_buffered_odd_T(pkg):
    """Odd T with a second states buffer: the buffers end swapped, and the
    further step of the comparison reads the right one."""
    P, A, O, H, T = 67, 3, 3, 50, 5
    probe = make_env(pkg, P, A, O, states_double_buffer=True)
    before = probe.states.data_ptr()
    pkg.collect_fused(probe, make_policy(pkg, A, O, H), pkg.RolloutBuffer(T))
    assert probe.states.data_ptr() != before
    pkg.collect_fused(probe, make_policy(pkg, A, O, H), pkg.RolloutBuffer(T + 1))
    swapped = probe.states.data_ptr()
    assert swapped != before                    # an even T keeps the current buffer
    pkg.collect_fused(probe, make_policy(pkg, A, O, H), pkg.RolloutBuffer(T))
    assert probe.states.data_ptr() == before
    run_pair(pkg, P, A, O, H, T, states_double_buffer=True)


def test_collect_fused_with_supplied_eps(pkg):
    P, A, O, H, T = 67, 3, 3, 50, 5
    eps = torch.randn(T, P * A, 2, generator=torch.Generator().manual_seed(3)).to(DEV)
    (_, pol, _, _), _ = run_pair(pkg, P, A, O, H, T, eps=eps)
    assert pol.step_idx == 0                    # the kernel's own stream was not used
    with pytest.raises(ValueError, match="eps"):
        pkg.collect_fused(make_env(pkg, P, A, O), make_policy(pkg, A, O, H),
                          pkg.RolloutBuffer(T), eps=eps[:-1])


def test_row_zero_is_the_torch_normaliser_of_the_observations(pkg):
    for P, A, O, H, T in SHAPES[:2] + SHAPES[3:5]:
        env, twin = make_env(pkg, P, A, O), make_env(pkg, P, A, O)
        buf = pkg.RolloutBuffer(T)
        pkg.collect_fused(env, make_policy(pkg, A, O, H), buf)
        want = twin._normalizer(twin.observations())
        assert_bits_equal(np_(buf.stacked(0)[0]), np_(want), f"row 0 of {P}x{A}x{O}")


def test_shards_fill_the_halves_of_the_whole(pkg):
    A, O, H, T, n = 3, 3, 50, 4, 64
    whole = make_env(pkg, 2 * n, A, O)
    buf = pkg.RolloutBuffer(T)
    pkg.collect_fused(whole, make_policy(pkg, A, O, H), buf)
    assert np_(buf.stacked(5)).any()
    for off in (0, n):
        env = make_env(pkg, n, A, O, env_offset=off, first=off)
        part = pkg.RolloutBuffer(T)
        pkg.collect_fused(env, make_policy(pkg, A, O, H, env_offset=off), part)
        for k, name in enumerate(ENTRIES):
            full = buf.stacked(k)
            if name == "log_probs":
                half = full.view(T, 2 * n, A)[:, off:off + n].reshape(T, n * A)
            else:
                half = full[:, off:off + n]
            assert_same(part.stacked(k), half, f"{name} of shard {off}")
        assert_same(env.states, whole.states[off:off + n], f"states of shard {off}")
    # a policy of another shard is refused by the library before any launch
    env = make_env(pkg, n, A, O, env_offset=n)
    with pytest.raises(RuntimeError, match="env_offset"):
        pkg.collect_fused(env, make_policy(pkg, A, O, H, env_offset=0), pkg.RolloutBuffer(T))
    assert env._step_idx == 1


def test_held_tensors_keep_their_pre_call_values(pkg):
    P, A, O, H, T = 67, 3, 3, 50, 3
    for extra in ({}, {"states_double_buffer": True}):
        env = make_env(pkg, P, A, O, **extra)
        held = {n: getattr(env, n) for n in ENV_STATE[:5]}
        was = {n: t.clone() for n, t in held.items()}
        buf = pkg.RolloutBuffer(T)
        pkg.collect_fused(env, make_policy(pkg, A, O, H), buf)
        for n, t in held.items():
            assert torch.equal(t, was[n]), n
            assert getattr(env, n).data_ptr() != t.data_ptr(), n
        assert not torch.equal(env.states, was["states"])
        del held
        twin = make_env(pkg, P, A, O, **extra)
        ref = pkg.RolloutBuffer(T)
        pkg.collect_fused(twin, make_policy(pkg, A, O, H), ref)
        for k, name in enumerate(ENTRIES):
            assert_same(buf.stacked(k), ref.stacked(k), name)
        assert_same(env.states, twin.states, "states")


# ------------------------------------------------- the flag merge at any placement
GUARD, FILL = 32, 0xA5      # guard bytes on either side of a flag region, and their fill


def collect_with_flags_at(pkg, P, A, O, H, T, done_offset, trunc_offset):
    """``collect_fused``'s call of marlnav_rollout_collect (rollout.py, from
    ``env._sync_params()`` to ``env._engine.rollout(...)``) on a fresh env and
    policy, with ``rollout.done`` and ``rollout.truncated`` taken at the given
    byte offsets past a 16-byte boundary inside larger uint8 allocations
    filled with FILL. -> (done region (T * P,), returns (T, P), the four guard
    slices), as numpy arrays."""
    abi = pkg.abi
    env, policy = make_env(pkg, P, A, O), make_policy(pkg, A, O, H)
    D = 2 + 2 * O + 2 * (A - 1)
    n = T * P
    buffer = pkg.RolloutBuffer(T)
    env._sync_params()
    if any(env._engine.shared_state()):
        env._unshare_state(multi_step=True)
    assert env._engine.fast_ok
    lib = abi.load_library()
    buffer.reserve(P, A, D, env.device)
    r = abi.MarlnavRolloutBuffers()
    for name, s in zip(abi.ROLLOUT_BUFFER_FIELDS, buffer._store):
        setattr(r, name, s.data_ptr())
    big = [torch.full((GUARD + 16 + n + GUARD,), FILL, dtype=torch.uint8, device=DEV)
           for _ in range(2)]
    regions = []
    for t, off in zip(big, (done_offset, trunc_offset)):
        assert t.data_ptr() % 16 == 0 and 0 <= off < 16
        regions.append(t[GUARD + off:GUARD + off + n])
        assert regions[-1].data_ptr() % 16 == off
    r.done, r.truncated, r.eps = regions[0].data_ptr(), regions[1].data_ptr(), None
    returns = torch.empty(T, P, dtype=torch.float64, device=DEV)
    stats = torch.empty(2, dtype=torch.float64, device=DEV)
    work = torch.empty(int(lib.marlnav_returns_work_size(P)), dtype=torch.float64, device=DEV)
    raw, last = env._new_obs(), env._new_obs()
    r.returns, r.returns_stats, r.returns_work = returns.data_ptr(), stats.data_ptr(), work.data_ptr()
    pd, pb = policy._dims, policy._bufs
    for f, t in policy._params:
        setattr(pb, f, t.data_ptr())
    pd.num_parallel = P
    env._engine.rollout(abi.fn_addr(lib.marlnav_rollout_collect), bytes(pd), bytes(pb), bytes(r),
                        raw.data_ptr(), last.data_ptr(), T, policy.seed, policy.step_idx,
                        float(GAMMA))
    torch.cuda.synchronize()
    guards = []
    for t, off in zip(big, (done_offset, trunc_offset)):
        guards += [np_(t[:GUARD + off]), np_(t[GUARD + off + n:])]
    return np_(regions[0]), np_(returns), guards


_aligned_flags = {}


def aligned_flags(pkg, T):
    """The run with both flag stacks on a 16-byte boundary, once per T."""
    if T not in _aligned_flags:
        _aligned_flags[T] = collect_with_flags_at(pkg, 67, 3, 3, 50, T, 0, 0)
    return _aligned_flags[T]


@pytest.mark.parametrize("done_offset,trunc_offset,T", [
    (0, 0, 5),        # head 0: 20 vectors and 15 tail bytes
    (1, 1, 5),        # head 15, vector body, tail
    (15, 15, 5),      # head 1
    (3, 3, 1),        # 67 bytes: head 13 + 3 vectors + tail 6
    (0, 4, 5),        # unequal placement: every byte singly
    (5, 0, 5)])
def test_flag_merge_at_every_placement(pkg, done_offset, trunc_offset, T):
    """merge_flags_kernel's head / vector / tail split and its all-bytes
    fallback are chosen from where ``done`` and ``truncated`` lie within 16
    bytes; Python's fresh allocations only ever give head 0, the C ABI takes
    any pointer. 67 x 3 x 3, 67 T flag bytes."""
    P, A, O, H = 67, 3, 3, 50
    want_done, want_returns, _ = aligned_flags(pkg, T)
    via_buffer = pkg.RolloutBuffer(T)
    pkg.collect_fused(make_env(pkg, P, A, O), make_policy(pkg, A, O, H), via_buffer, gamma=GAMMA)
    np.testing.assert_array_equal(want_done, np_(via_buffer.stacked(5).view(torch.uint8)).ravel(),
                                  "the helper's aligned run is collect_fused's")
    done, returns, guards = collect_with_flags_at(pkg, P, A, O, H, T, done_offset, trunc_offset)
    assert done.shape == (T * P,) and set(np.unique(done)) == {0, 1}, \
        "done must hold both values, and only 0 and 1"
    np.testing.assert_array_equal(done, want_done, "done")
    for g, what in zip(guards, ("before done", "after done", "before truncated",
                                "after truncated")):
        assert g.size >= GUARD and (g == FILL).all(), f"guard bytes {what} were written"
    assert returns.dtype == np.float64 and np.isfinite(returns).all()
    np.testing.assert_array_equal(returns, want_returns, "returns")


# ------------------------------------------------------------------- refusals
def untouched(env, policy):
    return env._engine.steps_done == 0 and env._step_idx == 1 and policy.step_idx == 0


def test_refuses_a_reference_rng_env(pkg):
    P, A, O, H, T = 8, 3, 3, 50, 3
    env = make_env(pkg, P, A, O, rng="reference")
    policy = make_policy(pkg, A, O, H)
    with pytest.raises(RuntimeError, match=r"native-RNG.*collect\(\)"):
        pkg.collect_fused(env, policy, pkg.RolloutBuffer(T))
    assert untouched(env, policy)
    env = make_env(pkg, P, A, O)
    env._init_sampler = lambda: None            # a user-assigned sampler: reference mode
    with pytest.raises(RuntimeError, match=r"init sampler.*collect\(\)"):
        pkg.collect_fused(env, policy, pkg.RolloutBuffer(T))
    assert untouched(env, policy)


@pytest.mark.parametrize("missing", ["normalizer", "scaler"])
def test_refuses_without_normaliser_or_scaler(pkg, missing):
    P, A, O, H, T = 8, 3, 3, 50, 3
    env = make_env(pkg, P, A, O, **{missing: False})
    policy = make_policy(pkg, A, O, H)
    with pytest.raises(RuntimeError, match=r"attach_normalizer.*attach_action_scaler.*collect"):
        pkg.collect_fused(env, policy, pkg.RolloutBuffer(T))
    assert untouched(env, policy)


def test_refuses_stream_capture_unless_allowed(pkg):
    P, A, O, H, T = 8, 3, 3, 50, 3
    env = make_env(pkg, P, A, O)
    policy = make_policy(pkg, A, O, H)
    buf = pkg.RolloutBuffer(T)
    env._sync_params()
    buf.reserve(P, A, 2 + 2 * O + 2 * (A - 1), env.device)
    torch.cuda.synchronize()
    assert not env.allow_graph_capture
    graph = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():             # torch notes the aborted capture is empty
        warnings.simplefilter("ignore", UserWarning)
        with pytest.raises(RuntimeError, match="allow_graph_capture"):
            with torch.cuda.graph(graph):
                pkg.collect_fused(env, policy, buf)
    torch.cuda.synchronize()
    assert untouched(env, policy) and len(buf) == 0
