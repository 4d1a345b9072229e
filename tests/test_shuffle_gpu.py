"""The shuffled-minibatch mode on the device. Everything here
has zero tolerance: bits of losses, every ``.grad``, parameters, both Adam
moments, step counts, norms and diagnostic rows.

The oracle of the gather kernels: a call over a list of steps equals the
existing contiguous call on a buffer whose storage was physically gathered
with ``index_select(0, steps)`` (tests/shuffle_ref.py ``gathered``). The
permutation kernel is held to tests/shuffle_ref.py's numpy restatement, the
phase call to the host loops over its own table. No test hands the kernels a
step outside the stored ones."""
import math

import numpy as np
import pytest
import torch

import ppo_ref as pp
import shuffle_ref as sr
import test_adam_gpu as tad
import test_ppo_gpu as tg
import test_rollout_gpu as tr
import test_train_gpu as tt
from conftest import cli_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 1234
MODES = ("reference", "gae")
NETS = ("actor", "critic")
NET_TAG = {"actor": sr.ACTOR, "critic": sr.CRITIC}


def bits(x):
    a = np.ascontiguousarray(tg.np_(x) if torch.is_tensor(x) else np.asarray(x))
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def value_targets(returns):
    """The GAE mode's second float64 (T, P) target, elementwise from the
    case's returns (so that gathering commutes with it)."""
    return 0.5 * returns + 0.25


def build(pkg, w, data, mode="reference"):
    """-> (ppo, buffer, parameters, the two FusedAdams) over device copies."""
    actor, critic, par = tg.modules(w)
    ppo = pkg.FusedPPO(actor, critic, tg.EPSILON, tg.ENT_CONST, advantage=mode)
    buf = tg.buffer_of(pkg, data)
    if mode == "gae":
        buf.advantages = data["returns"].to(DEV)
        buf.value_targets = value_targets(data["returns"]).to(DEV)
    adams = {"actor": tad.fused_adam(pkg, [par[k] for k in pp.ACTOR_PARAMS], True),
             "critic": tad.fused_adam(pkg, [par[k] for k in pp.CRITIC_PARAMS], False)}
    return ppo, buf, par, adams


def grads_of(par, net):
    keys = pp.ACTOR_PARAMS if net == "actor" else pp.CRITIC_PARAMS
    return {k: tg.np_(par[k].grad).copy() for k in keys}


def assert_call_equal(got, want, what):
    (lg, gg, dg), (lw, gw, dw) = got, want
    assert np.array_equal(bits(lg), bits(lw)), (what, "loss", float(lg), float(lw))
    assert math.isfinite(float(lg)), what
    for k in gw:
        assert np.array_equal(bits(gg[k]), bits(gw[k])), (what, k)
        assert np.abs(gw[k]).max() > 0, (what, k)
    if dw is not None:
        assert np.array_equal(bits(dg), bits(dw)), (what, "diag", tg.np_(dg), tg.np_(dw))


def call_steps(s, net, steps, diag=False):
    ppo, buf, par, _ = s
    row = torch.full((5,), -7.0, dtype=torch.float64, device=DEV) if diag else None
    if net == "actor":
        loss = ppo.actor_loss_grad_steps(buf, steps, diag_out=row)
    else:
        loss = ppo.critic_loss_grad_steps(buf, steps)
    return loss, grads_of(par, net), row


def call_range(s, net, lo, hi, diag=False):
    ppo, buf, par, _ = s
    row = torch.full((5,), -7.0, dtype=torch.float64, device=DEV) if diag else None
    if net == "actor":
        loss = ppo.actor_loss_grad(buf, lo, hi, diag_out=row)
    else:
        loss = ppo.critic_loss_grad(buf, lo, hi)
    return loss, grads_of(par, net), row


VARIANTS = (("actor", False), ("actor", True), ("critic", False))


# ------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,lo", [("tiny", 0), ("tiny", 1), ("chunks", 1)])
def test_a_range_as_a_step_list_is_the_contiguous_call(pkg, name, lo, mode):
    T, P, A, O, H, seed = tt.PHASE_SHAPES[name]
    w, data = tt.case(T + 1, P, A, O, H, seed)
    hi = T + 1
    for net, diag in VARIANTS:
        want = call_range(build(pkg, w, data, mode), net, lo, hi, diag)
        got = call_steps(build(pkg, w, data, mode), net, range(lo, hi), diag)
        assert_call_equal(got, want, (name, lo, mode, net, diag))


# --------------------------------------------------------------- 2. gather
# stored (T, P, A, O, H, seed) and a non-monotone step list with a repeat, at
# the smallest shapes that reach each addressing case
GATHER = {
    # several steps per tile; P A = 4 and N = 14 < 256: the n % N branch of the reference pairing
    "steps_per_tile_pa4": ((7, 2, 2, 1, 50, 11), [5, 0, 3, 3, 6, 1, 2]),
    "steps_per_tile": ((7, 5, 3, 3, 50, 12), [6, 2, 2, 0, 5]),
    # 201 rows per step: tiles straddle a step boundary at an offset, several per tile
    "straddle_offset": ((5, 67, 3, 3, 50, 13), [4, 1, 1, 3, 0, 2]),
    # blocks of >= 1 024 rows straddle steps (2 100 rows per step)
    "chunks": ((5,) + tt.PHASE_SHAPES["chunks"][1:], [3, 0, 4, 0]),
    "long_row": ((3,) + tt.PHASE_SHAPES["long_row"][1:], [2, 0, 2]),          # D + 1 > 256
    # six column tiles, the critic's own forward launch, dh through the workspace; P = 3
    "wide": ((3,) + tt.PHASE_SHAPES["wide"][1:], [1, 2, 1]),
    "unit_groups64": ((3,) + tt.PHASE_SHAPES["unit_groups64"][1:], [2, 2, 0]),
    "unit_groups_p65": ((3, 65, 3, 8, 7, 14), [1, 0, 1, 2]),                  # a critic tile straddles
    "fused64": ((3,) + tt.PHASE_SHAPES["fused64"][1:], [2, 0, 0]),            # critic_pass<64, kFused>
    "odd_row": ((3, 9, 3, 4, 8, 15), [2, 1, 2, 0]),                           # A D = 42: no vec4
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(GATHER))
def test_a_step_list_is_the_contiguous_call_on_the_gathered_buffer(pkg, name, mode):
    shape, steps = GATHER[name]
    w, data = tt.case(*shape)
    assert len(set(steps)) < len(steps) and steps != sorted(steps) and max(steps) < shape[0]
    phys = sr.gathered(data, steps)
    for net, diag in VARIANTS:
        want = call_range(build(pkg, w, phys, mode), net, 0, len(steps), diag)
        got = call_steps(build(pkg, w, data, mode), net, steps, diag)
        assert_call_equal(got, want, (name, mode, net, diag))
    # a CPU tensor and a numpy array are step lists too
    s = build(pkg, w, data, mode)
    a = call_steps(s, "critic", torch.tensor(steps, dtype=torch.int64))
    b = call_steps(s, "critic", np.array(steps, dtype=np.int32))
    assert_call_equal(a, b, name)


def test_update_steps_is_the_gradient_call_and_the_adam_step(pkg):
    shape, steps = GATHER["steps_per_tile"]
    w, data = tt.case(*shape)
    one, two = build(pkg, w, data), build(pkg, w, data)
    norm = torch.zeros(1, dtype=torch.float64, device=DEV)
    la = one[0].actor_update_steps(one[1], steps, one[3]["actor"])
    lc = one[0].critic_update_steps(one[1], steps, one[3]["critic"], max_grad_norm=0.05,
                                    norm_out=norm)
    wa = two[0].actor_loss_grad_steps(two[1], steps)
    two[3]["actor"].step()
    wc = two[0].critic_loss_grad_steps(two[1], steps)
    two[3]["critic"].step(max_grad_norm=0.05)
    assert np.array_equal(bits(la), bits(wa)) and np.array_equal(bits(lc), bits(wc))
    assert float(norm) > 0.0
    tad.assert_same_bits(tad.full_state(one[2], one[3]), tad.full_state(two[2], two[3]))
    with pytest.raises(ValueError, match="actor"):
        one[0].actor_update_steps(one[1], steps, one[3]["critic"])
    with pytest.raises(ValueError, match=r"train_phase\(shuffle="):
        one[0].actor_loss_grad_steps(one[1], torch.tensor(steps, device=DEV))
    for bad in ([], [0, shape[0]], [-1]):
        with pytest.raises(ValueError):
            one[0].critic_loss_grad_steps(one[1], bad)


# --------------------------------------------------- 3. the permutation kernel
@pytest.mark.parametrize("L,E", [(16, 4), (7, 300), (1, 2), (65535, 1)])
def test_the_permutation_kernel_is_the_restatement(pkg, L, E):
    lib = pkg.abi.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    for net in (sr.ACTOR, sr.CRITIC):
        for start in ((0, (1 << 32) + 5) if L < 1000 else ((1 << 32) + 5,)):
            cell = torch.tensor([start], dtype=torch.int64, device=DEV)
            guard = 3
            table = torch.full((E * L + 2 * guard,), -9, dtype=torch.int32, device=DEV)
            inner = table[guard:guard + E * L]
            for call in range(2):
                pkg.abi.check(lib.marlnav_minibatch_permutations(
                    L, E, SEED, net, cell.data_ptr(), inner.data_ptr(), stream), lib)
                got = tg.np_(inner).reshape(E, L)
                want = sr.permutations(L, E, SEED, net, counter=start + call)
                assert np.array_equal(got, want), (L, E, net, start, call)
                assert int(cell[0]) == start + call + 1       # advanced by exactly one
            assert (tg.np_(table[:guard]) == -9).all() and (tg.np_(table[-guard:]) == -9).all()


# ------------------------------------------------- 4. the phase and the loops
def run_phase(pkg, w, data, E, bs, mode="reference", seed=SEED, clip=None, **monitor):
    """``train_phase(shuffle=seed)`` for both networks on fresh state; ->
    (losses, state, extras) with the tables, the norms and the monitor's cells."""
    s = build(pkg, w, data, mode)
    ppo, buf, par, adams = s
    U = E * (len(buf) // bs)
    out, extra = {}, {"norms": {}, "tables": {}}
    for k in NETS:
        kw = dict(monitor) if k == "actor" else {}
        if clip is not None:
            extra["norms"][k] = torch.zeros(U, dtype=torch.float64, device=DEV)
            kw.update(max_grad_norm=clip, norm_out=extra["norms"][k])
        out[k] = tt.losses(pkg.training.train_phase(ppo, buf, adams[k], k, E, bs, shuffle=seed,
                                                    **kw))
        assert out[k].size == U
        extra["tables"][k] = tg.np_(ppo.last_steps[k]).copy()
        want = sr.permutations(len(buf), E, seed, NET_TAG[k], counter=0)
        assert np.array_equal(extra["tables"][k], want), k
        assert int(ppo._shuffle_counter[k][0]) == 1
    extra["norms"] = {k: tg.np_(v).copy() for k, v in extra["norms"].items()}
    extra["diag"], extra["stop"] = ppo.last_diag, ppo.last_stop
    return out, tad.full_state(par, adams), extra


def run_loops(pkg, w, data, E, bs, tables, mode="reference", clip=None):
    """The host loops over the same tables: rollout.train_actor / train_critic
    with ``steps_table``."""
    ppo, buf, par, adams = build(pkg, w, data, mode)
    logs = {k: [] for k in NETS}
    norms = {k: [] for k in NETS} if clip is not None else {k: None for k in NETS}
    pkg.train_actor(ppo, buf, adams["actor"], E, bs, log=logs["actor"], max_grad_norm=clip,
                    norm_log=norms["actor"], steps_table=tables["actor"])
    pkg.train_critic(ppo, buf, adams["critic"], E, bs, log=logs["critic"], max_grad_norm=clip,
                     norm_log=norms["critic"], steps_table=torch.from_numpy(tables["critic"]))
    out = {k: np.array([float(x) for x in v]) for k, v in logs.items()}
    norms = {k: np.array([float(x) for x in v]) for k, v in norms.items()} if clip else {}
    return out, tad.full_state(par, adams), norms


def assert_phase_equals_loops(pkg, w, data, E, bs, what, mode="reference", clip=None):
    got = run_phase(pkg, w, data, E, bs, mode, clip=clip)
    want = run_loops(pkg, w, data, E, bs, got[2]["tables"], mode, clip=clip)
    tt.assert_runs_equal(got[:2], want[:2], what)
    assert want[1]["actor count"] == want[1]["critic count"] == E * (data["returns"].shape[0] // bs)
    for k in w:
        assert not np.array_equal(got[1][k], w[k].numpy()), f"{what}: {k} did not move"
    for k in want[2]:
        assert np.array_equal(bits(got[2]["norms"][k]), bits(want[2][k])), (what, k, "norms")
        assert (want[2][k] > 0).all()
    return got, want


@pytest.mark.parametrize("L,bs", [(7, 3), (6, 3), (4, 4), (8, 2)])
def test_shuffled_phase_equals_the_loops(pkg, L, bs):
    w, data = tt.case(L, 3, 3, 3, 50, 77)
    assert_phase_equals_loops(pkg, w, data, 2, bs, (L, bs))


def test_shuffled_phase_equals_the_loops_over_many_blocks(pkg):
    T, P, A, O, H, seed = tt.PHASE_SHAPES["chunks"]
    w, data = tt.case(T + 1, P, A, O, H, seed)
    assert_phase_equals_loops(pkg, w, data, 1, 2, "chunks")      # minibatches of 2 and 3 steps


def test_shuffled_phase_with_a_clip_equals_the_loops(pkg):
    w, data = tt.case(7, 3, 3, 3, 50, 77)
    assert_phase_equals_loops(pkg, w, data, 2, 3, "clipped", clip=0.05)


def test_shuffled_phase_in_gae_mode_equals_the_loops(pkg):
    w, data = tt.case(7, 3, 3, 3, 50, 77)
    got, _ = assert_phase_equals_loops(pkg, w, data, 2, 3, "gae", mode="gae")
    ref = run_phase(pkg, w, data, 2, 3, "reference")
    assert not np.array_equal(got[0]["actor"], ref[0]["actor"])


def monitored_loop(pkg, w, data, E, bs, table, target):
    """The actor's host loop with the diagnostics and the stop decided on the
    host: -> (losses, rows, stopped_at, state)."""
    ppo, buf, par, adams = build(pkg, w, data)
    losses, rows, stopped = [], [], -1
    for perm in table:
        for steps in sr.minibatches(perm, bs):
            if stopped >= 0:
                losses.append(math.nan)
                rows.append([math.nan] * 4 + [2.0])
                continue
            row = torch.zeros(5, dtype=torch.float64, device=DEV)
            losses.append(float(ppo.actor_loss_grad_steps(buf, steps, diag_out=row)))
            row = tg.np_(row).copy()
            assert row[4] == 0.0
            if not row[2] <= target:
                stopped = len(losses) - 1
                row[4] = 1.0
            else:
                adams["actor"].step()
            rows.append(list(row))
    return np.array(losses), np.array(rows), stopped, tad.full_state(par, adams)


def actor_only(state):
    return {k: v for k, v in state.items() if "critic" not in k}


def test_shuffled_phase_with_diagnostics_equals_the_loop(pkg):
    L, bs, E = 7, 3, 2
    w, data = tt.case(L, 3, 3, 3, 50, 77)
    rows = torch.zeros(E * (L // bs), 5, dtype=torch.float64, device=DEV)
    got = run_phase(pkg, w, data, E, bs, diag_out=rows)
    assert got[2]["diag"] is rows
    want = monitored_loop(pkg, w, data, E, bs, got[2]["tables"]["actor"], math.inf)
    assert np.array_equal(bits(got[0]["actor"]), bits(want[0]))
    assert np.array_equal(bits(rows), bits(want[1])) and (want[1][:, 4] == 0).all()
    assert tg.np_(got[2]["stop"]).tolist() == [0, -1] and want[2] == -1
    tad.assert_same_bits(actor_only(got[1]), actor_only(want[3]))
    # monitoring changes no bit of the unmonitored shuffled phase
    plain = run_phase(pkg, w, data, E, bs)
    tt.assert_runs_equal(got[:2], plain[:2], "monitor only")


def test_shuffled_phase_stops_where_the_loop_stops(pkg):
    L, bs, E = 8, 2, 2
    w, data = tt.case(L, 3, 3, 3, 50, 77)
    free = run_phase(pkg, w, data, E, bs, target_kl=math.inf)
    kl = tg.np_(free[2]["diag"])[:, 2].copy()
    U = kl.size
    records = [j for j in range(1, U - 1) if kl[j] > kl[:j].max()]
    assert records, kl
    j = records[len(records) // 2]                          # a middle update
    target = math.sqrt(kl[j] * kl[:j].max())
    got = run_phase(pkg, w, data, E, bs, target_kl=target)
    want = monitored_loop(pkg, w, data, E, bs, got[2]["tables"]["actor"], target)
    assert want[2] == j and tg.np_(got[2]["stop"]).tolist() == [1, j]
    rows = tg.np_(got[2]["diag"])
    assert rows[:, 4].tolist() == [0.0] * j + [1.0] + [2.0] * (U - j - 1)
    assert np.array_equal(bits(rows), bits(want[1]))
    assert np.array_equal(bits(got[0]["actor"]), bits(want[0]))
    assert np.isnan(got[0]["actor"][j + 1:]).all() and np.isfinite(got[0]["actor"][:j + 1]).all()
    tad.assert_same_bits(actor_only(got[1]), actor_only(want[3]))
    assert got[1]["actor count"] == j
    with pytest.raises(ValueError, match="critic"):
        s = build(pkg, w, data)
        pkg.training.train_phase(s[0], s[1], s[3]["critic"], "critic", E, bs, shuffle=SEED,
                                 target_kl=1.0)


# ------------------------------------------------------ 5. the final step
def test_the_shuffled_critic_phase_trains_on_the_final_step(pkg):
    """L = bs = 4: the default phase's one minibatch is steps [0:3], so a
    change of step 3's value targets alone cannot move it; the shuffled
    minibatch holds all four steps."""
    L = 4
    w, data = tt.case(L, 3, 3, 3, 50, 77)
    other = dict(data)
    other["returns"] = data["returns"].clone()
    other["returns"][L - 1] += 1.0

    def critic(d, shuffle):
        ppo, buf, par, adams = build(pkg, w, d)
        loss = tt.losses(pkg.training.train_phase(ppo, buf, adams["critic"], "critic", 2, L,
                                                  shuffle=shuffle))
        state = tad.full_state(par, adams)
        return loss, {k: v for k, v in state.items() if "critic" in k}

    a, b = critic(data, None), critic(other, None)
    assert np.array_equal(bits(a[0]), bits(b[0]))
    tad.assert_same_bits(a[1], b[1])
    a, b = critic(data, SEED), critic(other, SEED)
    assert not np.array_equal(bits(a[0]), bits(b[0]))
    for k in pp.CRITIC_PARAMS:
        assert not np.array_equal(a[1][k], b[1][k]), k


# --------------------------------------------------------- 6. graph replay
def test_captured_shuffled_phases_draw_new_permutations_at_every_replay(pkg):
    L, bs, E = 8, 2, 1
    w, data = tt.case(L, 3, 3, 3, 50, 77)
    U = E * (L // bs)
    new_out = lambda: {k: torch.zeros(U, dtype=torch.float64, device=DEV) for k in NETS}

    def phases(s, out):
        ppo, buf, par, adams = s
        for k in NETS:
            pkg.training.train_phase(ppo, buf, adams[k], k, E, bs, out=out[k], shuffle=SEED)

    def warmed_up(s, out):
        """One call (workspace, counter cells, table), then the entry state
        again: the counters stand at 1."""
        ppo, buf, par, adams = s
        start = {k: p.detach().clone() for k, p in par.items()}
        start_sd = {k: a.state_dict() for k, a in adams.items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            phases(s, out)
        torch.cuda.current_stream().wait_stream(side)
        with torch.no_grad():
            for k, p in par.items():
                p.copy_(start[k])
        for k, a in adams.items():
            a.load_state_dict(start_sd[k])
            assert int(ppo._shuffle_counter[k][0]) == 1

    eager, eager_out = build(pkg, w, data), new_out()
    warmed_up(eager, eager_out)
    eager_tables = []
    for _ in range(2):
        phases(eager, eager_out)
        eager_tables.append({k: tg.np_(eager[0].last_steps[k]).copy() for k in NETS})

    cap, cap_out = build(pkg, w, data), new_out()
    warmed_up(cap, cap_out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        phases(cap, cap_out)
    tables = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        tables.append({k: tg.np_(cap[0].last_steps[k]).copy() for k in NETS})
    for k in NETS:
        assert not np.array_equal(tables[0][k], tables[1][k]), k
        for r in range(2):
            assert np.array_equal(tables[r][k], eager_tables[r][k]), (k, r)
            want = sr.permutations(L, E, SEED, NET_TAG[k], counter=1 + r)
            assert np.array_equal(tables[r][k], want), (k, r)
        assert int(cap[0]._shuffle_counter[k][0]) == 3
        assert np.array_equal(bits(cap_out[k]), bits(eager_out[k])), k
    for a in list(cap[3].values()) + list(eager[3].values()):
        assert a.step_count() == 2 * U
    tad.assert_same_bits(tad.full_state(cap[2], cap[3]), tad.full_state(eager[2], eager[3]))


# ------------------------------------------------------------- 7. the trainer
def make_mappo(pkg, tmp_path, extra=None, seed=5, P=96, A=3, O=3, H=50, L=6, bs=3, E=2,
               repeats=2):
    args = cli_args(num_parallel=P, num_agents=A, num_obstacles=O, episode_len=2,
                    risk_factor=2.0, distance_factor=3.0, hidden_size=H, buffer_len=L,
                    batch_size=bs, num_epochs=E, learning_rate=tt.LR,
                    num_total=repeats * L * P)
    env = tr.make_env(pkg, P, A, O, seed=21, normalizer=False, scaler=False)
    torch.manual_seed(11)
    params = pkg.set_model_params(args, DEV)
    params.update(extra or {})
    return pkg.MAPPO(params, env, seed=seed, out_dir=str(tmp_path))


def mappo_state(m):
    state = tt.trainer_state(m.actor, m.critic, m.actor_optimizer, m.critic_optimizer)
    logs = m.logs()
    for k in ("mean_rews", "actor", "critic"):
        state["log " + k] = np.array(logs[k], dtype=np.float64)
    return state


def test_mappo_without_the_option_is_mappo_with_it_off(pkg, tmp_path):
    a = make_mappo(pkg, tmp_path, P=3, L=3, bs=2, E=2)
    b = make_mappo(pkg, tmp_path, {"shuffle_minibatches": False}, P=3, L=3, bs=2, E=2)
    for m in (a, b):
        m.repeat()
        m.repeat()
        assert not m.shuffle_minibatches and m.ppo.last_steps == {}
    tad.assert_same_bits(mappo_state(a), mappo_state(b))


def test_mappo_with_shuffled_minibatches(pkg, tmp_path):
    L, bs, E = 6, 3, 2
    runs = []
    for seed in (5, 5, 6):
        m = make_mappo(pkg, tmp_path, {"shuffle_minibatches": True}, seed=seed, L=L, bs=bs, E=E)
        probe = torch.ones(1, device=DEV)
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                probe.item()                       # the mode bites on this build
            m.repeat()
            m.repeat()
        finally:
            torch.cuda.set_sync_debug_mode(before)
        logs = m.logs()
        U = E * (L // bs)
        assert len(logs["mean_rews"]) == 2 and len(logs["actor"]) == len(logs["critic"]) == 2 * U
        assert tuple(m._actor_log.shape) == tuple(m._critic_log.shape) == (2, U)
        assert all(math.isfinite(x) for x in logs["mean_rews"] + logs["actor"] + logs["critic"])
        tables = {k: tg.np_(m.ppo.last_steps[k]).copy() for k in NETS}
        for k in NETS:
            assert tables[k].shape == (E, L)
            assert (np.sort(tables[k], axis=1) == np.arange(L)).all()
            want = sr.permutations(L, E, seed, NET_TAG[k], counter=1)    # the second repeat
            assert np.array_equal(tables[k], want), k
        runs.append((mappo_state(m), tables))
    tad.assert_same_bits(runs[0][0], runs[1][0])
    for k in NETS:
        assert np.array_equal(runs[0][1][k], runs[1][1][k])
        assert not np.array_equal(runs[0][1][k], runs[2][1][k]), k
