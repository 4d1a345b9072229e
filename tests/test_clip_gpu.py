"""Global-norm gradient clipping in the device update on the GPU (DESIGN.md
§16): ``marlnav_adam_step_clipped`` through ``FusedAdam.step(max_grad_norm=)``,
``marlnav_ppo_*_update_clipped`` through ``FusedPPO.*_update``,
``marlnav_ppo_train_phase_clipped`` through ``training.train_phase`` and
``MAPPO`` with ``params['max_grad_norm']``.

Parity: truth is ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam`` in
float64 on the CPU, the reference side the same in float32, under the
criterion of tests/test_adam_gpu.py (``ppo_ref.Pooled``, ``FACTOR`` 4, floor
2^-24) per tensor for the parameter, both moments and the clipped ``.grad``;
``norm_out`` within 1e-12 of the float64 norm of the fp32 gradients. The
figures are printed past pytest's capture and appended to the file named by
MARLNAV_CLIP_PARITY_OUT, which is how profiles/clip_parity.txt was written.

Everything else is for equal bits, derived and not measured: the reduction
order is fixed and restated in tests/clip_ref.py, ``coef == 1.0`` multiplies
by one, and every launch path enqueues the same three launches after the same
gradient launches."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import clip_ref as cr
import ppo_ref as pp
import test_adam_gpu as tad
import test_gae_gpu as tga
import test_ppo_gpu as tg
import test_train_gpu as tt
from conftest import cli_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_NORM = 0.5
F64 = torch.float64


def norm_cell():
    return torch.zeros((), dtype=F64, device=DEV)


# ------------------------------------------------------------------ 1. parity
def torch_clipped_adam(params, grads, dtype, maximize, max_norm=MAX_NORM):
    """clip_grad_norm_ then Adam on the CPU in ``dtype``; -> per step
    ([(param, exp_avg, exp_avg_sq, clipped grad) per tensor], norm)."""
    ps = [p.detach().clone().to(dtype).requires_grad_(True) for p in params]
    opt = torch.optim.Adam(ps, lr=tad.LR, betas=tad.BETAS, eps=tad.EPS, maximize=maximize,
                           foreach=False)
    out = []
    for row in grads:
        for p, g in zip(ps, row):
            p.grad = g.detach().clone().to(dtype)       # a copy: the clip is in place
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        opt.step()
        out.append(([(tg.np_(p).copy(), tg.np_(opt.state[p]["exp_avg"]).copy(),
                      tg.np_(opt.state[p]["exp_avg_sq"]).copy(), tg.np_(p.grad).copy())
                     for p in ps], float(norm)))
    return out


_refs = {}


def references(name, maximize):
    key = (name, maximize)
    if key not in _refs:
        params, grads = tad.inputs(name)
        _refs[key] = (torch_clipped_adam(params, grads, torch.float64, maximize),
                      torch_clipped_adam(params, grads, torch.float32, maximize))
    return _refs[key]


def snapshot(adam):
    return [(tg.np_(p).copy(), tg.np_(m).copy(), tg.np_(v).copy(), tg.np_(p.grad).copy())
            for p, m, v in zip(adam.params, adam.exp_avg, adam.exp_avg_sq)]


def run_clipped(pkg, name, maximize, max_norm=MAX_NORM, rows=None):
    """FusedAdam.step(max_grad_norm=) over device copies of set ``name``;
    -> per step (snapshot, norm_out), the optimiser. max_norm None: step()."""
    params, grads = tad.inputs(name)
    adam = tad.fused_adam(pkg, tad.device_params(params), maximize)
    out = []
    for row in (grads if rows is None else rows):
        for p, g in zip(adam.params, row):
            p.grad.copy_(g)
        if max_norm is None:
            adam.step()
            out.append((snapshot(adam), None))
        else:
            cell = norm_cell()
            adam.step(max_grad_norm=max_norm, norm_out=cell)
            out.append((snapshot(adam), float(cell)))
    return out, adam


WHAT = tad.WHAT + ("clipped grad",)


def report(capsys, title, pooled, extra):
    text = "\n".join([f"{title} (largest |x - x64| / max|x64| over the steps, bound "
                      f"{pp.FACTOR:g} x max(reference, 2^-24))"]
                     + ["  " + line for line in pooled.lines()] + ["  " + extra])
    with capsys.disabled():
        print("\n" + text)
    out = os.environ.get("MARLNAV_CLIP_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(text + "\n")


@pytest.mark.parametrize("maximize", [False, True], ids=["minimize", "maximize"])
@pytest.mark.parametrize("name", list(tad.SETS))
def test_parity_over_six_steps(pkg, capsys, name, maximize):
    params, grads = tad.inputs(name)
    truth, ref = references(name, maximize)
    got, _ = run_clipped(pkg, name, maximize)
    names = [f"[{i}] {'x'.join(map(str, s))}" for i, s in enumerate(tad.SETS[name])]
    overall, worst_norm, coefs = pp.Pooled(), 0.0, []
    for step in range(tad.STEPS):
        pooled = pp.Pooled()
        for p in (pooled, overall):
            for i, key in enumerate(names):
                for j, what in enumerate(WHAT):
                    p.add(f"{key} {what}", got[step][0][i][j], ref[step][0][i][j],
                          truth[step][0][i][j])
        exact = math.sqrt(math.fsum(float(v) ** 2 for g in grads[step]
                                    for v in g.reshape(-1).double().tolist()))
        rel = abs(got[step][1] - exact) / exact
        worst_norm = max(worst_norm, rel)
        coefs.append(cr.coef(got[step][1], MAX_NORM))
        print(f"step {step}: norm {got[step][1]:.6e} (exact {exact:.6e}, rel {rel:.1e}), "
              f"torch64 {truth[step][1]:.6e}, coef {coefs[-1]:.3e}")
        assert rel <= 1e-12, (step, got[step][1], exact)
        assert not tad.held(pooled), (step, tad.held(pooled))
    report(capsys, f"Clipped Adam parity, {name}, maximize={maximize}, max_norm={MAX_NORM}, "
           f"{tad.STEPS} steps:", overall,
           f"norm_out against the fp64 norm: largest relative gap {worst_norm:.1e}; coef per "
           f"step {' '.join(f'{c:.3g}' for c in coefs)}")
    # SCALES moves the norm over seven decades: some steps clip, some do not
    assert min(coefs) < 1e-2 and max(coefs) == 1.0, coefs


# ------------------------------------------------- 2. the clip is what is seen
def test_the_moments_and_the_gradient_carry_the_coefficient(pkg):
    """Adam's first step is invariant to a rescaled gradient (m / sqrt(v) is
    its sign), so the parameters after one step cannot show the clip: the
    first moment and the stored gradient do, by the factor coef; the
    parameters do after a second step with another norm."""
    name = "actor 3x3"
    params, grads = tad.inputs(name)
    rows = [grads[3], grads[4]]                 # scales 10 and 1: two different norms
    clip, _ = run_clipped(pkg, name, True, rows=rows)
    plain, _ = run_clipped(pkg, name, True, max_norm=None, rows=rows)
    norm1, norm2 = clip[0][1], clip[1][1]
    coef = cr.coef(norm1, MAX_NORM)
    assert coef < 1e-2 and abs(norm2 - norm1) > 0.5 * norm2, (norm1, norm2)
    for i, g in enumerate(rows[0]):
        p_c, m_c, v_c, g_c = clip[0][0][i]
        p_u, m_u, v_u, g_u = plain[0][0][i]
        assert np.array_equal(tad.bits(g_u), tad.bits(g.numpy())), i      # step() leaves .grad
        assert np.array_equal(tad.bits(g_c), tad.bits(cr.clipped(g.numpy(), coef))), i
        scale = float(np.abs(m_u).max())
        # one fp32 rounding of g' and one of m on either side: 2^-22 of the largest entry
        assert float(np.abs(m_c - coef * m_u.astype(np.float64)).max()) <= 2.0 ** -22 * coef * scale
        assert float(np.abs(m_c).max()) < 2 * coef * scale
    moved = 0.0
    for i in range(len(rows[0])):
        p_c, p_u = clip[1][0][i][0], plain[1][0][i][0]
        moved = max(moved, float(np.abs(p_c.astype(np.float64) - p_u).max())
                    / float(np.abs(p_u).max()))
    # two steps of ~lr each whose mix of g1 and g2 differs (10 : 1 unclipped,
    # 1 : 1 clipped): a difference of the order of lr = 3e-4 of a parameter of
    # ~0.1, far above the 2^-24 of a rounding
    assert moved > 1e-5, moved


# ------------------------------------------- 3. coef == 1 is the unclipped call
def clip_slots(rows):
    return [g.numpy() for g in rows]


@pytest.mark.parametrize("max_norm", [math.inf, 1e30], ids=["inf", "1e30"])
def test_coef_one_is_the_unclipped_step(pkg, max_norm):
    params, grads = tad.inputs("table8")
    clip, adam_c = run_clipped(pkg, "table8", False, max_norm=max_norm)
    plain, adam_p = run_clipped(pkg, "table8", False, max_norm=None)
    for step in range(tad.STEPS):
        for i, (x, y) in enumerate(zip(clip[step][0], plain[step][0])):
            for j in range(4):
                assert np.array_equal(tad.bits(x[j]), tad.bits(y[j])), (step, i, WHAT[j])
            assert np.array_equal(tad.bits(x[3]), tad.bits(grads[step][i].numpy())), (step, i)
        assert clip[step][1] == cr.norm(clip_slots(grads[step])), step     # still the norm
    assert adam_c.step_count() == adam_p.step_count() == tad.STEPS
    assert adam_c._norm_work is not None and adam_p._norm_work is None


@pytest.mark.parametrize("max_norm", [math.inf, 1e30], ids=["inf", "1e30"])
def test_coef_one_is_the_unclipped_update(pkg, max_norm):
    for name, w, data in tad.update_cases():
        T = data["returns"].shape[0]
        clip = tad.ppo_setup(pkg, w, data)
        plain = tad.ppo_setup(pkg, w, data)
        for _ in range(2):
            ppo, buf, par, adams = plain
            la = ppo.actor_update(buf, 0, T, adams["actor"])
            lc = ppo.critic_update(buf, 0, T, adams["critic"])
            ppo, buf, par, adams = clip
            na, nc = norm_cell(), norm_cell()
            la1 = ppo.actor_update(buf, 0, T, adams["actor"], max_grad_norm=max_norm, norm_out=na)
            lc1 = ppo.critic_update(buf, 0, T, adams["critic"], max_grad_norm=max_norm,
                                    norm_out=nc)
            assert float(la1) == float(la) and float(lc1) == float(lc), name
            tad.assert_same_bits(tad.full_state(clip[2], clip[3]),
                                 tad.full_state(plain[2], plain[3]))
            # (the fixture's critic gradient is exactly zero: both rows take the
            # clamped branch; its norm is 0.0 and the coefficient still 1)
            for cell, keys in ((na, pp.ACTOR_PARAMS), (nc, pp.CRITIC_PARAMS)):
                assert float(cell) == cr.norm([tg.np_(par[k].grad) for k in keys]), name
            assert float(na) > 0.0, name
        assert clip[3]["actor"].step_count() == 2 and clip[3]["critic"].step_count() == 2


# ---------------------------------------------------------- 4. partition edges
def c_step_clipped(pkg, quads, state, work, out, maximize, max_norm=MAX_NORM):
    """``marlnav_adam_step_clipped`` through ctypes, as test_adam_gpu.c_step."""
    abi = pkg.abi
    lib = abi.load_library()
    d = abi.MarlnavAdamDims(num_tensors=len(quads), maximize=int(maximize), lr=tad.LR,
                            beta1=tad.BETAS[0], beta2=tad.BETAS[1], eps=tad.EPS)
    b = abi.MarlnavAdamBuffers(state=state.data_ptr())
    for i, quad in enumerate(quads):
        d.numel[i] = quad[0].numel()
        for f, t in zip(abi.ADAM_POINTER_FIELDS, quad):
            getattr(b, f)[i] = t.data_ptr()
    need = int(lib.marlnav_grad_norm_work_size(ctypes.byref(d)))
    assert 1 <= need <= work.numel() - 2
    abi.check(lib.marlnav_adam_step_clipped(ctypes.byref(d), ctypes.byref(b), max_norm,
                                            work[1:].data_ptr(), out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), lib)
    return need


# one block covers 256 threads x 4 elements; the second stage has 256 threads
@pytest.mark.parametrize("numel", [1023, 1024, 1025, 256 * 1024 + 1])
def test_partition_edges_stay_in_bounds_and_match_clip_ref(pkg, numel):
    gen = torch.Generator().manual_seed(numel)
    p0 = 0.1 * torch.randn(numel, generator=gen)
    rows = [torch.randn(numel, generator=gen), 1e-4 * torch.randn(numel, generator=gen)]
    lib = pkg.abi.load_library()
    runs = {}
    for shifted in (False, True):
        state = torch.zeros(int(lib.marlnav_adam_state_size()) // 8, dtype=torch.int64, device=DEV)
        # the partials scratch between two sentinels of its own
        blocks = (((numel + 3) // 4) + 255) // 256
        work = torch.full((blocks + 2,), tad.SENTINEL, dtype=F64, device=DEV)
        quad, bufs = [], []
        for src in (p0, torch.zeros(numel), torch.zeros(numel), torch.zeros(numel)):
            view, buf = tad.sentinel_view(src, offset=1 if shifted else 4)
            assert (view.data_ptr() % 16 != 0) == shifted
            quad.append(view)
            bufs.append((view, buf))
        norms, stored = [], []
        for g in rows:
            quad[1].copy_(g)
            out = norm_cell()
            assert c_step_clipped(pkg, [quad], state, work, out, True) == blocks
            norms.append(float(out))
            stored.append(tg.np_(quad[1]).copy())
        torch.cuda.synchronize()
        assert int(state[0]) == len(rows)
        for view, buf in bufs:
            off = view.storage_offset()
            outside = torch.cat([buf[:off], buf[off + view.numel():]])
            assert bool((outside == tad.SENTINEL).all()), "a sentinel was overwritten"
        assert float(work[0]) == tad.SENTINEL and float(work[-1]) == tad.SENTINEL
        assert np.array_equal(tg.np_(work[1:-1]), cr.block_partials([rows[-1].numpy()]))
        runs[shifted] = (norms, stored, [tg.np_(quad[k]).copy() for k in (0, 2, 3)])
    for s, g in enumerate(rows):
        want = cr.norm([g.numpy()])
        assert runs[False][0][s] == want and runs[True][0][s] == want, (s, runs[False][0][s], want)
        c = cr.coef(want, MAX_NORM)
        assert (c < 1.0) == (s == 0)            # the first gradient is clipped, the second not
        for shifted in (False, True):
            assert np.array_equal(tad.bits(runs[shifted][1][s]),
                                  tad.bits(cr.clipped(g.numpy(), c))), (s, shifted)
    for a, b in zip(runs[False][2], runs[True][2]):
        assert np.array_equal(tad.bits(a), tad.bits(b))
    assert not np.array_equal(runs[False][2][0], p0.numpy())


# ------------------------------------------------------ 5. determinism and paths
def setup(pkg, w, data, mode):
    """(ppo, buffer, parameters, {network: FusedAdam}) in advantage mode
    ``mode``; in the GAE mode the returns serve as advantages and the critic's
    targets are the stored values moved by a seeded 5%."""
    if mode == "reference":
        return tad.ppo_setup(pkg, w, data)
    g = torch.Generator().manual_seed(77)
    shape = data["returns"].shape
    vt = data["values"].reshape(shape).double() + \
        (0.05 * torch.randn(shape, generator=g, dtype=F64)).to(data["values"].device)
    ppo, buf, par = tga.fused_gae(pkg, w, data, vt)
    adams = {"actor": tad.fused_adam(pkg, [par[k] for k in pp.ACTOR_PARAMS], True),
             "critic": tad.fused_adam(pkg, [par[k] for k in pp.CRITIC_PARAMS], False)}
    return ppo, buf, par, adams


def run_paths(pkg, w, data, mode, nets, epochs, batch, max_norm):
    """The three launch paths of a clipped phase -> {path: (losses, norms,
    state)} per network in ``nets``."""
    out = {}
    n = data["returns"].shape[0]
    bounds = pkg.minibatch_bounds(n, batch)
    U = epochs * len(bounds)
    for path in ("phase", "phase again", "updates", "grad + step"):
        ppo, buf, par, adams = setup(pkg, w, data, mode)
        losses, norms = {}, {}
        for k in nets:
            if path.startswith("phase"):
                cells = torch.zeros(U, dtype=F64, device=DEV)
                loss = pkg.training.train_phase(ppo, buf, adams[k], k, epochs, batch,
                                                max_grad_norm=max_norm, norm_out=cells)
                losses[k], norms[k] = tt.losses(loss), tt.losses(cells)
            elif path == "updates":
                ll, nl = [], []
                train = pkg.train_actor if k == "actor" else pkg.train_critic
                train(ppo, buf, adams[k], epochs, batch, log=ll, max_grad_norm=max_norm,
                      norm_log=nl)
                losses[k] = np.array([float(x) for x in ll])
                norms[k] = np.array([float(x) for x in nl])
            else:
                grad = ppo.actor_loss_grad if k == "actor" else ppo.critic_loss_grad
                ll, nl = [], []
                for _ in range(epochs):
                    for lo, hi in bounds:
                        ll.append(grad(buf, lo, hi))
                        nl.append(norm_cell())
                        adams[k].step(max_grad_norm=max_norm, norm_out=nl[-1])
                losses[k] = np.array([float(x) for x in ll])
                norms[k] = np.array([float(x) for x in nl])
        state = tad.full_state(par, adams)
        out[path] = (losses, norms, state)
    return out, U


def assert_paths_agree(out, nets, U, max_norm, what):
    first = out["phase"]
    for k in nets:
        assert first[0][k].shape == first[1][k].shape == (U,), (what, k)
        # most updates of these cases are clipped (a critic minibatch whose
        # rows all take the clamped branch has the gradient 0 and the norm 0.0)
        assert np.isfinite(first[0][k]).all() and np.isfinite(first[1][k]).all(), (what, k)
        assert (first[1][k] >= 0.0).all() and (first[1][k] > max_norm).sum() >= U // 2, \
            (what, k, first[1][k])
        assert first[2][k + " count"] == U
    for path in ("phase again", "updates", "grad + step"):
        for k in nets:
            for j, name in ((0, "loss"), (1, "norm")):
                assert np.array_equal(tt.bits64(out[path][j][k]), tt.bits64(first[j][k])), \
                    (what, path, k, name, out[path][j][k], first[j][k])
        tad.assert_same_bits(out[path][2], first[2])


# 2 steps x 3 envs per minibatch; 854 actor elements (folded when unclipped)
# and 5 054 (never folded)
ACTOR_CASES = {"3x3": (3, 3, 50, 7), "16x32": (16, 32, 50, 101)}
# the largest max_norm below every update's norm would make the test vacuous
# (coef == 1): well below the norms these cases have (printed by the test)
PATH_MAX_NORM = 1e-3


@pytest.mark.parametrize("mode", ["reference", "gae"])
@pytest.mark.parametrize("name", sorted(ACTOR_CASES))
def test_every_path_of_a_clipped_phase_stores_the_same_bits(pkg, name, mode):
    A, O, H, seed = ACTOR_CASES[name]
    w, data = tt.case(5, 3, A, O, H, seed)
    assert pkg.minibatch_bounds(5, 2) == [(0, 2), (2, 4)]
    nets = ("actor", "critic")
    out, U = run_paths(pkg, w, data, mode, nets, 2, 2, PATH_MAX_NORM)
    print({k: out["phase"][1][k] for k in nets})
    assert U == 4
    assert_paths_agree(out, nets, U, PATH_MAX_NORM, (name, mode))
    for k in w:
        assert not np.array_equal(out["phase"][2][k], w[k].numpy()), f"{name}: {k} did not move"
    # and the clip is in what is stored: not the unclipped phase's bits
    ppo, buf, par, adams = setup(pkg, w, data, mode)
    for k in nets:
        pkg.training.train_phase(ppo, buf, adams[k], k, 2, 2)
    plain = tad.full_state(par, adams)
    assert any(not np.array_equal(plain[k], out["phase"][2][k]) for k in w)


@pytest.mark.parametrize("mode", ["reference", "gae"])
@pytest.mark.parametrize("P", [1 << 17, (1 << 17) + 1])
def test_the_critic_on_both_sides_of_its_fold_limit(pkg, P, mode):
    """test_train_gpu's two sizes around 2^17 env rows: the unclipped critic
    folds at the first and not at the second, the clipped one at neither."""
    w, data = tt.device_case(pkg, 2, P, 3, 3, 5, 31)
    assert pkg.minibatch_bounds(2, 2) == [(0, 1)]
    out, U = run_paths(pkg, w, data, mode, ("critic",), 2, 2, PATH_MAX_NORM)
    print(out["phase"][1]["critic"])
    assert_paths_agree(out, ("critic",), U, PATH_MAX_NORM, (P, mode))


# -------------------------------------------------------------------- 6. graph
def test_a_captured_clipped_epoch_replays_as_the_eager_epochs(pkg):
    """After test_adam_gpu's captured epoch. max_norm is a launch argument:
    the graph holds the value of capture time."""
    buffer_len, batch_size, replays = 4, 2, 3
    w, data, _, _ = tg.generated(buffer_len, 40, 3, 3, 50, 404)
    assert pkg.minibatch_bounds(buffer_len, batch_size) == [(0, 2), (2, 3)]

    def epoch(s, max_norm=PATH_MAX_NORM):
        ppo, buf, par, adams = s
        pkg.train_actor(ppo, buf, adams["actor"], 1, batch_size, max_grad_norm=max_norm)
        pkg.train_critic(ppo, buf, adams["critic"], 1, batch_size, max_grad_norm=max_norm)

    eager = tad.ppo_setup(pkg, w, data)
    for _ in range(replays):
        epoch(eager)
    cap = tad.ppo_setup(pkg, w, data)
    ppo, buf, par, adams = cap
    start = {k: p.detach().clone() for k, p in par.items()}
    start_sd = {k: a.state_dict() for k, a in adams.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        epoch(cap, max_norm=7.0)                     # warm-up with another value: the scratch
    torch.cuda.current_stream().wait_stream(side)
    scratch = [a._norm_work.data_ptr() for a in adams.values()]
    with torch.no_grad():
        for k, p in par.items():
            p.copy_(start[k])
    for k, a in adams.items():
        a.load_state_dict(start_sd[k])
        assert a.step_count() == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        epoch(cap)
    assert scratch == [a._norm_work.data_ptr() for a in adams.values()]   # never reallocated
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()
    for a in list(adams.values()) + list(eager[3].values()):
        assert a.step_count() == 2 * replays
    tad.assert_same_bits(tad.full_state(cap[2], cap[3]), tad.full_state(eager[2], eager[3]))
    # the unclipped epochs leave other bits: the captured launches did clip
    plain = tad.ppo_setup(pkg, w, data)
    for _ in range(replays):
        pkg.train_actor(plain[0], plain[1], plain[3]["actor"], 1, batch_size)
        pkg.train_critic(plain[0], plain[1], plain[3]["critic"], 1, batch_size)
    a, b = tad.full_state(plain[2], plain[3]), tad.full_state(cap[2], cap[3])
    assert any(not np.array_equal(a[k], b[k]) for k in par)


# -------------------------------------------------------------------- 7. MAPPO
P7, A7, O7, H7, BL, BS, NE = 64, 3, 3, 50, 4, 2, 2


def make_mappo(pkg, out_dir, max_grad_norm):
    import test_rollout_gpu as tr
    args = cli_args(num_parallel=P7, num_agents=A7, num_obstacles=O7, episode_len=2,
                    risk_factor=2.0, distance_factor=3.0, hidden_size=H7, buffer_len=BL,
                    batch_size=BS, num_epochs=NE, learning_rate=tt.LR, num_total=2 * BL * P7)
    args.max_grad_norm = max_grad_norm
    env = tr.make_env(pkg, P7, A7, O7, seed=21, normalizer=False, scaler=False)
    torch.manual_seed(11)
    params = pkg.set_model_params(args, DEV)
    assert ("max_grad_norm" in params) == (max_grad_norm is not None)
    return pkg.MAPPO(params, env, seed=5, out_dir=str(out_dir)), args


def test_trainer_with_clipping_equals_the_hand_assembled_loop(pkg, tmp_path):
    G = PATH_MAX_NORM
    m, args = make_mappo(pkg, tmp_path / "clip", G)
    assert m.max_grad_norm == G
    s = tt.hand_loop(pkg, args, P7, A7, O7, H7)
    norms = {"actor": [], "critic": []}
    before = torch.cuda.get_sync_debug_mode()
    for r in range(2):
        torch.cuda.set_sync_debug_mode("error")
        try:
            m.repeat()
        finally:
            torch.cuda.set_sync_debug_mode(before)
        mean, stats = pkg.collect_fused(s["env"], s["policy"], s["buffer"], gamma=args.gamma)
        s["logs"]["mean_rews"].append(float(mean))
        s["logs"]["epi"].append(stats)
        pkg.train_actor(s["ppo"], s["buffer"], s["adam_a"], NE, BS, log=s["logs"]["actor"],
                        max_grad_norm=G, norm_log=norms["actor"])
        pkg.train_critic(s["ppo"], s["buffer"], s["adam_c"], NE, BS, log=s["logs"]["critic"],
                         max_grad_norm=G, norm_log=norms["critic"])
        tt.assert_trainer_equals_loop(m, s, r + 1)
    logs = m.logs()
    U = 2 * NE * len(pkg.minibatch_bounds(BL, BS))
    for k in ("actor", "critic"):
        got = logs[k + "_grad_norm"]
        assert len(got) == U == len(logs[k])
        assert all(math.isfinite(x) and x > 0.0 for x in got), got
        assert np.array_equal(tt.bits64(got), tt.bits64([float(x) for x in norms[k]])), k
    print({k: logs[k + "_grad_norm"] for k in ("actor", "critic")})
    # run(2) is the two repeats; save_stats leaves the two extra CSVs
    m2, _ = make_mappo(pkg, tmp_path / "clip2", G)
    m2.run(2)
    tad.assert_same_bits(
        tt.trainer_state(m2.actor, m2.critic, m2.actor_optimizer, m2.critic_optimizer),
        tt.trainer_state(m.actor, m.critic, m.actor_optimizer, m.critic_optimizer))
    files = m2.save_stats({"model": "x"}, plot=False)
    assert len(files) == 7
    assert sorted(f[len(m2._time):] for f in os.listdir(tmp_path / "clip2" / "logs")) == [
        "_act_gnorm.csv", "_act_loss.csv", "_cri_gnorm.csv", "_cri_loss.csv", "_epi_stats.csv",
        "_mean_rews.csv", "_params.json"]


def test_trainer_without_the_key_is_the_trainer_of_before(pkg, tmp_path):
    m, args = make_mappo(pkg, tmp_path / "plain", None)
    assert m.max_grad_norm is None and m._actor_norm_log is None
    s = tt.hand_loop(pkg, args, P7, A7, O7, H7)
    m.run(2)
    for r in range(2):
        tt.hand_repeat(pkg, s)
    tt.assert_trainer_equals_loop(m, s, 2)
    assert sorted(m.logs()) == ["actor", "critic", "epi_stats", "mean_rews"]
    assert m.actor_optimizer._norm_work is None
    files = m.save_stats({"model": "x"}, plot=False)
    assert len(files) == 5 and len(os.listdir(tmp_path / "plain" / "logs")) == 5


def test_cli_train_with_max_grad_norm_leaves_the_norm_logs(pkg, tmp_path, capsys):
    import json
    rc = pkg.cli.main(["--train", "--max-grad-norm", "0.5", "--gae-lambda", "0.95", "-se", "3",
                       "-np", "8", "-bl", "4", "-bs", "2", "-ne", "2", "-nt", "64", "-el", "3",
                       "--no-plots", "--out-dir", str(tmp_path)])
    assert rc == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["repeats"] == 2 and len(res["files"]) == 7
    for tail in ("_act_gnorm.csv", "_cri_gnorm.csv"):
        rows = open([f for f in res["files"] if f.endswith(tail)][0]).read().split()
        assert rows[0] == "Value" and len(rows) == 1 + 2 * 2 * 2
        # (a critic minibatch of 2 x 8 rows can have the gradient 0: norm 0.0)
        assert all(float(x) >= 0.0 and math.isfinite(float(x)) for x in rows[1:]), rows
        assert any(float(x) > 0.5 for x in rows[1:]), rows
    assert pkg.cli.main(["--train", "--max-grad-norm", "0", "-np", "8", "-bl", "4", "-bs", "2",
                         "-nt", "64", "--out-dir", str(tmp_path)]) == 2
    assert "max_grad_norm" in capsys.readouterr().err


# ---------------------------------------------------- 8. the in-block actor fold
@pytest.mark.parametrize("mode", ["reference", "gae"])
@pytest.mark.parametrize("name", ["tiny", "fold_last", "fold_first_out"])
def test_the_in_block_actor_fold_stores_the_unfolded_bits(pkg, name, mode):
    """``marlnav_debug_clip_fold(1)``: actor_finish forms the norm and the
    coefficient in-block and updates, two launches per actor update. Equal
    bits with the five launches at 854 actor elements (215 items, one block
    of the reduction), at 1 024 (257 items: two blocks, the largest folded
    actor) and at 1 041 (not folded: the same launches either way); the state
    block is compared whole, the coefficient in its last 8 bytes included."""
    _, _, A, O, H, seed = tt.PHASE_SHAPES[name]
    w, data = tt.case(5, 3, A, O, H, seed)
    lib = pkg.abi.load_library()
    runs = {}
    for fold in (0, 1):
        before = lib.marlnav_debug_clip_fold(fold)
        try:
            assert lib.marlnav_debug_clip_fold(-1) == fold
            ppo, buf, par, adams = setup(pkg, w, data, mode)
            cells = torch.zeros(4, dtype=F64, device=DEV)
            loss = pkg.training.train_phase(ppo, buf, adams["actor"], "actor", 2, 2,
                                            max_grad_norm=PATH_MAX_NORM, norm_out=cells)
            pkg.training.train_phase(ppo, buf, adams["critic"], "critic", 2, 2,
                                     max_grad_norm=PATH_MAX_NORM)
            runs[fold] = (tt.losses(loss), tt.losses(cells), tad.full_state(par, adams),
                          tg.np_(adams["actor"]._state).copy())
        finally:
            lib.marlnav_debug_clip_fold(before)
    for j, what in ((0, "loss"), (1, "norm")):
        assert np.array_equal(tt.bits64(runs[1][j]), tt.bits64(runs[0][j])), (what, runs[1][j])
    assert (runs[0][1] > PATH_MAX_NORM).all(), runs[0][1]          # every update is clipped
    tad.assert_same_bits(runs[1][2], runs[0][2])
    assert np.array_equal(runs[1][3], runs[0][3]) and runs[0][3][0] == 4
    assert 0.0 < runs[0][3][3:4].view(np.float64)[0] < 1.0         # the last update's coefficient
