"""bench.py's command line: what a plain run does and leaves out, --full,
and --dump-outputs."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

DUMPED = ("obs", "reward", "terminated", "truncated", "states")


def test_options():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--cpu-baseline", "on"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)
    assert bench.parse(["--full", "--cpu-baseline", "on"]).cpu_baseline == "on"


def _fake_step(P, A=3, D=12):
    g = torch.Generator().manual_seed(5)
    obs = types.SimpleNamespace(_packed=torch.rand(P, A, D, generator=g))
    out = (obs, torch.rand(P, generator=g), torch.rand(P, generator=g) < 0.3,
           torch.rand(P, generator=g) < 0.3)
    return out, torch.rand(P, A, 5, generator=g)


def test_dump_outputs_whole(tmp_path):
    out, states = _fake_step(37)
    bench.dump_outputs(str(tmp_path / "d"), out, states, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(n + ".npy" for n in DUMPED)
    got = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in DUMPED}
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["obs"], out[0]._packed.numpy())
    assert np.array_equal(got["reward"], out[1].numpy())
    assert np.array_equal(got["terminated"], out[2].numpy().astype(np.float32))
    assert np.array_equal(got["truncated"], out[3].numpy().astype(np.float32))
    assert np.array_equal(got["states"], states.numpy())


def test_dump_outputs_sample_and_ranks(tmp_path, monkeypatch):
    """Beyond the budget: the same seeded env rows every time, their indices
    beside them, the files within the budget; ranks above 0 name theirs."""
    out, states = _fake_step(1000)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 40000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, states, 0, 1)
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float64 and 0 < idx.size < 1000
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 1000
    i = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "obs.npy"), out[0]._packed.numpy()[i])
    assert np.array_equal(np.load(tmp_path / "a" / "states.npy"), states.numpy()[i])
    data = 0
    for n in DUMPED + ("env_index",):
        a, b = (np.load(tmp_path / d / (n + ".npy")) for d in ("a", "b"))
        assert np.array_equal(a, b), n
        data += a.nbytes
    assert data <= 40000
    bench.dump_outputs(str(tmp_path / "r"), out, states, 1, 2)
    assert "obs.rank1.npy" in os.listdir(tmp_path / "r")
    assert np.load(tmp_path / "r" / "env_index.rank1.npy").size <= idx.size // 2


def _run(monkeypatch, capsys, argv):
    for k in ("WORLD_SIZE", "LOCAL_RANK", "RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    assert bench.main() == 0
    (line,) = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    return json.loads(line)


@pytest.mark.gpu
def test_plain_run_is_lean_and_repeatable(pkg, monkeypatch, capsys, tmp_path):
    """A plain run takes no step beyond warm-up + timed ones (its outputs are
    those of an Env stepped W + K times with the same actions), measures
    nothing behind --full, and two runs write the same outputs."""
    W, K, P = 2, 5, 300
    argv = ["--gpus", "1", "--steps", str(K), "--warmup", str(W), "--envs", str(P),
            "--prewarm", "0.02"]
    monkeypatch.setattr(bench, "cpu_baseline", None)    # calling either one is an error
    monkeypatch.setattr(bench, "kernel_time_us", None)
    lines = [_run(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / d)])
             for d in ("a", "b")]
    for d in lines:
        assert d["steps"] == K and d["warmup"] == W and d["full"] is False
        assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["ms_per_step"] > 0
        assert d["value"] == pytest.approx(P * 1e3 / d["ms_per_step"], rel=1e-9)
        assert d["cpu_baseline"] is None and d["roofline"]["launch_us"] is None
        assert d["roofline"]["timed_region_frac"] > 0
    device = torch.device("cuda", 0)
    env = bench.make_env(pkg, P, 3, 3, device, 0)
    actions = bench.make_actions(P, 3, device, 0)
    for i in range(W):
        env.step(actions[i % len(actions)])
    for i in range(K):
        obs, rew, term, trunc = env.step(actions[i % len(actions)])
    want = {"obs": obs._packed, "reward": rew, "terminated": term, "truncated": trunc,
            "states": env.states}
    for n in DUMPED:
        a, b = (np.load(tmp_path / d / (n + ".npy")) for d in ("a", "b"))
        assert a.dtype == np.float32 and np.array_equal(a, b, equal_nan=True), n
        assert np.array_equal(a, want[n].float().cpu().numpy(), equal_nan=True), n


@pytest.mark.gpu
def test_full_run_fills_every_figure(monkeypatch, capsys):
    d = _run(monkeypatch, capsys, ["--full", "--steps", "4", "--warmup", "1", "--envs", "300",
                                   "--prewarm", "0.02", "--cpu-seconds", "0.2"])
    r = d["roofline"]
    assert d["full"] is True and d["steps"] == 4
    assert len(r["event_launch_us_passes"]) == 3 and r["launch_us"] > 0 and r["frac"] > 0
    assert r["graph_replay_launch_us"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["value_1thread"] > 0
