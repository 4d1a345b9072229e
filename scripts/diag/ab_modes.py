"""Same-box, same-process A/B of libmarlnav builds in both launch modes, one
raw line per measurement: for each shape, REPS (default 5) alternating
repetitions over the builds; each repetition makes a fresh Env on that build,
steps it PRE (default 300) steps to the steady mix of finished envs, then
times (graph) bench.kernel_time_us's hipGraph replay, median us per launch,
and (stream) K = 200 host-launched steps behind a device spin, HIP events
around them, median of 5 passes (scripts/diag/launch_modes.py's stream mode).
The last line per shape and mode gives each build's min / max and the gap.
usage: python scripts/diag/ab_modes.py 65536x3x3[,16384x3x3] parent.so new.so"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402


def stream_us(env, acts, K=200, passes=5):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(passes):
        torch.cuda._sleep(bench.SPIN_CYCLES)
        s.record()
        for i in range(K):
            env.step(acts[i % 16])
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / K)
    return sorted(out)[passes // 2]


def main():
    import marlnav_amd as pkg
    libs = sys.argv[2:]
    handles = [pkg.abi.load_library(p) for p in libs]
    names = [os.path.basename(p) for p in libs]
    reps, pre = int(os.environ.get("REPS", "5")), int(os.environ.get("PRE", "300"))
    dev = torch.device("cuda", 0)
    for cfg in sys.argv[1].split(","):
        P, A, O = (int(x) for x in cfg.split("x"))
        acts = bench.make_actions(P, A, dev, 0, n=16)
        params = pkg.set_env_params(pkg.default_args(num_parallel=P, num_agents=A,
                                                     num_obstacles=O), dev)
        params.update(rng="native", seed=20251003)
        bench.prewarm(pkg.Env(dict(params, _lib=handles[0])), acts, 0.3)  # clock ramp
        res = {(n, m): [] for n in names for m in ("graph", "stream")}
        for rep in range(reps):
            for n, h in zip(names, handles):
                env = pkg.Env(dict(params, _lib=h))
                for i in range(pre):
                    env.step(acts[i % 16])
                torch.cuda.synchronize()
                st = stream_us(env, acts)
                ran = (h.marlnav_debug_last_block_traits()
                       if hasattr(h, "marlnav_debug_last_block_traits") else -1)
                gr = bench.kernel_time_us(env, acts)[1]
                res[(n, "graph")].append(gr)
                res[(n, "stream")].append(st)
                print(f"{cfg} rep {rep} {n:>16s} block_traits {ran:2d} graph {gr:.3f} "
                      f"stream {st:.3f} us", flush=True)
                del env
        for m in ("graph", "stream"):
            a, b = res[(names[0], m)], res[(names[-1], m)]
            print(f"{cfg} {m:6s} {names[0]} min {min(a):.3f} max {max(a):.3f} "
                  f"(spread {max(a) - min(a):.3f}) | {names[-1]} min {min(b):.3f} "
                  f"max {max(b):.3f} | slowest new - fastest parent {max(b) - min(a):+.3f} "
                  f"median diff {sorted(b)[len(b) // 2] - sorted(a)[len(a) // 2]:+.3f}",
                  flush=True)


if __name__ == "__main__":
    main()
