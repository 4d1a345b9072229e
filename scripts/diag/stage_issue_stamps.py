"""Stage phase of the env-block kernel per wave index, from the
MARLNAV_SUBSTAMPS=2 build (make -C marl-nav_amd/csrc substamps2): for each
wave w of the block, t0 -> its last staging load issued, -> its own actions
landed, -> every piece it issued landed, -> the stage barrier passed; median
and p90 in us (s_memrealtime: 10 ns ticks) over REPS (default 4) single steps
after WARM (default 150) steps.
usage: python scripts/diag/stage_issue_stamps.py 65536x3x3[,16384x3x3] [substamps2.so]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ["MARLNAV_LIB"] = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(
    ROOT, "marl-nav_amd", "lib", "substamps2.so")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import marlnav_amd as pkg  # noqa: E402


def main():
    for cfg in (sys.argv[1] if len(sys.argv) > 1 else "65536x3x3").split(","):
        P, A, O = (int(x) for x in cfg.split("x"))
        params = pkg.set_env_params(pkg.default_args(num_parallel=P, num_agents=A,
                                                     num_obstacles=O), "cuda")
        params["rng"], params["seed"] = "native", 5
        env = pkg.Env(params)
        lib = env._lib
        lib.marlnav_debug_stamps.argtypes = [ctypes.c_void_p]
        nb = P + 64
        buf = torch.zeros(nb * 24, dtype=torch.int64, device="cuda")
        assert lib.marlnav_debug_stamps(buf.data_ptr()) == 0
        g = torch.Generator(device="cuda").manual_seed(1234)
        acts = [torch.stack([torch.rand(P, A, generator=g, device="cuda") - 0.5,
                             torch.rand(P, A, generator=g, device="cuda") - 0.5], 2)
                for _ in range(8)]
        for i in range(int(os.environ.get("WARM", "150"))):
            env.step(acts[i % 8])
        rows, widx = [], []
        for rep in range(int(os.environ.get("REPS", "4"))):
            buf.zero_()  # one step per read-out: every stamp is from the same step
            env.step(acts[rep % 8])
            torch.cuda.synchronize()
            raw = buf.view(nb, 24).cpu().numpy().astype(np.int64)
            gidx = np.nonzero(raw[:, 0] > 0)[0]
            # waves per block: A, or A + 1 in the draw-wave instantiation
            wpb = A + 1 if gidx.max() >= (P // 64) * A else A
            rows.append(raw[gidx])
            widx.append(gidx % wpb)
        raw, widx = np.concatenate(rows), np.concatenate(widx)
        us = lambda c: raw[:, c] * 10.0 / 1e3  # noqa: E731
        t0, issued, acts_in, sincos, spans_in, barrier = us(0), us(23), us(20), us(21), us(22), us(2)
        ok = (raw[:, 20:24] > 0).all(axis=1)
        print(cfg, "lib", os.path.basename(os.environ["MARLNAV_LIB"]), "block traits ran",
              lib.marlnav_debug_last_block_traits(), "waves per block", wpb, flush=True)
        for w in range(A):
            m = ok & (widx == w)
            if not m.any():
                continue
            out = {}
            for name, t in (("t0->last_piece_issued", issued), ("t0->actions_landed", acts_in),
                            ("t0->sincos_done", sincos), ("t0->spans_landed", spans_in),
                            ("t0->stage_barrier", barrier)):
                d = (t - t0)[m]
                out[name] = (round(float(np.median(d)), 2), round(float(np.percentile(d, 90)), 2))
            print(cfg, f"wave {w} (n={int(m.sum())}) median, p90 us:", out, flush=True)
        del env


if __name__ == "__main__":
    main()
