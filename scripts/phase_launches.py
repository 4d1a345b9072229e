"""The launch sequence of every launch path of a PPO update (DESIGN.md §14,
"The launch paths"), for a kernel trace: after the setup (one rollout into
each buffer the named paths need) each path of ``--paths`` is run once and
nothing else.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- \\
        python scripts/phase_launches.py --paths all
    python scripts/phase_launches.py --list OUT/run_kernel_trace.csv

Shapes: the actor paths at P = 64, A = 3, O = 3 with two minibatches of T = 4
steps, H = 50 (854 actor elements: within the actor's fold limit) and H = 61
(1041: beyond it); the critic paths at P = 64 (folded) and at P = 16385 with
minibatches of T = 8 (131 080 env rows: beyond the critic's fold limit). One
epoch; the shuffled paths cut the stored steps into minibatches of 4 and 5 (8
and 9 at P = 16385).

Ahead of each path an int16 tensor is filled, a kernel nothing else here
launches: ``--list`` turns a trace into the ordered list of (kernel, grid,
workgroup, LDS bytes) of the library's update kernels with a ``## path`` line
at each of those fills, the text that two builds are compared by.
"""
import argparse
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("actor_pass", "actor_finish", "critic_pass", "critic_finish", "adam_advance",
           "adam_apply", "grad_sqsum", "minibatch_permutations")
# setup -> (P, H, buffer_len, batch_size)
SETUPS = {"h50": (64, 50, 9, 4), "h61": (64, 61, 9, 4), "big": (16385, 50, 17, 8)}
STEPS = [5, 0, 7, 2]
INF = float("inf")


def phase(setup, network, **kw):
    def run(pkg, m, batch):
        adam = m.actor_optimizer if network == "actor" else m.critic_optimizer
        pkg.training.train_phase(m.ppo, m.buffer, adam, network, 1, batch, **kw)
    return setup, run


def single(network, steps=None, **kw):
    def run(pkg, m, batch):
        adam = m.actor_optimizer if network == "actor" else m.critic_optimizer
        if steps is None:
            getattr(m.ppo, network + "_update")(m.buffer, 0, 4, adam, **kw)
        else:
            getattr(m.ppo, network + "_update_steps")(m.buffer, steps, adam, **kw)
    return "h50", run


def grad(network, steps=None, diag=False):
    def run(pkg, m, batch):
        import torch
        kw = {}
        if diag:
            kw["diag_out"] = torch.empty(pkg.abi.DIAG_ROW, dtype=torch.float64, device="cuda")
        if steps is None:
            getattr(m.ppo, network + "_loss_grad")(m.buffer, 0, 4, **kw)
        else:
            getattr(m.ppo, network + "_loss_grad_steps")(m.buffer, steps, **kw)
    return "h50", run


def clip_fold_off(path):
    setup, inner = path

    def run(pkg, m, batch):
        lib = pkg.abi.load_library()
        before = lib.marlnav_debug_clip_fold(0)
        try:
            inner(pkg, m, batch)
        finally:
            lib.marlnav_debug_clip_fold(before)
    return setup, run


PATHS = {
    # gradient-only entries
    "grad_actor": grad("actor"),
    "grad_actor_diag": grad("actor", diag=True),
    "grad_actor_steps": grad("actor", STEPS),
    "grad_actor_steps_diag": grad("actor", STEPS, True),
    "grad_critic": grad("critic"),
    "grad_critic_steps": grad("critic", STEPS),
    # single-update entries
    "update_actor": single("actor"),
    "update_actor_clipped": single("actor", max_grad_norm=0.5),
    "update_critic": single("critic"),
    "update_critic_clipped": single("critic", max_grad_norm=0.5),
    "update_actor_steps": single("actor", STEPS),
    "update_critic_steps_clipped": single("critic", STEPS, max_grad_norm=0.5),
    # contiguous phase, no clip, not monitored: both sides of each fold limit
    "phase_actor_h50": phase("h50", "actor"),
    "phase_actor_h61": phase("h61", "actor"),
    "phase_critic_p64": phase("h50", "critic"),
    "phase_critic_p16385": phase("big", "critic"),
    # contiguous phase, clipped
    "clipped_actor_h50": phase("h50", "actor", max_grad_norm=0.5),
    "clipped_actor_h50_fold_off": clip_fold_off(phase("h50", "actor", max_grad_norm=0.5)),
    "clipped_actor_h61": phase("h61", "actor", max_grad_norm=0.5),
    "clipped_critic_p64": phase("h50", "critic", max_grad_norm=0.5),
    # monitored phase
    "monitored_actor": phase("h50", "actor", target_kl=INF),
    "monitored_actor_clipped": phase("h50", "actor", target_kl=INF, max_grad_norm=0.5),
    # shuffled phase
    "shuffled_actor": phase("h50", "actor", shuffle=3),
    "shuffled_critic": phase("h50", "critic", shuffle=3),
    "shuffled_critic_p16385": phase("big", "critic", shuffle=3),
    "shuffled_actor_clipped": phase("h50", "actor", shuffle=3, max_grad_norm=0.5),
    "shuffled_actor_monitored": phase("h50", "actor", shuffle=3, target_kl=INF),
    "shuffled_actor_monitored_clipped": phase("h50", "actor", shuffle=3, target_kl=INF,
                                              max_grad_norm=0.5),
}


def listing(trace, names):
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    lds = next(c for c in rows[0] if "LDS" in c.upper() or "GROUP_SEGMENT" in c.upper())
    at = 0
    for r in rows:
        name = r["Kernel_Name"]
        if "FillFunctor<short>" in name:
            print(f"## path {names[at] if at < len(names) else at}")
            at += 1
            continue
        if not any(k in name for k in KERNELS):
            continue
        name = re.sub(r"^void ", "", name.replace("(anonymous namespace)::", "")).split("(")[0]
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        print(f"{name}  grid {grid}  workgroup {wg}  lds {r[lds]}")


def mappo(pkg, P, H, buffer_len, batch):
    import torch
    args = pkg.default_args(num_parallel=P, num_agents=3, num_obstacles=3, hidden_size=H,
                            buffer_len=buffer_len, batch_size=batch, num_epochs=1,
                            learning_rate=3e-4, num_total=buffer_len * P)
    params = pkg.set_env_params(args, "cuda")
    params["rng"], params["seed"] = "native", 17
    torch.manual_seed(0)
    m = pkg.MAPPO(pkg.set_model_params(args, "cuda"), pkg.Env(params), seed=1)
    m.get_data()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default="all", help="comma-separated path names, or all")
    ap.add_argument("--list", metavar="TRACE", help="print the launch list of a kernel trace")
    a = ap.parse_args()
    names = list(PATHS) if a.paths == "all" else a.paths.split(",")
    if a.list:
        return listing(a.list, names)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("phase_launches.py needs a HIP device")
    import marlnav_amd as pkg
    made = {s: mappo(pkg, *SETUPS[s]) for s in sorted({PATHS[n][0] for n in names})}
    sep = torch.empty(1, dtype=torch.int16, device="cuda")     # (zeros would be a fill itself)
    torch.cuda.synchronize()
    for n in names:
        setup, run = PATHS[n]
        sep.fill_(0)
        run(pkg, made[setup], SETUPS[setup][3])
    torch.cuda.synchronize()
    print(f"# ran {len(names)} paths: {','.join(names)}")


if __name__ == "__main__":
    main()
