"""The numbers of profiles/ppo_training.md: what PPO training costs next to pure stepping, and myo_ppo_gae next to the torch loop.

Part 1, per env id: `ppo.train` runs `--iterations` iterations (hyperparameters of tools/train_ppo.py, action_repeat 1) with the torch update,
then with the HIP update (`update="hip"`), and the two take turns like that for `--rounds` rounds in one process; after every iteration
the progress callback steps a second instance of the same id with device-resident random actions for `--steps` env steps between two
device synchronisations, so the two update modes and pure stepping alternate and clock drift hits all alike.  The first iteration of
every run (allocator and kernel warm-up) is reported but kept out of the medians.  One JSON line per id and update mode.
Part 2: one myo_ppo_gae call against the torch loop (`ppo._gae_torch`) on the same CUDA tensors at T = 50, B = 128 and 4096, `--reps`
calls per window between synchronisations, the two sides taking turns for `--windows` windows.
Prints one JSON line per measurement (median, min, max).  No threshold: the numbers are recorded.

    python tools/gpu_ppo_rates.py [--ids myoHandPoseRandom-v0:4096 MyoHandAirplaneRandom-v0:1024] [--iterations 4]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def main():
    import torch
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import ppo
    from myosuite_mjx_amd.envs import REGISTRY
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", nargs="*", default=["myoHandPoseRandom-v0:4096", "MyoHandAirplaneRandom-v0:1024"])
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--updates", nargs="*", default=["torch", "hip"], choices=["torch", "hip"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    for spec in a.ids:
        env_id, n = spec.split(":")
        n = int(n)
        kw = dict(autoreset=True) if REGISTRY[env_id].get("task") == "track" else {}
        env, other = myo.make(env_id, num_envs=n, seed=0, **kw), myo.make(env_id, num_envs=n, seed=1, **kw)
        other.reset()
        acts = torch.rand((64, n, other.act_dim), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1
        for i in range(30):
            other.step(acts[i % 64])
        train, first, step = {u: [] for u in a.updates}, {u: [] for u in a.updates}, []
        for _ in range(a.rounds):
            for update in a.updates:
                run = []

                def progress(num_steps, m):
                    run.append(m)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(a.steps):
                        other.step(acts[i % 64])
                    torch.cuda.synchronize()
                    if len(run) > 1:
                        step.append(a.steps * n / (time.perf_counter() - t0))

                ppo.train(env, a.iterations * n * 50, progress_fn=progress, seed=1, update=update)
                first[update].append(run[0])
                train[update] += run[1:] or run
        for update in a.updates:
            rest = train[update]
            print(json.dumps({"id": env_id, "envs": n, "update": update, "unroll_length": 50, "sgd_steps_per_iteration": 256,
                              "train_env_steps_per_s": med([m["steps_per_s"] for m in rest]),
                              "rollout_env_steps_per_s": med([n * 50 / m["rollout_s"] for m in rest]),
                              "pure_stepping_env_steps_per_s": med(step) if step else None,
                              "rollout_share": med([m["rollout_s"] / (m["rollout_s"] + m["update_s"]) for m in rest]),
                              "rollout_s": med([m["rollout_s"] for m in rest]), "update_s": med([m["update_s"] for m in rest]),
                              "update_ms_per_sgd_step": med([m["update_s"] / 256 * 1e3 for m in rest]),
                              "first_iterations": [{"rollout_s": m["rollout_s"], "update_s": m["update_s"]} for m in first[update]]}), flush=True)
        del env, other
    for T, B in ((50, 128), (50, 4096)):
        g = torch.Generator("cuda").manual_seed(T + B)
        r, v = torch.randn((T, B), device="cuda", generator=g), torch.randn((T, B), device="cuda", generator=g)
        boot = torch.randn(B, device="cuda", generator=g)
        term = (torch.rand((T, B), device="cuda", generator=g) < 0.05).float()
        trunc = (torch.rand((T, B), device="cuda", generator=g) < 0.05).float() * (1 - term)
        sides = {"myo_ppo_gae": lambda: ppo.compute_gae(r, v, boot, term, trunc, 0.95, 0.95),
                 "torch_loop": lambda: ppo._gae_torch(r, v, boot, term, trunc, 0.95, 0.95)}
        us = {k: [] for k in sides}
        for f in sides.values():
            f()
        for _ in range(a.windows):
            for k, f in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    f()
                torch.cuda.synchronize()
                us[k].append((time.perf_counter() - t0) / a.reps * 1e6)
        print(json.dumps({"gae": [T, B], "reps_per_window": a.reps, **{k + "_us_per_call": med(x) for k, x in us.items()}}), flush=True)


if __name__ == "__main__":
    main()
