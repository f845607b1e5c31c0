"""What the reward-term row and the episode statistics cost per env.step: env-steps/s at 4096 envs, plain vs rwd_dict=True vs
rwd_dict=True, episode_stats=True, for the flagship id, the walk task (term kernel after the step kernel) and a TrackEnv-class hand task.

Timing: actions live on the device, a warm-up of `--warmup` steps, then windows of at least `--window` seconds each bracketed by a device
synchronisation; the three configurations of an id take turns window by window, so clock drift hits them alike.  Prints one JSON line
per id and configuration (median and spread over the windows).  No threshold: the numbers are reported (profiles/reward_terms.md).

    python tools/gpu_reward_terms_rate.py [--envs 4096] [--windows 3] [--window 1.0]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IDS = ("myoHandPoseRandom-v0", "myoLegWalk-v0", "myoHandPenTwirlRandom-v0")
CONFIGS = (("plain", {}), ("rwd_dict", dict(rwd_dict=True)), ("rwd_dict+episode_stats", dict(rwd_dict=True, episode_stats=True)))


def main():
    import torch
    import myosuite_mjx_amd as myo
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--ids", nargs="*", default=IDS)
    a = ap.parse_args()
    for env_id in a.ids:
        envs, acts = [], None
        for name, kw in CONFIGS:
            env = myo.make(env_id, num_envs=a.envs, seed=0, **kw)
            env.reset()
            if acts is None:
                acts = torch.rand((64, a.envs, env.act_dim), device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1
            for i in range(a.warmup):
                env.step(acts[i % 64])
            envs.append((name, env))
        torch.cuda.synchronize()
        rates = {name: [] for name, _ in envs}
        for _ in range(a.windows):
            for name, env in envs:
                n, t0 = 0, time.perf_counter()
                while True:
                    for i in range(20):
                        env.step(acts[(n + i) % 64])
                    n += 20
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if dt >= a.window:
                        break
                rates[name].append(n * a.envs / dt)
        for name, r in rates.items():
            r = sorted(r)
            print(json.dumps({"id": env_id, "config": name, "envs": a.envs, "env_steps_per_s": r[len(r) // 2], "min": r[0], "max": r[-1],
                              "windows": len(r), "window_s": a.window}), flush=True)


if __name__ == "__main__":
    main()
