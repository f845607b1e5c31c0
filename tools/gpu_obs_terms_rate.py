"""What the observation-term rows cost per env.step: env-steps/s at 4096 envs, plain vs obs_dict=True vs a selection with proprioception
(obs_keys = the default keys reversed, proprio_keys = the first two of them), for the flagship id and the walk task (whose rows follow the
step launch), and the time of one launch of the terms kernel.

Timing of the rates: actions live on the device, a warm-up of `--warmup` steps, then windows of at least `--window` seconds each bracketed
by a device synchronisation; the configurations of an id take turns window by window, so clock drift hits them alike.  The kernel's time:
`--launches` observation-only passes (myo_obs_only) between two device events, on the plain env and on the obs_dict one, turn about; the
pass of the second is the pass of the first plus one launch of obs_terms_kernel, so the difference of the medians per launch is that
kernel's time, launch gap included.  Prints one JSON line per id and configuration.  No threshold: the numbers are reported
(profiles/obs_terms.md).

    python tools/gpu_obs_terms_rate.py [--envs 4096] [--windows 3] [--window 1.0] [--launches 300]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IDS = ("myoHandPoseRandom-v0", "myoLegWalk-v0")


def main():
    import torch
    import myosuite_mjx_amd as myo
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--ids", nargs="*", default=IDS)
    a = ap.parse_args()
    for env_id in a.ids:
        envs, acts = [], None
        keys = myo.make(env_id, num_envs=1).obs_keys
        configs = (("plain", {}), ("obs_dict", dict(obs_dict=True)),
                   ("obs_keys+proprio_keys", dict(obs_keys=list(reversed(keys)), proprio_keys=list(keys[:2]))))
        for name, kw in configs:
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
        for name, env in envs:
            r = sorted(rates[name])
            row = env.view(myo.capi.OBS_TERMS, "obs").shape[1] + env.obs_dim + sum(env._obs_width[k] for k in env.proprio_keys or []) if name != "plain" else 0
            print(json.dumps({"id": env_id, "config": name, "envs": a.envs, "env_steps_per_s": r[len(r) // 2], "min": r[0], "max": r[-1],
                              "windows": len(r), "window_s": a.window, "floats_written_per_env": row}), flush=True)
        # one launch of the terms kernel: observation-only passes without and with it, between device events
        per = {name: [] for name, _ in envs[:2]}
        for _ in range(5):
            for name, env in envs[:2]:
                s = env._stream()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    env.batch.obs_only(s)
                e1.record()
                e1.synchronize()
                per[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
        print(json.dumps({"id": env_id, "config": "obs_only pass", "envs": a.envs, "us_per_pass_plain": med["plain"], "us_per_pass_obs_dict": med["obs_dict"],
                          "us_per_terms_launch": med["obs_dict"] - med["plain"], "repeats": {k: [round(x, 2) for x in v] for k, v in per.items()},
                          "launches": a.launches}), flush=True)


if __name__ == "__main__":
    main()
