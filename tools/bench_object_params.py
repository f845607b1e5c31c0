"""Rate of the two P2 configurations with the per-env object parameters on, next to the same rollout with them off (bench.py cannot switch
the subsystem on): myo_bench_rollout (fresh random actions, observation, auto-reset with the re-draws) on the P1 id, off = the plain
TrackEnv-class kernel, on = step_kernel_obj with envs.P2_CONFIGS' draw table.  One process, alternating rounds, one JSON line.

    python tools/bench_object_params.py [--batch 4096] [--steps 100] [--warmup 20] [--rounds 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi, envs
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    mode = capi.BENCH_OBS | capi.BENCH_FRESH_ACTIONS | capi.BENCH_AUTORESET
    out = {}
    for name, (p1, make_kw, rand_kw) in envs.P2_CONFIGS.items():
        arms = {}
        for arm in ("off", "on"):
            env = myo.make(p1, num_envs=a.batch, seed=1, as_torch=False, **make_kw)
            if arm == "on":
                env.set_object_randomization(**rand_kw)
            env.reset()
            env.batch.bench_rollout(a.warmup, env.frame_skip, seed=1, mode=mode, max_episode_steps=env.max_episode_steps)
            arms[arm] = env
        rates = {"off": [], "on": []}
        for _ in range(a.rounds):                    # alternating rounds: both arms see the same clocks
            for arm, env in arms.items():
                ms = env.batch.bench_rollout(a.steps, env.frame_skip, seed=2, mode=mode, max_episode_steps=env.max_episode_steps)
                rates[arm].append(a.batch * a.steps / (ms * 1e-3))
        out[name] = {"p1_id": p1, "kernel_off": arms["off"].batch.last_kernel_name(), "kernel_on": arms["on"].batch.last_kernel_name(),
                     "env_steps_per_s_off": [round(r) for r in rates["off"]], "env_steps_per_s_on": [round(r) for r in rates["on"]],
                     "flags_off": sorted(set(int(f) for f in arms["off"].status())), "flags_on": sorted(set(int(f) for f in arms["on"].status()))}
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "configs": out}))


if __name__ == "__main__":
    main()
