"""The numbers of profiles/forward.md: what one forward launch (myo_forward) costs next to one 1-substep step launch (myo_step) on the
same batch, in one process.

Per env id: an env of `--envs` envs is reset and stepped `--settle` env steps with random actions (so the states carry the contacts of a
running task), then the two launches take turns, one of each per round, each between its own pair of events on the env's stream; the
first `--warmup` rounds are dropped.  The step launch advances the state, so every round measures both sides on the state of that round.
Prints one JSON line per id: median, min and max of the launch times in microseconds, their ratio, and the contacts per env at the end.
No threshold: the numbers are recorded.

    python tools/gpu_forward_rates.py [--ids myoHandPoseRandom-v0 myoLegWalk-v0 myoChallengeBaodingP1-v1] [--envs 4096] [--rounds 25]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 1), "min": round(xs[0], 1), "max": round(xs[-1], 1), "n": len(xs)}


def main():
    import torch
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", nargs="*", default=["myoHandPoseRandom-v0", "myoLegWalk-v0", "myoChallengeBaodingP1-v1"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--settle", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=25)
    a = ap.parse_args()
    for env_id in a.ids:
        env = myo.make(env_id, num_envs=a.envs, seed=0)
        env.reset()
        gen = torch.Generator("cuda").manual_seed(0)
        for _ in range(a.settle):
            env.step(torch.rand((a.envs, env.act_dim), device="cuda", generator=gen) * 2 - 1)
        b, s = env.batch, env._stream()
        b.forward(s)                      # allocates the buffers
        us = {"forward": [], "step_1_substep": []}
        sides = {"forward": lambda: b.forward(s), "step_1_substep": lambda: b.step(None, capi.ACTMAP_NONE, 1, s)}
        for r in range(a.warmup + a.rounds):
            for k, f in sides.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    us[k].append(e0.elapsed_time(e1) * 1e3)
        ncon = b.forward_read(capi.FWD_NCON)
        fm, sm = med(us["forward"]), med(us["step_1_substep"])
        print(json.dumps({"id": env_id, "envs": a.envs, "step_kernel": b.last_kernel_name(), "forward_us": fm, "step_1_substep_us": sm,
                          "forward_over_step": round(fm["median"] / sm["median"], 3), "ncon_mean": round(float(ncon.mean()), 2), "ncon_max": int(ncon.max()),
                          "forward_bytes_per_env": int(sum(b.forward_ptr(w)[2] for w in range(capi.FWD_COUNT) if not (w == capi.FWD_SITE_XMAT and not _has(b, w))) * 4)}),
              flush=True)
        del env


def _has(b, which):
    from myosuite_mjx_amd import capi
    try:
        b.forward_ptr(which)
        return True
    except capi.MyoError:
        return False


if __name__ == "__main__":
    main()
