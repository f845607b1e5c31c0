"""PPO training of a policy for one env id on one MI355X: the native counterpart of the reference's `mjx/ppo_continuous_action.py`
(brax `ppo.train` on a `TrackEnv`).  The defaults are that script's hyperparameters (reward_scaling 5, action_repeat 4, unroll_length 50,
32 minibatches, 8 updates per batch, discounting 0.95, learning rate 3e-4, entropy cost 1e-3, seed 1, 2 000 000 steps, 128 envs); its
batch_size, num_evals and max_devices_per_host have no counterpart (`myosuite_mjx_amd.ppo.train` says why), and episodes end by the env
id's own registered time limit rather than by its episode_length.  One progress line per iteration, like the script's callback.

    python tools/train_ppo.py --env myoHandPoseRandom-v0 --num-envs 4096 --num-timesteps 20000000 --out policy.npz
The .npz is what `myosuite_mjx_amd.BraxPolicy.from_npz` loads (the value network rides along under vw* / vb*)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--env", required=True, help="a registered env id; MyoDM ids are made with autoreset=True")
    ap.add_argument("--num-envs", type=int, default=128)
    ap.add_argument("--num-timesteps", type=int, default=2_000_000)
    ap.add_argument("--out", default=None, help="write the trained parameters here (.npz)")
    ap.add_argument("--unroll-length", type=int, default=50)
    ap.add_argument("--num-minibatches", type=int, default=32)
    ap.add_argument("--num-updates-per-batch", type=int, default=8)
    ap.add_argument("--action-repeat", type=int, default=4)
    ap.add_argument("--discounting", type=float, default=0.95)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--learning-rate", type=float, default=3e-4)
    ap.add_argument("--entropy-cost", type=float, default=1e-3)
    ap.add_argument("--clipping-epsilon", type=float, default=0.3)
    ap.add_argument("--reward-scaling", type=float, default=5.0)
    ap.add_argument("--no-normalize-observations", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--update", choices=["torch", "hip"], default="torch",
                    help="the SGD step: torch autograd and Adam (default), or the device learner's HIP kernels")
    a = ap.parse_args()
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import ppo
    from myosuite_mjx_amd.envs import REGISTRY
    kw = dict(autoreset=True) if REGISTRY.get(a.env, {}).get("task") == "track" else {}
    env = myo.make(a.env, num_envs=a.num_envs, seed=a.seed, **kw)
    times = [time.perf_counter()]

    def progress(num_steps, metrics):
        times.append(time.perf_counter())
        print(json.dumps({"num_steps": num_steps, "time_spent": round(times[-1] - times[-2], 3),
                          **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in metrics.items()}}), flush=True)

    _, params, _ = ppo.train(env, a.num_timesteps, unroll_length=a.unroll_length, num_minibatches=a.num_minibatches,
                             num_updates_per_batch=a.num_updates_per_batch, discounting=a.discounting, gae_lambda=a.gae_lambda,
                             learning_rate=a.learning_rate, entropy_cost=a.entropy_cost, clipping_epsilon=a.clipping_epsilon,
                             reward_scaling=a.reward_scaling, normalize_observations=not a.no_normalize_observations,
                             action_repeat=a.action_repeat, seed=a.seed, progress_fn=progress, update=a.update)
    print(f"time to train: {times[-1] - times[0]:.1f} s")
    if a.out:
        ppo.save(a.out, params)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
