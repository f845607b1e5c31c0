#!/usr/bin/env python3
"""Record what a reset draws, bit for bit, on a GPU (tests/test_gpu_reset_draws.py, tests/golden/reset_draws.npz).

    python tools/record_reset_draws.py tests/golden/reset_draws.npz

One case per piece of the reset (csrc/myo_reset.h), every case at B = 3 with set_env_offset(5) so that the counters are keyed by a global env
id that is not the local one.  Per case four stages, and after each the case's fields as the library holds them:

    reset      reset(seed=3)
    reset2     reset() again on the same seed: the episode counter has advanced, so the draws differ
    autoreset  one step of zero actions, then myo_autoreset(1, seed): reset_kernel with the done / elapsed test, every env due
    rollout    myo_bench_rollout(3 steps, max_episode_steps=1): reset_body<false> inside task_post_kernel.  Not for the walk ids, whose
               epilogue is the step kernel's own.

The terrain field is stored as the first and last 128 cells of every env and the 64-bit sum of all its words.

The file is written from the commit BEFORE a change of the reset and compared for equality after it.  The script runs every case twice
and refuses to write a file whose second run differs from its first."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, OFFSET, SEED = 3, 5, 3
OBJECT_TABLES = ("obj_size", "obj_pos", "obj_friction", "obj_mass")


def _p2(name, part):
    from myosuite_mjx_amd import envs
    return envs.P2_CONFIGS[name][part]


# case -> (env id, make kwargs, call on the made env or None, fields read, stages left out).  The kwargs and the call are functions: they
# read envs.P2_CONFIGS, which is imported with the package
CASES = {
    "pose_uniform_qpos": ("myoHandPoseRandom-v0", dict, None, ("QPOS", "TARGET"), ()),
    "stand_noise_clip": ("myoLegStandRandom-v0", dict, None, ("QPOS", "TARGET"), ()),
    "walk_keyframe_noise": ("myoLegWalk-v0", lambda: dict(reset_type="random"), None, ("QPOS", "QVEL"), ("rollout",)),
    "terrain_rough": ("myoLegRoughTerrainWalk-v0", dict, None, ("HFIELD",), ("rollout",)),
    "terrain_hilly": ("myoLegHillyTerrainWalk-v0", dict, None, ("HFIELD",), ("rollout",)),
    "terrain_stairs": ("myoLegStairTerrainWalk-v0", dict, None, ("HFIELD",), ("rollout",)),
    "fatigue_random": ("myoFatiHandPoseFixed-v0", lambda: dict(fatigue_reset_random=True), None, ("FATIGUE",), ()),
    "fatigue_vec": ("myoFatiHandPoseFixed-v0", lambda: dict(fatigue_reset_vec=np.linspace(0.1, 0.9, 39).astype(np.float32)), None, ("FATIGUE",), ()),
    "hold_geom_size": ("myoHandObjHoldRandom-v0", dict, None, ("GEOMSIZE", "TARGET"), ()),
    "elbow_body_mass": ("myoElbowPose1D6MExoFixed-v0", dict, lambda env: env.set_body_mass_range("carry_weight", 0.1, 2.0), ("BODYMASS",), ()),
    "keyturn_body_offset": ("myoHandKeyTurnRandom-v0", dict, None, ("BODYPOS", "QPOS"), ()),
    "pen_body_quat": ("myoHandPenTwirlRandom-v0", dict, None, ("BODYQUAT",), ()),
    "baoding_floored_target": ("myoChallengeBaodingP1-v1", lambda: _p2("myoChallengeBaodingP2-v1", 1), None, ("TARGET",), ()),
    "die_goal": ("myoChallengeDieReorientP1-v0", dict, None, ("TARGET", "BODYQUAT"), ()),
    "baoding_objects": ("myoChallengeBaodingP1-v1", lambda: _p2("myoChallengeBaodingP2-v1", 1),
                        lambda env: env.set_object_randomization(**_p2("myoChallengeBaodingP2-v1", 2)), OBJECT_TABLES, ()),
    "die_objects": ("myoChallengeDieReorientP1-v0", lambda: _p2("myoChallengeDieReorientP2-v0", 1),
                    lambda env: env.set_object_randomization(**_p2("myoChallengeDieReorientP2-v0", 2)), OBJECT_TABLES, ()),
    "walk_sensor_rows": ("myoLegWalk-v0", lambda: dict(sensors=True), None, ("SENSORDATA", "CFRC"), ("rollout",)),
}
STAGES = ("reset", "reset2", "autoreset", "rollout")
HF_EDGE = 128


def _read(env, what):
    from myosuite_mjx_amd import capi
    if what in OBJECT_TABLES:
        return {what: env.object_params.read(OBJECT_TABLES.index(what))}
    a = env.batch.read(getattr(capi, "F_" + what))
    if what != "HFIELD":
        return {what: a}
    a = a.reshape(B, -1)
    return {"HFIELD_first": a[:, :HF_EDGE].copy(), "HFIELD_last": a[:, -HF_EDGE:].copy(), "HFIELD_sum": a.view(np.uint32).sum(1, dtype=np.uint64)}


def draws(case):
    """{"<stage>/<field>": array} of one case."""
    import myosuite_mjx_amd as myo
    env_id, kwargs, call, fields, skipped = CASES[case]
    env = myo.make(env_id, num_envs=B, env_offset=OFFSET, autoreset=False, as_torch=False, **kwargs())
    if call is not None:
        call(env)
    out = {}

    def store(stage):
        for what in fields:
            out.update({f"{stage}/{k}": v for k, v in _read(env, what).items()})

    env.reset(seed=SEED)
    store("reset")
    env.reset()
    store("reset2")
    env.step(np.zeros((B, env.act_dim), np.float32))
    env.batch.autoreset(1, SEED)
    store("autoreset")
    if "rollout" not in skipped:
        env.batch.bench_rollout(3, env.frame_skip, seed=SEED, max_episode_steps=1)
        store("rollout")
    return out


def record():
    return {f"{case}/{k}": v for case in CASES for k, v in draws(case).items()}


if __name__ == "__main__":
    first, second = record(), record()
    assert sorted(first) == sorted(second)
    for k in first:
        assert first[k].dtype == second[k].dtype and np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)), f"{k}: two runs of the same build differ"
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    np.savez_compressed(sys.argv[1], **first)
    for case in CASES:
        ks = [k for k in first if k.startswith(case + "/")]
        print(f"{case}: {len(ks)} arrays, {sum(first[k].nbytes // 4 for k in ks)} 32-bit words")
    print(f"{sys.argv[1]}: {len(first)} arrays, {sum(v.nbytes // 4 for v in first.values())} 32-bit words, {os.path.getsize(sys.argv[1])} bytes")
