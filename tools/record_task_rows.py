#!/usr/bin/env python3
"""Record the canonical observation row, reward, done and solved of every task bit for bit, on a GPU (tests/test_gpu_task_rows.py,
tests/golden/task_rows.npz).

    python tools/record_task_rows.py tests/golden/task_rows.npz

The ten ids of tests/test_gpu_obs_terms.py (one per task, the terrain walk besides the walk) at B = 3: reset(seed=0), then three steps of
uniform actions from a seeded CPU generator -- that file's run.  Once plain and once with rwd_dict=True, which take the two reward branches
of each observation body (the weighted sum, and the term row with its dense column).  After the reset and after the last step MYO_F_OBS,
MYO_F_REWARD, MYO_F_DONE and MYO_F_SOLVED are stored as the library holds them, in the second run the reward-term row too.  The
observation-term rows are not stored: tests/test_gpu_obs_terms.py ties them to MYO_F_OBS exactly.

The file is written from the commit BEFORE a change of the task kernels or of the row layouts and compared for equality after it: such a
change moves index arithmetic only, so every float stays.  The script runs every case twice and refuses to write a file whose second run
differs from its first."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IDS = ("myoHandPoseRandom-v0", "myoHandReachRandom-v0", "myoHandObjHoldRandom-v0", "myoHandKeyTurnRandom-v0", "myoHandPenTwirlRandom-v0",
       "myoLegStandRandom-v0", "myoLegWalk-v0", "myoLegRoughTerrainWalk-v0", "myoChallengeBaodingP1-v1", "myoChallengeDieReorientP1-v0")
B, STEPS = 3, 3
MODES = {"plain": {}, "rwd": {"rwd_dict": True}}


def rows(env_id, mode):
    """{"<when>/<what>": array} of one id in one mode; when = reset | last, what = obs | reward | done | solved (| rwd in mode "rwd")."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make(env_id, num_envs=B, **MODES[mode])
    rng = np.random.default_rng(7)                                            # tests/test_gpu_obs_terms.py _actions
    actions = [rng.uniform(-1, 1, (B, env.act_dim)).astype(np.float32) for _ in range(STEPS)]
    out = {}

    def store(when):
        for what, field in (("obs", capi.F_OBS), ("reward", capi.F_REWARD), ("done", capi.F_DONE), ("solved", capi.F_SOLVED)):
            out[f"{when}/{what}"] = env.batch.read(field)
        if mode == "rwd":
            out[f"{when}/rwd"] = env.batch.read_rwd()

    env.reset(seed=0)
    store("reset")
    for a in actions:
        env.step(a)
    store("last")
    return out


def record():
    return {f"{env_id}/{mode}/{k}": v for env_id in IDS for mode in MODES for k, v in rows(env_id, mode).items()}


if __name__ == "__main__":
    first, second = record(), record()
    assert sorted(first) == sorted(second)
    for k in first:
        assert first[k].dtype == second[k].dtype and np.array_equal(first[k], second[k], equal_nan=True), f"{k}: two runs of the same build differ"
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    np.savez_compressed(sys.argv[1], **first)
    print(f"{sys.argv[1]}: {len(first)} arrays, {sum(v.size for v in first.values())} values, {os.path.getsize(sys.argv[1])} bytes")
