"""Reward terms of the batched envs: column names per task, the weight vector of `weighted_reward_keys`, and the validation of the four
constructor parameters (`rwd_dict`, `weighted_reward_keys`, `rwd_mode`, `episode_stats`) -- host arithmetic only, done before a model is
loaded or a GPU is touched.

The columns are the keys of the reference's `rwd_dict` for the task's env class, in its order (get_reward_dict of pose_v0.py:118-135,
reach_v0.py:126-141, obj_hold_v0.py:102-117, key_turn_v0.py:134-152, pen_v0.py:150-167, walk_v0.py:117-133 and :298-311,
baoding_v1.py:239-262, reorient_v0.py:148-176), `dense` last; the library carries the same table (csrc/myo_rewards.h) and
tests/golden/reward_terms.json pins both to the reference's text."""
from __future__ import annotations

import numpy as np

TAIL = ("sparse", "solved", "done", "dense")
TERMS = {
    "pose": ("pose", "bonus", "penalty", "act_reg"),
    "reach": ("reach", "bonus", "act_reg", "penalty"),
    "hold": ("goal_dist", "bonus", "act_reg", "penalty"),
    "keyturn": ("key_turn", "IFtip_approach", "THtip_approach", "act_reg", "bonus", "penalty"),
    "pen": ("pos_align", "rot_align", "act_reg", "drop", "bonus"),
    "stand": ("reach", "bonus", "act_reg", "penalty"),
    "walk": ("vel_reward", "cyclic_hip", "ref_rot", "joint_angle_rew", "act_mag"),
    "baoding": ("pos_dist_1", "pos_dist_2", "act_reg"),
    "die": ("pos_dist", "rot_dist", "bonus", "act_reg", "penalty"),
}
RWD_KEYS = {task: terms + TAIL for task, terms in TERMS.items()}
RWD_MODES = ("dense", "sparse")


def weight_vector(env_id, task, weights):
    """float32 vector with one entry per column of the task's row except `dense`: the weight of every key of `weights`, 0 for the keys it
    leaves out (env_base sums over rwd_keys_wt.items() only).  Any column but `dense` may be weighted; another key raises KeyError."""
    cols = RWD_KEYS[task][:-1]
    w = np.zeros(len(cols), np.float32)
    for k, v in dict(weights).items():
        if k not in cols:
            raise KeyError(f"{env_id}: weighted_reward_keys names {k!r}, which is no column of the {task} task's rwd_dict {cols}")
        w[cols.index(k)] = float(v)
    return w


def resolve(env_id, spec, rwd_dict=False, weighted_reward_keys=None, rwd_mode="dense", episode_stats=False):
    """What BatchedMyoEnv does with its four reward parameters: None when all are at their defaults (nothing is allocated, no launch is
    added), else (keys, weight vector, rwd_mode).  weighted_reward_keys=None: the task's registered weights."""
    if rwd_mode not in RWD_MODES:
        raise ValueError(f"{env_id}: rwd_mode must be one of {RWD_MODES}, got {rwd_mode!r}")
    if not (rwd_dict or weighted_reward_keys is not None or rwd_mode != "dense" or episode_stats):
        return None
    task = spec["task"]
    w = weight_vector(env_id, task, spec["weights"] if weighted_reward_keys is None else weighted_reward_keys)
    return RWD_KEYS[task], w, rwd_mode
