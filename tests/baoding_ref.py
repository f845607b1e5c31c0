"""Float64 restatement of BaodingEnvV1 (envs/myo/myochallenge/baoding_v1.py): the goal trajectory (create_goal_trajectory, :384-405), the
targets' site_pos after env step k (step, :147-181), and the observation, reward, done and solved (get_obs_dict / get_reward_dict,
:183-266), batched over envs.  Shared by tests/test_baoding_host.py (oracle states) and tests/test_gpu_baoding.py (HIP states)."""
import numpy as np

WEIGHTS = dict(pos_dist_1=5.0, pos_dist_2=5.0)
CENTER = (-0.0125, -0.07)
DT = 0.025               # frame_skip 10 x timestep 0.0025


def goal_trajectory(sign, time_step, time_period, n=1000):
    """create_goal_trajectory: [n, 2] angles before the start-angle shift (sign 0 hold, -1 CW, +1 CCW)."""
    t = np.arange(n, dtype=np.float64)
    a = sign * 2 * np.pi * (t * time_step / time_period)
    return np.stack([a, a], axis=1)


def target_xy(params, k, dt=DT):
    """site_pos[:2] of target1 and target2 after env step k (1-based; k = 0: the first observation of an episode, which shows goal[0]).
    params [B, 5] = start angle, sign, x radius, y radius, period.  Returns [B, 2, 2]."""
    p = np.atleast_2d(np.asarray(params, np.float64))
    j = np.maximum(np.asarray(k) - 1, 0)
    base = p[:, 1] * 2 * np.pi * (j * dt / p[:, 4])
    out = np.empty((len(p), 2, 2))
    for t, shift in ((0, 0.0), (1, -np.pi)):
        ang = base + p[:, 0] + shift
        out[:, t, 0] = p[:, 2] * np.cos(ang) + CENTER[0]
        out[:, t, 1] = p[:, 3] * np.sin(ang) + CENTER[1]
    return out


def baoding_restate(qpos, qvel, sites, dt=DT, drop_th=1.25, proximity_th=0.015, w=WEIGHTS):
    """qpos [B, nq], qvel [B, nv]; sites [B, 12] = ball1 | ball2 | target1 | target2 world positions.  Returns obs [B, nq - 14 + 24], dense
    reward, done, solved (float64 / bool)."""
    qpos, qvel, sites = (np.atleast_2d(np.asarray(a, np.float64)) for a in (qpos, qvel, sites))
    b1, b2, t1, t2 = (sites[:, 3 * k:3 * k + 3] for k in range(4))
    obs = np.concatenate([qpos[:, :-14], b1, qvel[:, -12:-9] * dt, b2, qvel[:, -6:-3] * dt, t1, t2, t1 - b1, t2 - b2], axis=1)
    d1, d2 = np.linalg.norm(t1 - b1, axis=1), np.linalg.norm(t2 - b2, axis=1)
    fall = (b1[:, 2] < drop_th) | (b2[:, 2] < drop_th)
    dense = w["pos_dist_1"] * -d1 + w["pos_dist_2"] * -d2
    return obs, dense, fall, (d1 < proximity_th) & (d2 < proximity_th) & ~fall
