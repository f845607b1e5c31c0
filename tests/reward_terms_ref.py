"""Float64 restatement of the reward-term rows of the batched envs (`info["rwd_dict"]`): get_reward_dict of the reference's env classes
(pose_v0.py:118-135, reach_v0.py:126-141, obj_hold_v0.py:102-117, key_turn_v0.py:134-152, pen_v0.py:150-167, walk_v0.py:117-133 and
:298-311, baoding_v1.py:239-262, reorient_v0.py:148-176), batched over envs, from state, task-site positions and thresholds.

`terms(task, **inputs)` returns ({column: float64[B]} for every column but dense, margin[B]): margin is the distance of the nearest
deciding quantity from its threshold, the quantity the step-valued columns (bonus / penalty / drop, solved, done) flip at.  A float32
kernel may legitimately disagree on those columns where margin is below its own error; the continuous columns carry no such caveat.
`dense(row, weights)` is env_base's sum over rwd_keys_wt.items().  Shared by tests/test_reward_terms_host.py (oracle states, against the
tasks' own *_restate functions) and tests/test_gpu_reward_terms.py (HIP states)."""
import numpy as np

from reorient_ref import mat2euler, site_frames

STEP_COLUMNS = ("bonus", "penalty", "drop", "solved", "done")


def _f64(*a):
    return tuple(np.atleast_2d(np.asarray(x, np.float64)) for x in a)


def _act_mag(act, na=None):
    act, = _f64(act)
    return np.linalg.norm(act, axis=1) / (na or act.shape[1])


def _margin(*pairs):
    """min over (quantity, threshold) pairs of |quantity - threshold|; infinite thresholds decide nothing."""
    m = np.full(np.shape(pairs[0][0]), np.inf)
    for q, th in pairs:
        th = np.broadcast_to(np.asarray(th, np.float64), np.shape(q))
        m = np.minimum(m, np.where(np.isfinite(th), np.abs(q - th), np.inf))
    return m


def pose(qpos, target, act, pose_thd, na=None):
    qpos, target = _f64(qpos, target)
    d = np.linalg.norm(target - qpos, axis=1)
    far_th = 4 * np.pi / 2
    row = dict(pose=-d, bonus=1.0 * (d < pose_thd) + 1.0 * (d < 1.5 * pose_thd), penalty=-1.0 * (d > far_th), act_reg=-_act_mag(act, na),
               sparse=-d, solved=1.0 * (d < pose_thd), done=1.0 * (d > far_th))
    return row, _margin((d, pose_thd), (d, 1.5 * pose_thd), (d, far_th))


def reach(tips, target, act, time, dt, far_th, near_th, na=None):
    """tips, target [B, 3 n]; far_th / near_th already scaled by the number of tips; far_th counts only after two env steps (reach_v0.py:121-124)."""
    tips, target = _f64(tips, target)
    d = np.linalg.norm(target - tips, axis=1)
    far = np.where(np.asarray(time, np.float64).reshape(-1) > 2 * dt, far_th, np.inf)
    row = dict(reach=-d, bonus=1.0 * (d < 2 * near_th) + 1.0 * (d < near_th), act_reg=-_act_mag(act, na), penalty=-1.0 * (d > far),
               sparse=-d, solved=1.0 * (d < near_th), done=1.0 * (d > far))
    return row, _margin((d, 2 * near_th), (d, near_th), (d, far))


def hold(obj_pos, goal, act, goal_th, drop_th, na=None):
    obj_pos, goal = _f64(obj_pos, goal)
    d = np.linalg.norm(goal - obj_pos, axis=1)
    drop = d > drop_th
    row = dict(goal_dist=-d, bonus=1.0 * (d < 2 * goal_th) + 1.0 * (d < goal_th), act_reg=-_act_mag(act, na), penalty=-1.0 * drop,
               sparse=-d, solved=1.0 * (d < goal_th), done=1.0 * drop)
    return row, _margin((d, 2 * goal_th), (d, goal_th), (d, drop_th))


def stand(tip, target, qvel, act, time, dt, far_th, near_th, na=None):
    """walk_v0.py:100-133 (ReachEnvV0 on the legs): vel_dist = |qvel dt|, act_reg = -100 act_mag."""
    tip, target, qvel = _f64(tip, target, qvel)
    d = np.linalg.norm(target - tip, axis=1)
    vel = np.linalg.norm(qvel * dt, axis=1)
    far = np.where(np.asarray(time, np.float64).reshape(-1) > 2 * dt, far_th, np.inf)
    row = dict(reach=10.0 - d - 10.0 * vel, bonus=1.0 * (d < 2 * near_th) + 1.0 * (d < near_th), act_reg=-100.0 * _act_mag(act, na),
               penalty=-1.0 * (d > far), sparse=-d, solved=1.0 * (d < near_th), done=1.0 * (d > far))
    return row, _margin((d, 2 * near_th), (d, near_th), (d, far))


def walk(com_vel, height, feet_heights, phase, qpos, act, qadr_hip_flexion, qadr_joint_angle, target_rot, min_height=0.8, max_rot=0.8,
         target_x_vel=0.0, target_y_vel=1.2, knee_height=0.0, na=None):
    """walk_v0.py:283-311, 395-470 (+ TerrainEnvV0's knee condition, :660-671) from the quantities of the observation: COM velocity (2),
    COM height, feet heights (2), phase; qpos [B, nq] with the root quaternion at 3:7."""
    com_vel, feet, qpos = _f64(com_vel, feet_heights, qpos)
    height, phase = (np.asarray(a, np.float64).reshape(-1) for a in (height, phase))
    vel = np.exp(-np.square(target_y_vel - com_vel[:, 1])) + np.exp(-np.square(target_x_vel - com_vel[:, 0]))
    des = np.stack([0.8 * np.cos(phase * 2 * np.pi + np.pi), 0.8 * np.cos(phase * 2 * np.pi)], axis=1)
    cyclic = np.linalg.norm(des - qpos[:, list(qadr_hip_flexion)], axis=1)
    quat = qpos[:, 3:7]
    ref_rot = np.exp(-5.0 * np.linalg.norm(quat - np.asarray(target_rot, np.float64), axis=1))
    ja = np.exp(-5.0 * np.mean(np.abs(qpos[:, list(qadr_joint_angle)]), axis=1))
    r00 = 1.0 - 2.0 * (quat[:, 2] ** 2 + quat[:, 3] ** 2) / np.sum(quat ** 2, axis=1)           # quat2mat(quat)[0, 0]
    done = (height < min_height) | (np.abs(r00) > max_rot)
    pairs = [(height, min_height), (np.abs(r00), max_rot), (vel, 1.0)]
    if knee_height > 0:
        knee = height - feet.mean(axis=1)
        done = done | (knee < knee_height)
        pairs.append((knee, knee_height))
    row = dict(vel_reward=vel, cyclic_hip=cyclic, ref_rot=ref_rot, joint_angle_rew=ja, act_mag=_act_mag(act, na),
               sparse=vel, solved=1.0 * (vel >= 1.0), done=1.0 * done)
    return row, _margin(*pairs)


def keyturn(qpos, sites, act, goal_th, na=None):
    """sites [B, 9] = key head | IFtip | THtip."""
    qpos, sites = _f64(qpos, sites)
    d_if = np.abs(np.linalg.norm(sites[:, 0:3] - sites[:, 3:6], axis=1) - 0.030)
    d_th = np.abs(np.linalg.norm(sites[:, 0:3] - sites[:, 6:9], axis=1) - 0.030)
    key_q, far_th = qpos[:, -1], 0.1
    row = dict(key_turn=key_q, IFtip_approach=-d_if, THtip_approach=-d_th, act_reg=-_act_mag(act, na),
               bonus=1.0 * (key_q > np.pi / 2) + 1.0 * (key_q > np.pi), penalty=-1.0 * (d_if > far_th / 2) - 1.0 * (d_th > far_th / 2),
               sparse=key_q, solved=1.0 * (key_q > goal_th), done=1.0 * ((d_if > far_th) | (d_th > far_th)))
    return row, _margin((key_q, np.pi / 2), (key_q, np.pi), (key_q, goal_th), (d_if, far_th / 2), (d_th, far_th / 2), (d_if, far_th), (d_th, far_th))


def pen(sites, obj_pos, act, length=0.13, na=None):
    """sites [B, 15] = object top | object bottom | target top | target bottom | eps_ball; obj_pos [B, 3] (body xpos of Object)."""
    sites, obj_pos = _f64(sites, obj_pos)
    ot, ob, tt, tb, eps = (sites[:, 3 * k:3 * k + 3] for k in range(5))
    rot, drot = (ot - ob) / length, (tt - tb) / length
    pos_align = np.linalg.norm(obj_pos - eps, axis=1)
    npr = np.linalg.norm(rot, axis=1) * np.linalg.norm(drot, axis=1)
    rot_align = np.einsum("ij,ij->i", rot, drot) / np.where(npr == 0, 1.0, npr)
    dropped = pos_align > 0.075
    row = dict(pos_align=-pos_align, rot_align=rot_align, act_reg=-_act_mag(act, na), drop=-1.0 * dropped,
               bonus=1.0 * (rot_align > 0.9) * (pos_align < 0.075) + 5.0 * (rot_align > 0.95) * (pos_align < 0.075),
               sparse=-pos_align + rot_align, solved=1.0 * ((rot_align > 0.95) & ~dropped), done=1.0 * dropped)
    return row, _margin((pos_align, 0.075), (rot_align, 0.9), (rot_align, 0.95))


def baoding(sites, act, drop_th=1.25, proximity_th=0.015, na=None):
    """sites [B, 12] = ball1 | ball2 | target1 | target2."""
    sites, = _f64(sites)
    b1, b2, t1, t2 = (sites[:, 3 * k:3 * k + 3] for k in range(4))
    d1, d2 = np.linalg.norm(t1 - b1, axis=1), np.linalg.norm(t2 - b2, axis=1)
    fall = (b1[:, 2] < drop_th) | (b2[:, 2] < drop_th)
    row = dict(pos_dist_1=-d1, pos_dist_2=-d2, act_reg=-_act_mag(act, na), sparse=-(d1 + d2),
               solved=1.0 * ((d1 < proximity_th) & (d2 < proximity_th) & ~fall), done=1.0 * fall)
    return row, _margin((b1[:, 2], drop_th), (b2[:, 2], drop_th), (d1, proximity_th), (d2, proximity_th))


def die(sites, act, goal_obj_offset=(-0.1, 0.0, 0.0), pos_th=0.025, rot_th=0.262, drop_th=0.2, na=None):
    """sites [B, 24] = object_o / x / y / z, target_o / x / y / z (reorient_ref.SITES)."""
    x = np.asarray(sites, np.float64).reshape(-1, 8, 3)
    Ro, Rt = site_frames(x)
    pos_err = x[:, 4] - x[:, 0] - np.asarray(goal_obj_offset, np.float64)
    rot_err = mat2euler(Rt) - mat2euler(Ro)
    pd, rd = np.linalg.norm(pos_err, axis=1), np.linalg.norm(rot_err, axis=1)
    drop = pd > drop_th
    row = dict(pos_dist=-pd, rot_dist=-rd, bonus=1.0 * (pd < 2 * pos_th) + 1.0 * (pd < pos_th), act_reg=-_act_mag(act, na), penalty=-1.0 * drop,
               sparse=-rd - 10.0 * pd, solved=1.0 * ((pd < pos_th) & (rd < rot_th) & ~drop), done=1.0 * drop)
    return row, _margin((pd, 2 * pos_th), (pd, pos_th), (pd, drop_th), (rd, rot_th))


_TASKS = dict(pose=pose, reach=reach, hold=hold, stand=stand, walk=walk, keyturn=keyturn, pen=pen, baoding=baoding, die=die)


def terms(task, **inputs):
    return _TASKS[task](**inputs)


def dense(row, weights):
    """env_base's dense: the sum over the weighted keys of weight * term (float64)."""
    return sum(float(w) * np.asarray(row[k], np.float64) for k, w in weights.items())
