"""Float64 restatement of the classic gym TrackEnv's observation, reward and termination (envs/myo/myodm/myodm_v0.py:189-311, 336-362;
`act` appended by base_v0.py:34-38), the checker of the HIP kernel csrc/myo_task_myodm.h.  Pinned to the reference's own code by
tests/golden/myodm_classic.npz (tools/make_myodm_classic_fixture.py)."""
import numpy as np

DEFAULT_WEIGHTS = {"pose": 0.0, "object": 1.0, "bonus": 1.0, "penalty": -2}     # myodm_v0.py:32-37
OBJ_ERR_SCALE, BASE_ERR_SCALE, LIFT_BONUS_MAG = 50.0, 40.0, 1.0                  # :127-130
QPOS_W, QPOS_ERR_SCALE, QVEL_W, QVEL_ERR_SCALE = 0.35, 5.0, 0.05, 0.1            # :133-137
OBJ_FAIL, BASE_FAIL, QPOS_FAIL = 0.25, 0.25, 0.75                                # :140-147


def mat2quat(R):
    """Unit quaternion (w >= 0) of a rotation matrix: the reference's utils/quat_math.mat2quat (largest eigenvector of its K matrix) up to
    the sign it leaves open; four branches by the largest diagonal term."""
    R = np.asarray(R, float).reshape(3, 3)
    tr = np.trace(R)
    if tr > 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = np.array([(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s])
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 - R[0, 0] + R[1, 1] - R[2, 2])
        q = np.array([(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s])
    else:
        s = 2.0 * np.sqrt(1.0 - R[0, 0] - R[1, 1] + R[2, 2])
        q = np.array([(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s])
    return -q if q[0] < 0 else q


def rotation_distance(curr, targ):
    """rotation_distance(curr, targ, euler=False) = |quatDiff2Vel(targ, curr, 1)[0]| (:181-186): diff = curr * conj(targ), speed
    2 atan2(|diff.xyz|, diff.w)."""
    a, b = np.asarray(curr, float), np.asarray(targ, float) * np.array([1.0, -1.0, -1.0, -1.0])
    d = np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                  a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])
    return abs(2.0 * np.arctan2(np.sqrt(np.sum(d[1:] ** 2)), d[0]))


def obs_reward(qpos, qvel, act, ref, obj_xipos, obj_ximat, wrist_xipos, lift_z, terminate_obj_fail=True, terminate_pose_fail=False,
               weights=None):
    """One env.  ref = dict(robot [nr], robot_vel [nr] or None, object [7]) at the post-step time; act = the muscle activations (na).
    Returns (obs vector, reward dict with pose / object / bonus / penalty / sparse / solved / done / dense, done)."""
    qpos, qvel = np.asarray(qpos, float), np.asarray(qvel, float)
    robot, robot_vel, obj = np.asarray(ref["robot"], float), ref.get("robot_vel"), np.asarray(ref["object"], float)
    nr = robot.shape[0]
    hand_qpos_err = qpos[:nr] - robot
    hand_qvel_err = np.zeros(1) if robot_vel is None or np.size(robot_vel) == 0 else qvel[:nr] - np.asarray(robot_vel, float)
    com = np.asarray(obj_xipos, float)
    obj_com_err_vec = com - obj[:3]
    obs = np.concatenate([qpos, qvel, hand_qpos_err, hand_qvel_err, obj_com_err_vec, np.asarray(act, float)])
    obj_com_err = np.sqrt(np.sum((obj[:3] - com) ** 2))
    obj_rot_err = rotation_distance(mat2quat(obj_ximat), obj[3:]) / np.pi
    obj_reward = np.exp(-OBJ_ERR_SCALE * (obj_com_err + 0.1 * obj_rot_err))
    lift_bonus = obj[2] >= lift_z and com[2] >= lift_z
    qpos_reward = np.exp(-QPOS_ERR_SCALE * np.sum(hand_qpos_err ** 2))
    qvel_reward = np.exp(-QVEL_ERR_SCALE * np.sum(hand_qvel_err ** 2))
    base = com - np.asarray(wrist_xipos, float)
    base_reward = np.exp(-BASE_ERR_SCALE * np.sqrt(np.sum(base ** 2)))
    done = False
    if terminate_obj_fail:
        done = np.sum(obj_com_err_vec ** 2) >= OBJ_FAIL ** 2 or np.sum(base ** 2) >= BASE_FAIL ** 2
    if terminate_pose_fail:
        done = done or np.sum(hand_qpos_err ** 2) >= QPOS_FAIL
    rwd = dict(pose=QPOS_W * qpos_reward + QVEL_W * qvel_reward, object=obj_reward + base_reward, bonus=LIFT_BONUS_MAG * float(lift_bonus),
               penalty=float(done), sparse=0.0, solved=0.0, done=float(done))
    w = DEFAULT_WEIGHTS if weights is None else weights
    rwd["dense"] = sum(wt * rwd[k] for k, wt in w.items())
    return obs, rwd, bool(done)
