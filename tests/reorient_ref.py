"""Float64 restatement of ReorientEnvV0's observation, reward, done and solved (envs/myo/myochallenge/reorient_v0.py:111-176), batched
over envs, from the state, the world positions of object_o / target_o and the two site rotation matrices, and the reference's mat2euler
(utils/quat_math.py:96-115).  euler2quat is tests/pen_ref.py's.  Shared by tests/test_die_host.py (oracle states) and
tests/test_gpu_die.py (HIP states)."""
import numpy as np

from pen_ref import euler2quat  # noqa: F401  (re-exported: the target's orientation draw)

WEIGHTS = dict(pos_dist=100.0, rot_dist=1.0, bonus=0.0, act_reg=0.0, penalty=0.0)
EPS4 = 4.0 * np.finfo(np.float64).eps
SITES = ("object_o", "object_x", "object_y", "object_z", "target_o", "target_x", "target_y", "target_z")


def mat2euler(mat):
    mat = np.asarray(mat, np.float64)
    cy = np.sqrt(mat[..., 2, 2] ** 2 + mat[..., 1, 2] ** 2)
    ok = cy > EPS4
    e = np.empty(mat.shape[:-1])
    e[..., 2] = np.where(ok, -np.arctan2(mat[..., 0, 1], mat[..., 0, 0]), -np.arctan2(-mat[..., 1, 0], mat[..., 1, 1]))
    e[..., 1] = -np.arctan2(-mat[..., 0, 2], cy)
    e[..., 0] = np.where(ok, -np.arctan2(mat[..., 1, 2], mat[..., 2, 2]), 0.0)
    return e


def euler_margin(mat):
    """How far a rotation matrix is from where mat2euler is ill-conditioned: (cy, distance in rad of the two atan2 arguments from the
    +-pi cut).  States with cy < 1e-3 or within 1e-3 rad of the cut are left out of float32 comparisons."""
    mat = np.asarray(mat, np.float64)
    cy = np.sqrt(mat[..., 2, 2] ** 2 + mat[..., 1, 2] ** 2)
    a2 = np.abs(np.arctan2(mat[..., 0, 1], mat[..., 0, 0]))
    a0 = np.abs(np.arctan2(mat[..., 1, 2], mat[..., 2, 2]))
    return cy, np.pi - np.maximum(a2, a0)       # (the middle angle is an atan2 with a non-negative second argument: never at the cut)


def site_frames(x, side=(0.028, 0.03)):
    """Rotation matrices of the object_o and target_o sites from the world positions x [B, 8, 3] of SITES: column k = (x_k - x_o) / side."""
    x = np.asarray(x, np.float64)
    Ro = np.stack([(x[:, 1 + k] - x[:, 0]) / side[0] for k in range(3)], axis=-1)
    Rt = np.stack([(x[:, 5 + k] - x[:, 4]) / side[1] for k in range(3)], axis=-1)
    return Ro, Rt


def reorient_restate(qpos, qvel, act, obj_pos, goal_pos, obj_mat, goal_mat, dt, goal_obj_offset=(-0.1, 0.0, 0.0), pos_th=0.025, rot_th=0.262,
                     drop_th=0.2, w=WEIGHTS):
    """qpos, qvel [B, nq]; act [B, na]; obj_pos, goal_pos [B, 3] (site_xpos of object_o / target_o); obj_mat, goal_mat [B, 3, 3] (their
    site_xmat).  Returns obs [B, 2 nq - 13 + 18], dense reward, done, solved (float64 / bool)."""
    qpos, qvel, act, obj_pos, goal_pos = (np.atleast_2d(np.asarray(a, np.float64)) for a in (qpos, qvel, act, obj_pos, goal_pos))
    obj_mat, goal_mat = (np.asarray(a, np.float64).reshape(-1, 3, 3) for a in (obj_mat, goal_mat))
    pos_err = goal_pos - obj_pos - np.asarray(goal_obj_offset, np.float64)
    obj_rot, goal_rot = mat2euler(obj_mat), mat2euler(goal_mat)
    rot_err = goal_rot - obj_rot
    obs = np.concatenate([qpos[:, :-7], qvel[:, :-6] * dt, obj_pos, goal_pos, pos_err, obj_rot, goal_rot, rot_err], axis=1)
    pos_dist, rot_dist = np.linalg.norm(pos_err, axis=1), np.linalg.norm(rot_err, axis=1)
    act_mag = np.linalg.norm(act, axis=1) / act.shape[1]
    drop = pos_dist > drop_th
    bonus = 1.0 * (pos_dist < 2 * pos_th) + 1.0 * (pos_dist < pos_th)
    dense = w["pos_dist"] * -pos_dist + w["rot_dist"] * -rot_dist + w["bonus"] * bonus + w["act_reg"] * -act_mag + w["penalty"] * -1.0 * drop
    return obs, dense, drop, (pos_dist < pos_th) & (rot_dist < rot_th) & ~drop
