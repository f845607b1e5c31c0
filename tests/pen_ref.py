"""Float64 restatement of PenTwirlFixedEnvV0's observation, reward, done and solved (envs/myo/myobase/pen_v0.py:98-170, act appended by
base_v0.py:34-38), batched over envs, from the state and the world positions of the five task sites, and the reference's euler2quat
(utils/quat_math.py:77-93).  Shared by tests/test_pen_host.py (oracle states) and tests/test_gpu_pen.py (HIP states)."""
import numpy as np

WEIGHTS = dict(pos_align=1.0, rot_align=1.0, act_reg=5.0, drop=5.0, bonus=10.0)
PEN_LENGTH = 0.13        # |site_pos[top] - site_pos[bottom]| of the object and of the target (myohand_pen.xml)


def euler2quat(euler):
    euler = np.asarray(euler, np.float64)
    ai, aj, ak = euler[..., 2] / 2, -euler[..., 1] / 2, euler[..., 0] / 2
    si, sj, sk = np.sin(ai), np.sin(aj), np.sin(ak)
    ci, cj, ck = np.cos(ai), np.cos(aj), np.cos(ak)
    cc, cs, sc, ss = ci * ck, ci * sk, si * ck, si * sk
    q = np.empty(euler.shape[:-1] + (4,))
    q[..., 0] = cj * cc + sj * ss
    q[..., 3] = cj * sc - sj * cs
    q[..., 2] = -(cj * ss + sj * cc)
    q[..., 1] = cj * cs - sj * sc
    return q


def pen_restate(qpos, qvel, act, sites, obj_pos, dt, w=WEIGHTS):
    """qpos, qvel [B, nq]; act [B, na]; sites [B, 15] = object top | object bottom | target top | target bottom | eps_ball; obj_pos [B, 3]
    (body xpos of Object).  Returns obs [B, nq - 6 + 21 + na], dense reward, done, solved (float64 / bool)."""
    qpos, qvel, act, sites, obj_pos = (np.atleast_2d(np.asarray(a, np.float64)) for a in (qpos, qvel, act, sites, obj_pos))
    ot, ob, tt, tb, eps = (sites[:, 3 * k:3 * k + 3] for k in range(5))
    rot, drot = (ot - ob) / PEN_LENGTH, (tt - tb) / PEN_LENGTH
    err_pos = obj_pos - eps
    obs = np.concatenate([qpos[:, :-6], obj_pos, qvel[:, -6:] * dt, rot, drot, err_pos, rot - drot, act], axis=1)
    pos_align = np.linalg.norm(err_pos, axis=1)
    npr = np.linalg.norm(rot, axis=1) * np.linalg.norm(drot, axis=1)
    rot_align = np.einsum("ij,ij->i", rot, drot) / np.where(npr == 0, 1.0, npr)
    dropped = pos_align > 0.075
    act_mag = np.linalg.norm(act, axis=1) / act.shape[1]
    bonus = 1.0 * (rot_align > 0.9) * (pos_align < 0.075) + 5.0 * (rot_align > 0.95) * (pos_align < 0.075)
    dense = w["pos_align"] * -pos_align + w["rot_align"] * rot_align + w["act_reg"] * -act_mag + w["drop"] * -1.0 * dropped + w["bonus"] * bonus
    return obs, dense, dropped, (rot_align > 0.95) & ~dropped
