"""Float64 restatement of KeyTurnEnvV0's observation, reward, done and solved (envs/myo/myobase/key_turn_v0.py:82-156, act appended by
base_v0.py:34-38), batched over envs, from the state and the world positions of the three sites (key head, index tip, thumb tip).
Shared by tests/test_keyturn_host.py (oracle states) and tests/test_gpu_keyturn.py (HIP states)."""
import numpy as np

WEIGHTS = dict(key_turn=1.0, IFtip_approach=10.0, THtip_approach=10.0, act_reg=1.0, bonus=4.0, penalty=25.0)


def keyturn_restate(qpos, qvel, act, sites, dt, goal_th, w=WEIGHTS):
    """qpos, qvel [B, nq]; act [B, na]; sites [B, 9] = key head | IFtip | THtip world positions.  Returns obs [B, 2 nq + 6 + na], dense
    reward, done, solved (float64 / bool)."""
    qpos, qvel, act, sites = (np.atleast_2d(np.asarray(a, np.float64)) for a in (qpos, qvel, act, sites))
    head, iftip, thtip = sites[:, 0:3], sites[:, 3:6], sites[:, 6:9]
    if_app, th_app = head - iftip, head - thtip
    obs = np.concatenate([qpos[:, :-1], qvel[:, :-1] * dt, qpos[:, -1:], qvel[:, -1:] * dt, if_app, th_app, act], axis=1)
    d_if = np.abs(np.linalg.norm(if_app, axis=1) - 0.030)
    d_th = np.abs(np.linalg.norm(th_app, axis=1) - 0.030)
    key_q = qpos[:, -1]
    act_mag = np.linalg.norm(act, axis=1) / act.shape[1]
    far_th = 0.1
    bonus = 1.0 * (key_q > np.pi / 2) + 1.0 * (key_q > np.pi)
    penalty = -1.0 * (d_if > far_th / 2) - 1.0 * (d_th > far_th / 2)
    dense = (w["key_turn"] * key_q + w["IFtip_approach"] * -d_if + w["THtip_approach"] * -d_th + w["act_reg"] * -act_mag
             + w["bonus"] * bonus + w["penalty"] * penalty)
    return obs, dense, (d_if > far_th) | (d_th > far_th), key_q > goal_th
