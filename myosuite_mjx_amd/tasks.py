"""One record per task of the batched envs: the Python counterpart of the library's `TaskHooks` records (csrc/myo_host.h).

A `Task` names the env kwargs its task accepts on top of COMMON_KWARGS, the kwargs it refuses (with the reason), and `setup(m, spec, env_id)`:
host arithmetic only (init pose, noise / clip vectors, goal ranges, site ids), no `capi` handle.  `setup` returns a `Setup`: the binding
call to make with its keyword arguments, and the calls that follow it (the width of the observation row is not among them: it is the sum of
the default keys' widths, observations.py).  `BatchedMyoEnv.__init__` (envs.py) looks the record up, filters the kwargs
with `filter_kwargs` and applies the `Setup`; a new task is one `setup` function and one entry of TASKS, next to its registry entries in envs.py."""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from . import capi

COMMON_KWARGS = ("reset_type", "fatigue_reset_random", "fatigue_reset_vec")     # honoured for every task (others raise)


class Setup(NamedTuple):
    call: str                      # "configure" or "configure_walk" (capi.HipBatch)
    kwargs: dict                   # the call's keyword arguments
    then: tuple = ()               # HipBatch calls after it, in order: (method, args) of set_body_pos_range / set_body_quat_range / set_geom_override
    body_mass_range: tuple = None  # (body, lo, hi) for BatchedMyoEnv.set_body_mass_range (PoseEnvV0 weight_bodyname / weight_range)


class Task(NamedTuple):
    setup: Callable                # setup(m, spec, env_id) -> Setup
    label: str                     # the task's name in messages
    kwargs: tuple = ()             # env kwargs of the reference's env class honoured for this task only
    refused: tuple = ()            # kwargs of that class that cannot be honoured (None is let through, anything else raises) ...
    refused_why: str = ""          # ... and why


def _open_hand(m, nobj, wrist):
    """init_qpos of the hand-and-object tasks: fully open hand, palm up (qpos[0] = wrist), the last `nobj` coordinates (the object) at qpos0."""
    init = np.array(m.qpos0, float)
    init[:-nobj] = 0.0
    init[0] = wrist
    return init


def target_jnt_range(m, spec):
    """pose_v0.py:67-75: {joint name: (lo, hi)} replaces the registered target range; it must name exactly the targeted joints."""
    n = len(spec["target_lo"])
    targeted = [m.names["joint"][j] for j in range(m.njnt) if int(m.jnt_qposadr[j]) < n]
    rng = dict(spec["target_jnt_range"])
    if sorted(rng) != sorted(targeted):
        raise ValueError(f"target_jnt_range must name exactly the joints {targeted} (got {sorted(rng)})")
    lo, hi = np.array(spec["target_lo"], float), np.array(spec["target_hi"], float)
    for name, (a, b) in rng.items():
        q = int(m.jnt_qposadr[m.name2id("joint", name)])
        lo[q], hi[q] = float(a), float(b)
    return lo, hi


def _pose(m, spec, env_id):
    w = spec["weights"]
    if spec.get("target_jnt_range") is not None:
        spec["target_lo"], spec["target_hi"] = target_jnt_range(m, spec)
    mass = None
    if spec.get("weight_bodyname") is not None:                # pose_v0.py:163-176: body mass ~ U(weight_range) at every reset
        if spec.get("weight_range") is None:
            raise ValueError(f"{env_id}: weight_bodyname needs weight_range")
        mass = (spec["weight_bodyname"], *spec["weight_range"])
    return Setup("configure", dict(
        task=capi.TASK_POSE, frame_skip=spec["frame_skip"],
        reset_random=spec["reset_type"] == "random", target_generate=spec["target_type"] == "generate",
        target_lo=spec["target_lo"], target_hi=spec["target_hi"], init_qpos=m.qpos0, pose_thd=spec["pose_thd"], far_th=4 * np.pi / 2,
        w_pose=w["pose"], w_bonus=w["bonus"], w_act_reg=w["act_reg"], w_penalty=w["penalty"]), body_mass_range=mass)


def _reach(m, spec, env_id):
    w = spec["weights"]
    tips = [m.name2id("site", t) for t in spec["tips"]]
    n = len(tips)
    return Setup("configure", dict(
        task=capi.TASK_REACH, frame_skip=spec["frame_skip"], reset_random=0, target_generate=spec["target_type"] == "generate",
        target_lo=spec["target_lo"], target_hi=spec["target_hi"], init_qpos=m.qpos0, tip_sites=tips, far_th=spec["far_th"] * n, near_th=0.0125 * n,
        w_reach=w["reach"], w_bonus=w["bonus"], w_act_reg=w["act_reg"], w_penalty=w["penalty"]))


def _walk(m, spec, env_id):
    w = spec["weights"]
    key_qpos = np.asarray(m.key_qpos).reshape(-1, m.nq)
    key_qvel = np.asarray(m.key_qvel).reshape(-1, m.nv)
    # walk_v0.py:254 init_qpos = key_qpos[0] (the reference orientation of ref_rot); reset "init" starts from keyframe 2
    # (walk_v0.py:339-349), "random" from keyframe 2 or 3 with N(0, 0.02) noise (:316-332; drawn by the reset kernel)
    if spec["reset_type"] not in ("init", "random"):
        raise NotImplementedError("myoLegWalk: reset_type 'init' (keyframe 2) or 'random' (walk_v0.py:316-332)")
    rnd = spec["reset_type"] == "random"
    jadr = lambda n: int(m.jnt_qposadr[m.name2id("joint", n)])
    return Setup("configure_walk", dict(
        frame_skip=spec["frame_skip"], hip_period=spec["hip_period"], min_height=spec["min_height"], max_rot=spec["max_rot"],
        target_x_vel=spec["target_x_vel"], target_y_vel=spec["target_y_vel"],
        target_rot=spec["target_rot"] if spec["target_rot"] is not None else key_qpos[0][3:7],
        bodies=[m.name2id("body", n) for n in ("talus_l", "talus_r", "pelvis", "torso")],
        qadr_hip_flexion=[jadr("hip_flexion_l"), jadr("hip_flexion_r")],
        qadr_joint_angle=[jadr(n) for n in ("hip_adduction_l", "hip_adduction_r", "hip_rotation_l", "hip_rotation_r")],
        weights=[w[k] for k in ("vel_reward", "done", "cyclic_hip", "ref_rot", "joint_angle_rew")],
        init_qpos=key_qpos[2], init_qvel=key_qvel[2], knee_height=spec.get("knee_height", 0.0),
        terrain={"rough": capi.TERRAIN_ROUGH, "hilly": capi.TERRAIN_HILLY, "stairs": capi.TERRAIN_STAIRS}.get(spec.get("terrain"), capi.TERRAIN_NONE),
        terrain_scalar=spec.get("terrain_scalar", (0.0, 0.0)),
        init_qpos_alt=key_qpos[3] if rnd else None, init_qvel_alt=key_qvel[3] if rnd else None, reset_noise_std=0.02 if rnd else 0.0))


def _stand(m, spec, env_id):
    from .mjcf import quat2mat
    w = spec["weights"]
    key_qpos = np.asarray(m.key_qpos).reshape(-1, m.nq)
    key_qvel = np.asarray(m.key_qvel).reshape(-1, m.nv)
    init = key_qpos[0].astype(float)                              # walk_v0.py:63-64
    adr = np.asarray(m.jnt_qposadr)
    nlo, nhi = np.zeros(m.nq), np.zeros(m.nq)
    clo, chi = np.full(m.nq, -1e30), np.full(m.nq, 1e30)
    nlo[adr], nhi[adr] = spec["joint_random_range"]               # generate_qpos (:152-167): only each joint's first coordinate moves ...
    clo[adr], chi[adr] = m.jnt_range[:, 0], m.jnt_range[:, 1]      # ... and is clipped to jnt_range -- (0, 0) for the unlimited free root: x = 0
    tsid = m.name2id("site", spec["tip"])
    if int(m.hip_site_link[tsid]) != 0:
        raise NotImplementedError("stand task: the tip site must ride on the free root link")
    lpos = np.asarray(m.hip_site_lpos[tsid], float)
    q0 = np.clip(init[:7] + 0.0, np.r_[clo[:1], [-1e30] * 6], np.r_[chi[:1], [1e30] * 6])
    p0 = q0[:3] + quat2mat(q0[3:7] / np.linalg.norm(q0[3:7])) @ lpos     # generate_targets (:140-149): the site in the first random pose
    span = np.asarray(spec["target_span"], float)
    return Setup("configure", dict(
        task=capi.TASK_STAND, frame_skip=spec["frame_skip"], reset_random=0, target_generate=1,
        target_lo=p0 + span[0], target_hi=p0 + span[1], init_qpos=init, init_qvel=key_qvel[0],
        reset_noise=(nlo, nhi), reset_clip=(clo, chi), tip_lpos=lpos, near_th=spec["near_th"], far_th=spec["far_th"],
        w_reach=w["reach"], w_bonus=w["bonus"], w_act_reg=w["act_reg"], w_penalty=w["penalty"]))


def _hold(m, spec, env_id):
    w = spec["weights"]
    if spec["goal"] is None:                                       # Random: around the object's site at the model's initial pose (:125-131)
        glo, ghi = np.asarray(m.qpos0[-7:-4], float) - spec["goal_span"], np.asarray(m.qpos0[-7:-4], float) + spec["goal_span"]
    else:
        glo = ghi = np.asarray(spec["goal"], float)
    then = (("set_geom_override", (m.name2id("geom", "object"), *spec["object_size"])),) if "object_size" in spec else ()
    return Setup("configure", dict(
        task=capi.TASK_HOLD, frame_skip=spec["frame_skip"], reset_random=0, target_generate=int(spec["goal"] is None),
        target_lo=glo, target_hi=ghi, init_qpos=_open_hand(m, 7, -1.5), near_th=spec["goal_th"], far_th=spec["drop_th"],       # obj_hold_v0.py:63-64
        w_reach=w["goal_dist"], w_bonus=w["bonus"], w_act_reg=w["act_reg"], w_penalty=w["penalty"]), then)


def _keyturn(m, spec, env_id):
    # key_turn_v0.py:54-75, 157-169: fully open hand (init_qpos[:-1] = 0), key angle ~ U(key_init_range) (a reset noise on the last
    # coordinate only); the Random variant (key_init_range[0] != key_init_range[1]) also re-draws the key body's position
    w = spec["weights"]
    lo_k, hi_k = (float(x) for x in spec["key_init_range"])
    if not hi_k >= lo_k:
        raise ValueError(f"{env_id}: key_init_range must be (lo, hi) with lo <= hi")
    nlo, nhi = np.zeros(m.nq), np.zeros(m.nq)
    nlo[-1], nhi[-1] = lo_k, hi_k
    big = np.full(m.nq, 1e30)
    # key_turn_v0.py:164-167: key_init_pos + U(-0.01, 0.01)^3
    then = (("set_body_pos_range", (np.full(3, -0.01), np.full(3, 0.01))),) if lo_k != hi_k else ()
    return Setup("configure", dict(
        task=capi.TASK_KEYTURN, frame_skip=spec["frame_skip"], reset_random=0, target_generate=0, init_qpos=np.zeros(m.nq),
        reset_noise=(nlo, nhi), reset_clip=(-big, big), tip_sites=[m.name2id("site", n) for n in ("keyhead", "IFtip", "THtip")],
        pose_thd=float(spec["goal_th"]), near_th=0.030, far_th=0.1,
        w_pose=w["key_turn"], w_reach=w["IFtip_approach"], w_act_reg=w["act_reg"], w_bonus=w["bonus"], w_penalty=w["penalty"]), then)


def _pen(m, spec, env_id):
    # pen_v0.py:60-96: palm-up open hand, pen at qpos0; sites object top / bottom, target top / bottom, eps_ball; the object body's
    # origin in its link frame.  Random (pen_v0.py:173-184): the target's orientation is re-drawn at every reset
    w = spec["weights"]
    ob = m.name2id("body", "Object")
    then = (("set_body_quat_range", tuple(spec["target_euler_range"])),) if spec.get("target_euler_range") is not None else ()
    return Setup("configure", dict(
        task=capi.TASK_PEN, frame_skip=spec["frame_skip"], reset_random=0, target_generate=0, init_qpos=_open_hand(m, 6, -1.5),
        tip_sites=[m.name2id("site", n) for n in ("object_top", "object_bottom", "target_top", "target_bottom", "eps_ball")],
        tip_lpos=tuple(np.asarray(m.hip_body_lpos).reshape(-1, 3)[ob]), pose_thd=0.95, far_th=0.075,
        w_pose=w["pos_align"], w_reach=w["rot_align"], w_act_reg=w["act_reg"], w_bonus=w["bonus"], w_penalty=w["drop"],
        quat_body=m.name2id("body", "target")), then)


def _baoding(m, spec, env_id):
    # baoding_v1.py:54-145, 325-383: palm-up open hand, balls at qpos0; sites ball1, ball2, target1, target2.  Goal parameters per env
    # (MYO_F_TARGET row: start angle, sign, x radius, y radius, period) ~ U(lo, hi) at every reset: "fixed" is BAODING_CCW from pi / 4,
    # "random" draws the direction from HOLD / CW / CCW (the sign U(-1, 2) rounded down) and the start angle from U(0, 2 pi)
    w = spec["weights"]
    if spec["task_choice"] not in ("fixed", "random"):
        raise ValueError(f"{env_id}: task_choice must be 'fixed' or 'random'")
    rnd = spec["task_choice"] == "random"
    (p0, p1), (x0, x1), (y0, y1) = ((float(a) for a in spec[k]) for k in ("goal_time_period", "goal_xrange", "goal_yrange"))
    if not (0 < p0 <= p1 and x0 <= x1 and y0 <= y1):
        raise ValueError(f"{env_id}: goal_time_period, goal_xrange and goal_yrange must be (lo, hi) with lo <= hi (periods > 0)")
    glo = [0.0 if rnd else np.pi / 4, -1.0 if rnd else 1.0, x0, y0, p0]
    ghi = [2 * np.pi if rnd else np.pi / 4, 2.0 if rnd else 1.0, x1, y1, p1]
    return Setup("configure", dict(
        task=capi.TASK_BAODING, frame_skip=spec["frame_skip"], reset_random=0, target_generate=1, target_lo=glo, target_hi=ghi,
        init_qpos=_open_hand(m, 14, -1.57), tip_sites=[m.name2id("site", n) for n in ("ball1_site", "ball2_site", "target1_site", "target2_site")],
        pose_thd=float(spec["proximity_th"]), far_th=float(spec["drop_th"]), w_pose=w["pos_dist_1"], w_reach=w["pos_dist_2"]))


def _die(m, spec, env_id):
    # reorient_v0.py:45-109, 209-250: palm-up open hand (init_qpos[:-7] = 0: the die's first slide is zeroed too, as the reference
    # does), die at qpos0; sites = the origin and axis points of the die's and the target's frames.  The goal offset (MYO_F_TARGET row)
    # ~ U(goal_pos)^3 and the target's Euler angles ~ U(goal_rot)^3 are re-drawn per env at every reset
    w = spec["weights"]
    (p0, p1), (r0, r1) = ((float(a) for a in spec[k]) for k in ("goal_pos", "goal_rot"))
    if not (p0 <= p1 and r0 <= r1):
        raise ValueError(f"{env_id}: goal_pos and goal_rot must be (lo, hi) with lo <= hi")
    return Setup("configure", dict(
        task=capi.TASK_DIE, frame_skip=spec["frame_skip"], reset_random=0, target_generate=1, target_lo=[p0] * 3, target_hi=[p1] * 3,
        init_qpos=_open_hand(m, 7, -1.5),
        tip_sites=[m.name2id("site", n) for n in ("object_o", "object_x", "object_y", "object_z", "target_o", "target_x", "target_y", "target_z")],
        near_th=float(spec["pos_th"]), pose_thd=float(spec["rot_th"]), far_th=float(spec["drop_th"]),
        w_pose=w["pos_dist"], w_reach=w["rot_dist"], w_bonus=w["bonus"], w_act_reg=w["act_reg"], w_penalty=w["penalty"],
        quat_body=m.name2id("body", "target")), (("set_body_quat_range", ([r0] * 3, [r1] * 3)),))


_NO_PER_ENV = "re-draws the {0} size, mass or friction per episode; the TrackEnv-class step kernel has no per-env {1} size, mass or friction"
TASKS = {
    "pose": Task(_pose, "pose", ("weight_bodyname", "weight_range", "target_jnt_range")),                      # PoseEnvV0 (pose_v0.py:56-75)
    "reach": Task(_reach, "reach"),
    "hold": Task(_hold, "hold"),
    "stand": Task(_stand, "stand"),
    "walk": Task(_walk, "walk"),
    "keyturn": Task(_keyturn, "key-turn", ("goal_th", "key_init_range")),                                      # KeyTurnEnvV0._setup (key_turn_v0.py:54-61)
    "pen": Task(_pen, "pen"),
    "baoding": Task(_baoding, "baoding", ("task_choice", "goal_time_period", "goal_xrange", "goal_yrange", "drop_th", "proximity_th"),
                    ("obj_size_range", "obj_mass_range", "obj_friction_change"), _NO_PER_ENV.format("balls'", "ball")),   # BaodingEnvV1._setup (baoding_v1.py:54-69)
    "die": Task(_die, "die", ("goal_pos", "goal_rot", "pos_th", "rot_th", "drop_th"),                           # ReorientEnvV0._setup (reorient_v0.py:45-62)
                ("obj_size_change", "obj_mass_range", "obj_friction_change"), _NO_PER_ENV.format("die's", "die")),
}
# every kwarg some task honours, each once, in the order of TASKS
ENV_KWARGS = tuple(dict.fromkeys(COMMON_KWARGS + sum((t.kwargs for t in TASKS.values()), ())))


def filter_kwargs(env_id, spec, env_kwargs):
    """Move the env kwargs the task of `spec` honours into `spec`; refuse the others (host only: before any model or GPU work)."""
    task = TASKS[spec["task"]]
    for k, v in env_kwargs.items():
        if k in task.refused:
            if v is not None:
                raise NotImplementedError(f"{env_id}: {k} {task.refused_why}")
            continue
        if k not in COMMON_KWARGS + task.kwargs:
            owners = " / ".join(t.label for t in TASKS.values() if k in t.kwargs)
            raise TypeError(f"{env_id}: unsupported env kwarg {k!r} (" + (f"{owners} task only" if owners else
                            f"the {task.label} task takes {COMMON_KWARGS + task.kwargs}") + ")")
        spec[k] = v
