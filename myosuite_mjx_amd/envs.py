"""Batched MyoSuite task envs on the HIP stepper, keeping the reference's gym-style API.

Mirrors (paths relative to /root/reference/myosuite/):
  * env ids, kwargs and episode lengths      envs/myo/myobase/__init__.py:258-297,300-413,523-571
  * action map + frame_skip                  envs/myo/base_v0.py:23-59,83-119
  * obs / reward / done / reset, pose task   envs/myo/myobase/pose_v0.py:98-138,141-255
  * obs / reward / done / reset, reach task  envs/myo/myobase/reach_v0.py:88-159
  * obs vector layout and float32 cast       envs/obs_vec_dict.py:86-98
  * gym step contract (obs, rwd, terminated, truncated, info)   envs/env_base.py:335-390

One env object steps `num_envs` environments in one kernel launch; tensors stay on the device
(torch views of the library's buffers, zero copy).  Physics runs only in libmyo_hip.so.
"""
from __future__ import annotations

import numpy as np

from . import capi, objects, observations, rewards, tasks, track
from . import model as _model

# ASL pose table (envs/myo/myobase/__init__.py:326-376): target joint vectors of myoHandPose{k}Fixed-v0;
# the per-joint min/max over the ten rows is the target range of myoHandPoseRandom-v0 (:396-399)
ASL_QPOS = np.array([
    [0, 0, 0, 0.5624, 0.28272, -0.75573, -1.309, 1.30045, -0.006982, 1.45492, 0.998897, 1.26466, 0, 1.40604, 0.227795, 1.07614, -0.020944, 1.46103, 0.06284, 0.83263, -0.14399, 1.571, 1.38248],
    [0, 0, 0, 0.0248, 0.04536, -0.7854, -1.309, 0.366605, 0.010473, 0.269258, 0.111722, 1.48459, 0, 1.45318, 1.44532, 1.44532, -0.204204, 1.46103, 1.44532, 1.48459, -0.2618, 1.47674, 1.48459],
    [0, 0, 0, 0.0248, 0.04536, -0.7854, -1.13447, 0.514973, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 1.44532, -0.204204, 1.46103, 1.44532, 1.48459, -0.2618, 1.47674, 1.48459],
    [0, 0, 0, 0.3384, 0.25305, 0.01569, -0.0262045, 0.645885, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 1.571, -0.036652, 1.52387, 1.45318, 1.40604, -0.068068, 1.39033, 1.571],
    [0, 0, 0, 0.6392, -0.147495, -0.7854, -1.309, 0.637158, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 0.306345, -0.010472, 0.400605, 0.133535, 0.21994, -0.068068, 0.274925, 0.01571],
    [0, 0, 0, 0.3384, 0.25305, 0.01569, -0.0262045, 0.645885, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 0.306345, -0.010472, 0.400605, 0.133535, 0.21994, -0.068068, 0.274925, 0.01571],
    [0, 0, 0, 0.6392, -0.147495, -0.7854, -1.309, 0.637158, 0.010473, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 0.306345, -0.010472, 0.400605, 0.133535, 1.1861, -0.2618, 1.35891, 1.48459],
    [0, 0, 0, 0.524, 0.01569, -0.7854, -1.309, 0.645885, -0.006982, 0.128305, 0.111722, 0.510575, 0, 0.37704, 0.117825, 1.28036, -0.115192, 1.52387, 1.45318, 0.432025, -0.068068, 0.18852, 0.149245],
    [0, 0, 0, 0.428, 0.22338, -0.7854, -1.309, 0.645885, -0.006982, 0.128305, 0.194636, 1.39033, 0, 1.08399, 0.573415, 0.667675, -0.020944, 0, 0.06284, 0.432025, -0.068068, 0.18852, 0.149245],
    [0, 0, 0, 0.5624, 0.28272, -0.75573, -1.309, 1.30045, -0.006982, 1.45492, 0.998897, 0.39275, 0, 0.18852, 0.227795, 0.667675, -0.020944, 0, 0.06284, 0.432025, -0.068068, 0.18852, 0.149245],
])
# myoHandPoseFixed-v0 target (envs/myo/myobase/__init__.py:265-291)
HAND_POSE_FIXED = np.array([0, 0, 0, -0.0904, 0.0824475, -0.681555, -0.514888, 0, -0.013964, -0.0458132, 0, 0.67553,
                            -0.020944, 0.76979, 0.65982, 0, 0, 0, 0, 0.479155, -0.099484, 0.95831, 0])
HAND_TIPS = ("THtip", "IFtip", "MFtip", "RFtip", "LFtip")
# myoHandReach* target spans (envs/myo/myobase/__init__.py:523-571)
_REACH_CENTRE = {"THtip": (-0.165, -0.537, 1.495), "IFtip": (-0.151, -0.547, 1.455), "MFtip": (-0.146, -0.547, 1.447),
                 "RFtip": (-0.148, -0.543, 1.445), "LFtip": (-0.148, -0.528, 1.434)}
_REACH_SPAN = {"THtip": ((-0.020, -0.040, -0.040), (0.040, 0.020, 0.040)),
               "IFtip": ((-0.040, -0.020, -0.010), (0.040, 0.020, 0.010)),
               "MFtip": ((-0.040, -0.020, -0.010), (0.040, 0.020, 0.010)),
               "RFtip": ((-0.040, -0.020, -0.010), (0.040, 0.020, 0.010)),
               "LFtip": ((-0.040, -0.020, -0.010), (0.040, 0.020, 0.010))}


def _pose_spec(target_lo, target_hi, reset_type, target_type, pose_thd=0.7, model="myohand_pose"):
    return dict(model=model, task="pose", max_episode_steps=100, frame_skip=10, normalize_act=True,
                target_lo=np.asarray(target_lo, float), target_hi=np.asarray(target_hi, float),
                reset_type=reset_type, target_type=target_type, pose_thd=pose_thd,
                weights=dict(pose=1.0, bonus=4.0, act_reg=1.0, penalty=50.0))


def _reach_spec(random, far_th):
    lo, hi = [], []
    for tip in HAND_TIPS:
        c = np.array(_REACH_CENTRE[tip])
        a, b = (np.array(_REACH_SPAN[tip][0]), np.array(_REACH_SPAN[tip][1])) if random else (np.zeros(3), np.zeros(3))
        lo.append(c + a)
        hi.append(c + b)
    return dict(model="myohand_pose", task="reach", max_episode_steps=100, frame_skip=10, normalize_act=True,
                target_lo=np.concatenate(lo), target_hi=np.concatenate(hi), tips=HAND_TIPS, far_th=far_th,
                reset_type="init", target_type="generate" if random else "fixed",
                weights=dict(reach=1.0, bonus=4.0, penalty=50.0, act_reg=0.0))


def _reach_box_spec(model, tips, lo, hi, far_th, max_episode_steps=100, frame_skip=10):
    """ReachEnvV0 with target_reach_range given as absolute boxes (reach_v0.py:147-153: the target is always re-drawn at reset)."""
    return dict(model=model, task="reach", max_episode_steps=max_episode_steps, frame_skip=frame_skip, normalize_act=True,
                target_lo=np.asarray(lo, float).ravel(), target_hi=np.asarray(hi, float).ravel(), tips=tuple(tips), far_th=far_th,
                reset_type="init", target_type="generate",
                weights=dict(reach=1.0, bonus=4.0, penalty=50.0, act_reg=0.0))


REGISTRY = {
    "myoHandPoseFixed-v0": _pose_spec(HAND_POSE_FIXED, HAND_POSE_FIXED, "init", "fixed"),
    "myoHandPoseRandom-v0": _pose_spec(ASL_QPOS.min(0), ASL_QPOS.max(0), "random", "generate"),
    "myoHandReachFixed-v0": _reach_spec(False, 0.044),
    "myoHandReachRandom-v0": _reach_spec(True, 0.034),
}
# myoFingerPose*-v0 (envs/myo/myobase/__init__.py:222-253): joints IFadb, IFmcp, IFpip, IFdip; defaults reset "init",
# target "generate", pose_thd 0.35 (pose_v0.py:46-57)
REGISTRY["myoFingerPoseFixed-v0"] = _pose_spec([0, 0, 0.75, 0.75], [0, 0, 0.75, 0.75], "init", "generate", 0.35, "myofinger_v0")
REGISTRY["myoFingerPoseRandom-v0"] = _pose_spec([-0.2, -0.4, 0.1, 0.1], [0.2, 1.0, 1.0, 1.0], "init", "generate", 0.35, "myofinger_v0")
# myoElbowPose1D6M*-v0 (envs/myo/myobase/__init__.py:108-137): 1-dof elbow with 6 muscles, reset "random", pose_thd 0.175
REGISTRY["myoElbowPose1D6MFixed-v0"] = _pose_spec([2.0], [2.0], "random", "generate", 0.175, "myoelbow_1dof6muscles")
REGISTRY["myoElbowPose1D6MRandom-v0"] = _pose_spec([0.0], [2.27], "random", "generate", 0.175, "myoelbow_1dof6muscles")
# motorFinger{Reach,Pose}*-v0 (envs/myo/myobase/__init__.py:55-81,188-219): the finger driven by five tendon motors (ctrlrange -1..0, no
# activation state: observations carry no act block), frame_skip 5, 200-step episodes
REGISTRY["motorFingerReachFixed-v0"] = _reach_box_spec("motorfinger_v0", ("IFtip",), [(0.2, 0.05, 0.20)], [(0.2, 0.05, 0.20)], 0.35, 200, 5)
REGISTRY["motorFingerReachRandom-v0"] = _reach_box_spec("motorfinger_v0", ("IFtip",), [(0.1, -0.1, 0.1)], [(0.27, 0.1, 0.3)], 0.35, 200, 5)
REGISTRY["motorFingerPoseFixed-v0"] = dict(_pose_spec([0, 0, 0.75, 0.75], [0, 0, 0.75, 0.75], "init", "generate", 0.35, "motorfinger_v0"),
                                           max_episode_steps=200, frame_skip=5)
REGISTRY["motorFingerPoseRandom-v0"] = dict(_pose_spec([-0.2, -0.4, 0.1, 0.1], [0.2, 1.0, 1.0, 1.0], "init", "generate", 0.35, "motorfinger_v0"),
                                            max_episode_steps=200, frame_skip=5)
# myoElbowPose1D6MExoFixed-v0 (envs/myo/myobase/__init__.py:140-160): the elbow with an exoskeleton motor on the joint (actuator 0) and
# act_reg weight 5.  (ExoRandom = this id with the reference's kwargs weight_bodyname="carry_weight", weight_range=(0.1, 2.0) and
# target_jnt_range={"r_elbow_flex": (0, 2.27)}: a per-env body mass re-drawn at every reset, see BatchedMyoEnv.body_mass.)
REGISTRY["myoElbowPose1D6MExoFixed-v0"] = dict(_pose_spec([2.0], [2.0], "random", "generate", 0.175, "myoelbow_1dof6muscles_1dofexo"),
                                               weights=dict(pose=1.0, bonus=4.0, act_reg=5.0, penalty=50.0))
# myoHandObjHoldFixed-v0 (envs/myo/myobase/__init__.py:596-604, obj_hold_v0.py:13-118): MyoHand palm up + a free ellipsoid object; goal = the
# model's goal site.  (ObjHoldRandom re-draws the object's geom size per episode: a per-env model edit, not offered.)
REGISTRY["myoHandObjHoldFixed-v0"] = dict(
    model="myohand_hold", task="hold", max_episode_steps=75, frame_skip=10, normalize_act=True, reset_type="init",
    goal=(-0.240, -0.520, 1.470), goal_th=0.010, drop_th=0.300,
    weights=dict(goal_dist=100.0, bonus=4.0, penalty=10.0, act_reg=0.0))
# myoHandObjHoldRandom-v0 (:605-613, ObjHoldRandomEnvV0 obj_hold_v0.py:121-140): goal = object's initial position + U(+-0.03)^3 and the object's
# ellipsoid semi-axes ~ U(0.02, 0.03)^3, both re-drawn per episode (the size is a per-env override of that one geom; mass / inertia stay)
REGISTRY["myoHandObjHoldRandom-v0"] = dict(REGISTRY["myoHandObjHoldFixed-v0"], goal=None, goal_span=0.030, object_size=((0.020,) * 3, (0.030,) * 3))
# myoFingerReach*-v0 (envs/myo/myobase/__init__.py:82-105): IFtip to an absolute target box; far_th = ReachEnvV0's default 0.35
REGISTRY["myoFingerReachFixed-v0"] = _reach_box_spec("myofinger_v0", ("IFtip",), [(0.2, 0.05, 0.20)], [(0.2, 0.05, 0.20)], 0.35)
REGISTRY["myoFingerReachRandom-v0"] = _reach_box_spec("myofinger_v0", ("IFtip",), [(0.1, -0.1, 0.1)], [(0.27, 0.1, 0.3)], 0.35)
for _k in range(10):
    REGISTRY[f"myoHandPose{_k}Fixed-v0"] = _pose_spec(ASL_QPOS[_k], ASL_QPOS[_k], "init", "fixed")
# myoLegWalk-v0 (envs/myo/myobase/__init__.py:443-459; WalkEnvV0 defaults walk_v0.py:187-266)
REGISTRY["myoLegWalk-v0"] = dict(
    model="myolegs", task="walk", max_episode_steps=1000, frame_skip=10, normalize_act=True, reset_type="init",
    min_height=0.8, max_rot=0.8, hip_period=100, target_x_vel=0.0, target_y_vel=1.2, target_rot=None,
    weights=dict(vel_reward=5.0, done=-100.0, cyclic_hip=-10.0, ref_rot=10.0, joint_angle_rew=5.0))
# myoLegStandRandom-v0 (envs/myo/myobase/__init__.py:424-441; walk_v0.py:13-183 ReachEnvV0): keep the pelvis site at a target drawn around its
# position in the (randomised) start pose; joint_random_range (-0.2, 0.2) on every joint's first coordinate, clipped to the joint range
REGISTRY["myoLegStandRandom-v0"] = dict(
    model="myolegs", task="stand", max_episode_steps=150, frame_skip=10, normalize_act=True, reset_type="random", tip="pelvis",
    joint_random_range=(-0.2, 0.2), target_span=((-0.05, -0.05, 0.0), (0.05, 0.05, 0.0)), far_th=0.44, near_th=0.050,
    weights=dict(reach=1.0, bonus=4.0, penalty=50.0, act_reg=1.0))
# myoLeg{Rough,Hilly,Stair}TerrainWalk-v0 (envs/myo/myobase/__init__.py:462-520; TerrainEnvV0, walk_v0.py:490-671): the walk task on a height
# field re-drawn per episode; hilly / stairs are registered with variant "fixed" (height scale 0.63 / 2.5; otherwise U(0.53, 0.73) / U(1.5, 3.5))
for _id, _kind, _sc in (("myoLegRoughTerrainWalk-v0", "rough", (0.0, 0.0)), ("myoLegHillyTerrainWalk-v0", "hilly", (0.63, 0.63)),
                        ("myoLegStairTerrainWalk-v0", "stairs", (2.5, 2.5))):
    REGISTRY[_id] = dict(REGISTRY["myoLegWalk-v0"], model="myolegs_terrain", terrain=_kind, terrain_scalar=_sc, knee_height=0.61)
# myoHandKeyTurn{Fixed,Random}-v0 (envs/myo/myobase/__init__.py:574-593, key_turn_v0.py): MyoHand + a key on a hinge with friction loss (a
# model of the TrackEnv class: the key's box bit, the hinge's frictionloss).  Fully open hand at reset, key angle ~ U(key_init_range); Random
# also moves the key body by U(-0.01, 0.01)^3 from its compiled position at every reset (BatchedMyoEnv.body_pos)
REGISTRY["myoHandKeyTurnFixed-v0"] = dict(
    model="myohand_keyturn", task="keyturn", max_episode_steps=200, frame_skip=10, normalize_act=True, goal_th=3.14, key_init_range=(0.0, 0.0),
    weights=dict(key_turn=1.0, IFtip_approach=10.0, THtip_approach=10.0, act_reg=1.0, bonus=4.0, penalty=25.0))
REGISTRY["myoHandKeyTurnRandom-v0"] = dict(REGISTRY["myoHandKeyTurnFixed-v0"], goal_th=2 * np.pi, key_init_range=(-np.pi / 2, np.pi / 2))
# myoHandPenTwirl{Fixed,Random}-v0 (envs/myo/myobase/__init__.py:616-635, pen_v0.py): MyoHand + a free-standing pen (TrackEnv class: its
# condim-4 pairs).  Palm-up open hand at reset (init_qpos[:-6] = 0, init_qpos[0] = -1.5), pen at qpos0; Random also turns the world-welded
# target by euler2quat(U(-1, 1), U(-1, 1), 0) at every reset (BatchedMyoEnv.body_quat)
REGISTRY["myoHandPenTwirlFixed-v0"] = dict(
    model="myohand_pen", task="pen", max_episode_steps=50, frame_skip=5, normalize_act=True, target_euler_range=None,
    weights=dict(pos_align=1.0, rot_align=1.0, act_reg=5.0, drop=5.0, bonus=10.0))
REGISTRY["myoHandPenTwirlRandom-v0"] = dict(REGISTRY["myoHandPenTwirlFixed-v0"], target_euler_range=((-1.0, -1.0, 0.0), (1.0, 1.0, 0.0)))
# myoChallengeBaodingP1-v1 (envs/myo/myochallenge/__init__.py:355-370, baoding_v1.py): MyoHand + two free balls (TrackEnv class: the balls'
# condim-4 pairs).  Palm-up open hand at reset (init_qpos[:-14] = 0, init_qpos[0] = -1.57), balls at qpos0; the two targets circle the palm
# (goal parameters per env: start angle, direction sign, x / y radius, period, re-drawn at every reset; BatchedMyoEnv.goal_params)
REGISTRY["myoChallengeBaodingP1-v1"] = dict(
    model="myohand_baoding", task="baoding", max_episode_steps=200, frame_skip=10, normalize_act=True, task_choice="fixed",
    goal_time_period=(5, 5), goal_xrange=(0.025, 0.025), goal_yrange=(0.028, 0.028), drop_th=1.25, proximity_th=0.015,
    weights=dict(pos_dist_1=5.0, pos_dist_2=5.0))
# myoChallengeDieReorient{Demo,P1}-v0 (envs/myo/myochallenge/__init__.py:308-335, reorient_v0.py): MyoHand + a die on 3 slides + 3 hinges
# (TrackEnv class: the die's boxes alone).  Palm-up open hand at reset (init_qpos[:-7] = 0, init_qpos[0] = -1.5), die at qpos0; the
# world-welded target is moved by U(goal_pos)^3 from its compiled position and turned to euler2quat(U(goal_rot)^3) at every reset
# (BatchedMyoEnv.goal_offset / body_quat).  The die's mass "re-draw" U(0.108, 0.108) is the compiled mass
REGISTRY["myoChallengeDieReorientDemo-v0"] = dict(
    model="myohand_die", task="die", max_episode_steps=150, frame_skip=5, normalize_act=True, goal_pos=(0.0, 0.0), goal_rot=(-0.785, 0.785),
    pos_th=np.inf, rot_th=0.262, drop_th=0.200,
    weights=dict(pos_dist=100.0, rot_dist=1.0, bonus=0.0, act_reg=0.0, penalty=0.0))
REGISTRY["myoChallengeDieReorientP1-v0"] = dict(REGISTRY["myoChallengeDieReorientDemo-v0"], goal_pos=(-0.010, 0.010), goal_rot=(-1.57, 1.57), pos_th=0.025)
# muscle-condition variants (register_env_with_variants, envs/myo/myobase/__init__.py:14-48): myoSarc* (sarcopenia), myoFati* (fatigue)
# for every myo* id, myoReaf* (EIP -> EPL tendon transfer) for the myoHand* ids
for _id in [k for k in list(REGISTRY) if k.startswith("myo")]:
    REGISTRY[_id[:3] + "Sarc" + _id[3:]] = dict(REGISTRY[_id], muscle_condition="sarcopenia")
    REGISTRY[_id[:3] + "Fati" + _id[3:]] = dict(REGISTRY[_id], muscle_condition="fatigue")
    if _id.startswith("myoHand"):
        REGISTRY[_id[:3] + "Reaf" + _id[3:]] = dict(REGISTRY[_id], muscle_condition="reafferentation")
# MyoDM (envs/myo/myodm/__init__.py:565-700), served by the MJX flavour of the env (mjx/myodm_v0.py TrackEnv -> track.TrackEnv, one fused
# launch per env step) for the objects that have a compiled asset: MyoHand<Object>Fixed-v0 (a one-row reference), MyoHand<Object>Random-v0 (the
# two-row randomisation range, also mjx/myodm_v0.py's module-level default) and the motion-tracking ids, whose motion file is the reference's
# data/<motion>.npz: pass `reference=<path or dict>` or point MYODM_DATA at a directory holding it (the files are not redistributed here).
# The id tables are data: assets/myodm_tasks.json = the reference's OBJECTS tuple and MyoHand_task_spec entries (tools/make_myodm_registry.py);
# an object is registered when its compiled asset assets/myohand_object_<name>.myob[.gz] is present (tools/compile_models.py: all 50).
def _myodm_tables():
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")
    with open(os.path.join(here, "myodm_tasks.json")) as f:
        t = json.load(f)
    have = [o for o in t["objects"] if os.path.exists(os.path.join(here, f"myohand_object_{o}.myob")) or os.path.exists(os.path.join(here, f"myohand_object_{o}.myob.gz"))]
    return tuple(have), [tuple(x) for x in t["tasks"] if x[1] in have]


MYODM_OBJECTS, _MYODM_TASKS = _myodm_tables()
_DOF_ROBOT = 29
for _obj in MYODM_OBJECTS:
    REGISTRY[f"MyoHand{_obj.title()}Fixed-v0"] = dict(task="track", object=_obj, max_episode_steps=50, reference=dict(
        time=np.array([0.0, 4.0]), robot=np.zeros((1, _DOF_ROBOT)), robot_vel=np.zeros((1, _DOF_ROBOT)),
        object_init=np.array([-0.2, -0.2, 0.1, 1.0, 0.0, 0.0, 0.0]), object=np.array([[0.2, 0.2, 0.1, 1.0, 0.0, 0.0, 0.1]])))
    REGISTRY[f"MyoHand{_obj.title()}Random-v0"] = dict(task="track", object=_obj, max_episode_steps=50, reference=dict(
        time=np.array([0.0, 4.0]), robot=np.zeros((2, _DOF_ROBOT)), robot_vel=np.zeros((2, _DOF_ROBOT)),
        object_init=np.array([0.0, 0.0, 0.1, 1.0, 0.0, 0.0, 0.0]),
        object=np.array([[-0.2, -0.2, 0.1, 1.0, 0.0, 0.0, -1.0], [0.2, 0.2, 0.1, 1.0, 0.0, 0.0, 1.0]])))
for _id, _obj, _motion in _MYODM_TASKS:      # MyoHand_task_spec (envs/myo/myodm/__init__.py:25-560): 89 motion-tracking ids
    REGISTRY[_id] = dict(task="track", object=_obj, max_episode_steps=75, motion=_motion)

# registered by the reference but not runnable on the HIP path (DESIGN.md "out of scope")
UNSUPPORTED = {
    # (nothing of the walk family: the terrain envs run on the height-field instantiation of the leg kernel)
    "myoElbowPose1D6MExoRandom-v0": "re-draws the mass of body carry_weight per episode (a per-env model edit)",
}
# myoChallengeBaodingP2-v1 (envs/myo/myochallenge/__init__.py:372-389) and its muscle-condition variants (the challenge registry has no Reaf one)
for _id in ("myoChallengeBaodingP2-v1", "myoSarcChallengeBaodingP2-v1", "myoFatiChallengeBaodingP2-v1"):
    UNSUPPORTED[_id] = ("re-draws the balls' size, mass and friction per episode (obj_size_range, obj_mass_range, obj_friction_change): "
                        "the TrackEnv-class step kernel has no per-env ball size, mass or friction")
# The registered numbers of the two P2 ids as (P1 id, make kwargs the P1 id honours, set_object_randomization kwargs): data only.  The ids
# themselves still raise (above): what runs a P2 configuration is
#     env = make(p1_id, num_envs, **make_kwargs); env.set_object_randomization(**randomization); env.reset()
P2_CONFIGS = {
    "myoChallengeBaodingP2-v1": ("myoChallengeBaodingP1-v1",
                                 dict(task_choice="random", goal_time_period=(4, 6), goal_xrange=(0.020, 0.030), goal_yrange=(0.022, 0.032)),
                                 dict(obj_size_range=(0.018, 0.024), obj_mass_range=(0.030, 0.300), obj_friction_change=(0.2, 0.001, 0.00002))),
    "myoChallengeDieReorientP2-v0": ("myoChallengeDieReorientP1-v0",
                                     dict(goal_pos=(-0.020, 0.020), goal_rot=(-3.14, 3.14)),
                                     dict(obj_size_change=0.007, obj_mass_range=(0.050, 0.250), obj_friction_change=(0.2, 0.001, 0.00002))),
}
# myoChallengeDieReorientP2-v0 (envs/myo/myochallenge/__init__.py:336-353) and its muscle-condition variants
for _id in ("myoChallengeDieReorientP2-v0", "myoSarcChallengeDieReorientP2-v0", "myoFatiChallengeDieReorientP2-v0"):
    UNSUPPORTED[_id] = ("re-draws the die's size, mass and friction per episode (obj_size_change, obj_mass_range, obj_friction_change): "
                        "the TrackEnv-class step kernel has no per-env die size, mass or friction")


class Box:
    """Minimal stand-in for gym.spaces.Box (gym is not a dependency of the stepper)."""

    def __init__(self, low, high, shape, dtype=np.float32):
        self.low = np.full(shape, low, dtype)
        self.high = np.full(shape, high, dtype)
        self.shape = tuple(shape)
        self.dtype = dtype

    def sample(self, rng=None):
        rng = rng or np.random.default_rng()
        return rng.uniform(self.low, self.high).astype(self.dtype)


def _field_property(name, field, width, task=None, doc=None):
    """Property of a per-env field [num_envs, width] (width None: one column per body): get = `view(field)`; set broadcasts one row or takes
    [num_envs, width], into the torch view or (as_torch=False) through a host write.  `task`: the only task that has the field."""
    def check(self):
        if task is not None and self.spec["task"] != task:
            raise AttributeError(f"{name}: {task} task only")

    def fget(self):
        check(self)
        return self.view(field)

    def fset(self, value):
        check(self)
        if self.as_torch:
            self.view(field).copy_(self._torch.as_tensor(value, dtype=self._torch.float32).expand(self.num_envs, -1))
        else:
            self.batch.write(field, np.broadcast_to(np.asarray(value, np.float32), (self.num_envs, width or self.mjmodel.nbody)))
    return property(fget, fset, doc=doc)


class BatchedMyoEnv(capi.FieldViews):
    """`num_envs` copies of one MyoSuite task, stepped together on one MI355X.

    step(action[B, nu] in [-1, 1]) -> (obs[B, obs_dim] f32, reward[B], terminated[B] bool, truncated[B] bool, info)
    following envs/env_base.py:335-365.  Finished episodes (done, or max_episode_steps like gym's TimeLimit)
    are reset in place and the returned obs row is the first observation of the new episode.

    rwd_dict=True (implied by weighted_reward_keys={key: weight}, rwd_mode="sparse" or episode_stats=True) adds the reference's reward
    dictionary to info (env_base.py:559-570): info["rwd_dict"][key] for key in `rwd_keys`, info["rwd_dense"], info["rwd_sparse"]; the
    weights re-weight or drop terms (None: the registered ones), rwd_mode picks the column step() returns.  episode_stats=True adds
    info["episode"] = {"finished", "r", "r_sparse", "l", "solved"}: the statistics of each env's last finished episode, which the in-place
    reset would otherwise wipe.  With the defaults nothing is allocated and no launch is added.

    obs_dict=True (implied by obs_keys=[...] or proprio_keys=[...]) adds the reference's observation dictionary: `obs_dict` /
    info["obs_dict"] = {key: [B, width]} for every key of the task's get_obs_dict (`observations.OBS_TERMS`), and reset() / step() return
    the concatenation of `obs_keys` instead of the canonical row (None: the class's DEFAULT_OBS_KEYS, i.e. the canonical row; `act` is
    appended for a model with muscles as base_v0.py:34-38 does), so `obs_dim` is that selection's width and a policy trains on it with no
    further change; `canonical_obs` stays the registered row.  proprio_keys adds get_proprioception() and info["proprio_dict"].  All of
    them describe the observation step() returns: with `autoreset`, an env that was just reset shows its first observation and
    obs_dict["time"] is 0 there -- unlike rwd_dict, which describes the transition just made.  One small launch per observation pass
    fills them; with the defaults nothing is allocated and no launch is added.
    """

    # env kwargs of the reference that gym.make forwards to the env class and that are honoured here (others raise): the task records' tables
    ENV_KWARGS = tasks.ENV_KWARGS
    POSE_KWARGS = tasks.TASKS["pose"].kwargs
    KEYTURN_KWARGS = tasks.TASKS["keyturn"].kwargs
    _target_jnt_range = staticmethod(tasks.target_jnt_range)

    def __init__(self, env_id, num_envs=1, device=0, seed=0, env_offset=0, autoreset=True, as_torch=True, sensors=False,
                 rwd_dict=False, weighted_reward_keys=None, rwd_mode="dense", episode_stats=False, obs_keys=None, proprio_keys=None,
                 obs_dict=False, **env_kwargs):
        if env_id in UNSUPPORTED:
            raise NotImplementedError(f"{env_id}: {UNSUPPORTED[env_id]}")
        if env_id not in REGISTRY:
            raise KeyError(f"unknown env id {env_id!r}; known: {sorted(REGISTRY)}")
        self.id = env_id
        self.spec = spec = dict(REGISTRY[env_id])
        tasks.filter_kwargs(env_id, spec, env_kwargs)
        # reward terms: any of the four parameters turns the term row on (rewards.resolve: KeyError / ValueError before anything is loaded)
        self._rwd = rewards.resolve(env_id, spec, rwd_dict, weighted_reward_keys, rwd_mode, episode_stats)
        self.rwd_dict, self.episode_stats, self.rwd_mode = self._rwd is not None, bool(episode_stats), rwd_mode
        # observation terms: any of the three parameters turns the rows on (observations.resolve: KeyError / ValueError before anything is loaded)
        self._obs_sel = observations.resolve(env_id, spec, obs_keys, proprio_keys, obs_dict)
        self.num_envs, self.device, self.seed, self.autoreset, self.as_torch = int(num_envs), device, int(seed), autoreset, as_torch
        self.mjmodel = m = _model.load_asset(spec["model"])
        self.muscle_condition = spec.get("muscle_condition", "")
        if self.muscle_condition == "sarcopenia":                      # base_v0.py:64-68: a model edit
            self.mjmodel = m = m.with_sarcopenia()
        self.model = capi.HipModel(m.blob(), device)                   # raises if there is no GPU / no library
        self.batch = capi.HipBatch(self.model, self.num_envs)
        self.batch.set_env_offset(env_offset)
        self.sensors = bool(sensors)
        if self.sensors:       # touch sensors / contact forces of the leg models; nothing is allocated without it
            _enable_sensors(env_id, self.batch)
        self.frame_skip, self.max_episode_steps = spec["frame_skip"], spec["max_episode_steps"]
        self.dt = m.timestep * self.frame_skip                        # env_base.py:616-617
        s = tasks.TASKS[spec["task"]].setup(m, spec, env_id)           # host arithmetic only; the calls it asks for follow
        getattr(self.batch, s.call)(**s.kwargs)
        for name, args in s.then:
            getattr(self.batch, name)(*args)
        if s.body_mass_range is not None:
            self.set_body_mass_range(*s.body_mass_range)
        if self.rwd_dict:      # nothing is allocated and no launch is added without it
            keys, w, mode = self._rwd
            assert self.batch.rwd_names() == keys, (self.batch.rwd_names(), keys)
            self.batch.enable_rewards(w, capi.RWD_SPARSE if mode == "sparse" else capi.RWD_DENSE)
            if self.episode_stats:
                self.batch.enable_episode_stats()
        self._setup_obs_terms(m, spec)
        self._obs_in_step = s.call == "configure_walk"                 # the walk task's observation / reward pass is fused into the step kernel
        self._set_condition(m, spec)
        self.act_dim = m.nu
        self.action_space = Box(-1.0, 1.0, (m.nu,))                    # env_base.py:101-113 (normalize_act)
        self.observation_space = Box(-10.0, 10.0, (self.obs_dim,))     # env_base.py:172-176
        self._episode_seed = self.seed
        self._views = {}
        self._action_buf = self._torch = None
        if as_torch:
            import torch
            self._torch = torch
            self._action_buf = torch.empty((self.num_envs, m.nu), dtype=torch.float32, device=f"cuda:{device}")

    def _setup_obs_terms(self, m, spec):
        """obs_keys / proprio_keys / obs_dim of this env, and with any of the three parameters given the library's rows.  The canonical row
        (MYO_F_OBS) is the concatenation of the default keys, so its width is the sum of theirs (tests/test_obs_terms_host.py holds that sum
        to the library's row record for every registered id)."""
        task, d = spec["task"], observations.dims(m, spec)
        self._obs_width = width = observations.widths(task, d)
        default = observations.default_keys(task, d["na"])
        self.canonical_obs_dim = sum(width[k] for k in default)
        sel = self._obs_sel
        self.obs_keys = list(default if sel is None or sel.obs_keys is None else observations.with_act(task, sel.obs_keys, d["na"]))
        self.proprio_keys = None if sel is None or sel.proprio_keys is None else list(sel.proprio_keys)
        for k in self.obs_keys + (self.proprio_keys or []):
            if width[k] <= 0:
                raise KeyError(f"{self.id}: the model has no obs_dict term {k!r} (no muscles)")
        self.obs_dim = sum(width[k] for k in self.obs_keys)
        self._obs_views = None
        if sel is None:         # nothing is allocated and no launch is added without the parameters
            return
        names = list(width)
        assert self.batch.obs_terms() == tuple(width.items()), (self.batch.obs_terms(), width)
        self.batch.enable_obs_terms([names.index(k) for k in self.obs_keys], [names.index(k) for k in self.proprio_keys or []])

    def _set_condition(self, m, spec):
        """The action map of the id's muscle condition and the library calls that go with it (base_v0.py:64-80, 100-109)."""
        self.actmap = capi.ACTMAP_MUSCLE_SIGMOID
        if self.muscle_condition == "fatigue":                         # base_v0.py:70-74, 100-104
            self.actmap = capi.ACTMAP_SIGMOID_FATIGUE
            self.batch.set_condition(self.frame_skip)
            if spec.get("fatigue_reset_random"):                       # base_v0.py:30-31, 120-127 -> fatigue.py:114-134
                if spec.get("fatigue_reset_vec") is not None:
                    raise AssertionError("Cannot use 'fatigue_reset_vec' if fatigue_reset_random=False.")   # the reference's own (oddly worded) assertion
                self.batch.set_fatigue_reset(1)
            elif spec.get("fatigue_reset_vec") is not None:
                vec = np.asarray(spec["fatigue_reset_vec"], np.float32)
                if len(vec) != m.n_muscle:
                    raise AssertionError(f"Invalid length of initial/reset fatigue vector (expected {m.n_muscle}, but obtained {len(vec)}).")
                full = np.zeros(m.nu, np.float32)
                full[np.asarray(m.actuator_kind) == 0] = vec
                self.batch.set_fatigue_reset(2, full)
        elif self.muscle_condition == "reafferentation":               # base_v0.py:76-80, 105-109
            self.actmap = capi.ACTMAP_SIGMOID_REAFFERENTATION
            self.batch.set_condition(self.frame_skip, m.name2id("actuator", "EPL"), m.name2id("actuator", "EIP"))

    # -- per-env fields: body masses (MYO_F_BODYMASS), root-body offset (MYO_F_BODYPOS), body orientation (MYO_F_BODYQUAT), goal (MYO_F_TARGET) --
    body_mass = _field_property("body_mass", capi.F_BODYMASS, None, doc=
        """[num_envs, nbody] mass of every body in every env: a torch view of the library's buffer (no copy; writes take effect at the
        next step) -- the batched `sim.model.body_mass[bid] = ...`.  First use starts the per-env body-mass override, which steps the model
        on the run-time-sizes kernel of its class.  With as_torch=False: a numpy copy (assign the property to write it back).""")

    def set_body_mass_range(self, body, lo, hi):
        """Re-draw the mass of `body` (id or name) ~ U(lo, hi) at every reset of every env (PoseEnvV0 weight_bodyname / weight_range);
        lo == hi: no re-draw.  Ranges of the other bodies are left as they are."""
        b = self.mjmodel.body_name2id(body) if isinstance(body, str) else int(body)
        r = self.batch.read(capi.F_BODYMASS_RANGE)
        r[:, b], r[:, self.mjmodel.nbody + b] = float(lo), float(hi)
        self.batch.write(capi.F_BODYMASS_RANGE, r)

    body_pos = _field_property("body_pos", capi.F_BODYPOS, 3, doc=
        """[num_envs, 3] offset of the key body from its compiled position in every env (the batched `sim.model.body_pos[-1] = ...` of
        KeyTurnEnvV0.reset, as an offset): a torch view of the library's buffer (no copy; writes take effect at the next step / observation).
        TrackEnv-class models whose last joint sits on a root body only.  With as_torch=False: a numpy copy (assign the property to write it).""")
    body_quat = _field_property("body_quat", capi.F_BODYQUAT, 4, doc=
        """[num_envs, 4] body_quat (w x y z) of the pen / die task's target in every env (the batched `sim.model.body_quat[target] = ...` of
        PenTwirlRandomEnvV0.reset / ReorientEnvV0.reset): a torch view of the library's buffer (no copy; writes take effect at the next step / observation).
        With as_torch=False: a numpy copy (assign the property to write it).""")
    goal_params = _field_property("goal_params", capi.F_TARGET, 5, task="baoding", doc=
        """[num_envs, 5] goal parameters of the baoding task in every env: start angle, direction sign (0 hold, -1 CW, +1 CCW), x radius, y
        radius, period (BaodingEnvV1's ball_1_starting_angle, which_task, x_radius, y_radius, time_period).  A torch view of the library's
        buffer (no copy; writes move the targets from the next observation on, until the env's next reset re-draws them).  With
        as_torch=False: a numpy copy (assign the property to write it).""")
    goal_offset = _field_property("goal_offset", capi.F_TARGET, 3, task="die", doc=
        """[num_envs, 3] offset of the die task's target from its compiled position in every env (the batched `sim.model.body_pos[target]
        = goal_init_pos + ...` of ReorientEnvV0.reset, as an offset); its orientation is `body_quat`.  A torch view of the library's buffer
        (no copy; writes move the goal from the next observation on, until the env's next reset re-draws it).  With as_torch=False: a
        numpy copy (assign the property to write it).""")

    # -- per-env object parameters (include/myo_hip_objects.h, objects.py): size / position / friction of geoms, mass of bodies --------------
    def enable_object_params(self, geoms=(), bodies=()):
        """Select the geoms and bodies (names or ids; up to 16 and 4) whose size / position / friction and mass become per-env values, and
        return the ObjectParams.  TrackEnv-class models only; everything else raises capi.MyoError with the library's reason.  The baoding
        and die tasks need no call: `object_params` selects their objects by itself."""
        if getattr(self, "_objects", None) is None:
            self._objects = objects.ObjectParams(self.batch, self.mjmodel, list(geoms), list(bodies), self._torch, self.device)
        elif (geoms or bodies) and (self._objects.geom_ids, self._objects.body_ids) != objects.resolve_ids(self.mjmodel, geoms, bodies):
            raise ValueError("object parameters are already enabled with another selection")
        return self._objects

    @property
    def object_params(self):
        """The ObjectParams of this env: `.size` / `.pos` / `.friction` [num_envs, ng, 3] and `.mass` [num_envs, nb] of the task's objects,
        torch views of the library's device memory (writes take effect at the next step / forward); with as_torch=False numpy copies,
        written back by assignment.  The first access enables the subsystem: baoding -- the geoms and bodies of ball1 and ball2; die -- the
        15 geoms and the body of `Object`; any other TrackEnv-class task after `enable_object_params(geoms=..., bodies=...)`."""
        if getattr(self, "_objects", None) is None:
            sel = objects.task_objects(self.mjmodel, self.spec["task"])
            if sel is None:
                raise AttributeError(f"{self.id}: no default objects for the {self.spec['task']} task; call enable_object_params(geoms=[...], bodies=[...]) first")
            self.enable_object_params(*sel)
        return self._objects

    def set_object_randomization(self, **kw):
        """Re-draw the objects' parameters at every reset of an env, with the reference's names and meaning: baoding -- obj_size_range,
        obj_mass_range, obj_friction_change (baoding_v1.py:115-135, 360-385); die -- obj_size_change, obj_mass_range, obj_friction_change
        (reorient_v0.py:94-101, 221-247; its visual `target_dice` geom collides with nothing and is not modelled).  Arguments left out are
        not re-drawn; no argument switches the draws off.  ValueError on lo > hi or a negative value, before any library call.  The draws
        happen in the reset kernel: call reset() to start the first randomised episode."""
        task = self.spec["task"]
        sel = objects.task_objects(self.mjmodel, task)
        table = objects.task_draws(self.mjmodel, task, *(sel or ((), ())), **kw)      # (raises before the subsystem is touched)
        if not kw and getattr(self, "_objects", None) is None:                        # nothing to switch off: the subsystem stays off
            return None
        self.object_params.set_draws(table if kw else None)
        self._object_draws = table if kw else None
        return table

    # -- touch sensors and contact forces (make(..., sensors=True)) ---------------------------------------
    def _need_sensors(self):
        if not self.sensors:
            raise AttributeError(f"{self.id}: made without sensors=True")

    @property
    def sensor_names(self):
        """Names of the model's sensors, in the column order of `sensordata`."""
        return list(self.mjmodel.names.get("sensor", []))

    @property
    def sensordata(self):
        """[num_envs, nsensor] touch sensors after the last step (`sim.data.sensordata` of every env): a torch view of the library's
        buffer (no copy).  The forces of the last substep's solve; zeros for an env that was just reset.  With as_torch=False: a numpy copy."""
        self._need_sensors()
        return self.view(capi.F_SENSORDATA)

    @property
    def contact_force(self):
        """[num_envs, nsensor + 1, 3] world force of the contacts each touch sensor counts, and in the last row the force of all contacts
        against world-fixed geoms (the ground reaction force).  A torch view (no copy); with as_torch=False a numpy copy."""
        self._need_sensors()
        v = self.view(capi.F_CFRC)
        return v.view(self.num_envs, -1, 3) if self.as_torch else v.reshape(self.num_envs, -1, 3)

    # -- reward terms and episode statistics (make(..., rwd_dict=True / weighted_reward_keys= / rwd_mode= / episode_stats=True)) ---------
    @property
    def rwd_keys(self):
        """Column names of the task's reward-term row, in the order of the reference's rwd_dict, `dense` last."""
        return rewards.RWD_KEYS[self.spec["task"]]

    @property
    def rwd_weights(self):
        """{key: weight} of the columns `dense` sums (the others have weight 0)."""
        if not self.rwd_dict:
            raise AttributeError(f"{self.id}: made without rwd_dict=True")
        return {k: float(w) for k, w in zip(self.rwd_keys, self._rwd[1]) if w != 0}

    @property
    def rwd_terms(self):
        """[num_envs, len(rwd_keys)] term row of the last step: a torch view of the library's buffer (no copy); as_torch=False: a numpy copy."""
        if not self.rwd_dict:
            raise AttributeError(f"{self.id}: made without rwd_dict=True")
        return self.view(None, "rwd")

    @property
    def episode_count(self):
        """[num_envs] int32 episodes ended so far per env (episode_stats=True)."""
        if not self.episode_stats:
            raise AttributeError(f"{self.id}: made without episode_stats=True")
        return self.view(capi.EP_COUNT, "episode")

    def _reward_info(self, info):
        """info["rwd_dict"] / ["rwd_dense"] / ["rwd_sparse"] (env_base.py:559-570) from the term row: one column view per key."""
        row = self.rwd_terms
        info["rwd_dict"] = {k: row[:, i] for i, k in enumerate(self.rwd_keys)}
        info["rwd_dense"], info["rwd_sparse"] = info["rwd_dict"]["dense"], info["rwd_dict"]["sparse"]

    def _episode_info(self, info):
        """info["episode"]: which envs' episodes the step ended and the statistics of each env's last finished episode."""
        last, fin = self.view(capi.EP_LAST, "episode"), self.view(capi.EP_FINISHED, "episode")
        i32 = (lambda x: x.to(self._torch.int32)) if self._torch is not None else (lambda x: x.astype(np.int32))
        info["episode"] = {"finished": fin > 0, "r": last[:, 0], "r_sparse": last[:, 1], "l": i32(last[:, 2]), "solved": i32(last[:, 3])}

    # -- observation terms (make(..., obs_dict=True / obs_keys=[...] / proprio_keys=[...])) ------------------------------------------------
    @property
    def canonical_obs(self):
        """[num_envs, canonical_obs_dim] the registered row of the id (MYO_F_OBS), whatever `obs_keys` selects."""
        return self.view(capi.F_OBS)

    @property
    def obs_slices(self):
        """{key: slice} of each of `obs_keys` in the row reset() / step() return."""
        return observations.slices(self.obs_keys, self._obs_width)

    def obsvec2obsdict(self, obs):
        """{key: obs[..., its columns]} of a row (or a stack of rows) [..., obs_dim] by `obs_keys`: slicing only, numpy or torch."""
        return observations.obsvec2obsdict(obs, self.obs_keys, self._obs_width)

    @property
    def obs_dict(self):
        """{key: [num_envs, width]} for every key of the task's get_obs_dict, of the observation last returned: column views of the
        library's term row (no copy); as_torch=False: slices of one numpy copy."""
        if self._obs_sel is None:
            raise AttributeError(f"{self.id}: made without obs_dict=True")
        if self._obs_views is not None:
            return self._obs_views
        row, sl = self.view(capi.OBS_TERMS, "obs"), observations.slices(self._obs_width, self._obs_width)
        out = {k: row[:, s] for k, s in sl.items() if s.stop > s.start}
        if self.as_torch:       # views of one buffer: they stay current
            self._obs_views = out
        return out

    def _proprio_dict(self, obs_dict):
        return {"time": obs_dict["time"], **{k: obs_dict[k] for k in self.proprio_keys}}

    def get_proprioception(self):
        """(time, vec, dict) of env_base.py:512-531: vec [num_envs, proprio width] is the concatenation of `proprio_keys` (a view of the
        library's row), dict = {"time": ..., key: ...}.  None when the env was made without proprio_keys."""
        if self.proprio_keys is None:
            return None
        d = self._proprio_dict(self.obs_dict)
        return d["time"], self.view(capi.OBS_PROPRIO, "obs"), d

    def _returned_obs(self, info=None):
        if self._obs_sel is None:
            return self.view(capi.F_OBS)
        if info is not None:
            info["obs_dict"] = od = self.obs_dict
            if self.proprio_keys is not None:
                info["proprio_dict"] = self._proprio_dict(od)
        return self.view(capi.OBS_SELECTED, "obs")

    # -- gym API -------------------------------------------------------------------------------------------
    def reset(self, seed=None):
        if seed is not None:
            self._episode_seed = int(seed)
        s = self._stream()
        self.batch.reset(None, self._episode_seed, s)
        if self.episode_stats:
            self.batch.episode_clear(s)
        self.batch.obs(s)
        return self._returned_obs()

    def step(self, action):
        s = self._stream()
        if self.as_torch:
            a = self._torch.as_tensor(action, dtype=self._torch.float32, device=self._action_buf.device)
            a = self._torch.clamp(a, -1.0, 1.0, out=self._action_buf)      # env_base.py:341 (clip to action space)
            self.batch.step(a.data_ptr(), self.actmap, self.frame_skip, s)
        else:
            a = np.clip(np.ascontiguousarray(action, np.float32).reshape(self.num_envs, self.act_dim), -1, 1)
            # host actions are uploaded into the library's action buffer; the action map runs in the step kernel either way
            self.batch.write(capi.F_ACTION, a)
            self.batch.step(self.batch.field_ptr(capi.F_ACTION)[0], self.actmap, self.frame_skip, s)
        if not self._obs_in_step:
            self.batch.obs(s)
        reward = self.view(capi.F_REWARD)[:, 0]
        if self.as_torch:          # (a view: the auto-reset's observation pass writes the row again)
            reward = reward.clone()
        done = self.view(capi.F_DONE)[:, 0] > 0
        truncated = (self.view(capi.F_ELAPSED)[:, 0] >= self.max_episode_steps) & ~done
        solved = self.view(capi.F_SOLVED)[:, 0] > 0
        info = {"solved": solved}
        if self.rwd_dict:
            self._reward_info(info)
        if self.episode_stats:     # after the observation pass, before the auto-reset clears done / elapsed
            self.batch.episode_update(self.max_episode_steps, s)
            self._episode_info(info)
        if self.autoreset:
            self.batch.autoreset(self.max_episode_steps, self._episode_seed, s)
            self.batch.obs_reset_only(s)
        info["time"] = self.view(capi.F_TIME)
        return self._returned_obs(info), reward, done, truncated, info

    # -- state access (env_base.py:643-705 get_env_state / set_env_state) ----------------------------------
    def get_env_state(self):
        return {k: self.batch.read(f) for k, f in (("qpos", capi.F_QPOS), ("qvel", capi.F_QVEL), ("act", capi.F_ACT),
                                                   ("time", capi.F_TIME), ("target", capi.F_TARGET))}

    def set_env_state(self, state):
        for k, f in (("qpos", capi.F_QPOS), ("qvel", capi.F_QVEL), ("act", capi.F_ACT), ("time", capi.F_TIME), ("target", capi.F_TARGET)):
            if k in state:
                self.batch.write(f, state[k])

    def status(self):
        """Per-env int32 flag bits since the last call (capi.FLAG_*); bad states were reset like mj_sim_scene.py:56-61."""
        return self.batch.status()


def _enable_sensors(env_id, batch):
    """sensors=True: turn the readout on, or say why this id's model cannot provide it (the library's own message)."""
    try:
        batch.enable_sensors()
    except capi.MyoError as e:
        raise NotImplementedError(f"{env_id}: sensors=True is not available: {e}") from None


def _make_track(env_id, num_envs, reference=None, flavour="mjx", sensors=False, rwd_dict=False, episode_stats=False, obs_keys=None,
                proprio_keys=None, obs_dict=False, **kw):
    if obs_keys is not None or proprio_keys is not None or obs_dict:
        raise NotImplementedError(f"{env_id}: obs_keys / proprio_keys / obs_dict are not offered for the MyoDM ids; their observation is the "
                                  "TrackEnv row (qpos, qvel and, in the classic flavour, the tracking errors and act) as one vector")
    if rwd_dict or episode_stats:
        raise NotImplementedError(f"{env_id}: rwd_dict / episode_stats are not offered for the MyoDM ids; their reward terms (pose, object, bonus, "
                                  'penalty) are info["metrics"] of every step')
    if flavour not in ("mjx", "classic"):
        raise ValueError(f"{env_id}: flavour must be 'mjx' (mjx/myodm_v0.py, the default) or 'classic' (envs/myo/myodm/myodm_v0.py), got {flavour!r}")
    reference = _myodm_reference(env_id, reference)
    kw.setdefault("max_episode_steps", REGISTRY[env_id]["max_episode_steps"])
    if flavour == "classic":
        env = track.ClassicTrackEnv(num_envs=num_envs, object_name=REGISTRY[env_id]["object"], reference=reference, **kw)
    else:
        env = track.TrackEnv(num_envs=num_envs, object_name=REGISTRY[env_id]["object"], reference=reference, gym_api=True, **kw)
    env.id = env_id
    if sensors:
        _enable_sensors(env_id, env.batch)
    return env


def _myodm_reference(env_id, reference=None):
    """The reference of a MyoDM id: `reference` if given, the registered one of the Fixed / Random ids, else the id's motion file."""
    import os
    spec = REGISTRY[env_id]
    if reference is None:
        reference = spec.get("reference")
    if reference is None:                      # a motion-tracking id: the reference's own motion file
        roots = [os.environ.get("MYODM_DATA"), "/root/reference/myosuite/envs/myo/myodm/data"]
        hits = [os.path.join(r, spec["motion"]) for r in roots if r and os.path.exists(os.path.join(r, spec["motion"]))]
        if not hits:
            raise FileNotFoundError(f"{env_id}: motion file {spec['motion']} not found; pass reference=<path or dict> or set MYODM_DATA to the "
                                    "directory of the reference's envs/myo/myodm/data")
        reference = hits[0]
    return reference


def myodm_spec(env_id, flavour="mjx", reference=None):
    """What make(env_id, flavour=...) builds for a MyoDM id, worked out on the host (no GPU): frame_skip, obs_dim, act_dim, init_qpos,
    max_episode_steps (the TimeLimit) and the reference type.  init_qpos = qpos0 with [:robot_dim] = robot_init, the object position from
    object_init[:3] and its three hinges from quat2euler(object_init[3:]) (envs/myo/myodm/myodm_v0.py:168-179, mjx/myodm_v0.py:144-150)."""
    if flavour not in ("mjx", "classic"):
        raise ValueError(f"{env_id}: flavour must be 'mjx' or 'classic', got {flavour!r}")
    spec = REGISTRY[env_id]
    if spec.get("task") != "track":
        raise KeyError(f"{env_id} is not a MyoDM id")
    m = _model.load_asset(f"myohand_object_{spec['object']}")
    ref = track.ReferenceMotion(_myodm_reference(env_id, reference))
    obs_dim = track.classic_obs_dim(m, ref) if flavour == "classic" else m.nq + m.nv
    return dict(frame_skip=10 if flavour == "classic" else 5, obs_dim=obs_dim, act_dim=m.nu, init_qpos=track.myodm_init_qpos(m, ref),
                max_episode_steps=spec["max_episode_steps"], ref_type=ref.type)


def make(env_id, num_envs=1, **kw):
    """gym.make counterpart for the batched envs (envs/myo/myobase/__init__.py and envs/myo/myodm/__init__.py register the same ids).
    The MyoDM ids take `flavour`: "mjx" (default, mjx/myodm_v0.py TrackEnv -> track.TrackEnv) or "classic" (the registered entry point,
    envs/myo/myodm/myodm_v0.py TrackEnv -> track.ClassicTrackEnv)."""
    if env_id in REGISTRY and REGISTRY[env_id].get("task") == "track":
        return _make_track(env_id, num_envs, **kw)
    return BatchedMyoEnv(env_id, num_envs=num_envs, **kw)
