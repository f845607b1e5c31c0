#!/usr/bin/env python3
"""Record what `envs.make` sends to the binding layer, without a GPU (tests/test_env_setup_host.py, tests/golden/env_setup_calls.json.gz).

    python tools/record_env_setup.py tests/golden/env_setup_calls.json.gz

`capi.HipModel` / `capi.HipBatch` are replaced by stand-ins that log every call in order with canonical arguments (floats as float.hex,
arrays as dtype + shape + bytes, the model blob as a digest); `read(F_BODYMASS_RANGE)` answers zeros, every other method None.  Every
case of CASES is built with as_torch=False, num_envs=3, seed=5, env_offset=7 (the MyoDM ids, which take none of the first and last:
num_envs=3, seed=5) and stored as its calls + the env's public attributes, or as the type of the exception it raised.  The golden
file is written from the commit BEFORE a change of the env layer and compared byte for byte after it."""
import contextlib
import gzip
import hashlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASE = dict(as_torch=False, num_envs=3, seed=5, env_offset=7)
TRACK_BASE = dict(num_envs=3, seed=5)
ATTRS = ("obs_dim", "act_dim", "actmap", "frame_skip", "dt", "max_episode_steps", "spec", "init_qpos")


def canon(x):
    if isinstance(x, np.ndarray):
        return ["nd", str(x.dtype), list(x.shape), x.tobytes().hex()]
    if isinstance(x, (bool, np.bool_, int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    if isinstance(x, (list, tuple)):
        return [canon(a) for a in x]
    if isinstance(x, dict):
        return {str(k): canon(v) for k, v in sorted(x.items())}
    if isinstance(x, bytes):
        return "sha256:" + hashlib.sha256(x).hexdigest()[:16]
    if x is None or isinstance(x, str):
        return x
    if isinstance(x, (FakeModel, FakeBatch)):
        return type(x).__name__
    raise TypeError(f"record_env_setup: no canonical form for {type(x)}")


LOG = []


class FakeModel:
    def __init__(self, blob, device=0):
        from myosuite_mjx_amd import blob as _blob
        LOG.append(["HipModel", canon(blob), canon(device)])
        self.nbody = int(_blob.unpack(blob)["sizes"][4])
        self.dims = types.SimpleNamespace(nbody=self.nbody)
        self.device = device


class FakeBatch:
    def __init__(self, model, B):
        LOG.append(["HipBatch", canon(B)])
        self.model, self.B = model, B

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **k):
            LOG.append([name, canon(a), canon(k)])
            from myosuite_mjx_amd import capi
            if name == "read" and a == (capi.F_BODYMASS_RANGE,):
                return np.zeros((self.B, 2 * self.model.nbody), np.float32)
        return call


@contextlib.contextmanager
def stand_ins():
    """capi.HipModel / capi.HipBatch -> the recorders; `torch` -> an empty module unless it is already imported (TrackEnv.__init__ imports
    it and touches nothing of it)."""
    from myosuite_mjx_amd import capi
    saved = capi.HipModel, capi.HipBatch
    stub = "torch" not in sys.modules
    capi.HipModel, capi.HipBatch = FakeModel, FakeBatch
    if stub:
        sys.modules["torch"] = types.ModuleType("torch")
    try:
        yield
    finally:
        capi.HipModel, capi.HipBatch = saved
        if stub:
            del sys.modules["torch"]


def cases():
    """[(case name, env id, kwargs)]: every non-track id plain, the kwarg cases, the MyoDM cases, the error cases."""
    from myosuite_mjx_amd import envs
    R = envs.REGISTRY
    out = [(i, i, {}) for i in sorted(R) if R[i].get("task") != "track"]
    bao, die, pen, key = "myoChallengeBaodingP1-v1", "myoChallengeDieReorientP1-v0", "myoHandPenTwirlFixed-v0", "myoHandKeyTurnFixed-v0"
    exo = "myoElbowPose1D6MExoFixed-v0"
    kw = [
        ("exo_random", exo, dict(weight_bodyname="carry_weight", weight_range=(0.1, 2.0), target_jnt_range={"r_elbow_flex": (0, 2.27)})),
        ("walk_reset_random", "myoLegWalk-v0", dict(reset_type="random")),
        ("walk_sensors", "myoLegWalk-v0", dict(sensors=True)),
        ("terrain_reset_random", "myoLegHillyTerrainWalk-v0", dict(reset_type="random")),
        ("pose_reset_init", "myoHandPoseRandom-v0", dict(reset_type="init")),
        ("fati_reset_random", "myoFatiHandPoseRandom-v0", dict(fatigue_reset_random=True)),
        ("fati_reset_vec", "myoFatiElbowPose1D6MRandom-v0", dict(fatigue_reset_vec=[0.1, 0.2, 0.3, 0.4, 0.5, 0.6])),
        ("fati_reset_vec_exo", "myoFatiElbowPose1D6MExoFixed-v0", dict(fatigue_reset_vec=np.linspace(0.0, 0.5, 6))),
        ("fatigue_kwargs_without_fatigue", "myoHandPoseFixed-v0", dict(fatigue_reset_random=True)),
        ("keyturn_overrides", key, dict(goal_th=1.5, key_init_range=(-0.5, 1.0))),
        ("keyturn_random_fixed_range", "myoHandKeyTurnRandom-v0", dict(key_init_range=(0.25, 0.25))),
        ("baoding_random", bao, dict(task_choice="random", goal_time_period=(4, 6), goal_xrange=(0.020, 0.030), goal_yrange=(0.022, 0.032),
                                     drop_th=1.0, proximity_th=0.02)),
        ("baoding_refused_none", bao, dict(obj_size_range=None, obj_mass_range=None, obj_friction_change=None)),
        ("die_overrides", die, dict(goal_pos=(-0.02, 0.015), goal_rot=(-1.0, 0.5), pos_th=0.05, rot_th=0.3, drop_th=0.15)),
        ("die_refused_none", die, dict(obj_size_change=None, obj_mass_range=None, obj_friction_change=None)),
        ("sarc_die_overrides", "myoSarcChallengeDieReorientDemo-v0", dict(goal_rot=(0.0, 0.0), pos_th=0.01)),
    ]
    for i in ("MyoHandAirplaneFixed-v0", "MyoHandAirplaneRandom-v0"):
        for fl in ("mjx", "classic"):
            kw.append((f"{i}/{fl}", i, dict(flavour=fl)))
    kw.append(("MyoHandCupFixed-v0/mjx/sensors_limit", "MyoHandCupFixed-v0", dict(flavour="mjx", sensors=True, max_episode_steps=20)))
    err = [("unknown_id", "myoNoSuchEnv-v0", {}), ("track_bad_flavour", "MyoHandAirplaneFixed-v0", dict(flavour="jax")),
           ("unknown_kwarg", "myoHandPoseFixed-v0", dict(weight_bodyname_typo="x")), ("unknown_kwarg_walk", "myoLegWalk-v0", dict(min_height=0.5))]
    err += [(f"unsupported/{i}", i, {}) for i in sorted(envs.UNSUPPORTED)]
    others = dict(pose="myoHandPoseFixed-v0", reach="myoHandReachFixed-v0", hold="myoHandObjHoldFixed-v0", walk="myoLegWalk-v0",
                  stand="myoLegStandRandom-v0", keyturn=key, pen=pen, baoding=bao, die=die)
    values = dict(weight_bodyname="carry_weight", weight_range=(0.1, 2.0), target_jnt_range={}, goal_th=1.0, key_init_range=(0, 1),
                  task_choice="random", goal_time_period=(4, 6), goal_xrange=(0.02, 0.03), goal_yrange=(0.02, 0.03), drop_th=0.1, proximity_th=0.02,
                  goal_pos=(0.0, 0.0), goal_rot=(0.0, 0.0), pos_th=0.02, rot_th=0.2)
    owners = dict(weight_bodyname=("pose",), weight_range=("pose",), target_jnt_range=("pose",), goal_th=("keyturn",), key_init_range=("keyturn",),
                  task_choice=("baoding",), goal_time_period=("baoding",), goal_xrange=("baoding",), goal_yrange=("baoding",),
                  drop_th=("baoding", "die"), proximity_th=("baoding",), goal_pos=("die",), goal_rot=("die",), pos_th=("die",), rot_th=("die",))
    for k, v in values.items():                 # every task kwarg on an id of every task that does not take it
        err += [(f"foreign/{k}/{t}", i, {k: v}) for t, i in others.items() if t not in owners[k]]
    for k in ("obj_size_range", "obj_mass_range", "obj_friction_change", "obj_size_change"):
        err += [(f"refused/{k}/{t}", others[t], {k: (0.1, 0.2)}) for t in ("baoding", "die", "pose", "pen")]
        err.append((f"refused_none/{k}/pen", pen, {k: None}))
    err += [
        ("key_init_range_order", key, dict(key_init_range=(1.0, 0.0))),
        ("task_choice_bad", bao, dict(task_choice="nope")),
        ("goal_time_period_zero", bao, dict(goal_time_period=(0, 5))),
        ("goal_time_period_order", bao, dict(goal_time_period=(6, 4))),
        ("goal_xrange_order", bao, dict(goal_xrange=(0.03, 0.02))),
        ("goal_yrange_order", bao, dict(goal_yrange=(0.03, 0.02))),
        ("goal_pos_order", die, dict(goal_pos=(0.01, -0.01))),
        ("goal_rot_order", die, dict(goal_rot=(1.0, -1.0))),
        ("walk_reset_type_bad", "myoLegWalk-v0", dict(reset_type="nope")),
        ("weight_bodyname_without_range", exo, dict(weight_bodyname="carry_weight")),
        ("weight_bodyname_unknown_body", exo, dict(weight_bodyname="no_such_body", weight_range=(0.1, 2.0))),
        ("target_jnt_range_wrong_joint", exo, dict(target_jnt_range={"nope": (0, 1)})),
        ("target_jnt_range_extra_joint", exo, dict(target_jnt_range={"r_elbow_flex": (0, 1), "nope": (0, 1)})),
        ("fatigue_random_and_vec", "myoFatiHandPoseRandom-v0", dict(fatigue_reset_random=True, fatigue_reset_vec=[0.0] * 39)),
        ("fatigue_vec_length", "myoFatiHandPoseRandom-v0", dict(fatigue_reset_vec=[0.0] * 5)),
    ]
    return out + kw + err


def run_case(env_id, kwargs):
    """One case under the stand-ins: dict(calls, attrs, mjmodel[, myodm_spec]) or dict(error=<exception type name>)."""
    from myosuite_mjx_amd import envs
    track = envs.REGISTRY.get(env_id, {}).get("task") == "track"
    del LOG[:]
    try:
        e = envs.make(env_id, **dict(TRACK_BASE if track else BASE, **kwargs))
    except Exception as ex:                     # the type, and only that
        return dict(error=type(ex).__name__)
    out = dict(calls=list(LOG), attrs={a: canon(getattr(e, a, None)) for a in ATTRS}, mjmodel=canon(e.mjmodel.blob()))
    if track:
        out["myodm_spec"] = canon(envs.myodm_spec(env_id, kwargs.get("flavour", "mjx")))
    return out


def record():
    with stand_ins():
        return {name: run_case(env_id, kwargs) for name, env_id, kwargs in cases()}


def main():
    rec = record()
    text = json.dumps(rec, sort_keys=True, separators=(",", ":")) + "\n"
    with open(sys.argv[1], "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:      # (no time stamp: same record, same file)
        g.write(text.encode())
    kinds = sorted({c[0] for r in rec.values() for c in r.get("calls", ())})
    print(f"{len(rec)} cases ({sum('error' in r for r in rec.values())} errors) -> {sys.argv[1]}; calls seen: {kinds}")


if __name__ == "__main__":
    main()
