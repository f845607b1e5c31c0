"""Classic gym flavour of the MyoDM TrackEnv (envs/myo/myodm/myodm_v0.py), host side: the float64 restatement against the reference's own
code (tests/golden/myodm_classic.npz, tools/make_myodm_classic_fixture.py), the env spec of the registered ids, the `flavour` argument
and the C ABI field."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "myodm_classic.npz")
CASES = ("fixed_obj", "fixed_pose", "random_obj", "random_pose", "track_obj", "track_pose", "trackmid_obj", "trackmid_pose")


def _motion():
    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_motion.npz"))
    return {k.split("__in__")[1]: f[k] for k in f.files if k.startswith("track_MyoHand_airplane_fly1__in__")}


def _case_reference(case):
    from myosuite_mjx_amd import envs
    name = case.rsplit("_", 1)[0]
    return {"fixed": envs.REGISTRY["MyoHandAirplaneFixed-v0"]["reference"], "random": envs.REGISTRY["MyoHandAirplaneRandom-v0"]["reference"]}.get(name, None) or _motion()


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(case):
    """get_obs_dict + obsdict2obsvec, get_reward_dict and check_termination of the reference on recorded states: the restatement gives the
    float32 obs vector to 1e-6, every reward term to 1e-9 and the same done.  The reference rows the restatement uses come from the project's
    ReferenceMotion (FIXED / TRACK, equal to what the reference looked up) or, for RANDOM draws, from the fixture."""
    import myodm_classic_ref as R
    from myosuite_mjx_amd import track as T
    g = np.load(GOLD)
    k = lambda s: g[f"{case}__{s}"]
    assert list(k("obs_keys")) == ["qp", "qv", "hand_qpos_err", "hand_qvel_err", "obj_com_err", "act"]
    ref = T.ReferenceMotion(_case_reference(case), motion_extrapolation=True)
    term_pose = case.endswith("_pose")
    n = len(k("time"))
    assert n >= 8
    for i in range(n):
        if ref.type == "RANDOM":
            row = dict(robot=k("ref_robot")[i], robot_vel=k("ref_robot_vel")[i], object=k("ref_object")[i])
            lo, hi = np.asarray(ref.reference["object"][0]), np.asarray(ref.reference["object"][1])
            assert ((row["object"] >= lo) & (row["object"] <= hi)).all()
        else:
            r = ref.get_reference(k("time")[i] + float(k("motion_start_time")))
            row = dict(robot=r["robot"][0], robot_vel=None if r["robot_vel"] is None else r["robot_vel"][0], object=r["object"][0])
            np.testing.assert_allclose(row["robot"], k("ref_robot")[i], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(row["object"], k("ref_object")[i], rtol=1e-12, atol=1e-12)
        obs, rwd, done = R.obs_reward(k("qpos")[i], k("qvel")[i], k("act")[i], row, k("obj_xipos")[i], k("obj_ximat")[i], k("wrist_xipos")[i],
                                      float(k("lift_z")), terminate_pose_fail=term_pose)
        assert obs.shape == k("obs")[i].shape
        np.testing.assert_allclose(obs.astype(np.float32), k("obs")[i], rtol=0, atol=1e-6)      # (obsdict2obsvec rounds to float32)
        for key in ("pose", "object", "bonus", "penalty", "sparse", "solved", "done", "dense"):
            assert abs(rwd[key] - float(k(f"rwd_{key}")[i])) <= 1e-9, (case, i, key, rwd[key], float(k(f"rwd_{key}")[i]))
        assert done == bool(k("terminate")[i])


def test_fixture_covers_interesting_ground():
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) < 1 << 20
    assert any(g[f"{c}__rwd_bonus"].any() for c in CASES)
    term = np.concatenate([g[f"{c}__terminate"] for c in CASES])
    assert term.any() and not term.all()
    assert g["trackmid_obj__motion_start_time"] == 0.01 and g["track_obj__time"].max() > 1.98     # between frames; past the motion's end
    assert g["track_obj__obs"].shape[1] == 142 and g["fixed_obj__obs"].shape[1] == 170 and g["random_obj__obs"].shape[1] == 170


@pytest.mark.parametrize("env_id,case,dim,limit", [("MyoHandAirplaneFixed-v0", "fixed_obj", 170, 50), ("MyoHandAirplaneRandom-v0", "random_obj", 170, 50),
                                                   ("MyoHandAirplaneFly-v0", "track_obj", 142, 75)])
def test_classic_spec_of_the_registered_ids(env_id, case, dim, limit):
    """frame_skip 10, the observation width (robot_vel present: 170; a motion file has none: 142), the TimeLimit of the id and init_qpos
    as the reference's TrackEnv._setup builds it (:168-179, from the fixture)."""
    from myosuite_mjx_amd import envs
    g = np.load(GOLD)
    sp = envs.myodm_spec(env_id, "classic", reference=_motion() if case == "track_obj" else None)
    assert sp["frame_skip"] == 10 and sp["obs_dim"] == dim and sp["max_episode_steps"] == limit and sp["act_dim"] == 45
    np.testing.assert_allclose(sp["init_qpos"], g[f"{case}__init_qpos"], rtol=0, atol=1e-6)
    mjx = envs.myodm_spec(env_id, "mjx", reference=_motion() if case == "track_obj" else None)
    assert mjx["frame_skip"] == 5 and mjx["obs_dim"] == 70 and np.array_equal(mjx["init_qpos"], sp["init_qpos"])


def test_unknown_flavour_is_refused():
    from myosuite_mjx_amd import envs
    for bad in ("gym", "", None, "MJX"):
        with pytest.raises(ValueError):
            envs.make("MyoHandAirplaneFixed-v0", 1, flavour=bad)
        with pytest.raises(ValueError):
            envs.myodm_spec("MyoHandAirplaneFixed-v0", bad)


def test_header_field_compiles_as_c99_and_cxx(tmp_path):
    """myo_track_config.flavour is the last field; the header compiles as C99 and C++ and the ctypes mirror puts it at the same offset."""
    from myosuite_mjx_amd import capi
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "myo_hip.h"\nint main(void) { myo_track_config c = {0}; c.flavour = 1;\n'
                   '  printf("%d %d %d\\n", (int)offsetof(myo_track_config, flavour), (int)offsetof(myo_track_config, seed), (int)sizeof(myo_track_config));\n'
                   '  return c.flavour == 1 ? 0 : 1; }\n')
    inc = os.path.join(ROOT, "include")
    outs = []
    for cc, std, name in (("gcc", "-std=c99", "t_c"), ("g++", "-std=c++17", "t_cxx")):
        exe = tmp_path / name
        args = [cc, std, "-Wall", "-Werror", "-I", inc, "-o", str(exe)] + (["-x", "c++"] if cc == "g++" else []) + [str(src)]
        subprocess.check_call(args)
        outs.append(subprocess.check_output([str(exe)], text=True).split())
    assert outs[0] == outs[1]
    off, seed_off, size = (int(x) for x in outs[0])
    assert off > seed_off
    assert capi.TrackConfig.flavour.offset == off and ctypes.sizeof(capi.TrackConfig) == size
