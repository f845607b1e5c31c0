"""CPU tests of the reward-term rows (rwd_dict / weighted_reward_keys / rwd_mode / episode_stats of the batched envs): the column table
and default weights against the reference's text (tests/golden/reward_terms.json), the constructor parameters' validation without a GPU,
the float64 helper tests/reward_terms_ref.py against the tasks' own *_restate functions on oracle states, the library's copy of the
column table, and the register / scratch figures of the kernels the feature adds or changes."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hand_task_checks as H
import reward_terms_ref as R
from conftest import REFERENCE, ROOT

# an id per task of the fixture (the registered weights of these ids are their class's defaults; ids that override them are left out)
IDS = {"pose": "myoHandPoseRandom-v0", "reach": "myoHandReachRandom-v0", "hold": "myoHandObjHoldRandom-v0", "keyturn": "myoHandKeyTurnRandom-v0",
       "pen": "myoHandPenTwirlRandom-v0", "stand": "myoLegStandRandom-v0", "walk": "myoLegWalk-v0", "terrain": "myoLegRoughTerrainWalk-v0",
       "baoding": "myoChallengeBaodingP1-v1", "die": "myoChallengeDieReorientP1-v0"}
BAND = 1e-5          # the float32 kernels' error on the deciding quantities (tests/test_gpu_reward_terms.py)


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reward_terms.json")))


def test_columns_and_default_weights_equal_the_reference_text(fixture):
    from myosuite_mjx_amd import envs, rewards
    assert sorted(fixture) == sorted(IDS)
    for task, ref in fixture.items():
        spec = envs.REGISTRY[IDS[task]]
        assert list(rewards.RWD_KEYS[spec["task"]]) == ref["keys"], task
        assert ref["keys"][-4:] == ["sparse", "solved", "done", "dense"]
        w = rewards.weight_vector(IDS[task], spec["task"], spec["weights"])
        want = rewards.weight_vector(IDS[task], spec["task"], ref["default_weights"])
        assert w.dtype == np.float32 and len(w) == len(ref["keys"]) - 1 and np.array_equal(w, want), task
    assert fixture["walk"]["default_weights"]["done"] == -100.0           # a weighted column outside the "optional keys"


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="reference tree not present")
def test_fixture_equals_a_fresh_parse(fixture):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_reward_terms_fixture as T
    assert T.parse(REFERENCE) == fixture


def test_library_column_table_equals_the_python_one():
    """Each csrc/myo_task_<name>.h carries its task's names for myo_batch_rwd_name; BatchedMyoEnv asserts they agree when it enables the row."""
    import glob
    from myosuite_mjx_amd import rewards
    src = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "myosuite_mjx_amd", "csrc", "myo_task_*.h"))))
    rows = {n: [x.strip().strip('"') for x in body.replace("RWD_TAIL", ", ".join(f'"{k}"' for k in rewards.TAIL)).split(",")]
            for n, body in re.findall(r"rwd_(\w+)\[\] = \{([^}]*)\}", src)}
    assert sorted(rows) == sorted(set(rewards.RWD_KEYS) - {"stand"})        # reach and stand share one C row
    for task, keys in rewards.RWD_KEYS.items():
        assert rows["reach" if task == "stand" else task] == list(keys), task


def test_parameter_validation_needs_no_gpu():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import envs, rewards
    with pytest.raises(KeyError, match="nope"):
        myo.make("myoHandPoseRandom-v0", num_envs=2, weighted_reward_keys={"nope": 1})
    with pytest.raises(KeyError, match="dense"):                          # dense is the sum, not a term
        myo.make("myoLegWalk-v0", num_envs=2, weighted_reward_keys={"dense": 1})
    with pytest.raises(ValueError, match="rwd_mode"):
        myo.make("myoHandPenTwirlRandom-v0", num_envs=2, rwd_mode="shaped")
    for kw in (dict(rwd_dict=True), dict(episode_stats=True)):
        with pytest.raises(NotImplementedError, match=r'info\["metrics"\]'):
            myo.make("MyoHandAirplaneFixed-v0", num_envs=2, **kw)
    spec = envs.REGISTRY["myoLegWalk-v0"]
    assert rewards.resolve("myoLegWalk-v0", spec) is None                  # the defaults: nothing to enable
    for kw in (dict(rwd_dict=True), dict(weighted_reward_keys={}), dict(rwd_mode="sparse"), dict(episode_stats=True)):
        keys, w, mode = rewards.resolve("myoLegWalk-v0", spec, **kw)
        assert keys == rewards.RWD_KEYS["walk"] and mode == kw.get("rwd_mode", "dense")
    # absent keys weigh 0, any column but dense may be weighted: walk_v0's own defaults weight `done`
    keys, w, _ = rewards.resolve("myoLegWalk-v0", spec, weighted_reward_keys={"vel_reward": 2.0, "done": -7.0, "act_mag": 0.5})
    assert dict(zip(keys, w.tolist())) == dict(vel_reward=2.0, cyclic_hip=0.0, ref_rot=0.0, joint_angle_rew=0.0, act_mag=0.5, sparse=0.0, solved=0.0, done=-7.0)
    # the new parameters are the constructor's own: the pinned env-kwarg tables do not know them
    from myosuite_mjx_amd import tasks
    assert not {"rwd_dict", "weighted_reward_keys", "rwd_mode", "episode_stats"} & set(tasks.ENV_KWARGS)


# ---- the float64 helper against the tasks' own restatements, on oracle states ----------------------------------------------------------

def _load(stem):
    from myosuite_mjx_amd import model as M
    return M.load_asset(stem)


def _keyturn_states():
    from keyturn_ref import WEIGHTS, keyturn_restate
    from oracle.oracle import Oracle
    m = _load("myohand_keyturn")
    o = Oracle(m.blob())
    rng = np.random.default_rng(0)
    lo, hi = np.asarray(m.jnt_range)[:, 0], np.asarray(m.jnt_range)[:, 1]
    q = lo + (hi - lo) * rng.uniform(0, 1, (48, m.nq)) * rng.uniform(0, 1, (48, 1))      # from open hands to fully flexed ones
    q[:, -1] = rng.uniform(-2, 7, 48)                                                     # key angles across pi / 2, pi, both goal_th
    q[0] = 0.0
    act = rng.uniform(0, 1, (48, 39))
    sites = np.stack([H.site_xpos(H.forward_at(o, qq), m, ("keyhead", "IFtip", "THtip")) for qq in q])
    row, margin = R.terms("keyturn", qpos=q, sites=sites, act=act, goal_th=3.14)
    _, dense, done, solved = keyturn_restate(q, np.zeros_like(q), act, sites, 0.02, 3.14)
    return row, margin, WEIGHTS, dense, done, solved


def _pen_states():
    from pen_ref import WEIGHTS, pen_restate
    from pen_states import branch_states
    from oracle.oracle import Oracle
    m = _load("myohand_pen")
    o = Oracle(m.blob())
    rng = np.random.default_rng(1)
    base = np.array(m.qpos0, float)
    base[:-6] = 0
    base[0] = -1.5
    qs = [base] + [q for _, q, _ in branch_states(m)]
    for _ in range(43):                                                                   # the pen moved and turned about its start
        q = base.copy()
        q[-6:-3] += rng.uniform(-0.06, 0.06, 3)
        q[-3:] += rng.uniform(-1.5, 1.5, 3)
        qs.append(q)
    q = np.stack(qs)
    act = rng.uniform(0, 1, (len(q), 39))
    sites, xp = [], []
    for qq in q:
        H.forward_at(o, qq)
        sites.append(H.site_xpos(o, m, ("object_top", "object_bottom", "target_top", "target_bottom", "eps_ball")))
        xp.append(o.field("xpos").reshape(-1, 3)[m.name2id("body", "Object")].copy())
    sites, xp = np.stack(sites), np.stack(xp)
    row, margin = R.terms("pen", sites=sites, obj_pos=xp, act=act)
    _, dense, done, solved = pen_restate(q, np.zeros_like(q), act, sites, xp, 0.01)
    return row, margin, WEIGHTS, dense, done, solved


def _die_states():
    from die_states import rollout_states
    from reorient_ref import SITES, WEIGHTS, reorient_restate, site_frames
    from oracle.oracle import Oracle
    m = _load("myohand_die")
    states = rollout_states(m, steps=40, seeds=(None, 1))                                 # the die drops within 40 steps of the U(-1, 1) episode
    o = Oracle(m.blob())
    sid = [m.name2id("site", n) for n in SITES]
    q, v, act = (np.stack([s[k] for s in states]) for k in range(3))
    x = np.stack([H.forward_at(o, qq).field("site_xpos").reshape(-1, 3)[sid].copy() for qq in q])
    Ro, Rt = site_frames(x)
    w = dict(WEIGHTS, bonus=4.0, act_reg=1.0, penalty=50.0)                               # (the registered weights zero three of the five terms)
    row, margin = R.terms("die", sites=x.reshape(len(q), 24), act=act)
    _, dense, done, solved = reorient_restate(q, v, act, x[:, 0], x[:, 4], Ro, Rt, 0.01, w=w)
    _, dense0, _, _ = reorient_restate(q, v, act, x[:, 0], x[:, 4], Ro, Rt, 0.01)
    assert np.abs(R.dense(row, WEIGHTS) - dense0).max() < 1e-12
    return row, margin, w, dense, done, solved


def _baoding_states():
    """The rollout of tests/test_baoding_host.py::test_restatement_on_oracle_states: palm up, zero control, the targets moved as the
    reference moves them; a ball rolls off near step 33."""
    import test_baoding_host as TB
    from baoding_ref import WEIGHTS, baoding_restate, target_xy
    from oracle.oracle import Oracle
    m = _load("myohand_baoding")
    p = np.array([[np.pi / 4, 1.0, 0.025, 0.028, 5.0]])
    o = Oracle(m.blob())
    o.reset()
    o.set_state(qpos=TB._init_q(m))
    sid = [m.name2id("site", n) for n in TB.SITES]
    q, v, act, x = [], [], [], []
    for k in range(1, 41):
        ok = Oracle(TB._with_target_xy(m, target_xy(p, k)[0]).blob())
        ok.reset()
        ok.set_state(qpos=o.field("qpos"), qvel=o.field("qvel"), act=o.field("act"), ctrl=o.field("ctrl"))
        assert ok.step(10) == 0
        ok.forward()
        q.append(ok.field("qpos").copy()); v.append(ok.field("qvel").copy()); act.append(ok.field("act").copy())
        x.append(ok.field("site_xpos").reshape(-1, 3)[sid].reshape(12).copy())
        o = ok
    q, v, act, x = (np.stack(a) for a in (q, v, act, x))
    row, margin = R.terms("baoding", sites=x, act=act)
    _, dense, done, solved = baoding_restate(q, v, x)
    return row, margin, WEIGHTS, dense, done, solved


@pytest.mark.parametrize("states", (_keyturn_states, _pen_states, _die_states, _baoding_states), ids=lambda f: f.__name__.strip("_"))
def test_helper_equals_the_tasks_own_restatement(states):
    """sum_k w_k t_k of the helper's row = the dense reward of the task's *_restate function to 1e-12, done and solved equal, and the 1e-5
    band around the thresholds leaves out less than 2 % of these states (what the GPU test is allowed to leave out)."""
    row, margin, w, dense, done, solved = states()
    assert set(row) | {"dense"} == set(_keys_of(row)) and np.abs(R.dense(row, w) - dense).max() < 1e-12
    assert np.array_equal(row["done"] > 0, done) and np.array_equal(row["solved"] > 0, solved)
    assert 0 < row["done"].mean() < 1                                                      # both values of done among the states
    assert (margin < BAND).mean() < 0.02, (margin < BAND).mean()


def _keys_of(row):
    from myosuite_mjx_amd import rewards
    return next(k for k in rewards.RWD_KEYS.values() if set(k) == set(row) | {"dense"})


def test_helper_on_the_state_tasks():
    """pose / reach / hold / stand / walk have no *_restate in the tree: the helper's rows against the numbers of their formulas worked out
    by hand, on both sides of every threshold."""
    z = np.zeros((1, 3))
    act = np.array([[0.3, 0.4]])
    row, margin = R.terms("pose", qpos=[[0.0, 0.0]], target=[[0.3, 0.4]], act=act, pose_thd=0.35)
    assert row["pose"][0] == -0.5 and row["bonus"][0] == 1.0 and row["penalty"][0] == 0 and row["act_reg"][0] == -0.25 and row["solved"][0] == 0
    assert margin[0] == pytest.approx(0.025)                                                # 1.5 pose_thd = 0.525
    row, _ = R.terms("pose", qpos=[[0.0, 0.0]], target=[[7.0, 0.0]], act=act, pose_thd=0.35)
    assert row["done"][0] == 1 and row["penalty"][0] == -1
    for t, far in ((0.01, 0.0), (0.1, -1.0)):                                               # far_th counts after two env steps only
        row, _ = R.terms("reach", tips=z, target=z + [0.3, 0, 0], act=act, time=[t], dt=0.02, far_th=0.2, near_th=0.0125)
        assert row["reach"][0] == -0.3 and row["penalty"][0] == far and row["done"][0] == -far and row["sparse"][0] == -0.3
    row, margin = R.terms("hold", obj_pos=z, goal=z + [0, 0.015, 0], act=act, goal_th=0.01, drop_th=0.3)
    assert row["goal_dist"][0] == -0.015 and row["bonus"][0] == 1 and row["solved"][0] == 0 and row["done"][0] == 0 and margin[0] == pytest.approx(0.005)
    row, _ = R.terms("stand", tip=z, target=z + [0.5, 0, 0], qvel=[[3.0, 4.0]], act=act, time=[1.0], dt=0.01, far_th=0.44, near_th=0.05)
    assert row["reach"][0] == pytest.approx(10 - 0.5 - 0.5) and row["act_reg"][0] == -25.0 and row["penalty"][0] == -1 and row["done"][0] == 1
    q = np.zeros((2, 10))
    q[:, 3] = 1.0
    q[1, 3:7] = [np.cos(0.6), np.sin(0.6), 0, 0]                                             # turned about x: r00 stays 1 > max_rot
    q[:, 7], q[:, 8] = -0.8, 0.8                                                             # the hips on the cycle at phase 0
    row, margin = R.terms("walk", com_vel=[[0.0, 1.2]] * 2, height=[0.9, 0.7], feet_heights=[[0.0, 0.1]] * 2, phase=[0.0, 0.0], qpos=q,
                          act=[[1.0, 0, 0, 0]] * 2, qadr_hip_flexion=(7, 8), qadr_joint_angle=(9, 9, 9, 9), target_rot=(1, 0, 0, 0))
    assert np.allclose(row["vel_reward"], 2.0) and np.allclose(row["cyclic_hip"], 0.0, atol=1e-15) and row["ref_rot"][0] == 1.0
    assert row["ref_rot"][1] == pytest.approx(np.exp(-5 * np.hypot(np.cos(0.6) - 1, np.sin(0.6)))) and np.allclose(row["act_mag"], 0.25)
    assert row["done"].tolist() == [1.0, 1.0] and row["solved"].tolist() == [1.0, 1.0]       # |r00| = 1 > 0.8 in both
    row, _ = R.terms("walk", com_vel=[[0.0, 1.2]] * 2, height=[0.9, 0.7], feet_heights=[[0.0, 0.1]] * 2, phase=[0.0, 0.0], qpos=q,
                     act=[[1.0, 0, 0, 0]] * 2, qadr_hip_flexion=(7, 8), qadr_joint_angle=(9, 9, 9, 9), target_rot=(1, 0, 0, 0), max_rot=2.0)
    assert row["done"].tolist() == [0.0, 1.0]                                                # the second is below min_height
    assert R.dense(dict(a=np.array([1.0, 2.0]), b=np.array([3.0, 4.0])), dict(a=2.0, b=-1.0)).tolist() == [-1.0, 0.0]


# ---- the kernels --------------------------------------------------------------------------------------------------------------------

def test_new_and_changed_kernels_have_no_spill_and_no_scratch():
    """The walk term kernel, the episode-statistics kernel and every task observation kernel whose body now writes the term row, read from
    the code object's metadata the way tests/test_kernel_resources.py reads the step kernels."""
    from myosuite_mjx_amd import capi
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    found, bodies = {}, {"task_obs_kernel<": [], "task_post_kernel<": []}
    for r in kernel_resources.resources(capi.LIB_PATH):
        name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
        for key in ("walk_terms_kernel(", "episode_stats_kernel(", "reach_obs_kernel<16>(", "task_obs_kernel<", "task_post_kernel<"):
            if name.startswith(("void " + key, key)) and "myodm_obs_body" not in name:
                found.setdefault(key, []).append(r)
                if key in bodies:     # (a TrackObs body other than myodm's would not match: give it a case of its own here)
                    bodies[key].append(re.match(r"(?:void )?task_\w+_kernel<StateObs<&\(?(\w+)\(", name).group(1))
    assert [len(found[k]) for k in ("walk_terms_kernel(", "episode_stats_kernel(", "reach_obs_kernel<16>(")] == [1, 1, 1], {k: len(v) for k, v in found.items()}
    # one body per task, each in one observation kernel and one fused epilogue; the MJX track row has no epilogue of its own (the step kernel's)
    tasks = ["baoding_obs_body", "die_obs_body", "hold_obs_body", "keyturn_obs_body", "pen_obs_body", "pose_obs_body", "stand_obs_body"]
    assert sorted(bodies["task_obs_kernel<"]) == sorted(tasks + ["mjx_track_obs_body"]), bodies
    assert sorted(bodies["task_post_kernel<"]) == tasks, bodies
    for rs in found.values():
        for r in rs:
            assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 128, r
