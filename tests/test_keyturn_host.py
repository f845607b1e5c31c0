"""CPU tests for myoHandKeyTurn{Fixed,Random}-v0 (envs/myo/myobase/key_turn_v0.py): registry entries and kwargs, the committed
myohand_keyturn asset and its TrackEnv-class lowering, the float64 restatement of the task's formulas
(tests/keyturn_ref.py) on oracle states, and Model.with_body_pos.  (The ABI ids are pinned in tests/test_capi_host.py, the lowered tables
of every committed asset in tests/test_compile_bytes.py.)"""
import os

import numpy as np
import pytest

import hand_task_checks as H
from keyturn_ref import keyturn_restate

IDS = ("myoHandKeyTurnFixed-v0", "myoHandKeyTurnRandom-v0")
SITES = ("keyhead", "IFtip", "THtip")


@pytest.fixture(scope="module")
def key():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_keyturn")


def test_registry_entries_and_variants():
    from myosuite_mjx_amd import envs
    f, r = (envs.REGISTRY[i] for i in IDS)
    assert f["model"] == r["model"] == "myohand_keyturn" and f["task"] == r["task"] == "keyturn"
    assert f["max_episode_steps"] == r["max_episode_steps"] == 200 and f["frame_skip"] == r["frame_skip"] == 10
    assert f["goal_th"] == 3.14 and tuple(f["key_init_range"]) == (0.0, 0.0)
    assert r["goal_th"] == 2 * np.pi and tuple(r["key_init_range"]) == (-np.pi / 2, np.pi / 2)
    assert f["weights"] == dict(key_turn=1.0, IFtip_approach=10.0, THtip_approach=10.0, act_reg=1.0, bonus=4.0, penalty=25.0)
    for i in IDS:
        for v in H.muscle_variants(i, H.CONDITIONS):
            assert v["task"] == "keyturn" and v["goal_th"] == envs.REGISTRY[i]["goal_th"]


def test_kwargs_are_key_turn_only():
    from myosuite_mjx_amd import envs
    assert set(envs.BatchedMyoEnv.KEYTURN_KWARGS) <= set(envs.BatchedMyoEnv.ENV_KWARGS)
    for other in ("myoHandPoseFixed-v0", "myoHandReachFixed-v0", "myoHandObjHoldFixed-v0"):
        for kw in (dict(goal_th=1.0), dict(key_init_range=(0, 1))):
            with pytest.raises(TypeError, match="key-turn task only"):      # refused before any GPU work
                envs.BatchedMyoEnv(other, num_envs=1, **kw)
    with pytest.raises(TypeError):
        envs.BatchedMyoEnv(IDS[0], num_envs=1, weight_bodyname="key")   # the pose kwargs stay pose-only


def test_asset_loads_and_is_trk_class(key):
    from myosuite_mjx_amd import model as M
    assert M.asset_stem("myohand_keyturn") == os.path.join(M.GOLDEN_DIR, "myohand_keyturn")    # a data fixture under tests/golden/
    assert M.asset_stem("myohand_pose") == os.path.join(M.ASSET_DIR, "myohand_pose")
    m = key
    assert (m.nq, m.nv, m.nu, m.ngeom) == (24, 24, 39, 62) and m.n_muscle == 39 and m.timestep == pytest.approx(0.002)
    assert "hip_unsupported" not in m.arrays
    assert list(m.hip_trk) == [0, 1, 1]                          # friction loss and a box, no condim-4 pair
    kj = m.name2id("joint", "keyjoint")
    assert kj == m.njnt - 1 and m.hip_fl[kj, 0] == pytest.approx(0.02) and m.dof_damping[kj] == pytest.approx(0.1)
    kb = m.jnt_bodyid[kj]
    assert m.names["body"][kb] == "key" and m.body_parentid[kb] == 0
    link = int(m.hip_body_link[kb])
    assert m.hip_link_parent[link] < 0 and int(m.hip_link_dofnum[link]) == 1
    types = sorted(int(m.geom_type[g]) for g in range(m.ngeom) if m.geom_bodyid[g] == kb)
    assert types == [3, 4, 6]                                    # capsule shaft, ellipsoid head, box bit
    assert any(int(m.geom_type[g]) == 6 for g in m.hip_cg_geom)
    # the key head site sits at the key body's origin: key_init_pos (key_turn_v0.py:66) is the body position
    s = m.name2id("site", "keyhead")
    assert m.site_bodyid[s] == kb and not np.asarray(m.hip_site_lpos[s]).any()


def test_restatement_on_oracle_states(key):
    """The restatement of key_turn_v0.py's formulas on oracle states: obs layout, the thresholds of bonus / penalty / done / solved."""
    from oracle.oracle import Oracle
    m = key
    o = Oracle(m.blob())
    rng = np.random.default_rng(0)
    q0 = np.zeros(m.nq)
    sites = H.site_xpos(H.forward_at(o, q0), m, SITES)
    assert np.allclose(sites[:3], m.body_pos[m.name2id("body", "key")])     # key head = key body origin
    act = rng.uniform(0, 1, (1, 39))
    qvel = rng.normal(0, 1, (1, 24))
    obs, rew, done, solved = keyturn_restate(q0, qvel, act, sites, 0.02, 3.14)
    assert obs.shape == (1, 93)
    assert np.array_equal(obs[0, 46:48], [0.0, qvel[0, 23] * 0.02]) and np.allclose(obs[0, 23:46], qvel[0, :23] * 0.02)
    assert np.allclose(obs[0, 48:51], sites[:3] - sites[3:6]) and np.allclose(obs[0, 51:54], sites[:3] - sites[6:9])
    assert np.array_equal(obs[0, 54:], act[0])
    d_if = abs(np.linalg.norm(sites[:3] - sites[3:6]) - 0.03)
    d_th = abs(np.linalg.norm(sites[:3] - sites[6:9]) - 0.03)
    pen = -float(d_if > 0.05) - float(d_th > 0.05)
    assert rew[0] == pytest.approx(-10 * d_if - 10 * d_th - np.linalg.norm(act) / 39 + 25 * pen)
    assert done[0] == (d_if > 0.1 or d_th > 0.1) and not solved[0]
    # key angle past pi/2, pi and goal_th: the bonus steps and `solved` (the key's hinge does not move the tips)
    for kq, bonus, sol_fixed, sol_random in ((1.0, 0, False, False), (2.0, 1, False, False), (3.145, 2, True, False), (6.5, 2, True, True)):
        q = q0.copy()
        q[-1] = kq
        s = H.site_xpos(H.forward_at(o, q), m, SITES)
        assert np.allclose(s[3:], sites[3:]) and np.allclose(s[:3], sites[:3])
        _, r, _, sf = keyturn_restate(q, np.zeros((1, 24)), np.zeros((1, 39)), s, 0.02, 3.14)
        _, _, _, sr = keyturn_restate(q, np.zeros((1, 24)), np.zeros((1, 39)), s, 0.02, 2 * np.pi)
        assert r[0] == pytest.approx(kq - 10 * d_if - 10 * d_th + 4 * bonus + 25 * pen) and sf[0] == sol_fixed and sr[0] == sol_random
    # a flexed index finger brings its tip to the key: approach distance and penalty change with the hand's state
    ds = []
    for f in np.linspace(0, 1, 6):
        q = q0.copy()
        for n in ("mcp2_flexion", "pm2_flexion", "md2_flexion"):
            j = m.name2id("joint", n)
            q[j] = f * m.jnt_range[j, 1]
        s = H.site_xpos(H.forward_at(o, q), m, SITES)
        ds.append(np.linalg.norm(s[:3] - s[3:6]))
    assert np.ptp(ds) > 0.01


def test_with_body_pos(key):
    from oracle.oracle import Oracle
    m = key
    kb = m.name2id("body", "key")
    d = np.array([0.004, -0.007, 0.01])
    mm = m.with_body_pos("key", m.body_pos[kb] + d)
    assert np.allclose(mm.body_pos[kb], m.body_pos[kb] + d) and np.array_equal(m.body_pos, key.body_pos)
    link = int(m.hip_body_link[kb])
    assert np.allclose(mm.hip_link_pos.reshape(-1, 3)[link] - m.hip_link_pos.reshape(-1, 3)[link], d)
    changed = [k for k in m.arrays if not np.array_equal(m.arrays[k], mm.arrays[k])]
    assert sorted(changed) == ["body_pos", "hip_link_pos"]
    o = Oracle(mm.blob())
    o.reset()
    o.forward()
    x = o.field("site_xpos").reshape(-1, 3)
    assert np.allclose(x[m.name2id("site", "keyhead")], m.body_pos[kb] + d)
    with pytest.raises(NotImplementedError):
        m.with_body_pos("distph2", [0, 0, 0])                 # not a root body
    with pytest.raises(ValueError):
        m.with_body_pos("key", [np.nan, 0, 0])
