"""CPU tests for myoHandPenTwirl{Fixed,Random}-v0 (envs/myo/myobase/pen_v0.py): registry entries, the committed myohand_pen fixture and
its TrackEnv-class lowering with the plane - cylinder pair, Model.with_body_quat, the float64 restatement of the
task's formulas (tests/pen_ref.py) on oracle states, its euler2quat against the reference's, and oracle states reaching one to four
plane - cylinder contacts."""
import os

import numpy as np
import pytest

import hand_task_checks as H
from hand_task_checks import ROOT
from pen_ref import euler2quat, pen_restate
from pen_states import branch_states

IDS = ("myoHandPenTwirlFixed-v0", "myoHandPenTwirlRandom-v0")
SITES = ("object_top", "object_bottom", "target_top", "target_bottom", "eps_ball")


@pytest.fixture(scope="module")
def pen():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_pen")


def test_registry_entries_and_variants():
    from myosuite_mjx_amd import envs
    f, r = (envs.REGISTRY[i] for i in IDS)
    assert f["model"] == r["model"] == "myohand_pen" and f["task"] == r["task"] == "pen"
    assert f["max_episode_steps"] == r["max_episode_steps"] == 50 and f["frame_skip"] == r["frame_skip"] == 5 and f["normalize_act"]
    assert f["weights"] == dict(pos_align=1.0, rot_align=1.0, act_reg=5.0, drop=5.0, bonus=10.0)
    assert f["target_euler_range"] is None and r["target_euler_range"] == ((-1.0, -1.0, 0.0), (1.0, 1.0, 0.0))
    ids = [i[:3] + c + i[3:] for i in IDS for c in ("Sarc", "Fati", "Reaf")]
    for v in ids:
        assert envs.REGISTRY[v]["task"] == "pen" and v not in envs.UNSUPPORTED
    assert len(set(ids) | set(IDS)) == 8
    for i in IDS:
        H.muscle_variants(i, H.CONDITIONS)


def test_fixture_is_trk_class_with_plane_cylinder_pair(pen):
    from myosuite_mjx_amd import model as M
    m = pen
    assert M.asset_stem("myohand_pen") == os.path.join(M.GOLDEN_DIR, "myohand_pen")
    assert (m.nq, m.nv, m.nu) == (29, 29, 39) and m.n_muscle == 39 and len(m.hip_cg_geom) == 31
    assert "hip_unsupported" not in m.arrays and list(m.hip_trk) == [1, 0, 0]     # condim-4 pairs only
    pi = np.asarray(m.hip_pair_i).reshape(-1, 6)
    cg = np.asarray(m.hip_cg_geom)
    assert len(pi) == 346                                                          # 345 pairs, the plane - cylinder one as two records
    pen_g = [g for g in range(m.ngeom) if m.geom_bodyid[g] == m.name2id("body", "Object")]
    tgt_g = [g for g in range(m.ngeom) if m.geom_bodyid[g] == m.name2id("body", "target")]
    pc = [(int(cg[p[0]]), int(cg[p[1]]), int(p[4])) for p in pi if p[4] in (6, 7)]
    assert pc == [(0, pen_g[0], 6), (0, pen_g[0], 7)] and int(m.geom_type[0]) == 0 and int(m.geom_type[pen_g[0]]) == 5
    # the target (world-welded, no joints) keeps every pair: they must hold in any per-env orientation
    assert sum(1 for p in pi if int(cg[p[0]]) in tgt_g or int(cg[p[1]]) in tgt_g) == 27
    assert m.body_jntnum[m.name2id("body", "target")] == 0 and m.body_parentid[m.name2id("body", "target")] == 0


def test_plane_cylinder_refused_outside_trk_class(pen):
    """Lowering keeps refusing plane - cylinder pairs of models outside the TrackEnv class."""
    from myosuite_mjx_amd.lowering import lower
    from myosuite_mjx_amd.mjcf import CompiledModel
    a = {k: np.array(v, copy=True) for k, v in pen.arrays.items() if not k.startswith("hip_")}
    a["geom_condim"] = np.where(a["geom_condim"] > 3, 3, a["geom_condim"])
    with pytest.raises(NotImplementedError, match="outside the TrackEnv"):
        lower(CompiledModel(arrays=a, names=pen.names))


def test_with_body_quat(pen):
    from oracle.oracle import Oracle
    m = pen
    tb = m.name2id("body", "target")
    q = euler2quat([0.4, -0.7, 0.0])
    mm = m.with_body_quat("target", q)
    assert np.allclose(mm.body_quat[tb], q) and np.array_equal(m.body_quat, pen.body_quat)
    changed = sorted(k for k in m.arrays if not np.array_equal(m.arrays[k], mm.arrays[k]))
    assert "body_quat" in changed and all(k == "body_quat" or k.startswith("hip_") for k in changed)
    o = Oracle(mm.blob())
    o.reset()
    o.forward()
    x = o.field("site_xpos").reshape(-1, 3)
    top, bot = x[m.name2id("site", "target_top")], x[m.name2id("site", "target_bottom")]
    Rz = np.array([2 * (q[1] * q[3] + q[0] * q[2]), 2 * (q[2] * q[3] - q[0] * q[1]), q[0] ** 2 - q[1] ** 2 - q[2] ** 2 + q[3] ** 2])
    assert np.allclose((top - bot) / 0.13, Rz) and np.allclose((top + bot) / 2, m.body_pos[tb])
    # the lowered static frames follow: the target site in the HIP tables
    s = m.name2id("site", "target_top")
    assert np.allclose(np.asarray(mm.hip_site_lpos).reshape(-1, 3)[s] + mm.hip_origin, top)
    with pytest.raises(NotImplementedError):
        m.with_body_quat("Object", [1, 0, 0, 0])                 # the pen has joints
    with pytest.raises(ValueError):
        m.with_body_quat("target", [1, 1, 0, 0])


def test_euler2quat_matches_reference():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_quat_math.npz"))
    assert np.abs(euler2quat(g["euler"]) - g["euler2quat"]).max() < 1e-12


def _oracle_obs_inputs(o, m):
    sites = H.site_xpos(o, m, SITES)
    xp = o.field("xpos").reshape(-1, 3)[m.name2id("body", "Object")]
    return sites, xp


def test_restatement_on_oracle_states(pen):
    from oracle.oracle import Oracle
    m = pen
    o = Oracle(m.blob())
    q = np.array(m.qpos0, float)
    q[:-6] = 0
    q[0] = -1.5
    sites, xp = _oracle_obs_inputs(H.forward_at(o, q), m)
    assert np.allclose(xp, m.body_pos[m.name2id("body", "Object")]) and np.allclose(sites[12:], xp)     # eps_ball = the pen's start
    rng = np.random.default_rng(0)
    act, v = rng.uniform(0, 1, (1, 39)), rng.normal(0, 1, (1, 29))
    obs, rew, done, solved = pen_restate(q, v, act, sites, xp, 0.01)
    assert obs.shape == (1, 83)
    assert np.array_equal(obs[0, :23], q[:23]) and np.allclose(obs[0, 23:26], xp) and np.allclose(obs[0, 26:32], v[0, 23:] * 0.01)
    rot, drot = obs[0, 32:35], obs[0, 35:38]
    assert np.isclose(np.linalg.norm(rot), 1) and np.isclose(np.linalg.norm(drot), 1)
    assert np.allclose(obs[0, 38:41], 0) and np.allclose(obs[0, 41:44], rot - drot) and np.array_equal(obs[0, 44:], act[0])
    ra = rot @ drot
    assert not done[0] and solved[0] == (ra > 0.95)
    assert rew[0] == pytest.approx(ra - 5 * np.linalg.norm(act) / 39 + 10 * ((ra > 0.9) + 5 * (ra > 0.95)))
    # the pen turned onto the target's axis: solved; moved 8 cm away: dropped (done, not solved, no bonus)
    ob = m.name2id("body", "Object")
    th0 = 2 * np.arctan2(m.body_quat[ob][2], m.body_quat[ob][0])
    for dq, d_exp, s_exp in (((0, 0, 0, 0, -th0, 0), False, True), ((0.08, 0, 0, 0, -th0, 0), True, False)):
        qq = q.copy()
        qq[-6:] = dq
        sites, xp = _oracle_obs_inputs(H.forward_at(o, qq), m)
        obs, rew, done, solved = pen_restate(qq, np.zeros((1, 29)), np.zeros((1, 39)), sites, xp, 0.01)
        assert done[0] == d_exp and solved[0] == s_exp
        pa = np.linalg.norm(obs[0, 38:41])
        assert rew[0] == pytest.approx(-pa + 1.0 - 5.0 * d_exp + (0 if d_exp else 60.0))


def test_oracle_reaches_every_plane_cylinder_branch(pen):
    from oracle.oracle import Oracle
    m = pen
    pg = [g for g in range(m.ngeom) if m.geom_bodyid[g] == m.name2id("body", "Object")][0]
    o = Oracle(m.blob())
    for name, q, n in branch_states(m):
        cs = [c for c in H.forward_at(o, q).contacts() if {int(c[7]), int(c[8])} == {0, pg}]
        assert len(cs) == n, (name, len(cs))
