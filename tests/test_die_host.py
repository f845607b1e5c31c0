"""CPU tests for myoChallengeDieReorient{Demo,P1}-v0 (envs/myo/myochallenge/reorient_v0.py): registry entries and variants, P2 and its
per-env die kwargs refused, the committed myohand_die fixture and its TrackEnv-class lowering (nothing but the die's boxes puts it there),
the box rule of lowering, the float64 restatement of the task (tests/reorient_ref.py: its mat2euler against the reference's, and on
oracle states), and the oracle rollouts the GPU tests draw their states from."""
import os

import numpy as np
import pytest

import hand_task_checks as H
from die_states import init_qpos, pick_states, rollout_states
from hand_task_checks import ROOT
from reorient_ref import SITES, euler2quat, euler_margin, mat2euler, reorient_restate, site_frames

IDS = ("myoChallengeDieReorientDemo-v0", "myoChallengeDieReorientP1-v0")
P2 = ("myoChallengeDieReorientP2-v0", "myoSarcChallengeDieReorientP2-v0", "myoFatiChallengeDieReorientP2-v0")
DT = 0.01


@pytest.fixture(scope="module")
def die():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_die")


@pytest.fixture(scope="module")
def rollouts(die):
    return rollout_states(die)


def test_registry_entries_and_variants():
    from myosuite_mjx_amd import envs
    d, p = (envs.REGISTRY[i] for i in IDS)
    for s in (d, p):
        assert s["model"] == "myohand_die" and s["task"] == "die" and s["normalize_act"]
        assert s["max_episode_steps"] == 150 and s["frame_skip"] == 5
        assert s["weights"] == dict(pos_dist=100.0, rot_dist=1.0, bonus=0.0, act_reg=0.0, penalty=0.0)
        assert s["rot_th"] == 0.262 and s["drop_th"] == 0.2
    assert d["pos_th"] == np.inf and d["goal_pos"] == (0.0, 0.0) and d["goal_rot"] == (-0.785, 0.785)
    assert p["pos_th"] == 0.025 and p["goal_pos"] == (-0.010, 0.010) and p["goal_rot"] == (-1.57, 1.57)
    for i in IDS:
        H.muscle_variants(i, H.CONDITIONS[:2])                                 # the challenge registry has no Reaf variant
    H.assert_p2_refused(P2)


@pytest.mark.parametrize("kw,val", [("obj_size_change", 0.007), ("obj_mass_range", (0.05, 0.25)), ("obj_friction_change", (0.2, 0.001, 0.00002))])
def test_per_env_die_kwargs_refused(kw, val):
    from myosuite_mjx_amd import envs
    with pytest.raises(NotImplementedError, match="size, mass or friction"):
        envs.make(IDS[1], num_envs=1, **{kw: val})
    for k in ("goal_pos", "goal_rot", "pos_th", "rot_th"):
        with pytest.raises(TypeError, match="die task only"):
            envs.make("myoHandPenTwirlFixed-v0", num_envs=1, **{k: (0.0, 0.0)})   # die kwargs belong to the die; refused before any GPU work
    with pytest.raises(TypeError, match="die task only"):
        envs.make("myoHandPenTwirlFixed-v0", num_envs=1, drop_th=0.1)             # shared by baoding and the die, nobody else


def test_fixture_lowers_to_trk_through_its_boxes_alone(die):
    from myosuite_mjx_amd import model as M
    from myosuite_mjx_amd.mjcf import GEOM_BOX, GEOM_CAPSULE, GEOM_PLANE
    m = die
    assert M.asset_stem("myohand_die") == os.path.join(M.GOLDEN_DIR, "myohand_die")
    assert (m.nq, m.nv, m.nu, m.nbody) == (29, 29, 39, 41) and m.n_muscle == 39
    assert "hip_unsupported" not in m.arrays and list(m.hip_trk) == [0, 0, 1]      # no condim-4 pair, no friction loss: the boxes
    pi = np.asarray(m.hip_pair_i).reshape(-1, 6)
    cg = np.asarray(m.hip_cg_geom)
    assert len(pi) == 694 and set(pi[:, 5].tolist()) == {3} and set(pi[:, 4].tolist()) == {0, 1}
    ob, tb = m.name2id("body", "Object"), m.name2id("body", "target")
    dg = [g for g in range(m.ngeom) if m.geom_bodyid[g] == ob]
    assert sorted(int(m.geom_type[g]) for g in dg) == [GEOM_CAPSULE] * 12 + [GEOM_BOX] * 3
    ty = [(int(m.geom_type[cg[p[0]]]), int(m.geom_type[cg[p[1]]])) for p in pi]
    assert not any(GEOM_PLANE in t for t in ty)                                      # floor pairs pruned: the die's slides are limited
    assert any(GEOM_BOX in t and GEOM_CAPSULE in t for t in ty)
    assert all(p[4] == 0 for p, t in zip(pi, ty) if GEOM_BOX in t)                   # boxes go through the generic MPR type
    # the target: a jointless child of the world without a colliding geom; the die: six trailing scalar dofs, the compiled mass of P1
    assert m.body_jntnum[tb] == 0 and m.body_parentid[tb] == 0
    assert not any(m.geom_bodyid[g] == tb for g in cg)
    assert m.body_parentid[ob] == 0 and m.body_jntnum[ob] == 6 and m.body_mass[ob] == 0.108
    assert np.asarray(m.jnt_range)[-6:-3].tolist() == [[-0.25, 0.25]] * 3 and not np.asarray(m.jnt_limited)[-3:].any()


def test_box_rule_of_lowering():
    """A model whose only TrackEnv-class feature is a box lowers (the key-turn model without its friction loss), and a plane against a
    moving box is still refused."""
    from myosuite_mjx_amd import model as M
    from myosuite_mjx_amd.lowering import lower
    from myosuite_mjx_amd.mjcf import GEOM_BOX, CompiledModel
    key = M.load_asset("myohand_keyturn")
    a = {k: np.array(v, copy=True) for k, v in key.arrays.items() if not k.startswith("hip_")}
    a["dof_frictionloss"][:] = 0
    cm = CompiledModel(arrays=a, names=key.names)
    lower(cm)
    assert list(cm.arrays["hip_trk"]) == [0, 0, 1]
    bd = M.load_asset("myohand_baoding")
    a = {k: np.array(v, copy=True) for k, v in bd.arrays.items() if not k.startswith("hip_")}
    g = bd.name2id("geom", "ball1")
    a["geom_type"][g] = GEOM_BOX
    a["geom_size"][g] = [0.02, 0.02, 0.02]
    with pytest.raises(NotImplementedError, match="cannot prune static geom 0 against moving geom|plane against a moving box"):
        lower(CompiledModel(arrays=a, names=bd.names))                              # the floor plane against a free box


def test_mat2euler_matches_reference():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_quat_math.npz"))
    assert np.abs(mat2euler(g["euler2mat"]) - g["mat2euler"]).max() < 1e-12
    # the second branch (cy = 0): the reference's formula, by hand
    R = np.array([[0.0, -np.sin(0.3), np.cos(0.3)], [0.0, np.cos(0.3), np.sin(0.3)], [-1.0, 0.0, 0.0]]).T
    assert np.hypot(R[2, 2], R[1, 2]) == 0
    assert np.allclose(mat2euler(R), [0.0, -np.arctan2(-R[0, 2], 0.0), -np.arctan2(-R[1, 0], R[1, 1])])


def _frames(o, m):
    x = o.field("site_xpos").reshape(-1, 3)[[m.name2id("site", n) for n in SITES]]
    xm = o.field("xmat").reshape(-1, 3, 3)
    Ro, Rt = xm[m.name2id("body", "Object")], xm[m.name2id("body", "target")]
    fo, ft = site_frames(x[None])
    assert np.abs(fo[0] - Ro).max() < 1e-12 and np.abs(ft[0] - Rt).max() < 1e-12     # the axis sites span the site frames (no site quat)
    return x, Ro, Rt


def test_restatement_on_oracle_states(die):
    from myosuite_mjx_amd.mjcf import quat2mat
    from oracle.oracle import Oracle
    m = die
    tb = m.name2id("body", "target")
    o = Oracle(m.blob())
    o.reset()
    o.forward()
    x, _, _ = _frames(o, m)
    assert np.abs(x[4] - x[0] - [-0.1, 0.0, 0.0]).max() < 1e-15                      # goal_obj_offset, at qpos0
    q = init_qpos(m)
    assert q[22] == 0 and np.array_equal(q[23:], m.qpos0[23:])                       # init_qpos[:-7] = 0 reaches the die's first slide
    x, Ro, Rt = _frames(H.forward_at(o, q), m)
    rng = np.random.default_rng(0)
    act, v = rng.uniform(0, 1, (1, 39)), rng.normal(0, 1, (1, 29))
    obs, rew, done, solved = reorient_restate(q, v, act, x[0], x[4], Ro, Rt, DT)
    assert obs.shape == (1, 63)
    assert np.array_equal(obs[0, :22], q[:22]) and np.allclose(obs[0, 22:45], v[0, :23] * DT)
    assert np.allclose(obs[0, 45:48], x[0]) and np.allclose(obs[0, 48:51], x[4]) and np.abs(obs[0, 51:54]).max() < 1e-15   # pos_err = 0 at reset
    assert np.allclose(obs[0, 54:57], 0) and np.allclose(obs[0, 57:60], 0.001, atol=1e-6) and np.allclose(obs[0, 60:63], obs[0, 57:60] - obs[0, 54:57])
    assert not done[0] and solved[0] and rew[0] == pytest.approx(-np.linalg.norm(obs[0, 60:63]))
    # the Demo id ignores the position: pos_th = inf
    assert reorient_restate(q, v, act, x[0] + [0.1, 0, 0], x[4], Ro, Rt, DT, pos_th=np.inf)[3][0]
    # the die moved 0.21 m away: done, not solved
    qq = q.copy()
    qq[-6] = 0.21
    x, Ro, Rt = _frames(H.forward_at(o, qq), m)
    obs, rew, done, solved = reorient_restate(qq, v, act, x[0], x[4], Ro, Rt, DT)
    assert done[0] and not solved[0] and np.isclose(np.linalg.norm(obs[0, 51:54]), 0.21) and rew[0] == pytest.approx(-21.0 - np.linalg.norm(obs[0, 60:63]))
    # the goal turned and moved (Model.with_body_quat / with_body_pos): the goal sites follow; the die turned onto it within rot_th: solved
    e = np.array([0.5, -0.3, 0.2])
    off = np.array([0.008, -0.006, 0.004])
    mm = m.with_body_quat("target", euler2quat(e)).with_body_pos("target", m.body_pos[tb] + off)
    for dq, s_exp in ((0.0, False), (1.0, True), (0.9, True), (0.5, False)):
        # the die's hinges OBJRx, OBJRy, OBJRz compose Rx Ry Rz, the matrix whose mat2euler is the three angles themselves: the die at
        # the hinge angles e has the target's frame, at 0.9 e it is 0.0616 rad away (solved), at 0.5 e 0.308 rad (rot_th = 0.262)
        ang = e
        qq = q.copy()
        qq[-6:-3] = off
        qq[-3:] = dq * ang
        x, Ro, Rt = _frames(H.forward_at(Oracle(mm.blob()), qq), mm)
        assert np.allclose(x[4], m.body_pos[tb] + off) and np.allclose(Rt, quat2mat(euler2quat(e)))
        obs, rew, done, solved = reorient_restate(qq, v, act, x[0], x[4], Ro, Rt, DT)
        assert np.allclose(obs[0, 57:60], e) and np.abs(obs[0, 51:54]).max() < 1e-12 and not done[0]
        assert solved[0] == s_exp, (dq, obs[0, 54:63])
        assert np.allclose(obs[0, 54:57], dq * e) and np.allclose(obs[0, 60:63], (1 - dq) * e)


def test_oracle_rollouts_stay_inside_the_kernel_limits(die, rollouts):
    """The four episodes the GPU tests draw their states from: contact count far below the kernel's 128, every kind of state and both
    contact types present, the die drops well inside the 150-step limit, and the float64 restatement alone keeps the states left out of
    the float32 Euler comparison (1e-3 rad from the atan2 cut, or cy < 1e-3) under 5 %."""
    from oracle.oracle import Oracle
    m = die
    S = rollouts
    assert len(S) == 600 and max(s[5] for s in S) <= 128 and max(s[5] for s in S) >= 10
    assert max(s[6] for s in S) <= 120 and max(s[7] for s in S) <= 10
    P = pick_states(S, 48)
    assert len(P) == 48
    for tag in ("palm", "finger", "falling"):
        assert sum(tag in s[3] for s in P) >= 8, tag
    assert sum((3, 3) in s[4] for s in P) >= 8 and sum((3, 6) in s[4] for s in P) >= 8     # capsule - capsule and capsule - box
    o = Oracle(m.blob())
    left_out, first_drop = 0, []
    for ep in range(4):
        drop_at = None
        for k, s in enumerate(S[150 * ep:150 * (ep + 1)]):
            x, Ro, Rt = _frames(H.forward_at(o, s[0]), m)
            cy, cut = euler_margin(Ro)
            left_out += bool(cy < 1e-3 or cut < 1e-3)
            if drop_at is None and reorient_restate(s[0], s[1], s[2], x[0], x[4], Ro, Rt, DT)[2][0]:
                drop_at = k + 1
        first_drop.append(drop_at)
    assert left_out <= 0.05 * len(S), left_out
    assert all(d is not None and 20 <= d <= 80 for d in first_drop), first_drop
