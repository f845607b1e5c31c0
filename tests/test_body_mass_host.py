"""Per-env body masses, host side (no GPU): Model.with_body_mass recomposes the merged link of an edited body exactly as lowering does.
(The two field ids of the C ABI are pinned in tests/test_capi_host.py.)"""
import numpy as np
import pytest

from myosuite_mjx_amd import model as M
from myosuite_mjx_amd.mjcf import quat2mat

LINK_KEYS = ("hip_link_mass", "hip_link_com", "hip_link_inertia")


@pytest.mark.parametrize("name", ["myoelbow_1dof6muscles_1dofexo", "myohand_pose", "myohand_hold"])
def test_unchanged_mass_reproduces_the_committed_link_tables(name):
    m = M.load_asset(name)
    for b in range(m.nbody):
        e = m.with_body_mass(b, m.body_mass[b])
        for k in LINK_KEYS:
            a, c = np.asarray(m.arrays[k], float), np.asarray(e.arrays[k], float)
            np.testing.assert_allclose(c, a, rtol=1e-12, atol=0, err_msg=f"{name} body {b} {k}")


def _recompose(m, link):
    """Parallel-axis recomposition of one link from its member bodies, written out here from the bodies' frames (float64)."""
    members = [b for b in range(1, m.nbody) if int(m.hip_body_link[b]) == link]
    lpos = np.asarray(m.hip_body_lpos, float).reshape(-1, 3)
    lquat = np.asarray(m.hip_body_lquat, float).reshape(-1, 4)
    mass = 0.0
    mc = np.zeros(3)
    parts = []
    for b in members:
        R = quat2mat(lquat[b])
        c = lpos[b] + R @ np.asarray(m.body_ipos[b], float)                # body COM in the link frame
        Ri = R @ quat2mat(np.asarray(m.body_iquat[b], float))
        Ib = Ri @ np.diag(np.asarray(m.body_inertia[b], float)) @ Ri.T     # body inertia about its COM, link axes
        mb = float(m.body_mass[b])
        mass += mb
        mc += mb * c
        parts.append((mb, c, Ib))
    com = mc / mass
    I = np.zeros((3, 3))
    for mb, c, Ib in parts:
        d = c - com
        I += Ib + mb * (np.dot(d, d) * np.eye(3) - np.outer(d, d))
    return len(members), mass, com, np.array([I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]])


def _check_link(e, link):
    n, mass, com, inert = _recompose(e, link)
    assert n >= 2, "the body must sit in a link of several bodies"
    np.testing.assert_allclose(np.asarray(e.hip_link_mass, float).reshape(-1)[link], mass, rtol=1e-12)
    np.testing.assert_allclose(np.asarray(e.hip_link_com, float).reshape(-1, 3)[link], com, rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(np.asarray(e.hip_link_inertia, float).reshape(-1, 6)[link], inert, rtol=1e-9, atol=1e-14)


@pytest.mark.parametrize("w", [0.1, 1.0, 2.0])
def test_carry_weight_link_recomposition(w):
    m = M.load_asset("myoelbow_1dof6muscles_1dofexo")
    b = m.body_name2id("carry_weight")
    e = m.with_body_mass("carry_weight", w)
    assert e.body_mass[b] == w
    link = int(m.hip_body_link[b])
    _check_link(e, link)
    # the link's mass changes by exactly the edit
    d = float(np.asarray(e.hip_link_mass).reshape(-1)[link] - np.asarray(m.hip_link_mass).reshape(-1)[link])
    assert d == pytest.approx(w - float(m.body_mass[b]), rel=1e-12, abs=1e-15)


def test_hand_body_in_a_merged_link():
    m = M.load_asset("myohand_pose")
    links = np.asarray(m.hip_body_link)
    # a body that is not its link's head body (welded into a link with other members)
    b = next(b for b in range(1, m.nbody) if links[b] >= 0 and int(m.body_jntnum[b]) == 0 and (links == links[b]).sum() >= 2)
    for w in (0.5 * float(m.body_mass[b]), 3.0 * float(m.body_mass[b])):
        e = m.with_body_mass(b, w)
        _check_link(e, int(links[b]))
        other = [l for l in range(len(np.asarray(m.hip_link_mass).reshape(-1))) if l != links[b]]
        for k in LINK_KEYS:   # only the edited body's link changes
            np.testing.assert_array_equal(np.asarray(e.arrays[k]).reshape(len(other) + 1, -1)[other],
                                          np.asarray(m.arrays[k]).reshape(len(other) + 1, -1)[other])


def test_with_body_mass_rejects_negative_mass():
    m = M.load_asset("myoelbow_1dof6muscles_1dofexo")
    with pytest.raises(ValueError):
        m.with_body_mass("carry_weight", -1.0)


def test_pose_kwargs_are_pose_only():
    from myosuite_mjx_amd import envs
    # checked before the library is touched: a non-pose id keeps raising TypeError on the pose kwargs
    for k, v in (("weight_bodyname", "carry_weight"), ("weight_range", (0.1, 2.0)), ("target_jnt_range", {})):
        with pytest.raises(TypeError):
            envs.BatchedMyoEnv("myoHandReachFixed-v0", num_envs=1, **{k: v})
    with pytest.raises(TypeError):
        envs.BatchedMyoEnv("myoElbowPose1D6MExoFixed-v0", num_envs=1, weight_bodyname_typo="carry_weight")


def test_target_jnt_range_must_name_the_targeted_joints():
    from myosuite_mjx_amd import envs
    m = M.load_asset("myoelbow_1dof6muscles_1dofexo")
    spec = dict(envs.REGISTRY["myoElbowPose1D6MExoFixed-v0"], target_jnt_range={"r_elbow_flex": (0, 2.27)})
    lo, hi = envs.BatchedMyoEnv._target_jnt_range(m, spec)
    assert lo.tolist() == [0.0] and hi.tolist() == [2.27]
    for bad in ({}, {"r_elbow_flex": (0, 1), "nope": (0, 1)}, {"nope": (0, 1)}):
        with pytest.raises(ValueError):
            envs.BatchedMyoEnv._target_jnt_range(m, dict(spec, target_jnt_range=bad))
    h = M.load_asset("myohand_pose")
    hs = dict(envs.REGISTRY["myoHandPoseRandom-v0"])
    full = {n: (0.0, 0.1) for n in reversed(h.names["joint"])}       # any order
    lo, hi = envs.BatchedMyoEnv._target_jnt_range(h, dict(hs, target_jnt_range=full))
    assert np.all(lo == 0.0) and np.all(hi == 0.1)
    full.pop(h.names["joint"][3])
    with pytest.raises(ValueError):
        envs.BatchedMyoEnv._target_jnt_range(h, dict(hs, target_jnt_range=full))
