"""GPU tests (pytest -m gpu) of the per-env object parameters (include/myo_hip_objects.h): size, position and friction of selected geoms
and the mass of selected bodies on the TrackEnv-class step kernel, for the baoding balls and the die.

  1. hip vs hip: every env of a batch with distinct explicit rows against a one-env batch of Model.with_geom_params / with_body_mass with
     the same float32 numbers and the subsystem off; 1e-5 on qpos / qvel / act (tests/test_gpu_body_mass.py's hip-vs-hip bound).
  2. hip vs the float64 oracle on the edited blobs, 1 and 10 substeps, with the tolerances and the same-contact-count share of
     tests/test_gpu_baoding.py / tests/test_gpu_die.py.
  3. The edits reach the physics: contact distance = centre height - the env's radius; friction and mass change the step; geom_xpos of the
     die's geoms follows the env's pos.
  4. Reset draws: ranges, independence, the die's exact correlation, the host twin, sharding, autoreset.
  5. Off is off.  6. Refusals.  7. A bad env keeps its rows.  8. The two P2 configurations, through env.step and through the fused bench epilogue.  9. The file against the poisoned build."""
import numpy as np
import pytest

import hand_task_checks as H
import object_params_cases as K
from object_params_cases import CH, bd_rows as _bd_rows, die_rows as _die_rows, edited as _edited
from test_gpu_baoding import CASE as BD
from test_gpu_die import CASE as DIE

pytestmark = pytest.mark.gpu
OBJ = "step_kernel_obj<36,20,32,2,2,false,0,false,true,false>"
TOL = 1e-5                       # the project's hip-vs-hip bound (tests/test_gpu_body_mass.py::_hip_vs_hip)
f32 = np.float32


@pytest.fixture(scope="module")
def bd():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_baoding")


@pytest.fixture(scope="module")
def die():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_die")


@pytest.fixture(scope="module")
def bd_states(bd):
    return K.baoding_states(bd)


@pytest.fixture(scope="module")
def die_picked(die):
    return K.die_states(die)


def _objects(b, m, task):
    from myosuite_mjx_amd import objects
    gs, bs = objects.task_objects(m, task)
    return objects.ObjectParams(b, m, gs, bs)


def _step(b, q, v, act, a, nsub, kernel):
    from myosuite_mjx_amd import capi
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act), (capi.F_ACTION, a)):
        b.write(f, x)
    b.step(b.field_ptr(capi.F_ACTION)[0], capi.ACTMAP_MUSCLE_SIGMOID, nsub)
    assert b.last_kernel_name() == kernel
    return b.read(capi.F_QPOS), b.read(capi.F_QVEL), b.read(capi.F_ACT), b.read(capi.F_CTRL), b.read(capi.F_DIAG), b.status()


# ---- 1. hip vs hip ------------------------------------------------------------------------------------------------------------------
def _hip_vs_hip(case, m, task, rows, state, nsub):
    from myosuite_mjx_amd import capi
    gs, bs, size, pos, fr, mass = rows
    q, v, act = state
    B = len(q)
    a = np.random.default_rng(5).uniform(-1, 1, (B, m.nu)).astype(f32)
    b = H.new_batch(case, m, B)
    p = _objects(b, m, task)
    p.size, p.friction, p.mass = size, fr, mass
    if pos is not None:
        p.pos = pos
    gq, gv, ga, _, _, fl = _step(b, q, v, act, a, nsub, OBJ)
    assert (fl == 0).all(), fl
    worst = 0.0
    for e in range(B):
        one = H.new_batch(case, _edited(m, gs, bs, size[e], None if pos is None else pos[e], fr[e], mass[e]), 1)
        rq, rv, ra, _, _, rfl = _step(one, q[e:e + 1], v[e:e + 1], act[e:e + 1], a[e:e + 1], nsub, H.TRK)
        assert (rfl == 0).all()
        err = max(float(np.abs(x[e] - y[0]).max()) for x, y in ((gq, rq), (gv, rv), (ga, ra)))
        print(f"{task} hip-vs-hip env {e}: {err:.3e}")
        worst = max(worst, err)
    assert worst < TOL, worst
    return gq, gv


def test_hip_vs_hip_baoding(bd, bd_states):
    q, v = bd_states["palm"]
    act = np.random.default_rng(2).uniform(0, 1, (8, bd.nu)).astype(f32)
    gs, bs, size, fr, mass = _bd_rows(bd, 8)
    gq, gv = _hip_vs_hip(BD, bd, "baoding", (gs, bs, size, None, fr, mass), (q, v, act), BD.nsub)
    assert np.abs(gq - q).max() > 1e-4


def test_hip_vs_hip_die(die, die_picked):
    q, v, act = (x[:4] for x in die_picked)
    _hip_vs_hip(DIE, die, "die", _die_rows(die, 4), (q, v, act), DIE.nsub)


# ---- 2. hip vs the float64 oracle on the edited blob ---------------------------------------------------------------------------------
def _vs_oracle(case, m, task, rows, state, nsub):
    from oracle.oracle import Oracle
    gs, bs, size, pos, fr, mass = rows
    q, v, act = state
    B = len(q)
    a = np.random.default_rng(9).uniform(-1, 1, (B, m.nu)).astype(f32)
    b = H.new_batch(case, m, B)
    p = _objects(b, m, task)
    p.size, p.friction, p.mass = size, fr, mass
    if pos is not None:
        p.pos = pos
    gq, gv, _, ctrl, diag, fl = _step(b, q, v, act, a, nsub, OBJ)
    eq, ev, nc = np.zeros(B), np.zeros(B), np.zeros(B, int)
    for e in range(B):
        o = Oracle(_edited(m, gs, bs, size[e], None if pos is None else pos[e], fr[e], mass[e]).blob())
        o.reset()
        o.set_state(qpos=q[e], qvel=v[e], act=act[e], ctrl=ctrl[e])
        assert o.step(nsub) == 0
        eq[e], ev[e], nc[e] = np.abs(gq[e] - o.field("qpos")).max(), np.abs(gv[e] - o.field("qvel")).max(), o.ncon
    same = H.same_contacts(fl, diag[:, 1], nc)
    print(f"{task} vs oracle nsub={nsub}: same {same.mean():.3f}, max|dqpos| {eq[same].max():.3e}, max|dqvel| {ev[same].max():.3e}, all {eq.max():.3e} / {ev.max():.3e}")
    return eq, ev, same


@pytest.mark.parametrize("nsub,tq,tv", [(1, 2e-5, 2e-2), (10, 2e-3, 0.2)])      # tests/test_gpu_baoding.py::test_contact_parity's numbers
def test_oracle_parity_baoding(bd, bd_states, nsub, tq, tv):
    gs, bs, size, fr, mass = _bd_rows(bd, 8)
    same_all = []
    for kind in ("palm", "ballball", "floor"):
        q, v = bd_states[kind]
        act = np.random.default_rng(3).uniform(0, 1, (8, bd.nu)).astype(f32)
        eq, ev, same = _vs_oracle(BD, bd, "baoding", (gs, bs, size, None, fr, mass), (q, v, act), nsub)
        assert eq[same].max() < tq and ev[same].max() < tv, (kind, eq.tolist(), ev.tolist(), same.tolist())
        same_all += same.tolist()
    assert np.mean(same_all) > 0.8, same_all


@pytest.mark.parametrize("nsub,tq,tv", [(1, 2e-5, 2e-2), (10, 2e-3, 0.2)])      # tests/test_gpu_die.py::test_contact_parity's numbers
def test_oracle_parity_die(die, die_picked, nsub, tq, tv):
    eq, ev, same = _vs_oracle(DIE, die, "die", K.die_rows8(die), die_picked, nsub)
    assert same.mean() > 0.8, same.tolist()
    assert eq[same].max() < tq and ev[same].max() < tv, (eq.tolist(), ev.tolist(), same.tolist())


# ---- 3. the edit reaches the physics --------------------------------------------------------------------------------------------------
def test_contact_distance_is_centre_height_minus_the_envs_radius(bd, bd_states):
    from myosuite_mjx_amd import capi
    q, v = bd_states["floor"]
    b = H.new_batch(BD, bd, 8)
    p = _objects(b, bd, "baoding")
    r = np.linspace(0.022, 0.024, 8).astype(f32)        # (the states hold the balls' centres 0.020 .. 0.022 above the floor: every radius here touches it)
    size = p.size
    size[:, 0, :], size[:, 1, :] = r[:, None], r[::-1, None]
    p.size = size
    b.write(capi.F_QPOS, q)
    b.write(capi.F_QVEL, v)
    b.forward()
    ncon, rec, gx = b.forward_read(capi.FWD_NCON), b.forward_read(capi.FWD_CONTACT), b.forward_read(capi.FWD_GEOM_XPOS)
    ids = rec[..., 13:16].view(np.int32)
    g = [bd.name2id("geom", n) for n in ("ball1", "ball2")]
    floor_z = float(bd.geom_pos[0][2])
    assert int(bd.geom_type[0]) == 0                    # geom 0 is the floor plane
    seen = 0
    for e in range(8):
        for k, rad in ((0, r[e]), (1, r[::-1][e])):
            hit = [c for c in range(ncon[e]) if {int(ids[e, c, 0]), int(ids[e, c, 1])} == {0, g[k]}]
            assert len(hit) == 1, (e, k, ncon[e])
            want = (float(gx[e, g[k], 2]) - floor_z) - float(rad)
            assert abs(float(rec[e, hit[0], 0]) - want) < 1e-6, (e, k, float(rec[e, hit[0], 0]), want)
            seen += 1
    assert seen == 16


def _pair_of_envs(case, m, task, q, v, act, nsub, edit):
    """Two envs in the same state, differing only in what edit(p, env) writes: their qvel after one env step."""
    b = H.new_batch(case, m, 2)
    p = _objects(b, m, task)
    edit(p)
    a = np.zeros((2, m.nu), f32)
    gq, gv, _, _, _, fl = _step(b, np.tile(q, (2, 1)), np.tile(v, (2, 1)), np.tile(act, (2, 1)), a, nsub, OBJ)
    assert (fl == 0).all()
    return gv


def test_friction_and_mass_change_the_step(bd, bd_states):
    q, v = (x[0].copy() for x in bd_states["floor"])
    v[23:26], v[29:32] = (0.5, 0.0, 0.0), (0.0, 0.5, 0.0)       # both balls sliding on the floor, no spin
    v[26:29] = v[32:35] = 0.0
    act = np.zeros(bd.nu, f32)

    def friction(p):
        fr = p.friction
        fr[0, :, 0], fr[1, :, 0] = 0.8, 1.2
        p.friction = fr
    gv = _pair_of_envs(BD, bd, "baoding", q, v, act, BD.nsub, friction)
    assert np.abs(gv[0] - gv[1]).max() > 10 * TOL, np.abs(gv[0] - gv[1]).max()
    q, v = (x[0] for x in bd_states["palm"])

    def mass(p):
        ms = p.mass
        ms[0], ms[1] = 0.03, 0.3
        p.mass = ms
    gv = _pair_of_envs(BD, bd, "baoding", q, v, act, BD.nsub, mass)
    assert np.abs(gv[0] - gv[1]).max() > 10 * TOL, np.abs(gv[0] - gv[1]).max()


def test_die_geom_xpos_follows_the_envs_pos(die, die_picked):
    from myosuite_mjx_amd import capi
    q = die_picked[0][:4]
    gs, bs, size, pos, fr, mass = _die_rows(die, 4)
    b = H.new_batch(DIE, die, 4)
    p = _objects(b, die, "die")
    p.pos = pos
    b.write(capi.F_QPOS, q)
    b.forward()
    gx, xm, xp = b.forward_read(capi.FWD_GEOM_XPOS), b.forward_read(capi.FWD_XMAT), b.forward_read(capi.FWD_XPOS)
    ob = die.name2id("body", "Object")
    moved = 0.0
    for e in range(4):
        want = xp[e, ob][None] + np.einsum("ij,gj->gi", xm[e, ob].astype(float), pos[e].astype(float))
        assert np.abs(gx[e, gs] - want).max() < 1e-6, (e, np.abs(gx[e, gs] - want).max())
        moved = max(moved, np.abs(pos[e] - pos[0]).max())
    others = [g for g in range(die.ngeom) if g not in gs]
    one = H.new_batch(DIE, die, 4)                              # and the geoms that are not selected stay where the plain model has them
    one.write(capi.F_QPOS, q)
    one.forward()
    assert np.array_equal(one.forward_read(capi.FWD_GEOM_XPOS)[:, others], gx[:, others]) and moved > 0.006


# ---- 4. reset draws -------------------------------------------------------------------------------------------------------------------
def _p2_env(name, B, seed=H.SEED, env_offset=0, randomize=True, **kw):
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import envs
    p1, mk, rk = envs.P2_CONFIGS[name]
    env = myo.make(p1, num_envs=B, seed=seed, env_offset=env_offset, as_torch=False, **mk, **kw)
    table = env.set_object_randomization(**rk) if randomize else None
    return env, table, rk


def test_reset_draws_baoding():
    from myosuite_mjx_amd import capi, objects
    B = 64
    env, t, rk = _p2_env("myoChallengeBaodingP2-v1", B)
    p = env.object_params
    before = p.rows()
    env.reset()
    r0 = p.rows()
    size, fr, mass = p.size, p.friction, p.mass
    assert (size >= 0.018).all() and (size <= 0.024).all() and (mass >= 0.030).all() and (mass <= 0.300).all()
    nom = np.array(env.mjmodel.geom_friction, float)[p.geom_ids[0]]
    assert (fr >= (nom - CH).astype(f32) - 1e-9).all() and (fr <= (nom + CH).astype(f32) + 1e-9).all() and np.array_equal(p.pos, before[:, 6:12].reshape(B, 2, 3))
    assert (size[:, :, 0] == size[:, :, 1]).all() and (size[:, :, 0] == size[:, :, 2]).all()           # one draw per ball, all three components
    for x in (size[:, 0, 0], size[:, 1, 0], mass[:, 0], mass[:, 1], fr[:, 0, 0], fr[:, 1, 1]):
        assert len(np.unique(x)) > B - 4                                                                # differ across envs
    assert abs(np.corrcoef(size[:, 0, 0], size[:, 1, 0])[0, 1]) < 0.4 and abs(np.corrcoef(mass[:, 0], mass[:, 1])[0, 1]) < 0.4      # independent per ball (64 samples: 3.2 sigma)
    # the host twin: episode 0 of global envs 0 .. 63 under the env's seed
    want = objects.predict_rows(H.SEED, 0, range(B), t, before)
    assert np.abs(r0 - want).max() <= 1e-6 * np.abs(want).max(), np.abs(r0 - want).max()
    env.reset()
    r1 = p.rows()
    assert (r1[:, :6] != r0[:, :6]).all()                                                             # another episode, other sizes
    assert np.abs(r1 - objects.predict_rows(H.SEED, 1, range(B), t, r0)).max() <= 1e-6 * np.abs(want).max()
    # sharding: the upper half at env_offset 32 draws what envs 32 .. 63 drew
    s, _, _ = _p2_env("myoChallengeBaodingP2-v1", 32, env_offset=32)
    s.reset()
    assert np.array_equal(s.object_params.rows(), r0[32:])
    # autoreset re-draws only the envs whose episode ended
    el = env.batch.read(capi.F_ELAPSED)
    el[::4] = env.max_episode_steps
    env.batch.write(capi.F_ELAPSED, el)
    env.batch.autoreset(env.max_episode_steps, H.SEED)
    r2 = p.rows()
    assert np.array_equal(r2[1::4], r1[1::4]) and np.array_equal(r2[2::4], r1[2::4]) and (r2[::4, :6] != r1[::4, :6]).all()
    assert np.abs(r2[::4] - objects.predict_rows(H.SEED, 2, range(0, B, 4), t, r1[::4])).max() <= 1e-6 * np.abs(want).max()


def test_reset_draws_die_are_exactly_correlated():
    from myosuite_mjx_amd import objects
    B = 64
    env, t, rk = _p2_env("myoChallengeDieReorientP2-v0", B)
    p = env.object_params
    before = p.rows()
    env.reset()
    r = p.rows()
    want = objects.predict_rows(H.SEED, 0, range(B), t, before)
    assert np.abs(r - want).max() <= 1e-6 * np.abs(want).max()
    driven = np.flatnonzero(t.draw == 0)
    assert len(driven) == 45
    b32, s32 = t.base.astype(f32).astype(float), t.scale.astype(f32).astype(float)
    # del from one geom's half length predicts the other 44 driven values of the env: exactly, up to the one float32 rounding of each
    u = (r[:, driven[0]].astype(float) - b32[driven[0]]) / s32[driven[0]]
    assert (u > -1e-3).all() and (u < 1 + 1e-3).all() and len(np.unique(r[:, driven[0]])) > B - 4
    pred = b32[driven][None] + s32[driven][None] * u[:, None]
    assert np.abs(r[:, driven] - pred).max() < 2 * 2.0 ** -24 * 0.05 + 0.014 * 2.0 ** -19, np.abs(r[:, driven] - pred).max()   # u is known to one ulp of the half length
    fr, mass = p.friction, p.mass
    assert (mass >= 0.05).all() and (mass <= 0.25).all() and len(np.unique(fr[:, :, 0])) > 15 * B - 30                          # friction: independent per geom and component
    assert np.array_equal(r[:, t.scale == 0], before[:, t.scale == 0])                                                          # nothing else is touched
    s, _, _ = _p2_env("myoChallengeDieReorientP2-v0", 32, env_offset=32)
    s.reset()
    assert np.array_equal(s.object_params.rows(), r[32:])


# ---- 5. off is off --------------------------------------------------------------------------------------------------------------------
def test_enabled_with_compiled_values_equals_never_enabled():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi, objects
    B, T = 8, 20
    envs = [myo.make("myoChallengeBaodingP1-v1", num_envs=B, seed=4, as_torch=False, task_choice="random") for _ in range(2)]
    on, off = envs
    p = on.object_params
    assert tuple(p.size.shape) == (B, 2, 3) and tuple(p.mass.shape) == (B, 2) and p.geom_names == ["ball1", "ball2"] and p.body_names == ["ball1", "ball2"]
    assert np.allclose(p.size, [0.022, 0, 0]) and np.allclose(p.mass, 0.043) and np.allclose(p.friction[0, 0], [1.0, 0.005, 0.0001])      # the compiled values
    for e in envs:
        e.reset()
    rng = np.random.default_rng(0)
    for _ in range(T):
        a = rng.uniform(-1, 1, (B, on.act_dim)).astype(f32)
        for e in envs:
            e.step(a)
    assert on.batch.last_kernel_name() == OBJ and off.batch.last_kernel_name() == H.TRK
    for f in (capi.F_QPOS, capi.F_QVEL, capi.F_ACT, capi.F_OBS):
        assert np.abs(on.batch.read(f) - off.batch.read(f)).max() < TOL, f
    # never enabled: the pointer calls report absent, and nothing was allocated
    ptr, pitch, width = capi.C.c_void_p(), capi.C.c_size_t(), capi.C.c_size_t()
    rc = objects.lib().myo_objects_table(off.batch.h, objects.OBJ_SIZE, capi.C.byref(ptr), capi.C.byref(pitch), capi.C.byref(width))
    assert rc == -1 and b"absent" in capi.lib().myo_last_error() and not ptr.value
    ng, nb = capi.C.c_int(-1), capi.C.c_int(-1)
    assert objects.lib().myo_objects_count(off.batch.h, capi.C.byref(ng), capi.C.byref(nb)) == 0 and (ng.value, nb.value) == (0, 0)


def test_torch_views_are_writable_and_take_effect(bd_states, bd):
    import torch
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make("myoChallengeBaodingP1-v1", num_envs=8, seed=4, autoreset=False)
    p = env.object_params
    assert p.size.is_cuda and tuple(p.friction.shape) == (8, 2, 3) and p.size.data_ptr() == p.table_ptr(0)[0]       # zero copy
    q, v = bd_states["floor"]
    env.set_env_state(dict(qpos=q, qvel=v))
    p.size[:4] = 0.024                                               # in place, through the view
    p.mass = torch.tensor([0.05, 0.06])                              # one row, broadcast
    rec = env.forward()
    torch.cuda.synchronize()
    d = np.array([[float(rec.contact.dist[e, c]) for c in range(int(rec.ncon[e])) if 0 in (int(rec.contact.geom1[e, c]), int(rec.contact.geom2[e, c]))] for e in range(8)])
    assert d.shape == (8, 2) and (d[:4].mean() < d[4:].mean() - 0.0015)      # the larger balls sit 2 mm deeper
    assert np.allclose(env.batch.read(capi.F_QPOS), q) and torch.allclose(p.mass.cpu(), torch.tensor([[0.05, 0.06]] * 8))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(b, m, geoms, bodies, match, code=-4):
    from myosuite_mjx_amd import capi, objects
    with pytest.raises(capi.MyoError, match=match) as e:
        objects.ObjectParams(b, m, geoms, bodies)
    assert f"error {code}:" in str(e.value), str(e.value)


def test_refusals(bd, die):
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi, envs, objects, model as M
    hand = M.load_asset("myohand_pose")
    hb = capi.HipBatch(capi.HipModel(hand.blob(), 0), 2)
    _refused(hb, hand, [int(hand.hip_cg_geom[0])], [], "TrackEnv class only")                                     # a non-TRK model
    rk = hand.with_integrator("RK4")
    _refused(capi.HipBatch(capi.HipModel(rk.blob(), 0), 2), rk, [int(rk.hip_cg_geom[0])], [], "RK4")              # the RK4 twin
    env = myo.make("myoHandPoseFixed-v0", num_envs=2, as_torch=False)
    with pytest.raises(capi.MyoError, match="TrackEnv class only"):
        env.enable_object_params(geoms=[int(hand.hip_cg_geom[0])])
    with pytest.raises(AttributeError, match="enable_object_params"):
        env.object_params
    b = H.new_batch(BD, bd, 2)
    cg = [int(g) for g in bd.hip_cg_geom]
    assert int(bd.geom_type[0]) == 0 and 0 in cg
    _refused(b, bd, [0], [], "plane and height-field")                                                            # the floor plane
    prim = [g for g in range(bd.ngeom) if g not in cg and int(bd.geom_type[g]) in (2, 3, 4, 5, 6)]
    _refused(b, bd, prim[:1], [], "not a collision geom")
    hand_caps = [g for g in cg if int(bd.geom_type[g]) == 3]
    assert len(hand_caps) >= 17
    _refused(b, bd, hand_caps[:17], [], "at most 16 geoms and 4 bodies")
    moving = [k for k in range(1, bd.nbody) if int(bd.hip_body_link[k]) >= 0]
    _refused(b, bd, [], moving[:5], "at most 16 geoms and 4 bodies")
    shared = [k for k in moving if (np.asarray(bd.hip_body_link) == bd.hip_body_link[k]).sum() > 1]
    assert shared                                                                                                 # (the hand has welded bodies)
    _refused(b, bd, [], shared[:1], "shares its kinematic link")
    _refused(b, bd, [bd.ngeom], [], "out of range", code=-1)
    _refused(b, bd, [cg[1], cg[1]], [], "listed twice", code=-1)
    air = M.load_asset("myohand_object_airplane")
    mesh = [int(g) for g in air.hip_cg_geom if int(air.geom_type[g]) == 7]
    ab = capi.HipBatch(capi.HipModel(air.blob(), 0), 2)
    _refused(ab, air, mesh[:1], [], "mesh / hull")
    # the MyoDM track task resets inside the step kernel: explicit values work, a draw table is refused
    tenv = myo.make("MyoHandAirplaneFixed-v0", num_envs=2)
    caps = [int(g) for g in tenv.mjmodel.hip_cg_geom if int(tenv.mjmodel.geom_type[g]) == 3 and int(tenv.mjmodel.hip_body_link[tenv.mjmodel.geom_bodyid[g]]) >= 0]
    tp = objects.ObjectParams(tenv.batch, tenv.mjmodel, caps[:2], [])
    tp.size = tp.read(objects.OBJ_SIZE) * 1.1
    t = objects.DrawTable(2, 0)
    t.set("size", 0, 0, 0.004, 0.006)
    with pytest.raises(capi.MyoError, match="resets inside the step kernel") as e:
        tp.set_draws(t)
    assert "error -4:" in str(e.value)
    # bad host values: MYO_E_ARG, and nothing is written
    p = _objects(b, bd, "baoding")
    before = p.rows()
    for name, bad in (("size", -0.01), ("friction", -1.0), ("mass", -0.1), ("size", np.nan), ("pos", np.inf), ("mass", np.nan)):
        a = np.array(getattr(p, name))
        a[1, 0] = bad
        with pytest.raises(capi.MyoError, match="error -1:"):
            setattr(p, name, a)
    t = objects.task_draws(bd, "baoding", p.geom_ids, p.body_ids, obj_mass_range=(0.03, 0.3))
    t.base[t.index("mass", 0)] = -0.5
    with pytest.raises(capi.MyoError, match="error -1:"):
        p.set_draws(t)
    assert np.array_equal(p.rows(), before)
    with pytest.raises(capi.MyoError, match="another selection"):
        objects.ObjectParams(b, bd, p.geom_ids[:1], [])
    objects.ObjectParams(b, bd, p.geom_ids, p.body_ids)                                                           # the same selection again: a no-op
    # the ids and kwargs that need the subsystem wired into make() still raise, as the pinned host tests say
    with pytest.raises(NotImplementedError, match="size, mass and friction"):
        envs.make("myoChallengeBaodingP2-v1", num_envs=1)
    with pytest.raises(NotImplementedError, match="size, mass or friction"):
        envs.make("myoChallengeDieReorientP1-v0", num_envs=1, obj_size_change=0.007)
    with pytest.raises(ValueError):
        myo.make("myoChallengeBaodingP1-v1", num_envs=2, as_torch=False).set_object_randomization(obj_size_range=(0.024, 0.018))


# ---- 7. a bad env keeps its rows --------------------------------------------------------------------------------------------------------
def test_bad_env_is_contained_with_the_subsystem_on():
    import bad_env as BE
    import myosuite_mjx_amd as myo
    envs = [myo.make(BD.bench_id, num_envs=8, seed=1, as_torch=False, autoreset=False, **BD.make_kwargs) for _ in range(2)]
    rows = []
    for e in envs:
        p = e.object_params
        p.size = np.linspace(0.019, 0.024, 8).astype(f32)[:, None, None] * np.ones((1, 2, 3), f32)
        p.mass = np.linspace(0.03, 0.3, 16).astype(f32).reshape(8, 2)
        fr = p.friction
        fr[:, :, 0] = np.linspace(0.8, 1.2, 8).astype(f32)[:, None]
        p.friction = fr
        e.reset()
        rows.append(p.rows())
    env, clean = envs
    BE.task_contained(env, clean, "nan_qvel", 5)
    assert env.batch.last_kernel_name() == OBJ
    assert np.array_equal(env.object_params.rows(), rows[0]) and np.array_equal(clean.object_params.rows(), rows[1])     # model data, not state


# ---- 8. the P2 configurations -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["myoChallengeBaodingP2-v1", "myoChallengeDieReorientP2-v0"])
def test_p2_configuration_runs(name):
    from myosuite_mjx_amd import capi
    B = 16
    env, t, rk = _p2_env(name, B, seed=3)
    p = env.object_params
    env.reset()
    lo, hi = np.minimum(t.base, t.base + t.scale).astype(f32), np.maximum(t.base, t.base + t.scale).astype(f32)
    drawn = t.scale != 0
    rng = np.random.default_rng(0)
    prev, ended_any = p.rows(), 0
    for k in range(31):
        if k == 30:                                                  # make sure an episode ends: env 0 runs into the time limit
            el = env.batch.read(capi.F_ELAPSED)
            el[0] = env.max_episode_steps - 1
            env.batch.write(capi.F_ELAPSED, el)
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (B, env.act_dim)).astype(f32))
        assert np.isfinite(obs).all() and np.isfinite(rew).all()
        assert not env.status().any(), k                             # every step: myo_status reads and clears the flag words
        rows = p.rows()
        assert (rows[:, drawn] >= lo[drawn] - 1e-9).all() and (rows[:, drawn] <= hi[drawn] + 1e-9).all()
        ended = np.asarray(term) | np.asarray(trunc)
        assert np.array_equal(rows[~ended], prev[~ended])
        if ended.any():
            assert (np.abs(rows[ended][:, drawn] - prev[ended][:, drawn]).max(axis=1) > 0).all()
        ended_any += int(ended.sum())
        prev = rows
    assert ended_any >= 1 and env.batch.last_kernel_name() == OBJ


@pytest.mark.parametrize("name", ["myoChallengeBaodingP2-v1", "myoChallengeDieReorientP2-v0"])
def test_fused_bench_epilogue_redraws(name):
    """myo_bench_rollout's one-launch epilogue (task_post_kernel) runs the same reset body: with episodes of two steps every env has ended
    at least once after three steps, so every drawn parameter has changed, lies inside its range, and equals the host twin's row for the
    env's episode count."""
    from myosuite_mjx_amd import capi, objects
    B = 16
    env, t, rk = _p2_env(name, B, seed=3)
    p = env.object_params
    env.reset()
    r0 = p.rows()
    env.batch.bench_rollout(3, env.frame_skip, seed=3, mode=capi.BENCH_OBS | capi.BENCH_FRESH_ACTIONS | capi.BENCH_AUTORESET, max_episode_steps=2)
    r1 = p.rows()
    drawn = t.scale != 0
    lo, hi = np.minimum(t.base, t.base + t.scale).astype(f32), np.maximum(t.base, t.base + t.scale).astype(f32)
    assert (r1[:, drawn] != r0[:, drawn]).all() and np.array_equal(r1[:, ~drawn], r0[:, ~drawn])
    assert (r1[:, drawn] >= lo[drawn] - 1e-9).all() and (r1[:, drawn] <= hi[drawn] + 1e-9).all()
    el = env.batch.read(capi.F_ELAPSED)[:, 0]
    # an env is reset after step 2 (time limit) and possibly earlier by `done`: its episode count is 1 more per reset, and the last reset's
    # row is the twin's for one of the counts 1 .. 3 under the rollout's seed
    cands = [objects.predict_rows(3, ep, range(B), t, r0) for ep in (1, 2, 3)]
    for e in range(B):
        assert any(np.abs(r1[e] - c[e]).max() <= 1e-6 * np.abs(c[e]).max() for c in cands), (e, int(el[e]))
    assert env.batch.last_kernel_name() == OBJ


# ---- 9. the poisoned build --------------------------------------------------------------------------------------------------------------
def test_guard_poisoned_build():
    H.rerun_file_against_poison_build(__file__, timeout=900)
