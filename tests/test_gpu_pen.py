"""GPU tests (pytest -m gpu) for myoHandPenTwirl{Fixed,Random}-v0 (envs/myo/myobase/pen_v0.py) on the TrackEnv-class ("TRK") step kernel:
MyoHand + a free pen (a condim-4 cylinder) + a world-welded target cylinder whose orientation is per env (MYO_F_BODYQUAT).

  * HIP vs the float64 oracle after 1 and 10 substeps: pen - floor contacts in the four branches of the plane - cylinder narrow phase,
    pen - finger contacts (a moving primitive cylinder against the hand), and pen / target contacts with the target turned per env
    (the oracle on Model.with_body_quat blobs).  Tolerances as in tests/test_gpu_keyturn.py.
  * MYO_F_SITEXPOS, observation, reward, done and solved against tests/pen_ref.py on 1024 envs; reset draws over 4096 envs and the
    device euler2quat against the reference's; determinism and sharding; orientation started with the compiled quaternion = off; the
    fused bench epilogue; the muscle-condition variants; refusals; the same file against the NaN-poisoned build."""
import os

import numpy as np
import pytest

import hand_task_checks as H
from pen_ref import euler2quat, pen_restate
from pen_states import branch_states

pytestmark = pytest.mark.gpu
SITES = ("object_top", "object_bottom", "target_top", "target_bottom", "eps_ball")
ID = "myoHandPenTwirlRandom-v0"


@pytest.fixture(scope="module")
def pen():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_pen")


def _bodies(m):
    ob, tb = m.name2id("body", "Object"), m.name2id("body", "target")
    pg = [g for g in range(m.ngeom) if m.geom_bodyid[g] == ob][0]
    tg = [g for g in range(m.ngeom) if m.geom_bodyid[g] == tb][0]
    return ob, tb, pg, tg


def _configure(b, m):
    from myosuite_mjx_amd import capi
    ob = m.name2id("body", "Object")
    b.configure(task=capi.TASK_PEN, frame_skip=5, tip_sites=[m.name2id("site", n) for n in SITES],
                tip_lpos=tuple(np.asarray(m.hip_body_lpos).reshape(-1, 3)[ob]), pose_thd=0.95, far_th=0.075,
                w_pose=1.0, w_reach=1.0, w_act_reg=5.0, w_bonus=10.0, w_penalty=5.0, init_qpos=np.zeros(m.nq), quat_body=m.name2id("body", "target"))


CASE = H.TaskCase(stem="myohand_pen", task="pen", bench_id=ID, obs_dim=83, nsub=5, configure=_configure, extra_fields=("F_BODYQUAT",),
                  env_ids=tuple(f"myo{c}HandPenTwirl{v}-v0" for c in ("", "Sarc", "Fati", "Reaf") for v in ("Fixed", "Random")))


_ROT = {}


def _rotated(m, k):
    """Oracle model k of a pool of eight target orientations (euler2quat of the Random variant's range), lowered once each."""
    if k not in _ROT:
        rng = np.random.default_rng(100 + k)
        quat = euler2quat([rng.uniform(-1, 1), rng.uniform(-1, 1), 0.0])
        _ROT[k] = (quat, m.with_body_quat(m.name2id("body", "target"), quat).blob())
    return _ROT[k]


def _init_q(m):
    q = np.array(m.qpos0, float)
    q[:-6] = 0
    q[0] = -1.5
    return q


def _states(m, kind, N, seed):
    """qpos, target quaternions and the contacts each state has, in one family: "floor" (the four plane - cylinder branches, jittered),
    "finger" (hand poses around the palm-up start with the pen near the fingers), "target" (the pen at the target turned per env)."""
    from oracle.oracle import Oracle
    ob, tb, pg, tg = _bodies(m)
    rng = np.random.default_rng(seed)
    o = Oracle(m.blob())
    lo, hi = m.jnt_range[:23, 0], m.jnt_range[:23, 1]
    qs, quats, tags = [], [], []
    base = branch_states(m)
    tries = 0
    while len(qs) < N:
        tries += 1
        assert tries < 400 * N
        quat = np.array([1.0, 0, 0, 0])
        if kind == "floor":
            name, q, n = base[len(qs) % 4]
            q = q.copy()
            q[-3:] += rng.normal(0, 0.003, 3) * (n != 3)     # (the cap state stays upright)
            q[-4] += rng.uniform(-0.0005, 0.0005)
            oo = o
        else:
            q = _init_q(m)
            q[1:23] = lo[1:] + rng.uniform(0.0, 0.5, 22) * (hi[1:] - lo[1:])
            if kind == "finger":
                q[-6:] += rng.normal(0, 0.02, 6)
                oo = o
            else:
                quat, blob = _rotated(m, int(rng.integers(8)))
                c, s = np.cos(2 * np.arctan2(m.body_quat[ob][2], m.body_quat[ob][0])), np.sin(2 * np.arctan2(m.body_quat[ob][2], m.body_quat[ob][0]))
                Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
                d = m.body_pos[tb] - m.body_pos[ob] + rng.normal(0, 0.012, 3) + np.array([0.028, 0, 0])
                q[-6:-3] = Ry.T @ d
                q[-3:] = rng.uniform(-1, 1, 3)
                oo = Oracle(blob)
        cs = H.forward_at(oo, q).contacts()
        pairs = {frozenset((int(c[7]), int(c[8]))) for c in cs}
        if not cs or min(c[0] for c in cs) < -0.004 and kind != "floor":
            continue
        if kind == "finger" and not any(pg in p and 0 not in p and tg not in p for p in pairs):
            continue
        if kind == "target" and not any(tg in p for p in pairs):
            continue
        qs.append(q)
        quats.append(quat)
        tags.append(pairs)
    f32 = np.float32
    v = rng.normal(0, 0.3, (N, m.nv))
    return (np.array(qs).astype(f32), np.array(quats).astype(f32), v.astype(f32), rng.uniform(0, 1, (N, m.nu)).astype(f32),
            rng.uniform(-1, 1, (N, m.nu)).astype(f32), tags)


@pytest.mark.parametrize("kind", ["floor", "finger", "target"])
@pytest.mark.parametrize("nsub,tq,tv", [(1, 2e-5, 2e-2), (10, 2e-3, 0.2)])
def test_contact_parity(pen, kind, nsub, tq, tv):
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = pen
    ob, tb, pg, tg = _bodies(m)
    N = 48
    q, quat, v, act, a, tags = _states(m, kind, N, {"floor": 1, "finger": 2, "target": 3}[kind])
    b = H.new_batch(CASE, m, N)
    state = {capi.F_QPOS: q, capi.F_QVEL: v, capi.F_ACT: act, capi.F_ACTION: a}
    if kind == "target":
        state[capi.F_BODYQUAT] = quat
    o0 = Oracle(m.blob())

    def oracle_for_env(e):
        return o0 if kind != "target" else Oracle(next(bl for qq, bl in _ROT.values() if np.allclose(qq, quat[e], atol=1e-6)))

    eq, ev, nc, dg, fl, same = H.step_and_compare_with_oracle(m, b, state, nsub, oracle_for_env)
    if kind == "floor" and nsub > 1:
        # the pen resting on its cap: the oracle skips a cylinder pair whose other geom's centre lies beyond the cylinder's cap planes
        # along its axis (its cap filter, with the plane's bounding radius 0), which drops the resting contacts of a tilted pen whose
        # centre is less than r sin(tilt) above hh -- MuJoCo, and the kernel, keep them.  One substep compares this branch (above)
        same[2::4] = False
    assert same.mean() > (0.6 if kind == "floor" and nsub > 1 else 0.8), (same.mean(), dg[:, 1].tolist(), nc.tolist())
    w = int(np.argmax(np.where(same, eq, 0)))
    assert eq[same].max() < tq and ev[same].max() < tv, (eq[same].max(), ev[same].max(), w, [sorted(p) for p in tags[w]], int(nc[w]))
    if kind == "floor" and nsub == 1:
        for k, n in enumerate((1, 2, 3, 4)):         # every branch among the compared states
            assert any(same[e] for e in range(k, N, 4)), n
    assert np.abs(b.read(capi.F_QPOS) - q).max() > 1e-5


def test_site_positions_and_restatement(pen):
    """MYO_F_SITEXPOS against the oracle's site_xpos (the target turned per env), the observation row / reward / done / solved against
    the float64 restatement, on 1024 envs whose states span the thresholds."""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = pen
    ob, tb, _, _ = _bodies(m)
    N = 1024
    rng = np.random.default_rng(5)
    lo, hi = m.jnt_range[:23, 0], m.jnt_range[:23, 1]
    q = np.tile(_init_q(m), (N, 1))
    q[:, 1:23] = lo[1:] + rng.uniform(0, 1, (N, 22)) * (hi[1:] - lo[1:])
    q[:, -6:-3] = rng.normal(0, 0.05, (N, 3))
    th0 = 2 * np.arctan2(m.body_quat[ob][2], m.body_quat[ob][0])
    q[:, -3:] = rng.normal(0, 0.3, (N, 3)) * rng.uniform(0, 1, (N, 1))
    q[:, -2] -= th0 * (rng.uniform(0, 1, N) < 0.5)                    # half of them near the target's upright axis
    pick = rng.integers(-8, 8, N)                                       # half of them at the compiled orientation
    quat = np.array([_rotated(m, k)[0] if k >= 0 else [1.0, 0, 0, 0] for k in pick]).astype(np.float32)
    q, v, act = q.astype(np.float32), rng.normal(0, 1, (N, m.nv)).astype(np.float32), rng.uniform(0, 1, (N, m.nu)).astype(np.float32)
    b = H.new_batch(CASE, m, N)
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act), (capi.F_BODYQUAT, quat)):
        b.write(f, x)
    b.obs()
    sx, obs, rew, done, solved = (b.read(f) for f in (capi.F_SITEXPOS, capi.F_OBS, capi.F_REWARD, capi.F_DONE, capi.F_SOLVED))
    assert sx.shape == (N, 15) and obs.shape == (N, 83)
    xp = np.zeros((N, 3))
    for e in range(N):
        if e % 16 == 0:
            o = Oracle(_rotated(m, pick[e])[1] if pick[e] >= 0 else m.blob())
            H.forward_at(o, q[e])
            assert np.abs(sx[e] - H.site_xpos(o, m, SITES)).max() < 5e-6, e
            assert np.abs(obs[e, 23:26] - o.field("xpos").reshape(-1, 3)[ob]).max() < 5e-6
        xp[e] = obs[e, 23:26]
    ro, rr, rd, rs = pen_restate(q, v, act, sx, xp, 0.01)
    assert np.abs(obs - ro).max() < 1e-5
    assert np.abs(rew[:, 0] - rr).max() < 1e-3 * max(1.0, np.abs(rr).max())
    assert np.array_equal(done[:, 0] > 0, rd) and np.array_equal(solved[:, 0] > 0, rs)
    assert rd.any() and not rd.all() and rs.any() and not rs.all()


def test_reset_draws_and_sharding():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B = 4096

    def make_env(n, seed, off):
        return myo.make(ID, num_envs=n, seed=seed, env_offset=off, as_torch=False)

    env = make_env(B, H.SEED, 0)
    obs = env.reset()
    m = env.mjmodel
    q, quat = env.batch.read(capi.F_QPOS), env.body_quat
    assert np.array_equal(q, np.tile(_init_q(m).astype(np.float32), (B, 1)))       # palm-up open hand, pen at qpos0
    assert np.abs(np.linalg.norm(quat, axis=1) - 1).max() < 1e-6
    # the reference's euler2quat(x, y, 0) = (cos(y/2) cos(x/2), cos(y/2) sin(x/2), sin(y/2) cos(x/2), -sin(y/2) sin(x/2)): recover the two
    # angles and check U(-1, 1)
    w, x, y, z = quat.T.astype(np.float64)
    ex, ey = 2 * np.arctan2(x, w), 2 * np.arctan2(y, w)
    assert np.abs(euler2quat(np.stack([ex, ey, np.zeros(B)], 1)) - quat).max() < 2e-6
    for a in (ex, ey):
        assert a.min() >= -1 - 1e-5 and a.max() <= 1 + 1e-5
        H.assert_uniform(a, -1, 1)
    assert np.abs(obs[:, 35:38] - env.batch.read(capi.F_SITEXPOS)[:, 6:9] / 0.13 + env.batch.read(capi.F_SITEXPOS)[:, 9:12] / 0.13).max() < 1e-5
    H.assert_deterministic_and_sharded(make_env, lambda e: (e.body_quat,), B, (quat,))
    f = myo.make("myoHandPenTwirlFixed-v0", num_envs=64, seed=H.SEED, as_torch=False)
    f.reset()
    assert np.array_equal(f.body_quat, np.tile([1, 0, 0, 0], (64, 1)).astype(np.float32))
    assert not f.batch.read(capi.F_BODYQUAT_RANGE).any()


def test_device_euler2quat_matches_reference(pen):
    """Ranges of zero width around the reference's test angles: the quaternions drawn at reset are the reference's euler2quat."""
    from myosuite_mjx_amd import capi
    g = np.load(os.path.join(H.ROOT, "tests", "golden", "ref_quat_math.npz"))
    eul = g["euler"].astype(np.float32)
    n = len(eul)
    b = H.new_batch(CASE, pen, n)
    b.set_body_quat_range(eul, np.nextafter(eul, np.float32(np.inf)))
    b.reset(seed=1)
    assert np.abs(b.read(capi.F_BODYQUAT) - g["euler2quat"]).max() < 2e-6


def test_override_with_compiled_quat_is_override_off(pen):
    from myosuite_mjx_amd import capi
    m = pen
    N = 48
    q, _, v, act, a, _ = _states(m, "finger", N, 4)
    hm = capi.HipModel(m.blob(), 0)
    out = []
    for on in (False, True):
        b = capi.HipBatch(hm, N)
        _configure(b, m)
        for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act), (capi.F_ACTION, a)):
            b.write(f, x)
        if on:
            b.write(capi.F_BODYQUAT, b.read(capi.F_BODYQUAT))         # the compiled quaternion
        for _ in range(3):
            b.step(b.field_ptr(capi.F_ACTION)[0], capi.ACTMAP_MUSCLE_SIGMOID, 5)
        b.obs()
        out.append([b.read(f) for f in (capi.F_QPOS, capi.F_QVEL, capi.F_ACT, capi.F_OBS, capi.F_REWARD, capi.F_SITEXPOS)])
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_bad_env_is_contained():
    H.bad_env_is_contained(CASE)


def test_fused_bench_epilogue_equals_step_obs_autoreset():
    H.fused_epilogue_equals_stepwise(CASE)


@pytest.mark.parametrize("env_id", CASE.env_ids)
def test_every_id_steps(env_id):
    H.every_id_steps(CASE, env_id)


def test_env_api_matches_restatement():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make(ID, num_envs=1024, seed=4, as_torch=False, autoreset=False)
    env.reset()
    rng = np.random.default_rng(1)
    for _ in range(3):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (1024, 39)).astype(np.float32))
    b = env.batch
    ro, rr, rd, rs = pen_restate(b.read(capi.F_QPOS), b.read(capi.F_QVEL), b.read(capi.F_ACT), b.read(capi.F_SITEXPOS), obs[:, 23:26], env.dt)
    assert np.abs(obs - ro).max() < 1e-5 and np.abs(rew - rr).max() < 1e-3 * max(1.0, np.abs(rr).max())
    assert np.array_equal(term, rd) and np.array_equal(info["solved"], rs)


def test_refusals(pen):
    from myosuite_mjx_amd import capi, model as M
    hand = capi.HipBatch(capi.HipModel(M.load_asset("myohand_pose").blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="error -4"):
        hand.configure(quat_body=1)                               # not a TrackEnv-class model
    with pytest.raises(capi.MyoError, match="error -4"):
        hand.configure(task=capi.TASK_PEN, frame_skip=5, tip_sites=[0, 1, 2, 3, 4], pose_thd=0.95, far_th=0.075)
    key = capi.HipBatch(capi.HipModel(M.load_asset("myohand_keyturn").blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="error -4"):          # TRK class, but the last joints are not a pen's
        key.configure(task=capi.TASK_PEN, frame_skip=5, tip_sites=[0, 1, 2, 3, 4], pose_thd=0.95, far_th=0.075)
    b = capi.HipBatch(capi.HipModel(pen.blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="error -1"):          # no body selected
        b.read(capi.F_BODYQUAT)
    with pytest.raises(capi.MyoError, match="error -4"):
        b.configure(quat_body=pen.name2id("body", "Object"))      # has joints
    with pytest.raises(capi.MyoError, match="error -4"):
        b.configure(quat_body=pen.name2id("body", "distph2"))     # not a child of the world
    b.configure(quat_body=pen.name2id("body", "target"))
    assert np.array_equal(b.read(capi.F_BODYQUAT), np.tile([1, 0, 0, 0], (4, 1)).astype(np.float32))   # not started: compiled value
    for bad in (np.full((4, 4), np.nan, np.float32), np.tile([1, 1, 0, 0], (4, 1)).astype(np.float32)):
        with pytest.raises(capi.MyoError, match="error -1"):
            b.write(capi.F_BODYQUAT, bad)
    with pytest.raises(capi.MyoError, match="error -1"):
        b.set_body_quat_range(np.full(3, 0.5), np.full(3, -0.5))
    # a plane - cylinder pair outside the TrackEnv class is refused at load, never dropped
    a = dict(pen.arrays)
    a["hip_trk"] = np.zeros(3, np.int32)
    with pytest.raises(capi.MyoError, match="error -4"):
        capi.HipModel(M.Model(a, pen.names, pen.source).blob(), 0)


def test_guard_poisoned_build():
    H.rerun_file_against_poison_build(__file__, timeout=1500)
