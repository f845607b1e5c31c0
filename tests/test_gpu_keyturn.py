"""GPU tests (pytest -m gpu) for myoHandKeyTurn{Fixed,Random}-v0 (envs/myo/myobase/key_turn_v0.py) on the TrackEnv-class ("TRK") step
kernel: MyoHand + a key on a hinge with friction loss, whose head (ellipsoid), shaft (capsule) and bit (box) collide with the hand.

  * HIP vs the float64 oracle after 1 and 10 substeps on states where fingertips touch the key (controls from the muscle sigmoid map, read
    back from MYO_F_CTRL), and the key's friction-loss row in the constraint set.  Tolerances as in tests/test_gpu_hold.py.
  * MYO_F_SITEXPOS against the oracle's site_xpos; observation / reward / done / solved against tests/keyturn_ref.py on 1024 envs.
  * reset draws over 4096 envs (key angle, key offset), determinism and sharding; the per-env key offset against the oracle on a blob whose
    key body was moved (Model.with_body_pos); the fused bench epilogue against step + obs + autoreset; the muscle-condition variants; the
    same file against the NaN-poisoned build."""
import os
import subprocess
import sys

import numpy as np
import pytest

from keyturn_ref import keyturn_restate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRK = "step_kernel_w<36,20,32,2,2,false,0,false,true>"
SITES = ("keyhead", "IFtip", "THtip")


@pytest.fixture(scope="module")
def key():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_keyturn")


def _sites(o, m):
    x = o.field("site_xpos").reshape(-1, 3)
    return np.concatenate([x[m.name2id("site", n)] for n in SITES])


def _key_geoms(m):
    kb = m.name2id("body", "key")
    return kb, [g for g in range(m.ngeom) if m.geom_bodyid[g] == kb]


def _hits(o, kg):
    return {int(c[k]) for c in o.contacts() for k in (7, 8) if int(c[k]) in kg}


def _contact_states(m, N, seed):
    """Hand poses (joints drawn over the middle of their ranges) in which the oracle finds hand-key contacts no deeper than 4 mm (random
    poses often sink a finger 1-3 cm into the key head, states no rollout reaches), key angle and velocities random.  In the compiled scene no finger reaches the key's box bit (10 cm out along the shaft): the second half of the states moves
    the key per env (MYO_F_BODYPOS offsets, the oracle on Model.with_body_pos blobs) so that the bit lies a few mm from a fingertip.
    Returns qpos, qvel, act, action, offsets and the key geoms each state touches."""
    from oracle.oracle import Oracle
    o = Oracle(m.blob())
    kb, kg = _key_geoms(m)
    box = [g for g in kg if int(m.geom_type[g]) == 6][0]
    tips = [m.name2id("site", n) for n in ("IFtip", "THtip", "MFtip")]
    rng = np.random.default_rng(seed)
    lo, hi = m.jnt_range[:23, 0], m.jnt_range[:23, 1]
    qs, ds, hits = [], [], []
    while len(qs) < N:
        q = np.zeros(m.nq)
        q[:23] = lo + rng.uniform(0.1, 0.9, 23) * (hi - lo)
        q[23] = rng.uniform(-1.5, 1.5)
        o.reset()
        o.set_state(qpos=q)
        o.forward()
        d = np.zeros(3)
        if len(qs) >= N // 2:      # bring the box bit to a fingertip
            tip = o.field("site_xpos").reshape(-1, 3)[tips[len(qs) % 3]]
            d = tip - o.field("geom_xpos").reshape(-1, 3)[box] + rng.normal(0, 0.006, 3)
            mo = Oracle(m.with_body_pos(kb, m.body_pos[kb] + d).blob())
            mo.set_state(qpos=q)
            mo.forward()
            h = _hits(mo, kg)
            if box not in h or min(c[0] for c in mo.contacts()) < -0.004:
                continue
        else:
            h = _hits(o, kg)
            if not h or min(c[0] for c in o.contacts()) < -0.004:
                continue
        qs.append(q)
        ds.append(d)
        hits.append(h)
    assert set().union(*hits) == set(kg)
    f32 = np.float32
    v = rng.normal(0, 0.5, (N, m.nv))
    return (np.array(qs).astype(f32), v.astype(f32), rng.uniform(0, 1, (N, m.nu)).astype(f32), rng.uniform(-1, 1, (N, m.nu)).astype(f32),
            np.array(ds).astype(f32), hits)


def _configure(b, m, goal_th=3.14):
    from myosuite_mjx_amd import capi
    b.configure(task=capi.TASK_KEYTURN, frame_skip=10, tip_sites=[m.name2id("site", n) for n in SITES], pose_thd=goal_th, near_th=0.030,
                far_th=0.1, w_pose=1.0, w_reach=10.0, w_act_reg=1.0, w_bonus=4.0, w_penalty=25.0, init_qpos=np.zeros(m.nq))


@pytest.mark.parametrize("nsub,tq,tv", [(1, 2e-5, 2e-2), (10, 2e-3, 0.2)])
def test_key_contact_parity(key, nsub, tq, tv):
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = key
    assert (m.nq, m.nv, m.nu) == (24, 24, 39) and list(m.hip_trk) == [0, 1, 1] and m.hip_fl[23, 0] == pytest.approx(0.02)
    hm = capi.HipModel(m.blob(), 0)
    o = Oracle(m.blob())
    N = 96
    q, v, act, a, d, hits = _contact_states(m, N, 3)
    kb = m.name2id("body", "key")
    b = capi.HipBatch(hm, N)
    _configure(b, m)                                      # a non-track task on the TRK instantiation
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act), (capi.F_ACTION, a), (capi.F_BODYPOS, d)):
        b.write(f, x)
    b.step(b.field_ptr(capi.F_ACTION)[0], capi.ACTMAP_MUSCLE_SIGMOID, nsub)
    assert b.last_kernel_name() == TRK
    gq, gv, ctrl, dg, fl = b.read(capi.F_QPOS), b.read(capi.F_QVEL), b.read(capi.F_CTRL), b.read(capi.F_DIAG), b.status()
    assert np.allclose(ctrl, 1 / (1 + np.exp(-5 * (a - 0.5))), atol=1e-6)    # base_v0.py:87-91
    eq, ev, nc, fr = np.zeros(N), np.zeros(N), np.zeros(N, int), np.zeros(N, int)
    for e in range(N):
        oe = o if not d[e].any() else Oracle(m.with_body_pos(kb, m.body_pos[kb] + d[e].astype(np.float64)).blob())
        oe.reset()
        oe.set_state(qpos=q[e], qvel=v[e], act=act[e], ctrl=ctrl[e])
        assert oe.step(nsub) == 0
        eq[e], ev[e], nc[e] = np.abs(gq[e] - oe.field("qpos")).max(), np.abs(gv[e] - oe.field("qvel")).max(), oe.ncon
        fr[e] = oe.nefc - 4 * oe.ncon        # rows beyond the condim-3 pyramids: limits and the key's friction loss
    assert (fr >= 1).all()
    same = (fl == 0) & (dg[:, 1] == nc)
    assert same.mean() > 0.85
    box = [g for g in range(m.ngeom) if m.geom_bodyid[g] == kb and int(m.geom_type[g]) == 6][0]
    assert sum(1 for e in range(N) if same[e] and box in hits[e]) >= N // 4            # box-bit contacts among the compared envs
    w = int(np.argmax(np.where(same, eq, 0)))
    assert eq[same].max() < tq and ev[same].max() < tv, (eq[same].max(), ev[same].max(), w, sorted(hits[w]), d[w].tolist(), int(nc[w]), np.sort(eq[same])[-5:].tolist())
    assert np.median(eq[same]) < (2e-6 if nsub == 1 else 3e-5) and np.median(ev[same]) < (2e-3 if nsub == 1 else 5e-3), (np.median(eq[same]), np.median(ev[same]))
    assert np.abs(gq[:, 23] - q[:, 23]).max() > 1e-4     # the key moves


def test_site_positions_and_restatement(key):
    """MYO_F_SITEXPOS against the oracle's site_xpos, and the observation row / reward / done / solved against the float64 restatement,
    on 1024 envs whose states span the thresholds (key angles past pi/2, pi and goal_th; tips near and far from the head)."""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = key
    hm = capi.HipModel(m.blob(), 0)
    N = 1024
    rng = np.random.default_rng(5)
    lo, hi = m.jnt_range[:23, 0], m.jnt_range[:23, 1]
    q = np.zeros((N, m.nq))
    q[:, :23] = lo + rng.uniform(0, 1, (N, 23)) * (hi - lo) * rng.uniform(0, 1, (N, 1))
    q[:, 23] = rng.uniform(-1, 7, N)
    q, v, act = q.astype(np.float32), rng.normal(0, 1, (N, m.nv)).astype(np.float32), rng.uniform(0, 1, (N, m.nu)).astype(np.float32)
    b = capi.HipBatch(hm, N)
    _configure(b, m, goal_th=2 * np.pi)
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act)):
        b.write(f, x)
    b.obs()
    sx, obs, rew, done, solved = (b.read(f) for f in (capi.F_SITEXPOS, capi.F_OBS, capi.F_REWARD, capi.F_DONE, capi.F_SOLVED))
    assert sx.shape == (N, 9) and obs.shape == (N, 93)
    o = Oracle(m.blob())
    for e in range(0, N, 8):
        o.reset()
        o.set_state(qpos=q[e])
        o.forward()
        assert np.abs(sx[e] - _sites(o, m)).max() < 5e-6, e
    ro, rr, rd, rs = keyturn_restate(q, v, act, sx, 0.02, 2 * np.pi)
    assert np.abs(obs - ro).max() < 1e-5
    assert np.abs(rew[:, 0] - rr).max() < 1e-3 * max(1.0, np.abs(rr).max())
    assert np.array_equal(done[:, 0] > 0, rd) and np.array_equal(solved[:, 0] > 0, rs)
    assert rd.any() and not rd.all() and rs.any() and not rs.all()        # both branches exercised


def test_reset_draws_and_sharding():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B = 4096
    env = myo.make("myoHandKeyTurnRandom-v0", num_envs=B, seed=7, as_torch=False)
    env.reset()
    q, off, obs = env.batch.read(capi.F_QPOS), env.body_pos, env.batch.read(capi.F_OBS)
    key_q = q[:, -1]
    assert np.abs(q[:, :-1]).max() == 0                                 # fully open hand
    assert key_q.min() >= -np.pi / 2 and key_q.max() <= np.pi / 2
    h = np.histogram(key_q, bins=8, range=(-np.pi / 2, np.pi / 2))[0]
    assert np.abs(h - B / 8).max() < 5 * np.sqrt(B / 8)
    assert np.abs(off).max() <= 0.01 and off.min(axis=0).max() < -0.0095 and off.max(axis=0).min() > 0.0095
    for k in range(3):
        hk = np.histogram(off[:, k], bins=8, range=(-0.01, 0.01))[0]
        assert np.abs(hk - B / 8).max() < 5 * np.sqrt(B / 8)
    assert np.allclose(obs[:, 46], key_q)
    # deterministic per seed, different across seeds
    env2 = myo.make("myoHandKeyTurnRandom-v0", num_envs=B, seed=7, as_torch=False)
    env2.reset()
    assert np.array_equal(env2.batch.read(capi.F_QPOS), q) and np.array_equal(env2.body_pos, off)
    env2.reset(seed=8)
    assert not np.array_equal(env2.body_pos, off)
    # two shards (env_offset 0 and B / 2) reproduce the single batch
    for off_e in (0, B // 2):
        s = myo.make("myoHandKeyTurnRandom-v0", num_envs=B // 2, seed=7, env_offset=off_e, as_torch=False)
        s.reset()
        assert np.array_equal(s.batch.read(capi.F_QPOS), q[off_e:off_e + B // 2])
        assert np.array_equal(s.body_pos, off[off_e:off_e + B // 2])
    # the Fixed variant: key at 0, no offset started
    f = myo.make("myoHandKeyTurnFixed-v0", num_envs=64, seed=7, as_torch=False)
    f.reset()
    assert not f.batch.read(capi.F_QPOS).any() and not f.body_pos.any() and not f.batch.read(capi.F_BODYPOS_RANGE).any()


@pytest.mark.parametrize("nsub", [1, 10])
def test_key_offset_against_moved_blob(key, nsub):
    """Per-env key offsets (MYO_F_BODYPOS) against the oracle on blobs whose key body was moved by the same amount."""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = key
    hm = capi.HipModel(m.blob(), 0)
    N = 32
    q, v, act, a, _, _ = _contact_states(m, 2 * N, 9)
    q, v, act, a = q[:N], v[:N], act[:N], a[:N]          # the states of the compiled scene
    rng = np.random.default_rng(2)
    d = rng.uniform(-0.01, 0.01, (N, 3)).astype(np.float32)
    b = capi.HipBatch(hm, N)
    _configure(b, m)
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act), (capi.F_BODYPOS, d)):
        b.write(f, x)
    ctrl = (1 / (1 + np.exp(-5 * (a - 0.5)))).astype(np.float32)
    b.write(capi.F_CTRL, ctrl)
    b.step(None, capi.ACTMAP_NONE, nsub)
    b.obs()
    assert b.last_kernel_name() == TRK
    gq, gv, sx, dg, fl = b.read(capi.F_QPOS), b.read(capi.F_QVEL), b.read(capi.F_SITEXPOS), b.read(capi.F_DIAG), b.status()
    kb = m.name2id("body", "key")
    eq, ev, es, same = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N, bool)
    for e in range(N):
        mm = m.with_body_pos(kb, m.body_pos[kb] + d[e].astype(np.float64))
        o = Oracle(mm.blob())
        o.set_state(qpos=q[e], qvel=v[e], act=act[e], ctrl=ctrl[e])
        assert o.step(nsub) == 0
        same[e] = fl[e] == 0 and dg[e, 1] == o.ncon         # contacts of the last substep, before the post-step forward pass
        o.forward()
        eq[e], ev[e] = np.abs(gq[e] - o.field("qpos")).max(), np.abs(gv[e] - o.field("qvel")).max()
        es[e] = np.abs(sx[e] - _sites(o, m)).max()
    tq, tv = (2e-5, 2e-2) if nsub == 1 else (2e-3, 0.2)
    assert same.mean() > 0.8 and eq[same].max() < tq and ev[same].max() < tv, (eq[same].max(), ev[same].max())
    assert es[same].max() < (1e-5 if nsub == 1 else 5e-4)
    # the offset moves the key: the same states without it differ
    b2 = capi.HipBatch(hm, N)
    _configure(b2, m)
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act), (capi.F_CTRL, ctrl)):
        b2.write(f, x)
    b2.step(None, capi.ACTMAP_NONE, nsub)
    assert np.abs(b2.read(capi.F_QPOS) - gq).max() > 1e-4


def test_offset_on_with_zero_offsets_is_offset_off(key):
    from myosuite_mjx_amd import capi
    m = key
    hm = capi.HipModel(m.blob(), 0)
    N = 64
    q, v, act, a, _, _ = _contact_states(m, 2 * N, 4)
    q, v, act, a = q[:N], v[:N], act[:N], a[:N]
    out = []
    for on in (False, True):
        b = capi.HipBatch(hm, N)
        _configure(b, m)
        for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act), (capi.F_ACTION, a)):
            b.write(f, x)
        if on:
            b.write(capi.F_BODYPOS, np.zeros((N, 3), np.float32))
        for _ in range(3):
            b.step(b.field_ptr(capi.F_ACTION)[0], capi.ACTMAP_MUSCLE_SIGMOID, 10)
        b.obs()
        out.append([b.read(f) for f in (capi.F_QPOS, capi.F_QVEL, capi.F_ACT, capi.F_OBS, capi.F_REWARD)])
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_fused_bench_epilogue_equals_step_obs_autoreset(key):
    """myo_bench_rollout's one-launch epilogue (keyturn_post_kernel) = step, myo_obs, myo_autoreset, myo_obs_reset_only."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B, seed, T = 512, 3, 5
    envs = [myo.make("myoHandKeyTurnRandom-v0", num_envs=B, seed=1, as_torch=False) for _ in range(2)]
    for e in envs:
        e.reset()
    a, r = envs
    a.batch.bench_rollout(T, 10, seed=seed, mode=capi.BENCH_OBS | capi.BENCH_FRESH_ACTIONS | capi.BENCH_AUTORESET, max_episode_steps=2)
    ptr = r.batch.field_ptr(capi.F_ACTION)[0]
    for t in range(T):
        r.batch.random_action(ptr, seed, t)
        r.batch.step(ptr, capi.ACTMAP_MUSCLE_SIGMOID, 10)
        r.batch.obs()
        r.batch.autoreset(2, seed)
        r.batch.obs_reset_only()
    for f in (capi.F_QPOS, capi.F_QVEL, capi.F_ACT, capi.F_OBS, capi.F_REWARD, capi.F_DONE, capi.F_SOLVED, capi.F_ELAPSED, capi.F_SITEXPOS,
              capi.F_BODYPOS):
        assert np.array_equal(a.batch.read(f), r.batch.read(f)), f
    assert a.batch.read(capi.F_ELAPSED).max() <= 2


@pytest.mark.parametrize("env_id", ["myoSarcHandKeyTurnFixed-v0", "myoFatiHandKeyTurnRandom-v0", "myoReafHandKeyTurnRandom-v0"])
def test_muscle_condition_variants_step(env_id):
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make(env_id, num_envs=256, seed=2, as_torch=False)
    obs = env.reset()
    assert obs.shape == (256, 93)
    rng = np.random.default_rng(0)
    for _ in range(5):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (256, 39)).astype(np.float32))
        assert np.isfinite(obs).all() and np.isfinite(rew).all()
    assert env.batch.last_kernel_name() == TRK and not env.status().any()
    assert np.abs(env.batch.read(capi.F_ACT)).max() > 0


def test_env_api_matches_restatement():
    """A few env steps through the gym API: the returned rows are the restatement of the stepped state (envs not reset in between)."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make("myoHandKeyTurnRandom-v0", num_envs=1024, seed=4, as_torch=False, autoreset=False)
    env.reset()
    rng = np.random.default_rng(1)
    for _ in range(3):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (1024, 39)).astype(np.float32))
    b = env.batch
    ro, rr, rd, rs = keyturn_restate(b.read(capi.F_QPOS), b.read(capi.F_QVEL), b.read(capi.F_ACT), b.read(capi.F_SITEXPOS), env.dt, 2 * np.pi)
    assert np.abs(obs - ro).max() < 1e-5 and np.abs(rew - rr).max() < 1e-3 * max(1.0, np.abs(rr).max())
    assert np.array_equal(term, rd) and np.array_equal(info["solved"], rs)


def test_refusals(key):
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi, model as M
    hand = capi.HipModel(M.load_asset("myohand_pose").blob(), 0)
    b = capi.HipBatch(hand, 4)
    for f in (capi.F_BODYPOS, capi.F_BODYPOS_RANGE):      # not a TrackEnv-class model
        with pytest.raises(capi.MyoError, match="error -4"):
            b.field_ptr(f)
    with pytest.raises(capi.MyoError, match="error -4"):
        b.configure(task=capi.TASK_KEYTURN, frame_skip=10, tip_sites=[0, 1, 2], pose_thd=3.14, near_th=0.03, far_th=0.1)
    air = M.load_asset("myohand_object_airplane")      # TRK class; its last joint belongs to a root body with six joints, not one hinge
    ab = capi.HipBatch(capi.HipModel(air.blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="error -4"):
        ab.configure(task=capi.TASK_KEYTURN, frame_skip=10, tip_sites=[0, 1, 2], pose_thd=3.14, near_th=0.03, far_th=0.1)
    off = np.full((4, 3), 0.005, np.float32)          # ... but that body is a root body: the per-env offset is accepted
    ab.write(capi.F_BODYPOS, off)
    assert np.array_equal(ab.read(capi.F_BODYPOS), off)
    kb = capi.HipBatch(capi.HipModel(key.blob(), 0), 4)
    assert not kb.read(capi.F_BODYPOS).any()           # not started: zeros
    for bad in (np.full((4, 3), np.nan, np.float32),):
        with pytest.raises(capi.MyoError, match="error -1"):
            kb.write(capi.F_BODYPOS, bad)
    with pytest.raises(capi.MyoError, match="error -1"):
        kb.set_body_pos_range(np.full(3, 0.01), np.full(3, -0.01))
    with pytest.raises(TypeError):
        myo.make("myoHandPoseFixed-v0", num_envs=2, goal_th=1.0)


def test_guard_poisoned_build():
    """This file once more against libmyo_hip_poison.so (NaN-filled LDS, scratch and registers before every step launch)."""
    lib = os.path.join(ROOT, "myosuite_mjx_amd", "libmyo_hip_poison.so")
    assert os.path.exists(lib), "libmyo_hip_poison.so is missing: run __graft_entry__.build()"
    env = dict(os.environ, MYO_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not guard",
                        "tests/test_gpu_keyturn.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout
