"""GPU tests (pytest -m gpu) for myoHandKeyTurn{Fixed,Random}-v0 (envs/myo/myobase/key_turn_v0.py) on the TrackEnv-class ("TRK") step
kernel: MyoHand + a key on a hinge with friction loss, whose head (ellipsoid), shaft (capsule) and bit (box) collide with the hand.

  * HIP vs the float64 oracle after 1 and 10 substeps on states where fingertips touch the key (controls from the muscle sigmoid map, read
    back from MYO_F_CTRL), and the key's friction-loss row in the constraint set.  Tolerances as in tests/test_gpu_hold.py.
  * MYO_F_SITEXPOS against the oracle's site_xpos; observation / reward / done / solved against tests/keyturn_ref.py on 1024 envs.
  * reset draws over 4096 envs (key angle, key offset), determinism and sharding; the per-env key offset against the oracle on a blob whose
    key body was moved (Model.with_body_pos); the fused bench epilogue against step + obs + autoreset; the muscle-condition variants; the
    same file against the NaN-poisoned build."""
import numpy as np
import pytest

import hand_task_checks as H
from keyturn_ref import keyturn_restate

pytestmark = pytest.mark.gpu
SITES = ("keyhead", "IFtip", "THtip")
ID = "myoHandKeyTurnRandom-v0"


@pytest.fixture(scope="module")
def key():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_keyturn")


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
        H.forward_at(o, q)
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


CASE = H.TaskCase(stem="myohand_keyturn", task="keyturn", bench_id=ID, obs_dim=93, nsub=10, configure=_configure, extra_fields=("F_BODYPOS",),
                  env_ids=("myoSarcHandKeyTurnFixed-v0", "myoFatiHandKeyTurnRandom-v0", "myoReafHandKeyTurnRandom-v0"))


@pytest.mark.parametrize("nsub,tq,tv", [(1, 2e-5, 2e-2), (10, 2e-3, 0.2)])
def test_key_contact_parity(key, nsub, tq, tv):
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = key
    assert (m.nq, m.nv, m.nu) == (24, 24, 39) and list(m.hip_trk) == [0, 1, 1] and m.hip_fl[23, 0] == pytest.approx(0.02)
    o = Oracle(m.blob())
    N = 96
    q, v, act, a, d, hits = _contact_states(m, N, 3)
    kb = m.name2id("body", "key")
    b = H.new_batch(CASE, m, N)                           # a non-track task on the TRK instantiation
    fr = np.zeros(N, int)

    def oracle_for_env(e):
        return o if not d[e].any() else Oracle(m.with_body_pos(kb, m.body_pos[kb] + d[e].astype(np.float64)).blob())

    def extra_rows(e, oe):
        fr[e] = oe.nefc - 4 * oe.ncon        # rows beyond the condim-3 pyramids: limits and the key's friction loss

    eq, ev, nc, dg, fl, same = H.step_and_compare_with_oracle(
        m, b, {capi.F_QPOS: q, capi.F_QVEL: v, capi.F_ACT: act, capi.F_ACTION: a, capi.F_BODYPOS: d}, nsub, oracle_for_env, extra_rows)
    gq = b.read(capi.F_QPOS)
    assert np.allclose(b.read(capi.F_CTRL), 1 / (1 + np.exp(-5 * (a - 0.5))), atol=1e-6)    # base_v0.py:87-91
    assert (fr >= 1).all()
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
    N = 1024
    rng = np.random.default_rng(5)
    lo, hi = m.jnt_range[:23, 0], m.jnt_range[:23, 1]
    q = np.zeros((N, m.nq))
    q[:, :23] = lo + rng.uniform(0, 1, (N, 23)) * (hi - lo) * rng.uniform(0, 1, (N, 1))
    q[:, 23] = rng.uniform(-1, 7, N)
    q, v, act = q.astype(np.float32), rng.normal(0, 1, (N, m.nv)).astype(np.float32), rng.uniform(0, 1, (N, m.nu)).astype(np.float32)
    b = capi.HipBatch(capi.HipModel(m.blob(), 0), N)
    _configure(b, m, goal_th=2 * np.pi)
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act)):
        b.write(f, x)
    b.obs()
    sx, obs, rew, done, solved = (b.read(f) for f in (capi.F_SITEXPOS, capi.F_OBS, capi.F_REWARD, capi.F_DONE, capi.F_SOLVED))
    assert sx.shape == (N, 9) and obs.shape == (N, 93)
    o = Oracle(m.blob())
    for e in range(0, N, 8):
        assert np.abs(sx[e] - H.site_xpos(H.forward_at(o, q[e]), m, SITES)).max() < 5e-6, e
    ro, rr, rd, rs = keyturn_restate(q, v, act, sx, 0.02, 2 * np.pi)
    assert np.abs(obs - ro).max() < 1e-5
    assert np.abs(rew[:, 0] - rr).max() < 1e-3 * max(1.0, np.abs(rr).max())
    assert np.array_equal(done[:, 0] > 0, rd) and np.array_equal(solved[:, 0] > 0, rs)
    assert rd.any() and not rd.all() and rs.any() and not rs.all()        # both branches exercised


def test_reset_draws_and_sharding():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B = 4096

    def make_env(n, seed, off):
        return myo.make(ID, num_envs=n, seed=seed, env_offset=off, as_torch=False)

    env = make_env(B, H.SEED, 0)
    env.reset()
    q, off, obs = env.batch.read(capi.F_QPOS), env.body_pos, env.batch.read(capi.F_OBS)
    key_q = q[:, -1]
    assert np.abs(q[:, :-1]).max() == 0                                 # fully open hand
    assert key_q.min() >= -np.pi / 2 and key_q.max() <= np.pi / 2
    H.assert_uniform(key_q, -np.pi / 2, np.pi / 2)
    assert np.abs(off).max() <= 0.01 and off.min(axis=0).max() < -0.0095 and off.max(axis=0).min() > 0.0095
    for k in range(3):
        H.assert_uniform(off[:, k], -0.01, 0.01)
    assert np.allclose(obs[:, 46], key_q)
    H.assert_deterministic_and_sharded(make_env, lambda e: (e.batch.read(capi.F_QPOS), e.body_pos), B, (q, off))
    # the Fixed variant: key at 0, no offset started
    f = myo.make("myoHandKeyTurnFixed-v0", num_envs=64, seed=H.SEED, as_torch=False)
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
    ctrl = (1 / (1 + np.exp(-5 * (a - 0.5)))).astype(np.float32)
    kb = m.name2id("body", "key")
    osx = np.zeros((N, 9))

    def sites_after_forward(e, o):       # (the contacts were counted after the last substep, before this forward pass)
        o.forward()
        osx[e] = H.site_xpos(o, m, SITES)

    eq, ev, nc, dg, fl, same = H.step_and_compare_with_oracle(
        m, b, {capi.F_QPOS: q, capi.F_QVEL: v, capi.F_ACT: act, capi.F_BODYPOS: d, capi.F_CTRL: ctrl}, nsub,
        lambda e: Oracle(m.with_body_pos(kb, m.body_pos[kb] + d[e].astype(np.float64)).blob()), sites_after_forward)
    b.obs()
    gq, es = b.read(capi.F_QPOS), np.abs(b.read(capi.F_SITEXPOS) - osx).max(axis=1)
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


def test_bad_env_is_contained():
    H.bad_env_is_contained(CASE)


def test_fused_bench_epilogue_equals_step_obs_autoreset(key):
    """myo_bench_rollout's one-launch epilogue (keyturn_post_kernel) = step, myo_obs, myo_autoreset, myo_obs_reset_only."""
    H.fused_epilogue_equals_stepwise(CASE)


@pytest.mark.parametrize("env_id", CASE.env_ids)
def test_muscle_condition_variants_step(env_id):
    H.every_id_steps(CASE, env_id)


def test_env_api_matches_restatement():
    """A few env steps through the gym API: the returned rows are the restatement of the stepped state (envs not reset in between)."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make(ID, num_envs=1024, seed=4, as_torch=False, autoreset=False)
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
    H.rerun_file_against_poison_build(__file__, timeout=900)
