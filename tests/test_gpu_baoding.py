"""GPU tests (pytest -m gpu) for myoChallengeBaodingP1-v1 (envs/myo/myochallenge/baoding_v1.py) on the TrackEnv-class ("TRK") step
kernel: MyoHand + two free balls (two free joints in one model, plane - sphere pairs).

  * HIP vs the float64 oracle after 1 and 10 substeps: ball - palm (oracle rollouts from the palm-up start), ball - ball, ball - pedestal,
    ball - floor (plane - sphere) and two spinning balls in free flight; qpos (both quaternions), qvel and contact counts.
  * A 40-step rollout env by env: every env step of HIP against the oracle restarted from HIP's state.
  * MYO_F_SITEXPOS, observation, reward, done and solved against tests/baoding_ref.py, the targets at steps 1, 2 and 200 against the
    oracle on models whose target sites are moved as the reference moves them.
  * Reset draws over 4096 envs and two shards; the fused bench epilogue; the muscle-condition variants; refusals; the same file against the
    NaN-poisoned build."""
import numpy as np
import pytest

import hand_task_checks as H
from baoding_ref import DT, baoding_restate, target_xy

pytestmark = pytest.mark.gpu
SITES = ("ball1_site", "ball2_site", "target1_site", "target2_site")
ID = "myoChallengeBaodingP1-v1"
R = 0.022


@pytest.fixture(scope="module")
def bd():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_baoding")


def _init_q(m):
    q = np.array(m.qpos0, float)
    q[:-14] = 0
    q[0] = -1.57
    return q


def _configure(b, m, params=(np.pi / 4, 1.0, 0.025, 0.028, 5.0)):
    from myosuite_mjx_amd import capi
    b.configure(task=capi.TASK_BAODING, frame_skip=10, target_generate=1, target_lo=list(params), target_hi=list(params), init_qpos=_init_q(m),
                tip_sites=[m.name2id("site", n) for n in SITES], pose_thd=0.015, far_th=1.25, w_pose=5.0, w_reach=5.0)


CASE = H.TaskCase(stem="myohand_baoding", task="baoding", bench_id=ID, obs_dim=47, nsub=10, configure=_configure, extra_fields=("F_TARGET",),
                  make_kwargs=dict(task_choice="random"), env_ids=(ID, "myoSarcChallengeBaodingP1-v1", "myoFatiChallengeBaodingP1-v1"))


def _unit(rng, n):
    q = rng.normal(0, 1, (n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _states(m, kind, N, seed):
    """qpos, qvel and the contact pairs each state has, in one family."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(seed)
    o = Oracle(m.blob())
    g1, g2 = m.name2id("geom", "ball1"), m.name2id("geom", "ball2")
    qs, vs, tags = [], [], []
    tries = 0
    if kind == "palm":      # oracle rollouts from the palm-up start (zero control): the balls rolling on the palm
        pool = []
        for r in range(4):
            o.reset()
            q = _init_q(m)
            q[1:23] += rng.normal(0, 0.05, 22)
            o.set_state(qpos=q)
            for k in range(30):
                o.set_state(ctrl=rng.uniform(0, 0.3, m.nu))
                o.step(10)
                pool.append((o.field("qpos").copy(), o.field("qvel").copy()))
    while len(qs) < N:
        tries += 1
        assert tries < 200 * N, kind
        q = _init_q(m)
        q[1:23] += rng.normal(0, 0.02, 22)
        v = np.zeros(m.nv)
        v[:23] = rng.normal(0, 0.3, 23)
        q[26:30], q[33:37] = _unit(rng, 2)
        v[23:26], v[29:32] = rng.normal(0, 0.1, (2, 3))
        v[26:29], v[32:35] = rng.normal(0, 3.0, (2, 3))
        if kind == "palm":
            q, v = (x.copy() for x in pool[int(rng.integers(len(pool)))])
            v[23:] += rng.normal(0, 0.02, 12)
        elif kind == "ballball":
            c = np.array([0.5, 0.5, 0.8]) + rng.normal(0, 0.05, 3)
            d = rng.normal(0, 1, 3)
            q[23:26], q[30:33] = c, c + d / np.linalg.norm(d) * (2 * R - rng.uniform(0.0, 0.002))
        elif kind == "pedestal":
            q[23:26] = [rng.uniform(-0.5, 0.5), rng.uniform(0.2, 0.6), 0.015 + R - rng.uniform(0.0, 0.002)]
            q[30:33] = [rng.uniform(-0.5, 0.5), rng.uniform(-0.6, -0.2), 0.015 + R - rng.uniform(0.0, 0.002)]
        elif kind == "floor":
            q[23:26] = [rng.uniform(-0.5, 0.5), 1.5, -0.4 + R - rng.uniform(0.0, 0.002)]
            q[30:33] = [rng.uniform(-0.5, 0.5), -1.5, -0.4 + R - rng.uniform(0.0, 0.002)]
        else:               # free flight, spinning fast
            q[23:26], q[30:33] = [0.5, 0.5, 0.8], [0.6, 0.4, 0.9]
            v[26:29], v[32:35] = rng.normal(0, 20.0, (2, 3))
        pairs = {frozenset((int(c[7]), int(c[8]))) for c in H.forward_at(o, q).contacts()}
        balls = {p for p in pairs if g1 in p or g2 in p}
        if kind == "flight":
            if balls:
                continue
        elif kind == "palm":
            if not any(len(p - {g1, g2}) == 1 and not (p & {0, 1}) for p in balls):
                continue
        elif kind == "ballball":
            if frozenset((g1, g2)) not in pairs:
                continue
        elif not (frozenset((0 if kind == "floor" else 1, g1)) in pairs and frozenset((0 if kind == "floor" else 1, g2)) in pairs):
            continue
        qs.append(q)
        vs.append(v)
        tags.append(pairs)
    return np.array(qs).astype(np.float32), np.array(vs).astype(np.float32), tags


@pytest.mark.parametrize("kind", ["palm", "ballball", "pedestal", "floor", "flight"])
@pytest.mark.parametrize("nsub,tq,tv", [(1, 2e-5, 2e-2), (10, 2e-3, 0.2)])
def test_contact_parity(bd, kind, nsub, tq, tv):
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = bd
    N = 32
    q, v, tags = _states(m, kind, N, {"palm": 1, "ballball": 2, "pedestal": 3, "floor": 4, "flight": 5}[kind])
    rng = np.random.default_rng(9)
    act, ctrl = rng.uniform(0, 1, (N, m.nu)).astype(np.float32), rng.uniform(0, 1, (N, m.nu)).astype(np.float32)
    b = H.new_batch(CASE, m, N)
    o = Oracle(m.blob())
    g1, g2 = m.name2id("geom", "ball1"), m.name2id("geom", "ball2")
    ball_con = np.zeros(N, int)

    def count_ball_contacts(e, oe):
        ball_con[e] = sum(1 for c in oe.contacts() if {int(c[7]), int(c[8])} & {g1, g2})

    eq, ev, nc, dg, fl, same = H.step_and_compare_with_oracle(m, b, {capi.F_QPOS: q, capi.F_QVEL: v, capi.F_ACT: act, capi.F_CTRL: ctrl}, nsub,
                                                              lambda e: o, count_ball_contacts)
    gq = b.read(capi.F_QPOS)
    for a in (26, 33):                                                # both quaternions stay unit
        assert np.abs(np.linalg.norm(gq[:, a:a + 4], axis=1) - 1).max() < 1e-5
    assert same.mean() > 0.8, (same.mean(), dg[:, 1].tolist(), nc.tolist())
    w = int(np.argmax(np.where(same, eq, 0)))
    assert eq[same].max() < tq and ev[same].max() < tv, (eq[same].max(), ev[same].max(), w, [sorted(p) for p in tags[w]], int(nc[w]))
    if kind == "flight":                           # (the moving hand may touch itself)
        assert not ball_con.any()
    elif nsub == 1:                                # (after ten substeps a ball may have bounced off)
        assert (ball_con[same] >= (2 if kind in ("pedestal", "floor") else 1)).all()
    assert np.abs(gq - q).max() > 1e-6


def test_rollout_env_by_env(bd):
    """40 env steps, palm up, zero control, from jittered starts: every step of every env against the oracle restarted from HIP's state
    before the step; the balls roll off the palm and ball 2 falls below drop_th near step 33 in HIP as in the oracle's own rollout."""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = bd
    N = 16
    rng = np.random.default_rng(11)
    q0 = np.tile(_init_q(m), (N, 1))
    q0[1:, 23:26] += rng.normal(0, 0.002, (N - 1, 3))
    q0 = q0.astype(np.float32)
    b = H.new_batch(CASE, m, N)
    zero = np.zeros((N, m.nu), np.float32)
    for f, x in ((capi.F_QPOS, q0), (capi.F_QVEL, np.zeros((N, m.nv), np.float32)), (capi.F_ACT, zero), (capi.F_CTRL, zero)):
        b.write(f, x)
    o = Oracle(m.blob())
    worst = 0.0
    z2 = np.zeros((40, N))
    for k in range(40):
        q, v, act = b.read(capi.F_QPOS), b.read(capi.F_QVEL), b.read(capi.F_ACT)
        b.step(None, capi.ACTMAP_NONE, 10)
        gq = b.read(capi.F_QPOS)
        z2[k] = gq[:, 32]
        assert not b.status().any()
        for e in range(N):
            o.reset()
            o.set_state(qpos=q[e], qvel=v[e], act=act[e], ctrl=zero[e])
            assert o.step(10) == 0
            worst = max(worst, np.abs(gq[e] - o.field("qpos")).max())
    assert worst < 2e-3, worst
    o.reset()
    o.set_state(qpos=q0[0])
    ref = []
    for k in range(40):
        o.step(10)
        ref.append(o.field("qpos")[32])
    drop_h, drop_o = int(np.argmax(z2[:, 0] < 1.25)), int(np.argmax(np.array(ref) < 1.25))
    assert 28 <= drop_o <= 36 and abs(drop_h - drop_o) <= 2, (drop_h, drop_o)
    assert np.abs(z2[:, 0] - np.array(ref))[:25].max() < 5e-3


def _with_targets(m, xy):
    from myosuite_mjx_amd import model as M
    from myosuite_mjx_amd.lowering import lower
    from myosuite_mjx_amd.mjcf import CompiledModel
    a = {k: np.array(v, copy=True) for k, v in m.arrays.items() if not k.startswith("hip_")}
    for t, n in enumerate(("target1_site", "target2_site")):
        a["site_pos"][m.name2id("site", n), :2] = xy[t]
    cm = CompiledModel(arrays=a, names=m.names)
    lower(cm)
    return M.Model(cm.arrays, m.names).blob()


def test_sites_observation_and_restatement(bd):
    """1024 envs with random hand poses, ball positions around the targets, goal parameters and step counters (0, 1, 2, 200 and random):
    MYO_F_SITEXPOS against the oracle on models with the targets moved (every 32nd env), the row / reward / done / solved against the
    restatement everywhere."""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = bd
    N = 1024
    rng = np.random.default_rng(5)
    lo, hi = m.jnt_range[:23, 0], m.jnt_range[:23, 1]
    q = np.tile(_init_q(m), (N, 1))
    q[:, 1:23] = lo[1:] + rng.uniform(0, 0.6, (N, 22)) * (hi[1:] - lo[1:])
    q[:, 0] = rng.uniform(-1.7, -1.4, N)
    q[:, 26:30], q[:, 33:37] = _unit(rng, N), _unit(rng, N)
    q[:, 23:26] += rng.normal(0, 0.02, (N, 3))
    q[:, 30:33] += rng.normal(0, 0.02, (N, 3))
    q[::7, 32] = 1.2                                                     # some balls dropped
    v = rng.normal(0, 1, (N, m.nv))
    params = np.stack([rng.uniform(0, 2 * np.pi, N), rng.integers(-1, 2, N), rng.uniform(0.02, 0.03, N), rng.uniform(0.022, 0.032, N),
                       rng.uniform(4, 6, N)], 1)
    el = rng.integers(0, 201, N)
    el[:4] = (0, 1, 2, 200)
    el[4:8] = (1, 2, 200, 1)
    q, v, params = q.astype(np.float32), v.astype(np.float32), params.astype(np.float32)
    b = H.new_batch(CASE, m, N)
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_TARGET, params), (capi.F_ELAPSED, el.astype(np.int32))):
        b.write(f, x)
    b.obs()
    sx, obs, rew, done, solved = (b.read(f) for f in (capi.F_SITEXPOS, capi.F_OBS, capi.F_REWARD, capi.F_DONE, capi.F_SOLVED))
    assert sx.shape == (N, 12) and obs.shape == (N, 47)
    sid = [m.name2id("site", n) for n in SITES]
    for e in list(range(8)) + list(range(8, N, 32)):
        o = Oracle(_with_targets(m, target_xy(params[e].astype(np.float64), el[e])[0]))
        x = H.forward_at(o, q[e]).field("site_xpos").reshape(-1, 3)[sid].reshape(12)
        assert np.abs(sx[e] - x).max() < 5e-6, (e, el[e], sx[e] - x)
    ro, rr, rd, rs = baoding_restate(q, v, sx, DT)
    assert np.abs(obs - ro).max() < 1e-5
    assert np.abs(rew[:, 0] - rr).max() < 1e-4
    assert np.array_equal(done[:, 0] > 0, rd) and np.array_equal(solved[:, 0] > 0, rs)
    assert rd.any() and not rd.all()
    # solved: balls put on their targets
    q2 = q.copy()
    q2[:, 23:26], q2[:, 30:33] = sx[:, 6:9] + 0.005, sx[:, 9:12] - 0.005
    q2[:, 26:30] = q2[:, 33:37] = [1, 0, 0, 0]
    b.write(capi.F_QPOS, q2)
    b.obs()
    sx2 = b.read(capi.F_SITEXPOS)
    ro, rr, rd, rs = baoding_restate(q2, v, sx2, DT)
    assert np.array_equal(b.read(capi.F_SOLVED)[:, 0] > 0, rs) and rs.mean() > 0.5 and np.array_equal(b.read(capi.F_DONE)[:, 0] > 0, rd)


def test_reset_draws_and_sharding():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B = 4096

    def make_env(n, seed, off):
        return myo.make(ID, num_envs=n, seed=seed, env_offset=off, as_torch=False, task_choice="random", goal_time_period=(4, 6),
                        goal_xrange=(0.02, 0.03), goal_yrange=(0.022, 0.032))

    env = make_env(B, H.SEED, 0)
    obs = env.reset()
    m = env.mjmodel
    assert np.array_equal(env.batch.read(capi.F_QPOS), np.tile(_init_q(m).astype(np.float32), (B, 1)))
    g = env.goal_params
    assert g.shape == (B, 5)
    assert g[:, 0].min() >= 0 and g[:, 0].max() < 2 * np.pi
    H.assert_uniform(g[:, 0], 0, 2 * np.pi)
    assert set(np.unique(g[:, 1]).tolist()) == {-1.0, 0.0, 1.0}
    assert np.abs(np.bincount((g[:, 1] + 1).astype(int)) - B / 3).max() < 5 * np.sqrt(B / 3)
    for c, (a, z) in ((2, (0.02, 0.03)), (3, (0.022, 0.032)), (4, (4.0, 6.0))):
        assert g[:, c].min() >= a - 1e-6 and g[:, c].max() <= z + 1e-6 and g[:, c].std() > 0.2 * (z - a)
    # the first observation shows goal[0]
    xy = target_xy(g.astype(np.float64), 0)
    sx = env.batch.read(capi.F_SITEXPOS)
    assert np.abs(obs[:, 35:38] - sx[:, 6:9]).max() == 0 and np.abs(obs[:, 38:41] - sx[:, 9:12]).max() == 0
    d = np.linalg.norm(sx[:, 6:9] - sx[:, 9:12], axis=1)                   # the targets are opposite on the ellipse
    assert np.abs(d - 2 * np.hypot(g[:, 2] * np.cos(g[:, 0]), g[:, 3] * np.sin(g[:, 0]))).max() < 1e-5
    assert xy.shape == (B, 2, 2)
    H.assert_deterministic_and_sharded(make_env, lambda e: (e.goal_params,), B, (g,))
    f = myo.make(ID, num_envs=64, seed=H.SEED, as_torch=False)
    f.reset()
    assert np.array_equal(f.goal_params, np.tile(np.array([np.pi / 4, 1, 0.025, 0.028, 5], np.float32), (64, 1)))


def test_targets_follow_the_goal_trajectory():
    """The env API: the targets after steps 1, 2 and 200 (the last step of an episode) are goal[0], goal[1] and goal[199]."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B = 64
    env = myo.make("myoChallengeBaodingP1-v1", num_envs=B, seed=3, as_torch=False, autoreset=False)
    env.reset()
    rng = np.random.default_rng(2)
    p = env.goal_params.astype(np.float64)
    for k in range(1, 201):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (B, 39)).astype(np.float32))
        if k in (1, 2, 200):
            sx = env.batch.read(capi.F_SITEXPOS)
            ro, rr, rd, rs = baoding_restate(env.batch.read(capi.F_QPOS), env.batch.read(capi.F_QVEL), sx, DT)
            assert np.abs(obs - ro).max() < 1e-5 and np.abs(rew - rr).max() < 1e-4 and np.array_equal(term, rd)
            assert (env.batch.read(capi.F_ELAPSED)[:, 0] == k).all()
            ang = p[:, 1] * 2 * np.pi * (k - 1) * DT / p[:, 4] + p[:, 0]
            r = np.linalg.norm(sx[:, 6:9] - sx[:, 9:12], axis=1)
            assert np.abs(r - 2 * np.hypot(p[:, 2] * np.cos(ang), p[:, 3] * np.sin(ang))).max() < 1e-5


def test_bad_env_is_contained():
    H.bad_env_is_contained(CASE)


def test_fused_bench_epilogue_equals_step_obs_autoreset():
    H.fused_epilogue_equals_stepwise(CASE)


@pytest.mark.parametrize("env_id", CASE.env_ids)
def test_every_id_steps(env_id):
    H.every_id_steps(CASE, env_id)


def test_goal_params_view_is_zero_copy():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make("myoChallengeBaodingP1-v1", num_envs=8, seed=2)
    env.reset()
    g = env.goal_params
    g[:, 0] = 1.0
    assert np.allclose(env.batch.read(capi.F_TARGET)[:, 0], 1.0)
    env.goal_params = [0.5, -1.0, 0.02, 0.03, 4.0]
    assert np.allclose(env.batch.read(capi.F_TARGET), [0.5, -1.0, 0.02, 0.03, 4.0])


def test_refusals(bd):
    from myosuite_mjx_amd import capi, model as M
    sites = [bd.name2id("site", n) for n in SITES]
    for stem in ("myohand_pose", "myohand_pen", "myohand_hold"):          # not TRK / no two free joints
        h = capi.HipBatch(capi.HipModel(M.load_asset(stem).blob(), 0), 4)
        with pytest.raises(capi.MyoError, match="error -4"):
            h.configure(task=capi.TASK_BAODING, frame_skip=10, target_lo=[0.0] * 5, tip_sites=[0, 1, 2, 3], pose_thd=0.015, far_th=1.25)
    b = capi.HipBatch(capi.HipModel(bd.blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="error -1"):                # five goal parameters
        b.configure(task=capi.TASK_BAODING, frame_skip=10, target_lo=[0.0] * 3, tip_sites=sites, pose_thd=0.015, far_th=1.25)
    with pytest.raises(capi.MyoError, match="error -4"):                # the ball sites swapped with the targets
        b.configure(task=capi.TASK_BAODING, frame_skip=10, target_lo=[0.0] * 5, tip_sites=sites[2:] + sites[:2], pose_thd=0.015, far_th=1.25)
    # a plane - sphere pair outside the TrackEnv class is refused at load, never dropped
    a = dict(bd.arrays)
    a["hip_trk"] = np.zeros(3, np.int32)
    with pytest.raises(capi.MyoError, match="error -4"):
        capi.HipModel(M.Model(a, bd.names, bd.source).blob(), 0)


def test_guard_poisoned_build():
    H.rerun_file_against_poison_build(__file__, timeout=1500)
