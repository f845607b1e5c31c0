"""GPU tests (pytest -m gpu) for myoChallengeDieReorient{Demo,P1}-v0 (envs/myo/myochallenge/reorient_v0.py) on the TrackEnv-class ("TRK")
step kernel: MyoHand + a die of 12 capsules and 3 boxes on 3 slides + 3 hinges + a world-welded target moved and turned per env
(MYO_F_TARGET row, MYO_F_BODYQUAT).

  * HIP vs the float64 oracle after 1, 5 (one env step) and 10 substeps on 48 states of oracle rollouts: the die resting on the palm,
    touched by fingers, falling; capsule - capsule and capsule - box contacts.  Bounds as in tests/test_gpu_pen.py.
  * MYO_F_SITEXPOS, observation, reward, done and solved against tests/reorient_ref.py on the 600 rollout states with goals drawn per env;
    reset draws over 4096 envs; the goal_offset / body_quat views; the fused bench epilogue; no dropped contact over a 150-step random
    rollout at 4096 envs; every id steps; refusals."""
import numpy as np
import pytest

import hand_task_checks as H
from die_states import init_qpos, pick_states, rollout_states
from hand_task_checks import TRK
from reorient_ref import SITES, euler2quat, euler_margin, mat2euler, reorient_restate

pytestmark = pytest.mark.gpu
ID = "myoChallengeDieReorientP1-v0"
DT = 0.01


@pytest.fixture(scope="module")
def die():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_die")


@pytest.fixture(scope="module")
def rollouts(die):
    return rollout_states(die)


def _configure(b, m, pos_th=0.025, goal_pos=(-0.010, 0.010)):
    from myosuite_mjx_amd import capi
    b.configure(task=capi.TASK_DIE, frame_skip=5, target_generate=1, target_lo=[goal_pos[0]] * 3, target_hi=[goal_pos[1]] * 3,
                init_qpos=init_qpos(m), tip_sites=[m.name2id("site", n) for n in SITES], near_th=pos_th, pose_thd=0.262, far_th=0.2,
                w_pose=100.0, w_reach=1.0, w_bonus=0.0, w_act_reg=0.0, w_penalty=0.0, quat_body=m.name2id("body", "target"))


CASE = H.TaskCase(stem="myohand_die", task="die", bench_id=ID, obs_dim=63, nsub=5, configure=_configure, extra_fields=("F_BODYQUAT", "F_TARGET"),
                  env_ids=tuple(f"myo{c}ChallengeDieReorient{v}-v0" for c in ("", "Sarc", "Fati") for v in ("Demo", "P1")))


def _quat2mat(q):
    from myosuite_mjx_amd.mjcf import quat2mat
    q = np.asarray(q, np.float64)
    return quat2mat(q / np.linalg.norm(q))


@pytest.mark.parametrize("nsub,tq,tv", [(1, 2e-5, 2e-2), (5, 2e-3, 0.2), (10, 2e-3, 0.2)])
def test_contact_parity(die, rollouts, nsub, tq, tv):
    """One substep, one env step (5 substeps) and 10 substeps against the float64 oracle; the bounds are those of tests/test_gpu_pen.py for
    1 and 10 substeps, the env step takes the 10-substep one.  (Float32 build of the oracle against float64 on these states, same
    controls: 2.3e-7 / 1.2e-4 after 1 substep, 2.1e-6 / 4.7e-4 after 5, 1.7e-4 / 2.1e-2 after 10.)"""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = die
    P = pick_states(rollouts, 48)
    N = len(P)
    assert N == 48
    for tag in ("palm", "finger", "falling"):
        assert sum(tag in s[3] for s in P) >= 8, tag
    assert sum((3, 3) in s[4] for s in P) >= 8 and sum((3, 6) in s[4] for s in P) >= 8
    f32 = np.float32
    rng = np.random.default_rng(9)
    q, v, act = (np.array([s[k] for s in P]).astype(f32) for k in range(3))
    a = rng.uniform(-1, 1, (N, m.nu)).astype(f32)
    b = H.new_batch(CASE, m, N)
    o = Oracle(m.blob())
    eq, ev, nc, dg, fl, same = H.step_and_compare_with_oracle(m, b, {capi.F_QPOS: q, capi.F_QVEL: v, capi.F_ACT: act, capi.F_ACTION: a}, nsub,
                                                              lambda e: o)
    print(f"die parity nsub={nsub}: same contact count {same.mean():.3f}, max|dqpos| {eq[same].max():.3e}, max|dqvel| {ev[same].max():.3e}, "
          f"all states {eq.max():.3e} / {ev.max():.3e}, flags {sorted(set(fl.tolist()))}, ncon max {nc.max()}")
    assert same.mean() > 0.8, (same.mean(), dg[:, 1].tolist(), nc.tolist())
    w = int(np.argmax(np.where(same, eq, 0)))
    assert eq[same].max() < tq and ev[same].max() < tv, (eq[same].max(), ev[same].max(), w, sorted(P[w][3]), sorted(P[w][4]), int(nc[w]))
    for tag in ("palm", "finger", "falling"):
        assert any(same[e] and tag in P[e][3] for e in range(N)), tag
    assert any(same[e] and (3, 6) in P[e][4] for e in range(N)) and any(same[e] and (3, 3) in P[e][4] for e in range(N))
    assert np.abs(b.read(capi.F_QPOS) - q).max() > 1e-5


def _goals(m, S, rng, Ro, xo):
    """Per-env goal offsets and target quaternions: P1's ranges, and for every third env a goal near the die's own pose (so that solved
    occurs)."""
    N = len(S)
    tb = m.name2id("body", "target")
    off = rng.uniform(-0.01, 0.01, (N, 3))
    eul = rng.uniform(-1.57, 1.57, (N, 3))
    near = np.arange(N) % 3 == 0
    off[near] = (xo[near] + [-0.1, 0, 0]) - m.body_pos[tb] + rng.normal(0, 0.012, (near.sum(), 3))
    eul[near] = mat2euler(Ro[near]) + rng.normal(0, 0.12, (near.sum(), 3))
    return off.astype(np.float32), euler2quat(eul).astype(np.float32)


def test_observation_against_restatement(die, rollouts):
    """The 600 states of the four oracle episodes with a goal per env.  The restatement is fed the GPU's own qpos / qvel / act, the oracle's
    frame of the die at that qpos, and the target frame the env's offset and quaternion give (checked against the oracle on
    Model.with_body_quat / with_body_pos blobs for eight envs).

    Bounds: positions 5e-6 and the state part of the row 1e-5, as in tests/test_gpu_pen.py.  Euler angles: an entry of a site frame is a
    difference of two float32 site positions (coordinates up to 0.3 m from the lowered origin: half an ulp is 1.5e-8 each) over the
    0.028 m between the sites, about 1e-6, plus the float32 rotation chain of the link, a few 1e-7: 4e-6 at most.  An atan2 whose
    arguments have the norm cy moves by at most sqrt(2) 4e-6 / cy: the bound is 1e-5 / cy per angle (cy >= 1e-3 for compared states),
    twice that for rot_err.  Reward = -100 pos_dist - rot_dist: 100 x 1e-5 (two positions) + sqrt(3) x the rot_err bound."""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    m = die
    S = rollouts
    N = len(S)
    ob, tb = m.name2id("body", "Object"), m.name2id("body", "target")
    f32 = np.float32
    q, v, act = (np.array([s[k] for s in S]).astype(f32) for k in range(3))
    o = Oracle(m.blob())
    Ro, xo = np.zeros((N, 3, 3)), np.zeros((N, 3))
    sid = [m.name2id("site", n) for n in SITES]
    xs = np.zeros((N, 8, 3))
    for e in range(N):
        H.forward_at(o, q[e])
        Ro[e], xo[e] = o.field("xmat").reshape(-1, 3, 3)[ob], o.field("site_xpos").reshape(-1, 3)[sid[0]]
        xs[e] = o.field("site_xpos").reshape(-1, 3)[sid]
    rng = np.random.default_rng(11)
    off, quat = _goals(m, S, rng, Ro, xo)
    b = H.new_batch(CASE, m, N)
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act), (capi.F_BODYQUAT, quat), (capi.F_TARGET, off)):
        b.write(f, x)
    b.obs()
    sx, obs, rew, done, solved = (b.read(f) for f in (capi.F_SITEXPOS, capi.F_OBS, capi.F_REWARD, capi.F_DONE, capi.F_SOLVED))
    assert sx.shape == (N, 24) and obs.shape == (N, 63)
    Rt = np.array([_quat2mat(quat[e]) for e in range(N)])
    xt = m.body_pos[tb] + off.astype(np.float64)
    lt = np.asarray(m.site_pos)[sid[4:]]                          # the target's sites in its body frame
    xs[:, 4:] = xt[:, None, :] + np.einsum("eij,kj->eki", Rt, lt)
    for e in range(0, N, 75):                                     # the analytic target frame = the oracle's on the edited model
        mm = m.with_body_quat(tb, quat[e].astype(np.float64) / np.linalg.norm(quat[e].astype(np.float64))).with_body_pos(tb, xt[e])
        oe = Oracle(mm.blob())
        oe.reset()
        oe.forward()
        assert np.abs(oe.field("site_xpos").reshape(-1, 3)[sid[4:]] - xs[e, 4:]).max() < 1e-12
        assert np.abs(oe.field("xmat").reshape(-1, 3, 3)[tb] - Rt[e]).max() < 1e-12
    print(f"die sites: max|dx| {np.abs(sx.reshape(N, 8, 3) - xs).max():.3e}")
    assert np.abs(sx.reshape(N, 8, 3) - xs).max() < 5e-6
    ro, rr, rd, rs = reorient_restate(q, v, act, xs[:, 0], xs[:, 4], Ro, Rt, DT)
    (cyo, cuto), (cyt, cutt) = euler_margin(Ro), euler_margin(Rt)
    keep = (cyo >= 1e-3) & (cyt >= 1e-3) & (cuto >= 1e-3) & (cutt >= 1e-3)
    assert (~keep).mean() <= 0.05, (~keep).sum()
    d = np.abs(obs - ro)
    d[:, 54:] = np.abs((d[:, 54:] + np.pi) % (2 * np.pi) - np.pi)                    # Euler angles modulo 2 pi
    te_o, te_t = 1e-5 / cyo, 1e-5 / cyt
    print(f"die obs: state part {d[:, :45].max():.3e}, positions {d[:, 45:54].max():.3e}, obj_rot x cy {(d[keep, 54:57].max(1) * cyo[keep]).max():.3e}, "
          f"goal_rot x cy {(d[keep, 57:60].max(1) * cyt[keep]).max():.3e}, rot_err {d[keep, 60:63].max():.3e}, left out {(~keep).sum()} of {N}")
    assert d[:, :45].max() < 1e-5 and d[:, 45:54].max() < 1e-5
    assert (d[keep, 54:57].max(1) < te_o[keep]).all() and (d[keep, 57:60].max(1) < te_t[keep]).all()
    assert (d[keep, 60:63].max(1) < (te_o + te_t)[keep]).all()
    tr = 100 * 1e-5 + np.sqrt(3) * (te_o + te_t)
    print(f"die reward: max|d| / bound {(np.abs(rew[:, 0] - rr)[keep] / tr[keep]).max():.3f}")
    assert (np.abs(rew[:, 0] - rr)[keep] < tr[keep]).all()
    pd, rd_ = np.linalg.norm(ro[:, 51:54], axis=1), np.linalg.norm(ro[:, 60:63], axis=1)
    clear = keep & (np.abs(pd - 0.2) > 1e-4) & (np.abs(pd - 0.025) > 1e-4) & (np.abs(rd_ - 0.262) > np.sqrt(3) * (te_o + te_t))
    assert clear.mean() > 0.9
    assert np.array_equal(done[clear, 0] > 0, rd[clear]) and np.array_equal(solved[clear, 0] > 0, rs[clear])
    assert rd[clear].any() and not rd[clear].all() and rs[clear].any() and not rs[clear].all()


def test_reset_draws_and_sharding():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B = 4096

    def make_env(n, seed, off):
        return myo.make(ID, num_envs=n, seed=seed, env_offset=off, as_torch=False)

    env = make_env(B, H.SEED, 0)
    obs = env.reset()
    m = env.mjmodel
    tb = m.name2id("body", "target")
    assert obs.shape == (B, 63) and env.obs_dim == 63
    assert np.array_equal(env.batch.read(capi.F_QPOS), np.tile(init_qpos(m).astype(np.float32), (B, 1)))     # palm-up open hand, die at qpos0
    assert not env.batch.read(capi.F_QVEL).any()
    off, quat = env.goal_offset, env.body_quat
    assert off.shape == (B, 3) and quat.shape == (B, 4)
    assert off.min() >= -0.010 and off.max() <= 0.010
    eul = mat2euler(np.array([_quat2mat(x) for x in quat]))
    assert np.abs(euler2quat(eul) - quat).max() < 2e-6                                 # the reference's euler2quat of ...
    assert eul.min() >= -1.57 - 1e-5 and eul.max() <= 1.57 + 1e-5                      # ... angles inside goal_rot
    for a, lo, hi in [(off[:, k], -0.010, 0.010) for k in range(3)] + [(eul[:, k], -1.57, 1.57) for k in range(3)]:
        H.assert_uniform(a, lo, hi)                                                    # uniform, and different from env to env
    assert len(np.unique(off[:, 0])) > 0.9 * B and abs(np.corrcoef(off[:, 0], off[:, 1])[0, 1]) < 0.1
    # the first observation shows the drawn goal
    assert np.abs(obs[:, 48:51] - (m.body_pos[tb] + off)).max() < 5e-6 and np.abs(obs[:, 51:54] - off).max() < 5e-6
    # goal_rot: the bound of test_observation_against_restatement, 1e-5 / cy per angle (U(-1.57, 1.57) reaches cy = cos 1.57 = 8e-4; a
    # flat bound would ignore the atan2's conditioning), the states it leaves out left out here too
    cy, cut = euler_margin(np.array([_quat2mat(x) for x in quat]))
    keep = (cy >= 1e-3) & (cut >= 1e-3)
    de = np.abs((np.abs(obs[:, 57:60] - eul) + np.pi) % (2 * np.pi) - np.pi).max(1)
    print(f"die reset: goal_rot error x cy {(de * cy)[keep].max():.3e}, left out {(~keep).sum()} of {B}")
    assert (~keep).mean() <= 0.05 and (de[keep] < 1e-5 / cy[keep]).all()
    # consecutive episodes differ: an auto-reset of every env after one step
    env.batch.step(None, capi.ACTMAP_NONE, 5)
    env.batch.autoreset(1, env.seed)
    off2, quat2 = env.goal_offset, env.body_quat
    assert (off2 != off).any(axis=1).mean() > 0.99 and (quat2 != quat).any(axis=1).mean() > 0.99
    assert off2.min() >= -0.010 and off2.max() <= 0.010
    # same seed: same draws; another seed: others; shards draw what the full batch draws
    H.assert_deterministic_and_sharded(make_env, lambda e: (e.goal_offset, e.body_quat), B, (off, quat))
    # Demo: no position draw, +-45 degrees, pos_th = inf
    d = myo.make("myoChallengeDieReorientDemo-v0", num_envs=256, seed=H.SEED, as_torch=False)
    od = d.reset()
    assert not d.goal_offset.any() and np.abs(od[:, 51:54]).max() < 5e-6
    ed = mat2euler(np.array([_quat2mat(x) for x in d.body_quat]))
    assert np.abs(ed).max() <= 0.785 + 1e-5 and np.abs(ed).max() > 0.7
    d.step(np.zeros((256, 39), np.float32))
    rd_ = np.linalg.norm(d.batch.read(capi.F_OBS)[:, 60:63], axis=1)
    assert np.isfinite(d.batch.read(capi.F_REWARD)).all() and np.array_equal(d.batch.read(capi.F_SOLVED)[:, 0] > 0, rd_ < 0.262)


def test_goal_views_are_writable_and_take_effect():
    import torch
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make(ID, num_envs=64, seed=3)
    env.reset()
    m = env.mjmodel
    tb = m.name2id("body", "target")
    assert env.goal_offset.data_ptr() == env.batch.field_ptr(capi.F_TARGET)[0] and env.body_quat.data_ptr() == env.batch.field_ptr(capi.F_BODYQUAT)[0]
    rng = np.random.default_rng(0)
    off = rng.uniform(-0.02, 0.02, (64, 3)).astype(np.float32)
    eul = rng.uniform(-1.2, 1.2, (64, 3))
    env.goal_offset[:] = torch.as_tensor(off, device=env.goal_offset.device)
    env.body_quat = euler2quat(eul).astype(np.float32)
    env.batch.obs()
    torch.cuda.synchronize()
    obs = env.view(capi.F_OBS).cpu().numpy()
    assert np.abs(obs[:, 48:51] - (m.body_pos[tb] + off)).max() < 5e-6
    assert np.abs(obs[:, 51:54] - off).max() < 5e-6                                    # the die sits at qpos0: pos_err = the offset
    tol = 1e-5 / np.cos(eul[:, 1]).min()                                              # 1e-5 / cy, cy = cos of the middle angle (>= 0.36 here)
    assert np.abs(obs[:, 57:60] - eul).max() < tol and np.abs(obs[:, 60:63] - (eul - obs[:, 54:57])).max() < 2 * tol
    env.goal_offset = np.zeros(3, np.float32)
    env.batch.obs()
    torch.cuda.synchronize()
    assert np.abs(env.view(capi.F_OBS).cpu().numpy()[:, 51:54]).max() < 5e-6
    with pytest.raises(AttributeError):
        myo.make("myoHandPenTwirlFixed-v0", num_envs=4).goal_offset


def test_bad_env_is_contained():
    H.bad_env_is_contained(CASE)


def test_fused_bench_epilogue_equals_step_obs_autoreset():
    assert H.fused_epilogue_equals_stepwise(CASE).last_kernel_name() == TRK


def test_no_dropped_contact_over_a_random_rollout():
    """150 env steps of U(-1, 1) actions at 4096 envs with auto-reset (the die drops and the episode restarts many times): no contact and no
    candidate pair is ever dropped (the other flag bits are printed)."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make(ID, num_envs=4096, seed=5, as_torch=False)
    env.reset()
    ncon, resets = 0, 0
    for k in range(6):
        env.batch.bench_rollout(25, 5, seed=17, mode=capi.BENCH_OBS | capi.BENCH_FRESH_ACTIONS | capi.BENCH_AUTORESET, max_episode_steps=150)
        fl = env.status()
        ncon = max(ncon, int(env.batch.read(capi.F_DIAG)[:, 1].max()))
        resets += int((env.batch.read(capi.F_ELAPSED)[:, 0] < 25).sum())
        assert not (fl & (capi.FLAG_CONTACT_OVERFLOW | capi.FLAG_CAND_OVERFLOW)).any(), (k, np.unique(fl, return_counts=True))
        print(f"die rollout chunk {k}: flags {dict(zip(*[x.tolist() for x in np.unique(fl, return_counts=True)]))}")
    print(f"die rollout: max contacts at a chunk's end {ncon}, envs seen freshly reset {resets}")
    assert np.isfinite(env.batch.read(capi.F_OBS)).all() and ncon >= 8 and resets > 4096


@pytest.mark.parametrize("env_id", CASE.env_ids)
def test_every_id_steps(env_id):
    env = H.every_id_steps(CASE, env_id)
    assert env.max_episode_steps == 150 and env.frame_skip == 5


def test_env_api_matches_restatement():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make(ID, num_envs=1024, seed=4, as_torch=False, autoreset=False)
    env.reset()
    rng = np.random.default_rng(1)
    for _ in range(12):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (1024, 39)).astype(np.float32))
    # the row is self-consistent: pos_err and rot_err from the row's own positions and angles, the reward and flags from those
    assert np.abs(obs[:, 51:54] - (obs[:, 48:51] - obs[:, 45:48] - np.float32([-0.1, 0, 0]))).max() < 1e-6
    assert np.abs(obs[:, 60:63] - (obs[:, 57:60] - obs[:, 54:57])).max() < 1e-6
    pd, rd_ = np.linalg.norm(obs[:, 51:54].astype(np.float64), axis=1), np.linalg.norm(obs[:, 60:63].astype(np.float64), axis=1)
    assert np.abs(rew + 100 * pd + rd_).max() < 1e-3
    clear = (np.abs(pd - 0.2) > 1e-5) & (np.abs(pd - 0.025) > 1e-5) & (np.abs(rd_ - 0.262) > 1e-5)
    assert np.array_equal(term[clear], (pd > 0.2)[clear]) and np.array_equal(info["solved"][clear], ((pd < 0.025) & (rd_ < 0.262))[clear])
    assert np.array_equal(obs[:, :22], env.batch.read(capi.F_QPOS)[:, :22]) and not trunc.any()
    assert np.abs(obs[:, 22:45] - env.batch.read(capi.F_QVEL)[:, :23] * np.float32(env.dt)).max() < 1e-6


def test_refusals(die):
    from myosuite_mjx_amd import capi, model as M
    m = die
    sites = [m.name2id("site", n) for n in SITES]
    tb = m.name2id("body", "target")
    kw = dict(task=capi.TASK_DIE, frame_skip=5, near_th=0.025, pose_thd=0.262, far_th=0.2)
    pen = M.load_asset("myohand_pen")
    pb = capi.HipBatch(capi.HipModel(pen.blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="error -1"):          # TRK class with six trailing scalar dofs, but not the die's sites / goal row
        pb.configure(tip_sites=[0, 1, 2, 3, 4], quat_body=pen.name2id("body", "target"), **kw)
    hand = capi.HipBatch(capi.HipModel(M.load_asset("myohand_pose").blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="error -4"):          # not a TrackEnv-class model
        hand.configure(tip_sites=sites, target_lo=[0] * 3, **kw)
    b = capi.HipBatch(capi.HipModel(m.blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="error -1"):          # quat_body not selected
        b.configure(tip_sites=sites, target_lo=[0] * 3, **kw)
    with pytest.raises(capi.MyoError, match="error -1"):          # ntarget must be 3
        b.configure(tip_sites=sites, target_lo=[0] * 5, quat_body=tb, **kw)
    with pytest.raises(capi.MyoError, match="error -1"):          # ntip must be 8
        b.configure(tip_sites=sites[:5], target_lo=[0] * 3, quat_body=tb, **kw)
    with pytest.raises(capi.MyoError, match="error -4"):          # the die's sites swapped with the target's
        b.configure(tip_sites=sites[4:] + sites[:4], target_lo=[0] * 3, quat_body=tb, **kw)
    with pytest.raises(capi.MyoError, match="error -1"):          # a threshold that is not a number
        b.configure(tip_sites=sites, target_lo=[0] * 3, quat_body=tb, **dict(kw, pose_thd=float("nan")))
    b.configure(tip_sites=sites, target_lo=[0] * 3, quat_body=tb, **dict(kw, near_th=float("inf")))       # pos_th = inf passes (Demo)
    assert b.read(capi.F_OBS).shape == (4, 63)
    with pytest.raises(capi.MyoError, match="error -4"):          # per-env masses are refused on TrackEnv-class models
        b.write(capi.F_BODYMASS, np.tile(np.asarray(m.body_mass, np.float32), (4, 1)))
