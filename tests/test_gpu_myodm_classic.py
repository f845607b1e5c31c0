"""GPU tests of the classic gym flavour of the MyoDM TrackEnv (envs/myo/myodm/myodm_v0.py; myo_track_config.flavour = 1,
csrc/myo_task_myodm.h): a rollout env by env against the float64 oracle and the float64 restatement tests/myodm_classic_ref.py, the
observation layouts, the reset observation, RANDOM draws per episode, the TimeLimit with its auto-reset, the refused action map, the
poisoned build, the new kernels' resources and the unchanged MJX flavour."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _motion():
    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_motion.npz"))
    return {k.split("__in__")[1]: f[k] for k in f.files if k.startswith("track_MyoHand_airplane_fly1__in__")}


def _frames(o, m):
    """Post-step kinematics the classic env reads: object xipos / ximat and wrist (lunate) xipos."""
    o.forward()
    xi, xm = o.field("xipos").reshape(-1, 3), o.field("ximat").reshape(-1, 9)
    ob, wb = m.name2id("body", "airplane"), m.name2id("body", "lunate")
    return xi[ob].copy(), xm[ob].copy(), xi[wb].copy()


def _lift_z(m):
    from oracle.oracle import Oracle
    o = Oracle(m.blob())
    o.reset()
    o.forward()
    return float(o.field("xipos").reshape(-1, 3)[m.name2id("body", "airplane"), 2]) + 0.02          # myodm_v0.py:154


def test_classic_rollout_against_oracle_and_restatement():
    """BaseV0.step (sigmoid on the muscles, raw clamped controls on the position actuators, 10 substeps) and get_obs_dict / get_reward_dict
    at the post-step time and kinematics, env by env, on the fly1 motion: against the oracle stepped with the same controls and the
    restatement evaluated on the oracle's state."""
    import torch
    import myodm_classic_ref as R
    from myosuite_mjx_amd import envs, track as T
    from oracle.oracle import Oracle
    B = 8
    motion = _motion()
    env = envs.make("MyoHandAirplaneFly-v0", B, flavour="classic", reference=motion)
    assert isinstance(env, T.ClassicTrackEnv) and env.frame_skip == 10 and env.obs_dim == 142
    m = env.mjmodel
    obs = env.reset(seed=0)
    assert obs.shape == (B, 142)
    muscle = np.asarray(m.arrays["actuator_kind"]) == 0
    lift_z = _lift_z(m)
    oracles = [Oracle(m.blob()) for _ in range(B)]
    for o in oracles:
        o.reset(); o.set_state(qpos=env.init_qpos.astype(np.float64), qvel=np.zeros(m.nv))
    ref = T.ReferenceMotion(motion, motion_extrapolation=True)
    rng = np.random.default_rng(7)
    worst_q = worst_o = worst_r = 0.0
    for k in range(3):
        a = rng.uniform(-1, 1, (B, m.nu)).astype(np.float32)
        a[:, ~muscle] *= 2.0                                      # raw position controls beyond [-1, 1]: clamped to ctrlrange by the force
        obs, reward, term, trunc, info = env.step(a)
        assert term.dtype == torch.bool and trunc.dtype == torch.bool and obs.dtype == torch.float32
        g = obs.cpu().numpy()
        r = ref.get_reference((k + 1) * 0.02)
        row = dict(robot=r["robot"][0], robot_vel=None, object=r["object"][0])
        for e, o in enumerate(oracles):
            c = a[e].astype(np.float64)
            c[muscle] = 1.0 / (1.0 + np.exp(-5.0 * (c[muscle] - 0.5)))     # base_v0.py:87-91
            o.set_state(ctrl=c)
            assert o.step(10) == 0
            xp, xm, wp = _frames(o, m)
            want, rwd, done = R.obs_reward(o.field("qpos"), o.field("qvel"), o.field("act")[muscle], row, xp, xm, wp, lift_z)
            worst_q = max(worst_q, float(np.abs(g[e, :35] - o.field("qpos")).max()))
            worst_o = max(worst_o, float(np.abs(g[e, 70:] - want[70:]).max()))     # errors and act
            worst_r = max(worst_r, abs(float(reward[e]) - rwd["dense"]))
            assert bool(term[e]) == done
            for key in ("pose", "object", "bonus", "penalty"):
                assert abs(float(info["metrics"][key][e]) - rwd[key]) < 2e-3
        if bool(term.any()):
            break
    assert (env.status() == 0).all()
    assert worst_q < 5e-4 and worst_r < 2e-3 and worst_o < 5e-3, (worst_q, worst_r, worst_o)


@pytest.mark.parametrize("env_id,dim,vel", [("MyoHandAirplaneFixed-v0", 170, True), ("MyoHandAirplaneRandom-v0", 170, True),
                                            ("MyoHandAirplaneFly-v0", 142, False)])
def test_obs_layout_and_reset_observation(env_id, dim, vel):
    """Reset: every env at init_qpos (myodm_v0.py:168-179), zero velocity / activation; the row is qp, qv, hand_qpos_err, hand_qvel_err,
    obj_com_err, act with the reference at t = 0 and the kinematics of init_qpos."""
    import myodm_classic_ref as R
    from myosuite_mjx_amd import envs
    from oracle.oracle import Oracle
    B = 4
    kw = dict(reference=_motion()) if not vel else {}
    env = envs.make(env_id, B, flavour="classic", **kw)
    sp = envs.myodm_spec(env_id, "classic", **kw)
    assert env.obs_dim == dim == sp["obs_dim"] and env.max_episode_steps == sp["max_episode_steps"]
    np.testing.assert_array_equal(env.init_qpos, sp["init_qpos"])
    g = env.reset(seed=3).cpu().numpy()
    assert g.shape == (B, dim) and np.isfinite(g).all()
    m = env.mjmodel
    np.testing.assert_array_equal(g[:, :35], np.broadcast_to(env.init_qpos, (B, 35)))
    assert not g[:, 35:70].any() and not g[:, dim - m.n_muscle:].any()
    o = Oracle(m.blob())
    o.reset(); o.set_state(qpos=env.init_qpos.astype(np.float64), qvel=np.zeros(m.nv))
    xp, xm, wp = _frames(o, m)
    for e in range(B):
        if sp["ref_type"] == "RANDOM":     # the draw is the kernel's: read it back from the row (qpos = init_qpos, qvel = 0)
            robot = env.init_qpos[:29] - g[e, 70:99]
            row = dict(robot=robot, robot_vel=-g[e, 99:128], object=np.r_[xp - g[e, 128:131], [1.0, 0.0, 0.0, 0.0]])
            lo, hi = env.ref.reference["object"][0, :3], env.ref.reference["object"][1, :3]
            assert ((row["object"][:3] >= lo - 1e-5) & (row["object"][:3] <= hi + 1e-5)).all()
        else:
            r = env.ref.get_reference(0.0)
            row = dict(robot=r["robot"][0], robot_vel=None if r["robot_vel"] is None else r["robot_vel"][0], object=r["object"][0])
        want, _, _ = R.obs_reward(env.init_qpos.astype(np.float64), np.zeros(m.nv), np.zeros(m.n_muscle), row, xp, xm, wp, 0.0)
        np.testing.assert_allclose(g[e], want, rtol=0, atol=2e-5)


def test_random_targets_differ_between_episodes():
    """RANDOM references draw per lookup, keyed by the reset seed and the episode count: two consecutive episodes of one env (same seed)
    see different targets, and so do two envs of one episode."""
    from myosuite_mjx_amd import envs
    env = envs.make("MyoHandAirplaneRandom-v0", 4, flavour="classic")
    a = env.reset(seed=5).cpu().numpy().copy()
    b = env.reset(seed=5).cpu().numpy().copy()
    err = slice(128, 131)                                           # obj_com_err = com - drawn target (the same com: init_qpos)
    assert (np.abs(a[:, err] - b[:, err]).max(1) > 1e-3).all()
    assert np.abs(a[0, err] - a[1, err]).max() > 1e-3
    env2 = envs.make("MyoHandAirplaneRandom-v0", 4, flavour="classic")
    np.testing.assert_array_equal(env2.reset(seed=5).cpu().numpy(), a)        # deterministic given the seed


def test_truncation_at_the_time_limit_and_autoreset():
    """TimeLimit 50 of the Fixed ids: without the object termination, steps 1-49 are neither terminated nor truncated, step 50 is
    truncated and its returned row is the first observation of the new episode (init_qpos, zero velocity)."""
    import torch
    from myosuite_mjx_amd import capi, envs
    B = 4
    env = envs.make("MyoHandAirplaneFixed-v0", B, flavour="classic", Termimate_obj_fail=False)
    first = env.reset(seed=0).clone()
    a = torch.zeros((B, env.act_dim), device="cuda")
    for k in range(1, 51):
        obs, reward, term, trunc, info = env.step(a)
        assert not bool(term.any())
        assert bool(trunc.all()) == (k == 50) and bool(trunc.any()) == (k == 50)
    assert torch.equal(obs[:, :70], first[:, :70])
    assert (env.batch.read(capi.F_ELAPSED)[:, 0] == 0).all() and (env.batch.read(capi.F_TIME)[:, 0] == 0).all()


def test_ctrlrange_action_map_is_refused_on_a_classic_batch():
    from myosuite_mjx_amd import capi, envs
    env = envs.make("MyoHandAirplaneFixed-v0", 2, flavour="classic")
    env.reset()
    ptr, _, _ = env.batch.field_ptr(capi.F_ACTION)
    with pytest.raises(capi.MyoError, match="CTRLRANGE"):
        env.batch.step(ptr, capi.ACTMAP_CTRLRANGE, 10)
    env.batch.step(ptr, capi.ACTMAP_MUSCLE_SIGMOID, 10)             # the classic env's own map still runs
    env.batch.obs()
    assert (env.status() == 0).all()


def test_mjx_flavour_unchanged_by_the_flavour_argument():
    """flavour="mjx" and no flavour build the same MJX env: bit-identical observations, rewards and dones over a few steps."""
    import torch
    from myosuite_mjx_amd import envs, track as T
    outs = []
    for kw in ({}, dict(flavour="mjx")):
        env = envs.make("MyoHandAirplaneRandom-v0", 16, seed=2, **kw)
        assert type(env) is T.TrackEnv and env.obs_dim == 70
        rows = [env.reset().clone()]
        g = torch.Generator(device="cuda").manual_seed(1)
        for _ in range(4):
            obs, rew, done, trunc, info = env.step(torch.rand((16, env.act_dim), device="cuda", generator=g) * 2 - 1)
            rows += [obs.clone(), rew.clone(), done.clone(), trunc.clone()]
        outs.append([r.cpu() for r in rows])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_classic_kernels_have_no_spills_and_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = [r for r in KR.resources() if "myodm_" in r["name"]]
    assert len(ks) == 2
    for r in ks:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r


def test_classic_tests_pass_on_the_poisoned_build():
    if os.environ.get("MYO_HIP_LIB"):
        pytest.skip("already running on a diagnostic build")
    lib = os.path.join(ROOT, "myosuite_mjx_amd", "libmyo_hip_poison.so")
    assert os.path.exists(lib), "libmyo_hip_poison.so is missing: run __graft_entry__.build()"
    env = dict(os.environ, MYO_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not poisoned and not resources",
                        "tests/test_gpu_myodm_classic.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout
