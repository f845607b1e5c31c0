"""GPU tests (pytest -m gpu) at BASELINE.json's FULL sizes, where the scalar oracle is too slow to step every env: size-independent
properties of the path instead (SURVEY.md 8d parity protocol, last sentence; task prompt section 3):

  * a full-size batch is bit-identical to the same envs stepped as small shards (env_offset) -- so every parity result the
    oracle pins on small batches carries over to the 4096 / 32768-env launches, whatever the placement / scheduler did;
  * state invariants of the physics after long rollouts (finite, activations in [0, 1], joint angles inside the soft limits,
    unit free-joint quaternion, the 14 polynomial knee / patella couplings of myolegs_assets.xml:88-103 satisfied);
  * observation / reward rows are consistent with the state they were computed from (pose_v0.py:98-138, reach_v0.py:88-144);
  * fingertip positions of a sample of envs of the full-size reach launch against the f64 oracle's kinematics.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _make(env_id, n, **kw):
    import myosuite_mjx_amd as myo
    return myo.make(env_id, num_envs=n, **kw)


def _actions(B, nu, seed, k):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed * 1000 + k)
    return torch.rand((B, nu), device="cuda", generator=g) * 2 - 1


def test_config3_32768_envs_equal_their_shards_and_keep_invariants(hand):
    """myoHandPoseRandom-v0, B=32768 (BASELINE.json configs[2])."""
    import torch
    B, K = 32768, 25
    env = _make("myoHandPoseRandom-v0", B, seed=11)
    env.reset(seed=11)
    # three 64-env shards of the same job (front, middle, end of the id range): same seeds, env_offset = first global id
    offs = [0, 16000, B - 64]
    shards = [_make("myoHandPoseRandom-v0", 64, seed=11, env_offset=o) for o in offs]
    for s in shards:
        s.reset(seed=11)
    nflag = 0
    for k in range(K):
        a = _actions(B, 39, 1, k)
        obs, rwd, term, trunc, info = env.step(a)
        nflag += int((env.status() != 0).sum())
        for o, s in zip(offs, shards):
            so, sr, st, _, _ = s.step(a[o:o + 64])
            assert torch.equal(so, obs[o:o + 64]) and torch.equal(sr, rwd[o:o + 64]) and torch.equal(st, term[o:o + 64]), (k, o)
    st = env.get_env_state()
    assert all(np.isfinite(v).all() for v in st.values())
    assert (st["act"] >= 0).all() and (st["act"] <= 1).all()
    lo, hi = hand.jnt_range[:, 0], hand.jnt_range[:, 1]
    over = np.maximum(lo - st["qpos"], st["qpos"] - hi).max()
    assert over < 0.3, over                                    # soft limits (solref 0.02) against full muscle force: overshoot stays bounded
    assert nflag <= 0.02 * B, nflag                              # contact-table overflows / resets stay rare (flags are per env-step)
    o = obs.cpu().numpy()
    assert np.allclose(o[:, :23], st["qpos"], atol=1e-7) and np.allclose(o[:, 23:46], st["qvel"] * 0.02, atol=1e-6)
    assert np.allclose(o[:, 46:69], st["target"] - st["qpos"], atol=1e-6) and np.allclose(o[:, 69:], st["act"], atol=1e-7)
    dist = np.linalg.norm(o[:, 46:69], axis=1)
    ref = -dist + 4.0 * ((dist < 0.7) * 1.0 + (dist < 1.05) * 1.0) - np.linalg.norm(st["act"], axis=1) / 39 - 50.0 * (dist > 2 * np.pi)
    assert np.allclose(rwd.cpu().numpy(), ref, atol=2e-5)


def test_config2_4096_envs_1000_steps_stay_physical(hand):
    """myoHandPoseFixed-v0, B=4096, 1000-step rollout (BASELINE.json configs[1] protocol: TimeLimit 100 auto-reset inside)."""
    from myosuite_mjx_amd import capi
    env = _make("myoHandPoseFixed-v0", 4096, seed=2, as_torch=False)
    env.reset(seed=2)
    ms = env.batch.bench_rollout(1050, 10, seed=2, max_episode_steps=100)    # 10 whole episodes + 50 steps into the 11th
    assert ms > 0
    st = env.get_env_state()
    assert all(np.isfinite(v).all() for v in st.values())
    assert (st["act"] >= 0).all() and (st["act"] <= 1).all()
    lo, hi = hand.jnt_range[:, 0], hand.jnt_range[:, 1]
    assert np.maximum(lo - st["qpos"], st["qpos"] - hi).max() < 0.3
    # PoseFixed has no early termination: every env was reset by the TimeLimit on the same steps, so all clocks read 50 env steps
    t = st["time"].ravel()
    assert np.allclose(t, 50 * 0.02, atol=1e-4)
    # U(-1,1) actions through the sigmoid: mean excitation 0.19 -> activations settle well inside (0, 1); joint speeds stay moderate
    assert 0.05 < st["act"].mean() < 0.5
    assert np.abs(st["qvel"]).mean() < 5.0
    # second identical job: bit-identical final state (device RNG is counter based, placement does not leak into results)
    env2 = _make("myoHandPoseFixed-v0", 4096, seed=2, as_torch=False)
    env2.reset(seed=2)
    env2.batch.bench_rollout(1050, 10, seed=2, max_episode_steps=100)
    st2 = env2.get_env_state()
    assert all(np.array_equal(st[k], st2[k]) for k in st)


def test_config4_reach_4096_rows_are_consistent(hand, oracle64):
    """myoHandReachRandom-v0, B=4096 per GPU (BASELINE.json configs[3]): observation / reward rows against the state, and a
    sample of envs against the oracle's site positions."""
    B = 4096
    env = _make("myoHandReachRandom-v0", B, seed=4, autoreset=False)
    env.reset(seed=4)
    for k in range(8):
        obs, rwd, term, trunc, info = env.step(_actions(B, 39, 4, k))
    st = env.get_env_state()
    o = obs.cpu().numpy()
    assert o.shape == (B, 115) and np.isfinite(o).all()
    assert np.allclose(o[:, :23], st["qpos"], atol=1e-7) and np.allclose(o[:, 23:46], st["qvel"] * 0.02, atol=1e-6)
    tip, err = o[:, 46:61], o[:, 61:76]
    assert np.allclose(o[:, 76:], st["act"], atol=1e-7)
    assert np.allclose(err, st["target"] - tip, atol=1e-6)                           # reach_v0.py:104-106
    tl, th = env.spec["target_lo"], env.spec["target_hi"]
    assert (st["target"] >= tl - 1e-6).all() and (st["target"] <= th + 1e-6).all()
    # reach_v0.py:116-144 at t = 0.16 > 2 dt: far_th applies
    dist = np.linalg.norm(err, axis=1)
    near, far = 0.0125 * 5, 0.034 * 5
    edge = (np.abs(dist - near) < 1e-5) | (np.abs(dist - 2 * near) < 1e-5) | (np.abs(dist - far) < 1e-5)
    ref = -dist + 4.0 * ((dist < 2 * near) * 1.0 + (dist < near) * 1.0) - 50.0 * (dist > far)
    r, d = rwd.cpu().numpy(), term.cpu().numpy()
    assert np.allclose(r[~edge], ref[~edge], atol=1e-5)
    assert (d[~edge] == (dist > far)[~edge]).all()
    tips = [hand.name2id("site", t) for t in ("THtip", "IFtip", "MFtip", "RFtip", "LFtip")]
    for e in np.random.default_rng(0).choice(B, 12, replace=False):
        oracle64.reset()
        oracle64.set_state(qpos=st["qpos"][e])
        oracle64.fwd_position()
        sx = oracle64.field("site_xpos").reshape(-1, 3)[tips].ravel()
        assert np.abs(tip[e] - sx).max() < 2e-6


def test_config5_walk_4096_envs_keep_constraints(legs):
    """myoLegWalk-v0, B=4096 (BASELINE.json configs[4]); substep scheduler + leg kernel at full size."""
    import torch
    B, K = 4096, 40
    env = _make("myoLegWalk-v0", B, seed=6)
    env.reset(seed=6)
    offs = [0, 2000, B - 32]
    shards = [_make("myoLegWalk-v0", 32, seed=6, env_offset=o) for o in offs]
    for s in shards:
        s.reset(seed=6)
    for k in range(K):
        a = _actions(B, 80, 6, k)
        obs, rwd, term, trunc, info = env.step(a)
        for o, s in zip(offs, shards):
            so, sr, st_, _, _ = s.step(a[o:o + 32])
            assert torch.equal(so, obs[o:o + 32]) and torch.equal(sr, rwd[o:o + 32]) and torch.equal(st_, term[o:o + 32]), (k, o)
    st = env.get_env_state()
    q = st["qpos"]
    assert np.isfinite(q).all() and np.isfinite(st["qvel"]).all() and np.isfinite(obs.cpu().numpy()).all()
    assert np.abs(np.linalg.norm(q[:, 3:7], axis=1) - 1).max() < 1e-5               # free-joint quaternion renormalised every substep
    assert (st["act"] >= 0).all() and (st["act"] <= 1).all()
    # the reset keyframe (key 2) itself violates the couplings by up to 0.74 rad (hand-edited in the reference, tests/test_oracle.py
    # test_legs_sizes_and_goldens); the soft rows pull it in within ~0.2 s, so the check is for envs at least 0.25 s into an episode
    settled = st["time"].ravel() >= 0.25
    assert settled.sum() > 100
    q = q[settled]
    worst = 0.0
    for e in range(14):                                                              # myolegs_assets.xml:88-103
        j1, j2 = legs.eq_obj1id[e], legs.eq_obj2id[e]
        c = legs.eq_data[e]
        x = q[:, legs.jnt_qposadr[j2]] - legs.qpos0[legs.jnt_qposadr[j2]]
        y = q[:, legs.jnt_qposadr[j1]] - legs.qpos0[legs.jnt_qposadr[j1]]
        worst = max(worst, np.abs(y - (c[0] + x * (c[1] + x * (c[2] + x * (c[3] + x * c[4]))))).max())
    assert worst < 3e-2, worst                                                       # soft equality rows (same bound the oracle test uses +50 %)
    assert st["qpos"][:, 2].min() > 0.2 and st["qpos"][:, 2].max() < 1.3             # nobody fell through the floor or took off
    assert int((env.status() & 16).sum()) == 0                                       # MYO_FLAG_SCHED_TIMEOUT never raised


def test_terrain_4096_envs_equal_their_shards():
    """myoLegRoughTerrainWalk-v0 at B = 4096 (substep scheduler + height-field instantiation) against 32-env shards (one wave per env): the
    per-env terrain draw is keyed by the global env id, and scheduled / unscheduled launches compute bit-identical steps (of envs that go bad in the launch too:
    tests/test_gpu_bad_env.py::test_scheduler_gives_the_same_bits)."""
    import torch
    from myosuite_mjx_amd import capi
    B, K = 4096, 25
    env = _make("myoLegRoughTerrainWalk-v0", B, seed=9)
    env.reset(seed=9)
    offs = [0, 1777, B - 32]
    shards = [_make("myoLegRoughTerrainWalk-v0", 32, seed=9, env_offset=o) for o in offs]
    for s in shards:
        s.reset(seed=9)
    H = env.batch.read(capi.F_HFIELD)
    for o, s in zip(offs, shards):
        assert np.array_equal(s.batch.read(capi.F_HFIELD), H[o:o + 32])
    assert env.batch.last_kernel_name() == "step_kernel"                       # nothing launched yet (reset only)
    for k in range(K):
        a = _actions(B, 80, 9, k)
        obs, rwd, term, trunc, info = env.step(a)
        for o, s in zip(offs, shards):
            so, sr, st_, _, _ = s.step(a[o:o + 32])
            assert torch.equal(so, obs[o:o + 32]) and torch.equal(sr, rwd[o:o + 32]) and torch.equal(st_, term[o:o + 32]), (k, o)
    import os
    if not (os.environ.get("MYO_NO_SPEC") or os.environ.get("MYO_SCHED")):     # default selection: scheduled full batch, one wave per env for the shards
        assert env.batch.last_kernel_name() == "step_kernel_w<36,20,32,2,2,true,3,true>" and shards[0].batch.last_kernel_name() == "step_kernel_w<36,20,32,2,2,false,3,true>"
    assert int((env.status() & 16).sum()) == 0


def test_config_models_run_on_their_specialised_instantiations():
    """The headline envs must take the size- and tree-specialised kernels (a mismatch between a compiled asset and the tables built into
    myo_kernel_wave.h silently falls back to the generic instantiation: correct, but several per cent slower)."""
    import torch
    import myosuite_mjx_amd as myo
    for env_id, n, want in (("myoHandPoseRandom-v0", 256, "step_kernel_w<24,8,32,1,4,false,1,false>"),
                            ("myoLegWalk-v0", 256, "step_kernel_w<36,20,32,2,2,false,2,false>")):
        env = myo.make(env_id, num_envs=n)
        env.reset(seed=0)
        env.step(torch.zeros((n, env.act_dim), device="cuda"))
        assert env.batch.last_kernel_name() == want, (env_id, env.batch.last_kernel_name())
