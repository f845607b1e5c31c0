"""GPU tests of the observation terms of the batched envs (make(..., obs_dict=True, obs_keys=[...], proprio_keys=[...])), one id per task.

Small batches: B = 3 and B = 130 (a multiple of neither 64 nor 256, so the last block of obs_terms_kernel is partly empty), three steps of
random actions after reset(seed=0).  Every check but one is an equality: the terms are copies (of the canonical row, MYO_F_TIME,
MYO_F_TARGET, MYO_F_QPOS, MYO_F_ACT).  The exception is the pen's obj_des_pos, a constant of the batch, held to the forward pass's
site_xpos within POS_TOL of tests/test_gpu_forward.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# an id per task (the ten of tests/test_obs_terms_host.py IDS)
IDS = ("myoHandPoseRandom-v0", "myoHandReachRandom-v0", "myoHandObjHoldRandom-v0", "myoHandKeyTurnRandom-v0", "myoHandPenTwirlRandom-v0",
       "myoLegStandRandom-v0", "myoLegWalk-v0", "myoLegRoughTerrainWalk-v0", "myoChallengeBaodingP1-v1", "myoChallengeDieReorientP1-v0")
BS = (3, 130)
STEPS = 3
POS_TOL = 5e-6          # tests/test_gpu_forward.py POS_TOL: the bound it holds forward().site_xpos to against the float64 oracle


def _np(x):
    return x.detach().cpu().numpy().copy() if hasattr(x, "detach") else np.array(x)


def _actions(env, steps=STEPS):
    rng = np.random.default_rng(7)
    return [rng.uniform(-1, 1, (env.num_envs, env.act_dim)).astype(np.float32) for _ in range(steps)]


@functools.lru_cache(maxsize=None)
def run(env_id, B, keys=None, **kw):
    """reset(seed=0) and three steps of the same actions.  keys: None = the defaults (no rows), "dict" = obs_dict=True, "reversed" = the
    default keys reversed, or a tuple of keys.  Returns the env (not to be stepped again) and host copies of what every step returned and
    of the state after the last one."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    if keys == "dict":
        kw = dict(kw, obs_dict=True)
    elif keys == "reversed":
        kw = dict(kw, obs_keys=list(reversed(run(env_id, B)[0].obs_keys)))
    elif keys is not None:
        kw = dict(kw, obs_keys=list(keys))
    env = myo.make(env_id, num_envs=B, **kw)
    out = dict(obs=[_np(env.reset(seed=0))], rew=[], done=[], trunc=[])
    for a in _actions(env):
        obs, rew, done, trunc, info = env.step(a)
        out["obs"].append(_np(obs)); out["rew"].append(_np(rew)); out["done"].append(_np(done)); out["trunc"].append(_np(trunc))
    out["info"] = info
    for name in ("F_QPOS", "F_OBS", "F_TIME", "F_TARGET", "F_ACT"):
        out[name] = env.batch.read(getattr(capi, name))
    if keys is not None:
        out["obs_dict"] = {k: _np(v) for k, v in env.obs_dict.items()}
    return env, out


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("env_id", IDS)
def test_default_selection_changes_nothing(env_id, B):
    """An env made with obs_dict=True and one made without step the same states and return the same rows, bit for bit; canonical_obs is the
    returned row.  (The two walk ids observe inside the step launch: the fused path.)"""
    e0, r0 = run(env_id, B)
    e1, r1 = run(env_id, B, "dict")
    assert e0.obs_dim == e1.obs_dim == e1.canonical_obs_dim and e0.obs_keys == e1.obs_keys and e1.proprio_keys is None
    assert e1._obs_in_step == (e1.spec["task"] == "walk")
    for k in ("obs", "rew", "done", "trunc"):
        for a, b in zip(r0[k], r1[k]):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (env_id, k)
    assert np.array_equal(r0["F_QPOS"], r1["F_QPOS"]) and np.array_equal(r0["F_OBS"], r1["F_OBS"])
    assert np.array_equal(_np(e1.canonical_obs), r1["obs"][-1]) and r1["obs"][-1].shape == (B, e1.obs_dim)
    assert "obs_dict" not in r0["info"] and "proprio_dict" not in r0["info"] and "proprio_dict" not in r1["info"]
    assert sorted(r1["info"]["obs_dict"]) == sorted(r1["obs_dict"])
    with pytest.raises(AttributeError, match="made without obs_dict=True"):
        e0.obs_dict
    assert e0.get_proprioception() is None and e1.get_proprioception() is None


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("env_id", IDS)
def test_terms_are_copies(env_id, B):
    """Every term of the canonical row equals its slice of it; time and t equal MYO_F_TIME, target_pos MYO_F_TARGET, the die's hand_qpos
    qpos[:, :-6], an act outside the row the muscles' MYO_F_ACT.  All exact."""
    from myosuite_mjx_amd import observations as O
    env, r = run(env_id, B, "dict")
    od, task = r["obs_dict"], env.spec["task"]
    width = env._obs_width
    assert list(od) == [k for k in O.term_names(task) if width[k] > 0] and all(od[k].shape == (B, width[k]) and od[k].dtype == np.float32 for k in od)
    at = 0
    for k in env.obs_keys:                        # the default keys: the canonical row's layout
        assert np.array_equal(od[k], r["F_OBS"][:, at:at + width[k]], equal_nan=True), (env_id, k)
        assert env.obs_slices[k] == slice(at, at + width[k])
        at += width[k]
    assert at == r["F_OBS"].shape[1]
    outside = set(od) - set(env.obs_keys)
    assert "time" in outside and np.array_equal(od["time"], r["F_TIME"]) and (r["F_TIME"] > 0).any()
    if task == "walk":
        assert np.array_equal(od["t"], r["F_TIME"])
    if task in ("reach", "stand"):
        assert np.array_equal(od["target_pos"], r["F_TARGET"]) and np.abs(od["target_pos"]).max() > 0
        assert np.abs(od["target_pos"] - od["tip_pos"] - od["reach_err"]).max() < 1e-6        # (the kernel's own subtraction, on these values)
    if task == "die":
        assert np.array_equal(od["hand_qpos"], r["F_QPOS"][:, :-6]) and np.array_equal(od["hand_qpos"][:, :-1], od["hand_qpos_noMD5"])
    if task in ("baoding", "die"):
        muscles = np.asarray(env.mjmodel.actuator_kind) == 0
        assert np.array_equal(od["act"], r["F_ACT"][:, muscles]) and np.abs(od["act"]).max() > 0
    want = {"pose": {"time"}, "reach": {"time", "target_pos"}, "stand": {"time", "target_pos"}, "hold": {"time"}, "keyturn": {"time"},
            "pen": {"time", "obj_des_pos"}, "walk": {"t", "time"}, "baoding": {"time", "act"}, "die": {"time", "hand_qpos", "act"}}[task]
    assert outside == want


@pytest.mark.parametrize("B", BS)
def test_pen_obj_des_pos_is_the_eps_ball_site(B):
    env, r = run("myoHandPenTwirlRandom-v0", B, "dict")
    sid = env.mjmodel.name2id("site", "eps_ball")
    ref = _np(env.forward().site_xpos)[:, sid]
    got = r["obs_dict"]["obj_des_pos"]
    assert got.shape == ref.shape == (B, 3) and np.abs(got - ref).max() < POS_TOL, np.abs(got - ref).max()
    assert np.abs(got).min() > 0.1                                                            # a real position (-.230 -.530 1.445), not zeros


def _check_selection(env, r, keys):
    od, obs = r["obs_dict"], r["obs"][-1]
    assert env.obs_keys == list(keys) and env.obs_dim == sum(od[k].shape[1] for k in keys) == obs.shape[1]
    assert env.observation_space.shape == (env.obs_dim,)
    for o in r["obs"]:
        assert o.shape == (env.num_envs, env.obs_dim)
    assert np.array_equal(obs, np.concatenate([od[k] for k in keys], axis=1), equal_nan=True)
    back = env.obsvec2obsdict(obs)
    assert list(back) == list(dict.fromkeys(keys)) and all(np.array_equal(back[k], od[k], equal_nan=True) for k in back)
    assert np.array_equal(_np(env.canonical_obs), r["F_OBS"]) and r["F_OBS"].shape[1] == env.canonical_obs_dim


@pytest.mark.parametrize("B", BS)
def test_selection_with_a_repeated_key(B):
    keys = ("qpos", "time", "act", "qpos")
    env, r = run("myoHandPoseRandom-v0", B, keys)
    _check_selection(env, r, keys)
    assert env.obs_dim == 23 + 1 + 39 + 23
    e0, r0 = run("myoHandPoseRandom-v0", B)                                                   # the selection does not touch the stepping
    assert np.array_equal(r0["F_QPOS"], r["F_QPOS"]) and np.array_equal(r0["F_OBS"], r["F_OBS"]) and np.array_equal(r0["rew"][-1], r["rew"][-1])


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("env_id", IDS)
def test_selection_reversed_defaults(env_id, B):
    env, r = run(env_id, B, "reversed")
    e0, r0 = run(env_id, B)
    keys = list(reversed(e0.obs_keys))
    _check_selection(env, r, keys)
    assert env.obs_dim == e0.obs_dim and np.array_equal(r0["F_OBS"], r["F_OBS"])
    if len(keys) > 1:
        assert not np.array_equal(r["obs"][-1], r0["obs"][-1])


def test_proprio_keys_and_numpy_io():
    import myosuite_mjx_amd as myo
    env, r = run("myoHandPoseRandom-v0", 130, None, proprio_keys=("qpos", "qvel"))
    assert env.proprio_keys == ["qpos", "qvel"] and env.obs_dim == env.canonical_obs_dim and "obs_dict" in r["info"]
    t, vec, d = env.get_proprioception()
    od = {k: _np(v) for k, v in env.obs_dict.items()}
    assert list(d) == ["time", "qpos", "qvel"] == list(r["info"]["proprio_dict"])
    assert np.array_equal(_np(vec), np.concatenate([od["qpos"], od["qvel"]], axis=1)) and _np(vec).shape == (130, 46)
    assert np.array_equal(_np(t), od["time"]) and all(np.array_equal(_np(d[k]), od[k]) for k in d)
    assert vec.data_ptr() == env.get_proprioception()[1].data_ptr()                          # a view of the library's row, not a copy
    assert env.obs_dict["qpos"].data_ptr() == env.view(myo.capi.OBS_TERMS, "obs")[:, 1:].data_ptr()
    # a single string is one key; as_torch=False returns numpy copies
    e2 = myo.make("myoHandPoseRandom-v0", num_envs=3, proprio_keys="pose_err", obs_keys=["pose_err", "qpos"], as_torch=False)
    obs = e2.reset(seed=0)
    obs, *_ , info = e2.step(np.zeros((3, e2.act_dim), np.float32))
    assert isinstance(obs, np.ndarray) and e2.proprio_keys == ["pose_err"] and e2.obs_keys == ["pose_err", "qpos", "act"]
    od2 = e2.obs_dict
    assert isinstance(od2["qpos"], np.ndarray) and np.array_equal(obs, np.concatenate([od2[k] for k in e2.obs_keys], axis=1))
    assert np.array_equal(e2.get_proprioception()[1], od2["pose_err"]) and np.array_equal(info["proprio_dict"]["pose_err"], od2["pose_err"])
    assert np.array_equal(e2.canonical_obs, e2.batch.read(myo.capi.F_OBS))


def test_autoreset_rows_describe_the_returned_observation():
    """Half the envs reach the time limit inside the run.  For them the rows are those of the new episode's first observation (time 0, the
    row a reset of the same seed and episode gives); for the others the second launch of the terms kernel (after the auto-reset's
    observation pass) rewrites what the first one wrote."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    keys, B = ["time", "qpos", "pose_err"], 130
    acts = _actions(myo.make("myoHandPoseRandom-v0", num_envs=B), 2)

    def two_steps(**kw):
        env = myo.make("myoHandPoseRandom-v0", num_envs=B, obs_keys=keys, **kw)
        env.reset(seed=0)
        _, _, done0, trunc0, _ = env.step(acts[0])
        el = env.batch.read(capi.F_ELAPSED)
        el[::2] = env.max_episode_steps - 1                        # the even envs are truncated by the next step
        env.batch.write(capi.F_ELAPSED, el)
        obs, rew, done, trunc, info = env.step(acts[1])
        return env, _np(obs), _np(done), _np(trunc), {k: _np(v) for k, v in info["obs_dict"].items()}, _np(done0) | _np(trunc0)

    env, obs, done, trunc, od, earlier = two_steps()
    was_reset = done | trunc
    assert trunc[::2].all() and not trunc[1::2].any() and was_reset[::2].all() and 0 < (~was_reset).sum()
    assert (od["time"][was_reset] == 0).all() and (od["time"][~was_reset] > 0).all()
    assert np.array_equal(obs, np.concatenate([od[k] for k in env.obs_keys], axis=1))
    assert np.array_equal(_np(env.canonical_obs)[:, :23], od["qpos"])
    # the envs that were not reset: the same env without auto-reset runs the terms kernel once per step
    e1, obs1, done1, trunc1, od1, _ = two_steps(autoreset=False)
    assert np.array_equal(done1, done) and np.array_equal(trunc1, trunc)
    assert np.array_equal(obs[~was_reset], obs1[~was_reset]) and not np.array_equal(obs[was_reset], obs1[was_reset])
    # the envs that were reset: episode 1 of the same seed, which a second reset() of a fresh env starts in every env
    e2 = myo.make("myoHandPoseRandom-v0", num_envs=B, obs_keys=keys)
    e2.reset(seed=0)
    first = _np(e2.reset(seed=0))
    only_timeout = trunc & ~done & ~earlier                        # (an env the first step had already reset is one episode further)
    assert only_timeout.sum() > 0 and np.array_equal(obs[only_timeout], first[only_timeout])


def test_one_ppo_iteration_on_a_selected_row():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import ppo
    env = myo.make("myoHandPoseRandom-v0", num_envs=64, obs_keys=["qpos", "pose_err"])
    assert env.obs_keys == ["qpos", "pose_err", "act"] and env.obs_dim == 23 + 23 + 39 and env.canonical_obs_dim == 108
    pol, params, metrics = ppo.train(env, 1, unroll_length=2, num_minibatches=2, num_updates_per_batch=1, seed=3)
    assert len(metrics) == 1 and pol is not None and pol.obs_dim == env.obs_dim
    assert np.isfinite(metrics[0]["policy_loss"]) and np.isfinite(metrics[0]["value_loss"])


def test_library_refusals():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    track = myo.make("MyoHandAirplaneFixed-v0", num_envs=2)
    assert track.batch.obs_terms() == ()
    with pytest.raises(capi.MyoError, match="no task with a term table is configured"):
        track.batch.enable_obs_terms([0])
    env = myo.make("myoHandPoseRandom-v0", num_envs=2)
    assert env.batch.obs_terms() == (("time", 1), ("qpos", 23), ("qvel", 23), ("act", 39), ("pose_err", 23))
    with pytest.raises(capi.MyoError, match="not enabled"):
        env.batch.buffer_ptr("obs", capi.OBS_TERMS)
    for bad in ([5], [-1], [0, 99]):
        with pytest.raises(capi.MyoError, match="term index out of range"):
            env.batch.enable_obs_terms(bad)
    with pytest.raises(capi.MyoError, match="term index out of range"):
        env.batch.enable_obs_terms([0], [7])
    with pytest.raises(capi.MyoError, match="at least one obs term"):
        env.batch.enable_obs_terms([])
    with pytest.raises(capi.MyoError, match="not enabled"):                                  # a refused call allocated nothing
        env.batch.buffer_ptr("obs", capi.OBS_SELECTED)
    env.batch.enable_obs_terms([1])
    assert env.batch.buffer_ptr("obs", capi.OBS_SELECTED)[1:] == (23, 23) and env.batch.buffer_ptr("obs", capi.OBS_TERMS)[1:] == (109, 109)
    with pytest.raises(capi.MyoError, match="no proprio terms"):
        env.batch.buffer_ptr("obs", capi.OBS_PROPRIO)
    with pytest.raises(capi.MyoError, match="already enabled"):
        env.batch.enable_obs_terms([2])
    walk = myo.make("myoLegWalk-v0", num_envs=2)                                             # the walk task observes in the wave kernel only
    capi.set_lanes(32)
    try:
        with pytest.raises(capi.MyoError, match="wave-per-env kernel only"):
            walk.batch.enable_obs_terms([0])
    finally:
        capi.set_lanes(64)
    walk.batch.enable_obs_terms([0])
    bare = capi.HipBatch(env.model, 2)                                                        # no task configured
    with pytest.raises(capi.MyoError, match="no task with a term table is configured"):
        bare.enable_obs_terms([0])


def test_guard_poisoned_build():
    import hand_task_checks as H
    H.rerun_file_against_poison_build(__file__, timeout=900)
