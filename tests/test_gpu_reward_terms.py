"""GPU tests of the reward-term rows, weighted_reward_keys, rwd_mode and the episode statistics of the batched envs
(make(..., rwd_dict=True, weighted_reward_keys=..., rwd_mode=..., episode_stats=True)), one id per task kernel.

Small batches: one wave is one env, so 96 envs cover every kernel; three steps put the time past the two env steps after which the reach /
stand tasks' far_th counts.  Before the steps half the envs get their object moved 0.5 m down (hold, pen, baoding, die) or their pelvis
lowered (stand: 0.9 m, walk: 0.4 m; on the float64 oracle the contacts lift the pelvis by 0.1 m per step at most, which leaves the stand envs
0.58 m from their target, beyond far_th = 0.44, and the walk envs at 0.69 m, below min_height = 0.8, after the three steps), so `done`
and the penalty column take both values in every task.  The float64 side is tests/reward_terms_ref.py, evaluated on the read-back state.

Bounds: continuous columns 1e-5 (what the env-API tests hold the observation row to; the terms are norms and sums of such entries, of
magnitude <= 10); step-valued columns equal wherever the deciding quantity is farther than that from every threshold, with at most 2 % of
a task's envs left out; dense against the float64 sum of the stored row: 16 * 2^-24 * sum |w_k row_k|, the float32 rounding bound of a sum
of up to 16 products; an episode's return against the float64 sum of its L returned rewards: L * 2^-23 * sum |r_i| (L float32 additions
of float32 terms)."""
import functools

import numpy as np
import pytest

import hand_task_checks as H
import reward_terms_ref as R

pytestmark = pytest.mark.gpu

IDS = ("myoHandPoseRandom-v0", "myoHandReachRandom-v0", "myoHandObjHoldRandom-v0", "myoLegStandRandom-v0", "myoLegWalk-v0",
       "myoLegRoughTerrainWalk-v0", "myoHandKeyTurnRandom-v0", "myoHandPenTwirlRandom-v0", "myoChallengeBaodingP1-v1",
       "myoChallengeDieReorientP1-v0", "myoFatiHandPoseRandom-v0")
B, STEPS, BAND = 96, 3, 1e-5
STATE_FIELDS = ("F_QPOS", "F_QVEL", "F_ACT", "F_OBS", "F_DONE", "F_SOLVED", "F_ELAPSED")
READ = STATE_FIELDS + ("F_TARGET", "F_TIME", "F_SITEXPOS", "F_REWARD")


def _custom_weights(keys):
    """A dict that drops the task's first two terms and weights `done`."""
    return dict({k: 0.5 + i for i, k in enumerate(keys[2:-4])}, done=-3.0)


def _perturb(env):
    """Half the envs (the odd ones) get their object moved 0.5 m down / their pelvis lowered, before the steps."""
    from myosuite_mjx_amd import capi
    task, q = env.spec["task"], env.batch.read(capi.F_QPOS)
    col, by = {"hold": (-5, 0.5), "baoding": (-12, 0.5), "pen": (-4, 0.5), "die": (-4, 0.5), "stand": (2, 0.9), "walk": (2, 0.4)}.get(task, (None, 0.0))
    if col is None:
        return
    q[1::2, col] -= by
    if task == "baoding":
        q[1::2, -5] -= by                                       # both balls
    env.batch.write(capi.F_QPOS, q)


@functools.lru_cache(maxsize=None)
def run(env_id, mode="off"):
    """Three steps of the same seed and actions; mode "off": the defaults, "on": rwd_dict=True, "custom": the custom weights and
    rwd_mode="sparse".  Returns the env, the last step's outputs and the read-back fields."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi, rewards
    keys = rewards.RWD_KEYS[myo.envs.REGISTRY[env_id]["task"]]
    kw = {"off": {}, "on": dict(rwd_dict=True), "custom": dict(weighted_reward_keys=_custom_weights(keys), rwd_mode="sparse")}[mode]
    env = myo.make(env_id, num_envs=B, seed=5, as_torch=False, autoreset=False, **kw)
    env.reset()
    _perturb(env)
    rng = np.random.default_rng(2)
    for _ in range(STEPS):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (B, env.act_dim)).astype(np.float32))
    fields = {f: env.batch.read(getattr(capi, f)) for f in READ}
    return env, (obs, rew, term, trunc, info), fields


def _helper_inputs(env, fields):
    """The helper's inputs for the env's task from the read-back state (and, for the walk task, the quantities of the observation row)."""
    spec, m, f = env.spec, env.mjmodel, fields
    task, act = spec["task"], fields["F_ACT"]
    q, sx = f["F_QPOS"], f["F_SITEXPOS"]
    if task == "pose":
        return dict(qpos=q, target=f["F_TARGET"], act=act, pose_thd=spec["pose_thd"])
    if task == "reach":
        n = len(spec["tips"])
        return dict(tips=sx, target=f["F_TARGET"], act=act, time=f["F_TIME"][:, 0], dt=env.dt, far_th=spec["far_th"] * n, near_th=0.0125 * n)
    if task == "hold":
        return dict(obj_pos=q[:, -7:-4], goal=f["F_TARGET"], act=act, goal_th=spec["goal_th"], drop_th=spec["drop_th"])
    if task == "stand":
        from myosuite_mjx_amd.mjcf import quat2mat
        lpos = np.asarray(m.hip_site_lpos[m.name2id("site", spec["tip"])], float)
        q64 = q.astype(np.float64)
        tip = np.stack([r[:3] + quat2mat(r[3:7] / np.linalg.norm(r[3:7])) @ lpos for r in q64])
        return dict(tip=tip, target=f["F_TARGET"], qvel=f["F_QVEL"], act=act, time=f["F_TIME"][:, 0], dt=env.dt, far_th=spec["far_th"], near_th=spec["near_th"])
    if task == "walk":
        sb = m.nq - 2 + m.nv
        o = f["F_OBS"]
        jadr = lambda n: int(m.jnt_qposadr[m.name2id("joint", n)])
        return dict(com_vel=o[:, sb:sb + 2], height=o[:, sb + 8], feet_heights=o[:, sb + 6:sb + 8], phase=o[:, sb + 15], qpos=q, act=act,
                    qadr_hip_flexion=(jadr("hip_flexion_l"), jadr("hip_flexion_r")),
                    qadr_joint_angle=[jadr(n) for n in ("hip_adduction_l", "hip_adduction_r", "hip_rotation_l", "hip_rotation_r")],
                    target_rot=np.asarray(m.key_qpos).reshape(-1, m.nq)[0][3:7], min_height=spec["min_height"], max_rot=spec["max_rot"],
                    target_x_vel=spec["target_x_vel"], target_y_vel=spec["target_y_vel"], knee_height=spec.get("knee_height", 0.0))
    if task == "keyturn":
        return dict(qpos=q, sites=sx, act=act, goal_th=spec["goal_th"])
    if task == "pen":
        return dict(sites=sx, obj_pos=f["F_OBS"][:, 23:26], act=act)
    if task == "baoding":
        return dict(sites=sx, act=act, drop_th=spec["drop_th"], proximity_th=spec["proximity_th"])
    return dict(sites=sx, act=act, pos_th=spec["pos_th"], rot_th=spec["rot_th"], drop_th=spec["drop_th"])


@pytest.mark.parametrize("env_id", IDS)
def test_off_is_off(env_id):
    """An env made with the defaults and one made with rwd_dict=True step the same states bit for bit; the rewards agree to the bound of
    test_env_api_matches_restatement (the dense column is a re-associated float32 sum); the default env's info is today's."""
    _, (obs0, rew0, term0, trunc0, info0), f0 = run(env_id, "off")
    env, (obs1, rew1, term1, trunc1, info1), f1 = run(env_id, "on")
    for f in STATE_FIELDS:
        assert np.array_equal(f0[f], f1[f]), f
    assert np.array_equal(obs0, obs1) and np.array_equal(term0, term1) and np.array_equal(trunc0, trunc1)
    print(env_id, "max |r_on - r_off|", np.abs(rew0 - rew1).max(), "max |r|", np.abs(rew0).max())
    assert np.abs(rew0 - rew1).max() <= 1e-3 * max(1.0, np.abs(rew0).max())
    assert sorted(info0) == ["solved", "time"]
    assert sorted(info1) == ["rwd_dense", "rwd_dict", "rwd_sparse", "solved", "time"] and tuple(info1["rwd_dict"]) == env.rwd_keys
    assert env.batch.rwd_names() == env.rwd_keys and np.array_equal(info1["rwd_dense"], rew1) and np.array_equal(info1["rwd_dense"], f1["F_REWARD"][:, 0])


@pytest.mark.parametrize("env_id", IDS)
def test_row_against_float64(env_id):
    env, (obs, rew, term, trunc, info), fields = run(env_id, "on")
    row, margin = R.terms(env.spec["task"], **_helper_inputs(env, fields))
    got = info["rwd_dict"]
    assert set(row) | {"dense"} == set(got)
    clear = margin > BAND
    print(env_id, "left out", (~clear).mean(), "done", row["done"].mean())
    assert (~clear).mean() <= 0.02
    for k, ref in row.items():
        if k in R.STEP_COLUMNS:
            assert np.array_equal(got[k][clear], ref[clear].astype(np.float32)), k
        else:
            err = np.abs(got[k].astype(np.float64) - ref).max()
            print(f"  {k}: max err {err:.2e} max |ref| {np.abs(ref).max():.3g}")
            assert err <= 1e-5, (k, err)
    assert 0 < row["done"].mean() < 1 if env.spec["task"] not in ("pose", "reach", "keyturn") else True     # both values where the states were moved
    assert np.array_equal(got["done"] > 0, term) and np.array_equal(got["solved"] > 0, info["solved"])


def _check_sum(env, row, dense):
    w = np.asarray([env.rwd_weights.get(k, 0.0) for k in env.rwd_keys[:-1]], np.float32).astype(np.float64)
    prod = w[None, :] * row[:, :-1].astype(np.float64)
    err, bound = np.abs(dense.astype(np.float64) - prod.sum(axis=1)), 16 * 2.0 ** -24 * np.abs(prod).sum(axis=1)
    print(env.id, "worst |dense - sum| / bound", (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (err - bound).max()


@pytest.mark.parametrize("env_id", IDS)
def test_dense_is_the_weighted_sum(env_id):
    """With the registered weights, and with a dict that drops two keys and weights `done`; with rwd_mode="sparse" the returned reward is
    the sparse column, info["rwd_dense"] keeps the weighted sum."""
    env, (_, rew, _, _, info), _ = run(env_id, "on")
    assert env.rwd_weights == {k: w for k, w in env.spec["weights"].items() if w != 0}
    _check_sum(env, env.rwd_terms, info["rwd_dense"])
    on_row = env.rwd_terms
    env, (_, rew, _, _, info), fields = run(env_id, "custom")
    row = env.rwd_terms
    assert env.rwd_weights == {k: w for k, w in _custom_weights(env.rwd_keys).items() if w != 0} and env.rwd_weights["done"] == -3.0
    assert np.array_equal(row[:, :-1], on_row[:, :-1])                       # the terms do not depend on the weights
    _check_sum(env, row, info["rwd_dense"])
    assert np.array_equal(rew, info["rwd_sparse"]) and np.array_equal(rew, row[:, -4]) and np.array_equal(fields["F_REWARD"][:, 0], row[:, -4])
    assert np.array_equal(info["rwd_dense"], row[:, -1]) and not np.array_equal(info["rwd_dense"], on_row[:, -1])


@pytest.mark.parametrize("env_id,ends", (("myoHandPenTwirlRandom-v0", None), ("myoLegWalk-v0", "done"), ("myoHandPoseRandom-v0", "timelimit")))
def test_episode_statistics(env_id, ends):
    """150 auto-reset steps of U(-1, 1) actions on 64 envs against a host that accumulates the returned rewards in float64 and cuts at
    terminated | truncated.  The walk envs fall (done), the pose envs run into their TimeLimit; the pen envs end either way."""
    import myosuite_mjx_amd as myo
    N, T = 64, 150
    env = myo.make(env_id, num_envs=N, seed=3, as_torch=False, autoreset=True, episode_stats=True)
    assert env.rwd_dict and sorted(env.rwd_weights) == sorted(k for k, w in env.spec["weights"].items() if w != 0)
    env.reset()
    rng = np.random.default_rng(4)
    acc = np.zeros((N, 6))                                                    # sum r, sum |r|, sum sparse, sum |sparse|, length, solved
    cuts, n_done, n_trunc, worst = np.zeros(N, int), 0, 0, 0.0
    for _ in range(T):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (N, env.act_dim)).astype(np.float32))
        sp = info["rwd_sparse"].astype(np.float64)
        r = rew.astype(np.float64)
        acc += np.stack([r, np.abs(r), sp, np.abs(sp), np.ones(N), info["solved"].astype(float)], axis=1)
        ep, cut = info["episode"], term | trunc
        assert np.array_equal(ep["finished"], cut)
        assert ep["l"].dtype == np.int32 and ep["solved"].dtype == np.int32
        assert np.array_equal(ep["l"][cut], acc[cut, 4].astype(np.int32)) and np.array_equal(ep["solved"][cut], acc[cut, 5].astype(np.int32))
        tol = acc[:, 4] * 2.0 ** -23
        assert (np.abs(ep["r"] - acc[:, 0]) <= tol * acc[:, 1])[cut].all() and (np.abs(ep["r_sparse"] - acc[:, 2]) <= tol * acc[:, 3])[cut].all()
        if cut.any():
            worst = max(worst, (np.abs(ep["r"] - acc[:, 0]) / np.maximum(tol * acc[:, 1], 1e-300))[cut].max())
        cuts += cut
        n_done, n_trunc = n_done + int(term.sum()), n_trunc + int(trunc.sum())
        acc[cut] = 0.0
    print(env_id, "episodes by done", n_done, "by TimeLimit", n_trunc, "worst |r - host| / bound", worst)
    assert np.array_equal(env.episode_count, cuts) and cuts.sum() == n_done + n_trunc > 0
    assert n_done > 0 if ends == "done" else (n_trunc > 0 if ends == "timelimit" else True)
    running = env.batch.read_episode(myo.capi.EP_RUNNING)
    assert np.array_equal(running[:, 2], acc[:, 4].astype(np.float32))       # the episodes under way
    env.reset()
    assert not env.batch.read_episode(myo.capi.EP_RUNNING).any() and np.array_equal(env.episode_count, cuts)   # reset clears the running rows only


def test_episode_statistics_without_autoreset_and_torch_views():
    """autoreset=False: the caller resets; the statistics still cut where an episode ends.  as_torch=True: info holds views of the
    library's buffers that read what the host copies read."""
    import torch
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make("myoHandPoseRandom-v0", num_envs=8, seed=1, autoreset=False, episode_stats=True)
    env.max_episode_steps = 3                                                 # (the TimeLimit step() and the statistics go by)
    env.reset()
    g = torch.Generator().manual_seed(0)
    total, early = torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.bool)
    for t in range(3):
        obs, rew, term, trunc, info = env.step(torch.rand((8, env.act_dim), generator=g) * 2 - 1)
        total += rew.double().cpu()
        fin = info["episode"]["finished"]
        assert fin.dtype == torch.bool and fin.is_cuda and torch.equal(fin, term | trunc) and bool(trunc.any()) == (t == 2)
        early |= term.cpu() & (t < 2)
    ep, whole = info["episode"], ~early                                       # an env that was done before keeps ending one-step episodes
    assert whole.any() and bool((term | trunc).all())
    assert ep["l"].dtype == torch.int32 and ep["l"].cpu()[whole].tolist() == [3] * int(whole.sum())
    assert (ep["r"].double().cpu() - total)[whole].abs().max() < 1e-5 * max(1.0, float(total.abs().max()))
    row = env.rwd_terms
    assert row.is_cuda and tuple(row.shape) == (8, len(env.rwd_keys)) and np.array_equal(row.cpu().numpy(), env.batch.read_rwd())
    assert np.array_equal(info["rwd_dict"]["pose"].cpu().numpy(), env.batch.read_rwd()[:, 0]) and torch.equal(info["rwd_dense"], rew)
    assert env.episode_count.dtype == torch.int32 and env.episode_count.cpu()[whole].tolist() == [1] * int(whole.sum())
    assert np.array_equal(env.batch.read_episode(capi.EP_FINISHED), np.ones(8, np.uint8))
    env.reset()                                                               # the caller's reset
    assert not env.batch.read_episode(capi.EP_RUNNING).any() and not env.batch.read_episode(capi.EP_FINISHED).any()


def test_abi_refusals_and_trace_rollout():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi, trace
    env = myo.make("myoHandPoseRandom-v0", num_envs=4, as_torch=False, autoreset=False)
    b = env.batch
    with pytest.raises(capi.MyoError, match="error -1"):                      # not enabled: no row, no statistics
        b.rwd_row_ptr()
    with pytest.raises(capi.MyoError, match="error -1"):
        b.enable_episode_stats()
    with pytest.raises(capi.MyoError, match="error -1"):                      # one weight per column except dense
        b.enable_rewards(np.ones(3, np.float32))
    with pytest.raises(capi.MyoError, match="error -1"):
        b.enable_rewards(np.ones(7, np.float32), mode=2)
    with pytest.raises(AttributeError):
        env.rwd_terms
    bare = capi.HipBatch(env.model, 4)                                        # no task configured: no columns
    assert bare.rwd_names() == ()
    with pytest.raises(capi.MyoError, match="error -4"):
        bare.enable_rewards(np.ones(7, np.float32))
    plain = trace.rollout(env, horizon=3, seed=0)
    env = myo.make("myoHandPoseRandom-v0", num_envs=4, as_torch=False, autoreset=False, rwd_dict=True)
    root = trace.rollout(env, horizon=3, seed=0)
    (t0,), (t1,) = (list(r.values()) for r in (plain, root))
    extra = {"env_infos/rwd_sparse"} | {f"env_infos/rwd_dict/{k}" for k in env.rwd_keys}
    assert set(t1["Trial0"]) - set(t0["Trial0"]) == extra and not set(t0["Trial0"]) - set(t1["Trial0"])
    for name, trial in t1.items():
        assert np.array_equal(trial["env_infos/rwd_dict/dense"], trial["env_infos/rwd_dense"]) and np.array_equal(trial["env_infos/rwd_dense"], trial["rewards"])
        assert np.array_equal(trial["env_infos/rwd_sparse"], trial["env_infos/rwd_dict/pose"]) and trial["env_infos/rwd_dict/pose"][-1] < 0
        assert np.array_equal(trial["observations"], t0[name]["observations"])


def test_guard_poisoned_build():
    H.rerun_file_against_poison_build(__file__, timeout=900)
