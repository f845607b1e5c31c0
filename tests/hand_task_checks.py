"""What the tests of the TrackEnv-class hand tasks (key turn, pen twirl, baoding, die) share: one `TaskCase` record per task, kept next to
the task's GPU tests, and the checks that are the same for every task, as plain functions that assert.  tests/test_gpu_<task>.py and
tests/test_<task>_host.py keep what is the task's own (states, tolerances, shares, branch coverage) and call these; a new task adds its
two files and a record.  tests/test_hand_task_checks_host.py shows on synthetic data that the assertions here fire."""
import os
import subprocess
import sys
from typing import Callable, NamedTuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRK = "step_kernel_w<36,20,32,2,2,false,0,false,true>"
SEED = 7                                                     # of the reset-draw tests; the "other seed" is SEED + 1
CONDITIONS = (("Sarc", "sarcopenia"), ("Fati", "fatigue"), ("Reaf", "reafferentation"))


class TaskCase(NamedTuple):
    stem: str                     # committed asset
    task: str                     # its name in envs.REGISTRY / tasks.TASKS (the capi id is configure's business)
    env_ids: tuple                # the ids test_every_id_steps is parametrised over
    bench_id: str                 # the id with per-env reset draws: fused epilogue, reset draws
    obs_dim: int
    nsub: int                     # substeps per env step (frame_skip)
    configure: Callable           # configure(b, m): the task on a bare HipBatch, as tasks.TASKS sets it up
    extra_fields: tuple = ()      # capi field names the fused-epilogue check compares on top of the common ones
    make_kwargs: dict = {}        # of the fused-epilogue check's envs
    nu: int = 39
    kernel: str = TRK


def new_batch(case, m, n):
    from myosuite_mjx_amd import capi
    b = capi.HipBatch(capi.HipModel(m.blob(), 0), n)
    case.configure(b, m)
    return b


def forward_at(o, qpos):
    o.reset()
    o.set_state(qpos=qpos)
    o.forward()
    return o


def site_xpos(o, m, names):
    x = o.field("site_xpos").reshape(-1, 3)
    return np.concatenate([x[m.name2id("site", n)] for n in names])


# ---- GPU side -------------------------------------------------------------------------------------------------------------------------

def fused_epilogue_equals_stepwise(case):
    """myo_bench_rollout's one-launch epilogue (task_post_kernel) = step, myo_obs, myo_autoreset, myo_obs_reset_only, bit for bit, over
    five steps of 512 envs with episodes of two steps.  Returns the fused batch."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B, seed, T = 512, 3, 5
    envs = [myo.make(case.bench_id, num_envs=B, seed=1, as_torch=False, **case.make_kwargs) for _ in range(2)]
    for e in envs:
        e.reset()
    a, r = envs
    a.batch.bench_rollout(T, case.nsub, seed=seed, mode=capi.BENCH_OBS | capi.BENCH_FRESH_ACTIONS | capi.BENCH_AUTORESET, max_episode_steps=2)
    ptr = r.batch.field_ptr(capi.F_ACTION)[0]
    for t in range(T):
        r.batch.random_action(ptr, seed, t)
        r.batch.step(ptr, capi.ACTMAP_MUSCLE_SIGMOID, case.nsub)
        r.batch.obs()
        r.batch.autoreset(2, seed)
        r.batch.obs_reset_only()
    for f in ("F_QPOS", "F_QVEL", "F_ACT", "F_OBS", "F_REWARD", "F_DONE", "F_SOLVED", "F_ELAPSED", "F_SITEXPOS") + case.extra_fields:
        assert np.array_equal(a.batch.read(getattr(capi, f)), r.batch.read(getattr(capi, f))), f
    assert a.batch.read(capi.F_ELAPSED).max() <= 2
    return a.batch


def bad_env_is_contained(case):
    """One bad env among 8 (include/myo_hip.h, "A bad env"; the checks are tests/bad_env.py's task_contained), by a NaN velocity and by a
    NaN action, through the env's step and observation pass.  The bad env is reset to qpos0 and flagged, its task rows are those of the
    reset state, every row is finite and the other seven envs are untouched bit for bit.  Then a NaN velocity through one step of
    myo_bench_rollout with its one-launch epilogue (task_post_kernel: observation, auto-reset, first observation of the new episodes):
    the env is flagged, every row is finite, the others are those of a clean batch bit for bit, and the bad env's rows are bit for bit
    what step, myo_obs, myo_autoreset, myo_obs_reset_only leave for the same injection."""
    import myosuite_mjx_amd as myo
    import bad_env as BE
    from myosuite_mjx_amd import capi

    def make(n):
        envs = [myo.make(case.bench_id, num_envs=8, seed=1, as_torch=False, autoreset=False, **case.make_kwargs) for _ in range(n)]
        for e in envs:
            e.reset()
        return envs
    for kind in ("nan_qvel", "nan_action"):
        env, clean = make(2)
        BE.task_contained(env, clean, kind, 5)
        assert env.batch.last_kernel_name() == case.kernel
    env, clean, stepwise = make(3)
    for e in (env, stepwise):
        e.batch.write(capi.F_QVEL, BE.inject("nan_qvel", {capi.F_QVEL: e.batch.read(capi.F_QVEL)}, (5,))[capi.F_QVEL])
    mode = capi.BENCH_OBS | capi.BENCH_FRESH_ACTIONS | capi.BENCH_AUTORESET
    for e in (env, clean):
        e.batch.bench_rollout(1, case.nsub, seed=3, mode=mode, max_episode_steps=env.max_episode_steps)
    b, ptr = stepwise.batch, stepwise.batch.field_ptr(capi.F_ACTION)[0]
    b.random_action(ptr, 3, 0)
    b.step(ptr, capi.ACTMAP_MUSCLE_SIGMOID, case.nsub)
    b.obs()
    b.autoreset(env.max_episode_steps, 3)
    b.obs_reset_only()
    rows, rows_clean, rows_step = (BE.read_all(BE.HipRows(e.batch, None)) for e in (env, clean, stepwise))
    flags = env.status()
    assert flags[5] & capi.FLAG_BAD_STATE and not (np.delete(flags, 5) & (capi.FLAG_BAD_STATE | capi.FLAG_BAD_QACC)).any()
    BE.assert_all_fields_finite(rows)
    BE.assert_neighbours_bitwise(rows, rows_clean, (5,))
    for f in ("F_QPOS", "F_QVEL", "F_ACT", "F_OBS", "F_REWARD", "F_DONE", "F_SOLVED", "F_ELAPSED", "F_SITEXPOS", "F_FLAGS"):      # (fused_epilogue_equals_stepwise's list)
        assert rows[getattr(capi, f)].tobytes() == rows_step[getattr(capi, f)].tobytes(), f


def every_id_steps(case, env_id):
    """Five env steps of U(-1, 1) actions at 256 envs: finite rows, the TRK kernel, no status flag, muscles activated.  Returns the env."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    env = myo.make(env_id, num_envs=256, seed=2, as_torch=False)
    obs = env.reset()
    assert obs.shape == (256, case.obs_dim)
    rng = np.random.default_rng(0)
    for _ in range(5):
        obs, rew, term, trunc, info = env.step(rng.uniform(-1, 1, (256, case.nu)).astype(np.float32))
        assert np.isfinite(obs).all() and np.isfinite(rew).all()
    assert env.batch.last_kernel_name() == case.kernel and not env.status().any()
    assert np.abs(env.batch.read(capi.F_ACT)).max() > 0
    return env


def rerun_file_against_poison_build(path, timeout):
    """The test file at `path` once more against libmyo_hip_poison.so (NaN-filled LDS, scratch and registers before every step launch)."""
    lib = os.path.join(ROOT, "myosuite_mjx_amd", "libmyo_hip_poison.so")
    assert os.path.exists(lib), "libmyo_hip_poison.so is missing: run __graft_entry__.build()"
    env = dict(os.environ, MYO_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not guard",
                        os.path.relpath(path, ROOT)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout


def assert_uniform(x, lo, hi):
    """Eight equal bins over [lo, hi]: every count within five standard deviations (sqrt(B / 8), the Poisson one) of B / 8."""
    B = len(x)
    h = np.histogram(x, bins=8, range=(lo, hi))[0]
    assert np.abs(h - B / 8).max() < 5 * np.sqrt(B / 8), h.tolist()


def assert_deterministic_and_sharded(make_env, read_draws, B, whole):
    """`whole` = read_draws of a reset make_env(B, SEED, 0).  The same seed draws the same, another seed draws something else in every
    array, and the two half batches at env_offset 0 and B // 2 draw what the whole batch draws for their envs."""
    env = make_env(B, SEED, 0)
    env.reset()
    for x, y in zip(read_draws(env), whole):
        assert np.array_equal(x, y)
    env.reset(seed=SEED + 1)
    for x, y in zip(read_draws(env), whole):
        assert not np.array_equal(x, y)
    for off in (0, B // 2):
        s = make_env(B // 2, SEED, off)
        s.reset()
        for x, y in zip(read_draws(s), whole):
            assert np.array_equal(x, y[off:off + B // 2]), off


def same_contacts(flags, ncon, ncon_oracle):
    """The envs a state comparison is fair on: no status flag, and as many contacts in the last substep as the oracle found."""
    return (np.asarray(flags) == 0) & (np.asarray(ncon) == np.asarray(ncon_oracle))


def step_and_compare_with_oracle(m, batch, state, nsub, oracle_for_env, after_env=None):
    """Write `state` ({field id: rows}; qpos, qvel, act, and either actions, mapped through the muscle sigmoid, or controls), step nsub
    substeps on the TRK kernel, and step oracle_for_env(e) from the same state with the controls the GPU used.  after_env(e, oracle), if
    given, sees each stepped oracle.  Returns max|dqpos| and max|dqvel| per env, the oracle's contact counts, MYO_F_DIAG, the status
    flags and the same_contacts mask; shares, tolerances and coverage are the caller's."""
    from myosuite_mjx_amd import capi
    for f, x in state.items():
        batch.write(f, x)
    if capi.F_ACTION in state:
        batch.step(batch.field_ptr(capi.F_ACTION)[0], capi.ACTMAP_MUSCLE_SIGMOID, nsub)
    else:
        batch.step(None, capi.ACTMAP_NONE, nsub)
    assert batch.last_kernel_name() == TRK
    gq, gv, ctrl, diag, flags = batch.read(capi.F_QPOS), batch.read(capi.F_QVEL), batch.read(capi.F_CTRL), batch.read(capi.F_DIAG), batch.status()
    q, v, act = state[capi.F_QPOS], state[capi.F_QVEL], state[capi.F_ACT]
    N = len(q)
    eq, ev, nc = np.zeros(N), np.zeros(N), np.zeros(N, int)
    for e in range(N):
        o = oracle_for_env(e)
        o.reset()
        o.set_state(qpos=q[e], qvel=v[e], act=act[e], ctrl=ctrl[e])
        assert o.step(nsub) == 0
        eq[e], ev[e], nc[e] = np.abs(gq[e] - o.field("qpos")).max(), np.abs(gv[e] - o.field("qvel")).max(), o.ncon
        if after_env is not None:
            after_env(e, o)
    return eq, ev, nc, diag, flags, same_contacts(flags, diag[:, 1], nc)


# ---- host side ------------------------------------------------------------------------------------------------------------------------

def muscle_variants(env_id, conditions):
    """The specs register_env_with_variants adds for env_id (envs/myo/myobase/__init__.py:14-48), one per (prefix, condition): each is
    the base spec with the muscle condition set, and supported; a prefix not listed has no entry."""
    from myosuite_mjx_amd import envs
    base, out = envs.REGISTRY[env_id], []
    assert env_id not in envs.UNSUPPORTED
    for c, cond in CONDITIONS:
        vid = env_id[:3] + c + env_id[3:]
        if (c, cond) not in conditions:
            assert vid not in envs.REGISTRY
            continue
        v = envs.REGISTRY[vid]
        assert v["muscle_condition"] == cond and {k: x for k, x in v.items() if k != "muscle_condition"} == base and vid not in envs.UNSUPPORTED
        out.append(v)
    return out


def assert_p2_refused(ids):
    """The MyoChallenge P2 ids draw size, mass and friction per env: not registered, listed with the reason, refused by make."""
    from myosuite_mjx_amd import envs
    for i in ids:
        assert i not in envs.REGISTRY and "size, mass and friction" in envs.UNSUPPORTED[i]
        with pytest.raises(NotImplementedError, match="size, mass and friction"):
            envs.make(i, num_envs=1)
