"""GPU tests (pytest -m gpu) of what a bad env leaves behind (include/myo_hip.h, "A bad env"), on every step kernel and task: the checks of
tests/bad_env.py, with the oracle's ABI twin as the expectation of the bare step (tests/test_bad_env_host.py runs the same sequence on it).
Shapes: 8 envs with envs 1 and 6 bad (lanes = 16: one in each of the two waves, so the wave-mates are the neighbours under test), 64 where
the substep scheduler is involved; one env step of the model's frame_skip and the two residue steps."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_backend as A  # noqa: E402
import bad_env as BE  # noqa: E402
import hand_task_checks as H  # noqa: E402
from myosuite_mjx_amd import capi, model as M  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = A.ROOT
DEAD = (1, 6)
HAND_RK4 = "step_kernel_w<24,8,32,1,3,false,0,false,false,true>"
HAND, HAND_GEN, LEG, LEG_SCHED, TERRAIN = ("step_kernel_w<24,8,32,1,4,false,1,false>", "step_kernel_w<24,8,32,1,3,false,0,false>",
                                           "step_kernel_w<36,20,32,2,2,false,2,false>", "step_kernel_w<36,20,32,2,2,true,2,false>",
                                           "step_kernel_w<36,20,32,2,2,false,3,true>")


def _hip():
    capi.lib()          # the library under test (MYO_HIP_LIB: the poisoned build), loaded after torch's HIP runtime (see capi.lib)
    return A.Backend(capi.LIB_PATH, 0)


@pytest.fixture(scope="module")
def hip():
    return _hip()


@contextlib.contextmanager
def _no_spec():
    old = os.environ.pop("MYO_NO_SPEC", None)
    os.environ["MYO_NO_SPEC"] = "1"        # read at model load: the run-time-sized instantiation
    try:
        yield
    finally:
        os.environ.pop("MYO_NO_SPEC", None)
        if old is not None:
            os.environ["MYO_NO_SPEC"] = old


@contextlib.contextmanager
def _lanes(n):
    capi.set_lanes(n)
    try:
        yield
    finally:
        capi.set_lanes(64)


def _object_state(m, B):
    """The TrackEnv-class model has no keyframe: qpos0 with small joint noise on the fingers, slow, muscles part activated."""
    rng = np.random.default_rng(15)
    st = BE.hand_state(m, B)
    q = np.tile(np.asarray(m.qpos0, np.float32), (B, 1))
    q[:, 6:29] += rng.normal(0, 0.02, (B, 23)).astype(np.float32)
    q[:, 31] = 0.1                                          # the object 10 cm above the table, where the default TrackEnv reference starts it
    st[capi.F_QPOS], st[capi.F_QVEL] = q, (0.2 * st[capi.F_QVEL]).astype(np.float32)
    for f in (capi.F_ACT, capi.F_CTRL):
        st[f][:, np.asarray(m.actuator_kind) != 0] = 0      # stateless actuators: activation stays zero, the base is held at zero
    return st


def _terrain_grids(b):
    from test_gpu_terrain import _grids
    b.write(capi.F_HFIELD, _grids(b.B, np.random.default_rng(0)).reshape(b.B, -1))


def _heavier_bodies(b):
    mass = b.read(capi.F_BODYMASS)            # (asking for the field starts the override)
    b.write(capi.F_BODYMASS, mass * np.linspace(1.0, 1.3, b.B, dtype=np.float32)[:, None])


# name: (asset, integrator, state, nsub, lanes, no_spec, per-batch preparation, kernel)
CASES = {
    "hand": ("myohand_pose", None, "hand", 10, 64, False, None, HAND),
    "hand_no_spec": ("myohand_pose", None, "hand", 10, 64, True, None, HAND_GEN),
    "hand_lanes16": ("myohand_pose", None, "hand", 10, 16, False, None, "step_kernel"),
    "hand_lanes32": ("myohand_pose", None, "hand", 10, 32, False, None, "step_kernel"),
    "hand_rk4": ("myohand_pose", "RK4", "hand", 10, 64, False, None, HAND_RK4),
    "hand_body_mass": ("myohand_pose", None, "hand", 10, 64, False, _heavier_bodies, HAND_GEN),
    "legs": ("myolegs", None, "key2", 10, 64, False, None, LEG),
    "terrain": ("myolegs_terrain", None, "key2", 10, 64, False, _terrain_grids, TERRAIN),
    "object": ("myohand_object_airplane", None, "object", 5, 64, False, None, H.TRK),
}


def _model_state(case, B):
    asset, integrator, state = CASES[case][:3]
    m = M.load_asset(asset)
    if integrator:
        m = m.with_integrator(integrator)
    st = {"hand": lambda: BE.hand_state(m, B), "key2": lambda: BE.key_state(m, B, 2), "object": lambda: _object_state(m, B)}[state]()
    return m, st


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", BE.KINDS)
def test_bare_step(hip, case, kind):
    """Every kernel class, every injection kind: the reset is exact with the flag the oracle twin raises for the kind (MYO_FLAG_BAD_QACC for
    nan_act and nan_ctrl), every field is finite, the neighbours are untouched bit for bit, and nothing of the bad env outlives the launch."""
    _, _, _, nsub, lanes, no_spec, prep, kernel = CASES[case]
    m, st = _model_state(case, 8)
    with contextlib.ExitStack() as stack:
        if no_spec:
            stack.enter_context(_no_spec())
        if lanes != 64:
            stack.enter_context(_lanes(lanes))
        rec = A.bad_env_scenario(hip, m, st, kind, nsub, DEAD, prep=prep)
    assert rec["kernel"] == kernel, rec["kernel"]
    assert (rec["flags"][list(DEAD)] == BE.FLAG_OF[kind]).all()
    assert np.abs(rec["after"][capi.F_QVEL][list(DEAD)]).max() > 0      # the residue steps moved the formerly bad envs


SCHED_CHILD = """
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import test_gpu_bad_env as T
np.savez({out!r}, **T.sched_rows())
"""
SCHED_DEAD = (1, 6, 40)


def sched_rows():
    """All injection kinds on 64 leg envs: {kind/field: rows after the launch, kind/after/field: rows after the residue steps}."""
    hip, out = _hip(), {}
    m = M.load_asset("myolegs")
    st = BE.key_state(m, 64, 2)
    for kind in BE.KINDS:
        rec = A.bad_env_scenario(hip, m, st, kind, 10, SCHED_DEAD)
        out[f"{kind}/kernel"] = np.array(rec["kernel"])
        for name in ("rows", "after"):
            for f, x in rec[name].items():
                out[f"{kind}/{name}/{BE.NAME[f]}"] = x
    return out


def test_scheduler_gives_the_same_bits(tmp_path):
    """The substep scheduler (one wave per (env, substep)) keeps the contract -- the child runs every check of test_bare_step under
    MYO_SCHED=1 -- and every field of every env, the bad ones included, is bit for bit what the one-wave-per-env launch writes: the waves
    of a bad env's remaining substeps do nothing (nan_ctrl: the env goes bad in substep 1 of 10)."""
    out = str(tmp_path / "sched.npz")
    r = subprocess.run([sys.executable, "-c", SCHED_CHILD.format(root=ROOT, out=out)], cwd=ROOT, env=dict(os.environ, MYO_SCHED="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    s, mine = np.load(out), sched_rows()
    assert set(s.files) == set(mine)
    for k in s.files:
        if k.endswith("/kernel"):
            assert str(s[k]) == LEG_SCHED and (os.environ.get("MYO_SCHED") or str(mine[k]) == LEG), (str(s[k]), str(mine[k]))
        else:
            assert s[k].tobytes() == mine[k].tobytes(), k


# ---- tasks -----------------------------------------------------------------------------------------------------------------------------

def _pair(env_id, B=8, **kw):
    import myosuite_mjx_amd as myo
    envs = [myo.make(env_id, num_envs=B, seed=3, as_torch=False, autoreset=False, **kw) for _ in range(2)]
    for e in envs:
        e.reset(seed=3)
    return envs


@pytest.mark.parametrize("env_id,kind,flag", [
    ("myoHandPoseRandom-v0", "nan_qvel", "kind"),
    ("myoHandPoseRandom-v0", "nan_act", "kind"),
    ("myoHandPoseRandom-v0", "nan_action", "kind"),
    ("myoFatiHandPoseRandom-v0", "nan_action", None),          # the fatigue clip drops the NaN (a stated deviation from np.clip, include/myo_hip.h)
    ("myoFatiHandPoseRandom-v0", "nan_qvel", "kind"),
    ("myoHandReachRandom-v0", "nan_act", "kind"),
    ("myoHandObjHoldRandom-v0", "huge_qvel", "kind"),
])
def test_separate_pass_tasks(env_id, kind, flag):
    env, clean = _pair(env_id)
    BE.task_contained(env, clean, kind, 5, flag=flag)


@pytest.mark.parametrize("env_id,kind,kw", [("myoLegWalk-v0", "nan_qvel", {}), ("myoLegWalk-v0", "nan_action", dict(sensors=True)),
                                             ("myoLegStandRandom-v0", "nan_act", {}), ("myoLegRoughTerrainWalk-v0", "nan_qvel", {})])
def test_walk_and_stand_fused_pass(env_id, kind, kw):
    """The observation pass inside the step launch runs on the reset state of a bad env.  Walk: its reward is also that of oracle/walk_ref.py
    at the reset state, within the tolerance tests/test_gpu_walk.py has for a live env (5e-3)."""
    env, clean = _pair(env_id, **kw)
    rows, _ = BE.task_contained(env, clean, kind, 5, fused_obs=True)
    if env_id == "myoLegWalk-v0":
        from oracle.oracle import Oracle
        from oracle.walk_ref import walk_obs_reward
        m = env.mjmodel
        o = Oracle(m.blob())
        o.reset(); o.switches(0, 0, 0)
        o.set_state(qpos=m.qpos0, qvel=np.zeros(m.nv), act=np.zeros(m.nu), ctrl=np.zeros(m.nu), warm=np.zeros(m.nv), time=0)
        _, dense, _, _, _ = walk_obs_reward(m, o, 0, env.dt, np.asarray(m.key_qpos).reshape(-1, m.nq)[0][3:7])
        print("walk reward of the bad env", float(rows[capi.F_REWARD][5, 0]), "walk_ref at the reset state", float(dense))
        assert abs(rows[capi.F_REWARD][5, 0] - dense) < 5e-3
    if kw.get("sensors"):
        assert capi.F_SENSORDATA in rows and capi.F_CFRC in rows


def test_reward_terms_and_episode_statistics():
    """The reward-term row of a bad env is finite and its weighted sum is MYO_F_REWARD; the episode buffers stay finite."""
    env, clean = _pair("myoHandPoseRandom-v0", rwd_dict=True, episode_stats=True)
    rows, _ = BE.task_contained(env, clean, "nan_action", 5)
    terms, w = env.batch.read_rwd(), env.rwd_weights
    assert np.isfinite(terms).all()
    s = sum(np.float64(w[k]) * terms[:, i] for i, k in enumerate(env.rwd_keys) if k in w)
    assert np.allclose(s, rows[capi.F_REWARD][:, 0], rtol=1e-5, atol=1e-5)
    assert np.array_equal(terms[:, env.rwd_keys.index("dense")], rows[capi.F_REWARD][:, 0])
    for which in (capi.EP_RUNNING, capi.EP_LAST, capi.EP_FINISHED, capi.EP_COUNT):
        assert np.isfinite(env.batch.read_episode(which).astype(np.float64)).all()


def _motion():
    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_motion.npz"))
    return {k.split("__in__")[1]: f[k] for k in f.files if k.startswith("track_MyoHand_airplane_fly1__in__")}


@pytest.mark.parametrize("kind", ["nan_qvel", "nan_action"])
@pytest.mark.parametrize("autoreset", [False, True])
def test_fused_trackenv_step_ends_the_episode_of_a_bad_env(autoreset, kind):
    """MYO_TASK_TRACK with MYO_ACTMAP_CTRLRANGE: a bad env is an ended episode with or without `autoreset` -- done, no reward, no metrics,
    TrackEnv.reset's state, step counter and time zero, observation [init_qpos, 0], the flag -- and then steps like an env that was reset."""
    from myosuite_mjx_amd import track as T
    B, D = 8, (5,)
    envs = [T.TrackEnv(num_envs=B, reference=_motion(), seed=0, autoreset=autoreset) for _ in range(3)]
    for e in envs:
        e.reset()
        for _ in range(2):                                     # two clean steps first: the step counter of a live env is not zero
            _track_step(e.batch, 0)
    env, clean, fresh = envs
    b, m = env.batch, env.mjmodel
    a = _track_action(B, m.nu, 1)
    if kind == "nan_action":
        b.write(capi.F_ACTION, BE.inject(kind, {capi.F_ACTION: a}, D)[capi.F_ACTION])
    else:
        b.write(capi.F_ACTION, a)
        b.write(capi.F_QVEL, BE.inject(kind, {capi.F_QVEL: b.read(capi.F_QVEL)}, D)[capi.F_QVEL])
    b.step(b.field_ptr(capi.F_ACTION)[0], capi.ACTMAP_CTRLRANGE, env.n_frames)
    _track_step(clean.batch, 1)
    assert b.last_kernel_name() == H.TRK
    rows, rows_clean, flags = BE.read_all(BE.HipRows(b, None)), BE.read_all(BE.HipRows(clean.batch, None)), env.status()
    BE.assert_all_fields_finite(rows)
    BE.assert_neighbours_bitwise(rows, rows_clean, D)
    BE.assert_reset_exact(rows, flags, D, env.init_qpos, BE.FLAG_OF[kind])
    e = D[0]
    assert rows[capi.F_DONE][e, 0] == 1 and rows[capi.F_REWARD][e, 0] == 0 and rows[capi.F_SOLVED][e, 0] == 0 and not rows[capi.F_METRICS][e].any()
    assert rows[capi.F_ELAPSED][e, 0] == 0
    assert np.array_equal(rows[capi.F_OBS][e, :m.nq], np.asarray(env.init_qpos, np.float32)) and not rows[capi.F_OBS][e, m.nq:].any()
    BE.assert_no_residue(BE.HipRows(b, lambda bb, n: _track_step(bb, 2)), BE.HipRows(fresh.batch, lambda bb, n: _track_step(bb, 2)), rows, D, env.init_qpos,
                         env.n_frames, fields=BE.STATE + (capi.F_QACC, capi.F_OBS, capi.F_REWARD, capi.F_DONE, capi.F_METRICS, capi.F_ELAPSED))


def _track_action(B, nu, seed):
    return np.random.default_rng(seed).uniform(-0.3, 0.3, (B, nu)).astype(np.float32)


def _track_step(b, seed):
    from myosuite_mjx_amd import capi
    b.write(capi.F_ACTION, _track_action(b.B, b.model.dims.nu, seed))
    b.step(b.field_ptr(capi.F_ACTION)[0], capi.ACTMAP_CTRLRANGE, 5)


def test_classic_trackenv():
    from myosuite_mjx_amd import track as T
    envs = [T.ClassicTrackEnv(num_envs=8, reference=_motion(), seed=0, autoreset=False) for _ in range(2)]
    for e in envs:
        e.reset()
    BE.task_contained(envs[0], envs[1], "nan_qvel", 5)


def test_env_layer_returns_finite_rows_and_reports_the_env():
    """myo.make(...).step with a NaN action for env 5 at step 2 of six: every observation and reward the caller sees is finite, and
    env.status() names env 5."""
    import myosuite_mjx_amd as myo
    import torch
    env = myo.make("myoElbowPose1D6MFixed-v0", num_envs=64, seed=1)
    env.reset()
    g = torch.Generator().manual_seed(0)
    for t in range(6):
        a = torch.rand((64, env.act_dim), generator=g) * 2 - 1
        if t == 2:
            a[5, 1] = float("nan")
        obs, rew, done, trunc, info = env.step(a)
        assert torch.isfinite(obs).all() and torch.isfinite(rew).all(), t
    fl = env.status()
    assert fl[5] & (capi.FLAG_BAD_STATE | capi.FLAG_BAD_QACC) and not np.delete(fl, 5).any()


class _NanActionAt:
    """An env whose step number `at` gets a NaN in env `e`'s action; everything else is the env's own."""

    def __init__(self, env, at, e):
        self._env, self._at, self._e, self.calls = env, at, e, 0

    def __getattr__(self, name):
        return getattr(self._env, name)

    def step(self, action):
        if self.calls == self._at:
            action = action.clone()
            action[self._e, 1] = float("nan")
        self.calls += 1
        return self._env.step(action)


def test_ppo_iteration_survives_a_bad_env():
    """One iteration of ppo.train (unroll of 8 steps, GAE, advantage normalisation, 2 x 4 Adam steps) on 64 envs, with a NaN in env 5's action
    at step 2 of the unroll: the rollout buffers and every parameter after the update are finite, and env.status() names env 5."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import ppo
    env = _NanActionAt(myo.make("myoElbowPose1D6MFixed-v0", num_envs=64, seed=1), 2, 5)
    pol, params, metrics = ppo.train(env, 64 * 8, unroll_length=8, num_minibatches=4, num_updates_per_batch=2, seed=5, keep_first_rollout=True)
    assert env.calls == 8 and len(metrics) == 1
    fl = env.status()
    assert fl[5] & (capi.FLAG_BAD_STATE | capi.FLAG_BAD_QACC) and not np.delete(fl, 5).any()
    roll = metrics[0]["first_rollout"]
    assert roll["obs"].shape[:2] == (9, 64)
    for k, x in roll.items():
        assert np.isfinite(x).all(), k
    for k, p in params.items():
        assert np.isfinite(p).all(), k
    assert all(np.isfinite(metrics[0][k]) for k in ("policy_loss", "value_loss", "entropy_loss"))


WALK_CHILD = """
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import test_gpu_bad_env as T
np.savez({out!r}, **T.walk_rows())
"""


def walk_rows():
    """myoLegWalk-v0 with touch sensors, 64 envs, two env steps; in the first, env 1 starts with a NaN velocity, env 6 with a NaN
    activation and env 40 gets a NaN action (bad in substep 1).  {step/field: rows}, the kernel's name and the flags."""
    import myosuite_mjx_amd as myo
    env = myo.make("myoLegWalk-v0", num_envs=64, seed=3, as_torch=False, autoreset=False, sensors=True)
    env.reset(seed=3)
    b, rng, out = env.batch, np.random.default_rng(2), {}
    for f, kind, e in ((capi.F_QVEL, "nan_qvel", 1), (capi.F_ACT, "nan_act", 6)):
        b.write(f, BE.inject(kind, {f: b.read(f)}, (e,))[f])
    for t in range(2):
        a = rng.uniform(-1, 1, (64, env.act_dim)).astype(np.float32)
        if t == 0:
            a = BE.inject("nan_action", {capi.F_ACTION: a}, (40,))[capi.F_ACTION]
        env.step(a)
        rows = BE.read_all(BE.HipRows(b, None))
        BE.assert_all_fields_finite(rows)
        for f, x in rows.items():
            out[f"{t}/{BE.NAME[f]}"] = x
        out[f"{t}/flags"] = env.status()
    out["kernel"] = np.array(b.last_kernel_name())
    return out


def test_scheduled_walk_with_sensors_gives_the_same_bits(tmp_path):
    """The default myoLegWalk configuration -- substep scheduler, fused observation pass as a task of its own, touch sensors -- with three
    bad envs: every field of every env after each of two env steps is bit for bit what the one-wave-per-env launch writes.  The bad envs
    carry their flags, sit at qpos0 with zero sensors, and their observation rows are finite (walk_rows asserts it on both sides)."""
    out = str(tmp_path / "walk.npz")
    r = subprocess.run([sys.executable, "-c", WALK_CHILD.format(root=ROOT, out=out)], cwd=ROOT, env=dict(os.environ, MYO_SCHED="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    s, mine = np.load(out), walk_rows()
    assert str(s["kernel"]) == LEG_SCHED and (os.environ.get("MYO_SCHED") or str(mine["kernel"]) == LEG), (str(s["kernel"]), str(mine["kernel"]))
    assert set(s.files) == set(mine)
    for k in s.files:
        if k != "kernel":
            assert s[k].tobytes() == mine[k].tobytes(), k
    fl, m = mine["0/flags"], M.load_asset("myolegs")
    assert fl[1] == capi.FLAG_BAD_STATE and fl[6] == capi.FLAG_BAD_QACC and fl[40] == capi.FLAG_BAD_QACC and not np.delete(fl, [1, 6, 40]).any()
    assert not mine["1/flags"].any()
    for e in (1, 6, 40):
        assert np.array_equal(mine["0/F_QPOS"][e], np.asarray(m.qpos0, np.float32)) and not mine["0/F_SENSORDATA"][e].any() and not mine["0/F_CFRC"][e].any()


def test_guard_the_file_passes_on_the_poisoned_build():
    """A bad env must not read LDS it never wrote: the whole file again on the build whose LDS starts as NaN."""
    H.rerun_file_against_poison_build(__file__, 600)
