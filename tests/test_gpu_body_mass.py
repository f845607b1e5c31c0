"""GPU tests (pytest -m gpu) for per-env body masses (MYO_F_BODYMASS / MYO_F_BODYMASS_RANGE; PoseEnvV0 weight_bodyname / weight_range,
envs/myo/myobase/pose_v0.py:163-176).

  * HIP vs HIP: a batch with per-env masses equals, env by env, batches of models edited with Model.with_body_mass (no override, same
    run-time-sizes kernel, same start state and actions) after 20 env steps.  The per-env link tables are recomposed from float32 masses in
    float64 and rounded once, as the edited blob's are, so the two agree to float32 round-off (about 1e-5 after 200 substeps).
  * HIP vs the float64 oracle loaded from the edited blob: the oracle composes its inertias per BODY, not per merged link.
  * the mass reaches the dynamics; reset draws; override on with unchanged masses is the override-off trajectory; refusals; the same file
    against the NaN-poisoned build; register / scratch figures of the two instantiations that read the per-env tables."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND_RT = "step_kernel_w<24,8,32,1,3,false,0,false>"          # run-time-sizes hand / finger class
BIG_RT = "step_kernel_w<36,20,32,2,2,false,0,false>"          # run-time-sizes 36-dof class
HAND_BODIES = ("lunate", "proxph2", "distph3")                  # lunate is welded into a link of several bodies


def _load(blob, no_spec=False):
    from myosuite_mjx_amd import capi
    old = os.environ.pop("MYO_NO_SPEC", None)
    if no_spec:
        os.environ["MYO_NO_SPEC"] = "1"                         # read at model load: force the run-time-sizes instantiation
    try:
        return capi.HipModel(blob, 0)
    finally:
        os.environ.pop("MYO_NO_SPEC", None)
        if old is not None:
            os.environ["MYO_NO_SPEC"] = old


def _rollout(hm, state, actions, nsub=10, masses=None, start=False):
    """Env steps of ACTMAP_MUSCLE_SIGMOID actions[t] from `state`; masses: [B, nbody] written through MYO_F_BODYMASS."""
    from myosuite_mjx_amd import capi
    q, v, a = state
    b = capi.HipBatch(hm, q.shape[0])
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, a)):
        b.write(f, x)
    if masses is not None:
        b.write(capi.F_BODYMASS, masses)
    elif start:
        b.field_ptr(capi.F_BODYMASS)                              # starts the override with the model's masses
    aptr = b.field_ptr(capi.F_ACTION)[0]
    for act in actions:
        b.write(capi.F_ACTION, act)
        b.step(aptr, capi.ACTMAP_MUSCLE_SIGMOID, nsub)
    out = b.read(capi.F_QPOS), b.read(capi.F_QVEL), b.read(capi.F_ACT)
    return out, b.last_kernel_name(), b.status()


def _hand_state(m, N, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    lo, hi = m.jnt_range[:, 0], m.jnt_range[:, 1]
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    f32 = np.float32
    return ((mid + spread * half * rng.uniform(-1, 1, (N, m.nq))).astype(f32), rng.normal(0, 0.2, (N, m.nv)).astype(f32),
            rng.uniform(0, 0.5, (N, m.nu)).astype(f32))


def _hold_state(m, N, seed):
    rng = np.random.default_rng(seed)
    q = np.tile(m.qpos0, (N, 1))
    q[:, :23] = 0
    q[:, 0] = -1.5                                                # palm up (obj_hold_v0.py:63-64)
    q[:, :23] += rng.normal(0, 0.1, (N, 23))
    q[:, :23] = np.clip(q[:, :23], m.jnt_range[:23, 0] + 0.01, m.jnt_range[:23, 1] - 0.01)
    return q.astype(np.float32), np.zeros((N, m.nv), np.float32), rng.uniform(0, 0.5, (N, m.nu)).astype(np.float32)


def _edited(m, bodies, w):
    e = m
    for b, x in zip(bodies, w):
        e = e.with_body_mass(b, float(x))
    return e


def _hip_vs_hip(m, bodies, masses32, state, actions, want_kernel, tol=1e-5):
    """masses32: [B, len(bodies)] float32; every env against a one-env batch of the model edited with the same (float32) masses."""
    B = masses32.shape[0]
    ids = [m.body_name2id(b) for b in bodies]
    full = np.tile(np.asarray(m.body_mass, np.float32), (B, 1))
    full[:, ids] = masses32
    g, kname, fl = _rollout(_load(m.blob()), state, actions, masses=full)
    assert kname == want_kernel and (fl == 0).all()
    worst = 0.0
    for e in range(B):
        hm = _load(_edited(m, bodies, masses32[e].astype(np.float64)).blob(), no_spec=True)
        r, rk, rfl = _rollout(hm, tuple(x[e:e + 1] for x in state), [a[e:e + 1] for a in actions])
        assert rk == want_kernel and (rfl == 0).all()
        worst = max(worst, *(float(np.abs(g[k][e] - r[k][0]).max()) for k in range(3)))
    assert worst < tol, worst
    return g


def test_hip_vs_hip_elbow_exo_through_env_body_mass(exo):
    """myoElbowPose1D6MExoFixed-v0: per-env carry_weight masses spanning [0.1, 2] written through the torch view env.body_mass."""
    import torch
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B, T = 16, 20
    env = myo.make("myoElbowPose1D6MExoFixed-v0", num_envs=B, seed=0, autoreset=False)
    bid = exo.body_name2id("carry_weight")
    w = np.linspace(0.1, 2.0, B).astype(np.float32)
    bm = env.body_mass
    assert tuple(bm.shape) == (B, exo.nbody) and torch.allclose(bm[0].cpu(), torch.tensor(exo.body_mass, dtype=torch.float32))
    bm[:, bid] = torch.from_numpy(w).to(bm.device)
    rng = np.random.default_rng(1)
    q = rng.uniform(0.2, 2.0, (B, 1)).astype(np.float32)
    st = (q, np.zeros((B, 1), np.float32), np.zeros((B, exo.nu), np.float32))
    env.set_env_state(dict(qpos=st[0], qvel=st[1], act=st[2]))
    actions = [rng.uniform(-1, 1, (B, exo.nu)).astype(np.float32) for _ in range(T)]
    for a in actions:
        env.step(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    assert env.batch.last_kernel_name() == HAND_RT and (env.status() == 0).all()
    gs = env.get_env_state()
    for e in range(B):
        hm = _load(exo.with_body_mass(bid, float(w[e])).blob())
        r, rk, _ = _rollout(hm, tuple(x[e:e + 1] for x in st), [a[e:e + 1] for a in actions])
        assert rk == HAND_RT
        for k, key in enumerate(("qpos", "qvel", "act")):
            assert np.abs(gs[key][e] - r[k][0]).max() < 1e-5, (e, key, np.abs(gs[key][e] - r[k][0]).max())
    # the masses drive the trajectories apart: the heaviest and lightest weight end in different poses
    assert abs(float(gs["qpos"][0, 0] - gs["qpos"][-1, 0])) > 1e-3


def test_hip_vs_hip_hand_pose(hand):
    """MyoHand (the size-specialised headline model) with three bodies re-weighted per env: routed to the run-time-sizes hand kernel."""
    B, T = 12, 20
    rng = np.random.default_rng(2)
    base = np.asarray([hand.body_mass[hand.body_name2id(b)] for b in HAND_BODIES])
    w = (base[None, :] * rng.uniform(0.5, 2.0, (B, 3))).astype(np.float32)
    st = _hand_state(hand, B, 3)
    actions = [rng.uniform(-1, 1, (B, hand.nu)).astype(np.float32) for _ in range(T)]
    _hip_vs_hip(hand, HAND_BODIES, w, st, actions, HAND_RT)


def test_hip_vs_hip_hold(hand):
    """myohand_hold (36-dof class: the free object's root link and the hand): the object's mass and a phalanx mass per env."""
    from myosuite_mjx_amd import model as M
    m = M.load_asset("myohand_hold")
    B, T = 8, 20
    rng = np.random.default_rng(4)
    bodies = ("object", "proxph2")
    base = np.asarray([m.body_mass[m.body_name2id(b)] for b in bodies])
    w = (base[None, :] * rng.uniform(0.5, 2.0, (B, 2))).astype(np.float32)
    actions = [rng.uniform(-1, 1, (B, m.nu)).astype(np.float32) for _ in range(T)]
    _hip_vs_hip(m, bodies, w, _hold_state(m, B, 5), actions, BIG_RT)


def _oracle_pair(m, bodies, w32, q, v, act, ctrl, nsub=10):
    """One env step (ACTMAP_NONE, ctrl given) with per-env masses on the GPU, and the float64 oracle loaded from each env's edited blob."""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    B = q.shape[0]
    ids = [m.body_name2id(b) for b in bodies]
    full = np.tile(np.asarray(m.body_mass, np.float32), (B, 1))
    full[:, ids] = w32
    b = capi.HipBatch(_load(m.blob()), B)
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, v), (capi.F_ACT, act), (capi.F_CTRL, ctrl), (capi.F_BODYMASS, full)):
        b.write(f, x)
    b.step(None, capi.ACTMAP_NONE, nsub)
    gq, gv, dg, fl = b.read(capi.F_QPOS), b.read(capi.F_QVEL), b.read(capi.F_DIAG), b.status()
    eq, ev, same = np.zeros(B), np.zeros(B), np.zeros(B, bool)
    for e in range(B):
        o = Oracle(_edited(m, bodies, w32[e].astype(np.float64)).blob())
        o.reset()
        o.set_state(qpos=q[e], qvel=v[e], act=act[e], ctrl=ctrl[e])
        assert o.step(nsub) == 0
        eq[e], ev[e] = np.abs(gq[e] - o.field("qpos")).max(), np.abs(gv[e] - o.field("qvel")).max()
        same[e] = fl[e] == 0 and dg[e, 1] == o.ncon
    return eq, ev, same


def test_hip_vs_oracle_elbow_exo(exo):
    # tolerances of test_gpu_parity.py::test_stateless_actuator_parity for this model at 10 substeps: qpos 1e-4, qvel 2e-2
    rng = np.random.default_rng(6)
    B = 8
    w = np.linspace(0.1, 2.0, B).astype(np.float32)[:, None]
    q = rng.uniform(0.1, 2.1, (B, 1)).astype(np.float32)
    v = rng.normal(0, 1.0, (B, 1)).astype(np.float32)
    act = np.concatenate([np.zeros((B, 1)), rng.uniform(0, 1, (B, 6))], 1).astype(np.float32)
    ctrl = np.concatenate([rng.uniform(-1, 1, (B, 1)), rng.uniform(0, 1, (B, 6))], 1).astype(np.float32)
    eq, ev, same = _oracle_pair(exo, ("carry_weight",), w, q, v, act, ctrl)
    assert same.all() and eq.max() < 1e-4 and ev.max() < 2e-2, (eq.max(), ev.max())


def test_hip_vs_oracle_hand(hand):
    # tolerances of test_gpu_parity.py (module docstring, one env step with contacts): qpos 1e-4, qvel 2e-2
    rng = np.random.default_rng(7)
    B = 8
    base = np.asarray([hand.body_mass[hand.body_name2id(b)] for b in HAND_BODIES])
    w = (base[None, :] * rng.uniform(0.5, 2.0, (B, 3))).astype(np.float32)
    q, v, act = _hand_state(hand, B, 8, spread=0.6)
    ctrl = rng.uniform(0, 1, (B, hand.nu)).astype(np.float32)
    eq, ev, same = _oracle_pair(hand, HAND_BODIES, w, q, v, act, ctrl)
    assert same.sum() >= B - 1 and eq[same].max() < 1e-4 and ev[same].max() < 2e-2, (eq.max(), ev.max())


def test_hip_vs_oracle_hold():
    # tolerances of test_gpu_hold.py::test_hand_object_parity at 10 substeps: qpos 2e-3, qvel 0.2 (states with equal contact counts)
    from myosuite_mjx_amd import model as M
    m = M.load_asset("myohand_hold")
    rng = np.random.default_rng(9)
    B = 8
    bodies = ("object", "proxph2")
    base = np.asarray([m.body_mass[m.body_name2id(b)] for b in bodies])
    w = (base[None, :] * rng.uniform(0.5, 2.0, (B, 2))).astype(np.float32)
    q, v, act = _hold_state(m, B, 10)
    ctrl = rng.uniform(0, 1, (B, m.nu)).astype(np.float32)
    eq, ev, same = _oracle_pair(m, bodies, w, q, v, act, ctrl)
    assert same.sum() >= B - 1 and eq[same].max() < 2e-3 and ev[same].max() < 0.2, (eq.max(), ev.max())


def test_mass_reaches_the_dynamics(exo):
    """Same state, zero control: the 2.0 kg and the 0.1 kg env differ in elbow qacc in the direction of the weight's gravity torque."""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    bid = exo.body_name2id("carry_weight")
    q = np.array([[0.3], [0.3]], np.float32)
    z1, zu = np.zeros((2, 1), np.float32), np.zeros((2, exo.nu), np.float32)
    masses = np.tile(np.asarray(exo.body_mass, np.float32), (2, 1))
    masses[:, bid] = (2.0, 0.1)
    b = capi.HipBatch(_load(exo.blob()), 2)
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, z1), (capi.F_ACT, zu), (capi.F_CTRL, zu)):
        b.write(f, x)
    env = capi.HipBatch(_load(exo.blob()), 2)      # the same state without the override
    for f, x in ((capi.F_QPOS, q), (capi.F_QVEL, z1), (capi.F_ACT, zu), (capi.F_CTRL, zu)):
        env.write(f, x)
    b.write(capi.F_BODYMASS, masses)
    b.step(None, capi.ACTMAP_NONE, 1)
    env.step(None, capi.ACTMAP_NONE, 1)
    qacc = b.read(capi.F_QACC)[:, 0]
    # gravity torque of the weight about the elbow axis at this pose, from the oracle's kinematics
    o = Oracle(exo.blob())
    o.reset()
    o.set_state(qpos=q[0].astype(float), qvel=np.zeros(1), act=np.zeros(exo.nu), ctrl=np.zeros(exo.nu))
    o.forward()
    g = np.asarray(exo.arrays["opt"][1:4], float)
    tau = float(np.dot(np.cross(o.field("xipos")[3 * bid:3 * bid + 3] - o.field("xanchor")[:3], g), o.field("xaxis")[:3]))
    assert abs(tau) > 0.1
    assert np.sign(qacc[0] - qacc[1]) == np.sign(tau) and abs(qacc[0] - qacc[1]) > 1.0, (qacc, tau)
    # and the size of the difference is the oracle's for the two edited models
    ref = []
    for w in (2.0, 0.1):
        o = Oracle(exo.with_body_mass(bid, w).blob())
        o.reset()
        o.set_state(qpos=q[0].astype(float), qvel=np.zeros(1), act=np.zeros(exo.nu), ctrl=np.zeros(exo.nu))
        o.step(1)
        ref.append(o.field("qacc")[0])
    assert abs((qacc[0] - qacc[1]) - (ref[0] - ref[1])) < 1e-2 * abs(ref[0] - ref[1]), (qacc, ref)
    # the batch without the override keeps the model's mass (0.1 kg) in both envs
    assert abs(env.read(capi.F_QACC)[0, 0] - qacc[1]) < 1e-3 * max(1.0, abs(qacc[1]))


EXO_RANDOM = dict(weight_bodyname="carry_weight", weight_range=(0.1, 2.0), target_jnt_range={"r_elbow_flex": (0, 2.27)})


def test_reset_draws(exo):
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B = 4096
    bid = exo.body_name2id("carry_weight")
    env = myo.make("myoElbowPose1D6MExoFixed-v0", num_envs=B, seed=11, as_torch=False, **EXO_RANDOM)
    assert np.allclose(env.batch.read(capi.F_BODYMASS)[:, bid], exo.body_mass[bid])     # before the first reset: the model's mass
    env.reset()
    w = env.body_mass[:, bid]
    others = np.delete(env.body_mass, bid, axis=1)
    assert np.allclose(others, np.delete(np.asarray(exo.body_mass, np.float32), bid)[None, :])
    assert w.min() >= 0.1 and w.max() <= 2.0
    assert abs(w.mean() - 1.05) < 0.02 and abs(w.std() - 0.548) < 0.02, (w.mean(), w.std())
    t = env.batch.read(capi.F_TARGET)[:, 0]
    assert t.min() >= 0 and t.max() <= 2.27 + 1e-6 and t.std() > 0.5
    # autoreset redraws only the envs it resets
    el = np.zeros((B, 1), np.int32)
    el[::3] = env.max_episode_steps
    env.batch.write(capi.F_ELAPSED, el)
    env.batch.autoreset(env.max_episode_steps, 99)
    w2 = env.body_mass[:, bid]
    reset = np.zeros(B, bool)
    reset[::3] = True
    assert (w2[~reset] == w[~reset]).all() and (w2[reset] != w[reset]).mean() > 0.99
    assert w2.min() >= 0.1 and w2.max() <= 2.0
    # the same seed gives the same masses
    env2 = myo.make("myoElbowPose1D6MExoFixed-v0", num_envs=B, seed=11, as_torch=False, **EXO_RANDOM)
    env2.reset()
    assert np.array_equal(env2.body_mass[:, bid], w)
    # two shards (env_offset 0 and 2048) reproduce the single batch
    parts = []
    for off in (0, B // 2):
        s = myo.make("myoElbowPose1D6MExoFixed-v0", num_envs=B // 2, seed=11, env_offset=off, as_torch=False, **EXO_RANDOM)
        s.reset()
        parts.append(s.body_mass[:, bid])
    assert np.array_equal(np.concatenate(parts), w)


def test_exo_random_configuration_steps(exo):
    """The reference's ExoRandom configuration through myo.make: masses re-drawn at every episode while it runs."""
    import torch
    import myosuite_mjx_amd as myo
    B = 256
    bid = exo.body_name2id("carry_weight")
    env = myo.make("myoElbowPose1D6MExoFixed-v0", num_envs=B, seed=3, **EXO_RANDOM)
    env.reset()
    w0 = env.body_mass[:, bid].clone()
    for _ in range(env.max_episode_steps):
        obs, rwd, done, trunc, info = env.step(torch.rand((B, env.act_dim), device="cuda") * 2 - 1)
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and (env.status() == 0).all()
    assert (env.body_mass[:, bid] != w0).float().mean() > 0.99           # every env went through at least one reset
    assert env.batch.last_kernel_name() == HAND_RT


@pytest.mark.parametrize("which", ["exo", "hand"])
def test_override_with_unchanged_masses_is_off(which, request):
    m = request.getfixturevalue(which)
    B, T = 16, 20
    rng = np.random.default_rng(12)
    st = _hand_state(m, B, 13) if which == "hand" else (rng.uniform(0.2, 2.0, (B, 1)).astype(np.float32), np.zeros((B, 1), np.float32),
                                                        np.zeros((B, m.nu), np.float32))
    actions = [rng.uniform(-1, 1, (B, m.nu)).astype(np.float32) for _ in range(T)]
    hm = _load(m.blob(), no_spec=True)
    off, k0, _ = _rollout(hm, st, actions)
    on, k1, fl = _rollout(hm, st, actions, start=True)
    assert k0 == k1 == HAND_RT and (fl == 0).all()
    for a, b in zip(off, on):
        assert np.abs(a - b).max() < 1e-5, np.abs(a - b).max()


def test_refusals(hand, exo):
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi, model as M

    def refused(batch, code=-4):
        with pytest.raises(capi.MyoError, match=f"error {code}"):
            batch.field_ptr(capi.F_BODYMASS)
    refused(capi.HipBatch(_load(hand.with_integrator("RK4").blob()), 2))
    refused(capi.HipBatch(_load(M.load_asset("myohand_object_airplane").blob()), 2))
    refused(capi.HipBatch(_load(M.load_asset("myolegs_terrain").blob()), 2))
    walk = myo.make("myoLegWalk-v0", num_envs=2, as_torch=False)
    refused(walk.batch)
    stand = myo.make("myoLegStandRandom-v0", num_envs=2, as_torch=False)
    refused(stand.batch)
    # bad host values: MYO_E_ARG, and the override is not started by them
    b = capi.HipBatch(_load(exo.blob()), 2)
    nb = exo.nbody
    m0 = np.tile(np.asarray(exo.body_mass, np.float32), (2, 1))
    bad = m0.copy()
    bad[1, 5] = -0.5
    with pytest.raises(capi.MyoError, match="error -1"):
        b.write(capi.F_BODYMASS, bad)
    for lo, hi in ((-0.1, 1.0), (1.0, 0.5)):
        r = np.zeros((2, 2 * nb), np.float32)
        r[:, 5], r[:, nb + 5] = lo, hi
        with pytest.raises(capi.MyoError, match="error -1"):
            b.write(capi.F_BODYMASS_RANGE, r)
    assert np.array_equal(b.read(capi.F_BODYMASS), m0) and not b.read(capi.F_BODYMASS_RANGE).any()
    # the env kwargs stay pose-only
    with pytest.raises(TypeError):
        myo.make("myoLegWalk-v0", num_envs=2, weight_bodyname="pelvis")


def test_guard_poisoned_build():
    """This file once more against libmyo_hip_poison.so (NaN-filled LDS, scratch and registers before every step launch)."""
    lib = os.path.join(ROOT, "myosuite_mjx_amd", "libmyo_hip_poison.so")
    assert os.path.exists(lib), "libmyo_hip_poison.so is missing: run __graft_entry__.build()"
    env = dict(os.environ, MYO_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not guard",
                        "tests/test_gpu_body_mass.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout


def test_guard_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    res = {r["name"]: r for r in kr.resources()}
    for tmpl, vmax in (("ILi24ELi8ELi32ELi1ELi3ELb0ELi0ELb0ELb0ELb0E", 128), ("ILi36ELi20ELi32ELi2ELi2ELb0ELi0ELb0ELb0ELb0E", 256)):
        r = res["_Z13step_kernel_w" + tmpl + "EvPK8DevModelPK9DevModelW8DevBatchPKfiiPxPKiPK7DevWalki8SchedDev"]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= vmax, r
