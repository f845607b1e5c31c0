"""GPU tests (pytest -m gpu) of the forward pass (include/myo_hip_forward.h): body, site and geom frames and the contact list at the batch's
state, without a step.  The yardstick is the float64 oracle's own forward pass at the same qpos (tests/forward_ref.py).

  1. Frames of eight assets (hand, 36-dof, plane, height-field and TrackEnv classes; hull geoms) within 5e-6, the bound MYO_F_SITEXPOS is
     held to in tests/test_gpu_baoding.py; B = 1 and B = 3 too.
  2. Contacts: per env the multiset of (geom1, geom2) equals the oracle's in at least 90 % of the envs of every state family (float32
     oracle against float64, measured on the CPU: 32 of 32 in every family used here, myolegs, myolegs_terrain and the airplane included);
     dist, pos and normal of the agreeing envs within 4 x the float32 oracle's own largest deviation over the same states (floors 5e-6 /
     5e-6 / 1e-5); frames orthonormal, right-handed, normal first.  The crowded family of the die asset has states with more than
     NC = 32 contacts (up to 63: overflow rows are exported; tests/die_states.py's episodes stop at 20), the grasp family of the cup
     asset (tests/test_gpu_track.py's frames) more than 64, up to 75: the TRK class's second bank.  The tangents of every contact frame
     are compared with a numpy restatement of the row stage's rule.
  3. Exact: ncon equals MYO_F_DIAG[:, 1] of a 1-substep step from the same state in every env; a 20-step rollout with forward() between
     the steps is bitwise the rollout without; forward alone changes no state field.
  5. Per-env overrides: MYO_F_BODYQUAT and the goal offset (die), MYO_F_BODYPOS (key turn), MYO_F_GEOMSIZE (hold), their contacts by
     check 2's convention (90 % of the envs, 4 x the float32 oracle's deviation on the same edited models); MYO_F_HFIELD is the
     terrain family of 1. and 2., a different grid per env.
  6. A bad env, and this file once more against the NaN-poisoned build.
  7. The surfaces: HipSimScene(kinematics=True) in both modes, sim.forward / get, env.forward(), refusals.

site_xmat is exported for blobs that carry site_quat (the two leg assets); for the others MYO_FWD_SITE_XMAT is refused.  The refusal for a
model on the generic lanes kernel is tested with lanes = 32, which puts the hand model there."""
import numpy as np
import pytest

import forward_ref as FR
import hand_task_checks as H

pytestmark = pytest.mark.gpu
POS_TOL = ROT_TOL = 5e-6
_CACHE = {}


def _asset(stem):
    """Per asset, once per module: model, state families with the float64 reference and the float32-derived bounds, and what one forward
    launch (then one 1-substep step) of a batch at those states left."""
    if stem in _CACHE:
        return _CACHE[stem]
    from myosuite_mjx_amd import capi, model as M
    m = M.load_asset(stem)
    hm = capi.HipModel(m.blob(), 0)
    fams = {}
    for name, (q, hf) in FR.families(stem, m).items():
        n = len(q)
        assert n >= 8, (stem, name, n)
        ref, agree, bounds = FR.f32_reference(m, q.astype(np.float64), hf)
        b = capi.HipBatch(hm, n)
        b.write(capi.F_QPOS, q)
        if hf is not None:
            b.write(capi.F_HFIELD, hf.reshape(n, -1))
        state0 = {f: b.read(f) for f in (capi.F_QPOS, capi.F_QVEL, capi.F_ACT, capi.F_CTRL, capi.F_WARMSTART, capi.F_TIME, capi.F_QACC, capi.F_DIAG)}
        b.forward()
        got = {k: b.forward_read(w) for k, w in capi.FWD_NAMES.items() if not (w == capi.FWD_SITE_XMAT and "site_quat" not in m.arrays)}
        flags = b.status()
        unchanged = all(np.array_equal(b.read(f), v) for f, v in state0.items())
        b.step(None, capi.ACTMAP_NONE, 1)
        fams[name] = dict(q=q, hf=hf, ref=ref, agree=agree, bounds=bounds, got=got, flags=flags, unchanged=unchanged, diag=b.read(capi.F_DIAG), batch=b)
    _CACHE[stem] = dict(m=m, hm=hm, fams=fams)
    return _CACHE[stem]


def _frame_errors(m, got, ref, e, row=None):
    """max |position| and |rotation entry| difference of env e's frames (row: its row in `got`, e by default) against the float64 record."""
    r = e if row is None else row
    dp = max(np.abs(got[k][r] - ref[e][k]).max() for k in ("xpos", "xipos", "geom_xpos", "site_xpos"))
    dr = max(np.abs(got[k][r] - ref[e][k]).max() for k in ("xmat", "geom_xmat"))
    if "site_xmat" in got:
        dr = max(dr, np.abs(got["site_xmat"][r] - ref[e]["site_xmat"]).max())
    return dp, dr


@pytest.mark.parametrize("stem", FR.ASSETS)
def test_frames(stem):
    from myosuite_mjx_amd import capi
    A = _asset(stem)
    m = A["m"]
    assert A["hm"].forward_dims()[:3] == (m.nbody, m.nsite, m.ngeom)
    for name, F in A["fams"].items():
        got = F["got"]
        n = len(F["q"])
        assert got["xpos"].shape == (n, m.nbody, 3) and got["xmat"].shape == (n, m.nbody, 3, 3) and got["geom_xmat"].shape == (n, m.ngeom, 3, 3)
        assert got["site_xpos"].shape == (n, m.nsite, 3) and got["ncon"].shape == (n,) and got["ncon"].dtype == np.int32
        assert ("site_xmat" in got) == ("site_quat" in m.arrays)
        err = np.array([_frame_errors(m, got, F["ref"], e) for e in range(n)])
        print(f"forward frames {stem}/{name}: max|dpos| {err[:, 0].max():.2e} max|drot| {err[:, 1].max():.2e}")
        assert err[:, 0].max() < POS_TOL and err[:, 1].max() < ROT_TOL, (stem, name, err.max(0))
        assert np.abs(got["xmat"]).max() <= 1 + 1e-6 and F["unchanged"]
    if "site_quat" not in m.arrays:
        with pytest.raises(capi.MyoError, match="error -4"):
            next(iter(A["fams"].values()))["batch"].forward_ptr(capi.FWD_SITE_XMAT)
    # B = 1 and B = 3: the first states of the first family
    name, F = next(iter(A["fams"].items()))
    for B in (1, 3):
        b = capi.HipBatch(A["hm"], B)
        b.write(capi.F_QPOS, F["q"][:B])
        if F["hf"] is not None:
            b.write(capi.F_HFIELD, F["hf"][:B].reshape(B, -1))
        b.forward()
        got = {k: b.forward_read(w) for k, w in capi.FWD_NAMES.items() if k in F["got"]}
        for e in range(B):
            dp, dr = _frame_errors(m, got, F["ref"], e)
            assert dp < POS_TOL and dr < ROT_TOL, (stem, B, e, dp, dr)
        assert np.array_equal(got["ncon"], F["got"]["ncon"][:B])


@pytest.mark.parametrize("stem", FR.ASSETS)
def test_contacts(stem):
    A = _asset(stem)
    m = A["m"]
    ncap = A["hm"].forward_dims()[3]
    assert ncap == (128 if stem in ("myohand_baoding", "myohand_die", "myohand_object_airplane", "myohand_object_cup") else 64)
    for name, F in A["fams"].items():
        got, ref, n = F["got"], F["ref"], len(F["q"])
        assert got["contact"].shape == (n, ncap, 16) and not F["flags"].any(), (stem, name, F["flags"].tolist())
        same = np.zeros(n, bool)
        worst = np.zeros(3)
        orth = tang = 0.0
        for e in range(n):
            con, frames = FR.gpu_contacts(got["contact"], got["ncon"], e)
            oc = ref[e]["contacts"]
            same[e] = FR.pair_multiset(con) == FR.pair_multiset(oc)
            if not same[e]:
                print(f"forward contacts {stem}/{name}: env {e} differs: gpu {FR.pair_multiset(con)} oracle {FR.pair_multiset(oc)}")
                continue
            dev = FR.deviation(oc, con)
            if (dev >= F["bounds"]).any():
                print(f"forward contacts {stem}/{name}: env {e} beyond the bounds: {FR.worst_contacts(oc, con)}")
            worst = np.maximum(worst, dev)
            for k, Fr in enumerate(frames):
                orth = max(orth, np.abs(Fr @ Fr.T - np.eye(3)).max(), np.abs(np.cross(Fr[0], Fr[1]) - Fr[2]).max(), np.abs(Fr[0] - con[k, 4:7]).max())
            # the tangents against a numpy restatement of the row stage's rule on the contact's own normal (mju_makeFrame; capsule axis for
            # plane - capsule pairs, the axis from the oracle's geom_xmat)
            tang = max(tang, FR.frame_error(m, con, frames, ref[e]["geom_xmat"]))
        noc = np.array([len(r["contacts"]) for r in ref])
        print(f"forward contacts {stem}/{name}: pair sets equal in {same.sum()} of {n} envs (float32 oracle: {F['agree'].sum()}), ncon {noc.min()}..{noc.max()}, "
              f"dist / pos / normal deviation {worst[0]:.2e} / {worst[1]:.2e} / {worst[2]:.2e}, bounds {F['bounds'][0]:.2e} / {F['bounds'][1]:.2e} / {F['bounds'][2]:.2e}, "
              f"|F F^T - I| {orth:.1e}, tangents against the restatement {tang:.1e}")
        assert same.mean() >= 0.9, (stem, name, same.sum(), n)
        assert (worst < F["bounds"]).all(), (stem, name, worst, F["bounds"])
        assert orth < 1e-5 and tang < 1e-5, (stem, name, orth, tang)
        if name == "feet_on_ground":      # plane - capsule contacts, whose first tangent follows the capsule axis, are among them
            assert any(int(m.geom_type[int(c[7])]) == 0 and int(m.geom_type[int(c[8])]) == 3 for r in ref for c in r["contacts"])
        if name == "free":
            assert not got["ncon"].any() and not noc.any()
        if name == "crowded":      # contacts beyond the NC = 32 rows of LDS come out of the overflow rows
            assert noc.max() > 32 and got["ncon"][same].max() > 32 and noc.max() < 64
        if name == "grasp":        # more than 64: the export's second round, the TRK class's second contact bank
            assert noc.max() > 64 and got["ncon"][same].max() > 64 and noc.max() <= 128


@pytest.mark.parametrize("stem", FR.ASSETS)
def test_ncon_is_the_next_steps_first_substep(stem):
    for name, F in _asset(stem)["fams"].items():
        assert np.array_equal(F["got"]["ncon"], F["diag"][:, 1]), (stem, name, F["got"]["ncon"].tolist(), F["diag"][:, 1].tolist())


ROLLOUT_FIELDS = ("F_QPOS", "F_QVEL", "F_ACT", "F_WARMSTART", "F_QACC", "F_DIAG", "F_OBS", "F_REWARD")


@pytest.mark.parametrize("env_id", ["myoHandPoseRandom-v0", "myoLegWalk-v0", "myoChallengeBaodingP1-v1"])
def test_rollout_with_forward_between_the_steps_is_bitwise_the_same(env_id):
    """Hand, 36-dof and TrackEnv classes through the env layer: two envs, same seed, same actions, one calls forward() before every step."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    B = 64
    envs = [myo.make(env_id, num_envs=B, seed=3, as_torch=False) for _ in range(2)]
    for env in envs:
        env.reset()
    state = ("F_QPOS", "F_QVEL", "F_ACT", "F_CTRL", "F_WARMSTART", "F_TIME", "F_QACC", "F_DIAG", "F_OBS", "F_REWARD", "F_ELAPSED")
    before = {f: envs[1].batch.read(getattr(capi, f)) for f in state}
    rec = envs[1].forward()
    for f in state:      # forward alone: every state field bitwise unchanged
        assert np.array_equal(envs[1].batch.read(getattr(capi, f)), before[f]), f
    assert rec.xpos.shape[:2] == (B, envs[1].batch.model.forward_dims()[0]) and np.isfinite(rec.xpos).all()
    rng = np.random.default_rng(5)
    nu = envs[0].batch.model.dims.nu
    for k in range(20):
        a = rng.uniform(-1, 1, (B, nu)).astype(np.float32)
        envs[1].forward()
        for env in envs:
            env.step(a)
    for f in ROLLOUT_FIELDS:
        x, y = (env.batch.read(getattr(capi, f)) for env in envs)
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), (env_id, f)
    assert np.abs(envs[0].batch.read(capi.F_QPOS) - before["F_QPOS"]).max() > 1e-4


def test_override_body_quat_and_goal_offset():
    """Die asset: the target body turned (MYO_F_BODYQUAT) and moved (the goal offset, MYO_F_TARGET) per env, against the oracle on
    Model.with_body_quat / with_body_pos blobs: the target's body frame, sites and geoms."""
    import test_gpu_die as TD
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    A = _asset("myohand_die")
    m = A["m"]
    N = 8
    q = A["fams"]["rollout"]["q"][:N]
    rng = np.random.default_rng(2)
    tb = m.name2id("body", "target")
    quat = rng.normal(0, 1, (N, 4))
    quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)
    off = rng.uniform(-0.01, 0.01, (N, 3)).astype(np.float32)
    b = H.new_batch(TD.CASE, m, N)
    for f, x in ((capi.F_QPOS, q), (capi.F_BODYQUAT, quat), (capi.F_TARGET, off)):
        b.write(f, x)
    b.forward()
    got = {k: b.forward_read(capi.FWD_NAMES[k]) for k in ("xpos", "xmat", "xipos", "geom_xpos", "geom_xmat", "site_xpos")}
    sites = [s for s in range(m.nsite) if m.site_bodyid[s] == tb]
    geoms = [g for g in range(m.ngeom) if m.geom_bodyid[g] == tb]
    assert len(sites) >= 4      # (the target carries sites only; its geoms, if a model has any, are compared with all the others below)
    for e in range(N):
        qe = quat[e].astype(np.float64)
        mm = m.with_body_quat(tb, qe / np.linalg.norm(qe)).with_body_pos(tb, m.body_pos[tb] + off[e].astype(np.float64))
        ref = FR.oracle_forward(Oracle(mm.blob()), mm, q[e].astype(np.float64))
        dp, dr = _frame_errors(m, got, [ref], 0, row=e)
        assert dp < POS_TOL and dr < ROT_TOL, (e, dp, dr)
        base = A["fams"]["rollout"]["ref"][e]      # ... and the override really moved the target
        assert np.abs(ref["site_xpos"][sites] - base["site_xpos"][sites]).max() > 1e-3 and np.abs(ref["xmat"][tb] - base["xmat"][tb]).max() > 1e-2
        assert not geoms or np.abs(ref["geom_xmat"][geoms] - base["geom_xmat"][geoms]).max() > 1e-2


def test_override_body_pos():
    """Key-turn asset: the key's root body moved per env (MYO_F_BODYPOS) against the oracle on Model.with_body_pos blobs."""
    from myosuite_mjx_amd import capi, model as M
    from oracle.oracle import Oracle
    m = M.load_asset("myohand_keyturn")
    N = 16
    rng = np.random.default_rng(4)
    kb = int(m.jnt_bodyid[-1])
    q = FR._range_states(m, rng, N, 0.5).astype(np.float32)
    d = rng.uniform(-0.02, 0.02, (N, 3)).astype(np.float32)
    b = capi.HipBatch(capi.HipModel(m.blob(), 0), N)
    b.write(capi.F_QPOS, q)
    b.write(capi.F_BODYPOS, d)
    b.forward()
    got = {k: b.forward_read(capi.FWD_NAMES[k]) for k in ("xpos", "xmat", "xipos", "geom_xpos", "geom_xmat", "site_xpos", "ncon", "contact")}
    same, worst, worst32 = 0, np.zeros(3), np.zeros(3)
    for e in range(N):
        mm = m.with_body_pos(kb, m.body_pos[kb] + d[e].astype(np.float64))
        ref = FR.oracle_forward(Oracle(mm.blob()), mm, q[e].astype(np.float64))
        c32 = FR.oracle_forward(Oracle(mm.blob(), f32=True), mm, q[e].astype(np.float64))["contacts"]
        if FR.pair_multiset(c32) == FR.pair_multiset(ref["contacts"]):
            worst32 = np.maximum(worst32, FR.deviation(ref["contacts"], c32))
        dp, dr = _frame_errors(m, got, [ref], 0, row=e)
        assert dp < POS_TOL and dr < ROT_TOL, (e, dp, dr)
        assert np.abs(got["xpos"][e, kb] - (FR.oracle_forward(Oracle(m.blob()), m, q[e].astype(np.float64))["xpos"][kb] + d[e])).max() < POS_TOL
        con = FR.gpu_contacts(got["contact"], got["ncon"], e)[0]
        if FR.pair_multiset(con) == FR.pair_multiset(ref["contacts"]):
            same += 1
            worst = np.maximum(worst, FR.deviation(ref["contacts"], con))
    bounds = FR.bounds_from(worst32)
    print(f"forward body pos: pair sets equal in {same} of {N}, deviation {worst}, bounds {bounds}")
    assert same >= 0.9 * N and (worst < bounds).all(), (same, worst, bounds)      # check 2's convention: 90 % of the envs, 4 x the float32 oracle's deviation


def test_override_geom_size():
    """Hold asset: the object's size per env (MYO_F_GEOMSIZE) shows in the contacts, against oracles with myoo_set_geom_size."""
    from myosuite_mjx_amd import capi
    from oracle.oracle import Oracle
    A = _asset("myohand_hold")
    m = A["m"]
    N = 16
    q = A["fams"]["object_in_palm"]["q"][:N]
    og = m.name2id("geom", "object")
    rng = np.random.default_rng(6)
    sizes = rng.uniform(0.020, 0.030, (N, 3)).astype(np.float32)
    b = capi.HipBatch(A["hm"], N)
    b.set_geom_override(og, (0.02,) * 3, (0.03,) * 3)
    b.write(capi.F_QPOS, q)
    b.write(capi.F_GEOMSIZE, np.concatenate([sizes, sizes.max(1, keepdims=True)], 1))
    b.forward()
    ncon, rec = b.forward_read(capi.FWD_NCON), b.forward_read(capi.FWD_CONTACT)
    same, worst, worst32, differs = 0, np.zeros(3), np.zeros(3), 0
    for e in range(N):
        o, o32 = Oracle(m.blob()), Oracle(m.blob(), f32=True)
        o.set_geom_size(og, sizes[e]); o32.set_geom_size(og, sizes[e])
        oc = FR.oracle_forward(o, m, q[e].astype(np.float64))["contacts"]
        c32 = FR.oracle_forward(o32, m, q[e].astype(np.float64))["contacts"]
        if FR.pair_multiset(c32) == FR.pair_multiset(oc):
            worst32 = np.maximum(worst32, FR.deviation(oc, c32))
        con = FR.gpu_contacts(rec, ncon, e)[0]
        if FR.pair_multiset(con) == FR.pair_multiset(oc):
            same += 1
            worst = np.maximum(worst, FR.deviation(oc, con))
        base = A["fams"]["object_in_palm"]["ref"][e]["contacts"]
        differs += len(base) != len(oc) or (len(oc) > 0 and np.abs(np.sort(base[:, 0]) - np.sort(oc[:, 0])).max() > 1e-4)
    bounds = FR.bounds_from(worst32)      # 4 x the float32 oracle's deviation on the same states with the same size edits
    print(f"forward geom size: pair sets equal in {same} of {N}, deviation {worst}, bounds {bounds}")
    assert same >= 0.9 * N and (worst < bounds).all() and differs >= N // 2      # (the size edit changes the contacts of most states)


def test_bad_env():
    """A NaN qpos in one env of eight: flagged, zero rows, ncon 0, state NOT reset; the other seven as without it."""
    from myosuite_mjx_amd import capi
    A = _asset("myohand_pose")
    F = A["fams"]["range90"]
    q = F["q"][:8].copy()
    v = np.full((8, A["m"].nv), 0.25, np.float32)
    b = capi.HipBatch(A["hm"], 8)
    b.write(capi.F_QPOS, q)
    b.write(capi.F_QVEL, v)
    b.forward()                     # (a good pass first: the bad env's rows hold something to be zeroed)
    assert b.forward_read(capi.FWD_XMAT)[3].any() and not b.status().any()
    q[3, 5] = np.nan
    b.write(capi.F_QPOS, q)
    b.forward()
    got = {k: b.forward_read(w) for k, w in capi.FWD_NAMES.items() if k in F["got"]}
    fl = b.status()
    assert fl.tolist() == [0, 0, 0, capi.FLAG_BAD_STATE, 0, 0, 0, 0]
    for k, x in got.items():
        assert not x[3].any(), k
        keep = [e for e in range(8) if e != 3]
        if k == "contact":
            for e in keep:
                assert np.array_equal(x[e, :got["ncon"][e]], F["got"][k][e, :got["ncon"][e]])
        else:
            assert np.array_equal(x[keep], F["got"][k][keep]), k
    assert np.array_equal(b.read(capi.F_QPOS), q, equal_nan=True) and np.array_equal(b.read(capi.F_QVEL), v)


def test_surfaces_and_refusals():
    import torch
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import capi
    A = _asset("myohand_pose")
    m, F = A["m"], A["fams"]["range90"]
    q = F["q"][:4]
    # capi: nothing before the first forward; bad ids
    b = capi.HipBatch(A["hm"], 4)
    for w in (capi.FWD_XPOS, capi.FWD_NCON):
        with pytest.raises(capi.MyoError, match="error -1"):
            b.forward_ptr(w)
    with pytest.raises(capi.MyoError, match="error -1"):
        b.forward_read(capi.FWD_XPOS)
    b.forward()
    for w in (-1, capi.FWD_COUNT):
        with pytest.raises(capi.MyoError, match="error -1"):
            b.forward_ptr(w)
    assert b.forward_ptr(capi.FWD_CONTACT)[2] == 16 * A["hm"].forward_dims()[3]
    # a model on the generic lanes kernel: with lanes != 64 the hand model steps there, and forward (the wave kernel's twin) is refused
    capi.set_lanes(32)
    try:
        with pytest.raises(capi.MyoError, match="error -4.*lanes"):
            b.forward()
        with pytest.raises(capi.MyoError, match="error -4.*lanes"):
            A["hm"].forward_dims()
        with pytest.raises(capi.MyoError, match="error -4.*lanes"):
            capi.HipBatch(A["hm"], 2).forward()
    finally:
        capi.set_lanes(64)
    b.forward()
    # functional surface
    dm = myo.put_model("myohand_pose")
    d = myo.make_data(dm, 4)
    myo.set_(d, "qpos", q)
    assert myo.forward(dm, d) is d
    for k in ("xpos", "xmat", "xipos", "site_xpos", "geom_xpos", "geom_xmat", "ncon", "contact"):
        assert np.array_equal(myo.get(d, k), F["got"][k][:4]), k
    # HipSimScene: opt-in; without the kwarg no attribute and no launch
    plain = myo.HipSimScene("myohand_pose", num_envs=4)
    plain.forward()
    assert not hasattr(plain.data, "xpos") and not hasattr(plain.data, "ncon")
    with pytest.raises(capi.MyoError, match="error -1"):
        plain._batch.forward_ptr(capi.FWD_XPOS)
    # device-resident: zero-copy views that a later forward() refreshes in place
    sim = myo.HipSimScene("myohand_pose", num_envs=4, kinematics=True)
    assert sim.data.xpos.data_ptr() == sim._batch.forward_ptr(capi.FWD_XPOS)[0] and sim.data.contact.dist.data_ptr() == sim._batch.forward_ptr(capi.FWD_CONTACT)[0]
    assert sim.data.body_xpos is sim.data.xpos and sim.data.ncon.dtype == torch.int32 and sim.data.contact.geom1.dtype == torch.int32
    x0 = sim.data.site_xpos
    sim.data.qpos[:] = q
    sim.forward()
    torch.cuda.synchronize()
    assert sim.data.site_xpos is x0
    assert sim.data.xpos.shape == (4, m.nbody, 3) and sim.data.geom_xmat.shape == (4, m.ngeom, 3, 3) and sim.data.contact.frame.shape[2] == 9
    for k in ("xpos", "xmat", "site_xpos", "geom_xpos", "ncon"):
        assert np.array_equal(getattr(sim.data, k).cpu().numpy(), F["got"][k][:4]), k
    for k, lo, hi in (("dist", 0, 1), ("pos", 1, 4), ("frame", 4, 13)):
        assert np.array_equal(getattr(sim.data.contact, k).cpu().numpy().reshape(4, -1, hi - lo), F["got"]["contact"][:4, :, lo:hi]), k
    n0 = int(F["got"]["ncon"][1])
    assert np.array_equal(sim.data.contact.geom1.cpu().numpy()[1, :n0], F["got"]["contact"][1, :n0, 13].copy().view(np.int32))
    # host mirrors: forward() pushes the dirty state and refreshes the arrays
    host = myo.HipSimScene("myohand_pose", num_envs=4, as_torch=False, kinematics=True)
    host.data.qpos[:] = q
    host.mark_dirty()
    host.forward()
    for k in ("xpos", "xipos", "geom_xmat", "ncon"):
        assert isinstance(getattr(host.data, k), np.ndarray) and np.array_equal(getattr(host.data, k), F["got"][k][:4]), k
    assert np.array_equal(host.data.body_xmat, F["got"]["xmat"][:4]) and host.data.contact.geom2.dtype == np.int32
    # envs: the record of the env's batch (the TrackEnv classes share the method)
    from myosuite_mjx_amd import track
    assert track.TrackEnv.forward is capi.FieldViews.forward and myo.BatchedMyoEnv.forward is capi.FieldViews.forward
    env = myo.make("myoHandPoseRandom-v0", num_envs=4, seed=1)
    env.reset()
    r = env.forward()
    torch.cuda.synchronize()
    assert r.xpos.data_ptr() == env.batch.forward_ptr(capi.FWD_XPOS)[0] and r.xpos.shape == (4, m.nbody, 3) and bool(torch.isfinite(r.geom_xpos).all())


def test_guard_poisoned_build():
    H.rerun_file_against_poison_build(__file__, timeout=900)
