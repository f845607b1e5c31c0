"""CPU tests of the per-env object parameters (include/myo_hip_objects.h, myosuite_mjx_amd/objects.py): the binding of the new header, what
licenses per-env sizes over one shared pair table (re-lowering the committed baoding and die models at the extreme P2 values changes the
size, position, bounding-radius and friction tables and nothing else), the draw tables of the two tasks against a float64 restatement of
the reference's reset bodies, the oracle alone on the states and rows the GPU comparison uses, and the argument errors.  Nothing here
needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_capi_host as T

ROOT = T.ROOT
HEADER = "myo_hip_objects.h"


# ---- binding ------------------------------------------------------------------------------------------------------------------------
def test_binding_of_the_objects_header(monkeypatch):
    from myosuite_mjx_amd import capi, objects
    monkeypatch.setattr(T, "HEADERS", (HEADER,))
    protos = T._header_prototypes()
    assert sorted(protos) == sorted(objects.SIGNATURES) and len(protos) == 6
    assert protos["myo_objects_write"] == (ctypes.c_int, ["pointer", ctypes.c_int, "pointer", ctypes.c_size_t])      # (the parser parses)
    for name, (ret, args) in protos.items():
        restype, argtypes = objects.SIGNATURES[name]
        assert (T._ctypes_kind(restype), [T._ctypes_kind(t) for t in argtypes]) == (ret, args), name
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    L = ctypes.CDLL(capi.LIB_PATH)
    assert not [n for n in protos if not hasattr(L, n)]
    L = objects.lib()                                             # and objects.lib() has applied its own table to capi's handle
    assert L is capi.lib()
    for name, (restype, argtypes) in objects.SIGNATURES.items():
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == list(argtypes), name
    # the core header and the core table do not know the subsystem
    assert HEADER not in open(os.path.join(ROOT, "include", "myo_hip.h")).read() and "myo_objects" not in T._header_text("myo_hip.h")
    assert len(capi.SIGNATURES) == 63 and not set(capi.SIGNATURES) & set(objects.SIGNATURES)
    enums = T._header_enums(open(os.path.join(ROOT, "include", HEADER)).read())
    assert [enums[k] for k in ("MYO_OBJ_SIZE", "MYO_OBJ_POS", "MYO_OBJ_FRICTION", "MYO_OBJ_MASS")] == [objects.OBJ_SIZE, objects.OBJ_POS, objects.OBJ_FRICTION, objects.OBJ_MASS]
    hdr = open(os.path.join(ROOT, "include", HEADER)).read()
    for name, val in (("MYO_OBJ_MAX_GEOMS", objects.MAX_GEOMS), ("MYO_OBJ_MAX_BODIES", objects.MAX_BODIES), ("MYO_OBJ_MAX_DRAWS", objects.MAX_DRAWS)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr), name


def test_header_is_plain_c(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "hdr.c"
    src.write_text('#include "include/%s"\nint main(void) { return MYO_OBJ_COUNT == 4 ? 0 : 1; }\n' % HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", ROOT, "-c", str(src), "-o", str(tmp_path / "a.o")])


# ---- re-lowering --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bd():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_baoding")


@pytest.fixture(scope="module")
def die():
    from myosuite_mjx_amd import model as M
    return M.load_asset("myohand_die")


SHARED = ("hip_pair_i", "hip_pair_dl", "hip_cg_geom")
MAY_CHANGE = {"geom_size", "geom_pos", "geom_friction", "geom_rbound", "hip_cg_size", "hip_cg_lpos", "hip_cg_rbound", "hip_pair_f"}


def _changed(a, b):
    assert sorted(a.arrays) == sorted(b.arrays)
    return {k for k in a.arrays if np.asarray(a.arrays[k]).tobytes() != np.asarray(b.arrays[k]).tobytes()}


def _die_edit(m, delta):
    """ReorientEnvV0.reset's size and position rule for one del_size (reorient_v0.py:232-247), float64."""
    from myosuite_mjx_amd import objects
    gs, _ = objects.task_objects(m, "die")
    size, pos = np.array(m.geom_size, float)[gs], np.array(m.geom_pos, float)[gs]
    size[:-3, 1] += delta
    size[-3:] += delta
    pos = pos / abs(pos + 1e-16) * (abs(pos) + delta)
    return gs, size, pos


def test_relowering_at_the_p2_extremes_keeps_the_pair_table(bd, die):
    from myosuite_mjx_amd import objects
    gs, _ = objects.task_objects(bd, "baoding")
    fr0 = np.array(bd.geom_friction, float)[gs]
    ch = np.array([0.2, 0.001, 0.00002])
    for r in (0.018, 0.024):
        for sgn in (-1, 1):
            e = bd.with_geom_params(gs, size=np.full((2, 3), r), friction=fr0 + sgn * ch)
            d = _changed(bd, e)
            assert d and d <= MAY_CHANGE and not d & set(SHARED), d
            assert {"hip_cg_size", "hip_cg_rbound", "hip_pair_f"} <= d and "hip_cg_lpos" not in d
            cg = [list(e.hip_cg_geom).index(g) for g in gs]
            assert np.allclose(np.asarray(e.hip_cg_rbound)[cg], r) and np.allclose(np.asarray(e.hip_cg_size).reshape(-1, 3)[cg], r)
    for delta in (-0.007, 0.007):
        g, size, pos = _die_edit(die, delta)
        e = die.with_geom_params(g, size=size, pos=pos, friction=np.array(die.geom_friction, float)[g] + ch)
        d = _changed(die, e)
        assert d <= MAY_CHANGE and {"hip_cg_size", "hip_cg_lpos", "hip_cg_rbound", "hip_pair_f"} <= d, d
        cg = [list(e.hip_cg_geom).index(x) for x in g]
        assert np.allclose(np.asarray(e.hip_cg_lpos).reshape(-1, 3)[cg], pos, atol=1e-15)      # the die's body frame is its link frame
    # friction alone can only touch the pair floats, and there the two friction columns only; a friction below the partners' (all geoms
    # of the model have the nominal 1.0) changes no pair at all: the mix is the component-wise maximum
    assert _changed(die, die.with_geom_params(g, friction=np.array(die.geom_friction, float)[g] - ch)) == {"geom_friction"}
    e = die.with_geom_params(g, friction=np.array(die.geom_friction, float)[g] + ch)
    assert _changed(die, e) == {"geom_friction", "hip_pair_f"}
    df = np.asarray(e.hip_pair_f).reshape(-1, 12) != np.asarray(die.hip_pair_f).reshape(-1, 12)
    assert df[:, [2, 11]].any() and not np.delete(df, [2, 11], axis=1).any()


def test_selected_bodies_are_alone_in_their_links(bd, die):
    """What lets the link's mass be the env's scalar: ball1, ball2 and the die's Object are the only bodies of their kinematic links, and
    their body frame is the link frame (so a geom position passes into the link frame unchanged)."""
    from myosuite_mjx_amd import objects
    for m, task in ((bd, "baoding"), (die, "die")):
        gs, bs = objects.task_objects(m, task)
        assert len(gs) == (2 if task == "baoding" else 15) and len(bs) == (2 if task == "baoding" else 1)
        link = np.asarray(m.hip_body_link)
        for b in bs:
            assert link[b] >= 0 and (link == link[b]).sum() == 1
            assert not np.asarray(m.hip_body_lpos).reshape(-1, 3)[b].any() and np.asarray(m.hip_body_lquat).reshape(-1, 4)[b].tolist() == [1, 0, 0, 0]
        assert all(g in list(m.hip_cg_geom) for g in gs) and {int(m.geom_bodyid[g]) for g in gs} == set(bs)
        assert len(set(np.asarray(m.geom_priority).tolist())) == 1      # equal priorities: the friction mix is the component-wise maximum


# ---- the oracle alone on the states the GPU tests use ------------------------------------------------------------------------------------
def _oracle_alone_share(m, rows, state, nsub, seed_a):
    """Float32 build of the oracle against the float64 one, on the edited blob of every env's row: the share of states where both end with
    the same contact count (the condition tests/test_gpu_object_params.py compares the kernel under), and the float64 counts."""
    import object_params_cases as K
    from die_states import muscle_ctrl
    from oracle.oracle import Oracle
    gs, bs, size, pos, fr, mass = rows
    q, v, act = state
    a = np.random.default_rng(seed_a).uniform(-1, 1, (len(q), m.nu)).astype(np.float32)
    out = {n: [] for n in nsub}
    for e in range(len(q)):
        blob = K.edited(m, gs, bs, size[e], None if pos is None else pos[e], fr[e], mass[e]).blob()
        for n in nsub:
            nc = []
            for f32 in (False, True):
                o = Oracle(blob, f32=f32)
                o.reset()
                o.set_state(qpos=q[e], qvel=v[e], act=act[e], ctrl=muscle_ctrl(a[e]))
                assert o.step(n) == 0
                nc.append(int(o.ncon))
            out[n].append(nc)
    return {n: np.array(x) for n, x in out.items()}


def test_oracle_alone_keeps_the_contact_count_share_baoding(bd):
    """The baoding states and rows of the GPU comparison (palm, ball - ball, floor; nominal row, both extremes of size, friction and mass,
    a mixed row), 1 and 10 substeps: the float32 oracle has the float64 oracle's contact count in more than 0.8 of the states, so no chosen
    state sits on a contact-count edge for its row -- the extreme radii included."""
    import object_params_cases as K
    gs, bs, size, fr, mass = K.bd_rows(bd, 8)
    S = K.baoding_states(bd)
    tot = {1: [], 10: []}
    for kind, _ in K.BD_KINDS:
        q, v = S[kind]
        act = np.random.default_rng(3).uniform(0, 1, (8, bd.nu)).astype(np.float32)
        r = _oracle_alone_share(bd, (gs, bs, size, None, fr, mass), (q, v, act), (1, 10), 9)
        for n in (1, 10):
            tot[n] += (r[n][:, 0] == r[n][:, 1]).tolist()
            print(f"baoding {kind} nsub={n}: float64 ncon {r[n][:, 0].tolist()}, float32 {r[n][:, 1].tolist()}")
        assert (r[1][:, 0] >= 1).sum() >= 6, kind                 # (a ball shrunk to 0.018 can lose its contact: that is the row's physics, not an edge)
    for n in (1, 10):
        assert np.mean(tot[n]) > 0.8, (n, tot[n])


def test_oracle_alone_keeps_the_contact_count_share_die(die):
    import object_params_cases as K
    r = _oracle_alone_share(die, K.die_rows8(die), K.die_states(die), (1, 10), 9)
    for n in (1, 10):
        print(f"die nsub={n}: float64 ncon {r[n][:, 0].tolist()}, float32 {r[n][:, 1].tolist()}")
        assert (r[n][:, 0] == r[n][:, 1]).mean() > 0.8, (n, r[n].tolist())


# ---- draw tables --------------------------------------------------------------------------------------------------------------------
def _np_uniform(low, high, u):
    """numpy's Generator / RandomState uniform for a given underlying u in [0, 1): low + (high - low) * u."""
    return np.asarray(low, float) + (np.asarray(high, float) - np.asarray(low, float)) * u


def _baoding_reset_ref(m, gs, bs, u, size_range, mass_range, friction_change):
    """BaodingEnvV1._setup / reset (baoding_v1.py:115-135, 360-385) in float64 on copies of the model's arrays, the uniforms given:
    u = dict(mass [2], friction [2, 3], size [2])."""
    mass, fr, size = np.array(m.body_mass, float), np.array(m.geom_friction, float), np.array(m.geom_size, float)
    fr_lo, fr_hi = fr[gs[0]] - friction_change, fr[gs[0]] + friction_change          # the range is built from ball 1's friction
    for k in range(2):
        mass[bs[k]] = _np_uniform(mass_range[0], mass_range[1], u["mass"][k])
    for k in range(2):
        fr[gs[k]] = _np_uniform(fr_lo, fr_hi, u["friction"][k])
    for k in range(2):
        size[gs[k]] = _np_uniform(size_range[0], size_range[1], u["size"][k])          # a scalar assigned to the row: all three components
    return size[gs], fr[gs], mass[bs]


def _die_reset_ref(m, gs, bs, u, size_change, mass_range, friction_change):
    """ReorientEnvV0._setup / reset (reorient_v0.py:94-101, 221-247) in float64: u = dict(friction [15, 3], mass, size)."""
    mass, fr, size, pos = (np.array(m.arrays[k], float) for k in ("body_mass", "geom_friction", "geom_size", "geom_pos"))
    g0, gn = gs[0], gs[-1] + 1
    default_size, default_pos = size[g0:gn].copy(), pos[g0:gn].copy()
    fr[g0:gn] = _np_uniform(fr[g0:gn] - friction_change, fr[g0:gn] + friction_change, u["friction"])
    mass[bs[0]] = _np_uniform(mass_range[0], mass_range[1], u["mass"])
    del_size = _np_uniform(-size_change, size_change, u["size"])
    size[g0:gn - 3][:, 1] = default_size[:-3][:, 1] + del_size
    size[gn - 3:gn] = default_size[-3:] + del_size
    gpos = pos[g0:gn]
    pos[g0:gn] = gpos / abs(gpos + 1e-16) * (abs(default_pos) + del_size)
    return size[g0:gn], pos[g0:gn], fr[g0:gn], mass[bs], del_size


def _rows(t, size, pos, fr, mass):
    return np.concatenate([np.ravel(size), np.ravel(pos), np.ravel(fr), np.ravel(mass)])


def test_baoding_draw_table_restates_the_reference_reset(bd):
    from myosuite_mjx_amd import envs, objects
    m = bd
    gs, bs = objects.task_objects(m, "baoding")
    kw = envs.P2_CONFIGS["myoChallengeBaodingP2-v1"][2]
    t = objects.task_draws(m, "baoding", gs, bs, **kw)
    assert (t.ng, t.nb, t.ndraw) == (2, 2, 2)
    cur = _rows(t, np.array(m.geom_size)[gs], np.array(m.geom_pos)[gs], np.array(m.geom_friction)[gs], np.array(m.body_mass)[bs])
    rng = np.random.default_rng(0)
    for trial in range(6):
        u_sh, u_own = rng.uniform(0, 1, objects.MAX_DRAWS), rng.uniform(0, 1, 9 * t.ng + t.nb)
        if trial < 2:                                                 # the two ends of every range
            u_sh[:], u_own[:] = trial * (1 - 2.0 ** -24), trial * (1 - 2.0 ** -24)
        u = dict(mass=[u_own[t.index("mass", k)] for k in range(2)], size=[u_sh[k] for k in range(2)],
                 friction=[[u_own[t.index("friction", k, c)] for c in range(3)] for k in range(2)])
        size, fr, mass = _baoding_reset_ref(m, gs, bs, u, kw["obj_size_range"], kw["obj_mass_range"], np.array(kw["obj_friction_change"]))
        want = _rows(t, size, np.array(m.geom_pos)[gs], fr, mass)
        got = t.values(u_sh, u_own, cur)
        assert got.dtype == np.float32 and np.abs(got - want).max() <= 1e-7 * np.abs(want).max()      # float32 base / scale against float64
        assert (t.scale[t.index("pos", 0):t.index("friction", 0)] == 0).all()                          # the balls' positions are not drawn
    # size: both draws shared by the three components of their ball, independent between the balls; everything else has a draw of its own
    assert t.draw[:3].tolist() == [0, 0, 0] and t.draw[3:6].tolist() == [1, 1, 1] and (t.draw[6:] == objects.DRAW_OWN).all()
    assert 0.018 <= got[:6].min() and got[:6].max() <= 0.024


def test_die_draw_table_restates_the_reference_reset(die):
    from myosuite_mjx_amd import envs, objects
    m = die
    gs, bs = objects.task_objects(m, "die")
    kw = envs.P2_CONFIGS["myoChallengeDieReorientP2-v0"][2]
    t = objects.task_draws(m, "die", gs, bs, **kw)
    assert (t.ng, t.nb, t.ndraw) == (15, 1, 1)
    size0, pos0 = np.array(m.geom_size, float)[gs], np.array(m.geom_pos, float)[gs]
    cur = _rows(t, size0, pos0, np.array(m.geom_friction)[gs], np.array(m.body_mass)[bs])
    driven = np.flatnonzero(t.draw == 0)
    n_size, n_pos = (driven < 45).sum(), ((driven >= 45) & (driven < 90)).sum()
    assert (n_size, n_pos) == (12 + 9, 24)      # 12 half lengths, the 3 boxes' 9 sizes; the 24 non-zero of the 15 x 3 position components
    assert (pos0 != 0).sum() == 24 and (t.scale[45:90].reshape(15, 3)[pos0 == 0] == 0).all()
    rng = np.random.default_rng(1)
    for trial in range(6):
        u_sh, u_own = rng.uniform(0, 1, objects.MAX_DRAWS), rng.uniform(0, 1, 9 * t.ng + t.nb)
        if trial < 2:
            u_sh[:], u_own[:] = trial * (1 - 2.0 ** -24), trial * (1 - 2.0 ** -24)
        u = dict(friction=np.array([[u_own[t.index("friction", g, c)] for c in range(3)] for g in range(15)]), mass=u_own[t.index("mass", 0)], size=u_sh[0])
        size, pos, fr, mass, delta = _die_reset_ref(m, gs, bs, u, kw["obj_size_change"], kw["obj_mass_range"], np.array(kw["obj_friction_change"]))
        want = _rows(t, size, pos, fr, mass)
        got = t.values(u_sh, u_own, cur).astype(np.float64)
        # bound: float32 rounding of base, scale and the result (3 x 2^-24 relative to the largest term, 0.0284 + 0.014), and the reference's
        # 1e-16 guard in pos / |pos + 1e-16|
        assert np.abs(got - want)[:90].max() < 4 * 2.0 ** -24 * 0.05 and np.abs(got - want)[90:].max() < 4 * 2.0 ** -24 * 1.2
        # the correlated values exactly, in the float32 the kernel writes: every driven parameter is base + scale * u of ONE u, so del
        # reconstructed from one geom predicts the other 44 (the scales are +-2 * obj_size_change, equal up to sign)
        b32, s32 = t.base.astype(np.float32).astype(np.float64), t.scale.astype(np.float32).astype(np.float64)
        u_rec = (got[driven[0]] - b32[driven[0]]) / s32[driven[0]]
        assert abs(u_rec - u_sh[0]) < 2.0 ** -20
        assert np.array_equal(got[driven], (b32[driven] + s32[driven] * u_sh[0]).astype(np.float32).astype(np.float64))
        assert np.abs(np.abs(s32[driven]) - 0.014).max() < 1e-9 and abs(delta) <= 0.007
        assert np.array_equal(np.sign(got[45:90]), np.sign(pos0.ravel()))


def test_host_twin_of_the_draws_is_the_counter_rng():
    from myosuite_mjx_amd import objects
    from myosuite_mjx_amd.shard import u01
    t = objects.DrawTable(2, 1)
    sh, own = objects.draw_u(7, 0, 5, t)
    assert len(sh) == objects.MAX_DRAWS and len(own) == 19
    key = 7 ^ objects._DRAW_KEY
    assert sh[3] == u01(key, 5 * 1024 + 3, 12) and own[4] == u01(key, 5 * 1024 + 8 + 4, 12)
    sh1, own1 = objects.draw_u(7, 1, 5, t)                         # another episode, another env: other draws
    sh2, own2 = objects.draw_u(7, 0, 6, t)
    assert not np.array_equal(sh, sh1) and not np.array_equal(own, own2) and not np.array_equal(own, own1) and not np.array_equal(sh, sh2)
    v = np.array([objects.draw_u(3, 0, e, t)[0][0] for e in range(2000)])
    assert 0 <= v.min() and v.max() < 1 and abs(v.mean() - 0.5) < 0.03 and abs(v.var() - 1 / 12) < 0.01


# ---- errors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,kw", [
    ("baoding", dict(obj_size_range=(0.024, 0.018))), ("baoding", dict(obj_mass_range=(0.3, 0.03))), ("baoding", dict(obj_mass_range=(-0.1, 0.3))),
    ("baoding", dict(obj_friction_change=(0.2, -0.001, 0.0))), ("baoding", dict(obj_friction_change=(1.2, 0.001, 0.00002))),
    ("baoding", dict(obj_size_range=(-0.01, 0.02))), ("die", dict(obj_size_change=-0.007)), ("die", dict(obj_size_change=0.03)),
    ("die", dict(obj_mass_range=(0.25, 0.05))), ("die", dict(obj_friction_change=(float("nan"), 0.0, 0.0))),
])
def test_bad_randomization_arguments_raise_before_any_library_call(bd, die, task, kw):
    from myosuite_mjx_amd import objects
    m = bd if task == "baoding" else die
    with pytest.raises(ValueError):
        objects.task_draws(m, task, *objects.task_objects(m, task), **kw)


def test_other_argument_errors(bd):
    from myosuite_mjx_amd import objects
    with pytest.raises(TypeError, match="obj_size_change"):
        objects.task_draws(bd, "baoding", *objects.task_objects(bd, "baoding"), obj_size_change=0.007)      # the die's name
    with pytest.raises(NotImplementedError, match="baoding and die"):
        objects.task_draws(bd, "pen", [], [])
    assert objects.task_objects(bd, "pen") is None
    with pytest.raises(ValueError):
        bd.with_geom_params(["ball1"], size=[[-0.01, 0, 0]])
    for bad in (-1, bd.ngeom):                                     # a bad id is refused before anything is edited
        with pytest.raises(ValueError, match="no geom"):
            bd.with_geom_params([bad], size=[[0.02, 0, 0]])
    with pytest.raises(ValueError, match="shared draws"):
        t = objects.DrawTable(1, 0)
        for _ in range(objects.MAX_DRAWS + 1):
            t.new_draw()


def test_p2_configs_are_the_registered_numbers():
    """envs.P2_CONFIGS against the reference's registration text (envs/myo/myochallenge/__init__.py:336-353, 371-386), and split so that the
    make kwargs are ones the P1 id honours; the P2 ids themselves stay refused."""
    from myosuite_mjx_amd import envs, tasks
    b, d = envs.P2_CONFIGS["myoChallengeBaodingP2-v1"], envs.P2_CONFIGS["myoChallengeDieReorientP2-v0"]
    assert b[0] == "myoChallengeBaodingP1-v1" and d[0] == "myoChallengeDieReorientP1-v0"
    assert b[1] == dict(task_choice="random", goal_time_period=(4, 6), goal_xrange=(0.020, 0.030), goal_yrange=(0.022, 0.032))
    assert b[2] == dict(obj_size_range=(0.018, 0.024), obj_mass_range=(0.030, 0.300), obj_friction_change=(0.2, 0.001, 0.00002))
    assert d[1] == dict(goal_pos=(-0.020, 0.020), goal_rot=(-3.14, 3.14))
    assert d[2] == dict(obj_size_change=0.007, obj_mass_range=(0.050, 0.250), obj_friction_change=(0.2, 0.001, 0.00002))
    for p1, mk, rk in (b, d):
        task = envs.REGISTRY[p1]["task"]
        assert set(mk) <= set(tasks.TASKS[task].kwargs) and p1 in envs.REGISTRY
    for i in envs.P2_CONFIGS:
        assert i in envs.UNSUPPORTED and i not in envs.REGISTRY
