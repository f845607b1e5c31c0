"""The rows and states that tests/test_gpu_object_params.py steps on the GPU and tests/test_object_params_host.py runs through the oracle
alone: one selection, so that the CPU check speaks about the states the GPU comparison uses."""
import numpy as np

CH = np.array([0.2, 0.001, 0.00002])           # obj_friction_change of both P2 ids
f32 = np.float32
BD_KINDS = (("palm", 1), ("ballball", 2), ("floor", 4))      # (kind, seed) of tests/test_gpu_baoding.py::_states


def baoding_states(m):
    """{kind: (qpos, qvel)} float32 [8, ...], one set per kind."""
    from test_gpu_baoding import _states
    return {k: _states(m, k, 8, s)[:2] for k, s in BD_KINDS}


def die_states(m):
    """(qpos, qvel, act) float32 [8, ...] picked from two oracle episodes of tests/die_states.py."""
    from die_states import pick_states, rollout_states
    P = pick_states(rollout_states(m, steps=60, seeds=(None, 1)), 8)
    assert len(P) == 8
    return tuple(np.array([s[k] for s in P]).astype(f32) for k in range(3))


def die_rows8(m):
    """die_rows for the eight picked states: the four rows twice."""
    gs, bs, size, pos, fr, mass = die_rows(m, 4)
    return gs, bs, np.tile(size, (2, 1, 1)), np.tile(pos, (2, 1, 1)), np.tile(fr, (2, 1, 1)), np.tile(mass, (2, 1))


def bd_rows(m, B):
    """[B] distinct explicit rows of the two balls: the nominal row, then both extremes of size, friction and mass, then a mixed one."""
    from myosuite_mjx_amd import objects
    gs, bs = objects.task_objects(m, "baoding")
    size = np.tile(np.array(m.geom_size, float)[gs], (B, 1, 1))
    fr = np.tile(np.array(m.geom_friction, float)[gs], (B, 1, 1))
    mass = np.tile(np.array(m.body_mass, float)[bs], (B, 1))
    size[1], size[2] = 0.018, 0.024
    fr[3], fr[4] = fr[3] - CH, fr[4] + CH
    mass[5], mass[6] = 0.030, 0.300
    size[7, 0], size[7, 1], fr[7, 0], fr[7, 1], mass[7] = 0.019, 0.0235, fr[7, 0] + 0.5 * CH, fr[7, 1] - 0.7 * CH, (0.1, 0.2)
    return gs, bs, size.astype(f32), fr.astype(f32), mass.astype(f32)


def die_rows(m, B):
    """[B] rows of the die: nominal, del_size = -0.007 and +0.007 with the reference's size / pos rule, and friction / mass at their ends."""
    from myosuite_mjx_amd import objects
    gs, bs = objects.task_objects(m, "die")
    size0, pos0, fr0 = (np.array(m.arrays[k], float)[gs] for k in ("geom_size", "geom_pos", "geom_friction"))
    size, pos, fr, mass = np.tile(size0, (B, 1, 1)), np.tile(pos0, (B, 1, 1)), np.tile(fr0, (B, 1, 1)), np.full((B, 1), float(m.body_mass[bs[0]]))
    for e, d in ((1, -0.007), (2, 0.007), (3, 0.004)):
        size[e, :-3, 1] += d
        size[e, -3:] += d
        pos[e] = pos0 + np.sign(pos0) * d
    fr[2], mass[2] = fr0 + CH, 0.25
    fr[3], mass[3] = fr0 - CH, 0.05
    return gs, bs, size.astype(f32), pos.astype(f32), fr.astype(f32), mass.astype(f32)


def edited(m, gs, bs, size, pos, fr, mass):
    """The model edited with one env's float32 rows: geoms first (re-lowered), then the masses (link tables only)."""
    e = m.with_geom_params(gs, size=np.asarray(size, float), pos=None if pos is None else np.asarray(pos, float), friction=np.asarray(fr, float))
    for b, x in zip(bs, mass):
        e = e.with_body_mass(int(b), float(x))
    return e
