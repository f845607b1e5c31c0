"""Per-env object parameters (include/myo_hip_objects.h): size, position and friction of selected collision geoms and the mass of selected
bodies, one value per env, with an optional re-draw at every reset -- what myoChallengeBaodingP2-v1 does to its balls and
myoChallengeDieReorientP2-v0 to its die.  TrackEnv-class models only.

The ctypes prototypes of the header live here, in a table of their own (`SIGNATURES`), applied to the handle `capi.lib()` returns;
`capi.SIGNATURES` stays the table of the five core headers."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .shard import u01

OBJ_SIZE, OBJ_POS, OBJ_FRICTION, OBJ_MASS = range(4)
MAX_GEOMS, MAX_BODIES, MAX_DRAWS = 16, 4, 8
DRAW_OWN = -1                     # draw id of a parameter with a draw of its own
_TABLES = {"size": OBJ_SIZE, "pos": OBJ_POS, "friction": OBJ_FRICTION, "mass": OBJ_MASS}

_V, _I, _SZ = C.c_void_p, C.c_int, C.c_size_t
_pI, _pF = C.POINTER(_I), C.POINTER(C.c_float)
SIGNATURES = {
    "myo_objects_enable": (_I, [_V, _pI, _I, _pI, _I]),
    "myo_objects_count": (_I, [_V, _pI, _pI]),
    "myo_objects_table": (_I, [_V, _I, C.POINTER(_V), C.POINTER(_SZ), C.POINTER(_SZ)]),
    "myo_objects_read": (_I, [_V, _I, _V, _SZ]),
    "myo_objects_write": (_I, [_V, _I, _V, _SZ]),
    "myo_objects_set_draws": (_I, [_V, _I, _I, _pF, _pF, _pI]),
}
_applied = None


def lib():
    """capi.lib() with the prototypes of include/myo_hip_objects.h applied."""
    global _applied
    L = capi.lib()
    if _applied is not L:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _applied = L
    return L


def _ids(a):
    a = np.ascontiguousarray(a, np.int32).reshape(-1)
    return a, (a.ctypes.data_as(_pI) if a.size else None)


# ---- the draw table --------------------------------------------------------------------------------------------------------------
class DrawTable:
    """base / scale / draw of the 9 * ng + nb scalar parameters of a selection, in the library's order size | pos | friction | mass.
    Parameter p of an env becomes base[p] + scale[p] * u at every reset; scale 0 leaves it alone; draw[p] = k < ndraw shares draw k,
    DRAW_OWN gives the parameter its own."""

    def __init__(self, ng, nb):
        self.ng, self.nb, self.ndraw = int(ng), int(nb), 0
        n = 9 * self.ng + self.nb
        self.base, self.scale, self.draw = np.zeros(n), np.zeros(n), np.full(n, DRAW_OWN, np.int32)

    def index(self, table, item, comp=0):
        return {"size": 0, "pos": 3 * self.ng, "friction": 6 * self.ng}[table] + 3 * item + comp if table != "mass" else 9 * self.ng + item

    def new_draw(self):
        if self.ndraw >= MAX_DRAWS:
            raise ValueError(f"at most {MAX_DRAWS} shared draws")
        self.ndraw += 1
        return self.ndraw - 1

    def set(self, table, item, comp, lo, hi, draw=DRAW_OWN):
        """parameter ~ lo + (hi - lo) * u"""
        p = self.index(table, item, comp)
        self.base[p], self.scale[p], self.draw[p] = lo, hi - lo, draw

    def values(self, u_shared, u_own, current):
        """The row a reset writes, in float32 as the kernel computes it (one rounding of base + scale * u): `u_shared[k]` the shared draws,
        `u_own[p]` the parameters' own, `current` the row before the reset (kept where scale is 0)."""
        base, scale = self.base.astype(np.float32).astype(np.float64), self.scale.astype(np.float32).astype(np.float64)
        u = np.where(self.draw >= 0, np.asarray(u_shared, np.float64)[np.maximum(self.draw, 0)] if self.ndraw else 0.0, np.asarray(u_own, np.float64))
        return np.where(scale != 0, (base + scale * u).astype(np.float32), np.asarray(current, np.float32)).astype(np.float32)


_DRAW_KEY = 0x7A5662DCDF6B1F6D
_EPISODE_KEY = 0x632BE59BD9B4E019
_M64 = (1 << 64) - 1


def draw_u(seed, episode, global_env, table: DrawTable):
    """Host twin of the reset kernel's draws for one env: (u_shared [MAX_DRAWS], u_own [n]) of the env with global id `global_env` at the
    reset that starts its episode number `episode` (0 for the first reset of the batch) under reset seed `seed`."""
    s = ((seed + _EPISODE_KEY * episode) & _M64) ^ _DRAW_KEY
    n = 9 * table.ng + table.nb
    shared = np.array([u01(s, global_env * 1024 + k, 12) for k in range(MAX_DRAWS)])
    own = np.array([u01(s, global_env * 1024 + MAX_DRAWS + p, 12) for p in range(n)])
    return shared, own


def predict_rows(seed, episode, global_envs, table: DrawTable, current):
    """[len(global_envs), n] float32 rows (size | pos | friction | mass) the reset writes, from the host twin of the draws."""
    current = np.broadcast_to(np.asarray(current, np.float32), (len(global_envs), 9 * table.ng + table.nb))
    return np.stack([table.values(*draw_u(seed, episode, int(e), table), current[i]) for i, e in enumerate(global_envs)])


def _pair(name, v):
    lo, hi = (float(x) for x in v)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo < 0 or hi < lo:
        raise ValueError(f"{name} must be (lo, hi) with 0 <= lo <= hi, got {v!r}")
    return lo, hi


def _change(name, v, nominal):
    c = np.broadcast_to(np.asarray(v, np.float64), (3,)).copy()
    if not np.isfinite(c).all() or (c < 0).any():
        raise ValueError(f"{name} must be >= 0 per component, got {v!r}")
    if (np.asarray(nominal) - c < 0).any():
        raise ValueError(f"{name} = {v!r} reaches below zero friction (nominal {np.asarray(nominal).tolist()})")
    return c


def baoding_draws(size0, pos0, friction0, mass0, obj_size_range=None, obj_mass_range=None, obj_friction_change=None):
    """BaodingEnvV1.reset (baoding_v1.py:115-135, 360-385) as a draw table over (ball1, ball2): mass ~ U(obj_mass_range) per ball;
    friction ~ U(nominal -+ obj_friction_change) per ball and component, the nominal being ball1's (as the reference builds its range);
    size ~ U(obj_size_range), one draw per ball written to all three components (numpy's scalar assignment to a row).  None: not re-drawn.
    Raises ValueError on a bad range before anything else happens."""
    t = DrawTable(2, 2)
    if obj_mass_range is not None:
        lo, hi = _pair("obj_mass_range", obj_mass_range)
        for b in range(2):
            t.set("mass", b, 0, lo, hi)
    if obj_friction_change is not None:
        c = _change("obj_friction_change", obj_friction_change, friction0[0])
        for b in range(2):
            for k in range(3):
                t.set("friction", b, k, friction0[0][k] - c[k], friction0[0][k] + c[k])
    if obj_size_range is not None:
        lo, hi = _pair("obj_size_range", obj_size_range)
        for b in range(2):
            d = t.new_draw()
            for k in range(3):
                t.set("size", b, k, lo, hi, d)
    return t


def die_draws(types, size0, pos0, friction0, mass0, obj_size_change=None, obj_mass_range=None, obj_friction_change=None):
    """ReorientEnvV0.reset (reorient_v0.py:94-101, 221-247) as a draw table over the die's 15 geoms (12 capsules, then 3 boxes) and its
    body: friction ~ U(nominal -+ obj_friction_change) per geom and component; mass ~ U(obj_mass_range); one del_size ~
    U(-obj_size_change, obj_size_change) drives the capsules' half lengths (size[1]), all three sizes of the boxes, and every geom position
    component, pos = sign(pos0) * (|pos0| + del_size) (a zero component stays zero).  The die's visual `target_dice` geom, which the
    reference resizes too, collides with nothing and is not modelled.  None: not re-drawn.  Raises ValueError on a bad value."""
    from .mjcf import GEOM_BOX, GEOM_CAPSULE
    ng = len(types)
    t = DrawTable(ng, 1)
    if obj_mass_range is not None:
        t.set("mass", 0, 0, *_pair("obj_mass_range", obj_mass_range))
    if obj_friction_change is not None:
        for g in range(ng):
            c = _change("obj_friction_change", obj_friction_change, friction0[g])
            for k in range(3):
                t.set("friction", g, k, friction0[g][k] - c[k], friction0[g][k] + c[k])
    if obj_size_change is not None:
        ch = float(obj_size_change)
        if not np.isfinite(ch) or ch < 0:
            raise ValueError(f"obj_size_change must be >= 0, got {obj_size_change!r}")
        d = t.new_draw()
        for g in range(ng):
            comps = (1,) if types[g] == GEOM_CAPSULE else ((0, 1, 2) if types[g] == GEOM_BOX else ())
            for k in comps:
                if size0[g][k] - ch < 0:
                    raise ValueError(f"obj_size_change = {ch} makes a size of the die negative")
                t.set("size", g, k, size0[g][k] - ch, size0[g][k] + ch, d)
            for k in range(3):
                sg = np.sign(pos0[g][k])
                if sg != 0:
                    if abs(pos0[g][k]) - ch <= 0:
                        raise ValueError(f"obj_size_change = {ch} moves a geom of the die across its centre")
                    t.set("pos", g, k, pos0[g][k] - sg * ch, pos0[g][k] + sg * ch, d)
    return t


def resolve_ids(mjmodel, geoms, bodies):
    """(geom ids, body ids) of a selection given by names or ids."""
    return ([mjmodel.geom_name2id(g) if isinstance(g, str) else int(g) for g in geoms],
            [mjmodel.body_name2id(b) if isinstance(b, str) else int(b) for b in bodies])


# ---- the env-side record ---------------------------------------------------------------------------------------------------------
class ObjectParams:
    """The per-env object parameters of a batch: `geom_names`, `body_names` (the selection, model names or ids), and the four tables
    `size` / `pos` / `friction` [B, ng, 3] and `mass` [B, nb].  With torch they are zero-copy views of the library's device memory: writable,
    and a write takes effect at the next step / forward.  Without (as_torch=False) every read is a fresh numpy copy and an assignment
    (`p.size = a`, one row broadcast or [B, ...]) goes through the library's validated host write."""

    def __init__(self, batch, mjmodel, geoms, bodies, torch=None, device=0):
        self._batch, self._torch, self._device = batch, torch, device
        name_of = lambda kind, i: (mjmodel.names[kind][i] or i) if 0 <= i < len(mjmodel.names[kind]) else i     # (a bad id is the library's to refuse)
        self.geom_ids, self.body_ids = resolve_ids(mjmodel, geoms, bodies)
        self.geom_names = [name_of("geom", g) for g in self.geom_ids]
        self.body_names = [name_of("body", b) for b in self.body_ids]
        (ga, gp), (ba, bp) = _ids(self.geom_ids), _ids(self.body_ids)
        capi._chk(lib().myo_objects_enable(batch.h, gp, ga.size, bp, ba.size))
        self.ng, self.nb = ga.size, ba.size
        self._views = {}

    def _shape(self, which):
        return (self._batch.B, self.nb) if which == OBJ_MASS else (self._batch.B, self.ng, 3)

    def table_ptr(self, which):
        return capi.buffer_lookup(lib().myo_objects_table, self._batch.h, int(which))

    def read(self, which):
        return capi.host_read(lib().myo_objects_read, self._batch.h, int(which), shape=self._shape(which), dtype=np.float32)

    def write(self, which, value):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(value, np.float32), self._shape(which)))
        capi._chk(lib().myo_objects_write(self._batch.h, int(which), a.ctypes.data, a.nbytes))

    def _get(self, which):
        if self._torch is None:
            return self.read(which)
        if which not in self._views:
            self._views[which] = capi.device_view(self._torch, self.table_ptr(which)[0], self._shape(which), np.float32, self._batch, self._device)
        return self._views[which]

    def _set(self, which, value):
        if self._torch is None:
            self.write(which, value)
        else:
            v = self._get(which)
            v.copy_(self._torch.as_tensor(value, dtype=self._torch.float32, device=v.device).expand(*v.shape))

    size = property(lambda s: s._get(OBJ_SIZE), lambda s, v: s._set(OBJ_SIZE, v), doc="[B, ng, 3] geom_size of the selected geoms")
    pos = property(lambda s: s._get(OBJ_POS), lambda s, v: s._set(OBJ_POS, v), doc="[B, ng, 3] geom_pos of the selected geoms (body frame)")
    friction = property(lambda s: s._get(OBJ_FRICTION), lambda s, v: s._set(OBJ_FRICTION, v), doc="[B, ng, 3] geom_friction of the selected geoms")
    mass = property(lambda s: s._get(OBJ_MASS), lambda s, v: s._set(OBJ_MASS, v), doc="[B, nb] body_mass of the selected bodies")

    def rows(self):
        """[B, 9 ng + nb] host copy of all parameters in the draw table's order."""
        B = self._batch.B
        parts = [self.read(w).reshape(B, -1) for w in (OBJ_SIZE, OBJ_POS, OBJ_FRICTION)] if self.ng else []
        if self.nb:
            parts.append(self.read(OBJ_MASS))
        return np.concatenate(parts, axis=1)

    def set_draws(self, table: DrawTable | None):
        """Install (None: remove) the draw table of the batch's resets."""
        if table is None:
            capi._chk(lib().myo_objects_set_draws(self._batch.h, 0, 0, None, None, None))
            return
        assert (table.ng, table.nb) == (self.ng, self.nb)
        base, scale, draw = np.ascontiguousarray(table.base, np.float32), np.ascontiguousarray(table.scale, np.float32), np.ascontiguousarray(table.draw, np.int32)
        capi._chk(lib().myo_objects_set_draws(self._batch.h, table.ndraw, base.size, base.ctypes.data_as(_pF), scale.ctypes.data_as(_pF), draw.ctypes.data_as(_pI)))


def task_objects(mjmodel, task):
    """(geom ids, body ids) of the task's objects: baoding -- the geoms and bodies of ball1 and ball2; die -- the 15 geoms and the body of
    `Object`; None for a task without a default selection."""
    if task == "baoding":
        return [mjmodel.geom_name2id("ball1"), mjmodel.geom_name2id("ball2")], [mjmodel.body_name2id("ball1"), mjmodel.body_name2id("ball2")]
    if task == "die":
        ob = mjmodel.body_name2id("Object")
        return [g for g in range(mjmodel.ngeom) if int(mjmodel.geom_bodyid[g]) == ob], [ob]
    return None


def task_draws(mjmodel, task, geom_ids, body_ids, **kw):
    """The draw table of `set_object_randomization(**kw)` for the baoding / die task, with the reference's kwarg names and meaning."""
    names = {"baoding": ("obj_size_range", "obj_mass_range", "obj_friction_change"), "die": ("obj_size_change", "obj_mass_range", "obj_friction_change")}
    if task not in names:
        raise NotImplementedError("set_object_randomization: the baoding and die tasks only (other tasks: ObjectParams.set_draws with a DrawTable)")
    bad = sorted(set(kw) - set(names[task]))
    if bad:
        raise TypeError(f"set_object_randomization: unknown argument(s) {bad} for the {task} task; it takes {names[task]}")
    size0, pos0, fr0 = (np.asarray(mjmodel.arrays[k], np.float64)[geom_ids] for k in ("geom_size", "geom_pos", "geom_friction"))
    mass0 = np.asarray(mjmodel.body_mass, np.float64)[body_ids]
    if task == "baoding":
        return baoding_draws(size0, pos0, fr0, mass0, **kw)
    return die_draws([int(mjmodel.geom_type[g]) for g in geom_ids], size0, pos0, fr0, mass0, **kw)
