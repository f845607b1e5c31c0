#!/usr/bin/env python3
"""Record what the batch half of the host library answers to one scripted sequence of calls, on a GPU (tests/test_gpu_batch_fields.py,
tests/golden/batch_field_responses.json.gz).

    python tools/record_batch_fields.py tests/golden/batch_field_responses.json.gz

Four models, one per code path of the per-env fields: myoelbow_1dof6muscles (hand class: body masses), myohand_keyturn (TrackEnv class:
root-body offset), myohand_pen (TrackEnv class: body orientation through quat_body), myolegs (leg class: body masses, touch sensors).
Each gets B = 3 envs, so a wrong `e * width` stride or a missing per-env broadcast shows, and the same script:

  batch 1  fresh: myo_batch_field (not for the override fields, whose pointer request would start them) and myo_batch_read of every id
           -1 .. MYO_F_CFRC + 1, short buffers; the rejected writes (negative mass, lo > hi, NaN, norm 1.1, one float short, read-only
           fields, absent fields) and the override rows again; one step: nothing has started.  configure(quat_body=...) and the
           orientation fields; the accepted writes, each read back; a second quat_body after the first has started; myo_batch_field
           of every id, with a read of the override fields and of the ids whose lookup fails.
  batch 2  the model's own override started through the pointer request alone; one step: the run-time-sizes kernel of its class.
  batch 3  myo_batch_enable_sensors, the sensor fields' widths, reads and writes, one step.

Every library call is stored as its name, arguments, return code, the myo_last_error text of a failed call, the width (and pitch, and
whether a pointer came back) it reported and the bytes of every array it read; a step as the kernel name and the status flags after it.
After a batch's first step only the override fields, which no kernel of a step writes, and rows the script has just written itself
(MYO_F_ELAPSED, MYO_F_TIME) are read, so the record holds host logic and no physics; tests/test_gpu_batch_fields.py checks that of the fixture.
The golden file is written from the commit BEFORE a change of the host library and compared for equality after it."""
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODELS = ("myoelbow_1dof6muscles", "myohand_keyturn", "myohand_pen", "myolegs")
# myo_task_config.quat_body: the body to select and a second one (names, or ids: 0 selects nothing, 1 is refused outside the TrackEnv class)
QUAT_BODY = {"myoelbow_1dof6muscles": (1, 1), "myohand_keyturn": (0, 0), "myohand_pen": ("target", "full_body"), "myolegs": (1, 1)}
OWN = {"myoelbow_1dof6muscles": "F_BODYMASS", "myohand_keyturn": "F_BODYPOS", "myohand_pen": "F_BODYQUAT", "myolegs": "F_BODYMASS"}
B = 3


class Script:
    """One batch and the log of what the library answered."""

    def __init__(self, hm, m, log):
        from myosuite_mjx_amd import capi
        self.capi, self.L, self.m, self.log = capi, capi.lib(), m, log
        self.b = capi.HipBatch(hm, B)
        nb = m.nbody
        self.override = {capi.F_BODYMASS: nb, capi.F_BODYMASS_RANGE: 2 * nb, capi.F_BODYPOS: 3, capi.F_BODYPOS_RANGE: 6,
                         capi.F_BODYQUAT: 4, capi.F_BODYQUAT_RANGE: 6}

    def _err(self, rc):
        return self.L.myo_last_error().decode() if rc else ""

    def field(self, f):
        p, pitch, width = C.c_void_p(), C.c_size_t(), C.c_size_t()
        rc = self.L.myo_batch_field(self.b.h, f, C.byref(p), C.byref(pitch), C.byref(width))
        self.log.append(["field", f, rc, self._err(rc), pitch.value, width.value, bool(p.value)])
        return rc, width.value

    def read(self, f, width, short=0):
        out = np.zeros(B * width - short, np.int32 if f in self.capi.INT_FIELDS else np.float32)
        rc = self.L.myo_batch_read(self.b.h, f, out.ctypes.data, out.nbytes)
        self.log.append(["read", f, out.nbytes, rc, self._err(rc), out.tobytes().hex() if rc == 0 else None])

    def write(self, f, rows, short=0):
        a = np.ascontiguousarray(rows, np.int32 if f in self.capi.INT_FIELDS else np.float32).ravel()
        a = a[:a.size - short].copy()
        rc = self.L.myo_batch_write(self.b.h, f, a.ctypes.data, a.nbytes)
        self.log.append(["write", f, a.tobytes().hex(), rc, self._err(rc)])
        return rc

    def configure(self, quat_body):
        try:
            self.b.configure(quat_body=quat_body)
            self.log.append(["configure", quat_body, ""])
        except self.capi.MyoError as ex:
            self.log.append(["configure", quat_body, str(ex)])

    def enable_sensors(self):
        rc = self.L.myo_batch_enable_sensors(self.b.h)
        self.log.append(["enable_sensors", rc, self._err(rc)])
        return rc

    def step(self):
        try:
            self.b.step(None, self.capi.ACTMAP_NONE, 1)
            self.log.append(["step", "", self.b.last_kernel_name(), self.b.status().tolist()])
        except self.capi.MyoError as ex:
            self.log.append(["step", str(ex), None, None])

    def every_id(self, fresh):
        """Fresh batch: field + read of every id, an override field read at its documented width without asking for its pointer, which
        would start it.  Later (a step has run): field of every id, and a read where it returns no state a step wrote -- the override
        fields and the ids whose lookup fails."""
        for f in range(-1, self.capi.F_CFRC + 2):
            rc, width = (0, self.override[f]) if fresh and f in self.override else self.field(f)
            if fresh or rc or f in self.override:
                self.read(f, self.override.get(f, 1) if rc else width)

    def read_overrides(self):
        for f, width in self.override.items():
            self.read(f, width)


def rows(width, *per_env):
    """[B, width] float32: row e = per_env[e] broadcast over the row."""
    return np.stack([np.broadcast_to(np.asarray(r, np.float32), (width,)) for r in per_env]).astype(np.float32)


def poke(a, e, i, v):
    a = np.array(a, np.float32).reshape(B, -1)
    a[e, i] = v
    return a


def rejected_writes(s):
    c, m, nb = s.capi, s.m, s.m.nbody
    mass = np.tile(np.asarray(m.body_mass, np.float32), (B, 1))
    mrange = np.concatenate([0.5 * mass, 1.5 * mass], axis=1)
    s.write(c.F_BODYMASS, poke(mass, 1, nb - 1, -0.25))                       # a negative mass, in env 1
    s.write(c.F_BODYMASS, poke(mass, 2, 0, np.nan))
    s.write(c.F_BODYMASS, mass, short=1)
    s.write(c.F_BODYMASS_RANGE, poke(poke(mrange, 2, 1, 1.0), 2, nb + 1, 0.5))   # hi < lo in env 2, body 1
    s.write(c.F_BODYMASS_RANGE, poke(mrange, 1, 0, -1.0))                     # lo < 0
    s.write(c.F_BODYMASS_RANGE, poke(mrange, 0, 2 * nb - 1, np.nan))
    s.write(c.F_BODYMASS_RANGE, mrange, short=1)
    off = rows(3, [0.001, 0.0, 0.002], [0.002, 0.0, 0.002], [0.003, 0.0, 0.002])
    box = np.concatenate([off - 0.001, off + 0.001], axis=1)
    for rng in (c.F_BODYPOS_RANGE, c.F_BODYQUAT_RANGE):
        s.write(rng, poke(box, 1, 4, -1.0))                                   # hi < lo in env 1, component 1
        s.write(rng, poke(box, 2, 0, np.nan))
        s.write(rng, poke(box, 0, 5, np.inf))
        s.write(rng, box, short=1)
    s.write(c.F_BODYPOS, poke(off, 2, 1, np.nan))
    s.write(c.F_BODYPOS, off, short=1)
    quat = rows(4, [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0])
    s.write(c.F_BODYQUAT, poke(quat, 1, 0, 1.1))                              # norm 1.1
    s.write(c.F_BODYQUAT, poke(quat, 2, 3, np.nan))
    s.write(c.F_BODYQUAT, quat, short=1)
    for f in (c.F_SENSORDATA, c.F_CFRC, c.F_LINKX, c.F_GEOMSIZE, c.F_HFIELD, c.F_METRICS, -1, c.F_CFRC + 1):
        s.write(f, np.zeros(B, np.float32))                                   # read-only, absent or unknown
    s.write(c.F_QPOS, np.zeros((B, m.nq)), short=1)
    s.write(c.F_ELAPSED, np.zeros(B + 1))


def accepted_writes(s):
    c, m = s.capi, s.m
    mass = np.asarray(m.body_mass, np.float32)[None, :] * np.array([[1.0], [1.25], [1.5]], np.float32)
    off = rows(3, [0.001, 0.0, 0.002], [0.002, 0.0, 0.002], [0.003, 0.0, 0.002])
    ang = np.array([0.1, 0.2, 0.3], np.float32)
    quat = np.stack([np.cos(ang / 2), 0 * ang, 0 * ang, np.sin(ang / 2)], axis=1).astype(np.float32)
    eul = rows(3, [0.0, 0.1, 0.2], [0.1, 0.2, 0.3], [0.2, 0.3, 0.4])
    for f, a in ((c.F_BODYMASS, mass), (c.F_BODYMASS_RANGE, np.concatenate([0.5 * mass, 1.5 * mass], axis=1)),
                 (c.F_BODYPOS_RANGE, np.concatenate([off - 0.001, off + 0.001], axis=1)), (c.F_BODYPOS, off),
                 (c.F_BODYQUAT, quat), (c.F_BODYQUAT_RANGE, np.concatenate([-eul, eul], axis=1))):
        s.write(f, a)
        s.read_overrides()                                                    # the written rows, and what the start filled in beside them
    s.write(c.F_ELAPSED, np.arange(B) + 5)
    s.read(c.F_ELAPSED, 1)
    s.write(c.F_TIME, np.arange(B) * 0.5)
    s.read(c.F_TIME, 1)


def record_model(name):
    from myosuite_mjx_amd import capi, model as M
    m = M.load_asset(name)
    hm = capi.HipModel(m.blob(), 0)
    first, second = (m.name2id("body", n) if isinstance(n, str) else n for n in QUAT_BODY[name])
    out = {}
    # batch 1
    s = Script(hm, m, out.setdefault("overrides", []))
    s.every_id(fresh=True)
    s.read(capi.F_QPOS, m.nq, short=1)
    s.read(capi.F_BODYMASS, m.nbody, short=1)
    s.read(capi.F_BODYPOS, 3, short=1)
    s.read(capi.F_BODYQUAT_RANGE, 6, short=1)
    rejected_writes(s)
    s.read_overrides()
    s.step()
    s.configure(first)
    s.read_overrides()
    rejected_writes(s)
    s.read_overrides()
    accepted_writes(s)
    s.configure(second)
    s.configure(first)
    s.every_id(fresh=False)
    # batch 2
    s = Script(hm, m, out.setdefault("pointer_start", []))
    s.configure(first)
    own = getattr(capi, OWN[name])
    s.field(own + 1)                                                          # the range field's pointer starts the override as well
    s.field(own)
    s.read_overrides()
    s.step()
    # batch 3
    s = Script(hm, m, out.setdefault("sensors", []))
    for f in (capi.F_SENSORDATA, capi.F_CFRC):
        s.field(f)
        s.read(f, 1)
    if s.enable_sensors() == 0:
        s.enable_sensors()                                                    # a second call changes nothing
    for f in (capi.F_SENSORDATA, capi.F_CFRC):
        rc, width = s.field(f)
        width = 1 if rc else width
        s.read(f, width)
        s.read(f, width, short=1)
        s.write(f, np.zeros(B * width, np.float32))
    s.step()
    return out


def record():
    return {name: record_model(name) for name in MODELS}


def main():
    rec = record()
    text = json.dumps(rec, sort_keys=True, separators=(",", ":")) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:      # (no time stamp: same record, same file)
        g.write(text.encode())
    n = sum(len(calls) for r in rec.values() for calls in r.values())
    print(f"{len(rec)} models, {n} calls -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
