#!/usr/bin/env python3
"""Record what the host library answers for the four buffer families next to the batch fields -- the reward-term row, the episode buffers,
the forward buffers and the per-env object tables -- and for myo_status, on a GPU (tests/test_gpu_buffer_responses.py,
tests/golden/buffer_responses.json.gz).

    python tools/record_buffer_responses.py tests/golden/buffer_responses.json.gz

Raw calls on `capi.lib()` / `objects.lib()` with the handles `HipModel.h` / `HipBatch.h` only: none of the binding's lookup, read, write or
view methods, so the script runs unchanged before and after a change of either side.  B = 3 envs, so a wrong row stride shows.  The parts:

  rewards   myolegs with the walk task configured: the row and the episode buffers before myo_batch_enable_rewards, the statistics
            before the rewards (refused), then ids -1 .. 4 with pitch and width, reads of the right size, one element short, and
            MYO_EP_FINISHED with 4 * B bytes; the bytes after myo_episode_clear and of the row before any step (zeros).
  forward_<model>   myoelbow_1dof6muscles (no site_quat) and myolegs (has it): ids -1 .. MYO_FWD_COUNT before the first myo_forward and
            after it, a right-size and a short read of each.  A forward read's bytes are kernel arithmetic and are not stored.
  objects   myohand_baoding: everything before myo_objects_enable; ball1 / ball2 enabled, ids -1 .. 4, the compiled values; the refused
            writes (NaN, negative size, negative mass, one float short), an accepted negative position, an accepted write of each
            table read back; a second batch with geoms only: the mass table's refusal.
  status    myo_status of a fresh batch.

Every part also passes a null handle, null out-arguments and a null host pointer to each entry point once.  A call is stored as
[kind, family, id, ...]: a lookup with return code, the myo_last_error text of a failed call, pitch, width and whether a pointer came
back; a read with its byte count, code, text and the bytes (hex) where the host decides them; a write with the bytes it passed.  No step
runs anywhere in the script.  The golden file is written from the commit BEFORE a change of the host library and compared for equality
after it."""
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 3
FORWARD_MODELS = ("myoelbow_1dof6muscles", "myolegs")
PARTS = ("rewards",) + tuple(f"forward_{m}" for m in FORWARD_MODELS) + ("objects", "status")
# family -> (ids asked: one below to one above the range; None: the family has one buffer)
EP_IDS, FWD_IDS, OBJ_IDS = range(-1, 5), range(-1, 10), range(-1, 5)


class Script:
    """One batch, the raw entry points of the four families and the log of what the library answered."""

    def __init__(self, hm, log, batch=None):
        from myosuite_mjx_amd import capi, objects
        self.capi, self.L, self.log = capi, objects.lib(), log
        self.b = batch if batch is not None else capi.HipBatch(hm, B)
        L = self.L
        self.lookup_fn = {"rwd": lambda h, i, *o: L.myo_batch_rwd_row(h, *o), "episode": L.myo_batch_episode_buffer,
                          "forward": L.myo_forward_buffer, "objects": L.myo_objects_table}
        self.read_fn = {"rwd": lambda h, i, *a: L.myo_batch_rwd_read(h, *a), "episode": L.myo_batch_episode_read,
                        "forward": L.myo_forward_read, "objects": L.myo_objects_read}

    def _err(self, rc):
        return self.L.myo_last_error().decode() if rc else ""

    def lookup(self, family, i=0, null=None):
        """null: "handle" or "out" passes a null batch or null out-arguments."""
        p, pitch, width = C.c_void_p(), C.c_size_t(), C.c_size_t()
        out = (None, None, None) if null == "out" else (C.byref(p), C.byref(pitch), C.byref(width))
        rc = self.lookup_fn[family](None if null == "handle" else self.b.h, i, *out)
        self.log.append(["lookup", family, i, null, rc, self._err(rc), pitch.value, width.value, bool(p.value)])
        return rc, width.value

    def read(self, family, i, nbytes, keep=True, null=None):
        """keep=False: the bytes are a kernel's arithmetic and are not stored."""
        buf = np.zeros(max(nbytes, 4), np.uint8)
        rc = self.read_fn[family](None if null == "handle" else self.b.h, i, None if null == "host" else buf.ctypes.data, nbytes)
        self.log.append(["read", family, i, null, nbytes, rc, self._err(rc), buf[:nbytes].tobytes().hex() if rc == 0 and keep else None])
        return buf[:nbytes]

    def write(self, i, values, short=0, null=None):
        a = np.ascontiguousarray(values, np.float32).ravel()
        a = a[:a.size - short].copy()
        rc = self.L.myo_objects_write(None if null == "handle" else self.b.h, i, None if null == "host" else a.ctypes.data, a.nbytes)
        self.log.append(["write", "objects", i, null, a.tobytes().hex(), rc, self._err(rc)])

    def call(self, name, *args):
        rc = getattr(self.L, name)(self.b.h, *args)
        self.log.append(["call", name, [a for a in args if isinstance(a, (int, type(None)))], rc, self._err(rc)])
        return rc

    def nulls(self, family, i=0):
        for null in ("handle", "out"):
            self.lookup(family, i, null)
        for null in ("handle", "host"):
            self.read(family, i, 4 * B, null=null)

    def every_id(self, family, ids, item_bytes=lambda i: 4, keep=True):
        """Lookup of every id, then a read of the right size and one an element short (4 * B bytes where the lookup fails)."""
        for i in ids:
            rc, width = self.lookup(family, i)
            n = 4 * B if rc else B * width * item_bytes(i)
            self.read(family, i, n, keep)
            if n >= item_bytes(i):
                self.read(family, i, n - item_bytes(i), keep)


def record_rewards():
    from myosuite_mjx_amd import capi, envs, model as M, tasks
    log = []
    m = M.load_asset("myolegs")
    hm = capi.HipModel(m.blob(), 0)
    s = Script(hm, log)
    s.b.configure_walk(**tasks.TASKS["walk"].setup(m, dict(envs.REGISTRY["myoLegWalk-v0"]), "myoLegWalk-v0").kwargs)
    ncol = s.L.myo_batch_rwd_ncol(s.b.h)
    log.append(["ncol", ncol])
    ep_bytes = lambda i: 1 if i == capi.EP_FINISHED else 4
    s.every_id("rwd", [0])
    s.every_id("episode", EP_IDS, ep_bytes)
    s.call("myo_batch_enable_episode_stats")                                   # before the rewards: refused
    w = np.ones(ncol - 1, np.float32)
    s.call("myo_batch_enable_rewards", w.ctypes.data_as(C.POINTER(C.c_float)), ncol - 2, capi.RWD_DENSE)   # one weight short: refused
    s.call("myo_batch_enable_rewards", w.ctypes.data_as(C.POINTER(C.c_float)), ncol - 1, capi.RWD_DENSE)
    s.every_id("rwd", [0])                                                     # before any step: zeros
    s.nulls("rwd")
    s.every_id("episode", EP_IDS, ep_bytes)                                    # the rewards alone do not enable the statistics
    s.call("myo_batch_enable_episode_stats")
    s.call("myo_batch_enable_episode_stats")                                   # a second call changes nothing
    s.call("myo_episode_clear", None)
    log.append(["sync", s.L.myo_sync(None)])
    s.every_id("episode", EP_IDS, ep_bytes)
    s.read("episode", capi.EP_FINISHED, 4 * B)                                 # a byte per env, not a word: refused
    s.nulls("episode", capi.EP_COUNT)
    return log


def record_forward(name):
    from myosuite_mjx_amd import capi, model as M
    log = []
    hm = capi.HipModel(M.load_asset(name).blob(), 0)
    s = Script(hm, log)
    s.every_id("forward", FWD_IDS, keep=False)
    s.call("myo_forward", None)
    log.append(["sync", s.L.myo_sync(None)])
    s.every_id("forward", FWD_IDS, keep=False)
    s.nulls("forward", capi.FWD_XPOS)
    return log


def record_objects():
    from myosuite_mjx_amd import capi, model as M, objects
    log = []
    m = M.load_asset("myohand_baoding")
    hm = capi.HipModel(m.blob(), 0)
    geoms = np.array([m.geom_name2id("ball1"), m.geom_name2id("ball2")], np.int32)
    bodies = np.array([m.body_name2id("ball1"), m.body_name2id("ball2")], np.int32)
    pI = C.POINTER(C.c_int)
    s = Script(hm, log)
    s.every_id("objects", OBJ_IDS)
    for i in OBJ_IDS:
        s.write(i, np.ones(B, np.float32))
    s.call("myo_objects_enable", geoms.ctypes.data_as(pI), 2, bodies.ctypes.data_as(pI), 2)
    s.every_id("objects", OBJ_IDS)                                             # the compiled values
    s.nulls("objects", objects.OBJ_SIZE)
    for null in ("handle", "host"):
        s.write(objects.OBJ_SIZE, np.ones(B * 6, np.float32), null=null)
    rows = {i: s.read("objects", i, B * (2 if i == objects.OBJ_MASS else 6) * 4).view(np.float32).copy() for i in range(4)}

    def poke(i, k, v):
        a = rows[i].copy()
        a[k] = v
        return a
    s.write(objects.OBJ_SIZE, poke(objects.OBJ_SIZE, 7, np.nan))               # refused: NaN (env 1), negative size, negative mass, one float short
    s.write(objects.OBJ_SIZE, poke(objects.OBJ_SIZE, 13, -0.01))
    s.write(objects.OBJ_FRICTION, poke(objects.OBJ_FRICTION, 2, np.inf))
    s.write(objects.OBJ_MASS, poke(objects.OBJ_MASS, 5, -0.5))
    for i in range(4):
        s.write(i, rows[i], short=1)
    s.write(-1, rows[0])
    s.write(4, rows[0])
    for i in range(4):                                                         # nothing of the refused writes arrived
        s.read("objects", i, rows[i].nbytes)
    s.write(objects.OBJ_POS, poke(objects.OBJ_POS, 8, -0.02))                  # accepted: a negative position
    s.read("objects", objects.OBJ_POS, rows[objects.OBJ_POS].nbytes)
    for i in range(4):                                                         # accepted: every table, another value per env, read back
        a = (rows[i].reshape(B, -1) * np.array([[1.0], [1.25], [1.5]], np.float32)).astype(np.float32)
        s.write(i, a)
        for j in range(4):
            s.read("objects", j, rows[j].nbytes)
    s2 = Script(hm, log)                                                       # geoms only: no mass table
    s2.call("myo_objects_enable", geoms.ctypes.data_as(pI), 2, None, 0)
    s2.every_id("objects", OBJ_IDS)
    s2.write(objects.OBJ_MASS, np.ones(B * 2, np.float32))
    return log


def record_status():
    from myosuite_mjx_amd import capi, model as M
    log = []
    hm = capi.HipModel(M.load_asset("myoelbow_1dof6muscles").blob(), 0)
    s = Script(hm, log)
    for handle, host in ((s.b.h, True), (None, True), (s.b.h, False)):
        out = np.full(B, -1, np.int32)
        rc = s.L.myo_status(handle, out.ctypes.data if host else None)
        log.append(["status", bool(handle), host, rc, s._err(rc), out.tobytes().hex()])
    return log


def record_part(name):
    if name.startswith("forward_"):
        return record_forward(name[len("forward_"):])
    return {"rewards": record_rewards, "objects": record_objects, "status": record_status}[name]()


def record():
    return {name: record_part(name) for name in PARTS}


def main():
    rec = record()
    text = json.dumps(rec, sort_keys=True, separators=(",", ":")) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:      # (no time stamp: same record, same file)
        g.write(text.encode())
    print(f"{len(rec)} parts, {sum(len(calls) for calls in rec.values())} calls -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
