"""The device-buffer families next to the batch fields -- reward-term row, episode buffers, forward buffers, per-env object tables -- and
myo_status, on both sides of the ABI.

The library against a recorded fixture: tools/record_buffer_responses.py runs one scripted sequence of raw calls with B = 3 envs (module
docstring there) and tests/golden/buffer_responses.json.gz holds what the library answered at the commit before the families' lookup, copy
and size-check code became one set of helpers (2d49a87), so the fixture is not a product of the code under test.  Equality is exact: return
code, error text, pitch and width, whether a pointer came back, and the bytes of every read whose bytes the host decides.  No step runs in the
script and a forward read's bytes are not stored, so no kernel arithmetic is compared (test_the_fixture_holds_the_cases checks that).

The binding: every family's accessor gives, with torch, a cached zero-copy view at the looked-up pointer in the family table's shape and
dtype after exactly one lookup, and without torch a host array of the same shape, dtype and bytes."""
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARTS = ("rewards", "forward_myoelbow_1dof6muscles", "forward_myolegs", "objects", "status")
B = 3


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "buffer_responses.json.gz"), "rt") as f:
        return json.load(f)


def test_the_fixture_holds_the_cases(golden):
    import record_buffer_responses as rec
    assert rec.PARTS == PARTS and sorted(golden) == sorted(PARTS) and rec.B == B
    calls = [c for part in PARTS for c in golden[part]]
    kinds = {c[0] for c in calls}
    assert kinds == {"lookup", "read", "write", "call", "sync", "ncol", "status"}                 # nothing that steps
    assert {c[1] for c in calls if c[0] == "call"} == {"myo_batch_enable_episode_stats", "myo_batch_enable_rewards", "myo_episode_clear",
                                                       "myo_forward", "myo_objects_enable"}
    lookups = [c for c in calls if c[0] == "lookup" and c[3] is None]                             # [kind, family, id, null, rc, err, pitch, width, ptr]
    reads = [c for c in calls if c[0] == "read" and c[3] is None]                                 # [kind, family, id, null, nbytes, rc, err, hex]
    writes = [c for c in calls if c[0] == "write" and c[3] is None]                               # [kind, family, id, null, hex, rc, err]
    for family, ids in (("episode", range(-1, 5)), ("forward", range(-1, 10)), ("objects", range(-1, 5))):
        for kind in (lookups, reads):                                                             # every id, one below and one above the range
            assert {c[2] for c in kind if c[1] == family} == set(ids), family
    for family in ("rwd", "episode", "forward", "objects"):
        mine = [c for c in reads if c[1] == family]
        assert any(c[5] == 0 for c in mine) and any(c[5] != 0 for c in mine), family              # an accepted and a refused read
        ok = [c for c in lookups if c[1] == family and c[4] == 0]
        assert ok and all(c[6] == c[7] > 0 and c[8] for c in ok), family                          # pitch = width, a pointer came back
        assert {c[3] for c in calls if c[0] in ("lookup", "read") and c[1] == family} == {None, "handle", "out", "host"}
    for i in range(4):                                                                            # every object table: a refused and an accepted write
        assert any(c[2] == i and c[5] == 0 for c in writes) and any(c[2] == i and c[5] != 0 for c in writes), i
    assert all(c[7] is None for c in reads if c[1] == "forward")                                  # kernel arithmetic is not stored
    assert all((c[7] is not None) == (c[5] == 0) for c in reads if c[1] != "forward")
    for part in ("forward_myoelbow_1dof6muscles", "forward_myolegs"):                             # ids asked before and after the first forward
        k = next(i for i, c in enumerate(golden[part]) if c[:2] == ["call", "myo_forward"])
        assert golden[part][k][3] == 0 and all(c[4] != 0 for c in golden[part][:k] if c[0] == "lookup")
        site_xmat = [c for c in golden[part][k:] if c[0] == "lookup" and c[2] == 4 and c[3] is None]
        assert [c[4] for c in site_xmat] == ([-4] if "elbow" in part else [0]), part               # MYO_E_UNSUPPORTED without site_quat
    widths = {c[2]: c[7] for c in golden["objects"] if c[0] == "lookup" and c[4] == 0}
    assert widths == {0: 6, 1: 6, 2: 6, 3: 2}
    assert [c[5] for c in reads if c[1] == "episode" and c[2] == 2 and c[4] == 4 * B] == [-1, -1, -1]   # MYO_EP_FINISHED is a byte per env
    status = golden["status"]
    assert [c[3] for c in status] == [0, -1, -1] and status[0][5] == "00" * 4 * B


_NOW = {}


@pytest.mark.parametrize("part", PARTS)
def test_every_call_answers_as_recorded(golden, part):
    import record_buffer_responses as rec
    if part not in _NOW:
        _NOW[part] = json.loads(json.dumps(rec.record_part(part)))
    g, n = golden[part], _NOW[part]
    k = next((i for i, (a, b) in enumerate(zip(g, n)) if a != b), min(len(g), len(n)))
    assert k == max(len(g), len(n)), f"{part}: call {k} of {len(g)} differs: expected {str(g[k:k + 1])[:400]}, got {str(n[k:k + 1])[:400]}"


# ---- the binding ---------------------------------------------------------------------------------------------------------------------
class _Counted:
    """Wraps the lookup functions of the loaded library: every call is logged as (name, batch handle, id)."""

    def __init__(self, monkeypatch, names):
        from myosuite_mjx_amd import objects
        self.log = []
        L = objects.lib()
        for name in names:
            monkeypatch.setattr(L, name, self._wrap(name, getattr(L, name)))

    def _wrap(self, name, fn):
        def counted(*args):
            self.log.append((name, args[0].value, args[1] if len(args) == 5 else None))       # (handle, id, void**, size_t*, size_t*), or without the id
            return fn(*args)
        return counted

    def count(self, name, batch, i=None):
        return self.log.count((name, batch.h.value, i))


def _check_view(view, again, ptr, dtype, shape):
    import torch
    tdt = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8}[dtype]
    assert view is again                                                       # cached: the second access is the same tensor object
    assert view.is_cuda and view.data_ptr() == ptr and view.dtype == tdt and tuple(view.shape) == tuple(shape), (view.dtype, view.shape, dtype, shape)


def _same(host, view, dtype, shape):
    assert isinstance(host, np.ndarray) and host.dtype == np.dtype(dtype) and host.shape == tuple(shape), (host.dtype, host.shape, dtype, shape)
    assert host.tobytes() == view.cpu().numpy().tobytes()


_WALK = []


def _walk_envs():
    """myoLegWalk-v0 with torch and with numpy I/O in the same state: made once for the module."""
    import torch
    import myosuite_mjx_amd as myo
    if _WALK:
        return _WALK
    envs = [myo.make("myoLegWalk-v0", num_envs=B, as_torch=t, rwd_dict=True, episode_stats=True, seed=5) for t in (True, False)]
    a = np.linspace(-1.0, 1.0, B * envs[0].act_dim, dtype=np.float32).reshape(B, -1)
    for env in envs:                                                           # the same state in both: reset and two steps
        env.reset(seed=11)
        for _ in range(2):
            env.step(torch.as_tensor(a, device="cuda") if env.as_torch else a)
    torch.cuda.synchronize()
    _WALK.extend(envs)
    return _WALK


def test_fields_reward_row_and_episode_buffers_through_the_binding(monkeypatch):
    import torch
    from myosuite_mjx_amd import capi
    names = {"field": "myo_batch_field", "rwd": "myo_batch_rwd_row", "episode": "myo_batch_episode_buffer"}
    calls = _Counted(monkeypatch, names.values())
    et, en = _walk_envs()
    nq, obs_dim, ncol = et.mjmodel.nq, et.obs_dim, len(et.rwd_keys)
    cases = [("field", capi.F_QPOS, np.float32, (B, nq)), ("field", capi.F_OBS, np.float32, (B, obs_dim)), ("field", capi.F_REWARD, np.float32, (B, 1)),
             ("field", capi.F_ELAPSED, np.int32, (B, 1)), ("field", capi.F_FLAGS, np.int32, (B, 1)), ("rwd", None, np.float32, (B, ncol)),
             ("episode", capi.EP_RUNNING, np.float32, (B, 4)), ("episode", capi.EP_LAST, np.float32, (B, 4)),
             ("episode", capi.EP_FINISHED, np.uint8, (B,)), ("episode", capi.EP_COUNT, np.int32, (B,))]
    for family, i, dtype, shape in cases:
        v = et.view(i, family)
        assert calls.count(names[family], et.batch, i) == 1, (family, i)               # reset / step / this access: one lookup in all
        ptr, pitch, width = et.batch.buffer_ptr(family, i)
        assert et.batch.buffer_spec(family, i, width) == (dtype, shape)        # the family table's statement
        _check_view(v, et.view(i, family), ptr, dtype, shape)
        _same(en.view(i, family), v, dtype, shape)
    assert et.view(capi.F_OBS) is et.view(capi.F_OBS, "field") and et.rwd_terms is et.view(None, "rwd") and et.episode_count is et.view(capi.EP_COUNT, "episode")
    _same(en.rwd_terms, et.rwd_terms, np.float32, (B, ncol))
    _same(en.episode_count, et.episode_count, np.int32, (B,))
    assert int(et.view(capi.F_ELAPSED).sum()) == 2 * B and float(et.view(capi.EP_RUNNING, "episode")[:, 2].sum()) == 2 * B   # two steps were counted
    for f, dtype, shape in ((capi.F_QPOS, np.float32, (B, nq)), (capi.F_ELAPSED, np.int32, (B, 1))):
        _same(en.batch.read(f), et.view(f), dtype, shape)
    _same(en.batch.read_rwd(), et.rwd_terms, np.float32, (B, ncol))
    _same(en.batch.read_episode(capi.EP_FINISHED), et.view(capi.EP_FINISHED, "episode"), np.uint8, (B,))
    assert en.status().dtype == np.int32 and en.status().shape == (B,)
    torch.cuda.synchronize()


def test_forward_buffers_through_the_binding(monkeypatch):
    from myosuite_mjx_amd import capi
    calls = _Counted(monkeypatch, ["myo_forward_buffer"])
    et, en = _walk_envs()
    rt, rn = et.forward(), en.forward()
    import torch
    torch.cuda.synchronize()
    assert et.forward() is rt                                                  # the record and its views are made once
    nbody, nsite, ngeom, ncap = et.model.forward_dims()
    n_of = {capi.FWD_XPOS: nbody, capi.FWD_XMAT: nbody, capi.FWD_XIPOS: nbody, capi.FWD_SITE_XPOS: nsite, capi.FWD_SITE_XMAT: nsite,
            capi.FWD_GEOM_XPOS: ngeom, capi.FWD_GEOM_XMAT: ngeom, capi.FWD_CONTACT: ncap}
    ncon = rt.ncon.cpu().numpy()
    for name, which in capi.FWD_NAMES.items():
        dtype = np.int32 if which == capi.FWD_NCON else np.float32
        shape = (B,) if which == capi.FWD_NCON else (B, n_of[which], *capi._FWD_ITEM[which])
        assert calls.count("myo_forward_buffer", et.batch, which) == 1, name          # two forward() calls, one lookup per buffer
        ptr, pitch, width = et.batch.forward_ptr(which)
        assert et.batch.buffer_spec("forward", which, width) == (dtype, shape) and et.batch.forward_shape(which) == shape
        if which == capi.FWD_CONTACT:                                          # a ContactList of slices of the one view
            c, cn = rt.contact, rn.contact
            assert c.dist.data_ptr() == ptr and tuple(c.frame.shape) == (B, ncap, 9) and c.geom1.dtype == torch.int32 and c is et.forward().contact
            assert cn.dist.shape == (B, ncap) and cn.pos.dtype == np.float32 and cn.pair.dtype == np.int32
            for e in range(B):                                                 # records at or beyond ncon are unspecified
                for attr in ("dist", "pos", "frame", "geom1", "geom2", "pair"):
                    assert getattr(cn, attr)[e, :ncon[e]].tobytes() == getattr(c, attr)[e, :ncon[e]].cpu().numpy().tobytes(), (e, attr)
            continue
        _check_view(getattr(rt, name), getattr(et.forward(), name), ptr, dtype, shape)
        _same(getattr(rn, name), getattr(rt, name), dtype, shape)
        _same(en.batch.forward_read(which), getattr(rt, name), dtype, shape)
    assert rt.body_xpos is rt.xpos and ncon.min() >= 0 and ncon.max() <= ncap


def test_object_tables_through_the_binding(monkeypatch):
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import objects
    calls = _Counted(monkeypatch, ["myo_objects_table"])
    et, en = (myo.make("myoChallengeBaodingP1-v1", num_envs=B, as_torch=t) for t in (True, False))
    pt, pn = et.object_params, en.object_params
    scale = np.array([1.0, 1.25, 1.5], np.float32)
    for p in (pt, pn):                                                         # another value per env, through each side's own write path
        p.mass = p.mass * (scale[:, None] if p is pn else pt.mass.new_tensor(scale)[:, None])
    for name, which in (("size", objects.OBJ_SIZE), ("pos", objects.OBJ_POS), ("friction", objects.OBJ_FRICTION), ("mass", objects.OBJ_MASS)):
        shape = (B, 2) if name == "mass" else (B, 2, 3)
        v = getattr(pt, name)
        assert calls.count("myo_objects_table", et.batch, which) == 1, name
        _check_view(v, getattr(pt, name), pt.table_ptr(which)[0], np.float32, shape)
        _same(getattr(pn, name), v, np.float32, shape)
        _same(pn.read(which), v, np.float32, shape)
    assert pt.mass[2, 0].item() == pytest.approx(1.5 * pt.mass[0, 0].item(), rel=1e-6)


def test_learner_tensors_through_the_binding(monkeypatch):
    import ppo_update_ref as R
    from test_gpu_ppo_update import CASES
    from myosuite_mjx_amd import capi, ppo
    shape, seed = min(CASES.values(), key=lambda c: c[0][0] * c[0][1] * c[0][2])       # the smallest case: one sample
    assert shape == CASES["one"][0]
    case = R.make_case(*shape, seed=seed)
    L = capi.lib()
    log = []
    raw = L.myo_ppo_learner_tensor
    monkeypatch.setattr(L, "myo_ppo_learner_tensor", lambda *a: (log.append(a[1:5]), raw(*a))[1])
    learner = ppo.Learner(case["obs_dim"], case["act_dim"], *case["params"], case["T"], case["mb"], learning_rate=R.LR, **R.HYPER)
    groups = learner.tensors("param")
    flat = [t for g in groups for t in g]
    assert len(log) == len(flat) == len(set(log)) and learner.tensors("param") is groups and len(log) == len(flat)      # one lookup per tensor, then none
    want = [a for g in case["params"] for a in g]
    for net, group_w, group_b in ((0, groups[0], groups[1]), (1, groups[2], groups[3])):
        for layer, (w, b) in enumerate(zip(group_w, group_b)):
            for what, t in ((0, w), (1, b)):
                p, n = C.c_void_p(), C.c_size_t()
                assert raw(learner.h, net, layer, what, learner.WHICH["param"], C.byref(p), C.byref(n)) == 0
                _check_view(t, t, p.value, np.float32, t.shape)
                assert n.value == t.numel()
    for t, a in zip(flat, want):                                               # the shapes and values the learner was created with
        assert tuple(t.shape) == np.asarray(a).shape and t.cpu().numpy().tobytes() == np.asarray(a, np.float32).tobytes()
