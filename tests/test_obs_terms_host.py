"""CPU tests of the observation terms (obs_dict / obs_keys / proprio_keys of the batched envs): the term table and the default keys
against the reference's text (tests/golden/obs_terms.json), the default keys' widths against every registered id's recorded obs_dim, the
library's table by value (myo_obs_term_table), the binding of include/myo_hip_obs.h, the constructor parameters' validation without a GPU, obsvec2obsdict on a numpy
array, and the register / scratch figures of the one kernel the feature adds."""
import ctypes
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_capi_host as TC
from conftest import REFERENCE, ROOT

# an id per entry of the fixture (tests/test_reward_terms_host.py IDS)
IDS = {"pose": "myoHandPoseRandom-v0", "reach": "myoHandReachRandom-v0", "hold": "myoHandObjHoldRandom-v0", "keyturn": "myoHandKeyTurnRandom-v0",
       "pen": "myoHandPenTwirlRandom-v0", "stand": "myoLegStandRandom-v0", "walk": "myoLegWalk-v0", "terrain": "myoLegRoughTerrainWalk-v0",
       "baoding": "myoChallengeBaodingP1-v1", "die": "myoChallengeDieReorientP1-v0"}


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "obs_terms.json")))


def test_terms_and_default_keys_equal_the_reference_text(fixture):
    from myosuite_mjx_amd import envs, observations as O
    assert sorted(fixture) == sorted(IDS)
    for entry, ref in fixture.items():
        task = envs.REGISTRY[IDS[entry]]["task"]
        assert list(O.term_names(task)) == ref["keys"], entry
        assert list(O.DEFAULT_OBS_KEYS[task]) == ref["default_obs_keys"], entry
        assert "time" in ref["keys"] and "act" in ref["keys"] and set(ref["default_obs_keys"]) < set(ref["keys"])
    assert sorted(O.OBS_TERMS) == sorted(O.DEFAULT_OBS_KEYS) == sorted(set(spec["task"] for spec in envs.REGISTRY.values()) - {"track"})
    # the keys the canonical rows lack
    assert "t" in fixture["walk"]["keys"] and "target_pos" in fixture["reach"]["keys"] and "target_pos" in fixture["stand"]["keys"]
    assert "obj_des_pos" in fixture["pen"]["keys"] and "hand_qpos" in fixture["die"]["keys"]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="reference tree not present")
def test_fixture_equals_a_fresh_parse(fixture):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_obs_terms_fixture as T
    assert T.parse(REFERENCE) == fixture


@pytest.fixture(scope="module")
def recorded_obs_dim():
    """{env id: obs_dim} of the 129 non-MyoDM ids as tests/golden/env_setup_calls.json.gz recorded them, before tasks.py and before the row
    records (tests/test_env_setup_host.py): not a product of the code under test."""
    with gzip.open(os.path.join(ROOT, "tests", "golden", "env_setup_calls.json.gz"), "rt") as f:
        golden = json.load(f)
    from myosuite_mjx_amd import envs
    out = {i: golden[i]["attrs"]["obs_dim"] for i, reg in envs.REGISTRY.items() if reg["task"] != "track"}
    assert len(out) == 129 and all(isinstance(v, int) and v > 0 for v in out.values())
    return out


def test_default_keys_restate_every_registered_row(recorded_obs_dim):
    """For every registered id outside MyoDM: the default keys (with `act` where base_v0.py appends it) are as wide as the obs_dim recorded
    for the id -- the canonical row is the concatenation of the default keys."""
    from myosuite_mjx_amd import envs, model as M, observations as O
    n = 0
    for env_id, reg in envs.REGISTRY.items():
        if reg["task"] == "track":
            continue
        spec = dict(reg)
        m = M.load_asset(spec["model"])
        d = O.dims(m, spec)
        w = O.widths(spec["task"], d)
        keys = O.default_keys(spec["task"], d["na"])
        assert sum(w[k] for k in keys) == recorded_obs_dim[env_id], env_id
        assert ("act" in keys) == (d["na"] > 0 and spec["task"] not in O.NO_ACT_APPENDED), env_id
        assert all(v >= 0 for v in w.values()) and w["time"] == 1, env_id
        n += 1
    assert n > 100
    m = M.load_asset("motorfinger_v0")                      # no muscles: PoseEnvV0 fills act with zeros_like(qpos), ReachEnvV0 has no act
    d = O.dims(m, envs.REGISTRY["motorFingerPoseFixed-v0"])
    assert d["na"] == 0 and O.widths("pose", d)["act"] == m.nq and O.widths("reach", dict(d, ntip=1))["act"] == 0


def _check_library_table(task, d, obs_dim=None):
    """The library's table of `task` for the dimensions `d` (myo_obs_term_table: no batch, no GPU) against observations.py, by value."""
    from myosuite_mjx_amd import capi, observations as O
    terms, dim = capi.obs_term_table(getattr(capi, "TASK_" + task.upper()), **d)      # (observations.dims names the export's six arguments)
    assert [(k, w) for k, w, _ in terms] == list(O.widths(task, d).items()), (task, d)
    # the canonical row: the terms that lie in it, by offset, are the default keys in order, end to end
    blocks = sorted((at, k, w) for k, w, at in terms if at >= 0 and w > 0)
    keys = O.with_act(task, O.DEFAULT_OBS_KEYS[task], d["na"])
    assert tuple(k for _, k, _ in blocks) == keys, (task, d)
    assert [at for at, _, _ in blocks] == [sum(w for _, _, w in blocks[:i]) for i in range(len(blocks))], (task, d)
    assert dim == sum(w for _, _, w in blocks) and (obs_dim is None or dim == obs_dim), (task, d, dim, obs_dim)
    return terms, dim


def test_library_term_table_equals_the_python_one(recorded_obs_dim):
    """The library states each task's row once, as a record of its blocks (csrc/myo_task_<name>.h), and builds its term table from it;
    BatchedMyoEnv asserts names and widths agree when it enables the rows.  Here, for every registered id outside MyoDM, the library's
    names and widths equal observations.widths, the default keys are the row's blocks in order at the running sum of their widths, and the
    row's total is the obs_dim recorded for the id."""
    from myosuite_mjx_amd import capi, envs, model as M, observations as O
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    seen = set()
    for env_id, reg in envs.REGISTRY.items():
        if reg["task"] == "track":
            continue
        spec = dict(reg)
        _check_library_table(spec["task"], O.dims(M.load_asset(spec["model"]), spec), recorded_obs_dim[env_id])
        seen.add(spec["task"])
    assert seen == set(O.OBS_TERMS)
    d = O.dims(M.load_asset("motorfinger_v0"), envs.REGISTRY["motorFingerPoseFixed-v0"])       # no muscles
    terms, dim = _check_library_table("pose", d)
    assert ("act", d["nq"], -1) in terms and dim == 3 * d["nq"]              # zeros_like(qpos): as wide as qpos, from outside the row
    terms, dim = _check_library_table("reach", dict(d, ntip=1))
    assert ("act", 0) in [(k, w) for k, w, _ in terms] and dim == 2 * d["nq"] + 6
    # what lies outside the rows (tests/test_gpu_obs_terms.py reads these from their sources)
    outside = lambda task: {k for k, _, at in capi.obs_term_table(getattr(capi, "TASK_" + task.upper()), **O.dims(
        M.load_asset(envs.REGISTRY[IDS[task]]["model"]), envs.REGISTRY[IDS[task]]))[0] if at < 0}
    assert outside("pen") == {"time", "obj_des_pos"} and outside("die") == {"time", "hand_qpos", "act"} and outside("walk") == {"t", "time"}
    assert outside("reach") == outside("stand") == {"time", "target_pos"} and outside("baoding") == {"time", "act"}
    # no table: no task, the MyoDM track task, an id out of range
    for task in (capi.TASK_NONE, capi.TASK_TRACK, 99, -1):
        assert capi.obs_term_table(task, **d) == ((), 0)


def test_binding_matches_the_header():
    """capi.OBS_SIGNATURES against the prototypes of include/myo_hip_obs.h, the way tests/test_capi_host.py checks the core headers, and
    the library exports them."""
    from myosuite_mjx_amd import capi
    protos = {}
    for ret, name, args in re.findall(r"^[ \t]*((?:const\s+)?\w+[\s*]+)(myo_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", TC._header_text("myo_hip_obs.h"), flags=re.M):
        protos[name] = (TC._c_kind(ret), [TC._c_kind(a) for a in args.split(",")])
    assert sorted(protos) == sorted(capi.OBS_SIGNATURES) and len(protos) == 7
    for name, (ret, args) in protos.items():
        restype, argtypes = capi.OBS_SIGNATURES[name]
        assert (TC._ctypes_kind(restype), [TC._ctypes_kind(t) for t in argtypes]) == (ret, args), name
    assert not set(capi.OBS_SIGNATURES) & set(capi.SIGNATURES)
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    L = ctypes.CDLL(capi.LIB_PATH)
    assert all(hasattr(L, n) for n in protos)
    hdr = open(os.path.join(ROOT, "include", "myo_hip_obs.h")).read()
    assert (capi.OBS_TERMS, capi.OBS_SELECTED, capi.OBS_PROPRIO) == tuple(int(re.search(r"%s = (\d)" % n, hdr).group(1))
                                                                          for n in ("MYO_OBS_TERMS", "MYO_OBS_SELECTED", "MYO_OBS_PROPRIO"))
    assert '#include "myo_hip_obs.h"' in open(os.path.join(ROOT, "include", "myo_hip.h")).read()


def test_parameter_validation_needs_no_gpu():
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import envs, observations as O, tasks
    with pytest.raises(KeyError, match="nope"):                              # (TypeError from tasks.filter_kwargs before the feature)
        myo.make("myoHandPoseRandom-v0", num_envs=2, obs_keys=["nope"])
    with pytest.raises(KeyError, match="hand_qpos"):                         # a key of another task
        myo.make("myoHandPoseRandom-v0", num_envs=2, proprio_keys=["qpos", "hand_qpos"])
    with pytest.raises(ValueError, match="empty"):
        myo.make("myoLegWalk-v0", num_envs=2, obs_keys=[])
    for kw in (dict(obs_keys=["qpos"]), dict(proprio_keys=["qpos"]), dict(obs_dict=True)):
        with pytest.raises(NotImplementedError, match="MyoDM"):
            myo.make("MyoHandAirplaneFixed-v0", num_envs=2, **kw)
    spec = envs.REGISTRY["myoHandPoseRandom-v0"]
    assert O.resolve("myoHandPoseRandom-v0", spec) is None                   # the defaults: nothing to enable
    s = O.resolve("myoHandPoseRandom-v0", spec, obs_dict=True)
    assert s.obs_keys is None and s.proprio_keys is None                     # the default selection
    s = O.resolve("myoHandPoseRandom-v0", spec, obs_keys=["qpos", "time", "qpos"], proprio_keys="qvel")
    assert s.obs_keys == ("qpos", "time", "qpos") and s.proprio_keys == ("qvel",)    # a key may repeat; a single string is one key
    assert O.with_act("pose", s.obs_keys, 39) == ("qpos", "time", "qpos", "act") and O.with_act("pose", s.obs_keys, 0) == s.obs_keys
    assert O.with_act("pose", ("act", "qpos"), 39) == ("act", "qpos") and O.with_act("die", ("obj_pos",), 39) == ("obj_pos",)
    # the new parameters are the constructor's own: the pinned env-kwarg tables do not know them
    assert not {"obs_keys", "proprio_keys", "obs_dict"} & set(tasks.ENV_KWARGS)


def test_obsvec2obsdict_on_numpy():
    from myosuite_mjx_amd import observations as O
    width = O.widths("pose", dict(nq=3, nv=3, nu=4, na=2, ntip=1, pose_act=2))
    assert width == dict(time=1, qpos=3, qvel=3, act=2, pose_err=3)
    keys = ("qvel", "time", "act", "qvel")
    obs = np.arange(2 * 5 * 9, dtype=np.float32).reshape(2, 5, 9)            # [..., obs_dim]: leading axes pass through
    d = O.obsvec2obsdict(obs, keys, width)
    assert list(d) == ["qvel", "time", "act"] and d["time"].shape == (2, 5, 1) and np.shares_memory(d["act"], obs)
    assert np.array_equal(d["time"], obs[..., 3:4]) and np.array_equal(d["act"], obs[..., 4:6]) and np.array_equal(d["qvel"], obs[..., 6:9])
    assert O.slices(keys, width) == dict(qvel=slice(6, 9), time=slice(3, 4), act=slice(4, 6))
    with pytest.raises(ValueError, match="columns"):
        O.obsvec2obsdict(obs[..., :8], keys, width)


def test_obs_terms_kernel_has_no_spill_and_no_scratch():
    """Read from the code object's metadata the way tests/test_forward_resources.py reads the forward kernels; 64 VGPRs leave the 256-thread
    block at full occupancy."""
    from myosuite_mjx_amd import capi
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    found = []
    for r in kernel_resources.resources(capi.LIB_PATH):
        if "obs_terms_kernel" in r["name"]:
            name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
            if name.startswith("obs_terms_kernel("):
                found.append(r)
    assert len(found) == 1, found
    r = found[0]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0 and r["vgpr"] + r["agpr"] <= 64, r
