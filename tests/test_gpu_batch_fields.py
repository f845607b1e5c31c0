"""The batch half of the host library (myo_batch_field / read / write, configure(quat_body), myo_batch_enable_sensors) against a recorded
fixture: tools/record_batch_fields.py runs one scripted sequence of calls on four models with B = 3 envs -- every field id from -1 to
MYO_F_CFRC + 1 on a fresh batch, the rejected and the accepted writes of every validated field with the rows read back, the order of
quat_body and the orientation fields, the sensor fields before and after they are enabled, one step per started override -- and
tests/golden/batch_field_responses.json.gz holds what the library answered at the commit before its field table and override records
(8908d51), so the fixture is not a product of the code under test.  Equality is exact: return code, error text, pitch and width, and the
bytes of every array a read returned.  These are what the host code decides: after a batch's first step the script reads only override
fields and rows it has just written, so no float arithmetic of a kernel is compared (test_the_fixture_holds_the_cases checks that)."""
import gzip
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
MODELS = ("myoelbow_1dof6muscles", "myohand_keyturn", "myohand_pen", "myolegs")
_NOW = {}


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "batch_field_responses.json.gz"), "rt") as f:
        return json.load(f)


def _now(name):
    import record_batch_fields
    if name not in _NOW:
        _NOW[name] = json.loads(json.dumps(record_batch_fields.record_model(name)))
    return _NOW[name]


def test_the_fixture_holds_the_cases(golden):
    import record_batch_fields
    from myosuite_mjx_amd import capi
    assert record_batch_fields.MODELS == MODELS and sorted(golden) == sorted(MODELS) and record_batch_fields.B == 3
    for name in MODELS:
        calls = golden[name]["overrides"]
        ids = {c[1] for c in calls if c[0] == "read"}
        assert ids >= set(range(-1, capi.F_CFRC + 2))                            # every id, one below and one above
        writes = [c for c in calls if c[0] == "write"]
        for f in range(capi.F_BODYMASS, capi.F_BODYQUAT_RANGE + 1):              # every validated field was written, and refused at least once
            assert any(c[1] == f and c[3] != 0 for c in writes), (name, f)
        assert any(c[1] == capi.F_SENSORDATA and c[3] == -1 for c in writes)
    own_rows = set(range(capi.F_BODYMASS, capi.F_BODYQUAT_RANGE + 1)) | {capi.F_ELAPSED, capi.F_TIME}
    for name in MODELS:                                                          # no array a step wrote: after a part's first step, reads
        for calls in golden[name].values():                                      # return bytes only of override fields and rows just written
            k = next((i for i, c in enumerate(calls) if c[0] == "step"), len(calls))
            assert all(c[1] in own_rows for c in calls[k:] if c[0] == "read" and c[3] == 0), name
    started = {"myoelbow_1dof6muscles": (capi.F_BODYMASS, "step_kernel_w<24,8,32,1,3,false,0,false>"),
               "myohand_keyturn": (capi.F_BODYPOS, "step_kernel_w<36,20,32,2,2,false,0,false,true>"),
               "myohand_pen": (capi.F_BODYQUAT, "step_kernel_w<36,20,32,2,2,false,0,false,true>"),
               "myolegs": (capi.F_BODYMASS, "step_kernel_w<36,20,32,2,2,false,0,false>")}
    for name, (f, kernel) in started.items():                                    # the model's own override took an accepted write, and its
        assert any(c[0] == "write" and c[1] == f and c[3] == 0 for c in golden[name]["overrides"])   # start routes to the run-time-sizes kernel
        assert [c for c in golden[name]["pointer_start"] if c[0] == "field"][-1][2] == 0
        assert golden[name]["pointer_start"][-1][:3] == ["step", "", kernel]
    assert [c[1] for c in golden["myolegs"]["sensors"] if c[0] == "enable_sensors"] == [0, 0]
    assert [c[1] for c in golden["myoelbow_1dof6muscles"]["sensors"] if c[0] == "enable_sensors"] == [-4]
    pen = golden["myohand_pen"]["overrides"]
    assert [c[2][:20] for c in pen if c[0] == "configure"][-2:] == ["libmyo_hip error -1:", ""]   # a second body after the start: refused


@pytest.mark.parametrize("name", MODELS)
def test_every_call_answers_as_recorded(golden, name):
    g, n = golden[name], _now(name)
    assert sorted(g) == sorted(n)
    bad = []
    for part in sorted(g):
        gc, nc = g[part], n[part]
        k = next((i for i, (a, b) in enumerate(zip(gc, nc)) if a != b), min(len(gc), len(nc)))
        if k < max(len(gc), len(nc)):
            bad.append(f"{name}/{part}: call {k} of {len(gc)} differs: expected {str(gc[k:k + 1])[:400]}, got {str(nc[k:k + 1])[:400]}")
    assert not bad, "\n".join(bad)
