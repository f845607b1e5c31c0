"""What `envs.make` sends to the binding layer, pinned without a GPU: tools/record_env_setup.py replaces capi.HipModel / capi.HipBatch by
recorders and builds every non-track id, the kwarg cases, four MyoDM cases and the error cases (exception type only).  The golden record
tests/golden/env_setup_calls.json.gz was written by that tool from the commit before the env layer got its per-task records (tasks.py), so it is
not a product of the code under test.  Equality is exact: floats are compared as float.hex, arrays as dtype + shape + bytes."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recorded():
    import record_env_setup
    with gzip.open(os.path.join(ROOT, "tests", "golden", "env_setup_calls.json.gz"), "rt") as f:
        golden = json.load(f)
    return golden, json.loads(json.dumps(record_env_setup.record()))


def test_the_recorded_cases_are_the_golden_ones(recorded):
    golden, now = recorded
    assert sorted(now) == sorted(golden)
    from myosuite_mjx_amd import envs
    plain = [i for i in envs.REGISTRY if envs.REGISTRY[i].get("task") != "track"]
    assert len(plain) == 129 and all("calls" in golden[i] for i in plain)        # every non-track id is a case of its own
    assert sum("error" in v for v in golden.values()) >= 100


def test_every_case_makes_the_same_calls_with_the_same_bytes(recorded):
    golden, now = recorded
    bad = []
    for name in sorted(golden):
        g, n = golden[name], now.get(name)
        if g == n:
            continue
        if n is None or "error" in g or "error" in n:
            bad.append(f"{name}: expected {g.get('error', 'a built env')}, got {(n or {}).get('error', 'a built env')}")
            continue
        gc, nc = g["calls"], n["calls"]
        k = next((i for i, (a, b) in enumerate(zip(gc, nc)) if a != b), min(len(gc), len(nc)))
        if k < max(len(gc), len(nc)):
            bad.append(f"{name}: call {k} differs: expected {str(gc[k:k + 1])[:300]}, got {str(nc[k:k + 1])[:300]}")
        else:
            keys = [a for a in ("attrs", "mjmodel", "myodm_spec") if g.get(a) != n.get(a)]
            sub = [a for a in g["attrs"] if g["attrs"][a] != n["attrs"].get(a)]
            bad.append(f"{name}: same calls, but {keys} differ ({sub})")
    assert not bad, "\n".join(bad[:20]) + f"\n({len(bad)} of {len(golden)} cases differ)"


def test_setup_of_every_task_runs_without_any_capi_object(monkeypatch):
    """`setup(m, spec, env_id)` is host arithmetic: with HipModel / HipBatch unusable it still returns the call and its follow-ups."""
    from myosuite_mjx_amd import capi, envs, model as M, tasks

    def unusable(*a, **k):
        raise AssertionError("a setup function touched the binding layer")
    real = capi.HipBatch
    monkeypatch.setattr(capi, "HipModel", unusable)
    monkeypatch.setattr(capi, "HipBatch", unusable)
    monkeypatch.setattr(capi, "lib", unusable)
    seen = {}
    for env_id, spec in envs.REGISTRY.items():
        if spec.get("task") == "track" or "muscle_condition" in spec:
            continue
        m = M.load_asset(spec["model"])
        s = tasks.TASKS[spec["task"]].setup(m, dict(spec), env_id)
        assert s.call == ("configure_walk" if spec["task"] == "walk" else "configure")
        assert hasattr(real, s.call) and all(name in ("set_body_pos_range", "set_body_quat_range", "set_geom_override") for name, _ in s.then)
        assert s.kwargs["frame_skip"] == spec["frame_skip"]
        seen.setdefault(spec["task"], s)
    assert sorted(seen) == sorted(tasks.TASKS)                                  # every record was exercised
    exo = dict(envs.REGISTRY["myoElbowPose1D6MExoFixed-v0"], weight_bodyname="carry_weight", weight_range=(0.1, 2.0))
    s = tasks.TASKS["pose"].setup(M.load_asset(exo["model"]), exo, "exo")
    assert s.body_mass_range == ("carry_weight", 0.1, 2.0) and s.then == ()
    legs = M.load_asset("myolegs")                                              # the stand tip must ride on the root link
    off_root = next(n for i, n in enumerate(legs.names["site"]) if int(legs.hip_site_link[i]) != 0)
    with pytest.raises(NotImplementedError):
        tasks.TASKS["stand"].setup(legs, dict(envs.REGISTRY["myoLegStandRandom-v0"], tip=off_root), "stand")


def test_kwarg_tables_are_derived_from_the_records():
    from myosuite_mjx_amd import envs, tasks
    E = envs.BatchedMyoEnv
    assert E.ENV_KWARGS == ("reset_type", "fatigue_reset_random", "fatigue_reset_vec", "weight_bodyname", "weight_range", "target_jnt_range",
                            "goal_th", "key_init_range", "task_choice", "goal_time_period", "goal_xrange", "goal_yrange", "drop_th", "proximity_th",
                            "goal_pos", "goal_rot", "pos_th", "rot_th")
    assert E.POSE_KWARGS == ("weight_bodyname", "weight_range", "target_jnt_range") and E.KEYTURN_KWARGS == ("goal_th", "key_init_range")
    assert {s["task"] for s in envs.REGISTRY.values()} - {"track"} == set(tasks.TASKS)
    with pytest.raises(TypeError, match=r"'drop_th' \(baoding / die task only\)"):   # the message names the tasks that take the kwarg
        envs.make("myoHandPenTwirlFixed-v0", drop_th=0.1)
    with pytest.raises(TypeError, match="the pen task takes"):
        envs.make("myoHandPenTwirlFixed-v0", no_such_kwarg=1)


def test_field_properties_keep_their_documentation_and_guards():
    from myosuite_mjx_amd import envs
    E = envs.BatchedMyoEnv
    for name, head in (("body_mass", "[num_envs, nbody] mass"), ("body_pos", "[num_envs, 3] offset of the key body"), ("body_quat", "[num_envs, 4] body_quat"),
                       ("goal_params", "[num_envs, 5] goal parameters"), ("goal_offset", "[num_envs, 3] offset of the die task's target")):
        p = getattr(E, name)
        assert isinstance(p, property) and p.fset is not None and p.__doc__.startswith(head) and "as_torch=False" in p.__doc__
    e = E.__new__(E)                                                           # the task guard needs no GPU
    e.spec = dict(task="pose")
    for name, msg in (("goal_params", "baoding task only"), ("goal_offset", "die task only")):
        with pytest.raises(AttributeError, match=msg):
            getattr(e, name)
        with pytest.raises(AttributeError, match=msg):
            setattr(e, name, np.zeros(3))
