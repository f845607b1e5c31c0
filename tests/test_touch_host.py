"""Touch sensors, host side (no GPU): the MJCF compiler and the lowering emit the sensor tables, the regenerated leg blobs keep every older
array byte for byte, and the float64 helper tests/touch_ref.py is pinned on the oracle alone."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import touch_ref as T  # noqa: E402
from myosuite_mjx_amd import blob as _blob  # noqa: E402
from myosuite_mjx_amd import model as M  # noqa: E402
from myosuite_mjx_amd.lowering import lower  # noqa: E402
from myosuite_mjx_amd.mjcf import GEOM_BOX, GEOM_CYLINDER, CompiledModel, quat2mat  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["r_foot", "r_toes", "l_foot", "l_toes"]
PRE_SENSOR_SHA256 = {"myolegs": "b725b3ed4ed074dc65060954042ff45d168d7644d6e5c2724b2e21b33df40916",
                     "myolegs_terrain": "9859342873782498ca4a9a9e7acdac31cda162285d89f0d770e5027fec29623c"}


def test_the_four_touch_sensors_compile_with_the_sizes_and_euler_of_the_xml(legs):
    m = legs
    assert m.names["sensor"] == NAMES
    assert [m.sensor_name2id(n) for n in NAMES] == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        m.sensor_name2id("nope")
    assert list(m.sensor_type) == [0] * 4 and list(m.sensor_adr) == [0, 1, 2, 3]
    sites = [m.site_name2id(n + "_touch") for n in NAMES]
    assert list(m.sensor_objid) == sites
    # myolegs_chain.xml: foot boxes .1 .01 .055 at (0.09, -.01, 0), euler 0; toes boxes .04 .01 .0675 at (0.0275, -.01, 0), euler 0 -+.7 0
    size = {"r_foot": (.1, .01, .055), "r_toes": (.04, .01, .0675), "l_foot": (.1, .01, .055), "l_toes": (.04, .01, .0675)}
    pitch = {"r_foot": 0.0, "r_toes": -0.7, "l_foot": 0.0, "l_toes": 0.7}
    for n, s in zip(NAMES, sites):
        assert int(m.site_type[s]) == GEOM_BOX
        np.testing.assert_allclose(m.site_size[s], size[n], atol=1e-15)
        np.testing.assert_allclose(m.site_pos[s], (0.09, -.01, 0) if "foot" in n else (0.0275, -.01, 0), atol=1e-15)
        a = pitch[n]
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        np.testing.assert_allclose(quat2mat(m.site_quat[s]), Ry, atol=1e-12)
    # defaults: the muscle sites of class myolegs are spheres of the class size; a marker site overrides the first entry only
    s = m.site_name2id("r_foot_touch") - 1
    assert int(m.site_type[s]) == 2
    assert m.site_size.shape == (m.nsite, 3) and m.site_quat.shape == (m.nsite, 4) and m.site_type.shape == (m.nsite,)


def test_lowered_touch_table(legs, terrain):
    for m in (legs, terrain):
        t = np.asarray(m.hip_touch)
        assert t.shape == (4, 18)
        for i, n in enumerate(NAMES):
            s = int(m.sensor_objid[i])
            assert int(t[i, 0]) == int(m.hip_site_link[s]) >= 0
            np.testing.assert_array_equal(t[i, 1:4], m.hip_site_lpos[s])
            assert int(t[i, 13]) == GEOM_BOX and int(t[i, 17]) == int(m.site_bodyid[s])
            np.testing.assert_array_equal(t[i, 14:17], m.site_size[s])
            R = t[i, 4:13].reshape(3, 3)
            np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
        cg = np.asarray(m.hip_cg_geom)
        np.testing.assert_array_equal(m.hip_cg_body, np.asarray(m.geom_bodyid)[cg])


@pytest.mark.parametrize("name", ["myolegs", "myolegs_terrain"])
def test_older_arrays_of_the_leg_models_are_byte_identical(name):
    """The new arrays are additive.  The model's own blob (assets/<name>.myob) is the file it was before the sensors, bit for bit, and the
    sensor arrays travel in the side-car tests/golden/sensors/<name>.myob.gz: every array of the blob file is in the loaded model with
    the same dtype, shape and bytes, the model has exactly the eight sensor arrays on top, and the blob the loader hands to the library
    unpacks to the same arrays."""
    with open(os.path.join(M.ASSET_DIR, name + ".myob"), "rb") as f:
        raw = f.read()
    assert hashlib.sha256(raw).hexdigest() == PRE_SENSOR_SHA256[name]      # the file of the commit before the sensors
    old = _blob.unpack(raw)
    m = M.load_asset(name)
    new = m.arrays
    assert len(old) > 100
    for k, v in old.items():
        assert k in new, k
        assert new[k].dtype == v.dtype and new[k].shape == v.shape and new[k].tobytes() == v.tobytes(), k
    assert sorted(set(new) - set(old)) == sorted(M.SENSOR_ARRAYS)
    again = _blob.unpack(m.blob())
    assert list(again) == list(new) and all(again[k].tobytes() == np.asarray(new[k]).tobytes() for k in new)


def test_split_and_merge_round_trip(legs):
    base, side = M.split_sensor_arrays(legs)
    assert "hip_touch" not in base.arrays and "sensor" not in base.names and sorted(side.arrays) == sorted(M.SENSOR_ARRAYS)
    with open(os.path.join(M.ASSET_DIR, "myolegs.myob"), "rb") as f:
        assert base.blob() == f.read()
    assert M.split_sensor_arrays(M.load_asset("myohand_pose"))[1] is None


def test_touch_sensor_on_another_site_shape_raises_in_lowering(legs):
    arrays = {k: np.array(v, copy=True) for k, v in legs.arrays.items() if not k.startswith("hip_")}
    arrays["site_type"][int(arrays["sensor_objid"][1])] = GEOM_CYLINDER
    with pytest.raises(NotImplementedError, match="r_toes"):
        lower(CompiledModel(arrays=arrays, names=legs.names))
    # a sphere site lowers
    arrays["site_type"][int(arrays["sensor_objid"][1])] = 2
    cm = lower(CompiledModel(arrays=arrays, names=legs.names))
    assert int(cm.arrays["hip_touch"][1, 13]) == 2


def test_hand_and_track_assets_have_no_touch_table(hand):
    assert "hip_touch" not in hand.arrays
    for n in ("myohand_object_airplane", "myohand_keyturn", "myofinger_v0"):
        m = M.load_asset(n)
        assert "hip_touch" not in m.arrays
        with pytest.raises(ValueError):
            m.sensor_name2id("r_foot")


@pytest.mark.parametrize("nsub", [1, 5])
def test_helper_forces_sum_to_the_constraint_force_on_the_root(legs, nsub):
    """Pins tests/touch_ref.py on the oracle alone: over the test states the per-contact world forces sum to qfrc_constraint[0:3] to 1e-9
    relative, and the states cover every sensor: non-zero in at least a third of the envs, zero in at least one."""
    from oracle.oracle import Oracle
    o = Oracle(legs.blob())
    q = T.states(legs)
    assert q.shape == (T.N_ENVS, legs.nq)
    for e in range(T.N_ENVS):
        o.reset()
        o.set_state(qpos=q[e], qvel=np.zeros(legs.nv), act=np.zeros(legs.nu), ctrl=np.zeros(legs.nu))
        o.step(nsub)
        _, cfrc, ncon, F = T.touch_reference(o, legs)
        qfc = np.array(o.field("qfrc_constraint"), float)[:3]
        assert np.abs(F.sum(0) - qfc).max() <= 1e-9 * np.abs(qfc).max()      # (an env that left the floor: 0 <= 0)
        assert np.abs(cfrc[-1] - qfc).max() <= 1e-9 * np.abs(qfc).max()
    ref = T.oracle_outputs(legs, nsub)
    nz = (ref["sens"] > 0).mean(0)
    assert (nz >= 1 / 3).all() and ((ref["sens"] == 0).sum(0) >= 1).all(), nz
    # the push is 0 - 8 mm, the roll within +-0.15 rad
    _, push, roll = T.make_states(legs)
    assert push.min() >= 0 and push.max() <= 0.008 and np.abs(roll).max() <= 0.15


def test_ray_rule_of_the_helper():
    box = np.array([0.1, 0.01, 0.05])
    assert T.ray_meets(GEOM_BOX, box, np.array([0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))          # inside: always
    assert T.ray_meets(GEOM_BOX, box, np.array([0.05, -0.5, 0.0]), np.array([0.0, 1.0, 0.0]))        # below, pointing at it
    assert not T.ray_meets(GEOM_BOX, box, np.array([0.05, -0.5, 0.0]), np.array([0.0, -1.0, 0.0]))   # pointing away
    assert not T.ray_meets(GEOM_BOX, box, np.array([0.2, -0.5, 0.0]), np.array([0.0, 1.0, 0.0]))     # passes beside it
    assert T.ray_meets(2, np.array([0.1, 0, 0]), np.array([0.0, 0.0, -1.0]), np.array([0.0, 0.0, 1.0]))
    assert not T.ray_meets(2, np.array([0.1, 0, 0]), np.array([0.0, 0.0, -1.0]), np.array([0.0, 0.0, -1.0]))
