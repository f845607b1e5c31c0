"""Fresh compile == committed asset, to the last byte (container only): one model per code path of mjcf.py / lowering.py.  And, without
the reference tree, the lowering pass alone: every committed asset's compiled arrays lowered again give its committed hip_* tables."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import REFERENCE, needs_reference
from myosuite_mjx_amd import model as M

# stem -> (MJCF under the reference tree, from_mjcf keywords), as tools/compile_models.py compiles it
CASES = {
    "myohand_pose": ("envs/myo/assets/hand/myohand_pose.xml", {}),
    "myofinger_v0": ("simhive/myo_sim/finger/myofinger_v0.xml", {}),                          # tendon limits, pulleys, pruned plane pairs
    "myolegs": ("simhive/myo_sim/leg/myolegs.xml", {}),                                       # free joint, equalities, touch side-car
    "myolegs_terrain": ("simhive/myo_sim/leg/myolegs.xml", {"terrain": True}),                # height field
    "myoelbow_1dof6muscles_1dofexo": ("envs/myo/assets/elbow/myoelbow_1dof6muscles_1dofexo.xml", {}),   # joint transmission
    "motorfinger_v0": ("simhive/myo_sim/finger/motorfinger_v0.xml", {}),                      # affine actuators
    "myohand_hold": ("envs/myo/assets/hand/myohand_hold.xml", {}),                            # free object
    "myohand_object_cup": ("envs/myo/assets/hand/myohand_object.xml", {"replace": {"OBJECT_NAME": "cup"}, "convex_meshes": True}),   # hulls
    "myohand_keyturn": ("envs/myo/assets/hand/myohand_keyturn.xml", {}),                      # friction loss, box
    "myohand_baoding": ("envs/myo/assets/hand/myohand_baoding.xml", {}),                      # two free bodies
    "myohand_die": ("envs/myo/assets/hand/myohand_die.xml", {}),
}


@needs_reference
@pytest.mark.parametrize("stem", list(CASES))
def test_fresh_compile_equals_the_committed_bytes(stem):
    rel, kw = CASES[stem]
    fresh, side = M.split_sensor_arrays(M.from_mjcf(os.path.join(REFERENCE, rel), **kw))
    asset = M.Model.load(M.asset_stem(stem))
    assert fresh.blob() == asset.blob()
    assert fresh.names == asset.names
    assert (side is not None) == (stem in ("myolegs", "myolegs_terrain"))
    if side is not None:
        committed = M.Model.load(os.path.join(M.SENSOR_DIR, stem))
        assert side.blob() == committed.blob() and side.names == committed.names


def test_every_committed_asset_lowers_to_the_same_bytes():
    """All committed assets and golden blobs, the gzip-compressed MyoDM objects included: lowering their compiled arrays again reproduces
    the committed hip_* tables byte for byte, and what lowering refuses is what the asset marks `hip_unsupported`.  The one place this is
    checked: a change of lowering.py that a new model needs must leave every other model's tables alone."""
    from myosuite_mjx_amd.lowering import lower
    from myosuite_mjx_amd.mjcf import CompiledModel
    stems = sorted({re.sub(r"\.myob(\.gz)?$", "", os.path.basename(p)) for d in (M.ASSET_DIR, M.GOLDEN_DIR) for p in glob.glob(os.path.join(d, "*.myob*"))})
    assert len(stems) >= 61
    for stem in ("myohand_baoding", "myohand_die", "myohand_keyturn", "myohand_object_teapot", "myohand_object_airplane"):
        assert stem in stems
    for stem in stems:
        m = M.load_asset(stem)
        cm = CompiledModel(arrays={k: np.array(v, copy=True) for k, v in m.arrays.items() if not k.startswith("hip_")}, names=m.names)
        try:
            lower(cm)
        except NotImplementedError:
            assert "hip_unsupported" in m.arrays, stem
            continue
        hip = {k: v for k, v in m.arrays.items() if k.startswith("hip_")}
        assert sorted(k for k in cm.arrays if k.startswith("hip_")) == sorted(hip), stem
        for k, v in hip.items():
            a, b = np.asarray(cm.arrays[k]), np.asarray(v)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (stem, k)
