"""Fresh compile == committed asset, to the last byte (container only): one model per code path of mjcf.py / lowering.py."""
import os

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
