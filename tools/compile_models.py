"""Compile the reference's MJCF config models into committed MYOB blobs.

Runs in the build container only (reads the model *data* files under /root/reference;
they do not travel to the GPU box).  Usage: python tools/compile_models.py [--check] [model ...]

--check compiles without writing and compares every model with the committed files: blob bytes after
decompression, the JSON side-car and the sensor side-car; one line per model, exit status 1 on any difference."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from myosuite_mjx_amd import model as M  # noqa: E402

REF = os.environ.get("MYO_REFERENCE", "/root/reference")
MODELS = {
    "myohand_pose": "myosuite/envs/myo/assets/hand/myohand_pose.xml",
    "myofinger_v0": "myosuite/simhive/myo_sim/finger/myofinger_v0.xml",
    "myolegs": "myosuite/simhive/myo_sim/leg/myolegs.xml",
    "myoelbow_1dof6muscles": "myosuite/envs/myo/assets/elbow/myoelbow_1dof6muscles.xml",
    "myoelbow_1dof6muscles_1dofexo": "myosuite/envs/myo/assets/elbow/myoelbow_1dof6muscles_1dofexo.xml",
    "motorfinger_v0": "myosuite/simhive/myo_sim/finger/motorfinger_v0.xml",
    "myohand_hold": "myosuite/envs/myo/assets/hand/myohand_hold.xml",
    "myolegs_terrain": ("myosuite/simhive/myo_sim/leg/myolegs.xml",),     # height field raised and colliding (TerrainEnvV0)
    # MyoDM TrackEnv (mjx/myodm_v0.py:306-308): myohand_object.xml with OBJECT_NAME -> airplane; meshes collide as convex hulls
    "myohand_object_airplane": ("myosuite/envs/myo/assets/hand/myohand_object.xml", {"OBJECT_NAME": "airplane"}),
    # a second MyoDM object (MyoHand_cup_drink1.npz is the other motion file of tests/golden/ref_motion.npz): same code, another asset
    "myohand_object_cup": ("myosuite/envs/myo/assets/hand/myohand_object.xml", {"OBJECT_NAME": "cup"}),
}
# more MyoDM objects (round 3): one per shape family of simhive/object_sim -- no new code, only assets (stored gzip-compressed: .myob.gz)
for _obj in ("apple", "cubesmall", "duck", "mug", "hammer", "bowl"):
    MODELS[f"myohand_object_{_obj}"] = ("myosuite/envs/myo/assets/hand/myohand_object.xml", {"OBJECT_NAME": _obj}, "gz")
# ... and the rest of the reference's OBJECTS tuple (envs/myo/myodm/__init__.py:586-637): every object MyoDM registers Fixed / Random / motion ids for
for _obj in ("alarmclock", "banana", "binoculars", "camera", "coffeemug", "cubelarge", "cubemedium", "cylinderlarge", "cylindermedium", "cylindersmall",
             "elephant", "eyeglasses", "flashlight", "flute", "gamecontroller", "hand", "headphones", "knife", "lightbulb", "mouse", "phone", "piggybank",
             "pyramidlarge", "pyramidmedium", "pyramidsmall", "scissors", "spherelarge", "spheremedium", "spheresmall", "stamp", "stanfordbunny", "stapler",
             "teapot", "toothbrush", "toothpaste", "toruslarge", "torusmedium", "torussmall", "train", "watch", "waterbottle", "wineglass"):
    MODELS[f"myohand_object_{_obj}"] = ("myosuite/envs/myo/assets/hand/myohand_object.xml", {"OBJECT_NAME": _obj}, "gz")

# compiled models committed as data fixtures under tests/golden/ (gzip-compressed; model.load_asset finds them there)
GOLDEN = {
    "myohand_keyturn": "myosuite/envs/myo/assets/hand/myohand_keyturn.xml",   # KeyTurnEnvV0: a box bit and joint friction loss (TrackEnv class)
    "myohand_pen": "myosuite/envs/myo/assets/hand/myohand_pen.xml",           # PenTwirl*EnvV0: condim-4 pen pairs (TrackEnv class), plane - cylinder
    "myohand_baoding": "myosuite/envs/myo/assets/hand/myohand_baoding.xml",   # BaodingEnvV1: two free balls (TrackEnv class), plane - sphere
    "myohand_die": "myosuite/envs/myo/assets/hand/myohand_die.xml",           # ReorientEnvV0: the die's boxes alone make it TrackEnv class
}


def compile_model(stem):
    """(model, sensor side-car or None, path stem of the model's files, stored gzip-compressed?) of one model of MODELS / GOLDEN."""
    if stem in GOLDEN:
        return M.from_mjcf(os.path.join(REF, GOLDEN[stem])), None, os.path.join(M.GOLDEN_DIR, stem), True
    rel = MODELS[stem]
    if isinstance(rel, tuple) and len(rel) >= 2:
        m = M.from_mjcf(os.path.join(REF, rel[0]), replace=rel[1], convex_meshes=True)
    else:
        m = M.from_mjcf(os.path.join(REF, rel[0]), terrain=True) if isinstance(rel, tuple) else M.from_mjcf(os.path.join(REF, rel))
    m, side = M.split_sensor_arrays(m)      # touch-sensor arrays go to a side-car of their own: the model's blob keeps its older arrays only
    return m, side, os.path.join(M.ASSET_DIR, stem), isinstance(rel, tuple) and len(rel) == 3


def differences(m, path):
    """What differs between a fresh model and the files committed at `path`: blob bytes (after decompression) and the JSON side-car."""
    if not (os.path.exists(path + ".myob") or os.path.exists(path + ".myob.gz")) or not os.path.exists(path + ".json"):
        return ["missing"]
    with open(path + ".json") as f:
        meta = json.load(f)
    return [what for what, same in (("blob", m.blob() == M.Model.load(path).blob()),
                                    ("json", meta == {"names": m.names, "source": os.path.basename(m.source)})) if not same]


def check(stem):
    """Compile one model without writing and compare with the committed files; returns the list of differences."""
    m, side, path, _ = compile_model(stem)
    diff = differences(m, path)
    side_path = os.path.join(M.SENSOR_DIR, stem)
    if side is not None:
        diff += ["sensors." + d for d in differences(side, side_path)]
    elif os.path.exists(side_path + ".json"):
        diff.append("sensors.stale")
    return diff


if __name__ == "__main__":
    only = [a for a in sys.argv[1:] if a != "--check"]
    stems = [s for s in (*MODELS, *GOLDEN) if not only or s in only]
    if "--check" in sys.argv[1:]:
        bad = 0
        for stem in stems:
            diff = check(stem)
            bad += bool(diff)
            print(stem, "identical" if not diff else "DIFFERS: " + ", ".join(diff), flush=True)
        print(f"{len(stems) - bad} of {len(stems)} models identical to the committed files")
        sys.exit(1 if bad else 0)
    for stem in stems:
        m, side, path, compress = compile_model(stem)
        if side is not None:
            os.makedirs(M.SENSOR_DIR, exist_ok=True)
            side.save(os.path.join(M.SENSOR_DIR, stem), compress=True)
        m.save(path, compress=compress)
        print(stem, dict(nq=m.nq, nv=m.nv, nu=m.nu, nbody=m.nbody, ntendon=m.ntendon, bytes=len(m.blob())))
