"""tests/golden/reward_terms.json from the reference's text: per task of the batched envs, the keys of its env class's `rwd_dict` (the
OrderedDict literal of get_reward_dict, in order) and the class's DEFAULT_RWD_KEYS_AND_WEIGHTS.  Names and numbers only; the files are
parsed (ast), never imported.

    python tools/make_reward_terms_fixture.py [reference root] [--check]"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "reward_terms.json")
REFERENCE = "/root/reference/myosuite"
# task of the batched envs -> (file under the reference root, env class)
CLASSES = {
    "pose": ("envs/myo/myobase/pose_v0.py", "PoseEnvV0"),
    "reach": ("envs/myo/myobase/reach_v0.py", "ReachEnvV0"),
    "hold": ("envs/myo/myobase/obj_hold_v0.py", "ObjHoldFixedEnvV0"),
    "keyturn": ("envs/myo/myobase/key_turn_v0.py", "KeyTurnEnvV0"),
    "pen": ("envs/myo/myobase/pen_v0.py", "PenTwirlFixedEnvV0"),
    "stand": ("envs/myo/myobase/walk_v0.py", "ReachEnvV0"),
    "walk": ("envs/myo/myobase/walk_v0.py", "WalkEnvV0"),
    "terrain": ("envs/myo/myobase/walk_v0.py", "TerrainEnvV0"),       # (its rwd_dict is WalkEnvV0's; its default weights are its own)
    "baoding": ("envs/myo/myochallenge/baoding_v1.py", "BaodingEnvV1"),
    "die": ("envs/myo/myochallenge/reorient_v0.py", "ReorientEnvV0"),
}


def _class(tree, name):
    return next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)


def _rwd_keys(tree, cls):
    """Keys of the OrderedDict literal assigned to rwd_dict in cls.get_reward_dict, then the keys added by `rwd_dict[<str>] = ...`; a class
    without the method takes its first base class's."""
    fn = next((n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "get_reward_dict"), None)
    if fn is None:
        return _rwd_keys(tree, _class(tree, cls.bases[0].id))
    keys = []
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id == "rwd_dict":
            keys = [ast.literal_eval(item.elts[0]) for item in node.value.args[0].elts] + keys
        elif (isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Subscript) and isinstance(node.targets[0].value, ast.Name)
              and node.targets[0].value.id == "rwd_dict" and isinstance(node.targets[0].slice, ast.Constant)):
            keys.append(node.targets[0].slice.value)
    return keys


def _default_weights(cls):
    node = next(n for n in cls.body if isinstance(n, ast.Assign) and n.targets[0].id == "DEFAULT_RWD_KEYS_AND_WEIGHTS")
    return {k: float(v) for k, v in ast.literal_eval(node.value).items()}


def parse(reference=REFERENCE):
    out = {}
    for task, (path, name) in CLASSES.items():
        with open(os.path.join(reference, path)) as f:
            tree = ast.parse(f.read())
        cls = _class(tree, name)
        out[task] = {"source": path, "class": name, "keys": _rwd_keys(tree, cls), "default_weights": _default_weights(cls)}
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--check"]
    doc = parse(args[0] if args else REFERENCE)
    if "--check" in sys.argv:
        assert doc == json.load(open(OUT)), "tests/golden/reward_terms.json is stale"
    else:
        with open(OUT, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    for task, d in doc.items():
        print(f"{task:8s} {d['class']:20s} {d['keys']}  {d['default_weights']}")
