"""tests/golden/obs_terms.json from the reference's text: per task of the batched envs, the keys of its env class's `obs_dict` (the
`obs_dict[<str>] = ...` assignments of get_obs_dict, in source order) and the class's DEFAULT_OBS_KEYS.  Names only; the files are parsed
(ast), never imported.

    python tools/make_obs_terms_fixture.py [reference root] [--check]"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "obs_terms.json")
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
    "terrain": ("envs/myo/myobase/walk_v0.py", "TerrainEnvV0"),       # (its get_obs_dict is WalkEnvV0's; its DEFAULT_OBS_KEYS are its own)
    "baoding": ("envs/myo/myochallenge/baoding_v1.py", "BaodingEnvV1"),
    "die": ("envs/myo/myochallenge/reorient_v0.py", "ReorientEnvV0"),
}


def _class(tree, name):
    return next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)


def _obs_keys(tree, cls):
    """Keys assigned by `obs_dict[<str>] = ...` in cls.get_obs_dict, each once, in source order (an assignment under `if` counts: a key the
    class defines for some models); a class without the method takes its first base class's."""
    fn = next((n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "get_obs_dict"), None)
    if fn is None:
        return _obs_keys(tree, _class(tree, cls.bases[0].id))
    hits = []
    for node in ast.walk(fn):
        if (isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Subscript) and isinstance(node.targets[0].value, ast.Name)
                and node.targets[0].value.id == "obs_dict" and isinstance(node.targets[0].slice, ast.Constant)):
            hits.append((node.lineno, node.col_offset, node.targets[0].slice.value))
    return list(dict.fromkeys(k for _, _, k in sorted(hits)))


def _default_keys(cls):
    node = next(n for n in cls.body if isinstance(n, ast.Assign) and n.targets[0].id == "DEFAULT_OBS_KEYS")
    return list(ast.literal_eval(node.value))


def parse(reference=REFERENCE):
    out = {}
    for task, (path, name) in CLASSES.items():
        with open(os.path.join(reference, path)) as f:
            tree = ast.parse(f.read())
        cls = _class(tree, name)
        out[task] = {"source": path, "class": name, "keys": _obs_keys(tree, cls), "default_obs_keys": _default_keys(cls)}
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--check"]
    doc = parse(args[0] if args else REFERENCE)
    if "--check" in sys.argv:
        assert doc == json.load(open(OUT)), "tests/golden/obs_terms.json is stale"
    else:
        with open(OUT, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    for task, d in doc.items():
        print(f"{task:8s} {d['class']:20s} {d['keys']}  {d['default_obs_keys']}")
