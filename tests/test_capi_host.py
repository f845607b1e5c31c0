"""Host-side checks that need no GPU: the C-ABI library loads and exports every symbol the header declares;
the product path fails loudly (no CPU fallback) when no MI355X is present; env registry mirrors the reference."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    from myosuite_mjx_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.LIB_PATH


HEADERS = ("myo_hip.h", "myo_hip_sensors.h", "myo_hip_rewards.h", "myo_hip_ppo.h", "myo_hip_forward.h")


def _header_text(name):
    """A public header without its comments."""
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))


def test_library_exports_every_declared_symbol(lib_path):
    names = sorted({n for h in HEADERS for n in re.findall(r"\b(myo_[a-z0-9_]+)\s*\(", _header_text(h))})
    assert len(names) >= 60 and "myo_ppo_learner_step" in names and "myo_forward" in names and "myo_episode_clear" in names
    lib = ctypes.CDLL(lib_path)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


# the kind of a C type as the binding has to spell it: scalar kinds by their ctypes class, every pointer as one kind
SCALAR_KINDS = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}


def _c_kind(decl):
    """Kind of a C parameter or return declaration (`const float* obs_dev`, `int B`, `myo_batch*`, `void`): "pointer", "void", or the
    ctypes class of its scalar type.  The parameter's name, if any, is dropped."""
    decl = " ".join(decl.replace("*", " * ").split())
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    assert words and (words[0] in SCALAR_KINDS or words == ["void"]) and len(words) <= 2, decl
    return "void" if words[0] == "void" else SCALAR_KINDS[words[0]]


def _ctypes_kind(t):
    """The same kind of a ctypes restype / argtypes entry."""
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    return t


def _header_prototypes():
    """{name: (return kind, [argument kinds])} of every function the five public headers declare."""
    protos = {}
    for h in HEADERS:
        for ret, name, args in re.findall(r"^[ \t]*((?:const\s+)?\w+[\s*]+)(myo_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", _header_text(h), flags=re.M):
            assert name not in protos, name
            args = [] if args.strip() == "void" else [a for a in args.split(",")]
            protos[name] = (_c_kind(ret), [_c_kind(a) for a in args])
    return protos


def test_binding_table_matches_the_header_prototypes():
    """capi.SIGNATURES against every prototype of the five public headers: the same names, and per function the same number of arguments, the
    same kind per argument (pointer / int / uint64_t / size_t / float / double; any pointer type matches c_void_p, c_char_p or POINTER(...))
    and the same return kind.  A c_int where the header says size_t or uint64_t fails here instead of truncating silently at run time."""
    from myosuite_mjx_amd import capi
    protos = _header_prototypes()
    assert len(protos) == 63 and protos["myo_sync"] == (ctypes.c_int, ["pointer"]) and protos["myo_model_free"] == ("void", ["pointer"])      # (the parser parses)
    assert protos["myo_reset"] == (ctypes.c_int, ["pointer", "pointer", ctypes.c_uint64, "pointer"]) and protos["myo_last_error"] == ("pointer", [])
    assert protos["myo_ppo_gae"][1][5:9] == [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    assert sorted(capi.SIGNATURES) == sorted(protos)
    wrong = {}
    for name, (ret, args) in protos.items():
        restype, argtypes = capi.SIGNATURES[name]
        bound = (_ctypes_kind(restype), [_ctypes_kind(t) for t in argtypes])
        if bound != (ret, args):
            wrong[name] = (bound, (ret, args))
    assert not wrong, wrong
    L = capi.lib()                              # and lib() has applied the table
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def _header_struct(name):
    """[(member, kind, array length or None)] of `typedef struct <name> { ... } <name>;`: a declaration is `type a, b[8], *c;`."""
    text = "".join(_header_text(h) for h in HEADERS)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
    members = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        base, first = re.fullmatch(r"((?:const )?\w+)\s*(.*)", decl).groups()
        for item in (x.strip() for x in first.split(",")):
            m = re.fullmatch(r"(\*?)\s*(\w+)(?:\[(\d+)\])?", item)
            assert m, decl
            members.append((m.group(2), _c_kind(base + (" *" if m.group(1) else "")), int(m.group(3)) if m.group(3) else None))
    return members


def _mirror_struct(cls):
    """The same list from a ctypes.Structure's _fields_."""
    out = []
    for member, t in cls._fields_:
        n = None
        if issubclass(t, ctypes.Array):
            t, n = t._type_, t._length_
        out.append((member, _ctypes_kind(t), n))
    return out


def _mirrors():
    from myosuite_mjx_amd import capi
    return {"myo_dims": capi.Dims, "myo_task_config": capi.TaskConfig, "myo_walk_config": capi.WalkConfig, "myo_track_config": capi.TrackConfig,
            "myo_ppo_config": capi.LearnerConfig}


def test_struct_mirrors_match_the_header_structs(tmp_path):
    """The five ctypes.Structure mirrors against the headers' typedef structs: member names, order, scalar kind and array length; and, with
    gcc, ctypes.sizeof against the C compiler's sizeof."""
    import shutil
    import subprocess
    for name, cls in _mirrors().items():
        parsed = _header_struct(name)
        assert len(parsed) >= 13 and parsed == _mirror_struct(cls), (name, [x for x in zip(parsed, _mirror_struct(cls)) if x[0] != x[1]])
    assert ("tip_site", ctypes.c_int, 8) in _header_struct("myo_task_config") and ("seed", ctypes.c_uint64, None) in _header_struct("myo_track_config")
    assert ("ref_robot_vel", "pointer", None) in _header_struct("myo_track_config")      # (the parser parses)
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "include/myo_hip.h"\n'
                   'int main(void) { printf("' + " ".join(["%zu"] * len(_mirrors())) + '\\n", ' + ", ".join(f"sizeof({n})" for n in _mirrors()) + "); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", ROOT, str(src), "-o", str(tmp_path / "sizes")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "sizes")]).split()]
    assert sizes == [ctypes.sizeof(cls) for cls in _mirrors().values()]


def _header_enums(hdr):
    """{name: value} of every enumerator of include/myo_hip.h: comments stripped, each `enum { ... }` body evaluated in order (an enumerator
    is `NAME`, `NAME = <int>` or `NAME = <expression over earlier names>`)."""
    values = {}
    for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)):
        nxt = 0
        for item in filter(None, (x.strip() for x in body.split(","))):
            name, _, expr = (x.strip() for x in item.partition("="))
            assert re.fullmatch(r"[A-Z][A-Z0-9_]*", name) and name not in values, item
            values[name] = eval(expr, {"__builtins__": {}}, dict(values)) if expr else nxt
            nxt = values[name] + 1
    return values


def test_capi_constants_equal_the_header_enums():
    """Every MYO_F_* / MYO_TASK_* / MYO_FLAG_* / MYO_ACTMAP_* value of the header is the capi constant of the same name, and INT_FIELDS is
    the set of fields whose header comment starts `[B][n] int32`."""
    from myosuite_mjx_amd import capi
    hdr = open(os.path.join(ROOT, "include", "myo_hip.h")).read()
    enums = _header_enums(hdr)
    assert enums["MYO_F_QPOS"] == 0 and enums["MYO_F_BODYPOS"] == enums["MYO_F_COUNT"] and enums["MYO_TASK_HOLD"] == 4    # (the parser parses)
    checked = {n: v for n, v in enums.items() if n.startswith(("MYO_F_", "MYO_TASK_", "MYO_FLAG_", "MYO_ACTMAP_"))}
    for prefix, known in (("MYO_F_", "MYO_F_CFRC"), ("MYO_TASK_", "MYO_TASK_DIE"), ("MYO_FLAG_", "MYO_FLAG_SCHED_TIMEOUT"), ("MYO_ACTMAP_", "MYO_ACTMAP_CTRLRANGE")):
        assert known in checked and sum(n.startswith(prefix) for n in checked) >= 5      # every family was found
    wrong = {n: (v, getattr(capi, n[4:], None)) for n, v in checked.items() if getattr(capi, n[4:], None) != v}
    assert not wrong, wrong
    extra = [n for n in dir(capi) if n.startswith(("F_", "TASK_", "FLAG_", "ACTMAP_")) and "MYO_" + n not in checked]
    assert not extra, extra                                                      # and capi names no id the header lacks
    fields = sorted(v for n, v in checked.items() if n.startswith("MYO_F_") and n != "MYO_F_COUNT")
    assert fields == list(range(enums["MYO_F_CFRC"] + 1))                       # the ids are dense: the library's field table has one row each
    documented = re.findall(r"\b(MYO_F_[A-Z_]+)\b[^,/]*,?\s*/\*\s*\[B\]\[[^\]]*\]\s*(int32)?", hdr)
    assert sorted(enums[n] for n, _ in documented) == fields                   # every field's comment was found, MYO_F_CFRC's included
    assert sorted(capi.INT_FIELDS) == sorted(enums[n] for n, i32 in documented if i32) and capi.F_FLAGS in capi.INT_FIELDS


def _documented_buffers(header, prefix):
    """{id: (dtype name, elements per item)} from the comments of an `enum { MYO_EP_* / MYO_FWD_* }`: `/* [B][n][3] ...`, `/* [B] uint8: ...`;
    a comment that names no type documents float32, a [B] one an item of no dimensions."""
    hdr = open(os.path.join(ROOT, "include", header)).read()
    enums = _header_enums(hdr)
    out = {}
    for name, dims, dtype in re.findall(r"\b(%s[A-Z_]+) = \d+,?\s*/\*\s*((?:\[[^\]]*\])+):?\s*(float32|int32|uint8)?" % prefix, hdr):
        dims = re.findall(r"\[([^\]]*)\]", dims)
        assert dims[0] == "B", name
        out[enums[name]] = (dtype or "float32", int(dims[-1]) if len(dims) > 1 else 0)
    return out, enums


def test_buffer_family_tables_say_what_the_headers_say():
    """capi's one statement of element type and per-env item shape per episode and forward buffer, against the comments of
    include/myo_hip_rewards.h and include/myo_hip_forward.h: uint8 for MYO_EP_FINISHED, int32 for MYO_EP_COUNT and MYO_FWD_NCON, float32 for
    the rest, [4] / [3] / [9] / [16] elements per item ([B] alone: a scalar per env), 16 words per contact record; what the family table
    hands out is that statement, and every dtype's typestr is one of the three a view can have."""
    from myosuite_mjx_amd import capi
    ep, ep_enums = _documented_buffers("myo_hip_rewards.h", "MYO_EP_")
    fwd, fwd_enums = _documented_buffers("myo_hip_forward.h", "MYO_FWD_")
    assert ep == {0: ("float32", 4), 1: ("float32", 4), 2: ("uint8", 0), 3: ("int32", 0)}                      # (the parser parses)
    assert len(fwd) == fwd_enums["MYO_FWD_COUNT"] == capi.FWD_COUNT == 9 and fwd[7] == ("int32", 0) and fwd[8] == ("float32", 16) and fwd[1] == ("float32", 9)
    for n, v in list(ep_enums.items()) + list(fwd_enums.items()):
        if n.startswith(("MYO_EP_", "MYO_FWD_")):
            assert getattr(capi, n[4:]) == v, n
    assert (capi.EP_FINISHED, capi.EP_COUNT, capi.FWD_NCON, capi.FWD_CONTACT) == (2, 3, 7, 8)
    assert capi.FWD_CONTACT_WORDS == 16 and "#define MYO_FWD_CONTACT_WORDS 16" in open(os.path.join(ROOT, "include", "myo_hip_forward.h")).read()
    for family, doc, dtypes, items in (("episode", ep, capi._EP_DTYPE, capi._EP_ITEM), ("forward", fwd, capi._FWD_DTYPE, capi._FWD_ITEM)):
        assert sorted(dtypes) == sorted(items) == sorted(doc), family
        for i, (dtype, n) in doc.items():
            assert np.dtype(dtypes[i]) == np.dtype(dtype) and int(np.prod(items[i])) == (n or 1) and (items[i] == ()) == (n == 0), (family, i)
            assert np.dtype(dtypes[i]).str in ("<f4", "<i4", "|u1"), (family, i)
            got_dtype, shape = capi.FAMILIES[family][2](3, i, lambda: 5 * (n or 1))                           # B = 3, rows of 5 items
            assert got_dtype is dtypes[i], (family, i)
            assert shape == ((3, *items[i]) if family == "episode" else ((3, 5, *items[i]) if items[i] else (3,))), (family, i, shape)
    assert capi._FWD_ITEM[capi.FWD_CONTACT] == (16,) and capi._FWD_ITEM[capi.FWD_XMAT] == (3, 3) and capi._EP_ITEM[capi.EP_LAST] == (4,)
    for f in range(capi.F_CFRC + 1):                                                                           # fields: int32 for INT_FIELDS, else float32
        dtype, shape = capi.FAMILIES["field"][2](3, f, lambda: 7)
        assert dtype is (np.int32 if f in capi.INT_FIELDS else np.float32) and shape == (3, 7) and np.dtype(dtype).str in ("<f4", "<i4")
    assert capi.FAMILIES["rwd"][2](3, None, lambda: 9) == (np.float32, (3, 9))


# capi name, value, and the text the header must spell it with (None: its place in a list gives the value).  Ids are appended, never
# renumbered: a feature that adds a field or a task adds its row at the end of its block, and changes no other row.
ABI_PINS = (
    ("F_METRICS", 23, None), ("F_BODYMASS", 24, None), ("F_BODYMASS_RANGE", 25, None),           # the tail of the myo_field list proper
    ("F_BODYPOS", 26, "MYO_F_BODYPOS = MYO_F_COUNT"), ("F_BODYPOS_RANGE", 27, None),             # ... the ids continue after MYO_F_COUNT
    ("F_BODYQUAT", 28, "MYO_F_BODYQUAT = MYO_F_BODYPOS_RANGE + 1"), ("F_BODYQUAT_RANGE", 29, None),
    ("TASK_HOLD", 4, None), ("TASK_STAND", 5, None), ("TASK_TRACK", 6, None),
    ("TASK_KEYTURN", 7, "MYO_TASK_KEYTURN = 7"), ("TASK_PEN", 8, "MYO_TASK_PEN = 8"), ("TASK_BAODING", 9, "MYO_TASK_BAODING = 9"),
    ("TASK_DIE", 10, "MYO_TASK_DIE = 10"),
)


def test_abi_numbering_is_append_only():
    """The numbers a client compiled against an older header relies on: the myo_field list proper and its end, the field ids that continue
    after MYO_F_COUNT, the task ids, and the layout of myo_task_config (new members go last).  Every per-feature ABI pin lives here."""
    from myosuite_mjx_amd import capi
    hdr = open(os.path.join(ROOT, "include", "myo_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = re.findall(r"^\s*(MYO_F_[A-Z_]+)", plain[plain.index("typedef enum myo_field"):plain.index("} myo_field;")], flags=re.M)
    assert names[-3:] == ["MYO_F_BODYMASS", "MYO_F_BODYMASS_RANGE", "MYO_F_COUNT"] and len(names) == 27
    assert names.index("MYO_F_METRICS") == 23 and names.index("MYO_F_BODYMASS") == 24 and names.index("MYO_F_BODYMASS_RANGE") == 25
    ext = plain[plain.index("} myo_field;"):plain.index("MYO_FLAG_BAD_STATE")]
    ext = re.findall(r"^\s*(MYO_F_[A-Z_]+(?: = MYO_F_COUNT)?)", ext, flags=re.M)
    assert ext == ["MYO_F_BODYPOS = MYO_F_COUNT", "MYO_F_BODYPOS_RANGE"]          # the ids continue after the list
    assert re.search(r"^\s*MYO_F_BODYQUAT_RANGE,", hdr, flags=re.M)
    for name, value, text in ABI_PINS:
        assert getattr(capi, name) == value, name
        assert text is None or text in hdr, text
    assert re.search(r"^\s*int quat_body;", hdr, flags=re.M) and capi.TaskConfig._fields_[-1] == ("quat_body", capi.C.c_int)
    assert len(capi.TaskConfig._fields_) == 25


def test_error_convention_without_gpu(lib_path, hand):
    """Bad arguments return negative codes with a message; without a GPU model upload raises (no silent fallback)."""
    import torch
    from myosuite_mjx_amd import capi
    L = capi.lib()
    assert L.myo_model_load(None, 0, 0, None) == -1 and b"bad arguments" in L.myo_last_error()
    h = ctypes.c_void_p()
    assert L.myo_model_load(b"XXXX" + bytes(32), 36, 0, ctypes.byref(h)) == -2
    if not torch.cuda.is_available():
        with pytest.raises(capi.MyoError):
            capi.HipModel(hand.blob(), 0)
        import myosuite_mjx_amd as myo
        with pytest.raises(capi.MyoError):
            myo.make("myoHandPoseFixed-v0", num_envs=2)


def test_product_does_not_import_oracle():
    """The shipped package must not reference the oracle (test infrastructure)."""
    pkg = os.path.join(ROOT, "myosuite_mjx_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "import oracle" not in src and "from oracle" not in src and "libmyo_oracle" not in src, f


def test_registry_matches_reference_specs():
    from myosuite_mjx_amd.envs import ASL_QPOS, HAND_POSE_FIXED, REGISTRY, UNSUPPORTED
    for k in ("myoHandPoseFixed-v0", "myoHandPoseRandom-v0", "myoHandReachFixed-v0", "myoHandReachRandom-v0", "myoHandPose3Fixed-v0"):
        assert k in REGISTRY and REGISTRY[k]["max_episode_steps"] == 100 and REGISTRY[k]["frame_skip"] == 10
    r = REGISTRY["myoHandPoseRandom-v0"]
    assert r["reset_type"] == "random" and r["target_type"] == "generate" and r["pose_thd"] == 0.7
    assert np.allclose(r["target_lo"], ASL_QPOS.min(0)) and np.allclose(r["target_hi"], ASL_QPOS.max(0))
    assert r["target_lo"][:3].tolist() == [0, 0, 0] and abs(r["target_hi"][21] - 1.571) < 1e-9
    f = REGISTRY["myoHandPoseFixed-v0"]
    assert np.allclose(f["target_lo"], HAND_POSE_FIXED) and f["reset_type"] == "init"
    rr = REGISTRY["myoHandReachRandom-v0"]
    assert rr["far_th"] == 0.034 and np.allclose(rr["target_lo"][:3], [-0.185, -0.577, 1.455]) and np.allclose(rr["target_hi"][:3], [-0.125, -0.517, 1.535])
    for tid, kind, sc in (("myoLegRoughTerrainWalk-v0", "rough", (0.0, 0.0)), ("myoLegHillyTerrainWalk-v0", "hilly", (0.63, 0.63)),
                          ("myoLegStairTerrainWalk-v0", "stairs", (2.5, 2.5))):      # envs/myo/myobase/__init__.py:462-520, walk_v0.py:569-597
        t = REGISTRY[tid]
        assert t["model"] == "myolegs_terrain" and t["terrain"] == kind and t["terrain_scalar"] == sc and t["knee_height"] == 0.61
        assert t["max_episode_steps"] == 1000 and t["weights"] == REGISTRY["myoLegWalk-v0"]["weights"] and tid not in UNSUPPORTED
    lw = REGISTRY["myoLegWalk-v0"]                               # envs/myo/myobase/__init__.py:443-459, walk_v0.py:203-209
    assert lw["model"] == "myolegs" and lw["max_episode_steps"] == 1000 and lw["frame_skip"] == 10 and lw["reset_type"] == "init"
    assert (lw["min_height"], lw["max_rot"], lw["hip_period"], lw["target_x_vel"], lw["target_y_vel"]) == (0.8, 0.8, 100, 0.0, 1.2)
    assert lw["weights"] == dict(vel_reward=5.0, done=-100.0, cyclic_hip=-10.0, ref_rot=10.0, joint_angle_rew=5.0)
    ff = REGISTRY["myoFingerPoseFixed-v0"]                       # envs/myo/myobase/__init__.py:222-236
    assert ff["model"] == "myofinger_v0" and ff["pose_thd"] == 0.35 and ff["target_lo"].tolist() == [0, 0, 0.75, 0.75]
    eb = REGISTRY["myoElbowPose1D6MRandom-v0"]                   # envs/myo/myobase/__init__.py:123-137
    assert eb["model"] == "myoelbow_1dof6muscles" and eb["pose_thd"] == 0.175 and eb["reset_type"] == "random"
    assert eb["target_lo"].tolist() == [0.0] and eb["target_hi"].tolist() == [2.27] and REGISTRY["myoElbowPose1D6MFixed-v0"]["target_lo"].tolist() == [2.0]
    fr = REGISTRY["myoFingerReachRandom-v0"]                     # envs/myo/myobase/__init__.py:94-105; far_th default reach_v0.py:47
    assert fr["tips"] == ("IFtip",) and fr["far_th"] == 0.35 and fr["target_lo"].tolist() == [0.1, -0.1, 0.1] and fr["target_hi"].tolist() == [0.27, 0.1, 0.3]
    assert "myoSarcElbowPose1D6MFixed-v0" in REGISTRY and "myoFatiFingerReachRandom-v0" in REGISTRY
    ls = REGISTRY["myoLegStandRandom-v0"]                        # envs/myo/myobase/__init__.py:424-441, walk_v0.py:15-21,105
    assert ls["max_episode_steps"] == 150 and ls["joint_random_range"] == (-0.2, 0.2) and ls["far_th"] == 0.44 and ls["near_th"] == 0.05
    assert ls["weights"] == dict(reach=1.0, bonus=4.0, penalty=50.0, act_reg=1.0) and ls["target_span"] == ((-0.05, -0.05, 0.0), (0.05, 0.05, 0.0))
    oh = REGISTRY["myoHandObjHoldFixed-v0"]                      # envs/myo/myobase/__init__.py:596-604, obj_hold_v0.py:16-20,96-97
    assert oh["max_episode_steps"] == 75 and oh["weights"] == dict(goal_dist=100.0, bonus=4.0, penalty=10.0, act_reg=0.0) and (oh["goal_th"], oh["drop_th"]) == (0.010, 0.300)
    ohr = REGISTRY["myoHandObjHoldRandom-v0"]                    # obj_hold_v0.py:121-140
    assert ohr["goal"] is None and ohr["goal_span"] == 0.030 and ohr["object_size"] == ((0.020,) * 3, (0.030,) * 3)
    assert "myoElbowPose1D6MExoRandom-v0" in UNSUPPORTED


def test_registry_numbers_against_reference_text():
    """The ASL table / fixed target are data copied from the reference registration; check them against the numbers of its text
    (tests/golden/ref_registration.json, tools/make_ref_registration.py)."""
    from myosuite_mjx_amd.envs import ASL_QPOS, HAND_POSE_FIXED
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_registration.json")))["myobase"]
    assert len(ref["ASL_qpos"]) == 10
    for k, row in ref["ASL_qpos"].items():
        assert np.allclose(np.array(row, float), ASL_QPOS[int(k)])
    assert np.allclose(np.array(ref["myoHandPoseFixed-v0_target"], float)[:23], HAND_POSE_FIXED)


def test_host_rng_twin_is_uniform():
    from myosuite_mjx_amd.shard import u01
    v = np.array([u01(7, a, 3) for a in range(4000)])
    assert 0 <= v.min() and v.max() < 1 and abs(v.mean() - 0.5) < 0.02 and abs(v.var() - 1 / 12) < 0.01
    assert u01(7, 5, 3) == u01(7, 5, 3) and u01(7, 5, 3) != u01(8, 5, 3)


def test_public_header_is_plain_c(tmp_path):
    """include/myo_hip.h is the drop-in boundary: it must compile as C99 (no torch / C++ types in the signatures) and as C++."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "hdr.c"
    src.write_text('#include "include/myo_hip.h"\nint main(void) { myo_task_config c; myo_walk_config w; myo_dims d; (void)c; (void)w; (void)d; return MYO_F_COUNT > 0 ? 0 : 1; }\n')
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", root, "-c", str(src), "-o", str(tmp_path / "a.o")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", root, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "b.o")])
