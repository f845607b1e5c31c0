"""Observation terms of the batched envs: term names and widths per task, the default selection, and the validation of the three
constructor parameters (`obs_keys`, `proprio_keys`, `obs_dict`) -- host arithmetic only, done before a model is loaded or a GPU is touched.

The terms are the keys of the reference's `get_obs_dict` for the task's env class, in its order (pose_v0.py, reach_v0.py, obj_hold_v0.py,
key_turn_v0.py, pen_v0.py, walk_v0.py ReachEnvV0 and WalkEnvV0, baoding_v1.py, reorient_v0.py); each carries its width as an expression of
the model's dimensions (`dims`).  The library builds its table from each task's row record (csrc/myo_task_<name>.h; capi.obs_term_table
reads it without a GPU): tests/test_obs_terms_host.py holds the names and widths here, and the default keys as the row's blocks in order,
to it by value for every registered id; tests/golden/obs_terms.json pins the names and the default keys to the reference's text."""
from __future__ import annotations

# (key, width): an expression of nq, nv, nu, na (muscles), ntip (reach tips) and pose_act (na, or nq for a model without muscles: PoseEnvV0
# fills `act` with zeros_like(qpos) then).  A width of 0 means the model lacks the term (`act` without muscles)
OBS_TERMS = {
    "pose": (("time", "1"), ("qpos", "nq"), ("qvel", "nv"), ("act", "pose_act"), ("pose_err", "nq")),
    "reach": (("time", "1"), ("qpos", "nq"), ("qvel", "nv"), ("act", "na"), ("tip_pos", "3 * ntip"), ("target_pos", "3 * ntip"),
              ("reach_err", "3 * ntip")),
    "hold": (("time", "1"), ("hand_qpos", "nq - 7"), ("hand_qvel", "nv - 6"), ("obj_pos", "3"), ("obj_err", "3"), ("act", "na")),
    "keyturn": (("time", "1"), ("hand_qpos", "nq - 1"), ("hand_qvel", "nv - 1"), ("key_qpos", "1"), ("key_qvel", "1"), ("IFtip_approach", "3"),
                ("THtip_approach", "3"), ("act", "na")),
    "pen": (("time", "1"), ("hand_jnt", "nq - 6"), ("obj_pos", "3"), ("obj_des_pos", "3"), ("obj_vel", "6"), ("obj_rot", "3"), ("obj_des_rot", "3"),
            ("obj_err_pos", "3"), ("obj_err_rot", "3"), ("act", "na")),
    "walk": (("t", "1"), ("time", "1"), ("qpos_without_xy", "nq - 2"), ("qvel", "nv"), ("com_vel", "2"), ("torso_angle", "4"), ("feet_heights", "2"),
             ("height", "1"), ("feet_rel_positions", "6"), ("phase_var", "1"), ("muscle_length", "nu"), ("muscle_velocity", "nu"),
             ("muscle_force", "nu"), ("act", "nu")),
    "baoding": (("time", "1"), ("hand_pos", "nq - 14"), ("object1_pos", "3"), ("object2_pos", "3"), ("object1_velp", "3"), ("object2_velp", "3"),
                ("target1_pos", "3"), ("target2_pos", "3"), ("target1_err", "3"), ("target2_err", "3"), ("act", "na")),
    "die": (("time", "1"), ("hand_qpos_noMD5", "nq - 7"), ("hand_qpos", "nq - 6"), ("hand_qvel", "nv - 6"), ("obj_pos", "3"), ("goal_pos", "3"),
            ("pos_err", "3"), ("obj_rot", "3"), ("goal_rot", "3"), ("rot_err", "3"), ("act", "na")),
}
OBS_TERMS["stand"] = OBS_TERMS["reach"]        # walk_v0.py's ReachEnvV0 repeats reach_v0.py's get_obs_dict (ntip = 1)
# the env classes' DEFAULT_OBS_KEYS
DEFAULT_OBS_KEYS = {
    "pose": ("qpos", "qvel", "pose_err"),
    "reach": ("qpos", "qvel", "tip_pos", "reach_err"),
    "stand": ("qpos", "qvel", "tip_pos", "reach_err"),
    "hold": ("hand_qpos", "hand_qvel", "obj_pos", "obj_err"),
    "keyturn": ("hand_qpos", "hand_qvel", "key_qpos", "key_qvel", "IFtip_approach", "THtip_approach"),
    "pen": ("hand_jnt", "obj_pos", "obj_vel", "obj_rot", "obj_des_rot", "obj_err_pos", "obj_err_rot"),
    "walk": ("qpos_without_xy", "qvel", "com_vel", "torso_angle", "feet_heights", "height", "feet_rel_positions", "phase_var", "muscle_length",
             "muscle_velocity", "muscle_force"),
    "baoding": ("hand_pos", "object1_pos", "object1_velp", "object2_pos", "object2_velp", "target1_pos", "target2_pos", "target1_err", "target2_err"),
    "die": ("hand_qpos_noMD5", "hand_qvel", "obj_pos", "goal_pos", "pos_err", "obj_rot", "goal_rot", "rot_err"),
}
# BaseV0._setup (base_v0.py:34-38) appends `act` to obs_keys when the model has muscles and the list does not name it.  The canonical rows of
# these two tasks (csrc/myo_task_baoding.h, myo_task_die.h) carry no act block, and the selection follows the canonical row: `act` is a
# term of their tables and may be named, but it is not appended
NO_ACT_APPENDED = ("baoding", "die")


class Selection:
    """What `resolve` returns: obs_keys (None: the task's default keys, completed once the model is known) and proprio_keys (None: none)."""

    def __init__(self, task, obs_keys, proprio_keys):
        self.task, self.obs_keys, self.proprio_keys = task, obs_keys, proprio_keys


def term_names(task):
    return tuple(k for k, _ in OBS_TERMS[task])


def dims(m, spec):
    """The dimensions the width expressions read, of model `m` for the registry entry `spec`."""
    na = int(m.n_muscle)
    ntip = len(spec["tips"]) if spec["task"] == "reach" else 1
    return dict(nq=int(m.nq), nv=int(m.nv), nu=int(m.nu), na=na, ntip=ntip, pose_act=na if na > 0 else int(m.nq))


def widths(task, d):
    """{key: width} of the task's terms for the dimensions `d`, in table order."""
    return {k: int(eval(w, {"__builtins__": {}}, d)) for k, w in OBS_TERMS[task]}


def with_act(task, keys, na):
    """base_v0.py:34-38: `act` joins the keys of a model with muscles (see NO_ACT_APPENDED)."""
    keys = tuple(keys)
    return keys + ("act",) if na > 0 and "act" not in keys and task not in NO_ACT_APPENDED else keys


def default_keys(task, na):
    return with_act(task, DEFAULT_OBS_KEYS[task], na)


def _check(env_id, task, keys, what):
    names = term_names(task)
    for k in keys:
        if k not in names:
            raise KeyError(f"{env_id}: {what} names {k!r}, which is no key of the {task} task's obs_dict {names}")
    return tuple(keys)


def resolve(env_id, spec, obs_keys=None, proprio_keys=None, obs_dict=False):
    """What BatchedMyoEnv does with its three observation parameters: None when none is given (nothing is allocated, no launch is added),
    else a Selection.  A key may repeat (the reference concatenates blindly); an unknown key raises KeyError, an empty obs_keys ValueError;
    proprio_keys gets no `act` appended (env_base.py:512-531) and a single string is one key (env_base.py:152-155)."""
    if obs_keys is None and proprio_keys is None and not obs_dict:
        return None
    task = spec["task"]
    if obs_keys is not None:
        if isinstance(obs_keys, str):
            raise TypeError(f"{env_id}: obs_keys must be a list of keys, got the string {obs_keys!r}")
        obs_keys = _check(env_id, task, obs_keys, "obs_keys")
        if not obs_keys:
            raise ValueError(f"{env_id}: obs_keys is empty")
    if proprio_keys is not None:
        proprio_keys = _check(env_id, task, [proprio_keys] if isinstance(proprio_keys, str) else proprio_keys, "proprio_keys")
    return Selection(task, obs_keys, proprio_keys)


def obsvec2obsdict(obs, obs_keys, width):
    """{key: obs[..., its columns]} of a row [..., sum of the keys' widths] built from `obs_keys` (numpy or torch: slicing only).  A key
    that repeats maps to its last occurrence, as a dict does."""
    out, at = {}, 0
    for k in obs_keys:
        out[k] = obs[..., at:at + width[k]]
        at += width[k]
    if at != obs.shape[-1]:
        raise ValueError(f"obsvec2obsdict: the row has {obs.shape[-1]} columns, the keys {tuple(obs_keys)} make {at}")
    return out


def slices(keys, width):
    """{key: slice} of each key's columns in the concatenation of `keys` (a repeated key: its last occurrence)."""
    out, at = {}, 0
    for k in keys:
        out[k] = slice(at, at + width[k])
        at += width[k]
    return out
