"""ctypes binding of libmyo_hip.so (include/myo_hip.h).  There is no CPU fallback: if the
library is missing or no MI355X is visible, loading / model upload raises."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MYO_HIP_LIB") or os.path.join(_HERE, "libmyo_hip.so")
SRC_PATH = os.path.join(_HERE, "csrc", "myo_hip.hip")

# field ids (myo_field and the enums that continue it in include/myo_hip.h; tests/test_capi_host.py compares every constant here with the header)
(F_QPOS, F_QVEL, F_ACT, F_CTRL, F_WARMSTART, F_TIME, F_TARGET, F_OBS, F_REWARD, F_DONE, F_SOLVED, F_FLAGS, F_DIAG,
 F_QACC, F_TENLEN, F_ACTFORCE, F_SITEXPOS, F_ELAPSED, F_ACTION, F_FATIGUE, F_HFIELD, F_GEOMSIZE, F_LINKX, F_METRICS,
 F_BODYMASS, F_BODYMASS_RANGE, F_BODYPOS, F_BODYPOS_RANGE,
 F_BODYQUAT, F_BODYQUAT_RANGE,              # per-env orientation of one world-welded body (TaskConfig.quat_body selects it)
 F_SENSORDATA, F_CFRC) = range(32)          # touch sensors [B, nsensor] and contact forces [B, (nsensor + 1) * 3] (HipBatch.enable_sensors)
F_COUNT = F_BODYPOS                         # size of the myo_field list proper
INT_FIELDS = (F_FLAGS, F_DIAG, F_ELAPSED)
# width of the per-env override fields as (per body, constant): known without asking for their device pointer, which would start the override
_OVERRIDE_WIDTH = {F_BODYMASS: (1, 0), F_BODYMASS_RANGE: (2, 0), F_BODYPOS: (0, 3), F_BODYPOS_RANGE: (0, 6), F_BODYQUAT: (0, 4), F_BODYQUAT_RANGE: (0, 6)}
BENCH_OBS, BENCH_FRESH_ACTIONS, BENCH_AUTORESET = 1, 2, 4
ACTMAP_NONE, ACTMAP_MUSCLE_SIGMOID, ACTMAP_SIGMOID_FATIGUE, ACTMAP_SIGMOID_REAFFERENTATION, ACTMAP_CTRLRANGE = 0, 1, 2, 3, 4
TASK_NONE, TASK_POSE, TASK_REACH, TASK_WALK, TASK_HOLD, TASK_STAND, TASK_TRACK, TASK_KEYTURN, TASK_PEN, TASK_BAODING, TASK_DIE = range(11)
FLAG_BAD_STATE, FLAG_BAD_QACC, FLAG_CONTACT_OVERFLOW, FLAG_CAND_OVERFLOW, FLAG_SCHED_TIMEOUT = 1, 2, 4, 8, 16
# reward terms and episode statistics (include/myo_hip_rewards.h): what MYO_F_REWARD holds, and the ids of the episode buffers with their dtypes
RWD_DENSE, RWD_SPARSE = 0, 1
EP_RUNNING, EP_LAST, EP_FINISHED, EP_COUNT = range(4)
_EP_DTYPE = {EP_RUNNING: np.float32, EP_LAST: np.float32, EP_FINISHED: np.uint8, EP_COUNT: np.int32}
_EP_ITEM = {EP_RUNNING: (4,), EP_LAST: (4,), EP_FINISHED: (), EP_COUNT: ()}
# observation terms (include/myo_hip_obs.h): the three rows of a batch with the terms on
OBS_TERMS, OBS_SELECTED, OBS_PROPRIO = range(3)
# forward pass (include/myo_hip_forward.h): buffer ids, words of a contact record, and the per-item shape of each buffer
FWD_XPOS, FWD_XMAT, FWD_XIPOS, FWD_SITE_XPOS, FWD_SITE_XMAT, FWD_GEOM_XPOS, FWD_GEOM_XMAT, FWD_NCON, FWD_CONTACT = range(9)
FWD_COUNT = 9
FWD_CONTACT_WORDS = 16
FWD_NAMES = {"xpos": FWD_XPOS, "xmat": FWD_XMAT, "xipos": FWD_XIPOS, "site_xpos": FWD_SITE_XPOS, "site_xmat": FWD_SITE_XMAT,
             "geom_xpos": FWD_GEOM_XPOS, "geom_xmat": FWD_GEOM_XMAT, "ncon": FWD_NCON, "contact": FWD_CONTACT}
_FWD_ITEM = {FWD_XPOS: (3,), FWD_XMAT: (3, 3), FWD_XIPOS: (3,), FWD_SITE_XPOS: (3,), FWD_SITE_XMAT: (3, 3), FWD_GEOM_XPOS: (3,),
             FWD_GEOM_XMAT: (3, 3), FWD_NCON: (), FWD_CONTACT: (FWD_CONTACT_WORDS,)}
_FWD_DTYPE = {which: np.int32 if which == FWD_NCON else np.float32 for which in _FWD_ITEM}


class Dims(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nq", "nv", "nu", "na", "nbody", "ntendon", "nsite", "nlink", "obs_dim",
                                       "env_lds_bytes", "lanes_per_env", "ncon_max")] + [("timestep", C.c_float)]


class TaskConfig(C.Structure):
    _fields_ = [("task", C.c_int), ("frame_skip", C.c_int), ("reset_random", C.c_int), ("target_generate", C.c_int),
                ("ntarget", C.c_int), ("ntip", C.c_int), ("tip_site", C.c_int * 8),
                ("pose_thd", C.c_float), ("far_th", C.c_float), ("near_th", C.c_float),
                ("w_pose", C.c_float), ("w_bonus", C.c_float), ("w_act_reg", C.c_float), ("w_penalty", C.c_float),
                ("w_reach", C.c_float),
                ("target_lo", C.POINTER(C.c_float)), ("target_hi", C.POINTER(C.c_float)), ("init_qpos", C.POINTER(C.c_float)),
                ("reset_noise_lo", C.POINTER(C.c_float)), ("reset_noise_hi", C.POINTER(C.c_float)),
                ("reset_clip_lo", C.POINTER(C.c_float)), ("reset_clip_hi", C.POINTER(C.c_float)),
                ("init_qvel", C.POINTER(C.c_float)), ("tip_lpos", C.c_float * 3), ("quat_body", C.c_int)]


class WalkConfig(C.Structure):
    """ctypes mirror of `myo_walk_config` (include/myo_hip.h)."""
    _fields_ = [("frame_skip", C.c_int), ("hip_period", C.c_int), ("min_height", C.c_float), ("max_rot", C.c_float),
                ("target_x_vel", C.c_float), ("target_y_vel", C.c_float), ("target_rot", C.c_float * 4),
                ("body_talus_l", C.c_int), ("body_talus_r", C.c_int), ("body_pelvis", C.c_int), ("body_torso", C.c_int),
                ("qadr_hip_flexion_l", C.c_int), ("qadr_hip_flexion_r", C.c_int), ("qadr_joint_angle", C.c_int * 4),
                ("w_vel_reward", C.c_float), ("w_done", C.c_float), ("w_cyclic_hip", C.c_float), ("w_ref_rot", C.c_float),
                ("w_joint_angle_rew", C.c_float), ("init_qpos", C.POINTER(C.c_float)), ("init_qvel", C.POINTER(C.c_float)),
                ("knee_height", C.c_float), ("terrain", C.c_int), ("terrain_scalar_lo", C.c_float), ("terrain_scalar_hi", C.c_float),
                ("init_qpos_alt", C.POINTER(C.c_float)), ("init_qvel_alt", C.POINTER(C.c_float)), ("reset_noise_std", C.c_float)]


TERRAIN_NONE, TERRAIN_ROUGH, TERRAIN_HILLY, TERRAIN_STAIRS = 0, 1, 2, 3


class TrackConfig(C.Structure):
    """ctypes mirror of `myo_track_config` (include/myo_hip.h)."""
    _fields_ = [("n_frames", C.c_int), ("ref_type", C.c_int), ("horizon", C.c_int), ("robot_horizon", C.c_int), ("object_horizon", C.c_int),
                ("robot_dim", C.c_int), ("object_dim", C.c_int), ("motion_extrapolation", C.c_int), ("interpolation_linear", C.c_int),
                ("motion_start_time", C.c_double),
                ("ref_time", C.POINTER(C.c_double)), ("ref_robot", C.POINTER(C.c_double)), ("ref_robot_vel", C.POINTER(C.c_double)),
                ("ref_object", C.POINTER(C.c_double)),
                ("init_qpos", C.POINTER(C.c_float)), ("ctrl_lo", C.POINTER(C.c_float)), ("ctrl_hi", C.POINTER(C.c_float)),
                ("object_link", C.c_int), ("wrist_link", C.c_int),
                ("object_ipos", C.c_float * 3), ("object_imat", C.c_float * 9), ("wrist_ipos", C.c_float * 3),
                ("lift_z", C.c_float), ("obj_err_scale", C.c_float), ("base_err_scale", C.c_float), ("lift_bonus_mag", C.c_float),
                ("qpos_reward_weight", C.c_float), ("qpos_err_scale", C.c_float), ("qvel_reward_weight", C.c_float), ("qvel_err_scale", C.c_float),
                ("obj_fail_thresh", C.c_float), ("base_fail_thresh", C.c_float), ("qpos_fail_thresh", C.c_float),
                ("terminate_obj_fail", C.c_int), ("terminate_pose_fail", C.c_int),
                ("w_pose", C.c_float), ("w_object", C.c_float), ("w_bonus", C.c_float), ("w_penalty", C.c_float),
                ("autoreset", C.c_int), ("max_episode_steps", C.c_int), ("seed", C.c_uint64), ("flavour", C.c_int)]


class LearnerConfig(C.Structure):
    """ctypes mirror of `myo_ppo_config` (include/myo_hip_ppo.h)."""
    _fields_ = [("obs_dim", C.c_int), ("act_dim", C.c_int), ("policy_nlayers", C.c_int), ("policy_out", C.c_int * 8),
                ("value_nlayers", C.c_int), ("value_out", C.c_int * 8), ("max_unroll", C.c_int), ("max_minibatch", C.c_int),
                ("learning_rate", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("adam_eps", C.c_double),
                ("discounting", C.c_float), ("gae_lambda", C.c_float), ("clipping_epsilon", C.c_float), ("entropy_cost", C.c_float),
                ("reward_scaling", C.c_float), ("normalize_advantage", C.c_int)]


# Every function of the five public headers: name -> (restype, argtypes), applied once by lib().  tests/test_capi_host.py parses the headers'
# prototypes and struct definitions and compares them with this table and with the mirrors above.  Handles (myo_model*, myo_batch*,
# myo_policy*, myo_ppo_learner*), streams and device pointers travel as c_void_p.
_V, _I, _U64, _SZ, _STR = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, C.c_char_p
_pV, _pI, _pF, _pD, _ppF = C.POINTER(_V), C.POINTER(_I), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.POINTER(C.c_float))
_BUF = [_pV, C.POINTER(_SZ), C.POINTER(_SZ)]       # the (device pointer, pitch, width) out-arguments of a buffer lookup
SIGNATURES = {
    # include/myo_hip.h
    "myo_last_error": (_STR, []),
    "myo_version": (_I, []),
    "myo_model_load": (_I, [_STR, _SZ, _I, _pV]),
    "myo_model_free": (None, [_V]),
    "myo_model_dims": (_I, [_V, C.POINTER(Dims)]),
    "myo_model_set_switch": (_I, [_V, _I, _I, _I]),
    "myo_batch_create": (_I, [_V, _I, _pV]),
    "myo_batch_free": (None, [_V]),
    "myo_batch_size": (_I, [_V]),
    "myo_batch_configure": (_I, [_V, C.POINTER(TaskConfig)]),
    "myo_batch_configure_walk": (_I, [_V, C.POINTER(WalkConfig)]),
    "myo_batch_configure_track": (_I, [_V, C.POINTER(TrackConfig)]),
    "myo_batch_set_condition": (_I, [_V, _I, _I, _I]),
    "myo_batch_set_fatigue_reset": (_I, [_V, _I, _V]),
    "myo_batch_set_geom_override": (_I, [_V, _I, _pF, _pF]),
    "myo_batch_field": (_I, [_V, _I, *_BUF]),
    "myo_batch_read": (_I, [_V, _I, _V, _SZ]),
    "myo_batch_write": (_I, [_V, _I, _V, _SZ]),
    "myo_reset": (_I, [_V, _V, _U64, _V]),
    "myo_set_state": (_I, [_V, _V, _V, _V, _V, _V]),
    "myo_step": (_I, [_V, _V, _I, _I, _V]),
    "myo_obs": (_I, [_V, _V]),
    "myo_obs_only": (_I, [_V, _V]),
    "myo_obs_reset_only": (_I, [_V, _V]),
    "myo_autoreset": (_I, [_V, _I, _U64, _V]),
    "myo_set_env_offset": (_I, [_V, _I]),
    "myo_status": (_I, [_V, _V]),
    "myo_random_action": (_I, [_V, _V, _U64, _U64, _I, _V]),
    "myo_sync": (_I, [_V]),
    "myo_set_balance": (_I, [_V, _I]),
    "myo_set_lanes": (_I, [_I]),
    "myo_read_stamps": (_I, [_V, _V, _I]),
    "myo_bench_rollout": (_I, [_V, _I, _I, _U64, _I, _I, _V, _pF]),
    "myo_bench_last_kernel_ms": (_I, [_V, _pF]),
    "myo_probe_valu": (_I, [_I, _I, _I, _pD, _pI]),
    "myo_bench_last_kernel_name": (_STR, [_V]),
    "myo_policy_load": (_I, [_I, _I, _I, _I, _pI, _V, _V, _pV, _pV, _pV]),
    "myo_policy_free": (None, [_V]),
    "myo_policy_act": (_I, [_V, _V, _I, _V, _I, _U64, _U64, _I, _V]),
    # include/myo_hip_sensors.h
    "myo_model_nsensor": (_I, [_V]),
    "myo_batch_enable_sensors": (_I, [_V]),
    # include/myo_hip_rewards.h
    "myo_batch_rwd_ncol": (_I, [_V]),
    "myo_batch_rwd_name": (_STR, [_V, _I]),
    "myo_batch_enable_rewards": (_I, [_V, _pF, _I, _I]),
    "myo_batch_rwd_row": (_I, [_V, *_BUF]),
    "myo_batch_rwd_read": (_I, [_V, _V, _SZ]),
    "myo_batch_enable_episode_stats": (_I, [_V]),
    "myo_batch_episode_buffer": (_I, [_V, _I, *_BUF]),
    "myo_batch_episode_read": (_I, [_V, _I, _V, _SZ]),
    "myo_episode_update": (_I, [_V, _I, _V]),
    "myo_episode_clear": (_I, [_V, _V]),
    # include/myo_hip_forward.h
    "myo_model_forward_dims": (_I, [_V, _pI, _pI, _pI, _pI]),
    "myo_forward": (_I, [_V, _V]),
    "myo_forward_buffer": (_I, [_V, _I, *_BUF]),
    "myo_forward_read": (_I, [_V, _I, _V, _SZ]),
    "myo_forward_host_tables": (_I, [_STR, _SZ, _I, _V, _SZ, _pI]),
    # include/myo_hip_ppo.h
    "myo_policy_update": (_I, [_V, _V, _V, _pV, _pV, _I, _V]),
    "myo_policy_sample": (_I, [_V, _V, _I, _V, _V, _V, _U64, _U64, _I, _V]),
    "myo_ppo_gae": (_I, [_V, _V, _V, _V, _V, _I, _I, C.c_float, C.c_float, _V, _V, _V]),
    "myo_ppo_learner_create": (_I, [_I, C.POINTER(LearnerConfig), _ppF, _ppF, _ppF, _ppF, _pV]),
    "myo_ppo_learner_free": (None, [_V]),
    "myo_ppo_learner_step": (_I, [_V, _V, _V, _V, _V, _V, _V, _I, _I, _V, _I, _V, _V, _V, _V, _V]),
    "myo_ppo_learner_tensor": (_I, [_V, _I, _I, _I, _I, _pV, C.POINTER(_SZ)]),
}

# include/myo_hip_obs.h, in a table of its own: SIGNATURES stays the table of the five core headers.  lib() applies both
OBS_SIGNATURES = {
    "myo_batch_obs_nterm": (_I, [_V]),
    "myo_batch_obs_term_name": (_STR, [_V, _I]),
    "myo_batch_obs_term_width": (_I, [_V, _I]),
    "myo_obs_term_table": (_I, [_I] * 8 + [C.POINTER(_STR), _pI, _pI, _pI]),
    "myo_batch_enable_obs_terms": (_I, [_V, _pI, _I, _pI, _I]),
    "myo_batch_obs_buffer": (_I, [_V, _I, *_BUF]),
    "myo_batch_obs_read": (_I, [_V, _I, _V, _SZ]),
}


# -mllvm -disable-machine-licm: the post-ISel loop-invariant code motion hoists constant materialisations (polynomial coefficients, masks) out
# of the 10-substep loop into the kernel prologue, where a dozen of them stay live in VGPRs for the whole kernel and push other values into
# scratch memory; with the pass off the headline kernel needs no register spill at all (35 before; tests/test_kernel_resources.py)
# -fno-slp-vectorize: the SLP vectoriser pairs float operations into v_pk_fma_f32 / v_pk_mul_f32 (1 064 of them in the headline kernel), which need
# 64-bit aligned register pairs: the static VALU count stays the same (the packed instructions are paid for in v_mov shuffles: 1 783 against 1 083
# moves), the register pressure rises (MyoLeg kernel 227 -> 213 VGPRs without it, and the headline kernel's 127 turn into spills with any small
# change), and the kernel is slower: measured +5.3 % at 4096 envs, +4.1 % at 32768 envs without the pass
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O2", "-std=c++17", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=on",
               "-fgpu-flush-denormals-to-zero", "-mllvm", "-disable-machine-licm", "-fno-slp-vectorize", *os.environ.get("MYO_HIPCC_EXTRA", "").split()]


def build_library(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -> libmyo_hip.so next to this file (cross-compiles without a GPU)."""
    csrc = os.path.dirname(SRC_PATH)
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    inc = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
    newest = max(newest, *(os.path.getmtime(os.path.join(inc, f)) for f in os.listdir(inc)))
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= newest:
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # -ffp-contract=on: multiply-adds are fused only where one source expression spells them, not across statements at the optimiser's
    # discretion (hipcc's default "fast").  Two effects, both measured: every template instantiation of the step kernel then rounds
    # identically (a scheduled full-batch launch is bit-identical to one-wave-per-env shards), and the MyoHand kernel is 6 % faster
    # -O2 rather than -O3: measured +0.8 % (hand) to +2 % (finger), neutral on the leg kernels
    # -fgpu-flush-denormals-to-zero: float32 division then lowers to v_rcp_f32 + multiply instead of the frexp / ldexp scaling that keeps
    # denormal quotients exact (about 100 divisions per substep: +3.5 % on the hand kernel, all parity tests unchanged; nothing in this
    # physics lives below 1e-38, the kernels' own guards sit at 1e-15)
    cmd = [hipcc, *HIPCC_FLAGS, "-shared", "-fPIC", "-o", LIB_PATH, SRC_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


def build_diagnostic(variant, force=False, verbose=False):
    """Diagnostic builds of the same sources next to libmyo_hip.so (selected at run time with MYO_HIP_LIB=<path>):
    "poison" (-DMYO_POISON=1): every LDS word of an env's slice starts as a NaN and the scratch memory of every wave slot is filled with NaNs
    before each step launch, so a read of a word the launch never wrote -- or a kernel whose addressing went wrong -- shows up in the parity
    tests (tests/test_gpu_poison.py runs them against this build);
    "stamps" (-DMYO_STAMPS=1): clock64 per stage (tools/gpu_stamps.py)."""
    flag = {"poison": "-DMYO_POISON=1", "stamps": "-DMYO_STAMPS=1"}[variant]
    out = os.path.join(os.path.dirname(LIB_PATH), f"libmyo_hip_{variant}.so")
    csrc = os.path.dirname(SRC_PATH)
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    if not force and os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *HIPCC_FLAGS, flag, "-shared", "-fPIC", "-o", out, SRC_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                               "(the HIP stepper has no CPU fallback)")
        # PyTorch-ROCm bundles its own HIP runtime.  Two HIP runtimes in one process do not share the device (the second one
        # reports "no HIP GPUs"), so when torch is installed let it load its runtime first: libmyo_hip.so's libamdhip64
        # dependency then resolves to that same, already loaded, library whichever side touches the GPU first.
        if not os.environ.get("MYO_NO_TORCH"):      # MYO_NO_TORCH=1: torch-free processes (profiling drivers) skip the import
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in {**SIGNATURES, **OBS_SIGNATURES}.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


class MyoError(RuntimeError):
    pass


def obs_term_table(task, nq, nv, nu, na, ntip, pose_act):
    """The library's observation-term table of task id `task` for a model of these dimensions, without a batch or a GPU:
    (((name, width, offset in the canonical row or -1), ...), width of the canonical row)."""
    name, width, offset, dim = _STR(), _I(), _I(), _I()
    ask = lambda k: lib().myo_obs_term_table(task, nq, nv, nu, na, ntip, pose_act, k, C.byref(name), C.byref(width), C.byref(offset), C.byref(dim))
    terms = []
    for k in range(ask(-1)):
        ask(k)
        terms.append((name.value.decode(), width.value, offset.value))
    return tuple(terms), dim.value


def _chk(rc):
    if rc != 0:
        raise MyoError(f"libmyo_hip error {rc}: {lib().myo_last_error().decode()}")


def _f32(a):
    return np.ascontiguousarray(a, np.float32) if a is not None else None


def _ptr(a, ctype=C.c_float):
    """Pointer to a contiguous array's data (None stays NULL); the caller keeps the array alive across the library call."""
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


# ---- device buffers: the one lookup, host copy and zero-copy view every buffer family goes through (objects.py and ppo.py use them too)
def buffer_lookup(fn, *args):
    """Call a lookup `fn(*args, void**, size_t*, size_t*)`: (device pointer, pitch, width), the last two in elements per env row."""
    p, pitch, width = C.c_void_p(), C.c_size_t(), C.c_size_t()
    _chk(fn(*args, C.byref(p), C.byref(pitch), C.byref(width)))
    return p.value, pitch.value, width.value


def host_read(fn, *args, shape, dtype, sized=True):
    """A fresh host array filled by a read `fn(*args, void* host[, size_t nbytes])`."""
    out = np.empty(shape, dtype)
    _chk(fn(*args, out.ctypes.data, out.nbytes) if sized else fn(*args, out.ctypes.data))
    return out


class _DevArray:
    """__cuda_array_interface__ holder so torch can view library-owned device memory without a copy."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
        self._owner = owner


def device_view(torch, ptr, shape, dtype, owner, device):
    """Zero-copy torch tensor over library-owned device memory; `owner` (the batch, the learner) stays alive as long as the tensor."""
    return torch.as_tensor(_DevArray(ptr, shape, np.dtype(dtype).str, owner), device=f"cuda:{device}")


# The buffer families of a batch: (lookup function, read function, spec).  spec(B, id, width) -> (dtype, shape) is the one statement of a
# family's element type and per-env item shape; width() gives the elements per env row and is called only where the shape depends on it
FAMILIES = {
    "field": ("myo_batch_field", "myo_batch_read", lambda B, f, width: (np.int32 if f in INT_FIELDS else np.float32, (B, width()))),
    "rwd": ("myo_batch_rwd_row", "myo_batch_rwd_read", lambda B, _, width: (np.float32, (B, width()))),
    "episode": ("myo_batch_episode_buffer", "myo_batch_episode_read", lambda B, which, width: (_EP_DTYPE[which], (B, *_EP_ITEM[which]))),
    "obs": ("myo_batch_obs_buffer", "myo_batch_obs_read", lambda B, _, width: (np.float32, (B, width()))),
    "forward": ("myo_forward_buffer", "myo_forward_read", lambda B, which, width: (
        _FWD_DTYPE[which], (B, width() // int(np.prod(_FWD_ITEM[which])), *_FWD_ITEM[which]) if _FWD_ITEM[which] else (B,))),
}


class HipModel:
    """Device-resident model (mjx.put_model counterpart, mjx/play.py:10)."""

    def __init__(self, blob: bytes, device: int = 0):
        self.h = C.c_void_p()
        _chk(lib().myo_model_load(blob, len(blob), device, C.byref(self.h)))
        self.dims = Dims()
        _chk(lib().myo_model_dims(self.h, C.byref(self.dims)))
        self.device = device

    @property
    def nsensor(self):
        return int(lib().myo_model_nsensor(self.h))

    def set_switch(self, disable_contact=0, disable_limit=0, disable_ellipsoid=0):
        _chk(lib().myo_model_set_switch(self.h, disable_contact, disable_limit, disable_ellipsoid))

    def forward_dims(self):
        """(nbody, nsite, ngeom, ncon_max) of the forward pass's buffers; MyoError for a model without one (generic lanes kernel)."""
        v = [C.c_int() for _ in range(4)]
        _chk(lib().myo_model_forward_dims(self.h, *(C.byref(x) for x in v)))
        return tuple(x.value for x in v)

    def __del__(self):
        try:
            if self.h:
                lib().myo_model_free(self.h)
        except Exception:
            pass


class HipBatch:
    """B environments' state on the device (vmapped mjx.Data counterpart, mjx/play.py:11)."""

    def __init__(self, model: HipModel, B: int):
        self.model = model
        self.B = B
        self.h = C.c_void_p()
        _chk(lib().myo_batch_create(model.h, B, C.byref(self.h)))
        self._keep = None

    def __del__(self):
        try:
            if self.h:
                lib().myo_batch_free(self.h)
        except Exception:
            pass

    def configure(self, task=TASK_NONE, frame_skip=1, reset_random=0, target_generate=0, target_lo=None, target_hi=None,
                  init_qpos=None, tip_sites=(), pose_thd=0.35, far_th=2 * np.pi, near_th=0.0,
                  w_pose=1.0, w_bonus=4.0, w_act_reg=1.0, w_penalty=50.0, w_reach=1.0, reset_noise=None, reset_clip=None, init_qvel=None,
                  tip_lpos=(0.0, 0.0, 0.0), quat_body=0):
        c = TaskConfig()
        c.quat_body = int(quat_body)
        c.task, c.frame_skip, c.reset_random, c.target_generate = task, frame_skip, int(reset_random), int(target_generate)
        lo = np.ascontiguousarray(target_lo if target_lo is not None else [], np.float32)
        hi = np.ascontiguousarray(target_hi if target_hi is not None else lo, np.float32)
        c.ntarget = lo.size
        c.ntip = len(tip_sites)
        for i, s in enumerate(tip_sites):
            c.tip_site[i] = int(s)
        c.pose_thd, c.far_th, c.near_th = pose_thd, far_th, near_th
        c.w_pose, c.w_bonus, c.w_act_reg, c.w_penalty, c.w_reach = w_pose, w_bonus, w_act_reg, w_penalty, w_reach
        iq, iv = _f32(init_qpos), _f32(init_qvel)
        extra = [_f32(a) for a in (*reset_noise, *reset_clip)] if reset_noise is not None else [None] * 4
        self._keep = (lo, hi, iq, extra, iv)
        c.reset_noise_lo, c.reset_noise_hi, c.reset_clip_lo, c.reset_clip_hi = [_ptr(a) for a in extra]
        c.init_qvel = _ptr(iv)
        c.tip_lpos = (C.c_float * 3)(*[float(x) for x in tip_lpos])
        c.target_lo, c.target_hi = _ptr(lo if lo.size else None), _ptr(hi if hi.size else None)
        c.init_qpos = _ptr(iq)
        _chk(lib().myo_batch_configure(self.h, C.byref(c)))

    def configure_walk(self, *, frame_skip, hip_period, min_height, max_rot, target_x_vel, target_y_vel, target_rot, bodies, qadr_hip_flexion,
                       qadr_joint_angle, weights, init_qpos, init_qvel=None, knee_height=0.0, terrain=0, terrain_scalar=(0.0, 0.0),
                       init_qpos_alt=None, init_qvel_alt=None, reset_noise_std=0.0):
        """walk task (WalkEnvV0).  bodies = (talus_l, talus_r, pelvis, torso) body ids; weights = (vel_reward, done, cyclic_hip,
        ref_rot, joint_angle_rew)."""
        c = WalkConfig()
        c.frame_skip, c.hip_period = int(frame_skip), int(hip_period)
        c.min_height, c.max_rot, c.target_x_vel, c.target_y_vel = float(min_height), float(max_rot), float(target_x_vel), float(target_y_vel)
        c.target_rot = (C.c_float * 4)(*[float(x) for x in target_rot])
        c.body_talus_l, c.body_talus_r, c.body_pelvis, c.body_torso = [int(x) for x in bodies]
        c.qadr_hip_flexion_l, c.qadr_hip_flexion_r = [int(x) for x in qadr_hip_flexion]
        c.qadr_joint_angle = (C.c_int * 4)(*[int(x) for x in qadr_joint_angle])
        c.w_vel_reward, c.w_done, c.w_cyclic_hip, c.w_ref_rot, c.w_joint_angle_rew = [float(x) for x in weights]
        iq, iv, iq2, iv2 = _f32(init_qpos), _f32(init_qvel), _f32(init_qpos_alt), _f32(init_qvel_alt)      # (alive until the call has returned)
        c.init_qpos, c.init_qvel, c.init_qpos_alt, c.init_qvel_alt = _ptr(iq), _ptr(iv), _ptr(iq2), _ptr(iv2)
        c.knee_height, c.terrain = float(knee_height), int(terrain)
        c.terrain_scalar_lo, c.terrain_scalar_hi = float(terrain_scalar[0]), float(terrain_scalar[1])
        c.reset_noise_std = float(reset_noise_std)
        _chk(lib().myo_batch_configure_walk(self.h, C.byref(c)))

    def configure_track(self, *, n_frames, reference, ref_type, init_qpos, ctrl_range, object_link, wrist_link, object_ipos, object_imat, wrist_ipos,
                        lift_z, motion_start_time=0.0, motion_extrapolation=True, interpolation_linear=False, terminate_obj_fail=True,
                        terminate_pose_fail=False, weights=(0.0, 1.0, 1.0, -2.0), autoreset=False, seed=0, max_episode_steps=0,
                        obj_err_scale=50.0, base_err_scale=40.0, lift_bonus_mag=1.0, qpos_reward_weight=0.35, qpos_err_scale=5.0,
                        qvel_reward_weight=0.05, qvel_err_scale=0.1, obj_fail_thresh=0.25, base_fail_thresh=0.25, qpos_fail_thresh=0.75, flavour=0):
        """MyoDM TrackEnv as a fused task of the step kernel (myo_track_config).  reference = dict(time [H], robot [Hr, nr], robot_vel | None,
        object [Ho, no]) in float64 (the reference's own arrays); ref_type 0 FIXED / 1 RANDOM / 2 TRACK; weights = (pose, object, bonus, penalty);
        flavour 0 MJX (fused into the step kernel), 1 classic gym TrackEnv (its own observation / reward kernel, myo_obs)."""
        f64 = lambda a: np.ascontiguousarray(a, np.float64) if a is not None else None
        T, Rb, Rv, Ob = (f64(reference.get(k)) for k in ("time", "robot", "robot_vel", "object"))
        c = TrackConfig()
        c.n_frames, c.ref_type = int(n_frames), int(ref_type)
        c.horizon, c.robot_horizon, c.object_horizon = max(Rb.shape[0], Ob.shape[0]), Rb.shape[0], Ob.shape[0]
        assert T.shape[0] >= c.horizon or ref_type != 2, "reference time axis shorter than the motion"
        c.robot_dim, c.object_dim = Rb.shape[1], Ob.shape[1]
        c.motion_extrapolation, c.interpolation_linear, c.motion_start_time = int(motion_extrapolation), int(interpolation_linear), float(motion_start_time)
        c.ref_time, c.ref_robot, c.ref_robot_vel, c.ref_object = (_ptr(a, C.c_double) for a in (T, Rb, Rv, Ob))
        cr = np.asarray(ctrl_range, np.float64)
        iq, lo, hi = _f32(init_qpos), _f32(cr[:, 0]), _f32(cr[:, 1])
        c.init_qpos, c.ctrl_lo, c.ctrl_hi = _ptr(iq), _ptr(lo), _ptr(hi)
        c.object_link, c.wrist_link = int(object_link), int(wrist_link)
        c.object_ipos = (C.c_float * 3)(*[float(x) for x in object_ipos])
        c.object_imat = (C.c_float * 9)(*[float(x) for x in np.asarray(object_imat).ravel()])
        c.wrist_ipos = (C.c_float * 3)(*[float(x) for x in wrist_ipos])
        c.lift_z, c.obj_err_scale, c.base_err_scale, c.lift_bonus_mag = float(lift_z), float(obj_err_scale), float(base_err_scale), float(lift_bonus_mag)
        c.qpos_reward_weight, c.qpos_err_scale, c.qvel_reward_weight, c.qvel_err_scale = float(qpos_reward_weight), float(qpos_err_scale), float(qvel_reward_weight), float(qvel_err_scale)
        c.obj_fail_thresh, c.base_fail_thresh, c.qpos_fail_thresh = float(obj_fail_thresh), float(base_fail_thresh), float(qpos_fail_thresh)
        c.terminate_obj_fail, c.terminate_pose_fail = int(terminate_obj_fail), int(terminate_pose_fail)
        c.w_pose, c.w_object, c.w_bonus, c.w_penalty = [float(x) for x in weights]
        c.autoreset, c.max_episode_steps, c.seed = int(autoreset), int(max_episode_steps), int(seed)
        c.flavour = int(flavour)
        _chk(lib().myo_batch_configure_track(self.h, C.byref(c)))

    def set_condition(self, frame_skip, epl_actuator=-1, eip_actuator=-1):
        _chk(lib().myo_batch_set_condition(self.h, int(frame_skip), int(epl_actuator), int(eip_actuator)))

    def set_fatigue_reset(self, mode=0, vec=None):
        """Fatigue compartments at reset: 0 rested, 1 random (fatigue_reset_random), 2 `vec` (fatigue_reset_vec); fatigue.py:114-134."""
        v = np.ascontiguousarray(vec, np.float32) if vec is not None else None
        _chk(lib().myo_batch_set_fatigue_reset(self.h, int(mode), v.ctypes.data_as(C.c_void_p) if v is not None else None))

    def set_geom_override(self, geom_id, size_lo=None, size_hi=None):
        """Per-env size of one collision geom, re-drawn ~ U(lo, hi) at every reset of an env (None: off)."""
        if size_lo is None:
            _chk(lib().myo_batch_set_geom_override(self.h, int(geom_id), None, None))
            return
        lo, hi = (C.c_float * 3)(*[float(x) for x in size_lo]), (C.c_float * 3)(*[float(x) for x in size_hi])
        _chk(lib().myo_batch_set_geom_override(self.h, int(geom_id), lo, hi))

    def enable_sensors(self):
        """Allocate F_SENSORDATA / F_CFRC and turn on their readout in the step kernel (36-dof-class Euler models with touch sensors,
        lanes = 64; anything else raises MyoError with the library's reason)."""
        _chk(lib().myo_batch_enable_sensors(self.h))

    def obs_reset_only(self, stream=None):
        _chk(lib().myo_obs_reset_only(self.h, stream))

    # -- reward terms and episode statistics (include/myo_hip_rewards.h) --
    def rwd_names(self):
        """Column names of the configured task's term row, `dense` last (empty: the task has no row)."""
        return tuple(lib().myo_batch_rwd_name(self.h, i).decode() for i in range(lib().myo_batch_rwd_ncol(self.h)))

    def enable_rewards(self, weights, mode=RWD_DENSE):
        """Turn the term row on: one weight per column except dense; MYO_F_REWARD becomes the row's dense (RWD_SPARSE: sparse) column."""
        w = np.ascontiguousarray(weights, np.float32)
        _chk(lib().myo_batch_enable_rewards(self.h, _ptr(w), w.size, int(mode)))

    def rwd_row_ptr(self):
        return self.buffer_ptr("rwd")

    def read_rwd(self) -> np.ndarray:
        return self.buffer_read("rwd")

    def enable_episode_stats(self):
        _chk(lib().myo_batch_enable_episode_stats(self.h))

    def episode_ptr(self, which):
        return self.buffer_ptr("episode", which)

    def read_episode(self, which) -> np.ndarray:
        """Host copy of an episode buffer: EP_RUNNING / EP_LAST [B, 4] float32, EP_FINISHED [B] uint8, EP_COUNT [B] int32."""
        return self.buffer_read("episode", which)

    def episode_update(self, max_episode_steps, stream=None):
        _chk(lib().myo_episode_update(self.h, int(max_episode_steps), stream))

    def episode_clear(self, stream=None):
        _chk(lib().myo_episode_clear(self.h, stream))

    # -- observation terms (include/myo_hip_obs.h) --
    def obs_terms(self):
        """((name, width), ...) of the configured task's term table, in the order of the reference's obs_dict (empty: the task has none)."""
        n = lib().myo_batch_obs_nterm(self.h)
        return tuple((lib().myo_batch_obs_term_name(self.h, k).decode(), int(lib().myo_batch_obs_term_width(self.h, k))) for k in range(n))

    def enable_obs_terms(self, obs_terms, proprio_terms=()):
        """Turn the rows on: OBS_TERMS (every term), OBS_SELECTED (the concatenation of the terms `obs_terms`, indices into the table) and,
        with proprio_terms, OBS_PROPRIO.  Once per batch, after the task was configured; MyoError with the library's reason otherwise."""
        o, p = np.ascontiguousarray(obs_terms, np.int32).ravel(), np.ascontiguousarray(proprio_terms, np.int32).ravel()
        _chk(lib().myo_batch_enable_obs_terms(self.h, _ptr(o, C.c_int), o.size, _ptr(p, C.c_int) if p.size else None, p.size))

    def _set_range(self, field, width, lo, hi):
        lo, hi = (np.broadcast_to(np.asarray(a, np.float32), (self.B, width)) for a in (lo, hi))
        self.write(field, np.concatenate([lo, hi], axis=1))

    def set_body_mass_range(self, lo, hi):
        """Per-env body-mass ranges ([B, nbody] or [nbody] each): every reset of an env draws mass ~ U(lo, hi) for the bodies with
        hi > lo (MYO_F_BODYMASS_RANGE); starts the per-env body-mass override."""
        self._set_range(F_BODYMASS_RANGE, self.model.dims.nbody, lo, hi)

    def set_body_pos_range(self, lo, hi):
        """Per-env offset ranges of the root body of MYO_F_BODYPOS ([B, 3] or [3] each): every reset of an env draws offset ~ U(lo, hi) for
        the components with hi > lo (MYO_F_BODYPOS_RANGE); starts the per-env offset."""
        self._set_range(F_BODYPOS_RANGE, 3, lo, hi)

    def set_body_quat_range(self, lo, hi):
        """Per-env Euler ranges of the selected body ([B, 3] or [3] each): every reset of an env sets body_quat = euler2quat(U(lo, hi))
        (MYO_F_BODYQUAT_RANGE); starts the per-env orientation."""
        self._set_range(F_BODYQUAT_RANGE, 3, lo, hi)

    # -- device buffers by family (FAMILIES) and id (None: the family has one buffer); the per-family methods below are these four --
    def _args(self, i):
        return (self.h,) if i is None else (self.h, int(i))

    def buffer_ptr(self, family, i=None):
        """(device pointer, pitch, width); MyoError with the library's reason where the buffer does not exist (yet)."""
        return buffer_lookup(getattr(lib(), FAMILIES[family][0]), *self._args(i))

    def _width(self, family, i):
        per_body, fixed = _OVERRIDE_WIDTH.get(i, (0, 0)) if family == "field" else (0, 0)
        return per_body * self.model.dims.nbody + fixed if per_body or fixed else self.buffer_ptr(family, i)[2]

    def buffer_spec(self, family, i=None, width=None):
        """(dtype, shape) of a buffer; `width`: its row's elements where a lookup has just reported them."""
        return FAMILIES[family][2](self.B, i, (lambda: self._width(family, i)) if width is None else (lambda: width))

    def buffer_read(self, family, i=None) -> np.ndarray:
        dtype, shape = self.buffer_spec(family, i)
        return host_read(getattr(lib(), FAMILIES[family][1]), *self._args(i), shape=shape, dtype=dtype)

    def buffer_view(self, torch, device, family, i=None):
        """Zero-copy torch view of a buffer in its shape: one library call."""
        ptr, _, width = self.buffer_ptr(family, i)
        dtype, shape = self.buffer_spec(family, i, width)
        return device_view(torch, ptr, shape, dtype, self, device)

    def field_ptr(self, field):
        return self.buffer_ptr("field", field)

    def read(self, field) -> np.ndarray:
        return self.buffer_read("field", field)

    def write(self, field, arr):
        dtype, shape = self.buffer_spec("field", field)
        a = np.ascontiguousarray(arr, dtype).reshape(shape)
        _chk(lib().myo_batch_write(self.h, field, a.ctypes.data, a.nbytes))

    def reset(self, mask_ptr=None, seed=0, stream=None):
        _chk(lib().myo_reset(self.h, mask_ptr, seed, stream))

    def step(self, action_ptr=None, actmap=ACTMAP_NONE, nsub=1, stream=None):
        _chk(lib().myo_step(self.h, action_ptr, actmap, nsub, stream))

    def obs(self, stream=None):
        _chk(lib().myo_obs(self.h, stream))

    # -- forward pass (include/myo_hip_forward.h) --
    def forward(self, stream=None):
        """Body, site and geom frames and the contact list at the current state, without a step (asynchronous; the first call allocates)."""
        _chk(lib().myo_forward(self.h, stream))

    def forward_ptr(self, which):
        """(device pointer, pitch, width) of forward buffer FWD_*; MyoError before the first forward()."""
        return self.buffer_ptr("forward", which)

    def forward_shape(self, which):
        """Shape of forward buffer FWD_*: [B, n, 3], [B, n, 3, 3], [B] (ncon) or [B, ncon_max, 16] (contact)."""
        return self.buffer_spec("forward", which)[1]

    def forward_read(self, which) -> np.ndarray:
        """Host copy of forward buffer FWD_* in its shape; FWD_NCON is int32, FWD_CONTACT float32 (words 13..15 of a record are int32 bits)."""
        return self.buffer_read("forward", which)

    def status(self) -> np.ndarray:
        return host_read(lib().myo_status, self.h, shape=self.B, dtype=np.int32, sized=False)

    def random_action(self, action_ptr, seed, step, env_offset=0, stream=None):
        _chk(lib().myo_random_action(self.h, action_ptr, seed, step, env_offset, stream))

    def last_kernel_name(self) -> str:
        return lib().myo_bench_last_kernel_name(self.h).decode()

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _chk(lib().myo_bench_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def obs_only(self, stream=None):
        _chk(lib().myo_obs_only(self.h, stream))

    def autoreset(self, max_episode_steps, seed=0, stream=None):
        _chk(lib().myo_autoreset(self.h, max_episode_steps, seed, stream))

    def set_balance(self, on):
        _chk(lib().myo_set_balance(self.h, int(on)))

    def set_env_offset(self, off):
        _chk(lib().myo_set_env_offset(self.h, off))

    def bench_rollout(self, steps, nsub, seed=0, mode=BENCH_OBS | BENCH_FRESH_ACTIONS | BENCH_AUTORESET, max_episode_steps=100,
                      stream=None) -> float:
        """Runs `steps` env steps on `stream`; returns the HIP-event elapsed milliseconds."""
        ms = C.c_float()
        _chk(lib().myo_bench_rollout(self.h, steps, nsub, seed, mode, max_episode_steps, stream, C.byref(ms)))
        return ms.value

    def bench_rollout_async(self, steps, nsub, seed=0, mode=BENCH_OBS | BENCH_FRESH_ACTIONS | BENCH_AUTORESET, max_episode_steps=100, stream=None):
        """Enqueues `steps` env steps on `stream` without waiting; `last_kernel_ms()` later collects the step-kernel time of all of them."""
        _chk(lib().myo_bench_rollout(self.h, steps, nsub, seed, mode, max_episode_steps, stream, None))


class FieldViews:
    """`view` / `_stream` of the env classes: the env has batch, device, _views = {} and _torch (the module, or None for numpy I/O)."""

    def view(self, i, family="field"):
        """torch view (zero copy, cached under (family, id): the first use makes one library call, later uses none) of a per-env field,
        or of buffer `i` of another family of FAMILIES; without torch a numpy copy."""
        if self._torch is None:
            return self.batch.buffer_read(family, i)
        v = self._views.get((family, i))
        if v is None:
            v = self._views[family, i] = self.batch.buffer_view(self._torch, self.device, family, i)
        return v

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream if self._torch is not None else None

    def forward(self):
        """Body, site and geom frames and the contact list of the env's batch at its current state, without a step (what the reference's
        get_obs_dict reads from sim.data: site_xpos, body_xpos, geom_xpos, ncon, contact): one launch, returns the ForwardRecord -- zero-copy
        torch views, or fresh numpy copies without torch.  The state, observation and reward rows are not touched."""
        self.batch.forward(self._stream())
        if getattr(self, "_fwd", None) is None:
            self._fwd = ForwardRecord(self.batch, self._torch, self.device)
        else:
            self._fwd.refresh()
        return self._fwd


class ContactList:
    """`contact` of a forward pass: dist [B, C], pos [B, C, 3], frame [B, C, 9] (normal, then the two tangents), geom1 / geom2 [B, C] (model
    geom ids, int32) and pair [B, C] (the kernel's pair index).  Entries at or beyond ncon[e] are unspecified; so is the order within an env."""

    def __init__(self, rec, as_int):
        ids = as_int(rec[..., 13:16])
        self.dist, self.pos, self.frame = rec[..., 0], rec[..., 1:4], rec[..., 4:13]
        self.geom1, self.geom2, self.pair = ids[..., 0], ids[..., 1], ids[..., 2]


class ForwardRecord:
    """What a forward pass leaves, as attributes: xpos / xipos / site_xpos / geom_xpos [B, n, 3], xmat / site_xmat / geom_xmat [B, n, 3, 3]
    (site_xmat: None for a model compiled without site_quat), body_xpos / body_xmat (the reference's spelling of xpos / xmat), ncon [B]
    int32 and contact (ContactList).  With a torch module they are zero-copy views of the library's buffers, valid for the batch's lifetime
    and current after every `HipBatch.forward` once the stream has run it; without one, host arrays that `refresh()` reads again."""

    def __init__(self, batch, torch=None, device=0):
        self._batch, self._torch, self._device = batch, torch, device
        self.refresh()

    def _get(self, which):
        if self._torch is None:
            return self._batch.forward_read(which)
        return self._batch.buffer_view(self._torch, self._device, "forward", which)

    def refresh(self):
        if self._torch is not None and hasattr(self, "xpos"):
            return self       # views: nothing to copy
        for name, which in FWD_NAMES.items():
            if which == FWD_CONTACT:
                as_int = (lambda t: t.view(self._torch.int32)) if self._torch is not None else (lambda a: a.view(np.int32))
                self.contact = ContactList(self._get(which), as_int)
            elif which == FWD_SITE_XMAT:
                try:
                    self.site_xmat = self._get(which)
                except MyoError:
                    self.site_xmat = None
            else:
                setattr(self, name, self._get(which))
        self.body_xpos, self.body_xmat = self.xpos, self.xmat
        return self


def forward_host_tables(blob: bytes):
    """The forward pass's export tables as the library builds them at model load (no GPU needed): (body, site, geom), each [n, 16] float64 =
    link | position (3) | rotation (9) in the link's frame | bodies: COM in the link's frame (3); sites, geoms: body id, 0, 0."""
    out = []
    for t in range(3):
        n = C.c_int()
        _chk(lib().myo_forward_host_tables(blob, len(blob), t, None, 0, C.byref(n)))
        a = np.zeros((n.value, 16), np.float64)
        if n.value:
            _chk(lib().myo_forward_host_tables(blob, len(blob), t, a.ctypes.data, a.size, C.byref(n)))
        out.append(a)
    return tuple(out)


def set_lanes(lanes):
    _chk(lib().myo_set_lanes(lanes))


def read_stamps(batch, nwg):
    out = np.zeros((nwg, 12), np.int64)
    rc = lib().myo_read_stamps(batch.h, out.ctypes.data, nwg)
    if rc < 0:
        _chk(rc)
    return out, rc == 0


def sync(stream=None):
    _chk(lib().myo_sync(stream))


def probe_valu(waves_per_simd, iters=20000, device=0):
    """Measured chip-wide issue rate of wave64 v_fma_f32 (instructions / s) with `waves_per_simd` waves resident per SIMD, and the CU count."""
    r, n = C.c_double(0), C.c_int(0)
    _chk(lib().myo_probe_valu(int(device), int(waves_per_simd), int(iters), C.byref(r), C.byref(n)))
    return r.value, n.value
