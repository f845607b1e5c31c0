"""CPU tests of the device learner's surroundings: the `update` argument of ppo.train, where the entry points are declared and that the
built library exports them, the register / scratch figures of the learner's kernels, and the float64 helper of the GPU tests
(tests/ppo_update_ref.py) against finite differences of its own loss."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ppo_update_ref as R
from myosuite_mjx_amd import capi, ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ENTRY_POINTS = ("myo_ppo_learner_create", "myo_ppo_learner_free", "myo_ppo_learner_step", "myo_ppo_learner_tensor")


class _CpuEnv:
    num_envs, obs_dim, act_dim = 8, 3, 2

    def reset(self, seed=None):
        return torch.zeros((self.num_envs, self.obs_dim))

    def step(self, action):
        raise AssertionError("step() was called: the update mode is checked before the first unroll")


def test_train_takes_update_and_defaults_to_none():
    assert inspect.signature(ppo.train).parameters["update"].default is None


@pytest.mark.parametrize("update", ["hip", "x"])
def test_train_refuses_the_update_mode(update):
    """'hip' needs the hip backend, which a CPU env cannot have; anything but None, 'torch' and 'hip' is refused outright."""
    with pytest.raises(ValueError, match="update"):
        ppo.train(_CpuEnv(), 64, unroll_length=4, num_minibatches=2, update=update)


def test_entry_points_are_declared_in_the_ppo_header_only():
    text = {name: open(os.path.join(ROOT, "include", name)).read() for name in ("myo_hip.h", "myo_hip_ppo.h")}
    for sym in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % sym, text["myo_hip_ppo.h"]), sym
        assert sym not in text["myo_hip.h"], sym
    assert "myo_ppo_config" in text["myo_hip_ppo.h"] and "myo_ppo_learner" not in text["myo_hip.h"]


def test_library_exports_the_entry_points():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ENTRY_POINTS:
        getattr(lib, sym)


def test_learner_kernels_have_no_spill_and_no_scratch():
    """Every kernel of csrc/myo_kernels_learner.h, read from the code object's metadata as tests/test_kernel_resources.py reads the step kernels."""
    import kernel_resources
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    src = open(os.path.join(ROOT, "myosuite_mjx_amd", "csrc", "myo_kernels_learner.h")).read()
    declared = set(re.findall(r"__launch_bounds__\(\d+\)\s+(learner_\w+)\(", src))
    assert declared == {"learner_gemm_kernel", "learner_gae_kernel", "learner_loss_kernel", "learner_loss_sum_kernel", "learner_adam_kernel"}
    built = {}
    for r in kernel_resources.resources(capi.LIB_PATH):
        name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip().split("(")[0]
        if "learner_" in name:
            built[name] = r
    assert {n.replace("void ", "").split("<")[0] for n in built} == declared, sorted(built)
    assert sum("learner_gemm_kernel<" in n for n in built) == 5      # forward and dW for either input, dX
    for name, r in built.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)


def test_helper_gradient_matches_finite_differences():
    """Central differences of the float64 loss on the smallest case, at a handful of entries of every tensor (the largest gradient entry
    among them).  h = 1e-6: the truncation error is ~h^2 and the rounding error ~1e-16 / h, both far below the 1e-6 asked for, relative to
    the tensor's largest gradient entry; rho stays 2e-2 away from the clip edges on this case, so no sample changes branch."""
    case = R.make_case(3, 5, 7, 1, (32,), (256,), seed=1)
    idx, noise = case["idx"][0], case["noise"][0]
    grads, _, rho, adv = R.gradients(case["params"], case, idx, noise)
    assert R.clip_figures(rho, adv)[0] > 1e-3

    base = tuple([np.asarray(a, np.float64) for a in group] for group in case["params"])
    as_tensors = lambda arrays: tuple([torch.tensor(a, dtype=torch.float64) for a in group] for group in arrays)
    with torch.no_grad():       # vs and the advantage at the base point: the gradient treats them as constants, so the differences do too
        x = (torch.tensor(case["obs"][:, idx], dtype=torch.float64) - torch.tensor(case["mean"], dtype=torch.float64)) / torch.tensor(case["std"], dtype=torch.float64)
        targets = R.gae_targets(R.mlp(x, *as_tensors(base)[2:]).squeeze(-1).numpy(), case, idx)

    def total(arrays):
        with torch.no_grad():
            policy, value, entropy, _, _ = R.losses(as_tensors(arrays), case, idx, noise, targets=targets)
            return float(policy + value + entropy)

    rng, h = np.random.default_rng(0), 1e-6
    for gi, group in enumerate(base):
        for ti, a in enumerate(group):
            g = grads[gi][ti]
            picks = {int(np.abs(g).argmax())} | {int(k) for k in rng.integers(0, a.size, 4)}
            for k in picks:
                at = np.unravel_index(k, a.shape)
                vals = []
                for sign in (1.0, -1.0):
                    moved = tuple([x.copy() for x in grp] for grp in base)
                    moved[gi][ti][at] += sign * h
                    vals.append(total(moved))
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - g[at]) <= 1e-6 * np.abs(g).max(), (gi, ti, at, fd, g[at])
