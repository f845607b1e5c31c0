"""The 24-dof step kernels move the mass matrix M, the Newton Hessian H and its factor L between LDS layouts with fewer LDS instructions
(csrc/myo_kernel_wave.h): the first Newton refactor of a substep builds H on the M the square buffer still holds (MYO_MHL_A), the packed copy
of M is made by the whole wave (MYO_MHL_B), and the later refactors of a substep bring back only what L overwrote, again with the whole wave
(MYO_MHL_E).  All of it is data movement, so the default build and the build of the same sources with every switch off must give the same
bits: short rollouts of two pose workloads from their uniform-over-range resets (interpenetrating fingers: several Newton iterations and
refactors per substep, so the later refactors run too), and both builds stay free of spills and scratch memory.  Each library runs in a child
process of its own, because the library is chosen when it is first loaded (MYO_HIP_LIB)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SWITCHES_OFF = ["-DMYO_MHL_A=0", "-DMYO_MHL_B=0", "-DMYO_MHL_E=0"]          # every MYO_MHL_* switch the sources have
ENVS = ["myoHandPoseRandom-v0", "myoFingerPoseFixed-v0"]
NENV, NSTEP = 64, 3
FIELDS = ["F_QPOS", "F_QVEL", "F_ACT", "F_OBS", "F_REWARD"]

WORKER = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from myosuite_mjx_amd import capi
from myosuite_mjx_amd.envs import make
env_id, nenv, nstep, out = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
env = make(env_id, num_envs=nenv, as_torch=False)
env.reset(seed=0)
rng = np.random.default_rng(0)
res, fact = {}, np.zeros(nenv, np.int64)
for s in range(nstep):
    env.step(rng.uniform(-1.0, 1.0, (nenv, env.act_dim)).astype(np.float32))
    fact = np.maximum(fact, env.batch.read(capi.F_DIAG)[:, 7].astype(np.int64) >> 16)    # dense refactors of this env step (all its substeps)
    for f in sys.argv[6:]:
        res[f"{f}_{s}"] = np.ascontiguousarray(env.batch.read(getattr(capi, f)))
res["fact_max"] = fact
res["frame_skip"] = np.array([env.frame_skip])
res["flags"] = np.asarray(env.status())
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def off_lib(tmp_path_factory):
    """The sources with every MYO_MHL_* switch off, built like the MYO_LDL_MFMA=0 variant of test_ldl_mfma_build.py."""
    from myosuite_mjx_amd import capi
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = str(tmp_path_factory.mktemp("mhl") / "libmyo_mhl_off.so")
    subprocess.check_call([hipcc, *capi.HIPCC_FLAGS, *SWITCHES_OFF, "-shared", "-fPIC", "-o", lib, capi.SRC_PATH])
    return lib


def _dof24(lib):
    import kernel_resources
    rs = [r for r in kernel_resources.resources(lib) if r["name"].startswith("_Z13step_kernel_wILi24E")]
    assert len(rs) == 3, [r["name"] for r in rs]          # headline, run-time sizes, RK4 twin
    return rs


def test_both_builds_compile_without_spills_or_scratch(off_lib):
    from myosuite_mjx_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    for lib in (capi.LIB_PATH, off_lib):
        for r in _dof24(lib):
            assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (lib, r)      # the figures test_kernel_resources.py holds every step kernel to


def _rollout(lib, env_id, out):
    env = dict(os.environ, MYO_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-c", WORKER, ROOT, env_id, str(NENV), str(NSTEP), out, *FIELDS], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.gpu
@pytest.mark.parametrize("env_id", ENVS)
def test_default_and_switched_off_builds_give_the_same_bits(off_lib, tmp_path, env_id):
    from myosuite_mjx_amd import capi
    a = _rollout(capi.LIB_PATH, env_id, str(tmp_path / "on.npz"))
    b = _rollout(off_lib, env_id, str(tmp_path / "off.npz"))
    # more refactors in one env step than it has substeps: some substep factorised more than once, i.e. went through the later-refactor path
    assert a["fact_max"].max() > int(a["frame_skip"][0]), (a["fact_max"].max(), int(a["frame_skip"][0]))
    assert np.array_equal(a["fact_max"], b["fact_max"]) and np.array_equal(a["flags"], b["flags"])
    for f in FIELDS:
        for s in range(NSTEP):
            x, y = a[f"{f}_{s}"], b[f"{f}_{s}"]
            assert x.dtype == y.dtype and x.shape == y.shape and x.size > 0
            assert x.tobytes() == y.tobytes(), (f, s, int((x != y).sum()))
