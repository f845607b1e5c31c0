"""Register / scratch figures of the built step kernels, read from the code object's metadata (no GPU needed).

Round 2 shipped step kernels with 35-45 VGPRs spilled to scratch memory inside divergent code (8.5x wasted HBM traffic, and a class of
order-dependent wrong results on two intermediate code shapes, DESIGN.md section 4 "Diagnostic builds").  Every instantiation of the wave
kernel that a model can be routed to must now be free of vector-register spills and of scratch memory altogether, and must keep the occupancy
its LDS slice is sized for (4 waves per SIMD = 128 registers for the hand class, 2 = 256 for the 36-dof class)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def kernels():
    from myosuite_mjx_amd import capi
    import kernel_resources
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    out = {}
    for r in kernel_resources.resources(capi.LIB_PATH):
        out[subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip().split("(")[0]] = r
    return out


# <NVT, KC, NC, NTR, WPE, SCHED, SPEC, HF, TRK, RK4>: what launch_step (csrc/myo_host_step.h, select_wave_kernel) can select
WAVE = {
    "headline: MyoHand, size-specialised": ("24, 8, 32, 1, 4, false, 1, false, false, false", 128),
    "hand / finger class, run-time sizes": ("24, 8, 32, 1, 3, false, 0, false, false, false", 128),   # budget of 3 waves per SIMD, lands on 128 registers = 4
    "36-dof class": ("36, 20, 32, 2, 2, false, 0, false, false, false", 256),
    "MyoLeg, size-specialised": ("36, 20, 32, 2, 2, false, 2, false, false, false", 256),
    "36-dof class, substep scheduler": ("36, 20, 32, 2, 2, true, 0, false, false, false", 256),
    "MyoLeg, scheduler (config 5 default)": ("36, 20, 32, 2, 2, true, 2, false, false, false", 256),
    "terrain": ("36, 20, 32, 2, 2, false, 0, true, false, false", 256),
    "terrain, size-specialised": ("36, 20, 32, 2, 2, false, 3, true, false, false", 256),
    "terrain, scheduler": ("36, 20, 32, 2, 2, true, 3, true, false, false", 256),
    "TrackEnv model class (TRK)": ("36, 20, 32, 2, 2, false, 0, false, true, false", 256),
    "RK4 hand class": ("24, 8, 32, 1, 3, false, 0, false, false, true", 168),
    "RK4 36-dof class": ("36, 20, 32, 2, 2, false, 0, false, false, true", 256),
}


@pytest.mark.parametrize("what", sorted(WAVE))
def test_wave_kernel_has_no_spills_and_no_scratch(kernels, what):
    args, vmax = WAVE[what]
    name = f"void step_kernel_w<{args}>"
    assert name in kernels, (name, sorted(k for k in kernels if "step_kernel_w" in k))
    r = kernels[name]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["vgpr"] + r["agpr"] <= vmax, r        # occupancy the LDS slice was sized for


def test_no_other_wave_instantiation_is_built(kernels):
    """Instantiations nobody can reach (round 2: a scheduled hand kernel with 86 spilled VGPRs, two 5-waves-per-SIMD experiments with 87-90) are gone."""
    built = sorted(k for k in kernels if k.startswith("void step_kernel_w<"))
    assert built == sorted(f"void step_kernel_w<{a}>" for a, _ in WAVE.values()), built


def test_new_kernels_have_no_spill_and_no_scratch():
    """Every task_obs_kernel / task_post_kernel instantiation, read from the code object's metadata the way the step kernels are read
    above (the `kernels` fixture keys kernels by the demangled name up to the first parenthesis, which the function-pointer template
    argument of the task kernels cuts short, so they are looked up by their mangled names here): no VGPR spill, no scratch, at most 128
    VGPRs.  The observation kernels spill no SGPR either; five of the fused epilogues did before the check covered them (to VGPR lanes,
    not to scratch) and are pinned at those figures."""
    from myosuite_mjx_amd import capi
    import kernel_resources
    bodies = ("pose", "stand", "hold", "keyturn", "pen", "baoding", "die", "myodm", "mjx_track")
    sgpr_spill = {("post", "keyturn"): 13, ("post", "pen"): 25, ("post", "baoding"): 13, ("post", "die"): 36, ("post", "myodm"): 26}
    seen = []
    for r in kernel_resources.resources(capi.LIB_PATH):
        name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
        m = re.match(r"void task_(obs|post)_kernel<\w+<&\((\w+)_obs_body\(", name)
        if not m:
            assert not name.startswith(("void task_obs_kernel<", "void task_post_kernel<")), name
            continue
        seen.append(m.groups())
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 128, (name, r)
        assert r["sgpr_spill"] <= sgpr_spill.get(m.groups(), 0), (name, r)
    assert sorted(seen) == sorted([("obs", b) for b in bodies] + [("post", b) for b in bodies if b != "mjx_track"]), seen
