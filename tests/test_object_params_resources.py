"""Register / scratch figures of the kernels the per-env object parameters touch or add, read from the built library's code object (no GPU
needed), after the pattern of tests/test_forward_resources.py: the TrackEnv-class step kernel, its twin with the object parameters compiled
in (step_kernel_obj), the TrackEnv-class forward twin, the reset kernels (the draws are part of reset_body) and the compose kernel.  That
every step_kernel_w instantiation -- the TRK one included -- still has the code it had before is tests/test_forward_resources.py's check."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TRK_ARGS = "36, 20, 32, 2, 2, false, 0, false, true, false"


@pytest.fixture(scope="module")
def kernels():
    from myosuite_mjx_amd import capi
    import kernel_resources
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    out = {}
    for r in kernel_resources.resources(capi.LIB_PATH):
        out[subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()] = r
    return out


def _one(kernels, prefix):
    hits = [r for n, r in kernels.items() if n.startswith(prefix)]
    assert len(hits) == 1, (prefix, [n for n in kernels if n.startswith(prefix[:20])])
    return hits[0]


@pytest.mark.parametrize("prefix", [f"void step_kernel_w<{TRK_ARGS}>(", f"void step_kernel_obj<{TRK_ARGS}>(",
                                    "void forward_kernel_w<36, 20, 32, 2, 2, false, true>("])
def test_trk_kernels_have_no_spill_and_no_scratch(kernels, prefix):
    r = _one(kernels, prefix)
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 256, r          # two waves per SIMD: what the TRK launch bounds and the LDS slice are sized for


def test_only_one_object_instantiation_is_built(kernels):
    built = sorted(n.split("(")[0] for n in kernels if n.startswith("void step_kernel_obj<"))
    assert built == [f"void step_kernel_obj<{TRK_ARGS}>"], built


def test_object_step_kernel_costs_no_occupancy(kernels):
    """The twin stays in the register class of the kernel it is a copy of (same waves per SIMD; a handful of registers more at most)."""
    a, b = _one(kernels, f"void step_kernel_w<{TRK_ARGS}>("), _one(kernels, f"void step_kernel_obj<{TRK_ARGS}>(")
    assert b["vgpr"] + b["agpr"] <= a["vgpr"] + a["agpr"] + 16 and b["lds"] == a["lds"], (a, b)


@pytest.mark.parametrize("prefix,vmax", [("obj_compose_kernel(", 64), ("reset_kernel(", 128)])
def test_small_kernels_have_no_spill_and_no_scratch(kernels, prefix, vmax):
    r = _one(kernels, prefix)
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= vmax, r


def test_task_post_kernels_with_the_draws_have_no_spill(kernels):
    """task_post_kernel<...> runs reset_body, and with it the draws, inside the fused epilogue of every task."""
    rs = {n: r for n, r in kernels.items() if n.startswith("void task_post_kernel<")}
    assert len(rs) >= 5, sorted(rs)
    for n, r in rs.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 128, (n, r)
