"""The forward pass left the step kernels alone, and its own kernels are clean (no GPU needed; reads the built library's code object).

tests/golden/step_kernel_figures.json holds, for every step_kernel_w instantiation, the VGPR / AGPR / SGPR counts, the spill counts, the
scratch and LDS sizes and the size of the kernel's code in bytes, recorded by tools/record_step_kernel_figures.py from a build of the commit
before the forward pass existed (same compiler, same flags).  forward_kernel_w calls the step kernel's stage functions; a change to one of
them, or to a shared header, that alters a step kernel's code shows up here as a different figure."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def lib():
    from myosuite_mjx_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    return capi.LIB_PATH


def test_every_step_kernel_has_its_recorded_figures(lib):
    import record_step_kernel_figures as R
    with open(R.GOLDEN) as f:
        golden = json.load(f)
    now = R.figures(lib)
    assert len(golden) == 12 and sorted(now) == sorted(golden)
    diff = {n: (golden[n], now[n]) for n in golden if golden[n] != now[n]}
    assert not diff, diff


def test_forward_kernels_have_no_spill_and_no_scratch(lib):
    """The four forward twins: template arguments <NVT, KC, NC, NTR, WPE, HF, TRK> of the hand, 36-dof, terrain and TrackEnv classes."""
    import record_step_kernel_figures as R
    fig = R.figures(lib, match="forward_kernel_w")
    names = {subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(")[0]: v for n, v in fig.items()}
    want = ["void forward_kernel_w<24, 8, 32, 1, 3, false, false>", "void forward_kernel_w<36, 20, 32, 2, 2, false, false>",
            "void forward_kernel_w<36, 20, 32, 2, 2, false, true>", "void forward_kernel_w<36, 20, 32, 2, 2, true, false>"]
    assert sorted(names) == want, sorted(names)
    for n, r in names.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["vgpr"] + r["agpr"] <= (168 if n.startswith("void forward_kernel_w<24") else 256), (n, r)     # the occupancy the launch bounds ask for
