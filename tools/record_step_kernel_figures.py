"""Register, spill, scratch, LDS and code-size figures of every step_kernel_w instantiation of a built library, as the record
tests/test_forward_resources.py compares the current build with (no GPU needed).

    python tools/record_step_kernel_figures.py [path/to/libmyo_hip.so]          # print
    python tools/record_step_kernel_figures.py path/to/libmyo_hip.so --write    # refresh tests/golden/step_kernel_figures.json

The record holds the step_kernel_w instantiations only.  step_kernel_obj (the TrackEnv-class body with the per-env object parameters compiled in,
csrc/myo_kernel_wave.h) is deliberately not in it: it is new code with nothing to be equal to; tests/test_object_params_resources.py bounds it.

The committed record is made from a build of the commit BEFORE a change that must leave the step kernels' code alone (same compiler, same
flags): check the parent out somewhere, build it there, and point this tool at that library."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_kernel_figures.json")
KEYS = ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch", "lds", "code_bytes")


def code_sizes(lib=KR.LIB):
    """{kernel symbol: size in bytes of its code} from the gfx950 code object's symbol table."""
    with tempfile.TemporaryDirectory(prefix="myo_co_") as tmp:
        subprocess.check_call([os.path.join(KR.LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, f"{tmp}/fat.bin"])
        subprocess.check_call([os.path.join(KR.LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={tmp}/fat.bin", f"--output={tmp}/k.co"])
        txt = subprocess.check_output([os.path.join(KR.LLVM, "llvm-readelf"), "-s", "-W", f"{tmp}/k.co"], text=True)
    out = {}
    for line in txt.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            out[f[7]] = int(f[2], 0)
    return out


def figures(lib=KR.LIB, match="step_kernel_w"):
    """{mangled kernel name: {vgpr, agpr, sgpr, vgpr_spill, sgpr_spill, scratch, lds, code_bytes}} of the kernels whose name holds `match`."""
    size = code_sizes(lib)
    out = {}
    for r in KR.resources(lib):
        if re.search(match, r["name"]):
            out[r["name"]] = {**{k: r[k] for k in KEYS if k != "code_bytes"}, "code_bytes": size[r["name"]]}
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--write"]
    fig = figures(args[0] if args else KR.LIB)
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(fig, f, indent=1, sort_keys=True)
            f.write("\n")
    for n, v in sorted(fig.items()):
        print(n, v)
