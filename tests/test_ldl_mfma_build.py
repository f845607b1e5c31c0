"""CPU checks of the matrix-core Newton factorisation (csrc/myo_ldl_mfma.h): the headline kernel runs it, and the MYO_LDL_MFMA=0 build that
A/B measurements compare against still compiles, with the VALU factorisation in its place."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLVM = "/opt/rocm/lib/llvm/bin"
HEADLINE = "_Z13step_kernel_wILi24ELi8ELi32ELi1ELi4ELb0ELi1ELb0ELb0ELb0EE"   # step_kernel_w<24, 8, 32, 1, 4, false, 1, false, false, false>
MFMA = "v_mfma_f32_32x32x2_f32"


def _kernel_asm(lib, tmp):
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, f"{tmp}/fat.bin"])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={tmp}/fat.bin", f"--output={tmp}/k.co"])
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f"{tmp}/k.co"], text=True)
    out, cur = {}, None
    for line in txt.splitlines():
        if line.endswith(">:") and "<" in line:
            cur = line.split("<", 1)[1][:-2]
            out[cur] = []
        elif cur is not None and line.strip():
            out[cur].append(line.split()[0])
    return out


def _headline(asm):
    names = [n for n in asm if n.startswith(HEADLINE)]
    assert len(names) == 1, names
    return asm[names[0]]


def test_headline_kernel_factorises_on_the_matrix_cores():
    from myosuite_mjx_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()
    with tempfile.TemporaryDirectory(prefix="myo_ldl_") as tmp:
        asm = _kernel_asm(capi.LIB_PATH, tmp)
    ins = _headline(asm)
    assert ins.count(MFMA) == 11             # 12 panel steps of two columns, no trailing update after the last one
    assert sum(n.count(MFMA) for k, n in asm.items() if "step_kernel_wILi36" in k) == 0   # the 36-dof kernels keep the VALU path


def test_valu_build_compiles_without_mfma():
    from myosuite_mjx_amd import capi
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory(prefix="myo_ldl_") as tmp:
        lib = os.path.join(tmp, "libmyo_valu.so")
        subprocess.check_call([hipcc, *capi.HIPCC_FLAGS, "-DMYO_LDL_MFMA=0", "-shared", "-fPIC", "-o", lib, capi.SRC_PATH])
        asm = _kernel_asm(lib, tmp)
    assert sum(n.count(MFMA) for n in asm.values()) == 0
    assert len(_headline(asm)) > 0
