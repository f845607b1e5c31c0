"""The Newton refactor on the matrix cores (ldl_mfma, csrc/myo_ldl_mfma.h) against the VALU factorisation chol_rows and a float64 L D L^T.

A small harness built from the kernel's own headers runs one wave per matrix: ldl_mfma on the buffer as the step kernel leaves it (row-major,
stride NVT + 1, lower triangle valid; here NaNs above the diagonal and in the 1/D column, which it must never let through), and chol_rows on
the same rows, stored the way the step kernel stores them.  About 10^4 SPD matrices: random ones, hand-like mass matrices (the MyoHand dof
tree) plus stiff contact blocks, singular ones whose pivots reach the MINVALF clamp, and nv < NVT with identity padding rows."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "myosuite_mjx_amd", "csrc")

HARNESS = r"""
#include "myo_common.h"
#include "myo_physics.h"
#include "myo_task_track.h"
#include "myo_kernel_lanes.h"
#include "myo_kernel_wave.h"

// mode 0: ldl_mfma in place; mode 1: chol_rows on the lower rows (zero above the diagonal, zero rows for the lanes >= NVT, as the step kernel)
template <int NVT, int MODE> __global__ void __launch_bounds__(64) ldl_kernel(const float* H, float* out) {
  __shared__ float S[NVT * (NVT + 1)];
  const int lane = threadIdx.x;
  const float* Hm = H + (size_t)blockIdx.x * NVT * (NVT + 1);
  for (int i = lane; i < NVT * (NVT + 1); i += 64) S[i] = Hm[i];
  __syncthreads();
  if constexpr (MODE == 0) {
    ldl_mfma<NVT>(S, lane);
  } else {
    float r[NVT];
    const int ll = lane < NVT ? lane : 0;
#pragma unroll
    for (int k = 0; k < NVT; k++) { const float v = S[ll * (NVT + 1) + k]; r[k] = (lane < NVT && k <= lane) ? v : 0.f; }
    __syncthreads();
    const float invd = chol_rows<NVT>(r, lane);
    if (lane < NVT) {
#pragma unroll
      for (int k = 0; k < NVT; k++) S[lane * (NVT + 1) + k] = r[k];
      S[lane * (NVT + 1) + NVT] = invd;
    }
  }
  __syncthreads();
  float* o = out + (size_t)blockIdx.x * NVT * (NVT + 1);
  for (int i = lane; i < NVT * (NVT + 1); i += 64) o[i] = S[i];
}

template <int NVT> static int run(int mode, const float* H, float* out, int n) {
  const size_t bytes = (size_t)n * NVT * (NVT + 1) * sizeof(float);
  float *dH = nullptr, *dO = nullptr;
  if (hipMalloc(&dH, bytes) != hipSuccess) return 1;
  if (hipMalloc(&dO, bytes) != hipSuccess) { hipFree(dH); return 2; }
  int rc = hipMemcpy(dH, H, bytes, hipMemcpyHostToDevice) != hipSuccess ? 3 : 0;
  if (!rc) {
    if (mode == 0) hipLaunchKernelGGL((ldl_kernel<NVT, 0>), dim3(n), dim3(64), 0, 0, dH, dO);
    else hipLaunchKernelGGL((ldl_kernel<NVT, 1>), dim3(n), dim3(64), 0, 0, dH, dO);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 4;
  }
  if (!rc && hipMemcpy(out, dO, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = 5;
  hipFree(dH); hipFree(dO);
  return rc;
}

extern "C" int ldl_run(int nvt, int mode, const float* H, float* out, int n) {
  if (nvt == 24) return run<24>(mode, H, out, n);
  if (nvt == 17) return run<17>(mode, H, out, n);
  return 9;
}
"""

# MyoHand dof tree (SpecTree<1> in csrc/myo_kernel_wave.h: parent dof of each dof)
HAND_PARENT = [-1, 0, 1, 2, 3, 4, 5, 2, 7, 8, 9, 2, 11, 12, 13, 2, 15, 16, 17, 2, 19, 20, 21]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    from myosuite_mjx_amd import capi
    d = tmp_path_factory.mktemp("ldl_mfma")
    src, so = d / "ldl_harness.hip", d / "libldl_harness.so"
    src.write_text(HARNESS)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *capi.HIPCC_FLAGS, "-I", CSRC, "-shared", "-fPIC", "-o", str(so), str(src)])
    try:
        import torch  # noqa: F401  (same HIP runtime as the rest of the suite: capi.lib)
    except ImportError:
        pass
    lib = ctypes.CDLL(str(so))
    lib.ldl_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return lib


def _run(lib, nvt, mode, Hbuf):
    Hbuf = np.ascontiguousarray(Hbuf, np.float32)
    out = np.full_like(Hbuf, np.nan)
    rc = lib.ldl_run(nvt, mode, Hbuf.ctypes.data, out.ctypes.data, Hbuf.shape[0])
    assert rc == 0, rc
    return out


def _buffer(H, nvt):
    """Step-kernel buffer: row-major, stride NVT + 1, lower triangle = H, NaN above the diagonal and in the 1/D column."""
    n = H.shape[0]
    buf = np.full((n, nvt, nvt + 1), np.nan, np.float32)
    il = np.tril_indices(nvt)
    buf[:, il[0], il[1]] = H[:, il[0], il[1]]
    return buf


def _ldl64(H):
    n, N, _ = H.shape
    L = np.zeros((n, N, N))
    D = np.zeros((n, N))
    A = H.astype(np.float64).copy()
    for j in range(N):
        D[:, j] = A[:, j, j]
        c = A[:, j + 1:, j] / D[:, j, None]
        L[:, j + 1:, j] = c
        A[:, j + 1:, j + 1:] -= c[:, :, None] * A[:, None, j, j + 1:]
    return L, D


def _spd_random(rng, n, N):
    G = rng.standard_normal((n, N, N))
    H = G @ G.transpose(0, 2, 1) / N + 0.05 * np.eye(N)
    return H * 10.0 ** rng.uniform(-3, 3, (n, 1, 1))


def _hand_like(rng, n, N):
    """Tree-structured mass matrix on the MyoHand dof tree (leaves first, as the kernel's rows) plus stiff contact blocks J^T D J."""
    nv = len(HAND_PARENT)
    anc = []
    for d in range(nv):
        chain, p = [d], HAND_PARENT[d]
        while p >= 0:
            chain.append(p)
            p = HAND_PARENT[p]
        anc.append(chain)
    perm = [nv - 1 - i for i in range(nv)]           # lane i <-> dof nv - 1 - i
    H = np.zeros((n, N, N))
    for e in range(n):
        M = np.zeros((nv, nv))
        for d in range(nv):                             # body d: a rank-3 inertia term on its chain of ancestors
            u = np.zeros((nv, 3))
            u[anc[d]] = rng.standard_normal((len(anc[d]), 3)) * 10.0 ** rng.uniform(-3, -1.5)
            M += u @ u.T
        M += np.diag(10.0 ** rng.uniform(-4, -3, nv))  # armature
        for _ in range(rng.integers(0, 7)):             # contacts: <= 8 dofs along one chain, three rows, D up to 1e5 (condition numbers to ~1e7)
            chain = anc[rng.integers(0, nv)][:8]
            J = np.zeros((3, nv))
            J[:, chain] = rng.standard_normal((3, len(chain))) * 10.0 ** rng.uniform(-2.5, -1.5)
            M += J.T @ np.diag(10.0 ** rng.uniform(2, 5, 3)) @ J
        Mp = M[np.ix_(perm, perm)]
        H[e, :nv, :nv] = Mp
        H[e, nv:, nv:] = np.eye(N - nv)
    return H


def _singular(rng, n, N):
    """SPD matrices with three zero-mass dofs (zero row and column): those pivots are exactly zero and clamped to MINVALF."""
    G = rng.standard_normal((n, N, N))
    H = G @ G.transpose(0, 2, 1) / N + 0.05 * np.eye(N)
    for e in range(n):
        z = rng.choice(N, 3, replace=False)
        H[e, z, :] = 0.0
        H[e, :, z] = 0.0
    return H


def _padded(rng, n, N):
    H = np.zeros((n, N, N))
    for e in range(n):
        nv = int(rng.integers(1, N))
        G = rng.standard_normal((nv, nv))
        H[e, :nv, :nv] = G @ G.T / nv + 0.1 * np.eye(nv)
        H[e, nv:, nv:] = np.eye(N - nv)
    return H


def _check(lib, H, nvt, vs_f64=True):
    H32 = H.astype(np.float32)
    buf = _buffer(H32, nvt)
    om = _run(lib, nvt, 0, buf)
    ov = _run(lib, nvt, 1, buf)
    for o in (om, ov):
        assert np.isfinite(o).all()
        iu = np.triu_indices(nvt)
        assert (o[:, iu[0], iu[1]] == 0).all()           # exact zeros from the diagonal on
    Lm, im = om[:, :, :nvt].astype(np.float64), om[:, :, nvt].astype(np.float64)
    Lv, iv = ov[:, :, :nvt].astype(np.float64), ov[:, :, nvt].astype(np.float64)
    scale = np.maximum(1.0, np.abs(Lv).max(axis=(1, 2)))[:, None, None]
    assert (np.abs(Lm - Lv) / scale).max() <= 1e-5
    assert (np.abs(im - iv) / np.abs(iv)).max() <= 1e-5
    if vs_f64:
        L64, D64 = _ldl64(H32.astype(np.float64))
        scale = np.maximum(1.0, np.abs(L64).max(axis=(1, 2)))[:, None, None]
        assert (np.abs(Lm - L64) / scale).max() <= 1e-4, (np.abs(Lm - L64) / scale).max()
        assert (np.abs(1.0 / im - D64) / np.abs(D64)).max() <= 1e-4
        # backward error of the float32 factor: L D L^T reproduces H to float32 round-off
        U = Lm + np.eye(nvt)
        R = U @ (U / im[:, None, :]).transpose(0, 2, 1) - H32
        assert (np.linalg.norm(R, axis=(1, 2)) / np.linalg.norm(H32, axis=(1, 2))).max() <= 1e-5
    # the MFMA's k-ordered fma chain applies each trailing update exactly as chol_rows does: the two factors are the same bits
    assert (om.view(np.uint32) == ov.view(np.uint32)).all(), int((om != ov).sum())


@pytest.mark.gpu
def test_ldl_mfma_random(harness):
    rng = np.random.default_rng(1)
    _check(harness, _spd_random(rng, 4000, 24), 24)


@pytest.mark.gpu
def test_ldl_mfma_hand_with_contacts(harness):
    rng = np.random.default_rng(2)
    H = _hand_like(rng, 3000, 24)
    # stiff contacts make the float64 forward error of L large; the VALU factor is the yardstick here, and the backward error below
    _check(harness, H, 24, vs_f64=False)
    om = _run(harness, 24, 0, _buffer(H.astype(np.float32), 24))
    U = om[:, :, :24].astype(np.float64) + np.eye(24)
    R = U @ (U / om[:, :, 24].astype(np.float64)[:, None, :]).transpose(0, 2, 1) - H.astype(np.float32)
    assert (np.linalg.norm(R, axis=(1, 2)) / np.linalg.norm(H, axis=(1, 2))).max() <= 1e-5


@pytest.mark.gpu
def test_ldl_mfma_clamped_pivots(harness):
    rng = np.random.default_rng(3)
    H = _singular(rng, 1500, 24)
    om = _run(harness, 24, 0, _buffer(H.astype(np.float32), 24))
    assert (om[:, :, 24] > 1e14).sum() == 3 * H.shape[0]   # every zero-mass dof's pivot reached the clamp (1 / D = 1 / MINVALF)
    _check(harness, H, 24, vs_f64=False)


@pytest.mark.gpu
def test_ldl_mfma_padded_rows(harness):
    rng = np.random.default_rng(4)
    _check(harness, _padded(rng, 1500, 24), 24)


@pytest.mark.gpu
def test_ldl_mfma_odd_size(harness):
    """NVT = 17: the partial register rows of the tile and a last panel whose second column is padding."""
    rng = np.random.default_rng(5)
    _check(harness, _spd_random(rng, 500, 17), 17)
    _check(harness, _padded(rng, 500, 17), 17)
