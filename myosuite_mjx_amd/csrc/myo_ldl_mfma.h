// myo_ldl_mfma.h -- the dense L D L^T of the Newton Hessian on the FP32 matrix cores (v_mfma_f32_32x32x2_f32).
// Part of the single translation unit myo_hip.hip (included by myo_kernel_wave.h after chol_rows); not a stand-alone header.
#ifndef MYO_LDL_MFMA_H
#define MYO_LDL_MFMA_H

// 0: the Newton refactor runs chol_rows on the VALU like every other factorisation (A/B builds differ only in this switch)
#ifndef MYO_LDL_MFMA
#define MYO_LDL_MFMA 1
#endif

typedef float myo_v16f __attribute__((ext_vector_type(16)));

// H = L D L^T of the NVT x NVT matrix in LDS (NVT <= 32), in place, with the contract of chol_rows at the Newton refactor site:
//   in:  S[i * (NVT + 1) + k] = H[i][k], row-major, lower triangle (k <= i) valid; the entries above the diagonal are read but never reach
//        the result;
//   out: S[i * (NVT + 1) + k] = L[i][k] for k < i and exact zeros from the diagonal on (unit lower L), S[i * (NVT + 1) + NVT] = 1 / D[i].
// The matrix sits in one 32 x 32 accumulator tile, transposed: tile[a][b] = H[b][a], so tile row a with lane = b holds the column a of H
// that chol_rows keeps in r[a] with lane = row.  Accumulator layout of the 32x32 MFMA: lane l, register r <-> tile row
// 8 (r / 4) + 4 (l / 32) + r % 4, tile column l % 32.  Rows and columns NVT..31 start as the identity; nothing reads a register before it
// is written.
// Two columns j, j + 1 per panel step: the pivots come from v_readlane at compile-time lanes (clamped and inverted as in chol_rows),
// column j + 1 takes its update from column j on the VALU, and the trailing update of both is one MFMA, tile += A B with
// A[a][k] = D_k L[a][k] (column k of the panel, zero on and above the pivot) and B[k][b] = -L[b][k].  The MFMA result is the k-ordered
// fma chain (one rounding per product), so each entry of the trailing block takes exactly the updates chol_rows applies to it, in the
// same order.  Rows j, j + 1 and columns <= j + 1 of the tile also change under that MFMA; no later step reads them (a panel reads its two
// rows only right of the pivot), and L goes to LDS column by column as each panel finishes.
// Cost per factorisation (NVT = 24): 16 LDS reads, 12 panels of ~20 VALU / 3 v_readlane / 1 permlane32_swap / 1 LDS write, 11 MFMAs --
// against ~650 VALU instructions of chol_rows, whose 24-lane FMAs the matrix core now runs beside the other waves' VALU work.
template <int NVT> __device__ __forceinline__ void ldl_mfma(float* S, int lane) {
  static_assert(NVT <= 32, "ldl_mfma: one 32 x 32 tile");
  const int c = lane & 31, hi = lane >> 5;             // tile column = row of H held by this lane, half of the wave
  const bool cin = c < NVT;
  const int row = (cin ? c : 0) * (NVT + 1);
  const float* Hc = S + row + 4 * hi;                   // row c of H from column 4 * hi on (the tile rows of the upper half are 4 further)
  myo_v16f t;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int a0 = 8 * (r / 4) + r % 4, a = a0 + 4 * hi;   // tile row of register r (a0: compile-time after unrolling)
    if (a0 + 4 < NVT) { const float v = Hc[a0]; t[r] = cin ? v : 0.f; }
    else if (a0 >= NVT) t[r] = c == a ? 1.f : 0.f;
    else t[r] = a < NVT ? (cin ? Hc[a0] : 0.f) : (c == a ? 1.f : 0.f);
  }
  float* Lc = S + row + hi;                             // this lane's stores: row c of L, column j (lower half) or j + 1 (upper half)
  const int ch = c - hi;                                // this lane keeps 1 / D of row c after the panel with j == c - hi
  float invd = 1.f;
#pragma unroll
  for (int j = 0; j < NVT; j += 2) {
    const int h = (j >> 2) & 1, rj = 4 * (j >> 3) + (j & 3);   // tile rows j, j + 1: registers rj, rj + 1 of half h
    const float x0 = t[rj], x1 = t[rj + 1];
    const float ip0 = __builtin_amdgcn_rcpf(fmaxf(rdlane(x0, 32 * h + j), MINVALF));
    const float e = rdlane(x0, 32 * h + j + 1);                // D_j L[j+1][j]
    const float col0 = c > j ? x0 : 0.f;
    const float lt0 = col0 * ip0;
    const float y1 = x1 - lt0 * e;                             // column j + 1 after column j's update (chol_rows: r[j+1] -= lt * rdlane(col, j+1))
    const float ip1 = __builtin_amdgcn_rcpf(fmaxf(rdlane(y1, 32 * h + j + 1), MINVALF));
    const float col1 = c > j + 1 ? y1 : 0.f;
    // both columns are in half h: one half-wave exchange makes [column j | column j + 1] = the A operand (lane = row a + 32 k)
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(col0), __float_as_uint(col1), false, false);
    const float A = __uint_as_float(h ? sw[1] : sw[0]);
    const float ipv = hi ? ip1 : ip0;
    const float Ls = A * ipv;                                  // [L[.][j] | L[.][j+1]], bitwise lt0 / col1 * ip1
    if (cin) Lc[j] = Ls;
    invd = ch == j ? ipv : invd;
    if (j + 2 < NVT) t = __builtin_amdgcn_mfma_f32_32x32x2f32(A, -Ls, t, 0, 0, 0);
  }
  if (cin && (c & 1) == hi) S[row + NVT] = invd;
}

#endif  // MYO_LDL_MFMA_H
