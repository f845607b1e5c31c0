// myo_wave_util.h -- register / cross-lane helpers of the wave kernel, WaveCfg (what the template parameters imply), the stage context
// Part of the single translation unit myo_hip.hip (included by myo_kernel_wave.h); not a stand-alone header.
#ifndef MYO_WAVE_UTIL_H
#define MYO_WAVE_UTIL_H

__device__ __forceinline__ float rdlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int rdlanei(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
// wave-uniform float kept in a scalar register (a VGPR copy of it would be one more value live across every stage)
__device__ __forceinline__ float uniformf(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// sum over the 64 lanes, result in every lane
__device__ __forceinline__ float wave_sum(float v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  v = dpp_add<0x140>(v);  // row_mirror  -> every lane of a 16-lane row holds the row sum
  return (rdlane(v, 0) + rdlane(v, 16)) + (rdlane(v, 32) + rdlane(v, 48));
}
#define WFOR(i, n) for (int i = lane; i < (n); i += 64)
// this lane's index in the wave, recomputed where it is needed (two instructions): a copy of threadIdx.x kept for the whole kernel is a
// register that is live across every stage, and was the first thing the allocator spilled
__device__ __forceinline__ int wave_lane() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
// dof id k (0..KC-1) of contact c from the byte-packed table (CDW = ints per contact, a constexpr of the kernel)
#define CDOF(E_, Y_, c_, k_) ((int)((((const unsigned int*)((E_) + (Y_).cdofs))[CDW * (c_) + ((k_) >> 2)] >> (8 * ((k_) & 3))) & 255u))
// same from a pointer to the contact's own packed words (LDS row or HBM overflow row)
#define CDOFP(W_, k_) ((int)(((W_)[(k_) >> 2] >> (8 * ((k_) & 3))) & 255u))

// Register factorisation H = L D L^T (unit lower L, D = pivots), lane = row.  in: r[k] = H[lane][k] for k <= lane and ZERO above the diagonal.
// out: r[k] = L[lane][k] for k < lane and zero from the diagonal on; returns 1 / D[lane].  All indices are compile-time.
// Right-looking (outer-product) order: once column j is final, every later column k takes its update r[k] -= L[.][j] (D_j L[k][j]) at once, so the
// NVT - 1 - j updates of a step are independent of each other and the dependent chain of a factorisation is the NVT pivot steps.
// Why L D L^T rather than Cholesky: no square root (v_rcp of the pivot), and both triangular solves run on the SAME unit-diagonal factor with no
// division or scaling per step -- two instructions per forward step, three per backward step (ldl_solve_rows), against seven before.  The zeros from
// the diagonal on are what lets the solves skip every lane test: a lane above the diagonal multiplies by an exact zero.
template <int NVT> __device__ __forceinline__ float chol_rows(float (&r)[NVT], int lane) {
  float invd = 1.0f;
#pragma unroll
  for (int j = 0; j < NVT; j++) {
    const float pj = fmaxf(rdlane(r[j], j), MINVALF);
    const float ip = __builtin_amdgcn_rcpf(pj);   // v_rcp_f32 (1 ulp); pj >= 1e-15, no denormal handling needed
    const float col = lane > j ? r[j] : 0.f;      // D_j L[lane][j]; zero on and above the diagonal, so those lanes take no update below
    const float lt = col * ip;
    r[j] = lt;
    if (lane == j) invd = ip;
#pragma unroll
    for (int k = j + 1; k < NVT; k++) r[k] -= lt * rdlane(col, k);
  }
  return invd;
}
#include "myo_ldl_mfma.h"
// 0: the dynamics stage writes M symmetrically into the square buffer and every Newton refactor refills the buffer from the packed copy, the first
// one of a substep included (A/B builds differ only in this switch)
#ifndef MYO_MHL_A
#define MYO_MHL_A 1
#endif
// 0: the packed copy of M is made one lane per row
#ifndef MYO_MHL_B
#define MYO_MHL_B 1
#endif
// 0: the later refactors of a substep refill the whole Hessian buffer from the packed copy, one lane per row
#ifndef MYO_MHL_E
#define MYO_MHL_E 1
#endif
// is dof a an ancestor of dof d?
template <int SPEC> __host__ __device__ constexpr bool tree_anc(int a, int d) {
  int p = SpecTree<SPEC>::parent[d];
  while (p >= 0) { if (p == a) return true; p = SpecTree<SPEC>::parent[p]; }
  return false;
}
// chol_rows on the leaves-first permuted matrix of a tree-structured model: the updates whose factor entry L[K][J] is structurally zero
// (dof of K is not an ancestor of the dof of J) are not emitted (`if constexpr` over index sequences: a run-time predicate inside
// `#pragma unroll` loops blocked the unrolling and put the rows into scratch memory).  Right-looking like chol_rows.
template <int NVT, int SPEC, int J, int K> __device__ __forceinline__ void tree_update(float (&r)[NVT], float lt, float col) {
  constexpr int nv = SpecTree<SPEC>::nv;
  if constexpr (K > J && J < nv && K < nv) {
    if constexpr (tree_anc<SPEC>(nv - 1 - K, nv - 1 - J)) r[K] -= lt * rdlane(col, K);
  }
}
template <int NVT, int SPEC, int J, int... Ks> __device__ __forceinline__ void tree_col(float (&r)[NVT], float lt, float col, std::integer_sequence<int, Ks...>) {
  (tree_update<NVT, SPEC, J, Ks>(r, lt, col), ...);
}
template <int NVT, int SPEC, int J> __device__ __forceinline__ void tree_step(float (&r)[NVT], float& invd, int lane) {
  const float pj = fmaxf(rdlane(r[J], J), MINVALF);
  const float ip = __builtin_amdgcn_rcpf(pj);
  const float col = lane > J ? r[J] : 0.f;
  const float lt = col * ip;
  r[J] = lt;
  if (lane == J) invd = ip;
  tree_col<NVT, SPEC, J>(r, lt, col, std::make_integer_sequence<int, NVT>{});
}
template <int NVT, int SPEC, int... Js> __device__ __forceinline__ void tree_all(float (&r)[NVT], float& invd, int lane, std::integer_sequence<int, Js...>) {
  (tree_step<NVT, SPEC, Js>(r, invd, lane), ...);
}
template <int NVT, int SPEC> __device__ __forceinline__ float chol_rows_tree(float (&r)[NVT], int lane) {
  float invd = 1.0f;
  tree_all<NVT, SPEC>(r, invd, lane, std::make_integer_sequence<int, NVT>{});
  return invd;
}
// x <- (L D L^T)^-1 b ; rows of the unit lower L in registers (zero from the diagonal on), invd = 1 / D[lane], the columns of L^T read from the
// LDS copy T[j * (NVT + 1) + lane] (row j of L: zero for lane >= j)
template <int NVT> __device__ __forceinline__ float chol_solve_rows(const float (&r)[NVT], float invd, float b, const float* T, int lane) {
  float y = b;
#pragma unroll
  for (int j = 0; j < NVT; j++) y = fmaf(-r[j], rdlane(y, j), y);
  y *= invd;
  const float* Tc = T + (lane < NVT ? lane : 0);
#pragma unroll
  for (int j = NVT - 1; j >= 0; j--) y = fmaf(-Tc[j * (NVT + 1)], rdlane(y, j), y);
  return y;
}
// y_lane = sum_k M[lane][k] x_k with M packed lower-triangular in LDS (rows beyond nv read as zero)
template <int NVT> __device__ __forceinline__ float symv_lds(const float* Mp, float x, int lane, int nv) {
  float s = 0;
  const int d = lane < nv ? lane : 0;
  const int based = (d * (d + 1)) / 2;
#pragma unroll
  for (int k = 0; k < NVT; k++) {
    int kk = k < nv ? k : 0;
    int adr = (kk <= d) ? based + kk : (kk * (kk + 1)) / 2 + d;
    float mv = (k < nv && lane < nv) ? Mp[adr] : 0.f;
    s += mv * rdlane(x, k);
  }
  return s;
}

// The lower triangle of an NVT x NVT matrix (diagonal included, NVT even) spread over the lanes: rows p and NVT - 1 - p have NVT + 1 entries together,
// so entry i of an NVT / 2 x (NVT + 1) grid is (row d, column k <= d) with no square root and no table; i = lane + 64 t covers TRI_N entries.
template <int NVT> constexpr int TRI_N = (NVT / 2) * (NVT + 1);
template <int NVT> __device__ __forceinline__ void tri_pair(int i, int& d, int& k) {
  const int p = i / (NVT + 1), c = i - p * (NVT + 1);
  d = c <= p ? p : NVT - 1 - p;
  k = c <= p ? c : c - p - 1;
}

template <class LY> __device__ __forceinline__ void site_world_w(const DevModel& M, const LY& Y, const float* E, int s, float* out) {
  int l = M.site_link[s];
  const float* lp = M.site_lpos + 3 * s;
  float a = lp[0], b = lp[1], c = lp[2];
  if (l < 0) { out[0] = a; out[1] = b; out[2] = c; return; }
  const float* R = E + Y.lmat + 9 * l;
  const float* P = E + Y.lpos + 3 * l;
  out[0] = P[0] + R[0] * a + R[1] * b + R[2] * c;
  out[1] = P[1] + R[3] * a + R[4] * b + R[5] * c;
  out[2] = P[2] + R[6] * a + R[7] * b + R[8] * c;
}
// world position of a point given in a link's frame (link < 0: world-fixed)
template <class LY> __device__ __forceinline__ void frame_point(const LY& Y, const float* E, int l, const float* lp, float* out) {
  if (l < 0) { out[0] = lp[0]; out[1] = lp[1]; out[2] = lp[2]; return; }
  const float* R = E + Y.lmat + 9 * l;
  const float* P = E + Y.lpos + 3 * l;
  out[0] = P[0] + R[0] * lp[0] + R[1] * lp[1] + R[2] * lp[2];
  out[1] = P[1] + R[3] * lp[0] + R[4] * lp[1] + R[5] * lp[2];
  out[2] = P[2] + R[6] * lp[0] + R[7] * lp[1] + R[8] * lp[2];
}
// per-env orientation of one world-welded body (MYO_F_BODYQUAT; the TRK instantiation passes it, every other one a constant nullptr): the
// body's static collision geoms turn about its origin p_b, x = p_b + D (x0 - p_b) and R = D R0 with D = R(q_env) R(q0)^T.  Wave-uniform.
struct BodyRot {
  const float* q;      // this env's quaternion (NULL: off)
  const float* c;      // R(q0)^T (9, row-major) | p_b (3)
  const int* flag;     // per collision geom: 1 on that body
  // per-env object parameters (DevBatch.objk; TRK instantiation only): this env's rows and the slot table; og NULL: off.  Wave-uniform too
  const float* og;     // [obj_ng][12]
  const int* oslot;    // per collision geom: its row, -1: not selected
};
// the BodyRot of env `env` (trk / obj: WaveCfg's TRK and OBJ; where they are false the members are constant nullptrs and the code behind them goes away)
__device__ __forceinline__ BodyRot body_rot_of(const DevBatch& Bt, int env, bool trk, bool obj) {
  return BodyRot{trk && Bt.bquat ? Bt.bquat + 4 * (size_t)env : nullptr, Bt.bq_c, Bt.bq_flag,
                 obj && Bt.objk ? Bt.objk + 12 * (size_t)env * Bt.obj_ng : nullptr, obj ? Bt.obj_slot : nullptr};
}
__device__ __forceinline__ void body_rot(const BodyRot& br, float* D) {
  const float q[4] = {br.q[0], br.q[1], br.q[2], br.q[3]};
  float Rq[9];
  quat2mat(Rq, q);
  matmul3(D, Rq, br.c);
}
// ... of a static point of that body, in place: x = p_b + D (x - p_b)
__device__ __forceinline__ void body_rot_point(const BodyRot& br, float* x) {
  float D[9], v[3];
  const float d[3] = {x[0] - br.c[9], x[1] - br.c[10], x[2] - br.c[11]};
  body_rot(br, D);
  matvec(v, D, d);
  x[0] = br.c[9] + v[0]; x[1] = br.c[10] + v[1]; x[2] = br.c[11] + v[2];
}
// world centre / rotation of collision geom g from its record (DevModelW::cg_rec: link, lpos | rotation | type, bounding radius)
template <class LY> __device__ __forceinline__ void geom_world_pos(const DevModelW& W, const LY& Y, const float* E, int g, float* out) {
  const float4 r0 = W.cg_rec[4 * g];
  const float lp[3] = {r0.y, r0.z, r0.w};
  frame_point(Y, E, __float_as_int(r0.x), lp, out);
}
template <class LY> __device__ __forceinline__ void geom_world_mat(const DevModelW& W, const LY& Y, const float* E, int g, float* R) {
  const gpf4 G = W.cg_rec + 4 * g;
  const float4 r0 = G[0], r1 = G[1], r2 = G[2], r3 = G[3];
  const int l = __float_as_int(r0.x);
  const float lm[9] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x};
  if (l < 0) {
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = lm[k];
  } else {
    matmul3(R, E + Y.lmat + 9 * l, lm);
  }
}
// ... with the per-env orientation of BodyRot (br: a constant nullptr outside the TRK instantiation, which leaves the two calls above)
template <class LY> __device__ __forceinline__ void geom_world_pos(const DevModelW& W, const LY& Y, const float* E, int g, float* out, const BodyRot* br) {
  if (br && br->og) {   // a selected geom's centre is the env's (a geom of a moving link: myo_objects_enable refuses world-welded ones)
    const int s = br->oslot[g];
    if (s >= 0) {
      const float* o = br->og + 12 * s + 4;
      const float lp[3] = {o[0], o[1], o[2]};
      frame_point(Y, E, __float_as_int(W.cg_rec[4 * g].x), lp, out);
      return;
    }
  }
  geom_world_pos(W, Y, E, g, out);
  if (br && br->q && __float_as_int(W.cg_rec[4 * g].x) < 0 && br->flag[g]) body_rot_point(*br, out);
}
template <class LY> __device__ __forceinline__ void geom_world_mat(const DevModelW& W, const LY& Y, const float* E, int g, float* R, const BodyRot* br) {
  geom_world_mat(W, Y, E, g, R);
  if (br && br->q && __float_as_int(W.cg_rec[4 * g].x) < 0 && br->flag[g]) {
    float D[9];
    body_rot(*br, D);
    matmul3(R, D, R);   // (matmul3 writes through a temporary)
  }
}
// moment-arm entries of one straight tendon piece
// Jt = this tendon's sparse jacobian row in LDS (zeroed before the segment rounds): the entries are accumulated with LDS float atomics
// by the segment lanes themselves (one wave: deterministic order) instead of being gathered entry by entry by the tendon's lane
#if defined(__HIP_DEVICE_COMPILE__)
typedef const int4 __attribute__((address_space(1)))* gpi4;
#else
typedef const int4* gpi4;
#endif
template <class LY> __device__ __forceinline__ float straight_w(const DevModelW& W, const LY& Y, float* E, float* Jt, const float* pa, const float* pb, int adr4, int n,
                                                              float invdiv, bool active, const int4& first) {
  float dif[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
  float dist = norm3(dif);
  float inv = dist > MINVALF ? __builtin_amdgcn_rcpf(dist) : 0.f;   // (the intrinsic: `1.0f / dist` times three became three full divisions)
  dif[0] *= inv; dif[1] *= inv; dif[2] *= inv;
  // a lane that does not keep this piece (wrapping segment vs direct piece, or the reverse) runs zero iterations: the wave's trip count is
  // the longest dof list among the lanes that DO keep it, and zero when none does.  Four entries per 16-byte load; the first row was
  // loaded by the caller ahead of the wrap geometry (`first`), so the usual list (<= 4 entries) costs no exposed load at all.
  const int nn = active ? n : 0;
  for (int k0 = 0; k0 < nn; k0 += 4) {
    int4 q = first;
    if (k0) q = ((gpi4)W.dl_pk)[adr4 + (k0 >> 2)];
    const int qe[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (k0 + u >= nn) continue;
      const int e = qe[u];            // dof | hinge << 7 | row slot << 8 | sign << 16: one word instead of three plus dof_type[dof]
      const int d = e & 127;
      const float* ax = E + Y.axis + 3 * d;
      float col;
      if (e & 128) {
        const float* an = E + Y.anchor + 3 * d;
        float r[3] = {pb[0] - an[0], pb[1] - an[1], pb[2] - an[2]}, c[3];
        cross3(c, ax, r);
        col = dot3(dif, c);
      } else col = dot3(dif, ax);
      atomicAdd(&Jt[(e >> 8) & 255], (float)(e >> 16) * col * invdiv);
    }
  }
  return active ? dist * invdiv : 0.f;
}

// ------------------------------------------------------------------------------------------------
// ---- height field vs convex primitive (mjc_ConvexHField [3P], restated in oracle/myo_oracle.c convex_hfield) -------------------------
// sub-grid of cells under the geom's AABB (rel = geom centre - height field position, ext = AABB half extents); false: cannot touch
__device__ __forceinline__ bool hf_range(const HfDev& H, const float* rel, const float* ext, float rb, float margin, int& r0, int& r1, int& c0, int& c1, float& zmin) {
  if (H.size[0] < rel[0] - rb - margin || -H.size[0] > rel[0] + rb + margin || H.size[1] < rel[1] - rb - margin || -H.size[1] > rel[1] + rb + margin) return false;
  if (H.size[2] < rel[2] - rb - margin || -H.size[3] > rel[2] + rb + margin) return false;
  const float lo[3] = {rel[0] - ext[0], rel[1] - ext[1], rel[2] - ext[2]}, hi[3] = {rel[0] + ext[0], rel[1] + ext[1], rel[2] + ext[2]};
  if (lo[0] - margin > H.size[0] || hi[0] + margin < -H.size[0] || lo[1] - margin > H.size[1] || hi[1] + margin < -H.size[1] ||
      lo[2] - margin > H.size[2] || hi[2] + margin < -H.size[3]) return false;
  c0 = max(0, (int)floorf((lo[0] + H.size[0]) / (2.f * H.size[0]) * (float)(H.ncol - 1)));
  c1 = min(H.ncol - 1, (int)ceilf((hi[0] + H.size[0]) / (2.f * H.size[0]) * (float)(H.ncol - 1)));
  r0 = max(0, (int)floorf((lo[1] + H.size[1]) / (2.f * H.size[1]) * (float)(H.nrow - 1)));
  r1 = min(H.nrow - 1, (int)ceilf((hi[1] + H.size[1]) / (2.f * H.size[1]) * (float)(H.nrow - 1)));
  zmin = lo[2];
  return r1 > r0 && c1 > c0;
}
// the three strip vertices ending at zig-zag index j of cell row r: vertex jj sits at column jj / 2, row r + 1 (jj even) or r (jj odd)
__device__ __forceinline__ void hf_prism(const HfDev& H, const float* data, int r, int j, float* x, float* y, float* z) {
  const float dx = 2.f * H.size[0] / (float)(H.ncol - 1), dy = 2.f * H.size[1] / (float)(H.nrow - 1);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int jj = j - 2 + k, c = jj >> 1, rr = r + ((jj & 1) ? 0 : 1);
    x[k] = dx * (float)c - H.size[0]; y[k] = dy * (float)rr - H.size[1]; z[k] = data[rr * H.ncol + c] * H.size[2];
  }
}
// walks the prisms of the sub-grid in mjc_ConvexHField's order; counts those whose top is not wholly below the geom and, when out != NULL,
// writes their candidate words (pair | row << 10 | zig-zag index << 17) from position `at`
__device__ __forceinline__ int hf_walk(const HfDev& H, const float* data, int r0, int r1, int c0, int c1, float zcut, int p, int* out, int at, int cap) {
  int n = 0;
  for (int r = r0; r < r1; r++)
    for (int j = 2 * c0 + 2; j <= 2 * c1 + 1; j++) {
      float x[3], y[3], z[3];
      hf_prism(H, data, r, j, x, y, z);
      if (z[0] < zcut && z[1] < zcut && z[2] < zcut) continue;
      if (out && at + n < cap) out[at + n] = p | (r << 10) | (j << 17);
      n++;
    }
  return n;
}

// state rows under the substep scheduler were written by another CU of the XCD: agent-scope loads read them from L2 instead of a possibly stale L1 line
template <bool S> __device__ __forceinline__ float ldstate(const float* p) {
  if (S) return __int_as_float(__hip_atomic_load((const int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  return *p;
}
template <bool S> __device__ __forceinline__ int ldstatei(const int* p) {
  if (S) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

// Everything the wave kernel and its stage functions derive from the ten template parameters, in one place.
template <int NVT_, int KC_, int NC_, int NTR_, int WPE_, bool SCHED_, int SPEC_, bool HF_, bool TRK_, bool RK4_, bool OBJ_ = false> struct WaveCfg {
  static constexpr int NVT = NVT_, KC = KC_, NC = NC_, NTR = NTR_, WPE = WPE_, SPEC = SPEC_;
  static constexpr bool SCHED = SCHED_, HF = HF_, TRK = TRK_, RK4 = RK4_;
  // per-env object parameters (DevBatch.objk / obj_mass): step_kernel_obj and the TRK forward twin; everywhere else the reads are not compiled
  static constexpr bool OBJ = OBJ_;
  static_assert(!OBJ || (TRK && !RK4 && !SCHED && SPEC == 0), "per-env object parameters: the run-time-sized Euler TRK instantiation only");
  static constexpr int CDW = (KC + 3) / 4;   // ints per contact holding its KC byte-packed dof ids
  static constexpr int NJ = TRK ? 4 : 3;     // jacobian rows per contact: normal, two tangents (, spin about the normal)
  static constexpr int NR = TRK ? 6 : 4;     // pyramid rows per contact
  // the small instantiation (hand / finger class) is compiled without the free-joint, equality, plane-contact and condim-1 code;
  // myo_model_load routes any model that needs one of those to the large instantiation
  static constexpr bool FULL = NVT > 24;
  // the lane's full row of the mass matrix stays in registers through the solver (see the row stage)
  static constexpr bool MROW = NVT > 24 && !RK4;      // (the Runge-Kutta twins keep four stage derivatives per lane: no room for the row)
  // the 24-dof kernels: the dynamics stage writes only the lower triangle of M into the square buffer (nothing reads the upper one without MROW),
  // and the first Newton refactor of a substep builds H on that copy instead of refilling the buffer from the packed one
  static constexpr bool MHL_A = MYO_MHL_A && NVT <= 32 && !MROW && !RK4;
  // ... and the later refactors of a substep refill only what L overwrote, with all 64 lanes
  static constexpr bool MHL_E = MYO_MHL_E && NVT <= 32 && !MROW && !RK4;
  // ... and the packed copy of M is made by all 64 lanes
  static constexpr bool MHL_B = MYO_MHL_B && NVT <= 32 && !MROW && !RK4;
  static_assert(!(MHL_E || MHL_B) || NVT % 2 == 0, "tri_pair needs an even NVT");
  static constexpr bool LDL_MFMA = MYO_LDL_MFMA && NVT <= 32;   // Newton refactor on the matrix cores
  // per-env size of one collision geom (DevBatch.gsize), generic FULL instantiations only: the size-specialised and hand kernels keep
  // reading the model tables unconditionally
  static constexpr bool OVR = FULL && SPEC == 0 && !HF;
  // contacts NC .. NC + NCXK - 1 live in this env's HBM overflow rows; lane = contact still holds for all 64.  The first NC contacts (all of
  // them for > 99.5 % of the states) never leave LDS.
  // TRK: a second bank of 64 (contacts 64 .. 127: lane = contact - 64), whose per-contact solver state lives in the contact's row as well
  static constexpr int NCXK = TRK ? (128 - NC) : ((64 - NC) < NCX ? (64 - NC) : NCX);   // overflow rows this instantiation uses
  // narrow-phase round width: the MPR's per-lane LDS scratch (9 floats) lives in the contact-jacobian area, which holds 64 lanes' worth only
  // when NC * NJ * KC >= 576; the low-LDS instantiations (NC = 16) run the narrow phase in rounds of 32 candidates (typical count: 10-20)
  static constexpr int RND = (NC * NJ * KC >= 768) ? 64 : 32;
  static_assert(RND * 12 <= NC * NJ * KC, "MPR scratch must fit the contact-jacobian area");
  static_assert(!(RK4 && SCHED), "the substep scheduler hands out Euler substeps");
  // fields of an overflow row (floats): dist | pos[3] | normal[3] | pair word | cJ[NJ][KC] | dof words[CDW] | (TRK) state block
  enum { O_DIST = 0, O_POS = 1, O_NRM = 4, O_PAIR = 7, O_CJ = 8, O_CDW = 8 + NJ * KC, ROWS = 8 + NJ * KC + CDW };
  // TRK, more than 64 contacts: contact c in [64, 128) belongs to lane c - 64 ("second bank").  Its per-contact solver state -- what bank 0
  // keeps in registers -- lives in a block at offset ROWS of the contact's overflow row, is loaded where a stage needs it and stored
  // back; loops over (contact, dof slot) read a bank-1 contact's coefficients from that block instead of shuffling them out of registers.
  // Everything of it sits behind `bank1` (wave-uniform, ncon > 64): the common case pays a scalar test per stage.
  enum { S_AREF = 0, S_D = NR, S_MU = NR + 1, S_MUT = NR + 2, S_D2 = NR + 3, S_KC = NR + 4, S_JAR = NR + 5, S_JV = 2 * NR + 5, S_FC = 3 * NR + 5, S_HC = 3 * NR + 9, S_SIG = 3 * NR + 16 };
  static_assert(!TRK || 3 * NR + 17 <= TRK_STATE, "state block of a second-bank contact");
};
// One way to reach the row of contact c: the first NC rows are LDS tables, the later ones the env's HBM overflow rows.  f is called from two
// separate branches, once with LDS pointers and once with global ones, so that each inlined copy keeps its own address space (one pointer
// selected by ?: would be a generic pointer and every access through it a flat one).
struct ConRow { float *dist, *pos, *nrm; int* pair; float* cJ; unsigned int* cdw; };
template <class C, class LY, class F> __device__ __forceinline__ void con_row(const LY& Y, float* E, float* ovf_env, int ovf_row, int c, F&& f) {
  if (c < C::NC) f(ConRow{E + Y.cdist + c, E + Y.cpos + 3 * c, E + Y.cnrm + 3 * c, (int*)(E + Y.cpair) + c, E + Y.cJ + c * C::NJ * C::KC, (unsigned int*)(E + Y.cdofs) + C::CDW * c});
  else { float* g = ovf_env + (c - C::NC) * ovf_row; f(ConRow{g + C::O_DIST, g + C::O_POS, g + C::O_NRM, (int*)g + C::O_PAIR, g + C::O_CJ, (unsigned int*)(g + C::O_CDW)}); }
}
// second-bank state block of contact c (TRK, c >= 64)
template <class C> __device__ __forceinline__ float* bank1_state(float* ovf_env, int ovf_row, int c) { return ovf_env + (size_t)(c - C::NC) * ovf_row + C::ROWS; }

// pair record -> locals.  (OVR: one geom's size / bounding radius may be a per-env value, DevBatch.gsize; TRK: those of the selected geoms
// are the env's rows, DevBatch.objk -- the OVR idea with a slot table, collision geom -> row or -1, instead of one geom id)
struct PairL { int g1, g2, dl, kc, pt, cd, t1, t2; float margin, gap, rb1, rb2, s1[3], s2[3]; };
struct PairRaw { float4 q0, q1, q2, q3; };
__device__ __forceinline__ PairRaw pair_raw(const DevModelW& W, int p) { const gpf4 Q = W.pair_rec + 4 * (size_t)p; return PairRaw{Q[0], Q[1], Q[2], Q[3]}; }
template <class C> __device__ __forceinline__ PairL pair_decode(const DevBatch& Bt, int env, const PairRaw& r) {
  constexpr bool OVR = C::OVR;
  const float4 q0 = r.q0, q1 = r.q1, q2 = r.q2, q3 = r.q3;
  const int w = __float_as_int(q0.x), tt = __float_as_int(q3.x);
  PairL L;
  L.g1 = w & 255; L.g2 = (w >> 8) & 255; L.pt = (w >> 16) & 15; L.cd = (w >> 20) & 15; L.kc = (w >> 24) & 255; L.dl = __float_as_int(q0.w);
  L.margin = q0.y; L.gap = q0.z; L.t1 = tt & 255; L.t2 = (tt >> 8) & 255;
  L.s1[0] = q1.x; L.s1[1] = q1.y; L.s1[2] = q1.z; L.rb1 = q1.w; L.s2[0] = q2.x; L.s2[1] = q2.y; L.s2[2] = q2.z; L.rb2 = q2.w;
  if (OVR && Bt.gsize) {
    const float* G = Bt.gsize + 4 * (size_t)env;
    if (L.g1 == Bt.gsize_cg) { L.s1[0] = G[0]; L.s1[1] = G[1]; L.s1[2] = G[2]; L.rb1 = G[3]; }
    if (L.g2 == Bt.gsize_cg) { L.s2[0] = G[0]; L.s2[1] = G[1]; L.s2[2] = G[2]; L.rb2 = G[3]; }
  }
  if (C::OBJ && Bt.objk) {
    const float* G = Bt.objk + 12 * (size_t)env * Bt.obj_ng;
    const int a = Bt.obj_slot[L.g1], b = Bt.obj_slot[L.g2];
    if (a >= 0) { const float* S = G + 12 * a; L.s1[0] = S[0]; L.s1[1] = S[1]; L.s1[2] = S[2]; L.rb1 = S[3]; }
    if (b >= 0) { const float* S = G + 12 * b; L.s2[0] = S[0]; L.s2[1] = S[1]; L.s2[2] = S[2]; L.rb2 = S[3]; }
  }
  return L;
}
// per-env friction of the pair (g1, g2) when one of its geoms is selected (Bt.objk set): lowering._contact_params' mix with the env's
// rows in place of the selected geoms' compiled friction -- priorities differ: the higher priority's, else the component-wise maximum; both
// floored at 1e-5 as MuJoCo floors them.  mu:
// sliding, mut: torsional (the caller uses it for condim-4 pairs only).  A pair without a selected geom keeps the pair table's values
__device__ __forceinline__ void obj_pair_friction(const DevBatch& Bt, int env, int g1, int g2, float& mu, float& mut) {
  const int a = Bt.obj_slot[g1], b = Bt.obj_slot[g2];
  if (a < 0 && b < 0) return;
  const float* G = Bt.objk + 12 * (size_t)env * Bt.obj_ng;
  const float *c1 = Bt.obj_cgf + 4 * g1, *c2 = Bt.obj_cgf + 4 * g2;
  const float *f1 = a >= 0 ? G + 12 * a + 8 : c1, *f2 = b >= 0 ? G + 12 * b + 8 : c2;
  const float p1 = c1[3], p2 = c2[3];
  if (p1 != p2) { const float* f = p1 > p2 ? f1 : f2; mu = f[0]; mut = f[1]; }
  else { mu = fmaxf(f1[0], f2[0]); mut = fmaxf(f1[1], f2[1]); }
  // mj_contactParam's floor (mjMINMU): a row of zeros must not turn a frictional pair into a frictionless one (mu == 0 is how the row stage
  // and the efc count recognise a condim-1 pair)
  mu = fmaxf(mu, 1e-5f); mut = fmaxf(mut, 1e-5f);
}
template <class C> __device__ __forceinline__ PairL pair_load(const DevModelW& W, const DevBatch& Bt, int env, int p) { return pair_decode<C>(Bt, env, pair_raw(W, p)); }

// What every stage of a substep needs, by reference or as a scalar: the model, the layout of the LDS slice, the batch, this wave's env, the
// sizes (compile-time constants in the size-specialised instantiations) and the env's overflow rows.  The LDS slice itself is not a member:
// a stage names it as the kernel does, `extern __shared__ float E[]` -- as a pointer carried in here it is a generic pointer that starts at LDS
// address 0, and every address formed from it pays a null test on the way back to LDS (measured: -1.8 % on the headline).  Values that cross a stage boundary in
// registers are NOT here: they are parameters of the stages that produce and consume them.
template <class LY> struct WaveCtx {
  const DevModel& M; const DevModelW& W; const LY& Y; const DevBatch& Bt; const DevWalk* wk;
  int env, nv, nu, nq, nl_, nlevel_, maxnnz_, ngt_, nseg_, ncg_, npair_;
  bool has_free; int neq; bool has_tl;
  float h; int nsub, kflags;
  float* ovf_env; int ovf_row, nct; int* ovf_cand;
};
// Per-lane values that travel together from the row stages to the solver (and the sensor readout)
struct LimRow { float sign, aref, D; };                                          // joint-limit row of lane = dof (sign 0: inactive)
template <int NR> struct ConConst { float aref[NR], D, mu, mut, D2; int kc; };   // lane = contact: aref of its pyramid rows, weight, friction (TRK: torsional), dof count
struct FricLoss { float f, D, aref, rf; };                                       // TRK friction-loss row of lane = dof (f 0: none)
struct EqRow { float J2, D, aref; int d1, d2; bool act; };                       // joint-coupling equality of lane = equality
// RK4: X0 and the weighted sums of the stage derivatives, lane = dof / lane = actuator
template <int NTR> struct RkAcc { float v0, q0, sv, sa, t0, quat[4], a0[NTR], sd[NTR]; };

// finer timing split of the diagnostic build (MYO_STAMPS): second and last third of the stamps buffer.  x: [0] cycles of the dense Newton
// refactors, [1] cycles of the tree-sparse M / M + h D factorisations (both out of sub[2]), [2] number of dense Newton refactors
#if MYO_STAMPS
struct SubStamps { long long sub[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, s0 = 0, x[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; };
#define SUB0() do { st_.s0 = clock64(); } while (0)
#define SUB(k) do { long long t1_ = clock64(); st_.sub[k] += t1_ - st_.s0; st_.s0 = t1_; } while (0)
#define SUBX(k) do { long long t1_ = clock64(); st_.x[k] += t1_ - st_.s0; st_.s0 = t1_; } while (0)
#define CNTX(k) do { st_.x[k]++; } while (0)
#else
struct SubStamps {};
#define SUB0() do { } while (0)
#define SUB(k) do { } while (0)
#define SUBX(k) do { } while (0)
#define CNTX(k) do { } while (0)
#endif
#define lane_id wave_lane()

#endif  // MYO_WAVE_UTIL_H
