// myo_kernel_forward.h -- forward pass without a step (include/myo_hip_forward.h): forward_kernel_w, one wave per env, runs the step kernel's
// own stages w_check_state, w_kinematics, w_broad_phase and w_narrow_phase on the batch's state and exports body, site and geom frames and
// the contact list.  Host half: the export tables, built at model load from arrays every blob has, and the batch's forward buffers.
// Part of the single translation unit myo_hip.hip (included there, after the host headers); not a stand-alone header.
#ifndef MYO_KERNEL_FORWARD_H
#define MYO_KERNEL_FORWARD_H

// Export tables, one 16-float record per body / site / geom (four 16-byte loads per lane, like DevModelW::cg_rec):
//   link (bits; < 0: welded to the world) | position (3) | rotation (9, row-major), both in the link's frame (world-welded: lowered world
//   coordinates, i.e. relative to DevModel::origin) | bodies: the body's COM in the link's frame (3); sites and geoms: their body (bits), -, -
// and what a launch writes.  Passed by value.
#define FWD_REC 16
#define FWD_CON 16   // floats of a contact record: dist | pos (3) | frame (9: normal, tangent 1, tangent 2) | geom1, geom2, pair (int32)
struct FwdDev {
  int nbody, nsite, ngeom, ncap;        // ncap: contact records per env (the LDS rows plus the overflow rows of the model's kernel class)
  int has_site_mat;                     // the blob carries site_quat: site_xmat is exported
  int bq_body;                          // body of MYO_F_BODYQUAT (-1: none): its items turn about the body's origin, as its collision geoms do in a step
  const float* goal_off;                // die task: [B][3] MYO_F_TARGET, the per-env offset of that body (the task's goal); NULL otherwise
  gpf4 body_rec, site_rec, geom_rec;
  gpi cg_geom;                          // collision geom -> model geom id
  float *xpos, *xmat, *xipos, *site_xpos, *site_xmat, *geom_xpos, *geom_xmat, *contact;
  int* ncon;
};

struct FwdItem { int link; float p[3], R[9], a[3]; };
__device__ __forceinline__ FwdItem fwd_item(gpf4 T, int i) {
  const float4 r0 = T[4 * (size_t)i], r1 = T[4 * (size_t)i + 1], r2 = T[4 * (size_t)i + 2], r3 = T[4 * (size_t)i + 3];
  return FwdItem{__float_as_int(r0.x), {r0.y, r0.z, r0.w}, {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x}, {r3.y, r3.z, r3.w}};
}
// a static point of the per-env posed body: turned about the body's origin (MYO_F_BODYQUAT), then moved by the env's goal offset (die task)
__device__ __forceinline__ void fwd_move_point(const BodyRot& br, const float* off, float* x) {
  if (br.q) body_rot_point(br, x);
  if (off) { x[0] += off[0]; x[1] += off[1]; x[2] += off[2]; }
}
// world frame (lowered coordinates) of an item from the link frames in LDS; moved: a static item of the per-env posed body
template <class LY> __device__ __forceinline__ void fwd_world(const LY& Y, const float* E, const FwdItem& I, const BodyRot& br, bool moved, const float* off, float* x, float* R) {
  frame_point(Y, E, I.link, I.p, x);
  if (I.link < 0) {
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = I.R[k];
  } else matmul3(R, E + Y.lmat + 9 * I.link, I.R);
  if (moved) {
    fwd_move_point(br, off, x);
    if (br.q) {
      float D[9];
      body_rot(br, D);
      matmul3(R, D, R);
    }
  }
}
__device__ __forceinline__ void fwd_store(float* xo, float* Ro, size_t i, const float* org, const float* x, const float* R) {
#pragma unroll
  for (int k = 0; k < 3; k++) xo[3 * i + k] = x[k] + org[k];
  if (Ro) {
#pragma unroll
    for (int k = 0; k < 9; k++) Ro[9 * i + k] = R[k];
  }
}

// One wave per env, dynamic LDS with the model's run-time layout W.lay.  The template arguments are those of the step kernel of the model's
// size class (WK_HAND, WK_LEG, WK_TERRAIN, WK_TRK), so the stages compile as they do there.  LDS regions: qpos, qvel (loaded here);
// lpos, lmat, axis, anchor and the scratch sq (w_kinematics); gpos, gax, cand (w_broad_phase); cdist, cpos, cnrm, cpair, the MPR scratch at
// the head of cJ, and mprw with no entry going in (w_narrow_phase).  Writes nothing of the batch but flags and the env's overflow rows
// (launch-local scratch of every step launch as well).
template <int NVT, int KC, int NC, int NTR, int WPE, bool HF, bool TRK>
__global__ void __launch_bounds__(64, WPE) forward_kernel_w(const DevModel* __restrict__ Mp, const DevModelW* __restrict__ Wp, DevBatch Bt, FwdDev F) {
  extern __shared__ __align__(16) float E[];
  const DevModel& M = *Mp;
  const DevModelW& W = *Wp;
  const LayW& Y = W.lay;
  typedef WaveCfg<NVT, KC, NC, NTR, WPE, false, 0, HF, TRK, false, TRK> C;   // (OBJ = TRK: the forward twin shows the per-env object parameters)
  constexpr bool FULL = C::FULL;
  constexpr int NCXK = C::NCXK;
  const int env = blockIdx.x;
  const int nv = M.nv, nu = M.nu, nq = W.nq;
  int lane = wave_lane();
#if MYO_POISON   // diagnostic build: every LDS word starts as a NaN, as in the step kernel
  for (int i = lane; i < Y.total; i += 64) E[i] = __int_as_float(MYO_POISON_BITS);
  SYNC();
#endif
  if (lane < nq) E[Y.qpos + lane] = Bt.qpos[(size_t)env * nq + lane];
  if (lane < nv) E[Y.qvel + lane] = Bt.qvel[(size_t)env * nv + lane];
  float* const ovf_env = Bt.ovf ? Bt.ovf + (size_t)env * Bt.ovf_rows * Bt.ovf_row : nullptr;
  const int ovf_row = Bt.ovf_row;
  const int nct = ovf_env ? NC + NCXK : NC;
  int* const ovf_cand = (!HF && Bt.ovf_cand) ? Bt.ovf_cand + (size_t)env * NCANDX : nullptr;
  // nsub = 0, step = 0: w_kinematics exports MYO_F_LINKX at step == nsub - 1 only
  const WaveCtx<LayW> X{M, W, Y, Bt, nullptr, env, nv, nu, nq, M.nl, M.nlevel, M.maxnnz, M.ngt, M.nseg, M.ncg, M.npair, FULL && W.has_free, FULL ? W.neq : 0,
                        false, M.timestep, 0, 0, ovf_env, ovf_row, nct, ovf_cand};
  SYNC();
  int flags = 0;
  bool alive = true;
  w_check_state<C>(X, lane, false, flags, alive);
  float* const xpos = F.xpos + (size_t)env * 3 * F.nbody;
  float* const xmat = F.xmat + (size_t)env * 9 * F.nbody;
  float* const xipos = F.xipos + (size_t)env * 3 * F.nbody;
  float* const sxpos = F.site_xpos + (size_t)env * 3 * F.nsite;
  float* const sxmat = F.has_site_mat ? F.site_xmat + (size_t)env * 9 * F.nsite : nullptr;
  float* const gxpos = F.geom_xpos + (size_t)env * 3 * F.ngeom;
  float* const gxmat = F.geom_xmat + (size_t)env * 9 * F.ngeom;
  float* const crow = F.contact + (size_t)env * FWD_CON * F.ncap;
  if (__builtin_expect(!alive, 0)) {   // a bad env (wave-uniform): zero rows, no contacts; the state stays as it is
    WFOR(i, 3 * F.nbody) { xpos[i] = 0.f; xipos[i] = 0.f; }
    WFOR(i, 9 * F.nbody) xmat[i] = 0.f;
    WFOR(i, 3 * F.nsite) sxpos[i] = 0.f;
    if (sxmat) WFOR(i, 9 * F.nsite) sxmat[i] = 0.f;
    WFOR(i, 3 * F.ngeom) gxpos[i] = 0.f;
    WFOR(i, 9 * F.ngeom) gxmat[i] = 0.f;
    WFOR(i, FWD_CON * F.ncap) crow[i] = 0.f;
    if (lane == 0) { F.ncon[env] = 0; Bt.flags[env] |= flags; }
    return;
  }
  w_kinematics<C>(X, lane, 0);
  {  // frames: lane = item
    const float org[3] = {M.origin[0], M.origin[1], M.origin[2]};
    const BodyRot BR = body_rot_of(Bt, env, TRK, TRK);
    // (The goal offset moves the exported frames only: the collision stages turn the body's geoms with BodyRot and do not translate them.  The
    // die task's target carries no collision geom -- launch_forward passes goal_off only then -- so geom_xpos and contact.pos cannot disagree.)
    const float* const off = TRK && F.goal_off ? F.goal_off + 3 * (size_t)env : nullptr;
    WFOR(i, F.nbody) {
      const FwdItem I = fwd_item(F.body_rec, i);
      const bool moved = TRK && I.link < 0 && i == F.bq_body;
      float x[3], R[9], xi[3];
      fwd_world(Y, E, I, BR, moved, off, x, R);
      frame_point(Y, E, I.link, I.a, xi);
      if (moved) fwd_move_point(BR, off, xi);
      fwd_store(xpos, xmat, i, org, x, R);
      fwd_store(xipos, nullptr, i, org, xi, R);
    }
    WFOR(i, F.nsite) {
      const FwdItem I = fwd_item(F.site_rec, i);
      const bool moved = TRK && I.link < 0 && __float_as_int(I.a[0]) == F.bq_body;
      float x[3], R[9];
      fwd_world(Y, E, I, BR, moved, off, x, R);
      fwd_store(sxpos, sxmat, i, org, x, R);
    }
    WFOR(i, F.ngeom) {
      FwdItem I = fwd_item(F.geom_rec, i);
      if (BR.og) {   // per-env centre of a selected geom (DevBatch.objk): the row the collision stages place it with
        const int s = Bt.obj_slot[Bt.obj_ncg + i];
        if (s >= 0) { I.p[0] = BR.og[12 * s + 4]; I.p[1] = BR.og[12 * s + 5]; I.p[2] = BR.og[12 * s + 6]; }
      }
      const bool moved = TRK && I.link < 0 && __float_as_int(I.a[0]) == F.bq_body;
      float x[3], R[9];
      fwd_world(Y, E, I, BR, moved, off, x, R);
      fwd_store(gxpos, gxmat, i, org, x, R);
    }
  }
  int ncon = 0;
  if (!M.disable_contact) {
    int f_cand = 0, f_mpr = 0, n_mprw = 0;   // no warm-start entry: the first substep of a step launch
    const int ncand = w_broad_phase<C>(X, lane, flags, f_cand);
    ncon = w_narrow_phase<C>(X, lane, ncand, n_mprw, flags, f_mpr);
  }
  // contacts: lane = contact (TRK: two rounds), through con_row: LDS rows below NC, the env's overflow rows above
  for (int c = lane; c < ncon; c += 64) {
    float dist = 0.f, cp[3] = {0.f, 0.f, 0.f}, n[3] = {1.f, 0.f, 0.f};
    int cw = 0;
    con_row<C>(Y, E, ovf_env, ovf_row, c, [&](const ConRow& R) {
      dist = R.dist[0]; cw = R.pair[0];
#pragma unroll
      for (int k = 0; k < 3; k++) { cp[k] = R.pos[k]; n[k] = R.nrm[k]; }
    });
    const int p = cw & 2047;
    const int pw = __float_as_int(W.pair_rec[4 * (size_t)p].x), g1 = pw & 255, g2 = (pw >> 8) & 255;
    float t1[3], t2[3];
    make_frame(n, t1, t2);   // the tangents the row stage builds for this contact
    if (KC == 20 && ((pw >> 16) & 15) == 2) {   // plane - capsule: first tangent along the capsule axis
      const float* ax = E + Y.gax + 3 * g2;
      float t = dot3(ax, n), y[3] = {ax[0] - t * n[0], ax[1] - t * n[1], ax[2] - t * n[2]};
      float yn = norm3(y);
      if (yn >= 0.5f) {
        float inv = 1.0f / yn;
        t1[0] = y[0] * inv; t1[1] = y[1] * inv; t1[2] = y[2] * inv;
        cross3(t2, n, t1);
      }
    }
    float* o = crow + (size_t)c * FWD_CON;
    o[0] = dist;
#pragma unroll
    for (int k = 0; k < 3; k++) { o[1 + k] = cp[k] + M.origin[k]; o[4 + k] = n[k]; o[7 + k] = t1[k]; o[10 + k] = t2[k]; }
    ((int*)o)[13] = F.cg_geom[g1]; ((int*)o)[14] = F.cg_geom[g2]; ((int*)o)[15] = p;
  }
  if (lane == 0) { F.ncon[env] = ncon; if (flags) Bt.flags[env] |= flags; }
}

// ---- host half
// The export tables in float64 from the blob alone (no device): per body, site and geom the link, and the pose inside the link's frame =
// pose of its body inside the link (hip_body_lpos / hip_body_lquat; a world-welded body: its constant world pose relative to hip_origin)
// composed with the item's pose inside its body.  site_rec's rotation is the body's where the blob has no site_quat (has_site_mat = false:
// site_xmat is then not exported).
struct FwdTables { std::vector<double> body, site, geom; bool has_site_mat = false; };
static int fwd_build_tables(const Blob& B, FwdTables* T) {
  for (const char* n : {"hip_body_link", "hip_body_lpos", "hip_body_lquat", "body_ipos", "site_bodyid", "site_pos", "geom_bodyid", "geom_pos", "geom_quat"})
    if (!B.has(n)) return fail(MYO_E_UNSUPPORTED, std::string("forward: the model blob lacks ") + n);
  const std::vector<int> bl = B.ints("hip_body_link"), sb = B.ints("site_bodyid"), gb = B.ints("geom_bodyid");
  const std::vector<double> lpos = B.doubles("hip_body_lpos"), lquat = B.doubles("hip_body_lquat"), ipos = B.doubles("body_ipos"), spos = B.doubles("site_pos"),
                            gpos = B.doubles("geom_pos"), gquat = B.doubles("geom_quat");
  std::vector<double> squat;
  if (B.has("site_quat")) squat = B.doubles("site_quat");
  if (B.rc) return B.rc;
  const size_t nb = bl.size(), ns = sb.size(), ng = gb.size();
  if (lpos.size() != 3 * nb || lquat.size() != 4 * nb || ipos.size() != 3 * nb || spos.size() != 3 * ns || gpos.size() != 3 * ng || gquat.size() != 4 * ng ||
      (!squat.empty() && squat.size() != 4 * ns)) return fail(MYO_E_BLOB, "forward: body / site / geom tables of unexpected shape");
  T->has_site_mat = !squat.empty() || ns == 0;
  auto item = [&](int body, const double* p, const double* q, double* R) {   // the record of an item at (p, q) inside `body`
    double Rb[9], Rq[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    quat2mat_d(Rb, &lquat[4 * (size_t)body]);
    if (q) quat2mat_d(Rq, q);
    R[0] = (double)bl[body];
    for (int i = 0; i < 3; i++) {
      R[1 + i] = lpos[3 * (size_t)body + i] + Rb[3 * i] * p[0] + Rb[3 * i + 1] * p[1] + Rb[3 * i + 2] * p[2];
      for (int j = 0; j < 3; j++) R[4 + 3 * i + j] = Rb[3 * i] * Rq[j] + Rb[3 * i + 1] * Rq[3 + j] + Rb[3 * i + 2] * Rq[6 + j];
    }
    R[13] = (double)body; R[14] = R[15] = 0.0;
  };
  const double zero[3] = {0, 0, 0};
  T->body.assign(FWD_REC * nb, 0.0); T->site.assign(FWD_REC * ns, 0.0); T->geom.assign(FWD_REC * ng, 0.0);
  for (size_t b = 0; b < nb; b++) {
    double com[FWD_REC];
    item((int)b, zero, nullptr, &T->body[FWD_REC * b]);
    item((int)b, &ipos[3 * b], nullptr, com);
    for (int k = 0; k < 3; k++) T->body[FWD_REC * b + 13 + k] = com[1 + k];
  }
  for (size_t s = 0; s < ns; s++) {
    if (sb[s] < 0 || (size_t)sb[s] >= nb) return fail(MYO_E_BLOB, "forward: site_bodyid out of range");
    item(sb[s], &spos[3 * s], squat.empty() ? nullptr : &squat[4 * s], &T->site[FWD_REC * s]);
  }
  for (size_t g = 0; g < ng; g++) {
    if (gb[g] < 0 || (size_t)gb[g] >= nb) return fail(MYO_E_BLOB, "forward: geom_bodyid out of range");
    item(gb[g], &gpos[3 * g], &gquat[4 * g], &T->geom[FWD_REC * g]);
  }
  return MYO_OK;
}

// float records for the device: the link and the body id travel as bits
static std::vector<float> fwd_pack(const std::vector<double>& rec, bool body_table) {
  std::vector<float> o(std::max<size_t>(rec.size(), FWD_REC), 0.f);
  for (size_t i = 0; i < rec.size(); i++) {
    const size_t k = i % FWD_REC;
    o[i] = (k == 0 || (k == 13 && !body_table)) ? bits_f((int)rec[i]) : (float)rec[i];
  }
  return o;
}

// at model load: tables to the device.  A blob without the body tables leaves the model without a forward pass (myo_forward refuses it)
static int fwd_model_tables(myo_model* m, const Blob& B) {
  if (!m->wave_ok) return MYO_OK;
  FwdTables T;
  if (fwd_build_tables(Blob{B.p}, &T)) { g_err.clear(); return MYO_OK; }
  int rc;
  if ((rc = upload(m, fwd_pack(T.body, true), &m->d_fwd_body)) || (rc = upload(m, fwd_pack(T.site, false), &m->d_fwd_site)) ||
      (rc = upload(m, fwd_pack(T.geom, false), &m->d_fwd_geom)) || (rc = upload(m, m->cg_geom, &m->d_fwd_cg_geom))) return rc;
  m->fwd_nbody = (int)(T.body.size() / FWD_REC); m->fwd_nsite = (int)(T.site.size() / FWD_REC); m->fwd_ngeom = (int)(T.geom.size() / FWD_REC);
  m->fwd_site_mat = T.has_site_mat;
  // contact records per env: what the narrow phase of the model's kernel class keeps (LDS rows + overflow rows; TRK: both banks)
  m->fwd_ncap = m->trk ? 128 : 64;
  m->fwd_ok = true;
  return MYO_OK;
}

// elements per env of forward buffer `which` (MYO_FWD_*), 0: no such buffer
static size_t fwd_width(const myo_model* m, int which) {
  switch (which) {
    case MYO_FWD_XPOS: case MYO_FWD_XIPOS: return 3 * (size_t)m->fwd_nbody;
    case MYO_FWD_XMAT: return 9 * (size_t)m->fwd_nbody;
    case MYO_FWD_SITE_XPOS: return 3 * (size_t)m->fwd_nsite;
    case MYO_FWD_SITE_XMAT: return 9 * (size_t)m->fwd_nsite;
    case MYO_FWD_GEOM_XPOS: return 3 * (size_t)m->fwd_ngeom;
    case MYO_FWD_GEOM_XMAT: return 9 * (size_t)m->fwd_ngeom;
    case MYO_FWD_NCON: return 1;
    case MYO_FWD_CONTACT: return (size_t)FWD_CON * m->fwd_ncap;
    default: return 0;
  }
}

// The refusals, shared by myo_forward and myo_model_forward_dims.  Forward is the twin of the wave-per-env step kernel: where myo_step would run
// the generic lanes kernel instead (launch_step: a model the wave kernel cannot take, or lanes != 64 set with myo_set_lanes / MYO_LANES for a
// model the lanes kernel can take), the contacts of a wave-kernel forward would not be those of the next step, so it is refused.
static int fwd_model_check(const myo_model* m) {
  if (!m->wave_ok) return fail(MYO_E_UNSUPPORTED, "forward: models of the wave-per-env kernel only (this model runs on the generic lanes kernel)");
  if (g_lanes != 64 && m->generic_ok) return fail(MYO_E_UNSUPPORTED, "forward: wave-per-env kernel only (lanes = 64); with the current lanes setting this model steps on the generic lanes kernel");
  if (!m->fwd_ok) return fail(MYO_E_UNSUPPORTED, "forward: the model blob lacks the body / site / geom tables");
  return MYO_OK;
}
static int fwd_check(const myo_batch* b) { return fwd_model_check(b->model); }

// the first myo_forward allocates the batch's buffers (zero-filled; a buffer of no elements still gets an allocation)
static int fwd_start(myo_batch* b) {
  if (b->fwd_on) return MYO_OK;
  HIPCHK(hipSetDevice(b->model->device));
  for (int w = 0; w < MYO_FWD_COUNT; w++) {
    int rc = b->pool.alloc(&b->fwd_buf[w], std::max<size_t>((size_t)b->db.B * fwd_width(b->model, w), 1) * 4);
    if (rc) return rc;
  }
  b->fwd_on = true;
  return MYO_OK;
}

#endif  // MYO_KERNEL_FORWARD_H
