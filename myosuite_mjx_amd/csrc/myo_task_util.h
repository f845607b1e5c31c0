// myo_task_util.h -- what the task files (myo_task_<name>.h) share: on the device the walk up a link chain, the row prologue, the site
// gather and the activation term; on the host the checks every *_configure repeats.  Included after myo_host.h and before the task files.
// The per-env orientation of a static point, body_rot_point, sits with BodyRot in myo_wave_util.h, where the step kernel uses it too.
#ifndef MYO_TASK_UTIL_H
#define MYO_TASK_UTIL_H

// world frame (relative to the lowered origin) of a frame fixed in link `link` (-1: the world) at the joint positions q of env e: point
// lp -> p and, with ROT, rotation Rl -> R.  The link chain is walked up to its root; each link's own joint chain, in its parent's frame, is
// applied on the way (the transform the wave kernel's kinematics phase 1 builds per link).  The per-env offset of MYO_F_BODYPOS moves its
// root link's origin, as in the TRK step kernel.  Hinge / slide joints only (nq == nv, checked at configure).
template <bool ROT>
__device__ __forceinline__ void link_chain(const DevModel& M, const DevBatch& Bt, const float* q, int e, int link, const float* lp, const float* Rl,
                                           float* p, float* R) {
  p[0] = lp[0]; p[1] = lp[1]; p[2] = lp[2];
  if constexpr (ROT) {
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = Rl[k];
  }
  for (int l = link; l >= 0; l = M.link_parent[l]) {
    float A[9], c[3] = {M.link_pos[3 * l], M.link_pos[3 * l + 1], M.link_pos[3 * l + 2]};
    const float lq[4] = {M.link_quat[4 * l], M.link_quat[4 * l + 1], M.link_quat[4 * l + 2], M.link_quat[4 * l + 3]};
    quat2mat(A, lq);
    if (Bt.bpos && l == Bt.bpos_link) {
      const float* o = Bt.bpos + 3 * (size_t)e;
      c[0] += o[0]; c[1] += o[1]; c[2] += o[2];
    }
    const int da = M.link_dofadr[l], dn = M.link_dofnum[l];
    for (int k = 0; k < dn; k++) {
      const int d = da + k;
      const float al[3] = {M.dof_axis[3 * d], M.dof_axis[3 * d + 1], M.dof_axis[3 * d + 2]};
      const float dp[3] = {M.dof_pos[3 * d], M.dof_pos[3 * d + 1], M.dof_pos[3 * d + 2]};
      const float ang = q[d] - M.qpos0[d];
      float ax[3], an[3];
      matvec(ax, A, al);
      matvec(an, A, dp);
      an[0] += c[0]; an[1] += c[1]; an[2] += c[2];
      if (M.dof_type[d] == 3) {   // hinge: rotate about the axis through the anchor
        float sn, cs;
        sincosf(ang, &sn, &cs);
        const float oc = 1 - cs, x = al[0], y = al[1], z = al[2];
        const float Rj[9] = {cs + oc * x * x, oc * x * y - sn * z, oc * x * z + sn * y, oc * x * y + sn * z, cs + oc * y * y, oc * y * z - sn * x,
                             oc * x * z - sn * y, oc * y * z + sn * x, cs + oc * z * z};
        float v[3];
        matmul3(A, A, Rj);
        matvec(v, A, dp);
        c[0] = an[0] - v[0]; c[1] = an[1] - v[1]; c[2] = an[2] - v[2];
      } else {                    // slide
        c[0] += ax[0] * ang; c[1] += ax[1] * ang; c[2] += ax[2] * ang;
      }
    }
    float w[3];
    matvec(w, A, p);
    p[0] = w[0] + c[0]; p[1] = w[1] + c[1]; p[2] = w[2] + c[2];
    if constexpr (ROT) matmul3(R, A, R);
  }
}
// ... of the point lp of a link, and of site s
__device__ __forceinline__ void link_point_pos(const DevModel& M, const DevBatch& Bt, const float* q, int e, int link, const float* lp, float* p) {
  link_chain<false>(M, Bt, q, e, link, lp, nullptr, p, nullptr);
}
__device__ __forceinline__ void site_pos(const DevModel& M, const DevBatch& Bt, const float* q, int e, int s, float* p) {
  link_point_pos(M, Bt, q, e, M.site_link[s], M.site_lpos + 3 * s, p);
}

// the rows of env e a body reads and the one it writes: `const auto [o, q, v, a, dt] = task_row(...)`.  nq = the width of a qpos row
struct TaskRow { float* o; const float *q, *v, *a; float dt; };   // dt: one env step
__device__ __forceinline__ TaskRow task_row(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int e, int nq) {
  return {Bt.obs + (size_t)e * T.obs_dim, Bt.qpos + (size_t)e * nq, Bt.qvel + (size_t)e * M.nv, Bt.act + (size_t)e * M.nu, (float)T.frame_skip * M.timestep};
}

// lanes 0 .. N-1 each hold a point p relative to the lowered origin: shifts it to world coordinates, writes the first nwrite of them to
// the env's MYO_F_SITEXPOS row ([nwrite][3]) and hands all N to every lane, x[i] = lane i's point.  Every lane calls it
template <int N>
__device__ __forceinline__ void site_gather(const DevModel& M, const DevBatch& Bt, int e, int lane, int nwrite, float* p, float (*x)[3]) {
  if (lane < N) {
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] += M.origin[k];
    if (lane < nwrite) {
#pragma unroll
      for (int k = 0; k < 3; k++) Bt.sitexpos[((size_t)e * nwrite + lane) * 3 + k] = p[k];
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) x[i][k] = __shfl(p[k], i);
}

// the activation term ||act|| / na over the observed actuators, in two halves around a body's obs_only return.  act_sq: this lane's share
// of the squares; given o_act it also writes act into the row there.  act_norm: the wave's norm
template <bool WRITE>
__device__ __forceinline__ float act_sq_lane(const DevModel& M, const float* a, int lane, float* o_act) {
  float act2 = 0.f;
  for (int i = lane; i < M.nu; i += 64) { const float ai = a[i]; const int sl = M.act_obs[i]; if (sl >= 0) { if constexpr (WRITE) o_act[sl] = ai; act2 += ai * ai; } }
  return act2;
}
__device__ __forceinline__ float act_sq(const DevModel& M, const float* a, int lane) { return act_sq_lane<false>(M, a, lane, nullptr); }
__device__ __forceinline__ float act_sq(const DevModel& M, const float* a, int lane, float* o_act) { return act_sq_lane<true>(M, a, lane, o_act); }
__device__ __forceinline__ float act_norm(const DevModel& M, float act2) { return sqrtf(wave_sum(act2)) / (float)(M.na_obs > 0 ? M.na_obs : 1); }

// host: how a task file states its two tables (RwdCols, ObsTable: myo_host.h).  Every reward row ends sparse, solved, done, dense.  A term of
// the canonical row is ROW(R, block): the block's name is the key, its width and offset come from the row record R; a term from outside the
// row is TERM(key, width, source, index).  Both fill `t`; a table function ends with t.dim = R.dim
#define RWD_TAIL "sparse", "solved", "done", "dense"
#define RWD_COLS(a) RwdCols{a, (int)(sizeof a / sizeof a[0])}
#define TERM(name, width, src, idx) t.push_back(ObsTerm{name, width, src, idx});
#define ROW(R, block) TERM(#block, R.block.n, OBS_SRC_ROW, R.block.at)

// host: the checks of the *_configure functions (each caller refuses with its own text).  trk_model: a TrackEnv-class model whose qpos row is nq_extra wider than its qvel row (0: hinge / slide joints only, what link_chain walks)
static bool trk_model(const myo_model* m, int nq_extra = 0) { return m->wave_ok && m->trk && m->nq == m->dm.nv + nq_extra; }
static bool sites_in_range(const myo_model* m, const myo_task_config* c, int n) {
  for (int k = 0; k < n; k++) if (c->tip_site[k] < 0 || c->tip_site[k] >= m->dims.nsite) return false;
  return true;
}
static bool is_number(float x) { return x == x; }
// the model's last six joints are 3 slides + 3 hinges of one root body (the pen, the die): that body's link, or -1
static int object_link_6dof(const myo_model* m) {
  const int nv = m->dm.nv, l = root_link_of_dofs(m, nv - 6, 6);
  for (int k = 0; k < 6; k++) if (m->dof_type[nv - 6 + k] != (k < 3 ? 2 : 3)) return -1;
  return l;
}

#endif  // MYO_TASK_UTIL_H
