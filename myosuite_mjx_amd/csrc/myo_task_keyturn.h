// myo_task_keyturn.h -- KeyTurnEnvV0 (envs/myo/myobase/key_turn_v0.py) observation / reward / done / solved, MYO_TASK_KEYTURN.
//
// The model is of the TrackEnv class (the key's box bit and the friction loss of its hinge), whose step kernel keeps no kinematics a
// separate pass could reuse, and the lanes kernel's reach_obs_kernel is not available to it.  So this kernel runs its own forward
// kinematics, and only of what the task reads: the ancestor chains of its three sites (key head, index tip, thumb tip), one lane per site,
// from the post-step qpos -- the site positions of the reference's post-step forward pass.  One 64-lane workgroup per env.
#ifndef MYO_TASK_KEYTURN_H
#define MYO_TASK_KEYTURN_H

// world position (relative to the lowered origin) of the point lp of link `link` (-1: the world) at the joint positions q of env e.  The
// link chain is walked up to its root; each link's own joint chain, in its parent's frame, is applied to the point on the way (the
// transform the wave kernel's kinematics phase 1 builds per link).  The per-env offset of MYO_F_BODYPOS moves its root link's origin, as in
// the TRK step kernel.  Hinge / slide joints only (nq == nv, checked at configure).
__device__ __forceinline__ void link_point_pos(const DevModel& M, const DevBatch& Bt, const float* q, int e, int link, const float* lp, float* p) {
  p[0] = lp[0]; p[1] = lp[1]; p[2] = lp[2];
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
  }
}
// ... of site s
__device__ __forceinline__ void keyturn_site_pos(const DevModel& M, const DevBatch& Bt, const float* q, int e, int s, float* p) {
  link_point_pos(M, Bt, q, e, M.site_link[s], M.site_lpos + 3 * s, p);
}

// key_turn_v0.py:82-156 (+ act, base_v0.py:34-38).  Row: hand qpos (nq - 1), hand qvel * dt (nv - 1), key qpos, key qvel * dt, head - index
// tip (3), head - thumb tip (3), act (na).  get_reward_dict reads the approach vectors and act from self.obs_dict but key_q from its argument;
// at step time both are the obs_dict of the stepped state, so one set of values serves both here.
__device__ __forceinline__ void keyturn_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int obs_only, const int e, const int lane) {
  const int nv = M.nv, nu = M.nu, nh = nv - 1;
  const float dt = (float)T.frame_skip * M.timestep;
  float* o = Bt.obs + (size_t)e * T.obs_dim;
  const float* q = Bt.qpos + (size_t)e * nv;
  const float* v = Bt.qvel + (size_t)e * nv;
  const float* a = Bt.act + (size_t)e * nu;
  float p[3] = {0.f, 0.f, 0.f};
  if (lane < 3) {   // lane 0: key head, 1: index tip, 2: thumb tip
    keyturn_site_pos(M, Bt, q, e, T.tip_site[lane], p);
#pragma unroll
    for (int k = 0; k < 3; k++) { p[k] += M.origin[k]; Bt.sitexpos[(size_t)e * 9 + 3 * lane + k] = p[k]; }
  }
  float h[3], dk = 0.f;
#pragma unroll
  for (int k = 0; k < 3; k++) h[k] = __shfl(p[k], 0);
  if (lane == 1 || lane == 2) {
    const float r[3] = {h[0] - p[0], h[1] - p[1], h[2] - p[2]};
#pragma unroll
    for (int k = 0; k < 3; k++) o[2 * nv + 3 * (lane - 1) + k] = r[k];
    dk = fabsf(norm3(r) - T.near_th);
  }
  for (int i = lane; i < nv; i += 64) {
    if (i < nh) { o[i] = q[i]; o[nh + i] = v[i] * dt; }
    else { o[2 * nh] = q[i]; o[2 * nh + 1] = v[i] * dt; }
  }
  float act2 = 0.f;
  for (int i = lane; i < nu; i += 64) { const float ai = a[i]; const int sl = M.act_obs[i]; if (sl >= 0) { o[2 * nv + 6 + sl] = ai; act2 += ai * ai; } }
  const float d_if = __shfl(dk, 1), d_th = __shfl(dk, 2);
  if (obs_only) return;
  const float actn = sqrtf(wave_sum(act2)) / (float)(M.na_obs > 0 ? M.na_obs : 1);
  if (lane == 0) {
    const float key_q = q[nh];
    const float bonus = (key_q > 1.57079632679489662f ? 1.f : 0.f) + (key_q > 3.14159265358979324f ? 1.f : 0.f);
    const float pen = -(d_if > 0.5f * T.far_th ? 1.f : 0.f) - (d_th > 0.5f * T.far_th ? 1.f : 0.f);
    const float solved = key_q > T.pose_thd ? 1.f : 0.f, done = (d_if > T.far_th || d_th > T.far_th) ? 1.f : 0.f;
    if (Bt.rwd) rwd_row(Bt, e, {key_q, -d_if, -d_th, -actn, bonus, pen, key_q, solved, done});   // key_turn_v0.py:134-152
    else Bt.reward[e] = T.w_pose * key_q + T.w_reach * (-d_if) + T.w_reach * (-d_th) + T.w_act_reg * (-actn) + T.w_bonus * bonus + T.w_penalty * pen;
    Bt.solved[e] = solved;
    Bt.done[e] = done;
  }
}

using KeyturnTask = StateObs<keyturn_obs_body>;
// key_turn_v0.py: the key is the model's last joint, one hinge of a root body; sites = key head, index tip, thumb tip
static int keyturn_configure(myo_batch* b, const myo_task_config* c) {
  const myo_model* m = b->model;
  const int nv = m->dm.nv;
  if (!(m->wave_ok && m->trk) || m->bp_link < 0 || m->nq != nv) return fail(MYO_E_UNSUPPORTED, "key-turn task: a TrackEnv-class model without free / ball joints whose last joint is the hinge of a root body");
  if (m->dof_type[nv - 1] != 3 || m->link_dofnum[m->bp_link] != 1 || m->dof_link[nv - 1] != m->bp_link) return fail(MYO_E_UNSUPPORTED, "key-turn task: the last joint must be the one hinge of its root body");
  if (c->ntip != 3 || c->ntarget != 0) return fail(MYO_E_ARG, "key-turn task: ntip = 3 (key head, index tip, thumb tip) and ntarget = 0");
  for (int k = 0; k < 3; k++) if (c->tip_site[k] < 0 || c->tip_site[k] >= m->dims.nsite) return fail(MYO_E_ARG, "key-turn task: site id out of range");
  if (!(c->near_th >= 0.f) || !(c->far_th > 0.f) || !(c->pose_thd == c->pose_thd)) return fail(MYO_E_ARG, "key-turn task: near_th >= 0, far_th > 0, goal_th (pose_thd) a number");
  b->task.obs_dim = 2 * nv + 6 + m->dm.na_obs;
  return MYO_OK;
}
static const TaskHooks keyturn_hooks = {keyturn_configure, launch_task_obs<KeyturnTask>, launch_task_post<KeyturnTask>};

#endif  // MYO_TASK_KEYTURN_H
