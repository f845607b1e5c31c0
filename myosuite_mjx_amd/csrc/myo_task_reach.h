// myo_task_reach.h -- ReachEnvV0 (envs/myo/myobase/reach_v0.py) observation / reward / done / solved, MYO_TASK_REACH.  Reach needs tip
// positions: its observation reuses the lanes kernel's kinematics stage (per-env groups of G lanes, the env's state in LDS) instead of the
// shared walk of myo_task_util.h, and it has no fused epilogue.
#ifndef MYO_TASK_REACH_H
#define MYO_TASK_REACH_H

// reach_v0.py:96-141 and walk_v0.py's ReachEnvV0 (myo_task_stand.h, ntip = 1).  Row: qpos, qvel * dt, tip positions, reach_err = target - tip, act
struct ReachRow {
  int nq, nv, ntip, na;
  Blk qpos = {0, nq}, qvel = qpos.then(nv), tip_pos = qvel.then(3 * ntip), reach_err = tip_pos.then(3 * ntip), act = reach_err.then(na);
  int dim = act.end();
};

template <int G>
__global__ void __launch_bounds__(64) reach_obs_kernel(DevModel M, DevBatch Bt, TaskDev T, int obs_only) {
  extern __shared__ __align__(16) float smem[];
  const Lay& Y = M.lay;
  const int lane = threadIdx.x, grp = lane / G, sub = lane % G;
  int env = blockIdx.x * (64 / G) + grp;
  const bool valid = env < Bt.B;
  if (!valid) env = Bt.B - 1;
  float* E = smem + grp * Y.total;
  const int nv = M.nv, nu = M.nu;
  const ReachRow R{nv, nv, T.ntip, M.na_obs};   // nq == nv: the lanes kernel's models have hinge / slide joints only
  GFOR(i, nv) E[Y.qpos + i] = Bt.qpos[(size_t)env * nv + i];
  SYNC();
  stage_kinematics<G>(M, E, sub);
  float dt = (float)T.frame_skip * M.timestep;
  float* o = Bt.obs + (size_t)env * T.obs_dim;
  float err2 = 0;
  GFOR(i, T.ntip) {
    float p[3];
    site_world(M, E, T.tip_site[i], p);
    for (int k = 0; k < 3; k++) {
      p[k] += M.origin[k];  // kernels work relative to the lowered origin; observations are world coordinates
      float tg = Bt.target[(size_t)env * T.ntarget + 3 * i + k];
      float re = tg - p[k];
      err2 += re * re;
      if (valid) {
        o[R.tip_pos.at + 3 * i + k] = p[k];
        o[R.reach_err.at + 3 * i + k] = re;
        Bt.sitexpos[(size_t)env * 3 * T.ntip + 3 * i + k] = p[k];
      }
    }
  }
  err2 = grp_sum<G>(err2);
  float actn = 0;
  GFOR(i, nu) { float a = Bt.act[(size_t)env * nu + i]; const int sl = M.act_obs[i]; if (sl >= 0) { actn += a * a; if (valid) o[R.act.at + sl] = a; } }
  actn = sqrtf(grp_sum<G>(actn)) / (float)(M.na_obs > 0 ? M.na_obs : 1);
  if (valid) {
    GFOR(i, nv) { o[R.qpos.at + i] = E[Y.qpos + i]; o[R.qvel.at + i] = Bt.qvel[(size_t)env * nv + i] * dt; }
    if (sub == 0 && !obs_only) {
      float dist = sqrtf(err2);
      float near_th = T.near_th, far_th = Bt.time[env] > 2 * dt ? T.far_th : 1e30f;
      float bonus = (dist < 2 * near_th ? 1.f : 0.f) + (dist < near_th ? 1.f : 0.f);
      float pen = dist > far_th ? -1.f : 0.f;
      const float solved = dist < near_th ? 1.f : 0.f, done = dist > far_th ? 1.f : 0.f;
      if (Bt.rwd) rwd_row(Bt, env, {-dist, bonus, -actn, pen, -dist, solved, done});      // reach_v0.py:126-141
      else Bt.reward[env] = T.w_reach * (-dist) + T.w_bonus * bonus + T.w_act_reg * (-actn) + T.w_penalty * pen;
      Bt.solved[env] = solved;
      Bt.done[env] = done;
    }
  }
}

static int reach_configure(myo_batch* b, const myo_task_config* c) {
  if (c->ntarget != 3 * c->ntip) return fail(MYO_E_ARG, "reach task: ntarget must be 3*ntip");
  const int nv = b->model->dm.nv;
  b->task.obs_dim = ReachRow{nv, nv, c->ntip, b->model->dm.na_obs}.dim;
  return MYO_OK;
}
// the two tables, shared with the stand task
static const char* const rwd_reach[] = {"reach", "bonus", "act_reg", "penalty", RWD_TAIL};   // reach_v0.py:126-141, walk_v0.py:117-133
static void obs_terms_reach(const ObsDims& D, ObsTable& t) {     // reach_v0.py and walk_v0.py ReachEnvV0 get_obs_dict
  const ReachRow R{D.nq, D.nv, D.ntip, D.na};
  TERM("time", 1, OBS_SRC_TIME, 0)
  ROW(R, qpos)
  ROW(R, qvel)
  ROW(R, act)
  ROW(R, tip_pos)
  TERM("target_pos", R.tip_pos.n, OBS_SRC_TARGET, 0)
  ROW(R, reach_err)
  t.dim = R.dim;
}
static int reach_obs(myo_batch* b, hipStream_t s, int obs_only, int) {
  const int EPW = 4;
  hipLaunchKernelGGL(reach_obs_kernel<16>, dim3((b->db.B + EPW - 1) / EPW), dim3(64), (size_t)EPW * b->model->env_lds_bytes, s, b->model->dm, b->db, b->task, obs_only);
  return MYO_OK;
}
static const TaskHooks reach_hooks = {reach_configure, reach_obs, nullptr, RWD_COLS(rwd_reach), obs_terms_reach};

#endif  // MYO_TASK_REACH_H
