// myo_obs_terms.h -- observation terms (include/myo_hip_obs.h): the lookup of a task's term table, the column program the host builds from
// it, the one kernel that runs the program and the host entry points.  Included by myo_hip.hip after myo_host_tasks.h, before
// myo_host_step.h (the walk task's step launch runs the kernel).
#ifndef MYO_OBS_TERMS_H
#define MYO_OBS_TERMS_H

// ---- the table (ObsTable, myo_host.h) of a task for the dimensions D, built by the task's own function (myo_task_<name>.h) from its row
// record.  Empty: no task, or the MyoDM track task, whose terms live in its own kernels
static ObsTable obs_table(int task, const ObsDims& D) {
  ObsTable t;
  const TaskHooks* hooks = task_hooks(task);
  if (hooks && hooks->obs_terms) hooks->obs_terms(D, t);
  for (ObsTerm& x : t) if (x.width < 0) x.width = 0;   // (a model too small for the task: its configure has refused it)
  return t;
}
// ... of the batch's configured task
static ObsTable obs_table(const myo_batch* b) {
  const myo_model* m = b->model;
  const int na = m->dm.na_obs;
  return obs_table(b->task.task, ObsDims{m->nq, m->dm.nv, m->dm.nu, na, b->task.task == MYO_TASK_STAND ? 1 : b->task.ntip, na > 0 ? na : m->nq});
}

// ---- the kernel.  One thread per output float of the three rows of one env laid end to end ([terms | selected | proprio], W floats): thread
// gid serves env gid / W, column gid % W, so a wave reads 64 consecutive program records and writes 64 consecutive floats of a row (rows of
// one buffer follow each other without padding), and its reads of a source row are consecutive wherever a term is a slice.  No LDS: nothing
// is read twice by a workgroup but the program, which the L1 / L2 serve (W records, a few kB, shared by all workgroups).  256 threads per
// block; the last block's tail is guarded.
struct ObsSources { const float *row, *time, *target, *qpos, *act, *cst; int row_w, target_w, qpos_w, act_w; };
struct ObsRows { float *terms, *sel, *prop; int wt, ws, wp; };
__global__ void __launch_bounds__(256) obs_terms_kernel(ObsSources S, ObsRows R, const int2* __restrict__ prog, unsigned total) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;
  if (gid >= total) return;
  const unsigned W = (unsigned)(R.wt + R.ws + R.wp), e = gid / W, c = gid - e * W;
  const int2 r = prog[c];   // x: source, y: index inside the source's row
  float v;
  switch (r.x) {
    case OBS_SRC_ROW: v = S.row[(size_t)e * S.row_w + r.y]; break;
    case OBS_SRC_TIME: v = S.time[e]; break;
    case OBS_SRC_TARGET: v = S.target[(size_t)e * S.target_w + r.y]; break;
    case OBS_SRC_QPOS: v = S.qpos[(size_t)e * S.qpos_w + r.y]; break;
    case OBS_SRC_ACT: v = S.act[(size_t)e * S.act_w + r.y]; break;
    default: v = S.cst[r.y]; break;
  }
  if (c < (unsigned)R.wt) R.terms[(size_t)e * R.wt + c] = v;
  else if (c < (unsigned)(R.wt + R.ws)) R.sel[(size_t)e * R.ws + (c - R.wt)] = v;
  else R.prop[(size_t)e * R.wp + (c - R.wt - R.ws)] = v;
}

// ---- host
static constexpr char OBS_TERMS_CONFIGURED[] = "observation terms are enabled: the batch cannot be configured again (the column program is built from the configured task)";
// elements per env row of a source, as the batch stands (the bound every program index is checked against)
static int obs_source_width(const myo_batch* b, int src) {
  switch (src) {
    case OBS_SRC_ROW: return b->task.obs_dim;
    case OBS_SRC_TIME: return 1;
    case OBS_SRC_TARGET: return b->task.ntarget;
    case OBS_SRC_QPOS: return b->model->nq;
    case OBS_SRC_ACT: return b->model->dm.nu;
    default: return 3 + b->model->nq;
  }
}

static int obs_terms_enable(myo_batch* b, const int* sel, int nsel, const int* prop, int nprop) {
  const myo_model* m = b->model;
  const ObsTable t = obs_table(b);
  if (t.empty()) return fail(MYO_E_UNSUPPORTED, "observation terms: no task with a term table is configured (the MyoDM track task has none)");
  if (b->obs_terms.terms) return fail(MYO_E_ARG, "observation terms: already enabled (a batch selects its obs_keys / proprio_keys once)");
  if (b->task.task == MYO_TASK_WALK && g_lanes != 64) return fail(MYO_E_UNSUPPORTED, "observation terms: the walk task runs on the wave-per-env kernel only (lanes = 64)");
  if (!sel || nsel < 1 || nprop < 0 || (nprop > 0 && !prop)) return fail(MYO_E_ARG, "observation terms: at least one obs term; proprio terms may be none");
  const int nt = (int)t.size();
  for (int k = 0; k < nsel + nprop; k++) {
    const int i = k < nsel ? sel[k] : prop[k - nsel];
    if (i < 0 || i >= nt) return fail(MYO_E_ARG, "observation terms: term index out of range");
    if (t[i].width <= 0) return fail(MYO_E_ARG, std::string("observation terms: this model has no term ") + t[i].name);
  }
  // the constants: the pen's eps_ball (T.tip_site[4]) is a site of the world body, so its world position is its compiled position
  std::vector<float> cst((size_t)3 + m->nq, 0.f);
  if (b->task.task == MYO_TASK_PEN) {
    const int s = b->task.tip_site[4];
    if (m->site_body.empty() || m->site_pos0.empty()) return fail(MYO_E_UNSUPPORTED, "observation terms: the model blob lacks the site tables (obj_des_pos)");
    if (m->site_body[s] != 0) return fail(MYO_E_UNSUPPORTED, "observation terms: the pen's eps_ball site must be a site of the world body (obj_des_pos is a constant of the batch)");
    for (int k = 0; k < 3; k++) cst[k] = (float)m->site_pos0[3 * (size_t)s + k];
  }
  // slot of sim.data.act -> actuator
  std::vector<int> act_obs((size_t)m->dm.nu, -1), slot_act((size_t)m->dm.nu, -1);
  int rc;
  if (m->dm.nu > 0 && (rc = copy_to_host(m->device, act_obs.data(), (const void*)m->dm.act_obs, (size_t)m->dm.nu * 4))) return rc;
  for (int i = 0; i < m->dm.nu; i++) if (act_obs[i] >= 0 && act_obs[i] < m->dm.nu) slot_act[act_obs[i]] = i;
  // the program: one record per float of [terms | selected | proprio]; every index is checked against its source's row here, so the
  // kernel reads inside the batch's buffers whatever the table says
  std::vector<int2> prog;
  auto emit = [&](const ObsTerm& x) -> bool {
    const int sw = obs_source_width(b, x.src);
    for (int j = 0; j < x.width; j++) {
      int idx = x.src == OBS_SRC_TIME ? 0 : x.idx + j;
      if (x.src == OBS_SRC_ACT) idx = idx < m->dm.nu ? slot_act[idx] : -1;
      if (idx < 0 || idx >= sw) return false;
      prog.push_back(make_int2(x.src, idx));
    }
    return true;
  };
  int wt = 0, ws = 0, wp = 0;
  for (const ObsTerm& x : t) { if (!emit(x)) return fail(MYO_E_ARG, std::string("observation terms: term ") + x.name + " does not fit the configured task's buffers"); wt += x.width; }
  for (int k = 0; k < nsel; k++) { emit(t[sel[k]]); ws += t[sel[k]].width; }
  for (int k = 0; k < nprop; k++) { emit(t[prop[k]]); wp += t[prop[k]].width; }
  const size_t B = b->db.B, W = (size_t)wt + ws + wp;
  if (B * W >= (size_t)1 << 31) return fail(MYO_E_ARG, "observation terms: rows too large (B * width must stay below 2^31)");
  myo_obs_terms o;
  HIPCHK(hipSetDevice(m->device));
  if ((rc = b->pool.alloc(&o.terms, B * wt * 4)) || (rc = b->pool.alloc(&o.sel, B * ws * 4)) || (wp && (rc = b->pool.alloc(&o.prop, B * wp * 4))) ||
      (rc = b->pool.upload(&o.prog, prog.data(), prog.size())) || (rc = b->pool.upload(&o.cst, cst.data(), cst.size()))) return rc;
  o.wt = wt; o.ws = ws; o.wp = wp;
  b->obs_terms = o;
  return MYO_OK;
}

// after every launch that wrote MYO_F_OBS of a batch with the rows on
static int obs_terms_launch(myo_batch* b, hipStream_t s) {
  const myo_obs_terms& o = b->obs_terms;
  const myo_model* m = b->model;
  const ObsSources S{b->db.obs, b->db.time, b->db.target, b->db.qpos, b->db.act, o.cst, b->task.obs_dim, b->task.ntarget, m->nq, m->dm.nu};
  const ObsRows R{o.terms, o.sel, o.prop, o.wt, o.ws, o.wp};
  const unsigned total = (unsigned)b->db.B * (unsigned)(o.wt + o.ws + o.wp);
  hipLaunchKernelGGL(obs_terms_kernel, dim3((total + 255) / 256), dim3(256), 0, s, S, R, (const int2*)o.prog, total);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

static int obs_terms_buf(const myo_batch* b, int which, DevBuf* d) {
  const myo_obs_terms& o = b->obs_terms;
  if (!o.terms) return fail(MYO_E_ARG, "observation terms are not enabled (myo_batch_enable_obs_terms)");
  switch (which) {
    case MYO_OBS_TERMS: *d = {o.terms, (size_t)o.wt, 4}; break;
    case MYO_OBS_SELECTED: *d = {o.sel, (size_t)o.ws, 4}; break;
    case MYO_OBS_PROPRIO:
      if (!o.prop) return fail(MYO_E_ARG, "MYO_OBS_PROPRIO: no proprio terms were selected");
      *d = {o.prop, (size_t)o.wp, 4};
      break;
    default: return fail(MYO_E_ARG, "myo_batch_obs_buffer: unknown buffer");
  }
  return MYO_OK;
}

// one term of a table: its name (a string literal: outlives the table), width and offset in the canonical row (-1: from outside the row)
static int obs_term_out(const ObsTable& t, int k, const char** name, int* width, int* offset) {
  const bool in = k >= 0 && k < (int)t.size();
  if (name) *name = in ? t[k].name : nullptr;
  if (width) *width = in ? t[k].width : -1;
  if (offset) *offset = in && t[k].src == OBS_SRC_ROW ? t[k].idx : -1;
  return (int)t.size();
}
int myo_obs_term_table(int task, int nq, int nv, int nu, int na, int ntip, int pose_act, int k, const char** name, int* width, int* offset, int* row_dim) {
  const ObsTable t = obs_table(task, ObsDims{nq, nv, nu, na, ntip, pose_act});
  if (row_dim) *row_dim = t.dim;
  return obs_term_out(t, k, name, width, offset);
}
int myo_batch_obs_nterm(const myo_batch* b) { return b ? (int)obs_table(b).size() : 0; }
const char* myo_batch_obs_term_name(const myo_batch* b, int k) {
  const char* name = nullptr;
  if (b) obs_term_out(obs_table(b), k, &name, nullptr, nullptr);
  return name;
}
int myo_batch_obs_term_width(const myo_batch* b, int k) {
  int width = -1;
  if (b) obs_term_out(obs_table(b), k, nullptr, &width, nullptr);
  return width;
}
int myo_batch_enable_obs_terms(myo_batch* b, const int* obs_terms, int nobs, const int* proprio_terms, int nproprio) {
  return b ? obs_terms_enable(b, obs_terms, nobs, proprio_terms, nproprio) : fail(MYO_E_ARG, "myo_batch_enable_obs_terms: null");
}
int myo_batch_obs_buffer(myo_batch* b, int which, void** dev_ptr, size_t* pitch, size_t* width) {
  return buf_lookup(obs_terms_buf, b, which, dev_ptr, pitch, width, "myo_batch_obs_buffer: null");
}
int myo_batch_obs_read(myo_batch* b, int which, void* host, size_t nbytes) {
  return b ? buf_read(obs_terms_buf, b, which, host, nbytes, "myo_batch_obs_read: size mismatch") : fail(MYO_E_ARG, "myo_batch_obs_read: null");
}

#endif  // MYO_OBS_TERMS_H
