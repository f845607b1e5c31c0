// myo_host_batch.h -- the batch half of the host library: creation and destruction of a myo_batch, the per-env overrides (body masses,
// root-body offset, body orientation) as one record each, the sensor switch, and the table of fields behind myo_batch_field / read / write.
// A new per-env field is one row of field_rows[]; a new override is one Override record and the rows of its fields.
#ifndef MYO_HOST_BATCH_H
#define MYO_HOST_BATCH_H

static int batch_create(const myo_model* m, int B, myo_batch** out) {
  HIPCHK(hipSetDevice(m->device));
  std::unique_ptr<myo_batch> owner(new myo_batch());   // a failed create frees what it had allocated
  myo_batch* b = owner.get();   // (value-initialised: every pointer, flag and size not set below is null / 0)
  DevBatch& d = b->db;
  int nv = m->dm.nv, nu = m->dm.nu, nq = m->nq, rc;
  b->model = m; d.B = B; b->ntarget_alloc = nv > 24 ? nv : 24; b->obs_alloc = 3 * nv + 4 * nu + 64;
  b->sched_stride = (B + 7) / 8 + 1;                 // per queue with 8 queues; launch_step widens it when the device shows fewer XCDs
  if (m->wave_ok) {   // contact-table overflow rows of the wave kernel (instantiations <24,8,...> and <36,20,...>)
    const int kc = m->wave_cfg == 0 ? 8 : 20, nj = m->trk ? 4 : 3;
    d.ovf_row = 8 + nj * kc + (kc + 3) / 4 + (m->trk ? TRK_STATE : 0);
    d.ovf_rows = m->trk ? NCX2 : NCX;
  }
#define BA(ptr, n) if ((rc = b->pool.alloc(&ptr, (size_t)(n) * 4))) return rc;
  BA(d.qpos, (size_t)B * nq) BA(d.qvel, (size_t)B * nv) BA(d.act, (size_t)B * nu) BA(d.ctrl, (size_t)B * nu) BA(d.warm, (size_t)B * nv)
  BA(d.time, B) BA(d.target, (size_t)B * b->ntarget_alloc) BA(d.obs, (size_t)B * b->obs_alloc) BA(d.reward, B) BA(d.done, B)
  BA(d.solved, B) BA(d.qacc, (size_t)B * nv) BA(d.tenlen, (size_t)B * nu) BA(d.actforce, (size_t)B * nu) BA(d.sitexpos, (size_t)B * 24)
  BA(d.flags, B) BA(d.diag, (size_t)B * 8) BA(d.elapsed, B) BA(d.episode, B) BA(d.mprw, (size_t)B * 64)
  BA(b->d_tlo, b->ntarget_alloc) BA(b->d_thi, b->ntarget_alloc) BA(b->d_init, nq) BA(b->d_jlo, nv) BA(b->d_jhi, nv) BA(b->d_rnd, 4 * (size_t)nq)
  BA(b->d_action, (size_t)B * nu) BA(d.fatigue, (size_t)B * 3 * nu)
  if (m->trk) { BA(d.linkx, (size_t)B * 12 * m->dm.nl) }
  if (m->wave_ok) { BA(d.ovf, (size_t)B * d.ovf_rows * d.ovf_row) BA(d.ovf_cand, (size_t)B * NCANDX) }
  if (m->dw.hf.on) { BA(d.hfield, (size_t)B * m->dw.hf.nrow * m->dw.hf.ncol) }   // zero-filled: flat terrain at the geom's height
  BA(b->d_initv, nv) BA(b->d_init2, nq) BA(b->d_initv2, nv) BA(b->d_fatvec, nu) BA(b->d_walk, sizeof(DevWalk) / 4) BA(b->d_order, B) BA(b->d_sched, 32 + B + 64)
  BA(b->d_stamps, (size_t)B * 12 * 3 * 2)      // 3 x 12 long long per workgroup (diagnostic build)
#undef BA
  if (const char* e = getenv("MYO_LANES")) { int g = atoi(e); if (g == 16 || g == 32 || g == 64) g_lanes = g; }
  HIPCHK(hipMemcpy(b->d_jlo, m->jnt_lo.data(), nv * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_jhi, m->jnt_hi.data(), nv * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_init, m->qpos0.data(), nq * 4, hipMemcpyHostToDevice));
  std::vector<float> q((size_t)B * nq);   // default: every env at qpos0
  for (int e = 0; e < B; e++) memcpy(&q[(size_t)e * nq], m->qpos0.data(), nq * 4);
  HIPCHK(hipMemcpy(d.qpos, q.data(), q.size() * 4, hipMemcpyHostToDevice));
  std::vector<float> f((size_t)B * 3 * nu, 0.f);
  for (int e = 0; e < B; e++) for (int i = 0; i < nu; i++) f[(size_t)e * 3 * nu + nu + i] = 1.f;      // MR = 1
  HIPCHK(hipMemcpy(d.fatigue, f.data(), f.size() * 4, hipMemcpyHostToDevice));
  d.fat_dt = m->dm.timestep; d.reaf_epl = d.reaf_eip = -1; d.gsize_cg = -1;
  b->task.frame_skip = 1;   // (task = MYO_TASK_NONE = 0)
  b->task.jnt_lo = b->d_jlo; b->task.jnt_hi = b->d_jhi; b->task.init_qpos = b->d_init; b->task.target_lo = b->d_tlo; b->task.target_hi = b->d_thi;
  HIPCHK(hipEventCreate(&b->ev0)); HIPCHK(hipEventCreate(&b->ev1));
  *out = owner.release();
  return MYO_OK;
}

// ---- per-env overrides.  One record each: `check` = the refusals (also made by the launches after the start), `start` = allocate and
// initialise, `validate` = what a host write must satisfy (before the start: a rejected write starts nothing), `fill_default` = the rows a
// read returns before the start.  `on` is the override's flag in myo_batch.
struct Override {
  bool myo_batch::*on;
  int (*check)(const myo_batch*);
  int (*start)(myo_batch*);
  int (*validate)(const myo_batch*, int field, const float* h, int B, size_t width);
  int (*fill_default)(const myo_batch*, int field, float* h, int B, size_t width);
};

static int override_start(myo_batch* b, const Override& o) {
  if (b->*o.on) return MYO_OK;
  int rc = o.check(b);
  if (rc || (rc = o.start(b))) return rc;
  b->*o.on = true;
  return MYO_OK;
}

// every value finite and, for a range field (rows of lo (3) | hi (3)), lo <= hi
static int finite_rows(const float* h, int B, size_t width, bool range, const char* not_finite, const char* not_ordered) {
  for (size_t i = 0; i < (size_t)B * width; i++) if (!std::isfinite(h[i])) return fail(MYO_E_ARG, not_finite);
  for (int e = 0; range && e < B; e++) for (int k = 0; k < 3; k++) if (!(h[6 * e + 3 + k] >= h[6 * e + k])) return fail(MYO_E_ARG, not_ordered);
  return MYO_OK;
}

// body masses (MYO_F_BODYMASS / MYO_F_BODYMASS_RANGE)
static int bm_check(const myo_batch* b) {
  const myo_model* m = b->model;
  if (m->rk4) return fail(MYO_E_UNSUPPORTED, "per-env body masses: RK4 models are not supported");
  if (m->trk) return fail(MYO_E_UNSUPPORTED, "per-env body masses: models of the TrackEnv class are not supported");
  if (m->dw.hf.on) return fail(MYO_E_UNSUPPORTED, "per-env body masses: height-field models are not supported");
  if (!m->wave_ok || g_lanes != 64) return fail(MYO_E_UNSUPPORTED, "per-env body masses: wave-per-env kernel only (lanes = 64)");
  const int t = b->task.task;
  if (t == MYO_TASK_WALK || t == MYO_TASK_STAND || t == MYO_TASK_TRACK)
    return fail(MYO_E_UNSUPPORTED, "per-env body masses: the walk / stand / track tasks use model-wide mass totals");
  if (m->body_mass0.empty() || !m->d_lm_adr) return fail(MYO_E_UNSUPPORTED, "per-env body masses: the model blob lacks the body tables");
  return MYO_OK;
}
static int bm_default(const myo_batch* b, int field, float* h, int B, size_t width) {   // the model's masses, empty ranges
  if (b->model->body_mass0.empty()) return fail(MYO_E_UNSUPPORTED, "per-env body masses: the model blob lacks the body tables");
  for (int e = 0; e < B; e++) {
    if (field == MYO_F_BODYMASS) memcpy(h + (size_t)e * width, b->model->body_mass0.data(), width * 4);
    else memset(h + (size_t)e * width, 0, width * 4);
  }
  return MYO_OK;
}
static int bm_start(myo_batch* b) {
  const myo_model* m = b->model;
  DevBatch& d = b->db;
  const int nb = (int)m->body_mass0.size();
  float *bm = nullptr, *br = nullptr, *lc = nullptr; int rc;
  if ((rc = b->pool.alloc(&bm, (size_t)d.B * nb * 4)) || (rc = b->pool.alloc(&br, (size_t)d.B * 2 * nb * 4)) ||
      (rc = b->pool.alloc(&lc, (size_t)d.B * m->dm.nl * 10 * 4))) return rc;
  std::vector<float> v((size_t)d.B * nb);
  bm_default(b, MYO_F_BODYMASS, v.data(), d.B, nb);
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipMemcpy(bm, v.data(), v.size() * 4, hipMemcpyHostToDevice));
  d.bmass = bm; d.bmass_range = br; d.linkc = lc; d.nbody = nb;
  return MYO_OK;
}
static int bm_validate(const myo_batch* b, int field, const float* h, int B, size_t) {
  if (b->model->body_mass0.empty()) return fail(MYO_E_UNSUPPORTED, "per-env body masses: the model blob lacks the body tables");
  const size_t nb = b->model->body_mass0.size();
  for (int e = 0; e < B; e++)
    for (size_t i = 0; i < nb; i++) {
      if (field == MYO_F_BODYMASS) { if (!(h[e * nb + i] >= 0.f)) return fail(MYO_E_ARG, "MYO_F_BODYMASS: masses must be >= 0"); }
      else {
        const float lo = h[2 * e * nb + i], hi = h[2 * e * nb + nb + i];
        if (!(lo >= 0.f) || !(hi >= lo)) return fail(MYO_E_ARG, "MYO_F_BODYMASS_RANGE: need 0 <= lo <= hi");
      }
    }
  return MYO_OK;
}
static constexpr Override bm_override = {&myo_batch::bm_on, bm_check, bm_start, bm_validate, bm_default};

// root-body offset (MYO_F_BODYPOS / MYO_F_BODYPOS_RANGE): TrackEnv-class models whose last joint sits on a root body only
static int bp_check(const myo_batch* b) {
  const myo_model* m = b->model;
  if (!(m->wave_ok && m->trk)) return fail(MYO_E_UNSUPPORTED, "per-env body position: models of the TrackEnv class only");
  if (m->bp_link < 0) return fail(MYO_E_UNSUPPORTED, "per-env body position: the body of the model's last joint is not a root body (a child of the world heading its link)");
  return MYO_OK;
}
static int bp_start(myo_batch* b) {
  DevBatch& d = b->db;
  float *bp = nullptr, *br = nullptr; int rc;
  HIPCHK(hipSetDevice(b->model->device));
  if ((rc = b->pool.alloc(&bp, (size_t)d.B * 3 * 4)) || (rc = b->pool.alloc(&br, (size_t)d.B * 6 * 4))) return rc;   // zero: no offset
  d.bpos = bp; d.bpos_range = br; d.bpos_link = b->model->bp_link;
  return MYO_OK;
}
static int bp_validate(const myo_batch* b, int field, const float* h, int B, size_t width) {
  if (int rc = bp_check(b)) return rc;
  return finite_rows(h, B, width, field == MYO_F_BODYPOS_RANGE, "MYO_F_BODYPOS / MYO_F_BODYPOS_RANGE: values must be finite", "MYO_F_BODYPOS_RANGE: need lo <= hi");
}
static int bp_default(const myo_batch* b, int, float* h, int B, size_t width) {   // no offsets, empty ranges
  if (int rc = bp_check(b)) return rc;
  memset(h, 0, (size_t)B * width * 4);
  return MYO_OK;
}
static constexpr Override bp_override = {&myo_batch::bp_on, bp_check, bp_start, bp_validate, bp_default};

// orientation of one world-welded body (MYO_F_BODYQUAT / MYO_F_BODYQUAT_RANGE): TrackEnv-class models, the body selected first
// (myo_task_config.quat_body)
static int set_quat_body(myo_batch* b, int body) {
  const myo_model* m = b->model;
  if (!(m->wave_ok && m->trk)) return fail(MYO_E_UNSUPPORTED, "per-env body orientation: models of the TrackEnv class only");
  if (body <= 0 || body >= (int)m->body_parent.size()) return fail(MYO_E_ARG, "quat_body: body id out of range");
  if (m->body_parent[body] != 0 || m->body_jntnum[body] != 0) return fail(MYO_E_UNSUPPORTED, "per-env body orientation: a jointless child of the world only");
  if (b->bq_on && body != b->bq_body) return fail(MYO_E_ARG, "quat_body: the orientation of another body has started");
  b->bq_body = body;
  return MYO_OK;
}
static int bq_check(const myo_batch* b) {
  const myo_model* m = b->model;
  if (!(m->wave_ok && m->trk)) return fail(MYO_E_UNSUPPORTED, "per-env body orientation: models of the TrackEnv class only");
  if (b->bq_body < 0) return fail(MYO_E_ARG, "per-env body orientation: no body selected (myo_task_config.quat_body)");
  return MYO_OK;
}
static int bq_default(const myo_batch* b, int field, float* h, int B, size_t width) {   // the compiled quaternion, empty ranges
  if (int rc = bq_check(b)) return rc;
  for (int e = 0; e < B; e++)
    for (size_t k = 0; k < width; k++) h[(size_t)e * width + k] = field == MYO_F_BODYQUAT ? (float)b->model->body_quat0[4 * (size_t)b->bq_body + k] : 0.f;
  return MYO_OK;
}
static int bq_start(myo_batch* b) {
  const myo_model* m = b->model;
  DevBatch& d = b->db;
  const int bd = b->bq_body, ncg = m->dm.ncg, ns = m->dims.nsite;
  std::vector<float> q((size_t)d.B * 4), c(12);
  double R0[9];
  quat2mat_d(R0, &m->body_quat0[4 * (size_t)bd]);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) c[3 * i + j] = (float)R0[3 * j + i];   // R(q0)^T
  for (int k = 0; k < 3; k++) c[9 + k] = (float)(m->body_pos0[3 * (size_t)bd + k] - m->dm.origin[k]);   // (lowered coordinates)
  bq_default(b, MYO_F_BODYQUAT, q.data(), d.B, 4);
  std::vector<int> fl((size_t)ncg + ns, 0);
  for (int g = 0; g < ncg; g++) fl[g] = m->cg_body[g] == bd;
  for (int s2 = 0; s2 < ns; s2++) fl[ncg + s2] = m->site_body[s2] == bd;
  float *bq = nullptr, *br = nullptr, *bc = nullptr;
  int *bf = nullptr, rc;
  HIPCHK(hipSetDevice(m->device));
  if ((rc = b->pool.alloc(&bq, (size_t)d.B * 4 * 4)) || (rc = b->pool.alloc(&br, (size_t)d.B * 6 * 4)) ||
      (rc = b->pool.alloc(&bc, 12 * 4)) || (rc = b->pool.alloc(&bf, fl.size() * 4))) return rc;
  HIPCHK(hipMemcpy(bq, q.data(), q.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(bc, c.data(), c.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(bf, fl.data(), fl.size() * 4, hipMemcpyHostToDevice));
  d.bquat = bq; d.bquat_range = br; d.bq_c = bc; d.bq_flag = bf;
  return MYO_OK;
}
static int bq_validate(const myo_batch* b, int field, const float* h, int B, size_t width) {
  const bool range = field == MYO_F_BODYQUAT_RANGE;
  int rc = bq_check(b);
  if (rc || (rc = finite_rows(h, B, width, range, "MYO_F_BODYQUAT / MYO_F_BODYQUAT_RANGE: values must be finite", "MYO_F_BODYQUAT_RANGE: need lo <= hi"))) return rc;
  for (int e = 0; !range && e < B; e++) {
    const float* r = h + 4 * (size_t)e;
    const double n = std::sqrt((double)r[0] * r[0] + (double)r[1] * r[1] + (double)r[2] * r[2] + (double)r[3] * r[3]);
    if (!(std::fabs(n - 1.0) <= 1e-4)) return fail(MYO_E_ARG, "MYO_F_BODYQUAT: quaternions must have norm 1");
  }
  return MYO_OK;
}
static constexpr Override bq_override = {&myo_batch::bq_on, bq_check, bq_start, bq_validate, bq_default};

// touch sensors and contact forces (MYO_F_SENSORDATA / MYO_F_CFRC): the refusals, shared by the start and the launches after it.  Host
// side only: a refused model never reaches the GPU
static int sens_check(const myo_batch* b) {
  const myo_model* m = b->model;
  if (m->dw.ntouch <= 0) return fail(MYO_E_UNSUPPORTED, "sensors: the model blob has no touch sensors (no hip_touch table)");
  if (m->rk4) return fail(MYO_E_UNSUPPORTED, "sensors: RK4 models are not supported");
  if (m->trk) return fail(MYO_E_UNSUPPORTED, "sensors: models of the TrackEnv class are not supported");
  if (!m->wave_ok || m->wave_cfg != 1) return fail(MYO_E_UNSUPPORTED, "sensors: models of the hand class (24-dof step kernels) are not supported");
  if (g_lanes != 64) return fail(MYO_E_UNSUPPORTED, "sensors: wave-per-env kernel only (lanes = 64)");
  return MYO_OK;
}
static int enable_sensors(myo_batch* b) {
  int rc = sens_check(b);
  if (rc || b->sens_on) return rc;
  DevBatch& d = b->db; const int n = b->model->dw.ntouch;
  float *sd = nullptr, *cf = nullptr;
  HIPCHK(hipSetDevice(b->model->device));
  if ((rc = b->pool.alloc(&sd, (size_t)d.B * n * 4)) || (rc = b->pool.alloc(&cf, (size_t)d.B * 3 * (n + 1) * 4))) return rc;
  d.sens = sd; d.cfrc = cf; d.ntouch = n; b->sens_on = true;
  return MYO_OK;
}

// ---- the field table: one row per field id 0 .. MYO_F_CFRC, in id order.  A field whose row has an `absent` message does not exist while
// its pointer is null (no link frames, no geom override, no height field, track task not configured, sensors not enabled); an override
// field's pointer is null until the override has started.  Every element is 4 bytes (float32, or int32 where include/myo_hip.h says so) and
// the host side only copies bytes, so a row carries no element type: the header's comments are its one statement.
struct FieldRow {
  int id;
  void* (*ptr)(const myo_batch*);      // where the device pointer lives
  size_t (*width)(const myo_batch*);   // elements per env row (= pitch)
  const char* read_only;               // the error text of a host write; nullptr: writable
  const char* absent;                  // the error text while the pointer is null; nullptr: a null pointer is no error
  const Override* ov;                  // the override the field belongs to, or nullptr
};
#define FIELD(id, ptr_expr, width_expr, ...) \
  {id, [](const myo_batch* b) -> void* { return (void*)(ptr_expr); }, [](const myo_batch* b) -> size_t { return (size_t)(width_expr); }, __VA_ARGS__}
static constexpr char SENS_READ_ONLY[] = "MYO_F_SENSORDATA / MYO_F_CFRC are read-only";
static constexpr char SENS_ABSENT[] = "MYO_F_SENSORDATA / MYO_F_CFRC: sensors are not enabled (myo_batch_enable_sensors)";
static constexpr FieldRow field_rows[] = {
  FIELD(MYO_F_QPOS, b->db.qpos, b->model->nq),
  FIELD(MYO_F_QVEL, b->db.qvel, b->model->dm.nv),
  FIELD(MYO_F_ACT, b->db.act, b->model->dm.nu),
  FIELD(MYO_F_CTRL, b->db.ctrl, b->model->dm.nu),
  FIELD(MYO_F_WARMSTART, b->db.warm, b->model->dm.nv),
  FIELD(MYO_F_TIME, b->db.time, 1),
  FIELD(MYO_F_TARGET, b->db.target, b->task.ntarget > 0 ? b->task.ntarget : 1),
  FIELD(MYO_F_OBS, b->db.obs, b->task.obs_dim > 0 ? b->task.obs_dim : 1),
  FIELD(MYO_F_REWARD, b->db.reward, 1),
  FIELD(MYO_F_DONE, b->db.done, 1),
  FIELD(MYO_F_SOLVED, b->db.solved, 1),
  FIELD(MYO_F_FLAGS, b->db.flags, 1),
  FIELD(MYO_F_DIAG, b->db.diag, 8),
  FIELD(MYO_F_QACC, b->db.qacc, b->model->dm.nv),
  FIELD(MYO_F_TENLEN, b->db.tenlen, b->model->dm.nu),
  FIELD(MYO_F_ACTFORCE, b->db.actforce, b->model->dm.nu),
  FIELD(MYO_F_SITEXPOS, b->db.sitexpos, b->task.ntip > 0 ? 3 * b->task.ntip : 1),
  FIELD(MYO_F_ELAPSED, b->db.elapsed, 1),
  FIELD(MYO_F_ACTION, b->d_action, b->model->dm.nu),
  FIELD(MYO_F_FATIGUE, b->db.fatigue, 3 * b->model->dm.nu),
  FIELD(MYO_F_HFIELD, b->db.hfield, b->model->dw.hf.nrow * b->model->dw.hf.ncol, nullptr, "MYO_F_HFIELD: the model has no colliding height field"),
  FIELD(MYO_F_GEOMSIZE, b->db.gsize, 4, nullptr, "MYO_F_GEOMSIZE: no geom override set (myo_batch_set_geom_override)"),
  FIELD(MYO_F_LINKX, b->db.linkx, 12 * b->model->dm.nl, nullptr, "MYO_F_LINKX: this model's kernel does not export link frames"),
  FIELD(MYO_F_METRICS, b->d_metrics, 4, nullptr, "MYO_F_METRICS: the track task is not configured (myo_batch_configure_track)"),
  FIELD(MYO_F_BODYMASS, b->db.bmass, b->model->body_mass0.size(), nullptr, nullptr, &bm_override),
  FIELD(MYO_F_BODYMASS_RANGE, b->db.bmass_range, 2 * b->model->body_mass0.size(), nullptr, nullptr, &bm_override),
  FIELD(MYO_F_BODYPOS, b->db.bpos, 3, nullptr, nullptr, &bp_override),
  FIELD(MYO_F_BODYPOS_RANGE, b->db.bpos_range, 6, nullptr, nullptr, &bp_override),
  FIELD(MYO_F_BODYQUAT, b->db.bquat, 4, nullptr, nullptr, &bq_override),
  FIELD(MYO_F_BODYQUAT_RANGE, b->db.bquat_range, 6, nullptr, nullptr, &bq_override),
  FIELD(MYO_F_SENSORDATA, b->db.sens, b->db.ntouch, SENS_READ_ONLY, SENS_ABSENT),
  FIELD(MYO_F_CFRC, b->db.cfrc, 3 * (b->db.ntouch + 1), SENS_READ_ONLY, SENS_ABSENT),
};
#undef FIELD
constexpr int N_FIELDS = sizeof field_rows / sizeof field_rows[0];
constexpr bool field_rows_in_id_order(int i = 0) { return i == N_FIELDS || (field_rows[i].id == i && field_rows_in_id_order(i + 1)); }
static_assert(N_FIELDS == MYO_F_CFRC + 1 && field_rows_in_id_order(), "field_rows: one row per field id of include/myo_hip.h, in id order");

static const FieldRow* field_row(int f) { return f >= 0 && f < N_FIELDS ? &field_rows[f] : nullptr; }
// pointer and width of a field as they are now (a write looks them up again after it has started an override)
static int field_info(const myo_batch* b, const FieldRow* row, DevBuf* d) {
  if (!row) return fail(MYO_E_ARG, "unknown field");
  void* p = row->ptr(b);
  if (!p && row->absent) return fail(MYO_E_ARG, row->absent);
  *d = {p, row->width(b), 4};
  return MYO_OK;
}

static int batch_field(myo_batch* b, int field, void** dev_ptr, size_t* pitch, size_t* width) {
  const FieldRow* row = field_row(field);
  DevBuf d; int rc;
  if ((row && row->ov && (rc = override_start(b, *row->ov))) || (rc = field_info(b, row, &d))) return rc;
  return buf_out(d, dev_ptr, pitch, width);
}
static int batch_read(myo_batch* b, int field, void* host, size_t nbytes) {
  const FieldRow* row = field_row(field);
  DevBuf d; int rc;
  if ((rc = field_info(b, row, &d)) || (rc = buf_check(b, d, host, nbytes, "myo_batch_read: size mismatch"))) return rc;
  if (row->ov && !(b->*row->ov->on)) return row->ov->fill_default(b, field, (float*)host, b->db.B, d.width);   // not started: a read starts nothing
  return copy_to_host(b->model->device, host, d.p, nbytes);
}
static int batch_write(myo_batch* b, int field, const void* host, size_t nbytes) {
  const FieldRow* row = field_row(field);
  DevBuf d; int rc;
  if (row && row->read_only) return fail(MYO_E_ARG, row->read_only);
  if ((rc = field_info(b, row, &d)) || (rc = buf_check(b, d, host, nbytes, "myo_batch_write: size mismatch"))) return rc;
  // a rejected write starts nothing; the start allocates, so the pointer is looked up again
  if (row->ov && ((rc = row->ov->validate(b, field, (const float*)host, b->db.B, d.width)) || (rc = override_start(b, *row->ov)) || (rc = field_info(b, row, &d)))) return rc;
  return copy_to_device(b->model->device, d.p, host, nbytes);
}

#endif  // MYO_HOST_BATCH_H
