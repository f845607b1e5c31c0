// myo_host_forward.h -- the forward pass on the host (include/myo_hip_forward.h): the table of forward_kernel_w instantiations, the launch
// and the entry points.  The kernel, the export tables and the batch's buffers are in myo_kernel_forward.h.
#ifndef MYO_HOST_FORWARD_H
#define MYO_HOST_FORWARD_H

// The forward twins: forward_kernel_w<NVT, KC, NC, NTR, WPE, HF, TRK> with the template arguments of the run-time-sized step kernel of each
// size class.  A model the loader routes to a SPEC, SCHED or RK4 step kernel uses the twin of its class.
#define MYO_FORWARD_KERNELS(X)                                       \
  X(FK_HAND, "forward_kernel_w<24,8,32,1,3,false,false>", 24, 8, 32, 1, 3, false, false)       \
  X(FK_LEG, "forward_kernel_w<36,20,32,2,2,false,false>", 36, 20, 32, 2, 2, false, false)      \
  X(FK_TERRAIN, "forward_kernel_w<36,20,32,2,2,true,false>", 36, 20, 32, 2, 2, true, false)    \
  X(FK_TRK, "forward_kernel_w<36,20,32,2,2,false,true>", 36, 20, 32, 2, 2, false, true)
struct ForwardKernel {
  const char* name;
  void (*fn)(const DevModel*, const DevModelW*, DevBatch, FwdDev);
};
enum ForwardKernelId {
#define X(id, name, ...) id,
  MYO_FORWARD_KERNELS(X)
#undef X
};
static const ForwardKernel forward_kernels[] = {
#define X(id, name, ...) {name, forward_kernel_w<__VA_ARGS__>},
  MYO_FORWARD_KERNELS(X)
#undef X
};
static ForwardKernelId select_forward_kernel(const myo_model* m) {
  if (m->wave_cfg == 2) return FK_TRK;
  if (m->wave_cfg == 0) return FK_HAND;
  return m->dw.hf.on ? FK_TERRAIN : FK_LEG;
}

static int launch_forward(myo_batch* b, hipStream_t s) {
  const myo_model* m = b->model;
  static OncePerDevice attr;
  int rc = fwd_check(b);
  if (rc || (rc = fwd_start(b)) || (rc = set_lds_limit(attr, forward_kernels, 64 * 1024, m->device)) || (rc = obj_compose(b, s))) return rc;
  FwdDev F{};
  F.nbody = m->fwd_nbody; F.nsite = m->fwd_nsite; F.ngeom = m->fwd_ngeom; F.ncap = m->fwd_ncap; F.has_site_mat = m->fwd_site_mat;
  F.bq_body = b->bq_body;
  // die task: the goal offset moves the target body's exported frames.  Only for a target without collision geoms (the collision stages
  // would not move them): otherwise the offset stays out of the frames, as it stays out of the contacts
  bool target_collides = false;
  for (int cb : m->cg_body) if (cb == b->bq_body) target_collides = true;
  F.goal_off = (b->task.task == MYO_TASK_DIE && b->task.ntarget == 3 && b->bq_body > 0 && !target_collides) ? b->db.target : nullptr;
  F.body_rec = (gpf4)(const float4*)m->d_fwd_body; F.site_rec = (gpf4)(const float4*)m->d_fwd_site; F.geom_rec = (gpf4)(const float4*)m->d_fwd_geom;
  F.cg_geom = (gpi)m->d_fwd_cg_geom;
  F.xpos = (float*)b->fwd_buf[MYO_FWD_XPOS]; F.xmat = (float*)b->fwd_buf[MYO_FWD_XMAT]; F.xipos = (float*)b->fwd_buf[MYO_FWD_XIPOS];
  F.site_xpos = (float*)b->fwd_buf[MYO_FWD_SITE_XPOS]; F.site_xmat = (float*)b->fwd_buf[MYO_FWD_SITE_XMAT];
  F.geom_xpos = (float*)b->fwd_buf[MYO_FWD_GEOM_XPOS]; F.geom_xmat = (float*)b->fwd_buf[MYO_FWD_GEOM_XMAT];
  F.contact = (float*)b->fwd_buf[MYO_FWD_CONTACT]; F.ncon = (int*)b->fwd_buf[MYO_FWD_NCON];
  const ForwardKernel& k = forward_kernels[select_forward_kernel(m)];
  hipLaunchKernelGGL(k.fn, dim3(b->db.B), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm, (const DevModelW*)m->d_dw, b->db, F);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

int myo_forward(myo_batch* b, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_forward: null");
  HIPCHK(hipSetDevice(b->model->device));
  return launch_forward(b, (hipStream_t)stream);
}

int myo_model_forward_dims(const myo_model* m, int* nbody, int* nsite, int* ngeom, int* ncon_max) {
  if (!m) return fail(MYO_E_ARG, "myo_model_forward_dims: null");
  if (const int rc = fwd_model_check(m)) return rc;
  if (nbody) *nbody = m->fwd_nbody;
  if (nsite) *nsite = m->fwd_nsite;
  if (ngeom) *ngeom = m->fwd_ngeom;
  if (ncon_max) *ncon_max = m->fwd_ncap;
  return MYO_OK;
}

static int fwd_buffer(const myo_batch* b, int which, DevBuf* d) {
  if (which < 0 || which >= MYO_FWD_COUNT) return fail(MYO_E_ARG, "myo_forward_buffer: unknown buffer id");
  if (!b->fwd_on) return fail(MYO_E_ARG, "myo_forward_buffer: no forward pass has run on this batch (myo_forward)");
  if (which == MYO_FWD_SITE_XMAT && !b->model->fwd_site_mat) return fail(MYO_E_UNSUPPORTED, "MYO_FWD_SITE_XMAT: the model blob carries no site_quat");
  *d = {b->fwd_buf[which], (size_t)fwd_width(b->model, which), 4};
  return MYO_OK;
}

int myo_forward_buffer(myo_batch* b, int which, void** dev_ptr, size_t* pitch, size_t* width) {
  return buf_lookup(fwd_buffer, b, which, dev_ptr, pitch, width, "myo_forward_buffer: null");
}

int myo_forward_read(myo_batch* b, int which, void* host, size_t nbytes) {
  if (!b || !host) return fail(MYO_E_ARG, "myo_forward_read: null");
  return buf_read(fwd_buffer, b, which, host, nbytes, "myo_forward_read: size mismatch");
}

int myo_forward_host_tables(const void* blobv, size_t nbytes, int table, double* out, size_t capacity, int* n) {
  if (!blobv || nbytes < 16 || !n || table < 0 || table > 2) return fail(MYO_E_ARG, "myo_forward_host_tables: bad arguments");
  Blob B{};
  FwdTables T;
  int rc = blob_open(blobv, nbytes, "myo_forward_host_tables", &B);
  if (rc || (rc = fwd_build_tables(B, &T))) return rc;
  const std::vector<double>& v = table == 0 ? T.body : (table == 1 ? T.site : T.geom);
  *n = (int)(v.size() / FWD_REC);
  if (out && capacity >= v.size() && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(double));
  return MYO_OK;
}

#endif  // MYO_HOST_FORWARD_H
