// myo_host_objects.h -- per-env object parameters (include/myo_hip_objects.h): size, position and friction of up to 16 selected collision
// geoms and the mass of up to 4 selected bodies of a TrackEnv-class model.  The compiled arrays kept at model load, the refusals, the
// kernel that composes the rows the step / forward kernels read (once per launch), and the entry points.  What the kernels do with the rows
// is in the stages themselves: geom_world_pos and pair_decode / obj_pair_friction (myo_wave_util.h), the contact-row stage
// (myo_wave_solver.h), the cinert stage (myo_wave_motion.h), the geom frames of forward_kernel_w; the draws are part of reset_body
// (myo_reset.h).
// Part of the single translation unit myo_hip.hip (included there, before myo_host_step.h, whose launch_step composes); not a stand-alone header.
#ifndef MYO_HOST_OBJECTS_H
#define MYO_HOST_OBJECTS_H

static_assert(OBJ_MAX_DRAWS == MYO_OBJ_MAX_DRAWS, "the draw keys of obj_draw_u and the header's limit");

// One thread per (env, selected geom): the 12-float row the kernels read from the env's size / pos / friction rows.  The centre goes from
// the body's frame to the link's (hip_body_lpos / hip_body_lquat; for the balls and the die the two frames coincide and the position passes
// through bit for bit); positions inside a moving link are the same in the user's and in the lowered coordinates (the origin shift of the
// lowering moves root links and world-fixed items only)
__global__ void __launch_bounds__(256) obj_compose_kernel(DevBatch Bt, float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bt.B * Bt.obj_ng) return;
  const int s = t % Bt.obj_ng;
  const float* gc = Bt.obj_gc + 16 * s;
  const float *sz = Bt.obj_size + 3 * (size_t)t, *ps = Bt.obj_pos + 3 * (size_t)t, *fr = Bt.obj_fric + 3 * (size_t)t;
  float* o = out + 12 * (size_t)t;
  const float s0 = sz[0], s1 = sz[1], s2 = sz[2], p[3] = {ps[0], ps[1], ps[2]};
  float rp[3];
  matvec(rp, gc + 4, p);
  o[0] = s0; o[1] = s1; o[2] = s2; o[3] = obj_rbound(__float_as_int(gc[0]), s0, s1, s2);
  o[4] = gc[1] + rp[0]; o[5] = gc[2] + rp[1]; o[6] = gc[3] + rp[2]; o[7] = 0.f;
  o[8] = fr[0]; o[9] = fr[1]; o[10] = fr[2]; o[11] = 0.f;
}

// the compiled arrays of the model a selection starts from; optional in the blob (absent or mis-sized: myo_objects_enable refuses)
static int obj_model_tables(myo_model* m, const Blob& B) {
  for (const char* n : {"geom_type", "geom_bodyid", "geom_priority", "geom_size", "geom_pos", "geom_friction", "body_mass"}) if (!B.has(n)) return MYO_OK;
  m->geom_type0 = B.ints("geom_type"); m->geom_body0 = B.ints("geom_bodyid"); m->geom_priority0 = B.ints("geom_priority");
  m->geom_size0 = B.doubles("geom_size"); m->geom_pos0 = B.doubles("geom_pos"); m->geom_friction0 = B.doubles("geom_friction");
  m->body_mass_d = B.doubles("body_mass");
  if (B.rc) return B.rc;
  const size_t ng = m->geom_type0.size(), nb = m->body_link.size();
  m->obj_ok = m->geom_body0.size() == ng && m->geom_priority0.size() == ng && m->geom_size0.size() == 3 * ng && m->geom_pos0.size() == 3 * ng &&
              m->geom_friction0.size() == 3 * ng && m->body_mass_d.size() == nb && m->body_lpos.size() == 3 * nb && m->body_lquat.size() == 4 * nb;
  for (int g : m->cg_geom) if (g < 0 || (size_t)g >= ng) m->obj_ok = false;
  for (int gb : m->geom_body0) if (gb < 0 || (size_t)gb >= nb) m->obj_ok = false;
  return MYO_OK;
}

// the refusals that depend on the model and the process, shared by the start and the launches after it (lanes may have changed)
static int obj_check(const myo_batch* b) {
  const myo_model* m = b->model;
  if (m->rk4) return fail(MYO_E_UNSUPPORTED, "object parameters: RK4 models are not supported");
  if (!(m->wave_ok && m->trk)) return fail(MYO_E_UNSUPPORTED, "object parameters: models of the TrackEnv class only (the other step kernels read the model's geom and link tables)");
  if (g_lanes != 64) return fail(MYO_E_UNSUPPORTED, "object parameters: wave-per-env kernel only (lanes = 64)");
  if (!m->obj_ok) return fail(MYO_E_UNSUPPORTED, "object parameters: the model blob lacks the compiled geom / body arrays");
  if (b->db.obj_draw && b->task.task == MYO_TASK_TRACK && b->track_flavour == 0)
    return fail(MYO_E_UNSUPPORTED, "object parameters: the MyoDM track task resets inside the step kernel, which draws nothing; write explicit values instead of a draw table");
  return MYO_OK;
}

// rows of the kernels from the tables, on the launch's stream: launch_step and launch_forward call it ahead of their kernel
static int obj_compose(myo_batch* b, hipStream_t s) {
  if (!b->obj_on) return MYO_OK;
  if (const int rc = obj_check(b)) return rc;
  if (b->db.obj_ng > 0) {
    const int n = b->db.B * b->db.obj_ng;
    hipLaunchKernelGGL(obj_compose_kernel, dim3((n + 255) / 256), dim3(256), 0, s, b->db, b->d_objk);
    HIPCHK(hipGetLastError());
  }
  return MYO_OK;
}

static int obj_enable(myo_batch* b, const int* geoms, int ng, const int* bodies, int nb) {
  const myo_model* m = b->model;
  DevBatch& d = b->db;
  int rc = obj_check(b);
  if (rc) return rc;
  if (ng > MYO_OBJ_MAX_GEOMS || nb > MYO_OBJ_MAX_BODIES) return fail(MYO_E_UNSUPPORTED, "object parameters: at most 16 geoms and 4 bodies");
  if (ng + nb == 0) return fail(MYO_E_ARG, "myo_objects_enable: no geom and no body selected");
  const std::vector<int> gsel(geoms, geoms + ng), bsel(bodies, bodies + nb);
  if (b->obj_on) return gsel == b->obj_geoms && bsel == b->obj_bodies ? MYO_OK : fail(MYO_E_ARG, "myo_objects_enable: the batch is enabled with another selection");
  const int ngeom = (int)m->geom_type0.size(), nbody = (int)m->body_link.size(), ncg = m->dm.ncg, nl = m->dm.nl;
  const int ngeom_tab = std::max(ngeom, m->fwd_ngeom);
  std::vector<int> slot((size_t)ncg + ngeom_tab + nl, -1);
  std::vector<float> gc((size_t)std::max(ng, 1) * 16, 0.f);
  for (int k = 0; k < ng; k++) {
    const int g = gsel[k];
    if (g < 0 || g >= ngeom) return fail(MYO_E_ARG, "myo_objects_enable: geom id out of range");
    const int ty = m->geom_type0[g];
    if (ty == 7) return fail(MYO_E_UNSUPPORTED, "object parameters: mesh / hull geoms are not supported (their shape is a vertex table, not a size)");
    if (ty == 0 || ty == 1) return fail(MYO_E_UNSUPPORTED, "object parameters: plane and height-field geoms are not supported");
    if (ty != GEOM_SPHERE && ty != GEOM_CAPSULE && ty != GEOM_ELLIPSOID && ty != GEOM_CYLINDER && ty != 6) return fail(MYO_E_UNSUPPORTED, "object parameters: sphere / capsule / ellipsoid / cylinder / box geoms only");
    int cg = -1;
    for (int i = 0; i < ncg; i++) if (m->cg_geom[i] == g) cg = i;
    if (cg < 0) return fail(MYO_E_UNSUPPORTED, "object parameters: not a collision geom of this model (it takes part in no collision pair)");
    if (slot[cg] >= 0) return fail(MYO_E_ARG, "myo_objects_enable: a geom is listed twice");
    const int body = m->geom_body0[g];
    if (m->body_link[body] < 0) return fail(MYO_E_UNSUPPORTED, "object parameters: geoms of a body welded to the world are not supported");
    slot[cg] = k; slot[(size_t)ncg + g] = k;
    float* G = &gc[16 * (size_t)k];
    double R[9];
    const double q[4] = {m->body_lquat[4 * (size_t)body], m->body_lquat[4 * (size_t)body + 1], m->body_lquat[4 * (size_t)body + 2], m->body_lquat[4 * (size_t)body + 3]};
    quat2mat_d(R, q);
    G[0] = bits_f(ty);
    for (int c = 0; c < 3; c++) G[1 + c] = m->body_lpos[3 * (size_t)body + c];
    for (int c = 0; c < 9; c++) G[4 + c] = (float)R[c];
  }
  for (int k = 0; k < nb; k++) {
    const int body = bsel[k];
    if (body <= 0 || body >= nbody) return fail(MYO_E_ARG, "myo_objects_enable: body id out of range");
    const int l = m->body_link[body];
    if (l < 0 || l >= nl) return fail(MYO_E_UNSUPPORTED, "object parameters: a body welded to the world has no mass in the dynamics");
    int members = 0;
    for (int o = 1; o < nbody; o++) members += m->body_link[o] == l;
    if (members != 1) return fail(MYO_E_UNSUPPORTED, "object parameters: the body shares its kinematic link with other bodies (its mass alone does not give the link's mass, COM and inertia)");
    if (slot[(size_t)ncg + ngeom_tab + l] >= 0) return fail(MYO_E_ARG, "myo_objects_enable: a body is listed twice");
    slot[(size_t)ncg + ngeom_tab + l] = k;
  }
  std::vector<float> cgf((size_t)std::max(ncg, 1) * 4, 0.f);
  for (int i = 0; i < ncg; i++) {
    const int g = m->cg_geom[i];
    for (int c = 0; c < 3; c++) cgf[4 * (size_t)i + c] = (float)m->geom_friction0[3 * (size_t)g + c];
    cgf[4 * (size_t)i + 3] = (float)m->geom_priority0[g];
  }
  const size_t B = (size_t)d.B;
  std::vector<float> sz(B * 3 * ng), ps(B * 3 * ng), fr(B * 3 * ng), ms(B * nb);
  for (size_t e = 0; e < B; e++) {
    for (int k = 0; k < ng; k++)
      for (int c = 0; c < 3; c++) {
        const size_t i = (e * ng + k) * 3 + c, j = 3 * (size_t)gsel[k] + c;
        sz[i] = (float)m->geom_size0[j]; ps[i] = (float)m->geom_pos0[j]; fr[i] = (float)m->geom_friction0[j];
      }
    for (int k = 0; k < nb; k++) ms[e * nb + k] = (float)m->body_mass_d[bsel[k]];
  }
  HIPCHK(hipSetDevice(m->device));
  float *dsz = nullptr, *dps = nullptr, *dfr = nullptr, *dms = nullptr, *dk = nullptr, *dgc = nullptr, *dcgf = nullptr;
  int* dslot = nullptr;
  if (ng > 0 && ((rc = b->pool.upload(&dsz, sz.data(), sz.size())) || (rc = b->pool.upload(&dps, ps.data(), ps.size())) || (rc = b->pool.upload(&dfr, fr.data(), fr.size())) ||
                 (rc = b->pool.alloc(&dk, B * ng * 12 * 4)))) return rc;
  if (nb > 0 && (rc = b->pool.upload(&dms, ms.data(), ms.size()))) return rc;
  if ((rc = b->pool.upload(&dslot, slot.data(), slot.size())) || (rc = b->pool.upload(&dgc, gc.data(), gc.size())) || (rc = b->pool.upload(&dcgf, cgf.data(), cgf.size()))) return rc;
  d.obj_size = dsz; d.obj_pos = dps; d.obj_fric = dfr; d.obj_mass = dms; d.objk = dk; b->d_objk = dk;
  d.obj_slot = dslot; d.obj_gc = dgc; d.obj_cgf = dcgf;
  d.obj_ng = ng; d.obj_nb = nb; d.obj_ncg = ncg; d.obj_ngeom = ngeom_tab;
  d.obj_draw = nullptr; d.obj_draw_k = nullptr;
  b->obj_geoms = gsel; b->obj_bodies = bsel; b->obj_on = true;
  return MYO_OK;
}

// pointer and width of table `which`
static int obj_table(const myo_batch* b, int which, DevBuf* t) {
  if (which < 0 || which >= MYO_OBJ_COUNT) return fail(MYO_E_ARG, "object parameters: unknown table id");
  if (!b->obj_on) return fail(MYO_E_ARG, "object parameters: absent (the batch is not enabled, myo_objects_enable)");
  const DevBatch& d = b->db;
  float* p = which == MYO_OBJ_SIZE ? d.obj_size : (which == MYO_OBJ_POS ? d.obj_pos : (which == MYO_OBJ_FRICTION ? d.obj_fric : d.obj_mass));
  if (!p) return fail(MYO_E_ARG, which == MYO_OBJ_MASS ? "object parameters: no body is selected" : "object parameters: no geom is selected");
  *t = {p, which == MYO_OBJ_MASS ? (size_t)d.obj_nb : 3 * (size_t)d.obj_ng, 4};
  return MYO_OK;
}

extern "C" {

int myo_objects_enable(myo_batch* b, const int* geom_ids, int ngeom, const int* body_ids, int nbody) {
  if (!b || ngeom < 0 || nbody < 0 || (ngeom > 0 && !geom_ids) || (nbody > 0 && !body_ids)) return fail(MYO_E_ARG, "myo_objects_enable: bad arguments");
  return obj_enable(b, geom_ids, ngeom, body_ids, nbody);
}

int myo_objects_count(const myo_batch* b, int* ngeom, int* nbody) {
  if (!b) return fail(MYO_E_ARG, "myo_objects_count: null");
  if (ngeom) *ngeom = b->obj_on ? b->db.obj_ng : 0;
  if (nbody) *nbody = b->obj_on ? b->db.obj_nb : 0;
  return MYO_OK;
}

int myo_objects_table(myo_batch* b, int which, void** dev_ptr, size_t* pitch, size_t* width) {
  return buf_lookup(obj_table, b, which, dev_ptr, pitch, width, "myo_objects_table: null");
}

int myo_objects_read(myo_batch* b, int which, void* host, size_t nbytes) {
  if (!b || !host) return fail(MYO_E_ARG, "myo_objects_read: null");
  return buf_read(obj_table, b, which, host, nbytes, "myo_objects_read: size mismatch");
}

int myo_objects_write(myo_batch* b, int which, const void* host, size_t nbytes) {
  if (!b || !host) return fail(MYO_E_ARG, "myo_objects_write: null");
  DevBuf t; int rc;
  if ((rc = obj_table(b, which, &t)) || (rc = buf_check(b, t, host, nbytes, "myo_objects_write: size mismatch"))) return rc;
  const float* h = (const float*)host;
  for (size_t i = 0; i < (size_t)b->db.B * t.width; i++) {
    if (!std::isfinite(h[i])) return fail(MYO_E_ARG, "myo_objects_write: values must be finite");
    if (which != MYO_OBJ_POS && !(h[i] >= 0.f)) return fail(MYO_E_ARG, "myo_objects_write: sizes, frictions and masses must be >= 0");
  }
  return copy_to_device(b->model->device, t.p, host, nbytes);
}

int myo_objects_set_draws(myo_batch* b, int ndraw, int n, const float* base, const float* scale, const int* draw) {
  if (!b) return fail(MYO_E_ARG, "myo_objects_set_draws: null");
  if (!b->obj_on) return fail(MYO_E_ARG, "object parameters: absent (the batch is not enabled, myo_objects_enable)");
  DevBatch& d = b->db;
  if (n == 0 || !base || !scale || !draw) { d.obj_draw = nullptr; d.obj_draw_k = nullptr; return MYO_OK; }
  const int ng3 = 3 * d.obj_ng, np = 9 * d.obj_ng + d.obj_nb;
  if (b->task.task == MYO_TASK_TRACK && b->track_flavour == 0)
    return fail(MYO_E_UNSUPPORTED, "object parameters: the MyoDM track task resets inside the step kernel, which draws nothing; write explicit values instead of a draw table");
  if (n != np || ndraw < 0 || ndraw > MYO_OBJ_MAX_DRAWS) return fail(MYO_E_ARG, "myo_objects_set_draws: n must be 9 * ngeom + nbody and ndraw at most 8");
  std::vector<float> tab(2 * (size_t)np);
  for (int p = 0; p < np; p++) {
    const float lo = base[p], hi = base[p] + scale[p];
    if (!std::isfinite(lo) || !std::isfinite(hi)) return fail(MYO_E_ARG, "myo_objects_set_draws: base and scale must be finite");
    if (draw[p] < -1 || draw[p] >= ndraw) return fail(MYO_E_ARG, "myo_objects_set_draws: draw must be -1 or below ndraw");
    const bool is_pos = p >= ng3 && p < 2 * ng3;
    if (scale[p] != 0.f && !is_pos && !(lo >= 0.f && hi >= 0.f)) return fail(MYO_E_ARG, "myo_objects_set_draws: sizes, frictions and masses must stay >= 0 over the whole draw");
    tab[2 * (size_t)p] = base[p]; tab[2 * (size_t)p + 1] = scale[p];
  }
  HIPCHK(hipSetDevice(b->model->device));
  int rc;
  if (!b->d_obj_draw && ((rc = b->pool.alloc(&b->d_obj_draw, 2 * (size_t)np * 4)) || (rc = b->pool.alloc(&b->d_obj_draw_k, (size_t)np * 4)))) return rc;
  if ((rc = copy_to_device(b->model->device, b->d_obj_draw, tab.data(), tab.size() * 4)) || (rc = copy_to_device(b->model->device, b->d_obj_draw_k, draw, (size_t)np * 4))) return rc;
  d.obj_draw = b->d_obj_draw; d.obj_draw_k = b->d_obj_draw_k;
  return MYO_OK;
}

}  // extern "C"

#endif  // MYO_HOST_OBJECTS_H
