// myo_host_model.h -- the pieces of myo_model_load over the blob view of myo_host.h: upload of the lowered tables, packing of the per-lane records (host only),
// choice of the kernel class (host only), member tables of the per-env overrides.
#ifndef MYO_HOST_MODEL_H
#define MYO_HOST_MODEL_H

// a table into the model's pool, four zero elements behind it
template <typename T, class P> static int upload(myo_model* m, const std::vector<T>& v, P* out) { return m->pool.upload(out, v.data(), v.size(), 4); }
// the tables the kernels read: blob array -> device (and, with keep, a host copy)
template <class P> static int load_f(myo_model* m, const Blob& B, const char* name, P* out, std::vector<float>* keep = nullptr) {
  const std::vector<float> v = B.floats(name);
  if (B.rc) return B.rc;
  if (keep) *keep = v;
  return upload(m, v, out);
}
template <class P> static int load_i(myo_model* m, const Blob& B, const char* name, P* out, std::vector<int>* keep = nullptr) {
  const std::vector<int> v = B.ints(name);
  if (B.rc) return B.rc;
  if (keep) *keep = v;
  return upload(m, v, out);
}

static void build_layout_w(const DevModel& d, DevModelW& w, int nvt, int kc, int nc, int nj = 3) {
  w.lay = layout_w(w.nq, d.nv, d.nu, d.nl, d.ngt, d.maxnnz, d.ncg, w.has_tl != 0, nvt, kc, nc, nj);   // (myo_kernel_wave.h: shared with the compile-time layouts)
}

static void build_layout(DevModel& d) {
  Lay& Y = d.lay;
  int o = 0;
  auto take = [&](int n) { int r = o; o += n; return r; };
  int nv = d.nv, nu = d.nu, nl = d.nl, ntri = nv * (nv + 1) / 2;
  Y.qpos = take(nv); Y.qvel = take(nv); Y.act = take(nu); Y.ctrl = take(nu); Y.warm = take(nv);
  Y.lpos = take(3 * nl); Y.lmat = take(9 * nl); Y.lquat = take(4 * nl); Y.axis = take(3 * nv); Y.anchor = take(3 * nv);
  Y.tJ = take(d.ngt * d.maxnnz); Y.tlen = take(d.ngt); Y.tforce = take(nu); Y.actdot = take(nu);
  Y.qfa = take(nv); Y.smooth = take(nv); Y.qas = take(nv); Y.qacc = take(nv); Y.Ma = take(nv); Y.grad = take(nv);
  Y.search = take(nv); Y.Mv = take(nv); Y.qfc = take(nv);
  Y.Mp = take(ntri); Y.Hp = take(ntri);
  Y.lsign = take(nv); Y.laref = take(nv); Y.lD = take(nv); Y.ljar = take(nv); Y.ljv = take(nv);
  // region A (spatial dynamics) is dead once Mp / smooth exist; region B (collision + contact rows) aliases it
  int regA = o;
  Y.cdof = take(6 * nv); Y.cinert = take(10 * nl); Y.crb = take(10 * nl); Y.cvel = take(6 * nl); Y.cacc = take(6 * nl); Y.cfrc = take(6 * nl);
  int endA = o;
  o = regA;
  Y.gpos = take(3 * d.ncg); Y.gmat = take(9 * d.ncg); Y.cand = take(NCAND);
  Y.cdist = take(NCON); Y.cpos = take(3 * NCON); Y.cnrm = take(3 * NCON); Y.cpair = take(NCON); Y.cJ = take(NCON * 3 * KCMAX);
  Y.caref = take(4 * NCON); Y.cD = take(NCON); Y.cjar = take(4 * NCON); Y.cjv = take(4 * NCON); Y.cimp = take(NCON);
  if (o < endA) o = endA;
  // pad so that the 64/G env slices start on different LDS banks
  o = (o + 31) / 32 * 32 + 8;
  Y.total = o;
}

// sizes and solver options
static int load_header(myo_model* m, const Blob& B) {
  DevModel& d = m->dm;
  const BlobRec *hs = B.find("hip_sizes"), *sz = B.find("sizes"), *op = B.find("opt");
  if (!hs || !sz || !op) return fail(MYO_E_BLOB, "myo_model_load: blob lacks hip_* tables (run lowering)");
  const int* H = (const int*)(B.p + hs->offset);
  const int* S = (const int*)(B.p + sz->offset);
  const double* O = (const double*)(B.p + op->offset);
  d.nl = H[0]; d.nlevel = H[1]; d.nv = H[2]; d.nu = H[3]; d.ngt = H[4]; d.nseg = H[5]; m->dw.ndl = H[6]; d.maxnnz = H[7]; d.nwg = H[8];
  d.ncg = H[9]; d.npair = H[10]; d.maxkc = H[11]; d.ns = H[12]; d.nM = S[11];
  m->nq = S[0];
  if (d.ngt != d.nu) return fail(MYO_E_UNSUPPORTED, "limited-only tendons are not supported by the HIP path yet");
  d.timestep = (float)O[0]; d.grav[0] = (float)O[1]; d.grav[1] = (float)O[2]; d.grav[2] = (float)O[3];
  d.tolerance = (float)O[4]; d.iterations = (int)O[5]; d.ls_iterations = (int)O[6]; d.ls_tolerance = (float)O[7];
  d.meaninertia = (float)O[9];
  d.newton_scale = 1.0f / (d.meaninertia * (float)(d.nv > 1 ? d.nv : 1));
  m->dims = myo_dims{S[0], S[1], S[2], 0, S[4], S[8], S[7], d.nl, 0, 0, 64, 0, d.timestep};   // (na, env_lds_bytes and ncon_max once the kernel class is known)
  return MYO_OK;
}

// the lowered tables both step kernels read, and the scalars that travel inside DevModel / DevModelW
static int load_tables(myo_model* m, const Blob& B) {
  DevModel& d = m->dm;
  DevModelW& w = m->dw;
  int rc = 0;
#define LF(field, name) if ((rc = load_f(m, B, name, &field))) return rc;
#define LI(field, name) if ((rc = load_i(m, B, name, &field))) return rc;
#define LIK(field, name, keep) if ((rc = load_i(m, B, name, &field, &m->keep))) return rc;
  LI(d.level_adr, "hip_level_adr") LIK(d.link_parent, "hip_link_parent", link_parent) LI(d.link_dofadr, "hip_link_dofadr") LIK(d.link_dofnum, "hip_link_dofnum", link_dofnum)
  LI(d.child_adr, "hip_child_adr") LI(d.child, "hip_child") LIK(d.dof_link, "hip_dof_link", dof_link) LIK(d.dof_type, "hip_dof_type", dof_type)
  LI(d.dof_parent, "dof_parentid") LIK(d.site_link, "hip_site_link", site_link) LI(d.wg_link, "hip_wg_link") LI(d.gt_seg_adr, "hip_gt_seg_adr")
  LI(d.gt_seg_num, "hip_gt_seg_num") LI(d.gt_dofs, "hip_gt_dofs") LI(d.seg, "hip_seg") LI(d.dl, "hip_dl") LI(d.col_adr, "hip_col_adr")
  LI(d.col, "hip_col") LI(d.cg_link, "hip_cg_link") LI(d.cg_type, "hip_cg_type") LI(d.pair_i, "hip_pair_i") LI(d.pair_dl, "hip_pair_dl")
  LF(d.link_pos, "hip_link_pos") LF(d.link_quat, "hip_link_quat") LF(d.link_mass, "hip_link_mass") LF(d.link_com, "hip_link_com")
  LF(d.link_inertia, "hip_link_inertia") LF(d.dof_pos, "hip_dof_pos") LF(d.dof_axis, "hip_dof_axis") LF(d.dof_damping, "dof_damping")
  LF(d.dof_armature, "dof_armature") LF(d.site_lpos, "hip_site_lpos") LF(d.wg_lpos, "hip_wg_lpos") LF(d.wg_lmat, "hip_wg_lmat")
  LF(d.wg_radius, "hip_wg_radius") LF(d.seg_div, "hip_seg_div") LF(d.gt_len0, "hip_gt_len0") LF(d.act, "hip_act") LF(d.cg_lpos, "hip_cg_lpos") LF(d.cg_lmat, "hip_cg_lmat")
  LF(d.cg_size, "hip_cg_size") LF(d.cg_rbound, "hip_cg_rbound") LF(d.pair_f, "hip_pair_f")
  std::vector<float> jl, tlv;
  if ((rc = load_f(m, B, "qpos0", &d.qpos0, &m->qpos0)) || (rc = load_f(m, B, "hip_jl", &d.jl, &jl))) return rc;
  const std::vector<float> c0 = B.floats("hip_c0"), org = B.floats("hip_origin");
  if (B.rc) return B.rc;
  for (int k = 0; k < 3; k++) { d.c0[k] = c0[k]; d.origin[k] = org[k]; }
  m->jnt_lo.resize(d.nv); m->jnt_hi.resize(d.nv);
  for (int i = 0; i < d.nv; i++) { m->jnt_lo[i] = jl[12 * i + 1]; m->jnt_hi[i] = jl[12 * i + 2]; }
  build_layout(d);
  m->env_lds_bytes = d.lay.total * 4;
  // wave-per-env kernel tables (one env per wavefront)
  LI(w.seg_order, "hip_seg_order") LI(w.seg_tendon, "hip_seg_tendon") LI(w.gt_dl, "hip_gt_dl") LF(w.link_mat0, "hip_link_mat0")
  const std::vector<int> nws = B.ints("hip_nwrapseg");
  if (B.rc) return B.rc;
  w.nwrapseg = nws[0];
  if ((rc = load_f(m, B, "hip_tl", &w.tl, &tlv))) return rc;
  w.has_tl = 0;
  for (int t = 0; t < d.ngt; t++) if (tlv[12 * t] != 0) w.has_tl = 1;
  m->has_tl = w.has_tl;
  const std::vector<int> fl = B.ints("hip_flags");
  if (B.rc) return B.rc;
  LI(w.link_free, "hip_link_free") LI(w.dof_qposadr, "hip_dof_qposadr") LI(w.link_chain_adr, "hip_link_chain_adr") LI(w.link_chain, "hip_link_chain")
  LI(w.eq_i, "hip_eq_i") LI(w.kin_base, "hip_kin_base") LI(w.kin_adr, "hip_kin_adr") LI(w.kin_vec, "hip_kin_vec") LF(w.eq_f, "hip_eq_f")
  const std::vector<int> ks = B.ints("hip_kin_size");
  if (B.rc) return B.rc;
  m->kin_floats = ks[0];   // checked against the Hessian scratch (nvt x (nvt + 1)) once the kernel class is known
  w.kin_dnmax = ks.size() > 1 ? ks[1] : 6;
  if (fl.size() < 6) return fail(MYO_E_BLOB, "hip_flags: blob predates the actuator-kind tables; recompile the model");
  w.has_free = fl[0]; w.nq = fl[1]; w.neq = fl[2]; w.has_j0 = fl[3]; d.na_obs = fl[4]; m->has_affine = fl[5] != 0;
  m->cg_geom = B.ints("hip_cg_geom"); m->cg_type_h = B.ints("hip_cg_type");
  const std::vector<int> hi = B.ints("hip_hf_i");
  const std::vector<float> hf = B.floats("hip_hf_f");
  if (B.rc) return B.rc;
  w.hf.on = hi[0]; w.hf.nrow = hi[1]; w.hf.ncol = hi[2]; w.hf.cg = hi[3];
  for (int k = 0; k < 4; k++) w.hf.size[k] = hf[k];
  for (int k = 0; k < 3; k++) w.hf.pos[k] = hf[4 + k];
  if (w.hf.on && (w.hf.nrow > 128 || w.hf.ncol > 100 || d.npair > 1023)) return fail(MYO_E_UNSUPPORTED, "height field: at most 128 x 100 cells and 1023 pairs");
  LF(w.gt_j0, "hip_gt_j0") LI(d.act_obs, "hip_act_obs")
  m->body_link = B.ints("hip_body_link"); m->body_lpos = B.floats("hip_body_lpos"); m->body_lquat = B.floats("hip_body_lquat"); m->mass = B.floats("hip_mass");
  if (B.rc) return B.rc;
  if (w.nq != m->nq) return fail(MYO_E_BLOB, "hip_flags disagrees with sizes");
  // TrackEnv model class (lowering: hip_trk = condim-4 pairs | friction loss | box / hull geoms): tables of the TRK instantiation
  w.fl = nullptr; w.mesh_vert = nullptr; w.mesh_rec = nullptr; w.mesh_startrec = nullptr; w.mesh_aabb = nullptr;
  if (B.has("hip_trk")) {
    const std::vector<int> tk = B.ints("hip_trk");
    if (B.rc) return B.rc;
    LF(w.fl, "hip_fl") LF(w.mesh_vert, "hip_mesh_vert") LF(w.mesh_rec, "hip_mesh_rec") LF(w.mesh_startrec, "hip_mesh_startrec") LF(w.mesh_aabb, "hip_mesh_aabb")
    m->trk = tk[0] || tk[1] || tk[2];
  }
#undef LF
#undef LI
#undef LIK
  return MYO_OK;
}

// compiled body tables of a TrackEnv-class model, for the per-env overrides of one body (all optional in the blob: absent = override refused)
static int load_body_tables(myo_model* m, const Blob& B) {
  auto opt_i = [&](const char* n) { return B.has(n) ? B.ints(n) : std::vector<int>(); };
  auto opt_d = [&](const char* n) { return B.has(n) ? B.doubles(n) : std::vector<double>(); };
  // bodies of MYO_F_BODYQUAT: the tree, compiled poses, and the body of every collision geom and site
  const std::vector<int> gb = opt_i("geom_bodyid"), jb = opt_i("jnt_bodyid"), jt = opt_i("jnt_type");
  m->body_parent = opt_i("body_parentid"); m->body_jntnum = opt_i("body_jntnum"); m->site_body = opt_i("site_bodyid");
  m->body_pos0 = opt_d("body_pos"); m->body_quat0 = opt_d("body_quat"); m->site_pos0 = opt_d("site_pos");
  if (B.rc) return B.rc;
  for (int g : m->cg_geom) m->cg_body.push_back(g >= 0 && g < (int)gb.size() ? gb[g] : -1);
  // the root body of MYO_F_BODYPOS: the body of the last joint, a child of the world at the origin of its own root link
  const std::vector<int>&bp = m->body_parent, &bl = m->body_link, &lpar = m->link_parent;
  const int bb = jb.empty() ? -1 : jb.back();
  if (bb > 0 && jt.size() == jb.size() && (jt.back() == 2 || jt.back() == 3)   // a slide / hinge (a free root takes its pose from qpos)
      && bb < (int)bp.size() && bb < (int)bl.size() && bp[bb] == 0) {
    const int l = bl[bb];
    bool head = l >= 0 && l < (int)lpar.size() && lpar[l] < 0;
    for (int k = 1; head && k < bb; k++) if (bl[k] == l) head = false;   // the body heads its link (no earlier body welded into it)
    if (head) m->bp_link = l;
  }
  return MYO_OK;
}

static float bits_f(int v) { float f; memcpy(&f, &v, 4); return f; }

// Packing: self-contained per-lane records (DevModelW::seg_rec, dl_pk, ...), denormalised copies of the lowered tables.  Host only.
struct PackedModel {
  std::vector<float> seg_rec, cg_rec, pair_rec;
  std::vector<int> dl_pk, pair_dl_pk, kin_pk, link_desc, link_adof, dof_anc;
};

// tendon segments: one SEGR x 4 float record each, and their three moment-arm lists as packed words in 16-byte rows
static int pack_segments(const myo_model* m, const Blob& B, PackedModel* P) {
  const DevModel& d = m->dm;
  const std::vector<int> seg = B.ints("hip_seg"), seg_order = B.ints("hip_seg_order"), seg_tendon = B.ints("hip_seg_tendon"), wg_link = B.ints("hip_wg_link"), dl = B.ints("hip_dl");
  const std::vector<float> seg_div = B.floats("hip_seg_div"), site_lpos = B.floats("hip_site_lpos"), wg_lpos = B.floats("hip_wg_lpos"), wg_lmat = B.floats("hip_wg_lmat"), wg_radius = B.floats("hip_wg_radius");
  if (B.rc) return B.rc;
  const std::vector<int>&site_link = m->site_link, &dof_type = m->dof_type;
  std::vector<int> dlp(std::max<size_t>(dl.size() / 3, 1), 0);
  for (size_t i = 0; i < dl.size() / 3; i++) {
    const int dd = dl[3 * i], sg = dl[3 * i + 1], slot = dl[3 * i + 2];
    if (dd < 0 || dd > 127 || slot < 0 || slot > 255 || sg < -32768 || sg > 32767) return fail(MYO_E_UNSUPPORTED, "moment-arm list entry does not fit the packed word");
    dlp[i] = dd | ((dof_type[dd] == 3 ? 1 : 0) << 7) | (slot << 8) | (int)((unsigned)sg << 16);
  }
  // (each segment's three lists are copied to 16-byte rows of their own: a lane reads a list four entries per load, the first row ahead of its use)
  std::vector<int>& dl4 = P->dl_pk;
  P->seg_rec.assign((size_t)std::max(d.nseg, 1) * SEGR * 4, 0.f);
  for (int idx = 0; idx < d.nseg; idx++) {
    const int si = seg_order[idx];
    const int* S = &seg[12 * (size_t)si];
    float* R = &P->seg_rec[(size_t)idx * SEGR * 4];
    for (int k = 0; k < 2; k++) { R[4 * k] = bits_f(site_link[S[k]]); for (int c = 0; c < 3; c++) R[4 * k + 1 + c] = site_lpos[3 * (size_t)S[k] + c]; }
    R[8] = bits_f(S[2]); R[9] = bits_f(S[3] >= 0 ? site_link[S[3]] : -2); R[10] = 1.0f / seg_div[si]; R[11] = bits_f(seg_tendon[si]);
    for (int k = 0; k < 3; k++) {
      const int a0 = S[4 + 2 * k], n = S[5 + 2 * k], adr4 = (int)(dl4.size() / 4);
      if (adr4 >= (1 << 20) || n < 0 || n >= (1 << 11) || (n > 0 && (a0 < 0 || (size_t)(a0 + n) > dl.size() / 3))) return fail(MYO_E_UNSUPPORTED, "tendon moment-arm lists too long for the packed segment record");
      for (int i = 0; i < n; i++) dl4.push_back(dlp[a0 + i]);
      while (dl4.size() % 4 || dl4.size() == (size_t)adr4 * 4) dl4.push_back(0);     // whole rows; an empty list still owns one (the lane loads it unconditionally)
      R[12 + k] = bits_f(adr4 | (n << 20));
    }
    R[15] = bits_f(S[10]);
    if (S[2] >= 0) {
      const int g = S[2];
      if (S[3] >= 0) for (int c = 0; c < 3; c++) R[16 + c] = site_lpos[3 * (size_t)S[3] + c];
      R[19] = wg_radius[g];
      R[20] = bits_f(wg_link[g]); for (int c = 0; c < 3; c++) R[21 + c] = wg_lpos[3 * (size_t)g + c];
      for (int c = 0; c < 9; c++) R[24 + c] = wg_lmat[9 * (size_t)g + c];
    }
  }
  if (dl4.empty()) dl4.resize(4, 0);
  return MYO_OK;
}

// collision geoms, pairs and the pairs' dof lists
static int pack_collision(const myo_model* m, const Blob& B, PackedModel* P) {
  const DevModel& d = m->dm;
  const std::vector<int> cg_link = B.ints("hip_cg_link"), pair_i = B.ints("hip_pair_i"), pair_dl = B.ints("hip_pair_dl");
  const std::vector<float> cg_lpos = B.floats("hip_cg_lpos"), cg_lmat = B.floats("hip_cg_lmat"), cg_size = B.floats("hip_cg_size"), cg_rb = B.floats("hip_cg_rbound"), pair_f = B.floats("hip_pair_f");
  if (B.rc) return B.rc;
  const std::vector<int>&cg_type = m->cg_type_h, &dof_type = m->dof_type;
  P->cg_rec.assign((size_t)std::max(d.ncg, 1) * 16, 0.f);
  P->pair_rec.assign((size_t)std::max(d.npair, 1) * 16, 0.f);
  for (int g = 0; g < d.ncg; g++) {
    float* R = &P->cg_rec[(size_t)g * 16];
    R[0] = bits_f(cg_link[g]); for (int c = 0; c < 3; c++) R[1 + c] = cg_lpos[3 * (size_t)g + c];
    for (int c = 0; c < 9; c++) R[4 + c] = cg_lmat[9 * (size_t)g + c];
    R[13] = bits_f(cg_type[g]); R[14] = cg_rb[g];
  }
  for (int q = 0; q < d.npair; q++) {
    const int* I = &pair_i[6 * (size_t)q];
    const float* F = &pair_f[12 * (size_t)q];
    if (I[0] > 255 || I[1] > 255 || I[3] > 255 || I[4] > 15 || I[5] > 15) return fail(MYO_E_UNSUPPORTED, "collision pair does not fit the packed pair record");
    float* R = &P->pair_rec[(size_t)q * 16];
    R[0] = bits_f(I[0] | (I[1] << 8) | (I[4] << 16) | (I[5] << 20) | (I[3] << 24)); R[1] = F[0]; R[2] = F[1]; R[3] = bits_f(I[2]);
    for (int c = 0; c < 3; c++) { R[4 + c] = cg_size[3 * (size_t)I[0] + c]; R[8 + c] = cg_size[3 * (size_t)I[1] + c]; }
    R[7] = cg_rb[I[0]]; R[11] = cg_rb[I[1]];
    R[12] = bits_f(cg_type[I[0]] | (cg_type[I[1]] << 8));
  }
  // (a contact carries pair | dofs << 11 | dof-list start << 16 in one word: step kernel, narrow phase -> row stage)
  if (d.npair > 2048 || pair_dl.size() / 2 >= (1u << 16) || d.maxkc > 31) return fail(MYO_E_UNSUPPORTED, "more than 2048 collision pairs, 65535 contact dof-list entries or 31 dofs per contact");
  P->pair_dl_pk.assign(std::max<size_t>(pair_dl.size() / 2, 1), 0);
  for (size_t i = 0; i < pair_dl.size() / 2; i++) {
    const int dd = pair_dl[2 * i], sg = pair_dl[2 * i + 1];
    if (dd < 0 || dd > 127 || sg < -(1 << 22) || sg > (1 << 22)) return fail(MYO_E_UNSUPPORTED, "contact dof-list entry does not fit the packed word");
    P->pair_dl_pk[i] = dd | ((dof_type[dd] == 3 ? 1 : 0) << 7) | (int)((unsigned)sg << 8);
  }
  return MYO_OK;
}

// tree words: one packed word per lane and round for the sweeps over the kinematic tree (DevModelW::kin_pk, link_desc, link_adof, dof_anc)
static int pack_tree(myo_model* m, const Blob& B, const std::vector<int>& dpar, PackedModel* P) {
  const DevModel& d = m->dm;
  DevModelW& w = m->dw;
  const std::vector<int> kadr = B.ints("hip_kin_adr"), kvec = B.ints("hip_kin_vec"), chadr = B.ints("hip_link_chain_adr"), chain = B.ints("hip_link_chain");
  if (B.rc) return B.rc;
  const std::vector<int>& lpar = m->link_parent;
  if (d.nl > 64 || d.nv > 64) return fail(MYO_E_UNSUPPORTED, "more than 64 links or dofs");
  std::vector<int>& kpk = P->kin_pk;
  for (size_t L = 0; L + 1 < kadr.size(); L++) {
    for (int e0 = kadr[L]; e0 < kadr[L + 1]; e0 += 64) {
      for (int i = 0; i < 64; i++) {
        const int e = e0 + i;
        if (e >= kadr[L + 1]) { kpk.push_back(-1); continue; }
        const int w0 = kvec[2 * (size_t)e], src = kvec[2 * (size_t)e + 1], l = w0 & 255, kind = (w0 >> 8) & 3, ix = w0 >> 16, par1 = lpar[l] + 1;
        if (src < 0 || src >= 2048 || l >= 64 || ix < 0 || ix >= 64 || par1 < 0 || par1 > 64) return fail(MYO_E_UNSUPPORTED, "kinematics entry does not fit the packed word");
        kpk.push_back((int)((unsigned)src | ((unsigned)l << 11) | ((unsigned)kind << 17) | ((unsigned)ix << 19) | ((unsigned)par1 << 25)));
      }
    }
  }
  w.kin_nround = (int)(kpk.size() / 64);
  kpk.resize(kpk.size() + 64, -1);                       // padding round: the loop prefetches one round ahead
  std::vector<unsigned long long> desc(d.nl, 0), adof(d.nl, 0), anc(d.nv, 0);
  for (int l = d.nl - 1; l >= 0; l--) { desc[l] |= 1ull << l; if (lpar[l] >= 0) { if (lpar[l] >= l) return fail(MYO_E_BLOB, "links are not in tree order"); desc[lpar[l]] |= desc[l]; } }
  for (int q = 0; q < d.nv; q++) { if (dpar[q] >= q) return fail(MYO_E_BLOB, "dofs are not in tree order"); anc[q] = (1ull << q) | (dpar[q] >= 0 ? anc[dpar[q]] : 0ull); }
  unsigned long long frot = 0, fj3 = 0;
  for (int l = 0; l < d.nl; l++) {
    int prev = -1;
    for (int c = chadr[l]; c < chadr[l + 1]; c++) {
      const int e = chain[c], q = e & 255, j = (e >> 8) & 7, fr = e >> 12;
      if (q <= prev || q >= d.nv) return fail(MYO_E_BLOB, "link dof chain is not root-first");
      prev = q;
      adof[l] |= 1ull << q;
      if (fr && j >= 3) frot |= 1ull << q;
      if (fr && j == 3) fj3 |= 1ull << q;
    }
  }
  w.free_rot[0] = (unsigned)frot; w.free_rot[1] = (unsigned)(frot >> 32); w.free_j3[0] = (unsigned)fj3; w.free_j3[1] = (unsigned)(fj3 >> 32);
  auto split = [](const std::vector<unsigned long long>& v) { std::vector<int> o(std::max<size_t>(2 * v.size(), 2), 0); for (size_t i = 0; i < v.size(); i++) { o[2 * i] = (int)(unsigned)v[i]; o[2 * i + 1] = (int)(unsigned)(v[i] >> 32); } return o; };
  P->link_desc = split(desc); P->link_adof = split(adof); P->dof_anc = split(anc);
  return MYO_OK;
}

// Kernel class: which step kernels can take the model, the wave kernel's class and LDS layout, and whether the size-specialised
// instantiations may be used.  A function of the sizes and flags already on m; calls no HIP API.
static int classify(myo_model* m, const std::vector<int>& pair_i, const std::vector<int>& dpar) {
  const DevModel& d = m->dm;
  DevModelW& w = m->dw;
  bool plane_pairs = false, condim1 = false;
  for (int p = 0; p < d.npair; p++) { if (pair_i[6 * p + 4] >= 2) plane_pairs = true; if (pair_i[6 * p + 5] == 1) condim1 = true; }
  // the 16/32-lane generic kernel covers fixed-base models with hinge / slide joints and capsule / convex pairs only
  m->generic_ok = !w.has_free && w.neq == 0 && !plane_pairs && !condim1 && w.nq == d.nv && d.maxkc <= KCMAX && !w.has_tl && !m->has_affine;
  const bool common = d.nl <= 64 && d.ncg <= (m->trk ? 128 : 64) && w.nq <= 64 && w.neq <= 64 && d.maxnnz <= 20;   // (geom ids are bytes in the pair record; the TRK kernel loops over geoms)
  const bool needs_full = w.has_free || w.neq > 0 || plane_pairs || condim1 || m->trk;
  if (m->trk) {
    if (!(common && d.nv <= 36 && d.nu <= 128 && d.ngt <= 128 && d.maxkc <= 20 && !w.hf.on && !w.has_tl)) return fail(MYO_E_UNSUPPORTED, "condim-4 / friction-loss / box / mesh model exceeds the limits of the TRK step kernel");
    m->wave_ok = true; m->wave_cfg = 2; m->generic_ok = false;
    build_layout_w(d, w, 36, 20, 32, 4);
  }
  else if (common && !needs_full && d.nv <= 24 && d.nu <= 64 && d.ngt <= 64 && d.maxkc <= 8) { m->wave_ok = true; m->wave_cfg = 0; build_layout_w(d, w, 24, 8, 32); }
  else if (common && d.nv <= 36 && d.nu <= 128 && d.ngt <= 128 && d.maxkc <= 20) { m->wave_ok = true; m->wave_cfg = 1; build_layout_w(d, w, 36, 20, 32); }
  else { m->wave_ok = false; build_layout_w(d, w, 24, 8, 32); }
  if (m->rk4) {
    if (!m->wave_ok || m->trk || w.hf.on) return fail(MYO_E_UNSUPPORTED, "RK4: wave kernel models without height field / TrackEnv features only");
    m->generic_ok = false;
  }
  // the specialised instantiations build in the table sizes, the dof tree (tree-sparse factorisation), no tendon-limit rows and their LDS
  // layout: all must be the model's.  They have no RK4 variant
  auto same_tree = [&](const int* ref, int n) { if ((int)dpar.size() != n) return false; for (int i = 0; i < n; i++) if (dpar[i] != ref[i]) return false; return true; };
  const bool spec = m->wave_ok && !m->rk4 && !w.has_tl;
  const bool leg_tree = m->wave_cfg == 1 && same_tree(SpecTree<2>::parent, SpecTree<2>::nv);
  m->hand_sizes = spec && m->wave_cfg == 0 && sizes_match<1>(w.nq, d.nv, d.nu, d.nl, d.nlevel, d.maxnnz, d.ngt, d.nseg, d.ncg, d.npair) &&
                  same_tree(SpecTree<1>::parent, SpecTree<1>::nv) && layout_match<1, 24, 8, 32, 3>(w.lay);
  m->leg_sizes = spec && leg_tree && sizes_match<2>(w.nq, d.nv, d.nu, d.nl, d.nlevel, d.maxnnz, d.ngt, d.nseg, d.ncg, d.npair) && layout_match<2, 36, 20, 32, 3>(w.lay);
  m->terrain_sizes = spec && leg_tree && w.hf.on && sizes_match<3>(w.nq, d.nv, d.nu, d.nl, d.nlevel, d.maxnnz, d.ngt, d.nseg, d.ncg, d.npair) && layout_match<3, 36, 20, 32, 3>(w.lay);
  if (const char* e = getenv("MYO_NO_SPEC")) if (atoi(e) == 1) m->hand_sizes = m->leg_sizes = m->terrain_sizes = false;   // tests: force the run-time-sized instantiations
  if (!m->wave_ok && !m->generic_ok) return fail(MYO_E_UNSUPPORTED, "model exceeds the limits of both step kernels (nv <= 36, nu <= 128, pair dofs <= 20)");
  const int nvt = m->wave_cfg == 0 ? 24 : 36;
  if (m->wave_ok && m->kin_floats > nvt * (nvt + 1)) return fail(MYO_E_UNSUPPORTED, "kinematics scratch exceeds the Hessian scratch it borrows");
  m->env_lds_bytes_w = w.lay.total * 4;
  if (m->wave_ok && m->env_lds_bytes_w > 64 * 1024) return fail(MYO_E_UNSUPPORTED, "wave kernel working set exceeds 64 KB of LDS");
  if (4 * m->env_lds_bytes > 160 * 1024) {
    if (!m->wave_ok) return fail(MYO_E_UNSUPPORTED, "model working set exceeds 160 KB of LDS per workgroup");
    m->generic_ok = false;
  }
  return MYO_OK;
}

// member tables of the per-env body-mass override (lowering.py's link recomposition, per body); absent or mis-sized body tables leave it off
static int load_body_mass_tables(myo_model* m, const Blob& B) {
  for (const char* n : {"body_mass", "body_ipos", "body_iquat", "body_inertia"}) if (!B.has(n)) return MYO_OK;
  const std::vector<double> bmass = B.doubles("body_mass"), ipos = B.doubles("body_ipos"), iquat = B.doubles("body_iquat"), inert = B.doubles("body_inertia"),
                            lpos = B.doubles("hip_body_lpos"), lquat = B.doubles("hip_body_lquat");
  if (B.rc) return B.rc;
  const int nb = (int)m->body_link.size(), nl = m->dm.nl;
  if (!((int)bmass.size() == nb && (int)ipos.size() == 3 * nb && (int)iquat.size() == 4 * nb && (int)inert.size() == 3 * nb &&
        (int)lpos.size() == 3 * nb && (int)lquat.size() == 4 * nb)) return MYO_OK;
  std::vector<int> adr(nl + 1, 0), body;
  std::vector<double> tab;
  for (int l = 0; l < nl; l++) {
    adr[l] = (int)body.size();
    for (int b = 1; b < nb; b++) {
      if (m->body_link[b] != l) continue;
      double Rl[9], Rq[9], Ri[9], c[3], I[9];
      quat2mat_d(Rl, &lquat[4 * b]); quat2mat_d(Rq, &iquat[4 * b]);
      for (int i = 0; i < 3; i++) {
        c[i] = lpos[3 * b + i];
        for (int j = 0; j < 3; j++) { c[i] += Rl[3 * i + j] * ipos[3 * b + j]; Ri[3 * i + j] = Rl[3 * i] * Rq[j] + Rl[3 * i + 1] * Rq[3 + j] + Rl[3 * i + 2] * Rq[6 + j]; }
      }
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) I[3 * i + j] = Ri[3 * i] * inert[3 * b] * Ri[3 * j] + Ri[3 * i + 1] * inert[3 * b + 1] * Ri[3 * j + 1] + Ri[3 * i + 2] * inert[3 * b + 2] * Ri[3 * j + 2];
      body.push_back(b);
      for (double v : {c[0], c[1], c[2], I[0], I[4], I[8], I[1], I[2], I[5], bmass[b]}) tab.push_back(v);
    }
  }
  adr[nl] = (int)body.size();
  int rc;
  if ((rc = upload(m, adr, &m->d_lm_adr)) || (rc = upload(m, body, &m->d_lm_body)) || (rc = upload(m, tab, &m->d_lm_tab))) return rc;
  m->body_mass0.assign(bmass.begin(), bmass.end());
  return MYO_OK;
}

// touch sensors (lowering.py hip_touch / hip_cg_body); optional in the blob: absent tables leave the model without sensors
static int load_touch_tables(myo_model* m, const Blob& B) {
  DevModelW& w = m->dw;
  w.ntouch = 0; w.touch = nullptr; w.cg_body = nullptr;
  if (!B.has("hip_touch") || !B.has("hip_cg_body")) return MYO_OK;
  const std::vector<double> t = B.doubles("hip_touch");
  const std::vector<int> cb = B.ints("hip_cg_body");
  if (B.rc) return B.rc;
  const int n = (int)(t.size() / 18);
  if (n == 0) return MYO_OK;
  if (t.size() != (size_t)n * 18 || (int)cb.size() != m->dm.ncg) return fail(MYO_E_BLOB, "hip_touch / hip_cg_body: unexpected shape");
  if (n > MYO_MAX_TOUCH) return fail(MYO_E_UNSUPPORTED, "more than 8 touch sensors");
  std::vector<float> rec((size_t)n * TOUCHR, 0.f);
  for (int s = 0; s < n; s++) {
    const double* T = &t[18 * (size_t)s];
    float* R = &rec[(size_t)s * TOUCHR];
    const int link = (int)T[0], type = (int)T[13], body = (int)T[17];
    if (link >= m->dm.nl || (type != GEOM_SPHERE && type != 6)) return fail(MYO_E_BLOB, "hip_touch: bad link or site type");
    R[0] = bits_f(link); R[13] = bits_f(type); R[17] = bits_f(body);
    for (int k = 1; k < 13; k++) R[k] = (float)T[k];
    for (int k = 14; k < 17; k++) R[k] = (float)T[k];
  }
  int rc;
  if ((rc = upload(m, rec, &w.touch)) || (rc = upload(m, cb, &w.cg_body))) return rc;
  w.ntouch = n;
  return MYO_OK;
}

// the whole load into a model that the caller owns (and frees on any failure)
static int load_model(myo_model* m, const Blob& B) {
  DevModel& d = m->dm;
  DevModelW& w = m->dw;
  int rc;
  if ((rc = load_header(m, B)) || (rc = load_tables(m, B))) return rc;
  if (m->trk && (rc = load_body_tables(m, B))) return rc;
  const std::vector<int> pair_i = B.ints("hip_pair_i"), dpar = B.ints("dof_parentid");   // (both uploaded above: present)
  // plane - cylinder and plane - sphere pairs (lowering.py pair types 6 / 7 and 8) have a narrow phase in the TRK instantiation only: never
  // dropped silently
  for (int p = 0; p < d.npair; p++) {
    if ((pair_i[6 * p + 4] == 6 || pair_i[6 * p + 4] == 7) && !m->trk) return fail(MYO_E_UNSUPPORTED, "plane - cylinder pairs need a model of the TrackEnv class");
    if (pair_i[6 * p + 4] == 8 && !m->trk) return fail(MYO_E_UNSUPPORTED, "plane - sphere pairs need a model of the TrackEnv class");
  }
  PackedModel P;
  if ((rc = pack_segments(m, B, &P)) || (rc = pack_collision(m, B, &P)) || (rc = pack_tree(m, B, dpar, &P))) return rc;
  if ((rc = upload(m, P.seg_rec, &w.seg_rec)) || (rc = upload(m, P.dl_pk, &w.dl_pk)) || (rc = upload(m, P.cg_rec, &w.cg_rec)) ||
      (rc = upload(m, P.pair_rec, &w.pair_rec)) || (rc = upload(m, P.pair_dl_pk, &w.pair_dl_pk)) || (rc = upload(m, P.kin_pk, &w.kin_pk)) ||
      (rc = upload(m, P.link_desc, &w.link_desc)) || (rc = upload(m, P.link_adof, &w.link_adof)) || (rc = upload(m, P.dof_anc, &w.dof_anc))) return rc;
  if (B.has("integrator")) { const std::vector<int> ig = B.ints("integrator"); if (B.rc) return B.rc; m->rk4 = !ig.empty() && ig[0] == 1; }
  if ((rc = classify(m, pair_i, dpar))) return rc;
  if ((rc = load_touch_tables(m, B))) return rc;
  if ((rc = m->pool.upload(&m->d_dm, &d, 1)) || (rc = m->pool.upload(&m->d_dw, &w, 1))) return rc;
  m->dims.na = d.na_obs;
  m->dims.env_lds_bytes = m->wave_ok ? m->env_lds_bytes_w : m->env_lds_bytes;
  m->dims.ncon_max = m->wave_ok ? (m->wave_cfg >= 1 ? 32 : NCONW) : NCON;
  if (m->wave_ok && !m->body_link.empty() && (rc = load_body_mass_tables(m, B))) return rc;
  return MYO_OK;
}

#endif  // MYO_HOST_MODEL_H
