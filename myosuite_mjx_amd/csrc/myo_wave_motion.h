// myo_wave_motion.h -- stages of the wave kernel: state check, kinematics, tendons and muscles, CRB + RNE, integration
// Part of the single translation unit myo_hip.hip (included by myo_kernel_wave.h); not a stand-alone header.
#ifndef MYO_WAVE_MOTION_H
#define MYO_WAVE_MOTION_H

// mj_checkPos / mj_checkVel.
// LDS: reads qpos, qvel; writes nothing.
template <class C, class LY> __device__ __forceinline__ void w_check_state(const WaveCtx<LY>& X, int lane, bool op, int& flags, bool& alive) {
  const LY& Y = X.Y; extern __shared__ __align__(16) float E[];
  const int nv = X.nv, nq = X.nq;
  bool bad = false;
  if (lane < nq) { float a = E[Y.qpos + lane]; bad = !(a == a) || fabsf(a) > MAXVALF; }
  if (lane < nv) { float b = E[Y.qvel + lane]; bad = bad || !(b == b) || fabsf(b) > MAXVALF; }
  if (__any(bad) && alive && !op) { flags |= MYO_FLAG_BAD_STATE; alive = false; }
}

// Kinematics (lane = link, then level by level).
// LDS: reads qpos; writes lpos, lmat, axis, anchor.  Scratch: sq holds the local vectors of phase 1 (the Hessian buffer is dead between the
// solver of one substep and the dynamics stage of the next) and is dead again on return.
template <class C, class LY> __device__ __forceinline__ void w_kinematics(const WaveCtx<LY>& X, int lane, int step) {
  constexpr bool TRK = C::TRK;
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; const DevBatch& Bt = X.Bt;
  const int env = X.env, nl_ = X.nl_, nsub = X.nsub;
  const bool has_free = X.has_free;
  // Phase 1, lane = link: the link's own joint chain in its PARENT's frame -- rotation columns, origin and, per dof, axis and anchor --
  // written as 4 + 2 * dofnum vectors to the (at this point dead) Hessian scratch; no link waits for another one here, so the sines /
  // cosines and the joint rotations of all links are evaluated side by side instead of level after level.  Free-joint links (roots)
  // take their world pose straight from qpos.  All 64 lanes run the arithmetic on a clamped link index and only the stores are
  // predicated (a variant with the trigonometry inside `if (lane < ...)` miscompiled in the generic instantiation).
  unsigned int kw = (unsigned int)W.kin_pk[lane];   // phase 2, round 0 (its latency hides behind the joint trigonometry of phase 1)
  {
    const int l = lane < nl_ ? lane : 0;
    const bool mine = lane < nl_;
    const float* lp = M.link_pos + 3 * l;
    float A[9], c[3] = {lp[0], lp[1], lp[2]};
    if constexpr (TRK) {   // per-env translation of one root link (MYO_F_BODYPOS): its origin, and with it its joints' anchors, moves
      if (Bt.bpos && l == Bt.bpos_link) {
        const float* o = Bt.bpos + 3 * (size_t)env;
        c[0] += o[0]; c[1] += o[1]; c[2] += o[2];
      }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) A[k] = W.link_mat0[9 * l + k];
    const int da = M.link_dofadr[l];
    int dn = M.link_dofnum[l];
    const bool isfree = has_free && W.link_free[l];
    if (isfree) {
      // free joint: pose straight from qpos (position + unit quaternion); its 3 translational dofs act like slides along
      // the world axes and its 3 rotational dofs like hinges about the body axes through the body origin
      const int qa = W.dof_qposadr[da];
      float pos[3] = {E[Y.qpos + qa], E[Y.qpos + qa + 1], E[Y.qpos + qa + 2]}, R[9];
      float q[4] = {E[Y.qpos + qa + 3], E[Y.qpos + qa + 4], E[Y.qpos + qa + 5], E[Y.qpos + qa + 6]};
      float qn = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      q[0] *= qn; q[1] *= qn; q[2] *= qn; q[3] *= qn;
      quat2mat(R, q);
      if (mine) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          E[Y.axis + 3 * (da + k)] = k == 0 ? 1.f : 0.f; E[Y.axis + 3 * (da + k) + 1] = k == 1 ? 1.f : 0.f; E[Y.axis + 3 * (da + k) + 2] = k == 2 ? 1.f : 0.f;
          E[Y.axis + 3 * (da + 3 + k)] = R[k]; E[Y.axis + 3 * (da + 3 + k) + 1] = R[3 + k]; E[Y.axis + 3 * (da + 3 + k) + 2] = R[6 + k];
#pragma unroll
          for (int cc = 0; cc < 3; cc++) { E[Y.anchor + 3 * (da + k) + cc] = pos[cc]; E[Y.anchor + 3 * (da + 3 + k) + cc] = pos[cc]; }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) E[Y.lpos + 3 * l + k] = pos[k];
#pragma unroll
        for (int k = 0; k < 9; k++) E[Y.lmat + 9 * l + k] = R[k];
      }
      dn = 0;
    }
    float* const ks = E + Y.sq + W.kin_base[l];
    // uniform trip count (the model's longest chain) with the body predicated per lane: a loop whose trip count differs between the lanes
    // would be a long divergent region around the trigonometry, with register spills inside it
    const int dnmax = W.kin_dnmax;
    for (int k = 0; k < dnmax; k++) {
      const bool act = k < dn;
      const int d = act ? da + k : da;
      const float* al = M.dof_axis + 3 * d;
      const float* dp = M.dof_pos + 3 * d;
      float ax[3], an[3];
      matvec(ax, A, al);
      matvec(an, A, dp);
      an[0] += c[0]; an[1] += c[1]; an[2] += c[2];
      if (mine && act) {
        ks[12 + 6 * k] = ax[0]; ks[13 + 6 * k] = ax[1]; ks[14 + 6 * k] = ax[2];
        ks[15 + 6 * k] = an[0]; ks[16 + 6 * k] = an[1]; ks[17 + 6 * k] = an[2];
      }
      const int qa = W.dof_qposadr[d];
      const float ang = E[Y.qpos + qa] - M.qpos0[qa];
      const bool hinge = M.dof_type[d] == 3;
      float sn, cs;
      sincos_jf(ang, &sn, &cs);
      const float oc = 1 - cs, x = al[0], y = al[1], z = al[2];
      const float Rj[9] = {cs + oc * x * x, oc * x * y - sn * z, oc * x * z + sn * y, oc * x * y + sn * z, cs + oc * y * y, oc * y * z - sn * x,
                           oc * x * z - sn * y, oc * y * z + sn * x, cs + oc * z * z};
      float An[9], v[3];
      matmul3(An, A, Rj);
      matvec(v, An, dp);
      const bool rot = act && hinge, lin = act && !hinge;
#pragma unroll
      for (int i = 0; i < 9; i++) A[i] = rot ? An[i] : A[i];
#pragma unroll
      for (int i = 0; i < 3; i++) c[i] = rot ? an[i] - v[i] : (lin ? c[i] + ax[i] * ang : c[i]);
    }
    if (mine && !isfree) {
#pragma unroll
      for (int cc = 0; cc < 3; cc++) { ks[3 * cc] = A[cc]; ks[3 * cc + 1] = A[3 + cc]; ks[3 * cc + 2] = A[6 + cc]; }   // column cc of the local rotation
      ks[9] = c[0]; ks[10] = c[1]; ks[11] = c[2];
    }
  }
  SYNC();
  // Phase 2, level by level, lane = (link of the level, vector): world = parent rotation x local vector (+ parent origin for points).
  // One packed word per lane and round (DevModelW::kin_pk), the next round's word in flight while this one is worked on.
  for (int r = 0; r < W.kin_nround; r++) {
    const unsigned int w0 = kw;
    kw = (unsigned int)W.kin_pk[(r + 1) * 64 + lane];
    if (w0 != 0xFFFFFFFFu) {
      const int src = w0 & 2047, l = (w0 >> 11) & 63, kind = (w0 >> 17) & 3, ix = (w0 >> 19) & 63, par = (int)(w0 >> 25) - 1;
      const float v[3] = {E[Y.sq + src], E[Y.sq + src + 1], E[Y.sq + src + 2]};
      float w[3] = {v[0], v[1], v[2]};
      if (par >= 0) {
        matvec(w, E + Y.lmat + 9 * par, v);
        if (kind & 1) { w[0] += E[Y.lpos + 3 * par]; w[1] += E[Y.lpos + 3 * par + 1]; w[2] += E[Y.lpos + 3 * par + 2]; }
      }
      if (kind == 0) { E[Y.lmat + 9 * l + ix] = w[0]; E[Y.lmat + 9 * l + 3 + ix] = w[1]; E[Y.lmat + 9 * l + 6 + ix] = w[2]; }
      else {
        float* const dst = kind == 1 ? E + Y.lpos + 3 * l : (kind == 2 ? E + Y.axis + 3 * ix : E + Y.anchor + 3 * ix);
        dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
      }
    }
    SYNC();
  }
  if constexpr (TRK) {   // link frames of the last substep's position stage (MYO_F_LINKX), world coordinates
    if (Bt.linkx && step == nsub - 1) {
      float* o = Bt.linkx + (size_t)env * 12 * nl_;
      for (int i = lane; i < 12 * nl_; i += 64) { const int l = i / 12, k = i - 12 * l; o[i] = k < 3 ? E[Y.lpos + 3 * l + k] + M.origin[k] : E[Y.lmat + 9 * l + (k - 3)]; }
    }
  }
}

// Tendons (lane = segment), muscles and actuator forces (lane = tendon).  Returns J^T f of the actuators for lane = dof.
// LDS: reads qpos, qvel, ctrl, lpos, lmat, axis, anchor; writes act (Euler: advanced here; RK4: actdot instead), region X in its tendon phase
// (tJ, tlen, tforce) and, for models with tendon limits, the persistent copy tJp.  Scratch: qfc collects J^T f and is dead on return.  Region X
// changes owner behind the last barrier: tJ / tlen / tforce are dead on return.
template <class C, class LY> __device__ __forceinline__ float w_tendons(const WaveCtx<LY>& X, int lane, int step, bool op, float (&actdot)[C::NTR], SubStamps& st_) {
  constexpr int NTR = C::NTR;
  constexpr bool RK4 = C::RK4, FULL = C::FULL;
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; const DevBatch& Bt = X.Bt; const DevWalk* const wk = X.wk;
  const int env = X.env, nv = X.nv, nu = X.nu, nq = X.nq, maxnnz_ = X.maxnnz_, ngt_ = X.ngt_, nseg_ = X.nseg_, nsub = X.nsub;
  const bool has_tl = X.has_tl;
  const float h = X.h;
  float tlen_r[NTR], tvel_r[NTR];
  if (W.has_j0) {   // joint transmission: constant moment arm, length = arm * joint coordinate (mj_transmission, mjTRN_JOINT)
    WFOR(i, ngt_ * maxnnz_) E[Y.tJ + i] = W.gt_j0[i];
    WFOR(i, ngt_) {
      float L = M.gt_len0[i];
      for (int k = 0; k < maxnnz_; k++) { const float a = W.gt_j0[i * maxnnz_ + k]; if (a != 0.f) L += a * E[Y.qpos + W.dof_qposadr[M.gt_dofs[i * maxnnz_ + k]]]; }
      E[Y.tlen + i] = L;
    }
  } else {
  WFOR(i, ngt_ * maxnnz_) E[Y.tJ + i] = 0.f;
  WFOR(i, ngt_) E[Y.tlen + i] = M.gt_len0[i];   // constant same-link segments, folded at lowering time
  }
  SYNC();
  for (int base = 0; base < nseg_; base += 64) {
    int idx = base + lane;
    if (idx < nseg_) {
      // the segment's record: four independent 16-byte loads (five more for a wrapping segment) carry everything the old chain
      // seg_order -> seg -> site_link / site_lpos / wg_* read word by word
      const gpf4 SR = W.seg_rec + (size_t)idx * SEGR;
      const float4 r0 = SR[0], r1 = SR[1], r2 = SR[2], r3 = SR[3];
      // (the wrapping segments come first in the order: in their rounds every lane asks for the whole record at once instead of waiting for
      // `g` to arrive before the second half is requested)
      float4 r4 = r0, r5 = r0, r6 = r0, r7 = r0, r8 = r0;
      if (base < W.nwrapseg) { r4 = SR[4]; r5 = SR[5]; r6 = SR[6]; r7 = SR[7]; r8 = SR[8]; }
      const int g = __float_as_int(r2.x), side_l = __float_as_int(r2.y), gts = __float_as_int(r2.w);
      const float invdiv = r2.z;
      float p0[3], p1[3];
      { const float lp[3] = {r0.y, r0.z, r0.w}; frame_point(Y, E, __float_as_int(r0.x), lp, p0); }
      { const float lp[3] = {r1.y, r1.z, r1.w}; frame_point(Y, E, __float_as_int(r1.x), lp, p1); }
      // first rows of the segment's moment-arm lists, in flight while the wrap geometry is worked out
      const int wa = __float_as_int(r3.x), wb = __float_as_int(r3.y), wc = __float_as_int(r3.z);
      const gpi4 DL = (gpi4)W.dl_pk;
      const int4 ea = DL[wa & 0xFFFFF];
      int4 eb = ea, ec = ea;
      if (g >= 0) { eb = DL[wb & 0xFFFFF]; ec = DL[wc & 0xFFFFF]; }
      float wlen = -1, wp[6];
      if (g >= 0) {
        const int gl = __float_as_int(r5.x);
        const float glp[3] = {r5.y, r5.z, r5.w}, glm[9] = {r6.x, r6.y, r6.z, r6.w, r7.x, r7.y, r7.z, r7.w, r8.x};
        float gpos[3], gmat[9], side[3] = {0, 0, 0};
        if (gl < 0) {
#pragma unroll
          for (int k = 0; k < 3; k++) gpos[k] = glp[k];
#pragma unroll
          for (int k = 0; k < 9; k++) gmat[k] = glm[k];
        } else {
          float v[3];
          matvec(v, E + Y.lmat + 9 * gl, glp);
#pragma unroll
          for (int k = 0; k < 3; k++) gpos[k] = E[Y.lpos + 3 * gl + k] + v[k];
          matmul3(gmat, E + Y.lmat + 9 * gl, glm);
        }
        if (side_l != -2) { const float lp[3] = {r4.x, r4.y, r4.z}; frame_point(Y, E, side_l, lp, side); }
        wlen = wrap_geom_inl(wp, p0, p1, gpos, gmat, r4.w, __float_as_int(r3.w) != 0, side, side_l != -2);   // always inline: an out-of-line copy passes its arrays through scratch memory
      }
      SUB(7);
      bool wr = wlen >= 0;
      float* Jt = E + Y.tJ + gts * maxnnz_;
      float L = straight_w(W, Y, E, Jt, p0, p1, wa & 0xFFFFF, wa >> 20, invdiv, !wr, ea);
      if (g >= 0) {
        L += straight_w(W, Y, E, Jt, p0, wp, wb & 0xFFFFF, wb >> 20, invdiv, wr, eb);
        L += straight_w(W, Y, E, Jt, wp + 3, p1, wc & 0xFFFFF, wc >> 20, invdiv, wr, ec);
        if (wr) L += wlen * invdiv;
      }
      atomicAdd(&E[Y.tlen + gts], L);
    }
  }
  if (lane < nv) E[Y.qfc + lane] = 0.f;   // actuator forces are scattered to their dofs below (the solver's force scratch is free here)
  SYNC();
  SUB(8);
#pragma unroll
  for (int rr = 0; rr < NTR; rr++) {  // lane = tendon (NTR rounds of 64): gather its segments, then the muscle
    int gt = lane + 64 * rr;
    tlen_r[rr] = 0.f; tvel_r[rr] = 0.f;
    if (gt >= ngt_) continue;
    const float* Jrow = E + Y.tJ + gt * maxnnz_;
    const float L = E[Y.tlen + gt];
    tlen_r[rr] = L;
    float vel = 0;
    for (int k = 0; k < maxnnz_; k++) {
      int d = M.gt_dofs[gt * maxnnz_ + k];
      if (d >= 0) vel += Jrow[k] * E[Y.qvel + d];
      if (has_tl) E[Y.tJp + gt * maxnnz_ + k] = Jrow[k];
    }
    tvel_r[rr] = vel;
    if (has_tl) { E[Y.tJp + ngt_ * maxnnz_ + gt] = L; E[Y.tJp + ngt_ * maxnnz_ + ngt_ + gt] = vel; }
    if (gt < nu) {
      const float* A = M.act + 16 * gt;
      float f, ad;
      if (A[10] < 0.f) { f = A[0] * clip_ctrlf(E[Y.ctrl + gt], A[12], A[13]) + A[1] + A[14] * (A[2] * L + A[3] * vel); ad = 0.f; }   // stateless affine actuator
      else muscle(A, A[14] * L, A[14] * vel, E[Y.act + gt], E[Y.ctrl + gt], &f, &ad);
      if constexpr (RK4) actdot[rr] = ad;
      else if (!op) E[Y.act + gt] += h * ad;   // Euler: the activation is advanced right here (nothing reads it again in this substep; a bad-state env is
                                               // reset as a whole afterwards), so no derivative stays live in a register across collision and solver
      const float ft = f * A[14];
      E[Y.tforce + gt] = ft;
      // J^T f of the actuators, lane = tendon: its <= maxnnz moment arms go to their dofs with LDS atomics (one lane per dof walking the
      // dof's whole column -- two dozen tendons for the wrist dofs -- was the longer chain)
      for (int k = 0; k < maxnnz_; k++) {
        const int d = M.gt_dofs[gt * maxnnz_ + k];
        if (d >= 0) atomicAdd(&E[Y.qfc + d], Jrow[k] * ft);
      }
    }
  }
  SYNC();
  const float qfa = lane < nv ? E[Y.qfc + lane] : 0.f;
  if (step == nsub - 1) {   // diagnostics of the last substep
    for (int i = lane; i < nu; i += 64) { Bt.tenlen[(size_t)env * nu + i] = E[Y.tlen + i]; Bt.actforce[(size_t)env * nu + i] = E[Y.tforce + i]; }
  }
  if (FULL && op) {   // walk observation, muscle block (walk_v0.py:283-285,354-361): length, clipped velocity, clipped force / 1000, then act
    // (WalkRow's muscle_length .. act, myo_common.h; the offsets stay spelled out here: through the record the step kernels' code changes)
    float* o = Bt.obs + (size_t)env * wk->obs_dim + (nq - 2 + nv + 16);
#pragma unroll
    for (int rr = 0; rr < NTR; rr++) {
      int gt = lane + 64 * rr;
      if (gt < nu) {
        float g = M.act[16 * gt + 14];
        o[gt] = g * tlen_r[rr];
        o[nu + gt] = clipf(g * tvel_r[rr], -100.f, 100.f);
        o[2 * nu + gt] = clipf(E[Y.tforce + gt] / (g != 0.f ? g : 1.f) * 1e-3f, -100.f, 100.f);
        o[3 * nu + gt] = E[Y.act + gt];
      }
    }
  }
  SYNC();  // region X changes owner: tendon scratch -> spatial dynamics
  SUB(9);
  return qfa;
}

// CRB + RNE (lane = link / dof): mass matrix and the smooth force  smooth = -damping qvel - bias + qfa.  Returns true when this was the walk
// task's observation pass (op): observation and reward are written from the link frames and velocities, and the substep ends here.
// LDS: reads qpos, qvel, lpos, lmat, axis, anchor; writes sq = M (row stride NVT + 1; lower triangle, MHL_A off or MROW: symmetric; zero
// elsewhere).  Scratch: region X in its dynamics phase (cdof, cinert, crb, cvel, cacc, cfrc), dead on return -- it changes owner to the
// collision stage behind the last barrier.
template <class C, class LY> __device__ __forceinline__ bool w_dynamics(const WaveCtx<LY>& X, int lane, bool op, float qfa, float& smooth, SubStamps& st_) {
  constexpr int NVT = C::NVT, SPEC = C::SPEC;
  constexpr bool SCHED = C::SCHED, HF = C::HF, TRK = C::TRK, RK4 = C::RK4, FULL = C::FULL, MROW = C::MROW, MHL_A = C::MHL_A;
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; const DevBatch& Bt = X.Bt; const DevWalk* const wk = X.wk;
  const int env = X.env, nv = X.nv, nq = X.nq, nl_ = X.nl_, kflags = X.kflags;
  const bool has_free = X.has_free;
  typedef Sizes<SPEC> Z;
  // reference point of the spatial (6-D) quantities: fixed for fixed-base models, the root link's origin for free-floating ones
  const float c0[3] = {has_free ? E[Y.lpos] : M.c0[0], has_free ? E[Y.lpos + 1] : M.c0[1], has_free ? E[Y.lpos + 2] : M.c0[2]};
  // tree words of this lane's link / dof and of the subtree-sum tasks, loaded here so that the sweeps below find them in registers
  typedef unsigned long long ull;
  constexpr bool M64 = NVT > 32;      // link / dof masks of the small instantiations fit the low word
  auto ld_mask = [&](gpi tab, int i) -> ull { const unsigned int lo = (unsigned int)tab[2 * i], hi = M64 ? (unsigned int)tab[2 * i + 1] : 0u; return (ull)lo | ((ull)hi << 32); };
  constexpr int BKG = SPEC ? (16 * Z::nl + 63) / 64 : 4;   // rounds of subtree-sum tasks per group (size-specialised: all of them)
  const ull adof_m = lane < nl_ ? ld_mask(W.link_adof, lane) : 0ull, anc_m = lane < nv ? ld_mask(W.dof_anc, lane) : 0ull;
  ull desc_m[BKG];
#pragma unroll
  for (int u = 0; u < BKG; u++) { const int l = (u * 64 + lane) >> 4; desc_m[u] = l < nl_ ? ld_mask(W.link_desc, l) : 0ull; }
  const int my_link = M.dof_link[lane < nv ? lane : 0];
  const float my_arm = M.dof_armature[lane < nv ? lane : 0], my_damp = M.dof_damping[lane < nv ? lane : 0];
  // per-env body masses (DevBatch.linkc, MYO_F_BODYMASS): the run-time-sizes hand / 36-dof instantiations read the link mass, COM and
  // inertia that link_compose_kernel recomposed for this env at the start of the launch; every other instantiation keeps the model's
  constexpr bool BMO = !SCHED && SPEC == 0 && !HF && !TRK && !RK4;
  if (lane < nl_) {
    int l = lane;
    const float* R = E + Y.lmat + 9 * l;
    const float* I = M.link_inertia + 6 * l;
    const float* lcom = M.link_com + 3 * l;
    const float* lmass = M.link_mass + l;
    if constexpr (BMO) {
      if (Bt.linkc) {   // [nl][10] of this env: mass, COM (3), inertia (xx yy zz xy xz yz) in the link frame
        const float* L = Bt.linkc + ((size_t)env * nl_ + l) * 10;
        lmass = L; lcom = L + 1; I = L + 4;
      }
    }
    float Il[9] = {I[0], I[3], I[4], I[3], I[1], I[5], I[4], I[5], I[2]}, T[9], Iw[9], com[3];
    matmul3(T, R, Il);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Iw[3 * i + j] = T[3 * i] * R[3 * j] + T[3 * i + 1] * R[3 * j + 1] + T[3 * i + 2] * R[3 * j + 2];
    matvec(com, R, lcom);
    float mass = *lmass;
    if constexpr (C::OBJ) {   // per-env mass of a selected body (DevBatch.obj_mass): the body is its link's only one, so the link's mass is the env's scalar
      if (Bt.obj_mass) { const int s = Bt.obj_slot[Bt.obj_ncg + Bt.obj_ngeom + l]; if (s >= 0) mass = Bt.obj_mass[(size_t)env * Bt.obj_nb + s]; }
    }
    float dif[3] = {E[Y.lpos + 3 * l] + com[0] - c0[0], E[Y.lpos + 3 * l + 1] + com[1] - c0[1], E[Y.lpos + 3 * l + 2] + com[2] - c0[2]};
    float ci[10];
    ci[0] = Iw[0] + mass * (dif[1] * dif[1] + dif[2] * dif[2]);
    ci[1] = Iw[4] + mass * (dif[0] * dif[0] + dif[2] * dif[2]);
    ci[2] = Iw[8] + mass * (dif[0] * dif[0] + dif[1] * dif[1]);
    ci[3] = Iw[1] - mass * dif[0] * dif[1];
    ci[4] = Iw[2] - mass * dif[0] * dif[2];
    ci[5] = Iw[5] - mass * dif[1] * dif[2];
    ci[6] = mass * dif[0]; ci[7] = mass * dif[1]; ci[8] = mass * dif[2]; ci[9] = mass;
#pragma unroll
    for (int k = 0; k < 10; k++) { E[Y.cinert + 10 * l + k] = ci[k]; E[Y.crb + 10 * l + k] = ci[k]; }
  }
  if (lane < nv) {
    int d = lane;
    const float* ax = E + Y.axis + 3 * d;
    float c[6];
    if (M.dof_type[d] == 3) {
      float off[3] = {c0[0] - E[Y.anchor + 3 * d], c0[1] - E[Y.anchor + 3 * d + 1], c0[2] - E[Y.anchor + 3 * d + 2]};
      c[0] = ax[0]; c[1] = ax[1]; c[2] = ax[2];
      cross3(c + 3, ax, off);
    } else { c[0] = c[1] = c[2] = 0; c[3] = ax[0]; c[4] = ax[1]; c[5] = ax[2]; }
#pragma unroll
    for (int k = 0; k < 6; k++) E[Y.cdof + 6 * d + k] = c[k];
  }
  WFOR(i, NVT * (NVT + 1)) E[Y.sq + i] = 0;
  SYNC();
  SUB(10);
  // velocity / acceleration sweep (mj_comVel + the forward half of mj_rne), ONE pass: lane = link walks the dofs of its whole
  // ancestor chain root-first (lowering table).  The chains are <= 7 dofs long, so redoing a parent's sums in every descendant
  // lane costs less than a level-by-level sweep with one barrier and a handful of active lanes per level.
  if (lane < nl_) {
    const int l = lane;
    float cvel[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, cacc[6] = {0.f, 0.f, 0.f, -M.grav[0], -M.grav[1], -M.grav[2]}, cvel_rot[6];
    const ull frot = has_free ? ((ull)W.free_rot[0] | ((ull)W.free_rot[1] << 32)) : 0ull, fj3 = has_free ? ((ull)W.free_j3[0] | ((ull)W.free_j3[1] << 32)) : 0ull;
    for (ull am = adof_m; am; am &= am - 1ull) {   // dofs of the chain root-first = ascending (DevModelW::link_adof): no table read inside the loop
      const int d = __builtin_ctzll(am);
      const bool rotf = has_free && ((frot >> d) & 1ull), j3 = has_free && ((fj3 >> d) & 1ull);
      float cd[6], cdd[6], qv = E[Y.qvel + d];
#pragma unroll
      for (int k = 0; k < 6; k++) cd[k] = E[Y.cdof + 6 * d + k];
      if (j3) {
#pragma unroll
        for (int k = 0; k < 6; k++) cvel_rot[k] = cvel[k];   // velocity after the translations, before any of the 3 rotations
      }
      cross_motion(cdd, rotf ? cvel_rot : cvel, cd);
#pragma unroll
      for (int k = 0; k < 6; k++) { cacc[k] += cdd[k] * qv; cvel[k] += cd[k] * qv; }
    }
    float ci[10], f[6], t[6], t1[6];
#pragma unroll
    for (int k = 0; k < 10; k++) ci[k] = E[Y.cinert + 10 * l + k];
    mul_inert_vec(f, ci, cacc);
    mul_inert_vec(t, ci, cvel);
    cross_force(t1, cvel, t);
#pragma unroll
    for (int k = 0; k < 6; k++) { E[Y.cvel + 6 * l + k] = cvel[k]; E[Y.cfrc + 6 * l + k] = f[k] + t1[k]; }
  }
  SYNC();
  if (FULL && op) {
    // ---- walk observation / reward (walk_v0.py:268-316, 363-470) from link frames and link velocities of this pass; the row is WalkRow's
    // qpos_without_xy .. phase_var (myo_common.h), its offsets spelled out here for the same reason (tests/test_gpu_task_rows.py holds the two together)
    float* o = Bt.obs + (size_t)env * wk->obs_dim;
    if (lane < nq - 2) o[lane] = E[Y.qpos + 2 + lane];                    // qpos_without_xy
    if (lane < nv) o[nq - 2 + lane] = E[Y.qvel + lane] * wk->dt;          // qvel * dt
    float mc[3] = {0.f, 0.f, 0.f}, ml = 0.f;
    if (lane < nl_) {
      float cw[3];
      matvec(cw, E + Y.lmat + 9 * lane, M.link_com + 3 * lane);
      ml = M.link_mass[lane];
#pragma unroll
      for (int k = 0; k < 3; k++) mc[k] = ml * (E[Y.lpos + 3 * lane + k] + cw[k]);
    }
    const float mmov = wave_sum(ml);
    const float sx = wave_sum(mc[0]), sy = wave_sum(mc[1]), sz = wave_sum(mc[2]);
    // MuJoCo's cvel is the velocity of the body-fixed point that coincides with the root's subtree COM (COM of the moving bodies)
    const float cm[3] = {sx / mmov, sy / mmov, sz / mmov};
    float mv[2] = {0.f, 0.f};
    if (lane < nl_) {
      const float* cv = E + Y.cvel + 6 * lane;
      float r[3] = {cm[0] - c0[0], cm[1] - c0[1], cm[2] - c0[2]}, wr[3];
      cross3(wr, cv, r);
      mv[0] = ml * (cv[3] + wr[0]); mv[1] = ml * (cv[4] + wr[1]);
    }
    const float cvx = -wave_sum(mv[0]) / wk->mass_total, cvy = -wave_sum(mv[1]) / wk->mass_total;   // walk_v0.py:438-444 (note the minus)
    const float height = (sz + wk->static_mcom[2]) / wk->mass_total;                                  // walk_v0.py:446-450,465-470
    if (lane == 0) {
      const int sb = nq - 2 + nv;
      o[sb] = cvx; o[sb + 1] = cvy;
      float q[4] = {E[Y.qpos + 3], E[Y.qpos + 4], E[Y.qpos + 5], E[Y.qpos + 6]};
      float qn = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      float u[4] = {q[0] * qn, q[1] * qn, q[2] * qn, q[3] * qn};
      const float* t = wk->lquat_tor;
      float tq[4] = {u[0] * t[0] - u[1] * t[1] - u[2] * t[2] - u[3] * t[3], u[0] * t[1] + u[1] * t[0] + u[2] * t[3] - u[3] * t[2],
                     u[0] * t[2] - u[1] * t[3] + u[2] * t[0] + u[3] * t[1], u[0] * t[3] + u[1] * t[2] - u[2] * t[1] + u[3] * t[0]};
      float tn = 1.0f / sqrtf(tq[0] * tq[0] + tq[1] * tq[1] + tq[2] * tq[2] + tq[3] * tq[3]);
      o[sb + 2] = tq[0] * tn; o[sb + 3] = tq[1] * tn; o[sb + 4] = tq[2] * tn; o[sb + 5] = tq[3] * tn;   // torso xquat
      float pl[3], pr[3], pp[3], v[3];
      matvec(v, E + Y.lmat + 9 * wk->link_tl, wk->lpos_tl);
#pragma unroll
      for (int k = 0; k < 3; k++) pl[k] = E[Y.lpos + 3 * wk->link_tl + k] + v[k];
      matvec(v, E + Y.lmat + 9 * wk->link_tr, wk->lpos_tr);
#pragma unroll
      for (int k = 0; k < 3; k++) pr[k] = E[Y.lpos + 3 * wk->link_tr + k] + v[k];
      matvec(v, E + Y.lmat + 9 * wk->link_pel, wk->lpos_pel);
#pragma unroll
      for (int k = 0; k < 3; k++) pp[k] = E[Y.lpos + 3 * wk->link_pel + k] + v[k];
      o[sb + 6] = pl[2]; o[sb + 7] = pr[2];                                    // feet heights (talus_l, talus_r)
      o[sb + 8] = height;
#pragma unroll
      for (int k = 0; k < 3; k++) { o[sb + 9 + k] = pl[k] - pp[k]; o[sb + 12 + k] = pr[k] - pp[k]; }   // feet relative to the pelvis
      const float phase = fmodf((float)Bt.elapsed[env] / (float)wk->hip_period, 1.0f);
      o[sb + 15] = phase;
      if (!(kflags & KF_OBS_ONLY)) {
        float dvy = wk->target_y_vel - cvy, dvx = wk->target_x_vel - cvx;
        float vel_reward = expf(-dvy * dvy) + expf(-dvx * dvx);
        float d0 = 0.8f * cosf(phase * 6.283185307179586f + 3.141592653589793f) - E[Y.qpos + wk->qadr_hfl];
        float d1 = 0.8f * cosf(phase * 6.283185307179586f) - E[Y.qpos + wk->qadr_hfr];
        float cyclic = sqrtf(d0 * d0 + d1 * d1);
        float dq[4] = {q[0] - wk->target_rot[0], q[1] - wk->target_rot[1], q[2] - wk->target_rot[2], q[3] - wk->target_rot[3]};
        float ref_rot = expf(-5.0f * sqrtf(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]));
        float mag = 0.25f * (fabsf(E[Y.qpos + wk->qadr_ja[0]]) + fabsf(E[Y.qpos + wk->qadr_ja[1]]) + fabsf(E[Y.qpos + wk->qadr_ja[2]]) +
                             fabsf(E[Y.qpos + wk->qadr_ja[3]]));
        float ja = expf(-5.0f * mag);
        float r00 = 1.0f - 2.0f * (q[2] * q[2] + q[3] * q[3]) / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        float done = (height < wk->min_height || fabsf(r00) > wk->max_rot) ? 1.f : 0.f;
        if (wk->knee_height > 0.f && height - 0.5f * (pl[2] + pr[2]) < wk->knee_height) done = 1.f;   // TerrainEnvV0._get_knee_condition (walk_v0.py:660-671)
        Bt.reward[env] = wk->w_vel * vel_reward + wk->w_done * done + wk->w_cyc * cyclic + wk->w_rot * ref_rot + wk->w_ja * ja;
        Bt.done[env] = done;
        Bt.solved[env] = vel_reward >= 1.0f ? 1.f : 0.f;
      }
    }
    return true;
  }
  // subtree sums of the link forces (6) and composite inertias (10): lane = (link, component) adds up the link's whole subtree (DevModelW::link_desc)
  // from the values the links wrote themselves, so no task waits for another one -- no level-by-level sweep with its chain of
  // level_adr -> child_adr -> child reads.  In place: a group of rounds reads, then writes; a later group (higher links) only reads links above its
  // own, which no earlier group has written.
  {
    const int nbk = (16 * nl_ + 63) >> 6;
    for (int r0 = 0; r0 < nbk; r0 += BKG) {
      float acc[BKG];
#pragma unroll
      for (int u = 0; u < BKG; u++) {
        const int idx = (r0 + u) * 64 + lane, l = idx >> 4, k = idx & 15;
        const int base = k < 6 ? Y.cfrc + k : Y.crb + (k - 6), str = k < 6 ? 6 : 10;
        ull dm = r0 == 0 ? desc_m[u] : (l < nl_ ? ld_mask(W.link_desc, l) : 0ull);
        float a = 0.f;
        for (; dm; dm &= dm - 1ull) a += E[base + str * __builtin_ctzll(dm)];
        acc[u] = a;
      }
      SYNC();
#pragma unroll
      for (int u = 0; u < BKG; u++) {
        const int idx = (r0 + u) * 64 + lane, l = idx >> 4, k = idx & 15;
        if (l < nl_) E[(k < 6 ? Y.cfrc + k : Y.crb + (k - 6)) + (k < 6 ? 6 : 10) * l] = acc[u];
      }
      SYNC();
    }
  }
  smooth = 0.f;
  if (lane < nv) {
    int d = lane, l = my_link;
    float cd[6], buf[6], crb[10];
#pragma unroll
    for (int k = 0; k < 6; k++) cd[k] = E[Y.cdof + 6 * d + k];
#pragma unroll
    for (int k = 0; k < 10; k++) crb[k] = E[Y.crb + 10 * l + k];
    float bias = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) bias += cd[k] * E[Y.cfrc + 6 * l + k];
    mul_inert_vec(buf, crb, cd);
    for (ull am = anc_m; am;) {   // the dof and its ancestors (DevModelW::dof_anc), highest first
      const int a = 63 - __builtin_clzll(am);
      am ^= 1ull << a;
      float sdot = 0;
#pragma unroll
      for (int k = 0; k < 6; k++) sdot += E[Y.cdof + 6 * a + k] * buf[k];
      if (a == d) sdot += my_arm;
      E[Y.sq + d * (NVT + 1) + a] = sdot;   // full symmetric copy: (d,a) and (a,d); a <= d, and only the MROW kernels read above the diagonal
      if (!MHL_A) E[Y.sq + a * (NVT + 1) + d] = sdot;
    }
    smooth = -my_damp * E[Y.qvel + d] - bias + qfa;
  }
  SYNC();  // region X changes owner: dynamics scratch -> collision / contact rows
  SUB(11);
  return false;
}

// One stage of mj_RungeKutta(4): accumulates the stage derivative and sets the state the next stage (or, after the fourth, the next
// substep) starts from.
// LDS: reads and writes qpos, qvel, act.  Scratch: xv (the integration velocity, for the free joint's quaternion).
template <class C, class LY> __device__ __forceinline__ void w_integrate_rk4(const WaveCtx<LY>& X, int lane, int rk_stage, RkAcc<C::NTR>& rk, const float (&actdot)[C::NTR], float qaccE, float& time) {
  constexpr int NTR = C::NTR;
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[];
  const int nv = X.nv, nu = X.nu;
  const bool has_free = X.has_free;
  const float h = X.h;
    const float Bw = (rk_stage == 0 || rk_stage == 3) ? (1.f / 6.f) : (1.f / 3.f), a = rk_stage < 2 ? 0.5f : 1.f;
    const bool last = rk_stage == 3;
    bool frot = false;
    if (rk_stage == 0) rk.t0 = time;
#pragma unroll
    for (int rr = 0; rr < NTR; rr++) {
      const int i = lane + 64 * rr;
      if (i < nu) {
        if (rk_stage == 0) { rk.a0[rr] = E[Y.act + i]; rk.sd[rr] = 0.f; }
        rk.sd[rr] += Bw * actdot[rr];
        E[Y.act + i] = rk.a0[rr] + h * (last ? rk.sd[rr] : a * actdot[rr]);
      }
    }
    float vint = 0.f;   // the velocity this lane's coordinate is advanced with, from X0, over h
    if (lane < nv) {
      const float vcur = E[Y.qvel + lane];
      const int fl = M.dof_link[lane];
      frot = has_free && W.link_free[fl] && lane - M.link_dofadr[fl] >= 3;
      if (rk_stage == 0) { rk.v0 = vcur; rk.sv = 0.f; rk.sa = 0.f; if (!frot) rk.q0 = E[Y.qpos + W.dof_qposadr[lane]]; }
      rk.sv += Bw * vcur; rk.sa += Bw * qaccE;
      vint = last ? rk.sv : a * vcur;
      E[Y.qvel + lane] = rk.v0 + h * (last ? rk.sa : a * qaccE);
      if (!frot) E[Y.qpos + W.dof_qposadr[lane]] = rk.q0 + h * vint;
      E[Y.xv + lane] = vint;
    }
    if (has_free) {
      SYNC();
      const int fl = lane < nv ? M.dof_link[lane] : 0;
      if (frot && lane - M.link_dofadr[fl] == 3) {
        const int qa = W.dof_qposadr[M.link_dofadr[fl]] + 3;
        if (rk_stage == 0) { rk.quat[0] = E[Y.qpos + qa]; rk.quat[1] = E[Y.qpos + qa + 1]; rk.quat[2] = E[Y.qpos + qa + 2]; rk.quat[3] = E[Y.qpos + qa + 3]; }
        float w[3] = {E[Y.xv + lane], E[Y.xv + lane + 1], E[Y.xv + lane + 2]};
        float wn = norm3(w), ang = h * wn;
        float o[4] = {rk.quat[0], rk.quat[1], rk.quat[2], rk.quat[3]};
        if (wn >= MINVALF) {
          float sn, cs;
          sincosf(0.5f * ang, &sn, &cs);
          const float inv = sn / wn, r[4] = {cs, w[0] * inv, w[1] * inv, w[2] * inv}, *q = rk.quat;
          o[0] = q[0] * r[0] - q[1] * r[1] - q[2] * r[2] - q[3] * r[3];
          o[1] = q[0] * r[1] + q[1] * r[0] + q[2] * r[3] - q[3] * r[2];
          o[2] = q[0] * r[2] - q[1] * r[3] + q[2] * r[0] + q[3] * r[1];
          o[3] = q[0] * r[3] + q[1] * r[2] - q[2] * r[1] + q[3] * r[0];
        }
        const float on = 1.0f / sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
        E[Y.qpos + qa] = o[0] * on; E[Y.qpos + qa + 1] = o[1] * on; E[Y.qpos + qa + 2] = o[2] * on; E[Y.qpos + qa + 3] = o[3] * on;
      }
    }
    time = uniformf(rk.t0 + (last ? h : a * h));
}

// Semi-implicit Euler: qvel += h qacc, qpos += h qvel (free joints through the quaternion).
// LDS: reads and writes qpos, qvel.
template <class C, class LY> __device__ __forceinline__ void w_integrate_euler(const WaveCtx<LY>& X, int lane, float qaccE, float& time) {
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[];
  const int nv = X.nv;
  const bool has_free = X.has_free;
  const float h = X.h;
  bool frot = false;
  if (lane < nv) {
    float v = E[Y.qvel + lane] + h * qaccE;
    E[Y.qvel + lane] = v;
    // rotational dofs of a free joint (dofs 3..5 of its link) integrate through the quaternion below
    const int fl = M.dof_link[lane];
    frot = has_free && W.link_free[fl] && lane - M.link_dofadr[fl] >= 3;
    if (!frot) E[Y.qpos + W.dof_qposadr[lane]] += h * v;
  }
  if (has_free) {   // free joints: quaternion integrated with the body-frame angular velocity (mju_quatIntegrate); one lane per joint
    SYNC();
    const int fl = lane < nv ? M.dof_link[lane] : 0;
    if (frot && lane - M.link_dofadr[fl] == 3) {
      const int qa = W.dof_qposadr[M.link_dofadr[fl]] + 3;
      float w[3] = {E[Y.qvel + lane], E[Y.qvel + lane + 1], E[Y.qvel + lane + 2]};
      float wn = norm3(w), ang = h * wn;
      float q[4] = {E[Y.qpos + qa], E[Y.qpos + qa + 1], E[Y.qpos + qa + 2], E[Y.qpos + qa + 3]};
      if (wn >= MINVALF) {
        float sn, cs;
        sincosf(0.5f * ang, &sn, &cs);
        float inv = sn / wn, r[4] = {cs, w[0] * inv, w[1] * inv, w[2] * inv}, o[4];
        o[0] = q[0] * r[0] - q[1] * r[1] - q[2] * r[2] - q[3] * r[3];
        o[1] = q[0] * r[1] + q[1] * r[0] + q[2] * r[3] - q[3] * r[2];
        o[2] = q[0] * r[2] - q[1] * r[3] + q[2] * r[0] + q[3] * r[1];
        o[3] = q[0] * r[3] + q[1] * r[2] - q[2] * r[1] + q[3] * r[0];
        float on = 1.0f / sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
        E[Y.qpos + qa] = o[0] * on; E[Y.qpos + qa + 1] = o[1] * on; E[Y.qpos + qa + 2] = o[2] * on; E[Y.qpos + qa + 3] = o[3] * on;
      }
    }
  }
  time = uniformf(time + h);
}

#endif  // MYO_WAVE_MOTION_H
