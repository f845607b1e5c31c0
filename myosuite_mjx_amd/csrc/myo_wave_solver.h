// myo_wave_solver.h -- stages of the wave kernel: constraint rows, Newton / Euler solver, sensor readout, per-task epilogue
// Part of the single translation unit myo_hip.hip (included by myo_kernel_wave.h); not a stand-alone header.
#ifndef MYO_WAVE_SOLVER_H
#define MYO_WAVE_SOLVER_H

// Joint-limit rows (lane = dof).
// LDS: reads qpos, qvel; writes nothing.
template <class C, class LY> __device__ __forceinline__ LimRow w_limit_rows(const WaveCtx<LY>& X, int lane) {
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[];
  const int nv = X.nv;
  LimRow lim{0.f, 0.f, 0.f};
  if (lane < nv && !M.disable_limit) {
    const float* J = M.jl + 12 * lane;
    if (J[0] != 0) {
      float q = E[Y.qpos + W.dof_qposadr[lane]], margin = J[3];
      float dlo = q - J[1], dhi = J[2] - q, dist = 0;
      if (dlo < margin && dlo <= dhi) { lim.sign = 1; dist = dlo; }
      else if (dhi < margin) { lim.sign = -1; dist = dhi; }
      if (lim.sign != 0) {
        float imp = impedance(J + 6, dist, margin), K, B;
        float R = fmaxf(MINVALF, (1 - imp) / imp * J[11]);
        kbi(J[4], J[5], J[7], M.timestep, &K, &B);
        lim.aref = -B * (lim.sign * E[Y.qvel + lane]) - K * imp * (dist - margin);
        lim.D = __builtin_amdgcn_rcpf(R);
      }
    }
  }
  return lim;
}

// Contact rows: jacobians with lane = (contact of the pass, dof slot), then the row constants with lane = contact; TRK: friction-loss rows
// (lane = dof).  Returns the efc row count (limit rows included) as MuJoCo reports it.
// LDS: reads cdist, cpos, cnrm, cpair (overflow rows for contacts >= NC), axis, anchor, qvel, gax; writes cJ and cdofs (overflow rows: O_CJ,
// O_CDW; second-bank contacts also their state block).  Scratch: KC == 20 sums a contact's row velocities in xv[0..11] (the solver's search
// vector, dead here).
template <class C, class LY> __device__ __forceinline__ int w_contact_rows(const WaveCtx<LY>& X, int lane, int ncon, const LimRow& lim, ConConst<C::NR>& con, FricLoss& fl, bool& bank1, bool& b1lane) {
  constexpr int KC = C::KC, NR = C::NR;
  constexpr bool TRK = C::TRK, FULL = C::FULL;
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; float* const ovf_env = X.ovf_env;
  const int nv = X.nv, ovf_row = X.ovf_row;
  con = ConConst<NR>{};   // (TRK: mut = torsional coefficient, D2 = weight of the two torsional rows, 0 for a condim-3 contact)
  // TRK, more than 64 contacts: the second bank (WaveCfg: state block S_* at offset ROWS of the contact's overflow row)
  bank1 = TRK && ncon > 64;
  b1lane = bank1 && lane + 64 < ncon;   // this lane also owns a bank-1 contact
  int nefc_b1 = 0;
  if constexpr (KC == 8 && !FULL && !TRK) {
    // hand / finger kernels: jacobians with lane = (contact of the pass, dof slot), eight contacts per pass -- each lane one column of the
    // three rows (normal, two tangents) instead of one lane walking its contact's eight dofs -- then the row constants with lane = contact
    float vn_c = 0.f, vt1_c = 0.f, vt2_c = 0.f;
    const int rg = lane >> 3, rk = lane & 7;
    for (int c0 = 0; c0 < ncon; c0 += 8) {
      const int c = c0 + rg;
      float pv0 = 0.f, pv1 = 0.f, pv2 = 0.f;
      auto row_cols = [&](const ConRow& R) {
        const float *ppos = R.pos, *pnrm = R.nrm;
        float* const cJ = R.cJ;
        unsigned int* const cdw = R.cdw;
        const int cw_ = R.pair[0];
        const int P[4] = {0, 0, (int)((unsigned int)cw_ >> 16), (cw_ >> 11) & 31};      // dof-list start and length travel with the contact: no pair-table read here
        const float n[3] = {pnrm[0], pnrm[1], pnrm[2]}, cp[3] = {ppos[0], ppos[1], ppos[2]};
        float t1[3], t2[3];
        make_frame(n, t1, t2);
        float jn = 0.f, j1 = 0.f, j2 = 0.f;
        int d = 0;
        if (rk < P[3]) {
          const int de_ = W.pair_dl_pk[P[2] + rk];   // dof | hinge << 7 | sign << 8
          d = de_ & 127;
          const float sg = (float)(de_ >> 8);
          const float* ax = E + Y.axis + 3 * d;
          float col[3];
          if (de_ & 128) {
            const float r[3] = {cp[0] - E[Y.anchor + 3 * d], cp[1] - E[Y.anchor + 3 * d + 1], cp[2] - E[Y.anchor + 3 * d + 2]};
            cross3(col, ax, r);
          } else { col[0] = ax[0]; col[1] = ax[1]; col[2] = ax[2]; }
          jn = sg * dot3(n, col); j1 = sg * dot3(t1, col); j2 = sg * dot3(t2, col);
          const float qv = E[Y.qvel + d];
          pv0 = jn * qv; pv1 = j1 * qv; pv2 = j2 * qv;
        }
        cJ[rk] = jn; cJ[KC + rk] = j1; cJ[2 * KC + rk] = j2;
        ((unsigned char*)cdw)[rk] = (unsigned char)d;   // padded entries: zero jacobian, dof 0
      };
      if (c < ncon) con_row<C>(Y, E, ovf_env, ovf_row, c, row_cols);
#pragma unroll
      for (int m_ = 1; m_ < 8; m_ <<= 1) { pv0 += __shfl_xor(pv0, m_); pv1 += __shfl_xor(pv1, m_); pv2 += __shfl_xor(pv2, m_); }
      const int src = (8 * (lane - c0)) & 63;      // lane = contact c0 + j takes the sums of group j
      const float a0 = __shfl(pv0, src), a1 = __shfl(pv1, src), a2 = __shfl(pv2, src);
      if (lane >= c0 && lane < c0 + 8) { vn_c = a0; vt1_c = a1; vt2_c = a2; }
    }
    SYNC();
    if (lane < ncon) {
      int cw_ = 0;
      float dist = 0.f;
      con_row<C>(Y, E, ovf_env, ovf_row, lane, [&](const ConRow& R) { cw_ = R.pair[0]; dist = R.dist[0]; });
      const int p = cw_ & 2047;
      const float* F = M.pair_f + 12 * p;
      con.kc = (cw_ >> 11) & 31;
      const float incl = F[0] - F[1];
      con.mu = F[2];
      float imp = impedance(F + 6, dist, incl), K, B;
      kbi(F[4], F[5], F[7], M.timestep, &K, &B);
      const float R0 = fmaxf(MINVALF, (1 - imp) / imp * F[3] * (1 + con.mu * con.mu));
      con.D = __builtin_amdgcn_rcpf(fmaxf(MINVALF, 2 * con.mu * con.mu * R0));
      const float pos = -K * imp * (dist - incl);
      con.aref[0] = -B * (vn_c + con.mu * vt1_c) + pos; con.aref[1] = -B * (vn_c - con.mu * vt1_c) + pos;
      con.aref[2] = -B * (vn_c + con.mu * vt2_c) + pos; con.aref[3] = -B * (vn_c - con.mu * vt2_c) + pos;
    }
  } else if constexpr (KC == 20) {
    // 36-dof kernels: the same idea with three contacts per pass (lane = (contact of the pass, one of its 20 dof slots)); the three or four
    // velocity sums of a contact meet in LDS atomics on the (still unused) search-vector scratch
    const int rg = lane / KC, rk = lane - rg * KC;
    float vn_c = 0.f, vt1_c = 0.f, vt2_c = 0.f, vs_c = 0.f;
    float vn_1 = 0.f, vt1_1 = 0.f, vt2_1 = 0.f, vs_1 = 0.f;   // (TRK: the lane's bank-1 contact)
    for (int c0 = 0; c0 < ncon; c0 += 3) {
      if (lane < 12) E[Y.xv + lane] = 0.f;
      SYNC();
      const int c = c0 + rg;
      auto row_cols = [&](const ConRow& R) {
        const float *ppos = R.pos, *pnrm = R.nrm;
        float* const cJ = R.cJ;
        unsigned int* const cdw = R.cdw;
        const int cw_ = R.pair[0];
        const float4 pq0_ = W.pair_rec[4 * (size_t)(cw_ & 2047)]; const int pw_ = __float_as_int(pq0_.x); const int P[6] = {pw_ & 255, (pw_ >> 8) & 255, (int)((unsigned int)cw_ >> 16), (cw_ >> 11) & 31, (pw_ >> 16) & 15, (pw_ >> 20) & 15};
        const float n[3] = {pnrm[0], pnrm[1], pnrm[2]}, cp[3] = {ppos[0], ppos[1], ppos[2]};
        float t1[3], t2[3];
        make_frame(n, t1, t2);
        if (P[4] == 2) {   // plane - capsule: first tangent along the capsule axis (MuJoCo's frame for this pair type)
          const float* ax = E + Y.gax + 3 * P[1];
          float t = dot3(ax, n), y[3] = {ax[0] - t * n[0], ax[1] - t * n[1], ax[2] - t * n[2]};
          float yn = norm3(y);
          if (yn >= 0.5f) {
            float inv = 1.0f / yn;
            t1[0] = y[0] * inv; t1[1] = y[1] * inv; t1[2] = y[2] * inv;
            cross3(t2, n, t1);
          }
        }
        float jn = 0.f, j1 = 0.f, j2 = 0.f, js = 0.f;
        int d = 0;
        if (rk < P[3]) {
          const int de_ = W.pair_dl_pk[P[2] + rk];   // dof | hinge << 7 | sign << 8
          d = de_ & 127;
          const float sg = (float)(de_ >> 8);
          const float* ax = E + Y.axis + 3 * d;
          float col[3];
          const bool hinge = (de_ & 128) != 0;
          if (hinge) {
            const float r[3] = {cp[0] - E[Y.anchor + 3 * d], cp[1] - E[Y.anchor + 3 * d + 1], cp[2] - E[Y.anchor + 3 * d + 2]};
            cross3(col, ax, r);
          } else { col[0] = ax[0]; col[1] = ax[1]; col[2] = ax[2]; }
          jn = sg * dot3(n, col); j1 = sg * dot3(t1, col); j2 = sg * dot3(t2, col);
          const float qv = E[Y.qvel + d];
          atomicAdd(&E[Y.xv + 4 * rg], jn * qv); atomicAdd(&E[Y.xv + 4 * rg + 1], j1 * qv); atomicAdd(&E[Y.xv + 4 * rg + 2], j2 * qv);
          if constexpr (TRK) { js = hinge ? sg * dot3(n, ax) : 0.f; atomicAdd(&E[Y.xv + 4 * rg + 3], js * qv); }   // relative angular velocity about the normal
        }
        cJ[rk] = jn; cJ[KC + rk] = j1; cJ[2 * KC + rk] = j2;
        if constexpr (TRK) cJ[3 * KC + rk] = js;
        ((unsigned char*)cdw)[rk] = (unsigned char)d;   // padded entries: zero jacobian, dof 0
      };
      if (rg < 3 && c < ncon) con_row<C>(Y, E, ovf_env, ovf_row, c, row_cols);
      SYNC();
      if (lane >= c0 && lane < c0 + 3) { const int g = lane - c0; vn_c = E[Y.xv + 4 * g]; vt1_c = E[Y.xv + 4 * g + 1]; vt2_c = E[Y.xv + 4 * g + 2]; vs_c = E[Y.xv + 4 * g + 3]; }
      if constexpr (TRK) {
        if (b1lane && lane + 64 >= c0 && lane + 64 < c0 + 3) { const int g = lane + 64 - c0; vn_1 = E[Y.xv + 4 * g]; vt1_1 = E[Y.xv + 4 * g + 1]; vt2_1 = E[Y.xv + 4 * g + 2]; vs_1 = E[Y.xv + 4 * g + 3]; }
      }
      SYNC();
    }
    // row constants of contact c from its velocity sums (lane = contact & 63)
    auto row_consts = [&](const int cc, const float vn_c, const float vt1_c, const float vt2_c, const float vs_c, float (&caref)[NR], float& cD, float& cmu, float& cmut,
                          float& cD2, int& ckc) {
      const int lane = cc;     // (the body below is the one-bank code: it indexes the contact tables with `lane`)
      int cw_ = 0;
      float dist = 0.f;
      con_row<C>(Y, E, ovf_env, ovf_row, lane, [&](const ConRow& R) { cw_ = R.pair[0]; dist = R.dist[0]; });
      const int p = cw_ & 2047;
      const float4 pq0_ = W.pair_rec[4 * (size_t)(p)]; const int pw_ = __float_as_int(pq0_.x); const int P[6] = {pw_ & 255, (pw_ >> 8) & 255, __float_as_int(pq0_.w), (pw_ >> 24) & 255, (pw_ >> 16) & 15, (pw_ >> 20) & 15};
      const float* F = M.pair_f + 12 * p;
      ckc = P[3];
      const float incl = F[0] - F[1];
      cmu = F[2];
      float tors = 0.f;
      if constexpr (C::OBJ) {   // per-env friction of the selected geoms (DevBatch.objk): the pair's sliding and torsional coefficients mixed again
        tors = F[11];
        if (X.Bt.objk) obj_pair_friction(X.Bt, X.env, P[0], P[1], cmu, tors);
      }
      float imp = impedance(F + 6, dist, incl), K, B;
      kbi(F[4], F[5], F[7], M.timestep, &K, &B);
      if (P[5] == 1) {
        // condim 1 (explicit <pair>): one frictionless row = four identical "pyramid" rows with mu = 0 and D/4 each
        cmu = 0.f;
        cD = 0.25f / fmaxf(MINVALF, (1 - imp) / imp * F[3]);
      } else {
        float R0 = fmaxf(MINVALF, (1 - imp) / imp * F[3] * (1 + cmu * cmu));
        cD = __builtin_amdgcn_rcpf(fmaxf(MINVALF, 2 * cmu * cmu * R0));
      }
      const float pos = -K * imp * (dist - incl);
      caref[0] = -B * (vn_c + cmu * vt1_c) + pos; caref[1] = -B * (vn_c - cmu * vt1_c) + pos;
      caref[2] = -B * (vn_c + cmu * vt2_c) + pos; caref[3] = -B * (vn_c - cmu * vt2_c) + pos;
      if constexpr (TRK) {
        if (P[5] == 4) { cmut = C::OBJ ? tors : F[11]; cD2 = cD; caref[4] = -B * (vn_c + cmut * vs_c) + pos; caref[5] = -B * (vn_c - cmut * vs_c) + pos; }
      }
    };
    if (lane < ncon) row_consts(lane, vn_c, vt1_c, vt2_c, vs_c, con.aref, con.D, con.mu, con.mut, con.D2, con.kc);
    if constexpr (TRK) {
      float a1[NR], D1 = 0.f, mu1 = 0.f, mut1 = 0.f, D21 = 0.f;
      int kc1 = 0;
#pragma unroll
      for (int k = 0; k < NR; k++) a1[k] = 0.f;
      if (b1lane) {
        row_consts(lane + 64, vn_1, vt1_1, vt2_1, vs_1, a1, D1, mu1, mut1, D21, kc1);
        float* S = bank1_state<C>(ovf_env, ovf_row, lane + 64);
#pragma unroll
        for (int k = 0; k < NR; k++) S[C::S_AREF + k] = a1[k];
        S[C::S_D] = D1; S[C::S_MU] = mu1; S[C::S_MUT] = mut1; S[C::S_D2] = D21; ((int*)S)[C::S_KC] = kc1; ((int*)S)[C::S_SIG] = -1;
      }
      if (bank1) nefc_b1 = 2 * __popcll(__ballot(b1lane && D21 != 0.f)) - 3 * __popcll(__ballot(b1lane && mu1 == 0.f));
    }
  } else static_assert(KC == 20, "an instantiation is (KC == 8 && !FULL && !TRK) or KC == 20: a third shape would silently get no contact rows");
  // efc row count as MuJoCo reports it: 4 pyramid rows per condim-3 contact, 1 per frictionless (condim-1) contact
  int nefc = __popcll(__ballot(lim.sign != 0.f)) + 4 * ncon - 3 * __popcll(__ballot(lane < ncon && con.mu == 0.f));
  // TRK: friction-loss rows (mj_instantiateFriction): lane = dof, J = e_dof, aref = -B qvel; force saturates at +-f outside |jar| < f / D
  fl = FricLoss{0.f, 0.f, 0.f, 0.f};
  if constexpr (TRK) {
    nefc += 2 * __popcll(__ballot(lane < ncon && con.D2 != 0.f));
    nefc += nefc_b1;
    if (lane < nv) {
      const float* FL = W.fl + 4 * lane;
      fl.f = FL[0];
      if (fl.f > 0.f) { fl.D = FL[1]; fl.aref = -FL[2] * E[Y.qvel + lane]; fl.rf = fl.f / fl.D; }
    }
    nefc += __popcll(__ballot(fl.f > 0.f));
  }
  return nefc;
}

// Tendon-limit rows (models with tendon limits only): each active one becomes a pseudo-contact in the lanes after the real contacts; ncon and
// nefc grow by their number.
// LDS: reads tJp; writes cJ, cdofs of the new slots, and uses their cdist / cpos words (overflow rows: O_DIST, O_POS) to hand aref, D and the
// dof count from lane = tendon to lane = slot.
template <class C, class LY> __device__ __forceinline__ void w_tendon_limit_rows(const WaveCtx<LY>& X, int lane, ConConst<C::NR>& con, int& ncon, int& nefc, int& flags) {
  constexpr int KC = C::KC, NC = C::NC, NTR = C::NTR, CDW = C::CDW, NJ = C::NJ;
  constexpr bool TRK = C::TRK;
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; float* const ovf_env = X.ovf_env;
  const int maxnnz_ = X.maxnnz_, ngt_ = X.ngt_, ovf_row = X.ovf_row, nct = X.nct;
  const bool has_tl = X.has_tl;
  // an active tendon limit becomes a frictionless pseudo-contact: jacobian = +-(sparse tendon row), mu = 0 and D/4 on each
  // of the four identical "pyramid" rows, which together act exactly like the single MuJoCo limit row
  int nt = ncon;
#pragma unroll
  for (int rr = 0; rr < NTR; rr++) {
  const int gt = lane + 64 * rr;
  bool tact = false;
  float t_aref = 0.f, t_D = 0.f, t_sign = 0.f;
  if (gt < ngt_ && !M.disable_limit) {
    const float* T = W.tl + 12 * gt;
    if (T[0] != 0) {
      const float tl_len = E[Y.tJp + ngt_ * maxnnz_ + gt], tl_vel = E[Y.tJp + ngt_ * maxnnz_ + ngt_ + gt];   // (LDS copies: not live in registers across collision)
      float margin = T[3], dlo = tl_len - T[1], dhi = T[2] - tl_len, dist = 0;
      if (dlo < margin && dlo <= dhi) { t_sign = 1; dist = dlo; }
      else if (dhi < margin) { t_sign = -1; dist = dhi; }
      if (t_sign != 0) {
        float imp = impedance(T + 6, dist, margin), K, B;
        float R = fmaxf(MINVALF, (1 - imp) / imp * T[11]);
        kbi(T[4], T[5], T[7], M.timestep, &K, &B);
        t_aref = -B * (t_sign * tl_vel) - K * imp * (dist - margin);
        t_D = 1.0f / R;
        tact = true;
      }
    }
  }
  unsigned long long bal = __ballot(tact);
  int slot = nt + __popcll(bal & ((1ull << lane) - 1ull));
  const int ntcap = min(nct, 64);     // tendon-limit rows share the 64 lanes with the contacts; slots beyond the LDS table live in the overflow rows like contacts
  if (tact && slot < ntcap) {
    float* const row = slot < NC ? nullptr : ovf_env + (slot - NC) * ovf_row;
    float* cJ = slot < NC ? E + Y.cJ + slot * NJ * KC : row + C::O_CJ;
    unsigned int dpk[CDW];
#pragma unroll
    for (int k = 0; k < CDW; k++) dpk[k] = 0;
    int kc = 0;
#pragma unroll
    for (int k = 0; k < KC; k++) {
      int d = k < maxnnz_ ? M.gt_dofs[gt * maxnnz_ + k] : -1;
      float jv = d >= 0 ? t_sign * E[Y.tJp + gt * maxnnz_ + k] : 0.f;
      if (d >= 0) kc = k + 1; else d = 0;
      cJ[k] = jv; cJ[KC + k] = 0.f; cJ[2 * KC + k] = 0.f;
      if constexpr (TRK) cJ[3 * KC + k] = 0.f;
      dpk[k >> 2] |= (unsigned int)d << (8 * (k & 3));
    }
    unsigned int* const dw = slot < NC ? (unsigned int*)(E + Y.cdofs) + CDW * slot : (unsigned int*)(row + C::O_CDW);
#pragma unroll
    for (int k = 0; k < CDW; k++) dw[k] = dpk[k];
    if (slot < NC) { E[Y.cdist + slot] = t_aref; E[Y.cpos + 3 * slot] = t_D; E[Y.cpos + 3 * slot + 1] = (float)kc; }
    else { row[C::O_DIST] = t_aref; row[C::O_POS] = t_D; row[C::O_POS + 1] = (float)kc; }   // (the same fields as the LDS branch)
  }
  nt += __popcll(bal);
  }
  // only a tendon-limit row that found no slot is a loss (a has_tl model with more than NC contacts used to be cut back to NC
  // and flagged even when no tendon limit was active)
  if (nt > min(nct, 64)) { flags |= MYO_FLAG_CONTACT_OVERFLOW; nt = min(nct, 64); }
  SYNC();
  if (lane >= ncon && lane < nt) {
    const float* const row = lane < NC ? nullptr : ovf_env + (lane - NC) * ovf_row;
    const float a = lane < NC ? E[Y.cdist + lane] : row[C::O_DIST];
    con.aref[0] = con.aref[1] = con.aref[2] = con.aref[3] = a;   // (TRK: con.D2 stays 0 for these rows)
    con.D = 0.25f * (lane < NC ? E[Y.cpos + 3 * lane] : row[C::O_POS]); con.mu = 0.f; con.kc = (int)(lane < NC ? E[Y.cpos + 3 * lane + 1] : row[C::O_POS + 1]);
  }
  nefc += nt - ncon;
  ncon = nt;
}

// Joint-coupling equalities q1 - q1_0 = poly(q2 - q2_0) (mj_instantiateEquality, mjEQ_JOINT): lane = equality, two jacobian entries
// (+1 at dof 1, -poly' at dof 2), always active (quadratic cost on both sides).
// LDS: reads qpos, qvel; writes nothing.
template <class C, class LY> __device__ __forceinline__ EqRow w_equality_rows(const WaveCtx<LY>& X, int lane) {
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[];
  const int neq = X.neq;
  EqRow eq{0.f, 0.f, 0.f, 0, 0, lane < neq};
  if (eq.act) {
    const int* Q = W.eq_i + 4 * lane;
    const float* F = W.eq_f + 16 * lane;
    eq.d1 = Q[0]; eq.d2 = Q[1];
    float x = E[Y.qpos + Q[3]] - F[6];
    float pos = E[Y.qpos + Q[2]] - F[5] - (F[0] + x * (F[1] + x * (F[2] + x * (F[3] + x * F[4]))));
    eq.J2 = -(F[1] + x * (2 * F[2] + x * (3 * F[3] + x * 4 * F[4])));
    float vel = E[Y.qvel + eq.d1] + eq.J2 * E[Y.qvel + eq.d2];
    float imp = impedance(F + 9, pos, 0.f), K, B;
    kbi(F[7], F[8], F[10], M.timestep, &K, &B);
    eq.aref = -B * vel - K * imp * pos;
    eq.D = __builtin_amdgcn_rcpf(fmaxf(MINVALF, (1 - imp) / imp * F[14]));
  }
  return eq;
}

// Packed copy of the mass matrix.
// the mass matrix moves from the square buffer (about to be reused for the Hessian) to a packed copy that
// aliases the now dead broad-phase scratch
// ... and this lane's full (symmetric) row stays in registers for the solver: M * x is then NVT broadcast-multiply-adds with no LDS read or
// address arithmetic (twice and a half per substep), and the Newton rows H = M + J^T D J start from it
// (36-dof instantiations only: they run two waves per SIMD on a 256-register budget.  In the 24-dof kernels, at four waves per SIMD, the 24 extra
// live registers spill -- 23 in the headline kernel -- so those keep reading the packed copy.)
// (MROW: with the kernel's constants)
// LDS: reads sq = M; writes Mp (packed lower triangle), which aliases gpos / gax / cand -- dead since the row stage.  sq stays as it is: the first
// Newton refactor of the 24-dof kernels builds H on it (MHL_A).
template <class C, class LY> __device__ __forceinline__ void w_pack_mass(const WaveCtx<LY>& X, int lane, float (&mrow)[C::MROW ? C::NVT : 1]) {
  constexpr int NVT = C::NVT;
  constexpr bool MROW = C::MROW, MHL_B = C::MHL_B;
  const LY& Y = X.Y; extern __shared__ __align__(16) float E[];
  const int nv = X.nv;
  SYNC();
  if constexpr (MROW) {
    const int ml = lane < nv ? lane : 0;
#pragma unroll
    for (int k = 0; k < NVT; k++) mrow[k] = lane < nv ? E[Y.sq + ml * (NVT + 1) + k] : 0.f;
  }
  if constexpr (MHL_B) {      // the whole wave moves the triangle: 2 x 5 LDS instructions for 24 dofs where lane = row takes 2 x 24
#pragma unroll
    for (int i0 = 0; i0 < TRI_N<NVT>; i0 += 64) {
      int d, k;
      tri_pair<NVT>(i0 + lane, d, k);
      if (i0 + lane < TRI_N<NVT> && d < nv) E[Y.Mp + (d * (d + 1)) / 2 + k] = E[Y.sq + d * (NVT + 1) + k];
    }
  } else if (lane < nv) {
    const int based = (lane * (lane + 1)) / 2;
#pragma unroll
    for (int k = 0; k < NVT; k++) if (k <= lane) E[Y.Mp + based + k] = E[Y.sq + lane * (NVT + 1) + k];
  }
  SYNC();
}

// Touch sensors and contact forces (DevBatch.sens), read out of the solve that has just finished.
// lane = contact: the pyramid forces of the final iterate are -cD * cjar on the active rows, exactly what the last J^T f used; the contact
// frame is rebuilt as the row stage built it.  A touch sensor counts a contact by MuJoCo's rule (mj_computeSensor): one of
// its geoms on the sensor's body, a positive normal force, and the ray from the contact point along the normal (reversed when the
// sensor's body is geom 2's) meeting the site volume.  The 24-dof, TRK and RK4 instantiations have no such code.
// LDS: reads cpos, cnrm, cpair (overflow rows for contacts >= NC), lpos, lmat; writes nothing.
template <class C, class LY> __device__ __forceinline__ void w_touch_sensors(const WaveCtx<LY>& X, int lane, int ncon_real, const ConConst<C::NR>& con, const float (&cjar)[C::NR]) {
  const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; const DevBatch& Bt = X.Bt; float* const ovf_env = X.ovf_env;
  const int env = X.env, ovf_row = X.ovf_row;
  const int nts = Bt.ntouch;
  float fn = 0.f, Fw[3] = {0.f, 0.f, 0.f}, cp[3] = {0.f, 0.f, 0.f}, cn[3] = {0.f, 0.f, 1.f};
  int cb1 = -1, cb2 = -1;
  if (lane < ncon_real) {   // (lanes beyond the contacts -- tendon-limit rows included -- contribute exact zeros, whatever their registers hold)
    int cw_ = 0;
    con_row<C>(Y, E, ovf_env, ovf_row, lane, [&](const ConRow& R) {
      cw_ = R.pair[0];
#pragma unroll
      for (int k = 0; k < 3; k++) { cp[k] = R.pos[k]; cn[k] = R.nrm[k]; }
    });
    const int pw_ = __float_as_int(W.pair_rec[4 * (size_t)(cw_ & 2047)].x);
    const int g1 = pw_ & 255, g2 = (pw_ >> 8) & 255;
    float t1[3], t2[3];
    make_frame(cn, t1, t2);
    if (((pw_ >> 16) & 15) == 2) {   // plane - capsule: first tangent along the capsule axis, as in the row stage (its gax table is gone by now)
      float R[9];
      geom_world_mat(W, Y, E, g2, R);
      const float ax[3] = {R[2], R[5], R[8]};
      float t = dot3(ax, cn), y[3] = {ax[0] - t * cn[0], ax[1] - t * cn[1], ax[2] - t * cn[2]};
      float yn = norm3(y);
      if (yn >= 0.5f) {
        float inv = 1.0f / yn;
        t1[0] = y[0] * inv; t1[1] = y[1] * inv; t1[2] = y[2] * inv;
        cross3(t2, cn, t1);
      }
    }
    const float f0 = fmaxf(0.f, -con.D * cjar[0]), f1 = fmaxf(0.f, -con.D * cjar[1]), f2 = fmaxf(0.f, -con.D * cjar[2]), f3 = fmaxf(0.f, -con.D * cjar[3]);
    fn = f0 + f1 + f2 + f3;
    const float a1 = con.mu * (f0 - f1), a2 = con.mu * (f2 - f3);
    // the force acts on geom 2's body and its opposite on geom 1's: what reaches the model from outside is the force of a contact whose
    // other geom is world-fixed; a contact between two moving geoms is internal and adds nothing
    const float sg = __float_as_int(W.cg_rec[4 * g1].x) < 0 ? 1.f : (__float_as_int(W.cg_rec[4 * g2].x) < 0 ? -1.f : 0.f);
#pragma unroll
    for (int k = 0; k < 3; k++) Fw[k] = sg * (fn * cn[k] + a1 * t1[k] + a2 * t2[k]);
    cb1 = W.cg_body[g1]; cb2 = W.cg_body[g2];
  }
  float* const srow = Bt.sens + (size_t)env * nts;
  float* const crow = Bt.cfrc + (size_t)env * 3 * (nts + 1);
  // (an env reset in this launch never gets here: w_reset_bad wrote its zeros, like mj_resetData)
  for (int s = 0; s < nts; s++) {
    const gpf T = W.touch + TOUCHR * s;
    const int sl = __float_as_int(T[0]), sty = __float_as_int(T[13]), sb = __float_as_int(T[17]);
    const float sgn = cb2 == sb ? -1.f : 1.f;
    float x[3] = {cp[0], cp[1], cp[2]}, r[3] = {sgn * cn[0], sgn * cn[1], sgn * cn[2]};
    if (sl >= 0) {   // into the link frame of the last position stage (wave-uniform branch)
      const float* P = E + Y.lpos + 3 * sl;
      const float* R = E + Y.lmat + 9 * sl;
      x[0] -= P[0]; x[1] -= P[1]; x[2] -= P[2];
      matTvec(x, R, x);
      matTvec(r, R, r);
    }
    const float sm[9] = {T[4], T[5], T[6], T[7], T[8], T[9], T[10], T[11], T[12]}, sz[3] = {T[14], T[15], T[16]};
    x[0] -= T[1]; x[1] -= T[2]; x[2] -= T[3];
    float p[3], d[3];
    matTvec(p, sm, x);
    matTvec(d, sm, r);
    bool meets;
    if (sty == GEOM_SPHERE) {
      const float bq = dot3(p, d), det = bq * bq - (dot3(p, p) - sz[0] * sz[0]);
      meets = det >= 0.f && sqrtf(fmaxf(det, 0.f)) - bq >= 0.f;
    } else {   // box: slab test
      float tmin = 0.f, tmax = 3.0e38f;
      meets = true;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (fabsf(d[k]) < 1e-12f) meets = meets && fabsf(p[k]) <= sz[k];
        else {
          const float inv = 1.0f / d[k], ta = (-sz[k] - p[k]) * inv, tb = (sz[k] - p[k]) * inv;
          tmin = fmaxf(tmin, fminf(ta, tb)); tmax = fminf(tmax, fmaxf(ta, tb));
        }
      }
      meets = meets && tmax >= tmin;
    }
    const bool counts = fn > 0.f && (cb1 == sb || cb2 == sb) && meets;
    const float S = wave_sum(counts ? fn : 0.f), Sx = wave_sum(counts ? Fw[0] : 0.f), Sy = wave_sum(counts ? Fw[1] : 0.f), Sz = wave_sum(counts ? Fw[2] : 0.f);
    if (lane == 0) { srow[s] = S; crow[3 * s] = Sx; crow[3 * s + 1] = Sy; crow[3 * s + 2] = Sz; }
  }
  const float Gx = wave_sum(Fw[0]), Gy = wave_sum(Fw[1]), Gz = wave_sum(Fw[2]);
  if (lane == 0) { crow[3 * nts] = Gx; crow[3 * nts + 1] = Gy; crow[3 * nts + 2] = Gz; }
}

// A bad env is reset like mj_resetData (mj_sim_scene.py:56-61), at the substep that finds it bad; the launch runs no further substep of it.
// Its diagnostic rows read zeros: actuator lengths and forces, link frames, touch sensors and contact forces.
// LDS: writes qpos, qvel, act, ctrl.
template <class C, class LY> __device__ __forceinline__ void w_reset_bad(const WaveCtx<LY>& X, float* warm_row, float& time) {
  constexpr bool TRK = C::TRK, RK4 = C::RK4, FULL = C::FULL;
  const DevModel& M = X.M; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; const DevBatch& Bt = X.Bt;
  const int env = X.env, nv = X.nv, nu = X.nu, nq = X.nq;
  SYNC();
  if (lane_id < nq) E[Y.qpos + lane_id] = M.qpos0[lane_id];
  if (lane_id < nv) { E[Y.qvel + lane_id] = 0; warm_row[lane_id] = 0.f; }
  for (int i = lane_id; i < nu; i += 64) {
    E[Y.act + i] = 0; E[Y.ctrl + i] = 0;
    Bt.tenlen[(size_t)env * nu + i] = 0.f; Bt.actforce[(size_t)env * nu + i] = 0.f;
  }
  time = 0;
  if constexpr (TRK) {
    if (Bt.linkx) for (int i = lane_id; i < 12 * X.nl_; i += 64) Bt.linkx[(size_t)env * 12 * X.nl_ + i] = 0.f;
  }
  if constexpr (FULL && !TRK && !RK4) {
    if (Bt.sens) {
      const int nts = Bt.ntouch;
      for (int i = lane_id; i < nts; i += 64) Bt.sens[(size_t)env * nts + i] = 0.f;
      for (int i = lane_id; i < 3 * (nts + 1); i += 64) Bt.cfrc[(size_t)env * 3 * (nts + 1) + i] = 0.f;
    }
  }
  SYNC();
}

// Epilogue of TrackEnv.step (mjx/myodm_v0.py:185-267, 297-304): reward / done / metrics on the stepped state, masked reset, observation.  Returns
// true when the env was reset.
// LDS: reads qpos, qvel, lpos, lmat; a reset writes qpos, qvel, act, ctrl.
template <class C, class LY> __device__ __forceinline__ bool w_track_epilogue(const WaveCtx<LY>& X, float* warm_row, float& time, bool dead) {
  const DevModel& M = X.M; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; const DevBatch& Bt = X.Bt;
  const int env = X.env, nv = X.nv, nu = X.nu, nq = X.nq;
  bool track_reset = false;
  SYNC();
  const DevTrack& K = *Bt.track;
  float done = 1.f;
  // an env that the step found bad (wave-uniform) is an ended episode, with or without `autoreset`: done, no reward, no metrics, and the
  // state of TrackEnv.reset (the MJX reference has no error path; include/myo_hip.h states this one).  No reward is evaluated on the link
  // frames of a faulted substep
  if (dead) {
    if (lane_id == 0) {
      Bt.reward[env] = 0.f; Bt.done[env] = 1.f;
      float* mt = K.metrics + 4 * (size_t)env;
      mt[0] = 0.f; mt[1] = 0.f; mt[2] = 0.f; mt[3] = 0.f;
    }
  } else done = uniformf(track_reward(K, Bt, env, lane_id, E + Y.qpos, E + Y.qvel, E + Y.lpos, E + Y.lmat, M.origin, [](float v) { return wave_sum(v); }));
  const bool trunc = !dead && K.max_steps > 0 && !(done > 0.f) && Bt.elapsed[env] + 1 >= K.max_steps;   // gym TimeLimit of the registered ids
  if (lane_id == 0) Bt.solved[env] = trunc ? 1.f : 0.f;
  if (dead || (K.autoreset && (done > 0.f || trunc))) {   // (wave-uniform) TrackEnv.reset of this env: init_qpos, zero velocity / activation / control / warm start / time
    SYNC();
    if (lane_id < nq) E[Y.qpos + lane_id] = K.init_qpos[lane_id];
    if (lane_id < nv) { E[Y.qvel + lane_id] = 0.f; warm_row[lane_id] = 0.f; }
    for (int i = lane_id; i < nu; i += 64) { E[Y.act + i] = 0.f; E[Y.ctrl + i] = 0.f; }
    time = 0.f;
    track_reset = true;
  }
  SYNC();
  float* o = Bt.obs + (size_t)env * (nq + nv);
  if (lane_id < nq) o[lane_id] = E[Y.qpos + lane_id];
  if (lane_id < nv) o[nq + lane_id] = E[Y.qvel + lane_id];
  return track_reset;
}

#endif  // MYO_WAVE_SOLVER_H
