// myo_wave_collision.h -- stages of the wave kernel: broad phase and narrow phase of the collision
// Part of the single translation unit myo_hip.hip (included by myo_kernel_wave.h); not a stand-alone header.
#ifndef MYO_WAVE_COLLISION_H
#define MYO_WAVE_COLLISION_H

// Broad phase (lane = pair, rounds of 64): bounding tests of every pair; returns the number of candidates.
// LDS: reads lpos, lmat; writes gpos, gax (world centre and long axis of every collision geom; they stay live through the narrow phase and the
// row stage) and cand (candidates beyond NCAND: the env's HBM row ovf_cand).  These three alias the packed mass matrix Mp, which is dead
// here: the solver of the previous substep was its last reader.
template <class C, class LY> __device__ __forceinline__ int w_broad_phase(const WaveCtx<LY>& X, int lane, int& flags, int& f_cand) {
  constexpr bool HF = C::HF, TRK = C::TRK, FULL = C::FULL;
  const DevModel& M = X.M; const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; const DevBatch& Bt = X.Bt; int* const ovf_cand = X.ovf_cand;
  const int env = X.env, ncg_ = X.ncg_, npair_ = X.npair_;
  // TRK: per-env orientation of one world-welded body (MYO_F_BODYQUAT) and per-env centres of the selected geoms (DevBatch.objk), applied
  // wherever a geom frame is built; constant nullptrs elsewhere
  const BodyRot BR = body_rot_of(Bt, env, TRK, C::OBJ);
  const BodyRot* const brp = TRK ? &BR : nullptr;
  int ncand = 0;
  int* cand = (int*)(E + Y.cand);
  PairRaw pnext = pair_raw(W, min(lane, npair_ > 0 ? npair_ - 1 : 0));   // broad phase, round 0: requested here, behind the geom frames
  for (int g = lane; g < ncg_; g += 64) {   // world centre and long axis (3rd column) of every collision geom (more than 64: MyoDM teapot, wineglass)
    float x[3], R[9];
    geom_world_pos(W, Y, E, g, x, brp);
    geom_world_mat(W, Y, E, g, R, brp);
    E[Y.gpos + 3 * g] = x[0]; E[Y.gpos + 3 * g + 1] = x[1]; E[Y.gpos + 3 * g + 2] = x[2];
    E[Y.gax + 3 * g] = R[2]; E[Y.gax + 3 * g + 1] = R[5]; E[Y.gax + 3 * g + 2] = R[8];
  }
  SYNC();
  for (int base = 0; base < npair_; base += 64) {
    int p = base + lane;
    bool hit = false;
    int nh = 0, hr0 = 0, hr1 = 0, hc0 = 0, hc1 = 0;   // height-field pair: cell range under the geom, prisms that can touch it
    float hzcut = 0.f;
    const PairRaw praw = pnext;                                   // this round's record was requested a round ago
    pnext = pair_raw(W, min(p + 64, npair_ > 0 ? npair_ - 1 : 0));   // next round's, in flight while this one is tested
    if (p < npair_) {
      const PairL Q = pair_decode<C>(Bt, env, praw);   // one record: four independent 16-byte loads (was pair_i -> cg_rbound / cg_type / cg_size -> pair_f, word by word)
      const int P[6] = {Q.g1, Q.g2, Q.dl, Q.kc, Q.pt, Q.cd};
      if (HF && P[4] == 4) {
        const int g2 = P[1], ty = Q.t2;
        const float *x2 = E + Y.gpos + 3 * g2, *ax = E + Y.gax + 3 * g2, *sz = Q.s2;
        const float rel[3] = {x2[0] - W.hf.pos[0], x2[1] - W.hf.pos[1], x2[2] - W.hf.pos[2]}, margin = Q.margin;
        float ext[3];
        if (ty == GEOM_ELLIPSOID) {
          float R[9];
          geom_world_mat(W, Y, E, g2, R, brp);
#pragma unroll
          for (int k = 0; k < 3; k++) { const float a = R[3 * k] * sz[0], b = R[3 * k + 1] * sz[1], c = R[3 * k + 2] * sz[2]; ext[k] = sqrtf(a * a + b * b + c * c); }
        } else {
#pragma unroll
          for (int k = 0; k < 3; k++)
            ext[k] = ty == GEOM_SPHERE ? sz[0] : (ty == GEOM_CAPSULE ? sz[0] + sz[1] * fabsf(ax[k]) : sz[1] * fabsf(ax[k]) + sz[0] * sqrtf(fmaxf(0.f, 1.f - ax[k] * ax[k])));
        }
        float zmin;
        if (hf_range(W.hf, rel, ext, Q.rb2, margin, hr0, hr1, hc0, hc1, zmin)) {
          hzcut = zmin - margin;
          nh = hf_walk(W.hf, Bt.hfield + (size_t)env * W.hf.nrow * W.hf.ncol, hr0, hr1, hc0, hc1, hzcut, p, nullptr, 0, 0);
        }
      } else if (!(M.disable_ellipsoid && P[4] == 0)) {
        int g1 = P[0], g2 = P[1];
        const float *x1 = E + Y.gpos + 3 * g1, *x2 = E + Y.gpos + 3 * g2;
        float dif[3] = {x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]};
        float bound = Q.rb1 + Q.rb2 + Q.margin;
        if (FULL && P[4] >= 2) hit = dot3(dif, E + Y.gax + 3 * g1) <= Q.rb2 + Q.margin;   // plane: signed distance of the bounding sphere
        else hit = dot3(dif, dif) <= bound * bound;
        if constexpr (TRK) {
          // a box (table top: bounding sphere 0.7 m) is tested as a box, a hull as the bounding box of its vertices in the mesh frame
          // (lowering.py hip_mesh_aabb: centre | half sizes): distance from the other geom's centre to that box against the other
          // geom's bounding sphere + margin.  The airplane's outer hull has a 0.10 m bounding sphere and thin wings.
          const int t1 = Q.t1, t2 = Q.t2;
          if (hit && P[4] == 5) {   // plane - hull: the lowest corner of the hull's vertex bounding box along the plane normal
            float R2[9], nl[3];
            const float* n = E + Y.gax + 3 * g1;
            geom_world_mat(W, Y, E, g2, R2, brp);
            matTvec(nl, R2, n);
            gpf bx = W.mesh_aabb + 6 * (int)Q.s2[2];
            const float low = dot3(dif, n) + nl[0] * bx[0] + nl[1] * bx[1] + nl[2] * bx[2] - (fabsf(nl[0]) * bx[3] + fabsf(nl[1]) * bx[4] + fabsf(nl[2]) * bx[5]);
            hit = low <= Q.margin;
          }
          if (hit && (t1 >= 6 || t2 >= 6) && P[4] == 0) {
#pragma unroll
            for (int side = 0; side < 2; side++) {
              const int gb = side ? g2 : g1, go = side ? g1 : g2, tb = side ? t2 : t1;
              if (tb < 6 || !hit) continue;
              float Rb[9], cl[3], dd[3] = {E[Y.gpos + 3 * go] - E[Y.gpos + 3 * gb], E[Y.gpos + 3 * go + 1] - E[Y.gpos + 3 * gb + 1], E[Y.gpos + 3 * go + 2] - E[Y.gpos + 3 * gb + 2]};
              geom_world_mat(W, Y, E, gb, Rb, brp);
              matTvec(cl, Rb, dd);
              const float* sb = side ? Q.s2 : Q.s1;
              float hx = sb[0], hy = sb[1], hz = sb[2];
              if (tb == 7) { gpf bx = W.mesh_aabb + 6 * (int)sb[2]; cl[0] -= bx[0]; cl[1] -= bx[1]; cl[2] -= bx[2]; hx = bx[3]; hy = bx[4]; hz = bx[5]; }
              const float ex = fmaxf(fabsf(cl[0]) - hx, 0.f), ey = fmaxf(fabsf(cl[1]) - hy, 0.f), ez = fmaxf(fabsf(cl[2]) - hz, 0.f);
              const float lim = (side ? Q.rb1 : Q.rb2) + Q.margin;
              hit = ex * ex + ey * ey + ez * ez <= lim * lim;
            }
          }
        }
        if (hit && !P[4]) {
          // conservative refinement before the expensive MPR: replace a capsule's bounding sphere by the distance
          // from the other geom's centre to the capsule's SEGMENT (a bound on the true distance, never excludes a contact)
          float b1 = Q.rb1, b2 = Q.rb2;
          float c1[3] = {x1[0], x1[1], x1[2]}, c2[3] = {x2[0], x2[1], x2[2]};
          if (Q.t1 == GEOM_CAPSULE) {
            const float* a = E + Y.gax + 3 * g1;
            float hh = Q.s1[1], t = clipf(dot3(dif, a), -hh, hh);
            c1[0] += t * a[0]; c1[1] += t * a[1]; c1[2] += t * a[2];
            b1 = Q.s1[0];
          }
          if (Q.t2 == GEOM_CAPSULE) {
            const float* a = E + Y.gax + 3 * g2;
            float nd[3] = {c1[0] - x2[0], c1[1] - x2[1], c1[2] - x2[2]};
            float hh = Q.s2[1], t = clipf(dot3(nd, a), -hh, hh);
            c2[0] += t * a[0]; c2[1] += t * a[1]; c2[2] += t * a[2];
            b2 = Q.s2[0];
          }
          float d2[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
          float bb = b1 + b2 + Q.margin;
          hit = dot3(d2, d2) <= bb * bb;
          if (hit) {
            // separating-axis test along the centre line: the two (margin-inflated) convex shapes cannot touch if their
            // support widths along that axis do not reach across the centre distance.  MPR would report "no contact" for
            // exactly these pairs, after a dozen support evaluations; this costs one support width per shape
            float dn = norm3(dif);
            if (dn > MINVALF) {
              float inv = 1.0f / dn, ax[3] = {dif[0] * inv, dif[1] * inv, dif[2] * inv}, wsum = Q.margin;
#pragma unroll
              for (int side = 0; side < 2; side++) {
                const int g = side ? g2 : g1;
                const float* sz = side ? Q.s2 : Q.s1;
                const int ty = side ? Q.t2 : Q.t1;
                if (TRK && ty >= 6) wsum += 1e9f;   // box / hull: no cheap support width here, the pair goes to MPR
                else if (ty == GEOM_CAPSULE) wsum += sz[0] + sz[1] * fabsf(dot3(E + Y.gax + 3 * g, ax));
                else if (ty == GEOM_SPHERE) wsum += sz[0];
                else {
                  float R[9], dl[3];
                  geom_world_mat(W, Y, E, g, R, brp);
                  matTvec(dl, R, ax);
                  if (ty == GEOM_ELLIPSOID) { float sv[3] = {sz[0] * dl[0], sz[1] * dl[1], sz[2] * dl[2]}; wsum += norm3(sv); }
                  else wsum += sz[0] * sqrtf(dl[0] * dl[0] + dl[1] * dl[1]) + sz[1] * fabsf(dl[2]);   // cylinder
                }
              }
              hit = dn <= wsum * 1.0001f + 1e-6f;   // conservative: never excludes a touching pair
            }
          }
        }
      }
    }
    unsigned long long bal = __ballot(hit);
    int pos = ncand + __popcll(bal & ((1ull << lane) - 1ull));
    if (hit) { if (pos < NCAND) cand[pos] = p; else if (ovf_cand && pos < NCAND + NCANDX) ovf_cand[pos - NCAND] = p; }
    ncand += __popcll(bal);
    if (HF) {   // height-field pairs expand into one candidate per prism, appended in pair order
      unsigned long long hb = __ballot(nh > 0);
      int myat = 0;
      while (hb) {
        const int L = __ffsll((long long)hb) - 1;
        hb &= hb - 1ull;
        if (lane == L) myat = ncand;
        ncand += rdlanei(nh, L);
      }
      if (nh > 0) hf_walk(W.hf, Bt.hfield + (size_t)env * W.hf.nrow * W.hf.ncol, hr0, hr1, hc0, hc1, hzcut, p, cand, myat, NCAND);
    }
  }
  { const int candcap = ovf_cand ? NCAND + NCANDX : NCAND; if (ncand > candcap) { flags |= MYO_FLAG_CAND_OVERFLOW; ncand = candcap; } }
  f_cand += ncand;
  SYNC();
  return ncand;
}

// Narrow phase (lane = candidate, rounds of RND): analytic pairs and MPR; returns the number of contacts (capped at nct).
// LDS: reads gpos, gax, cand, lpos, lmat and the MPR warm-start table mprw (n_mprw entries of the previous substep); writes cdist, cpos, cnrm,
// cpair of contacts < NC (the later ones: overflow rows, fields O_DIST .. O_PAIR) and rebuilds mprw.  Scratch: the first 12 * RND words of cJ
// hold the portal witnesses of the MPR (12 per lane); cJ is dead on return, the row stage fills it.
template <class C, class LY> __device__ __forceinline__ int w_narrow_phase(const WaveCtx<LY>& X, int lane, int ncand, int& n_mprw, int& flags, int& f_mpr) {
  constexpr int RND = C::RND;
  constexpr bool HF = C::HF, TRK = C::TRK, FULL = C::FULL;
  const DevModelW& W = X.W; const LY& Y = X.Y; extern __shared__ __align__(16) float E[]; const DevBatch& Bt = X.Bt; float* const ovf_env = X.ovf_env; int* const ovf_cand = X.ovf_cand;
  const int env = X.env, ovf_row = X.ovf_row, nct = X.nct;
  // TRK: per-env orientation of one world-welded body (MYO_F_BODYQUAT) and per-env centres of the selected geoms (DevBatch.objk), applied
  // wherever a geom frame is built; constant nullptrs elsewhere
  const BodyRot BR = body_rot_of(Bt, env, TRK, C::OBJ);
  const BodyRot* const brp = TRK ? &BR : nullptr;
  int* cand = (int*)(E + Y.cand);
  int ncon = 0;
  int n_mprw_new = 0;
  MeshTab MT;   // hull tables of the TRK models (wave-uniform)
  if constexpr (TRK) { MT.vert = W.mesh_vert; MT.rec = (gpf4)W.mesh_rec; MT.srec = (gpf4)W.mesh_startrec; }
  for (int base = 0; base < ncand; base += RND) {
    int ci = (RND == 64 || lane < RND) ? base + lane : ncand;
    int nsup = -8;                    // support evaluations of this lane's MPR refinement (-8: not an MPR pair)
    bool mpr_hit = false;             // this lane's MPR call found a contact: its normal seeds the next substep's call
    float mpr_n[3] = {0.f, 0.f, 0.f};
    bool hit = false, hit2 = false;   // a plane-capsule pair can give two contacts (one per end sphere)
    float dist = 0, dist2 = 0, cpos[3] = {0, 0, 0}, cpos2[3] = {0, 0, 0}, nrm[3] = {1, 0, 0};
    int p = -1, cword = 0;            // cword: what the row stage needs of the pair without another table read (pair | dofs << 11 | dof-list start << 16)
    if (ci < ncand) {
      const int cw = (ci < NCAND) ? cand[ci] : ovf_cand[ci - NCAND];
      p = HF ? (cw & 1023) : cw;
      const PairL Q = pair_load<C>(W, Bt, env, p);
      cword = p | (Q.kc << 11) | (Q.dl << 16);
      const int P[6] = {Q.g1, Q.g2, Q.dl, Q.kc, Q.pt, Q.cd};
      int g1 = P[0], g2 = P[1];
      float margin = Q.margin;
      const float *x1 = E + Y.gpos + 3 * g1, *x2 = E + Y.gpos + 3 * g2;
      const float *sz1 = Q.s1, *sz2 = Q.s2;
      if (P[4] == 1) {
        const float *a1 = E + Y.gax + 3 * g1, *a2 = E + Y.gax + 3 * g2;
        float dif[3] = {x1[0] - x2[0], x1[1] - x2[1], x1[2] - x2[2]};
        float mb = -dot3(a1, a2), u = -dot3(a1, dif), v = dot3(a2, dif), det = 1 - mb * mb, xa, xb;
        if (fabsf(det) >= MINVALF) {
          xa = (u - mb * v) / det;
          xb = (v - mb * u) / det;
          if (xa > sz1[1]) { xa = sz1[1]; xb = v - mb * sz1[1]; }
          else if (xa < -sz1[1]) { xa = -sz1[1]; xb = v + mb * sz1[1]; }
          if (xb > sz2[1]) { xb = sz2[1]; xa = clipf(u - mb * sz2[1], -sz1[1], sz1[1]); }
          else if (xb < -sz2[1]) { xb = -sz2[1]; xa = clipf(u + mb * sz2[1], -sz1[1], sz1[1]); }
        } else {
          xa = clipf(u, -sz1[1], sz1[1]);
          xb = clipf(v - mb * xa, -sz2[1], sz2[1]);
          xa = clipf(u - mb * xb, -sz1[1], sz1[1]);
        }
        float v1[3] = {x1[0] + a1[0] * xa, x1[1] + a1[1] * xa, x1[2] + a1[2] * xa};
        float v2[3] = {x2[0] + a2[0] * xb, x2[1] + a2[1] * xb, x2[2] + a2[2] * xb};
        float dd[3] = {v2[0] - v1[0], v2[1] - v1[1], v2[2] - v1[2]};
        float cd = norm3(dd);
        if (cd <= margin + sz1[0] + sz2[0]) {
          if (cd < MINVALF) { dd[0] = 1; dd[1] = 0; dd[2] = 0; } else { float inv = 1.0f / cd; dd[0] *= inv; dd[1] *= inv; dd[2] *= inv; }
          dist = cd - sz1[0] - sz2[0];
#pragma unroll
          for (int k = 0; k < 3; k++) { cpos[k] = v1[k] + dd[k] * (sz1[0] + 0.5f * dist); nrm[k] = dd[k]; }
          hit = true;
        }
      } else if (FULL && P[4] == 2) {   // plane - capsule (mjc_PlaneCapsule): the two end spheres against the plane
        const float *n = E + Y.gax + 3 * g1, *ax = E + Y.gax + 3 * g2;
        float r = sz2[0], hh = sz2[1];
#pragma unroll
        for (int k = 0; k < 3; k++) nrm[k] = n[k];
        float eA[3] = {x2[0] - hh * ax[0] - x1[0], x2[1] - hh * ax[1] - x1[1], x2[2] - hh * ax[2] - x1[2]};
        float eB[3] = {x2[0] + hh * ax[0] - x1[0], x2[1] + hh * ax[1] - x1[1], x2[2] + hh * ax[2] - x1[2]};
        float dA = dot3(eA, n) - r, dB = dot3(eB, n) - r;
        if (dA <= margin) {
          hit = true; dist = dA;
#pragma unroll
          for (int k = 0; k < 3; k++) cpos[k] = eA[k] + x1[k] - n[k] * (r + 0.5f * dA);
        }
        if (dB <= margin) {
          hit2 = true; dist2 = dB;
#pragma unroll
          for (int k = 0; k < 3; k++) cpos2[k] = eB[k] + x1[k] - n[k] * (r + 0.5f * dB);
        }
      } else if (FULL && TRK && P[4] == 5) {   // plane - convex hull: deepest vertex along -normal (one contact)
        const float* n = E + Y.gax + 3 * g1;
        float R2[9], nl[3], pw[3];
        geom_world_mat(W, Y, E, g2, R2, brp);
        matTvec(nl, R2, n);
        CObj oh;
        cobj_shape_poly(oh, 7, sz2);
        const float dn[3] = {-nl[0], -nl[1], -nl[2]};
        float sp[3];
        support_shape<2>(oh, dn, sp, MT);        // vertex-graph climb (scan for small hulls) instead of a pass over all vertices
        matvec(pw, R2, sp);
        float rel[3] = {x2[0] - x1[0] + pw[0], x2[1] - x1[1] + pw[1], x2[2] - x1[2] + pw[2]};
        float d = dot3(rel, n);
#pragma unroll
        for (int k = 0; k < 3; k++) nrm[k] = n[k];
        if (d <= margin) {
          hit = true; dist = d;
#pragma unroll
          for (int k = 0; k < 3; k++) cpos[k] = x2[k] + pw[k] - n[k] * 0.5f * d;
        }
      } else if (FULL && TRK && (P[4] == 6 || P[4] == 7)) {
        // plane - cylinder (mjc_PlaneCylinder as oracle/myo_oracle.c states it), one pair lowered as two records: 6 gives the deepest rim
        // point and the opposite cap's rim point, 7 the two triangle points at 0.8660254 r on the deep cap; both need the deepest point
        // within the margin
        const float* n = E + Y.gax + 3 * g1;
        const float r = sz2[0];
        float ax[3] = {E[Y.gax + 3 * g2], E[Y.gax + 3 * g2 + 1], E[Y.gax + 3 * g2 + 2]};
        float prjaxis = dot3(n, ax);
        if (prjaxis > 0) { ax[0] = -ax[0]; ax[1] = -ax[1]; ax[2] = -ax[2]; prjaxis = -prjaxis; }
        float vec[3] = {ax[0] * prjaxis - n[0], ax[1] * prjaxis - n[1], ax[2] * prjaxis - n[2]};
        const float len2 = dot3(vec, vec);
        if (len2 >= MINVALF) {
          const float sc = r / sqrtf(len2);
          vec[0] *= sc; vec[1] *= sc; vec[2] *= sc;
        } else {   // axis along the normal: any radius
          float R2[9];
          geom_world_mat(W, Y, E, g2, R2, brp);
          vec[0] = R2[0] * r; vec[1] = R2[3] * r; vec[2] = R2[6] * r;
        }
        const float prjvec = dot3(vec, n);
        ax[0] *= sz2[1]; ax[1] *= sz2[1]; ax[2] *= sz2[1];
        prjaxis *= sz2[1];
        const float rel[3] = {x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]};
        const float dist0 = dot3(rel, n), d1 = dist0 + prjaxis + prjvec;
#pragma unroll
        for (int k = 0; k < 3; k++) nrm[k] = n[k];
        if (d1 <= margin) {
          if (P[4] == 6) {
            const float d2 = dist0 - prjaxis + prjvec;
            hit = true; dist = d1;
#pragma unroll
            for (int k = 0; k < 3; k++) cpos[k] = x2[k] + vec[k] + ax[k] - n[k] * d1 * 0.5f;
            if (d2 <= margin) {
              hit2 = true; dist2 = d2;
#pragma unroll
              for (int k = 0; k < 3; k++) cpos2[k] = x2[k] + vec[k] - ax[k] - n[k] * d2 * 0.5f;
            }
          } else {
            const float d3 = dist0 + prjaxis - 0.5f * prjvec;
            if (d3 <= margin) {
              float v1[3];
              cross3(v1, vec, ax);
              normalize3(v1);
              const float s3 = r * 0.8660254037844386f;
              hit = hit2 = true; dist = dist2 = d3;
#pragma unroll
              for (int k = 0; k < 3; k++) {
                const float c = x2[k] + ax[k] - vec[k] * 0.5f - n[k] * d3 * 0.5f;
                cpos[k] = c + s3 * v1[k]; cpos2[k] = c - s3 * v1[k];
              }
            }
          }
        }
      } else if (FULL && TRK && P[4] == 8) {   // plane - sphere (mjc_PlaneSphere): the sphere's lowest point along -normal (one contact)
        const float* n = E + Y.gax + 3 * g1;
        const float r = sz2[0];
        const float rel[3] = {x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]};
        const float d = dot3(rel, n) - r;
#pragma unroll
        for (int k = 0; k < 3; k++) nrm[k] = n[k];
        if (d <= margin) {
          hit = true; dist = d;
#pragma unroll
          for (int k = 0; k < 3; k++) cpos[k] = x2[k] - n[k] * (r + 0.5f * d);
        }
      } else if (FULL && P[4] == 3) {   // plane - ellipsoid (mjc_PlaneConvex): deepest support point along -normal
        const float* n = E + Y.gax + 3 * g1;
        float R2[9], nl[3], sp[3], pw[3];
        geom_world_mat(W, Y, E, g2, R2, brp);
        matTvec(nl, R2, n);
        float sv[3] = {sz2[0] * nl[0], sz2[1] * nl[1], sz2[2] * nl[2]};
        float nn = norm3(sv), inv = nn > MINVALF ? -1.0f / nn : 0.f;
        sp[0] = sz2[0] * sv[0] * inv; sp[1] = sz2[1] * sv[1] * inv; sp[2] = sz2[2] * sv[2] * inv;
        matvec(pw, R2, sp);
        float rel[3] = {x2[0] - x1[0] + pw[0], x2[1] - x1[1] + pw[1], x2[2] - x1[2] + pw[2]};
        float d = dot3(rel, n);
#pragma unroll
        for (int k = 0; k < 3; k++) nrm[k] = n[k];
        if (d <= margin) {
          hit = true; dist = d;
#pragma unroll
          for (int k = 0; k < 3; k++) cpos[k] = x2[k] + pw[k] - n[k] * 0.5f * d;
        }
      } else {
        if constexpr (HF) {   // height-field kernels: generic convex pairs and prisms share one MPR call site
        const float zero3[3] = {0.f, 0.f, 0.f};
        nsup = 0;
        // MPR in geom1's own frame: obj1 needs no rotation / translation at all (identity frame), obj2 carries the
        // relative pose R1^T R2, R1^T (x2 - x1); normal and position are rotated back afterwards
        float R1[9], cen[3] = {0.f, 0.f, 0.f};   // (cen: prism centroid; dead code unless HF -- nothing extra stays live across the MPR call)
        CObj o1, o2;
        const bool prism = HF && P[4] == 4;
        if (prism) {
          // obj1 = one triangular prism of the height field, about its centroid, in the (axis-aligned) height-field frame
          float hx[3], hy[3], hz[3];
          hf_prism(W.hf, Bt.hfield + (size_t)env * W.hf.nrow * W.hf.ncol, (cw >> 10) & 127, cw >> 17, hx, hy, hz);
          cen[0] = (hx[0] + hx[1] + hx[2]) * (1.f / 3.f); cen[1] = (hy[0] + hy[1] + hy[2]) * (1.f / 3.f); cen[2] = 0.5f * ((hz[0] + hz[1] + hz[2]) * (1.f / 3.f) - W.hf.size[3]);
#pragma unroll
          for (int k = 0; k < 3; k++) { o1.mat[k] = hx[k] - cen[0]; o1.mat[3 + k] = hy[k] - cen[1]; o1.mat[6 + k] = hz[k] - cen[2]; o1.pos[k] = 0.f; }
          o1.S[0] = -W.hf.size[3] - cen[2]; o1.S[1] = o1.S[2] = 0.f; o1.h = -1.f;
#pragma unroll
          for (int k = 0; k < 9; k++) R1[k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
          geom_world_mat(W, Y, E, g2, o2.mat, brp);
#pragma unroll
          for (int k = 0; k < 3; k++) o2.pos[k] = x2[k] - x1[k] - cen[k];
          cobj_shape(o2, Q.t2, sz2);
        } else {
        geom_world_mat(W, Y, E, g1, R1, brp);
        {
          float R2[9], rel[3] = {x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]};
          geom_world_mat(W, Y, E, g2, R2, brp);
#pragma unroll
          for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) o2.mat[3 * i + j] = R1[i] * R2[j] + R1[3 + i] * R2[3 + j] + R1[6 + i] * R2[6 + j];
          matTvec(o2.pos, R1, rel);
        }
#pragma unroll
        for (int k = 0; k < 9; k++) o1.mat[k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) o1.pos[k] = 0.f;
        cobj_shape(o1, Q.t1, sz1); cobj_shape(o2, Q.t2, sz2);
        }
        o1.margin = o2.margin = 0.5f * margin;
        float depth, dir[3], pos[3], nw[3] = {0.f, 0.f, 0.f};
        bool have_nw = false;
        for (int i = 0; i < (prism ? 0 : n_mprw); i++) {   // (prisms are not warm-started: the table is keyed by pair)
          if (((const int*)(E + Y.mprw))[4 * i] == p) { nw[0] = E[Y.mprw + 4 * i + 1]; nw[1] = E[Y.mprw + 4 * i + 2]; nw[2] = E[Y.mprw + 4 * i + 3]; have_nw = true; }
        }
        bool pen;
        if constexpr (HF) pen = mpr_penetration_wl<true>(o1, o2, MPR_TOL, 60, &depth, dir, pos, &nsup, have_nw ? nw : nullptr, E + Y.cJ + 12 * lane);
        else pen = mpr_penetration(o1, o2, MPR_TOL, 60, &depth, dir, pos, &nsup, have_nw ? nw : nullptr);
        if (pen) {
          dist = margin - depth;
          normalize3(dir);
          mpr_hit = !prism; mpr_n[0] = dir[0]; mpr_n[1] = dir[1]; mpr_n[2] = dir[2];
          float dw[3], pw[3];
          matvec(dw, R1, dir);
          matvec(pw, R1, pos);
#pragma unroll
          for (int k = 0; k < 3; k++) { cpos[k] = pw[k] + x1[k] + (prism ? cen[k] : 0.f); nrm[k] = dw[k]; }
          hit = true;
        }
                  } else {   // all other kernels: the code exactly as it was before the height-field variant existed (register allocation of the hand kernel is sensitive to it)
        const float zero3[3] = {0.f, 0.f, 0.f};
        nsup = 0;
        // MPR in geom1's own frame: obj1 needs no rotation / translation at all (identity frame), obj2 carries the
        // relative pose R1^T R2, R1^T (x2 - x1); normal and position are rotated back afterwards
        float R1[9];
        geom_world_mat(W, Y, E, g1, R1, brp);
        CObj o1, o2;
        {
          float R2[9], rel[3] = {x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]};
          geom_world_mat(W, Y, E, g2, R2, brp);
#pragma unroll
          for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) o2.mat[3 * i + j] = R1[i] * R2[j] + R1[3 + i] * R2[3 + j] + R1[6 + i] * R2[6 + j];
          matTvec(o2.pos, R1, rel);
        }
#pragma unroll
        for (int k = 0; k < 9; k++) o1.mat[k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) o1.pos[k] = 0.f;
        if constexpr (TRK) {
          cobj_shape_poly(o1, Q.t1, sz1);
          cobj_shape_poly(o2, Q.t2, sz2);
        }
        else { cobj_shape(o1, Q.t1, sz1); cobj_shape(o2, Q.t2, sz2); }
        o1.margin = o2.margin = 0.5f * margin;
        float depth, dir[3], pos[3], nw[3] = {0.f, 0.f, 0.f};
        bool have_nw = false;
        for (int i = 0; i < n_mprw; i++) {
          if (((const int*)(E + Y.mprw))[4 * i] == p) { nw[0] = E[Y.mprw + 4 * i + 1]; nw[1] = E[Y.mprw + 4 * i + 2]; nw[2] = E[Y.mprw + 4 * i + 3]; have_nw = true; }
        }
        // portal witnesses in per-lane LDS scratch: the contact-jacobian area of region X, not written before the rows stage
        // (TRK: a 1e-6 tolerance -- MuJoCo's ccd default -- was measured: narrow phase -15 %, but the one-substep qpos error p50 grows 2.7e-6 -> 1.5e-5)
        if (mpr_penetration_wl<TRK ? 2 : 0>(o1, o2, MPR_TOL, 60, &depth, dir, pos, &nsup, have_nw ? nw : nullptr, E + Y.cJ + 12 * lane, MT)) {
          dist = margin - depth;
          normalize3(dir);
          mpr_hit = true; mpr_n[0] = dir[0]; mpr_n[1] = dir[1]; mpr_n[2] = dir[2];
          float dw[3], pw[3], R1b[9];
          geom_world_mat(W, Y, E, g1, R1b, brp);   // recomputed (9 LDS reads + a 3x3 product) instead of kept live across the portal refinement
          matvec(dw, R1b, dir);
          matvec(pw, R1b, pos);
#pragma unroll
          for (int k = 0; k < 3; k++) { cpos[k] = pw[k] + x1[k]; nrm[k] = dw[k]; }
          hit = true;
        }
                  }
      }
      if (hit && !(dist < margin - Q.gap)) hit = false;
      if (hit2 && !(dist2 < margin - Q.gap)) hit2 = false;
    }
    {  // slowest lane of this round: MPR lanes cost ~8 + refinement steps, analytic pairs ~1
      int w = nsup + 8;
      w = max(w, __builtin_amdgcn_update_dpp(0, w, 0xB1, 0xf, 0xf, true));
      w = max(w, __builtin_amdgcn_update_dpp(0, w, 0x4E, 0xf, 0xf, true));
      w = max(w, __builtin_amdgcn_update_dpp(0, w, 0x141, 0xf, 0xf, true));
      w = max(w, __builtin_amdgcn_update_dpp(0, w, 0x140, 0xf, 0xf, true));
      f_mpr += max(max(rdlanei(w, 0), rdlanei(w, 16)), max(rdlanei(w, 32), rdlanei(w, 48)));
    }
    {  // rebuild the warm-start table from this round's MPR contacts (all lookups of the round are done)
      SYNC();
      unsigned long long wb = __ballot(mpr_hit);
      int wpos = n_mprw_new + __popcll(wb & ((1ull << lane) - 1ull));
      if (mpr_hit && wpos < MPRW) {
        ((int*)(E + Y.mprw))[4 * wpos] = p;
        E[Y.mprw + 4 * wpos + 1] = mpr_n[0]; E[Y.mprw + 4 * wpos + 2] = mpr_n[1]; E[Y.mprw + 4 * wpos + 3] = mpr_n[2];
      }
      n_mprw_new = min(n_mprw_new + (int)__popcll(wb), MPRW);
    }
    unsigned long long bal = __ballot(hit);
    int pos = ncon + __popcll(bal & ((1ull << lane) - 1ull));
    if (hit && pos < nct) con_row<C>(Y, E, ovf_env, ovf_row, pos, [&](const ConRow& R) {
      R.dist[0] = dist;
#pragma unroll
      for (int k = 0; k < 3; k++) { R.pos[k] = cpos[k]; R.nrm[k] = nrm[k]; }
      R.pair[0] = cword;
    });
    ncon += __popcll(bal);
    bal = FULL ? __ballot(hit2) : 0ull;
    if (bal) {
      pos = ncon + __popcll(bal & ((1ull << lane) - 1ull));
      if (hit2 && pos < nct) con_row<C>(Y, E, ovf_env, ovf_row, pos, [&](const ConRow& R) {
        R.dist[0] = dist2;
#pragma unroll
        for (int k = 0; k < 3; k++) { R.pos[k] = cpos2[k]; R.nrm[k] = nrm[k]; }
        R.pair[0] = cword;
      });
      ncon += __popcll(bal);
    }
  }
  if (ncon > nct) { flags |= MYO_FLAG_CONTACT_OVERFLOW; ncon = nct; }
  n_mprw = n_mprw_new;
  SYNC();
  return ncon;
}

#endif  // MYO_WAVE_COLLISION_H
