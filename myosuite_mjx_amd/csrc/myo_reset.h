// myo_reset.h -- the reset of an env: its pieces (one per owner: a task, a muscle condition, a per-env override), reset_body that calls them in
// order, reset_kernel, the record task_post_kernel's reset reads (ResetArgs), and on the host launch_reset with myo_reset / myo_autoreset.
// Part of the single translation unit myo_hip.hip, which includes this file twice: the device half before myo_kernels_aux.h (task_post_kernel
// calls reset_body) and myo_host.h (myo_batch holds a ResetArgs), the host half after myo_host.h, which defines the myo_batch it launches on.
#ifndef MYO_RESET_H
#define MYO_RESET_H

// Every piece takes what it reads of: the batch and task records (read through ResetArgs in the fused epilogue), the episode's seed
// (rng_episode_seed), the global env id ge that keys every counter, the env and the lane.  A piece draws through rng_u<stream> (the table in
// myo_common.h) only, tests no task id, and is switched by the members it names.  All lanes of the env's wave call every piece.

// Episode bookkeeping.  Reads Bt.episode; lane 0 writes Bt.episode, elapsed, done, time.  Returns the seed of the new episode: a fresh RNG
// stream per (env, episode).  Draws nothing
__device__ __forceinline__ uint64_t reset_episode(const DevBatch& Bt, uint64_t seed, const int e, const int lane) {
  seed = rng_episode_seed(seed, Bt.episode[e]);
  __syncthreads();                                            // every lane has read done / elapsed / episode before lane 0 updates them
  if (lane == 0) { Bt.episode[e] += 1; Bt.elapsed[e] = 0; Bt.done[e] = 0.f; Bt.time[e] = 0; }
  return seed;
}

// qpos, walk: reset_type "random" (walk_v0.py:316-332): one coin per episode picks the keyframe.  Reads T.init_qpos_alt.  Stream RS_KEYFRAME_COIN
__device__ __forceinline__ bool walk_keyframe_coin(const TaskDev& T, uint64_t seed, uint64_t ge) {
  return T.init_qpos_alt && rng_u<RS_KEYFRAME_COIN>(seed, ge, 0) >= 0.5f;
}
// qpos, walk: normal noise on every coordinate of the keyframe but the root height and quaternion (walk_v0.py:316-332).  Reads T.init_qpos_alt,
// T.reset_noise_std.  Streams RS_KEYFRAME_NOISE_U1 / _U2 (Box-Muller)
__device__ __forceinline__ float walk_keyframe_noise(const TaskDev& T, uint64_t seed, uint64_t ge, float q, const int i) {
  if (T.init_qpos_alt && T.reset_noise_std > 0.f && !(i >= 2 && i <= 6)) {   // every coordinate but the root height and quaternion
    const float u1 = fmaxf(rng_u<RS_KEYFRAME_NOISE_U1>(seed, ge, i), 1e-7f), u2 = rng_u<RS_KEYFRAME_NOISE_U2>(seed, ge, i);
    q += T.reset_noise_std * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
  }
  return q;
}
// qpos, pose (reset_random): uniform over the joint range, whatever q was (nq == nv checked at configure).  Reads T.jnt_lo, T.jnt_hi.  Stream RS_QPOS
__device__ __forceinline__ float pose_joint_draw(const TaskDev& T, uint64_t seed, uint64_t ge, const int i) {
  return T.jnt_lo[i] + (T.jnt_hi[i] - T.jnt_lo[i]) * rng_u<RS_QPOS>(seed, ge, i);
}
// qpos, stand: init + U(noise), clipped (walk_v0.py:152-167).  Reads T.rnd.  Stream RS_QPOS
__device__ __forceinline__ float stand_noise_clip(const TaskDev& T, uint64_t seed, uint64_t ge, const float q, const int nq, const int i) {
  const float nl = T.rnd[i], nh = T.rnd[nq + i];
  return fminf(fmaxf(q + nl + (nh - nl) * rng_u<RS_QPOS>(seed, ge, i), T.rnd[2 * nq + i]), T.rnd[3 * nq + i]);
}
// qpos: the keyframe (the coin's, the task's, or the model's), then the draws above.  Reads T.init_qpos_alt, T.init_qpos, T.reset_random, T.rnd;
// writes Bt.qpos
__device__ __forceinline__ void reset_qpos(const DevBatch& Bt, const TaskDev& T, uint64_t seed, uint64_t ge, const int e, const int lane, const bool alt, const int nq, const float* qpos0) {
  for (int i = lane; i < nq; i += 64) {
    float q = alt ? T.init_qpos_alt[i] : (T.init_qpos ? T.init_qpos[i] : qpos0[i]);
    q = walk_keyframe_noise(T, seed, ge, q, i);
    if (T.reset_random) q = pose_joint_draw(T, seed, ge, i);
    else if (T.rnd) q = stand_noise_clip(T, seed, ge, q, nq, i);
    Bt.qpos[(size_t)e * nq + i] = q;
  }
}
// qvel (the chosen keyframe's, the task's, or zero) and the solver's warm start.  Reads T.init_qvel_alt, T.init_qvel; writes Bt.qvel, Bt.warm.
// Draws nothing
__device__ __forceinline__ void reset_qvel_warm(const DevBatch& Bt, const TaskDev& T, const int e, const int lane, const bool alt, const int nv) {
  for (int i = lane; i < nv; i += 64) {
    Bt.qvel[(size_t)e * nv + i] = (alt && T.init_qvel_alt) ? T.init_qvel_alt[i] : (T.init_qvel ? T.init_qvel[i] : 0.f);
    Bt.warm[(size_t)e * nv + i] = 0;
  }
}
// Actuators: act and ctrl to zero, and the fatigue compartments: all motor units resting (CumulativeFatigue.reset defaults, fatigue.py:130-134),
// fatigue_reset_random (fatigue.py:115-122) or fatigue_reset_vec (:124-130).  Reads T.fatigue_mode, T.fatigue_vec; writes Bt.act, Bt.ctrl,
// Bt.fatigue.  Streams RS_FATIGUE_NF / _AP
__device__ __forceinline__ void reset_actuators_fatigue(const DevBatch& Bt, const TaskDev& T, uint64_t seed, uint64_t ge, const int e, const int lane, const int nu) {
  for (int i = lane; i < nu; i += 64) {
    Bt.act[(size_t)e * nu + i] = 0; Bt.ctrl[(size_t)e * nu + i] = 0;
    float MA = 0.f, MR = 1.f, MF = 0.f;
    if (T.fatigue_mode == 1) {   // fatigue_reset_random (fatigue.py:115-122)
      const float nf = rng_u<RS_FATIGUE_NF>(seed, ge, i), ap = rng_u<RS_FATIGUE_AP>(seed, ge, i);
      MA = nf * ap; MR = nf * (1.f - ap); MF = 1.f - nf;
    } else if (T.fatigue_mode == 2 && T.fatigue_vec) { MF = T.fatigue_vec[i]; MR = 1.f - MF; }   // fatigue_reset_vec (:124-130)
    Bt.fatigue[(size_t)e * 3 * nu + i] = MA; Bt.fatigue[(size_t)e * 3 * nu + nu + i] = MR; Bt.fatigue[(size_t)e * 3 * nu + 2 * nu + i] = MF;
  }
}
// Sensor rows of a fresh episode read zero, like mj_resetData.  Reads Bt.ntouch; writes Bt.sens, Bt.cfrc.  Draws nothing
__device__ __forceinline__ void reset_sensor_rows(const DevBatch& Bt, const int e, const int lane) {
  if (Bt.sens) {
    for (int i = lane; i < Bt.ntouch; i += 64) Bt.sens[(size_t)e * Bt.ntouch + i] = 0.f;
    for (int i = lane; i < 3 * (Bt.ntouch + 1); i += 64) Bt.cfrc[(size_t)e * 3 * (Bt.ntouch + 1) + i] = 0.f;
  }
}
// Target row: target_lo, or U(target_lo, target_hi) per component; component T.target_floor (-1: none) is rounded down and capped at its
// hi -- the baoding task's direction sign: U(-1, 2) rounded down, one of -1, 0, +1.  Reads T.ntarget, T.target_lo, T.target_hi,
// T.target_generate, T.target_floor; writes Bt.target.  Stream RS_TARGET
__device__ __forceinline__ void reset_target(const DevBatch& Bt, const TaskDev& T, uint64_t seed, uint64_t ge, const int e, const int lane) {
  for (int i = lane; i < T.ntarget; i += 64) {
    float lo = T.target_lo[i], hi = T.target_hi[i];
    float t = T.target_generate ? lo + (hi - lo) * rng_u<RS_TARGET>(seed, ge, i) : lo;
    if (i == T.target_floor) t = fminf(floorf(t), hi);
    Bt.target[(size_t)e * T.ntarget + i] = t;
  }
}
// Geom size, hold: ObjHoldRandomEnvV0.reset (obj_hold_v0.py:133-139): a fresh size for the object's geom per episode (its mass and inertia
// stay).  Reads T.gsize_type, T.gsize_lo, T.gsize_hi; writes Bt.gsize.  Stream RS_GEOM_SIZE
__device__ __forceinline__ void hold_geom_size(const DevBatch& Bt, const TaskDev& T, uint64_t seed, uint64_t ge, const int e, const int lane) {
  if (T.gsize_type && Bt.gsize && lane == 0) {
    float sz[3];
    for (int k = 0; k < 3; k++) sz[k] = T.gsize_lo[k] + (T.gsize_hi[k] - T.gsize_lo[k]) * rng_u<RS_GEOM_SIZE>(seed, ge, k);
    float rb = T.gsize_type == GEOM_ELLIPSOID ? fmaxf(sz[0], fmaxf(sz[1], sz[2])) : (T.gsize_type == GEOM_CAPSULE ? sz[0] + sz[1] : (T.gsize_type == GEOM_CYLINDER ? sqrtf(sz[0] * sz[0] + sz[1] * sz[1]) : sz[0]));
    float* G = Bt.gsize + 4 * (size_t)e;
    G[0] = sz[0]; G[1] = sz[1]; G[2] = sz[2]; G[3] = rb;
  }
}
// Body mass: PoseEnvV0.reset (pose_v0.py:163-176, weight_bodyname / weight_range): a fresh mass per episode for every body whose range is
// not empty.  Reads Bt.bmass_range, Bt.nbody; writes Bt.bmass.  Stream RS_BODY_MASS
__device__ __forceinline__ void reset_body_mass(const DevBatch& Bt, uint64_t seed, uint64_t ge, const int e, const int lane) {
  if (Bt.bmass_range) {
    const float* lo = Bt.bmass_range + (size_t)e * 2 * Bt.nbody;
    for (int i = lane; i < Bt.nbody; i += 64) {
      const float l = lo[i], h = lo[Bt.nbody + i];
      if (h > l) Bt.bmass[(size_t)e * Bt.nbody + i] = l + (h - l) * rng_u<RS_BODY_MASS>(seed, ge, i);
    }
  }
}
// Body offset: KeyTurnEnvV0.reset (key_turn_v0.py:164-167, Random variant): the key body's position = its compiled position + U(-0.01, 0.01)^3
// per episode.  Reads Bt.bpos_range; writes Bt.bpos.  Stream RS_BODY_OFFSET
__device__ __forceinline__ void reset_body_offset(const DevBatch& Bt, uint64_t seed, uint64_t ge, const int e, const int lane) {
  if (Bt.bpos_range && lane < 3) {
    const float l = Bt.bpos_range[(size_t)e * 6 + lane], h = Bt.bpos_range[(size_t)e * 6 + 3 + lane];
    if (h > l) Bt.bpos[(size_t)e * 3 + lane] = l + (h - l) * rng_u<RS_BODY_OFFSET>(seed, ge, lane);
  }
}
// Body quaternion: PenTwirlRandomEnvV0.reset (pen_v0.py:173-184): the target's body_quat = euler2quat(U(-1, 1), U(-1, 1), 0) per episode.
// Reads Bt.bquat_range; writes Bt.bquat.  Stream RS_BODY_QUAT
__device__ __forceinline__ void reset_body_quat(const DevBatch& Bt, uint64_t seed, uint64_t ge, const int e, const int lane) {
  if (Bt.bquat_range && lane == 0) {
    const float* r = Bt.bquat_range + (size_t)e * 6;
    if (r[3] > r[0] || r[4] > r[1] || r[5] > r[2]) {
      float a[3];
#pragma unroll
      for (int k = 0; k < 3; k++) a[k] = r[3 + k] > r[k] ? r[k] + (r[3 + k] - r[k]) * rng_u<RS_BODY_QUAT>(seed, ge, k) : r[k];
      euler2quat(Bt.bquat + (size_t)e * 4, a);
    }
  }
}
// Object parameters (myo_objects_set_draws; BaodingEnvV1.reset baoding_v1.py:360-385, ReorientEnvV0.reset reorient_v0.py:221-247): scalar
// parameter p = base + scale * u, u one of the env's shared draws or the parameter's own; scale 0: the parameter stays.  Reads Bt.obj_draw,
// Bt.obj_draw_k, Bt.obj_ng, Bt.obj_nb; writes Bt.obj_size, obj_pos, obj_fric, obj_mass.  Stream RS_OBJECT (obj_draw_u)
__device__ __forceinline__ void reset_object_params(const DevBatch& Bt, uint64_t seed, uint64_t ge, const int e, const int lane) {
  if (Bt.obj_draw) {
    const int ng3 = 3 * Bt.obj_ng, np = 9 * Bt.obj_ng + Bt.obj_nb;
    for (int p = lane; p < np; p += 64) {
      const float base = Bt.obj_draw[2 * p], scale = Bt.obj_draw[2 * p + 1];
      if (scale == 0.f) continue;
      const float v = fmaf(scale, obj_draw_u(seed, ge, Bt.obj_draw_k[p], p), base);   // (one rounding: the host twin computes it in float64)
      if (p < ng3) Bt.obj_size[(size_t)e * ng3 + p] = v;
      else if (p < 2 * ng3) Bt.obj_pos[(size_t)e * ng3 + p - ng3] = v;
      else if (p < 3 * ng3) Bt.obj_fric[(size_t)e * ng3 + p - 2 * ng3] = v;
      else Bt.obj_mass[(size_t)e * Bt.obj_nb + p - 3 * ng3] = v;
    }
  }
}
// Terrain, rough ~ U(-0.5, 0.5)^n, min-max normalised over the grid, * 0.08 - 0.02 (walk_v0.py:563-567).  Writes H[n].  Stream RS_TERRAIN_ROUGH
__device__ __forceinline__ void terrain_rough(uint64_t seed, uint64_t ge, const int lane, float* H, const int n) {
  float mn = 1e30f, mx = -1e30f;
  for (int i = lane; i < n; i += 64) { float u = rng_u<RS_TERRAIN_ROUGH>(seed, ge, i); mn = fminf(mn, u); mx = fmaxf(mx, u); }
  for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off)); mx = fmaxf(mx, __shfl_xor(mx, off)); }
  const float inv = 1.0f / fmaxf(mx - mn, 1e-12f);
  for (int i = lane; i < n; i += 64) H[i] = (rng_u<RS_TERRAIN_ROUGH>(seed, ge, i) - mn) * inv * 0.08f - 0.02f;
}
// Terrain, hilly: 3000 flat cells at the top level, then -2 + 0.5 (sin(linspace(0, 3 pi, 7000) + pi/2) - 1), min-max normalised: 0.5 + 0.5 cos(t)
// (walk_v0.py:569-592).  Cell k of the unflipped grid.  Draws nothing
__device__ __forceinline__ float terrain_hilly(const int k) {
  return k < 3000 ? 1.0f : 0.5f + 0.5f * cosf((float)(k - 3000) * (3.0f * 3.14159265358979f / 6999.0f));
}
// Terrain, stairs: 52 flat rows, then 12 stairs of 4 rows each, 0.1 high, normalised by 2 + 0.1 * 12 (walk_v0.py:594-620).  Cell k of the
// unflipped grid.  Draws nothing
__device__ __forceinline__ float terrain_stairs(const int k) {
  const int row = k / 100;
  return row < 52 ? 0.0f : 0.1f * (float)((row - 52) / 4) / 3.2f;
}
// Terrain: TerrainEnvV0.reset (walk_v0.py:563-622): a fresh 100 x 100 elevation grid per episode (in units of the height field's z scale).
// Distribution parity only for the random draws, as for every reset.  Reads T.terrain, T.hf_n, T.terrain_lo, T.terrain_hi; writes Bt.hfield.
// Stream RS_TERRAIN_SCALE: the height of the hilly and stairs grids
__device__ __forceinline__ void reset_terrain(const DevBatch& Bt, const TaskDev& T, uint64_t seed, uint64_t ge, const int e, const int lane) {
  if (T.terrain && Bt.hfield) {
    float* H = Bt.hfield + (size_t)e * T.hf_n;
    const int n = T.hf_n;
    if (T.terrain == MYO_TERRAIN_ROUGH) terrain_rough(seed, ge, lane, H, n);
    else {
      const float sc = T.terrain_lo + (T.terrain_hi - T.terrain_lo) * rng_u<RS_TERRAIN_SCALE>(seed, ge, 0);
      for (int i = lane; i < n; i += 64) {
        const int k = n - 1 - i;             // np.flip(grid, [0, 1]) of a row-major grid = the flat array reversed
        H[i] = (T.terrain == MYO_TERRAIN_HILLY ? terrain_hilly(k) : terrain_stairs(k)) * sc;
      }
    }
  }
}

// auto_max > 0: gym TimeLimit / done auto-reset (reset iff done or elapsed >= auto_max); else mask-driven reset.
// One 64-lane workgroup per env: envs that are not reset leave after one test, the others write their rows coalesced
// (one thread per env needed ~500 serialised scattered stores per reset: 27 ms for a full reset of 4096 leg envs)
// TEST = false: the caller has made the test itself (task_post_kernel, which reads Bt and T of the reset from memory only afterwards)
template <bool TEST = true>
__device__ __forceinline__ bool reset_body(const DevBatch& Bt, const TaskDev& T, int nq, int nv, int nu, const float* qpos0, const uint8_t* mask, uint64_t seed,
                                           int env_offset, int auto_max, const int e, const int lane) {
  if constexpr (TEST) {
    if (auto_max > 0) { if (!(Bt.done[e] > 0.f || Bt.elapsed[e] >= auto_max)) return false; }
    else if (mask && !mask[e]) return false;
  }
  seed = reset_episode(Bt, seed, e, lane);
  const uint64_t ge = (uint64_t)(e + env_offset);
  const bool alt = walk_keyframe_coin(T, seed, ge);
  reset_qpos(Bt, T, seed, ge, e, lane, alt, nq, qpos0);
  reset_qvel_warm(Bt, T, e, lane, alt, nv);
  reset_actuators_fatigue(Bt, T, seed, ge, e, lane, nu);
  reset_sensor_rows(Bt, e, lane);
  reset_target(Bt, T, seed, ge, e, lane);
  hold_geom_size(Bt, T, seed, ge, e, lane);
  reset_body_mass(Bt, seed, ge, e, lane);
  reset_body_offset(Bt, seed, ge, e, lane);
  reset_body_quat(Bt, seed, ge, e, lane);
  reset_object_params(Bt, seed, ge, e, lane);
  reset_terrain(Bt, T, seed, ge, e, lane);
  return true;
}
__global__ void __launch_bounds__(64) reset_kernel(DevBatch Bt, TaskDev T, int nq, int nv, int nu, const float* qpos0, const uint8_t* mask, uint64_t seed,
                                                  int env_offset, int auto_max) {
  if ((int)blockIdx.x >= Bt.B) return;
  reset_body(Bt, T, nq, nv, nu, qpos0, mask, seed, env_offset, auto_max, blockIdx.x, threadIdx.x);
}
// what reset_apply reads of a batch, as one record in device memory (myo_batch::d_reset, kept equal to db / task by launch_task_post)
struct ResetArgs { DevBatch Bt; TaskDev T; };

#endif  // MYO_RESET_H

// ---- the host half: compiled by the second inclusion, once myo_host.h has defined myo_batch
#if defined(MYO_HOST_H) && !defined(MYO_RESET_HOST)
#define MYO_RESET_HOST

static int launch_reset(myo_batch* b, const uint8_t* mask_dev, uint64_t seed, void* stream, int max_episode_steps) {
  b->reset_seed = seed;
  const DevModel& dm = b->model->dm;
  HIPCHK(hipSetDevice(b->model->device));
  hipLaunchKernelGGL(reset_kernel, dim3(b->db.B), dim3(64), 0, (hipStream_t)stream, b->db, b->task, b->model->nq, dm.nv, dm.nu, dm.qpos0, mask_dev, seed,
                     b->env_offset, max_episode_steps);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

extern "C" {

int myo_reset(myo_batch* b, const uint8_t* mask_dev, uint64_t seed, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_reset: null");
  return launch_reset(b, mask_dev, seed, stream, 0);
}

int myo_autoreset(myo_batch* b, int max_episode_steps, uint64_t seed, void* stream) {
  if (!b || max_episode_steps <= 0) return fail(MYO_E_ARG, "myo_autoreset: bad arguments");
  return launch_reset(b, nullptr, seed, stream, max_episode_steps);
}

}  // extern "C"

#endif  // MYO_RESET_HOST
