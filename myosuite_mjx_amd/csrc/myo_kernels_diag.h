// myo_kernels_diag.h -- kernels that measure or disturb the machine, not the simulation: the register and scratch poison kernels of the
// diagnostic build (MYO_POISON) and the VALU issue-rate probe (myo_probe_valu).
// Part of the single translation unit myo_hip.hip; not a stand-alone header.
#ifndef MYO_KERNELS_DIAG_H
#define MYO_KERNELS_DIAG_H

// VALU issue-rate probe (bench.py roofline): every wave runs `iters` x 256 independent v_fma_f32 (8 accumulator chains, so that a wave's
// own dependent-issue latency is not the limit), with W waves resident on every SIMD (workgroup = 4 W waves, one workgroup per CU forced
// by its LDS request).  wave-instructions / elapsed time = what the chip's VALUs can issue at that occupancy, at the clock the chip
// actually holds under this load.
#if MYO_POISON
// diagnostic build: fills the private (scratch) memory of every wave slot with NaNs before each step launch, so that a register spill
// which is stored under a partial exec mask and reloaded under a wider one (or any other read of a scratch word the kernel did not write)
// turns into wrong numbers instead of depending on what earlier kernels left there
__global__ void __launch_bounds__(64) scratch_poison_kernel(float* sink, int n) {
  volatile float buf[512];
  for (int i = 0; i < 512; i++) buf[i] = __int_as_float(0x7fc00000 | i);
  if (n < 0) sink[threadIdx.x] = buf[(-n) & 511];
}
// ... and the register files: a wave starts with whatever the previous wave left in its VGPR / AGPR / SGPR allocation, so a read of a
// register the kernel never wrote (a value defined under a lane predicate and read by other lanes through a shuffle / v_readlane, an
// `implicit-def`) is order-dependent in exactly the way a stale scratch word is.  One wave per SIMD owning all 512 vector registers writes
// NaN patterns into every one of them; a second kernel at 8 waves per SIMD does the same for the scalar registers.
#define MYO_R1(p, n) p #n
#define MYO_R10(M, p, t) M(p, t##0) M(p, t##1) M(p, t##2) M(p, t##3) M(p, t##4) M(p, t##5) M(p, t##6) M(p, t##7) M(p, t##8) M(p, t##9)
#define MYO_R100(M, p, h) MYO_R10(M, p, h##0) MYO_R10(M, p, h##1) MYO_R10(M, p, h##2) MYO_R10(M, p, h##3) MYO_R10(M, p, h##4) \
                          MYO_R10(M, p, h##5) MYO_R10(M, p, h##6) MYO_R10(M, p, h##7) MYO_R10(M, p, h##8) MYO_R10(M, p, h##9)
#define MYO_R256(M, p) MYO_R10(M, p, ) MYO_R10(M, p, 1) MYO_R10(M, p, 2) MYO_R10(M, p, 3) MYO_R10(M, p, 4) MYO_R10(M, p, 5) MYO_R10(M, p, 6) \
                       MYO_R10(M, p, 7) MYO_R10(M, p, 8) MYO_R10(M, p, 9) MYO_R100(M, p, 1) MYO_R10(M, p, 20) MYO_R10(M, p, 21) MYO_R10(M, p, 22) \
                       MYO_R10(M, p, 23) MYO_R10(M, p, 24) M(p, 250) M(p, 251) M(p, 252) M(p, 253) M(p, 254) M(p, 255)
#define MYO_R102(M, p) MYO_R10(M, p, ) MYO_R10(M, p, 1) MYO_R10(M, p, 2) MYO_R10(M, p, 3) MYO_R10(M, p, 4) MYO_R10(M, p, 5) MYO_R10(M, p, 6) \
                       MYO_R10(M, p, 7) MYO_R10(M, p, 8) MYO_R10(M, p, 9) M(p, 100) M(p, 101)
#define MYO_WV(p, n) "v_mov_b32 v" #n ", %0\n\t"
#define MYO_WA(p, n) "v_accvgpr_write_b32 a" #n ", %0\n\t"
#define MYO_WS(p, n) "s_mov_b32 s" #n ", 0x7fc0beef\n\t"
#define MYO_CL(p, n) , p #n
__global__ void __launch_bounds__(64, 1) vgpr_poison_kernel(int bits) {
  asm volatile(MYO_R256(MYO_WV, "") MYO_R256(MYO_WA, "") "s_nop 0" : : "s"(bits) : "memory" MYO_R256(MYO_CL, "v") MYO_R256(MYO_CL, "a"));
}
__global__ void __launch_bounds__(64, 8) sgpr_poison_kernel() {
  asm volatile(MYO_R102(MYO_WS, "") "s_nop 0" : : : "memory" MYO_R102(MYO_CL, "s"));
}
#endif
__global__ void __launch_bounds__(1024) valu_probe_kernel(float* out, int iters, float seed) {
  extern __shared__ float lds_dummy[];
  float a0 = seed, a1 = seed + 1.f, a2 = seed + 2.f, a3 = seed + 3.f, a4 = seed + 4.f, a5 = seed + 5.f, a6 = seed + 6.f, a7 = seed + 7.f;
  const float m = 1.0000001f, c = 1e-9f * (float)threadIdx.x;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int u = 0; u < 32; u++) {
      asm volatile("v_fma_f32 %0, %0, %8, %9\n\tv_fma_f32 %1, %1, %8, %9\n\tv_fma_f32 %2, %2, %8, %9\n\tv_fma_f32 %3, %3, %8, %9\n\t"
                   "v_fma_f32 %4, %4, %8, %9\n\tv_fma_f32 %5, %5, %8, %9\n\tv_fma_f32 %6, %6, %8, %9\n\tv_fma_f32 %7, %7, %8, %9"
                   : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(c));
    }
  }
  if (out) out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) + (threadIdx.x == 4096 ? lds_dummy[0] : 0.f);
}

#endif  // MYO_KERNELS_DIAG_H
