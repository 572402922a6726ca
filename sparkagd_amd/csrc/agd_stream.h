// Device code shared by the translation units that stream a dense shard:
// agd_kernels.hip (the full passes) and agd_rows.hip (the passes over a
// compacted row list). The 16-byte lane loads of the shard and of the
// accumulator-typed vectors live here, and the two-stage f64 reduction, so
// that both families convert the features the same way and leave the same
// partial layout.
#pragma once

#include <hip/hip_runtime.h>

#include "agd_tasks.h"

typedef unsigned short ubf16;  // raw bf16 bits

__device__ __forceinline__ float bf2f(ubf16 u) {
  union { unsigned int i; float f; } v;
  v.i = ((unsigned int)u) << 16;
  return v.f;
}

// Block-level fp64 reduction of NACC accumulators into a per-block partial
// slot; a one-block k_reduce_partials finishes the sum. Two stages instead
// of leader atomics: 8192 same-word fp64 atomics serialize to ~0.5 ms
// (measured, d=1e7 fused-scalars) and are order-nondeterministic; the
// partial buffer costs ~30 us and is bitwise reproducible.
template <int NACC>
__device__ __forceinline__ void block_reduce_partial(double (&acc)[NACC],
                                                     double* part) {
  __shared__ double lds[WAVES_PER_BLOCK][NACC];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < NACC; ++k) {
    acc[k] = wave_reduce_sum(acc[k]);
    if (lane == 0) lds[wid][k] = acc[k];
  }
  __syncthreads();
  if (wid == 0 && lane < WAVES_PER_BLOCK) {
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
      double v = lds[lane][k];
#pragma unroll
      for (int off = WAVES_PER_BLOCK / 2; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
      if (lane == 0) part[(ll)blockIdx.x * NACC + k] = v;
    }
  }
}

// Final stage: one block sums the per-block partials into out[NACC]
// (ACCUMULATES into out so callers may chain; callers zero out first).
// SET overwrites out instead: nothing to zero, for slots of a scalar block
// that lives across calls (agd_at_step_tail).
template <int NACC, bool SET = false>
__global__ __launch_bounds__(BLOCK) void k_reduce_partials(
    const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += BLOCK)
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] += part[(ll)i * NACC + k];
  __shared__ double lds[WAVES_PER_BLOCK][NACC];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < NACC; ++k) {
    acc[k] = wave_reduce_sum(acc[k]);
    if (lane == 0) lds[wid][k] = acc[k];
  }
  __syncthreads();
  if (wid == 0 && lane < WAVES_PER_BLOCK) {
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
      double v = lds[lane][k];
#pragma unroll
      for (int off = WAVES_PER_BLOCK / 2; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
      if (lane == 0) out[k] = SET ? v : out[k] + v;
    }
  }
}

// Vector load of W elements of TA starting at p (16-byte pattern for W>1),
// converted to the accumulator type TACC.
template <typename TA, typename TACC, int W, bool NT = false>
__device__ __forceinline__ void loadW(const TA* __restrict__ p, TACC (&out)[W]) {
  if constexpr (W == 1) {
    if constexpr (sizeof(TA) == 1)
      out[0] = __builtin_amdgcn_cvt_f32_fp8((int)*(const unsigned char*)p, 0);
    else if constexpr (sizeof(TA) == 2) out[0] = bf2f(*(const ubf16*)p);
    else out[0] = (TACC)p[0];
  } else if constexpr (sizeof(TA) == 1) {  // fp8 e4m3fn, W == 16 (16 B)
    using i32x4 = __attribute__((ext_vector_type(4))) int;
    using f32x2 = __attribute__((ext_vector_type(2))) float;
    i32x4 v = NT ? __builtin_nontemporal_load((const i32x4*)p) : *(const i32x4*)p;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(v[ch], false);
      const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(v[ch], true);
      out[ch * 4 + 0] = lo[0];
      out[ch * 4 + 1] = lo[1];
      out[ch * 4 + 2] = hi[0];
      out[ch * 4 + 3] = hi[1];
    }
  } else if constexpr (sizeof(TA) == 2) {  // bf16, W == 8 (16 B)
    using u16x8 = __attribute__((ext_vector_type(8))) unsigned short;
    u16x8 v = NT ? __builtin_nontemporal_load((const u16x8*)p) : *(const u16x8*)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = bf2f((ubf16)v[k]);
  } else if constexpr (sizeof(TA) == 4) {  // f32, W == 4 (16 B)
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    f32x4 v = NT ? __builtin_nontemporal_load((const f32x4*)p) : *(const f32x4*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = (TACC)v[k];
  } else {  // f64, W == 2 (16 B)
    using f64x2 = __attribute__((ext_vector_type(2))) double;
    f64x2 v = NT ? __builtin_nontemporal_load((const f64x2*)p) : *(const f64x2*)p;
#pragma unroll
    for (int k = 0; k < 2; ++k) out[k] = (TACC)v[k];
  }
}

// Vector load of W accumulator-typed elements (16-B chunks; the address is
// W-element aligned by construction in the margins kernel).
template <typename TACC, int W>
__device__ __forceinline__ void loadAcc(const TACC* __restrict__ p, TACC (&out)[W]) {
  constexpr int EPC = 16 / sizeof(TACC);
  if constexpr (W >= EPC) {
#pragma unroll
    for (int ch = 0; ch < W / EPC; ++ch) {
      if constexpr (sizeof(TACC) == 4) {
        using f32x4 = __attribute__((ext_vector_type(4))) float;
        f32x4 v = *(const f32x4*)(p + ch * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[ch * 4 + k] = v[k];
      } else {
        using f64x2 = __attribute__((ext_vector_type(2))) double;
        f64x2 v = *(const f64x2*)(p + ch * 2);
#pragma unroll
        for (int k = 0; k < 2; ++k) out[ch * 2 + k] = v[k];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] = p[k];
  }
}
