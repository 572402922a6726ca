// Device code shared by the translation units that hold multi-task kernels:
// agd_kernels.hip (one binary label per row, the CV sweep),
// agd_tasks_ovr.hip (one-vs-rest: a target class per column) and
// agd_tasks_bias.hip (a bias per task). The launch geometry, the binary
// losses and the per-group evaluation live here, so that both multiplier
// families run the same loss_mult on the same 4-column groups and leave the
// same partial layout; prox_elem, so that the free-row prox runs the element
// of k_prox_tasks.
#pragma once

#include <hip/hip_runtime.h>

#define WAVE 64
#define BLOCK 256
#define WAVES_PER_BLOCK (BLOCK / WAVE)

typedef long long ll;

template <typename T>
__device__ __forceinline__ T wave_reduce_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// loss conventions (z = <w, x_i>; identical algebra to MLlib 1.3's
// LogisticGradient/LeastSquaresGradient/HingeGradient with margin = -z):
//   logistic: m = sigmoid(z) - y ; loss = y>0 ? softplus(-z) : softplus(z)
//   lsq:      m = 2(z-y)         ; loss = (z-y)^2
//   hinge:    s = 2y-1 ; m = (s z < 1) ? -s : 0 ; loss = max(0, 1-s z)
#define LOSS_LOGISTIC 0
#define LOSS_LSQ 1
#define LOSS_HINGE 2
#define LOSS_SMOOTH_HINGE 3  // quadratically smoothed (Rennie) hinge

template <typename TACC>
__device__ __forceinline__ TACC softplus(TACC t) {
  // log(1 + e^t), overflow-stable
  if (t > (TACC)0) return t + log1p(exp(-t));
  return log1p(exp(t));
}
template <>
__device__ __forceinline__ float softplus<float>(float t) {
  if (t > 0.f) return t + log1pf(__expf(-t));
  return log1pf(__expf(t));
}

// Per-example multiplier + loss for the binary losses (shared by the
// margins-array and affine-combination kernels and the task multipliers).
template <typename TACC>
__device__ __forceinline__ void loss_mult(int loss_type, TACC z, TACC y,
                                          TACC& m, TACC& l) {
  if (loss_type == LOSS_LOGISTIC) {
    m = (TACC)1 / ((TACC)1 + exp(-z)) - y;
    l = (y > (TACC)0) ? softplus<TACC>(-z) : softplus<TACC>(z);
  } else if (loss_type == LOSS_LSQ) {
    const TACC diff = z - y;
    m = (TACC)2 * diff;
    l = diff * diff;
  } else if (loss_type == LOSS_HINGE) {
    const TACC s = (TACC)2 * y - (TACC)1;
    const TACC sz = s * z;
    m = (sz < (TACC)1) ? -s : (TACC)0;
    l = (sz < (TACC)1) ? (TACC)1 - sz : (TACC)0;
  } else {  // LOSS_SMOOTH_HINGE: 0 if sz>=1; (1-sz)^2/2 if 0<sz<1; 0.5-sz else
    const TACC s = (TACC)2 * y - (TACC)1;
    const TACC sz = s * z;
    if (sz >= (TACC)1) {
      m = (TACC)0;
      l = (TACC)0;
    } else if (sz > (TACC)0) {
      m = -s * ((TACC)1 - sz);
      l = (TACC)0.5 * ((TACC)1 - sz) * ((TACC)1 - sz);
    } else {
      m = -s;
      l = (TACC)0.5 - sz;
    }
  }
}

// Grid cap of the task multiplier: each block leaves KC + 1 f64 partials, so
// the workspace is TASKS_MAX_GRID * (KC + 1) doubles (sized by the wrapper
// through agd_tasks_ws_doubles) and the one-block finish reads all of it.
#define TASKS_MAX_GRID 1024

static inline int tasks_grid(ll work_items, ll per_block) {
  ll g = (work_items + per_block - 1) / per_block;
  if (g > TASKS_MAX_GRID) g = TASKS_MAX_GRID;
  if (g < 1) g = 1;
  return (int)g;
}

// One 4-column group of one row: a_ir from the fold test, the binary
// loss_mult per live column, M scaled by s_i * scale_r, the unscaled
// weighted loss into the caller's f64 partials. OVR: y is the row's class
// index and column j is evaluated with the label [int(y) == tg[j]] (one
// convert per row, one compare per column); otherwise y is the label itself
// and tg is not read.
template <bool OVR>
__device__ __forceinline__ void tasks_group(
    const float* __restrict__ zp, float y, float s, int f, int loss_type,
    int invert, const int (&h)[4], const float (&sc)[4], const bool (&live)[4],
    const int (&tg)[4], float* __restrict__ mp, double (&ls)[4]) {
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  const f32x4 zv = *(const f32x4*)zp;
  f32x4 mv = {0.f, 0.f, 0.f, 0.f};
  const int cls = OVR ? (int)y : 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool train = (f != h[j]);
    if (live[j] && (train != (invert != 0))) {
      float m, l;
      loss_mult<float>(loss_type, zv[j], OVR ? (cls == tg[j] ? 1.f : 0.f) : y,
                       m, l);
      mv[j] = m * s * sc[j];
      ls[j] += (double)l * (double)s;
    }
  }
  if (mp) *(f32x4*)mp = mv;
}

// Columns one lane-step of the any-K kernels covers: a wave per row, four
// columns per lane.
#define TASKS_CHUNK (WAVE * 4)

// One element of the proximal step, every prox kind (k_prox, k_prox_free,
// k_prox_tasks in agd_kernels.hip; k_prox_tasks_free in agd_tasks_bias.hip).
#define PROX_SIMPLE 0
#define PROX_L1 1
#define PROX_L2 2
#define PROX_ELASTIC 3  // l1 soft-threshold then l2 shrink (elastic net)

template <typename T>
__device__ __forceinline__ T prox_elem(int kind, T wi, T gi, T ts, T tl,
                                       T tl2, double& racc) {
  if (kind == PROX_SIMPLE) return wi - ts * gi;
  if (kind == PROX_L1) {
    const T w1 = wi - ts * gi;
    const T aw = fabs(w1) - tl * ts;
    const T wn = (aw > (T)0) ? ((w1 > (T)0) ? aw : -aw) : (T)0;
    racc += (double)tl * fabs((double)wn);
    return wn;
  }
  if (kind == PROX_L2) {
    const T wn = wi * ((T)1 - ts * tl) - ts * gi;
    racc += 0.5 * (double)tl * (double)wn * (double)wn;
    return wn;
  }
  // PROX_ELASTIC: prox of tl*|w|_1 + tl2/2*|w|^2 —
  // soft-threshold by ts*tl, then shrink by 1/(1 + ts*tl2)
  const T w1 = wi - ts * gi;
  const T aw = fabs(w1) - tl * ts;
  const T wsoft = (aw > (T)0) ? ((w1 > (T)0) ? aw : -aw) : (T)0;
  const T wn = wsoft / ((T)1 + ts * tl2);
  racc += (double)tl * fabs((double)wn) +
          0.5 * (double)tl2 * (double)wn * (double)wn;
  return wn;
}
