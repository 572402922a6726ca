// A bias per task for the multi-task family (one-vs-rest, CV sweeps).
//
// The weights are the flat feature-major block [(d+1), R]: the first d*R
// entries are the [d, R] block every data pass already runs on (a contiguous
// 16-B aligned prefix view: no copy), the last R entries are the biases. With
// the shard extended by a column of ones,
//   A~ . [W; b^T] = A.W + 1.b^T        A~^T . M = [A^T.M ; sum_i M[i, :]]
// so the two shard streams stay as they are and the bias lives in the four
// small kernels of this file, in n*KC space or d*R space:
//   k_colsum_multi              out[c] = sum_i M[i, c]   (the gradient's tail)
//   k_add_bias_cols             Z[i, c] += coef * src[idx0 + c]
//   k_at_margin_update_tasks_off  the tracked margin update with a free row
//   k_prox_tasks_free           the per-task prox that leaves the bias row free
// All four are atomics-free and bitwise reproducible, and read the biases on
// the device from the weight vector (src + idx0), never from a host value:
// an intercept adds no host synchronisation and no H2D copy.
//
// The column sum is a kernel of its own and NOT a third accumulator forked
// into the seven multiplier kernels (k_multiplier_tasks<KC>, _anyk, the two
// one-vs-rest variants, later the softmax ones): one kernel serves all of
// them, the loss-only calls skip it, and what it re-reads is n*KC*4 bytes
// (16 MB against a 5.4 GB shard stream at the one-vs-rest benchmark shape).
//
// A translation unit of its own, compiled like agd_tasks_ovr.hip and linked
// into libagd_hip.so next to agd_kernels.hip, whose error string it sets.

#include <hip/hip_runtime.h>

#include <cstdio>

#include "agd_tasks.h"

extern "C" void agd_set_last_error(const char* msg);

static int bias_fail(const char* fmt, long long a, long long b, long long c) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  agd_set_last_error(buf);
  return 2;
}

static int bias_launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  agd_set_last_error(buf);
  return 1;
}

// Grid of the element-wise kernels (the cap of agd_kernels.hip's grid_for).
static inline int bias_grid(ll work_items, ll per_block) {
  ll g = (work_items + per_block - 1) / per_block;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (int)g;
}

// 16-B vector of T (4 f32 or 2 f64).
template <typename T>
struct Vec16 {
  static constexpr int VE = 16 / sizeof(T);
  typedef T type __attribute__((ext_vector_type(VE)));
};

template <typename T>
__device__ __forceinline__ void load16(const T* __restrict__ p,
                                       T (&out)[Vec16<T>::VE]) {
  const typename Vec16<T>::type v = *(const typename Vec16<T>::type*)p;
#pragma unroll
  for (int k = 0; k < Vec16<T>::VE; ++k) out[k] = v[k];
}

template <typename T>
__device__ __forceinline__ void store16(T* __restrict__ p,
                                        const T (&in)[Vec16<T>::VE]) {
  typename Vec16<T>::type v;
#pragma unroll
  for (int k = 0; k < Vec16<T>::VE; ++k) v[k] = in[k];
  *(typename Vec16<T>::type*)p = v;
}

// ---------------------------------------------------------------------------
// Column sums of the padded multiplier M [n, KC] (f32), accumulated in f64.
// ---------------------------------------------------------------------------

// KC in {4, 8, 16, 32}: the work split of k_multiplier_tasks<KC>. One 16-B
// load per 4-column group; the grid stride is a multiple of KC/4, so a thread
// keeps ONE column group for its whole loop and holds 4 f64 partials whatever
// KC is. Lanes with equal (lane % G4) own the same columns: the xor tree
// stops at G4, the four waves meet in a [4][KC] f64 LDS tile and the block
// stores KC partials.
template <int KC>
__global__ __launch_bounds__(BLOCK) void k_colsum_multi(
    const float* __restrict__ M, ll n, double* __restrict__ part) {
  constexpr int G4 = KC / 4;
  static_assert(BLOCK % G4 == 0 && WAVE % G4 == 0, "column group must tile");
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  const ll gid = (ll)blockIdx.x * BLOCK + threadIdx.x;
  const ll ngroups = n * G4;
  const ll stride = (ll)gridDim.x * BLOCK;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (ll g = gid; g < ngroups; g += stride) {
    const f32x4 v = *(const f32x4*)(M + g * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] += (double)v[j];
  }
  __shared__ double lds[WAVES_PER_BLOCK][KC];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double v = a[j];
#pragma unroll
    for (int off = 32; off >= G4; off >>= 1) v += __shfl_xor(v, off, WAVE);
    if (lane < G4) lds[wid][lane * 4 + j] = v;
  }
  __syncthreads();
  if (threadIdx.x < KC) {
    double v = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) v += lds[w][threadIdx.x];
    part[(ll)blockIdx.x * KC + threadIdx.x] = v;
  }
}

// Any 4-aligned KC (> 32 in practice): the work split of
// k_multiplier_tasks_anyk. One wave per row, lane l on the column group at
// chunk + 4l, the column axis walked in chunks of 256.
__global__ __launch_bounds__(BLOCK) void k_colsum_multi_anyk(
    const float* __restrict__ M, ll n, int KC, double* __restrict__ part) {
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  __shared__ double lds[WAVES_PER_BLOCK][TASKS_CHUNK];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const ll wave_gid = (ll)blockIdx.x * WAVES_PER_BLOCK + wid;
  const ll n_waves = (ll)gridDim.x * WAVES_PER_BLOCK;
  for (int chunk = 0; chunk < KC; chunk += TASKS_CHUNK) {
    const int c0 = chunk + lane * 4;
    const bool active = c0 < KC;  // KC % 4 == 0: the whole group is inside
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (active)
      for (ll i = wave_gid; i < n; i += n_waves) {
        const f32x4 v = *(const f32x4*)(M + i * KC + c0);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += (double)v[j];
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) lds[wid][lane * 4 + j] = a[j];
    __syncthreads();
    const int c = chunk + threadIdx.x;  // BLOCK == TASKS_CHUNK columns
    if (c < KC) {
      double v = lds[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < WAVES_PER_BLOCK; ++w) v += lds[w][threadIdx.x];
      part[(ll)blockIdx.x * KC + c] = v;
    }
    __syncthreads();
  }
  static_assert(BLOCK == TASKS_CHUNK, "one finishing thread per chunk column");
}

// One-block finish (OVERWRITES its outputs): out[c] = sum_b part[b, c] for
// c < R in fixed block order, written in the gradient's dtype T straight to
// `tail` (the last R entries of the gradient block) and, when out64 is given,
// as f64 too. Wave w sums blocks w, w+4, ... of 64 columns at a time.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_colsum_finish(
    const double* __restrict__ part, int nblocks, int KC, int R,
    T* __restrict__ tail, double* __restrict__ out64) {
  __shared__ double lds[WAVES_PER_BLOCK][WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  for (int chunk = 0; chunk < KC; chunk += WAVE) {
    const int c = chunk + lane;
    double a = 0.0;
    if (c < KC) {
      // the loads are independent, the sum stays in block order
#pragma unroll 8
      for (int b = wid; b < nblocks; b += WAVES_PER_BLOCK)
        a += part[(ll)b * KC + c];
    }
    lds[wid][lane] = a;
    __syncthreads();
    if (wid == 0 && c < R) {
      double v = lds[0][lane];
#pragma unroll
      for (int w = 1; w < WAVES_PER_BLOCK; ++w) v += lds[w][lane];
      if (tail) tail[c] = (T)v;
      if (out64) out64[c] = v;
    }
    __syncthreads();
  }
}

// Doubles of workspace agd_colsum_multi needs: KC partials per block.
extern "C" long long agd_colsum_ws_doubles(int kc) {
  return (long long)TASKS_MAX_GRID * (long long)kc;
}

// tail (dtype 1 = f32, 2 = f64; R entries) and out64 (f64[R]) are
// overwritten; either may be null. M is the f32 [n * kc] flat.
extern "C" int agd_colsum_multi(const void* M, long long n, int R, int kc,
                                int dtype, void* tail, void* out64, void* ws,
                                void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (kc < 4 || (kc & 3) || R < 1 || R > kc || n < 0)
    return bias_fail("colsum_multi: bad R %lld / KC %lld / n %lld", R, kc, n);
  if (dtype != 1 && dtype != 2)
    return bias_fail("colsum_multi: bad dtype %lld", dtype, 0, 0);
  double* part = (double*)ws;
  int grid;
#define LAUNCH_CS(KCV)                                                       \
  grid = tasks_grid(n * (KCV / 4), BLOCK);                                   \
  hipLaunchKernelGGL((k_colsum_multi<KCV>), dim3(grid), dim3(BLOCK), 0, s,   \
                     (const float*)M, (ll)n, part)
  switch (kc) {
    case 4: LAUNCH_CS(4); break;
    case 8: LAUNCH_CS(8); break;
    case 16: LAUNCH_CS(16); break;
    case 32: LAUNCH_CS(32); break;
    default:
      grid = tasks_grid(n, WAVES_PER_BLOCK);
      hipLaunchKernelGGL(k_colsum_multi_anyk, dim3(grid), dim3(BLOCK), 0, s,
                         (const float*)M, (ll)n, kc, part);
      break;
  }
#undef LAUNCH_CS
  if (dtype == 1)
    hipLaunchKernelGGL((k_colsum_finish<float>), dim3(1), dim3(BLOCK), 0, s,
                       part, grid, kc, R, (float*)tail, (double*)out64);
  else
    hipLaunchKernelGGL((k_colsum_finish<double>), dim3(1), dim3(BLOCK), 0, s,
                       part, grid, kc, R, (double*)tail, (double*)out64);
  return bias_launched("colsum_multi");
}

// ---------------------------------------------------------------------------
// Z[i, c] += coef * src[idx0 + c] in place on the padded [n, KC] flat.
// ---------------------------------------------------------------------------

// coef * b with the product rounded on its own (never fused into the add).
template <typename T>
__device__ __forceinline__ T bias_term(T coef, T b) {
#pragma clang fp contract(off)
  return coef * b;
}

// KC % 4 == 0, so a 16-B vector never straddles a row and n*KC has no vector
// tail; the column of a thread's vector is carried along the grid-stride loop
// as in k_at_margin_update_tasks and the R biases are read through the cache
// with guarded loads (no LDS staging: nothing caps R). Pad columns c >= R are
// stored back exactly as they were loaded.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_add_bias_cols(
    T* __restrict__ Z, double coef, const T* __restrict__ src, ll idx0, ll n,
    int R, int KC) {
  constexpr int VE = Vec16<T>::VE;
  const ll stride = (ll)gridDim.x * BLOCK;
  const ll gid = (ll)blockIdx.x * BLOCK + threadIdx.x;
  const ll nv = n * KC / VE;
  int c0 = (int)((gid * VE) % KC);
  const int dc = (int)((stride * VE) % KC);
  T add[VE];
  bool live[VE];
  auto terms = [&]() {
#pragma unroll
    for (int k = 0; k < VE; ++k) {
      live[k] = c0 + k < R;
      add[k] = live[k] ? bias_term<T>((T)coef, src[idx0 + c0 + k]) : (T)0;
    }
  };
  terms();
  for (ll i = gid; i < nv; i += stride) {
    T zv[VE];
    load16<T>(Z + i * VE, zv);
#pragma unroll
    for (int k = 0; k < VE; ++k)
      if (live[k]) zv[k] += add[k];
    store16<T>(Z + i * VE, zv);
    if (dc != 0) {
      c0 += dc;
      if (c0 >= KC) c0 -= KC;
      terms();
    }
  }
}

// src holds at least idx0 + R entries (checked by the caller).
extern "C" int agd_add_bias_cols(void* Z, double coef, const void* src,
                                 long long idx0, long long n, int R, int kc,
                                 int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (kc < 4 || (kc & 3) || R < 1 || R > kc || n < 0 || idx0 < 0 ||
      src == nullptr)
    return bias_fail("add_bias_cols: bad R %lld / KC %lld / n %lld", R, kc, n);
  const int grid = bias_grid(n * kc / (dtype == 2 ? 2 : 4), BLOCK);
  if (dtype == 1)
    hipLaunchKernelGGL((k_add_bias_cols<float>), dim3(grid), dim3(BLOCK), 0, s,
                       (float*)Z, coef, (const float*)src, (ll)idx0, (ll)n, R,
                       kc);
  else if (dtype == 2)
    hipLaunchKernelGGL((k_add_bias_cols<double>), dim3(grid), dim3(BLOCK), 0,
                       s, (double*)Z, coef, (const double*)src, (ll)idx0,
                       (ll)n, R, kc);
  else
    return bias_fail("add_bias_cols: bad dtype %lld", dtype, 0, 0);
  return bias_launched("add_bias_cols");
}

// ---------------------------------------------------------------------------
// k_at_margin_update_tasks with the free-row correction of
// k_at_margin_update_off, per column.
// ---------------------------------------------------------------------------

// pz_c = 1 - step*lam[c] and 1 - pz_c in f64 as the host rounds them (product
// and differences separately; k_at_margin_update_tasks' task_shrink).
__device__ __forceinline__ void task_shrink_pair(double step, double lam,
                                                 double& pz, double& omp) {
#pragma clang fp contract(off)
  const double p = step * lam;
  pz = 1.0 - p;
  omp = 1.0 - pz;
}

// One element, the fma forms of k_at_margin_update_tasks' at_update_elem
// spelled out, with the free-row term folded in by one more fma:
//   zn = fma(c, zb, fma(pz, zo, pg*g))     xn = fma(1-th, xo, th*zn)
// c == 0 (lam == 0) or zb == 0 leaves the inner fma's value as it is, so the
// result is then bitwise that kernel's. Three roundings for zn, two for xn.
template <typename T>
__device__ __forceinline__ void at_update_off_elem(T tpz, T tc, T zb, T tpg,
                                                   T tom, T tth, T zo, T xo,
                                                   T gv, T& zn, T& xn) {
#pragma clang fp contract(off)
  const T pg_g = tpg * gv;
  const T z0 = fma(tpz, zo, pg_g);
  zn = fma(tc, zb, z0);
  const T th_z = tth * zn;
  xn = fma(tom, xo, th_z);
}

// With a free (unpenalised) bias row the prox maps column c of z = [Z; b^T]
// to [pz_c*Z_c - step*G_c ; b_c - step*g_b,c], and with zm = A.Z + 1.b^T,
// gm = A.G + 1.g_b^T
//   zm'[:, c] = pz_c*zm[:, c] - step*gm[:, c] + (1 - pz_c)*z_b[c]
//   xm'       = (1 - theta)*xm + theta*zm'
// z_b[c] = z_old[idx0 + c] is read on the device. Pad columns c >= R of both
// outputs are exact zeros whatever the inputs hold there. The loop, the
// carried column and the guarded coefficient loads are those of
// k_at_margin_update_tasks.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_at_margin_update_tasks_off(
    const T* __restrict__ zm_old, const T* __restrict__ xm_old,
    const T* __restrict__ gm, double step, const double* __restrict__ lam,
    double theta, const T* __restrict__ z_old, ll idx0, ll n, int R, int KC,
    T* __restrict__ zm_new, T* __restrict__ xm_new) {
  constexpr int VE = Vec16<T>::VE;
  const T tpg = (T)(-step), tth = (T)theta, tom = (T)(1.0 - theta);
  const ll stride = (ll)gridDim.x * BLOCK;
  const ll gid = (ll)blockIdx.x * BLOCK + threadIdx.x;
  const ll nv = n * KC / VE;
  int c0 = (int)((gid * VE) % KC);
  const int dc = (int)((stride * VE) % KC);
  T tpz[VE], tc[VE], zb[VE];
  bool live[VE];
  auto coeffs = [&]() {
#pragma unroll
    for (int k = 0; k < VE; ++k) {
      live[k] = c0 + k < R;
      double pz = 0.0, omp = 0.0;
      if (live[k]) task_shrink_pair(step, lam[c0 + k], pz, omp);
      tpz[k] = (T)pz;
      tc[k] = (T)omp;
      zb[k] = live[k] ? z_old[idx0 + c0 + k] : (T)0;
    }
  };
  coeffs();
  for (ll i = gid; i < nv; i += stride) {
    T zo[VE], xo[VE], gv[VE], zn[VE], xn[VE];
    load16<T>(zm_old + i * VE, zo);
    load16<T>(xm_old + i * VE, xo);
    load16<T>(gm + i * VE, gv);
#pragma unroll
    for (int k = 0; k < VE; ++k) {
      at_update_off_elem(tpz[k], tc[k], zb[k], tpg, tom, tth, zo[k], xo[k],
                         gv[k], zn[k], xn[k]);
      if (!live[k]) zn[k] = xn[k] = (T)0;
    }
    store16<T>(zm_new + i * VE, zn);
    store16<T>(xm_new + i * VE, xn);
    if (dc != 0) {
      c0 += dc;
      if (c0 >= KC) c0 -= KC;
      coeffs();
    }
  }
}

// lam is f64[R] device; z_old holds at least idx0 + R entries of the
// margins' dtype; the margins are [n * kc] with kc % 4 == 0, R <= kc.
extern "C" int agd_at_margin_update_tasks_off(
    const void* zm_old, const void* xm_old, const void* gm, double step,
    const void* lam, double theta, const void* z_old, long long idx0,
    long long n, int R, int kc, int dtype, void* zm_new, void* xm_new,
    void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (kc < 4 || (kc & 3) || R < 1 || R > kc || n < 0 || idx0 < 0 ||
      lam == nullptr || z_old == nullptr)
    return bias_fail("at_margin_update_tasks_off: bad R %lld / KC %lld / n %lld",
                     R, kc, n);
  const int grid = bias_grid(n * kc / (dtype == 2 ? 2 : 4), BLOCK);
  if (dtype == 1)
    hipLaunchKernelGGL((k_at_margin_update_tasks_off<float>), dim3(grid),
                       dim3(BLOCK), 0, s, (const float*)zm_old,
                       (const float*)xm_old, (const float*)gm, step,
                       (const double*)lam, theta, (const float*)z_old,
                       (ll)idx0, (ll)n, R, kc, (float*)zm_new, (float*)xm_new);
  else if (dtype == 2)
    hipLaunchKernelGGL((k_at_margin_update_tasks_off<double>), dim3(grid),
                       dim3(BLOCK), 0, s, (const double*)zm_old,
                       (const double*)xm_old, (const double*)gm, step,
                       (const double*)lam, theta, (const double*)z_old,
                       (ll)idx0, (ll)n, R, kc, (double*)zm_new,
                       (double*)xm_new);
  else
    return bias_fail("at_margin_update_tasks_off: bad dtype %lld", dtype, 0, 0);
  return bias_launched("at_margin_update_tasks_off");
}

// ---------------------------------------------------------------------------
// k_prox_tasks whose last n_free elements are free.
// ---------------------------------------------------------------------------

// w - step*g with the product rounded in T (the plain step of a free element,
// whatever the prox kind).
template <typename T>
__device__ __forceinline__ T free_step(T wi, T gi, T ts) {
#pragma clang fp contract(off)
  const T p = ts * gi;
  return wi - p;
}

// w is the flat feature-major [(d+1), R] block: element j < n - n_free
// belongs to task j % R and takes prox_elem with (lam[r], lam2[r]), exactly
// as in k_prox_tasks (same loop, same carried task index); the last n_free
// elements (the bias row: n_free = R) take the plain step and add nothing to
// the regularisation value. The first free element may sit in the 16-B body
// or in the scalar tail, so both test the element index (k_prox_free). Each
// block leaves one f64 partial of the regularisation value.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_prox_tasks_free(
    int kind, const T* __restrict__ w, const T* __restrict__ g, double step,
    const double* __restrict__ lam, const double* __restrict__ lam2, int R,
    T* __restrict__ out, double* __restrict__ reg_part, ll n, ll n_free) {
  constexpr int VE = Vec16<T>::VE;
  const ll stride = (ll)gridDim.x * BLOCK;
  const ll gid = (ll)blockIdx.x * BLOCK + threadIdx.x;
  const T ts = (T)step;
  const ll n_reg = n - n_free;  // elements [0, n_reg) are regularised
  double racc = 0.0;
  const ll nv = n / VE;
  int r0 = (int)((gid * VE) % R);
  const int dr = (int)((stride * VE) % R);
  for (ll i = gid; i < nv; i += stride) {
    T wv[VE], gv[VE], ov[VE];
    load16<T>(w + i * VE, wv);
    load16<T>(g + i * VE, gv);
    int r = r0;
#pragma unroll
    for (int k = 0; k < VE; ++k) {
      ov[k] = (i * VE + k < n_reg)
                  ? prox_elem(kind, wv[k], gv[k], ts, (T)lam[r], (T)lam2[r],
                              racc)
                  : free_step(wv[k], gv[k], ts);
      if (++r == R) r = 0;
    }
    store16<T>(out + i * VE, ov);
    r0 += dr;
    if (r0 >= R) r0 -= R;
  }
  const ll t = nv * VE + gid;
  if (t < n) {
    const int r = (int)(t % R);
    out[t] = (t < n_reg) ? prox_elem(kind, w[t], g[t], ts, (T)lam[r],
                                     (T)lam2[r], racc)
                         : free_step(w[t], g[t], ts);
  }
  if (kind != PROX_SIMPLE) {
    __shared__ double lds[WAVES_PER_BLOCK];
    racc = wave_reduce_sum(racc);
    if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x / WAVE] = racc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double v = lds[0];
#pragma unroll
      for (int wv = 1; wv < WAVES_PER_BLOCK; ++wv) v += lds[wv];
      reg_part[blockIdx.x] = v;
    }
  }
}

// One-block sum of the per-block partials in fixed order; OVERWRITES out[0].
__global__ __launch_bounds__(BLOCK) void k_sum_block_partials(
    const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  __shared__ double lds[WAVES_PER_BLOCK];
  double a = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += BLOCK) a += part[b];
  a = wave_reduce_sum(a);
  if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x / WAVE] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = lds[0];
#pragma unroll
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) v += lds[w];
    out[0] = v;
  }
}

// reg (f64[1]) is overwritten for every kind but the simple one, which
// leaves it as the caller set it; lam / lam2 are f64[R] device; red_ws holds
// at least 8192 doubles.
extern "C" int agd_prox_tasks_free(int kind, const void* w, const void* g,
                                   double step, const void* lam,
                                   const void* lam2, int R, void* out,
                                   void* reg, long long n, long long n_free,
                                   int dtype, void* red_ws, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (R < 1 || lam == nullptr || lam2 == nullptr)
    return bias_fail("prox_tasks_free: bad R %lld or null lambdas", R, 0, 0);
  if (n_free < 0 || n_free > n)
    return bias_fail("prox_tasks_free: n_free %lld outside [0, %lld]", n_free,
                     n, 0);
  if (kind < PROX_SIMPLE || kind > PROX_ELASTIC)
    return bias_fail("prox_tasks_free: bad kind %lld", kind, 0, 0);
  const int grid = bias_grid(n, BLOCK * 4);
  if (dtype == 1)
    hipLaunchKernelGGL((k_prox_tasks_free<float>), dim3(grid), dim3(BLOCK), 0,
                       s, kind, (const float*)w, (const float*)g, step,
                       (const double*)lam, (const double*)lam2, R, (float*)out,
                       (double*)red_ws, (ll)n, (ll)n_free);
  else if (dtype == 2)
    hipLaunchKernelGGL((k_prox_tasks_free<double>), dim3(grid), dim3(BLOCK), 0,
                       s, kind, (const double*)w, (const double*)g, step,
                       (const double*)lam, (const double*)lam2, R,
                       (double*)out, (double*)red_ws, (ll)n, (ll)n_free);
  else
    return bias_fail("prox_tasks_free: bad dtype %lld", dtype, 0, 0);
  if (kind != PROX_SIMPLE)
    hipLaunchKernelGGL(k_sum_block_partials, dim3(1), dim3(BLOCK), 0, s,
                       (const double*)red_ws, grid, (double*)reg);
  return bias_launched("prox_tasks_free");
}
