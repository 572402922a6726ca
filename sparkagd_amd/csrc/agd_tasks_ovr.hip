// One-vs-rest task multipliers: the multi-task n-space stage with a target
// class per column. Column r of row i is one binary problem with the label
//   y_ir = [int(label_i) == target[r]],
// label_i being the shard's float class index (as on the softmax path), so K
// one-vs-rest models, or K x folds x lambdas of them, train as the columns of
// one [d, R] block in one stream of the shard.
//
// The kernels are siblings of k_multiplier_tasks / k_multiplier_tasks_anyk
// (agd_kernels.hip) and share the per-group evaluation, agd_tasks.h's
// tasks_group, with them: the work split, the 16-B accesses, loss_mult, the
// f64 partial layout [blocks][KC + 1] and the finish (k_reduce_task_partials)
// are the same, which is what makes a column bitwise equal to the binary
// kernel run on the relabelled vector. (The loops are written out here and
// not shared as one device function: wrapping the existing kernels' bodies
// changes their register allocation, and their code is to stay as it is.) What is
// added per thread: the four targets of its column group, read once through
// the cache next to holdout and scale (once per 256-column chunk in the
// any-K kernel; never staged in LDS, so no LDS budget caps R); per row, one
// float->int convert of the label and four integer compares.
//
// A translation unit of its own, compiled with
//   -Xclang -target-feature -Xclang -packed-fp32-ops
// and linked into libagd_hip.so next to agd_kernels.hip, which it reaches
// through the two host helpers declared below.

#include <hip/hip_runtime.h>

#include <cstdio>

#include "agd_tasks.h"

// agd_kernels.hip: the library's error string and the one-block finish.
extern "C" void agd_set_last_error(const char* msg);
extern "C" int agd_tasks_finish(void* ws, int grid, int kc, int R,
                                const void* task_scale, void* task_loss,
                                void* loss_count, void* stream);

// KC in {4, 8, 16, 32}: the work split of k_multiplier_tasks<KC>. A thread
// keeps ONE 4-column group for its whole grid-stride loop (the stride is a
// multiple of KC/4), so its four targets are loaded once, with holdout and
// scale; per-thread state is 4 f64 loss partials whatever KC is.
template <int KC>
__global__ __launch_bounds__(BLOCK) void k_multiplier_tasks_ovr(
    const float* __restrict__ Z, const float* __restrict__ labels,
    const unsigned char* __restrict__ mask,
    const float* __restrict__ sample_weight, const int* __restrict__ fold_id,
    const int* __restrict__ holdout, const float* __restrict__ task_scale,
    const int* __restrict__ target, int loss_type, int invert, ll n, int R,
    float* __restrict__ M, double* __restrict__ part,
    double* __restrict__ cnt_part) {
  constexpr int G4 = KC / 4;
  static_assert(BLOCK % G4 == 0 && WAVE % G4 == 0, "column group must tile");
  const ll gid = (ll)blockIdx.x * BLOCK + threadIdx.x;
  const int c0 = (int)(threadIdx.x % G4) * 4;
  int h[4], tg[4];
  float sc[4];
  bool live[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = c0 + j;
    live[j] = r < R;
    h[j] = (live[j] && holdout) ? holdout[r] : -1;
    sc[j] = live[j] ? task_scale[r] : 0.f;
    tg[j] = live[j] ? target[r] : -1;
  }
  double ls[4] = {0.0, 0.0, 0.0, 0.0};
  double cnt = 0.0;
  const ll ngroups = n * G4;
  const ll stride = (ll)gridDim.x * BLOCK;
  for (ll g = gid; g < ngroups; g += stride) {
    const ll i = g / G4;
    float* mp = M ? M + g * 4 : nullptr;
    if (mask && !mask[i]) {
      using f32x4 = __attribute__((ext_vector_type(4))) float;
      if (mp) *(f32x4*)mp = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const float s = sample_weight ? sample_weight[i] : 1.0f;
    // no fold vector: no row is in any fold (never equals a holdout, -1 too)
    const int f = fold_id ? fold_id[i] : -2;
    if (c0 == 0) cnt += (double)s;
    tasks_group<true>(Z + g * 4, labels[i], s, f, loss_type, invert, h, sc,
                      live, tg, mp, ls);
  }
  // lanes with equal (lane % G4) own the same columns: the xor tree stops
  // at G4, then a 4-term LDS sum per column
  __shared__ double lds[WAVES_PER_BLOCK][KC];
  __shared__ double ldc[WAVES_PER_BLOCK];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double v = ls[j];
#pragma unroll
    for (int off = 32; off >= G4; off >>= 1) v += __shfl_xor(v, off, WAVE);
    if (lane < G4) lds[wid][lane * 4 + j] = v;
  }
  cnt = wave_reduce_sum(cnt);
  if (lane == 0) ldc[wid] = cnt;
  __syncthreads();
  if (threadIdx.x < KC) {
    double v = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) v += lds[w][threadIdx.x];
    part[(ll)blockIdx.x * KC + threadIdx.x] = v;
  }
  if (threadIdx.x == 0) {
    double v = ldc[0];
#pragma unroll
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) v += ldc[w];
    cnt_part[blockIdx.x] = v;
  }
}

// Any 4-aligned KC (> 32 in practice): the work split of
// k_multiplier_tasks_anyk. One wave per row, lane l owns the column group at
// chunk + 4l; the column axis is walked in chunks of 256, and a lane reloads
// its four targets (with holdout and scale) once per chunk.
__global__ __launch_bounds__(BLOCK) void k_multiplier_tasks_ovr_anyk(
    const float* __restrict__ Z, const float* __restrict__ labels,
    const unsigned char* __restrict__ mask,
    const float* __restrict__ sample_weight, const int* __restrict__ fold_id,
    const int* __restrict__ holdout, const float* __restrict__ task_scale,
    const int* __restrict__ target, int loss_type, int invert, ll n, int R,
    int KC, float* __restrict__ M, double* __restrict__ part,
    double* __restrict__ cnt_part) {
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  __shared__ double lds[WAVES_PER_BLOCK][TASKS_CHUNK];
  __shared__ double ldc[WAVES_PER_BLOCK];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const ll wave_gid = (ll)blockIdx.x * WAVES_PER_BLOCK + wid;
  const ll n_waves = (ll)gridDim.x * WAVES_PER_BLOCK;
  double cnt = 0.0;
  for (int chunk = 0; chunk < KC; chunk += TASKS_CHUNK) {
    const int c0 = chunk + lane * 4;
    const bool active = c0 < KC;  // KC % 4 == 0: the whole group is inside
    int h[4], tg[4];
    float sc[4];
    bool live[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = c0 + j;
      live[j] = active && r < R;
      h[j] = (live[j] && holdout) ? holdout[r] : -1;
      sc[j] = live[j] ? task_scale[r] : 0.f;
      tg[j] = live[j] ? target[r] : -1;
    }
    double ls[4] = {0.0, 0.0, 0.0, 0.0};
    for (ll i = wave_gid; i < n; i += n_waves) {
      float* mp = (M && active) ? M + i * KC + c0 : nullptr;
      if (mask && !mask[i]) {
        if (mp) *(f32x4*)mp = f32x4{0.f, 0.f, 0.f, 0.f};
        continue;
      }
      const float s = sample_weight ? sample_weight[i] : 1.0f;
      const int f = fold_id ? fold_id[i] : -2;
      if (chunk == 0 && lane == 0) cnt += (double)s;
      if (active)
        tasks_group<true>(Z + i * KC + c0, labels[i], s, f, loss_type, invert,
                          h, sc, live, tg, mp, ls);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) lds[wid][lane * 4 + j] = ls[j];
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
  cnt = wave_reduce_sum(cnt);
  if (lane == 0) ldc[wid] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = ldc[0];
#pragma unroll
    for (int w = 1; w < WAVES_PER_BLOCK; ++w) v += ldc[w];
    cnt_part[blockIdx.x] = v;
  }
}

static int ovr_fail(const char* fmt, int a, int b, long long c) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  agd_set_last_error(buf);
  return 2;
}

// agd_multiplier_tasks with per-column targets: target is i32[R] on the
// device, labels hold class indices. M may be null (loss-only call).
// task_loss f64[R] and loss_count f64[2] are overwritten. ws holds
// agd_tasks_ws_doubles(kc) doubles.
extern "C" int agd_multiplier_tasks_ovr(
    const void* Z, const void* labels, const void* mask,
    const void* sample_weight, const void* fold_id, const void* holdout,
    const void* task_scale, const void* target, int loss_type, int invert,
    long long n, int R, int kc, void* M, void* task_loss, void* loss_count,
    void* ws, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (kc < 4 || (kc & 3) || R < 1 || R > kc || n < 0)
    return ovr_fail("multiplier_tasks_ovr: bad R %d / KC %d / n %lld", R, kc, n);
  if (loss_type < 0 || loss_type > LOSS_SMOOTH_HINGE)
    return ovr_fail("multiplier_tasks_ovr: bad loss_type %d", loss_type, 0, 0);
  if (target == nullptr)
    return ovr_fail("multiplier_tasks_ovr: target is null", 0, 0, 0);
  double* part = (double*)ws;
  double* cnt_part = part + (ll)TASKS_MAX_GRID * kc;
  int grid;
#define LAUNCH_OVR(KCV)                                                       \
  grid = tasks_grid(n * (KCV / 4), BLOCK);                                    \
  hipLaunchKernelGGL((k_multiplier_tasks_ovr<KCV>), dim3(grid), dim3(BLOCK),  \
                     0, s, (const float*)Z, (const float*)labels,             \
                     (const unsigned char*)mask, (const float*)sample_weight, \
                     (const int*)fold_id, (const int*)holdout,                \
                     (const float*)task_scale, (const int*)target, loss_type, \
                     invert, (ll)n, R, (float*)M, part, cnt_part)
  switch (kc) {
    case 4: LAUNCH_OVR(4); break;
    case 8: LAUNCH_OVR(8); break;
    case 16: LAUNCH_OVR(16); break;
    case 32: LAUNCH_OVR(32); break;
    default:
      grid = tasks_grid(n, WAVES_PER_BLOCK);
      hipLaunchKernelGGL(k_multiplier_tasks_ovr_anyk, dim3(grid), dim3(BLOCK),
                         0, s, (const float*)Z, (const float*)labels,
                         (const unsigned char*)mask,
                         (const float*)sample_weight, (const int*)fold_id,
                         (const int*)holdout, (const float*)task_scale,
                         (const int*)target, loss_type, invert, (ll)n, R, kc,
                         (float*)M, part, cnt_part);
      break;
  }
#undef LAUNCH_OVR
  return agd_tasks_finish(ws, grid, kc, R, task_scale, task_loss, loss_count,
                          stream);
}
