// Row-sampled mini-batch passes: both data passes of an SGD step over a
// compacted list of the sampled rows, so that a step at fraction f streams
// about 2f of the shard instead of 1 + f.
//
//   k_compact_*            uint8 mask [n] -> ascending int32 row list + its
//                          length, both in device memory (no atomics)
//   k_dense_margins_rows   part[s*cap + i] = <A[rows[i], slab s], w[slab s]>
//   k_multiplier_rows      slab sum, gathered labels / weights, loss_mult,
//                          compact multiplier, {loss, count, sum of mult}
//   k_dense_grad_rows      part[rb, c] = sum_{i in rb} m[i] * A[rows[i], c]
//
// The list length never reaches the host: every kernel reads it from device
// memory and sizes its own task loop with it, and the host plans grids, slabs
// and row blocks from the expected length. All kernels are atomics-free and
// bitwise reproducible. Design and resource figures: docs/KERNELS.md
// "Row-sampled mini-batch passes".
//
// A translation unit of its own, linked into libagd_hip.so next to
// agd_kernels.hip, whose error string, k_grad_reduce and k_add_bias it uses
// through host helpers.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "agd_stream.h"

extern "C" void agd_set_last_error(const char* msg);
extern "C" int agd_grad_reduce_f32(const void* part, long long n_rb,
                                   long long len, void* out, void* stream);
extern "C" int agd_grad_reduce_f64(const void* part, long long n_rb,
                                   long long len, void* out, void* stream);
extern "C" int agd_add_bias(void* margins, double coef, const void* src,
                            long long idx, long long n, int dtype,
                            void* stream);

static int rows_fail(const char* fmt, long long a, long long b, long long c) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  agd_set_last_error(buf);
  return 2;
}

static int rows_launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  agd_set_last_error(buf);
  return 1;
}

// Grid of the grid-stride kernels (the cap of agd_kernels.hip's grid_for).
static inline int rows_grid(ll work_items, ll per_block) {
  ll g = (work_items + per_block - 1) / per_block;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------------------
// Mask compaction. A thread owns 16 adjacent mask bytes (one 16-B load), a
// block 4096. Three launches: per-block counts, a one-block exclusive scan of
// the counts (which also leaves the list length), and the scatter, which
// recomputes the thread prefixes from the mask (n bytes, read twice) instead
// of storing n / 16 offsets. Thread order == row order at every level, so the
// list is ascending and the same on every run.
// ---------------------------------------------------------------------------

#define COMPACT_BYTES 16
#define COMPACT_PER_BLOCK (BLOCK * COMPACT_BYTES)

// Bit k is set when mask[base + k] is non-zero (k < 16, base + k < n).
__device__ __forceinline__ unsigned compact_bits(
    const unsigned char* __restrict__ mask, ll base, ll n) {
  unsigned bits = 0;
  if (base + COMPACT_BYTES <= n) {
    using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
    const u32x4 v = *(const u32x4*)(mask + base);
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if ((v[ch] >> (8 * b)) & 0xffu) bits |= 1u << (ch * 4 + b);
  } else {  // scalar tail of the mask (and threads past it: no bytes)
    for (int k = 0; k < COMPACT_BYTES; ++k)
      if (base + k < n && mask[base + k]) bits |= 1u << k;
  }
  return bits;
}

// Exclusive prefix of v in thread order, and the block total: a wave prefix
// by shuffles, the four wave totals through LDS.
__device__ __forceinline__ int block_excl_scan(int v, int& total) {
  __shared__ int wsum[WAVES_PER_BLOCK];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  int inc = v;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int t = __shfl_up(inc, off, WAVE);
    if (lane >= off) inc += t;
  }
  if (lane == WAVE - 1) wsum[wid] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < WAVES_PER_BLOCK; ++k) {
    const int s = wsum[k];
    if (k < wid) before += s;
    total += s;
  }
  __syncthreads();  // wsum is written again by the caller's next round
  return before + inc - v;
}

__global__ __launch_bounds__(BLOCK) void k_compact_count(
    const unsigned char* __restrict__ mask, ll n, int* __restrict__ btot) {
  const ll base = ((ll)blockIdx.x * BLOCK + threadIdx.x) * COMPACT_BYTES;
  int total;
  block_excl_scan(__popc(compact_bits(mask, base, n)), total);
  if (threadIdx.x == 0) btot[blockIdx.x] = total;
}

// In place: ws[b] = sum of ws[0 .. b-1]; count[0] = the sum of all. One
// block, BLOCK totals per round with a running carry.
__global__ __launch_bounds__(BLOCK) void k_compact_scan(int* __restrict__ ws,
                                                        ll nblk,
                                                        int* __restrict__ count) {
  int carry = 0;
  for (ll b0 = 0; b0 < nblk; b0 += BLOCK) {
    const ll b = b0 + threadIdx.x;
    const int v = (b < nblk) ? ws[b] : 0;
    int total;
    const int ex = block_excl_scan(v, total);
    if (b < nblk) ws[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) count[0] = carry;
}

__global__ __launch_bounds__(BLOCK) void k_compact_scatter(
    const unsigned char* __restrict__ mask, ll n, const int* __restrict__ boff,
    int* __restrict__ rows) {
  const ll base = ((ll)blockIdx.x * BLOCK + threadIdx.x) * COMPACT_BYTES;
  unsigned bits = compact_bits(mask, base, n);
  int total;
  ll o = (ll)boff[blockIdx.x] + block_excl_scan(__popc(bits), total);
  while (bits) {  // ascending k
    rows[o++] = (int)(base + (__ffs(bits) - 1));
    bits &= bits - 1;
  }
}

static int compact_launch(const unsigned char* mask, ll n, int* rows,
                          int* count, int* scan_ws, hipStream_t s) {
  const ll nblk = (n + COMPACT_PER_BLOCK - 1) / COMPACT_PER_BLOCK;
  hipLaunchKernelGGL(k_compact_count, dim3((unsigned)nblk), dim3(BLOCK), 0, s,
                     mask, n, scan_ws);
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(BLOCK), 0, s, scan_ws, nblk,
                     count);
  hipLaunchKernelGGL(k_compact_scatter, dim3((unsigned)nblk), dim3(BLOCK), 0, s,
                     mask, n, (const int*)scan_ws, rows);
  return rows_launched("agd_compact_rows");
}

static int compact_args_ok(const char* who, const void* mask, ll n) {
  if (n < 1 || n > 0x7fffffffLL) {
    char buf[128];
    snprintf(buf, sizeof(buf), "%s: n=%lld outside [1, 2^31)", who, n);
    agd_set_last_error(buf);
    return 0;
  }
  if (!mask || ((uintptr_t)mask & 15)) {
    char buf[128];
    snprintf(buf, sizeof(buf), "%s: mask must be a 16-byte aligned pointer", who);
    agd_set_last_error(buf);
    return 0;
  }
  return 1;
}

// int32 entries of the scan workspace for a mask of n bytes.
extern "C" long long agd_compact_ws_ints(long long n) {
  return (n + COMPACT_PER_BLOCK - 1) / COMPACT_PER_BLOCK;
}

// rows [n] int32 (the first count[0] entries are written), count [1] int32.
extern "C" int agd_compact_rows(const void* mask, long long n, void* rows,
                                void* count, void* scan_ws, void* stream) {
  if (!compact_args_ok("agd_compact_rows", mask, n)) return 2;
  if (!rows || !count || !scan_ws)
    return rows_fail("agd_compact_rows: null output (n=%lld)", n, 0, 0);
  return compact_launch((const unsigned char*)mask, n, (int*)rows, (int*)count,
                        (int*)scan_ws, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// A·w over the list. A wave takes R listed rows x one column slab, as
// k_dense_margins does with R adjacent rows. The wave index goes through
// readfirstlane, so the task, the R list reads and the R row base pointers are
// scalar (SGPR pairs); a lane adds only its column offset. The rows of the
// last, short group are clamped to the last listed row: it is read again and
// its sums are dropped, which keeps one sweep for every group and reads
// nothing outside the list. Two sweeps per iteration keep 2R 16-byte loads
// per lane in flight (a listed row is a fresh DRAM page, so a wave has no
// neighbour row to ride on); the single-sweep loop finishes the slab. With
// W > 1 the row length and every slab edge are multiples of W, so there is
// no partial lane load; W = 1 serves unaligned shapes.
// ---------------------------------------------------------------------------

template <typename TA>
constexpr int rows_per_wave() {
  return sizeof(TA) == 1 ? 8 : 4;  // fp8: w bytes would match the A bytes at 4
}

template <typename TA, typename TACC, int W, bool NT>
__global__ __launch_bounds__(BLOCK) void k_dense_margins_rows(
    const TA* __restrict__ A, const TACC* __restrict__ w,
    const int* __restrict__ rows, const int* __restrict__ count, ll d, ll cap,
    ll slab_w, int n_slabs, TACC* __restrict__ part) {
  constexpr int R = rows_per_wave<TA>();
  constexpr ll SW = (ll)WAVE * W;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const ll cnt = count[0];
  const ll wave_gid = (ll)blockIdx.x * WAVES_PER_BLOCK + wid;
  const ll n_waves = (ll)gridDim.x * WAVES_PER_BLOCK;
  const ll n_tasks = ((cnt + R - 1) / R) * n_slabs;
  for (ll t = wave_gid; t < n_tasks; t += n_waves) {
    const ll rg = t / n_slabs;
    const ll s = t - rg * n_slabs;
    const ll i0 = rg * R;
    const ll c_lo = s * slab_w;
    const ll c_hi = (c_lo + slab_w < d) ? c_lo + slab_w : d;
    const TA* __restrict__ rp[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const ll i = (i0 + j < cnt) ? i0 + j : cnt - 1;
      rp[j] = A + (ll)rows[i] * d;
    }
    TACC acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = (TACC)0;
    ll c = c_lo + (ll)lane * W;
    for (; c + SW + W <= c_hi; c += 2 * SW) {
      TACC v0[R][W], v1[R][W], w0[W], w1[W];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        loadW<TA, TACC, W, NT>(rp[j] + c, v0[j]);
        loadW<TA, TACC, W, NT>(rp[j] + c + SW, v1[j]);
      }
      loadAcc<TACC, W>(w + c, w0);
      loadAcc<TACC, W>(w + c + SW, w1);
#pragma unroll
      for (int j = 0; j < R; ++j)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[j] += v0[j][k] * w0[k];
#pragma unroll
      for (int j = 0; j < R; ++j)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[j] += v1[j][k] * w1[k];
    }
    for (; c + W <= c_hi; c += SW) {
      TACC v[R][W], wv[W];
#pragma unroll
      for (int j = 0; j < R; ++j) loadW<TA, TACC, W, NT>(rp[j] + c, v[j]);
      loadAcc<TACC, W>(w + c, wv);
#pragma unroll
      for (int j = 0; j < R; ++j)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[j] += v[j][k] * wv[k];
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      acc[j] = wave_reduce_sum(acc[j]);
      if (lane == 0 && i0 + j < cnt) part[s * cap + i0 + j] = acc[j];
    }
  }
}

// ---------------------------------------------------------------------------
// The multiplier over the compact margins: k_multiplier_sum with the slab
// sum of k_multiplier and gathered labels / weights. Every listed row is a
// sampled row, so loss and count are k_multiplier's under the mask; the third
// sum is the gradient of an intercept.
// ---------------------------------------------------------------------------

template <typename TACC>
__global__ __launch_bounds__(BLOCK) void k_multiplier_rows(
    const TACC* __restrict__ part, const int* __restrict__ rows,
    const int* __restrict__ count, const float* __restrict__ labels,
    const float* __restrict__ sample_weight, int loss_type, ll cap,
    int n_slabs, TACC* __restrict__ mult, double* __restrict__ red_part) {
  double lsum = 0.0, cnt = 0.0, msum = 0.0;
  const ll len = count[0];
  const ll stride = (ll)gridDim.x * BLOCK;
  for (ll i = (ll)blockIdx.x * BLOCK + threadIdx.x; i < len; i += stride) {
    TACC z = part[i];
    for (int s = 1; s < n_slabs; ++s) z += part[(ll)s * cap + i];
    const ll r = rows[i];
    const TACC y = (TACC)labels[r];
    TACC m, l;
    loss_mult<TACC>(loss_type, z, y, m, l);
    if (sample_weight) {
      const TACC sw = (TACC)sample_weight[r];
      const TACC ms = m * sw;
      mult[i] = ms;
      msum += (double)ms;
      lsum += (double)l * (double)sw;
      cnt += (double)sw;
    } else {
      mult[i] = m;
      msum += (double)m;
      lsum += (double)l;
      cnt += 1.0;
    }
  }
  double acc[3] = {lsum, cnt, msum};
  block_reduce_partial<3>(acc, red_part);
}

// ---------------------------------------------------------------------------
// Aᵀ·m over the list: k_dense_grad's split (thread per W adjacent columns,
// row-block x column-slab grid, private partial slabs), with the row blocks
// partitioning the LIST. i is block-uniform, so rows[i] and m[i] are scalar
// loads of consecutive words; four list entries are taken per iteration and
// their row loads issued together. A listed row with m == 0 (an inactive
// hinge row) is not read.
// ---------------------------------------------------------------------------

#define GRAD_ROWS_UNROLL 4

template <typename TA, typename TACC, int W, bool NT>
__global__ __launch_bounds__(BLOCK) void k_dense_grad_rows(
    const TA* __restrict__ A, const TACC* __restrict__ mult,
    const int* __restrict__ rows, const int* __restrict__ count, ll d, ll n_rb,
    TACC* __restrict__ part) {
  constexpr int U = GRAD_ROWS_UNROLL;
  const ll cols_per_block = (ll)BLOCK * W;
  const ll n_cs = (d + cols_per_block - 1) / cols_per_block;
  const ll cnt = count[0];
  for (ll b = blockIdx.x; b < n_rb * n_cs; b += gridDim.x) {
    const ll rb = b / n_cs;
    const ll cs = b - rb * n_cs;
    const ll i_lo = rb * cnt / n_rb;
    const ll i_hi = (rb + 1) * cnt / n_rb;
    const ll c0 = cs * cols_per_block + (ll)threadIdx.x * W;
    if (c0 + W > d) continue;  // d % W == 0: a thread is whole or outside
    TACC acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = (TACC)0;
    ll i = i_lo;
    for (; i + U <= i_hi; i += U) {
      TACC m[U], v[U][W];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        m[u] = mult[i + u];
#pragma unroll
        for (int k = 0; k < W; ++k) v[u][k] = (TACC)0;
        if (m[u] != (TACC)0)  // block-uniform
          loadW<TA, TACC, W, NT>(A + (ll)rows[i + u] * d + c0, v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] += m[u] * v[u][k];
    }
    for (; i < i_hi; ++i) {
      const TACC m = mult[i];
      if (m == (TACC)0) continue;
      TACC v[W];
      loadW<TA, TACC, W, NT>(A + (ll)rows[i] * d + c0, v);
#pragma unroll
      for (int k = 0; k < W; ++k) acc[k] += m * v[k];
    }
    TACC* __restrict__ dst = part + rb * d + c0;
#pragma unroll
    for (int k = 0; k < W; ++k) dst[k] = acc[k];
  }
}

// ---------------------------------------------------------------------------
// Host API
// ---------------------------------------------------------------------------

static inline int rows_wfull(int dtype) {
  return (dtype == 3) ? 16 : (dtype == 0) ? 8 : (dtype == 1) ? 4 : 2;
}

// Column slabs of the list margins pass for an expected list length: the
// full pass's rule (about 16384 wave tasks, slabs of at least four sweeps)
// on the listed rows, so a sampled pass splits columns long before the full
// pass over the same shard would. The partials are n_slabs * n accumulators
// (the list may be the whole shard), kept under 512 MiB.
extern "C" int agd_rows_margin_slabs(long long expected, long long n,
                                     long long d, int a_dtype) {
  const int r = (a_dtype == 3) ? 8 : 4;
  if (expected < 1) expected = 1;
  const ll n_units = (expected + r - 1) / r;
  const ll target = 16384;
  if (n_units >= target) return 1;
  const int w = (d % rows_wfull(a_dtype) == 0) ? rows_wfull(a_dtype) : 1;
  const ll min_slab = (ll)WAVE * w * 4;
  const ll max_slabs = (d + min_slab - 1) / min_slab;
  ll s = (target + n_units - 1) / n_units;
  if (s > max_slabs) s = max_slabs;
  if (s > 1024) s = 1024;
  const ll acc_bytes = (a_dtype == 2) ? 8 : 4;
  while (s > 1 && s * n * acc_bytes > (512LL << 20)) s /= 2;
  return (int)(s < 1 ? 1 : s);
}

// Row blocks of the list gradient pass: agd_dense_rowblocks on the expected
// list length.
extern "C" long long agd_rows_rowblocks(long long expected, long long d,
                                        int a_dtype) {
  const int w = (d % rows_wfull(a_dtype) == 0) ? rows_wfull(a_dtype) : 1;
  const ll cols_per_block = (ll)BLOCK * w;
  const ll n_cs = (d + cols_per_block - 1) / cols_per_block;
  ll n_rb = 4096 / n_cs;
  if (n_rb < 1) n_rb = 1;
  if (n_rb > expected) n_rb = expected;
  if (n_rb < 1) n_rb = 1;
  const ll acc_bytes = (a_dtype == 2) ? 8 : 4;
  while (n_rb > 1 && n_rb * d * acc_bytes > (512LL << 20)) n_rb /= 2;
  return n_rb;
}

struct RowsArgs {
  const void* A;
  const float* labels;
  const unsigned char* mask;
  const float* sample_weight;
  const void* w;
  ll n, d, expected;
  void* grad;
  double* out3;
  int* rows;
  int* count;
  int* scan_ws;
  void* margins;
  void* mult;
  void* part;
  ll n_rb;
  int loss_type, n_slabs, need_grad, nt_loads;
  const void* bias_src;
  ll bias_idx;
  double* red_ws;
  hipStream_t stream;
};

template <typename TA, typename TACC, int W>
static int rows_eval_t(const RowsArgs& a) {
  const TA* A = (const TA*)a.A;
  const TACC* w = (const TACC*)a.w;
  TACC* margins = (TACC*)a.margins;
  TACC* mult = (TACC*)a.mult;
  TACC* grad = (TACC*)a.grad;
  const ll n = a.n, d = a.d, cap = a.n;
  hipStream_t s = a.stream;
  constexpr int R = rows_per_wave<TA>();

  int rc = compact_launch(a.mask, n, a.rows, a.count, a.scan_ws, s);
  if (rc) return rc;

  int n_slabs = a.n_slabs;
  ll slab_w = d;
  if (n_slabs > 1) {  // whole sweeps per slab, as in the full pass
    const ll align = (ll)WAVE * W;
    slab_w = (d + n_slabs - 1) / n_slabs;
    slab_w = ((slab_w + align - 1) / align) * align;
    n_slabs = (int)((d + slab_w - 1) / slab_w);
  }
  {
    const ll tasks = ((a.expected + R - 1) / R) * n_slabs;
    const int grid = rows_grid(tasks, WAVES_PER_BLOCK);
    if (a.nt_loads)
      hipLaunchKernelGGL((k_dense_margins_rows<TA, TACC, W, true>), dim3(grid),
                         dim3(BLOCK), 0, s, A, w, (const int*)a.rows,
                         (const int*)a.count, d, cap, slab_w, n_slabs, margins);
    else
      hipLaunchKernelGGL((k_dense_margins_rows<TA, TACC, W, false>), dim3(grid),
                         dim3(BLOCK), 0, s, A, w, (const int*)a.rows,
                         (const int*)a.count, d, cap, slab_w, n_slabs, margins);
  }
  if (a.bias_src) {  // onto slab 0; the slab sum carries it into the margin
    rc = agd_add_bias(margins, 1.0, a.bias_src, a.bias_idx, cap,
                      sizeof(TACC) == 8 ? 2 : 1, (void*)s);
    if (rc) return rc;
  }
  {
    const int grid = rows_grid(a.expected, BLOCK);
    hipLaunchKernelGGL((k_multiplier_rows<TACC>), dim3(grid), dim3(BLOCK), 0, s,
                       (const TACC*)margins, (const int*)a.rows,
                       (const int*)a.count, a.labels, a.sample_weight,
                       a.loss_type, cap, n_slabs, mult, a.red_ws);
    hipLaunchKernelGGL((k_reduce_partials<3>), dim3(1), dim3(BLOCK), 0, s,
                       (const double*)a.red_ws, grid, a.out3);
  }
  if (a.need_grad) {
    TACC* part = (a.n_rb == 1) ? grad : (TACC*)a.part;
    const ll cols_per_block = (ll)BLOCK * W;
    const ll n_cs = (d + cols_per_block - 1) / cols_per_block;
    const int grid = rows_grid(a.n_rb * n_cs, 1);
    if (a.nt_loads)
      hipLaunchKernelGGL((k_dense_grad_rows<TA, TACC, W, true>), dim3(grid),
                         dim3(BLOCK), 0, s, A, (const TACC*)mult,
                         (const int*)a.rows, (const int*)a.count, d, a.n_rb,
                         part);
    else
      hipLaunchKernelGGL((k_dense_grad_rows<TA, TACC, W, false>), dim3(grid),
                         dim3(BLOCK), 0, s, A, (const TACC*)mult,
                         (const int*)a.rows, (const int*)a.count, d, a.n_rb,
                         part);
    if (a.n_rb > 1) {
      rc = (sizeof(TACC) == 8)
               ? agd_grad_reduce_f64(part, a.n_rb, d, grad, (void*)s)
               : agd_grad_reduce_f32(part, a.n_rb, d, grad, (void*)s);
      if (rc) return rc;
    }
  }
  return rows_launched("agd_dense_eval_rows");
}

// compact -> margins -> (bias) -> multiplier -> gradient -> reduce over the
// rows with mask[r] != 0, on the caller's stream, no host synchronisation.
//   rows_ws [n] int32, count_ws [1] int32, scan_ws [agd_compact_ws_ints(n)]
//   margins_ws [n_slabs * n], mult_ws [n] accumulators (compact: entry i
//   belongs to row rows_ws[i]); part_ws [n_rb * d] when n_rb > 1
//   out3 [3] f64 = {loss, count, sum of mult}, zeroed by the caller
//   expected: the list length the grids are planned for (any list length is
//   served); bias_src / bias_idx: optional intercept, read on the device.
extern "C" int agd_dense_eval_rows(
    const void* A, int a_dtype, const void* labels, const void* mask,
    const void* sample_weight, const void* w, long long n, long long d,
    long long expected, void* grad_out, void* out3, void* rows_ws,
    void* count_ws, void* scan_ws, void* margins_ws, void* mult_ws,
    void* part_ws, long long n_rb, int loss_type, int n_slabs, int need_grad,
    int nt_loads, const void* bias_src, long long bias_idx, void* red_ws,
    void* stream) {
  if (!compact_args_ok("agd_dense_eval_rows", mask, n)) return 2;
  if (d < 1 || n_slabs < 1 || n_slabs > 1024 || n_rb < 1 || n_rb > 8192)
    return rows_fail("agd_dense_eval_rows: bad plan d=%lld n_slabs=%lld "
                     "n_rb=%lld", d, n_slabs, n_rb);
  if (a_dtype < 0 || a_dtype > 3)
    return rows_fail("agd_dense_eval_rows: bad dtype %lld", a_dtype, 0, 0);
  if (loss_type < 0 || loss_type > 3)
    return rows_fail("agd_dense_eval_rows: bad loss %lld", loss_type, 0, 0);
  if (!A || !labels || !w || !out3 || !rows_ws || !count_ws || !scan_ws ||
      !margins_ws || !mult_ws || !red_ws || (need_grad && !grad_out) ||
      (need_grad && n_rb > 1 && !part_ws))
    return rows_fail("agd_dense_eval_rows: null buffer (n=%lld d=%lld)", n, d,
                     0);
  if (expected < 1) expected = 1;
  if (expected > n) expected = n;
  RowsArgs a{A, (const float*)labels, (const unsigned char*)mask,
             (const float*)sample_weight, w, n, d, expected, grad_out,
             (double*)out3, (int*)rows_ws, (int*)count_ws, (int*)scan_ws,
             margins_ws, mult_ws, part_ws, n_rb, loss_type, n_slabs, need_grad,
             nt_loads, bias_src, bias_idx, (double*)red_ws,
             (hipStream_t)stream};
  // 16-byte lane loads need whole W-groups per row and aligned bases
  const bool vec = (d % rows_wfull(a_dtype) == 0) &&
                   !((uintptr_t)A & 15) && !((uintptr_t)w & 15);
  switch (a_dtype * 10 + (vec ? 1 : 0)) {
    case 1:  return rows_eval_t<ubf16, float, 8>(a);
    case 0:  return rows_eval_t<ubf16, float, 1>(a);
    case 11: return rows_eval_t<float, float, 4>(a);
    case 10: return rows_eval_t<float, float, 1>(a);
    case 21: return rows_eval_t<double, double, 2>(a);
    case 20: return rows_eval_t<double, double, 1>(a);
    case 31: return rows_eval_t<unsigned char, float, 16>(a);
    default: return rows_eval_t<unsigned char, float, 1>(a);
  }
}
