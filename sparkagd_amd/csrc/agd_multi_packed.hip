// Multi-column MFMA kernels over the 12-bit packed copy of a bf16 shard:
//   Z[n, KC] = A·W   (k_margins_multi_pk)   and   G[d, KC] = Aᵀ·M
// (k_grad_multi_pk) for the multinomial softmax and multi-task (CV sweep)
// gradients, with their operand preparation and escape corrections. Both
// stream the packed rows (1.5 B/element) with nt 12-byte loads, decode
// straight to bf16 pairs and feed v_mfma_f32_32x32x16_bf16. Layouts and the
// lane/tile maps are in docs/KERNELS.md, "Packed multi-column MFMA kernels".
// The second half of the file is the same pair of passes over a raw fp8
// (e4m3fn) shard, k_margins_multi_f8 and k_grad_multi_f8 (docs/KERNELS.md,
// "fp8 multi-column MFMA kernels").
//
// A translation unit of its own: it is compiled with
//   -Xclang -target-feature -Xclang -packed-fp32-ops
// and linked into libagd_hip.so next to agd_kernels.hip, which it reaches
// through the three small host helpers declared below.
//
// Fragment layouts of the MFMA (benchmarks/mfma_probe.hip):
//   A operand: lane l holds row    l&31, k = 8·(l>>5) … +7
//   B operand: lane l holds column l&31, k = 8·(l>>5) … +7
//   acc[r]:    row (r&3) + 8·(r>>2) + 4·(l>>5), column l&31

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

typedef long long ll;
typedef unsigned short ubf16;

// agd_kernels.hip: the library's error string and its fixed-order reducers.
extern "C" void agd_set_last_error(const char* msg);
extern "C" int agd_grad_reduce_f32(const void* part, long long n_rb,
                                   long long len, void* out, void* stream);
extern "C" int agd_slab_reduce_f32(void* part, long long len, int n_slabs,
                                   void* stream);

#define MP_WAVE 64
#define MP_ROWS 32          // rows a margins wave owns
#define MP_GROUPS 32        // groups (of 8 columns) per step: 256 columns
#define MP_COLS (MP_GROUPS * 8)
#define MP_LDS_STRIDE 33    // 16-B units per staged row: 32 groups + 1 pad
#define MP_GRAD_ROWS 16     // rows a gradient wave step covers (the MFMA k)
#define MP_PREP_TILE 64

using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;
using f32x16_t = __attribute__((ext_vector_type(16))) float;
using u32x4_t = __attribute__((ext_vector_type(4))) unsigned int;
typedef unsigned int mp_u32x3 __attribute__((ext_vector_type(3), aligned(4)));

// Row stride of a packed shard in groups (agd_kernels.hip pk_row_groups).
__host__ __device__ __forceinline__ ll mp_row_groups(ll d) {
  return (((d >> 3) + MP_GROUPS - 1) / MP_GROUPS) * MP_GROUPS;
}

__device__ __forceinline__ float mp_bf2f(ubf16 u) {
  return __uint_as_float(((unsigned)u) << 16);
}

__device__ __forceinline__ ubf16 mp_f2bf_rne(float f) {
  const unsigned u = __float_as_uint(f);
  return (ubf16)((u + 0x7FFF + ((u >> 16) & 1)) >> 16);
}

// One packed group to four dwords of bf16 pairs (elements 2i, 2i+1 in dword
// i): the table/perm scheme of pk_decode_bits, but the last permutes build
// pairs, so there are four of them and not eight.
__device__ __forceinline__ u32x4_t mp_decode_pairs(const mp_u32x3 v,
                                                   unsigned lut_lo,
                                                   unsigned lut_hi) {
  const unsigned z = v[2];
  const unsigned hA =
      __builtin_amdgcn_perm(lut_hi, lut_lo, z & 0x07070707u) |
      ((z & 0x08080808u) << 4);
  const unsigned hB =
      __builtin_amdgcn_perm(lut_hi, lut_lo, (z >> 4) & 0x07070707u) |
      (z & 0x80808080u);
  u32x4_t o;
  o[0] = __builtin_amdgcn_perm(hA, v[0], 0x05010400u);
  o[1] = __builtin_amdgcn_perm(hA, v[0], 0x07030602u);
  o[2] = __builtin_amdgcn_perm(hB, v[1], 0x05010400u);
  o[3] = __builtin_amdgcn_perm(hB, v[1], 0x07030602u);
  return o;
}

__device__ __forceinline__ mp_u32x3 mp_load_group(const unsigned* __restrict__ p) {
  return __builtin_nontemporal_load((const mp_u32x3*)p);
}

// ---------------------------------------------------------------------------
// Operand preparation: columns col0 .. col0 + k_in of src [rows, src_ld] f32
// row-major (k_in <= 128) -> transposed bf16 planes [kc32, ld]: hi = bf16(x),
// lo = bf16(x - hi) (lo may be null).
// Everything outside rows x k_in is written as zero, so the stream kernels
// can run whole 32-class tiles and whole steps over the pad. A 64-row tile
// goes through LDS: the reads are contiguous in src, the writes contiguous
// along a plane row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mp_prep_planes(
    const float* __restrict__ src, ll src_ld, int col0, ll rows, int k_in,
    int kc32, ll ld, ubf16* __restrict__ hi, ubf16* __restrict__ lo) {
  __shared__ float tile[128][MP_PREP_TILE + 1];
  const ll n_tiles = (ld + MP_PREP_TILE - 1) / MP_PREP_TILE;
  for (ll t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const ll r0 = t * MP_PREP_TILE;
    const ll live = (rows - r0 < MP_PREP_TILE) ? rows - r0 : MP_PREP_TILE;
    __syncthreads();
    for (ll i = threadIdx.x; i < live * k_in; i += 256) {
      const int rr = (int)(i / k_in);
      const int cc = (int)(i - (ll)rr * k_in);
      tile[cc][rr] = src[(r0 + rr) * src_ld + col0 + cc];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kc32 * MP_PREP_TILE; i += 256) {
      const int c = i / MP_PREP_TILE, rr = i % MP_PREP_TILE;
      if (r0 + rr >= ld) continue;
      const float x = (c < k_in && rr < live) ? tile[c][rr] : 0.f;
      const ubf16 h = mp_f2bf_rne(x);
      hi[(ll)c * ld + r0 + rr] = h;
      if (lo) lo[(ll)c * ld + r0 + rr] = mp_f2bf_rne(x - mp_bf2f(h));
    }
  }
}

// ---------------------------------------------------------------------------
// Margins. One wave (one 64-thread block) owns 32 rows and one column slab.
// Per 256-column step:
//   * 16 nt 12-byte loads per lane: instruction i has the lower half-wave on
//     the 32 groups (384 contiguous bytes) of row 2i, the upper on row 2i+1;
//   * decode to bf16 pairs, one 16-byte LDS store per group into the wave's
//     tile [32 rows][33 x 16 B] (the pad unit makes the fragment reads below
//     conflict-free: consecutive rows start 4 banks apart);
//   * 16 A fragments read back as one 16-byte LDS load each (lane l: row
//     l&31, group 2j + (l>>5)); per fragment and 32-class tile two MFMAs,
//     against the hi and the lo plane of W, into the same accumulator.
// Rows past n are clamped (their accumulator rows are never stored); the
// zero groups that pad a packed row and the zero pad of the W planes make
// every step whole. part is [n_slabs][n][kc].
// ---------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(MP_WAVE) void k_margins_multi_pk(
    const unsigned* __restrict__ P, unsigned lut_lo, unsigned lut_hi,
    const ubf16* __restrict__ whi, const ubf16* __restrict__ wlo, ll n, ll d,
    int kc, ll steps_per_slab, int n_slabs, float* __restrict__ part) {
  __shared__ u32x4_t tile[MP_ROWS * MP_LDS_STRIDE];
  const int l = threadIdx.x;
  const int half = l >> 5, li = l & 31;
  const ll gs = mp_row_groups(d);
  const ll dp = gs * 8;
  const ll n_steps = gs / MP_GROUPS;
  const ll n_rb = (n + MP_ROWS - 1) / MP_ROWS;
  for (ll t = blockIdx.x; t < n_rb * n_slabs; t += gridDim.x) {
    const ll rb = t / n_slabs;
    const ll s = t - rb * n_slabs;
    const ll st_lo = s * steps_per_slab;
    const ll st_hi = (st_lo + steps_per_slab < n_steps) ? st_lo + steps_per_slab
                                                        : n_steps;
    const ll r0 = rb * MP_ROWS;
    f32x16_t acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = f32x16_t{};
    for (ll st = st_lo; st < st_hi; ++st) {
      const ll g0 = st * MP_GROUPS;
      mp_u32x3 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        ll row = r0 + 2 * i + half;
        row = (row < n) ? row : n - 1;
        v[i] = mp_load_group(P + (row * gs + g0 + li) * 3);
      }
      __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
      for (int i = 0; i < 16; ++i)
        tile[(2 * i + half) * MP_LDS_STRIDE + li] =
            mp_decode_pairs(v[i], lut_lo, lut_hi);
      __syncthreads();
      const ll kbase = (g0 + half) * 8;
#pragma unroll 4
      for (int j = 0; j < 16; ++j) {
        const bf16x8_t a = __builtin_bit_cast(
            bf16x8_t, tile[li * MP_LDS_STRIDE + 2 * j + half]);
#pragma unroll
        for (int c = 0; c < NT; ++c) {
          const ll off = (ll)(c * 32 + li) * dp + kbase + 16 * j;
          const bf16x8_t bh = *(const bf16x8_t*)(whi + off);
          const bf16x8_t bl = *(const bf16x8_t*)(wlo + off);
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bh, acc[c], 0, 0, 0);
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc[c], 0, 0, 0);
        }
      }
    }
    float* __restrict__ dst = part + s * n * kc;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      const int cls = c * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const ll row = r0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row < n && cls < kc) dst[row * kc + cls] = acc[c][r];
      }
    }
  }
}

// Z[row, c] += sum_k val[k] · W[col[k], c] over the row's escapes, with the
// exact f32 W [d, k]: one wave per row, lane per class (the
// k_csr_margins_multi split). Rows without escapes are left untouched.
__global__ __launch_bounds__(256) void k_mp_fix_margins(
    const int* __restrict__ rowptr, const int* __restrict__ col,
    const float* __restrict__ val, const float* __restrict__ W, ll n, ll d,
    int k, int kc, float* __restrict__ Z) {
  const int lane = threadIdx.x & (MP_WAVE - 1);
  const ll wave_gid = (ll)blockIdx.x * 4 + threadIdx.x / MP_WAVE;
  const ll n_waves = (ll)gridDim.x * 4;
  for (ll r = wave_gid; r < n; r += n_waves) {
    const int k_lo = rowptr[r], k_hi = rowptr[r + 1];
    if (k_lo == k_hi) continue;
    for (int c = lane; c < k; c += MP_WAVE) {
      float acc = 0.f;
      for (int e = k_lo; e < k_hi; ++e) {
        const ll cc = col[e];
        if (cc >= 0 && cc < d) acc += val[e] * W[cc * k + c];
      }
      Z[r * kc + c] += acc;
    }
  }
}

// ---------------------------------------------------------------------------
// Gradient. k of the MFMA is the shard ROW, so the transpose happens inside
// a lane and the shard never touches LDS. A wave step covers 16 rows x 256
// columns: lane l owns group g0 + (l&31) for rows r0 + 8·(l>>5) … +7, eight
// 12-byte loads (each instruction: 384 contiguous bytes of two rows). After
// the decode the lane holds an 8-row x 8-column block as bf16 pairs; for
// column j it gathers the 8 rows with four permutes into the A operand of
// MFMA j, so accumulator tile j holds shard columns c0 + 8·(l&31) + j (its
// 32 MFMA rows) x 32 classes. The B operand is one 16-byte load from the
// transposed bf16 plane of M [kc32][n16]. A task is (row block, 32-class
// tile, 256-column tile); the four waves of a block take neighbouring column
// tiles. part is [n_rb][d][kc]; k_grad_reduce sums it in row-block order.
// SPLIT carries M as bf16(M) + bf16(M - bf16(M)), a second plane and a second
// MFMA per column into the same accumulator: the gradient of the f32
// multiplier and not of its bf16 rounding. The solver routes use it, because
// the 2^-9 rounding of every M entry does not shrink with the gradient near
// the optimum and was measured to swallow the restart test of a mixed sweep.
// ---------------------------------------------------------------------------

// The eight MFMAs of a gradient wave step: p[i] is row i of the lane's 8 x 8
// block as four dwords of bf16 pairs, b (and bl with SPLIT) the M fragment.
template <bool SPLIT>
__device__ __forceinline__ void mp_grad_mfma(const u32x4_t (&p)[8],
                                             const bf16x8_t b,
                                             const bf16x8_t bl,
                                             f32x16_t (&acc)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // element j of rows i, i+1 -> one dword: low halves for even j
    const unsigned sel = (j & 1) ? 0x07060302u : 0x05040100u;
    u32x4_t a;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      a[i] = __builtin_amdgcn_perm(p[2 * i + 1][j >> 1], p[2 * i][j >> 1], sel);
    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
        __builtin_bit_cast(bf16x8_t, a), b, acc[j], 0, 0, 0);
    if constexpr (SPLIT)
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          __builtin_bit_cast(bf16x8_t, a), bl, acc[j], 0, 0, 0);
  }
}

// Accumulator tile j holds columns c0 + 8·(its MFMA row) + j of class cls.
__device__ __forceinline__ void mp_grad_store(const f32x16_t (&acc)[8], ll c0,
                                              int half, int cls, ll d, int kc,
                                              float* __restrict__ dst) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const ll c = c0 + 8 * ((r & 3) + 8 * (r >> 2) + 4 * half) + j;
      if (c < d && cls < kc) dst[c * kc + cls] = acc[j][r];
    }
  }
}

template <bool SPLIT>
__global__ __launch_bounds__(256) void k_grad_multi_pk(
    const unsigned* __restrict__ P, unsigned lut_lo, unsigned lut_hi,
    const ubf16* __restrict__ mt, const ubf16* __restrict__ mt_lo, ll n, ll d,
    int kc, int n_ctiles, ll n_rb, float* __restrict__ part) {
  const int l = threadIdx.x & (MP_WAVE - 1);
  const int half = l >> 5, li = l & 31;
  const ll gs = mp_row_groups(d);
  const ll n_ct = gs / MP_GROUPS;
  const ll n_steps = (n + MP_GRAD_ROWS - 1) / MP_GRAD_ROWS;
  const ll n16 = n_steps * MP_GRAD_ROWS;
  const ll wave_gid = (ll)blockIdx.x * 4 + threadIdx.x / MP_WAVE;
  const ll n_waves = (ll)gridDim.x * 4;
  const ll n_tasks = n_rb * n_ctiles * n_ct;
  for (ll t = wave_gid; t < n_tasks; t += n_waves) {
    const ll ct = t % n_ct;
    const ll q = t / n_ct;
    const int ctile = (int)(q % n_ctiles);
    const ll rb = q / n_ctiles;
    const ll st_lo = rb * n_steps / n_rb;
    const ll st_hi = (rb + 1) * n_steps / n_rb;
    const ll g = ct * MP_GROUPS + li;
    const ll moff = (ll)(ctile * 32 + li) * n16 + 8 * half;
    const ubf16* __restrict__ mrow = mt + moff;
    f32x16_t acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = f32x16_t{};
    for (ll st = st_lo; st < st_hi; ++st) {
      const ll r0 = st * MP_GRAD_ROWS + 8 * half;
      u32x4_t p[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const ll row = r0 + i;
        // rows past n decode to +0.0 (the all-zero group), at a clamped address
        mp_u32x3 v = mp_load_group(P + (((row < n) ? row : n - 1) * gs + g) * 3);
        if (row >= n) v = mp_u32x3{0u, 0u, 0u};
        p[i] = mp_decode_pairs(v, lut_lo, lut_hi);
      }
      const bf16x8_t b = *(const bf16x8_t*)(mrow + st * MP_GRAD_ROWS);
      bf16x8_t bl = b;
      if constexpr (SPLIT)
        bl = *(const bf16x8_t*)(mt_lo + moff + st * MP_GRAD_ROWS);
      mp_grad_mfma<SPLIT>(p, b, bl, acc);
    }
    mp_grad_store(acc, ct * MP_COLS, half, ctile * 32 + li, d, kc,
                  part + rb * d * kc);
  }
}

// G[col, c] += sum_k cval[k] · M[row[k], c] over the column's escapes, M
// rounded to bf16 when the stream's plane is (round_m), so the correction
// matches the stream: one wave per column, lane per class (the
// k_csc_grad_multi split).
__global__ __launch_bounds__(256) void k_mp_fix_grad(
    const int* __restrict__ colptr, const int* __restrict__ row,
    const float* __restrict__ cval, const float* __restrict__ M, ll n, ll d,
    int kc, int round_m, float* __restrict__ G) {
  const int lane = threadIdx.x & (MP_WAVE - 1);
  const ll wave_gid = (ll)blockIdx.x * 4 + threadIdx.x / MP_WAVE;
  const ll n_waves = (ll)gridDim.x * 4;
  for (ll c = wave_gid; c < d; c += n_waves) {
    const int k_lo = colptr[c], k_hi = colptr[c + 1];
    if (k_lo == k_hi) continue;
    for (int cls = lane; cls < kc; cls += MP_WAVE) {
      float acc = 0.f;
      for (int e = k_lo; e < k_hi; ++e) {
        const ll r = row[e];
        if (r >= 0 && r < n) {
          const float m = M[r * kc + cls];
          acc += cval[e] * (round_m ? mp_bf2f(mp_f2bf_rne(m)) : m);
        }
      }
      G[c * kc + cls] += acc;
    }
  }
}

// ---------------------------------------------------------------------------
// Host API
// ---------------------------------------------------------------------------

static int mp_fail(const char* fmt, const char* who, ll a = 0, ll b = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, who, a, b);
  agd_set_last_error(buf);
  return 2;
}

// The agd_dense_eval_packed argument checks plus the class-dimension ones.
static int mp_args_ok(const char* who, const void* packed, ll n, ll d, int kc,
                      unsigned lut_lo, ll esc_nnz, const void* e0,
                      const void* e1, const void* e2) {
  if (n < 1 || d < 8 || d % 8 != 0)
    return mp_fail("%s: needs n >= 1 and d %% 8 == 0 (n=%lld d=%lld)", who, n, d);
  if (((uintptr_t)packed & 15) != 0)
    return mp_fail("%s: base pointer must be 16-byte aligned", who);
  if ((lut_lo & 0xffu) != 0u)
    return mp_fail("%s: table slot 0 must be 0x00 (escapes decode to +0.0)", who);
  if (kc < 4 || kc > 128 || (kc & 3))
    return mp_fail("%s: KC must be a multiple of 4 in [4, 128] (KC=%lld)", who, kc);
  if (esc_nnz > 0 && (!e0 || !e1 || !e2))
    return mp_fail("%s: escape lists missing (nnz=%lld)", who, esc_nnz);
  return 0;
}

static int mp_launch_ok(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", who, hipGetErrorString(e));
  agd_set_last_error(buf);
  return 1;
}

static inline int mp_grid(ll items, ll per_block, ll cap) {
  ll g = (items + per_block - 1) / per_block;
  if (g > cap) g = cap;
  return (int)(g < 1 ? 1 : g);
}

static inline int mp_class_tiles(int kc) { return (kc + 31) / 32; }

// Elements of one bf16 W plane [KC32, padded d] / of the M plane [KC32, n16].
extern "C" long long agd_multi_packed_wplane_elems(long long d, int kc) {
  const int nt = mp_class_tiles(kc) == 3 ? 4 : mp_class_tiles(kc);
  return (ll)nt * 32 * mp_row_groups(d) * 8;
}

extern "C" long long agd_multi_packed_mplane_elems(long long n, int kc) {
  return (ll)mp_class_tiles(kc) * 32 *
         ((n + MP_GRAD_ROWS - 1) / MP_GRAD_ROWS * MP_GRAD_ROWS);
}

// Column slabs of the margins pass (> 1 only when n/32 waves cannot fill the
// chip): the agd_margin_slabs recipe with a 32-row unit and a floor of four
// 256-column steps per slab. Callers size Z as n_slabs * n * kc floats.
static int mp_slabs(ll n, ll n_steps, ll min_steps) {
  const ll units = (n + MP_ROWS - 1) / MP_ROWS;
  const ll target = 4096;  // ~4 one-wave blocks per SIMD on 256 CUs
  if (units >= target) return 1;
  ll s = (target + units - 1) / units;
  const ll max_slabs = (n_steps + min_steps - 1) / min_steps;
  if (s > max_slabs) s = max_slabs;
  if (s > 256) s = 256;
  if (s < 1) s = 1;
  const ll per = (n_steps + s - 1) / s;
  return (int)((n_steps + per - 1) / per);
}

extern "C" int agd_multi_packed_slabs(long long n, long long d) {
  return mp_slabs(n, mp_row_groups(d) / MP_GROUPS, 4);
}

// Z [n, kc] f32 (pad columns exact zeros) = A · W from the packed copy.
// W is the logical [d, k] f32 block; whi/wlo are agd_multi_packed_wplane_elems
// bf16 each; Z is n_slabs * n * kc floats, the result in its first n * kc.
extern "C" int agd_margins_multi_packed(
    const void* packed, unsigned lut_lo, unsigned lut_hi, const void* esc_rowptr,
    const void* esc_col, const void* esc_val, long long esc_nnz, const void* W,
    long long n, long long d, int k, int kc, void* whi, void* wlo, void* Z,
    int n_slabs, void* stream) {
  const char* who = "agd_margins_multi_packed";
  if (mp_args_ok(who, packed, n, d, kc, lut_lo, esc_nnz, esc_rowptr, esc_col,
                 esc_val))
    return 2;
  if (k < 1 || k > kc) return mp_fail("%s: needs 1 <= k <= KC (k=%lld)", who, k);
  if (n_slabs != agd_multi_packed_slabs(n, d))
    return mp_fail("%s: n_slabs %lld is not agd_multi_packed_slabs()", who, n_slabs);
  hipStream_t s = (hipStream_t)stream;
  const ll gs = mp_row_groups(d);
  const ll dp = gs * 8;
  const ll n_steps = gs / MP_GROUPS;
  const ll per = (n_steps + n_slabs - 1) / n_slabs;
  const int tiles = mp_class_tiles(kc);
  const int nt = tiles == 3 ? 4 : tiles;
  hipLaunchKernelGGL(k_mp_prep_planes,
                     dim3(mp_grid(dp, MP_PREP_TILE, 4096)), dim3(256), 0, s,
                     (const float*)W, (ll)k, 0, (ll)d, k, nt * 32, dp, (ubf16*)whi,
                     (ubf16*)wlo);
  const ll n_rb = (n + MP_ROWS - 1) / MP_ROWS;
  const int grid = mp_grid(n_rb * n_slabs, 1, 1 << 16);
#define MP_LAUNCH_MARGINS(NTV)                                                 \
  hipLaunchKernelGGL((k_margins_multi_pk<NTV>), dim3(grid), dim3(MP_WAVE), 0,  \
                     s, (const unsigned*)packed, lut_lo, lut_hi,               \
                     (const ubf16*)whi, (const ubf16*)wlo, (ll)n, (ll)d, kc,   \
                     per, n_slabs, (float*)Z)
  if (nt == 1) MP_LAUNCH_MARGINS(1);
  else if (nt == 2) MP_LAUNCH_MARGINS(2);
  else MP_LAUNCH_MARGINS(4);
#undef MP_LAUNCH_MARGINS
  if (mp_launch_ok(who)) return 1;
  if (n_slabs > 1 && agd_slab_reduce_f32(Z, n * kc, n_slabs, stream)) return 1;
  if (esc_nnz > 0) {
    hipLaunchKernelGGL(k_mp_fix_margins, dim3(mp_grid(n, 4, 8192)), dim3(256),
                       0, s, (const int*)esc_rowptr, (const int*)esc_col,
                       (const float*)esc_val, (const float*)W, (ll)n, (ll)d, k,
                       kc, (float*)Z);
    if (mp_launch_ok(who)) return 1;
  }
  return 0;
}

// G [d, kc] f32 = Aᵀ · bf16(M) from the packed copy, or Aᵀ · M with M as a
// bf16 hi + lo pair when mt_lo is given. M is the padded [n, kc] f32
// multiplier; mt (and mt_lo) are agd_multi_packed_mplane_elems bf16; part is
// n_rb * d * kc floats (unused when n_rb == 1), n_rb from agd_multi_rowblocks.
extern "C" int agd_grad_multi_packed(
    const void* packed, unsigned lut_lo, unsigned lut_hi, const void* esc_colptr,
    const void* esc_row, const void* esc_cval, long long esc_nnz, const void* M,
    long long n, long long d, int kc, void* mt, void* mt_lo, void* part,
    long long n_rb, void* grad, void* stream) {
  const char* who = "agd_grad_multi_packed";
  if (mp_args_ok(who, packed, n, d, kc, lut_lo, esc_nnz, esc_colptr, esc_row,
                 esc_cval))
    return 2;
  if (n_rb < 1) return mp_fail("%s: n_rb must be >= 1 (n_rb=%lld)", who, n_rb);
  hipStream_t s = (hipStream_t)stream;
  const int tiles = mp_class_tiles(kc);
  const ll n16 = (n + MP_GRAD_ROWS - 1) / MP_GRAD_ROWS * MP_GRAD_ROWS;
  hipLaunchKernelGGL(k_mp_prep_planes,
                     dim3(mp_grid(n16, MP_PREP_TILE, 4096)), dim3(256), 0, s,
                     (const float*)M, (ll)kc, 0, (ll)n, kc, tiles * 32, n16, (ubf16*)mt,
                     (ubf16*)mt_lo);
  const ll n_ct = mp_row_groups(d) / MP_GROUPS;
  float* p = (n_rb == 1) ? (float*)grad : (float*)part;
#define MP_LAUNCH_GRAD(SPLITV)                                                  \
  hipLaunchKernelGGL((k_grad_multi_pk<SPLITV>),                                \
                     dim3(mp_grid(n_rb * tiles * n_ct, 4, 1 << 16)), dim3(256), \
                     0, s, (const unsigned*)packed, lut_lo, lut_hi,            \
                     (const ubf16*)mt, (const ubf16*)mt_lo, (ll)n, (ll)d, kc,  \
                     tiles, (ll)n_rb, p)
  if (mt_lo) MP_LAUNCH_GRAD(true);
  else MP_LAUNCH_GRAD(false);
#undef MP_LAUNCH_GRAD
  if (mp_launch_ok(who)) return 1;
  if (n_rb > 1 && agd_grad_reduce_f32(part, n_rb, d * kc, grad, stream)) return 1;
  if (esc_nnz > 0) {
    hipLaunchKernelGGL(k_mp_fix_grad, dim3(mp_grid(d, 4, 8192)), dim3(256), 0,
                       s, (const int*)esc_colptr, (const int*)esc_row,
                       (const float*)esc_cval, (const float*)M, (ll)n, (ll)d,
                       kc, mt_lo ? 0 : 1, (float*)grad);
    if (mp_launch_ok(who)) return 1;
  }
  return 0;
}

// ===========================================================================
// fp8 (e4m3fn) shards. Rows are plain bytes (row stride d, d % 16 == 0), every
// e4m3 value is exactly a bf16 value, and v_cvt_scalef32_pk_bf16_fp8 with
// scale 1.0 turns two bytes into one dword of two bf16: no table, no escapes,
// no side lists. The W / M operands are the bf16 planes of k_mp_prep_planes.
// ===========================================================================

#define F8_STEP 128       // columns a margins wave step covers
#define F8_SLAB_STEPS 8   // floor of a margins column slab, in steps

typedef unsigned int f8_u32x2 __attribute__((ext_vector_type(2)));

template <bool HI>
__device__ __forceinline__ unsigned f8_pair(unsigned v) {
  return __builtin_bit_cast(
      unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, HI));
}

// Eight fp8 bytes (two dwords) to four dwords of bf16 pairs, element order
// kept: the layout mp_decode_pairs gives for a packed group.
__device__ __forceinline__ u32x4_t f8_decode8(unsigned lo, unsigned hi) {
  return u32x4_t{f8_pair<false>(lo), f8_pair<true>(lo), f8_pair<false>(hi),
                 f8_pair<true>(hi)};
}

__host__ __device__ __forceinline__ ll f8_padded_d(ll d) {
  return (d + F8_STEP - 1) / F8_STEP * F8_STEP;
}

// Class tiles one margins wave carries: 1, 2 or 4 (three run as four over a
// zero tile); above 128 padded classes the groups of four tiles are a grid
// dimension.
static inline int f8_group_tiles(int kc) {
  const int tiles = mp_class_tiles(kc);
  return tiles <= 2 ? tiles : 4;
}

static inline int f8_class_groups(int kc) {
  const int nt = f8_group_tiles(kc);
  return (mp_class_tiles(kc) + nt - 1) / nt;
}

// ---------------------------------------------------------------------------
// Margins, without LDS. One wave (one 64-thread block) owns 32 rows, one
// column slab and one group of NT class tiles. Lane l is row r0 + (l&31),
// half h = l>>5. Per 128-column step at column c a lane issues four 16-byte
// loads at columns c + 16·(2j + h), j = 0..3 (each instruction: 32 contiguous
// bytes of every row). A load decodes to two A fragments (s = 0, 1): the k
// order inside a dot product is free as long as W follows it, so the B
// operand of fragment (j, s) is the 16-byte load
//   W[class][c + 16·(2j + h) + 8s … +8)
// of the hi plane and again of the lo plane: two MFMAs per fragment and class
// tile into one accumulator. Rows past n are clamped and never stored. A
// load wholly past d (only in the last step) reads the row's first 16 bytes
// instead and meets the exact zeros that pad the W planes to dp, so it adds
// ±0. part is [n_slabs][n][kc].
// ---------------------------------------------------------------------------
__device__ __forceinline__ void f8_load_step(
    const unsigned char* __restrict__ arow, ll c, ll d, u32x4_t (&v)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const ll col = c + 32 * j;
    // plain loads: nt ones were measured slower here (docs/KERNELS.md)
    v[j] = *(const u32x4_t*)(arow + ((col < d) ? col : 0));
  }
}

template <int NT>
__global__ __launch_bounds__(MP_WAVE) void k_margins_multi_f8(
    const unsigned char* __restrict__ A, const ubf16* __restrict__ whi,
    const ubf16* __restrict__ wlo, ll n, ll d, int kc, ll steps_per_slab,
    int n_slabs, int n_groups, float* __restrict__ part) {
  const int l = threadIdx.x;
  const int half = l >> 5, li = l & 31;
  const ll dp = f8_padded_d(d);
  const ll n_steps = dp / F8_STEP;
  const ll n_rb = (n + MP_ROWS - 1) / MP_ROWS;
  const ll n_tasks = n_rb * n_slabs * n_groups;
  for (ll t = blockIdx.x; t < n_tasks; t += gridDim.x) {
    const int grp = (int)(t % n_groups);
    const ll q = t / n_groups;
    const ll s = q % n_slabs;
    const ll rb = q / n_slabs;
    const ll st_lo = s * steps_per_slab;
    const ll st_hi = (st_lo + steps_per_slab < n_steps) ? st_lo + steps_per_slab
                                                        : n_steps;
    const ll r0 = rb * MP_ROWS;
    const ll row = (r0 + li < n) ? r0 + li : n - 1;
    const unsigned char* __restrict__ arow = A + row * d;
    const ll wrow = ((ll)grp * NT * 32 + li) * dp;
    f32x16_t acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = f32x16_t{};
    // the next step's four loads are in flight while this step's MFMAs run
    // (the last step of a task loads itself again)
    u32x4_t v[4], vn[4];
    f8_load_step(arow, st_lo * F8_STEP + 16 * half, d, vn);
    for (ll st = st_lo; st < st_hi; ++st) {
      const ll c = st * F8_STEP + 16 * half;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = vn[j];
      f8_load_step(arow, c + ((st + 1 < st_hi) ? F8_STEP : 0), d, vn);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int sf = 0; sf < 2; ++sf) {
          const bf16x8_t a = __builtin_bit_cast(
              bf16x8_t, f8_decode8(v[j][2 * sf], v[j][2 * sf + 1]));
#pragma unroll
          for (int ct = 0; ct < NT; ++ct) {
            const ll off = wrow + (ll)ct * 32 * dp + c + 32 * j + 8 * sf;
            const bf16x8_t bh = *(const bf16x8_t*)(whi + off);
            const bf16x8_t bl = *(const bf16x8_t*)(wlo + off);
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bh, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc[ct], 0, 0, 0);
          }
        }
      }
    }
    float* __restrict__ dst = part + s * n * kc;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      const int cls = (grp * NT + ct) * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const ll ro = r0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (ro < n && cls < kc) dst[ro * kc + cls] = acc[ct][r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Gradient: k_grad_multi_pk's design on plain byte rows. Lane l owns columns
// c0 + 8·(l&31) … +7 for rows r0 + 8·(l>>5) … +7: eight nt 8-byte loads (each
// instruction: 256 contiguous bytes of two rows), decoded to the same 8 x 8
// block of bf16 pairs, then the shared mp_grad_mfma / mp_grad_store. Rows
// past n are read at a clamped address and zeroed. With d % 16 == 0 a lane's
// eight columns are wholly inside d or wholly past it; those past it read
// column 0 instead, feed only MFMA rows of their own and are never stored.
// ---------------------------------------------------------------------------
template <bool SPLIT>
__global__ __launch_bounds__(256) void k_grad_multi_f8(
    const unsigned char* __restrict__ A, const ubf16* __restrict__ mt,
    const ubf16* __restrict__ mt_lo, ll n, ll d, int kc, int n_ctiles, ll n_rb,
    float* __restrict__ part) {
  const int l = threadIdx.x & (MP_WAVE - 1);
  const int half = l >> 5, li = l & 31;
  const ll n_ct = (d + MP_COLS - 1) / MP_COLS;
  const ll n_steps = (n + MP_GRAD_ROWS - 1) / MP_GRAD_ROWS;
  const ll n16 = n_steps * MP_GRAD_ROWS;
  const ll wave_gid = (ll)blockIdx.x * 4 + threadIdx.x / MP_WAVE;
  const ll n_waves = (ll)gridDim.x * 4;
  const ll n_tasks = n_rb * n_ctiles * n_ct;
  for (ll t = wave_gid; t < n_tasks; t += n_waves) {
    const ll ct = t % n_ct;
    const ll q = t / n_ct;
    const int ctile = (int)(q % n_ctiles);
    const ll rb = q / n_ctiles;
    const ll st_lo = rb * n_steps / n_rb;
    const ll st_hi = (rb + 1) * n_steps / n_rb;
    const ll c = ct * MP_COLS + 8 * li;
    const unsigned char* __restrict__ acol = A + ((c < d) ? c : 0);
    const ll moff = (ll)(ctile * 32 + li) * n16 + 8 * half;
    f32x16_t acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = f32x16_t{};
    for (ll st = st_lo; st < st_hi; ++st) {
      const ll r0 = st * MP_GRAD_ROWS + 8 * half;
      u32x4_t p[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const ll row = r0 + i;
        f8_u32x2 v = __builtin_nontemporal_load(
            (const f8_u32x2*)(acol + ((row < n) ? row : n - 1) * d));
        if (row >= n) v = f8_u32x2{0u, 0u};
        p[i] = f8_decode8(v[0], v[1]);
      }
      const bf16x8_t b = *(const bf16x8_t*)(mt + moff + st * MP_GRAD_ROWS);
      bf16x8_t bl = b;
      if constexpr (SPLIT)
        bl = *(const bf16x8_t*)(mt_lo + moff + st * MP_GRAD_ROWS);
      mp_grad_mfma<SPLIT>(p, b, bl, acc);
    }
    mp_grad_store(acc, ct * MP_COLS, half, ctile * 32 + li, d, kc,
                  part + rb * d * kc);
  }
}

static int f8_args_ok(const char* who, const void* A, ll n, ll d, int kc) {
  if (n < 1 || d < 16 || d % 16 != 0)
    return mp_fail("%s: needs n >= 1 and d %% 16 == 0 (n=%lld d=%lld)", who, n, d);
  if (((uintptr_t)A & 15) != 0)
    return mp_fail("%s: base pointer must be 16-byte aligned", who);
  if (kc < 4 || (kc & 3))
    return mp_fail("%s: KC must be a multiple of 4, >= 4 (KC=%lld)", who, kc);
  return 0;
}

// k_mp_prep_planes over a class dimension of any width, 128 columns a launch:
// plane rows [0, rows_out) of hi (and lo) from columns [0, k_in) of src.
static void f8_prep_planes(const float* src, ll src_ld, ll rows, int k_in,
                           int rows_out, ll ld, ubf16* hi, ubf16* lo,
                           hipStream_t s) {
  for (int c0 = 0; c0 < rows_out; c0 += 128) {
    const int live = k_in - c0 < 0 ? 0 : (k_in - c0 > 128 ? 128 : k_in - c0);
    const int out = rows_out - c0 > 128 ? 128 : rows_out - c0;
    hipLaunchKernelGGL(k_mp_prep_planes, dim3(mp_grid(ld, MP_PREP_TILE, 4096)),
                       dim3(256), 0, s, src, src_ld, c0, rows, live, out, ld,
                       hi + (ll)c0 * ld, lo ? lo + (ll)c0 * ld : nullptr);
  }
}

// Elements of one bf16 W plane [class groups x tiles x 32, padded d]. The M
// plane of the gradient is agd_multi_packed_mplane_elems (any KC).
extern "C" long long agd_multi_f8_wplane_elems(long long d, int kc) {
  return (ll)f8_class_groups(kc) * f8_group_tiles(kc) * 32 * f8_padded_d(d);
}

// Column slabs of the fp8 margins pass: the agd_multi_packed_slabs recipe
// with a floor of eight 128-column steps per slab.
extern "C" int agd_multi_f8_slabs(long long n, long long d) {
  return mp_slabs(n, f8_padded_d(d) / F8_STEP, F8_SLAB_STEPS);
}

// Z [n, kc] f32 (pad columns exact zeros) = A · W from an fp8 e4m3fn shard
// [n, d]. W is the logical [d, k] f32 block; whi/wlo are
// agd_multi_f8_wplane_elems bf16 each; Z is n_slabs * n * kc floats, the
// result in its first n * kc.
extern "C" int agd_margins_multi_f8(const void* A, const void* W, long long n,
                                    long long d, int k, int kc, void* whi,
                                    void* wlo, void* Z, int n_slabs,
                                    void* stream) {
  const char* who = "agd_margins_multi_f8";
  if (f8_args_ok(who, A, n, d, kc)) return 2;
  if (k < 1 || k > kc) return mp_fail("%s: needs 1 <= k <= KC (k=%lld)", who, k);
  if (n_slabs != agd_multi_f8_slabs(n, d))
    return mp_fail("%s: n_slabs %lld is not agd_multi_f8_slabs()", who, n_slabs);
  hipStream_t s = (hipStream_t)stream;
  const ll dp = f8_padded_d(d);
  const ll per = (dp / F8_STEP + n_slabs - 1) / n_slabs;
  const int nt = f8_group_tiles(kc), groups = f8_class_groups(kc);
  f8_prep_planes((const float*)W, k, d, k, groups * nt * 32, dp, (ubf16*)whi,
                 (ubf16*)wlo, s);
  const ll n_rb = (n + MP_ROWS - 1) / MP_ROWS;
  const int grid = mp_grid(n_rb * n_slabs * groups, 1, 1 << 16);
#define F8_LAUNCH_MARGINS(NTV)                                                 \
  hipLaunchKernelGGL((k_margins_multi_f8<NTV>), dim3(grid), dim3(MP_WAVE), 0,  \
                     s, (const unsigned char*)A, (const ubf16*)whi,            \
                     (const ubf16*)wlo, (ll)n, (ll)d, kc, per, n_slabs,        \
                     groups, (float*)Z)
  if (nt == 1) F8_LAUNCH_MARGINS(1);
  else if (nt == 2) F8_LAUNCH_MARGINS(2);
  else F8_LAUNCH_MARGINS(4);
#undef F8_LAUNCH_MARGINS
  if (mp_launch_ok(who)) return 1;
  if (n_slabs > 1 && agd_slab_reduce_f32(Z, n * kc, n_slabs, stream)) return 1;
  return 0;
}

// G [d, kc] f32 = Aᵀ · bf16(M) from an fp8 e4m3fn shard, or Aᵀ · M with M as
// a bf16 hi + lo pair when mt_lo is given. M is the padded [n, kc] f32
// multiplier; mt (and mt_lo) are agd_multi_packed_mplane_elems bf16; part is
// n_rb * d * kc floats (unused when n_rb == 1), n_rb from agd_multi_rowblocks.
extern "C" int agd_grad_multi_f8(const void* A, const void* M, long long n,
                                 long long d, int kc, void* mt, void* mt_lo,
                                 void* part, long long n_rb, void* grad,
                                 void* stream) {
  const char* who = "agd_grad_multi_f8";
  if (f8_args_ok(who, A, n, d, kc)) return 2;
  if (n_rb < 1) return mp_fail("%s: n_rb must be >= 1 (n_rb=%lld)", who, n_rb);
  hipStream_t s = (hipStream_t)stream;
  const int tiles = mp_class_tiles(kc);
  const ll n16 = (n + MP_GRAD_ROWS - 1) / MP_GRAD_ROWS * MP_GRAD_ROWS;
  f8_prep_planes((const float*)M, kc, n, kc, tiles * 32, n16, (ubf16*)mt,
                 (ubf16*)mt_lo, s);
  const ll n_ct = (d + MP_COLS - 1) / MP_COLS;
  float* p = (n_rb == 1) ? (float*)grad : (float*)part;
#define F8_LAUNCH_GRAD(SPLITV)                                                  \
  hipLaunchKernelGGL((k_grad_multi_f8<SPLITV>),                                \
                     dim3(mp_grid(n_rb * tiles * n_ct, 4, 1 << 16)), dim3(256), \
                     0, s, (const unsigned char*)A, (const ubf16*)mt,          \
                     (const ubf16*)mt_lo, (ll)n, (ll)d, kc, tiles, (ll)n_rb, p)
  if (mt_lo) F8_LAUNCH_GRAD(true);
  else F8_LAUNCH_GRAD(false);
#undef F8_LAUNCH_GRAD
  if (mp_launch_ok(who)) return 1;
  if (n_rb > 1 && agd_grad_reduce_f32(part, n_rb, d * kc, grad, stream)) return 1;
  return 0;
}
