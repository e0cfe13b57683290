// pnode_amd -- the parameter sensitivities of a Linear layer, fused: dW and db of `out = x W^T + b` from the cotangent G at the
// layer's output, accumulated over the stages and time steps of a reverse sweep (row a-9 of the hot path:
// RHSJacPShell.multTranspose + the VecAXPY on mu inside TSAdjointStep_RK, reference pnode/petsc_adjoint.py:341-363).
//
//   PW[s][m][n] += sum_{k in K-range s} (alpha G[k][m]) X[k][n]        s = 0..7   (G: rows x out, X: rows x in, row-major)
//   PB[s][j][m] += sum_{k in the slabs of K-range s that tile column j adds up}  alpha G[k][m]
//
// and, once per reverse sweep,  mu_W[m][n] += sum_s PW[s][m][n],  mu_b[m] += sum_{s,j} PB[s][j][m]  (then PW = PB = 0).
//
// Why a kernel of its own: the product is K-deep (K = rows = 4096 at BASELINE's target configuration, 512 x 512 out) -- the
// one GEMM shape of the time step the BLAS library serves badly (fp32: 25.6 us against 19.5 for the forward- and dX-shaped
// products of the same size; fp64: 129 us against 40) -- and everything around it was extra passes: the column sum for db, a copy
// of the last layer's cotangent, the accumulation into mu.  Here:
//   * K is split eight ways and the split index is blockIdx % 8: workgroups are dealt to the 8 XCDs round-robin, so each XCD
//     works on ONE K range and the G and X rows it needs stay in its own 4 MB L2;
//   * 64 x 64 output tiles per workgroup of eight waves; each wave owns a 32 x 32 tile (fp32: one v_mfma_f32_32x32x2_f32
//     accumulator, exact fp32, a k-ordered fmaf chain; fp64: 2 x 2 accumulators of v_mfma_f64_16x16x4_f64) and HALF of every K
//     slab -- waves 0-3 the first half of its rows, waves 4-7 the second, added through LDS at the end;
//   * slabs of 32 rows per operand (8 KB fp32, 16 KB fp64) through TWO LDS buffers, one barrier per slab: while slab s is
//     multiplied, slab s+1 goes from registers to the other buffer and the global loads of slab s+2 are in flight
//     (round 5 had one buffer and two barriers per slab: 41 500 cycles per tile against 39 500, tools/mb_wgrad6.hip);
//   * the partial tile in PW is read under the K loop and added at its end: the sum over stages and time steps costs no pass;
//   * the workgroups of a tile row share the column sums of their G slabs between them (slab s: tile column s % ntn): db for free;
//   * GROUPED launches (pn_linear_wgrad_group): the pairs of all Linear layers of one stage VJP go through ONE launch --
//     workgroups of the next pair start while the last ones of the previous pair drain, and there is one launch boundary per
//     stage instead of one per layer: 20.1 us per 4096 x 512 x 512 pair against 22.6 alone (and 25 inside the sweep in round 5).
// Bit-reproducible (fixed split, fixed order, no atomics); independent of how pairs are grouped into launches.
// rows >= 256 (any number: a ragged last slab is zero-filled), out % 64 == 0, in % 64 == 0, out * in <= 2^22; everything else takes the general path (torch GEMM +
// pn_colsum_accum_multi).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>

#include "pn_launch.h"
#include "pnode_amd.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kSplit = 8;        // K ranges = XCDs
constexpr int BM = 64, BN = 64;
constexpr int kThreads = 512;    // eight waves: 2 x 2 tiles of 32 x 32, times the two halves of a K slab
constexpr int kMaxPairs = PN_WGRAD_MAX_PAIRS;
// Above 2048 x 2048 weights a layer has tiles enough to fill the chip without a K split and the partial buffers (8 x the weight)
// stop being small change: such layers are left to the library GEMM.
constexpr int64_t kMaxWeights = (int64_t)1 << 22;

template <typename T>
struct Shape {                   // one slab = 32 rows of G and of X in either precision (fp32: 8 KB per operand, fp64: 16 KB)
  static constexpr int BK = 32;
  static constexpr int VEC = 16 / (int)sizeof(T);
  static constexpr int VPT = BK * BM / VEC / kThreads;          // 16-byte vectors per thread per operand: 1 (fp32), 2 (fp64)
  static constexpr int LD = BM;                                 // unpadded rows
  // fp32: a half-wave of ds_read_b32 reads 32 consecutive floats of one row: conflict-free as it stands.  fp64: a half-wave of
  // ds_read_b64 reads 16 doubles of each of TWO consecutive rows, which start 128 dwords = 0 banks apart: odd rows are stored with
  // their two halves of 16 doubles swapped pairwise (column ^ 16), so that the two rows sit 32 banks apart
  static __device__ __forceinline__ int col(int row, int c) { return std::is_same<T, float>::value ? c : (c ^ ((row & 1) << 4)); }
};

struct GroupArgs {
  const void *g[kMaxPairs], *x[kMaxPairs];
  void *pw[kMaxPairs];
  double *pb[kMaxPairs];
  double alpha[kMaxPairs];
  int M[kMaxPairs], N[kMaxPairs];
  int first[kMaxPairs + 1];      // first workgroup of pair p; first[npairs] = grid size
  int npairs, K;
};

// RAGGED: rows is not a multiple of 8 slabs -- rows that do not exist are loaded as zeros (an instantiation of its own: the test in
// front of every load costs the aligned case 2-17 %)
template <typename T, bool RAGGED>
__device__ __forceinline__ void wgrad_body(const GroupArgs &ga_) {
  using S = Shape<T>;
  constexpr bool F32 = std::is_same<T, float>::value;
  constexpr int BK = S::BK, LD = S::LD, VEC = S::VEC;
  typedef T vec_t __attribute__((ext_vector_type(VEC)));
  constexpr int SLAB = BK * LD;                                  // elements per operand per buffer
  __shared__ T smem[2 * 2 * SLAB];                               // [buffer][G | X][BK][LD]; staging for the two reductions at the end
  int p = 0;
#pragma unroll
  for (int q = 1; q < kMaxPairs; ++q) p += (q < ga_.npairs && (int)blockIdx.x >= ga_.first[q]) ? 1 : 0;
  const T *__restrict__ G = static_cast<const T *>(ga_.g[p]);
  const T *__restrict__ X = static_cast<const T *>(ga_.x[p]);
  T *__restrict__ PW = static_cast<T *>(ga_.pw[p]);
  double *__restrict__ PB = ga_.pb[p];
  const int M = ga_.M[p], N = ga_.N[p], K = ga_.K;
  const T alpha = (T)ga_.alpha[p];
  const int bid = (int)blockIdx.x - ga_.first[p];
  const int split = bid % kSplit, tile = bid / kSplit;
  const int ntn = N / BN;
  const int tm = tile / ntn, tn = tile % ntn;
  // rows per K range: whole slabs; rows that do not exist (K is not a multiple of 8 slabs) are loaded as zeros
  const int kper = RAGGED ? (K + kSplit * BK - 1) / (kSplit * BK) * BK : K / kSplit, k0 = split * kper, nslab = kper / BK;
  constexpr bool ragged = RAGGED;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int kh = w >> 2, wm = w & 1, wn = (w >> 1) & 1;          // K half, tile row, tile column of this wave
  constexpr int GROW = BM / VEC, VPT = S::VPT;                   // 16-byte vectors per slab row; VPT G and VPT X vectors per thread
  static_assert(VPT * kThreads * VEC == BK * BM && kThreads % GROW == 0, "whole vectors per thread, every thread in one column group");
  const int lrow = t / GROW, lc = t % GROW;                      // vector v of this thread: row lrow + v * (kThreads / GROW), column group lc
  constexpr int RSTEP = kThreads / GROW;
  const bool bias = PB != nullptr;
  vec_t gv[VPT], xv[VPT];
  // this thread's columns of the G slabs that are this workgroup's to add up: K / 8 / BK / ntn values each, summed in the state's
  // precision (packed adds; four double adds per thread per slab in front of the barrier cost 1 us per 4096 x 512 x 512 pair), the
  // threads of a column group then in double
  T colsum[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) colsum[e] = (T)0;

  // element e of this lane's accumulator registers -> (row, column) of the wave's 32 x 32 tile
  auto tile_row = [&](int e) { return F32 ? (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) : ((e >> 3) * 16 + (lane >> 4) + 4 * (e & 3)); };
  auto tile_col = [&](int e) { return F32 ? (lane & 31) : (((e >> 2) & 1) * 16 + (lane & 15)); };
  // (fp64: e = 8 i + 4 j + r for accumulator (i, j), register r: C/D of v_mfma_f64_16x16x4_f64 is col = lane & 15, row = (lane >> 4) + 4 r)

  T *pw = PW + (size_t)split * M * N;
  T acc[16], old[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = (T)0;
  double *pbp = bias && t < BM ? PB + ((size_t)split * ntn + tn) * M + tm * BM + t : nullptr;

  auto gload = [&](int slab) {
    const int kb = k0 + slab * BK;
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
      const int row = kb + lrow + v * RSTEP;
      if (!ragged || row < K) {
        gv[v] = *reinterpret_cast<const vec_t *>(G + (size_t)row * M + tm * BM + lc * VEC);
        xv[v] = *reinterpret_cast<const vec_t *>(X + (size_t)row * N + tn * BN + lc * VEC);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) gv[v][e] = (T)0, xv[v][e] = (T)0;
      }
    }
  };
  // The workgroups of a tile row (tn = 0..ntn-1) see the same G slabs: slab s is added up by the one with tn == s % ntn,
  // so that no workgroup carries the column sums alone (the launch ends with its slowest workgroup).
  auto lstore = [&](int slab, int buf) {
    T *Gs = smem + buf * 2 * SLAB, *Xs = Gs + SLAB;
    if constexpr (VPT == 1) {                    // (fp32: one vector per thread, no swizzle)
      const vec_t g = alpha * gv[0];             // here, not at the load: the product would wait for the load in front of the MFMAs
      *reinterpret_cast<vec_t *>(&Gs[lrow * LD + lc * VEC]) = g;
      if (bias && slab % ntn == tn) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) colsum[e] += g[e];
      }
      *reinterpret_cast<vec_t *>(&Xs[lrow * LD + lc * VEC]) = xv[0];
    } else {
#pragma unroll
      for (int v = 0; v < VPT; ++v) {
        const int row = lrow + v * RSTEP;
        const vec_t g = alpha * gv[v];
        *reinterpret_cast<vec_t *>(&Gs[row * LD + S::col(row, lc * VEC)]) = g;
        if (bias && slab % ntn == tn) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) colsum[e] += g[e];
        }
        *reinterpret_cast<vec_t *>(&Xs[row * LD + S::col(row, lc * VEC)]) = xv[v];
      }
    }
  };
  auto compute = [&](int buf) {
    const T *Gs = smem + buf * 2 * SLAB, *Xs = Gs + SLAB;
    if constexpr (F32) {
      const int lr = lane & 31, lh = lane >> 5;
      f32x16 c;
#pragma unroll
      for (int e = 0; e < 16; ++e) c[e] = acc[e];
#pragma unroll
      for (int kk = 0; kk < BK / 2; kk += 2) {
        const float a = Gs[(kh * (BK / 2) + kk + lh) * LD + wm * 32 + lr];
        const float b = Xs[(kh * (BK / 2) + kk + lh) * LD + wn * 32 + lr];
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = c[e];
    } else {
      const int lr = lane & 15, lq = lane >> 4;
      f64x4 c[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) c[i][j][r] = acc[8 * i + 4 * j + r];
#pragma unroll
      for (int kk = 0; kk < BK / 2; kk += 4) {
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = Gs[(kh * (BK / 2) + kk + lq) * LD + S::col(kk + lq, wm * 32 + i * 16 + lr)];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = Xs[(kh * (BK / 2) + kk + lq) * LD + S::col(kk + lq, wn * 32 + j * 16 + lr)];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) c[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], c[i][j], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[8 * i + 4 * j + r] = c[i][j][r];
    }
  };

  gload(0);
  // what the earlier stages / time steps left in PW (and PB): needed after the K loop, loaded now -- BEHIND the first slab's loads:
  // loads return in order, and the first LDS store must not wait for a tile that comes from HBM
#pragma unroll
  for (int e = 0; e < 16; ++e)
    old[e] = kh == 0 ? pw[(size_t)(tm * BM + wm * 32 + tile_row(e)) * N + tn * BN + wn * 32 + tile_col(e)] : (T)0;
  const double pbold = pbp ? *pbp : 0.0;
  lstore(0, 0);
  if (nslab > 1) gload(1);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    compute(s & 1);
    if (s + 1 < nslab) lstore(s + 1, (s + 1) & 1);      // the other buffer: its last readers passed the barrier of slab s-1
    if (s + 2 < nslab) gload(s + 2);                    // in flight while slab s+1 is multiplied
    __syncthreads();
  }
  // ---- the end, ONE barrier (the slab buffers are free now): the second K half hands its tile to the first through
  // [4 waves x 16 registers][64 lanes]; behind it [kThreads / GROW][BM] doubles: the threads of a column group, added in thread order
  T(*red)[64] = reinterpret_cast<T(*)[64]>(&smem[0]);
  double(*cs)[BM] = reinterpret_cast<double(*)[BM]>(&smem[4 * 16 * 64]);
  static_assert(sizeof(smem) >= 4 * 16 * 64 * sizeof(T) + (kThreads / GROW) * BM * sizeof(double), "the reductions are staged in the slab buffers");
  if (kh == 1) {
#pragma unroll
    for (int e = 0; e < 16; ++e) red[(w & 3) * 16 + e][lane] = acc[e];
  }
  if (bias) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) cs[lrow][lc * VEC + e] = (double)colsum[e];
  }
  __syncthreads();
  if (kh == 0) {                                      // PW = PW + (first + second)
#pragma unroll
    for (int e = 0; e < 16; ++e)
      pw[(size_t)(tm * BM + wm * 32 + tile_row(e)) * N + tn * BN + wn * 32 + tile_col(e)] = old[e] + (acc[e] + red[(w & 3) * 16 + e][lane]);
  }
  if (pbp) {
    double sum = cs[0][t];
#pragma unroll
    for (int j = 1; j < kThreads / GROW; ++j) sum += cs[j][t];
    *pbp = pbold + sum;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The fp32 product on the BF16 matrix cores, by exact operand splitting (the default for fp32 states).
// Every fp32 operand a is split exactly into three bf16 terms a = a_hi + a_mid + a_lo (the top 16 bits of an fp32 pattern ARE a bf16:
// three truncations cover the 24-bit significand, every remainder is exact in fp32); a*b is then the sum of nine bf16 x bf16
// products, each of them exact in fp32.  The six largest -- hi*lo, lo*hi, mid*mid, hi*mid, mid*hi, hi*hi; what is dropped is below
// 2^-23 |a b| -- go through v_mfma_f32_32x32x16_bf16 with fp32 accumulation: 6 x 32 cycles of matrix pipe per 32 x 32 x 16 block
// against 8 x 64 for v_mfma_f32_32x32x2_f32 (the bf16 pipe is 16 times as fast per product).  Measured against float64 on
// cotangent-like operands (tools/mb_wgrad_bf16x3.hip, error / sum |g x|): max 5.7e-8, rms 1.1e-8 -- BELOW the plain fp32 fmaf chain
// (1.0e-7 / 1.8e-8: fewer roundings), and 16.4 us per 4096 x 512 x 512 pair against 20.5.  What bounds it now is no longer the matrix
// pipe: one MFMA instead of six takes 9.9 us (the split's VALU work, 1.5 x the LDS store volume, HBM: G + X + the partial tiles).
// LDS image per (operand, part): [32 rows k][64 bf16], 128-byte rows with the two 64-byte halves swapped on rows with (k >> 1) & 1,
// so that the four rows of a transposed read fall on disjoint banks; operand fragments by ds_read_b64_tr_b16 (4 rows x 16 columns
// per 16-lane group, delivered column-major: the k-contiguous fragment the MFMA wants from a [k][m] image).
// Inf operands give NaN (inf - inf in the split); everything finite, subnormals included, is exact up to the dropped terms.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// The helpers every split-bf16 kernel of this file shares (the two wgrad forms below, pn_linear_fwd and pn_linear_bwd further down).
// Four fp32 values -> their three bf16 terms, packed four to a u32x2 in element order.
struct Split3 {
  u32x2 hi, mid, lo;
};
__device__ __forceinline__ Split3 split3(const f32x4 v) {
  unsigned a[4], r1[4], r2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = __float_as_uint(v[e]);
    const float f1 = v[e] - __uint_as_float(a[e] & 0xFFFF0000u);               // exact
    r1[e] = __float_as_uint(f1);
    r2[e] = __float_as_uint(f1 - __uint_as_float(r1[e] & 0xFFFF0000u));       // exact; at most 8 significant bits are left
  }
  // v_perm_b32 with this selector: the top halves of two patterns side by side = two bf16, truncated
  Split3 s;
  s.hi = u32x2{__builtin_amdgcn_perm(a[1], a[0], 0x07060302u), __builtin_amdgcn_perm(a[3], a[2], 0x07060302u)};
  s.mid = u32x2{__builtin_amdgcn_perm(r1[1], r1[0], 0x07060302u), __builtin_amdgcn_perm(r1[3], r1[2], 0x07060302u)};
  s.lo = u32x2{__builtin_amdgcn_perm(r2[1], r2[0], 0x07060302u), __builtin_amdgcn_perm(r2[3], r2[2], 0x07060302u)};
  return s;
}
// the six largest of the nine cross terms, the small ones first
__device__ __forceinline__ void six_products(f32x16 &acc, const s16x8 ah, const s16x8 am, const s16x8 al, const s16x8 bh, const s16x8 bm,
                                             const s16x8 bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}
// [k][64 bf16] images read transposed (wgrad: the operands are k-major): the two 64-byte halves of a row swapped on rows with (k >> 1) & 1
__device__ __forceinline__ int swz_tr(int k, int c) { return c ^ (((k >> 1) & 1) << 5); }
// [row][32 bf16] images read along the row by ds_read_b128 (fwd: the operands are k-contiguous): the four 16-byte slots of a 64-byte
// row rotated by (row >> 2) & 3, so that the 16 rows of a ds_read_b128 lane group fall on the 16 slots of the 256-byte bank row
__device__ __forceinline__ int swz_row(int row, int slot) { return slot ^ ((row >> 2) & 3); }

template <bool RAGGED>
__device__ __forceinline__ void wgrad_body_x3(const GroupArgs &ga_) {
  constexpr int BK = 32, ROWB = 128, PART = BK * ROWB, BUF = 2 * 3 * PART;      // bytes: row, (operand, part), buffer
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];                   // 48 KB; staging for the two reductions at the end
  int p = 0;
#pragma unroll
  for (int q = 1; q < kMaxPairs; ++q) p += (q < ga_.npairs && (int)blockIdx.x >= ga_.first[q]) ? 1 : 0;
  const float *__restrict__ G = static_cast<const float *>(ga_.g[p]);
  const float *__restrict__ X = static_cast<const float *>(ga_.x[p]);
  float *__restrict__ PW = static_cast<float *>(ga_.pw[p]);
  double *__restrict__ PB = ga_.pb[p];
  const int M = ga_.M[p], N = ga_.N[p], K = ga_.K;
  const float alpha = (float)ga_.alpha[p];
  const int bid = (int)blockIdx.x - ga_.first[p];
  const int split = bid % kSplit, tile = bid / kSplit;
  const int ntn = N / BN;
  const int tm = tile / ntn, tn = tile % ntn;
  // rows per K range: whole slabs; rows that do not exist (K is not a multiple of 8 slabs) are loaded as zeros
  const int kper = RAGGED ? (K + kSplit * BK - 1) / (kSplit * BK) * BK : K / kSplit, k0 = split * kper, nslab = kper / BK;
  constexpr bool ragged = RAGGED;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int kh = w >> 2, wm = w & 1, wn = (w >> 1) & 1;          // K half, tile row, tile column of this wave
  const int lrow = t >> 4, lc = t & 15;                          // this thread's vector of a slab: row lrow, columns 4 lc .. 4 lc + 3
  const bool bias = PB != nullptr;
  f32x4 gv, xv;
  float colsum[4] = {0.f, 0.f, 0.f, 0.f};
  float *pw = PW + (size_t)split * M * N;
  f32x16 acc, old;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  double *pbp = bias && t < BM ? PB + ((size_t)split * ntn + tn) * M + tm * BM + t : nullptr;
  auto swz = [](int k, int c) { return swz_tr(k, c); };

  auto gload = [&](int slab) {
    const int row = k0 + slab * BK + lrow;
    if (!ragged || row < K) {
      gv = *reinterpret_cast<const f32x4 *>(G + (size_t)row * M + tm * BM + lc * 4);
      xv = *reinterpret_cast<const f32x4 *>(X + (size_t)row * N + tn * BN + lc * 4);
    } else {
      gv = f32x4{0.f, 0.f, 0.f, 0.f}, xv = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto split_store = [&](const f32x4 v, char *base) {
    const Split3 s = split3(v);
    const int off = lrow * ROWB + swz(lrow, lc * 4) * 2;
    *reinterpret_cast<u32x2 *>(base + off) = s.hi;
    *reinterpret_cast<u32x2 *>(base + PART + off) = s.mid;
    *reinterpret_cast<u32x2 *>(base + 2 * PART + off) = s.lo;
  };
  // The workgroups of a tile row (tn = 0..ntn-1) see the same G slabs: slab s is added up by the one with tn == s % ntn.
  int mine = tn;                                                // the next slab whose column sums are this workgroup's
  auto lstore = [&](int slab, int buf) {
    char *b = smem + buf * BUF;
    const f32x4 g = alpha * gv;
    split_store(g, b);
    if (slab == mine) {
      mine += ntn;
      if (bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) colsum[e] += g[e];
      }
    }
    split_store(xv, b + 3 * PART);
  };
  // the operand fragment of v_mfma_f32_32x32x16_bf16 for this wave's 32 columns and its half of the slab's rows: lane l holds
  // element [k = 8 (l >> 5) + j][col0 + (l & 31)], j = 0..7 -- two transposed reads: lane 4q + p of a 16-lane group supplies the
  // address of row q, columns 4p .. 4p + 3 of the group's 4 x 16 block and receives column (lane & 15), rows 0..3
  const int g4 = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
  auto frag = [&](const char *part, int col0) -> s16x8 {
    s16x4 r[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = kh * 16 + 8 * (g4 >> 1) + 4 * u + q4;
      const int c = col0 + (g4 & 1) * 16 + 4 * p4;
      r[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(part + k * ROWB + swz(k, c) * 2));
    }
    const s16x8 f = {r[0][0], r[0][1], r[0][2], r[0][3], r[1][0], r[1][1], r[1][2], r[1][3]};
    return f;
  };
  auto compute = [&](int buf) {
    const char *b = smem + buf * BUF;
    const s16x8 ah = frag(b, wm * 32), am = frag(b + PART, wm * 32), al = frag(b + 2 * PART, wm * 32);
    const s16x8 bh = frag(b + 3 * PART, wn * 32), bm = frag(b + 4 * PART, wn * 32), bl = frag(b + 5 * PART, wn * 32);
    six_products(acc, ah, am, al, bh, bm, bl);
  };
  auto tile_row = [&](int e) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); };      // (C/D map of the 32 x 32 MFMAs: dtype-independent)

  gload(0);
  // what the earlier stages / time steps left in PW (and PB): BEHIND the first slab's loads (loads return in order)
#pragma unroll
  for (int e = 0; e < 16; ++e) old[e] = kh == 0 ? pw[(size_t)(tm * BM + wm * 32 + tile_row(e)) * N + tn * BN + wn * 32 + (lane & 31)] : 0.f;
  const double pbold = pbp ? *pbp : 0.0;
  lstore(0, 0);
  if (nslab > 1) gload(1);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    // the split and the stores of the next slab FIRST (its loads were issued a slab ago; the other buffer's last readers passed the
    // barrier before), the MFMAs behind them: they are still in the pipe while the wave goes on to the barrier (-4 % in
    // tools/mb_wgrad_bf16x3.hip, nothing measurable here)
    if (s + 1 < nslab) lstore(s + 1, (s + 1) & 1);
    compute(s & 1);
    if (s + 2 < nslab) gload(s + 2);
    __syncthreads();
  }
  float(*red)[64] = reinterpret_cast<float(*)[64]>(smem);
  double(*cs)[BM] = reinterpret_cast<double(*)[BM]>(smem + 4 * 16 * 64 * sizeof(float));
  static_assert(sizeof(smem) >= 4 * 16 * 64 * sizeof(float) + 8 * BM * sizeof(double), "the reductions are staged in the slab buffers");
  if (kh == 1) {
#pragma unroll
    for (int e = 0; e < 16; ++e) red[(w & 3) * 16 + e][lane] = acc[e];
  }
  if (bias) {
    // the four rows of a wave (lanes 16 apart hold the same columns) are added by shuffles, the eight waves through LDS: the last
    // thread's serial sum is 8 long, not 32 (it sits in the tail of every workgroup)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = colsum[e];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (lane < 16) cs[w][lc * 4 + e] = (double)v;
    }
  }
  __syncthreads();
  if (kh == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e)
      pw[(size_t)(tm * BM + wm * 32 + tile_row(e)) * N + tn * BN + wn * 32 + (lane & 31)] = old[e] + (acc[e] + red[(w & 3) * 16 + e][lane]);
  }
  if (pbp) {
    double sum = cs[0][t];
#pragma unroll
    for (int j = 1; j < 8; ++j) sum += cs[j][t];
    *pbp = pbold + sum;
  }
}

// The same product on workgroup tiles of 128 x 128 by SIXTEEN waves (1024 threads): 2 K halves x (2 x 4) wave tiles of 64 x 32 --
// two accumulators per wave, the three X fragments feed both.  What bounds the 64 x 64 form is not the matrix pipe but what feeds it:
// per MFMA 1 KB of fragments read from LDS, 0.5 KB of split parts stored, and the split's VALU work, done once per workgroup that
// shares a slab (8 of them at 512 columns).  Here: 0.75 KB read, 0.25 KB stored, half the split work per MFMA -- 14.3 against 17.2 us
// per 4096 x 512 x 512 pair, four pairs per launch (tools/mb_wgrad_bf16x3.hip, profiles/r06_microbench.txt).  12 parts of 4 KB per
// buffer, two buffers = 96 KB: ONE workgroup per CU, so the launcher takes this form only when the launch fills whole rounds of
// the chip.  The arithmetic of every element of dW and of db is that of the 64 x 64 form, operation for operation (same K ranges,
// same slabs, same order of the six terms, the K halves added last; db: per (row of a slab, column) float sums over the slabs the
// 64-wide tile column would have taken, rows paired as its shuffles pair them, eight double adds): the SAME BITS, so a result
// does not depend on which form a launch took -- tests/test_gpu_kernels.py compares them.
template <bool RAGGED>
__device__ __forceinline__ void wgrad_body_x3_wide(const GroupArgs &ga_) {
  constexpr int BK = 32, ROWB = 128, PART = BK * ROWB, BUF = 12 * PART, TM = 128, TN = 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];                   // 96 KB
  int p = 0;
#pragma unroll
  for (int q = 1; q < kMaxPairs; ++q) p += (q < ga_.npairs && (int)blockIdx.x >= ga_.first[q]) ? 1 : 0;
  const float *__restrict__ G = static_cast<const float *>(ga_.g[p]);
  const float *__restrict__ X = static_cast<const float *>(ga_.x[p]);
  float *__restrict__ PW = static_cast<float *>(ga_.pw[p]);
  double *__restrict__ PB = ga_.pb[p];
  const int M = ga_.M[p], N = ga_.N[p], K = ga_.K;
  const float alpha = (float)ga_.alpha[p];
  const int bid = (int)blockIdx.x - ga_.first[p];
  const int split = bid % kSplit, tile = bid / kSplit;
  const int ntn = N / TN, ntn64 = N / BN;
  const int tm = tile / ntn, tn = tile % ntn;
  const int kper = RAGGED ? (K + kSplit * BK - 1) / (kSplit * BK) * BK : K / kSplit, k0 = split * kper, nslab = kper / BK;
  constexpr bool ragged = RAGGED;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int kh = w >> 3, wm = w & 1, wn = (w >> 1) & 3;          // K half; rows 64 wm .. +63, columns 32 wn .. +31 of the tile
  const int lrow = t >> 5, lc5 = t & 31, sub = lc5 >> 4, lc = lc5 & 15;       // this thread's vector: row lrow, columns 4 lc5 .. +3 (64-column sub-tile `sub`)
  const bool bias = PB != nullptr;
  f32x4 gv, xv;
  float colsum[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float *pw = PW + (size_t)split * M * N;
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc0[e] = 0.f, acc1[e] = 0.f;
  // db: this workgroup stands for the 64-wide tile columns 2 tn and 2 tn + 1 of its tile row -- their slots of PB, their slabs
  double *pbp = bias && t < 2 * TM ? PB + ((size_t)split * ntn64 + 2 * tn + (t >> 7)) * M + tm * TM + (t & 127) : nullptr;
  auto swz = [](int k, int c) { return swz_tr(k, c); };

  auto gload = [&](int slab) {
    const int row = k0 + slab * BK + lrow;
    if (!ragged || row < K) {
      gv = *reinterpret_cast<const f32x4 *>(G + (size_t)row * M + tm * TM + lc5 * 4);
      xv = *reinterpret_cast<const f32x4 *>(X + (size_t)row * N + tn * TN + lc5 * 4);
    } else {
      gv = f32x4{0.f, 0.f, 0.f, 0.f}, xv = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto split_store = [&](const f32x4 v, char *base) {
    const Split3 s = split3(v);
    const int off = lrow * ROWB + swz(lrow, lc * 4) * 2;
    *reinterpret_cast<u32x2 *>(base + off) = s.hi;
    *reinterpret_cast<u32x2 *>(base + PART + off) = s.mid;
    *reinterpret_cast<u32x2 *>(base + 2 * PART + off) = s.lo;
  };
  int mine0 = 2 * tn, mine1 = 2 * tn + 1;                        // the next slabs of the two 64-wide tile columns
  auto lstore = [&](int slab, int buf) {
    char *b = smem + buf * BUF;
    const f32x4 g = alpha * gv;
    split_store(g, b + sub * 3 * PART);                          // G: two sub-tiles of 64 columns x (hi, mid, lo)
    if (slab == mine0) {
      mine0 += ntn64;
      if (bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) colsum[0][e] += g[e];
      }
    }
    if (slab == mine1) {
      mine1 += ntn64;
      if (bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) colsum[1][e] += g[e];
      }
    }
    split_store(xv, b + (6 + sub * 3) * PART);                   // X: the same
  };
  const int g4 = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
  auto frag = [&](const char *part, int col0) -> s16x8 {
    s16x4 r[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = kh * 16 + 8 * (g4 >> 1) + 4 * u + q4;
      const int c = col0 + (g4 & 1) * 16 + 4 * p4;
      r[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(part + k * ROWB + swz(k, c) * 2));
    }
    const s16x8 f = {r[0][0], r[0][1], r[0][2], r[0][3], r[1][0], r[1][1], r[1][2], r[1][3]};
    return f;
  };
  auto six = [&](f32x16 &acc, const s16x8 ah, const s16x8 am, const s16x8 al, const s16x8 bh, const s16x8 bm, const s16x8 bl) {
    six_products(acc, ah, am, al, bh, bm, bl);                                 // the order of the 64 x 64 form
  };
  auto compute = [&](int buf) {
    const char *b = smem + buf * BUF;
    const char *ga = b + wm * 3 * PART;                          // this wave's 64 rows of dW = G sub-tile wm
    const char *xb = b + (6 + (wn >> 1) * 3) * PART;
    const int bc = (wn & 1) * 32;
    const s16x8 bh = frag(xb, bc), bm = frag(xb + PART, bc), bl = frag(xb + 2 * PART, bc);
    {
      const s16x8 ah = frag(ga, 0), am = frag(ga + PART, 0), al = frag(ga + 2 * PART, 0);
      six(acc0, ah, am, al, bh, bm, bl);
    }
    {
      const s16x8 ah = frag(ga, 32), am = frag(ga + PART, 32), al = frag(ga + 2 * PART, 32);
      six(acc1, ah, am, al, bh, bm, bl);
    }
  };
  auto tile_row = [&](int e) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); };

  gload(0);
  const double pbold = pbp ? *pbp : 0.0;
  lstore(0, 0);
  if (nslab > 1) gload(1);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    if (s + 1 < nslab) lstore(s + 1, (s + 1) & 1);
    compute(s & 1);
    if (s + 2 < nslab) gload(s + 2);
    __syncthreads();
  }
  // the partial tile left by the earlier stages / time steps: loaded HERE (64 registers that the loop does not carry)
  f32x16 old0, old1;
  float *tp = pw + (size_t)(tm * TM + wm * 64) * N + tn * TN + wn * 32 + (lane & 31);
  if (kh == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) old0[e] = tp[(size_t)tile_row(e) * N], old1[e] = tp[(size_t)(32 + tile_row(e)) * N];
  }
  float(*red)[64] = reinterpret_cast<float(*)[64]>(smem);                                  // 8 waves x 32 values x 64 lanes = 64 KB
  float(*csf)[16][TM] = reinterpret_cast<float(*)[16][TM]>(smem + 8 * 32 * 64 * sizeof(float));      // + 16 KB
  static_assert(sizeof(smem) >= 8 * 32 * 64 * sizeof(float) + 2 * 16 * TM * sizeof(float), "the reductions are staged in the slab buffers");
  if (kh == 1) {
#pragma unroll
    for (int e = 0; e < 16; ++e) red[(w & 7) * 32 + e][lane] = acc0[e], red[(w & 7) * 32 + 16 + e][lane] = acc1[e];
  }
  if (bias) {
    // a wave holds two rows of the slab (lanes 32 apart: the same columns); the 64 x 64 form adds rows 4j .. 4j + 3 by shuffles in
    // float ((r0 + r1) + (r2 + r3)) and its eight waves in double: waves 2j and 2j + 1 here are its wave j
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = colsum[h][e];
        v += __shfl_xor(v, 32);
        if (lane < 32) csf[h][w][lc5 * 4 + e] = v;
      }
  }
  __syncthreads();
  if (kh == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      tp[(size_t)tile_row(e) * N] = old0[e] + (acc0[e] + red[(w & 7) * 32 + e][lane]);
      tp[(size_t)(32 + tile_row(e)) * N] = old1[e] + (acc1[e] + red[(w & 7) * 32 + 16 + e][lane]);
    }
  }
  if (pbp) {
    const int h = t >> 7, m = t & 127;
    double sum = (double)(csf[h][0][m] + csf[h][1][m]);
#pragma unroll
    for (int j = 1; j < 8; ++j) sum += (double)(csf[h][2 * j][m] + csf[h][2 * j + 1][m]);
    *pbp = pbold + sum;
  }
}

// (fp64: 128 VGPRs as it compiles, two workgroups per CU; its ragged form 131: one.)  fp32: at most 80 VGPRs, so that THREE workgroups fit a CU (six waves per SIMD; LDS 3 x 32 KB): while one is in its prologue or
// its tail the other two keep the matrix pipes busy.  fp64 needs 118 VGPRs (two per CU).
__global__ __launch_bounds__(kThreads, 6) void pn_linear_wgrad_kernel_f32(GroupArgs a) { wgrad_body<float, false>(a); }
__global__ __launch_bounds__(kThreads) void pn_linear_wgrad_kernel_f64(GroupArgs a) { wgrad_body<double, false>(a); }
__global__ __launch_bounds__(kThreads, 4) void pn_linear_wgrad_kernel_f32x3(GroupArgs a) { wgrad_body_x3<false>(a); }
__global__ __launch_bounds__(kThreads, 6) void pn_linear_wgrad_kernel_f32_ragged(GroupArgs a) { wgrad_body<float, true>(a); }
__global__ __launch_bounds__(kThreads) void pn_linear_wgrad_kernel_f64_ragged(GroupArgs a) { wgrad_body<double, true>(a); }
__global__ __launch_bounds__(kThreads, 4) void pn_linear_wgrad_kernel_f32x3_ragged(GroupArgs a) { wgrad_body_x3<true>(a); }
__global__ __launch_bounds__(1024, 4) void pn_linear_wgrad_kernel_f32x3w(GroupArgs a) { wgrad_body_x3_wide<false>(a); }
__global__ __launch_bounds__(1024, 4) void pn_linear_wgrad_kernel_f32x3w_ragged(GroupArgs a) { wgrad_body_x3_wide<true>(a); }

// mu_W += sum_s PW[s] (s = 0..7, in that order); PW = 0
template <typename T>
__global__ __launch_bounds__(256) void pn_linear_wgrad_finish_kernel(T *__restrict__ PW, size_t mn, T *__restrict__ mu) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(VEC)));
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (i >= mn) return;
  vec_t v[kSplit];
#pragma unroll
  for (int s = 0; s < kSplit; ++s) v[s] = *reinterpret_cast<const vec_t *>(PW + (size_t)s * mn + i);
  vec_t m = *reinterpret_cast<const vec_t *>(mu + i);
  vec_t sum = v[0];
#pragma unroll
  for (int s = 1; s < kSplit; ++s) sum += v[s];
  m += sum;
  *reinterpret_cast<vec_t *>(mu + i) = m;
  vec_t z;
#pragma unroll
  for (int e = 0; e < VEC; ++e) z[e] = (T)0;
#pragma unroll
  for (int s = 0; s < kSplit; ++s) *reinterpret_cast<vec_t *>(PW + (size_t)s * mn + i) = z;
}

template <typename T>
__global__ __launch_bounds__(256) void pn_linear_bgrad_finish_kernel(double *__restrict__ PB, int M, int parts, T *__restrict__ mu) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  double s = 0.0;
  int k = 0;
  for (; k + 8 <= parts; k += 8) {               // (parts = 8 * tile columns) eight loads in flight, added in index order
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = PB[(size_t)(k + j) * M + m];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; k < parts; ++k) s += PB[(size_t)k * M + m];
  mu[m] += (T)s;
  for (k = 0; k < parts; ++k) PB[(size_t)k * M + m] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The PIPELINED K loop of pn_linear_fwd / pn_linear_bwd on aligned shapes (the plain loops further down stay: the ragged bodies, an odd
// number of slabs -- K = 96, 160, ... --, and PN_LINEAR_FORM_PLAIN).  The plain loop runs three phases per slab that all eight waves enter together after the barrier -- split and
// store of the next slab (VALU), fragment reads (LDS latency, exposed), twelve MFMAs -- and the matrix pipe idles through the first two.
// Here every wave keeps TWO sets of fragment registers and TWO sets of load registers, and the slabs go through THREE LDS buffers.
// Step s, between two barriers:
//   * global loads of slab s + 3 are issued (they have two steps to arrive);
//   * the fragments of slab s + 1 are read from buffer (s + 1) % 3 into the set the MFMAs of slab s - 1 have left;
//   * the twelve MFMAs of slab s run from the set read one step ago -- no LDS read stands in front of an MFMA;
//   * slab s + 2 is split and stored to buffer (s + 2) % 3, spread between the MFMAs (__builtin_amdgcn_sched_group_barrier: per MFMA
//     one or two fragment reads, eight VALU, one ds_write_b64).
// What orders LDS: a buffer is read one step after the barrier that follows its stores, and stored again two steps after the barrier
// that follows its reads (__syncthreads waits for this wave's LDS operations before it signals) -- no read or store is ordered by
// anything but a barrier.  Every accumulator takes exactly the MFMAs of the plain loop in its order (slabs ascending, six_products,
// acc0 before acc1 is immaterial: they are separate chains), so the results are the plain loop's bit for bit.
struct Frags {                   // one slab's operand fragments of a wave: A (hi, mid, lo), B of accumulator 0, B of accumulator 1
  s16x8 ah, am, al, b0h, b0m, b0l, b1h, b1m, b1l;
};

template <int I, int NREAD, int RPG, bool RD, bool ST, int NVALU = 8>
__device__ __forceinline__ void pipe_groups() {
  if constexpr (I < 12) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                          // one MFMA
    constexpr int left = NREAD - I * RPG, nr = left < 0 ? 0 : (left < RPG ? left : RPG);
    if constexpr (ST) __builtin_amdgcn_sched_group_barrier(0x002, NVALU, 0);    // the split's VALU work
    if constexpr (RD && nr > 0) __builtin_amdgcn_sched_group_barrier(0x100, nr, 0);      // fragment reads of the next slab
    if constexpr (ST) {
      // its LDS stores (the nine ds_write_b64 of a thread leave the compiler as five: pairs a part apart go as ds_write2st64_b64)
      if constexpr (I >= 3 && (I & 1)) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    }
    pipe_groups<I + 1, NREAD, RPG, RD, ST, NVALU>();
  }
}

// NREAD: LDS read instructions per slab and wave (9 ds_read_b128 forward; 3 + 12 transposed ones backward); NLOAD: global loads per slab
// and thread.  gload(G &, slab), lstore(const G &, slab, byte offset of the buffer), read(Frags &, byte offset of the buffer).
// nslab is even and >= 2.
template <int NREAD, int NLOAD, typename G, int NVALU = 8, typename GL, typename LS, typename RF>
__device__ __forceinline__ void pipelined_slabs(const int nslab, const int BUF, f32x16 &acc0, f32x16 &acc1, GL gload, LS lstore, RF read) {
  constexpr int RPG = NREAD > 12 ? 2 : 1;
  G g0, g1;
  Frags f0, f1;
  int rb = BUF, wb = 2 * BUF, fb = 0;            // step s reads slab s + 1 from rb and stores slab s + 2 to wb
  // step s: loads slab s + 3 into gnxt, reads slab s + 1 into nxt, multiplies slab s from cur, splits and stores slab s + 2 from gcur
  auto step = [&](auto ld, auto rd, auto st, const Frags &cur, Frags &nxt, const G &gcur, G &gnxt, int s) {
    constexpr bool LD = decltype(ld)::value, RD = decltype(rd)::value, ST = decltype(st)::value;
    if constexpr (LD) gload(gnxt, s + 3);
    if constexpr (RD) read(nxt, rb);
    if constexpr (ST) lstore(gcur, s + 2, wb);
    six_products(acc0, cur.ah, cur.am, cur.al, cur.b0h, cur.b0m, cur.b0l);
    six_products(acc1, cur.ah, cur.am, cur.al, cur.b1h, cur.b1m, cur.b1l);
    if constexpr (LD) {                          // the global loads first, behind their addresses: they have two steps to arrive
      __builtin_amdgcn_sched_group_barrier(0x002, 2 * NLOAD, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, NLOAD, 0);
    }
    pipe_groups<0, NREAD, RPG, RD, ST, NVALU>();
    // nothing of a step moves across its barrier: the MFMAs of the next step would wait for fragments that were read just now
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    const int r = rb;
    rb = wb, wb = fb, fb = r;
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  gload(g0, 0);
  gload(g1, 1);
  lstore(g0, 0, 0);
  if (nslab > 2) gload(g0, 2);
  lstore(g1, 1, BUF);
  __syncthreads();
  read(f0, 0);
  __builtin_amdgcn_sched_barrier(0);
  int s = 0;
  for (; s + 4 < nslab; s += 2) {
    step(yes, yes, yes, f0, f1, g0, g1, s);
    step(yes, yes, yes, f1, f0, g1, g0, s + 1);
  }
  if (nslab >= 4) {                              // s == nslab - 4: the last two stores, the last load
    step(yes, yes, yes, f0, f1, g0, g1, s);
    step(no, yes, yes, f1, f0, g1, g0, s + 1);
    s += 2;
  }
  step(no, yes, no, f0, f1, g0, g1, s);          // s == nslab - 2
  step(no, no, no, f1, f0, g1, g0, s + 1);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The forward product of a Linear layer with its activation: Y = act(X W^T + b), X rows x in, W out x in, Y rows x out, row-major
// fp32 (pn_linear_fwd) -- func's Linear -> Tanh pairs in ONE launch instead of a library GEMM and an elementwise kernel.
// The arithmetic is the split-bf16 product above (split3, six_products).  What differs from wgrad is the shape: K = in is short
// (64 to a few thousand) and BOTH operands are k-contiguous, so
//   * no K split across workgroups: a workgroup of eight waves owns a 64 x 128 tile of Y over all of K and writes it once (4096 x 512:
//     256 workgroups, one per CU; workgroups are dealt to the XCDs round-robin, so the tile index is rotated to give each XCD a
//     contiguous range of tile rows: the four workgroups that share a 64-row slab of X share an L2);
//   * slabs of 32 k through two LDS buffers, one barrier per slab, as wgrad; LDS image per (operand, part): [row][32 bf16], 64-byte rows
//     whose 16-byte slots are rotated by swz_row; operand fragments by plain ds_read_b128 (lane l: row l & 31, k 8 (l >> 5) .. + 7 -- what
//     v_mfma_f32_32x32x16_bf16 takes as it lies in memory), conflict-free;
//   * waves 0-3 take k 0..15 of every slab, waves 4-7 k 16..31; a wave owns 32 x 64 of the tile (two accumulators, the three X
//     fragments feed both: 0.75 KB of fragments per MFMA).  At the end the two K halves swap one accumulator each through LDS and
//     each finishes ONE 32 x 32 block: (first half + second half) + bias, tanhf, one store -- all eight waves share the epilogue.
// Fixed order, no atomics: the same bits on every launch.  tanhf is the device library's (at most 2 ulp by its documentation; exactly +-1
// from |z| of about 9 on, NaN for NaN).  An infinite X or W gives NaN in the rows / columns it takes part in (inf - inf in the split).
// RAGGED: rows % 64 != 0 or out % 128 != 0 -- rows of X / W that do not exist are loaded as zeros, their outputs not stored.
constexpr int FM = 64, FN = 128, FK = 32, kFwdThreads = 512;

struct FwdArgs {
  const float *x, *w, *b;
  float *y;
  float *z;                      // the pre-activation beside y (pn_linear_fwd_pre), or null
  int rows, out_f, in_f, act, ntn;
};

// Exact GELU of the biased sum, y = z Phi(z): the one spelling of all three forms.  Contraction is off, so the three products and the add
// stay what they are wherever this is inlined: the same bits of y in every form.  erff is the device library's: exactly +-1 from |z| of
// about 5.6 on, so y is z itself (0.5 z * 2) above and -0 below (0.5 z * 0, z negative); 1 + erff cancels for negative z -- the error is
// small in absolute terms, large relative to y there; a NaN goes through.
__device__ __forceinline__ float gelu_y(const float z) {
#pragma clang fp contract(off)
  return 0.5f * z * (1.f + erff(z * 0.70710678f));
}

// Softplus of the biased sum at aten's default parameters (beta 1, threshold 20), aten's formula: z itself above the threshold (where
// log1pf(expf(z)) - z is below 2.1e-9, under half an ulp of z), else log1pf(expf(z)).  expf underflows to +0 from z of about -104 on:
// y is an exact +0; above that y is positive.  A NaN fails the comparison and goes through expf and log1pf.  Contraction has nothing to
// fuse here; it is off so that the spelling stays what is written wherever this is inlined.
__device__ __forceinline__ float softplus_y(const float z) {
#pragma clang fp contract(off)
  return z > 20.f ? z : log1pf(expf(z));
}

// ELU of the biased sum at alpha 1: z itself where z > 0, else expm1f(z) -- -0 for -0, exactly -1 from z of about -17.4 down; a NaN
// fails the comparison and goes through expm1f.
__device__ __forceinline__ float elu_y(const float z) {
#pragma clang fp contract(off)
  return z > 0.f ? z : expm1f(z);
}

struct FwdLoads {                // one slab's global loads of a thread
  f32x4 x, w0, w1;
};

// PIPE: the pipelined K loop (pipelined_slabs above; aligned shapes only), else the plain one
template <bool RAGGED, bool PIPE>
__device__ __forceinline__ void linear_fwd_body(const FwdArgs &a) {
  static_assert(!(RAGGED && PIPE), "the pipelined loop loads without tests");
  constexpr int ROWB = 2 * FK, XPART = FM * ROWB, WPART = FN * ROWB, BUF = 3 * XPART + 3 * WPART;      // bytes: 64, 4 K, 8 K, 36 K
  __shared__ __attribute__((aligned(16))) char smem[(PIPE ? 3 : 2) * BUF];                             // 72 KB; pipelined: 108 KB
  const float *__restrict__ X = a.x;
  const float *__restrict__ W = a.w;
  const int rows = a.rows, out_f = a.out_f, in_f = a.in_f, ntn = a.ntn;
  const int nblk = (int)gridDim.x, bid = (int)blockIdx.x;
  const int tile = nblk % 8 == 0 ? (bid & 7) * (nblk >> 3) + (bid >> 3) : bid;
  const int tm = tile / ntn, tn = tile % ntn;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int kh = w >> 2, wm = w & 1, wn = (w >> 1) & 1;          // K half; rows 32 wm .. + 31, columns 64 wn .. + 63 of the tile
  const int lrow = t >> 3, lc = t & 7;                           // this thread's vectors of a slab: rows lrow (X, W) and 64 + lrow (W), k 4 lc .. + 3
  const int nslab = in_f / FK;
  const bool xok = !RAGGED || tm * FM + lrow < rows;
  const bool wok0 = !RAGGED || tn * FN + lrow < out_f, wok1 = !RAGGED || tn * FN + 64 + lrow < out_f;
  const float *xp = X + (size_t)(tm * FM + lrow) * in_f + lc * 4;
  const float *wp0 = W + (size_t)(tn * FN + lrow) * in_f + lc * 4;
  const float *wp1 = wp0 + (size_t)64 * in_f;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 xv, wv0, wv1;
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc0[e] = 0.f, acc1[e] = 0.f;

  auto gload = [&](int slab) {
    xv = xok ? *reinterpret_cast<const f32x4 *>(xp + slab * FK) : zero4;
    wv0 = wok0 ? *reinterpret_cast<const f32x4 *>(wp0 + slab * FK) : zero4;
    wv1 = wok1 ? *reinterpret_cast<const f32x4 *>(wp1 + slab * FK) : zero4;
  };
  // (rows lrow and 64 + lrow rotate alike)
  const int soff = lrow * ROWB + (swz_row(lrow, lc >> 1) << 4) + ((lc & 1) << 3);
  auto split_store = [&](const f32x4 v, char *base, int part) {
    const Split3 s = split3(v);
    *reinterpret_cast<u32x2 *>(base + soff) = s.hi;
    *reinterpret_cast<u32x2 *>(base + part + soff) = s.mid;
    *reinterpret_cast<u32x2 *>(base + 2 * part + soff) = s.lo;
  };
  auto lstore = [&](int buf) {
    char *b = smem + buf * BUF;
    split_store(xv, b, XPART);
    split_store(wv0, b + 3 * XPART, WPART);
    split_store(wv1, b + 3 * XPART + 64 * ROWB, WPART);
  };
  // lane l: row r0 + (l & 31), this wave's K half, k 8 (l >> 5) .. + 7 of it
  auto frag = [&](const char *part, int r0) -> s16x8 {
    const int row = r0 + (lane & 31);
    return *reinterpret_cast<const s16x8 *>(part + row * ROWB + (swz_row(row, 2 * kh + (lane >> 5)) << 4));
  };
  auto compute = [&](int buf) {
    const char *xb = smem + buf * BUF, *wb = xb + 3 * XPART;
    const s16x8 ah = frag(xb, wm * 32), am = frag(xb + XPART, wm * 32), al = frag(xb + 2 * XPART, wm * 32);
    {
      const s16x8 bh = frag(wb, wn * 64), bm = frag(wb + WPART, wn * 64), bl = frag(wb + 2 * WPART, wn * 64);
      six_products(acc0, ah, am, al, bh, bm, bl);
    }
    {
      const s16x8 bh = frag(wb, wn * 64 + 32), bm = frag(wb + WPART, wn * 64 + 32), bl = frag(wb + 2 * WPART, wn * 64 + 32);
      six_products(acc1, ah, am, al, bh, bm, bl);
    }
  };

  if constexpr (PIPE) {
    pipelined_slabs<9, 3, FwdLoads>(
        nslab, BUF, acc0, acc1,
        [&](FwdLoads &g, int slab) {
          g.x = *reinterpret_cast<const f32x4 *>(xp + slab * FK);
          g.w0 = *reinterpret_cast<const f32x4 *>(wp0 + slab * FK);
          g.w1 = *reinterpret_cast<const f32x4 *>(wp1 + slab * FK);
        },
        [&](const FwdLoads &g, int, int boff) {
          char *b = smem + boff;
          split_store(g.x, b, XPART);
          split_store(g.w0, b + 3 * XPART, WPART);
          split_store(g.w1, b + 3 * XPART + 64 * ROWB, WPART);
        },
        [&](Frags &f, int boff) {
          const char *xb = smem + boff, *wb = xb + 3 * XPART;
          f.ah = frag(xb, wm * 32), f.am = frag(xb + XPART, wm * 32), f.al = frag(xb + 2 * XPART, wm * 32);
          f.b0h = frag(wb, wn * 64), f.b0m = frag(wb + WPART, wn * 64), f.b0l = frag(wb + 2 * WPART, wn * 64);
          f.b1h = frag(wb, wn * 64 + 32), f.b1m = frag(wb + WPART, wn * 64 + 32), f.b1l = frag(wb + 2 * WPART, wn * 64 + 32);
        });
  } else {
    gload(0);
    lstore(0);
    if (nslab > 1) gload(1);
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
      if (s + 1 < nslab) lstore((s + 1) & 1);         // the other buffer: its last readers passed the barrier of slab s - 1
      compute(s & 1);
      if (s + 2 < nslab) gload(s + 2);
      __syncthreads();
    }
  }
  // ---- the end (the slab buffers are free): K half 0 finishes block 0 of its wave tile, K half 1 block 1 of the same tile (waves w and
  // w ^ 4 hold the two halves of one tile): each hands the accumulator it does not finish to the other, [8 waves x 16 registers][64 lanes]
  float(*red)[64] = reinterpret_cast<float(*)[64]>(smem);
  static_assert(sizeof(smem) >= 8 * 16 * 64 * sizeof(float), "the exchange is staged in the slab buffers");
#pragma unroll
  for (int e = 0; e < 16; ++e) red[w * 16 + e][lane] = kh == 0 ? acc1[e] : acc0[e];
  __syncthreads();
  const int col = tn * FN + wn * 64 + kh * 32 + (lane & 31);
  const bool colok = !RAGGED || col < out_f;
  const float bias = (a.b != nullptr && colok) ? a.b[col] : 0.f;
  const int row0 = tm * FM + wm * 32 + 4 * (lane >> 5);          // (C/D map of the 32 x 32 MFMAs: register e is row (e & 3) + 8 (e >> 2) + 4 (lane >> 5))
  float *yp = a.y + (size_t)row0 * out_f + col;
  const bool tanh_act = a.act == PN_ACT_TANH;
  const bool relu_act = a.act == PN_ACT_RELU;
  // the Sigmoid epilogue is a loop of its own behind ONE uniform branch: inside the loop of the other three, its sixteen expf and
  // divisions cost the tanh pairs 0.2 us per launch (the headline, option absent: -0.68 % over five interleaved runs)
  // The GELU epilogue (gelu_y) is a loop of its own in the same way, and so is every epilogue that also stores the pre-activation
  // (a.z, pn_linear_fwd_pre): the loops of a launch without z are what they were before there was one -- one more uniform branch in
  // front of them.  With z: the biased sum goes to z at y's tile positions under y's guards, one more 4-byte store per element; the
  // GELU pairs -- the ones that save z -- have that loop to themselves, every other act shares one that tests act per element.
  // The Softplus and ELU epilogues (softplus_y, elu_y) are loops of their own too, behind the last two uniform branches, and with z as
  // well, as GELU's: as two more per-element tests inside the shared loop with z they cost all three kernels four scalar registers.
  auto finish = [&](auto own_c, auto pre_c) {
    constexpr int OWN = decltype(own_c)::value;                     // the act that has this loop to itself, or PN_ACT_IDENTITY: the shared one
    constexpr bool SIGMOID = OWN == PN_ACT_SIGMOID, GELU = OWN == PN_ACT_GELU, PRE = decltype(pre_c)::value;
    const bool sigmoid_act = a.act == PN_ACT_SIGMOID;               // (looked at by the shared loop with z only)
    float *zp = PRE ? a.z + (size_t)row0 * out_f + col : nullptr;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float other = red[(w ^ 4) * 16 + e][lane];
      const float first = kh == 0 ? acc0[e] : other, second = kh == 0 ? other : acc1[e];
      float z = (first + second) + bias;
      const float pre = z;
      if constexpr (GELU) {
        z = gelu_y(z);
      } else if constexpr (OWN == PN_ACT_SOFTPLUS) {
        z = softplus_y(z);
      } else if constexpr (OWN == PN_ACT_ELU) {
        z = elu_y(z);
      } else if constexpr (PRE) {
        if (sigmoid_act) z = 1.f / (1.f + expf(-z));                // (the Sigmoid loop's expression)
        if (tanh_act) z = tanhf(z);
        if (relu_act) z = z > 0.f ? z : (z == z ? 0.f : z);
      } else if constexpr (SIGMOID) {
        // the logistic function of the identity's value: expf within 1 ulp, one rounded add, one correctly rounded division (2.5 ulp of
        // 2^-24 in all, never above 1).  expf(-z) overflows to +inf from z <= -88.8 on: 1 / inf is +0; it is below 2^-25 from z >= 17.4
        // on: 1 / 1 is 1; a NaN goes through all three
        z = 1.f / (1.f + expf(-z));
      } else {
        if (tanh_act) z = tanhf(z);
        // relu of the identity's value: a positive z as it is, a NaN stays a NaN, everything else (-0 too) is +0 (not fmaxf: it drops a NaN)
        if (relu_act) z = z > 0.f ? z : (z == z ? 0.f : z);
      }
      const int r = (e & 3) + 8 * (e >> 2);
      if (colok && (!RAGGED || row0 + r < rows)) {
        yp[(size_t)r * out_f] = z;
        if constexpr (PRE) zp[(size_t)r * out_f] = pre;
      }
    }
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  constexpr std::integral_constant<int, PN_ACT_IDENTITY> shared{};
  constexpr std::integral_constant<int, PN_ACT_SIGMOID> sigmoid{};
  constexpr std::integral_constant<int, PN_ACT_GELU> gelu{};
  constexpr std::integral_constant<int, PN_ACT_SOFTPLUS> softplus{};
  constexpr std::integral_constant<int, PN_ACT_ELU> elu{};
  if (a.z != nullptr) {
    if (a.act == PN_ACT_GELU)
      finish(gelu, yes);
    else if (a.act == PN_ACT_SOFTPLUS)
      finish(softplus, yes);
    else if (a.act == PN_ACT_ELU)
      finish(elu, yes);
    else
      finish(shared, yes);
  } else if (a.act == PN_ACT_GELU)
    finish(gelu, no);
  else if (a.act == PN_ACT_SIGMOID)
    finish(sigmoid, no);
  else if (a.act == PN_ACT_SOFTPLUS)
    finish(softplus, no);
  else if (a.act == PN_ACT_ELU)
    finish(elu, no);
  else
    finish(shared, no);
}

// (pipelined: two sets of fragment and of load registers -- two waves per SIMD, as the LDS allows anyway)
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_fwd_kernel_f32x3(FwdArgs a) { linear_fwd_body<false, false>(a); }
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_fwd_kernel_f32x3_ragged(FwdArgs a) { linear_fwd_body<true, false>(a); }
__global__ __launch_bounds__(kFwdThreads, 2) void pn_linear_fwd_kernel_f32x3_pipe(FwdArgs a) { linear_fwd_body<false, true>(a); }

// ---------------------------------------------------------------------------------------------------------------------------------
// The backward of the same pair with respect to its input (pn_linear_bwd): for g, a rows x out, W out x in AS IT LIES,
//   gz[r][k] = g[r][k] (1 - a[r][k]^2)      dx[r][n] = sum_k gz[r][k] W[k][n]
// in ONE launch instead of an elementwise kernel and a library GEMM.  The sibling of linear_fwd_body: the same 64 x 128 tile of the
// output over all of K (= out here) per workgroup of eight waves, the same slabs of 32 k through two LDS buffers, the same XCD rotation,
// K halves, exchange at the end and ragged form; 36 KB per buffer as there.  What differs is where the operands come from:
//   * A = gz is k-contiguous like the forward's x: a thread loads the f32x4 of g and of a, forms gz in fp32 in registers (1 - a a may
//     contract to an fma), splits it into the [row][32 bf16] image (swz_row, ds_read_b128 fragments).  The workgroups of tile column 0
//     also store that f32x4 to gz in HBM: every element of gz is written by exactly one workgroup -- the cotangent pn_linear_wgrad reads;
//   * B = W is NOT k-contiguous: a slab is 32 rows k of W, 128 columns n, read along n (coalesced f32x4) and stored as two
//     [32 k][64 bf16] images per part -- wgrad's layout (swz_tr) -- whose fragments are wgrad's transposed reads.  No transposed copy
//     of W is kept anywhere: an optimiser changes W in place between two replays of a captured sweep.
// Fixed order, no atomics, no work buffers: the same bits on every launch.  A NaN or Inf in g or a stays in its row of gz and dx (an
// infinite gz gives NaN in its row of dx: inf - inf in the split, as an infinite W does in its columns); a == +-1 with finite g: gz == 0.
struct BwdArgs {
  const float *g, *a, *w;
  float *gz, *dx;
  int rows, out_f, in_f, ntn;
};

struct BwdLoads {
  f32x4 g, a, w0, w1;
};

// BARE: the layer has no activation behind it (pn_linear_dx): z = g -- its bits unchanged --, no load of a, nothing stored to gz (q.a and
// q.gz are null and never touched); the tile map, the W images, the order of the products and the exchange are the tanh body's, so dx has
// the bits this body gives for a == 0 (g (1 - 0 0) is g exactly, with or without the fma).
// ACT: the activation behind the layer, a's: PN_ACT_TANH (above), PN_ACT_IDENTITY (BARE) or PN_ACT_RELU (pn_linear_bwd_act):
//   gz[r][k] = a[r][k] <= 0 ? +0 : g[r][k]
// -- aten.threshold_backward(g, a, 0): a NaN in a lets g through, a == +-0 gives +0.  No arithmetic touches g: every element of gz is
// g's bits or +0, so gz is threshold_backward's bit for bit and dx is what the bare body gives when fed that gz, in every form.
// PN_ACT_SIGMOID (pn_linear_bwd_act), a the pair's output sigma(z):
//   gz[r][k] = g[r][k] (a[r][k] - a[r][k]^2)
// by sigmoid_gz below, the one spelling of all three forms: the same bits of gz in each, and dx is what the bare body gives when fed it.
// a in {0, 1} with finite g: gz == 0; a NaN in a or g stays in its element; g = +-inf where a (1 - a) is 0: NaN (aten.sigmoid_backward's).

// s = a - a a in ONE fma (a (1 - a) with one rounding, exactly 0 at a == 0 and a == 1), then ONE rounded product: two roundings in gz.
// Contraction is off so that the product stays a product wherever this is inlined: in the pipelined loop it would otherwise be fused
// into the split's first subtraction (fma(g, s, -hi)) -- other mid and lo terms, other bits in dx than the plain loop's.
__device__ __forceinline__ f32x4 sigmoid_gz(const f32x4 g, const f32x4 a) {
#pragma clang fp contract(off)
  f32x4 z;
#pragma unroll
  for (int e = 0; e < 4; ++e) z[e] = g[e] * __builtin_fmaf(-a[e], a[e], a[e]);
  return z;
}

// PN_ACT_GELU (pn_linear_bwd_act): the operand called a holds the pair's PRE-activation z (GELU is not monotonic: z cannot be had from
// the output), and
//   gz[r][k] = g[r][k] d,   d = cdf + z pdf,   cdf = 0.5 (1 + erff(z 0.70710678)),   pdf = expf(-0.5 z z) 0.3989423
// -- aten.gelu_backward's formula (approximate='none') by gelu_gz below, the one spelling of all three forms, contraction off: the same
// bits of gz in each, and dx is what the bare body gives when fed it.  d is 1 from z = 6 on (gz == g); from -6 down cdf is 0 and d = z pdf,
// below 4e-8 in size and an exact -0 once expf underflows (z below -14.4); a NaN in z or g stays in its element; g = +-inf where d is 0: NaN.
__device__ __forceinline__ f32x4 gelu_gz(const f32x4 g, const f32x4 zin) {
#pragma clang fp contract(off)
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float z = zin[e];
    const float cdf = 0.5f * (1.f + erff(z * 0.70710678f));
    const float pdf = expf(-0.5f * z * z) * 0.3989423f;
    r[e] = g[e] * (cdf + z * pdf);
  }
  return r;
}

// PN_ACT_SOFTPLUS (pn_linear_bwd_act), a the pair's output log(1 + e^z) >= 0:
//   gz[r][k] = g[r][k] (1 - e^(-a[r][k]))
// -- sigma(z) written in the OUTPUT: 1 - e^(-a) = e^z / (1 + e^z).  -expm1f(-a) has no cancellation for any a >= 0: exactly 1 from a of
// about 17.4 on (gz == g; the forward's y == z branch starts at 20), +-0 at a == 0 (z below -104).  ONE rounded product, contraction off
// (sigmoid_gz says why); a NaN in a or g stays in its element; g = +-inf at a == 0: NaN.
__device__ __forceinline__ f32x4 softplus_gz(const f32x4 g, const f32x4 a) {
#pragma clang fp contract(off)
  f32x4 z;
#pragma unroll
  for (int e = 0; e < 4; ++e) z[e] = g[e] * (-expm1f(-a[e]));
  return z;
}

// PN_ACT_ELU (pn_linear_bwd_act), a the pair's output (alpha 1: z where z > 0, else e^z - 1):
//   gz[r][k] = a[r][k] > 0 ? g[r][k] : g[r][k] (a[r][k] + 1)
// -- aten.elu_backward on the result: g's bits where a > 0; else one rounded add (e^z from the output) and ONE rounded product,
// contraction off.  The comparison is a > 0 and not a <= 0, so that a NaN in a takes the arithmetic branch and gives a NaN (ReLU's
// comparison lets g through); a == -1 with finite g gives 0.
__device__ __forceinline__ f32x4 elu_gz(const f32x4 g, const f32x4 a) {
#pragma clang fp contract(off)
  f32x4 z;
#pragma unroll
  for (int e = 0; e < 4; ++e) z[e] = a[e] > 0.f ? g[e] : g[e] * (a[e] + 1.f);
  return z;
}

template <bool RAGGED, bool PIPE, int ACT = PN_ACT_TANH>
__device__ __forceinline__ void linear_bwd_body(const BwdArgs &q) {
  static_assert(!(RAGGED && PIPE), "the pipelined loop loads without tests");
  static_assert(ACT == PN_ACT_TANH || ACT == PN_ACT_IDENTITY || ACT == PN_ACT_RELU || ACT == PN_ACT_SIGMOID || ACT == PN_ACT_GELU ||
                    ACT == PN_ACT_SOFTPLUS || ACT == PN_ACT_ELU,
                "tanh, none, ReLU, sigmoid, GELU, softplus or ELU");
  constexpr bool BARE = ACT == PN_ACT_IDENTITY, RELU = ACT == PN_ACT_RELU, SIGMOID = ACT == PN_ACT_SIGMOID, GELU = ACT == PN_ACT_GELU;
  constexpr bool SOFTPLUS = ACT == PN_ACT_SOFTPLUS, ELU = ACT == PN_ACT_ELU;
  // VALU instructions per MFMA group of the pipelined loop (pipe_groups): the split's eight, plus room for the prologue's -- ELU's
  // sixteen per step (a compare, an add, a product and a select per element), Softplus' four inlined expm1f.  With the siblings' eight
  // the work that does not fit piles up behind the last MFMA and the kernels need 234 and 230 VGPRs; so: 227 and 225 (Sigmoid: 228)
  constexpr int PVALU = ELU ? 12 : (SOFTPLUS ? 24 : 8);
  constexpr int AROWB = 2 * FK, APART = FM * AROWB;              // gz: [64 rows][32 bf16], 4 KB per part
  constexpr int WROWB = 128, WIMG = FK * WROWB, WPART = 2 * WIMG;      // W: two [32 k][64 bf16] images, 8 KB per part
  constexpr int BUF = 3 * APART + 3 * WPART;                     // 36 KB
  __shared__ __attribute__((aligned(16))) char smem[(PIPE ? 3 : 2) * BUF];      // 72 KB; pipelined: 108 KB
  const float *__restrict__ G = q.g;
  const float *__restrict__ A = q.a;
  const float *__restrict__ W = q.w;
  const int rows = q.rows, out_f = q.out_f, in_f = q.in_f, ntn = q.ntn;
  const int nblk = (int)gridDim.x, bid = (int)blockIdx.x;
  const int tile = nblk % 8 == 0 ? (bid & 7) * (nblk >> 3) + (bid >> 3) : bid;
  const int tm = tile / ntn, tn = tile % ntn;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int kh = w >> 2, wm = w & 1, wn = (w >> 1) & 1;          // K half; rows 32 wm .. + 31, columns 64 wn .. + 63 of the tile
  const int lrow = t >> 3, lc = t & 7;                           // gz: row lrow of the tile, k 4 lc .. + 3 of the slab
  const int krow = t >> 5, sub = (t >> 4) & 1, kc = t & 15;      // W: rows k krow and 16 + krow of the slab, columns 64 sub + 4 kc .. + 3 of the tile
  const int nslab = out_f / FK;
  const bool aok = !RAGGED || tm * FM + lrow < rows;
  const bool wok = !RAGGED || tn * FN + sub * 64 + kc * 4 < in_f;
  const bool keep = !BARE && tn == 0 && aok;                     // this workgroup writes gz
  const size_t aoff = (size_t)(tm * FM + lrow) * out_f + lc * 4;
  const float *wp = W + (size_t)krow * in_f + tn * FN + sub * 64 + kc * 4;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 gv, av, wv0, wv1;
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc0[e] = 0.f, acc1[e] = 0.f;

  auto gload = [&](int slab) {
    gv = aok ? *reinterpret_cast<const f32x4 *>(G + aoff + slab * FK) : zero4;
    if constexpr (!BARE) av = aok ? *reinterpret_cast<const f32x4 *>(A + aoff + slab * FK) : zero4;
    wv0 = wok ? *reinterpret_cast<const f32x4 *>(wp + (size_t)(slab * FK) * in_f) : zero4;
    wv1 = wok ? *reinterpret_cast<const f32x4 *>(wp + (size_t)(slab * FK + 16) * in_f) : zero4;
  };
  const int aso = lrow * AROWB + (swz_row(lrow, lc >> 1) << 4) + ((lc & 1) << 3);
  // (rows k krow and 16 + krow swap alike)
  const int wso = sub * WIMG + krow * WROWB + swz_tr(krow, kc * 4) * 2;
  auto split_store = [&](const f32x4 v, char *base, int part) {
    const Split3 s = split3(v);
    *reinterpret_cast<u32x2 *>(base) = s.hi;
    *reinterpret_cast<u32x2 *>(base + part) = s.mid;
    *reinterpret_cast<u32x2 *>(base + 2 * part) = s.lo;
  };
  auto lstore = [&](int slab, int buf) {
    char *b = smem + buf * BUF;
    f32x4 z = gv;                                                // here, not at the load: the products would wait for the loads in front of the MFMAs
    if constexpr (RELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) z[e] = av[e] <= 0.f ? 0.f : gv[e];
      if (keep) *reinterpret_cast<f32x4 *>(q.gz + aoff + slab * FK) = z;
    } else if constexpr (SIGMOID) {
      z = sigmoid_gz(gv, av);
      if (keep) *reinterpret_cast<f32x4 *>(q.gz + aoff + slab * FK) = z;
    } else if constexpr (GELU) {
      z = gelu_gz(gv, av);
      if (keep) *reinterpret_cast<f32x4 *>(q.gz + aoff + slab * FK) = z;
    } else if constexpr (SOFTPLUS || ELU) {
      z = SOFTPLUS ? softplus_gz(gv, av) : elu_gz(gv, av);
      if (keep) *reinterpret_cast<f32x4 *>(q.gz + aoff + slab * FK) = z;
    } else if constexpr (!BARE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) z[e] = gv[e] * (1.f - av[e] * av[e]);
      if (keep) *reinterpret_cast<f32x4 *>(q.gz + aoff + slab * FK) = z;
    }
    split_store(z, b + aso, APART);
    split_store(wv0, b + 3 * APART + wso, WPART);
    split_store(wv1, b + 3 * APART + wso + 16 * WROWB, WPART);
  };
  // gz, lane l: row r0 + (l & 31), this wave's K half, k 8 (l >> 5) .. + 7 of it (linear_fwd_body::frag)
  auto afrag = [&](const char *part, int r0) -> s16x8 {
    const int row = r0 + (lane & 31);
    return *reinterpret_cast<const s16x8 *>(part + row * AROWB + (swz_row(row, 2 * kh + (lane >> 5)) << 4));
  };
  // W, lane l: element [k = 8 (l >> 5) + j][col0 + (l & 31)] of this wave's K half of a [32 k][64] image, j = 0..7 (wgrad_body_x3::frag)
  const int g4 = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
  auto wfrag = [&](const char *img, int col0) -> s16x8 {
    s16x4 r[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = kh * 16 + 8 * (g4 >> 1) + 4 * u + q4;
      const int c = col0 + (g4 & 1) * 16 + 4 * p4;
      r[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(img + k * WROWB + swz_tr(k, c) * 2));
    }
    const s16x8 f = {r[0][0], r[0][1], r[0][2], r[0][3], r[1][0], r[1][1], r[1][2], r[1][3]};
    return f;
  };
  auto compute = [&](int buf) {
    const char *ab = smem + buf * BUF, *wb = ab + 3 * APART + wn * WIMG;      // this wave's 64 columns: image wn
    const s16x8 ah = afrag(ab, wm * 32), am = afrag(ab + APART, wm * 32), al = afrag(ab + 2 * APART, wm * 32);
    {
      const s16x8 bh = wfrag(wb, 0), bm = wfrag(wb + WPART, 0), bl = wfrag(wb + 2 * WPART, 0);
      six_products(acc0, ah, am, al, bh, bm, bl);
    }
    {
      const s16x8 bh = wfrag(wb, 32), bm = wfrag(wb + WPART, 32), bl = wfrag(wb + 2 * WPART, 32);
      six_products(acc1, ah, am, al, bh, bm, bl);
    }
  };

  if constexpr (PIPE) {
    // (the store of gz is a branch of its own in the plain loop; here the loop is instantiated with and without it, so that a step
    // stays one basic block for the interleave)
    auto run = [&](auto keep_c) {
      constexpr bool KEEP = decltype(keep_c)::value;
      pipelined_slabs<15, BARE ? 3 : 4, BwdLoads, PVALU>(
          nslab, BUF, acc0, acc1,
          [&](BwdLoads &l, int slab) {
            l.g = *reinterpret_cast<const f32x4 *>(G + aoff + slab * FK);
            if constexpr (!BARE) l.a = *reinterpret_cast<const f32x4 *>(A + aoff + slab * FK);
            l.w0 = *reinterpret_cast<const f32x4 *>(wp + (size_t)(slab * FK) * in_f);
            l.w1 = *reinterpret_cast<const f32x4 *>(wp + (size_t)(slab * FK + 16) * in_f);
          },
          [&](const BwdLoads &l, int slab, int boff) {
            char *b = smem + boff;
            // gz as the plain loop forms it, spelled out: 1 - a a in one fma, then ONE rounded product.  Left to contraction, the product
            // here is fused into the split's first subtraction (fma(g, t, -hi)): other mid and lo terms, other bits in dx
            f32x4 z = l.g;
            if constexpr (RELU) {                // (nothing to contract: a compare and a select)
#pragma unroll
              for (int e = 0; e < 4; ++e) z[e] = l.a[e] <= 0.f ? 0.f : l.g[e];
            } else if constexpr (SIGMOID) {
              z = sigmoid_gz(l.g, l.a);
            } else if constexpr (GELU) {
              z = gelu_gz(l.g, l.a);
            } else if constexpr (SOFTPLUS || ELU) {
              z = SOFTPLUS ? softplus_gz(l.g, l.a) : elu_gz(l.g, l.a);
            } else if constexpr (!BARE) {
#pragma clang fp contract(off)
#pragma unroll
              for (int e = 0; e < 4; ++e) z[e] = l.g[e] * __builtin_fmaf(-l.a[e], l.a[e], 1.f);
            }
            if constexpr (KEEP) *reinterpret_cast<f32x4 *>(q.gz + aoff + slab * FK) = z;
            split_store(z, b + aso, APART);
            split_store(l.w0, b + 3 * APART + wso, WPART);
            split_store(l.w1, b + 3 * APART + wso + 16 * WROWB, WPART);
          },
          [&](Frags &f, int boff) {
            const char *ab = smem + boff, *wb = ab + 3 * APART + wn * WIMG;
            f.ah = afrag(ab, wm * 32), f.am = afrag(ab + APART, wm * 32), f.al = afrag(ab + 2 * APART, wm * 32);
            f.b0h = wfrag(wb, 0), f.b0m = wfrag(wb + WPART, 0), f.b0l = wfrag(wb + 2 * WPART, 0);
            f.b1h = wfrag(wb, 32), f.b1m = wfrag(wb + WPART, 32), f.b1l = wfrag(wb + 2 * WPART, 32);
          });
    };
    if constexpr (BARE)
      run(std::false_type{});
    else if (keep)
      run(std::true_type{});
    else
      run(std::false_type{});
  } else {
    gload(0);
    lstore(0, 0);
    if (nslab > 1) gload(1);
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
      if (s + 1 < nslab) lstore(s + 1, (s + 1) & 1);  // the other buffer: its last readers passed the barrier of slab s - 1
      compute(s & 1);
      if (s + 2 < nslab) gload(s + 2);
      __syncthreads();
    }
  }
  // ---- the end, as the forward's: K half 0 finishes block 0 of its wave tile, K half 1 block 1; each hands the other its accumulator
  float(*red)[64] = reinterpret_cast<float(*)[64]>(smem);
  static_assert(sizeof(smem) >= 8 * 16 * 64 * sizeof(float), "the exchange is staged in the slab buffers");
#pragma unroll
  for (int e = 0; e < 16; ++e) red[w * 16 + e][lane] = kh == 0 ? acc1[e] : acc0[e];
  __syncthreads();
  const int col = tn * FN + wn * 64 + kh * 32 + (lane & 31);
  const bool colok = !RAGGED || col < in_f;
  const int row0 = tm * FM + wm * 32 + 4 * (lane >> 5);
  float *dp = q.dx + (size_t)row0 * in_f + col;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float other = red[(w ^ 4) * 16 + e][lane];
    const float first = kh == 0 ? acc0[e] : other, second = kh == 0 ? other : acc1[e];
    const int r = (e & 3) + 8 * (e >> 2);
    if (colok && (!RAGGED || row0 + r < rows)) dp[(size_t)r * in_f] = first + second;
  }
}

__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_kernel_f32x3(BwdArgs a) { linear_bwd_body<false, false>(a); }
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_kernel_f32x3_ragged(BwdArgs a) { linear_bwd_body<true, false>(a); }
__global__ __launch_bounds__(kFwdThreads, 2) void pn_linear_bwd_kernel_f32x3_pipe(BwdArgs a) { linear_bwd_body<false, true>(a); }
// the bare ones (pn_linear_dx): a and gz of BwdArgs are null
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_dx_kernel_f32x3(BwdArgs a) { linear_bwd_body<false, false, PN_ACT_IDENTITY>(a); }
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_dx_kernel_f32x3_ragged(BwdArgs a) { linear_bwd_body<true, false, PN_ACT_IDENTITY>(a); }
__global__ __launch_bounds__(kFwdThreads, 2) void pn_linear_dx_kernel_f32x3_pipe(BwdArgs a) { linear_bwd_body<false, true, PN_ACT_IDENTITY>(a); }
// the ReLU pairs' (pn_linear_bwd_act with PN_ACT_RELU): the launch bounds of their tanh siblings
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_relu_kernel_f32x3(BwdArgs a) { linear_bwd_body<false, false, PN_ACT_RELU>(a); }
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_relu_kernel_f32x3_ragged(BwdArgs a) { linear_bwd_body<true, false, PN_ACT_RELU>(a); }
__global__ __launch_bounds__(kFwdThreads, 2) void pn_linear_bwd_relu_kernel_f32x3_pipe(BwdArgs a) { linear_bwd_body<false, true, PN_ACT_RELU>(a); }
// the Sigmoid pairs' (pn_linear_bwd_act with PN_ACT_SIGMOID): the same
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_sigmoid_kernel_f32x3(BwdArgs a) { linear_bwd_body<false, false, PN_ACT_SIGMOID>(a); }
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_sigmoid_kernel_f32x3_ragged(BwdArgs a) { linear_bwd_body<true, false, PN_ACT_SIGMOID>(a); }
__global__ __launch_bounds__(kFwdThreads, 2) void pn_linear_bwd_sigmoid_kernel_f32x3_pipe(BwdArgs a) { linear_bwd_body<false, true, PN_ACT_SIGMOID>(a); }
// the GELU pairs' (pn_linear_bwd_act with PN_ACT_GELU; a of BwdArgs is the pre-activation): the same
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_gelu_kernel_f32x3(BwdArgs a) { linear_bwd_body<false, false, PN_ACT_GELU>(a); }
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_gelu_kernel_f32x3_ragged(BwdArgs a) { linear_bwd_body<true, false, PN_ACT_GELU>(a); }
__global__ __launch_bounds__(kFwdThreads, 2) void pn_linear_bwd_gelu_kernel_f32x3_pipe(BwdArgs a) { linear_bwd_body<false, true, PN_ACT_GELU>(a); }
// the Softplus and ELU pairs' (pn_linear_bwd_act with PN_ACT_SOFTPLUS / PN_ACT_ELU): the same
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_softplus_kernel_f32x3(BwdArgs a) { linear_bwd_body<false, false, PN_ACT_SOFTPLUS>(a); }
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_softplus_kernel_f32x3_ragged(BwdArgs a) { linear_bwd_body<true, false, PN_ACT_SOFTPLUS>(a); }
__global__ __launch_bounds__(kFwdThreads, 2) void pn_linear_bwd_softplus_kernel_f32x3_pipe(BwdArgs a) { linear_bwd_body<false, true, PN_ACT_SOFTPLUS>(a); }
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_elu_kernel_f32x3(BwdArgs a) { linear_bwd_body<false, false, PN_ACT_ELU>(a); }
__global__ __launch_bounds__(kFwdThreads, 4) void pn_linear_bwd_elu_kernel_f32x3_ragged(BwdArgs a) { linear_bwd_body<true, false, PN_ACT_ELU>(a); }
__global__ __launch_bounds__(kFwdThreads, 2) void pn_linear_bwd_elu_kernel_f32x3_pipe(BwdArgs a) { linear_bwd_body<false, true, PN_ACT_ELU>(a); }

int cu_count() {
  static int n = 0;             // (the calling thread's current device; every device of a node is the same part)
  if (n == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      n = v;
    else
      n = 256;
  }
  return n;
}

// the byte ranges [p, p + np) and [r, r + nr) share a byte (a null r: an operand that is not there shares none)
bool overlap(const void *p, size_t np, const void *r, size_t nr) {
  if (r == nullptr) return false;
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(p), r0 = reinterpret_cast<uintptr_t>(r);
  return p0 < r0 + nr && r0 < p0 + np;
}

template <typename T>
int finish_t(hipStream_t st, int64_t out_f, int64_t in_f, void *pw, void *pb, void *mu_w, void *mu_b) {
  const size_t mn = (size_t)out_f * (size_t)in_f;
  constexpr int VEC = 16 / (int)sizeof(T);
  const char *name = "pn_linear_wgrad_finish";
  int rc = pn::launch(name, pn_linear_wgrad_finish_kernel<T>, dim3((unsigned)((mn / VEC + 255) / 256)), dim3(256), st, (T *)pw, mn, (T *)mu_w);
  if (!rc && pb != nullptr && mu_b != nullptr)
    rc = pn::launch(name, pn_linear_bgrad_finish_kernel<T>, dim3((unsigned)((out_f + 255) / 256)), dim3(256), st, (double *)pb, (int)out_f,
                    (int)(kSplit * (in_f / BN)), (T *)mu_b);
  return rc;
}

// what pn_linear_bwd_form and pn_linear_bwd_act share behind their own checks of `flags` (and of `act`): the shape rules, the null,
// alignment and aliasing refusals, the choice of the form; act is PN_ACT_TANH, PN_ACT_RELU, PN_ACT_SIGMOID, PN_ACT_GELU, PN_ACT_SOFTPLUS
// or PN_ACT_ELU
int bwd_pair(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *a, const void *w, int act,
             void *gz, void *dx, int flags) {
  if (!pn_linear_bwd_supported(dtype, rows, out_f, in_f)) return pn::fail("pn_linear_bwd: unsupported dtype or shape (see pn_linear_bwd_supported)");
  if (g == nullptr || a == nullptr || w == nullptr || gz == nullptr || dx == nullptr) return pn::fail("pn_linear_bwd: null operand");
  if (!pn::aligned16(g, a, w, gz, dx)) return pn::fail("pn_linear_bwd: operands must be 16-byte aligned");
  // an output that shares bytes with anything else the launch touches: other workgroups still read (or also write) them
  const size_t nz = (size_t)rows * (size_t)out_f * sizeof(float), nw = (size_t)out_f * (size_t)in_f * sizeof(float),
               nx = (size_t)rows * (size_t)in_f * sizeof(float);
  if (overlap(gz, nz, g, nz) || overlap(gz, nz, a, nz) || overlap(gz, nz, w, nw))
    return pn::fail("pn_linear_bwd: gz must not alias g, a or w (other workgroups still read them)");
  if (overlap(dx, nx, g, nz) || overlap(dx, nx, a, nz) || overlap(dx, nx, w, nw) || overlap(dx, nx, gz, nz))
    return pn::fail("pn_linear_bwd: dx must not alias g, a, w or gz");
  BwdArgs q;
  q.g = (const float *)g, q.a = (const float *)a, q.w = (const float *)w, q.gz = (float *)gz, q.dx = (float *)dx;
  q.rows = (int)rows, q.out_f = (int)out_f, q.in_f = (int)in_f;
  q.ntn = (int)((in_f + FN - 1) / FN);
  const unsigned blocks = (unsigned)((rows + FM - 1) / FM) * (unsigned)q.ntn;
  const bool ragged = rows % FM != 0 || in_f % FN != 0;
  const bool plain = (flags & PN_LINEAR_FORM_PLAIN) || (out_f / FK) % 2 != 0;      // (the pipelined loop takes an even number of slabs)
  if (act == PN_ACT_RELU) {
    auto kern = ragged ? pn_linear_bwd_relu_kernel_f32x3_ragged : (plain ? pn_linear_bwd_relu_kernel_f32x3 : pn_linear_bwd_relu_kernel_f32x3_pipe);
    return pn::launch("pn_linear_bwd_act", kern, dim3(blocks), dim3(kFwdThreads), (hipStream_t)stream, q);
  }
  if (act == PN_ACT_SIGMOID) {
    auto kern = ragged ? pn_linear_bwd_sigmoid_kernel_f32x3_ragged
                       : (plain ? pn_linear_bwd_sigmoid_kernel_f32x3 : pn_linear_bwd_sigmoid_kernel_f32x3_pipe);
    return pn::launch("pn_linear_bwd_act", kern, dim3(blocks), dim3(kFwdThreads), (hipStream_t)stream, q);
  }
  if (act == PN_ACT_GELU) {
    auto kern = ragged ? pn_linear_bwd_gelu_kernel_f32x3_ragged : (plain ? pn_linear_bwd_gelu_kernel_f32x3 : pn_linear_bwd_gelu_kernel_f32x3_pipe);
    return pn::launch("pn_linear_bwd_act", kern, dim3(blocks), dim3(kFwdThreads), (hipStream_t)stream, q);
  }
  if (act == PN_ACT_SOFTPLUS) {
    auto kern = ragged ? pn_linear_bwd_softplus_kernel_f32x3_ragged
                       : (plain ? pn_linear_bwd_softplus_kernel_f32x3 : pn_linear_bwd_softplus_kernel_f32x3_pipe);
    return pn::launch("pn_linear_bwd_act", kern, dim3(blocks), dim3(kFwdThreads), (hipStream_t)stream, q);
  }
  if (act == PN_ACT_ELU) {
    auto kern = ragged ? pn_linear_bwd_elu_kernel_f32x3_ragged : (plain ? pn_linear_bwd_elu_kernel_f32x3 : pn_linear_bwd_elu_kernel_f32x3_pipe);
    return pn::launch("pn_linear_bwd_act", kern, dim3(blocks), dim3(kFwdThreads), (hipStream_t)stream, q);
  }
  auto kern = ragged ? pn_linear_bwd_kernel_f32x3_ragged : (plain ? pn_linear_bwd_kernel_f32x3 : pn_linear_bwd_kernel_f32x3_pipe);
  return pn::launch("pn_linear_bwd", kern, dim3(blocks), dim3(kFwdThreads), (hipStream_t)stream, q);
}

// what pn_linear_fwd_form and pn_linear_fwd_pre share behind their own checks of `flags` (and of a null z): z is the second output or null
int fwd_pair(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *x, const void *w, const void *b, int act,
             void *y, void *z, int flags) {
  if (!pn_linear_fwd_supported(dtype, rows, out_f, in_f)) return pn::fail("pn_linear_fwd: unsupported dtype or shape (see pn_linear_fwd_supported)");
  if (act != PN_ACT_IDENTITY && act != PN_ACT_TANH && act != PN_ACT_RELU && act != PN_ACT_SIGMOID && act != PN_ACT_GELU &&
      act != PN_ACT_SOFTPLUS && act != PN_ACT_ELU)
    return pn::fail("pn_linear_fwd: act is PN_ACT_IDENTITY, PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID or PN_ACT_GELU or PN_ACT_SOFTPLUS or PN_ACT_ELU");
  if (x == nullptr || w == nullptr || y == nullptr) return pn::fail("pn_linear_fwd: null operand");
  if (!pn::aligned16(x, w, y) || (reinterpret_cast<uintptr_t>(b) & 3)) return pn::fail("pn_linear_fwd: operands must be 16-byte aligned");
  // an output that shares bytes with anything the launch reads: other workgroups still read x, w and b while a tile of y is stored
  const size_t ny = (size_t)rows * (size_t)out_f * sizeof(float), nx = (size_t)rows * (size_t)in_f * sizeof(float),
               nw = (size_t)out_f * (size_t)in_f * sizeof(float), nb = (size_t)out_f * sizeof(float);
  if (overlap(y, ny, x, nx) || overlap(y, ny, w, nw) || overlap(y, ny, b, nb))
    return pn::fail("pn_linear_fwd: y must not alias x, w or b (other workgroups still read them)");
  if (z != nullptr) {              // (pn_linear_fwd_pre) the second output: y's size, y's rules, and no byte of y
    if (!pn::aligned16(z)) return pn::fail("pn_linear_fwd_pre: z must be 16-byte aligned");
    if (overlap(z, ny, y, ny) || overlap(z, ny, x, nx) || overlap(z, ny, w, nw) || overlap(z, ny, b, nb))
      return pn::fail("pn_linear_fwd_pre: z must not alias y, x, w or b");
  }
  FwdArgs a;
  a.x = (const float *)x, a.w = (const float *)w, a.b = (const float *)b, a.y = (float *)y, a.z = (float *)z;
  a.rows = (int)rows, a.out_f = (int)out_f, a.in_f = (int)in_f, a.act = act;
  a.ntn = (int)((out_f + FN - 1) / FN);
  const unsigned blocks = (unsigned)((rows + FM - 1) / FM) * (unsigned)a.ntn;
  const bool ragged = rows % FM != 0 || out_f % FN != 0;
  const bool plain = (flags & PN_LINEAR_FORM_PLAIN) || (in_f / FK) % 2 != 0;       // (the pipelined loop takes an even number of slabs)
  auto kern = ragged ? pn_linear_fwd_kernel_f32x3_ragged : (plain ? pn_linear_fwd_kernel_f32x3 : pn_linear_fwd_kernel_f32x3_pipe);
  return pn::launch("pn_linear_fwd", kern, dim3(blocks), dim3(kFwdThreads), (hipStream_t)stream, a);
}

}  // namespace

extern "C" {

int pn_linear_wgrad_supported(int dtype, int64_t rows, int64_t out_f, int64_t in_f) {
  if (dtype != PN_F32 && dtype != PN_F64) return 0;
  // any number of rows from 256 on (a K range is rounded up to whole slabs of 32 rows, the missing rows are zeros); fewer rows than
  // that leave most of the eight K ranges empty: the general path then
  return (rows >= 256 && rows < (int64_t)1 << 30 && out_f > 0 && out_f % BM == 0 && in_f > 0 && in_f % BN == 0 && out_f * in_f <= kMaxWeights) ? 1 : 0;
}

int64_t pn_linear_wgrad_work_bytes(int dtype, int64_t out_f, int64_t in_f, int64_t *bias_bytes) {
  if (bias_bytes) *bias_bytes = (int64_t)kSplit * (in_f / BN) * out_f * (int64_t)sizeof(double);
  return (int64_t)kSplit * out_f * in_f * (int64_t)(dtype == PN_F64 ? sizeof(double) : sizeof(float));
}

int pn_linear_wgrad_group(void *stream, int dtype, int64_t rows, int npairs, const pn_wgrad_pair *pairs, int flags) {
  if (npairs < 1 || npairs > kMaxPairs) return pn::fail("pn_linear_wgrad_group: 1 <= npairs <= PN_WGRAD_MAX_PAIRS");
  GroupArgs a;
  a.npairs = npairs;
  a.K = (int)rows;
  int64_t blocks = 0, wblocks = 0;
  double flops = 0;
  bool wide = dtype == PN_F32 && !(flags & (PN_WGRAD_EXACT_FP32 | PN_WGRAD_TILE_64));
  for (int p = 0; p < kMaxPairs; ++p) {
    const pn_wgrad_pair &q = pairs[p < npairs ? p : 0];
    if (p < npairs) {
      if (!pn_linear_wgrad_supported(dtype, rows, q.out_f, q.in_f))
        return pn::fail("pn_linear_wgrad: unsupported dtype or shape (see pn_linear_wgrad_supported)");
      if (!pn::aligned16(q.g, q.x, q.pw)) return pn::fail("pn_linear_wgrad: operands must be 16-byte aligned");
      if (q.g == nullptr || q.x == nullptr || q.pw == nullptr) return pn::fail("pn_linear_wgrad: null operand");
    }
    a.g[p] = q.g, a.x[p] = q.x, a.pw[p] = q.pw, a.pb[p] = (double *)q.pb, a.alpha[p] = q.alpha;
    a.M[p] = (int)q.out_f, a.N[p] = (int)q.in_f;
    if (p < npairs) {
      flops += 2.0 * (double)rows * (double)q.out_f * (double)q.in_f;
      wblocks += (q.out_f / 128) * (q.in_f / 128) * kSplit;
      if (q.out_f % 128 || q.in_f % 128) wide = false;
    }
  }
  // The 128 x 128 form runs ONE workgroup per CU: taken when the launch fills whole rounds of the chip (at most a fifth of the last
  // round idle) -- the four 512 x 512 layers of a stage VJP are two rounds of 256 -- and not by a single small layer, which the
  // 64 x 64 form spreads over four times as many workgroups.  Same bits either way (wgrad_body_x3_wide).
  if (wide) {
    const int64_t ncu = cu_count(), rounds = (wblocks + ncu - 1) / ncu;
    wide = wblocks >= ncu && rounds * ncu * 5 <= wblocks * 6;
  }
  for (int p = 0; p < kMaxPairs; ++p) {
    a.first[p] = (int)blocks;
    if (p < npairs) blocks += wide ? (pairs[p].out_f / 128) * (pairs[p].in_f / 128) * kSplit : (pairs[p].out_f / BM) * (pairs[p].in_f / BN) * kSplit;
  }
  a.first[kMaxPairs] = (int)blocks;
  for (int p = npairs; p < kMaxPairs; ++p) a.first[p] = (int)blocks;
  if (blocks > (int64_t)1 << 30) return pn::fail("pn_linear_wgrad_group: too many workgroups");
  hipStream_t st = (hipStream_t)stream;
  const bool ragged = rows % (kSplit * 32) != 0;
  if (wide) {
    auto kw = ragged ? pn_linear_wgrad_kernel_f32x3w_ragged : pn_linear_wgrad_kernel_f32x3w;
    return pn::launch(PN_K_LINEAR_WGRAD, flops, kw, dim3((unsigned)blocks), dim3(1024), st, a);
  }
  auto kern = dtype == PN_F64 ? (ragged ? pn_linear_wgrad_kernel_f64_ragged : pn_linear_wgrad_kernel_f64)
                              : ((flags & PN_WGRAD_EXACT_FP32) ? (ragged ? pn_linear_wgrad_kernel_f32_ragged : pn_linear_wgrad_kernel_f32)
                                                               : (ragged ? pn_linear_wgrad_kernel_f32x3_ragged : pn_linear_wgrad_kernel_f32x3));
  return pn::launch(PN_K_LINEAR_WGRAD, flops, kern, dim3((unsigned)blocks), dim3(kThreads), st, a);
}

int pn_linear_wgrad(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *x, double alpha,
                    void *pw, void *pb) {
  pn_wgrad_pair q;
  q.g = g, q.x = x, q.pw = pw, q.pb = pb, q.alpha = alpha, q.out_f = out_f, q.in_f = in_f;
  return pn_linear_wgrad_group(stream, dtype, rows, 1, &q, 0);
}

int pn_linear_wgrad_finish(void *stream, int dtype, int64_t out_f, int64_t in_f, void *pw, void *pb, void *mu_w, void *mu_b) {
  if (dtype != PN_F32 && dtype != PN_F64) return pn::fail("pn_linear_wgrad_finish: fp32 or fp64");
  if (!pn::aligned16(pw, mu_w)) return pn::fail("pn_linear_wgrad_finish: operands must be 16-byte aligned");
  return pn::with_dtype(dtype, [&](auto t) { return finish_t<decltype(t)>((hipStream_t)stream, out_f, in_f, pw, pb, mu_w, mu_b); });
}

int pn_linear_fwd_supported(int dtype, int64_t rows, int64_t out_f, int64_t in_f) {
  if (dtype != PN_F32) return 0;
  const int64_t lim = (int64_t)1 << 30;
  // (K = in_f: whole slabs of 32, at least two; an odd number of them takes the plain loop)
  if (!(rows >= 256 && rows < lim && out_f > 0 && out_f < lim && out_f % 64 == 0 && in_f >= 64 && in_f < lim && in_f % FK == 0)) return 0;
  return ((rows + FM - 1) / FM) * ((out_f + FN - 1) / FN) < lim ? 1 : 0;
}

int pn_linear_fwd(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *x, const void *w, const void *b, int act,
                  void *y) {
  return pn_linear_fwd_form(stream, dtype, rows, out_f, in_f, x, w, b, act, y, 0);
}

int pn_linear_fwd_form(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *x, const void *w, const void *b,
                       int act, void *y, int flags) {
  if (flags & ~PN_LINEAR_FORM_PLAIN) return pn::fail("pn_linear_fwd_form: unknown flag (PN_LINEAR_FORM_PLAIN is the only one)");
  return fwd_pair(stream, dtype, rows, out_f, in_f, x, w, b, act, y, nullptr, flags);
}

int pn_linear_fwd_pre(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *x, const void *w, const void *b, int act,
                      void *y, void *z, int flags) {
  if (flags & ~PN_LINEAR_FORM_PLAIN) return pn::fail("pn_linear_fwd_pre: unknown flag (PN_LINEAR_FORM_PLAIN is the only one)");
  if (z == nullptr) return pn::fail("pn_linear_fwd_pre: z is null (y alone: pn_linear_fwd_form)");
  return fwd_pair(stream, dtype, rows, out_f, in_f, x, w, b, act, y, z, flags);
}
int pn_linear_bwd_supported(int dtype, int64_t rows, int64_t out_f, int64_t in_f) {
  if (dtype != PN_F32) return 0;
  const int64_t lim = (int64_t)1 << 30;
  // (K = out_f: whole slabs of 32, at least two; an odd number of them takes the plain loop)
  if (!(rows >= 256 && rows < lim && out_f >= 64 && out_f < lim && out_f % FK == 0 && in_f > 0 && in_f < lim && in_f % 64 == 0)) return 0;
  return ((rows + FM - 1) / FM) * ((in_f + FN - 1) / FN) < lim ? 1 : 0;
}

int pn_linear_bwd(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *a, const void *w, void *gz,
                  void *dx) {
  return pn_linear_bwd_form(stream, dtype, rows, out_f, in_f, g, a, w, gz, dx, 0);
}

int pn_linear_bwd_form(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *a, const void *w,
                       void *gz, void *dx, int flags) {
  if (flags & ~PN_LINEAR_FORM_PLAIN) return pn::fail("pn_linear_bwd_form: unknown flag (PN_LINEAR_FORM_PLAIN is the only one)");
  return bwd_pair(stream, dtype, rows, out_f, in_f, g, a, w, PN_ACT_TANH, gz, dx, flags);
}

int pn_linear_bwd_act(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *a, const void *w, int act,
                      void *gz, void *dx, int flags) {
  if (flags & ~PN_LINEAR_FORM_PLAIN) return pn::fail("pn_linear_bwd_act: unknown flag (PN_LINEAR_FORM_PLAIN is the only one)");
  if (act == PN_ACT_IDENTITY) return pn::fail("pn_linear_bwd_act: PN_ACT_IDENTITY has no prologue and no gz: use pn_linear_dx");
  if (act != PN_ACT_TANH && act != PN_ACT_RELU && act != PN_ACT_SIGMOID && act != PN_ACT_GELU && act != PN_ACT_SOFTPLUS && act != PN_ACT_ELU)
    return pn::fail("pn_linear_bwd_act: act is PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID or PN_ACT_GELU or PN_ACT_SOFTPLUS or PN_ACT_ELU "
                    "(PN_ACT_IDENTITY: use pn_linear_dx)");
  return bwd_pair(stream, dtype, rows, out_f, in_f, g, a, w, act, gz, dx, flags);
}

int pn_linear_dx_supported(int dtype, int64_t rows, int64_t out_f, int64_t in_f) { return pn_linear_bwd_supported(dtype, rows, out_f, in_f); }

int pn_linear_dx(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *w, void *dx) {
  return pn_linear_dx_form(stream, dtype, rows, out_f, in_f, g, w, dx, 0);
}

int pn_linear_dx_form(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *w, void *dx, int flags) {
  if (flags & ~PN_LINEAR_FORM_PLAIN) return pn::fail("pn_linear_dx_form: unknown flag (PN_LINEAR_FORM_PLAIN is the only one)");
  if (!pn_linear_dx_supported(dtype, rows, out_f, in_f)) return pn::fail("pn_linear_dx: unsupported dtype or shape (see pn_linear_dx_supported)");
  if (g == nullptr || w == nullptr || dx == nullptr) return pn::fail("pn_linear_dx: null operand");
  if (!pn::aligned16(g, w, dx)) return pn::fail("pn_linear_dx: operands must be 16-byte aligned");
  const size_t ng = (size_t)rows * (size_t)out_f * sizeof(float), nw = (size_t)out_f * (size_t)in_f * sizeof(float),
               nx = (size_t)rows * (size_t)in_f * sizeof(float);
  if (overlap(dx, nx, g, ng) || overlap(dx, nx, w, nw)) return pn::fail("pn_linear_dx: dx must not alias g or w (other workgroups still read them)");
  BwdArgs q;
  q.g = (const float *)g, q.a = nullptr, q.w = (const float *)w, q.gz = nullptr, q.dx = (float *)dx;
  q.rows = (int)rows, q.out_f = (int)out_f, q.in_f = (int)in_f;
  q.ntn = (int)((in_f + FN - 1) / FN);
  const unsigned blocks = (unsigned)((rows + FM - 1) / FM) * (unsigned)q.ntn;
  const bool ragged = rows % FM != 0 || in_f % FN != 0;
  const bool plain = (flags & PN_LINEAR_FORM_PLAIN) || (out_f / FK) % 2 != 0;      // (the pipelined loop takes an even number of slabs)
  auto kern = ragged ? pn_linear_dx_kernel_f32x3_ragged : (plain ? pn_linear_dx_kernel_f32x3 : pn_linear_dx_kernel_f32x3_pipe);
  return pn::launch("pn_linear_dx", kern, dim3(blocks), dim3(kFwdThreads), (hipStream_t)stream, q);
}

}  // extern "C"
