// pnode_amd -- the two reductions behind the gradient with respect to the output times: scalar
// products of stage cotangents with stage derivatives, accumulated into one fp64 slot per output time on the device.  See
// include/pnode_amd.h, section 3a''.
//
// Both kernels stream their vectors once with 16-byte lane-contiguous loads (a scalar form of the same kernel when a base
// address or the row stride is not 16-byte aligned), sum in double per thread, reduce each workgroup with the wave-64
// shuffle tree and publish one partial per workgroup and sum; the workgroup that draws the last ticket adds the partials
// in index order (pn_device.h: no float atomics, bit-reproducible) and writes the slot.  The grid is capped at
// kTgMaxBlocks workgroups and depends on n alone, so the same call gives the same bits.  Coefficients are kernel
// arguments; nothing synchronises with the host, so the launches are capturable.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "pnode_amd.h"
#include "pn_launch.h"
#include "pn_device.h"

namespace {

constexpr int kTgMaxBlocks = 1024;

template <typename T>
struct TgDotArgs {
  const T *x[PN_MAX_STAGES];
  const T *y[PN_MAX_STAGES];
  double c[PN_MAX_STAGES];
  double *acc;                              // the slot written
  int accumulate;
};

template <typename T>
struct TgDenseArgs {
  const T *g;
  int64_t ld;                               // row stride of `g`, elements
  const T *k[PN_MAX_STAGES];
  double c[PN_DENSE_CHUNK][PN_MAX_STAGES];  // beta'_j(theta_o)
  double *acc;                              // acc[o], o < m
  int m;
  int accumulate;
};

// acc[0] (+)= sum_p c_p <x_p, y_p>: per element the pairs in p order, per thread the elements in grid-stride order
template <typename T, int NP, int VW>
__global__ __launch_bounds__(kBlock) void pn_tgrad_dots_kernel(TgDotArgs<T> a, double *work, int64_t nvec, int64_t n) {
  using V = Vec<T, VW>;
  double *partial = work + kTicketDoubles;
  double s = 0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += stride) {
    V xv[NP], yv[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      xv[p] = reinterpret_cast<const V *>(a.x[p])[i];
      yv[p] = reinterpret_cast<const V *>(a.y[p])[i];
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      double d = 0;
#pragma unroll
      for (int e = 0; e < VW; ++e) d += (double)xv[p][e] * (double)yv[p][e];
      s += a.c[p] * d;
    }
  }
  if (VW > 1 && blockIdx.x == 0) {
    const int64_t q = nvec * VW + threadIdx.x;
    if (q < n) {
#pragma unroll
      for (int p = 0; p < NP; ++p) s += a.c[p] * ((double)a.x[p][q] * (double)a.y[p][q]);
    }
  }
  const double b = block_sum(s);
  if (threadIdx.x == 0) publish_partial(partial + blockIdx.x, b);
  __syncthreads();
  if (draw_ticket(work, gridDim.x, blockIdx.x)) {
    const double tot = ordered_sum(partial, (int)gridDim.x);
    if (threadIdx.x == 0) a.acc[0] = a.accumulate ? a.acc[0] + tot : tot;
  }
}

// acc[o] (+)= sum_j c[o][j] <g_o, K_j>, o < m: the K_j of a thread's elements are loaded once, then every row g_o once.
// The m per-thread sums live in a fully unrolled register array (indices are compile-time constants: no scratch).
template <typename T, int NK, int VW>
__global__ __launch_bounds__(kBlock) void pn_rk_dense_tgrad_kernel(TgDenseArgs<T> a, double *work, int64_t nvec, int64_t n) {
  using V = Vec<T, VW>;
  double *partial = work + kTicketDoubles;
  double s[PN_DENSE_CHUNK];
#pragma unroll
  for (int o = 0; o < PN_DENSE_CHUNK; ++o) s[o] = 0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += stride) {
    V k[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) k[j] = reinterpret_cast<const V *>(a.k[j])[i];
#pragma unroll
    for (int o = 0; o < PN_DENSE_CHUNK; ++o) {
      if (o < a.m) {
        const V g = reinterpret_cast<const V *>(a.g + (int64_t)o * a.ld)[i];
#pragma unroll
        for (int j = 0; j < NK; ++j) {
          double d = 0;
#pragma unroll
          for (int e = 0; e < VW; ++e) d += (double)g[e] * (double)k[j][e];
          s[o] += a.c[o][j] * d;
        }
      }
    }
  }
  if (VW > 1 && blockIdx.x == 0) {
    const int64_t q = nvec * VW + threadIdx.x;
    if (q < n) {
      T k[NK];
#pragma unroll
      for (int j = 0; j < NK; ++j) k[j] = a.k[j][q];
#pragma unroll
      for (int o = 0; o < PN_DENSE_CHUNK; ++o) {
        if (o < a.m) {
          const double g = (double)a.g[(int64_t)o * a.ld + q];
#pragma unroll
          for (int j = 0; j < NK; ++j) s[o] += a.c[o][j] * (g * (double)k[j]);
        }
      }
    }
  }
  // the workgroup's m sums: every wave reduces all of its rows, one barrier, then thread o adds the waves' values in order
  constexpr int kWaves = kBlock / kWave;
  __shared__ double lds[kWaves][PN_DENSE_CHUNK];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
  for (int o = 0; o < PN_DENSE_CHUNK; ++o) {
    if (o < a.m) {
      const double v = wave_sum(s[o]);
      if (lane == 0) lds[wid][o] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < a.m) {
    double b = 0;
    for (int w = 0; w < kWaves; ++w) b += lds[w][threadIdx.x];
    publish_partial(partial + (int64_t)threadIdx.x * gridDim.x + blockIdx.x, b);
  }
  // (draw_ticket: lane 0 of wave 0 drains its stores before it draws; rows published by the other lanes of wave 0 leave with
  // them, since m <= PN_DENSE_CHUNK < kWave keeps every publishing lane inside wave 0)
  if (draw_ticket(work, gridDim.x, blockIdx.x)) {
    // one wave per row: lanes stride the workgroup partials in index order, then the wave tree
    for (int o = wid; o < a.m; o += kWaves) {
      double t = 0;
      for (int b = lane; b < (int)gridDim.x; b += kWave) t += read_partial(partial + (int64_t)o * gridDim.x + b);
      t = wave_sum(t);
      if (lane == 0) a.acc[o] = a.accumulate ? a.acc[o] + t : t;
    }
  }
}

template <typename T>
int tgrad_dots(hipStream_t st, int64_t n, int np, const void *const *x, const void *const *y, const double *coef, void *work,
               double *acc, int accumulate) {
  TgDotArgs<T> a = {};
  const bool vec = pn::aligned16(x, np) && pn::aligned16(y, np);
  for (int p = 0; p < np; ++p) {
    a.x[p] = (const T *)x[p];
    a.y[p] = (const T *)y[p];
    a.c[p] = coef[p];
  }
  a.acc = acc;
  a.accumulate = accumulate ? 1 : 0;
  double *w = (double *)work;
  const int rc = pn::with_count<1, PN_MAX_STAGES>(np, [&](auto N) {
    return pn::with_width<T>(vec, [&](auto W) {
      constexpr int NP = decltype(N)::value, VW = decltype(W)::value;
      const int64_t nvec = n / VW;
      return pn::launch("pn_tgrad_dots", pn_tgrad_dots_kernel<T, NP, VW>, dim3((unsigned)pn::blocks_for(nvec, kBlock, kTgMaxBlocks)),
                        dim3(kBlock), st, a, w, nvec, n);
    });
  });
  return pn::or_fail(rc, "pn_tgrad_dots: np must be 1..7");
}

template <typename T>
int dense_tgrad(hipStream_t st, int64_t n, int m, const void *g, int64_t ld, int nk, const void *const *K, const double *coef,
                void *work, double *acc, int accumulate) {
  constexpr int VW = 16 / sizeof(T);
  const bool vec = pn::aligned16(g) && (ld % VW) == 0 && pn::aligned16(K, nk);
  double *w = (double *)work;
  for (int o0 = 0; o0 < m; o0 += PN_DENSE_CHUNK) {
    TgDenseArgs<T> a = {};
    a.g = (const T *)g + (int64_t)o0 * ld;
    a.ld = ld;
    a.m = m - o0 < PN_DENSE_CHUNK ? m - o0 : PN_DENSE_CHUNK;
    a.acc = acc + o0;
    a.accumulate = accumulate ? 1 : 0;
    for (int j = 0; j < nk; ++j) a.k[j] = (const T *)K[j];
    for (int o = 0; o < a.m; ++o)
      for (int j = 0; j < nk; ++j) a.c[o][j] = coef[(int64_t)(o0 + o) * nk + j];
    const int rc = pn::with_count<1, PN_MAX_STAGES>(nk, [&](auto N) {
      return pn::with_width<T>(vec, [&](auto W) {
        constexpr int NK = decltype(N)::value, VW = decltype(W)::value;
        const int64_t nvec = n / VW;
        return pn::launch("pn_rk_dense_tgrad", pn_rk_dense_tgrad_kernel<T, NK, VW>, dim3((unsigned)pn::blocks_for(nvec, kBlock, kTgMaxBlocks)),
                          dim3(kBlock), st, a, w, nvec, n);
      });
    });
    if (rc) return pn::or_fail(rc, "pn_rk_dense_tgrad: nk must be 1..7");
  }
  return 0;
}

}  // namespace

extern "C" {

int64_t pn_tgrad_work_bytes(int64_t n) {
  (void)n;
  return (int64_t)sizeof(double) * (kTicketDoubles + (int64_t)PN_DENSE_CHUNK * kTgMaxBlocks);
}

int pn_tgrad_dots(void *stream, int dtype, int64_t n, int np, const void *const *x, const void *const *y, const double *coef,
                  void *work, double *acc, int accumulate) {
  if (np < 1 || np > PN_MAX_STAGES) return pn::fail("pn_tgrad_dots: np must be 1..7");
  if (!x || !y || !coef || !work || !acc) return pn::fail("pn_tgrad_dots: null argument");
  for (int p = 0; p < np; ++p)
    if (!x[p] || !y[p]) return pn::fail("pn_tgrad_dots: null vector");
  if (n < 0) return pn::fail("pn_tgrad_dots: negative length");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return tgrad_dots<decltype(t)>(st, n, np, x, y, coef, work, acc, accumulate); });
  return pn::or_fail(rc, "pn_tgrad_dots: unknown dtype");
}

int pn_rk_dense_tgrad(void *stream, int dtype, int64_t n, int m, const void *g, int64_t ld, int nk, const void *const *K,
                      const double *coef, void *work, double *acc, int accumulate) {
  if (m <= 0) return 0;
  if (!g || !K || !coef || !work || !acc) return pn::fail("pn_rk_dense_tgrad: null argument");
  if (nk < 1 || nk > PN_MAX_STAGES) return pn::fail("pn_rk_dense_tgrad: nk must be 1..7");
  if (n < 0) return pn::fail("pn_rk_dense_tgrad: negative length");
  if (ld < n) return pn::fail("pn_rk_dense_tgrad: row stride shorter than a row");
  for (int j = 0; j < nk; ++j)
    if (!K[j]) return pn::fail("pn_rk_dense_tgrad: null stage derivative");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return dense_tgrad<decltype(t)>(st, n, m, g, ld, nk, K, coef, work, acc, accumulate); });
  return pn::or_fail(rc, "pn_rk_dense_tgrad: unknown dtype");
}

}  // extern "C"
