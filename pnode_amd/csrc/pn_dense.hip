// pnode_amd -- dense output of the explicit-RK sweeps (-pn_output_times interpolate): the continuous extension of a step
// evaluated at all its output times in ONE launch, and its transpose for the reverse sweep.  See include/pnode_amd.h,
// section 3a'.
//
// Both kernels are HBM streams like pn_lincomb_kernel (pn_kernels.hip): 16-byte lane-contiguous accesses, every input of
// a thread loaded before the first use, a ragged tail (n not a multiple of the vector width) done by the first lanes of
// block 0, and a scalar form of the same kernel when a base address or the row stride is not 16-byte aligned.  The grid is
// capped at kDenseMaxBlocks workgroups and grid-strides over the rest.  The coefficients are kernel arguments (at most
// PN_DENSE_CHUNK rows of PN_MAX_STAGES), read with uniform indices: scalar LOADS of the argument segment, nothing else.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "pnode_amd.h"
#include "pn_launch.h"
#include "pn_device.h"

namespace {

constexpr int kDenseMaxBlocks = 2048;

template <typename T>
struct DenseEvalArgs {
  const T *u;
  const T *k[PN_MAX_STAGES];
  T *out;
  int64_t ld;                               // row stride of `out`, elements
  int m;                                    // output rows of this launch
  T c[PN_DENSE_CHUNK][PN_MAX_STAGES];       // h*beta_j(theta_o), rounded once from double
};

template <typename T>
struct DenseAdjArgs {
  const T *g;
  int64_t ld;                               // row stride of `g`, elements
  int m;
  int accumulate;
  T *d[PN_MAX_STAGES];
  T *G;                                     // may be null
  T c[PN_DENSE_CHUNK][PN_MAX_STAGES];
};

// out_o = u + sum_j c[o][j] K_j: u first, then fma in j order (pn_lincomb_kernel's order with c_0 = 1)
template <typename T, int NK, int VW, int ST>
__global__ __launch_bounds__(kBlock) void pn_rk_dense_eval_kernel(DenseEvalArgs<T> a, int64_t nvec, int64_t n) {
  using V = Vec<T, VW>;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += stride) {
    const V u = reinterpret_cast<const V *>(a.u)[i];
    V k[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) k[j] = reinterpret_cast<const V *>(a.k[j])[i];
    for (int o = 0; o < a.m; ++o) {
      V r;
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        T acc = u[e];
#pragma unroll
        for (int j = 0; j < NK; ++j) acc = fma(a.c[o][j], k[j][e], acc);
        r[e] = acc;
      }
      pn_store<ST>(reinterpret_cast<V *>(a.out + (int64_t)o * a.ld) + i, r);
    }
  }
  if (VW > 1 && blockIdx.x == 0) {
    const int64_t i = nvec * VW + threadIdx.x;
    if (i < n) {
      const T u = a.u[i];
      T k[NK];
#pragma unroll
      for (int j = 0; j < NK; ++j) k[j] = a.k[j][i];
      for (int o = 0; o < a.m; ++o) {
        T acc = u;
#pragma unroll
        for (int j = 0; j < NK; ++j) acc = fma(a.c[o][j], k[j], acc);
        a.out[(int64_t)o * a.ld + i] = acc;
      }
    }
  }
}

// D_j = sum_o c[o][j] g_o (fma, o ascending), G = sum_o g_o; accumulate: from the values already in D / G
template <typename T, int ND, int VW, bool WITH_G>
__global__ __launch_bounds__(kBlock) void pn_rk_dense_adjoint_kernel(DenseAdjArgs<T> a, int64_t nvec, int64_t n) {
  using V = Vec<T, VW>;
  constexpr int kRows = 4;                  // rows loaded before the first of them is used
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += stride) {
    V d[ND > 0 ? ND : 1], G;
    int o0 = 0;
    if (a.accumulate) {
#pragma unroll
      for (int j = 0; j < ND; ++j) d[j] = reinterpret_cast<const V *>(a.d[j])[i];
      if (WITH_G) G = reinterpret_cast<const V *>(a.G)[i];
    } else {
      const V g0 = reinterpret_cast<const V *>(a.g)[i];
#pragma unroll
      for (int j = 0; j < ND; ++j) d[j] = a.c[0][j] * g0;
      if (WITH_G) G = g0;
      o0 = 1;
    }
    for (int o = o0; o < a.m; o += kRows) {
      V g[kRows];
#pragma unroll
      for (int r = 0; r < kRows; ++r)
        if (o + r < a.m) g[r] = reinterpret_cast<const V *>(a.g + (int64_t)(o + r) * a.ld)[i];
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        if (o + r < a.m) {
#pragma unroll
          for (int j = 0; j < ND; ++j)
#pragma unroll
            for (int e = 0; e < VW; ++e) d[j][e] = fma(a.c[o + r][j], g[r][e], d[j][e]);
          if (WITH_G) G += g[r];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) reinterpret_cast<V *>(a.d[j])[i] = d[j];
    if (WITH_G) reinterpret_cast<V *>(a.G)[i] = G;
  }
  if (VW > 1 && blockIdx.x == 0) {
    const int64_t i = nvec * VW + threadIdx.x;
    if (i < n) {
      T d[ND > 0 ? ND : 1], G = 0;
      int o0 = 0;
      if (a.accumulate) {
#pragma unroll
        for (int j = 0; j < ND; ++j) d[j] = a.d[j][i];
        if (WITH_G) G = a.G[i];
      } else {
        const T g0 = a.g[i];
#pragma unroll
        for (int j = 0; j < ND; ++j) d[j] = a.c[0][j] * g0;
        G = g0;
        o0 = 1;
      }
      for (int o = o0; o < a.m; ++o) {
        const T g = a.g[(int64_t)o * a.ld + i];
#pragma unroll
        for (int j = 0; j < ND; ++j) d[j] = fma(a.c[o][j], g, d[j]);
        G += g;
      }
#pragma unroll
      for (int j = 0; j < ND; ++j) a.d[j][i] = d[j];
      if (WITH_G) a.G[i] = G;
    }
  }
}

template <typename T>
int dense_eval(hipStream_t st, int64_t n, const void *u, int nk, const void *const *K, int m, const double *coef, void *out,
               int64_t ld, int flags) {
  constexpr int VW = 16 / sizeof(T);
  const bool vec = pn::aligned16(u, out) && (ld % VW) == 0 && pn::aligned16(K, nk), nt = (flags & PN_DENSE_NONTEMPORAL) != 0;
  for (int o0 = 0; o0 < m; o0 += PN_DENSE_CHUNK) {
    DenseEvalArgs<T> a = {};
    a.u = (const T *)u;
    for (int j = 0; j < nk; ++j) a.k[j] = (const T *)K[j];
    a.out = (T *)out + (int64_t)o0 * ld;
    a.ld = ld;
    a.m = m - o0 < PN_DENSE_CHUNK ? m - o0 : PN_DENSE_CHUNK;
    for (int o = 0; o < a.m; ++o)
      for (int j = 0; j < nk; ++j) a.c[o][j] = (T)coef[(int64_t)(o0 + o) * nk + j];
    const int rc = pn::with_count<1, PN_MAX_STAGES>(nk, [&](auto N) {
      return pn::with_width<T>(vec, [&](auto W) {
        constexpr int NK = decltype(N)::value, VW = decltype(W)::value;
        const int64_t nvec = n / VW;
        const dim3 grid((unsigned)pn::blocks_for(nvec, kBlock, kDenseMaxBlocks));
        return nt ? pn::launch("pn_rk_dense_eval", pn_rk_dense_eval_kernel<T, NK, VW, 1>, grid, dim3(kBlock), st, a, nvec, n)
                  : pn::launch("pn_rk_dense_eval", pn_rk_dense_eval_kernel<T, NK, VW, 0>, grid, dim3(kBlock), st, a, nvec, n);
      });
    });
    if (rc) return pn::or_fail(rc, "pn_rk_dense_eval: nk out of range");
  }
  return 0;
}

template <typename T>
int dense_adjoint(hipStream_t st, int64_t n, int m, const void *g, int64_t ld, int nd, const double *coef, void *const *D,
                  void *G, int accumulate) {
  constexpr int VW = 16 / sizeof(T);
  const bool vec = pn::aligned16(g, G) && (ld % VW) == 0 && pn::aligned16(D, nd);
  for (int o0 = 0; o0 < m; o0 += PN_DENSE_CHUNK) {
    DenseAdjArgs<T> a = {};
    a.g = (const T *)g + (int64_t)o0 * ld;
    a.ld = ld;
    a.m = m - o0 < PN_DENSE_CHUNK ? m - o0 : PN_DENSE_CHUNK;
    a.accumulate = (accumulate || o0 > 0) ? 1 : 0;      // later chunks continue the sums of the first
    for (int j = 0; j < nd; ++j) a.d[j] = (T *)D[j];
    a.G = (T *)G;
    for (int o = 0; o < a.m; ++o)
      for (int j = 0; j < nd; ++j) a.c[o][j] = (T)coef[(int64_t)(o0 + o) * nd + j];
    const int rc = pn::with_count<0, PN_MAX_STAGES>(nd, [&](auto N) {
      return pn::with_width<T>(vec, [&](auto W) {
        constexpr int ND = decltype(N)::value, VW = decltype(W)::value;
        const int64_t nvec = n / VW;
        const dim3 grid((unsigned)pn::blocks_for(nvec, kBlock, kDenseMaxBlocks));
        if (G) return pn::launch("pn_rk_dense_adjoint", pn_rk_dense_adjoint_kernel<T, ND, VW, true>, grid, dim3(kBlock), st, a, nvec, n);
        // (no stage cotangent and no G: there is no such kernel)
        if constexpr (ND == 0) return pn::fail("pn_rk_dense_adjoint: nothing to compute");
        else return pn::launch("pn_rk_dense_adjoint", pn_rk_dense_adjoint_kernel<T, ND, VW, false>, grid, dim3(kBlock), st, a, nvec, n);
      });
    });
    if (rc) return pn::or_fail(rc, "pn_rk_dense_adjoint: nd out of range");
  }
  return 0;
}

}  // namespace

extern "C" {

int pn_rk_dense_eval(void *stream, int dtype, int64_t n, const void *u, int nk, const void *const *K, int m,
                     const double *coef, void *out, int64_t ld, int flags) {
  if (m <= 0 || n <= 0) return 0;
  if (!u || !out || !coef || (nk > 0 && !K)) return pn::fail("pn_rk_dense_eval: null argument");
  if (nk < 1 || nk > PN_MAX_STAGES) return pn::fail("pn_rk_dense_eval: nk must be 1..7");
  if (ld < n) return pn::fail("pn_rk_dense_eval: row stride shorter than a row");
  for (int j = 0; j < nk; ++j)
    if (!K[j]) return pn::fail("pn_rk_dense_eval: null stage derivative");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return dense_eval<decltype(t)>(st, n, u, nk, K, m, coef, out, ld, flags); });
  return pn::or_fail(rc, "pn_rk_dense_eval: unknown dtype");
}

int pn_rk_dense_adjoint(void *stream, int dtype, int64_t n, int m, const void *g, int64_t ld, int nd, const double *coef,
                        void *const *D, void *G, int accumulate) {
  if (m <= 0 || n <= 0) return 0;
  if (!g || (nd > 0 && (!coef || !D))) return pn::fail("pn_rk_dense_adjoint: null argument");
  if (nd < 0 || nd > PN_MAX_STAGES) return pn::fail("pn_rk_dense_adjoint: nd must be 0..7");
  if (nd == 0 && !G) return pn::fail("pn_rk_dense_adjoint: nothing to compute");
  if (ld < n) return pn::fail("pn_rk_dense_adjoint: row stride shorter than a row");
  for (int j = 0; j < nd; ++j)
    if (!D[j]) return pn::fail("pn_rk_dense_adjoint: null output vector");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return dense_adjoint<decltype(t)>(st, n, m, g, ld, nd, coef, D, G, accumulate); });
  return pn::or_fail(rc, "pn_rk_dense_adjoint: unknown dtype");
}

}  // extern "C"
