// pnode_amd -- per-sample adaptive step control (-pn_adapt_scope sample): the state is B rows of d entries and every row
// carries its own time, step size and accept / reject decision.  The kernels here are the row-scaled forms of
// pn_lincomb_kernel / pn_combine_wrms_kernel (pn_kernels.hip) plus the per-row controller.  See include/pnode_amd.h,
// section 3a'''.
//
// Geometry.  A row is cut into chunks of 16 bytes (VW = 16 / sizeof(T) elements); a GROUP of G threads, G the smallest
// power of two >= the number of chunks (at most the 256 threads of a workgroup), owns a row: thread g of the group takes
// chunks g, g + G, ...  A workgroup holds 256 / G rows; the grid is capped and block-strides over the rows.  G depends on
// d alone -- never on B or on where a row sits in its workgroup -- and so does every summation order: a row's result is
// the same bits whatever batch it is part of.  Vector path (all bases 16-byte aligned and d % VW == 0): one
// global_load_dwordx4 / global_store_dwordx4 per chunk, lane-contiguous.  Otherwise the scalar form of the same kernel
// walks the same chunks element by element (the ragged last chunk is bounds-checked), so both give the same bits.
// Coefficients h_r * a_ij are formed in double and rounded once to the storage type, then used in pn_lincomb_kernel's
// order (first term, then fused multiply-adds in j order).  Per-row step sizes, masks and hit indices are read from
// device vectors (double / int32); tableau coefficients are kernel arguments.  No float atomics.
//
// With -pn_output_times interpolate the rows also serve the output times themselves (pn_rows_dense_eval and its transpose
// pn_rows_dense_adjoint, the per-row forms of pn_dense.hip's two kernels): a row's range of outputs and the coefficients
// h_r beta_j(theta) come from the shared text of pn_adapt.h, formed in double from the polynomial table (a kernel argument)
// and rounded once; the output times and the row's "next output" counter live on the device.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "pnode_amd.h"
#include "pn_launch.h"
#include "pn_device.h"
#include "pn_adapt.h"

static_assert(PN_ROWS_DENSE_POW == PN_DENSE_MAX_POW, "pn_adapt.h and pnode_amd.h disagree on the width of a continuous extension's table");

namespace {

constexpr int kRowsMaxBlocks = 4096;

template <typename T>
struct RowsLinArgs {
  T *out;
  const T *base;                 // u (stage), or null (cotangent: the first term is a product)
  const T *x[PN_MAX_TERMS];
  double c[PN_MAX_TERMS];        // tableau coefficients, multiplied by h[r] in double
  const double *h;               // null: every row uses 1
  const T *tail;                 // added last, unscaled (the D_i of a row's interpolated outputs); HAS_TAIL kernels only
};

template <typename T>
struct RowsErrArgs {
  T *unew;                       // null: `u` already is the new state (first same as last)
  const T *u;
  const T *k[PN_MAX_STAGES];
  double cb[PN_MAX_STAGES], ce[PN_MAX_STAGES];
  const double *h;
  double *enorm;
  double atol, rtol;
};

template <typename T>
struct RowsCommitArgs {
  T *unext;                      // may be `u` itself: then only accepted rows are written
  const T *u, *unew;
  T *sol;                        // [T][B*d] with row stride ld; may be null
  const int32_t *accept, *hit;
  int64_t ld;
  int nout;
};

template <typename T>
struct RowsAccumArgs {
  T *out;
  const T *lam;
  const T *x[PN_MAX_TERMS];
  const T *g;                    // [T][.] with row stride ld; may be null
  const int32_t *hit;
  int64_t ld;
  int nout;
};

template <typename T>
struct RowsDenseEvalArgs {
  const T *u, *unew;
  const T *k[PN_MAX_STAGES];
  T *sol;                        // [nout][B*d] with row stride ld
  int64_t ld;
  int nout;
  const double *times;           // [nout]
  const double *heff, *trow;     // the round's log: h_eff and the time at the round's start
  const double *tnew;            // the time the controller wrote
  int32_t *hit;                  // in: the controller's hit (>= 0: the final time); out: the output copied, or -1
  int32_t *next;                 // the row's first output not yet served
  int32_t *range;                // out: [2][B] = lo, hi
  double P[PN_MAX_STAGES][PN_DENSE_MAX_POW];
};

template <typename T>
struct RowsDenseAdjArgs {
  const T *g;                    // [nout][B*d] with row stride ld
  int64_t ld;
  int nout;
  const double *times, *heff, *trow;
  const int32_t *range;
  T *d[PN_MAX_STAGES];
  T *G;
  double P[PN_MAX_STAGES][PN_DENSE_MAX_POW];
};

struct RowsGeom {
  int64_t B, d, nch;
  int lgG;
};

template <typename T, bool VEC>
__device__ __forceinline__ void load_chunk(const T *row, int64_t c, int64_t d, T (&v)[16 / sizeof(T)]) {
  constexpr int VW = 16 / sizeof(T);
  if (VEC) {
    const Vec<T, VW> x = reinterpret_cast<const Vec<T, VW> *>(row)[c];
#pragma unroll
    for (int e = 0; e < VW; ++e) v[e] = x[e];
  } else {
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      const int64_t i = c * VW + e;
      v[e] = i < d ? row[i] : (T)0;
    }
  }
}
// (vector path: stored non-temporally, the policy pn_lincomb_kernel / pn_combine_wrms_kernel run with by default -- the
// outputs are not read again before func has run)
// (ST = 0, plain stores: the row copies around func below, whose outputs func or autograd reads next)
template <typename T, bool VEC, int ST = 1>
__device__ __forceinline__ void store_chunk(T *row, int64_t c, int64_t d, const T (&v)[16 / sizeof(T)]) {
  constexpr int VW = 16 / sizeof(T);
  if (VEC) {
    Vec<T, VW> x;
#pragma unroll
    for (int e = 0; e < VW; ++e) x[e] = v[e];
    pn_store<ST>(reinterpret_cast<Vec<T, VW> *>(row) + c, x);
  } else {
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      const int64_t i = c * VW + e;
      if (i < d) row[i] = v[e];
    }
  }
}

// out[r] = base[r] + sum_j (h_r c_j) x_j[r]   (HAS_BASE: pn_rk_stage's order -- u, then fma in j)
// out[r] = (h_r c_0) x_0[r] + sum_{j>0} ...   (!HAS_BASE: pn_adj_theta's order -- the first product, then fma)
// HAS_TAIL: ... + tail[r], added last with coefficient one (pn_rk_adjoint_step_dense's last term)
template <typename T, int NK, bool VEC, bool HAS_BASE, bool HAS_TAIL = false>
__global__ __launch_bounds__(kBlock) void pn_rows_lin_kernel(RowsLinArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t r = (int64_t)blockIdx.x * rpb + sub; r < q.B; r += (int64_t)gridDim.x * rpb) {
    const double h = a.h ? a.h[r] : 1.0;
    T c[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) c[j] = (T)(h * a.c[j]);
    const int64_t off = r * q.d;
    for (int64_t ch = g; ch < q.nch; ch += G) {
      T b[VW], x[NK][VW], o[VW], t[VW];
      if (HAS_BASE) load_chunk<T, VEC>(a.base + off, ch, q.d, b);
#pragma unroll
      for (int j = 0; j < NK; ++j) load_chunk<T, VEC>(a.x[j] + off, ch, q.d, x[j]);
      if (HAS_TAIL) load_chunk<T, VEC>(a.tail + off, ch, q.d, t);
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        T acc = HAS_BASE ? b[e] : c[0] * x[0][e];
#pragma unroll
        for (int j = HAS_BASE ? 0 : 1; j < NK; ++j) acc = fma(c[j], x[j][e], acc);
        if (HAS_TAIL) {
          // one addition of its own: with a single scaled term the product before it must not be fused into it
#pragma clang fp contract(off)
          acc = acc + t[e];
        }
        o[e] = acc;
      }
      store_chunk<T, VEC>(a.out + off, ch, q.d, o);
    }
  }
}

// unew[r] = u[r] + sum_j (h_r cb_j) K_j[r], err = sum_j (h_r ce_j) K_j[r], enorm[r] = sqrt(sum_e term^2 / d): one pass.
// Per-thread sums in double over the thread's chunks in ascending order, then the group's tree: shuffles inside a wave
// (width G), and for G > 64 the waves of the group through LDS in wave order.
template <typename T, int NK, bool VEC, bool WRITE>
__global__ __launch_bounds__(kBlock) void pn_rows_combine_wrms_kernel(RowsErrArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ double lds[kBlock / kWave];
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < q.B; r0 += (int64_t)gridDim.x * rpb) {
    const int64_t r = r0 + sub;
    const bool live = r < q.B;
    double sum = 0;
    if (live) {
      const double h = a.h[r];
      T cb[NK], ce[NK];
#pragma unroll
      for (int j = 0; j < NK; ++j) {
        cb[j] = (T)(h * a.cb[j]);
        ce[j] = (T)(h * a.ce[j]);
      }
      const int64_t off = r * q.d;
      for (int64_t ch = g; ch < q.nch; ch += G) {
        T u[VW], k[NK][VW], o[VW];
        load_chunk<T, VEC>(a.u + off, ch, q.d, u);
#pragma unroll
        for (int j = 0; j < NK; ++j) load_chunk<T, VEC>(a.k[j] + off, ch, q.d, k[j]);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          T un = u[e], er = (T)0;
#pragma unroll
          for (int j = 0; j < NK; ++j) {
            if (WRITE) un = fma(cb[j], k[j][e], un);
            er = fma(ce[j], k[j][e], er);
          }
          o[e] = un;
          if (VEC || ch * VW + e < q.d) sum += wrms_term<T>(un, er, a.atol, a.rtol);
        }
        if (WRITE) store_chunk<T, VEC>(a.unew + off, ch, q.d, o);
      }
    }
    if (G <= kWave) {
      for (int o = G >> 1; o > 0; o >>= 1) sum += __shfl_down(sum, o, G);
    } else {
      sum = wave_sum(sum);
      const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
      if (lane == 0) lds[wid] = sum;
      __syncthreads();
      if (g == 0) {
        const int w0 = sub * (G / kWave);
        sum = 0;
        for (int w = 0; w < G / kWave; ++w) sum += lds[w0 + w];
      }
      __syncthreads();
    }
    if (live && g == 0) a.enorm[r] = sqrt(sum / (double)q.d);
  }
}

// pn_rows_combine_wrms_kernel under -ts_adapt_wnormtype infinity: enorm[r] = the largest term of the row, NaN if any is.  That
// kernel statement for statement -- the same rows per workgroup, chunks, update and err chains, stores and dead rows -- with
// nan_max (pn_device.h) where it adds, at every level of the same tree (thread, shuffles of width G, the group's waves through LDS),
// and no sqrt(. / d).  (A text of its own, so that the default kernel's code stays what it was.)
template <typename T, int NK, bool VEC, bool WRITE>
__global__ __launch_bounds__(kBlock) void pn_rows_combine_winf_kernel(RowsErrArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ double lds[kBlock / kWave];
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < q.B; r0 += (int64_t)gridDim.x * rpb) {
    const int64_t r = r0 + sub;
    const bool live = r < q.B;
    double sum = 0;
    if (live) {
      const double h = a.h[r];
      T cb[NK], ce[NK];
#pragma unroll
      for (int j = 0; j < NK; ++j) {
        cb[j] = (T)(h * a.cb[j]);
        ce[j] = (T)(h * a.ce[j]);
      }
      const int64_t off = r * q.d;
      for (int64_t ch = g; ch < q.nch; ch += G) {
        T u[VW], k[NK][VW], o[VW];
        load_chunk<T, VEC>(a.u + off, ch, q.d, u);
#pragma unroll
        for (int j = 0; j < NK; ++j) load_chunk<T, VEC>(a.k[j] + off, ch, q.d, k[j]);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          T un = u[e], er = (T)0;
#pragma unroll
          for (int j = 0; j < NK; ++j) {
            if (WRITE) un = fma(cb[j], k[j][e], un);
            er = fma(ce[j], k[j][e], er);
          }
          o[e] = un;
          if (VEC || ch * VW + e < q.d) sum = nan_max(sum, winf_term<T>(un, er, a.atol, a.rtol));
        }
        if (WRITE) store_chunk<T, VEC>(a.unew + off, ch, q.d, o);
      }
    }
    if (G <= kWave) {
      for (int o = G >> 1; o > 0; o >>= 1) sum = nan_max(sum, __shfl_down(sum, o, G));
    } else {
      sum = wave_max(sum);
      const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
      if (lane == 0) lds[wid] = sum;
      __syncthreads();
      if (g == 0) {
        const int w0 = sub * (G / kWave);
        sum = 0;
        for (int w = 0; w < G / kWave; ++w) sum = nan_max(sum, lds[w0 + w]);
      }
      __syncthreads();
    }
    if (live && g == 0) a.enorm[r] = sum;
  }
}

// Per-component tolerances (pn_rows_combine_wrms_v / pn_rows_combine_winf_v): the two kernels above with column c's term formed
// from vatol[c], vrtol[c] -- the period is the row, so the entry is the element's column and no remainder is taken.  The same
// rows per workgroup, chunks, update and err chains, stores, dead rows, trees and finishes, and the same wrms_term / winf_term:
// vectors filled with one value give those kernels' bits.  The 2 d doubles are re-read by every row from L1 / L2.  (A text of
// its own, so that the scalar kernels' code stays what it was; INF picks the norm.)
template <typename T>
struct RowsErrVArgs {
  T *unew;
  const T *u;
  const T *k[PN_MAX_STAGES];
  double cb[PN_MAX_STAGES], ce[PN_MAX_STAGES];
  const double *h;
  double *enorm;
  const double *vatol, *vrtol;   // d entries each
};

template <typename T, int NK, bool VEC, bool WRITE, bool INF>
__global__ __launch_bounds__(kBlock) void pn_rows_combine_v_kernel(RowsErrVArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ double lds[kBlock / kWave];
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < q.B; r0 += (int64_t)gridDim.x * rpb) {
    const int64_t r = r0 + sub;
    const bool live = r < q.B;
    double sum = 0;
    if (live) {
      const double h = a.h[r];
      T cb[NK], ce[NK];
#pragma unroll
      for (int j = 0; j < NK; ++j) {
        cb[j] = (T)(h * a.cb[j]);
        ce[j] = (T)(h * a.ce[j]);
      }
      const int64_t off = r * q.d;
      for (int64_t ch = g; ch < q.nch; ch += G) {
        T u[VW], k[NK][VW], o[VW];
        double ta[VW], tr[VW];
        load_chunk<T, VEC>(a.u + off, ch, q.d, u);
#pragma unroll
        for (int j = 0; j < NK; ++j) load_chunk<T, VEC>(a.k[j] + off, ch, q.d, k[j]);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          const int64_t c = ch * VW + e;
          const bool in = VEC || c < q.d;
          ta[e] = in ? a.vatol[c] : 1.0;
          tr[e] = in ? a.vrtol[c] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          T un = u[e], er = (T)0;
#pragma unroll
          for (int j = 0; j < NK; ++j) {
            if (WRITE) un = fma(cb[j], k[j][e], un);
            er = fma(ce[j], k[j][e], er);
          }
          o[e] = un;
          if (VEC || ch * VW + e < q.d) {
            if (INF) sum = nan_max(sum, winf_term<T>(un, er, ta[e], tr[e]));
            else sum += wrms_term<T>(un, er, ta[e], tr[e]);
          }
        }
        if (WRITE) store_chunk<T, VEC>(a.unew + off, ch, q.d, o);
      }
    }
    if (G <= kWave) {
      for (int o = G >> 1; o > 0; o >>= 1) {
        const double other = __shfl_down(sum, o, G);
        sum = INF ? nan_max(sum, other) : sum + other;
      }
    } else {
      sum = INF ? wave_max(sum) : wave_sum(sum);
      const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
      if (lane == 0) lds[wid] = sum;
      __syncthreads();
      if (g == 0) {
        const int w0 = sub * (G / kWave);
        sum = 0;
        for (int w = 0; w < G / kWave; ++w) sum = INF ? nan_max(sum, lds[w0 + w]) : sum + lds[w0 + w];
      }
      __syncthreads();
    }
    if (live && g == 0) a.enorm[r] = INF ? sum : sqrt(sum / (double)q.d);
  }
}

// unext[r] = accept[r] ? unew[r] : u[r];  sol[hit[r]][r] = unew[r] where hit[r] >= 0
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void pn_rows_commit_kernel(RowsCommitArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  const bool inplace = a.unext == a.u;
  for (int64_t r = (int64_t)blockIdx.x * rpb + sub; r < q.B; r += (int64_t)gridDim.x * rpb) {
    const int acc = a.accept[r];
    int hit = (acc && a.sol && a.hit) ? a.hit[r] : -1;
    if (hit >= a.nout) hit = -1;
    if (!acc && inplace) continue;
    const int64_t off = r * q.d;
    const T *src = acc ? a.unew : a.u;
    for (int64_t ch = g; ch < q.nch; ch += G) {
      T v[VW];
      load_chunk<T, VEC>(src + off, ch, q.d, v);
      store_chunk<T, VEC>(a.unext + off, ch, q.d, v);
      if (hit >= 0) store_chunk<T, VEC>(a.sol + (int64_t)hit * a.ld + off, ch, q.d, v);
    }
  }
}

// out[r] = lam[r] + sum_j x_j[r] (+ g[hit[r]][r] where hit[r] >= 0): pn_adj_accum's order (every coefficient is one)
template <typename T, int NK, bool VEC>
__global__ __launch_bounds__(kBlock) void pn_rows_adj_accum_kernel(RowsAccumArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t r = (int64_t)blockIdx.x * rpb + sub; r < q.B; r += (int64_t)gridDim.x * rpb) {
    int hit = (a.g && a.hit) ? a.hit[r] : -1;
    if (hit >= a.nout) hit = -1;
    const int64_t off = r * q.d;
    for (int64_t ch = g; ch < q.nch; ch += G) {
      T l[VW], x[NK > 0 ? NK : 1][VW], f[VW];
      load_chunk<T, VEC>(a.lam + off, ch, q.d, l);
#pragma unroll
      for (int j = 0; j < NK; ++j) load_chunk<T, VEC>(a.x[j] + off, ch, q.d, x[j]);
      if (hit >= 0) load_chunk<T, VEC>(a.g + (int64_t)hit * a.ld + off, ch, q.d, f);
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        T acc = l[e];
#pragma unroll
        for (int j = 0; j < NK; ++j) acc += x[j][e];
        if (hit >= 0) acc += f[e];
        l[e] = acc;
      }
      store_chunk<T, VEC>(a.out + off, ch, q.d, l);
    }
  }
}

// The outputs of a round (-pn_output_times interpolate).  Per row: the shared classification (pn_adapt.h) from the round's
// log, the time the controller wrote, the row's counter and the output times; then, chunk by chunk, u and the used K_j are
// loaded once and every output o in [lo, hi) is written as u + sum_j c_j K_j (u first, then fma in j order) with
// c_j = (T)(h_r beta_j(theta_o)) formed in double; an exact landing or the final time copies unew[r].  Every thread of a
// row's group classifies for itself; thread 0 of the group writes the counter, [lo, hi) and the hit after a barrier (the
// other waves of the group have read them by then).  Rows outside every range are not touched.
template <typename T, int NK, bool VEC>
__global__ __launch_bounds__(kBlock) void pn_rows_dense_eval_kernel(RowsDenseEvalArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < q.B; r0 += (int64_t)gridDim.x * rpb) {
    const int64_t r = r0 + sub;
    const bool live = r < q.B;
    PnDensePlan p = {0, 0, -1, 0};
    double h = 0, tr = 0;
    if (live) {
      h = a.heff[r];
      tr = a.trow[r];
      p = pn_rows_dense_plan_row(a.times, a.nout, h, a.tnew[r], a.hit[r], a.next[r]);
    }
    __syncthreads();
    if (live && g == 0) {
      a.next[r] = p.next;
      a.range[r] = p.lo;
      a.range[q.B + r] = p.hi;
      a.hit[r] = p.hit;
    }
    if (!live || (p.hi == p.lo && p.hit < 0)) continue;
    const int64_t off = r * q.d;
    for (int64_t ch = g; ch < q.nch; ch += G) {
      if (p.hi > p.lo) {
        T u[VW], k[NK][VW];
        load_chunk<T, VEC>(a.u + off, ch, q.d, u);
#pragma unroll
        for (int j = 0; j < NK; ++j) load_chunk<T, VEC>(a.k[j] + off, ch, q.d, k[j]);
        for (int o = p.lo; o < p.hi; ++o) {
          const double to = a.times[o];
          T c[NK], v[VW];
#pragma unroll
          for (int j = 0; j < NK; ++j) c[j] = (T)pn_rows_dense_coef(a.P[j], to, tr, h);
#pragma unroll
          for (int e = 0; e < VW; ++e) {
            T acc = u[e];
#pragma unroll
            for (int j = 0; j < NK; ++j) acc = fma(c[j], k[j][e], acc);
            v[e] = acc;
          }
          store_chunk<T, VEC>(a.sol + (int64_t)o * a.ld + off, ch, q.d, v);
        }
      }
      if (p.hit >= 0) {
        T v[VW];
        load_chunk<T, VEC>(a.unew + off, ch, q.d, v);
        store_chunk<T, VEC>(a.sol + (int64_t)p.hit * a.ld + off, ch, q.d, v);
      }
    }
  }
}

// The transpose, for a reversed round: D_j[r] = sum_{o in [lo_r, hi_r)} c_{o,j,r} g[o][r] (from zero, fma, o ascending) and
// G[r] = sum_o g[o][r]; a row with an empty range gets zeros.  kAhead rows of g are loaded before the first is used.
template <typename T, int ND, bool VEC>
__global__ __launch_bounds__(kBlock) void pn_rows_dense_adjoint_kernel(RowsDenseAdjArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  constexpr int kAhead = 4;
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t r = (int64_t)blockIdx.x * rpb + sub; r < q.B; r += (int64_t)gridDim.x * rpb) {
    int lo = a.range[r], hi = a.range[q.B + r];
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.nout ? a.nout : hi;
    const double h = a.heff[r], tr = a.trow[r];
    const int64_t off = r * q.d;
    for (int64_t ch = g; ch < q.nch; ch += G) {
      T D[ND][VW], S[VW];
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        S[e] = (T)0;
#pragma unroll
        for (int j = 0; j < ND; ++j) D[j][e] = (T)0;
      }
      for (int o = lo; o < hi; o += kAhead) {
        T f[kAhead][VW];
#pragma unroll
        for (int w = 0; w < kAhead; ++w)
          if (o + w < hi) load_chunk<T, VEC>(a.g + (int64_t)(o + w) * a.ld + off, ch, q.d, f[w]);
#pragma unroll
        for (int w = 0; w < kAhead; ++w) {
          if (o + w < hi) {
            const double to = a.times[o + w];
#pragma unroll
            for (int j = 0; j < ND; ++j) {
              const T c = (T)pn_rows_dense_coef(a.P[j], to, tr, h);
#pragma unroll
              for (int e = 0; e < VW; ++e) D[j][e] = fma(c, f[w][e], D[j][e]);
            }
#pragma unroll
            for (int e = 0; e < VW; ++e) S[e] += f[w][e];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < ND; ++j) store_chunk<T, VEC>(a.d[j] + off, ch, q.d, D[j]);
      store_chunk<T, VEC>(a.G + off, ch, q.d, S);
    }
  }
}

// One thread per row runs the shared controller (pn_adapt.h).  Every workgroup publishes (unfinished rows, first failing
// row) and draws a ticket; the last to arrive adds / compares them in index order and writes the summary.
__global__ __launch_bounds__(kBlock) void pn_rows_control_kernel(PnRowsCtl rc, const double *span, int64_t B, const double *enorm,
                                                                 double *sd, int32_t *si, double *log_d, int32_t *log_hit,
                                                                 int32_t *accept, int32_t *summary, double *work) {
  __shared__ int s_open[kBlock / kWave];
  __shared__ long long s_fail[kBlock / kWave];
  constexpr long long kNone = 1ll << 62;
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int open = 0;
  long long key = kNone;                       // 4 * row + failure code of the first failing row
  if (r < B) {
    open = pn_rows_judge_row(rc, span, B, r, enorm, sd, si, log_d, log_hit, accept);
    const int f = si[PN_ROWS_FAIL * B + r];
    if (f) key = 4 * (long long)r + f;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    open += __shfl_down(open, o, kWave);
    const long long other = __shfl_down(key, o, kWave);
    key = other < key ? other : key;
  }
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) {
    s_open[wid] = open;
    s_fail[wid] = key;
  }
  __syncthreads();
  double *partial = work + kTicketDoubles;
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / kWave; ++w) {
      open += s_open[w];
      key = s_fail[w] < key ? s_fail[w] : key;
    }
    publish_partial(partial + 2 * blockIdx.x, (double)open);
    publish_partial(partial + 2 * blockIdx.x + 1, (double)key);
  }
  if (draw_ticket(work, gridDim.x, blockIdx.x)) {
    // the last workgroup: every thread takes the partials b = tid, tid + 256, ... (loads issued side by side), then the
    // block's tree; an integer sum and a minimum do not depend on the order
    double tot = 0, first = (double)kNone;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += kBlock) {
      const double c = read_partial(partial + 2 * b), f = read_partial(partial + 2 * b + 1);
      tot += c;
      first = f < first ? f : first;
    }
    int cnt = (int)tot;
    long long k = (long long)first;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      cnt += __shfl_down(cnt, o, kWave);
      const long long other = __shfl_down(k, o, kWave);
      k = other < k ? other : k;
    }
    __syncthreads();                      // s_open / s_fail were read by thread 0 above
    if (lane == 0) {
      s_open[wid] = cnt;
      s_fail[wid] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < kBlock / kWave; ++w) {
        cnt += s_open[w];
        k = s_fail[w] < k ? s_fail[w] : k;
      }
      summary[0] = cnt;
      summary[1] = k < kNone ? (int32_t)(k >> 2) : -1;
      summary[2] = k < kNone ? (int32_t)(k & 3) : 0;
      summary[3] = 0;
    }
  }
}

// ------------------------------------------------------------------------------------------
// dL/dt of a per-sample solve: two row-wise reductions in the geometry above, the per-row scatter
// of a reversed round into the row's column of dtrow (the shared text of pn_adapt.h) and the ordered sum over the rows.
// ------------------------------------------------------------------------------------------
template <typename T>
struct RowsTgDotArgs {
  const T *x[PN_MAX_STAGES];
  const T *y[PN_MAX_STAGES];
  double c[PN_MAX_STAGES];
  double *rowacc;
  int accumulate;
};

template <typename T>
struct RowsTgDenseArgs {
  const T *g;                    // [nout][B*d] with row stride ld
  int64_t ld;
  int nout;
  const T *k[PN_MAX_STAGES];
  const double *times, *heff, *trow;
  const int32_t *range;
  double *erow;                  // [nout][B]
  double P[PN_MAX_STAGES][PN_DENSE_MAX_POW];
};

// the sum of a row's group, valid in thread 0 of the group: shuffles inside a wave (width G), and for G > 64 the waves of
// the group through LDS in wave order (pn_rows_combine_wrms_kernel's tree).  Every thread of the workgroup calls it.
__device__ __forceinline__ double rows_group_sum(double sum, int lgG, double *lds) {
  const int G = 1 << lgG;
  if (G <= kWave) {
    for (int o = G >> 1; o > 0; o >>= 1) sum += __shfl_down(sum, o, G);
    return sum;
  }
  sum = wave_sum(sum);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) lds[wid] = sum;
  __syncthreads();
  if ((threadIdx.x & (G - 1)) == 0) {
    const int w0 = (threadIdx.x >> lgG) * (G / kWave);
    sum = 0;
    for (int w = 0; w < G / kWave; ++w) sum += lds[w0 + w];
  }
  __syncthreads();
  return sum;
}

// rowacc[r] (+)= sum_p c_p <x_p[r], y_p[r]>: products and sums in double; per thread the chunks in ascending order, per chunk
// the pairs in p order, per pair the elements in order; then the group's tree.
template <typename T, int NP, bool VEC>
__global__ __launch_bounds__(kBlock) void pn_rows_tgrad_dots_kernel(RowsTgDotArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ double lds[kBlock / kWave];
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < q.B; r0 += (int64_t)gridDim.x * rpb) {
    const int64_t r = r0 + sub;
    const bool live = r < q.B;
    double sum = 0;
    if (live) {
      const int64_t off = r * q.d;
      for (int64_t ch = g; ch < q.nch; ch += G) {
        T x[NP][VW], y[NP][VW];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          load_chunk<T, VEC>(a.x[p] + off, ch, q.d, x[p]);
          load_chunk<T, VEC>(a.y[p] + off, ch, q.d, y[p]);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          double dot = 0;
#pragma unroll
          for (int e = 0; e < VW; ++e) dot += (double)x[p][e] * (double)y[p][e];
          sum += a.c[p] * dot;
        }
      }
    }
    sum = rows_group_sum(sum, q.lgG, lds);
    if (live && g == 0) a.rowacc[r] = a.accumulate ? a.rowacc[r] + sum : sum;
  }
}

// erow[o][r] = sum_j beta'_j(theta_{o,r}) <g[o][r], K_j[r]> for the outputs o of the row's logged range, kTgTile outputs at a
// time: a thread that owns one chunk of the row loads its K_j once for all tiles; a thread that strides loads them once per
// tile.  The tile count is the workgroup's largest (the tree of a group wider than a wave meets at barriers): rows with
// fewer tiles ride along with nothing to add.  Entries outside a row's range are not written.
constexpr int kTgTile = 8;

template <typename T, int NK, bool VEC>
__global__ __launch_bounds__(kBlock) void pn_rows_dense_tgrad_kernel(RowsTgDenseArgs<T> a, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ double lds[kBlock / kWave];
  __shared__ int s_tiles;
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  const bool single = q.nch <= G;
  for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < q.B; r0 += (int64_t)gridDim.x * rpb) {
    const int64_t r = r0 + sub;
    const bool live = r < q.B;
    int lo = 0, hi = 0;
    double h = 1, tr = 0;
    if (live) {
      lo = a.range[r];
      hi = a.range[q.B + r];
      lo = lo < 0 ? 0 : lo;
      hi = hi > a.nout ? a.nout : hi;
      h = a.heff[r];
      tr = a.trow[r];
      if (!(h > 0.0)) hi = lo;
    }
    if (threadIdx.x == 0) s_tiles = 0;
    __syncthreads();
    if (live && g == 0 && hi > lo) atomicMax(&s_tiles, (hi - lo + kTgTile - 1) / kTgTile);
    __syncthreads();
    const int tiles = s_tiles;
    const int64_t off = r * q.d;
    T k[NK][VW];
    if (single && live && hi > lo && g < q.nch) {
#pragma unroll
      for (int j = 0; j < NK; ++j) load_chunk<T, VEC>(a.k[j] + off, g, q.d, k[j]);
    }
    for (int t = 0; t < tiles; ++t) {
      const int o0 = lo + t * kTgTile;
      double s[kTgTile];
#pragma unroll
      for (int w = 0; w < kTgTile; ++w) s[w] = 0;
      if (live && o0 < hi) {
        for (int64_t ch = g; ch < q.nch; ch += G) {
          if (!single) {
#pragma unroll
            for (int j = 0; j < NK; ++j) load_chunk<T, VEC>(a.k[j] + off, ch, q.d, k[j]);
          }
#pragma unroll
          for (int w = 0; w < kTgTile; ++w) {
            if (o0 + w < hi) {
              T f[VW];
              load_chunk<T, VEC>(a.g + (int64_t)(o0 + w) * a.ld + off, ch, q.d, f);
              const double th = pn_rows_dense_theta(a.times[o0 + w], tr, h);
#pragma unroll
              for (int j = 0; j < NK; ++j) {
                double dot = 0;
#pragma unroll
                for (int e = 0; e < VW; ++e) dot += (double)f[e] * (double)k[j][e];
                s[w] += pn_rows_dense_dcoef(a.P[j], th) * dot;
              }
            }
          }
        }
      }
#pragma unroll
      for (int w = 0; w < kTgTile; ++w) {
        const double v = rows_group_sum(s[w], q.lgG, lds);
        if (live && g == 0 && o0 + w < hi) a.erow[(int64_t)(o0 + w) * q.B + r] = v;
      }
    }
    __syncthreads();                      // s_tiles is rewritten by the next rows of this workgroup
  }
}

// One thread per row sends the round into the row's own column of dtrow (pn_adapt.h): no atomics.
__global__ __launch_bounds__(kBlock) void pn_rows_tgrad_scatter_kernel(PnRowsTgScatter a, int64_t B) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r < B) pn_rows_tgrad_scatter_row(a, B, r);
}

// dt[i] = sum_r dtrow[i][r]: workgroup (bx, i) adds the columns bx*256 + tid, + 256*gridDim.x, ... of row i (per thread in that
// order, then the block tree) and publishes one partial; the last workgroup of the grid adds every row's partials in index
// order (one wave per row, as pn_rk_dense_tgrad_kernel finishes).  gridDim.x depends on B alone: the same call, the same bits.
constexpr int kTgReduceBlocks = 64;

__global__ __launch_bounds__(kBlock) void pn_rows_tgrad_reduce_kernel(const double *dtrow, int64_t B, int nout, double *dt, double *work) {
  double *partial = work + kTicketDoubles;
  const int i = blockIdx.y;
  double s = 0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < B; r += (int64_t)gridDim.x * kBlock) s += dtrow[(int64_t)i * B + r];
  const double b = block_sum(s);
  if (threadIdx.x == 0) publish_partial(partial + (int64_t)i * gridDim.x + blockIdx.x, b);
  if (draw_ticket(work, gridDim.x * gridDim.y, blockIdx.y * gridDim.x + blockIdx.x)) {
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    for (int o = wid; o < nout; o += kBlock / kWave) {
      double t = 0;
      for (int bx = lane; bx < (int)gridDim.x; bx += kWave) t += read_partial(partial + (int64_t)o * gridDim.x + bx);
      t = wave_sum(t);
      if (lane == 0) dt[o] = t;
    }
  }
}

// ------------------------------------------------------------------------------------------
// -pn_rows_compact 1: the ordered list of the rows with work to do, and the two row copies that carry
// func's operands into a dense sub-batch and its results back.  Nothing here computes: values travel as bits.
// ------------------------------------------------------------------------------------------
// The list.  ONE workgroup of kListBlock threads; wave w owns the contiguous rows [w*seg, (w+1)*seg), seg a multiple of 64.
// Pass 1: every wave counts its listed rows, 64 rows a step (a ballot and a population count: no shuffles, no LDS).  One
// barrier; a wave's first place is the sum of the counts of the waves before it.  Pass 2: the wave walks its rows again;
// a listed row's place is the wave's running offset plus the listed lanes below it.  Places depend on the row numbers
// alone -- never on which wave ran first -- so idx is ascending and two launches write the same bytes; no atomics, no
// hand-off between workgroups, no work area.  Places written are < m, the -1 tail is >= m: the two never meet.
constexpr int kListBlock = 1024;

__global__ __launch_bounds__(kListBlock) void pn_rows_list_kernel(int kind, const void *src, int64_t B, int32_t *idx, int32_t *pos,
                                                                  int32_t *count) {
  constexpr int kWaves = kListBlock / kWave;
  __shared__ int s_cnt[kWaves];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int64_t seg = ((B + kWaves - 1) / kWaves + kWave - 1) / kWave * kWave;
  const int64_t lo = (int64_t)wid * seg;
  const int64_t hi = lo + seg < B ? lo + seg : B;
  int cnt = 0;
  for (int64_t r0 = lo; r0 < hi; r0 += kWave) {
    const int64_t r = r0 + lane;
    const bool on = r < hi && pn_rows_listed(kind, src, r);
    cnt += __popcll(__ballot(on));
  }
  if (lane == 0) s_cnt[wid] = cnt;
  __syncthreads();
  int off = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int c = s_cnt[w];
    off += w < wid ? c : 0;
    total += c;
  }
  for (int64_t r0 = lo; r0 < hi; r0 += kWave) {
    const int64_t r = r0 + lane;
    const bool on = r < hi && pn_rows_listed(kind, src, r);
    const unsigned long long mask = __ballot(on);
    if (r < hi) {
      const int p = on ? off + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
      pos[r] = p;
      if (on) idx[p] = (int32_t)r;
    }
    off += __popcll(mask);
  }
  for (int64_t k = (int64_t)total + threadIdx.x; k < B; k += kListBlock) idx[k] = -1;
  if (threadIdx.x == 0) count[0] = total;
}

// out[k] = src[idx[k]] for the m rows of `out` (a row with idx[k] < 0 is written as zeros and nothing is read for it)
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void pn_rows_gather_kernel(T *out, const T *src, const int32_t *idx, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t k = (int64_t)blockIdx.x * rpb + sub; k < q.B; k += (int64_t)gridDim.x * rpb) {
    const int64_t from = idx[k];
    for (int64_t ch = g; ch < q.nch; ch += G) {
      T v[VW];
      if (from >= 0) {
        load_chunk<T, VEC>(src + from * q.d, ch, q.d, v);
      } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) v[e] = (T)0;
      }
      store_chunk<T, VEC, 0>(out + k * q.d, ch, q.d, v);
    }
  }
}

// out[r] = pos[r] >= 0 ? src[pos[r]] : +0 for all B rows of `out`: every row is written, none is read
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void pn_rows_scatter_kernel(T *out, const T *src, const int32_t *pos, RowsGeom q) {
  constexpr int VW = 16 / sizeof(T);
  const int G = 1 << q.lgG, g = threadIdx.x & (G - 1), sub = threadIdx.x >> q.lgG, rpb = kBlock >> q.lgG;
  for (int64_t r = (int64_t)blockIdx.x * rpb + sub; r < q.B; r += (int64_t)gridDim.x * rpb) {
    const int64_t from = src ? pos[r] : -1;
    for (int64_t ch = g; ch < q.nch; ch += G) {
      T v[VW];
      if (from >= 0) {
        load_chunk<T, VEC>(src + from * q.d, ch, q.d, v);
      } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) v[e] = (T)0;
      }
      store_chunk<T, VEC, 0>(out + r * q.d, ch, q.d, v);
    }
  }
}

template <typename T>
RowsGeom geom(int64_t B, int64_t d) {
  constexpr int VW = 16 / sizeof(T);
  RowsGeom q;
  q.B = B;
  q.d = d;
  q.nch = (d + VW - 1) / VW;
  q.lgG = 0;
  while (((int64_t)1 << q.lgG) < q.nch && (1 << q.lgG) < kBlock) ++q.lgG;
  return q;
}

dim3 grid_for(const RowsGeom &q) { return dim3((unsigned)pn::blocks_for(q.B, kBlock >> q.lgG, kRowsMaxBlocks)); }

// What the launchers below end in: the row geometry of (B, d), the vector form when the caller's operands are `aligned` and d is
// a whole number of chunks, and for the N == n of [LO, HI] the kernel pick(N, V) names (V: std::true_type for the vector form)
// on the capped grid.  pn::kNoCase when n is outside [LO, HI]: the caller's refusal.
template <typename T, int LO, int HI, typename Args, typename Pick>
int rows_launch(const char *name, hipStream_t st, int64_t B, int64_t d, bool aligned, int n, const Args &a, Pick pick, int kid = -1,
                double bytes = 0.0) {
  const bool vec = aligned && d % (int64_t)(16 / sizeof(T)) == 0;
  const RowsGeom q = geom<T>(B, d);
  return pn::with_count<LO, HI>(n, [&](auto N) {     // kid >= 0: booked under that kernel id while profiling is on
    return pn::launch_as(name, kid, bytes, vec ? pick(N, std::true_type{}) : pick(N, std::false_type{}), grid_for(q), dim3(kBlock), st, a, q);
  });
}

template <typename T>
int rows_lin(hipStream_t st, int64_t B, int64_t d, void *out, const void *base, int nk, const void *const *x, const double *c,
             const double *h, const char *name, const void *tail = nullptr) {
  RowsLinArgs<T> a = {};
  a.out = (T *)out;
  a.base = (const T *)base;
  a.h = h;
  a.tail = (const T *)tail;
  for (int j = 0; j < nk; ++j) {
    a.x[j] = (const T *)x[j];
    a.c[j] = c[j];
  }
  const bool al = pn::aligned16(out, base, tail) && pn::aligned16(x, nk);
  const int rc = rows_launch<T, 1, PN_MAX_STAGES>(name, st, B, d, al, nk, a, [&](auto N, auto V) {
    constexpr int NK = decltype(N)::value;
    constexpr bool VEC = decltype(V)::value;
    auto kern = base ? pn_rows_lin_kernel<T, NK, VEC, true> : pn_rows_lin_kernel<T, NK, VEC, false>;
    if (tail && !base) kern = pn_rows_lin_kernel<T, NK, VEC, false, true>;
    return kern;
  });
  if (rc == pn::kNoCase) return pn::fail(std::string(name) + ": nk out of range");
  return rc;
}

template <typename T, bool INF = false>
int rows_combine(hipStream_t st, int64_t B, int64_t d, void *unew, const void *u, int nk, const void *const *K, const double *cb,
                 const double *ce, const double *h, double atol, double rtol, double *enorm) {
  RowsErrArgs<T> a = {};
  a.unew = (T *)unew;
  a.u = (const T *)u;
  a.h = h;
  a.enorm = enorm;
  a.atol = atol;
  a.rtol = rtol;
  for (int j = 0; j < nk; ++j) {
    a.k[j] = (const T *)K[j];
    a.cb[j] = cb ? cb[j] : 0.0;
    a.ce[j] = ce[j];
  }
  const bool al = pn::aligned16(u, unew) && pn::aligned16(K, nk);
  if constexpr (INF) {
    // booked with pn_rk_combine_winf's launches under the error-norm kernels' id: (nk + 1 (+ 1)) vectors of B * d entries
    const double bytes = (double)B * (double)d * sizeof(T) * (nk + 1 + (unew ? 1 : 0));
    const int rc = rows_launch<T, 1, PN_MAX_STAGES>("pn_rows_combine_winf", st, B, d, al, nk, a, [&](auto N, auto V) {
      constexpr int NK = decltype(N)::value;
      constexpr bool VEC = decltype(V)::value;
      return unew ? pn_rows_combine_winf_kernel<T, NK, VEC, true> : pn_rows_combine_winf_kernel<T, NK, VEC, false>;
    }, PN_K_COMBINE_WRMS, bytes);
    return pn::or_fail(rc, "pn_rows_combine_winf: nk out of range");
  }
  const int rc = rows_launch<T, 1, PN_MAX_STAGES>("pn_rows_combine_wrms", st, B, d, al, nk, a, [&](auto N, auto V) {
    constexpr int NK = decltype(N)::value;
    constexpr bool VEC = decltype(V)::value;
    return unew ? pn_rows_combine_wrms_kernel<T, NK, VEC, true> : pn_rows_combine_wrms_kernel<T, NK, VEC, false>;
  });
  return pn::or_fail(rc, "pn_rows_combine_wrms: nk out of range");
}

// rows_combine with the period vectors (d entries each); booked under the error-norm kernels' id like pn_rows_combine_winf
template <typename T, bool INF>
int rows_combine_v(const char *name, hipStream_t st, int64_t B, int64_t d, void *unew, const void *u, int nk, const void *const *K,
                   const double *cb, const double *ce, const double *h, const double *vatol, const double *vrtol, double *enorm) {
  RowsErrVArgs<T> a = {};
  a.unew = (T *)unew;
  a.u = (const T *)u;
  a.h = h;
  a.enorm = enorm;
  a.vatol = vatol;
  a.vrtol = vrtol;
  for (int j = 0; j < nk; ++j) {
    a.k[j] = (const T *)K[j];
    a.cb[j] = cb ? cb[j] : 0.0;
    a.ce[j] = ce[j];
  }
  const bool al = pn::aligned16(u, unew) && pn::aligned16(K, nk);
  const double bytes = (double)B * (double)d * sizeof(T) * (nk + 1 + (unew ? 1 : 0)) + 2.0 * (double)d * sizeof(double);
  const int rc = rows_launch<T, 1, PN_MAX_STAGES>(name, st, B, d, al, nk, a, [&](auto N, auto V) {
    constexpr int NK = decltype(N)::value;
    constexpr bool VEC = decltype(V)::value;
    return unew ? pn_rows_combine_v_kernel<T, NK, VEC, true, INF> : pn_rows_combine_v_kernel<T, NK, VEC, false, INF>;
  }, PN_K_COMBINE_WRMS, bytes);
  return pn::or_fail(rc, (std::string(name) + ": nk out of range").c_str());
}

template <typename T>
int rows_commit(hipStream_t st, int64_t B, int64_t d, void *unext, const void *u, const void *unew, const int32_t *accept,
                const int32_t *hit, void *sol, int64_t ld, int nout) {
  constexpr int VW = 16 / sizeof(T);
  RowsCommitArgs<T> a = {};
  a.unext = (T *)unext;
  a.u = (const T *)u;
  a.unew = (const T *)unew;
  a.sol = (T *)sol;
  a.accept = accept;
  a.hit = hit;
  a.ld = ld;
  a.nout = nout;
  const bool vec = (d % VW) == 0 && pn::aligned16(unext, u, unew, sol) && (!sol || (ld % VW) == 0);
  const RowsGeom q = geom<T>(B, d);
  return pn::launch("pn_rows_commit", vec ? pn_rows_commit_kernel<T, true> : pn_rows_commit_kernel<T, false>, grid_for(q), dim3(kBlock), st,
                    a, q);
}

template <typename T>
int rows_accum(hipStream_t st, int64_t B, int64_t d, void *out, const void *lam, int nk, const void *const *x, const void *g,
               int64_t ld, const int32_t *hit, int nout) {
  constexpr int VW = 16 / sizeof(T);
  RowsAccumArgs<T> a = {};
  a.out = (T *)out;
  a.lam = (const T *)lam;
  a.g = (const T *)g;
  a.hit = hit;
  a.ld = ld;
  a.nout = nout;
  for (int j = 0; j < nk; ++j) a.x[j] = (const T *)x[j];
  const bool al = pn::aligned16(out, lam, g) && (!g || (ld % VW) == 0) && pn::aligned16(x, nk);
  const int rc = rows_launch<T, 0, PN_MAX_STAGES>("pn_rows_adj_accum", st, B, d, al, nk, a, [](auto N, auto V) {
    return pn_rows_adj_accum_kernel<T, decltype(N)::value, decltype(V)::value>;
  });
  return pn::or_fail(rc, "pn_rows_adj_accum: nk out of range");
}

template <typename T>
int rows_dense_eval(hipStream_t st, int64_t B, int64_t d, const void *u, int nk, const void *const *K, const double *P,
                    const void *unew, void *sol, int64_t ld, int nout, const double *times, const double *log_d, const double *tnew,
                    int32_t *hit, int32_t *next, int32_t *range) {
  constexpr int VW = 16 / sizeof(T);
  RowsDenseEvalArgs<T> a = {};
  a.u = (const T *)u;
  a.unew = (const T *)unew;
  a.sol = (T *)sol;
  a.ld = ld;
  a.nout = nout;
  a.times = times;
  a.heff = log_d;
  a.trow = log_d + B;
  a.tnew = tnew;
  a.hit = hit;
  a.next = next;
  a.range = range;
  for (int j = 0; j < nk; ++j) {
    a.k[j] = (const T *)K[j];
    for (int p = 0; p < PN_DENSE_MAX_POW; ++p) a.P[j][p] = P[j * PN_DENSE_MAX_POW + p];
  }
  const bool al = pn::aligned16(u, unew, sol) && (ld % VW) == 0 && pn::aligned16(K, nk);
  const int rc = rows_launch<T, 1, PN_MAX_STAGES>("pn_rows_dense_eval", st, B, d, al, nk, a, [](auto N, auto V) {
    return pn_rows_dense_eval_kernel<T, decltype(N)::value, decltype(V)::value>;
  });
  return pn::or_fail(rc, "pn_rows_dense_eval: nk out of range");
}

template <typename T>
int rows_dense_adjoint(hipStream_t st, int64_t B, int64_t d, const void *g, int64_t ld, int nout, const double *times,
                       const double *log_d, const int32_t *range, int nd, const double *P, void *const *D, void *G) {
  constexpr int VW = 16 / sizeof(T);
  RowsDenseAdjArgs<T> a = {};
  a.g = (const T *)g;
  a.ld = ld;
  a.nout = nout;
  a.times = times;
  a.heff = log_d;
  a.trow = log_d + B;
  a.range = range;
  a.G = (T *)G;
  for (int j = 0; j < nd; ++j) {
    a.d[j] = (T *)D[j];
    for (int p = 0; p < PN_DENSE_MAX_POW; ++p) a.P[j][p] = P[j * PN_DENSE_MAX_POW + p];
  }
  const bool al = pn::aligned16(g, G) && (ld % VW) == 0 && pn::aligned16(D, nd);
  const int rc = rows_launch<T, 1, PN_MAX_STAGES>("pn_rows_dense_adjoint", st, B, d, al, nd, a, [](auto N, auto V) {
    return pn_rows_dense_adjoint_kernel<T, decltype(N)::value, decltype(V)::value>;
  });
  return pn::or_fail(rc, "pn_rows_dense_adjoint: nd out of range");
}

template <typename T>
int rows_tgrad_dots(hipStream_t st, int64_t B, int64_t d, int np, const void *const *x, const void *const *y, const double *coef,
                    double *rowacc, int accumulate) {
  RowsTgDotArgs<T> a = {};
  for (int p = 0; p < np; ++p) {
    a.x[p] = (const T *)x[p];
    a.y[p] = (const T *)y[p];
    a.c[p] = coef[p];
  }
  a.rowacc = rowacc;
  a.accumulate = accumulate ? 1 : 0;
  const bool al = pn::aligned16(x, np) && pn::aligned16(y, np);
  const int rc = rows_launch<T, 1, PN_MAX_STAGES>("pn_rows_tgrad_dots", st, B, d, al, np, a, [](auto N, auto V) {
    return pn_rows_tgrad_dots_kernel<T, decltype(N)::value, decltype(V)::value>;
  });
  return pn::or_fail(rc, "pn_rows_tgrad_dots: np out of range");
}

template <typename T>
int rows_dense_tgrad(hipStream_t st, int64_t B, int64_t d, const void *g, int64_t ld, int nout, const double *times,
                     const double *log_d, const int32_t *range, int nk, const double *P, const void *const *K, double *erow) {
  constexpr int VW = 16 / sizeof(T);
  RowsTgDenseArgs<T> a = {};
  a.g = (const T *)g;
  a.ld = ld;
  a.nout = nout;
  a.times = times;
  a.heff = log_d;
  a.trow = log_d + B;
  a.range = range;
  a.erow = erow;
  for (int j = 0; j < nk; ++j) {
    a.k[j] = (const T *)K[j];
    for (int p = 0; p < PN_DENSE_MAX_POW; ++p) a.P[j][p] = P[j * PN_DENSE_MAX_POW + p];
  }
  const bool al = pn::aligned16(g) && (ld % VW) == 0 && pn::aligned16(K, nk);
  const int rc = rows_launch<T, 1, PN_MAX_STAGES>("pn_rows_dense_tgrad", st, B, d, al, nk, a, [](auto N, auto V) {
    return pn_rows_dense_tgrad_kernel<T, decltype(N)::value, decltype(V)::value>;
  });
  return pn::or_fail(rc, "pn_rows_dense_tgrad: nk out of range");
}

// the two row copies of -pn_rows_compact: `rows` rows of `out` are written; unprofiled, as pn_rows_stage / pn_rows_commit are
template <typename T, bool GATHER>
int rows_copy(const char *name, hipStream_t st, int64_t rows, int64_t d, void *out, const void *src, const int32_t *map) {
  constexpr int VW = 16 / sizeof(T);
  const bool vec = (d % VW) == 0 && pn::aligned16(out, src);
  const RowsGeom q = geom<T>(rows, d);
  auto kern = GATHER ? (vec ? pn_rows_gather_kernel<T, true> : pn_rows_gather_kernel<T, false>)
                     : (vec ? pn_rows_scatter_kernel<T, true> : pn_rows_scatter_kernel<T, false>);
  return pn::launch(name, kern, grid_for(q), dim3(kBlock), st, (T *)out, (const T *)src, map, q);
}

int tgrad_reduce_blocks(int64_t B) { return (int)pn::blocks_for(B, kBlock, kTgReduceBlocks); }

int bad_shape(const char *name, int64_t B, int64_t d) {
  if (B < 1 || d < 1 || B > ((int64_t)1 << 40) / d) return pn::fail(std::string(name) + ": B and d must be positive");
  return 0;
}

// pn_rows_adj_theta and, with the D_i of a row's interpolated outputs as the last term (`dense`), pn_rows_adj_theta_dense
int rows_adj_theta(const char *name, void *stream, int dtype, int64_t B, int64_t d, void *w, const void *lambda, double c_lam, int nk,
                   const void *const *dlam, const double *coef, const double *h, const void *dense_w, bool dense) {
  if (bad_shape(name, B, d)) return 1;
  if (!w || !h || (dense && !dense_w) || nk < 0 || nk > PN_MAX_STAGES - 1 || (nk > 0 && (!dlam || !coef)) || (!lambda && nk == 0))
    return pn::fail(std::string(name) + ": null argument or nk outside 0..6");
  const void *x[PN_MAX_TERMS];
  double c[PN_MAX_TERMS];
  int n = 0;
  if (lambda) {
    x[n] = lambda;
    c[n++] = c_lam;
  }
  for (int j = 0; j < nk; ++j) {
    if (!dlam[j]) return pn::fail(std::string(name) + ": null vector");
    x[n] = dlam[j];
    c[n++] = coef[j];
  }
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return rows_lin<decltype(t)>(st, B, d, w, nullptr, n, x, c, h, name, dense_w); });
  return rc == pn::kNoCase ? pn::fail(std::string(name) + ": unknown dtype") : rc;
}

template <bool INF>
int rows_combine_v_entry(const char *name, void *stream, int dtype, int64_t B, int64_t d, void *unew, const void *u, int nk,
                         const void *const *K, const double *coef_b, const double *coef_e, const double *h, const double *vatol,
                         const double *vrtol, int64_t period, double *enorm) {
  if (bad_shape(name, B, d)) return 1;
  const std::string who(name);
  if (!u || !h || !enorm || nk < 1 || nk > PN_MAX_STAGES || !K || !coef_e || (unew && !coef_b))
    return pn::fail(who + ": null argument or nk outside 1..7");
  if (!vatol || !vrtol) return pn::fail(who + ": the tolerance vectors are required (two scalars: the entry point without _v)");
  if (period != d) return pn::fail(who + ": the period must be d (one entry per column; the rows share the vectors)");
  for (int j = 0; j < nk; ++j)
    if (!K[j]) return pn::fail(who + ": null stage derivative");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) {
    return rows_combine_v<decltype(t), INF>(name, st, B, d, unew, u, nk, K, coef_b, coef_e, h, vatol, vrtol, enorm);
  });
  return pn::or_fail(rc, (who + ": unknown dtype").c_str());
}

}  // namespace

extern "C" {

int pn_rows_stage(void *stream, int dtype, int64_t B, int64_t d, void *y, const void *u, int nk, const void *const *K,
                  const double *coef, const double *h) {
  if (bad_shape("pn_rows_stage", B, d)) return 1;
  if (!y || !u || !h || nk < 1 || nk > PN_MAX_STAGES || !K || !coef) return pn::fail("pn_rows_stage: null argument or nk outside 1..7");
  for (int j = 0; j < nk; ++j)
    if (!K[j]) return pn::fail("pn_rows_stage: null stage derivative");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return rows_lin<decltype(t)>(st, B, d, y, u, nk, K, coef, h, "pn_rows_stage"); });
  return pn::or_fail(rc, "pn_rows_stage: unknown dtype");
}

int pn_rows_combine_wrms(void *stream, int dtype, int64_t B, int64_t d, void *unew, const void *u, int nk, const void *const *K,
                         const double *coef_b, const double *coef_e, const double *h, double atol, double rtol, double *enorm) {
  if (bad_shape("pn_rows_combine_wrms", B, d)) return 1;
  if (!u || !h || !enorm || nk < 1 || nk > PN_MAX_STAGES || !K || !coef_e || (unew && !coef_b))
    return pn::fail("pn_rows_combine_wrms: null argument or nk outside 1..7");
  for (int j = 0; j < nk; ++j)
    if (!K[j]) return pn::fail("pn_rows_combine_wrms: null stage derivative");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return rows_combine<decltype(t)>(st, B, d, unew, u, nk, K, coef_b, coef_e, h, atol, rtol, enorm); });
  return pn::or_fail(rc, "pn_rows_combine_wrms: unknown dtype");
}

int pn_rows_combine_winf(void *stream, int dtype, int64_t B, int64_t d, void *unew, const void *u, int nk, const void *const *K,
                         const double *coef_b, const double *coef_e, const double *h, double atol, double rtol, double *enorm) {
  if (bad_shape("pn_rows_combine_winf", B, d)) return 1;
  if (!u || !h || !enorm || nk < 1 || nk > PN_MAX_STAGES || !K || !coef_e || (unew && !coef_b))
    return pn::fail("pn_rows_combine_winf: null argument or nk outside 1..7");
  for (int j = 0; j < nk; ++j)
    if (!K[j]) return pn::fail("pn_rows_combine_winf: null stage derivative");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return rows_combine<decltype(t), true>(st, B, d, unew, u, nk, K, coef_b, coef_e, h, atol, rtol, enorm); });
  return pn::or_fail(rc, "pn_rows_combine_winf: unknown dtype");
}

int pn_rows_combine_wrms_v(void *stream, int dtype, int64_t B, int64_t d, void *unew, const void *u, int nk, const void *const *K,
                           const double *coef_b, const double *coef_e, const double *h, const double *vatol, const double *vrtol,
                           int64_t period, double *enorm) {
  return rows_combine_v_entry<false>("pn_rows_combine_wrms_v", stream, dtype, B, d, unew, u, nk, K, coef_b, coef_e, h, vatol, vrtol, period, enorm);
}

int pn_rows_combine_winf_v(void *stream, int dtype, int64_t B, int64_t d, void *unew, const void *u, int nk, const void *const *K,
                           const double *coef_b, const double *coef_e, const double *h, const double *vatol, const double *vrtol,
                           int64_t period, double *enorm) {
  return rows_combine_v_entry<true>("pn_rows_combine_winf_v", stream, dtype, B, d, unew, u, nk, K, coef_b, coef_e, h, vatol, vrtol, period, enorm);
}

int64_t pn_rows_work_bytes(int64_t B) {
  const int64_t nb = (B + kBlock - 1) / kBlock;
  return (int64_t)sizeof(double) * (kTicketDoubles + 2 * (nb < 1 ? 1 : nb));
}

int pn_rows_control(void *stream, const pn_ts *ts, int64_t B, int nspan, const double *span_dev, double max_time,
                    const double *enorm, double *sd, int32_t *si, double *log_d, int32_t *log_hit, int32_t *accept,
                    int32_t *summary, void *work) {
  if (!ts || B < 1 || B > 0x7fffff00 || !enorm || !sd || !si || !log_d || !log_hit || !accept || !summary || !work ||
      (nspan > 0 && !span_dev))
    return pn::fail("pn_rows_control: null argument");
  PnRowsCtl rc;
  pn::rows_ctl_config(ts, nspan, max_time, &rc);
  return pn::launch("pn_rows_control", pn_rows_control_kernel, dim3((unsigned)pn::blocks_for(B, kBlock)), dim3(kBlock), (hipStream_t)stream,
                    rc, span_dev, B, enorm, sd, si, log_d, log_hit, accept, summary, (double *)work);
}

int pn_rows_commit(void *stream, int dtype, int64_t B, int64_t d, void *unext, const void *u, const void *unew,
                   const int32_t *accept, const int32_t *hit, void *sol, int64_t ld, int nout) {
  if (bad_shape("pn_rows_commit", B, d)) return 1;
  if (!unext || !u || !unew || !accept || (sol && (!hit || nout < 1 || ld < B * d)))
    return pn::fail("pn_rows_commit: null argument or an output stride shorter than a state");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return rows_commit<decltype(t)>(st, B, d, unext, u, unew, accept, hit, sol, ld, nout); });
  return pn::or_fail(rc, "pn_rows_commit: unknown dtype");
}

int pn_rows_adj_theta(void *stream, int dtype, int64_t B, int64_t d, void *w, const void *lambda, double c_lam, int nk,
                      const void *const *dlam, const double *coef, const double *h) {
  return rows_adj_theta("pn_rows_adj_theta", stream, dtype, B, d, w, lambda, c_lam, nk, dlam, coef, h, nullptr, false);
}

int pn_rows_adj_accum(void *stream, int dtype, int64_t B, int64_t d, void *lambda_out, const void *lambda, int nk,
                      const void *const *dlam, const void *g, int64_t ld, const int32_t *hit, int nout) {
  if (bad_shape("pn_rows_adj_accum", B, d)) return 1;
  if (!lambda_out || !lambda || nk < 0 || nk > PN_MAX_STAGES || (nk > 0 && !dlam) || (g && (!hit || nout < 1 || ld < B * d)))
    return pn::fail("pn_rows_adj_accum: null argument, nk outside 0..7 or a cotangent stride shorter than a state");
  for (int j = 0; j < nk; ++j)
    if (!dlam[j]) return pn::fail("pn_rows_adj_accum: null vector");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return rows_accum<decltype(t)>(st, B, d, lambda_out, lambda, nk, dlam, g, ld, hit, nout); });
  return pn::or_fail(rc, "pn_rows_adj_accum: unknown dtype");
}

int pn_rows_adj_theta_dense(void *stream, int dtype, int64_t B, int64_t d, void *w, const void *lambda, double c_lam, int nk,
                            const void *const *dlam, const double *coef, const double *h, const void *dense_w) {
  return rows_adj_theta("pn_rows_adj_theta_dense", stream, dtype, B, d, w, lambda, c_lam, nk, dlam, coef, h, dense_w, true);
}

int pn_rows_dense_eval(void *stream, int dtype, int64_t B, int64_t d, const void *u, int nk, const void *const *K, const double *P,
                       const void *unew, void *sol, int64_t ld, int nout, const double *times_dev, const double *log_d,
                       const double *tnew, int32_t *log_hit, int32_t *next, int32_t *range) {
  if (bad_shape("pn_rows_dense_eval", B, d)) return 1;
  if (!u || !unew || !sol || !P || !K || nk < 1 || nk > PN_MAX_STAGES || !times_dev || !log_d || !tnew || !log_hit || !next || !range)
    return pn::fail("pn_rows_dense_eval: null argument or nk outside 1..7");
  if (nout < 2 || ld < B * d) return pn::fail("pn_rows_dense_eval: fewer than two output times or an output stride shorter than a state");
  for (int j = 0; j < nk; ++j)
    if (!K[j]) return pn::fail("pn_rows_dense_eval: null stage derivative");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) {
    return rows_dense_eval<decltype(t)>(st, B, d, u, nk, K, P, unew, sol, ld, nout, times_dev, log_d, tnew, log_hit, next, range);
  });
  return pn::or_fail(rc, "pn_rows_dense_eval: unknown dtype");
}

int pn_rows_dense_adjoint(void *stream, int dtype, int64_t B, int64_t d, const void *g, int64_t ld, int nout, const double *times_dev,
                          const double *log_d, const int32_t *range, int nd, const double *P, void *const *D, void *G) {
  if (bad_shape("pn_rows_dense_adjoint", B, d)) return 1;
  if (!g || !times_dev || !log_d || !range || !P || !D || !G || nd < 1 || nd > PN_MAX_STAGES)
    return pn::fail("pn_rows_dense_adjoint: null argument or nd outside 1..7");
  if (nout < 2 || ld < B * d) return pn::fail("pn_rows_dense_adjoint: fewer than two output times or a cotangent stride shorter than a state");
  for (int j = 0; j < nd; ++j)
    if (!D[j]) return pn::fail("pn_rows_dense_adjoint: null output vector");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) {
    return rows_dense_adjoint<decltype(t)>(st, B, d, g, ld, nout, times_dev, log_d, range, nd, P, D, G);
  });
  return pn::or_fail(rc, "pn_rows_dense_adjoint: unknown dtype");
}

// The plan of pn_rows_dense_eval on host arrays (no device; the CPU-only tests' stand-in): the shared text of pn_adapt.h.
int pn_rows_dense_plan_host(int64_t B, int nout, const double *times, const double *log_d, const double *tnew, int32_t *log_hit,
                            int32_t *next, int32_t *range, int nk, const double *P, double *coef) {
  if (B < 1 || nout < 2 || !times || !log_d || !range || (next && (!tnew || !log_hit)) || nk < 0 || nk > PN_MAX_STAGES ||
      (coef && (nk < 1 || !P)))
    return pn::fail("pn_rows_dense_plan_host: null argument, fewer than two output times or nk outside 0..7");
  for (int64_t r = 0; r < B; ++r) {
    const double h = log_d[r], tr = log_d[B + r];
    if (next) {
      const PnDensePlan p = pn_rows_dense_plan_row(times, nout, h, tnew[r], log_hit[r], next[r]);
      next[r] = p.next;
      range[r] = p.lo;
      range[B + r] = p.hi;
      log_hit[r] = p.hit;
    }
    if (!coef) continue;
    const int lo = range[r] < 0 ? 0 : range[r], hi = range[B + r] > nout ? nout : range[B + r];
    for (int o = lo; o < hi; ++o)
      for (int j = 0; j < nk; ++j) coef[((int64_t)o * B + r) * nk + j] = pn_rows_dense_coef(P + j * PN_DENSE_MAX_POW, times[o], tr, h);
  }
  return 0;
}

/* -pn_rows_compact 1: the ordered list of the rows with work to do (one workgroup; `work` is not used: the list needs no
 * arrival counters) and the row copies around func. */
int pn_rows_list(void *stream, int64_t B, int kind, const void *src, int32_t *idx, int32_t *pos, int32_t *count, void *work) {
  (void)work;
  if (B < 1 || B > 0x7fffff00 || (kind != 0 && kind != 1) || !src || !idx || !pos || !count)
    return pn::fail("pn_rows_list: null argument, B not positive or kind outside 0..1");
  return pn::launch("pn_rows_list", pn_rows_list_kernel, dim3(1), dim3(kListBlock), (hipStream_t)stream, kind, src, B, idx, pos, count);
}

int pn_rows_list_host(int64_t B, int kind, const void *src, int32_t *idx, int32_t *pos, int32_t *count) {
  if (B < 1 || B > 0x7fffff00 || (kind != 0 && kind != 1) || !src || !idx || !pos || !count)
    return pn::fail("pn_rows_list_host: null argument, B not positive or kind outside 0..1");
  pn_rows_list_rows(kind, src, B, idx, pos, count);
  return 0;
}

int pn_rows_gather(void *stream, int dtype, int64_t m, int64_t d, void *out, const void *src, const int32_t *idx) {
  if (m == 0) return 0;
  if (bad_shape("pn_rows_gather", m, d)) return 1;
  if (!out || !src || !idx) return pn::fail("pn_rows_gather: null argument");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return rows_copy<decltype(t), true>("pn_rows_gather", st, m, d, out, src, idx); });
  return pn::or_fail(rc, "pn_rows_gather: unknown dtype");
}

int pn_rows_scatter(void *stream, int dtype, int64_t B, int64_t d, void *out, const void *src, const int32_t *pos) {
  if (bad_shape("pn_rows_scatter", B, d)) return 1;
  if (!out || !pos) return pn::fail("pn_rows_scatter: null argument");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return rows_copy<decltype(t), false>("pn_rows_scatter", st, B, d, out, src, pos); });
  return pn::or_fail(rc, "pn_rows_scatter: unknown dtype");
}

int pn_rows_tgrad_dots(void *stream, int dtype, int64_t B, int64_t d, int np, const void *const *x, const void *const *y,
                       const double *coef, double *rowacc, int accumulate) {
  if (bad_shape("pn_rows_tgrad_dots", B, d)) return 1;
  if (np < 1 || np > PN_MAX_STAGES || !x || !y || !coef || !rowacc) return pn::fail("pn_rows_tgrad_dots: null argument or np outside 1..7");
  for (int p = 0; p < np; ++p)
    if (!x[p] || !y[p]) return pn::fail("pn_rows_tgrad_dots: null vector");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) { return rows_tgrad_dots<decltype(t)>(st, B, d, np, x, y, coef, rowacc, accumulate); });
  return pn::or_fail(rc, "pn_rows_tgrad_dots: unknown dtype");
}

int pn_rows_dense_tgrad(void *stream, int dtype, int64_t B, int64_t d, const void *g, int64_t ld, int nout, const double *times_dev,
                        const double *log_d, const int32_t *range, int nk, const double *P, const void *const *K, double *erow) {
  if (bad_shape("pn_rows_dense_tgrad", B, d)) return 1;
  if (!g || !times_dev || !log_d || !range || !P || !K || !erow || nk < 1 || nk > PN_MAX_STAGES)
    return pn::fail("pn_rows_dense_tgrad: null argument or nk outside 1..7");
  if (nout < 2 || ld < B * d) return pn::fail("pn_rows_dense_tgrad: fewer than two output times or a cotangent stride shorter than a state");
  for (int j = 0; j < nk; ++j)
    if (!K[j]) return pn::fail("pn_rows_dense_tgrad: null stage derivative");
  hipStream_t st = (hipStream_t)stream;
  const int rc = pn::with_dtype(dtype, [&](auto t) {
    return rows_dense_tgrad<decltype(t)>(st, B, d, g, ld, nout, times_dev, log_d, range, nk, P, K, erow);
  });
  return pn::or_fail(rc, "pn_rows_dense_tgrad: unknown dtype");
}

int pn_rows_tgrad_scatter(void *stream, int64_t B, int nout, double *dtrow, const double *rowacc, int nt, const double *const *tbar,
                          const double *coef, const double *tbar0, double c_last, int fsal, const double *log_d,
                          const int32_t *log_hit, const int32_t *range, const double *erow, const double *times_dev, double *held,
                          int32_t *iv, int flush) {
  PnRowsTgScatter a;
  const char *why = pn::rows_tgrad_scatter_args(B, nout, dtrow, rowacc, nt, tbar, coef, tbar0, c_last, fsal, log_d, log_hit, range, erow,
                                       times_dev, held, iv, flush, &a);
  if (why) return pn::fail(std::string("pn_rows_tgrad_scatter: ") + why);
  return pn::launch("pn_rows_tgrad_scatter", pn_rows_tgrad_scatter_kernel, dim3((unsigned)pn::blocks_for(B, kBlock)), dim3(kBlock),
                    (hipStream_t)stream, a, B);
}

int64_t pn_rows_tgrad_work_bytes(int64_t B, int nout) {
  return (int64_t)sizeof(double) * (kTicketDoubles + (int64_t)(nout < 1 ? 1 : nout) * tgrad_reduce_blocks(B));
}

int pn_rows_tgrad_reduce(void *stream, int64_t B, int nout, const double *dtrow, double *dt, void *work) {
  if (B < 1 || nout < 1 || nout > 65535 || !dtrow || !dt || !work)
    return pn::fail("pn_rows_tgrad_reduce: null argument, B not positive or nout outside 1..65535");
  return pn::launch("pn_rows_tgrad_reduce", pn_rows_tgrad_reduce_kernel, dim3((unsigned)tgrad_reduce_blocks(B), (unsigned)nout),
                    dim3(kBlock), (hipStream_t)stream, dtrow, B, nout, dt, (double *)work);
}

}  // extern "C"
