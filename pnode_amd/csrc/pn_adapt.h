// pnode_amd -- the step-size controller as ONE piece of text for the host engine and the device: TSAdaptChoose (none |
// basic), the MATCHSTEP / time-span adjustment and the bookkeeping TSSolve does after an accepted step, over a small POD
// state.  pn_ts_judge (pn_ts.cpp) runs it on the solver's own state; -pn_adapt_scope sample runs it once per batch row and
// round, on the device (pn_rows_control, pn_rows.hip) or on host arrays (pn_rows_control_host, the CPU-only tests).
// Plain C++ (also read by g++ without HIP).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PN_HD inline
#endif

struct pn_ts;

struct PnCtlCfg {
  double safety, reject_safety, clip_lo, clip_hi;
  double dt_min, dt_max;
  double match_stretch, match_halve;
  double span_reltol, span_abstol;
  double max_time;
  int64_t max_steps;
  int max_reject;
  int order;        // exponent of the controller
  int nspan;        // 0: no time span (integrate to max_time)
};

struct PnCtlState {
  double ptime, time_step, dt_span_cached;
  int64_t steps, rejections;
  int spanctr, rejections_this_step;
  int prev_attempt_rejected, finished;
};

enum { PN_CTL_OK = 0, PN_CTL_NAN = 1, PN_CTL_MAX_REJECT = 2 };

#define PN_CTL_EPS 2.220446049250313e-16        /* DBL_EPSILON */
#define PN_CTL_SQRT_EPS 1.4901161193847656e-08  /* 2^-26, exactly sqrt(DBL_EPSILON) */

PN_HD double pn_ctl_min(double a, double b) { return (b < a) ? b : a; }        // std::min / std::max, argument for argument
PN_HD double pn_ctl_max(double a, double b) { return (a < b) ? b : a; }

PN_HD double pn_ctl_next_target(const PnCtlCfg &c, const double *span, const PnCtlState &s) {
  if (c.nspan > 0 && s.spanctr < c.nspan) return span[s.spanctr];
  return c.max_time;
}

PN_HD bool pn_ctl_close_rel(double a, double b, double rtol) {
  return fabs(a - b) <= rtol * pn_ctl_max(fabs(a), fabs(b));
}

// One judgement of the attempt of size s.time_step from s.ptime.  enorm < 0: no error estimate (fixed step).  Returns
// PN_CTL_OK, or a failure (the state is then finished).  *accept, *hit_span (index of the span point this step reached, or
// -1) and *done (1 final time reached, 2 stopped by max_steps) as pn_ts_judge documents them.
PN_HD int pn_ctl_judge(const PnCtlCfg &c, const double *span, PnCtlState &s, double enorm, int *accept_out, int *hit_span,
                       int *done) {
  // (see pn_rows_judge_row: the host and the device must round alike; here span_reltol * fabs(h) + span_abstol is the candidate)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double h = s.time_step;
  bool accept = true;
  double hnew = h;
  *hit_span = -1;
  *done = 0;
  *accept_out = 0;
  if (enorm >= 0 || enorm != enorm) {
    if (!(enorm == enorm) || std::isinf(enorm)) {
      s.finished = 1;
      return PN_CTL_NAN;
    }
    double safety = c.safety;
    if (enorm > 1.0) {
      if (s.prev_attempt_rejected) safety *= c.reject_safety;
      accept = h < (1 + PN_CTL_SQRT_EPS) * c.dt_min;
    }
    double hfac = enorm > 0 ? safety * pow(enorm, -1.0 / (double)c.order) : (double)INFINITY;
    hfac = pn_ctl_min(pn_ctl_max(hfac, c.clip_lo), c.clip_hi);
    hnew = pn_ctl_min(pn_ctl_max(h * hfac, c.dt_min), c.dt_max);
  }
  if (!accept) {
    s.time_step = hnew;
    s.rejections++;
    s.prev_attempt_rejected = 1;
    if (++s.rejections_this_step > c.max_reject && c.max_reject >= 0) {
      s.finished = 1;
      return PN_CTL_MAX_REJECT;
    }
    return PN_CTL_OK;
  }
  // --- accepted: choose the next step so that every target time is hit exactly
  double t = s.ptime + h;
  {
    double tend;
    if (c.nspan > 0) {
      const bool hit = s.spanctr < c.nspan && fabs(t - span[s.spanctr]) <= c.span_reltol * fabs(h) + c.span_abstol;
      if (hit) {
        tend = s.spanctr + 1 < c.nspan ? span[s.spanctr + 1] : c.max_time;
        if (s.dt_span_cached > 0) {
          // the steps that approached this point were cut (or stretched) to land on it: go back to the step that was
          // wanted before the first of those adjustments -- unless the controller has chosen a new one meanwhile
          if (hnew == h) hnew = s.dt_span_cached;
          s.dt_span_cached = 0;
        }
      } else {
        tend = pn_ctl_next_target(c, span, s);
      }
    } else {
      tend = c.max_time;
    }
    if (t < tend) {
      const double hmax = tend - t, wanted = hnew;
      if (wanted * c.match_halve > hmax) hnew = hmax / 2;
      if (wanted * (1.0 + c.match_stretch) > hmax) hnew = hmax;
      // remember the unadjusted step ONCE per approach: a halved step that is later stretched onto the point must
      // not replace the user's step in the cache (it would never come back)
      if (c.nspan > 0 && hnew != wanted && !(s.dt_span_cached > 0)) s.dt_span_cached = wanted;
    }
  }
  // land exactly on the target when the matched step is within round-off of it
  const double tgt = pn_ctl_next_target(c, span, s);
  if (t != tgt && pn_ctl_close_rel(t, tgt, 16 * PN_CTL_EPS)) t = tgt;
  const double tprev = s.ptime;
  s.ptime = t;
  s.time_step = hnew;
  s.steps++;
  s.prev_attempt_rejected = 0;
  s.rejections_this_step = 0;
  if (c.nspan > 0 && s.spanctr < c.nspan && fabs(t - span[s.spanctr]) <= c.span_reltol * fabs(t - tprev) + c.span_abstol) {
    *hit_span = s.spanctr;
    s.spanctr++;
  }
  *accept_out = 1;
  if (s.ptime >= c.max_time) {
    s.finished = 1;
    *done = 1;
  } else if (s.steps >= c.max_steps) {
    s.finished = 1;
    *done = 2;                         // TS_CONVERGED_ITS: stopped by ts_max_steps
  }
  return PN_CTL_OK;
}

// ------------------------------------------------------------------------------------------
// -pn_adapt_scope sample: the state of B controllers as device (or host) arrays, one row each.
//   sd: doubles [4][B]   t, h, t_first (where the row's next first stage derivative is evaluated), dt_span_cached
//   si: int32   [8][B]   spanctr, steps, rejections, rejections_this_step, prev_attempt_rejected, finished, failure, -
// and one row's judgement of a round.  Writes the round's log (h_eff, t and t_first at the round's start, hit index) and
// the accept mask; returns 1 when the row is still unfinished afterwards.
// ------------------------------------------------------------------------------------------
enum { PN_ROWS_T = 0, PN_ROWS_H = 1, PN_ROWS_TFIRST = 2, PN_ROWS_CACHED = 3, PN_ROWS_ND = 4 };
enum { PN_ROWS_SPANCTR = 0, PN_ROWS_STEPS, PN_ROWS_REJ, PN_ROWS_REJ_STEP, PN_ROWS_PREV_REJ, PN_ROWS_FINISHED, PN_ROWS_FAIL,
       PN_ROWS_NI = 8 };

struct PnRowsCtl {
  PnCtlCfg cfg;
  double c_last;     // c of the last stage of a first-same-as-last tableau
  int fsal;
};

PN_HD int pn_rows_judge_row(const PnRowsCtl &rc, const double *span, int64_t B, int64_t r, const double *enorm, double *sd,
                            int32_t *si, double *log_d, int32_t *log_hit, int32_t *accept) {
  // Contraction is switched off, as in pn_rows_dense_coef below: hipcc fused t0 + c_last * h0 (the first-stage time of a
  // first-same-as-last tableau) into one rounding on the device, the host rounds twice.  5dp's c_last is 1 - 2^-52, so the
  // product rounds whenever h0 is no power of two, and the two forms of t_first differed in the last bit: from t0 = 11/128
  // with h0 = 5/128 the host gives 1/8, the fused form 1/8 - 2^-56 (tests/test_gpu_rows_controller.py, exact scripts).
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double t0 = sd[PN_ROWS_T * B + r], h0 = sd[PN_ROWS_H * B + r], tf0 = sd[PN_ROWS_TFIRST * B + r];
  log_d[B + r] = t0;
  log_d[2 * B + r] = tf0;
  if (si[PN_ROWS_FINISHED * B + r]) {
    log_d[r] = 0.0;
    log_hit[r] = -1;
    accept[r] = 0;
    return 0;
  }
  PnCtlState s;
  s.ptime = t0;
  s.time_step = h0;
  s.dt_span_cached = sd[PN_ROWS_CACHED * B + r];
  s.spanctr = si[PN_ROWS_SPANCTR * B + r];
  s.steps = si[PN_ROWS_STEPS * B + r];
  s.rejections = si[PN_ROWS_REJ * B + r];
  s.rejections_this_step = si[PN_ROWS_REJ_STEP * B + r];
  s.prev_attempt_rejected = si[PN_ROWS_PREV_REJ * B + r];
  s.finished = 0;
  int acc = 0, hit = -1, done = 0;
  const int fail = pn_ctl_judge(rc.cfg, span, s, enorm[r], &acc, &hit, &done);
  if (done && rc.cfg.nspan == 0) hit = 0;              // no time span: the final state is the one output
  if (s.finished) s.time_step = 0.0;                   // later rounds are the identity on this row
  sd[PN_ROWS_T * B + r] = s.ptime;
  sd[PN_ROWS_H * B + r] = s.time_step;
  sd[PN_ROWS_CACHED * B + r] = s.dt_span_cached;
  if (acc) sd[PN_ROWS_TFIRST * B + r] = rc.fsal ? t0 + rc.c_last * h0 : s.ptime;
  si[PN_ROWS_SPANCTR * B + r] = s.spanctr;
  si[PN_ROWS_STEPS * B + r] = (int32_t)s.steps;
  si[PN_ROWS_REJ * B + r] = (int32_t)s.rejections;
  si[PN_ROWS_REJ_STEP * B + r] = s.rejections_this_step;
  si[PN_ROWS_PREV_REJ * B + r] = s.prev_attempt_rejected;
  si[PN_ROWS_FINISHED * B + r] = s.finished ? (done ? done : 3) : 0;
  si[PN_ROWS_FAIL * B + r] = fail;
  log_d[r] = acc ? h0 : 0.0;
  log_hit[r] = acc ? hit : -1;
  accept[r] = acc;
  return s.finished ? 0 : 1;
}

// ------------------------------------------------------------------------------------------
// -pn_adapt_scope sample with -pn_output_times interpolate: what one row's accepted attempt serves of the output times.
// The controller above sees [t[0], t[T-1]] only; after it has judged a round, a row that was accepted from t_r with h_r
// to tnew_r (the time the controller wrote) interpolates the outputs next <= o <= T-2 with t[o] < tnew_r, copies its new
// state into the output with t[o] == tnew_r (if any) and into output T-1 when the controller reports the final time.
// ODEPetsc._dense_step's classification, per row; a rejected or finished row (h_eff == 0) serves nothing.
// ------------------------------------------------------------------------------------------
#define PN_ROWS_DENSE_POW 4                     /* PN_DENSE_MAX_POW (include/pnode_amd.h) */

struct PnDensePlan {
  int lo, hi;        // outputs [lo, hi) are interpolated from this attempt
  int hit;           // the output that is a copy of the row's new state, or -1
  int next;          // the row's first output not yet served afterwards
};

PN_HD PnDensePlan pn_rows_dense_plan_row(const double *times, int nout, double h_eff, double tnew, int ctl_hit, int next) {
  PnDensePlan p;
  int o = next < 0 ? 0 : (next > nout ? nout : next);
  p.lo = p.hi = o;
  p.hit = -1;
  if (h_eff > 0.0) {
    while (o < nout - 1 && times[o] < tnew) ++o;
    p.hi = o;
    if (o < nout - 1 && times[o] == tnew) p.hit = o++;
    if (ctl_hit >= 0) {                          // the controller landed on t[T-1]: every output before it is served
      p.hit = nout - 1;
      o = nout;
    }
  }
  p.next = o;
  return p;
}

// h * beta(theta) of one stage, theta = (to - tn) / h, beta(theta) = sum_p P[p] theta^(p+1): ODEPetsc._dense_coefs' Horner
// form.  Inside one Horner step an add feeds a multiply, but the product of one step is an operand of the next step's add:
// contraction is switched off here, or the device (where hipcc fuses across statements) would round differently from the host.
PN_HD double pn_rows_dense_coef(const double *P, double to, double tn, double h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = to - tn;
  const double th = d / h;
  double v = 0.0;
  for (int p = PN_ROWS_DENSE_POW - 1; p >= 0; --p) {
    const double s = v + P[p];
    v = s * th;
  }
  return h * v;
}

// theta = (to - tn) / h of an interpolated output, as pn_rows_dense_coef forms it, and beta'(theta) = sum_p (p+1) P[p] theta^p of
// one stage (dL/dt of a per-sample solve): Horner from the highest power.  Contraction is off for the same
// reason as above: the host stand-in and the device must round alike.
PN_HD double pn_rows_dense_theta(double to, double tn, double h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = to - tn;
  return d / h;
}

PN_HD double pn_rows_dense_dcoef(const double *P, double th) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double v = 0.0;
  for (int p = PN_ROWS_DENSE_POW - 1; p >= 0; --p) {
    const double m = v * th;
    v = m + (double)(p + 1) * P[p];
  }
  return v;
}

// ------------------------------------------------------------------------------------------
// dL/dt of a per-sample solve: what one reversed round sends into row r's column of dtrow = doubles [nout][B] (pn_rows_tgrad_scatter
// on the device, pn_rows_tgrad_scatter_host on host arrays).  The output interval [t[is], t[ie]] a round belongs to: one interval
// [0, nout-1] with interpolated outputs (`dense`), else ie = the output the row last landed on in the reversed order (kept in iv[r])
// and is = ie - 1 (none for a single output time, whose start 0 does not move).  P = dL/dH of the interval's last step goes to
// dtrow[ie] and, negated, to dtrow[is]; Q = dL/dtau of every step to dtrow[is] (ODEPetsc._tg_finish's P_i - P_{i+1} + Q_{i+1}).
//   own stages:        Q += tbar_j, P += c_j tbar_j
//   first same as last: stage 0 was evaluated by the row's previous accepted step at tau + c_last H: its tbar_0 is HELD for the
//                       round that reverses that step (held[r]); the held scalar of the step after this one arrives here
//   interpolated o:     dtrow[o] += e_o, Q -= e_o, P -= theta_o e_o
// A round with h_eff = 0 sends nothing.  `flush` (after the last reversed round): the scalar still held belongs to the row's
// first step, evaluated at t[0] itself.
// ------------------------------------------------------------------------------------------
struct PnRowsTgScatter {
  double *dtrow;
  const double *rowacc;              // sum_j <w_j, K_j> of the round
  const double *tbar[7];             // PN_MAX_STAGES
  double c[7];
  int nt;
  const double *tbar0;               // null: stage 0 is an own stage (or func is autonomous)
  double c_last;
  int fsal;
  const double *heff, *trow;
  const int32_t *hit;
  const int32_t *range;              // [2][B], with interpolated outputs
  const double *erow;                // [nout][B]
  const double *times;
  double *held;
  int32_t *iv;
  int nout, dense, flush;
};

PN_HD void pn_rows_tgrad_scatter_row(const PnRowsTgScatter &a, int64_t B, int64_t r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (a.flush) {
    if (a.fsal && a.nout > 1) a.dtrow[r] += a.held[r];
    a.held[r] = 0.0;
    return;
  }
  const double h = a.heff[r];
  if (!(h > 0.0)) return;
  int hit = a.hit[r];
  if (hit >= a.nout) hit = -1;
  int ie, is;
  bool last;
  if (a.dense) {
    ie = a.nout - 1;
    is = 0;
    last = hit == ie;
  } else {
    last = hit >= 0;
    if (last) a.iv[r] = hit;
    ie = a.iv[r];
    is = ie - 1;
  }
  if (ie < 0 || ie >= a.nout) return;
  double q = 0.0, p = 0.0;
  // (a fixed trip count: indices into the argument block stay compile-time constants on the device)
#if defined(__clang__)
#pragma unroll
#endif
  for (int j = 0; j < 7; ++j) {
    if (j < a.nt) {
      const double tb = a.tbar[j][r];
      q += tb;
      p += a.c[j] * tb;
    }
  }
  if (a.fsal) {
    const double hd = a.held[r];
    q += hd;
    p += a.c_last * hd;
    a.held[r] = a.tbar0 ? a.tbar0[r] : 0.0;
  }
  p += a.rowacc[r] / h;
  if (a.dense && a.range) {
    int lo = a.range[r], hi = a.range[B + r];
    lo = lo < 0 ? 0 : lo;
    hi = hi > a.nout ? a.nout : hi;
    const double tr = a.trow[r];
    for (int o = lo; o < hi; ++o) {
      const double e = a.erow[(int64_t)o * B + r];
      a.dtrow[(int64_t)o * B + r] += e;
      q -= e;
      p -= pn_rows_dense_theta(a.times[o], tr, h) * e;
    }
  }
  if (is >= 0) a.dtrow[(int64_t)is * B + r] += q;
  if (last) {
    a.dtrow[(int64_t)ie * B + r] += p;
    if (is >= 0) a.dtrow[(int64_t)is * B + r] -= p;
  }
}

// ------------------------------------------------------------------------------------------
// -pn_rows_compact 1: which rows of a round have work to do, and the ordered list of them (pn_rows_list on the device,
// pn_rows_list_host on host arrays).  kind 0, the open rows: `src` is the int32 PN_ROWS_FINISHED row of si and a row is listed
// when its entry is 0.  kind 1, the stepped rows: `src` is the fp64 h_eff row of a round's log and a row is listed when its
// entry is > 0 (a NaN is not).  The list is the listed row numbers in ascending order: idx[0..m), -1 behind them up to B;
// pos[r] is row r's place in idx or -1; count[0] = m.  The device forms the same list from the same predicate, every row's
// place being the number of listed rows before it.
// ------------------------------------------------------------------------------------------
PN_HD bool pn_rows_listed(int kind, const void *src, int64_t r) {
  if (kind == 0) return static_cast<const int32_t *>(src)[r] == 0;
  return static_cast<const double *>(src)[r] > 0.0;
}

inline void pn_rows_list_rows(int kind, const void *src, int64_t B, int32_t *idx, int32_t *pos, int32_t *count) {
  int32_t m = 0;
  for (int64_t r = 0; r < B; ++r) {
    const bool on = pn_rows_listed(kind, src, r);
    pos[r] = on ? m : -1;
    if (on) idx[m++] = (int32_t)r;
  }
  for (int64_t k = m; k < B; ++k) idx[k] = -1;
  count[0] = m;
}

namespace pn {
// the controller constants of `ts` and what the row controllers need of its tableau (pn_ts.cpp)
void rows_ctl_config(const pn_ts *ts, int nspan, double max_time, PnRowsCtl *out);
// the argument block of one pn_rows_tgrad_scatter (device and host entry points alike, pn_ts.cpp); a non-null return is the
// refusal's text
const char *rows_tgrad_scatter_args(int64_t B, int nout, double *dtrow, const double *rowacc, int nt, const double *const *tbar,
                                    const double *coef, const double *tbar0, double c_last, int fsal, const double *log_d,
                                    const int32_t *log_hit, const int32_t *range, const double *erow, const double *times, double *held,
                                    int32_t *iv, int flush, PnRowsTgScatter *a);
}  // namespace pn
