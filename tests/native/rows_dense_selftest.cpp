// Stand-alone driver for the sanitizers (tests/test_sample_dense_sanitize.py): the per-row text of pn_adapt.h -- the
// controller of one row and the plan / coefficients of its interpolated outputs -- on heap arrays of exactly the sizes
// the entry points document, so that an index past a row, a counter or the output times is an error here.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pn_adapt.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
  const int T = 9;
  const int64_t B = 5;
  std::vector<double> times(T);
  for (int o = 0; o < T; ++o) times[o] = 0.125 * o;
  // --- plan: hand-made rows (empty, one, many, exact landing, h = 0, final) and counters at and beyond their ends
  struct Row { double t, h, tnew; int ctl, next, lo, hi, hit, after; };
  const Row rows[] = {
      {0.13, 0.05, 0.18, -1, 2, 2, 2, -1, 2},        {0.13, 0.2, 0.33, -1, 2, 2, 3, -1, 3},
      {0.01, 0.9, 0.91, -1, 1, 1, 8, -1, 8},         {0.13, 0.245, 0.375, -1, 2, 2, 3, 3, 4},
      {0.3, 0.0, 0.3, -1, 3, 3, 3, -1, 3},           {0.9, 0.1, 1.0, 1, 8, 8, 8, 8, 9},
      {0.6, 0.4, 1.0, 1, 5, 5, 8, 8, 9},             {1.0, 0.0, 1.0, -1, 9, 9, 9, -1, 9},
      {0.5, 0.1, 0.6, -1, -3, 0, 5, -1, 5},          {0.5, 0.1, 0.6, -1, 99, 9, 9, -1, 9},
  };
  for (const Row &r : rows) {
    const PnDensePlan p = pn_rows_dense_plan_row(times.data(), T, r.h, r.tnew, r.ctl, r.next);
    EXPECT(p.lo == r.lo && p.hi == r.hi && p.hit == r.hit && p.next == r.after);
    EXPECT(p.lo >= 0 && (p.hi <= T - 1 || p.hi == p.lo) && p.hit < T && p.next <= T);      // a finished row's range is empty
  }
  // --- coefficients: beta(1) = sum of the row, beta(0) = 0, Horner against the plain powers
  std::vector<double> P = {1.0, -1.5, 0.75, -0.125};
  EXPECT(pn_rows_dense_coef(P.data(), 0.25, 0.25, 0.5) == 0.0);
  EXPECT(std::fabs(pn_rows_dense_coef(P.data(), 0.75, 0.25, 0.5) - 0.5 * 0.125) < 1e-16);
  const double th = 0.3 / 0.5;
  double plain = 0;
  for (int p = 0; p < PN_ROWS_DENSE_POW; ++p) plain += P[p] * std::pow(th, p + 1);
  EXPECT(std::fabs(pn_rows_dense_coef(P.data(), 0.55, 0.25, 0.5) - 0.5 * plain) < 1e-15);
  // --- the controller of B rows over [0, 1] with the end points as its span, and the plan after every round
  PnRowsCtl rc = {};
  rc.cfg.safety = 0.9; rc.cfg.reject_safety = 0.5; rc.cfg.clip_lo = 0.1; rc.cfg.clip_hi = 10.0;
  rc.cfg.dt_min = 1e-20; rc.cfg.dt_max = 1e50; rc.cfg.match_stretch = 0.01; rc.cfg.match_halve = 1.5;
  rc.cfg.span_reltol = 1e-10; rc.cfg.span_abstol = 1e-10; rc.cfg.max_time = 1.0; rc.cfg.max_steps = 1000;
  rc.cfg.max_reject = 10; rc.cfg.order = 5; rc.cfg.nspan = 2;
  rc.fsal = 1; rc.c_last = 1.0;
  const std::vector<double> span = {0.0, 1.0};
  std::vector<double> sd(PN_ROWS_ND * B), enorm(B), log_d(3 * B);
  std::vector<int32_t> si(PN_ROWS_NI * B, 0), log_hit(B), accept(B), next(B, 1), range(2 * B);
  for (int64_t r = 0; r < B; ++r) {
    sd[PN_ROWS_T * B + r] = 0.0; sd[PN_ROWS_H * B + r] = 0.01 * (r + 1); sd[PN_ROWS_TFIRST * B + r] = 0.0; sd[PN_ROWS_CACHED * B + r] = 0.0;
    si[PN_ROWS_SPANCTR * B + r] = 1;
  }
  std::vector<int> served(T * B, 0);
  int open = (int)B, rounds = 0;
  while (open > 0 && rounds < 500) {
    for (int64_t r = 0; r < B; ++r) enorm[r] = ((rounds + r) % 4 == 3) ? 2.5 : 0.02 * (r + 1);      // every fourth attempt is rejected
    open = 0;
    for (int64_t r = 0; r < B; ++r) open += pn_rows_judge_row(rc, span.data(), B, r, enorm.data(), sd.data(), si.data(), log_d.data(), log_hit.data(), accept.data());
    for (int64_t r = 0; r < B; ++r) {
      const PnDensePlan p = pn_rows_dense_plan_row(times.data(), T, log_d[r], sd[PN_ROWS_T * B + r], log_hit[r], next[r]);
      next[r] = p.next; range[r] = p.lo; range[B + r] = p.hi; log_hit[r] = p.hit;
      for (int o = p.lo; o < p.hi; ++o) {
        ++served[o * B + r];
        const double c = pn_rows_dense_coef(P.data(), times[o], log_d[B + r], log_d[r]);
        EXPECT(std::isfinite(c));
      }
      if (p.hit >= 0) ++served[p.hit * B + r];
      if (!accept[r]) EXPECT(p.lo == p.hi && p.hit < 0);
    }
    ++rounds;
  }
  EXPECT(open == 0);
  for (int64_t r = 0; r < B; ++r) {
    EXPECT(next[r] == T);
    for (int o = 1; o < T; ++o) EXPECT(served[o * B + r] == 1);        // every output once, by exactly one round
    EXPECT(served[r] == 0);
  }
  if (fails == 0) std::printf("rows dense selftest ok (%d rounds)\n", rounds);
  return fails ? 1 : 0;
}
