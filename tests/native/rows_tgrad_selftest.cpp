// Stand-alone driver for the sanitizers (tests/test_sample_time_grads_sanitize.py): the host entry points behind dL/dt of a
// per-sample solve -- theta and beta' of a row's interpolated outputs (pn_rows_dense_tgrad_host) and the per-row scatter of a
// reversed round (pn_rows_tgrad_scatter_host) -- on heap arrays of exactly the sizes the header documents, so that an index
// past a row, a range or the output times is an error here.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pnode_amd.h"
#include "pn_adapt.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static bool close(double a, double b, double tol) { return std::fabs(a - b) <= tol * (1.0 + std::fabs(b)); }

int main() {
  const int T = 9, nk = 2;
  const int64_t B = 4;
  std::vector<double> times(T);
  for (int o = 0; o < T; ++o) times[o] = 0.125 * o;
  // two stages of a made-up extension: beta_j(theta) = sum_p P[j][p] theta^(p+1)
  const std::vector<double> P = {1.0, -1.5, 0.75, -0.125, 0.0, 2.0, -1.0, 0.25};
  // --- beta' against a central difference of the existing beta (h = 1, t_n = 0: pn_rows_dense_coef is beta itself), and at the
  // edges of the range: beta'(0) = P[0], beta'(1) = sum_p (p + 1) P[p]
  for (int j = 0; j < nk; ++j) {
    const double *Pj = P.data() + j * PN_DENSE_MAX_POW;
    const double thetas[] = {0.0, 0.1, 0.37, 0.5, 0.93, 1.0};
    for (double th : thetas) {
      const double e = 1e-5;
      const double fd = (pn_rows_dense_coef(Pj, th + e, 0.0, 1.0) - pn_rows_dense_coef(Pj, th - e, 0.0, 1.0)) / (2 * e);
      EXPECT(close(pn_rows_dense_dcoef(Pj, th), fd, 1e-9));       // the difference's own error: e^2 |beta'''| / 6 ~ 1e-10
    }
    double at_one = 0;
    for (int p = 0; p < PN_DENSE_MAX_POW; ++p) at_one += (p + 1) * Pj[p];
    EXPECT(pn_rows_dense_dcoef(Pj, 0.0) == Pj[0]);
    EXPECT(close(pn_rows_dense_dcoef(Pj, 1.0), at_one, 1e-15));
  }
  EXPECT(pn_rows_dense_theta(0.25, 0.25, 0.5) == 0.0 && pn_rows_dense_theta(0.75, 0.25, 0.5) == 1.0);
  // --- the entry point: rows with an empty range, one output, every interior output, h = 0, and ranges clamped to [0, T)
  std::vector<double> log_d(3 * B, 0.0), theta(T * B, -7.0), dcoef(T * B * nk, -7.0);
  std::vector<int32_t> range(2 * B);
  const double hs[] = {0.05, 0.2, 0.95, 0.0}, ts[] = {0.13, 0.13, 0.01, 0.3};
  const int los[] = {2, 2, -3, 3}, his[] = {2, 3, 99, 5};
  for (int64_t r = 0; r < B; ++r) {
    log_d[r] = hs[r];
    log_d[B + r] = ts[r];
    range[r] = los[r];
    range[B + r] = his[r];
  }
  EXPECT(pn_rows_dense_tgrad_host(B, T, times.data(), log_d.data(), range.data(), nk, P.data(), theta.data(), dcoef.data()) == 0);
  for (int64_t r = 0; r < B; ++r) {
    const int lo = los[r] < 0 ? 0 : los[r], hi = hs[r] > 0 ? (his[r] > T ? T : his[r]) : lo;
    for (int o = 0; o < T; ++o) {
      const bool in = o >= lo && o < hi;
      EXPECT(in ? theta[o * B + r] == (times[o] - ts[r]) / hs[r] : theta[o * B + r] == -7.0);
      for (int j = 0; j < nk; ++j)
        EXPECT(in ? dcoef[(o * B + r) * nk + j] == pn_rows_dense_dcoef(P.data() + j * PN_DENSE_MAX_POW, theta[o * B + r])
                  : dcoef[(o * B + r) * nk + j] == -7.0);
    }
  }
  EXPECT(pn_rows_dense_tgrad_host(B, 1, times.data(), log_d.data(), range.data(), nk, P.data(), theta.data(), dcoef.data()) != 0);
  EXPECT(pn_rows_dense_tgrad_host(B, T, times.data(), log_d.data(), range.data(), nk, P.data(), nullptr, dcoef.data()) != 0);
  // --- the scatter, match mode, first same as last: row 0 reverses the last step of interval 2, then the step that is both
  // the first of the solve and the last of interval 1; the other rows ride along with h_eff = 0 and are not touched
  {
    const int nout = 3;
    std::vector<double> dtrow(nout * B, 0.0), rowacc(B), tb0(B), tb1(B), held(B, 0.0), lg(3 * B, 0.0);
    std::vector<int32_t> hit(B), iv(B, nout - 1);
    const double *tbar[] = {tb1.data()};
    const double c1[] = {0.5};
    const double c_last = 1.0;
    // round 2 (reversed first): row 0 lands on output 2 with h = 0.25; rows 1..3 have h_eff = 0
    lg[0] = 0.25; rowacc[0] = 2.0; tb0[0] = 0.3; tb1[0] = 0.7; hit[0] = 2;
    for (int64_t r = 1; r < B; ++r) { lg[r] = 0.0; rowacc[r] = 99.0; tb0[r] = 99.0; tb1[r] = 99.0; hit[r] = -1; }
    EXPECT(pn_rows_tgrad_scatter_host(B, nout, dtrow.data(), rowacc.data(), 1, tbar, c1, tb0.data(), c_last, 1, lg.data(), hit.data(),
                                      nullptr, nullptr, nullptr, held.data(), iv.data(), 0) == 0);
    // P = 2/0.25 + 0.5*0.7 = 8.35 to t_2 and off t_1; Q = 0.7 to t_1; 0.3 is held
    EXPECT(close(dtrow[2 * B], 8.35, 1e-15) && close(dtrow[1 * B], 0.7 - 8.35, 1e-15) && dtrow[0] == 0.0 && held[0] == 0.3);
    for (int64_t r = 1; r < B; ++r) EXPECT(dtrow[2 * B + r] == 0.0 && dtrow[B + r] == 0.0 && held[r] == 0.0 && iv[r] == nout - 1);
    // round 1: row 0 lands on output 1 with h = 0.5: the held 0.3 belongs to this step (tau and, it being last, c_last H)
    lg[0] = 0.5; rowacc[0] = 1.0; tb0[0] = 0.2; tb1[0] = 0.1; hit[0] = 1;
    EXPECT(pn_rows_tgrad_scatter_host(B, nout, dtrow.data(), rowacc.data(), 1, tbar, c1, tb0.data(), c_last, 1, lg.data(), hit.data(),
                                      nullptr, nullptr, nullptr, held.data(), iv.data(), 0) == 0);
    const double p1 = 1.0 / 0.5 + 0.5 * 0.1 + 1.0 * 0.3, q1 = 0.1 + 0.3;
    EXPECT(close(dtrow[1 * B], 0.7 - 8.35 + p1, 1e-15) && close(dtrow[0], q1 - p1, 1e-15) && held[0] == 0.2 && iv[0] == 1);
    // the flush: the first step's stage 0 was evaluated at t[0]
    EXPECT(pn_rows_tgrad_scatter_host(B, nout, dtrow.data(), nullptr, 0, nullptr, nullptr, nullptr, 0.0, 1, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, held.data(), iv.data(), 1) == 0);
    EXPECT(close(dtrow[0], q1 - p1 + 0.2, 1e-15) && held[0] == 0.0);
    // refusals: a range without the outputs' sums, more vectors than stages
    EXPECT(pn_rows_tgrad_scatter_host(B, nout, dtrow.data(), rowacc.data(), 1, tbar, c1, nullptr, c_last, 1, lg.data(), hit.data(),
                                      range.data(), nullptr, nullptr, held.data(), iv.data(), 0) != 0);
    EXPECT(pn_rows_tgrad_scatter_host(B, nout, dtrow.data(), rowacc.data(), 8, tbar, c1, nullptr, c_last, 1, lg.data(), hit.data(),
                                      nullptr, nullptr, nullptr, held.data(), iv.data(), 0) != 0);
  }
  // --- the scatter with interpolated outputs: one interval, the final step with two outputs inside it; a range that
  // overshoots is clamped to the output times
  {
    std::vector<double> dtrow(T * B, 0.0), rowacc(B, 0.0), held(B, 0.0), lg(3 * B, 0.0), erow(T * B, 0.0);
    std::vector<int32_t> hit(B, -1), iv(B, T - 1), rg(2 * B, 0);
    lg[0] = 0.4; lg[B] = 0.6; rowacc[0] = 0.8; hit[0] = T - 1; rg[0] = 5; rg[B] = 7;
    erow[5 * B] = 0.5; erow[6 * B] = -0.25;
    lg[1] = 0.5; lg[B + 1] = 0.1; hit[1] = -1; rg[1] = -2; rg[B + 1] = 40;
    for (int o = 0; o < T; ++o) erow[o * B + 1] = 1.0;
    EXPECT(pn_rows_tgrad_scatter_host(B, T, dtrow.data(), rowacc.data(), 0, nullptr, nullptr, nullptr, 1.0, 0, lg.data(), hit.data(),
                                      rg.data(), erow.data(), times.data(), held.data(), iv.data(), 0) == 0);
    const double th5 = (times[5] - 0.6) / 0.4, th6 = (times[6] - 0.6) / 0.4;
    const double p = 0.8 / 0.4 - th5 * 0.5 + th6 * 0.25, q = -0.5 + 0.25;
    EXPECT(dtrow[5 * B] == 0.5 && dtrow[6 * B] == -0.25);
    EXPECT(close(dtrow[(T - 1) * B], p, 1e-15) && close(dtrow[0], q - p, 1e-15));
    EXPECT(close(dtrow[1], -(double)T + 1.0, 1e-15) && dtrow[(T - 1) * B + 1] == 1.0);       // row 1: not the last step, nothing to t_N but e
  }
  if (fails == 0) std::printf("rows tgrad selftest ok\n");
  return fails ? 1 : 0;
}
