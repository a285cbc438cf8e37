// crn_cfar.cpp — the per-bin CFAR detector's host side: setting and reading it on a handle, and the threshold factor alpha of each
// method for a wanted false-alarm probability.  (The entry points take their C linkage from include/crn_sense.h.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "crn_handle.h"
#include "crn_kernels.h"

static_assert((int)CRN_CFAR_CA == crn::CRN_CFAR_CA_K && (int)CRN_CFAR_GO == crn::CRN_CFAR_GO_K && (int)CRN_CFAR_SO == crn::CRN_CFAR_SO_K &&
              (int)CRN_CFAR_OS == crn::CRN_CFAR_OS_K, "crn_kernels.h mirrors crn_cfar_method");

namespace {
// Regularised incomplete beta I_x(a, b) by its continued fraction (modified Lentz), on the side where it converges fast.
double inc_beta(double a, double b, double x) {
  if (x <= 0.0) return 0.0;
  if (x >= 1.0) return 1.0;
  if (x > (a + 1.0) / (a + b + 2.0)) return 1.0 - inc_beta(b, a, 1.0 - x);
  const double ln_front = std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + a * std::log(x) + b * std::log1p(-x);
  const double tiny = 1e-300;
  double c = 1.0, d = 1.0 - (a + b) * x / (a + 1.0);
  d = std::fabs(d) < tiny ? tiny : d;
  d = 1.0 / d;
  double f = d;
  for (int m = 1; m <= 10000; m++) {
    for (int odd = 0; odd < 2; odd++) {
      const double num = odd ? -(a + m) * (a + b + m) * x / ((a + 2.0 * m) * (a + 2.0 * m + 1.0))
                             : m * (b - m) * x / ((a + 2.0 * m - 1.0) * (a + 2.0 * m));
      d = 1.0 + num * d;
      d = std::fabs(d) < tiny ? tiny : d;
      c = 1.0 + num / c;
      c = std::fabs(c) < tiny ? tiny : c;
      d = 1.0 / d;
      const double step = c * d;
      f *= step;
      if (odd && std::fabs(step - 1.0) < 1e-16) return std::exp(ln_front) * f / a;
    }
  }
  return std::exp(ln_front) * f / a;
}
// P(F(d1, d2) > alpha) = I_{d2 / (d2 + d1 alpha)}(d2 / 2, d1 / 2)
double f_tail(double alpha, double d1, double d2) { return inc_beta(0.5 * d2, 0.5 * d1, d2 / (d2 + d1 * alpha)); }

// The tail falls monotonically from 1 at alpha = 0: bracket, then bisect to the last bit.  False: no bracket below 1e300 (pfa too small).
template <class Tail>
bool solve_alpha(const Tail &tail, double pfa, double *alpha) {
  double lo = 0.0, hi = 1.0;
  while (tail(hi) > pfa) {
    lo = hi;
    hi *= 2.0;
    if (hi > 1e300) return false;
  }
  for (int i = 0; i < 2000 && hi - lo > 1e-16 * hi; i++) {
    const double mid = 0.5 * (lo + hi);
    if (mid <= lo || mid >= hi) break;
    (tail(mid) > pfa ? lo : hi) = mid;
  }
  *alpha = 0.5 * (lo + hi);
  return true;
}

// Regularised lower and upper incomplete gamma P(a, x), Q(a, x) = 1 - P, each evaluated on the side where it does not cancel:
// the power series for x < a + 1, the continued fraction (modified Lentz) beyond.  lga = lgamma(a).
void inc_gamma(double a, double x, double lga, double *P, double *Q) {
  if (x <= 0.0) {
    *P = 0.0;
    *Q = 1.0;
    return;
  }
  const double front = std::exp(a * std::log(x) - x - lga);
  if (x < a + 1.0) {
    double ap = a, del = 1.0 / a, sum = del;
    for (int n = 0; n < 100000 && std::fabs(del) > 1e-17 * std::fabs(sum); n++) {
      ap += 1.0;
      del *= x / ap;
      sum += del;
    }
    *P = sum * front;
    *Q = 1.0 - *P;
    return;
  }
  const double tiny = 1e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int i = 1; i < 100000; i++) {
    const double an = -i * (i - a);
    b += 2.0;
    d = an * d + b;
    d = std::fabs(d) < tiny ? tiny : d;
    c = b + an / c;
    c = std::fabs(c) < tiny ? tiny : c;
    d = 1.0 / d;
    const double step = d * c;
    h *= step;
    if (std::fabs(step - 1.0) < 1e-17) break;
  }
  *Q = front * h;
  *P = 1.0 - *Q;
}
}  // namespace

static int set_cfar_impl(crn_handle *h, const crn_cfar_params_ex *q, const char *fn) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  if (!q) {
    h->cfar_on = false;
    return CRN_OK;
  }
  const crn_cfg &c = h->cfg;
  char msg[160];
  auto bad = [&](int rc, const char *why) {
    std::snprintf(msg, sizeof msg, "%s: %s", fn, why);
    return crn::fail(rc, msg);
  };
  if (c.mode != CRN_MODE_ENERGY) return bad(CRN_ERR_ARG, "CFAR needs mode CRN_MODE_ENERGY");
  if (c.decide == CRN_DECIDE_ANN) return bad(CRN_ERR_STATE, "not on a DECIDE_ANN handle (THRESHOLD or NONE)");
  if (h->n_rings.load(std::memory_order_acquire) > 0)
    return bad(CRN_ERR_STATE, "an ingest ring is attached (CFAR with the ring is not supported yet)");
  if (q->method < CRN_CFAR_CA || q->method > CRN_CFAR_OS) return bad(CRN_ERR_ARG, "method must be CRN_CFAR_CA, _GO, _SO or _OS");
  if (q->train < 1 || q->train > 64) return bad(CRN_ERR_ARG, "train must be in 1..64");
  if (q->guard < 0) return bad(CRN_ERR_ARG, "guard < 0");
  if (2 * ((int64_t)q->guard + q->train) + 1 > c.fft_len) return bad(CRN_ERR_ARG, "2 (guard + train) + 1 > fft_len");
  if (!(q->alpha > 0.f) || !std::isfinite(q->alpha)) return bad(CRN_ERR_ARG, "alpha must be > 0 and finite");
  if (q->min_bins < 1) return bad(CRN_ERR_ARG, "min_bins < 1");
  if (q->method == CRN_CFAR_OS ? q->rank < 1 || q->rank > 2 * q->train : q->rank != 0)
    return bad(CRN_ERR_ARG, q->method == CRN_CFAR_OS ? "OS rank must be in 1..2 train" : "rank must be 0 unless the method is OS");
  if (q->reserved != 0) return bad(CRN_ERR_ARG, "reserved must be 0");
  h->cfar = *q;
  h->cfar_on = true;
  return CRN_OK;
}

int crn_sense_set_cfar_ex(crn_handle *h, const crn_cfar_params_ex *q) { return set_cfar_impl(h, q, "crn_sense_set_cfar_ex"); }

int crn_sense_set_cfar(crn_handle *h, const crn_cfar_params *q) {
  if (!q) return set_cfar_impl(h, nullptr, "crn_sense_set_cfar");
  crn_cfar_params_ex x{};
  x.method = CRN_CFAR_CA;
  x.guard = q->guard;
  x.train = q->train;
  x.min_bins = q->min_bins;
  x.rank = 0;
  x.reserved = q->reserved;
  x.alpha = q->alpha;
  return set_cfar_impl(h, &x, "crn_sense_set_cfar");
}

int crn_sense_get_cfar_ex(crn_handle *h, crn_cfar_params_ex *q, int32_t *on) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  if (q) *q = h->cfar;
  if (on) *on = h->cfar_on ? 1 : 0;
  return CRN_OK;
}

int crn_sense_get_cfar(crn_handle *h, crn_cfar_params *q, int32_t *on) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  if (q) {
    q->guard = h->cfar.guard;
    q->train = h->cfar.train;
    q->min_bins = h->cfar.min_bins;
    q->reserved = 0;
    q->alpha = h->cfar.alpha;
  }
  if (on) *on = h->cfar_on ? 1 : 0;
  return CRN_OK;
}

int crn_cfar_alpha(double pfa, int32_t frames_per_epoch, int32_t train, double *alpha) {
  if (!alpha) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha: null alpha");
  if (!(pfa > 0.0 && pfa < 1.0)) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha: pfa must be in (0, 1)");
  if (frames_per_epoch < 1) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha: frames_per_epoch < 1");
  if (train < 1 || train > 64) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha: train must be in 1..64");
  const double d1 = 2.0 * frames_per_epoch, d2 = 4.0 * train * frames_per_epoch;
  if (!solve_alpha([&](double al) { return f_tail(al, d1, d2); }, pfa, alpha)) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha: pfa too small");
  return CRN_OK;
}

int crn_cfar_alpha_ex(int32_t method, double pfa, int32_t frames_per_epoch, int32_t train, int32_t rank, double *alpha) {
  if (!alpha) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha_ex: null alpha");
  if (method < CRN_CFAR_CA || method > CRN_CFAR_OS) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha_ex: method must be CA, GO, SO or OS");
  if (!(pfa > 0.0 && pfa < 1.0)) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha_ex: pfa must be in (0, 1)");
  if (frames_per_epoch < 1) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha_ex: frames_per_epoch < 1");
  if (train < 1 || train > 64) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha_ex: train must be in 1..64");
  if (method == CRN_CFAR_OS ? rank < 1 || rank > 2 * train : rank != 0)
    return crn::fail(CRN_ERR_ARG, method == CRN_CFAR_OS ? "crn_cfar_alpha_ex: OS rank must be in 1..2 train"
                                                        : "crn_cfar_alpha_ex: rank must be 0 unless the method is OS");
  if (method == CRN_CFAR_CA) return crn_cfar_alpha(pfa, frames_per_epoch, train, alpha);
  // In units of the noise power, P and every training cell are Gamma(K), one side's sum is Gamma(WK).  A bin is detected when
  // P > c S, S the method's statistic: GO / SO the larger / smaller side sum with c = alpha / W, OS the rank-th smallest cell with
  // c = alpha.  So pfa(alpha) = E[Q(K, c S)] = int Q(K, c s) w(s) ds, w the density of S:
  //   GO 2 F_WK f_WK,  SO 2 (1 - F_WK) f_WK,  OS (2W)! / ((r-1)! (2W-r)!) F_K^(r-1) (1 - F_K)^(2W-r) f_K
  // (OS: the issue's Beta(u; r, 2W - r + 1) integral with u = F_K(s)).  The integral is taken on s = e^v, where w(s) s is a smooth
  // bump decaying at least exponentially on both sides; the trapezoid rule is then accurate far beyond double at the step below.
  const double K = frames_per_epoch, W = train, n = 2.0 * train;
  const bool os = method == CRN_CFAR_OS;
  const double a = os ? K : W * K;   // shape of the Gamma the statistic is built from
  const double lga = std::lgamma(a), lgk = std::lgamma(K);
  const double ln_comb = os ? std::lgamma(n + 1.0) - std::lgamma((double)rank) - std::lgamma(n - rank + 1.0) : std::log(2.0);
  // below s_lo the statistic has probability < e^-40 pfa (it is at least the smallest of 2W cells: P < 2W s^K / K!); above s_hi
  // the Gamma(a) tail is < e^-80
  const double v_lo = std::log(a) - 2.0 - (std::log(n) + 40.0 - std::log(pfa)) / K;
  const double v_hi = std::log(a + 20.0 * std::sqrt(a) + 100.0);
  const double h = std::min(0.05, 0.25 / std::sqrt(n * K));
  const int npts = (int)std::ceil((v_hi - v_lo) / h) + 1;
  std::vector<double> s(npts), w(npts);
  for (int i = 0; i < npts; i++) {
    const double v = v_lo + i * h, si = std::exp(v);
    double F, Fc;
    inc_gamma(a, si, lga, &F, &Fc);
    const double ln_f = a * v - si - lga;   // ln(f_a(s) s): the density times ds / dv
    double lw;
    if (method == CRN_CFAR_GO) lw = F > 0.0 ? ln_comb + std::log(F) + ln_f : -INFINITY;
    else if (method == CRN_CFAR_SO) lw = Fc > 0.0 ? ln_comb + std::log(Fc) + ln_f : -INFINITY;
    else lw = (rank > 1 && F <= 0.0) || (rank < n && Fc <= 0.0) ? -INFINITY
              : ln_comb + (rank - 1) * std::log(F) + (n - rank) * std::log(Fc) + ln_f;
    s[i] = si;
    w[i] = std::exp(lw) * h;
  }
  const double c_per_alpha = os ? 1.0 : 1.0 / W;
  auto tail = [&](double al) {
    double sum = 0.0;
    for (int i = 0; i < npts; i++) {
      if (w[i] == 0.0) continue;
      double P, Q;
      inc_gamma(K, al * c_per_alpha * s[i], lgk, &P, &Q);
      sum += w[i] * Q;
    }
    return sum;
  };
  if (!solve_alpha(tail, pfa, alpha)) return crn::fail(CRN_ERR_ARG, "crn_cfar_alpha_ex: pfa too small");
  return CRN_OK;
}

int crn_lad_factor(double pfa, int32_t frames_per_epoch, double t_cme, double *factor) {
  if (!factor) return crn::fail(CRN_ERR_ARG, "crn_lad_factor: null factor");
  if (!(pfa > 0.0 && pfa < 1.0)) return crn::fail(CRN_ERR_ARG, "crn_lad_factor: pfa must be in (0, 1)");
  if (frames_per_epoch < 1) return crn::fail(CRN_ERR_ARG, "crn_lad_factor: frames_per_epoch < 1");
  if (!std::isfinite(t_cme) || t_cme < 0.0) return crn::fail(CRN_ERR_ARG, "crn_lad_factor: t_cme must be finite and >= 0");
  // In units of the noise power P is Gamma(K) with mean 1: K P has the unit-scale Gamma(K) law, whose upper tail is Q(K, .)
  const double K = frames_per_epoch, lgk = std::lgamma(K), lgk1 = std::lgamma(K + 1.0);
  double q = 0.0;
  auto tail = [&](double s) {
    double P, Q;
    inc_gamma(K, s, lgk, &P, &Q);
    return Q;
  };
  if (!solve_alpha(tail, pfa, &q)) return crn::fail(CRN_ERR_ARG, "crn_lad_factor: pfa too small");
  double m = 1.0;
  if (t_cme > 0.0) {
    // the mean of the values FCME keeps, those below t_cme times that mean: E[P; P < c] / Pr(P < c) = P(K + 1, K c) / P(K, K c)
    for (int it = 0; it < 10000; it++) {
      double P1, Pk, Q;
      inc_gamma(K + 1.0, K * t_cme * m, lgk1, &P1, &Q);
      inc_gamma(K, K * t_cme * m, lgk, &Pk, &Q);
      const double next = P1 / Pk;
      if (!(next > 0.0) || !std::isfinite(next)) return crn::fail(CRN_ERR_ARG, "crn_lad_factor: t_cme too small: the excised mean vanishes");
      const bool still = std::fabs(next - m) <= 1e-16 * m;
      m = next;
      if (still) break;
    }
  }
  *factor = q / K / m;
  return CRN_OK;
}

int crn_cyclo_zmin(double pfa, int32_t frames, int32_t n_pairs, double *z_min) {
  if (!z_min) return crn::fail(CRN_ERR_ARG, "crn_cyclo_zmin: null z_min");
  if (!(pfa > 0.0 && pfa < 1.0)) return crn::fail(CRN_ERR_ARG, "crn_cyclo_zmin: pfa must be in (0, 1)");
  if (frames != 8 && frames != 16 && frames != 32 && frames != 64) return crn::fail(CRN_ERR_ARG, "crn_cyclo_zmin: frames must be 8, 16, 32 or 64");
  if (n_pairs < 1) return crn::fail(CRN_ERR_ARG, "crn_cyclo_zmin: n_pairs < 1");
  // sum of n Beta(1, F - 1): mean n / F, variance n (F - 1) / (F^2 (F + 1)); the Gamma law of that mean and variance has shape
  // g = n (F + 1) / (F - 1), and in its unit scale the sum is x = g + z sqrt(g)
  const double F = frames, g = n_pairs * (F + 1.0) / (F - 1.0), lg = std::lgamma(g);
  double x = 0.0;
  auto tail = [&](double s) {
    double P, Q;
    inc_gamma(g, s, lg, &P, &Q);
    return Q;
  };
  if (!solve_alpha(tail, pfa, &x)) return crn::fail(CRN_ERR_ARG, "crn_cyclo_zmin: pfa too small");
  *z_min = (x - g) / std::sqrt(g);
  return CRN_OK;
}
