// combine_table.cpp -- the quadratic forms of a random-vibration and of a response-spectrum analysis on the modes held
// (host only, no HIP).  k_response_combine (kernels_combine.hip) evaluates on every dof
//   out_i^2 = x_i' C x_i + 2 u_s,i (b' x_i) + s u_s,i^2,     x_i the mode values of the dof;
// C[n][n], b[n] and s are made here, by ascending mode, accumulated in long double and rounded to double once.
//   random_form     a one-sided PSD S(w) of the load factor on the caller's grid, trapezoid weights wt_j:
//                     C_kl = sum_j wt_j S_j w_j^(2p) Re(a_k conj(a_l)),  b_k = sum_j wt_j S_j w_j^(2p) Re(a_k),
//                     s = sum_j wt_j S_j w_j^(2p),  a(w_j) the row of response_coefficients -- that very code, so out_i^2 is
//                   the trapezoid rule of S |(i w)^p u_i(w)|^2 over the fields feahip_response_field returns.
//                   b = 0 and s = 0 without the static correction
//   moment_form     the same form with the weight wt_j S_j w_j^n, n in {0, 1, 2, 4}: the spectral moment m_n of every linear
//                   combination of the response (the orders 0, 2, 4 are random_form at quantity 0, 1, 2, bit for bit)
//   random_grid     a grid that resolves every peak: a uniform background, and per damped mode the points
//                   w_k + (d_k / 2) tan(theta), theta uniform in (-pi / 2, pi / 2) -- the substitution that makes a
//                   Lorentzian of half width d_k / 2 flat
//   spectrum_form   peak modal displacements a_k = q_k sa_k / lam_k (times sqrt(lam_k), lam_k for the pseudo-velocity and
//                   -acceleration) combined by SRSS (C = diag a^2), CQC (C = rho_jk a_j a_k, Der Kiureghian's coefficient
//                   for unequal damping) or ABS (C = |a||a|', taken on |phi|); the missing mass enters as
//                   C += zpa^2 c c', b = zpa^2 c, s = zpa^2 with c_k = -q_k / lam_k: the rigid residual
//                   zpa (u_s + sum_k phi_k c_k), combined by SRSS
//   table_value     linear or log-log interpolation in a table of points
#include "../../include/fea_hip.h"
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

// kernels_response.hip: the coefficient rows of a sweep, coef[n_freq][2][64]
int response_coefficients(int n_modes, const double *lam, const double *q, const int *order, int n_freq, const double *omega,
                          double alpha, double beta, const double *zeta, int correction, double *coef, std::string *why);

#define ML FEA_MODAL_MAX_LOCKED

static double to_double(long double v) { return fabsl(v) <= 1.7976931348623157e308L ? (double)v : (v != v ? NAN : (v > 0 ? HUGE_VAL : -HUGE_VAL)); }

// the form with the weight wt_j S_j w_j^order: order 2 p is the quantity p of random_form, order 1 the first spectral
// moment.  w^order is taken as order / 2 factors w^2 and then one w for an odd order, so the even orders keep the bits
// random_form always gave
static int weighted_form(int n_modes, const double *lam, const double *q, int n_freq, const double *omega, const double *S, double alpha,
                         double beta, const double *zeta, int correction, int order, double *C, double *b, double *s, std::string *why)
{
  auto refuse = [&](const std::string &t) { if (why) *why = t; return FEAHIP_EINVAL; };
  if (n_modes < 1 || n_modes > ML) return refuse("the number of modes must be in [1, 64]");
  if (n_freq < 2 || n_freq > FEA_RANDOM_MAX_FREQ) return refuse("n_freq must be in [2, " + std::to_string(FEA_RANDOM_MAX_FREQ) + "]");
  if (!lam || !q || !omega || !S || !C || !b || !s) return refuse("null argument");
  for (int j = 0; j < n_freq; ++j) {
    if (!(omega[j] >= 0.0) || !std::isfinite(omega[j])) return refuse("omega must be finite and not negative");
    if (j > 0 && !(omega[j] > omega[j - 1])) return refuse("omega must be strictly ascending");
    if (!(S[j] >= 0.0) || !std::isfinite(S[j])) return refuse("S must be finite and not negative");
  }
  const int n = n_modes, CH = FEA_RESPONSE_MAX_FREQ;
  std::vector<long double> acc((size_t)n * n, 0.0L), bacc(n, 0.0L);
  long double sacc = 0.0L;
  std::vector<double> coef((size_t)std::min(CH, n_freq) * 2 * ML);
  for (int j0 = 0; j0 < n_freq; j0 += CH) {
    const int count = std::min(CH, n_freq - j0);
    const int rc = response_coefficients(n, lam, q, nullptr, count, omega + j0, alpha, beta, zeta, correction, coef.data(), why);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) {
      const int j = j0 + r;
      const long double lo = j > 0 ? omega[j - 1] : omega[0], hi = j + 1 < n_freq ? omega[j + 1] : omega[n_freq - 1];
      const long double w = omega[j];
      long double g = 0.5L * (hi - lo) * (long double)S[j];
      for (int e = 0; e < order / 2; ++e) g *= w * w;
      if (order & 1) g *= w;
      if (g == 0.0L) continue;
      const double *re = coef.data() + (size_t)r * 2 * ML, *im = re + ML;
      for (int k = 0; k < n; ++k) {
        const long double gr = g * re[k], gi = g * im[k];
        long double *row = acc.data() + (size_t)k * n;
        for (int l = k; l < n; ++l) row[l] += gr * re[l] + gi * im[l];
        bacc[k] += gr;
      }
      sacc += g;
    }
  }
  for (int k = 0; k < n; ++k) {
    for (int l = k; l < n; ++l) C[(size_t)k * n + l] = C[(size_t)l * n + k] = to_double(acc[(size_t)k * n + l]);
    b[k] = correction ? to_double(bacc[k]) : 0.0;
  }
  *s = correction ? to_double(sacc) : 0.0;
  for (int e = 0; e < n * n; ++e)
    if (!std::isfinite(C[e])) return refuse("the form is not finite");
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(b[k])) return refuse("the form is not finite");
  if (!std::isfinite(*s)) return refuse("the form is not finite");
  return FEAHIP_OK;
}

int random_form(int n_modes, const double *lam, const double *q, int n_freq, const double *omega, const double *S, double alpha,
                double beta, const double *zeta, int correction, int quantity, double *C, double *b, double *s, std::string *why)
{
  if (quantity < 0 || quantity > 2) {
    if (why) *why = "quantity must be 0 (displacement), 1 (velocity) or 2 (acceleration)";
    return FEAHIP_EINVAL;
  }
  return weighted_form(n_modes, lam, q, n_freq, omega, S, alpha, beta, zeta, correction, 2 * quantity, C, b, s, why);
}

int moment_form(int n_modes, const double *lam, const double *q, int n_freq, const double *omega, const double *S, double alpha,
                double beta, const double *zeta, int correction, int order, double *C, double *b, double *s, std::string *why)
{
  if (order != 0 && order != 1 && order != 2 && order != 4) {
    if (why) *why = "the order of a spectral moment must be 0, 1, 2 or 4";
    return FEAHIP_EINVAL;
  }
  return weighted_form(n_modes, lam, q, n_freq, omega, S, alpha, beta, zeta, correction, order, C, b, s, why);
}

// d_k in long double, as transient_table.cpp takes it; FEAHIP_EINVAL for what the sweep refuses of the damping
static int damping_of(int n_modes, const double *lam, double alpha, double beta, const double *zeta, long double *d, std::string *why)
{
  auto refuse = [&](const std::string &t) { if (why) *why = t; return FEAHIP_EINVAL; };
  if (!(alpha >= 0.0) || !std::isfinite(alpha) || !(beta >= 0.0) || !std::isfinite(beta))
    return refuse("alpha and beta_k must be finite and not negative");
  for (int k = 0; k < n_modes; ++k) {
    const double z = zeta ? zeta[k] : 0.0;
    if (!(z >= 0.0) || !std::isfinite(z)) return refuse("zeta must be finite and not negative");
    if (!std::isfinite(lam[k])) return refuse("lam must be finite");
    d[k] = (long double)alpha + (long double)beta * lam[k] + 2.0L * z * sqrtl(lam[k] > 0.0 ? (long double)lam[k] : 0.0L);
  }
  return FEAHIP_OK;
}

// the peak modal values a[n] as well (null: not wanted)
int spectrum_form(int n_modes, const double *lam, const double *q, const double *sa, double alpha, double beta, const double *zeta,
                  int rule, int correction, double zpa, int quantity, double *C, double *b, double *s, double *a_out, std::string *why)
{
  auto refuse = [&](const std::string &t) { if (why) *why = t; return FEAHIP_EINVAL; };
  if (n_modes < 1 || n_modes > ML) return refuse("the number of modes must be in [1, 64]");
  if (!lam || !q || !sa || !C || !b || !s) return refuse("null argument");
  if (rule < FEAHIP_SRSS || rule > FEAHIP_ABS) return refuse("rule must be 0 (SRSS), 1 (CQC) or 2 (ABS)");
  if (quantity < 0 || quantity > 2) return refuse("quantity must be 0 (displacement), 1 (pseudo-velocity) or 2 (pseudo-acceleration)");
  if (!(zpa >= 0.0) || !std::isfinite(zpa)) return refuse("zpa must be finite and not negative");
  if (zpa != 0.0 && quantity != 0) return refuse("the missing mass (zpa) belongs to the displacement alone");
  if (zpa != 0.0 && !correction) return refuse("the missing mass (zpa) needs the static correction");
  if (zpa != 0.0 && rule == FEAHIP_ABS) return refuse("the missing mass (zpa) needs the signed mode values: not with ABS");
  const int n = n_modes;
  long double d[ML], a[ML], w[ML], z[ML];
  const int rc = damping_of(n, lam, alpha, beta, zeta, d, why);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) {
    if (!(lam[k] > 0.0)) return refuse("a response spectrum needs lam_k > 0 for every mode");
    if (!std::isfinite(q[k])) return refuse("q must be finite");
    if (!(sa[k] >= 0.0) || !std::isfinite(sa[k])) return refuse("sa must be finite and not negative");
    w[k] = sqrtl((long double)lam[k]);
    z[k] = d[k] / (2.0L * w[k]);
    a[k] = (long double)q[k] * sa[k] / lam[k];
    if (quantity == 1) a[k] *= w[k];
    if (quantity == 2) a[k] *= lam[k];
    if (a_out) a_out[k] = to_double(a[k]);
  }
  const long double z2 = (long double)zpa * zpa;
  for (int j = 0; j < n; ++j)
    for (int k = j; k < n; ++k) {
      long double v;
      if (rule == FEAHIP_ABS) v = fabsl(a[j]) * fabsl(a[k]);
      else if (j == k) v = a[j] * a[j];                                // rho_kk = 1 exactly
      else if (rule == FEAHIP_SRSS) v = 0.0L;
      else {
        const long double r = w[k] / w[j], zz = z[j] * z[k], r2 = r * r;
        const long double num = 8.0L * sqrtl(zz) * (z[j] + r * z[k]) * r * sqrtl(r);
        const long double den = (1.0L - r2) * (1.0L - r2) + 4.0L * zz * r * (1.0L + r2) + 4.0L * (z[j] * z[j] + z[k] * z[k]) * r2;
        const long double rho = den == 0.0L ? 1.0L : num / den;        // (equal undamped frequencies)
        v = rho * a[j] * a[k];
      }
      if (zpa != 0.0) v += z2 * ((long double)q[j] / lam[j]) * ((long double)q[k] / lam[k]);
      C[(size_t)j * n + k] = C[(size_t)k * n + j] = to_double(v);
    }
  for (int k = 0; k < n; ++k) b[k] = zpa != 0.0 ? to_double(-z2 * ((long double)q[k] / lam[k])) : 0.0;
  *s = zpa != 0.0 ? to_double(z2) : 0.0;
  for (int e = 0; e < n * n; ++e)
    if (!std::isfinite(C[e])) return refuse("the form is not finite");
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(b[k])) return refuse("the form is not finite");
  return FEAHIP_OK;
}

// the value at x of the table (w[n], v[n]), w strictly ascending: the point's own value at a point, linear or log-log in
// between (a segment with a value or an abscissa that is not positive is linear), `outside` 0: zero outside the table,
// 1: the end values.  NaN for a table that is no table
static double table_value(int n, const double *w, const double *v, int loglog, double x, int outside)
{
  if (n < 1 || !w || !v || !std::isfinite(x)) return NAN;
  for (int j = 0; j < n; ++j)
    if (!std::isfinite(w[j]) || !std::isfinite(v[j]) || (j > 0 && !(w[j] > w[j - 1]))) return NAN;
  if (x < w[0]) return outside ? v[0] : 0.0;
  if (x > w[n - 1]) return outside ? v[n - 1] : 0.0;
  const int hi = (int)(std::lower_bound(w, w + n, x) - w);               // w[hi - 1] < x <= w[hi]
  if (w[hi] == x) return v[hi];
  const int lo = hi - 1;
  if (loglog && w[lo] > 0.0 && v[lo] > 0.0 && v[hi] > 0.0) {
    const long double t = (logl((long double)x) - logl((long double)w[lo])) / (logl((long double)w[hi]) - logl((long double)w[lo]));
    return (double)expl(logl((long double)v[lo]) + t * (logl((long double)v[hi]) - logl((long double)v[lo])));
  }
  const long double t = ((long double)x - w[lo]) / ((long double)w[hi] - w[lo]);
  return (double)(v[lo] + t * ((long double)v[hi] - v[lo]));
}

extern "C" double feahip_host_psd_value(int n_pts, const double *w, const double *S, int loglog, double at)
{
  return table_value(n_pts, w, S, loglog, at, 0);
}

extern "C" double feahip_host_spectrum_value(int n_pts, const double *w, const double *sa, int loglog, double at)
{
  return table_value(n_pts, w, sa, loglog, at, 1);
}

extern "C" int feahip_host_random_form(int n_modes, const double *lam, const double *q, int n_freq, const double *omega,
                                       const double *S, double alpha, double beta_k, const double *zeta, int static_correction,
                                       int quantity, double *C, double *b, double *s)
{
  return random_form(n_modes, lam, q, n_freq, omega, S, alpha, beta_k, zeta, static_correction, quantity, C, b, s, nullptr);
}

extern "C" int feahip_host_moment_form(int n_modes, const double *lam, const double *q, int n_freq, const double *omega,
                                       const double *S, double alpha, double beta_k, const double *zeta, int static_correction,
                                       int order, double *C, double *b, double *s)
{
  return moment_form(n_modes, lam, q, n_freq, omega, S, alpha, beta_k, zeta, static_correction, order, C, b, s, nullptr);
}

extern "C" int feahip_host_spectrum_form(int n_modes, const double *lam, const double *q, const double *sa, double alpha,
                                         double beta_k, const double *zeta, int rule, int static_correction, double zpa,
                                         int quantity, double *C, double *b, double *s)
{
  return spectrum_form(n_modes, lam, q, sa, alpha, beta_k, zeta, rule, static_correction, zpa, quantity, C, b, s, nullptr, nullptr);
}

extern "C" int feahip_host_random_grid(int n_modes, const double *lam, double alpha, double beta_k, const double *zeta, double w_lo,
                                       double w_hi, int n_background, int n_per_mode, double *omega_out, int *n_out)
{
  if (!n_out || n_modes < 0 || n_modes > ML || (n_modes > 0 && !lam)) return FEAHIP_EINVAL;
  if (!(w_lo >= 0.0) || !(w_hi > w_lo) || !std::isfinite(w_hi)) return FEAHIP_EINVAL;
  if (n_background < 2 || n_per_mode < 0) return FEAHIP_EINVAL;
  const int n_break = omega_out ? *n_out : 0;
  if (n_break < 0) return FEAHIP_EINVAL;
  long double d[ML];
  if (damping_of(n_modes, lam, alpha, beta_k, zeta, d, nullptr)) return FEAHIP_EINVAL;
  std::vector<double> g;
  g.reserve((size_t)n_background + (size_t)n_modes * n_per_mode + n_break);
  for (int i = 0; i < n_break; ++i) {
    if (!std::isfinite(omega_out[i])) return FEAHIP_EINVAL;
    g.push_back(omega_out[i]);
  }
  for (int i = 0; i < n_background; ++i)
    g.push_back(i == n_background - 1 ? w_hi : (double)((long double)w_lo + ((long double)w_hi - w_lo) * i / (n_background - 1)));
  const long double pi = 4.0L * atanl(1.0L);
  for (int k = 0; k < n_modes; ++k) {
    if (!(lam[k] > 0.0) || !(d[k] > 0.0L)) continue;
    const long double wk = sqrtl((long double)lam[k]);
    for (int i = 0; i < n_per_mode; ++i) {
      const long double theta = ((i + 0.5L) / n_per_mode) * pi - pi / 2.0L;
      g.push_back((double)(wk + 0.5L * d[k] * tanl(theta)));
    }
  }
  g.erase(std::remove_if(g.begin(), g.end(), [&](double v) { return !(v >= w_lo && v <= w_hi); }), g.end());
  std::sort(g.begin(), g.end());
  g.erase(std::unique(g.begin(), g.end()), g.end());
  if (g.size() > (size_t)FEA_RANDOM_MAX_FREQ) return FEAHIP_EINVAL;
  if (omega_out) std::copy(g.begin(), g.end(), omega_out);
  *n_out = (int)g.size();
  return FEAHIP_OK;
}
