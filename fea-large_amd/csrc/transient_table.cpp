// transient_table.cpp -- the coefficient table of a transient response by mode superposition (host only, no HIP).
//
// Every mode held obeys  q'' + d q' + lam q = p(t),  p = q_k g(t),  g given at t_n = n dt and linear in between, from rest.
// With y = (q, q') the step is exact:  y_{n+1} = A y_n + b0 p_n + b1 p_{n+1},  A = exp(dt [[0, 1], [-lam, -d]]).
//   g(t)   the solution of the homogeneous equation with g(0) = 0, g'(0) = 1 (the impulse response)
//   G1, G2 its first and second integrals from 0 (the responses to p = 1 and to p = t)
//   A  = [[1 - lam G1, g], [-lam g, g']]
//   b1 = (G2, G1) / dt,   b0 = (G1, g) - b1
// g, g', G1 and G2 are entire functions of dt whose derivatives at 0 obey c_{n+2} = -d c_{n+1} - lam c_n, c_0 = 0, c_1 = 1:
// they are summed as power series on a step h = dt / 2^s short enough that |lam| h^2 and d h are at most 1/2 -- nothing
// cancels there, whatever the sign of lam and whether the mode is under-, critically or over-damped, and lam = 0 is no
// special case -- and the step is then doubled s times:  A <- A A,  (G1, g) <- A (G1, g) + (G1, g),
// (G2, G1) <- A (G2, G1) + h (G1, g) + (G2, G1), the square of the propagator of (q, q', p, p') written out.  All of it
// and the recurrence run in long double; a table entry is rounded to double once, when it is written.
//   quantity 0  a_k(n) = q(t_n), or with the static correction q(t_n) - q_k g_n / lam_k (mode acceleration)
//   quantity 1  a_k(n) = q'(t_n)
//   quantity 2  a_k(n) = p(t_n) - d q'(t_n) - lam q(t_n)
#include "../../include/fea_hip.h"
#include <cmath>
#include <string>

struct TransientTable {
  int n_modes = 0, n_steps = 0, correction = 0, quantity = 0;
  int col[FEA_MODAL_MAX_LOCKED];
  long double lam[FEA_MODAL_MAX_LOCKED], d[FEA_MODAL_MAX_LOCKED], q[FEA_MODAL_MAX_LOCKED];
  long double A[FEA_MODAL_MAX_LOCKED][4], b0[FEA_MODAL_MAX_LOCKED][2], b1[FEA_MODAL_MAX_LOCKED][2];
  long double y[FEA_MODAL_MAX_LOCKED][2];
  int step = 0;                        // y is the state at t_step
};

static void propagator(long double lam, long double d, long double dt, long double *A, long double *b0, long double *b1)
{
  int s = 0;
  long double h = dt;
  while ((fabsl(lam) * h * h > 0.5L || d * h > 0.5L) && s < 4000) { h *= 0.5L; ++s; }
  // the series: term_n = c_n h^n / n!, and g = sum term_n, g' = sum term_{n+1} (n + 1) / h, G1 = sum term_n h / (n + 1),
  // G2 = sum term_n h^2 / ((n + 1) (n + 2))
  long double g = 0, dg = 0, G1 = 0, G2 = 0;
  long double c0 = 0, c1 = 1, pw = 1;  // c_n, c_{n+1}, h^n / n!
  for (int n = 0; n < 32; ++n) {
    const long double t = c0 * pw;
    g += t;
    G1 += t * h / (n + 1);
    G2 += t * h * h / ((long double)(n + 1) * (n + 2));
    dg += c1 * pw;
    const long double c2 = -d * c1 - lam * c0;
    c0 = c1; c1 = c2;
    pw *= h / (n + 1);
  }
  long double a[4] = {1 - lam * G1, g, -lam * g, dg};
  long double v1[2] = {G1, g}, v2[2] = {G2, G1};
  for (int k = 0; k < s; ++k) {
    const long double w1[2] = {a[0] * v1[0] + a[1] * v1[1] + v1[0], a[2] * v1[0] + a[3] * v1[1] + v1[1]};
    const long double w2[2] = {a[0] * v2[0] + a[1] * v2[1] + h * v1[0] + v2[0], a[2] * v2[0] + a[3] * v2[1] + h * v1[1] + v2[1]};
    const long double a2[4] = {a[0] * a[0] + a[1] * a[2], a[0] * a[1] + a[1] * a[3], a[2] * a[0] + a[3] * a[2], a[2] * a[1] + a[3] * a[3]};
    for (int e = 0; e < 4; ++e) a[e] = a2[e];
    v1[0] = w1[0]; v1[1] = w1[1]; v2[0] = w2[0]; v2[1] = w2[1];
    h *= 2;
  }
  for (int e = 0; e < 4; ++e) A[e] = a[e];
  b1[0] = v2[0] / dt; b1[1] = v2[1] / dt;
  b0[0] = v1[0] - b1[0]; b0[1] = v1[1] - b1[1];
}

// what both entries refuse, in one place
int transient_check(int n_modes, const double *lam, const double *q, int n_steps, double dt, const double *g, double alpha,
                    double beta, const double *zeta, int correction, int quantity, std::string *why)
{
  auto refuse = [&](const std::string &s) { if (why) *why = s; return FEAHIP_EINVAL; };
  if (n_modes < 1 || n_modes > FEA_MODAL_MAX_LOCKED) return refuse("the number of modes must be in [1, 64]");
  if (n_steps < 1 || n_steps > FEA_TRANSIENT_MAX_STEPS) return refuse("n_steps must be in [1, " + std::to_string(FEA_TRANSIENT_MAX_STEPS) + "]");
  if (!lam || !q || !g) return refuse("null argument");
  if (!(dt > 0.0) || !std::isfinite(dt)) return refuse("dt must be positive and finite");
  if (quantity < 0 || quantity > 2) return refuse("quantity must be 0 (displacement), 1 (velocity) or 2 (acceleration)");
  if (!(alpha >= 0.0) || !std::isfinite(alpha) || !(beta >= 0.0) || !std::isfinite(beta))
    return refuse("alpha and beta_k must be finite and not negative");
  for (int k = 0; k < n_modes; ++k) {
    const double z = zeta ? zeta[k] : 0.0;
    if (!(z >= 0.0) || !std::isfinite(z)) return refuse("zeta must be finite and not negative");
    if (!std::isfinite(lam[k]) || !std::isfinite(q[k])) return refuse("lam and q must be finite");
    if (correction && !(lam[k] > 0.0)) return refuse("the static correction needs lam_k > 0 for every mode");
  }
  for (int n = 0; n <= n_steps; ++n)
    if (!std::isfinite(g[n])) return refuse("g is not finite");
  return FEAHIP_OK;
}

// mode k of the arrays given goes to column order[k] (null: k) of a row
TransientTable *transient_begin(int n_modes, const double *lam, const double *q, const int *order, int n_steps, double dt,
                                double alpha, double beta, const double *zeta, int correction, int quantity)
{
  TransientTable *T = new TransientTable;
  T->n_modes = n_modes; T->n_steps = n_steps; T->correction = correction ? 1 : 0; T->quantity = quantity;
  for (int k = 0; k < n_modes; ++k) {
    const double z = zeta ? zeta[k] : 0.0;
    T->col[k] = order ? order[k] : k;
    T->lam[k] = lam[k];
    T->q[k] = q[k];
    T->d[k] = (long double)alpha + (long double)beta * lam[k] + 2.0L * z * sqrtl(lam[k] > 0.0 ? (long double)lam[k] : 0.0L);
    propagator(T->lam[k], T->d[k], dt, T->A[k], T->b0[k], T->b1[k]);
    T->y[k][0] = T->y[k][1] = 0;
  }
  return T;
}

void transient_end(TransientTable *T) { delete T; }

// the rows of the steps [T->step, T->step + count) into coef[count][64]; g is the whole history [n_steps + 1].
// FEAHIP_EINVAL and *why for an entry that is not finite
int transient_rows(TransientTable *T, const double *g, int count, double *coef, std::string *why)
{
  for (int r = 0; r < count; ++r) {
    const int n = T->step;
    double *row = coef + (size_t)r * FEA_MODAL_MAX_LOCKED;
    for (int e = 0; e < FEA_MODAL_MAX_LOCKED; ++e) row[e] = 0.0;
    const long double gn = g[n], gn1 = n < T->n_steps ? g[n + 1] : 0.0L;
    for (int k = 0; k < T->n_modes; ++k) {
      long double *y = T->y[k];
      const long double p = T->q[k] * gn;
      long double a;
      if (T->quantity == 0) a = T->correction ? y[0] - p / T->lam[k] : y[0];
      else if (T->quantity == 1) a = y[1];
      else a = p - T->d[k] * y[1] - T->lam[k] * y[0];
      const double out = fabsl(a) <= 1.7976931348623157e308L ? (double)a : HUGE_VAL;   // (NaN fails the comparison too)
      if (!std::isfinite(out)) {
        if (why) *why = "the coefficient of mode " + std::to_string(k + 1) + " at step " + std::to_string(n) + " is not finite";
        return FEAHIP_EINVAL;
      }
      row[T->col[k]] = out;
      if (n < T->n_steps) {
        const long double p1 = T->q[k] * gn1;
        const long double *A = T->A[k], *b0 = T->b0[k], *b1 = T->b1[k];
        const long double y0 = A[0] * y[0] + A[1] * y[1] + b0[0] * p + b1[0] * p1;
        const long double y1 = A[2] * y[0] + A[3] * y[1] + b0[1] * p + b1[1] * p1;
        y[0] = y0; y[1] = y1;
      }
    }
    ++T->step;
  }
  return FEAHIP_OK;
}
