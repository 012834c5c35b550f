// fatigue_table.cpp -- random-vibration fatigue on the host (no HIP), in long double: the constants of an S-N curve that
// k_fatigue_rates takes, and feahip_host_fatigue, the statistics of fatigue_point.h evaluated in long double and rounded to
// double once -- the reference of the device kernel at the device's own moments, and an entry for callers with moments
// of their own.
#include "../../include/fea_hip.h"
#include "fatigue_point.h"
#include <cmath>

static double to_double(long double v) { return fabsl(v) <= 1.7976931348623157e308L ? (double)v : (v != v ? NAN : (v > 0 ? HUGE_VAL : -HUGE_VAL)); }

// false for what the entries refuse of an S-N curve N s^b = A: b outside [1, 64], A not positive, either not finite
static bool sn_curve(double sn_b, double sn_a, FatigueConsts<long double> *k)
{
  if (!(sn_b >= 1.0) || !(sn_b <= 64.0) || !(sn_a > 0.0) || !std::isfinite(sn_a)) return false;
  const long double b = sn_b;
  k->b = b;
  k->inv_a = 1.0L / (long double)sn_a;
  k->gamma_b = tgammal(1.0L + b);
  k->gamma_hb = tgammal(1.0L + 0.5L * b);
  k->two_hb = powl(2.0L, 0.5L * b);
  return true;
}

// kernels_stress_fatigue.hip: the same constants rounded to double, k[5] = b, 1 / A, Gamma(1 + b), Gamma(1 + b / 2), 2^(b / 2)
int fatigue_constants(double sn_b, double sn_a, double *k)
{
  FatigueConsts<long double> c;
  if (!sn_curve(sn_b, sn_a, &c)) return FEAHIP_EINVAL;
  k[0] = sn_b; k[1] = to_double(c.inv_a); k[2] = to_double(c.gamma_b); k[3] = to_double(c.gamma_hb); k[4] = to_double(c.two_hb);
  return FEAHIP_OK;
}

extern "C" int feahip_host_fatigue(int n, const double *m, double sn_b, double sn_a, double *rates, double *damage, int *status)
{
  FatigueConsts<long double> k;
  if (n < 0 || (n > 0 && !m) || !sn_curve(sn_b, sn_a, &k)) return FEAHIP_EINVAL;
  for (size_t e = 0; e < (size_t)n * 4; ++e)
    if (!(m[e] >= 0.0) || !std::isfinite(m[e])) return FEAHIP_EINVAL;
  for (int i = 0; i < n; ++i) {
    const long double mi[4] = {m[4 * (size_t)i], m[4 * (size_t)i + 1], m[4 * (size_t)i + 2], m[4 * (size_t)i + 3]};
    long double r[2], d[3];
    const int st = fatigue_point<long double>(mi, k, r, d);
    if (rates) for (int e = 0; e < 2; ++e) rates[2 * (size_t)i + e] = to_double(r[e]);
    if (damage) for (int e = 0; e < 3; ++e) damage[3 * (size_t)i + e] = to_double(d[e]);
    if (status) status[i] = st;
  }
  return FEAHIP_OK;
}
