// fatigue_point.h -- the statistics of ONE stationary Gaussian stress process from its spectral moments m0, m1, m2, m4
// (m_n = integral of w^n G(w) dw, w in rad per unit time, G one-sided): the rates of zero up-crossings and of peaks, and
// the damage per unit time on the S-N curve N s^b = A (s the stress AMPLITUDE) by the narrow-band formula, by Dirlik's
// density and by Tovo and Benasciutti's interpolation.  One copy of the arithmetic: k_fatigue_rates
// (kernels_stress_fatigue.hip) runs it in double on the device, feahip_host_fatigue (fatigue_table.cpp) in long double on
// the host -- the reference the device is held to.
//   nu0 = sqrt(m2 / m0) / 2 pi,  nup = sqrt(m4 / m2) / 2 pi          (0 where a moment under the root is 0)
//   alpha1 = m1 / sqrt(m0 m2),   alpha2 = m2 / sqrt(m0 m4)           clamped to [0, 1]
//   D_NB = (nu0 / A) (2 m0)^(b/2) Gamma(1 + b/2)
//   D_TB = [bw + (1 - bw) alpha2^(b - 1)] D_NB,
//          bw = (alpha1 - alpha2) [1.112 (1 + alpha1 alpha2 - alpha1 - alpha2) exp(2.11 alpha2) + alpha1 - alpha2] / (alpha2 - 1)^2
//   D_DK = (nup / A) m0^(b/2) [D1 Q^b Gamma(1 + b) + 2^(b/2) Gamma(1 + b/2) (D2 |R|^b + D3)]   with Dirlik's D1, D2, D3, R, Q
// The status: FEA_FATIGUE_NO_STRESS m0 = 0 or m2 = 0, everything 0; FEA_FATIGUE_NARROW 1 - alpha2 <= 1e-6, where Dirlik's
// parameters leave their range (Q <= 0 from 1 - alpha2 ~ 1e-8 on): the three damages are D_NB; FEA_FATIGUE_NO_DIRLIK the
// parameters are no density (one not finite, a negative weight, Q <= 0): D_DK takes D_TB.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define FEA_HD __host__ __device__
#else
#define FEA_HD
#endif

#define FEA_FATIGUE_NO_STRESS 1
#define FEA_FATIGUE_NARROW 2
#define FEA_FATIGUE_NO_DIRLIK 4

// what depends on the S-N curve alone: made once on the host in long double (fatigue_constants)
template <class T>
struct FatigueConsts {
  T b;                                 // the exponent
  T inv_a;                             // 1 / A
  T gamma_b;                           // Gamma(1 + b)
  T gamma_hb;                          // Gamma(1 + b / 2)
  T two_hb;                            // 2^(b / 2)
};

template <class T> FEA_HD inline bool fatigue_finite(T v) { return v - v == T(0); }
template <class T> FEA_HD inline T fatigue_clamp01(T v) { return !(v > T(0)) ? T(0) : (v > T(1) ? T(1) : v); }

// m = (m0, m1, m2, m4), none negative; rates = (nu0, nup), damage = (D_NB, D_DK, D_TB) per unit time; the status returned
template <class T>
FEA_HD inline int fatigue_point(const T (&m)[4], const FatigueConsts<T> &k, T (&rates)[2], T (&damage)[3])
{
  using std::sqrt; using std::pow; using std::exp; using std::fabs;
  const T m0 = m[0], m1 = m[1], m2 = m[2], m4 = m[3];
  const T two_pi = T(6.283185307179586476925286766559L);
  rates[0] = rates[1] = T(0);
  damage[0] = damage[1] = damage[2] = T(0);
  if (!(m0 > T(0)) || !(m2 > T(0))) return FEA_FATIGUE_NO_STRESS;
  const T nu0 = sqrt(m2 / m0) / two_pi;
  const T nup = m4 > T(0) ? sqrt(m4 / m2) / two_pi : T(0);
  rates[0] = nu0; rates[1] = nup;
  const T hb = T(0.5) * k.b;
  const T d_nb = (nu0 * k.inv_a) * pow(T(2) * m0, hb) * k.gamma_hb;
  const T g = m2 / sqrt(m0 * m4);                                      // (alpha2 before clamping; +inf where m4 = 0)
  const T a1 = fatigue_clamp01(m1 / sqrt(m0 * m2)), a2 = fatigue_clamp01(g);
  if (T(1) - a2 <= T(1e-6L)) {
    damage[0] = damage[1] = damage[2] = d_nb;
    return FEA_FATIGUE_NARROW;
  }
  const T da = a1 - a2;
  const T bw = da * (T(1.112L) * (T(1) + a1 * a2 - a1 - a2) * exp(T(2.11L) * a2) + da) / ((a2 - T(1)) * (a2 - T(1)));
  const T d_tb = (bw + (T(1) - bw) * pow(a2, k.b - T(1))) * d_nb;
  const T xm = (m1 / m0) * sqrt(m2 / m4);
  const T g2 = g * g;
  const T D1 = T(2) * (xm - g2) / (T(1) + g2);
  const T den = T(1) - g - D1 + D1 * D1;
  const T R = (g - xm - D1 * D1) / den;
  const T D2 = den / (T(1) - R);
  const T D3 = T(1) - D1 - D2;
  const T Q = T(1.25) * (g - D3 - D2 * R) / D1;
  const bool valid = fatigue_finite(D1) && fatigue_finite(D2) && fatigue_finite(D3) && fatigue_finite(R) && fatigue_finite(Q) &&
                     D1 >= T(0) && D2 >= T(0) && D3 >= T(0) && (!(D1 > T(0)) || Q > T(0));
  damage[0] = d_nb; damage[2] = d_tb;
  if (!valid) {
    damage[1] = d_tb;
    return FEA_FATIGUE_NO_DIRLIK;
  }
  damage[1] = (nup * k.inv_a) * pow(m0, hb) * (D1 * pow(Q, k.b) * k.gamma_b + k.two_hb * k.gamma_hb * (D2 * pow(fabs(R), k.b) + D3));
  return 0;
}
