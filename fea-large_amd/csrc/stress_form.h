// stress_form.h -- what the kernels that evaluate quadratic forms on the stress store share (k_stress_combine of
// kernels_stress_combine.hip, k_stress_moments of kernels_stress_fatigue.hip): the difference of two stress rows taken on
// load, and one form (C, b, s) of a combination's 8 P values against the folded table of superpose.h.  Both kernels run
// these very functions, so a moment of order 0 has the bits of the square the combine kernel takes the root of.
#pragma once
#include "superpose.h"

// x[8 p + a] = T_p[r0][a] - T_p[r1][a]: load_mode_values on the difference of two rows
template <int P>
__device__ __forceinline__ void load_mode_difference(const double *__restrict__ Q, size_t pstride, int r0, int r1, bool in,
                                                     double (&x)[MC * P])
{
#pragma unroll
  for (int e = 0; e < MC * P; ++e) x[e] = 0.0;
  if (!in) return;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const mode_v2d *Q0 = reinterpret_cast<const mode_v2d *>(Q + (size_t)p * pstride) + (size_t)r0 * 4;
    const mode_v2d *Q1 = reinterpret_cast<const mode_v2d *>(Q + (size_t)p * pstride) + (size_t)r1 * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const mode_v2d t = Q0[k] - Q1[k];
      x[p * MC + 2 * k] = t.x; x[p * MC + 2 * k + 1] = t.y;
    }
  }
}

// x' T x + u0 (2 b' x + s u0) over the columns c < 8 P, T the folded table: the sums of k_response_combine, two rows of
// the triangle at a time
template <int P>
__device__ __forceinline__ double stress_form(const double (&x)[MC * P], double u0, const double *__restrict__ form)
{
  constexpr int M = MC * P;
  constexpr int R = 2;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < M; j += R) {
    const double *row = form + j * ML;
    double t[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      t[r] = row[r * ML + j + r] * x[j + r];
#pragma unroll
      for (int k = j + r + 1; k < j + R; ++k) t[r] = fma(row[r * ML + k], x[k], t[r]);
    }
#pragma unroll
    for (int k = j + R; k < M; ++k) {
#pragma unroll
      for (int r = 0; r < R; ++r) t[r] = fma(row[r * ML + k], x[k], t[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc = fma(x[j + r], t[r], acc);
  }
  const double *b = form + ML * ML;
  double bx = 0.0;
#pragma unroll
  for (int k = 0; k < M; ++k) bx = fma(b[k], x[k], bx);
  return fma(u0, fma(b[ML], u0, 2.0 * bx), acc);                       // (b[64] is s)
}
