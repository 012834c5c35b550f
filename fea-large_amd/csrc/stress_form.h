// stress_form.h -- what the kernels that evaluate quadratic forms on the stress store share (k_stress_combine of
// kernels_stress_combine.hip, k_stress_moments of kernels_stress_fatigue.hip): the difference of two stress rows taken on
// load, and one form (C, b, s) of a combination's 8 P values against the folded table of superpose.h.  Both kernels run
// these very functions, so a moment of order 0 has the bits of the square the combine kernel takes the root of.
#pragma once
#include "superpose.h"
#include <algorithm>

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

// ------------------------------------------------------------------------
// What the kernels that walk a coefficient table with a lane per stress ROW share (k_stress_sweep and k_stress_transient of
// kernels_stress_sweep.hip, k_stress_rainflow of kernels_stress_rainflow.hip): the lane layout, the grid and the probes'
// rows on the host.  (The host side of a chunked transient is transient_stream.h.)
// ------------------------------------------------------------------------
#define SS_NODES_PER_WAVE 10
#define SS_NODES_PER_BLOCK (4 * SS_NODES_PER_WAVE)
// rows per loop iteration of k_stress_transient: k_transient_sweep's choice (kernels_transient.hip)
#ifdef STRESS_SWEEP_STEPS
#define STRESS_SWEEP_STEPS_OF(P) STRESS_SWEEP_STEPS
#else
#define STRESS_SWEEP_STEPS_OF(P) ((P) >= 2 ? 2 : 1)
#endif

// where a lane stands in its wave: component c of the node `node`, row r = 6 node + c; `in` false for the idle lanes and
// past the last node; `base` the lane of the node's component 0 (for an idle lane: itself, so no source leaves the wave)
struct StressLane {
  int node, c, r, base, lane;
  bool in, normal, leader;
};

__device__ __forceinline__ StressLane stress_lane(int N)
{
  StressLane L;
  L.lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = L.lane < 6 * SS_NODES_PER_WAVE;
  const int k = live ? L.lane / 6 : 0;
  L.c = live ? L.lane - 6 * k : 5;                                     // (an idle lane is nobody's leader and no normal lane)
  L.node = wave * SS_NODES_PER_WAVE + k;
  L.in = live && L.node < N;
  L.r = L.in ? 6 * L.node + L.c : 0;
  L.base = live ? 6 * k : L.lane - 5;
  L.normal = L.c < 3;
  L.leader = L.c == 0;
  return L;
}

static inline dim3 stress_sweep_grid(const feahip_ctx *c) { return dim3((c->N + SS_NODES_PER_BLOCK - 1) / SS_NODES_PER_BLOCK); }

namespace {
// The six rows of every probe node of the stress store and of T_s on the host, as ProbeRows has the dofs' (superpose.h):
// sum() is the kernels' sum in the kernels' order, so a probe has the bits of k_stress_field for its row
struct StressProbeRows {
  int width = 0;                       // 8 panels
  std::vector<double> rows;            // [n_probe][6][width + 1]: the values by store column, then T_s
  int read(feahip_ctx *c, int n_probe, const int *node)
  {
    const StressState &S = c->stress;
    width = panels_of(c) * MC;
    const size_t pstride = (size_t)6 * c->N * MC;
    rows.resize((size_t)n_probe * 6 * (width + 1));
    for (int r = 0; r < n_probe; ++r) {
      for (int e = 0; e < 6; ++e) {
        double *row = rows.data() + ((size_t)r * 6 + e) * (width + 1);
        const size_t srow = (size_t)6 * node[r] + e;
        for (int p = 0; p * MC < width; ++p)
          FEA_HIP_CHECK(c, hipMemcpyAsync(row + p * MC, S.d_store + (size_t)p * pstride + srow * MC, sizeof(double) * MC,
                                          hipMemcpyDeviceToHost, c->stream));
        FEA_HIP_CHECK(c, hipMemcpyAsync(row + width, S.d_ts + srow, sizeof(double), hipMemcpyDeviceToHost, c->stream));
      }
    }
    return FEAHIP_OK;
  }
  // cs T_s + sum_col row[col] coef[col] of component e of probe r
  double sum(int r, int e, const double *coef, double cs) const
  {
    const double *row = rows.data() + ((size_t)r * 6 + e) * (width + 1);
    double y = cs * row[width];
    for (int col = 0; col < width; ++col) y = std::fma(row[col], coef[col], y);
    return y;
  }
};
}
