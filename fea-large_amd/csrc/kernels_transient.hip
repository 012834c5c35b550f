// kernels_transient.hip -- transient response by mode superposition on the locked store, and the base-excitation load,
// on gfx950.
//
// The load held by feahip_response_load or feahip_response_base_load is F g(t), g piecewise linear on a uniform grid.
// The host integrates every mode exactly (transient_table.cpp) and hands one real coefficient row per step to
//   k_transient_sweep<P, D, S, FIELD>   the structure of k_response_sweep, real: a lane owns D dofs and loads their 8 P
//                           mode values once (superpose.h); it then walks the rows of a chunk: the 8 P coefficients
//                           and g_n of a step are wave-uniform (scalar loads), u = fma(us, g_n, 0) and 8 P v_fma_f64 in
//                           column order follow per dof, S rows at a time (S independent chains).  It keeps the largest
//                           |u| and its GLOBAL step -- a strict comparison, so ties keep the lowest step -- and every
//                           launch after the first of a call continues from the best / at it finds in the output
//                           buffer.  FIELD writes u of one row (a snapshot) instead.
//   k_base_load             f = -(M r) on the free dofs, 0 on the prescribed ones
// The history goes through the coefficient buffer of the response state, FEA_TRANSIENT_CHUNK rows of 64 at a time with
// their g_n behind them (transient_stream.h owns the host side of that): no device allocation grows with the step count.
// No atomics, the same bits on every call.
// A context that never calls a transient entry allocates and launches nothing of this file.
#include "transient_stream.h"

// Rows per loop iteration of k_transient_sweep.  One row is a single chain of 8 P dependent v_fma_f64 per dof, which at
// eight panels runs at the rate of ONE frequency of the complex sweep (two chains); two rows give two chains.  Measured
// (DESIGN.md section 22): two rows win from two panels on, one row with a single panel.  TRANSIENT_STEPS forces one value
// for every P, for measurements: `make variant NAME=ts2 VSRC=kernels_transient VFLAGS=-DTRANSIENT_STEPS=2`
#ifdef TRANSIENT_STEPS
#define TRANSIENT_STEPS_OF(P) TRANSIENT_STEPS
#else
#define TRANSIENT_STEPS_OF(P) ((P) >= 2 ? 2 : 1)
#endif

// u_d(t_j) = us[d] g[j] + sum_c Q[d][c] coef[j][c] over the columns c < 8 P, summed in column order.
// !FIELD: o0[d] = max_j |u_d(t_j)| and o1[d] = step0 + the lowest j that attains it, over the rows of this launch and,
// unless `first`, what o0 / o1 held.  FIELD: o0[d] = u_d of row 0 with g0 for g.  A workgroup takes 256 D consecutive
// dofs, lane t the dofs t, t + 256, ...
template <int P, int D, int S, bool FIELD>
__global__ __launch_bounds__(256)
void k_transient_sweep(int ndof, int n_rows, int step0, int first, const double *__restrict__ Q, size_t pstride,
                       const double *__restrict__ us, const double *__restrict__ coef, const double *__restrict__ g, double g0,
                       double *__restrict__ o0, int *__restrict__ o1)
{
  const int d0 = blockIdx.x * (256 * D) + threadIdx.x;
  double phi[D][MC * P], u0[D], best[D];
  int at[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    const int d = d0 + 256 * i;
    const bool in = d < ndof;
    u0[i] = in ? us[d] : 0.0;
    best[i] = -1.0;
    at[i] = 0;
    if constexpr (!FIELD)
      if (!first && in) { best[i] = o0[d]; at[i] = o1[d]; }
    load_mode_values<P>(Q, pstride, d, in, phi[i]);
  }
  int j = 0;
  // S rows per iteration: S independent FMA chains per dof and S rows' loads in flight.  The comparisons keep the order
  // of the steps, so the bits and the ties are those of the one-row loop below, which also takes what is left
  if constexpr (!FIELD && S > 1) {
    for (; j + S <= n_rows; j += S) {
      const double *cr = coef + (size_t)j * FEA_MODAL_MAX_LOCKED;
      double u[S][D];
#pragma unroll
      for (int r = 0; r < S; ++r) {
        const double gr = g[j + r];
#pragma unroll
        for (int i = 0; i < D; ++i) u[r][i] = fma(u0[i], gr, 0.0);
      }
#pragma unroll
      for (int c = 0; c < MC * P; ++c) {
#pragma unroll
        for (int r = 0; r < S; ++r) {
          const double a = cr[r * FEA_MODAL_MAX_LOCKED + c];
#pragma unroll
          for (int i = 0; i < D; ++i) u[r][i] = fma(phi[i][c], a, u[r][i]);
        }
      }
#pragma unroll
      for (int r = 0; r < S; ++r) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const double m = fabs(u[r][i]);
          if (m > best[i]) { best[i] = m; at[i] = step0 + j + r; }
        }
      }
    }
  }
  for (; j < n_rows; ++j) {
    const double *cr = coef + (size_t)j * FEA_MODAL_MAX_LOCKED;         // (uniform: scalar loads)
    const double gj = FIELD ? g0 : g[j];
    double u[D];
#pragma unroll
    for (int i = 0; i < D; ++i) u[i] = fma(u0[i], gj, 0.0);
#pragma unroll
    for (int c = 0; c < MC * P; ++c) {
      const double a = cr[c];
#pragma unroll
      for (int i = 0; i < D; ++i) u[i] = fma(phi[i][c], a, u[i]);
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      if constexpr (FIELD) {
        const int d = d0 + 256 * i;
        if (d < ndof) o0[d] = u[i];
      } else {
        const double m = fabs(u[i]);
        if (m > best[i]) { best[i] = m; at[i] = step0 + j; }
      }
    }
  }
  if constexpr (!FIELD) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int d = d0 + 256 * i;
      if (d < ndof) { o0[d] = best[i]; o1[d] = at[i]; }
    }
  }
}

__global__ __launch_bounds__(256)
void k_base_load(int ndof, const uint8_t *__restrict__ mask, const double *__restrict__ mr, double *__restrict__ f)
{
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d < ndof) f[d] = mask[d] ? 0.0 : -mr[d];
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
int launch_base_load(feahip_ctx *c, const double *d_mr, double *d_f)
{
  hipLaunchKernelGGL(k_base_load, dim3((c->ndof + 255) / 256), dim3(256), 0, c->stream, c->ndof, (const uint8_t *)c->d_dofmask,
                     d_mr, d_f);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

template <int P, bool FIELD>
static void enq_transient_p(feahip_ctx *c, int n_rows, int step0, int first, const double *d_coef, double g0, double *d_o0)
{
  constexpr int D = 1, S = FIELD ? 1 : TRANSIENT_STEPS_OF(P);        // (two dofs per lane leave one wave on a SIMD: section 21)
  ResponseState &R = c->response;
  hipLaunchKernelGGL((k_transient_sweep<P, D, S, FIELD>), dim3((c->ndof + 256 * D - 1) / (256 * D)), dim3(256), 0, c->stream,
                     c->ndof, n_rows, step0, first, (const double *)locked_panel(c, 0, 0), (size_t)c->ndof * MC,
                     (const double *)R.d_us, d_coef, (const double *)chunk_g(R.d_coef), g0, d_o0, (int *)(R.d_out + c->ndof));
}

template <bool FIELD>
static void enq_transient(feahip_ctx *c, int n_rows, int step0, int first, const double *d_coef, double g0, double *d_o0)
{
  for_panels(panels_of(c), [&](auto P) { enq_transient_p<decltype(P)::value, FIELD>(c, n_rows, step0, first, d_coef, g0, d_o0); });
}

int response_transient(feahip_ctx *c, int n_steps, double dt, const double *g, double alpha, double beta, const double *zeta,
                       int quantity, double *h_peak, int *h_at, int n_probe, const int *probe, double *h_probe, int n_snap,
                       const int *snap_step, double *h_snap)
{
  ResponseState &R = c->response;
  const size_t nd = (size_t)c->ndof;
  const int n_rows = n_steps + 1;
  TransientStream T;                                                   // (the static term u_s g_n belongs to the displacement alone)
  int rc;
  if ((rc = T.open(c, "response_transient", n_steps, dt, g, alpha, beta, zeta, quantity, quantity == 0, 0))) return rc;
  R.swept_freq = 0;                                                    // the table of a frequency sweep is gone from d_coef
  R.trans_rows = 0;
  ProbeRows rows;                                                      // read back once
  if ((rc = rows.read(c, n_probe, probe))) return rc;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  // the probes' values and the snapshots' rows, taken from a chunk as the host fills it
  std::vector<double> snap_rows((size_t)n_snap * (FEA_MODAL_MAX_LOCKED + 1));
  auto on_host = [&](int step0, int count, const double *coef, const double *gs) {
    for (int r = 0; r < n_probe; ++r)
      for (int j = 0; j < count; ++j)
        h_probe[(size_t)r * n_rows + step0 + j] = rows.sum(r, coef + (size_t)j * FEA_MODAL_MAX_LOCKED, std::fma(rows.us(r), gs[j], 0.0));
    for (int s = 0; s < n_snap; ++s)
      if (snap_step[s] >= step0 && snap_step[s] < step0 + count) {
        double *keep = snap_rows.data() + (size_t)s * (FEA_MODAL_MAX_LOCKED + 1);
        std::copy_n(coef + (size_t)(snap_step[s] - step0) * FEA_MODAL_MAX_LOCKED, FEA_MODAL_MAX_LOCKED, keep);
        keep[FEA_MODAL_MAX_LOCKED] = gs[snap_step[s] - step0];
      }
  };
  auto launch = [&](int count, int step0, bool first, bool) { enq_transient<false>(c, count, step0, first, R.d_coef, 0.0, R.d_out); };
  if ((rc = T.pass(R.d_coef, true, on_host, launch))) return rc;
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_peak, R.d_out, sizeof(double) * nd, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_at, R.d_out + nd, sizeof(int) * nd, hipMemcpyDeviceToHost, c->stream));
  // the snapshots: one launch each, its row through the 64 doubles of d_q (free between two loads), its g by value;
  // the field goes through the front of d_out, behind the copy of the peaks in stream order
  for (int s = 0; s < n_snap; ++s) {
    const double *keep = snap_rows.data() + (size_t)s * (FEA_MODAL_MAX_LOCKED + 1);
    FEA_HIP_CHECK(c, hipMemcpyAsync(R.d_q, keep, sizeof(double) * FEA_MODAL_MAX_LOCKED, hipMemcpyHostToDevice, c->stream));
    enq_transient<true>(c, 1, snap_step[s], 1, R.d_q, keep[FEA_MODAL_MAX_LOCKED], R.d_out);
    FEA_HIP_CHECK(c, hipGetLastError());
    FEA_HIP_CHECK(c, hipMemcpyAsync(h_snap + (size_t)s * nd, R.d_out, sizeof(double) * nd, hipMemcpyDeviceToHost, c->stream));
  }
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  R.trans_rows = T.last_count;
  R.trans_step0 = T.last_step0;
  return FEAHIP_OK;
}

// hook 25 of feahip_time_kernel: the sweep over the last chunk of the last feahip_response_transient, as a first launch
int time_transient_kernel(feahip_ctx *c)
{
  enq_transient<false>(c, c->response.trans_rows, c->response.trans_step0, 1, c->response.d_coef, 0.0, c->response.d_out);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
