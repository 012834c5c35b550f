// kernels_combine.hip -- one quadratic form of the mode values on every dof of the locked store, on gfx950: what a response
// spectrum and a random-vibration analysis ask of the modes and the load held (combine_table.cpp builds their forms).
//
// With x_i = (phi_i1 .. phi_im) the mode values of dof i, u_s,i its static correction, a symmetric C[m][m], b[m] and s,
//   out_i = sqrt(max(0,  x_i' C x_i  +  2 u_s,i (b' x_i)  +  s u_s,i^2 ))
// C, b and s are the same for every dof and come from the host: a PSD's covariance of the modal coordinates, rho_jk a_j a_k
// of SRSS and CQC, |a||a|' of ABS; the missing-mass term and the mode-acceleration correction enter through b and s.
//   k_response_combine<P, ABSX>   the structure of k_response_sweep: a lane owns one dof and loads its 8 P mode values once
//                           (superpose.h) and its u_s.  The form table is a device buffer of its own, [64][64] by
//                           store column, then b[64], then s.  The host folds C onto its upper triangle (the diagonal as
//                           it is, the entries above it doubled, which is exact, zero below), so the kernel evaluates
//                             sum_j x_j (sum_{k >= j} T_jk x_k):  m (m + 1) / 2 + m v_fma_f64 where the full form has
//                           m^2 + m.  Every table address is wave-uniform: the compiler takes the table through the
//                           scalar data cache; it is never read per lane and never staged in LDS.  The triangle is
//                           unrolled whole -- every register index is static -- COMBINE_ROWS rows at a time, so that
//                           many independent FMA chains are in flight per dof.  ABSX takes |phi| on load: the ABS rule,
//                           (sum_k |phi_ik| |a_k|)^2, is the form with C = |a||a|'.
// d_coef is not touched: the tables of the last sweep and transient stay (hooks 23 and 25).  No atomics, the same bits on
// every call.  A context that never calls a combine entry allocates and launches nothing of this file.
#include "superpose.h"

// Rows of the triangle evaluated together: so many independent FMA chains per dof.  Measured;
// `make variant NAME=cr4 VSRC=kernels_combine VFLAGS=-DCOMBINE_ROWS=4` forces another value
#ifndef COMBINE_ROWS
#define COMBINE_ROWS 2
#endif
static_assert(COMBINE_ROWS == 1 || COMBINE_ROWS == 2 || COMBINE_ROWS == 4 || COMBINE_ROWS == 8, "COMBINE_ROWS divides 8");

// out[d] = sqrt(max(0, x' T x + us (2 b' x + s us))) over the columns c < 8 P, T the folded table (see above).
// A workgroup takes 256 consecutive dofs
template <int P, bool ABSX>
__global__ __launch_bounds__(256)
void k_response_combine(int ndof, const double *__restrict__ Q, size_t pstride, const double *__restrict__ us,
                        const double *__restrict__ form, double *__restrict__ out)
{
  constexpr int M = MC * P;
  const int d = blockIdx.x * 256 + threadIdx.x;
  const bool in = d < ndof;
  double x[M];
  const double u0 = in ? us[d] : 0.0;
  load_mode_values<P, ABSX>(Q, pstride, d, in, x);
  // R rows together (R divides 8): t[r] = sum_{k >= j + r} T_{j+r,k} x_k, column by column over the R chains, then
  // acc += x_{j+r} t[r] (uniform addresses: scalar loads)
  constexpr int R = COMBINE_ROWS;
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
  const double v = fma(u0, fma(b[ML], u0, 2.0 * bx), acc);            // (b[64] is s)
  if (in) out[d] = sqrt(fmax(v, 0.0));
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
template <int P, bool ABSX>
static void enq_combine_p(feahip_ctx *c)
{
  ResponseState &R = c->response;
  hipLaunchKernelGGL((k_response_combine<P, ABSX>), dim3((c->ndof + 255) / 256), dim3(256), 0, c->stream, c->ndof,
                     (const double *)locked_panel(c, 0, 0), (size_t)c->ndof * MC, (const double *)R.d_us, (const double *)R.d_form, R.d_out);
}

static void enq_combine(feahip_ctx *c, bool absx)
{
  for_panels(panels_of(c), [&](auto P) { absx ? enq_combine_p<decltype(P)::value, true>(c) : enq_combine_p<decltype(P)::value, false>(c); });
}

// C[n][n], b[n] (null: zero) and s by ascending mode; the table goes to the device folded and by store column
int response_combine(feahip_ctx *c, const double *C, const double *b, double s, bool absx, double *h_out)
{
  ModalState &S = c->modal;
  ResponseState &R = c->response;
  if (!R.d_form) FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_form, sizeof(double) * FEA_COMBINE_TABLE));
  const std::vector<double> T = folded_form(S, C, b, s);
  // (pageable memory: the copy has left T when the call returns)
  FEA_HIP_CHECK(c, hipMemcpyAsync(R.d_form, T.data(), sizeof(double) * FEA_COMBINE_TABLE, hipMemcpyHostToDevice, c->stream));
  R.form_set = false;
  enq_combine(c, absx);
  FEA_HIP_CHECK(c, hipGetLastError());
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_out, R.d_out, sizeof(double) * (size_t)c->ndof, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  R.form_set = true;
  R.form_abs = absx;
  R.form_gen = S.lock_gen;
  return FEAHIP_OK;
}

// hook 26 of feahip_time_kernel: the kernel over the last form, the store and the u_s in force
int time_combine_kernel(feahip_ctx *c)
{
  enq_combine(c, c->response.form_abs);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
