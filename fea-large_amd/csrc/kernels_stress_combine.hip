// kernels_stress_combine.hip -- quadratic forms of the modal stresses on every node, on gfx950: the RMS and the design peak of
// the six stress components and of the von Mises stress under a PSD or a response spectrum (Segalman et al.: the mean
// square of the von Mises stress is a quadratic form of its own in the modal covariance, not a function of the
// component RMS values), and one linear combination of the modal stresses.
//
// The stress store is P panels of [6N][8] doubles (kernels_modal_stress.hip), row 6a + c component c of node a, T_s[6N] the
// stress of the static correction.  For a linear combination y = L T_a (an m-vector of mode values) and y_s = L T_s,a,
//   q(y) = y' C y + 2 y_s (b' y) + s y_s^2
// the form (C, b, s) as k_response_combine takes it: the same folded table, by store column, read through the scalar data
// cache.  The table is a buffer of this file's own, so the form of the last displacement combination stays (hook 26).
//   k_stress_combine<P, ABSX>  a lane owns a NODE and loops over nine combinations, one at a time: the six components, then
//                           xx - yy, yy - zz, zz - xx.  Each holds its 8 P values in registers (the differences are
//                           taken on load: two rows read, one kept), never the 6 x 8 P of the node at once; the triangle
//                           is unrolled whole inside the loop body as in k_response_combine, two rows at a time.
//                             out6[a][c] = sqrt(max(0, q(T_a,c)))
//                             vm[a]      = sqrt(max(0, (q(xx-yy) + q(yy-zz) + q(zz-xx)) / 2 + 3 (q(xy) + q(yz) + q(xz))))
//                           ABSX takes |T| on load and evaluates the six components alone: the differences need the signs.
//   k_stress_field<P>       cs T_s + sum_k coef_k T_k on the six rows of a node, one fma per store column in ascending
//                           order onto cs T_s, and the von Mises stress of the sum.
// No atomics, the same bits on every call.  A context that never calls a stress entry allocates and launches nothing here.
#include "stress_form.h"                                               // load_mode_difference, stress_form

// A workgroup takes 256 consecutive nodes
template <int P, bool ABSX>
__global__ __launch_bounds__(256)
void k_stress_combine(int N, const double *__restrict__ T, size_t pstride, const double *__restrict__ ts,
                      const double *__restrict__ form, double *__restrict__ out6, double *__restrict__ vm)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  const bool in = a < N;
  const int r = in ? 6 * a : 0;
  double qn = 0.0, qs = 0.0;                                           // the forms of the three differences, of the three shears
#pragma unroll 1
  for (int k = 0; k < (ABSX ? 6 : 9); ++k) {
    double x[MC * P], u0;
    if (k < 6) {
      load_mode_values<P, ABSX>(T, pstride, r + k, in, x);
      u0 = in ? ts[r + k] : 0.0;
    } else {
      const int c0 = k - 6, c1 = c0 == 2 ? 0 : c0 + 1;
      load_mode_difference<P>(T, pstride, r + c0, r + c1, in, x);
      u0 = in ? ts[r + c0] - ts[r + c1] : 0.0;
    }
    const double v = stress_form<P>(x, u0, form);
    if (k < 6) {
      if (in) out6[r + k] = sqrt(fmax(v, 0.0));
      if (k >= 3) qs += v;
    } else
      qn += v;
  }
  if (!ABSX && in) vm[a] = sqrt(fmax(fma(3.0, qs, 0.5 * qn), 0.0));
}

// coef[64] by store column, then cs.  A workgroup takes 256 consecutive nodes
template <int P>
__global__ __launch_bounds__(256)
void k_stress_field(int N, const double *__restrict__ T, size_t pstride, const double *__restrict__ ts,
                    const double *__restrict__ coef, double *__restrict__ out6, double *__restrict__ vm)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  const bool in = a < N;
  const int r = in ? 6 * a : 0;
  const double cs = coef[ML];
  double s6[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double x[MC * P];
    load_mode_values<P>(T, pstride, r + c, in, x);
    double y = in ? cs * ts[r + c] : 0.0;
#pragma unroll
    for (int k = 0; k < MC * P; ++k) y = fma(x[k], coef[k], y);
    s6[c] = y;
    if (in) out6[r + c] = y;
  }
  const double p = (s6[0] + s6[1] + s6[2]) * (1.0 / 3.0);
  const double dx = s6[0] - p, dy = s6[1] - p, dz = s6[2] - p;
  if (in) vm[a] = sqrt(1.5 * (dx * dx + dy * dy + dz * dz + 2.0 * (s6[3] * s6[3] + s6[4] * s6[4] + s6[5] * s6[5])));
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
template <int P, bool ABSX>
static void enq_stress_combine_p(feahip_ctx *c)
{
  StressState &S = c->stress;
  hipLaunchKernelGGL((k_stress_combine<P, ABSX>), dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->N,
                     (const double *)S.d_store, (size_t)6 * c->N * MC, (const double *)S.d_ts, (const double *)S.d_form, S.d_out6, S.d_vm);
}

static void enq_stress_combine(feahip_ctx *c, bool absx)
{
  for_panels(panels_of(c), [&](auto P) { absx ? enq_stress_combine_p<decltype(P)::value, true>(c) : enq_stress_combine_p<decltype(P)::value, false>(c); });
}

// C[n][n], b[n] (null: zero) and s by ascending mode, as response_combine takes them; h_out6[6N] and h_vm[N] (null with
// absx) in library ids
int stress_combine(feahip_ctx *c, const double *C, const double *b, double s, bool absx, double *h_out6, double *h_vm)
{
  ModalState &M = c->modal;
  StressState &S = c->stress;
  if (!S.d_form) FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_form, sizeof(double) * FEA_COMBINE_TABLE));
  const std::vector<double> T = folded_form(M, C, b, s);
  // (pageable memory: the copy has left T when the call returns)
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.d_form, T.data(), sizeof(double) * FEA_COMBINE_TABLE, hipMemcpyHostToDevice, c->stream));
  S.form_set = false;
  enq_stress_combine(c, absx);
  FEA_HIP_CHECK(c, hipGetLastError());
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_out6, S.d_out6, sizeof(double) * 6 * (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
  if (!absx && h_vm) FEA_HIP_CHECK(c, hipMemcpyAsync(h_vm, S.d_vm, sizeof(double) * (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  S.form_set = true;
  S.form_abs = absx;
  return FEAHIP_OK;
}

// coef[n] by ascending mode and cs; h_out6[6N] and h_vm[N] in library ids
int stress_field(feahip_ctx *c, const double *coef, double cs, double *h_out6, double *h_vm)
{
  ModalState &M = c->modal;
  StressState &S = c->stress;
  if (!S.d_fcoef) FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_fcoef, sizeof(double) * (ML + 8)));
  double t[ML + 8] = {0};
  for (int j = 0; j < M.n_locked; ++j) t[M.lock_order[j]] = coef[j];
  t[ML] = cs;
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.d_fcoef, t, sizeof(t), hipMemcpyHostToDevice, c->stream));
  for_panels(panels_of(c), [&](auto P) {
    hipLaunchKernelGGL((k_stress_field<decltype(P)::value>), dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->N,
                       (const double *)S.d_store, (size_t)6 * c->N * MC, (const double *)S.d_ts, (const double *)S.d_fcoef, S.d_out6, S.d_vm);
  });
  FEA_HIP_CHECK(c, hipGetLastError());
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_out6, S.d_out6, sizeof(double) * 6 * (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_vm, S.d_vm, sizeof(double) * (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

// hook 28 of feahip_time_kernel: the kernel over the last form, the stress store and the T_s in force
int time_stress_combine(feahip_ctx *c)
{
  enq_stress_combine(c, c->stress.form_abs);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
