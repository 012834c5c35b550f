// kernels_response.hip -- steady-state response to a harmonic load by mode superposition on the locked store, on gfx950.
//
// With (lam_k, phi_k), k < m <= 64, the M-orthonormal modes the store of feahip_solve_modes_locked (or of
// feahip_response_set_basis) holds, a real load F and the modal damping d_k = alpha + beta_k lam_k + 2 zeta_k sqrt(lam_k):
//   q_k = phi_k' F,   H_k(w) = 1 / (lam_k - w^2 + i w d_k),   u(w) = u_s + sum_k phi_k a_k(w)
//   mode displacement:  u_s = 0,          a_k = q_k H_k
//   mode acceleration:  K u_s = F,        a_k = q_k (H_k - 1 / lam_k)
// Nothing here is indefinite or complex on the device: one projection and one positive definite solve per load, then per
// frequency 2 m real coefficients that are the same for every dof.
//   k_response_project      q = Q' F: one read of F and of the panels in use on a fixed grid, a lane keeps one column of
//                           every panel over its share of the dofs; the lanes of a wave that hold the same column meet in
//                           a butterfly, the four waves in LDS in wave order, the workgroups in k_response_reduce.  No
//                           atomics, the same bits on every call
//   k_response_sweep<P, D, FIELD>   a lane owns D dofs and loads their 8 P mode values once (the layout and the instance
//                           for the panels in use: superpose.h); it then walks the coefficient
//                           table [n_freq][2][64]: the 16 P coefficients of a frequency are wave-uniform (the compiler takes
//                           them through the scalar data cache), 16 P D v_fma_f64 follow.  It keeps the largest re^2 + im^2
//                           and its index -- a strict comparison, so ties keep the lowest frequency -- and writes one sqrt
//                           and one index at the end; FIELD writes re and im of every frequency instead.
// The host builds the table (response_coefficients): it is small, and where it would not be finite -- w = 0 on a zero
// mode, w^2 = lam_k without damping -- the sweep is refused before anything is launched.
// A context that never calls a response entry allocates and launches nothing of this file.
#include "superpose.h"
#include "reduce_device.h"

#define RB FEA_RED_BLOCKS
#define RESPONSE_PANELS (FEA_MODAL_MAX_LOCKED / MC)
// dofs per lane of k_response_sweep: 1 keeps three waves on a SIMD at eight panels, 2 halves the coefficient traffic of
// a dof and leaves one (DESIGN.md section 21 has both measured; `make variant VSRC=kernels_response VFLAGS=-DRESPONSE_DOFS=2`)
#ifndef RESPONSE_DOFS
#define RESPONSE_DOFS 1
#endif

// v[e] = 0 where the dof e >> shift is prescribed: a vector [3N] (shift 0) or a block vector [3N][8] (shift 3)
__global__ __launch_bounds__(256)
void k_response_mask(size_t n, int shift, const uint8_t *__restrict__ mask, double *__restrict__ v)
{
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n && mask[e >> shift]) v[e] = 0.0;
}

// part[(p 8 + a) RB + block] = the workgroup's share of sum_d Q_p[d][a] F[d], for every panel p < npanels.  Thread t of a
// tile of 32 dofs reads element t of every panel's tile (coalesced) and F of the dof t >> 3: it keeps column t & 7
__global__ __launch_bounds__(256)
void k_response_project(int ndof, int npanels, const double *__restrict__ F, const double *__restrict__ Q, size_t pstride,
                        double *__restrict__ part)
{
  __shared__ double sh[4][RESPONSE_PANELS][MC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double acc[RESPONSE_PANELS];
#pragma unroll
  for (int p = 0; p < RESPONSE_PANELS; ++p) acc[p] = 0.0;
  const int ntiles = (ndof + 31) / 32;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t e = (size_t)tile * 256 + threadIdx.x;                  // element of a block vector
    const bool in = e < (size_t)ndof * MC;
    const double f = in ? F[e >> 3] : 0.0;
#pragma unroll
    for (int p = 0; p < RESPONSE_PANELS; ++p)
      if (p < npanels) acc[p] += (in ? Q[(size_t)p * pstride + e] : 0.0) * f;
  }
#pragma unroll
  for (int p = 0; p < RESPONSE_PANELS; ++p) {
    double v = acc[p];
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < MC) sh[wave][p][lane] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < npanels * MC; e += 256) {
    const int p = e >> 3, a = e & 7;
    part[(size_t)e * RB + blockIdx.x] = ((sh[0][p][a] + sh[1][p][a]) + sh[2][p][a]) + sh[3][p][a];
  }
}

// out[b] = the sum of part[b RB .. b RB + n), one workgroup per store column
__global__ __launch_bounds__(256)
void k_response_reduce(int n, const double *__restrict__ part, double *__restrict__ out)
{
  __shared__ double scratch[5];
  const double v = reduce_partials(part + (size_t)blockIdx.x * RB, n, scratch);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// u_d(w_j) = us[d] + sum_c Q[d][c] (coef[j][0][c] + i coef[j][1][c]) over the columns c < 8 P, summed in column order.
// !FIELD: o0[d] = max_j |u_d(w_j)|, o1[d] (int) = the lowest j that attains it.  FIELD: o0[j ndof + d] = re, o1 (double)
// [j ndof + d] = im.  A workgroup takes 256 D consecutive dofs, lane t the dofs t, t + 256, ...
template <int P, int D, bool FIELD>
__global__ __launch_bounds__(256)
void k_response_sweep(int ndof, int n_freq, const double *__restrict__ Q, size_t pstride, const double *__restrict__ us,
                      const double *__restrict__ coef, double *__restrict__ o0, void *__restrict__ o1)
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
    // load_mode_values (superpose.h) written out, every load under its own predicate: with the helper's one branch the
    // frequency loop is scheduled differently and measures 0.3 % slower at eight panels
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const mode_v2d *Qd = reinterpret_cast<const mode_v2d *>(Q + (size_t)p * pstride) + (size_t)(in ? d : 0) * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const mode_v2d t = in ? Qd[k] : mode_v2d{0.0, 0.0};
        phi[i][p * MC + 2 * k] = t.x; phi[i][p * MC + 2 * k + 1] = t.y;
      }
    }
  }
  for (int j = 0; j < n_freq; ++j) {
    const double *cr = coef + (size_t)j * (2 * FEA_MODAL_MAX_LOCKED);   // (uniform: scalar loads)
    double re[D], im[D];
#pragma unroll
    for (int i = 0; i < D; ++i) { re[i] = u0[i]; im[i] = 0.0; }
#pragma unroll
    for (int c = 0; c < MC * P; ++c) {
      const double a = cr[c], b = cr[FEA_MODAL_MAX_LOCKED + c];
#pragma unroll
      for (int i = 0; i < D; ++i) { re[i] = fma(phi[i][c], a, re[i]); im[i] = fma(phi[i][c], b, im[i]); }
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      if constexpr (FIELD) {
        const int d = d0 + 256 * i;
        if (d < ndof) {
          o0[(size_t)j * ndof + d] = re[i];
          static_cast<double *>(o1)[(size_t)j * ndof + d] = im[i];
        }
      } else {
        const double m = fma(re[i], re[i], im[i] * im[i]);
        if (m > best[i]) { best[i] = m; at[i] = j; }
      }
    }
  }
  if constexpr (!FIELD) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int d = d0 + 256 * i;
      if (d < ndof) { o0[d] = sqrt(best[i]); static_cast<int *>(o1)[d] = at[i]; }
    }
  }
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
int launch_response_mask8(feahip_ctx *c, double *d_v8)
{
  const size_t n8 = (size_t)c->ndof * MC;
  hipLaunchKernelGGL(k_response_mask, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, c->stream, n8, 3,
                     (const uint8_t *)c->d_dofmask, d_v8);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// One entry of the table: with a = lam - w^2 (one rounding: the product is exact inside the fma), b = w d,
//   q H = q (a - i b) / (a^2 + b^2),   q (H - 1 / lam) = q (w^2 a - b^2 - i b lam) / (lam (a^2 + b^2)):
// the second form has no difference of two nearly equal terms for w^2 << lam, where H is close to 1 / lam
int response_coefficients(int n_modes, const double *lam, const double *q, const int *order, int n_freq, const double *omega,
                          double alpha, double beta, const double *zeta, int correction, double *coef, std::string *why)
{
  auto refuse = [&](const std::string &s) { if (why) *why = s; return FEAHIP_EINVAL; };
  if (n_modes < 1 || n_modes > FEA_MODAL_MAX_LOCKED) return refuse("the number of modes must be in [1, 64]");
  if (n_freq < 1 || n_freq > FEA_RESPONSE_MAX_FREQ) return refuse("n_freq must be in [1, " + std::to_string(FEA_RESPONSE_MAX_FREQ) + "]");
  if (!lam || !q || !omega || !coef) return refuse("null argument");
  if (!(alpha >= 0.0) || !std::isfinite(alpha) || !(beta >= 0.0) || !std::isfinite(beta))
    return refuse("alpha and beta_k must be finite and not negative");
  double d[FEA_MODAL_MAX_LOCKED];
  for (int k = 0; k < n_modes; ++k) {
    const double z = zeta ? zeta[k] : 0.0;
    if (!(z >= 0.0) || !std::isfinite(z)) return refuse("zeta must be finite and not negative");
    if (!std::isfinite(lam[k]) || !std::isfinite(q[k])) return refuse("lam and q must be finite");
    if (correction && !(lam[k] > 0.0)) return refuse("the static correction needs lam_k > 0 for every mode");
    d[k] = alpha + beta * lam[k] + 2.0 * z * std::sqrt(lam[k] > 0.0 ? lam[k] : 0.0);
  }
  for (int j = 0; j < n_freq; ++j) {
    const double w = omega[j];
    if (!(w >= 0.0) || !std::isfinite(w)) return refuse("omega must be finite and not negative");
    double *re = coef + (size_t)j * (2 * FEA_MODAL_MAX_LOCKED), *im = re + FEA_MODAL_MAX_LOCKED;
    for (int e = 0; e < 2 * FEA_MODAL_MAX_LOCKED; ++e) re[e] = 0.0;
    for (int k = 0; k < n_modes; ++k) {
      const int col = order ? order[k] : k;
      const double a = std::fma(-w, w, lam[k]), b = w * d[k], den = a * a + b * b;
      if (correction) {
        re[col] = q[k] * (w * w * a - b * b) / (lam[k] * den);
        im[col] = -(q[k] * b) / den;
      } else {
        re[col] = q[k] * a / den;
        im[col] = -(q[k] * b) / den;
      }
      if (!std::isfinite(re[col]) || !std::isfinite(im[col]))
        return refuse("the coefficient of mode " + std::to_string(k + 1) + " at omega = " + std::to_string(w) +
                      " is not finite (omega = 0 on a zero mode, or omega^2 = lam_k without damping)");
    }
  }
  return FEAHIP_OK;
}

static int ensure_response(feahip_ctx *c)
{
  ResponseState &R = c->response;
  if (R.d_us) return FEAHIP_OK;
  const size_t n = (size_t)c->ndof;
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_us, sizeof(double) * n));
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_out, sizeof(double) * 2 * n));
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_part, sizeof(double) * (size_t)FEA_MODAL_MAX_LOCKED * RB));
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_q, sizeof(double) * FEA_MODAL_MAX_LOCKED));
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_coef, sizeof(double) * (size_t)FEA_RESPONSE_MAX_FREQ * 2 * FEA_MODAL_MAX_LOCKED));
  FEA_HIP_CHECK(c, hipMemsetAsync(R.d_us, 0, sizeof(double) * n, c->stream));
  FEA_HIP_CHECK(c, hipMemsetAsync(R.d_part, 0, sizeof(double) * (size_t)FEA_MODAL_MAX_LOCKED * RB, c->stream));
  return FEAHIP_OK;
}

static int project_grid(const feahip_ctx *c)
{
  const int g = (c->ndof + 31) / 32;
  return g < RB ? (g > 0 ? g : 1) : RB;
}

static void enq_project(feahip_ctx *c, int panels)
{
  hipLaunchKernelGGL(k_response_project, dim3(project_grid(c)), dim3(256), 0, c->stream, c->ndof, panels,
                     (const double *)c->d_f, (const double *)locked_panel(c, 0, 0), (size_t)c->ndof * MC, c->response.d_part);
}

int response_load(feahip_ctx *c, const double *h_F, int correction, int solver_type, double tol, int max_it, double *q,
                  int *iters, double *resid)
{
  ModalState &S = c->modal;
  ResponseState &R = c->response;
  R.loaded = false;
  int rc;
  if ((rc = ensure_response(c))) return rc;
  const int n = S.n_locked, panels = panels_of(c);
  const size_t nd = (size_t)c->ndof;
  // f <- F, zero on the prescribed dofs (the base load is made there: kernels_transient.hip); q = Q' f
  if (h_F) {
    FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_f, h_F, sizeof(double) * nd, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_response_mask, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, c->stream, nd, 0,
                       (const uint8_t *)c->d_dofmask, c->d_f);
  }
  enq_project(c, panels);
  hipLaunchKernelGGL(k_response_reduce, dim3(panels * MC), dim3(256), 0, c->stream, project_grid(c),
                     (const double *)R.d_part, R.d_q);
  FEA_HIP_CHECK(c, hipGetLastError());
  double qs[FEA_MODAL_MAX_LOCKED];
  FEA_HIP_CHECK(c, hipMemcpyAsync(qs, R.d_q, sizeof(double) * panels * MC, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));                   // (h_F is free again as well)
  for (int k = 0; k < n; ++k) R.q[k] = qs[S.lock_order[k]];
  if (correction) {
    // K(x) masked with factor 0 and K u_s = f by the context's own PCG: K, f and u are another system's from here on
    int its = 0;
    double res = 0.0;
    if ((rc = feahip_create_stiffness(c)) || (rc = feahip_apply_prescribed_bc(c, 0.0)) ||
        (rc = solve_pcg(c, solver_type, tol, max_it, &its, &res))) return rc;
    if (iters) *iters = its;
    if (resid) *resid = res;
    // (the solver itself reports a breakdown only; a u_s that is not one would be wrong at every frequency)
    if (solver_type != FEAHIP_CHOLESKY && its >= max_it && !(res <= tol)) {
      c->err = "response_load: the static solve ran out of its " + std::to_string(max_it) + " iterations at a residual of " + std::to_string(res);
      return FEAHIP_ENOTCONVERGED;
    }
    FEA_HIP_CHECK(c, hipMemcpyAsync(R.d_us, c->d_u, sizeof(double) * nd, hipMemcpyDeviceToDevice, c->stream));
  } else
    FEA_HIP_CHECK(c, hipMemsetAsync(R.d_us, 0, sizeof(double) * nd, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  if (q) for (int k = 0; k < n; ++k) q[k] = R.q[k];
  R.correction = correction ? 1 : 0;
  R.gen = S.lock_gen;
  R.loaded = true;
  ++R.load_count;
  return FEAHIP_OK;
}

template <int P, bool FIELD>
static void enq_sweep_p(feahip_ctx *c, int n_freq)
{
  constexpr int D = FIELD ? 1 : RESPONSE_DOFS;
  ResponseState &R = c->response;
  hipLaunchKernelGGL((k_response_sweep<P, D, FIELD>), dim3((c->ndof + 256 * D - 1) / (256 * D)), dim3(256), 0, c->stream,
                     c->ndof, n_freq, (const double *)locked_panel(c, 0, 0), (size_t)c->ndof * MC, (const double *)R.d_us,
                     (const double *)R.d_coef, R.d_out, (void *)(R.d_out + c->ndof));
}

template <bool FIELD>
static void enq_sweep(feahip_ctx *c, int n_freq)
{
  for_panels(panels_of(c), [&](auto P) { enq_sweep_p<decltype(P)::value, FIELD>(c, n_freq); });
}

int response_sweep(feahip_ctx *c, bool field, int n_freq, const double *omega, double alpha, double beta, const double *zeta,
                   double *h_out0, void *h_out1, int n_probe, const int *probe, double *probe_re, double *probe_im)
{
  ModalState &S = c->modal;
  ResponseState &R = c->response;
  const int n = S.n_locked;
  const size_t nd = (size_t)c->ndof;
  std::vector<double> coef((size_t)n_freq * 2 * FEA_MODAL_MAX_LOCKED);
  std::string why;
  if (response_coefficients(n, S.lam, R.q, S.lock_order, n_freq, omega, alpha, beta, zeta, R.correction, coef.data(), &why)) {
    c->err = std::string(field ? "response_field: " : "response_sweep: ") + why;
    return FEAHIP_EINVAL;
  }
  FEA_HIP_CHECK(c, hipMemcpyAsync(R.d_coef, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice, c->stream));
  if (field) enq_sweep<true>(c, n_freq); else enq_sweep<false>(c, n_freq);
  FEA_HIP_CHECK(c, hipGetLastError());
  R.swept_freq = n_freq;
  R.trans_rows = 0;                                                    // (a transient's last chunk is gone from d_coef)
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_out0, R.d_out, sizeof(double) * nd, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_out1, R.d_out + nd, (field ? sizeof(double) : sizeof(int)) * nd, hipMemcpyDeviceToHost, c->stream));
  // the probes: re from u_s, im from 0, as the kernel sums them
  ProbeRows rows;
  if (const int rc = rows.read(c, n_probe, probe)) return rc;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  for (int r = 0; r < n_probe; ++r)
    for (int j = 0; j < n_freq; ++j) {
      const double *cr = coef.data() + (size_t)j * 2 * FEA_MODAL_MAX_LOCKED;
      probe_re[(size_t)r * n_freq + j] = rows.sum(r, cr, rows.us(r));
      probe_im[(size_t)r * n_freq + j] = rows.sum(r, cr + FEA_MODAL_MAX_LOCKED, 0.0);
    }
  return FEAHIP_OK;
}

// hooks of feahip_time_kernel: 23 the sweep over the table of the last feahip_response_sweep, 24 the projection of f
int time_response_kernel(feahip_ctx *c, int what)
{
  if (what == 23) enq_sweep<false>(c, c->response.swept_freq);
  else enq_project(c, panels_of(c));
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
