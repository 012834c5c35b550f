// kernels_stress_sweep.hip -- stress peaks over a whole frequency sweep or transient in one launch, on gfx950: for every
// node the largest magnitude of its six stress components and the largest von Mises stress over the rows of a coefficient
// table, with the row that attains each.
//
// The stress store is P panels of [6N][8] doubles (kernels_modal_stress.hip), row 6a + c component c of node a, T_s[6N] the
// stress of the static correction.  A node's 6 x 8 P values do not fit one lane, so a lane owns a stress ROW as the lanes
// of k_response_sweep own a dof: a wave takes 10 consecutive nodes, 60 contiguous rows, lanes 60 to 63 idle, and a
// workgroup of four waves 40 nodes.  The lane loads its 8 P values once (load_mode_values) and walks the table; the
// coefficients of a table row are wave-uniform scalar loads.
//   k_stress_sweep<P>         complex rows [n_freq][2][64]: s = 1 T_s + sum_k T_k re_k + i (0 T_s + sum_k T_k im_k), one fma
//                             per store column in ascending order, the order of k_stress_field (the start values are its
//                             cs T_s with cs = 1 and 0).  Per row |s|^2; per node the cycle peak of the von Mises stress
//                               vm_peak^2 = (A + B) / 2 + sqrt(((A - B) / 2)^2 + C^2),  A = re' V re, B = im' V im, C = re' V im
//   k_stress_transient<P, S>  real rows [n][64] and g[n]: sigma = g T_s + sum_k T_k a_k, S rows per iteration (S independent
//                             chains); per row |sigma|, per node vm^2 = sigma' V sigma.  Every launch after the first of a
//                             call continues from the best / at of the output buffers (vm^2 between launches, its root
//                             written by the last one).
// The six lanes of a node combine across lanes: the three normal lanes read each other's values for the mean, every lane
// forms its share of the von Mises form on the DEVIATOR (1.5 d^2 for a normal lane, 3 s^2 for a shear lane -- never the
// expanded sum p^2 - (sum p)^2 / 3, whose error grows with the hydrostatic part), and a fixed tree
// ((x0 + x3) + (x1 + x4)) + (x2 + x5) brings the sums to the node's first lane, which keeps the node's best and index.
// Every comparison is strict, so ties keep the lowest row.  No LDS memory, no atomics, the same bits on every call.
// The cross-lane moves are DPP shifts of the whole wave by one lane (dpp_device.h: they cross the rows of sixteen, so the
// 60 rows stay contiguous): VALU work that a wave's own FMAs hide.  -DSTRESS_SWEEP_SHFL takes them through __shfl
// (ds_bpermute_b32, the LDS pipe) instead, fewer moves and each a round trip the three waves of a SIMD cannot cover: 1.9
// times slower at eight panels (DESIGN.md section 25 has both measured;
// `make variant NAME=ssshfl VSRC=kernels_stress_sweep VFLAGS=-DSTRESS_SWEEP_SHFL`).
// A context that never calls these entries allocates and launches nothing here.
#include "stress_form.h"
#include "transient_stream.h"
#include "dpp_device.h"

#ifdef STRESS_SWEEP_SHFL
// the mean of the three normal components of the lane's node, (s0 + s1) + s2 as k_stress_field has it, on every lane of
// the node: three moves
__device__ __forceinline__ double node_mean(const StressLane &L, double v)
{
  const double s0 = __shfl(v, L.base, 64), s1 = __shfl(v, L.base + 1, 64), s2 = __shfl(v, L.base + 2, 64);
  return (s0 + s1 + s2) * (1.0 / 3.0);
}
// ((x0 + x3) + (x1 + x4)) + (x2 + x5) over the six lanes of the node, valid on its leader: three moves
__device__ __forceinline__ double node_sum(const StressLane &L, double x)
{
  const int up3 = L.lane + 3 < 64 ? L.lane + 3 : L.lane;
  const double y = x + __shfl(x, up3, 64);                             // lanes 0..2 of the node: x_c + x_(c+3)
  const double y1 = __shfl(y, L.base + 1, 64), y2 = __shfl(y, L.base + 2, 64);
  return (y + y1) + y2;
}
#else
// the same sums in the same order by shifts of the wave by one lane (DPP wave_shl:1, wave_shr:1): four moves for the mean
// on the three normal lanes, five for a sum on the leader
__device__ __forceinline__ double up1(double x) { return dpp_wave_up1(x); }       // lane l takes lane l + 1
__device__ __forceinline__ double down1(double x) { return dpp_wave_down1(x); }   // lane l takes lane l - 1
__device__ __forceinline__ double node_mean(const StressLane &L, double v)
{
  const double t1 = up1(v), t2 = up1(t1);
  const double p = (v + t1 + t2) * (1.0 / 3.0);                        // valid on the leader
  const double q1 = down1(p), q2 = down1(q1);
  return L.c == 0 ? p : (L.c == 1 ? q1 : q2);
}
__device__ __forceinline__ double node_sum(const StressLane &L, double x)
{
  const double y = x + up1(up1(up1(x)));
  const double y1 = up1(y), y2 = up1(y1);
  return (y + y1) + y2;
}
#endif

// o6[r] = max_j |s_r(w_j)| and a6[r] the lowest j that attains it, for every row; ovm[a] = max_j vm_peak_a(w_j) and avm[a]
// likewise, for every node
template <int P>
__global__ __launch_bounds__(256)
void k_stress_sweep(int N, int n_freq, const double *__restrict__ T, size_t pstride, const double *__restrict__ ts,
                    const double *__restrict__ coef, double *__restrict__ o6, int *__restrict__ a6, double *__restrict__ ovm,
                    int *__restrict__ avm)
{
  const StressLane L = stress_lane(N);
  double x[MC * P];
  load_mode_values<P>(T, pstride, L.r, L.in, x);
  const double t0 = L.in ? ts[L.r] : 0.0;
  const double re0 = 1.0 * t0, im0 = 0.0 * t0;                         // (cs T_s of k_stress_field for cs = 1 and cs = 0)
  const double w = L.normal ? 1.5 : 3.0;
  double best = -1.0, vbest = -1.0;
  int at = 0, vat = 0;
  for (int j = 0; j < n_freq; ++j) {
    const double *cr = coef + (size_t)j * (2 * ML);                     // (uniform: scalar loads)
    double re = re0, im = im0;
#pragma unroll
    for (int k = 0; k < MC * P; ++k) {
      const double a = cr[k], b = cr[ML + k];
      re = fma(x[k], a, re); im = fma(x[k], b, im);
    }
    const double m = fma(re, re, im * im);
    if (m > best) { best = m; at = j; }
    const double pr = node_mean(L, re), pi = node_mean(L, im);
    const double dr = L.normal ? re - pr : re, di = L.normal ? im - pi : im;
    const double A = node_sum(L, w * dr * dr), B = node_sum(L, w * di * di), Cm = node_sum(L, w * dr * di);
    const double h = 0.5 * (A + B), d = 0.5 * (A - B);
    const double v = h + sqrt(fma(d, d, Cm * Cm));
    if (v > vbest) { vbest = v; vat = j; }
  }
  if (L.in) {
    o6[L.r] = sqrt(best); a6[L.r] = at;
    if (L.leader) { ovm[L.node] = sqrt(vbest); avm[L.node] = vat; }
  }
}

// o6[r] = max_j |sigma_r(t_j)| and a6[r] = step0 + the lowest j that attains it over the rows of this launch and, unless
// `first`, what o6 / a6 held; ovm / avm likewise for the von Mises stress of every node: ovm holds vm^2 between the launches
// of a call and the root after the `last`.  (amdgpu_waves_per_eu: the budget of three waves on a SIMD, 168 VGPRs, stated;
// at eight panels and two rows the kernel takes 157)
template <int P, int S>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3)))
void k_stress_transient(int N, int n_rows, int step0, int first, int last, const double *__restrict__ T, size_t pstride,
                        const double *__restrict__ ts, const double *__restrict__ coef, const double *__restrict__ g,
                        double *__restrict__ o6, int *__restrict__ a6, double *__restrict__ ovm, int *__restrict__ avm)
{
  const StressLane L = stress_lane(N);
  double x[MC * P];
  load_mode_values<P>(T, pstride, L.r, L.in, x);
  const double t0 = L.in ? ts[L.r] : 0.0;
  const double w = L.normal ? 1.5 : 3.0;
  double best = -1.0, vbest = -1.0;
  int at = 0, vat = 0;
  if (!first && L.in) {
    best = o6[L.r]; at = a6[L.r];
    if (L.leader) { vbest = ovm[L.node]; vat = avm[L.node]; }
  }
  // the per-row and per-node comparison of one table row
  auto take = [&](double u, int step) {
    const double m = fabs(u);
    if (m > best) { best = m; at = step; }
    const double p = node_mean(L, u);                                   // (every lane makes the moves: no branch around them)
    const double d = L.normal ? u - p : u;
    const double v = node_sum(L, w * d * d);
    if (v > vbest) { vbest = v; vat = step; }
  };
  int j = 0;
  if constexpr (S > 1) {
    for (; j + S <= n_rows; j += S) {
      const double *cr = coef + (size_t)j * ML;
      double u[S];
#pragma unroll
      for (int r = 0; r < S; ++r) u[r] = g[j + r] * t0;
#pragma unroll
      for (int k = 0; k < MC * P; ++k) {
#pragma unroll
        for (int r = 0; r < S; ++r) u[r] = fma(x[k], cr[r * ML + k], u[r]);
      }
#pragma unroll
      for (int r = 0; r < S; ++r) take(u[r], step0 + j + r);
    }
  }
  for (; j < n_rows; ++j) {
    const double *cr = coef + (size_t)j * ML;                           // (uniform: scalar loads)
    double u = g[j] * t0;
#pragma unroll
    for (int k = 0; k < MC * P; ++k) u = fma(x[k], cr[k], u);
    take(u, step0 + j);
  }
  if (L.in) {
    o6[L.r] = best; a6[L.r] = at;
    if (L.leader) { ovm[L.node] = last ? sqrt(vbest) : vbest; avm[L.node] = vat; }
  }
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
// The cycle peak of the von Mises stress of re cos wt - im sin wt, in the kernel's arithmetic: deviators first, the shares
// summed over the fixed tree
double harmonic_von_mises(const double re6[6], const double im6[6])
{
  const double pr = (re6[0] + re6[1] + re6[2]) * (1.0 / 3.0), pi = (im6[0] + im6[1] + im6[2]) * (1.0 / 3.0);
  double a[6], b[6], m[6];
  for (int c = 0; c < 6; ++c) {
    const double w = c < 3 ? 1.5 : 3.0;
    const double dr = c < 3 ? re6[c] - pr : re6[c], di = c < 3 ? im6[c] - pi : im6[c];
    a[c] = w * dr * dr; b[c] = w * di * di; m[c] = w * dr * di;
  }
  auto tree = [](const double *y) { return ((y[0] + y[3]) + (y[1] + y[4])) + (y[2] + y[5]); };
  const double A = tree(a), B = tree(b), Cm = tree(m);
  const double h = 0.5 * (A + B), d = 0.5 * (A - B);
  return std::sqrt(h + std::sqrt(std::fma(d, d, Cm * Cm)));
}

// the table and the two index arrays, on the first call
static int ensure_stress_sweep(feahip_ctx *c)
{
  StressState &S = c->stress;
  if (S.d_scoef) return FEAHIP_OK;
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_scoef, sizeof(double) * (size_t)FEA_RESPONSE_MAX_FREQ * 2 * ML));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_at6, sizeof(int) * 6 * (size_t)c->N));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_vmat, sizeof(int) * (size_t)c->N));
  return FEAHIP_OK;
}

static void enq_stress_sweep(feahip_ctx *c, int n_freq)
{
  StressState &S = c->stress;
  for_panels(panels_of(c), [&](auto P) {
    hipLaunchKernelGGL((k_stress_sweep<decltype(P)::value>), stress_sweep_grid(c), dim3(256), 0, c->stream, c->N, n_freq,
                       (const double *)S.d_store, (size_t)6 * c->N * MC, (const double *)S.d_ts, (const double *)S.d_scoef,
                       S.d_out6, S.d_at6, S.d_vm, S.d_vmat);
  });
}

static void enq_stress_transient(feahip_ctx *c, int n_rows, int step0, int first, int last)
{
  StressState &S = c->stress;
  for_panels(panels_of(c), [&](auto P) {
    constexpr int PP = decltype(P)::value;
    hipLaunchKernelGGL((k_stress_transient<PP, STRESS_SWEEP_STEPS_OF(PP)>), stress_sweep_grid(c), dim3(256), 0, c->stream, c->N,
                       n_rows, step0, first, last, (const double *)S.d_store, (size_t)6 * c->N * MC, (const double *)S.d_ts,
                       (const double *)S.d_scoef, (const double *)chunk_g(S.d_scoef), S.d_out6, S.d_at6, S.d_vm, S.d_vmat);
  });
}

// the four outputs in library ids, behind the launches in stream order
static int read_stress_peaks(feahip_ctx *c, double *h_peak6, int *h_at6, double *h_vm, int *h_vmat)
{
  StressState &S = c->stress;
  const size_t N = (size_t)c->N;
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_peak6, S.d_out6, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_at6, S.d_at6, sizeof(int) * 6 * N, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_vm, S.d_vm, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_vmat, S.d_vmat, sizeof(int) * N, hipMemcpyDeviceToHost, c->stream));
  return FEAHIP_OK;
}

// the table of response_sweep on the stress rows: h_peak6 / h_at6 [6N], h_vm / h_vmat [N] in library ids, the probes'
// curves [n_probe][n_freq][6] (probe in library node ids)
int stress_sweep(feahip_ctx *c, int n_freq, const double *omega, double alpha, double beta, const double *zeta, double *h_peak6,
                 int *h_at6, double *h_vm, int *h_vmat, int n_probe, const int *probe, double *probe_re, double *probe_im)
{
  ModalState &M = c->modal;
  ResponseState &R = c->response;
  StressState &S = c->stress;
  std::vector<double> coef((size_t)n_freq * 2 * ML);
  std::string why;
  if (response_coefficients(M.n_locked, M.lam, R.q, M.lock_order, n_freq, omega, alpha, beta, zeta, R.correction, coef.data(), &why)) {
    c->err = "response_stress_sweep: " + why;
    return FEAHIP_EINVAL;
  }
  int rc;
  if ((rc = ensure_stress_sweep(c))) return rc;
  S.swept_freq = 0;
  S.trans_rows = 0;
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.d_scoef, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice, c->stream));
  enq_stress_sweep(c, n_freq);
  FEA_HIP_CHECK(c, hipGetLastError());
  if ((rc = read_stress_peaks(c, h_peak6, h_at6, h_vm, h_vmat))) return rc;
  StressProbeRows rows;
  if ((rc = rows.read(c, n_probe, probe))) return rc;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  S.swept_freq = n_freq;
  S.table_gen = M.lock_gen;
  for (int r = 0; r < n_probe; ++r)
    for (int j = 0; j < n_freq; ++j) {
      const double *cr = coef.data() + (size_t)j * 2 * ML;
      for (int e = 0; e < 6; ++e) {
        probe_re[((size_t)r * n_freq + j) * 6 + e] = rows.sum(r, e, cr, 1.0);
        probe_im[((size_t)r * n_freq + j) * 6 + e] = rows.sum(r, e, cr + ML, 0.0);
      }
    }
  return FEAHIP_OK;
}

// the chunked launches of k_stress_transient over the whole displacement history (transient_stream.h): the probes'
// histories [n_probe][n_steps + 1][6]
int stress_transient(feahip_ctx *c, int n_steps, double dt, const double *g, double alpha, double beta, const double *zeta,
                     double *h_peak6, int *h_at6, double *h_vm, int *h_vmat, int n_probe, const int *probe, double *h_probe)
{
  StressState &S = c->stress;
  const int n_rows = n_steps + 1;
  TransientStream T;
  int rc;
  if ((rc = T.open(c, "response_stress_transient", n_steps, dt, g, alpha, beta, zeta, 0, true, 0)) || (rc = ensure_stress_sweep(c)))
    return rc;
  S.swept_freq = 0;
  S.trans_rows = 0;
  StressProbeRows rows;                                                // read back once
  if ((rc = rows.read(c, n_probe, probe))) return rc;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  // the probes' values, taken from a chunk as the host fills it
  auto on_host = [&](int step0, int count, const double *coef, const double *gs) {
    for (int r = 0; r < n_probe; ++r)
      for (int j = 0; j < count; ++j)
        for (int e = 0; e < 6; ++e)
          h_probe[((size_t)r * n_rows + step0 + j) * 6 + e] = rows.sum(r, e, coef + (size_t)j * ML, gs[j]);
  };
  auto launch = [&](int count, int step0, bool first, bool last) { enq_stress_transient(c, count, step0, first, last); };
  if ((rc = T.pass(S.d_scoef, true, on_host, launch)) || (rc = read_stress_peaks(c, h_peak6, h_at6, h_vm, h_vmat))) return rc;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  S.trans_rows = T.last_count;
  S.trans_step0 = T.last_step0;
  S.table_gen = c->modal.lock_gen;
  return FEAHIP_OK;
}

// hooks of feahip_time_kernel: 29 the sweep over the table of the last feahip_response_stress_sweep, 30 the last chunk of
// the last feahip_response_stress_transient as a first and last launch
int time_stress_sweep_kernel(feahip_ctx *c, int what)
{
  if (what == 29) enq_stress_sweep(c, c->stress.swept_freq);
  else enq_stress_transient(c, c->stress.trans_rows, c->stress.trans_step0, 1, 1);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
