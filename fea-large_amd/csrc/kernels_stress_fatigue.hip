// kernels_stress_fatigue.hip -- random-vibration fatigue on the stress store, on gfx950: the spectral moments m0, m1, m2, m4 of
// seven stress processes per node -- the six components and the equivalent von Mises process of Preumont and Piefort,
// whose PSD is trace(V G_sigma(w)), so that its moments are the von Mises combination of the nine forms -- and from them
// the rates of zero up-crossings and of peaks and the damage per unit time on an S-N curve (fatigue_point.h).
//
// A moment of order n of a linear combination y = L T_a is the form (C_n, b_n, s_n) of feahip_host_moment_form on y, as
// k_stress_combine (kernels_stress_combine.hip) evaluates one form: the same loads, the same stress_form, the same
// fma(3.0, qs, 0.5 * qn) for the von Mises combination -- without the root.
//   k_stress_moments<P, RESIDENT>  the body of k_stress_combine<P, false> on four forms, two ways:
//                         RESIDENT = false: the FORM is the grid's second dimension.  The table pointer form + blockIdx.y *
//                         FEA_COMBINE_TABLE is uniform over the workgroup and invariant in the loop over the nine
//                         combinations, so the table's loads stay scalar and hoisted as they are there; the store is read
//                         four times (by four workgroups).
//                         RESIDENT = true: a combination's 8 P values stay in registers and run against the four tables
//                         in turn.  The store is read once, but the tables' loads are issued per combination.
//                         Measured on the bench's block: reading the store once wins up to five
//                         panels (2.2 times at one, 1.1 at five), the hoisted tables win from six on (1.8 times at
//                         eight); the host picks by the panel count (FEA_MOMENTS_RESIDENT_MAX).  The bits are the same
//                         either way.
//                           mom[n][a][k] = max(0, q_n(T_a,k)) for k < 6,  mom[n][a][6] = max(0, (q_n(xx-yy) + ...) / 2 + 3 (...))
//   k_fatigue_rates       pointwise, a lane per (node, process) pair: its four moments (coalesced: mom[n] is [7N]), then
//                         rates[2], damage[3] and the status.
// The four tables are a buffer of this file's own: the form of the last feahip_response_stress_combine stays (hook 28).
// No atomics, the same bits on every call.  A context that never calls a fatigue entry allocates and launches nothing here.
#include "fatigue_point.h"
#include "stress_form.h"

// Which k_stress_moments a panel count gets: the resident one up to this many panels, the one with the form on the grid
// above (measured on the bench's block).  0 and 8 force one of them for a measurement (`make variant`)
#ifndef FEA_MOMENTS_RESIDENT_MAX
#define FEA_MOMENTS_RESIDENT_MAX 5
#endif

// A workgroup takes 256 consecutive nodes and one of the four forms (RESIDENT: all four)
template <int P, bool RESIDENT>
__global__ __launch_bounds__(256)
void k_stress_moments(int N, const double *__restrict__ T, size_t pstride, const double *__restrict__ ts,
                      const double *__restrict__ forms, double *__restrict__ mom)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  const bool in = a < N;
  const int r = in ? 6 * a : 0;
  constexpr int NF = RESIDENT ? 4 : 1;                                 // the forms a lane evaluates
  const int f0 = RESIDENT ? 0 : blockIdx.y;
  const double *__restrict__ form = forms + (size_t)f0 * FEA_COMBINE_TABLE;
  double *__restrict__ out = mom + ((size_t)f0 * N + (in ? a : 0)) * 7;   // form f of this node: out + f * 7 N
  double qn[NF], qs[NF];                                               // the forms of the three differences, of the three shears
#pragma unroll
  for (int f = 0; f < NF; ++f) qn[f] = qs[f] = 0.0;
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    double x[MC * P], u0;
    if (k < 6) {
      load_mode_values<P, false>(T, pstride, r + k, in, x);
      u0 = in ? ts[r + k] : 0.0;
    } else {
      const int c0 = k - 6, c1 = c0 == 2 ? 0 : c0 + 1;
      load_mode_difference<P>(T, pstride, r + c0, r + c1, in, x);
      u0 = in ? ts[r + c0] - ts[r + c1] : 0.0;
    }
#pragma unroll 1
    for (int f = 0; f < NF; ++f) {
      const double v = stress_form<P>(x, u0, form + (size_t)f * FEA_COMBINE_TABLE);
      if (k < 6) {
        if (in) out[(size_t)f * 7 * N + k] = fmax(v, 0.0);
        if (k >= 3) qs[f] += v;
      } else
        qn[f] += v;
    }
  }
  if (in)
    for (int f = 0; f < NF; ++f) out[(size_t)f * 7 * N + 6] = fmax(fma(3.0, qs[f], 0.5 * qn[f]), 0.0);
}

// n = 7 N pairs; mom[4][n]; rates[n][2], damage[n][3], status[n]
__global__ __launch_bounds__(256)
void k_fatigue_rates(int n, const double *__restrict__ mom, FatigueConsts<double> k, double *__restrict__ rates,
                     double *__restrict__ damage, int *__restrict__ status)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double m[4] = {mom[i], mom[(size_t)n + i], mom[2 * (size_t)n + i], mom[3 * (size_t)n + i]};
  double r[2], d[3];
  status[i] = fatigue_point<double>(m, k, r, d);
  rates[2 * (size_t)i] = r[0]; rates[2 * (size_t)i + 1] = r[1];
  damage[3 * (size_t)i] = d[0]; damage[3 * (size_t)i + 1] = d[1]; damage[3 * (size_t)i + 2] = d[2];
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
static int fatigue_ensure(feahip_ctx *c)
{
  FatigueState &F = c->fatigue;
  if (F.d_forms) return FEAHIP_OK;
  const size_t n = 7 * (size_t)c->N;
  FEA_HIP_CHECK(c, hipMalloc((void **)&F.d_forms, sizeof(double) * 4 * FEA_COMBINE_TABLE));
  FEA_HIP_CHECK(c, hipMalloc((void **)&F.d_mom, sizeof(double) * 4 * n));
  FEA_HIP_CHECK(c, hipMalloc((void **)&F.d_rates, sizeof(double) * 2 * n));
  FEA_HIP_CHECK(c, hipMalloc((void **)&F.d_damage, sizeof(double) * 3 * n));
  FEA_HIP_CHECK(c, hipMalloc((void **)&F.d_status, sizeof(int) * n));
  return FEAHIP_OK;
}

static void enq_stress_moments(feahip_ctx *c)
{
  StressState &S = c->stress;
  FatigueState &F = c->fatigue;
  const unsigned blocks = (c->N + 255) / 256;
  for_panels(panels_of(c), [&](auto P) {
    constexpr int p = decltype(P)::value;
    constexpr bool resident = p <= FEA_MOMENTS_RESIDENT_MAX;
    hipLaunchKernelGGL((k_stress_moments<p, resident>), resident ? dim3(blocks) : dim3(blocks, 4), dim3(256), 0, c->stream, c->N,
                       (const double *)S.d_store, (size_t)6 * c->N * MC, (const double *)S.d_ts, (const double *)F.d_forms, F.d_mom);
  });
}

static void enq_fatigue_rates(feahip_ctx *c)
{
  FatigueState &F = c->fatigue;
  const int n = 7 * c->N;
  FatigueConsts<double> k;
  k.b = F.consts[0]; k.inv_a = F.consts[1]; k.gamma_b = F.consts[2]; k.gamma_hb = F.consts[3]; k.two_hb = F.consts[4];
  hipLaunchKernelGGL(k_fatigue_rates, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, (const double *)F.d_mom, k, F.d_rates,
                     F.d_damage, F.d_status);
}

// four forms by ascending mode: C4[4][n][n], b4[4][n] (null: zero), s4[4] (null: zero); h_mom[4][N][7] in library ids (null: not
// wanted).  The moments stay on the device for stress_fatigue_rates and hook 32
int stress_moments(feahip_ctx *c, const double *C4, const double *b4, const double *s4, double *h_mom)
{
  ModalState &M = c->modal;
  FatigueState &F = c->fatigue;
  int rc;
  if ((rc = fatigue_ensure(c))) return rc;
  const int n = M.n_locked;
  std::vector<double> T4;
  T4.reserve(4 * (size_t)FEA_COMBINE_TABLE);
  for (int k = 0; k < 4; ++k) {
    const std::vector<double> T = folded_form(M, C4 + (size_t)k * n * n, b4 ? b4 + (size_t)k * n : nullptr, s4 ? s4[k] : 0.0);
    T4.insert(T4.end(), T.begin(), T.end());
  }
  F.forms_set = F.mom_set = F.rates_set = false;
  // (pageable memory: the copy has left T4 when the call returns)
  FEA_HIP_CHECK(c, hipMemcpyAsync(F.d_forms, T4.data(), sizeof(double) * T4.size(), hipMemcpyHostToDevice, c->stream));
  enq_stress_moments(c);
  FEA_HIP_CHECK(c, hipGetLastError());
  if (h_mom) FEA_HIP_CHECK(c, hipMemcpyAsync(h_mom, F.d_mom, sizeof(double) * 28 * (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  F.forms_set = F.mom_set = true;
  return FEAHIP_OK;
}

// the statistics of the moments held on the S-N curve whose constants are k[5] (fatigue_constants); h_rates[N][7][2],
// h_damage[N][7][3], h_status[N][7] in library ids, each null where not wanted
int stress_fatigue_rates(feahip_ctx *c, const double *k, double *h_rates, double *h_damage, int *h_status)
{
  FatigueState &F = c->fatigue;
  const size_t n = 7 * (size_t)c->N;
  F.rates_set = false;
  for (int e = 0; e < 5; ++e) F.consts[e] = k[e];
  enq_fatigue_rates(c);
  FEA_HIP_CHECK(c, hipGetLastError());
  if (h_rates) FEA_HIP_CHECK(c, hipMemcpyAsync(h_rates, F.d_rates, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
  if (h_damage) FEA_HIP_CHECK(c, hipMemcpyAsync(h_damage, F.d_damage, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, c->stream));
  if (h_status) FEA_HIP_CHECK(c, hipMemcpyAsync(h_status, F.d_status, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  F.rates_set = true;
  return FEAHIP_OK;
}

// hook 31 of feahip_time_kernel: k_stress_moments over the last four forms, the stress store and the T_s in force
int time_stress_moments(feahip_ctx *c)
{
  enq_stress_moments(c);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// hook 32: k_fatigue_rates over the last moments and the last S-N curve
int time_fatigue_rates(feahip_ctx *c)
{
  enq_fatigue_rates(c);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
