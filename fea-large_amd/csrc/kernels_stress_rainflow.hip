// kernels_stress_rainflow.hip -- the rainflow count of a transient on the stress store, on gfx950: for every stress row the
// cycles ASTM E1049-85's three-point rule counts over the rows of a coefficient table, and Miner's sum on an S-N curve
// (rainflow_point.h has the rule, one copy for this kernel and for feahip_host_rainflow).
//
// The count is sequential in time and independent across the 6N stress rows, which is the layout of k_stress_transient
// (stress_form.h: a lane owns a stress row, ten nodes per wave, lanes 60 to 63 idle, four waves per workgroup).  Per table
// row a lane runs the FMA chain of k_stress_transient -- g T_s + sum_k T_k a_k, one fma per store column in ascending
// order, so the six components have its bits -- and hands the value to its counter.  There are no cross-lane moves.
//   the stack   a ring of `depth` points per row in device memory, laid out [depth][6N] so that lanes at the same slot
//               coalesce, addressed through the lane's base and count; it persists between the launches of a call.  No
//               private array is indexed at run time, so nothing goes to scratch memory.
//   the state   per row, between launches: the last kept sample, the direction, the ring's base and count, the damage, the
//               cycles, the largest range, the depth used, the status (RainflowBuffers::d_real, d_int).  The first launch
//               of a pass starts it, the last one pushes the final reversal and counts the residue.
//   the passes  pass 0 counts the six components.  Pass 1 + q counts the projections 6 q .. 6 q + 5: lane c of a node
//               forms x[k] = sum_e proj[6 q + c][e] T_k[a][e], one fma per component in ascending order from 0, and T_s
//               likewise, in the prologue -- a projection is linear in the store -- and then runs the same chain.  The
//               passes are the outer loop on the host, the chunks of FEA_TRANSIENT_CHUNK rows the inner one; a pass
//               reuses the state buffers of the one before, whose results the host has read by then.
//   the power   two instances per panel count: a whole exponent b squares and multiplies (RainflowIntPower), any other takes
//               pow (RainflowPower), which costs some sixty VGPRs beside the lane's 8 P values: 182 against 256 and 16 in
//               AGPRs at eight panels, two waves on a SIMD against one (DESIGN.md section 27 has both measured).
// The host builds the coefficient chunks once per call and keeps them for the later passes where the whole table fits
// RAINFLOW_TABLE_CACHE bytes; above that every pass builds its chunks again through the two buffers of transient_stream.h
// (`make variant NAME=rfnocache VSRC=kernels_stress_rainflow VFLAGS=-DRAINFLOW_TABLE_CACHE=0` takes every call that way).
// No LDS memory, no atomics, the same bits on every call.  A context that never calls the entry allocates and launches
// nothing here.
#include "stress_form.h"
#include "transient_stream.h"
#include "rainflow_point.h"

#ifndef RAINFLOW_TABLE_CACHE
#define RAINFLOW_TABLE_CACHE ((size_t)256 << 20)
#endif
#define RF_REAL 4                      // d_real: last, damage, cycles, max_range
#define RF_INT 6                       // d_int: dir, base, count, depth_used, status, seen

namespace {
// the ring of one row: slot s at p[s stride]
struct DeviceRing {
  double *p;
  size_t stride;
  __device__ __forceinline__ double get(int slot) const { return p[(size_t)slot * stride]; }
  __device__ __forceinline__ void set(int slot, double v) { p[(size_t)slot * stride] = v; }
};
struct NoList {
  __device__ __forceinline__ void operator()(double, double, double) const {}
};
}

// The count of the processes of one pass over the rows of this launch.  proj null: lane c of a node counts component c;
// otherwise the projection proj[c][6] of the node's six rows.  n_live <= 6 processes of the pass are counted.
template <int P, int S, class Curve>
__global__ __launch_bounds__(256)
void k_stress_rainflow(int N, int n_rows, int first, int last, const double *__restrict__ T, size_t pstride,
                       const double *__restrict__ ts, const double *__restrict__ coef, const double *__restrict__ g,
                       const double *__restrict__ proj, int n_live, Curve curve, int depth,
                       double *__restrict__ stack, double *__restrict__ real, int *__restrict__ ints)
{
  const StressLane L = stress_lane(N);
  const bool live = L.in && L.c < n_live;
  const size_t rows6 = (size_t)6 * N;
  double x[MC * P];
  double t0 = 0.0;
  if (!proj) {
    load_mode_values<P>(T, pstride, L.r, live, x);
    if (live) t0 = ts[L.r];
  } else {
#pragma unroll
    for (int e = 0; e < MC * P; ++e) x[e] = 0.0;
    if (live) {
      const double *w = proj + 6 * L.c;
      for (int e = 0; e < 6; ++e) {
        const double we = w[e];
        const int row = 6 * L.node + e;
#pragma unroll
        for (int p = 0; p < P; ++p) {
          double y[MC];
          load_mode_values<1>(T + (size_t)p * pstride, pstride, row, true, y);
#pragma unroll
          for (int a = 0; a < MC; ++a) x[p * MC + a] = fma(we, y[a], x[p * MC + a]);
        }
        t0 = fma(we, ts[row], t0);
      }
    }
  }
  RainflowState<double> st;
  rainflow_begin(st);
  if (!first && live) {
    st.last = real[L.r]; st.damage = real[rows6 + L.r]; st.cycles = real[2 * rows6 + L.r]; st.max_range = real[3 * rows6 + L.r];
    st.dir = ints[L.r]; st.base = ints[rows6 + L.r]; st.count = ints[2 * rows6 + L.r]; st.depth_used = ints[3 * rows6 + L.r];
    st.status = ints[4 * rows6 + L.r]; st.seen = ints[5 * rows6 + L.r];
  }
  DeviceRing ring{stack + L.r, rows6};
  NoList none;
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
      if (live) {
#pragma unroll
        for (int r = 0; r < S; ++r) rainflow_sample(st, u[r], depth, curve, ring, none);
      }
    }
  }
  for (; j < n_rows; ++j) {
    const double *cr = coef + (size_t)j * ML;                           // (uniform: scalar loads)
    double u = g[j] * t0;
#pragma unroll
    for (int k = 0; k < MC * P; ++k) u = fma(x[k], cr[k], u);
    if (live) rainflow_sample(st, u, depth, curve, ring, none);
  }
  if (live) {
    if (last) rainflow_end(st, depth, curve, ring, none);
    real[L.r] = st.last; real[rows6 + L.r] = st.damage; real[2 * rows6 + L.r] = st.cycles; real[3 * rows6 + L.r] = st.max_range;
    ints[L.r] = st.dir; ints[rows6 + L.r] = st.base; ints[2 * rows6 + L.r] = st.count; ints[3 * rows6 + L.r] = st.depth_used;
    ints[4 * rows6 + L.r] = st.status; ints[5 * rows6 + L.r] = st.seen;
  }
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
// the chunk, the projections and the row state on the first call; the stack on the first call and for a larger depth: the
// new one is allocated before the old one goes, so a failed growth leaves the buffers as they were
static int ensure_rainflow(feahip_ctx *c, int depth)
{
  RainflowBuffers &R = c->rainflow;
  const size_t rows6 = (size_t)6 * c->N;
  if (!R.d_coef) FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_coef, sizeof(double) * (size_t)FEA_TRANSIENT_CHUNK * (ML + 1)));
  if (!R.d_proj) FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_proj, sizeof(double) * FEA_RAINFLOW_MAX_PROJ * 6));
  if (!R.d_real) FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_real, sizeof(double) * RF_REAL * rows6));
  if (!R.d_int) FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_int, sizeof(int) * RF_INT * rows6));
  if (depth > R.depth_cap) {
    double *grown = nullptr;
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    FEA_HIP_CHECK(c, hipMalloc((void **)&grown, sizeof(double) * (size_t)depth * rows6));
    dev_free({R.d_stack});
    R.d_stack = grown;
    R.depth_cap = depth;
  }
  return FEAHIP_OK;
}

// one launch over the `count` rows in d_coef; proj (device) null for the component pass
static void enq_rainflow(feahip_ctx *c, int count, int first, int last, const double *d_proj, int n_live)
{
  StressState &S = c->stress;
  RainflowBuffers &R = c->rainflow;
  auto launch = [&](auto P, auto curve) {
    constexpr int PP = decltype(P)::value;
    hipLaunchKernelGGL((k_stress_rainflow<PP, STRESS_SWEEP_STEPS_OF(PP), decltype(curve)>), stress_sweep_grid(c), dim3(256), 0,
                       c->stream, c->N, count, first, last, (const double *)S.d_store, (size_t)6 * c->N * MC, (const double *)S.d_ts,
                       (const double *)R.d_coef, (const double *)chunk_g(R.d_coef), d_proj, n_live, curve, R.depth, R.d_stack,
                       R.d_real, R.d_int);
  };
  // a whole exponent takes the instance without pow (RainflowIntPower): 182 registers at eight panels where pow takes all 256
  const bool whole = R.sn[0] == (double)(int)R.sn[0];
  for_panels(panels_of(c), [&](auto P) {
    if (whole) launch(P, RainflowIntPower<double>{(int)R.sn[0], R.sn[1]});
    else launch(P, RainflowPower<double>{R.sn[0], R.sn[1]});
  });
}

int stress_rainflow(feahip_ctx *c, int n_steps, double dt, const double *g, double alpha, double beta, const double *zeta,
                    double sn_b, double sn_a, int depth, int n_proj, const double *proj, double *h_damage, double *h_cycles,
                    double *h_range, int *h_status, int *h_used, int n_probe, const int *probe, double *h_probe)
{
  RainflowBuffers &R = c->rainflow;
  const int n_rows = n_steps + 1, W = 6 + n_proj, passes = 1 + (n_proj + 5) / 6;
  const size_t rows6 = (size_t)6 * c->N;
  // the host keeps the whole table where later passes read it again and it fits
  TransientStream T;
  int rc;
  if ((rc = T.open(c, "response_stress_rainflow", n_steps, dt, g, alpha, beta, zeta, 0, true, passes > 1 ? RAINFLOW_TABLE_CACHE : 0)))
    return rc;
  double k[5];
  if (fatigue_constants(sn_b, sn_a, k)) { c->err = "response_stress_rainflow: the S-N curve was refused"; return FEAHIP_EINVAL; }
  R.rows = 0;                                                          // (nothing for hook 33 to time until this call is through)
  if ((rc = ensure_rainflow(c, depth))) return rc;
  R.depth = depth; R.sn[0] = k[0]; R.sn[1] = k[1];
  if (n_proj > 0)
    FEA_HIP_CHECK(c, hipMemcpyAsync(R.d_proj, proj, sizeof(double) * 6 * (size_t)n_proj, hipMemcpyHostToDevice, c->stream));
  StressProbeRows rows;                                                // read back once
  if ((rc = rows.read(c, n_probe, probe))) return rc;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  // the probes' rows of every projection, formed as the kernel's prologue forms them: [n_probe][n_proj][width + 1]
  const int width = rows.width;
  std::vector<double> prow((size_t)n_probe * n_proj * (width + 1), 0.0);
  for (int r = 0; r < n_probe; ++r)
    for (int p = 0; p < n_proj; ++p) {
      double *dst = prow.data() + ((size_t)r * n_proj + p) * (width + 1);
      for (int e = 0; e < 6; ++e) {
        const double *src = rows.rows.data() + ((size_t)r * 6 + e) * (width + 1);
        for (int col = 0; col <= width; ++col) dst[col] = std::fma(proj[6 * p + e], src[col], dst[col]);
      }
    }
  // the probes' values, taken from a chunk as the host fills it in the first pass
  auto on_host = [&](int step0, int count, const double *coef, const double *gs) {
    for (int r = 0; r < n_probe; ++r)
      for (int j = 0; j < count; ++j) {
        double *out = h_probe + ((size_t)r * n_rows + step0 + j) * W;
        const double *cr = coef + (size_t)j * ML;
        for (int e = 0; e < 6; ++e) out[e] = rows.sum(r, e, cr, gs[j]);
        for (int p = 0; p < n_proj; ++p) {
          const double *row = prow.data() + ((size_t)r * n_proj + p) * (width + 1);
          double y = gs[j] * row[width];
          for (int col = 0; col < width; ++col) y = std::fma(row[col], cr[col], y);
          out[6 + p] = y;
        }
      }
  };
  const bool want_real = h_damage || h_cycles || h_range, want_int = h_status || h_used;
  std::vector<double> preal(want_real ? 3 * rows6 : 0);               // one pass's results, scattered before the next pass's arrive
  std::vector<int> pint(want_int ? 2 * rows6 : 0);
  for (int pass = 0; pass < passes; ++pass) {
    const double *d_proj = pass == 0 ? nullptr : R.d_proj + (size_t)36 * (pass - 1);
    const int n_live = std::min(6, W - 6 * pass);
    auto launch = [&](int count, int, bool first, bool last) { enq_rainflow(c, count, first, last, d_proj, n_live); };
    if ((rc = T.pass(R.d_coef, pass == 0, on_host, launch))) return rc;
    // the pass's results, before the next pass starts the state again: process 6 pass + e of node a from row 6 a + e
    if (want_real)
      FEA_HIP_CHECK(c, hipMemcpyAsync(preal.data(), R.d_real + rows6, sizeof(double) * 3 * rows6, hipMemcpyDeviceToHost, c->stream));
    if (want_int)
      FEA_HIP_CHECK(c, hipMemcpyAsync(pint.data(), R.d_int + 3 * rows6, sizeof(int) * 2 * rows6, hipMemcpyDeviceToHost, c->stream));
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    const double *pr = preal.data();
    const int *pi = pint.data();
    for (size_t a = 0; a < (size_t)c->N; ++a)
      for (int e = 0; e < n_live; ++e) {
        const size_t src = 6 * a + e, dst = a * W + 6 * pass + e;
        if (h_damage) h_damage[dst] = pr[src];
        if (h_cycles) h_cycles[dst] = pr[rows6 + src];
        if (h_range) h_range[dst] = pr[2 * rows6 + src];
        if (h_used) h_used[dst] = pi[src];
        if (h_status) h_status[dst] = pi[rows6 + src];
      }
  }
  R.rows = T.last_count;
  R.step0 = T.last_step0;
  R.table_gen = c->modal.lock_gen;
  return FEAHIP_OK;
}

// hook 33 of feahip_time_kernel: the component pass over the last chunk of the last feahip_response_stress_rainflow, as a
// first and last launch
int time_rainflow_kernel(feahip_ctx *c)
{
  enq_rainflow(c, c->rainflow.rows, 1, 1, nullptr, 6);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
