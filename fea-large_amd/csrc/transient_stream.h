// transient_stream.h -- the host side of a transient that goes to the device FEA_TRANSIENT_CHUNK rows at a time, one owner
// for response_transient (kernels_transient.hip), stress_transient (kernels_stress_sweep.hip) and stress_rainflow
// (kernels_stress_rainflow.hip).  A chunk on the device is [CHUNK][64] coefficients, then g[CHUNK] (chunk_g); on the host
// its `count` rows stand packed with their g behind them.  The stream builds the rows (transient_table.cpp), copies a chunk,
// has the caller launch on it and fills the next chunk under the running one.  Two host buffers take turns, each behind the
// event of its last copy; or, within a byte limit, the whole table is kept and a later pass replays it.
#pragma once
#include "superpose.h"
#include <algorithm>
#include <string>

// the chunk's rows and their g share the table of a frequency sweep where that is the buffer they go through
static_assert((size_t)FEA_TRANSIENT_CHUNK * (ML + 1) <= (size_t)FEA_RESPONSE_MAX_FREQ * 2 * ML,
              "a chunk and its g fit the coefficient table of the sweeps");

// the g of a chunk in the device buffer that holds its rows
static inline double *chunk_g(double *d_coef) { return d_coef + (size_t)FEA_TRANSIENT_CHUNK * ML; }

namespace {
struct TransientStream {
  int last_count = 0, last_step0 = 0;  // the last chunk launched: what the hooks of feahip_time_kernel time

  ~TransientStream()
  {
    for (hipEvent_t e : copied) if (e) (void)hipEventDestroy(e);
    if (table) transient_end(table);
  }

  // transient_check (FEAHIP_EINVAL and "who: why" for what it refuses) and transient_begin on the modes and the load held,
  // then the host buffers.  with_g: the g column is g[step], otherwise zero (no static term).  A table of at most
  // cache_limit bytes is kept whole for the later passes; 0: two buffers
  int open(feahip_ctx *ctx, const char *who_, int n_steps_, double dt_, const double *g_, double alpha_, double beta_,
           const double *zeta_, int quantity_, bool with_g_, size_t cache_limit)
  {
    c = ctx; who = who_; n_steps = n_steps_; dt = dt_; g = g_; alpha = alpha_; beta = beta_; zeta = zeta_;
    quantity = quantity_; with_g = with_g_;
    const ModalState &M = c->modal;
    std::string why;
    if (transient_check(M.n_locked, M.lam, c->response.q, n_steps, dt, g, alpha, beta, zeta, c->response.correction, quantity, &why))
      return refuse(why);
    begin();
    n_rows = n_steps + 1;
    n_chunks = (n_rows + FEA_TRANSIENT_CHUNK - 1) / FEA_TRANSIENT_CHUNK;
    chunk_doubles = (size_t)std::min(FEA_TRANSIENT_CHUNK, n_rows) * (ML + 1);
    cached = (size_t)n_rows * (ML + 1) * sizeof(double) <= cache_limit;
    host.resize((cached ? (size_t)n_chunks : 2) * chunk_doubles);
    if (!cached)
      for (hipEvent_t &e : copied) FEA_HIP_CHECK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return FEAHIP_OK;
  }

  // One pass over all chunks through d_coef.  A pass that builds its chunks -- the first, and every one without the cache
  // -- calls on_host(step0, count, coef, gs) on each filled chunk if with_host.  Every pass calls
  // launch(count, step0, first, last) behind the chunk's copies.  The caller's stream is synchronised before an error
  // return from a fill, which may have launches in front of it
  template <class OnHost, class Launch>
  int pass(double *d_coef, bool with_host, OnHost &&on_host, Launch &&launch)
  {
    const int CH = FEA_TRANSIENT_CHUNK;
    const bool build = !cached || fresh;
    auto fill = [&](int kc) -> int {
      const int step0 = kc * CH, count = std::min(CH, n_rows - step0);
      double *coef = chunk(kc), *gs = coef + (size_t)count * ML;
      if (recorded[kc & 1]) FEA_HIP_CHECK(c, hipEventSynchronize(copied[kc & 1]));   // the buffer's last copy has to be over
      std::string why;
      if (transient_rows(table, g, count, coef, &why)) return refuse(why);
      for (int j = 0; j < count; ++j) gs[j] = with_g ? g[step0 + j] : 0.0;
      if (with_host) on_host(step0, count, (const double *)coef, (const double *)gs);
      return FEAHIP_OK;
    };
    int rc;
    if (build) {
      if (!fresh) { transient_end(table); begin(); }                     // (a pass before this one walked the table to its end)
      fresh = false;
      if ((rc = fill(0))) { (void)hipStreamSynchronize(c->stream); return rc; }
    }
    for (int kc = 0; kc < n_chunks; ++kc) {
      const int step0 = kc * CH, count = std::min(CH, n_rows - step0);
      const double *src = chunk(kc);
      FEA_HIP_CHECK(c, hipMemcpyAsync(d_coef, src, sizeof(double) * (size_t)count * ML, hipMemcpyHostToDevice, c->stream));
      FEA_HIP_CHECK(c, hipMemcpyAsync(chunk_g(d_coef), src + (size_t)count * ML, sizeof(double) * (size_t)count,
                                      hipMemcpyHostToDevice, c->stream));
      if (!cached) { FEA_HIP_CHECK(c, hipEventRecord(copied[kc & 1], c->stream)); recorded[kc & 1] = true; }
      launch(count, step0, kc == 0, kc == n_chunks - 1);
      FEA_HIP_CHECK(c, hipGetLastError());
      last_count = count; last_step0 = step0;
      // the next chunk on the host while this one runs
      if (build && kc + 1 < n_chunks && (rc = fill(kc + 1))) { (void)hipStreamSynchronize(c->stream); return rc; }
    }
    return FEAHIP_OK;
  }

private:
  feahip_ctx *c = nullptr;
  const char *who = "";
  int n_steps = 0, quantity = 0, n_rows = 0, n_chunks = 0;
  double dt = 0.0, alpha = 0.0, beta = 0.0;
  const double *g = nullptr, *zeta = nullptr;
  bool with_g = true, cached = false, fresh = false;
  TransientTable *table = nullptr;     // at step 0 while `fresh`
  size_t chunk_doubles = 0;
  std::vector<double> host;            // chunk kc at kc chunk_doubles (cached), or (kc & 1) chunk_doubles
  hipEvent_t copied[2] = {nullptr, nullptr};   // behind the last copy out of either buffer
  bool recorded[2] = {false, false};

  double *chunk(int kc) { return host.data() + (size_t)(cached ? kc : kc & 1) * chunk_doubles; }
  int refuse(const std::string &why) { c->err = std::string(who) + ": " + why; return FEAHIP_EINVAL; }
  void begin()
  {
    const ModalState &M = c->modal;
    table = transient_begin(M.n_locked, M.lam, c->response.q, M.lock_order, n_steps, dt, alpha, beta, zeta, c->response.correction, quantity);
    fresh = true;
  }
};
}
