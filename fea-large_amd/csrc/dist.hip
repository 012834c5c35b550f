// dist.hip -- row-sharded (multi-GPU) operation: shard installation, the RCCL
// transport, the Newton loop over one or more ranks.
//
// Production shape (bench.py, torch.distributed launch): one process per GPU,
// one context per process, halo rows over ncclSend/ncclRecv (point-to-point
// over xGMI; every rank talks to its slab neighbours only) and one to three
// doubles per ncclAllReduce.  No all-gather on the path; the only vector all-reduce is the coarse level's
// (preconditioner kind 2, coarse.h: at most 768 doubles per CG iteration, on the communication stream).
// The same loop also drives an in-process group of contexts (GroupTransport),
// which is how the sharded path is exercised where one process sees the GPU.
#include "feahip_internal.h"
#include <rccl/rccl.h>
#include <cmath>
#include <cstring>

// halo lists of a plan to the device, and the longest run of this rank's SpMV chunks whose rows touch no halo column:
// they can be multiplied while the halo rows are in flight (a slab has its halo-touching chunks at its two ends)
int install_plan(feahip_ctx *c, const ShardPlan &plan)
{
  c->rank = plan.rank; c->nranks = plan.nranks; c->row0 = plan.row0; c->row1 = plan.row1;
  {
    int best_lo = 0, best_hi = 0, lo = -1;
    for (int k = 0; k <= c->nchunks_local; ++k) {
      bool interior = false;
      if (k < c->nchunks_local) {
        interior = true;
        const int r0 = c->h_chunk[c->chunk0 + k], r1 = c->h_chunk[c->chunk0 + k + 1];
        for (int q = c->h_rowptr[r0]; q < c->h_rowptr[r1] && interior; ++q)
          if (c->h_colidx[q] < plan.row0 || c->h_colidx[q] >= plan.row1) interior = false;
      }
      if (interior) { if (lo < 0) lo = k; }
      else if (lo >= 0) { if (k - lo > best_hi - best_lo) { best_lo = lo; best_hi = k; } lo = -1; }
    }
    c->ichunk_lo = best_lo; c->ichunk_hi = best_hi;
    // what the overlapped exchange relies on, checked outright: no chunk of the interior range reads a halo column
    for (int k = best_lo; k < best_hi; ++k) {
      const int r0 = c->h_chunk[c->chunk0 + k], r1 = c->h_chunk[c->chunk0 + k + 1];
      for (int q = c->h_rowptr[r0]; q < c->h_rowptr[r1]; ++q)
        if (c->h_colidx[q] < plan.row0 || c->h_colidx[q] >= plan.row1) { c->err = "interior chunk range reads a halo column"; return FEAHIP_ESTATE; }
    }
  }
  c->peer = plan.peer; c->send_off = plan.send_off; c->recv_off = plan.recv_off;
  c->nsend = (int)plan.send_idx.size(); c->nrecv = (int)plan.recv_idx.size();
  for (void *p : {(void *)c->d_send_idx, (void *)c->d_recv_idx, (void *)c->d_send_buf, (void *)c->d_recv_buf})
    if (p) (void)hipFree(p);
  c->d_send_idx = c->d_recv_idx = nullptr; c->d_send_buf = c->d_recv_buf = nullptr;
  auto up = [&](int **dst, const std::vector<int> &v) -> int {
    FEA_HIP_CHECK(c, hipMalloc((void **)dst, sizeof(int) * (v.size() ? v.size() : 1)));
    if (!v.empty()) FEA_HIP_CHECK(c, hipMemcpy(*dst, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice));
    return FEAHIP_OK;
  };
  int rc;
  if ((rc = up(&c->d_send_idx, plan.send_idx))) return rc;
  if ((rc = up(&c->d_recv_idx, plan.recv_idx))) return rc;
  FEA_HIP_CHECK(c, hipMalloc((void **)&c->d_send_buf, sizeof(double) * 3 * (size_t)(c->nsend ? c->nsend : 1)));
  FEA_HIP_CHECK(c, hipMalloc((void **)&c->d_recv_buf, sizeof(double) * 3 * (size_t)(c->nrecv ? c->nrecv : 1)));
  return FEAHIP_OK;
}

int install_shard(feahip_ctx *c, int rank, int nranks)
{
  if (nranks < 1 || rank < 0 || rank >= nranks) { c->err = "bad shard (rank, nranks)"; return FEAHIP_EINVAL; }
  if (c->rank_own >= 0) {                                     // a rank context is its shard: nothing to cut
    if (rank == c->rank && nranks == c->nranks) return FEAHIP_OK;
    c->err = "a rank context (feahip_create_rank) holds one rank's sub-mesh and cannot be re-sharded";
    return FEAHIP_EINVAL;
  }
  const int nsuper = (c->nchunks + FEA_SUPER_CHUNKS - 1) / FEA_SUPER_CHUNKS;
  const int s0 = (int)((long long)nsuper * rank / nranks), s1 = (int)((long long)nsuper * (rank + 1) / nranks);
  c->chunk0 = s0 * FEA_SUPER_CHUNKS < c->nchunks ? s0 * FEA_SUPER_CHUNKS : c->nchunks;
  c->nchunks_local = (s1 * FEA_SUPER_CHUNKS < c->nchunks ? s1 * FEA_SUPER_CHUNKS : c->nchunks) - c->chunk0;
  if (!c->h_super_achunk.empty()) {
    c->achunk0 = c->h_super_achunk[s0];
    c->nachunks_local = c->h_super_achunk[s1] - c->achunk0;
  }
  ShardPlan plan;
  build_shard_plan(c->h_rowptr, c->h_colidx, c->h_chunk, rank, nranks, plan);
  if (plan.row0 != c->row0 || plan.row1 != c->row1) release_k(c);     // K is re-allocated for the new rows on next use
  return install_plan(c, plan);
}

// ---- RCCL ------------------------------------------------------------------
struct RcclTransport : Transport {
  ncclComm_t comm = nullptr;
  ~RcclTransport() override { if (comm) (void)ncclCommDestroy(comm); }
  int fail(feahip_ctx *c, const char *what, ncclResult_t r)
  {
    c->err = std::string(what) + ": " + ncclGetErrorString(r);
    return FEAHIP_ECOMM;
  }
  int exchange(std::vector<feahip_ctx *> &R, int which) override
  {
    feahip_ctx *c = R[0];
    int stride = (which == 2) ? 4 : 3;
    double *v = which == 0 ? c->d_p : (which == 1 ? c->d_u : c->d_x);
    extern void feahip_enq_pack(feahip_ctx *, double *, int);
    extern void feahip_enq_unpack(feahip_ctx *, double *, int);
    feahip_enq_pack(c, v, stride);
    ncclResult_t r = ncclGroupStart();
    if (r != ncclSuccess) return fail(c, "ncclGroupStart", r);
    for (size_t k = 0; k < c->peer.size(); ++k) {
      const size_t ns = (size_t)3 * (c->send_off[k + 1] - c->send_off[k]), nr = (size_t)3 * (c->recv_off[k + 1] - c->recv_off[k]);
      if (ns && (r = ncclSend(c->d_send_buf + (size_t)3 * c->send_off[k], ns, ncclDouble, c->peer[k], comm, c->stream)) != ncclSuccess)
        return fail(c, "ncclSend", r);
      if (nr && (r = ncclRecv(c->d_recv_buf + (size_t)3 * c->recv_off[k], nr, ncclDouble, c->peer[k], comm, c->stream)) != ncclSuccess)
        return fail(c, "ncclRecv", r);
    }
    if ((r = ncclGroupEnd()) != ncclSuccess) return fail(c, "ncclGroupEnd", r);
    feahip_enq_unpack(c, v, stride);
    return FEAHIP_OK;
  }
  // the same exchange on a stream of its own: pack on the context's stream, send / receive / unpack on the
  // communication stream, so that the product of the rows that touch no halo column runs meanwhile
  int exchange_begin(std::vector<feahip_ctx *> &R, int which) override
  {
    feahip_ctx *c = R[0];
    if (!c->comm_stream) {
      FEA_HIP_CHECK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
      FEA_HIP_CHECK(c, hipEventCreateWithFlags(&c->ev_packed, hipEventDisableTiming));
      FEA_HIP_CHECK(c, hipEventCreateWithFlags(&c->ev_unpacked, hipEventDisableTiming));
    }
    const int stride = (which == 2) ? 4 : 3;
    double *v = which == 0 ? c->d_p : (which == 1 ? c->d_u : (which == 2 ? c->d_x : c->d_z));
    extern void feahip_enq_pack(feahip_ctx *, double *, int);
    extern void feahip_enq_unpack_on(feahip_ctx *, double *, int, hipStream_t);
    feahip_enq_pack(c, v, stride);
    FEA_HIP_CHECK(c, hipEventRecord(c->ev_packed, c->stream));
    FEA_HIP_CHECK(c, hipStreamWaitEvent(c->comm_stream, c->ev_packed, 0));
    ncclResult_t r = ncclGroupStart();
    if (r != ncclSuccess) return fail(c, "ncclGroupStart", r);
    for (size_t k = 0; k < c->peer.size(); ++k) {
      const size_t ns = (size_t)3 * (c->send_off[k + 1] - c->send_off[k]), nr = (size_t)3 * (c->recv_off[k + 1] - c->recv_off[k]);
      if (ns && (r = ncclSend(c->d_send_buf + (size_t)3 * c->send_off[k], ns, ncclDouble, c->peer[k], comm, c->comm_stream)) != ncclSuccess)
        return fail(c, "ncclSend", r);
      if (nr && (r = ncclRecv(c->d_recv_buf + (size_t)3 * c->recv_off[k], nr, ncclDouble, c->peer[k], comm, c->comm_stream)) != ncclSuccess)
        return fail(c, "ncclRecv", r);
    }
    if ((r = ncclGroupEnd()) != ncclSuccess) return fail(c, "ncclGroupEnd", r);
    feahip_enq_unpack_on(c, v, stride, c->comm_stream);
    FEA_HIP_CHECK(c, hipEventRecord(c->ev_unpacked, c->comm_stream));
    return FEAHIP_OK;
  }
  int exchange_end(std::vector<feahip_ctx *> &R) override
  {
    feahip_ctx *c = R[0];
    FEA_HIP_CHECK(c, hipStreamWaitEvent(c->stream, c->ev_unpacked, 0));
    return FEAHIP_OK;
  }
  int allreduce(std::vector<feahip_ctx *> &R, int slot, int n) override
  {
    feahip_ctx *c = R[0];
    ncclResult_t r = ncclAllReduce(c->d_scal + 8 + slot, c->d_scal + 8 + slot, (size_t)n, ncclDouble, ncclSum, comm, c->stream);
    if (r != ncclSuccess) return fail(c, "ncclAllReduce", r);
    return FEAHIP_OK;
  }
  int allreduce_max(std::vector<feahip_ctx *> &R, int slot, int n) override
  {
    feahip_ctx *c = R[0];
    ncclResult_t r = ncclAllReduce(c->d_scal + 8 + slot, c->d_scal + 8 + slot, (size_t)n, ncclDouble, ncclMax, comm, c->stream);
    if (r != ncclSuccess) return fail(c, "ncclAllReduce (max)", r);
    return FEAHIP_OK;
  }
  int allreduce_vec(std::vector<feahip_ctx *> &R, size_t n, bool comm) override
  {
    feahip_ctx *c = R[0];
    ncclResult_t r = ncclAllReduce(c->d_vred, c->d_vred, n, ncclDouble, ncclSum, this->comm, comm ? c->comm_stream : c->stream);
    if (r != ncclSuccess) return fail(c, "ncclAllReduce (vector)", r);
    return FEAHIP_OK;
  }
};

int rccl_unique_id(void *out, int cap)
{
  if (!out || cap < (int)sizeof(ncclUniqueId)) return FEAHIP_EINVAL;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return FEAHIP_ECOMM;
  memcpy(out, &id, sizeof(id));
  return (int)sizeof(id);
}

Transport *make_rccl_transport(feahip_ctx *c, int rank, int nranks, const void *unique_id, std::string &err)
{
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  RcclTransport *t = new RcclTransport();
  (void)hipSetDevice(c->device);
  ncclResult_t r = ncclCommInitRank(&t->comm, nranks, id, rank);
  if (r != ncclSuccess) { err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r); delete t; return nullptr; }
  return t;
}

// ---- the loop of solve() over one or more ranks -------------------------------
int dist_newton(std::vector<feahip_ctx *> &R, int load_increments, int max_newton, int modified_newton,
                double desired_tolerance, int solver_type, double solver_tolerance, int solver_max_iter,
                double *tol_log, int tol_log_cap, int *its_log, int *steps_done)
{
  int rc, nlog = 0, step = 0;
#define EACH(call) for (feahip_ctx *c : R) { if ((rc = (call))) return rc; }
  for (; step < load_increments; ++step) {                           // fea_solver.c:163
    int it = 0;
    double tolerance = 0;
    EACH(feahip_update_nodes_with_bc(c, 1.0));                        // :168 (prescribed values are replicated)
    EACH(feahip_update_state(c, nullptr));                            // :171-174
    EACH(feahip_create_stiffness(c));                                 // :177 (owned rows, ghost elements recomputed)
    if (modified_newton) EACH(feahip_stash_stiffness(c));             // :179
    do {
      it++;
      if (modified_newton) {
        EACH(feahip_create_residual_forces(c));                       // :185
        EACH(feahip_restore_stiffness(c));                            // :194-195
      } else if (it == 1) {
        EACH(feahip_create_residual_forces(c));                       // K of :177 is current
      } else {
        EACH(feahip_create_stiffness_and_residual(c));                // :185 + :200
      }
      EACH(feahip_apply_prescribed_bc(c, 0.0));                       // :203
      if ((rc = dist_solve_pcg(R, solver_type, solver_tolerance, solver_max_iter, nullptr, nullptr))) return rc;  // :205
      if ((rc = dist_energy(R, &tolerance))) return rc;               // :208-210, identical on every rank
      if (tol_log && nlog < tol_log_cap) tol_log[nlog] = tolerance;
      nlog++;
      const int ls_max = R[0]->linesearch_max;
      if (ls_max <= 0) {
        if ((rc = dist_update_nodes_with_solution(R, nullptr))) return rc;   // :216
      } else {
        // Golden-section search for the step length eta in [1/2, 1] that minimises |eta <u, R(x + eta u)>|
        // (solver-prototype/cartesian3d/large/cartesian3d_large.m:85-119; the C solver parses
        // line-search :max and never uses it, fea_solver.c:1517).  Two residual assemblies per iteration.
        const double tau = (sqrt(5.0) - 1.0) / 2.0;
        double a = 0.5, b = 1.0, eta = 1.0, at = 0.0;                 // at: the multiple of u currently added to x
        for (int ls = 0; ls < ls_max; ++ls) {
          const double x1 = b - tau * (b - a), x2 = a + tau * (b - a);
          double f[2];
          for (int k = 0; k < 2; ++k) {
            const double xk = k == 0 ? x1 : x2;
            if ((rc = dist_nodes_add_scaled(R, xk - at, at == 0.0))) return rc;
            at = xk;
            EACH(feahip_create_residual_forces(c));
            double uf = 0;
            if ((rc = dist_energy(R, &uf))) return rc;                // <u, -R> with the sign of the residual vector f
            f[k] = fabs(xk * uf);
          }
          if (f[0] > f[1]) a = x1; else b = x2;
          if (fabs(tolerance) < f[0] && fabs(tolerance) < f[1]) { eta = 1.0; break; }
          eta = 0.5 * (x1 + x2);
        }
        if ((rc = dist_nodes_add_scaled(R, eta - at, at == 0.0))) return rc;
      }
      EACH(feahip_update_state(c, nullptr));                          // :217-218
    } while (fabs(tolerance) > desired_tolerance && it < max_newton); // :220-221
    if (its_log) its_log[step] = it;
    if (it == max_newton) break;                                      // :225-231
  }
#undef EACH
  if (steps_done) *steps_done = step;
  for (feahip_ctx *c : R) { (void)hipSetDevice(c->device); FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream)); }
  return FEAHIP_OK;
}

// ---- implicit dynamics: Newmark steps in displacement form, full Newton (feahip_solve_dynamic) ----------------
// Per step, a0 = 1 / (beta dt^2): predictor xt = x + dt v + dt^2 (1/2 - beta) a, vt = v + dt (1 - gamma) a on all nodes
// of every context; one increment of the prescribed dofs and the load factor; Newton on K + a0 M with the residual
// f = lambda F_ext - T - a0 M (x - xt); corrector a = a0 (x - xt), v = vt + gamma dt a.  Acceleration and velocity are
// pointwise functions of x, which every rank holds at its halo nodes after dist_update_nodes_with_solution: no
// exchange beyond the static loop's.
namespace {
struct NodeCopies {
  std::vector<double *> p;
  ~NodeCopies() { for (double *q : p) if (q) (void)hipFree(q); }
};
}

int dist_dynamic(std::vector<feahip_ctx *> &R, int n_steps, double dt, double beta, double gamma, double dlambda,
                 int max_newton, double desired_tolerance, int solver_type, double solver_tolerance, int solver_max_iter,
                 double *tol_log, int tol_log_cap, int *its_log, int *steps_done)
{
  int rc, nlog = 0, step = 0;
  const double a0 = 1.0 / (beta * dt * dt);
  NodeCopies xn;                                                      // x at the start of the step in hand
#define EACH(call) for (feahip_ctx *c : R) { (void)hipSetDevice(c->device); if ((rc = (call))) return rc; }
  EACH(mass_ensure(c, "feahip_solve_dynamic"));
  for (feahip_ctx *c : R) {
    (void)hipSetDevice(c->device);
    c->mass.ke_parts = 0;                                             // (host only: the velocities are about to change)
    double *q = nullptr;
    FEA_HIP_CHECK(c, hipMalloc((void **)&q, sizeof(double) * 4 * (size_t)c->N));
    xn.p.push_back(q);
  }
  // (full Newton only: the context's line search and modified Newton are not consulted)
  for (; step < n_steps; ++step) {
    int it = 0, k = 0;
    double tolerance = 0;
    for (feahip_ctx *c : R) {
      (void)hipSetDevice(c->device);
      FEA_HIP_CHECK(c, hipMemcpyAsync(xn.p[k++], c->d_x, sizeof(double) * 4 * (size_t)c->N, hipMemcpyDeviceToDevice, c->stream));
    }
    EACH(launch_newmark_predict(c, dt, beta, gamma));
    EACH(feahip_update_nodes_with_bc(c, dlambda));
    do {
      it++;
      EACH(feahip_create_stiffness_and_residual(c));
      EACH(launch_mass_residual(c, a0));
      EACH(launch_mass_add(c, a0));
      EACH(feahip_apply_prescribed_bc(c, 0.0));
      if ((rc = dist_solve_pcg(R, solver_type, solver_tolerance, solver_max_iter, nullptr, nullptr))) return rc;
      if ((rc = dist_energy(R, &tolerance))) return rc;
      if (tol_log && nlog < tol_log_cap) tol_log[nlog] = tolerance;
      nlog++;
      if ((rc = dist_update_nodes_with_solution(R, nullptr))) return rc;
      EACH(feahip_update_state(c, nullptr));
    } while (fabs(tolerance) > desired_tolerance && it < max_newton);
    if (its_log) its_log[step] = it;
    if (it == max_newton) {                                           // as feahip_solve: the step is not counted ...
      k = 0;
      for (feahip_ctx *c : R) {                                       // ... and the state stays that of the last completed one
        (void)hipSetDevice(c->device);
        FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_x, xn.p[k++], sizeof(double) * 4 * (size_t)c->N, hipMemcpyDeviceToDevice, c->stream));
        c->load_factor -= dlambda;
        c->state_valid = false;
      }
      break;
    }
    EACH(launch_newmark_correct(c, dt, beta, gamma));
    for (feahip_ctx *c : R) c->mass.time += dt;
  }
  if (steps_done) *steps_done = step;
  for (feahip_ctx *c : R) { (void)hipSetDevice(c->device); FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream)); }
  return FEAHIP_OK;
}

// M a = lambda F_ext(x) - T(x), a = 0 on the prescribed dofs: the ordinary solve with K := M
int dist_consistent_acceleration(std::vector<feahip_ctx *> &R, int solver_type, double tol, int max_iter)
{
  int rc;
  EACH(mass_ensure(c, "feahip_consistent_acceleration"));
  for (feahip_ctx *c : R) {
    (void)hipSetDevice(c->device);
    FEA_HIP_CHECK(c, hipMemsetAsync(c->d_K_base, 0, sizeof(double) * 9 * (size_t)(c->kb1 - c->kb0), c->stream));
    c->k_bc = false; c->k_valid = true;
  }
  EACH(launch_mass_add(c, 1.0));
  EACH(feahip_create_residual_forces(c));
  EACH(feahip_apply_prescribed_bc(c, 0.0));
  if ((rc = dist_solve_pcg(R, solver_type, tol, max_iter, nullptr, nullptr))) return rc;
  if (R[0]->tr && (rc = R[0]->tr->exchange(R, 1))) return rc;        // the owners' rows of u to the halo copies
  EACH(launch_vec3_to_nodes(c, c->d_u, c->mass.d_acc));
  for (feahip_ctx *c : R) { (void)hipSetDevice(c->device); ++c->k_epoch; FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream)); }
  return FEAHIP_OK;
}

// ---- explicit dynamics: central differences in the velocity-Verlet form on the HRZ-lumped mass (feahip_solve_explicit) ----
// State (x, v, a) at t_n, the Newmark state.  Per step: kick and drift (vh = v + dt/2 a, u = dt vh on the owned rows, 0 on
// prescribed dofs); the static loop's exchange of u and x += u; one increment of the prescribed dofs and the load factor;
// ONE residual assembly f = lambda (F_surf + F_body) - T(x); finish (a = f / ml, v = vh + dt/2 a).  No K is assembled, no
// system solved; with a fixed dt nothing is read back between the first and the last step.  v and a are authoritative on
// owned nodes only: a halo node gets v = u / dt and a = 0, which needs no second exchange.

// Gershgorin: omega_max^2 <= max_i (sum_j |K_ij|) / ml(i), K the unmasked tangent at x; dt_crit = 2 / sqrt(bound)
int dist_stable_step(std::vector<feahip_ctx *> &R, double *dt_crit)
{
  int rc;
  EACH(lump_ensure(c, "feahip_stable_step"));
  EACH(feahip_create_stiffness(c));                                   // (K is another matrix from here on: k_epoch)
  EACH(launch_gershgorin(c));
  if (R[0]->tr && (rc = R[0]->tr->allreduce_max(R, 0, 1))) return rc;
  feahip_ctx *c0 = R[0];
  (void)hipSetDevice(c0->device);
  double bound = 0;
  FEA_HIP_CHECK(c0, hipMemcpyAsync(&bound, c0->d_scal + 8, sizeof(double), hipMemcpyDeviceToHost, c0->stream));
  FEA_HIP_CHECK(c0, hipStreamSynchronize(c0->stream));
  // (a NaN or an infinity in K reaches here: the reductions propagate it.  Every rank reads the same all-reduced number,
  // so every rank takes this branch or none does)
  if (!(bound > 0.0) || !std::isfinite(bound)) {
    for (feahip_ctx *c : R) c->err = "feahip_stable_step: the stiffness has no positive finite row sum";
    return FEAHIP_ESTATE;
  }
  *dt_crit = 2.0 / sqrt(bound);
  return FEAHIP_OK;
}

// 1/2 sum ml |v|^2 over all ranks
int dist_kinetic_energy(std::vector<feahip_ctx *> &R, double *e)
{
  int rc;
  EACH(lump_ensure(c, "feahip_kinetic_energy"));
  EACH(launch_kinetic_energy(c, c->d_scal + 8));
  if (R[0]->tr && (rc = R[0]->tr->allreduce(R, 0, 1))) return rc;
  feahip_ctx *c0 = R[0];
  (void)hipSetDevice(c0->device);
  FEA_HIP_CHECK(c0, hipMemcpyAsync(e, c0->d_scal + 8, sizeof(double), hipMemcpyDeviceToHost, c0->stream));
  FEA_HIP_CHECK(c0, hipStreamSynchronize(c0->stream));
  return FEAHIP_OK;
}

int dist_explicit(std::vector<feahip_ctx *> &R, int n_steps, double dt_fixed, double safety, int restep, double dlambda,
                  double *dt_log, int dt_log_cap, int *steps_done)
{
  int rc, step = 0, checked = 0, result = FEAHIP_OK;
  double dt = dt_fixed;
  EACH(lump_ensure(c, "feahip_solve_explicit"));
  for (feahip_ctx *c : R) {
    (void)hipSetDevice(c->device);
    // u is zero outside the owned and the halo rows (dist_update_nodes_with_solution adds all of it)
    FEA_HIP_CHECK(c, hipMemsetAsync(c->d_u, 0, sizeof(double) * (size_t)c->ndof, c->stream));
  }
  // Elements with det J <= 0 (or NaN) at a Gauss point of the current x, on ANY rank.  Every rank counts its own and its
  // ghost elements (launch_count_inverted, read through feahip_update_state); the counts meet in a max all-reduce BEFORE
  // anything branches on them, so all ranks of an RCCL run leave the loop together, with the same code and the same
  // steps_done, and none is left waiting in a collective its peers never enter.
  auto inverted = [&](bool &bad) -> int {
    double most = 0.0;
    for (feahip_ctx *c : R) {
      (void)hipSetDevice(c->device);
      int n = 0;
      if ((rc = launch_count_inverted(c)) || (rc = feahip_update_state(c, &n))) return rc;
      most = n != 0 ? 1.0 : most;
    }
    if (Transport *T = R[0]->tr) {
      for (feahip_ctx *c : R) {
        (void)hipSetDevice(c->device);
        FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_scal + 8, &most, sizeof(double), hipMemcpyHostToDevice, c->stream));
        FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
      }
      if ((rc = T->allreduce_max(R, 0, 1))) return rc;
      feahip_ctx *c0 = R[0];
      (void)hipSetDevice(c0->device);
      FEA_HIP_CHECK(c0, hipMemcpyAsync(&most, c0->d_scal + 8, sizeof(double), hipMemcpyDeviceToHost, c0->stream));
      FEA_HIP_CHECK(c0, hipStreamSynchronize(c0->stream));
    }
    bad = bad || most != 0.0;
    return FEAHIP_OK;
  };
  auto refuse = [&](int at) {
    for (feahip_ctx *c : R) c->err = "solve_explicit: inverted elements (det J <= 0) found at the check of step " + std::to_string(at) +
                "; the state is left as it is (explicit steps are not rolled back)";
    result = FEAHIP_ENOTCONVERGED;
  };
  for (; step < n_steps; ++step) {
    if (dt_fixed == 0.0 && (step == 0 || (restep > 0 && step % restep == 0))) {
      bool bad = false;
      double dtc = 0;
      if ((rc = inverted(bad))) return rc;
      if (bad) { refuse(step); break; }
      if ((rc = dist_stable_step(R, &dtc))) return rc;
      checked = step;
      dt = safety * dtc;
    }
    EACH(launch_explicit_kick(c, dt));
    if ((rc = dist_update_nodes_with_solution(R, nullptr))) return rc;
    EACH(feahip_update_nodes_with_bc(c, dlambda));
    EACH(launch_explicit_presc(c, dlambda, dt));
    EACH(feahip_create_residual_forces(c));
    EACH(launch_explicit_finish(c, dt));
    for (feahip_ctx *c : R) c->mass.time += dt;
    if (dt_log && step < dt_log_cap) dt_log[step] = dt;
  }
  if (result == FEAHIP_OK && n_steps > 0) {
    bool bad = false;
    if ((rc = inverted(bad))) return rc;
    if (bad) refuse(n_steps); else checked = n_steps;
  }
  if (steps_done) *steps_done = result == FEAHIP_OK ? step : checked;
  for (feahip_ctx *c : R) { (void)hipSetDevice(c->device); FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream)); }
  return result;
}
#undef EACH

// ---- arc-length continuation on the surface loads (feahip_solve_arclength) -------
// Crisfield's cylindrical arc length, one unsharded context.  The linear algebra of a corrector iteration is ONE
// two-column solve K [du_R, du_F] = [R, F] (kernels_solve2.hip) and one fused reduction over Du, du_R, du_F, R.
#define ARC_SUMS 7
// partial sums, block b: part[s * FEA_RED_BLOCKS + b] of
//   0 du_F.du_F   1 Du.du_F   2 du_R.du_F   3 |Du + du_R|^2   4 Du.(Du + du_R)   5 du_R.R   6 du_F.R
// (a, the two parts of b, c + dl^2, the root choice, and the two parts of the energy <du, R>)
__global__ __launch_bounds__(256)
void k_arc_dots_partial(int n, const double *Du, const double *dR, const double *dF, const double *R, double *part)
{
  __shared__ double sh[ARC_SUMS][4];
  double s[ARC_SUMS] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double u = Du[i], r = dR[i], f = dF[i], g = R[i], w = u + r;
    s[0] += f * f; s[1] += u * f; s[2] += r * f; s[3] += w * w; s[4] += u * w; s[5] += r * g; s[6] += f * g;
  }
#pragma unroll
  for (int k = 0; k < ARC_SUMS; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < ARC_SUMS) {
    const double *q = sh[threadIdx.x];
    part[(size_t)threadIdx.x * FEA_RED_BLOCKS + blockIdx.x] = q[0] + q[1] + q[2] + q[3];
  }
}
// out[s] = sum of part[s * FEA_RED_BLOCKS .. + nparts) for s < nsums: one block, fixed order
__global__ __launch_bounds__(256)
void k_arc_dots_final(int nparts, int nsums, const double *part, double *out)
{
  __shared__ double sh[4];
  for (int s = 0; s < nsums; ++s) {
    double v = 0;
    for (int i = threadIdx.x; i < nparts; i += 256) v += part[(size_t)s * FEA_RED_BLOCKS + i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[s] = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
  }
}
__global__ void k_arc_scale(int n, double s, const double *v, double *Du)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) Du[i] = s * v[i];
}
__global__ void k_arc_update(int n, double dlam, const double *dR, const double *dF, double *Du)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) Du[i] += dR[i] + dlam * dF[i];
}
// x = x_n + Du; x and x_n are [N][4]
__global__ void k_arc_nodes(int n, const double *xn, const double *Du, double *x)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[(size_t)(i / 3) * 4 + i % 3] = xn[(size_t)(i / 3) * 4 + i % 3] + Du[i];
}
__global__ void k_arc_mask(int n, const uint8_t *mask, double *f)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && mask[i]) f[i] = 0.0;
}

namespace {
struct ArcBuffers {
  double *xn = nullptr, *Du = nullptr, *Dprev = nullptr, *v = nullptr, *F = nullptr;
  ~ArcBuffers() { dev_free({xn, Du, Dprev, v, F}); }
};
}

// F(x) at load factor 1 into d_F, zero at the prescribed dofs: the surface kernels with another destination and factor
static int arc_external_forces(feahip_ctx *c, double *d_F)
{
  const double lf = c->load_factor;
  FEA_HIP_CHECK(c, hipMemsetAsync(d_F, 0, sizeof(double) * (size_t)c->ndof, c->stream));
  c->load_factor = 1.0;
  const int rc = launch_surface_loads(c, d_F);
  c->load_factor = lf;
  if (rc) return rc;
  hipLaunchKernelGGL(k_arc_mask, dim3((c->ndof + 255) / 256), dim3(256), 0, c->stream, c->ndof, c->d_dofmask, d_F);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// the seven sums of a corrector iteration (or, with R = dR = dF = v and Du = Dprev, v.v in [0] and Dprev.v in [1])
static int arc_dots(feahip_ctx *c, const double *Du, const double *dR, const double *dF, const double *R, double *out)
{
  int g = (c->ndof + 255) / 256;
  g = g < FEA_RED_BLOCKS ? g : FEA_RED_BLOCKS;
  hipLaunchKernelGGL(k_arc_dots_partial, dim3(g), dim3(256), 0, c->stream, c->ndof, Du, dR, dF, R, c->d2_part);
  hipLaunchKernelGGL(k_arc_dots_final, dim3(1), dim3(256), 0, c->stream, g, ARC_SUMS, c->d2_part, c->d2_scal);
  FEA_HIP_CHECK(c, hipGetLastError());
  FEA_HIP_CHECK(c, hipMemcpyAsync(out, c->d2_scal, sizeof(double) * ARC_SUMS, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

int arclength_solve(feahip_ctx *c, double lambda_max, int max_steps, int max_newton, double desired_tolerance,
                    int solver_type, double solver_tolerance, int solver_max_iter, double *lambda_log, double *tol_log,
                    int log_cap, int *its_log, int *steps_done)
{
  int rc, nlog = 0, step = 0, n_bad = 0;
  const int n = c->ndof;
  const size_t vb = sizeof(double) * (size_t)n, xb = sizeof(double) * 4 * (size_t)c->N;
  const dim3 gn((n + 255) / 256), b256(256);
  ArcBuffers B;
  FEA_HIP_CHECK(c, hipMalloc((void **)&B.xn, xb));
  for (double **p : {&B.Du, &B.Dprev, &B.v, &B.F}) {
    FEA_HIP_CHECK(c, hipMalloc((void **)p, vb));
    FEA_HIP_CHECK(c, hipMemsetAsync(*p, 0, vb, c->stream));
  }
  double lambda_n = c->load_factor, dl = 0.0, s[ARC_SUMS];
  FEA_HIP_CHECK(c, hipMemcpyAsync(B.xn, c->d_x, xb, hipMemcpyDeviceToDevice, c->stream));
  auto restore = [&]() -> int {
    c->state_valid = false;
    c->load_factor = lambda_n;
    FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_x, B.xn, xb, hipMemcpyDeviceToDevice, c->stream));
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return FEAHIP_OK;
  };
  int result = FEAHIP_OK;
  for (; step < max_steps && lambda_n < lambda_max; ++step) {
    // predictor: K v = F at the converged point
    if ((rc = feahip_create_stiffness(c)) || (rc = feahip_update_state(c, &n_bad))) return rc;
    if (n_bad) { c->err = "solve_arclength: bad Jacobians at a converged point"; result = FEAHIP_ENOTCONVERGED; break; }
    if ((rc = feahip_apply_prescribed_bc(c, 0.0)) || (rc = arc_external_forces(c, B.F))) return rc;
    FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_f, B.F, vb, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = solve_pcg(c, solver_type, solver_tolerance, solver_max_iter, nullptr, nullptr))) return rc;
    FEA_HIP_CHECK(c, hipMemcpyAsync(B.v, c->d_u, vb, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = arc_dots(c, B.Dprev, B.v, B.v, B.v, s))) return rc;
    const double vnorm = sqrt(s[0]);
    if (!(vnorm > 0.0)) { c->err = "solve_arclength: the loads move nothing (K v = F gave v = 0)"; result = FEAHIP_ENOTCONVERGED; break; }
    const double sgn = (step > 0 && s[1] < 0.0) ? -1.0 : 1.0;
    if (step == 0) dl = vnorm;
    bool converged = false;
    int it = 0;
    for (int cut = 0; cut <= 8 && !converged; ++cut) {
      if (cut > 0) dl *= 0.5;
      double Dlambda = sgn * dl / vnorm;
      hipLaunchKernelGGL(k_arc_scale, gn, b256, 0, c->stream, n, Dlambda, B.v, B.Du);
      bool failed = false;
      for (it = 1; it <= max_newton && !failed; ++it) {
        c->state_valid = false;
        c->load_factor = lambda_n + Dlambda;
        hipLaunchKernelGGL(k_arc_nodes, gn, b256, 0, c->stream, n, B.xn, B.Du, c->d_x);
        if ((rc = feahip_create_stiffness_and_residual(c)) || (rc = feahip_update_state(c, &n_bad))) return rc;
        if (n_bad) { failed = true; break; }
        if ((rc = feahip_apply_prescribed_bc(c, 0.0)) || (rc = arc_external_forces(c, B.F))) return rc;
        if ((rc = launch_interleave(c, c->d_f, B.F, c->d2_f))) return rc;
        rc = solve_pcg2(c, solver_type, solver_tolerance, solver_max_iter, nullptr, nullptr);
        if (rc == FEAHIP_ENOTCONVERGED) { failed = true; break; }
        if (rc) return rc;
        if ((rc = arc_dots(c, B.Du, c->d_u, c->d_u2, c->d_f, s))) return rc;
        const double qa = s[0], qb = 2.0 * (s[1] + s[2]), qc = s[3] - dl * dl;
        const double disc = qb * qb - 4.0 * qa * qc;
        if (!(qa > 0.0) || !(disc >= 0.0)) { failed = true; break; }
        // both roots without cancellation; the one that keeps Du pointing forward: larger Du.(Du + du_R + dlam du_F)
        const double q = -0.5 * (qb + (qb >= 0.0 ? 1.0 : -1.0) * sqrt(disc));
        const double r1 = q / qa, r2 = q != 0.0 ? qc / q : r1;
        const double dlam = (s[4] + r1 * s[1] >= s[4] + r2 * s[1]) ? r1 : r2;
        const double tolerance = s[5] + dlam * s[6];
        if (tol_log && nlog < log_cap) tol_log[nlog] = tolerance;
        nlog++;
        hipLaunchKernelGGL(k_arc_update, gn, b256, 0, c->stream, n, dlam, c->d_u, c->d_u2, B.Du);
        Dlambda += dlam;
        if (!(tolerance == tolerance)) { failed = true; break; }
        if (fabs(tolerance) <= desired_tolerance) { converged = true; break; }
      }
      if (converged) {
        hipLaunchKernelGGL(k_arc_nodes, gn, b256, 0, c->stream, n, B.xn, B.Du, c->d_x);
        FEA_HIP_CHECK(c, hipMemcpyAsync(B.xn, c->d_x, xb, hipMemcpyDeviceToDevice, c->stream));
        FEA_HIP_CHECK(c, hipMemcpyAsync(B.Dprev, B.Du, vb, hipMemcpyDeviceToDevice, c->stream));
        lambda_n += Dlambda;
      } else if ((rc = restore())) return rc;
    }
    if (!converged) {
      c->err = "solve_arclength: step " + std::to_string(step) + " did not converge after 8 halvings of the arc length";
      result = FEAHIP_ENOTCONVERGED;
      break;
    }
    if (lambda_log) lambda_log[step] = lambda_n;
    if (its_log) its_log[step] = it;
  }
  if (steps_done) *steps_done = step;
  const std::string why = c->err;
  if ((rc = restore())) return rc;
  if (result != FEAHIP_OK) c->err = why;
  return result;
}
