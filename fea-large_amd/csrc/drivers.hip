// drivers.hip -- the loops that drive one or more ranks through a computation: the Newton loop of solve(), the
// Newmark and the explicit time steps with their collective helpers (consistent acceleration, stable step, kinetic
// energy), and the arc-length continuation on one unsharded context.
//
// Everything here is host code over the launchers, the PCG (kernels_solve.hip, kernels_solve2.hip) and the transports
// (dist.hip: RCCL; kernels_solve.hip: in-process group), plus the few pointwise kernels of the arc length.  R = the
// ranks this process drives; every collective is entered by all of them, in the same order.
#include "feahip_internal.h"
#include "reduce_device.h"
#include <cmath>

// ---- the loop of solve() over one or more ranks -------------------------------
int dist_newton(std::vector<feahip_ctx *> &R, int load_increments, int max_newton, int modified_newton,
                double desired_tolerance, int solver_type, double solver_tolerance, int solver_max_iter,
                double *tol_log, int tol_log_cap, int *its_log, int *steps_done)
{
  int rc, nlog = 0, step = 0;
  // (the feahip_* entry points set the device in their guard; that FOR_RANKS sets it as well is harmless)
  // One pass of Newton iterations at the nodes and the load in force: K, then iterations until the energy passes or
  // max_newton of them are spent (failed).  A load increment is one pass; with contact multipliers to update, one more
  // per augmentation.  it counts the iterations of all passes of the step.
  auto newton_pass = [&](int &it, bool &failed) -> int {
    int k = 0;
    double tolerance = 0;
    FOR_RANKS(c) { if ((rc = feahip_create_stiffness(c))) return rc; }   // :177 (owned rows, ghost elements recomputed)
    if (modified_newton) { FOR_RANKS(c) { if ((rc = feahip_stash_stiffness(c))) return rc; } }   // :179
    do {
      it++; k++;
      if (modified_newton) {
        FOR_RANKS(c) { if ((rc = feahip_create_residual_forces(c))) return rc; }   // :185
        FOR_RANKS(c) { if ((rc = feahip_restore_stiffness(c))) return rc; }   // :194-195
      } else if (k == 1) {
        FOR_RANKS(c) { if ((rc = feahip_create_residual_forces(c))) return rc; }   // K of :177 is current
      } else {
        FOR_RANKS(c) { if ((rc = feahip_create_stiffness_and_residual(c))) return rc; }   // :185 + :200
      }
      FOR_RANKS(c) { if ((rc = feahip_apply_prescribed_bc(c, 0.0))) return rc; }   // :203
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
          for (int j = 0; j < 2; ++j) {
            const double xk = j == 0 ? x1 : x2;
            if ((rc = dist_nodes_add_scaled(R, xk - at, at == 0.0))) return rc;
            at = xk;
            FOR_RANKS(c) { if ((rc = feahip_create_residual_forces(c))) return rc; }
            double uf = 0;
            if ((rc = dist_energy(R, &uf))) return rc;                // <u, -R> with the sign of the residual vector f
            f[j] = fabs(xk * uf);
          }
          if (f[0] > f[1]) a = x1; else b = x2;
          if (fabs(tolerance) < f[0] && fabs(tolerance) < f[1]) { eta = 1.0; break; }
          eta = 0.5 * (x1 + x2);
        }
        if ((rc = dist_nodes_add_scaled(R, eta - at, at == 0.0))) return rc;
      }
      FOR_RANKS(c) { if ((rc = feahip_update_state(c, nullptr))) return rc; }   // :217-218
    } while (fabs(tolerance) > desired_tolerance && k < max_newton); // :220-221
    failed = k == max_newton;                                         // :225-231
    return FEAHIP_OK;
  };
  ContactState none;                                                  // (the parameters are the same on every rank that has them)
  const ContactState *with = &none;
  for (feahip_ctx *c : R) if (c->contact.set) { with = &c->contact; break; }
  const ContactState &contact = *with;
  for (; step < load_increments; ++step) {                           // fea_solver.c:163
    int it = 0;
    bool failed = false;
    FOR_RANKS(c) { if ((rc = feahip_update_nodes_with_bc(c, 1.0))) return rc; }   // :168 (prescribed values are replicated)
    FOR_RANKS(c) { if ((rc = feahip_update_state(c, nullptr))) return rc; }   // :171-174
    if ((rc = newton_pass(it, failed))) return rc;
    // augmented Lagrangian: while the largest penetration of an active pair exceeds the tolerance, update the multipliers
    // and iterate again at the same load (every rank reads the same all-reduced number and takes the same branch)
    for (int aug = 0; contact.set && !failed && aug < contact.augment_max; ++aug) {
      double info[4];
      if ((rc = dist_contact_info(R, info))) return rc;
      if (info[1] <= contact.gap_tolerance) break;
      if ((rc = dist_contact_augment(R, nullptr))) return rc;
      if ((rc = newton_pass(it, failed))) return rc;
    }
    if (its_log) its_log[step] = it;
    if (failed) break;
  }
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
// With Rayleigh damping C = alpha M + beta_k K_d (feahip_set_damping), c1 = gamma / (beta dt) and w = vt + c1 (x - xt), the
// velocity the corrector will assign: the residual is f - a0 M (x - xt) - C w and the matrix K + (a0 + c1 alpha) M +
// c1 beta_k K_d (kernels_damping.hip).  C is constant, so this tangent is exact; w is pointwise too and needs no exchange.
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
  const double a0 = 1.0 / (beta * dt * dt), c1 = gamma / (beta * dt);
  NodeCopies xn;                                                      // x at the start of the step in hand
  FOR_RANKS(c) { if ((rc = mass_ensure(c, "feahip_solve_dynamic")) || (rc = damping_ready(c, "feahip_solve_dynamic"))) return rc; }
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
    FOR_RANKS(c) { if ((rc = launch_newmark_predict(c, dt, beta, gamma))) return rc; }
    FOR_RANKS(c) { if ((rc = feahip_update_nodes_with_bc(c, dlambda))) return rc; }
    do {
      it++;
      FOR_RANKS(c) { if ((rc = feahip_create_stiffness_and_residual(c))) return rc; }
      FOR_RANKS(c) {                                                  // (a context without damping: the launches as before)
        const DampingState &D = c->damping;
        if ((rc = D.on() ? launch_damp_residual(c, a0, c1) : launch_mass_residual(c, a0))) return rc;
      }
      FOR_RANKS(c) {
        const DampingState &D = c->damping;
        if ((rc = D.beta > 0.0 ? launch_damp_add(c, a0 + c1 * D.alpha, c1 * D.beta)
                               : launch_mass_add(c, D.on() ? a0 + c1 * D.alpha : a0))) return rc;
      }
      FOR_RANKS(c) { if ((rc = feahip_apply_prescribed_bc(c, 0.0))) return rc; }
      if ((rc = dist_solve_pcg(R, solver_type, solver_tolerance, solver_max_iter, nullptr, nullptr))) return rc;
      if ((rc = dist_energy(R, &tolerance))) return rc;
      if (tol_log && nlog < tol_log_cap) tol_log[nlog] = tolerance;
      nlog++;
      if ((rc = dist_update_nodes_with_solution(R, nullptr))) return rc;
      FOR_RANKS(c) { if ((rc = feahip_update_state(c, nullptr))) return rc; }
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
    FOR_RANKS(c) { if ((rc = launch_newmark_correct(c, dt, beta, gamma))) return rc; }
    for (feahip_ctx *c : R) c->mass.time += dt;
  }
  if (steps_done) *steps_done = step;
  for (feahip_ctx *c : R) { (void)hipSetDevice(c->device); FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream)); }
  return FEAHIP_OK;
}

// M a = lambda F_ext(x) - T(x) - C v, a = 0 on the prescribed dofs: the ordinary solve with K := M
int dist_consistent_acceleration(std::vector<feahip_ctx *> &R, int solver_type, double tol, int max_iter)
{
  int rc;
  FOR_RANKS(c) { if ((rc = mass_ensure(c, "feahip_consistent_acceleration")) || (rc = damping_ready(c, "feahip_consistent_acceleration"))) return rc; }
  for (feahip_ctx *c : R) {
    (void)hipSetDevice(c->device);
    FEA_HIP_CHECK(c, hipMemsetAsync(c->d_K_base, 0, sizeof(double) * 9 * (size_t)(c->kb1 - c->kb0), c->stream));
    c->k_bc = false; c->k_valid = true;
  }
  FOR_RANKS(c) { if ((rc = launch_mass_add(c, 1.0))) return rc; }
  FOR_RANKS(c) { if ((rc = feahip_create_residual_forces(c))) return rc; }
  FOR_RANKS(c) { if (c->damping.on() && (rc = launch_damp_force(c))) return rc; }   // the velocities are valid on halo nodes
  FOR_RANKS(c) { if ((rc = feahip_apply_prescribed_bc(c, 0.0))) return rc; }
  if ((rc = dist_solve_pcg(R, solver_type, tol, max_iter, nullptr, nullptr))) return rc;
  if (R[0]->tr && (rc = R[0]->tr->exchange(R, 1))) return rc;        // the owners' rows of u to the halo copies
  FOR_RANKS(c) { if ((rc = launch_vec3_to_nodes(c, c->d_u, c->mass.d_acc))) return rc; }
  for (feahip_ctx *c : R) { (void)hipSetDevice(c->device); ++c->k_epoch; FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream)); }
  return FEAHIP_OK;
}

// ---- explicit dynamics: central differences in the velocity-Verlet form on the HRZ-lumped mass (feahip_solve_explicit) ----
// State (x, v, a) at t_n, the Newmark state.  Per step: kick and drift (vh = v + dt/2 a, u = dt vh on the owned rows, 0 on
// prescribed dofs); the static loop's exchange of u and x += u; one increment of the prescribed dofs and the load factor;
// ONE residual assembly f = lambda (F_surf + F_body) - T(x); finish (a = f / ml, v = vh + dt/2 a).  No K is assembled, no
// system solved; with a fixed dt nothing is read back between the first and the last step.  v and a are authoritative on
// owned nodes only: a halo node gets v = u / dt and a = 0, which needs no second exchange.
// Mass-proportional damping (feahip_set_damping with beta_k = 0) changes the finish alone: M_L a = f - alpha M_L v with the
// end-of-step v, a = (f / ml - alpha vh) / (1 + alpha dt / 2).  In vh this is central differences with the centred velocity
// (vh_- + vh_+) / 2, whose stability limit stays 2 / omega_max for every alpha >= 0: dist_stable_step is as it was.  A
// stiffness-proportional part is refused: there is no K in this loop, and a lagged K_d vh would shrink the stable step.

// Gershgorin: omega_max^2 <= max_i (sum_j |K_ij|) / ml(i), K the unmasked tangent at x; dt_crit = 2 / sqrt(bound)
int dist_stable_step(std::vector<feahip_ctx *> &R, double *dt_crit)
{
  int rc;
  FOR_RANKS(c) { if ((rc = lump_ensure(c, "feahip_stable_step"))) return rc; }
  // contact: the plain assembly, then w eps n n' of EVERY contact pair in place of the active pairs' term (positive
  // semi-definite, so still a bound for the active ones): a node that enters contact between two estimates does not push the
  // step over the bound.  K stays as this leaves it
  FOR_RANKS(c) {                                                       // (K is another matrix from here on: k_epoch)
    if (c->contact.n == 0) { if ((rc = feahip_create_stiffness(c))) return rc; continue; }
    ++c->k_epoch; c->k_bc = false;                                     // feahip_create_stiffness, without the contact term
    if ((rc = launch_assemble(c, true, false, true))) return rc;
  }
  FOR_RANKS(c) { if ((rc = launch_contact_bound(c))) return rc; }
  FOR_RANKS(c) { if ((rc = launch_gershgorin(c))) return rc; }
  double bound = 0;
  if ((rc = dist_read_scalars(R, RankReduce::max, 1, &bound))) return rc;
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
  FOR_RANKS(c) { if ((rc = lump_ensure(c, "feahip_kinetic_energy"))) return rc; }
  FOR_RANKS(c) { if ((rc = launch_kinetic_energy(c, c->d_scal + 8))) return rc; }
  return dist_read_scalars(R, RankReduce::sum, 1, e);
}

// contact over all ranks: active pairs, the largest penetration over them, sum w t, Pi_c (identical on every rank)
int dist_contact_info(std::vector<feahip_ctx *> &R, double *out)
{
  int rc;
  double s[4];
  FOR_RANKS(c) { if ((rc = launch_contact_info(c))) return rc; }
  if (Transport *T = R[0]->tr)                                        // three sums in [8 .. 11), the maximum in [11]
    if ((rc = T->allreduce(R, 0, 3)) || (rc = T->allreduce_max(R, 3, 1))) return rc;
  feahip_ctx *c0 = R[0];
  (void)hipSetDevice(c0->device);
  FEA_HIP_CHECK(c0, hipMemcpyAsync(s, c0->d_scal + 8, sizeof(s), hipMemcpyDeviceToHost, c0->stream));
  FEA_HIP_CHECK(c0, hipStreamSynchronize(c0->stream));
  out[0] = s[0]; out[1] = s[3]; out[2] = s[1]; out[3] = s[2];
  return FEAHIP_OK;
}

// the largest penetration over the active pairs as it stands (where asked for), then mu <- max(0, mu + eps p) on every
// rank's own nodes
int dist_contact_augment(std::vector<feahip_ctx *> &R, double *max_penetration)
{
  int rc;
  double info[4];
  if (max_penetration) {                                              // (a caller that has just read it passes null)
    if ((rc = dist_contact_info(R, info))) return rc;
    *max_penetration = info[1];
  }
  FOR_RANKS(c) { if ((rc = launch_contact_augment(c))) return rc; }
  for (feahip_ctx *c : R) { (void)hipSetDevice(c->device); FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream)); }
  return FEAHIP_OK;
}

// sum_e W_e over all ranks: every rank sums the shares W_e / npe of the nodes it owns, so that an element a rank holds as
// a ghost is counted once
int dist_strain_energy(std::vector<feahip_ctx *> &R, double *W)
{
  int rc;
  FOR_RANKS(c) { if ((rc = launch_results(c, -1, c->d_scal + 8))) return rc; }
  return dist_read_scalars(R, RankReduce::sum, 1, W);
}

int dist_explicit(std::vector<feahip_ctx *> &R, int n_steps, double dt_fixed, double safety, int restep, double dlambda,
                  double *dt_log, int dt_log_cap, int *steps_done)
{
  int rc, step = 0, checked = 0, result = FEAHIP_OK;
  double dt = dt_fixed;
  for (feahip_ctx *c : R)
    if (c->damping.beta > 0.0) {
      for (feahip_ctx *e : R)
        e->err = "solve_explicit: the damping has beta_k = " + std::to_string(c->damping.beta) +
                 " > 0; the explicit loop takes mass-proportional damping only (feahip_set_damping(ctx, alpha, 0))";
      return FEAHIP_EINVAL;
    }
  FOR_RANKS(c) { if ((rc = lump_ensure(c, "feahip_solve_explicit"))) return rc; }
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
    if (R[0]->tr) {                                                   // (one process, one count: nothing to reduce)
      for (feahip_ctx *c : R) {
        (void)hipSetDevice(c->device);
        FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_scal + 8, &most, sizeof(double), hipMemcpyHostToDevice, c->stream));
        FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
      }
      if ((rc = dist_read_scalars(R, RankReduce::max, 1, &most))) return rc;
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
    FOR_RANKS(c) { if ((rc = launch_explicit_kick(c, dt))) return rc; }
    if ((rc = dist_update_nodes_with_solution(R, nullptr))) return rc;
    FOR_RANKS(c) { if ((rc = feahip_update_nodes_with_bc(c, dlambda))) return rc; }
    FOR_RANKS(c) { if ((rc = launch_explicit_presc(c, dlambda, dt))) return rc; }
    FOR_RANKS(c) { if ((rc = feahip_create_residual_forces(c))) return rc; }
    FOR_RANKS(c) { if ((rc = launch_explicit_finish(c, dt))) return rc; }
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

// ---- arc-length continuation on the surface loads (feahip_solve_arclength) -------
// Crisfield's cylindrical arc length, one unsharded context.  The linear algebra of a corrector iteration is ONE
// two-column solve K [du_R, du_F] = [R, F] (kernels_solve2.hip) and one fused reduction over Du, du_R, du_F, R.
#define ARC_SUMS 7
static_assert(ARC_SUMS <= 8, "the sums are read from d_scal[8 .. 16)");
// partial sums, block b: part[s * FEA_RED_BLOCKS + b] of
//   0 du_F.du_F   1 Du.du_F   2 du_R.du_F   3 |Du + du_R|^2   4 Du.(Du + du_R)   5 du_R.R   6 du_F.R
// (a, the two parts of b, c + dl^2, the root choice, and the two parts of the energy <du, R>)
__global__ __launch_bounds__(256)
void k_arc_dots_partial(int n, const double *Du, const double *dR, const double *dF, const double *R, double *part)
{
  __shared__ double sh[4][ARC_SUMS];
  double s[ARC_SUMS] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double u = Du[i], r = dR[i], f = dF[i], g = R[i], w = u + r;
    s[0] += f * f; s[1] += u * f; s[2] += r * f; s[3] += w * w; s[4] += u * w; s[5] += r * g; s[6] += f * g;
  }
  const double t = block_sums<ARC_SUMS>(s, sh);
  if (threadIdx.x < ARC_SUMS) part[(size_t)threadIdx.x * FEA_RED_BLOCKS + blockIdx.x] = t;
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
  enq_reduce_final(c, g, ARC_SUMS, FEA_RED_BLOCKS, c->d2_part, c->d_scal + 8);   // (seven of the eight slots behind [8])
  FEA_HIP_CHECK(c, hipGetLastError());
  std::vector<feahip_ctx *> self(1, c);
  return dist_read_scalars(self, RankReduce::sum, ARC_SUMS, out);              // (no transport: the read-back alone)
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
