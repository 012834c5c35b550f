/*
 * fea_export.c -- Gmsh export and the per-load-step snapshots it needs.
 * Mirrors solver_export_tetrahedra10_gmsh (fea_solver.c:1375-1488) and
 * solver_load_step_init (:605-636) so that post-processing written for the
 * reference's .msh files (utilities/gmshanalyser.py) reads these unchanged.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fea_host.h"

void fea_export_name(const char *deck_path, char *out)
{
  const char *dot = strrchr(deck_path, '.');
  const char *slash = strrchr(deck_path, '/');
  size_t n = (dot && (!slash || dot > slash)) ? (size_t)(dot - deck_path) : strlen(deck_path);
  memcpy(out, deck_path, n);
  strcpy(out + n, ".msh");
}

void fea_snapshots_free(fea_step_snapshot *steps, int n)
{
  int i;
  if (!steps) return;
  for (i = 0; i < n; ++i) {
    free(steps[i].nodes); free(steps[i].stress0); free(steps[i].nodal_stress); free(steps[i].von_mises);
    free(steps[i].contact_pressure);
    steps[i].nodes = steps[i].stress0 = steps[i].nodal_stress = steps[i].von_mises = steps[i].contact_pressure = NULL;
  }
}

/* what solver_load_step_init keeps of a finished increment (fea_solver.c:605-636): the nodes and, for the
 * export, the stress of Gauss point 0 of every element (:1480) */
struct snap_sink { fea_step_snapshot *steps; int cap; double *S; FILE *log; int explicit_run; };

static int keep_snapshot(const fea_deck *d, feahip_ctx *ctx, int step, void *user)
{
  struct snap_sink *k = (struct snap_sink *)user;
  const int G = d->gauss_nodes_count;
  int e, rc;
  if ((rc = fea_log_results(d, ctx, k->log, k->explicit_run))) return rc;
  if (!k->steps || step >= k->cap) return 0;
  k->steps[step].nodes = (double *)malloc(sizeof(double) * 3 * (size_t)d->nodes_count);
  k->steps[step].stress0 = (double *)malloc(sizeof(double) * 9 * (size_t)d->elements_count);
  if (!k->S) k->S = (double *)malloc(sizeof(double) * 9 * (size_t)d->elements_count * G);
  if (!k->steps[step].nodes || !k->steps[step].stress0 || !k->S) return FEAHIP_ENOMEM;
  if ((rc = feahip_get_nodes(ctx, k->steps[step].nodes))) return rc;
  if ((rc = feahip_get_stresses(ctx, k->S))) return rc;
  for (e = 0; e < d->elements_count; ++e)
    memcpy(k->steps[step].stress0 + (size_t)e * 9, k->S + (size_t)e * G * 9, sizeof(double) * 9);
  if (d->results_nodal_stress) {
    k->steps[step].nodal_stress = (double *)malloc(sizeof(double) * 6 * (size_t)d->nodes_count);
    k->steps[step].von_mises = (double *)malloc(sizeof(double) * (size_t)d->nodes_count);
    if (!k->steps[step].nodal_stress || !k->steps[step].von_mises) return FEAHIP_ENOMEM;
    if ((rc = feahip_get_nodal_stresses(ctx, -1, k->steps[step].nodal_stress, k->steps[step].von_mises, NULL))) return rc;
  }
  if (d->contact_faces_count > 0 && d->contact_obstacles_count > 0) {
    k->steps[step].contact_pressure = (double *)malloc(sizeof(double) * (size_t)d->nodes_count);
    if (!k->steps[step].contact_pressure) return FEAHIP_ENOMEM;
    if ((rc = feahip_get_contact_status(ctx, NULL, k->steps[step].contact_pressure))) return rc;
  }
  return 0;
}

int fea_solve_with_snapshots(const fea_deck *d, feahip_ctx *ctx, void *logp, fea_step_snapshot *steps, int cap)
{
  struct snap_sink k;
  int done;
  k.steps = steps; k.cap = cap; k.S = NULL; k.log = NULL; k.explicit_run = 0;   /* (fea_solve_steps writes the result lines) */
  done = fea_solve_steps(d, ctx, logp, keep_snapshot, &k);     /* the one Newton loop of the host side (fea_solve.c) */
  free(k.S);
  return done;
}

/* (arc-length :max N) with N > 0 on a deck with surface loads: the path is followed by feahip_solve_arclength,
 * max_steps = N, lambda_max = load-increments; the final state is the one snapshot */
int fea_solve_arclength_with_snapshot(const fea_deck *d, feahip_ctx *ctx, void *logp, fea_step_snapshot *last)
{
  FILE *log = (FILE *)logp;
  struct snap_sink k;
  const int n = d->arclength_max;
  double *lam = (double *)calloc((size_t)n, sizeof *lam);
  int *its = (int *)calloc((size_t)n, sizeof *its);
  int done = 0, rc, i;
  if (!lam || !its) { free(lam); free(its); return FEAHIP_ENOMEM; }
  rc = feahip_solve_arclength(ctx, (double)d->load_increments_count, n, d->max_newton_count, d->desired_tolerance,
                              d->solver_type, d->solver_tolerance, d->solver_max_iter, lam, NULL, 0, its, &done);
  if (log)
    for (i = 0; i < done; ++i)
      fprintf(log, "Arc-length step %d finished: load factor %.17g, %d iterations\n", i + 1, lam[i], its[i]);
  free(lam); free(its);
  if (rc == FEAHIP_ENOTCONVERGED && log) fprintf(log, "Unable to finish arc-length step %d, exit\n", done + 1);
  if (rc && rc != FEAHIP_ENOTCONVERGED) return rc;
  k.steps = last; k.cap = 1; k.S = NULL; k.log = log; k.explicit_run = 0;
  rc = keep_snapshot(d, ctx, 0, &k);
  free(k.S);
  return rc ? rc : done;
}

/* (dynamics :steps N ...) with N > 0: the Newmark steps of feahip_solve_dynamic, or the explicit steps of
 * feahip_solve_explicit; the final state is the one snapshot */
int fea_solve_dynamic_with_snapshot(const fea_deck *d, feahip_ctx *ctx, void *logp, fea_step_snapshot *last)
{
  FILE *log = (FILE *)logp;
  struct snap_sink k;
  const int n = d->dynamics_steps;
  int *its = (int *)calloc((size_t)(n > 0 ? n : 1), sizeof *its);
  int done = 0, rc, i;
  const int per_step = d->results_energy || d->results_reactions;
  if (!its) return FEAHIP_ENOMEM;
  if (d->dynamics_explicit) {                         /* :scheme explicit: central differences on the lumped mass */
    double *dts = (double *)calloc((size_t)(n > 0 ? n : 1), sizeof *dts), t = 0;
    free(its);
    if (!dts) return FEAHIP_ENOMEM;
    k.steps = NULL; k.cap = 0; k.S = NULL; k.log = log; k.explicit_run = 1;
    if (per_step && d->dynamics_dt > 0) {             /* a fixed step: one call per step, the result lines after each */
      for (rc = 0, i = 0; i < n && !rc; ++i) {
        int one = 0;
        rc = feahip_solve_explicit(ctx, 1, d->dynamics_dt, d->dynamics_safety, d->dynamics_restep, d->dynamics_dlambda, dts + i, 1, &one);
        done += one;
        if (!one) break;
        t += dts[i];
        if (log) fprintf(log, "Explicit step %d finished: time %.17g, dt %.17g\n", i + 1, t, dts[i]);
        if (!rc && i + 1 < n) rc = fea_log_results(d, ctx, log, 1);   /* (the last step's lines come with its snapshot) */
      }
    } else {
      rc = feahip_solve_explicit(ctx, n, d->dynamics_dt, d->dynamics_safety, d->dynamics_restep, d->dynamics_dlambda, dts, n, &done);
      if (log)
        for (i = 0; i < done; ++i) {
          t += dts[i];
          fprintf(log, "Explicit step %d finished: time %.17g, dt %.17g\n", i + 1, t, dts[i]);
        }
    }
    free(dts);
    if (rc == FEAHIP_ENOTCONVERGED && log) fprintf(log, "Inverted elements after explicit step %d, exit\n", done);
    if (rc && rc != FEAHIP_ENOTCONVERGED) return rc;
    k.steps = last; k.cap = 1;
    rc = keep_snapshot(d, ctx, 0, &k);
    free(k.S);
    return rc ? rc : done;
  }
  if (per_step) {                                     /* one call per step, the result lines after each */
    for (rc = 0, i = 0; i < n && !rc; ++i) {
      int one = 0;
      rc = feahip_solve_dynamic(ctx, 1, d->dynamics_dt, d->dynamics_beta, d->dynamics_gamma, d->dynamics_dlambda,
                                d->max_newton_count, d->desired_tolerance, d->solver_type, d->solver_tolerance,
                                d->solver_max_iter, NULL, 0, its + i, &one);
      if (rc || !one) break;
      done += one;
      if (log) fprintf(log, "Dynamic step %d finished: time %.17g, %d iterations\n", i + 1, (i + 1) * d->dynamics_dt, its[i]);
      if (i + 1 < n) rc = fea_log_results(d, ctx, log, 0);            /* (the last step's lines come with its snapshot) */
    }
  } else {
    rc = feahip_solve_dynamic(ctx, n, d->dynamics_dt, d->dynamics_beta, d->dynamics_gamma, d->dynamics_dlambda,
                              d->max_newton_count, d->desired_tolerance, d->solver_type, d->solver_tolerance,
                              d->solver_max_iter, NULL, 0, its, &done);
    if (log)
      for (i = 0; i < done; ++i)
        fprintf(log, "Dynamic step %d finished: time %.17g, %d iterations\n", i + 1, (i + 1) * d->dynamics_dt, its[i]);
  }
  free(its);
  if (rc) return rc;
  if (done < n && log) fprintf(log, "Unable to finish dynamic step %d in %d Newton iterations,exit\n", done + 1, d->max_newton_count);
  k.steps = last; k.cap = 1; k.S = NULL; k.log = log; k.explicit_run = 0;
  rc = keep_snapshot(d, ctx, 0, &k);
  free(k.S);
  return rc ? rc : done;
}

int fea_modal_run(const fea_deck *d, feahip_ctx *ctx, void *log_, const char *msh_path)
{
  FILE *log = (FILE *)log_, *f;
  const int locked = d->modal_count > 0 || d->modal_shift != 0.0;       /* :count or :shift: the locked solve */
  int n = d->modal_count > 0 ? d->modal_count : d->modal_modes;
  double lam[FEA_MODAL_MAX_LOCKED], res[FEA_MODAL_MAX_LOCKED], *phi;
  int k, i, its = 0, rc, solved;
  if (n <= 0) return 0;
  solved = locked ? feahip_solve_modes_locked(ctx, n, d->modal_shift, d->modal_tolerance, d->modal_max, lam, res, &its, NULL)
                  : feahip_solve_modes(ctx, n, d->modal_tolerance, d->modal_max, 0, lam, res, &its);
  if (solved && solved != FEAHIP_ENOTCONVERGED) return solved;
  if (log) {
    if (solved) fprintf(log, "Modal analysis not converged in %d steps\n", its);
    else fprintf(log, "Modal analysis finished: %d modes, %d steps\n", n, its);
  }
  if (locked && solved && (rc = feahip_get_locked_count(ctx, &n))) return rc;   /* the steps ran out: the modes locked so far */
  if (log) {
    for (k = 0; k < n; ++k)
      fprintf(log, "Mode %d: omega^2 = %.17g, f = %.17g Hz\n", k + 1, lam[k], sqrt(lam[k] > 0 ? lam[k] : 0.0) / 6.283185307179586);
  }
  if (!msh_path || n == 0) return 0;
  phi = (double *)malloc(sizeof(double) * 3 * (size_t)d->nodes_count * (size_t)n);
  if (!phi) return FEAHIP_ENOMEM;
  if ((rc = locked ? feahip_get_locked_modes(ctx, 0, n, phi) : feahip_get_modes(ctx, 0, n, phi))) { free(phi); return rc; }
  if (!(f = fopen(msh_path, "a"))) { free(phi); return FEAHIP_EINVAL; }
  for (k = 0; k < n; ++k) {
    const double *p = phi + (size_t)k * 3 * d->nodes_count;
    fprintf(f, "$NodeData\n1\n\"Mode %d\"\n1\n%f\n3\n%d\n3\n%d\n", k + 1, sqrt(lam[k] > 0 ? lam[k] : 0.0) / 6.283185307179586, k,
            d->nodes_count);
    for (i = 0; i < d->nodes_count; ++i) fprintf(f, "%d %f %f %f\n", i + 1, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    fprintf(f, "$EndNodeData\n");
  }
  fclose(f);
  free(phi);
  return 0;
}

static int append_scalar(const char *msh_path, const fea_deck *d, const char *name, const double *v);
static double largest_of(const double *vm, int n, int *node);

/* :stress t of (harmonic ...) and (transient ...): the stress store on the modes and the load held, then the largest von
 * Mises stress of every node over the sweep (g NULL: n frequencies omega) or over the history (n steps of dt under g), one
 * log line and one $NodeData section */
static int stress_peak_run(const fea_deck *d, feahip_ctx *ctx, FILE *log, const char *msh_path, int n, const double *omega,
                           const double *g, double dt, const double *zeta)
{
  const size_t N = (size_t)d->nodes_count;
  const double alpha = d->has_dynamics ? d->damping_alpha : 0.0, beta = d->has_dynamics ? d->damping_beta : 0.0;
  double *p6 = (double *)malloc(sizeof(double) * 7 * N), *vm, best;
  int *a6 = (int *)malloc(sizeof(int) * 7 * N), *vat, node = 0, rc;
  if (!p6 || !a6) { free(p6); free(a6); return FEAHIP_ENOMEM; }
  vm = p6 + 6 * N; vat = a6 + 6 * N;
  rc = feahip_response_stress_basis(ctx, -1);
  if (!rc) rc = g ? feahip_response_stress_transient(ctx, n, dt, g, alpha, beta, zeta, p6, a6, vm, vat, 0, NULL, NULL)
                  : feahip_response_stress_sweep(ctx, n, omega, alpha, beta, zeta, p6, a6, vm, vat, 0, NULL, NULL, NULL);
  if (!rc && log) {
    best = largest_of(vm, d->nodes_count, &node);
    if (g) fprintf(log, "Transient peak von Mises: vm = %.17g, node %d, t = %.17g\n", best, node + 1, vat[node] * dt);
    else fprintf(log, "Harmonic peak von Mises: vm = %.17g, node %d, f = %.17g Hz\n", best, node + 1, omega[vat[node]] / 6.283185307179586);
  }
  if (!rc && msh_path) rc = append_scalar(msh_path, d, g ? "Transient peak von Mises stress" : "Harmonic peak von Mises stress", vm);
  free(p6); free(a6);
  return rc;
}

/* :sn-exponent b of (transient ... :stress t): the rainflow count of the six components of every node over the history on
 * the stress store stress_peak_run made, one log line (two if a stack overflowed) and one $NodeData section */
static int rainflow_run(const fea_deck *d, feahip_ctx *ctx, FILE *log, const char *msh_path, int n, const double *g, double dt,
                        const double *zeta)
{
  const size_t N = (size_t)d->nodes_count;
  const double alpha = d->has_dynamics ? d->damping_alpha : 0.0, beta = d->has_dynamics ? d->damping_beta : 0.0;
  double *dmg = (double *)malloc(sizeof(double) * 13 * N), *cyc, *top, best = -1.0;
  int *st = (int *)malloc(sizeof(int) * 6 * N), rc, over = 0, at = 0;
  size_t i;
  if (!dmg || !st) { free(dmg); free(st); return FEAHIP_ENOMEM; }
  cyc = dmg + 6 * N; top = dmg + 12 * N;
  rc = feahip_response_stress_rainflow(ctx, n, dt, g, alpha, beta, zeta, d->transient_sn_exponent, d->transient_sn_coefficient,
                                       d->transient_rainflow_depth, 0, NULL, dmg, cyc, NULL, st, NULL, 0, NULL, NULL);
  if (!rc) {
    for (i = 0; i < 6 * N; ++i) {                        /* the largest damage (the lowest row among equals), per node the largest of six */
      if (dmg[i] > best) { best = dmg[i]; at = (int)i; }
      if (i % 6 == 0 || dmg[i] > top[i / 6]) top[i / 6] = dmg[i];
      over += (st[i] & FEAHIP_RAINFLOW_OVERFLOW) != 0;
    }
    if (log) {
      fprintf(log, "Transient fatigue: damage = %.17g (rainflow), node %d, component %d, cycles = %.17g\n", best, at / 6 + 1, at % 6, cyc[at]);
      if (over) fprintf(log, "Transient fatigue: %d of %d stress rows overflowed the stack of %d points\n", over, (int)(6 * N), d->transient_rainflow_depth);
    }
    if (msh_path) rc = append_scalar(msh_path, d, "Fatigue damage (rainflow)", top);
  }
  free(dmg); free(st);
  return rc;
}

int fea_harmonic_run(const fea_deck *d, feahip_ctx *ctx, void *log_, const char *msh_path)
{
  FILE *log = (FILE *)log_, *f;
  const int n = d->harmonic_count, nd = 3 * d->nodes_count;
  const double two_pi = 6.283185307179586;
  double *F, *peak, *omega, zeta[FEA_MODAL_MAX_LOCKED], best = -1.0;
  int *at, i, k, m = 0, rc, any = 0, best_dof = 0;
  if (n <= 0) return 0;
  if ((rc = feahip_get_locked_count(ctx, &m))) return rc;
  F = (double *)malloc(sizeof(double) * 2 * (size_t)nd);
  omega = (double *)malloc(sizeof(double) * (size_t)n);
  at = (int *)malloc(sizeof(int) * (size_t)nd);
  if (!F || !omega || !at) { free(F); free(omega); free(at); return FEAHIP_ENOMEM; }
  peak = F + nd;
  for (k = 0; k < n; ++k)                               /* n linearly spaced frequencies in Hz, the ends included */
    omega[k] = two_pi * (n > 1 ? d->harmonic_from + (d->harmonic_to - d->harmonic_from) * k / (n - 1) : d->harmonic_from);
  for (k = 0; k < FEA_MODAL_MAX_LOCKED; ++k) zeta[k] = d->harmonic_zeta;
  rc = feahip_get_surface_forces(ctx, F);
  for (i = 0; !rc && i < nd; ++i) any |= F[i] != 0.0;
  if (!rc && !any) {
    if (log) fprintf(log, "Harmonic: the surface load at the state reached is zero, nothing to sweep\n");
    rc = FEAHIP_EINVAL;
  }
  if (!rc && log)
    fprintf(log, "Harmonic: %d frequencies %.17g .. %.17g Hz, %d modes, static correction %s\n", n, d->harmonic_from,
            d->harmonic_to, m, d->harmonic_static ? "on" : "off");
  if (!rc) rc = feahip_response_load(ctx, F, d->harmonic_static, d->solver_type, d->solver_tolerance, d->solver_max_iter, NULL, NULL, NULL);
  if (!rc) rc = feahip_response_sweep(ctx, n, omega, d->has_dynamics ? d->damping_alpha : 0.0, d->has_dynamics ? d->damping_beta : 0.0,
                                      d->harmonic_zeta > 0 ? zeta : NULL, peak, at, 0, NULL, NULL, NULL);
  if (rc) { free(F); free(omega); free(at); return rc; }
  for (i = 0; i < nd; ++i) if (peak[i] > best) { best = peak[i]; best_dof = i; }
  if (log)
    fprintf(log, "Harmonic peak: |u| = %.17g at f = %.17g Hz, node %d dof %d\n", best, omega[at[best_dof]] / two_pi,
            best_dof / 3 + 1, best_dof % 3);
  if (msh_path) {
    if (!(f = fopen(msh_path, "a"))) { free(F); free(omega); free(at); return FEAHIP_EINVAL; }
    fprintf(f, "$NodeData\n1\n\"Harmonic peak amplitude\"\n1\n%f\n3\n0\n3\n%d\n", omega[at[best_dof]] / two_pi, d->nodes_count);
    for (i = 0; i < d->nodes_count; ++i) fprintf(f, "%d %.9e %.9e %.9e\n", i + 1, peak[3 * i], peak[3 * i + 1], peak[3 * i + 2]);
    fprintf(f, "$EndNodeData\n");
    fprintf(f, "$NodeData\n1\n\"Harmonic peak frequency\"\n1\n%f\n3\n0\n3\n%d\n", omega[at[best_dof]] / two_pi, d->nodes_count);
    for (i = 0; i < d->nodes_count; ++i)
      fprintf(f, "%d %.9e %.9e %.9e\n", i + 1, omega[at[3 * i]] / two_pi, omega[at[3 * i + 1]] / two_pi, omega[at[3 * i + 2]] / two_pi);
    fprintf(f, "$EndNodeData\n");
    fclose(f);
  }
  if (d->harmonic_stress) rc = stress_peak_run(d, ctx, log, msh_path, n, omega, NULL, 0.0, d->harmonic_zeta > 0 ? zeta : NULL);
  free(F); free(omega); free(at);
  return rc;
}

/* g(t) of (transient :shape ...) */
static double transient_shape_at(const fea_deck *d, double t)
{
  const double pi = 3.141592653589793;
  if (d->transient_shape == FEA_SHAPE_RAMP) return t < d->transient_rise ? t / d->transient_rise : 1.0;
  if (d->transient_shape == FEA_SHAPE_HALF_SINE) return t < d->transient_rise ? sin(pi * t / d->transient_rise) : 0.0;
  return 1.0;
}

int fea_transient_run(const fea_deck *d, feahip_ctx *ctx, void *log_, const char *msh_path)
{
  static const char *shape[] = {"step", "ramp", "half-sine"};
  FILE *log = (FILE *)log_, *f;
  const int n = d->transient_steps, nd = 3 * d->nodes_count;
  double *F, *peak, *g, zeta[FEA_MODAL_MAX_LOCKED], gamma[FEA_MODAL_MAX_LOCKED], eff[FEA_MODAL_MAX_LOCKED], total = 0, best = -1.0;
  int *at, i, k, m = 0, rc, any = 0, best_dof = 0;
  if (n <= 0) return 0;
  if ((rc = feahip_get_locked_count(ctx, &m))) return rc;
  F = (double *)malloc(sizeof(double) * 2 * (size_t)nd);
  g = (double *)malloc(sizeof(double) * ((size_t)n + 1));
  at = (int *)malloc(sizeof(int) * (size_t)nd);
  if (!F || !g || !at) { free(F); free(g); free(at); return FEAHIP_ENOMEM; }
  peak = F + nd;
  for (k = 0; k <= n; ++k) g[k] = transient_shape_at(d, k * d->transient_dt);
  for (k = 0; k < FEA_MODAL_MAX_LOCKED; ++k) zeta[k] = d->transient_zeta;
  if (!d->transient_has_base) {
    rc = feahip_get_surface_forces(ctx, F);
    for (i = 0; !rc && i < nd; ++i) any |= F[i] != 0.0;
    if (!rc && !any) {
      if (log) fprintf(log, "Transient: the surface load at the state reached is zero, nothing to run\n");
      rc = FEAHIP_EINVAL;
    }
  }
  if (!rc && log)
    fprintf(log, "Transient: %d steps of %.17g, shape %s, %d modes, static correction %s\n", n, d->transient_dt,
            shape[d->transient_shape], m, d->transient_static ? "on" : "off");
  if (!rc && d->transient_has_base) {
    rc = feahip_response_base_load(ctx, d->transient_base, d->transient_static, d->solver_type, d->solver_tolerance,
                                   d->solver_max_iter, NULL, gamma, eff, &total, NULL, NULL);
    if (!rc && log) {
      double sum = 0;
      for (k = 0; k < m; ++k) {
        sum += eff[k];
        fprintf(log, "Effective mass: mode %d, gamma %.17g, m_eff %.17g, cumulative fraction %.17g of total %.17g\n", k + 1,
                gamma[k], eff[k], sum / total, total);
      }
    }
  } else if (!rc)
    rc = feahip_response_load(ctx, F, d->transient_static, d->solver_type, d->solver_tolerance, d->solver_max_iter, NULL, NULL, NULL);
  if (!rc) rc = feahip_response_transient(ctx, n, d->transient_dt, g, d->has_dynamics ? d->damping_alpha : 0.0,
                                          d->has_dynamics ? d->damping_beta : 0.0, d->transient_zeta > 0 ? zeta : NULL, 0, peak, at,
                                          0, NULL, NULL, 0, NULL, NULL);
  if (rc) { free(F); free(g); free(at); return rc; }
  for (i = 0; i < nd; ++i) if (peak[i] > best) { best = peak[i]; best_dof = i; }
  if (log)
    fprintf(log, "Transient peak: |u| = %.17g at t = %.17g, node %d dof %d\n", best, at[best_dof] * d->transient_dt,
            best_dof / 3 + 1, best_dof % 3);
  if (msh_path) {
    if (!(f = fopen(msh_path, "a"))) { free(F); free(g); free(at); return FEAHIP_EINVAL; }
    fprintf(f, "$NodeData\n1\n\"Transient peak displacement\"\n1\n%f\n3\n0\n3\n%d\n", at[best_dof] * d->transient_dt, d->nodes_count);
    for (i = 0; i < d->nodes_count; ++i) fprintf(f, "%d %.9e %.9e %.9e\n", i + 1, peak[3 * i], peak[3 * i + 1], peak[3 * i + 2]);
    fprintf(f, "$EndNodeData\n");
    fprintf(f, "$NodeData\n1\n\"Transient peak time\"\n1\n%f\n3\n0\n3\n%d\n", at[best_dof] * d->transient_dt, d->nodes_count);
    for (i = 0; i < d->nodes_count; ++i)
      fprintf(f, "%d %.9e %.9e %.9e\n", i + 1, at[3 * i] * d->transient_dt, at[3 * i + 1] * d->transient_dt, at[3 * i + 2] * d->transient_dt);
    fprintf(f, "$EndNodeData\n");
    fclose(f);
  }
  if (d->transient_stress) rc = stress_peak_run(d, ctx, log, msh_path, n, NULL, g, d->transient_dt, d->transient_zeta > 0 ? zeta : NULL);
  if (!rc && d->transient_stress && d->transient_sn_exponent > 0)
    rc = rainflow_run(d, ctx, log, msh_path, n, g, d->transient_dt, d->transient_zeta > 0 ? zeta : NULL);
  free(F); free(g); free(at);
  return rc;
}

/* the load of (spectrum ...) and (random ...): with a base direction the base load, else the surface load of the state
 * reached (all zero: a log line and FEAHIP_EINVAL); F[3N] is scratch */
static int combine_load(const fea_deck *d, feahip_ctx *ctx, FILE *log, const char *who, int has_base, const double *base,
                        int correction, double *F)
{
  const int nd = 3 * d->nodes_count;
  int i, rc, any = 0;
  if (has_base)
    return feahip_response_base_load(ctx, base, correction, d->solver_type, d->solver_tolerance, d->solver_max_iter, NULL, NULL,
                                     NULL, NULL, NULL, NULL);
  if ((rc = feahip_get_surface_forces(ctx, F))) return rc;
  for (i = 0; i < nd; ++i) any |= F[i] != 0.0;
  if (!any) {
    if (log) fprintf(log, "%s: the surface load at the state reached is zero, nothing to run\n", who);
    return FEAHIP_EINVAL;
  }
  return feahip_response_load(ctx, F, correction, d->solver_type, d->solver_tolerance, d->solver_max_iter, NULL, NULL, NULL);
}

/* one $NodeData section of three components per node behind the file */
static int append_field(const char *msh_path, const fea_deck *d, const char *name, const double *v)
{
  FILE *f = fopen(msh_path, "a");
  int i;
  if (!f) return FEAHIP_EINVAL;
  fprintf(f, "$NodeData\n1\n\"%s\"\n1\n%f\n3\n0\n3\n%d\n", name, 0.0, d->nodes_count);
  for (i = 0; i < d->nodes_count; ++i) fprintf(f, "%d %.9e %.9e %.9e\n", i + 1, v[3 * i], v[3 * i + 1], v[3 * i + 2]);
  fprintf(f, "$EndNodeData\n");
  fclose(f);
  return 0;
}

/* one $NodeData section of one component per node behind the file */
static int append_scalar(const char *msh_path, const fea_deck *d, const char *name, const double *v)
{
  FILE *f = fopen(msh_path, "a");
  int i;
  if (!f) return FEAHIP_EINVAL;
  fprintf(f, "$NodeData\n1\n\"%s\"\n1\n%f\n3\n0\n1\n%d\n", name, 0.0, d->nodes_count);
  for (i = 0; i < d->nodes_count; ++i) fprintf(f, "%d %.9e\n", i + 1, v[i]);
  fprintf(f, "$EndNodeData\n");
  fclose(f);
  return 0;
}

/* the largest of vm[n] and its node (the lowest among equals) */
static double largest_of(const double *vm, int n, int *node)
{
  double best = -1.0;
  int i;
  *node = 0;
  for (i = 0; i < n; ++i) if (vm[i] > best) { best = vm[i]; *node = i; }
  return best;
}

int fea_spectrum_run(const fea_deck *d, feahip_ctx *ctx, void *log_, const char *msh_path)
{
  static const char *rule[] = {"srss", "cqc", "abs"};
  FILE *log = (FILE *)log_;
  const int n = d->spectrum_count, nd = 3 * d->nodes_count;
  const double two_pi = 6.283185307179586;
  double *F, *peak, *w, *sa, zeta[FEA_MODAL_MAX_LOCKED], best = -1.0;
  int i, k, m = 0, rc, best_dof = 0;
  if (!d->has_spectrum || n <= 0) return 0;
  if ((rc = feahip_get_locked_count(ctx, &m))) return rc;
  F = (double *)malloc(sizeof(double) * 2 * (size_t)nd);
  w = (double *)malloc(sizeof(double) * 2 * (size_t)n);
  if (!F || !w) { free(F); free(w); return FEAHIP_ENOMEM; }
  peak = F + nd; sa = w + n;
  for (k = 0; k < n; ++k) { w[k] = two_pi * d->spectrum_points[2 * k]; sa[k] = d->spectrum_points[2 * k + 1]; }
  for (k = 0; k < FEA_MODAL_MAX_LOCKED; ++k) zeta[k] = d->spectrum_zeta;
  rc = combine_load(d, ctx, log, "Spectrum", d->spectrum_has_base, d->spectrum_base, d->spectrum_static, F);
  if (!rc) rc = feahip_response_spectrum(ctx, n, w, sa, d->spectrum_loglog, d->spectrum_rule, d->has_dynamics ? d->damping_alpha : 0.0,
                                         d->has_dynamics ? d->damping_beta : 0.0, d->spectrum_zeta > 0 ? zeta : NULL, d->spectrum_zpa,
                                         0, peak, NULL);
  if (rc) { free(F); free(w); return rc; }
  for (i = 0; i < nd; ++i) if (peak[i] > best) { best = peak[i]; best_dof = i; }
  if (log)
    fprintf(log, "Spectrum peak: |u| = %.17g, node %d dof %d, rule %s, %d modes\n", best, best_dof / 3 + 1, best_dof % 3,
            rule[d->spectrum_rule], m);
  if (msh_path) rc = append_field(msh_path, d, "Spectrum peak displacement", peak);
  if (!rc && d->spectrum_stress) {                      /* :stress t: the peak von Mises stress on the same modes and load */
    double *p6 = (double *)malloc(sizeof(double) * 7 * (size_t)d->nodes_count), *vm;
    int node = 0;
    if (!p6) { free(F); free(w); return FEAHIP_ENOMEM; }
    vm = p6 + 6 * (size_t)d->nodes_count;
    rc = feahip_response_stress_basis(ctx, -1);
    if (!rc) rc = feahip_response_stress_spectrum(ctx, n, w, sa, d->spectrum_loglog, d->spectrum_rule, d->has_dynamics ? d->damping_alpha : 0.0,
                                                  d->has_dynamics ? d->damping_beta : 0.0, d->spectrum_zeta > 0 ? zeta : NULL,
                                                  d->spectrum_zpa, p6, vm, NULL);
    if (!rc && log) {
      best = largest_of(vm, d->nodes_count, &node);
      fprintf(log, "Spectrum peak von Mises: vm = %.17g, node %d, rule %s, %d modes\n", best, node + 1, rule[d->spectrum_rule], m);
    }
    if (!rc && msh_path) rc = append_scalar(msh_path, d, "Spectrum peak von Mises stress", vm);
    free(p6);
  }
  free(F); free(w);
  return rc;
}

int fea_random_run(const fea_deck *d, feahip_ctx *ctx, void *log_, const char *msh_path)
{
  FILE *log = (FILE *)log_;
  const int n = d->random_count, nd = 3 * d->nodes_count;
  const double two_pi = 6.283185307179586;
  const double alpha = d->has_dynamics ? d->damping_alpha : 0.0, beta = d->has_dynamics ? d->damping_beta : 0.0;
  double *F, *rms, *w, *S, *omega = NULL, *Sw, lam[FEA_MODAL_MAX_LOCKED], zeta[FEA_MODAL_MAX_LOCKED], best = -1.0;
  int i, k, m = 0, rc, best_dof = 0, n_grid = 0, cap;
  if (!d->has_random || n < 2) return 0;
  if ((rc = feahip_get_locked_count(ctx, &m))) return rc;
  F = (double *)malloc(sizeof(double) * 2 * (size_t)nd);
  w = (double *)malloc(sizeof(double) * 2 * (size_t)n);
  cap = d->random_background + FEA_MODAL_MAX_LOCKED * d->random_per_mode + n;
  omega = (double *)malloc(sizeof(double) * 2 * (size_t)cap);
  if (!F || !w || !omega) { free(F); free(w); free(omega); return FEAHIP_ENOMEM; }
  rms = F + nd; S = w + n; Sw = omega + cap;
  for (k = 0; k < n; ++k) {                             /* per Hz over Hz to per rad/s over rad/s: S_f df = S_w dw */
    w[k] = two_pi * d->random_points[2 * k]; S[k] = d->random_points[2 * k + 1] / two_pi;
    omega[k] = w[k];                                    /* the table's abscissae are breakpoints of the grid */
  }
  for (k = 0; k < FEA_MODAL_MAX_LOCKED; ++k) zeta[k] = d->random_zeta;
  rc = combine_load(d, ctx, log, "Random", d->random_has_base, d->random_base, d->random_static, F);
  if (!rc) rc = feahip_get_locked_lambda(ctx, 0, m, lam);
  if (!rc) {
    n_grid = n;
    rc = feahip_host_random_grid(m, lam, alpha, beta, d->random_zeta > 0 ? zeta : NULL, w[0], w[n - 1], d->random_background,
                                 d->random_per_mode, omega, &n_grid);
  }
  for (k = 0; !rc && k < n_grid; ++k) Sw[k] = feahip_host_psd_value(n, w, S, d->random_loglog, omega[k]);
  if (!rc) rc = feahip_response_random(ctx, n_grid, omega, Sw, alpha, beta, d->random_zeta > 0 ? zeta : NULL, 0, rms, NULL);
  if (rc) { free(F); free(w); free(omega); return rc; }
  for (i = 0; i < nd; ++i) if (rms[i] > best) { best = rms[i]; best_dof = i; }
  if (log)
    fprintf(log, "Random RMS: |u| = %.17g, node %d dof %d, %d grid points, %d modes\n", best, best_dof / 3 + 1, best_dof % 3, n_grid, m);
  if (msh_path) rc = append_field(msh_path, d, "RMS displacement", rms);
  if (!rc && d->random_stress) {                        /* :stress t: the RMS von Mises stress on the same modes, load and grid */
    double *p6 = (double *)malloc(sizeof(double) * 7 * (size_t)d->nodes_count), *vm;
    int node = 0;
    if (!p6) { free(F); free(w); free(omega); return FEAHIP_ENOMEM; }
    vm = p6 + 6 * (size_t)d->nodes_count;
    rc = feahip_response_stress_basis(ctx, -1);
    if (!rc) rc = feahip_response_stress_random(ctx, n_grid, omega, Sw, alpha, beta, d->random_zeta > 0 ? zeta : NULL, p6, vm, NULL);
    if (!rc && log) {
      best = largest_of(vm, d->nodes_count, &node);
      fprintf(log, "Random RMS von Mises: vm = %.17g, node %d, %d grid points, %d modes\n", best, node + 1, n_grid, m);
    }
    if (!rc && msh_path) rc = append_scalar(msh_path, d, "RMS von Mises stress", vm);
    free(p6);
  }
  if (!rc && d->random_sn_exponent > 0) {               /* :sn-exponent b: fatigue of the von Mises process on the same modes, load and grid */
    const size_t N = (size_t)d->nodes_count;
    double *rates = (double *)malloc(sizeof(double) * (14 + 21 + 2) * N), *damage, *dk, *nu0;
    int node = 0;
    if (!rates) { free(F); free(w); free(omega); return FEAHIP_ENOMEM; }
    damage = rates + 14 * N; dk = damage + 21 * N; nu0 = dk + N;
    rc = feahip_response_stress_basis(ctx, -1);
    if (!rc) rc = feahip_response_stress_fatigue(ctx, n_grid, omega, Sw, alpha, beta, d->random_zeta > 0 ? zeta : NULL, d->random_sn_exponent,
                                                 d->random_sn_coefficient, NULL, rates, damage, NULL);
    for (i = 0; !rc && i < d->nodes_count; ++i) {       /* process 6: von Mises; damage 1: Dirlik */
      dk[i] = d->random_duration * damage[((size_t)i * 7 + 6) * 3 + 1];
      nu0[i] = rates[((size_t)i * 7 + 6) * 2];
    }
    if (!rc && log) {
      best = largest_of(dk, d->nodes_count, &node);
      fprintf(log, "Random fatigue: damage = %.17g (Dirlik), node %d, nu0 = %.17g, life = %.17g\n", best, node + 1, nu0[node],
              d->random_duration / best);
    }
    if (!rc && msh_path) rc = append_scalar(msh_path, d, "Fatigue damage (Dirlik)", dk);
    if (!rc && msh_path) rc = append_scalar(msh_path, d, "Zero-upcrossing rate", nu0);
    free(rates);
  }
  free(F); free(w); free(omega);
  return rc;
}

int fea_buckling_run(const fea_deck *d, feahip_ctx *ctx, void *log_, const char *msh_path)
{
  FILE *log = (FILE *)log_, *f;
  const int n = d->buckling_modes;
  double fac[FEA_MODAL_COLS], nu[FEA_MODAL_COLS], *phi;
  int k, i, its = 0, rc, solved;
  if (n <= 0) return 0;
  solved = feahip_solve_buckling(ctx, n, d->buckling_tolerance, d->buckling_max, fac, nu, NULL, &its);
  if (solved == FEAHIP_ENOTCONVERGED && nu[0] != nu[0]) return solved;  /* K not positive definite: nothing to report */
  if (solved && solved != FEAHIP_ENOTCONVERGED) return solved;
  if (log) {
    if (solved) fprintf(log, "Buckling analysis not converged in %d steps\n", its);
    else fprintf(log, "Buckling analysis finished: %d modes, %d steps\n", n, its);
    for (k = 0; k < n; ++k) fprintf(log, "Buckling mode %d: factor = %.17g, nu = %.17g\n", k + 1, fac[k], nu[k]);
  }
  if (!msh_path) return 0;
  phi = (double *)malloc(sizeof(double) * 3 * (size_t)d->nodes_count * (size_t)n);
  if (!phi) return FEAHIP_ENOMEM;
  if ((rc = feahip_get_buckling_modes(ctx, 0, n, phi))) { free(phi); return rc; }
  if (!(f = fopen(msh_path, "a"))) { free(phi); return FEAHIP_EINVAL; }
  for (k = 0; k < n; ++k) {
    const double *p = phi + (size_t)k * 3 * d->nodes_count;
    fprintf(f, "$NodeData\n1\n\"Buckling mode %d\"\n1\n%f\n3\n%d\n3\n%d\n", k + 1, fac[k], k, d->nodes_count);
    for (i = 0; i < d->nodes_count; ++i) fprintf(f, "%d %f %f %f\n", i + 1, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    fprintf(f, "$EndNodeData\n");
  }
  fclose(f);
  free(phi);
  return 0;
}

int fea_export_gmsh(const char *filename, const fea_deck *d, const fea_step_snapshot *steps, int nsteps)
{
  FILE *f = fopen(filename, "w+");
  int i, j, k, load;
  const int npe = d->nodes_per_element;
  if (!f) return -1;
  fprintf(f, "$MeshFormat\n2.0 0 8\n$EndMeshFormat\n");
  fprintf(f, "$Nodes\n%d\n", d->nodes_count);
  for (i = 0; i < d->nodes_count; ++i)
    fprintf(f, "%d %f %f %f\n", i + 1, d->nodes[3 * i], d->nodes[3 * i + 1], d->nodes[3 * i + 2]);
  fprintf(f, "$EndNodes\n$Elements\n%d\n", d->elements_count);
  for (i = 0; i < d->elements_count; ++i) {
    const int *c = d->elements + (size_t)i * npe;
    const int tag = d->materials_count > 0 ? d->element_material[i] + 1 : 1;   /* physical entity: the material, from 1 */
    if (npe == 10) {                       /* our 8 <-> Gmsh 9 (fea_solver.c:1430-1434) */
      fprintf(f, "%d 11 3 %d 1 1 ", i + 1, tag);
      for (j = 0; j < 8; ++j) fprintf(f, "%d ", c[j] + 1);
      fprintf(f, "%d %d \n", c[9] + 1, c[8] + 1);
    } else if (npe == 8) {                 /* Gmsh type 5, 8-node hexahedron: the same corner order */
      fprintf(f, "%d 5 3 %d 1 1 ", i + 1, tag);
      for (j = 0; j < 8; ++j) fprintf(f, "%d ", c[j] + 1);
      fprintf(f, "\n");
    } else {
      fprintf(f, "%d 4 3 %d 1 1 ", i + 1, tag);
      for (j = 0; j < 4; ++j) fprintf(f, "%d ", c[j] + 1);
      fprintf(f, "\n");
    }
  }
  fprintf(f, "$EndElements\n");
  for (load = 0; load <= nsteps; ++load) {                       /* :1440, load 0 = zeros */
    fprintf(f, "$NodeData\n1\n\"Displacements\"\n1\n%f\n3\n%d\n3\n%d\n", load * 0.83333333, load, d->nodes_count);
    for (i = 0; i < d->nodes_count; ++i) {
      double u[3] = {0, 0, 0};
      if (load)
        for (j = 0; j < 3; ++j) u[j] = steps[load - 1].nodes[3 * i + j] - d->nodes[3 * i + j];
      fprintf(f, "%d %f %f %f\n", i + 1, u[0], u[1], u[2]);
    }
    fprintf(f, "$EndNodeData\n");
    fprintf(f, "$ElementData\n1\n\"Stress tensor\"\n1\n%f\n3\n%d\n9\n%d\n", load * 0.83333333, load, d->elements_count);
    for (i = 0; i < d->elements_count; ++i) {
      fprintf(f, "%d ", i + 1);
      for (j = 0; j < 3; ++j)
        for (k = 0; k < 3; ++k)
          fprintf(f, "%f ", load ? steps[load - 1].stress0[(size_t)i * 9 + 3 * j + k] : 0.0);
      fprintf(f, "\n");
    }
    fprintf(f, "$EndElementData\n");
    if (load && steps[load - 1].nodal_stress && steps[load - 1].von_mises) {   /* (results :nodal-stress t) */
      static const int at[9] = {0, 3, 5, 3, 1, 4, 5, 4, 2};                    /* xx xy xz / xy yy yz / xz yz zz */
      const double *s6 = steps[load - 1].nodal_stress, *vm = steps[load - 1].von_mises;
      fprintf(f, "$NodeData\n1\n\"Nodal stress\"\n1\n%f\n3\n%d\n9\n%d\n", load * 0.83333333, load, d->nodes_count);
      for (i = 0; i < d->nodes_count; ++i) {
        fprintf(f, "%d ", i + 1);
        for (j = 0; j < 9; ++j) fprintf(f, "%f ", s6[(size_t)i * 6 + at[j]]);
        fprintf(f, "\n");
      }
      fprintf(f, "$EndNodeData\n");
      fprintf(f, "$NodeData\n1\n\"Von Mises\"\n1\n%f\n3\n%d\n1\n%d\n", load * 0.83333333, load, d->nodes_count);
      for (i = 0; i < d->nodes_count; ++i) fprintf(f, "%d %f\n", i + 1, vm[i]);
      fprintf(f, "$EndNodeData\n");
    }
    if (load && steps[load - 1].contact_pressure) {                            /* a deck with (contact ...) */
      const double *t = steps[load - 1].contact_pressure;
      fprintf(f, "$NodeData\n1\n\"Contact pressure\"\n1\n%f\n3\n%d\n1\n%d\n", load * 0.83333333, load, d->nodes_count);
      for (i = 0; i < d->nodes_count; ++i) fprintf(f, "%d %f\n", i + 1, t[i]);
      fprintf(f, "$EndNodeData\n");
    }
  }
  fclose(f);
  return 0;
}
