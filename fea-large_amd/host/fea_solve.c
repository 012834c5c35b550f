/*
 * fea_solve.c -- the load-increment / Newton driver and the Gmsh export,
 * in C on the host, exactly where the reference has them.
 *
 * fea_solve() is solve() of solver-large/fea_solver.c:130-242 with each
 * solver_* call replaced by its C-ABI twin (include/fea_hip.h).  The host
 * never touches element data inside the loops: one scalar (<u,f>) comes back
 * per Newton iteration, which is all the control flow needs.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fea_host.h"

int fea_mass_points(int ele_type)
{
  return ele_type == FEA_TETRAHEDRA4 ? 4 : ele_type == FEA_TETRAHEDRA10 ? 27 : ele_type == FEA_HEXAHEDRA8 ? 8 : 0;
}

/* the deck's uniform mass, its body force and its damping (at the reference configuration the context starts from) */
static int install_mass(const fea_deck *d, feahip_ctx *ctx)
{
  double w[32], forms[32 * 10], dforms[32 * 3 * 10];
  const int gm = fea_mass_points(d->ele_type);
  int rc;
  if (gm <= 0 || fea_element_tables(d->ele_type, gm, w, forms, dforms) != d->nodes_per_element) return FEAHIP_EINVAL;
  if ((rc = feahip_set_mass(ctx, 1, &d->density, gm, w, forms, dforms))) return rc;
  if (d->has_body_force && (rc = feahip_set_body_force(ctx, d->body_force))) return rc;
  return (d->damping_alpha != 0 || d->damping_beta != 0) ? feahip_set_damping(ctx, d->damping_alpha, d->damping_beta) : 0;
}

int fea_deck_create_solver(const fea_deck *d, int device, feahip_ctx **ctx, char *errbuf, int errlen)
{
  double w[32], dforms[32 * 3 * 10];
  int npe = fea_element_tables(d->ele_type, d->gauss_nodes_count, w, NULL, dforms);
  int rc;
  if (npe < 0 || npe != d->nodes_per_element) {
    if (errbuf) snprintf(errbuf, (size_t)errlen, "unsupported element type / gauss rule (%d nodes, %d points)",
                         d->nodes_per_element, d->gauss_nodes_count);
    return FEAHIP_EINVAL;
  }
  rc = feahip_create(ctx, device, d->nodes_count, d->elements_count, npe, d->gauss_nodes_count, w, dforms,
                     d->elements, d->nodes, d->model, d->parameters, d->parameters_count,
                     d->prescribed_nodes_count, d->presc_node, d->presc_type, d->presc_values);
  if (rc) {
    if (errbuf) snprintf(errbuf, (size_t)errlen, "%s", feahip_create_error());
    return rc;
  }
  if (d->surface_faces_count > 0 &&
      (rc = feahip_set_surface_loads(*ctx, d->surface_faces_count, d->surface_nodes_per_face, d->surface_nodes,
                                     d->surface_kind, d->surface_values))) {
    if (errbuf) snprintf(errbuf, (size_t)errlen, "%s", feahip_last_error(*ctx));
    feahip_destroy(*ctx);
    *ctx = NULL;
    return rc;
  }
  if (d->contact_faces_count > 0 && d->contact_obstacles_count > 0 &&
      (rc = feahip_set_contact(*ctx, d->contact_faces_count, d->contact_nodes_per_face, d->contact_nodes,
                               d->contact_obstacles_count, d->contact_kind, d->contact_geom, d->contact_penalty,
                               d->contact_augment, d->contact_gap_tolerance))) {
    if (errbuf) snprintf(errbuf, (size_t)errlen, "%s", feahip_last_error(*ctx));
    feahip_destroy(*ctx);
    *ctx = NULL;
    return rc;
  }
  if (d->materials_count > 0 &&
      (rc = feahip_set_materials(*ctx, d->materials_count, d->material_params, d->element_material))) {
    if (errbuf) snprintf(errbuf, (size_t)errlen, "%s", feahip_last_error(*ctx));
    feahip_destroy(*ctx);
    *ctx = NULL;
    return rc;
  }
  if (d->has_dynamics && (rc = install_mass(d, *ctx))) {
    if (errbuf) snprintf(errbuf, (size_t)errlen, "%s", feahip_last_error(*ctx));
    feahip_destroy(*ctx);
    *ctx = NULL;
  }
  return rc;
}

/* the log lines of (results :energy t :reactions t) after a finished step */
int fea_log_results(const fea_deck *d, feahip_ctx *ctx, void *logp, int explicit_run)
{
  FILE *log = (FILE *)logp;
  int rc, i;
  if (!log) return 0;
  if (d->results_energy) {
    double W = 0, T = 0;
    if ((rc = feahip_strain_energy(ctx, &W))) return rc;
    if (explicit_run) {
      if ((rc = feahip_kinetic_energy(ctx, &T))) return rc;
      fprintf(log, "Strain energy %.17g, kinetic energy %.17g, total %.17g\n", W, T, W + T);
    } else
      fprintf(log, "Strain energy %.17g\n", W);
  }
  if (d->results_reactions) {
    double *r = (double *)malloc(sizeof(double) * 3 * (size_t)d->nodes_count), sum[3] = {0, 0, 0};
    if (!r) return FEAHIP_ENOMEM;
    if ((rc = feahip_get_reactions(ctx, r))) { free(r); return rc; }
    for (i = 0; i < 3 * d->nodes_count; ++i) sum[i % 3] += r[i];
    free(r);
    fprintf(log, "Reactions sum %.17g %.17g %.17g\n", sum[0], sum[1], sum[2]);
  }
  return 0;
}

#define CALL(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

/* One pass of Newton iterations at the nodes and the load in force (fea_solver.c:177-221): K, its stash, then
 * iterations until the energy passes or max_newton_count of them are spent (*failed).  A load increment is one pass; a
 * deck with (contact ... :augment k) adds one per multiplier update.  *it counts the iterations of all passes. */
static int newton_pass(const fea_deck *d, feahip_ctx *ctx, FILE *log, int *it, int *failed)
{
  int k = 0;
  double tolerance;
  CALL(feahip_create_stiffness(ctx));                                        /* :177 */
  CALL(feahip_stash_stiffness(ctx));                                         /* :179 */
  do {
    (*it)++; k++;
    CALL(feahip_create_residual_forces(ctx));                                /* :185 */
    if (d->modified_newton) CALL(feahip_restore_stiffness(ctx));             /* :194-195 */
    else CALL(feahip_create_stiffness(ctx));                                 /* :200 */
    CALL(feahip_apply_prescribed_bc(ctx, 0));                                /* :203 */
    CALL(feahip_solve_slae(ctx, d->solver_type, d->solver_tolerance,         /* :205 */
                           d->solver_max_iter, NULL, NULL));
    CALL(feahip_energy(ctx, &tolerance));                                    /* :208-210 */
    if (log) {
      fprintf(log, "Tolerance <X,R> = %e\n", tolerance);                     /* :212 */
      fprintf(log, "Newton iteration %d finished\n", *it);                   /* :213 */
    }
    CALL(feahip_update_nodes_with_solution(ctx, NULL));                      /* :216 */
    CALL(feahip_update_state(ctx, NULL));                                    /* :217-218 */
  } while (fabs(tolerance) > d->desired_tolerance && k < d->max_newton_count);   /* :220-221 */
  *failed = k == d->max_newton_count;
  return 0;
}

/* solve() of fea_solver.c:163-236: THE load-increment / Newton loop of the host side (fea_solve and
 * fea_solve_with_snapshots are this loop with two different things done after a converged increment, :233-235).
 * Returns the number of finished increments, or a negative FEAHIP_* code. */
int fea_solve_steps(const fea_deck *d, feahip_ctx *ctx, void *logp, fea_step_fn after_step, void *user)
{
  FILE *log = (FILE *)logp;
  const int contact = d->contact_faces_count > 0 && d->contact_obstacles_count > 0;
  int step, it, failed, aug;
  double info[4] = {0, 0, 0, 0};
  for (step = 0; step < d->load_increments_count; ++step) {                 /* :163 */
    it = 0;
    CALL(feahip_update_nodes_with_bc(ctx, 1));                               /* :168 */
    CALL(feahip_update_state(ctx, NULL));                                    /* :171-174 */
    CALL(newton_pass(d, ctx, log, &it, &failed));
    /* (contact ... :augment k): while the largest penetration exceeds :gap-tolerance, update the multipliers and iterate
     * again at the same load */
    if (contact && !failed) CALL(feahip_contact_info(ctx, info));            /* one reduction per pass: decision and log line */
    for (aug = 0; contact && !failed && aug < d->contact_augment && info[1] > d->contact_gap_tolerance; ++aug) {
      if (log) fprintf(log, "Contact augmentation %d: max penetration %.17g\n", aug + 1, info[1]);
      CALL(feahip_contact_augment(ctx, NULL));
      CALL(newton_pass(d, ctx, log, &it, &failed));
      if (!failed) CALL(feahip_contact_info(ctx, info));
    }
    if (log) fprintf(log, "Load increment %d finished\n", step + 1);         /* :224 */
    if (failed) {                                                            /* :225-231 */
      if (log) fprintf(log, "Unable to finish load step in %d Newton iterations,exit\n", d->max_newton_count);
      break;
    }
    if (contact && log) {
      fprintf(log, "Contact: active %d, force %.17g, max penetration %.17g\n", (int)info[0], info[2], info[1]);
    }
    CALL(fea_log_results(d, ctx, log, 0));                                   /* (results ...): nothing without the section */
    if (after_step) CALL(after_step(d, ctx, step, user));                    /* :233-235 */
  }
  return step;
}

struct node_sink { double *x; int cap; };

static int keep_nodes(const fea_deck *d, feahip_ctx *ctx, int step, void *user)
{
  struct node_sink *k = (struct node_sink *)user;
  if (!k->x || step >= k->cap) return 0;
  return feahip_get_nodes(ctx, k->x + (size_t)step * d->nodes_count * 3);
}

int fea_solve(const fea_deck *d, feahip_ctx *ctx, void *logp, double *x_steps, int x_steps_cap)
{
  struct node_sink k;
  k.x = x_steps; k.cap = x_steps_cap;
  return fea_solve_steps(d, ctx, logp, keep_nodes, &k);
}
