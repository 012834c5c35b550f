/*
 * feasolver_main.c -- `feasolver_hip deck.sexp`: the reference's command line
 * (fea_solver.c:64-128, 324-333) on top of the HIP path.  Loads the deck,
 * runs the load-increment / Newton loop through the C ABI, writes
 * "<base>.msh" like initial_data_load + solve() do.
 *
 * A deck with (arc-length :max N), N > 0, and a (surface-loads ...) section is
 * followed along its equilibrium path by feahip_solve_arclength (N steps at
 * most, up to the load factor load-increments); the file then holds the final
 * state as its one step.  A deck with (dynamics :steps N ...), N > 0, takes N
 * Newmark steps (feahip_solve_dynamic), or with :scheme explicit N explicit
 * steps (feahip_solve_explicit), and likewise writes the final state.
 * Every other deck takes the reference's loop.  A deck with a (results ...)
 * section gets the nodal stress in the file and the strain energy and the
 * reaction sums in the log (fea_host.h).  A deck with (modal :modes N ...)
 * then gets its N lowest natural frequencies at the final state in the log
 * and the mode shapes in the file (feahip_solve_modes).  A deck with
 * (harmonic ...) then gets the frequency sweep of its surface load on those
 * modes: two log lines and the peak amplitude and peak frequency of every dof
 * in the file (feahip_response_load, feahip_response_sweep).  A deck with
 * (transient ...) then gets the time history of that load, or of a base
 * acceleration, on the same modes: the peak displacement and its time per dof
 * (feahip_response_base_load, feahip_response_transient).  A deck with
 * (spectrum ...) or (random ...) then gets the design peak under a response
 * spectrum or the RMS under a PSD on the same modes, one log line and one
 * field each (feahip_response_spectrum, feahip_response_random), and with
 * :stress t in the section the peak or the RMS of the von Mises stress as
 * well, one more log line and one more field (feahip_response_stress_basis,
 * feahip_response_stress_spectrum, feahip_response_stress_random); :stress t
 * in (harmonic ...) or (transient ...) likewise adds the largest von Mises
 * stress of every node over the sweep or the history
 * (feahip_response_stress_sweep, feahip_response_stress_transient);
 * :sn-exponent b :sn-coefficient A :duration T in (random ...) adds the fatigue
 * of the von Mises process, one log line with the largest Dirlik damage and
 * two fields (feahip_response_stress_fatigue); :sn-exponent b
 * :sn-coefficient A :rainflow-depth d in (transient ... :stress t) adds the
 * rainflow count of the history, one log line with the largest Miner damage
 * and one field (feahip_response_stress_rainflow).  A deck with
 * (buckling :modes N ...) then gets its N lowest buckling load factors in the
 * log and their mode shapes in the file (feahip_solve_buckling).  A deck
 * with a (contact ...) section presses its contact faces against rigid
 * obstacles in every loop above but the arc length (feahip_set_contact); the
 * reference's loop then adds the multiplier updates of :augment, one
 * "Contact: active n, force F, max penetration p" line per step and one
 * "Contact pressure" section per step in the file.
 *
 * One option the reference does not have, after the deck name:
 *   --multigrid   PCG_ILU / CHOLESKY solves use the aggregation-multigrid
 *                 preconditioner (feahip_set_preconditioner); an error, not a
 *                 silent return to block-Jacobi, when the mesh is too small
 *                 to coarsen.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fea_host.h"

int main(int argc, char **argv)
{
  fea_deck deck;
  feahip_ctx *ctx = NULL;
  char err[512], *msh;
  fea_step_snapshot *steps;
  int done, rc, cap, arc, dyn, status = 0;
  if (argc < 2) {
    printf("Usage: fea_solve input_data.sexp\n");            /* fea_solver.c:328 */
    return 1;
  }
  if (fea_deck_load(argv[1], &deck, err, sizeof err)) {
    fprintf(stderr, "Error. Unable to load %s: %s\n", argv[1], err);
    return 1;
  }
  printf("Initial data loaded\n");
  if ((rc = fea_deck_create_solver(&deck, 0, &ctx, err, sizeof err))) {
    fprintf(stderr, "feasolve error encountered: %s\n", err);
    fea_deck_free(&deck);
    return 1;
  }
  if (argc > 2 && strcmp(argv[2], "--multigrid") == 0 && feahip_set_preconditioner(ctx, 1)) {
    /* asked for and not available: say so and stop, never run another preconditioner in its place */
    fprintf(stderr, "feasolve error encountered: --multigrid: %s\n", feahip_last_error(ctx));
    feahip_destroy(ctx);
    fea_deck_free(&deck);
    return 1;
  }
  if (deck.has_dynamics && (deck.damping_alpha != 0 || deck.damping_beta != 0))
    printf("Damping: alpha %.17g, beta %.17g\n", deck.damping_alpha, deck.damping_beta);
  cap = deck.load_increments_count > 0 ? deck.load_increments_count : 1;
  steps = (fea_step_snapshot *)calloc((size_t)cap, sizeof *steps);
  /* (arc-length :max N) with N > 0 and surface loads: path following instead of load control */
  arc = deck.arclength_max > 0 && deck.surface_faces_count > 0;
  dyn = deck.has_dynamics && deck.dynamics_steps > 0;
  if (dyn) done = fea_solve_dynamic_with_snapshot(&deck, ctx, stdout, steps);
  else if (arc) done = fea_solve_arclength_with_snapshot(&deck, ctx, stdout, steps);
  else done = fea_solve_with_snapshots(&deck, ctx, stdout, steps, deck.load_increments_count);
  if (done < 0) {
    /* a HIP failure or a broken-down linear solve: the reference's error() exits with EXIT_FAILURE
     * (fea_solver.c:57-61); nothing is exported */
    fprintf(stderr, "feasolve error encountered: %s\n", feahip_last_error(ctx));
    status = 1;
  } else {
    printf("Exporting data...\n");
    msh = (char *)malloc(strlen(argv[1]) + 8);
    fea_export_name(argv[1], msh);
    /* a failed increment leaves current_load_step one lower (fea_solver.c:227), so the
     * reference then drops the last completed step from the file: same here */
    if (fea_export_gmsh(msh, &deck, steps, (arc || dyn) ? 1 : (done == deck.load_increments_count ? done : done - 1))) {
      fprintf(stderr, "could not write %s\n", msh);
      status = 1;
    } else if ((deck.modal_modes > 0 || deck.modal_count > 0) && (rc = fea_modal_run(&deck, ctx, stdout, msh))) {
      /* (modal :modes N ...): the natural frequencies at the state reached, the mode shapes behind the steps */
      fprintf(stderr, "feasolve error encountered: %s\n", feahip_last_error(ctx));
      status = 1;
    } else if (deck.harmonic_count > 0 && (rc = fea_harmonic_run(&deck, ctx, stdout, msh))) {
      /* (harmonic ...): the frequency sweep on the locked modes the modal run left, before anything drops them */
      fprintf(stderr, "feasolve error encountered: harmonic sweep refused or failed (%d): %s\n", rc, feahip_last_error(ctx));
      status = 1;
    } else if (deck.transient_steps > 0 && (rc = fea_transient_run(&deck, ctx, stdout, msh))) {
      /* (transient ...): the time history on the same locked modes, before the buckling run drops them */
      fprintf(stderr, "feasolve error encountered: transient run refused or failed (%d): %s\n", rc, feahip_last_error(ctx));
      status = 1;
    } else if (deck.has_spectrum && (rc = fea_spectrum_run(&deck, ctx, stdout, msh))) {
      /* (spectrum ...): the design peak under a response spectrum on the same locked modes */
      fprintf(stderr, "feasolve error encountered: spectrum run refused or failed (%d): %s\n", rc, feahip_last_error(ctx));
      status = 1;
    } else if (deck.has_random && (rc = fea_random_run(&deck, ctx, stdout, msh))) {
      /* (random ...): the RMS under a PSD on the same locked modes, before the buckling run drops them */
      fprintf(stderr, "feasolve error encountered: random run refused or failed (%d): %s\n", rc, feahip_last_error(ctx));
      status = 1;
    } else if (deck.buckling_modes > 0 && (rc = fea_buckling_run(&deck, ctx, stdout, msh))) {
      /* (buckling :modes N ...): the load factors at the state reached, the mode shapes behind everything else */
      fprintf(stderr, "feasolve error encountered: %s\n", feahip_last_error(ctx));
      status = 1;
    }
    free(msh);
  }
  fea_snapshots_free(steps, cap);                      /* by capacity: an error may leave snapshots behind */
  free(steps);
  feahip_destroy(ctx);
  fea_deck_free(&deck);
  return status;
}
