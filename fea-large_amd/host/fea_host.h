/*
 * fea_host.h -- host side (plain C) above the C ABI of include/fea_hip.h.
 *
 * Keeps what the reference keeps on the host: the S-expression input deck
 * (solver-large/sexp_loader.c), the element plug-in tables
 * (fea_solver.c:32-54, 503-535, 1287-1373), the load-increment / Newton
 * control flow of solve() (fea_solver.c:130-242) and the Gmsh export
 * (fea_solver.c:1375-1488).  Names follow the reference's so that a
 * maintainer can map one onto the other; layouts are flat arrays instead of
 * the reference's pointer-per-row heap objects.
 */
#ifndef FEA_HOST_H
#define FEA_HOST_H

#include "../../include/fea_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FEA_MAX_MATERIAL_PARAMETERS 10   /* defines.h:22 */

typedef enum { FEA_TETRAHEDRA10 = 0, FEA_TETRAHEDRA4 = 1, FEA_HEXAHEDRA8 = 2 } fea_element_type;
#define FEA_DECK_MAX_POINTS 4096               /* points of (spectrum (points ...)) and of (random (psd ...)) */
/* g(t) of (transient :shape ...): 1 from t = 0; min(t / T, 1); sin(pi t / T) up to T and 0 after */
enum { FEA_SHAPE_STEP = 0, FEA_SHAPE_RAMP = 1, FEA_SHAPE_HALF_SINE = 2 };

/* fea_task + fea_solution_params + the three input arrays of the reference
 * (fea_solver.h:94-155), as one flat record                                 */
typedef struct fea_deck {
  /* task */
  int model;                    /* FEAHIP_MODEL_*                            */
  double parameters[FEA_MAX_MATERIAL_PARAMETERS]; /* [0]=lambda [1]=mu       */
  int parameters_count;
  int solver_type;              /* FEAHIP_CG / PCG_ILU / CHOLESKY            */
  double solver_tolerance;
  int solver_max_iter;
  int ele_type;                 /* fea_element_type                          */
  int load_increments_count;
  double desired_tolerance;
  int max_newton_count;
  int linesearch_max, arclength_max;   /* line search: parsed, unused (as the reference); arc length: steps of
                                        * feahip_solve_arclength when > 0 and the deck has surface loads     */
  int modified_newton;
  /* solution params */
  int nodes_per_element, gauss_nodes_count;
  /* geometry */
  int nodes_count;
  double *nodes;                /* [nodes_count][3]                          */
  int elements_count;
  int *elements;                /* [elements_count][nodes_per_element]       */
  /* prescribed displacements, deck order */
  int prescribed_nodes_count;
  int *presc_node, *presc_type;
  double *presc_values;         /* [count][3]                                */
  /* surface loads, deck order: (surface-loads (pressure :value p :nodes (...))
   * (traction :x :y :z :nodes (...)) ...) inside (boundary-conditions ...);
   * node ids as :node-id of prescribed-displacements.  Values are per load
   * increment (feahip_set_surface_loads)                                     */
  int surface_faces_count;
  int surface_nodes_per_face;
  int *surface_nodes;           /* [count][nodes_per_face]                   */
  int *surface_kind;            /* [count] FEAHIP_LOAD_*                     */
  double *surface_values;       /* [count][3]: pressure in [0], or t0        */
  /* material table (feahip_set_materials), optional: (materials (material
   * :lambda l :mu m) ...) inside (model ...) and (element-materials i0 i1 ...)
   * inside (geometry ...), one id per element in deck order.  Both or neither;
   * materials_count = 0: the single pair `parameters`                         */
  int materials_count;
  double *material_params;      /* [materials_count][2] = lambda, mu         */
  int *element_material;        /* [elements_count], values in [0, count)    */
  /* implicit dynamics, optional: (dynamics :steps N :dt x :beta b :gamma g
   * :dlambda l :density rho) inside (solution ...) -- :beta 0.25, :gamma 0.5 and
   * :dlambda 0 where absent -- installs a uniform consistent mass
   * (feahip_set_mass); :steps > 0 runs feahip_solve_dynamic instead of the load
   * increments.  (body-force :x :y :z) inside (boundary-conditions ...) needs
   * the density (feahip_set_body_force).  Written by fea_deck_save only when
   * present                                                                   */
  int has_dynamics;
  int dynamics_steps;
  double dynamics_dt, dynamics_beta, dynamics_gamma, dynamics_dlambda, density;
  int has_body_force;
  double body_force[3];
  /* explicit dynamics: (dynamics ... :scheme explicit :safety s :restep n) runs feahip_solve_explicit on the lumped mass
   * instead of the Newmark steps.  :dt 0 (legal with this scheme only) asks for dt = :safety times the stable-step
   * estimate, made again every :restep steps (:safety 0.9 and :restep 0, once, where absent); :beta and :gamma are
   * ignored.  :safety and :restep without :scheme explicit, a :scheme other than newmark / explicit and :dt 0 with
   * Newmark are load errors.  The three attributes are written only for the explicit scheme                    */
  int dynamics_explicit;
  double dynamics_safety;
  int dynamics_restep;
  /* results, optional: (results :nodal-stress t :energy t :reactions t) inside (solution ...), each attribute t or nil
   * (absent: nil).  :nodal-stress keeps the nodal stress with every snapshot and adds two $NodeData sections per step
   * to the .msh file; :energy and :reactions add one log line each per finished step.  Written by fea_deck_save only
   * when one of them is set; without the section the file and the log are what they were                        */
  int results_nodal_stress, results_energy, results_reactions;
  /* frequency response, optional: (harmonic :from f0 :to f1 :count n :zeta z :static-correction t) inside (solution ...):
   * n <= FEA_RESPONSE_MAX_FREQ linearly spaced frequencies in Hz, 0 <= f0 <= f1, a modal damping ratio z >= 0 for every
   * mode (:zeta 0 and :static-correction t where absent).  It uses the locked store, so it needs (modal ...) with :count or
   * :shift, and the static correction excludes a non-zero :shift: load errors otherwise.  After the modal run
   * feasolver_hip calls feahip_response_load with the surface load of the state reached and feahip_response_sweep with
   * :damping-alpha and :damping-beta of (dynamics ...) (fea_harmonic_run), logs two lines and appends two $NodeData
   * sections to the .msh file.  Written by fea_deck_save only when n > 0: a deck without the section is read, run and
   * written as before.  The five fields are the newest of the struct and stand in front of damping_alpha, whose place
   * (with everything behind it) the host tests pin                                                                 */
  /* transient response, optional: (transient :steps n :dt x :shape step|ramp|half-sine :rise T :zeta z :static-correction t
   * :base (bx by bz)) inside (solution ...): n <= FEA_TRANSIENT_MAX_STEPS steps of x > 0 under the load times g(t), g = 1
   * from t = 0 (step), min(t / T, 1) (ramp) or sin(pi t / T) up to T and 0 after (half-sine); :shape step, :zeta 0 and
   * :static-correction t where absent, :rise T > 0 needed by ramp and half-sine.  Without :base the load is the surface load
   * of the state reached, as for (harmonic ...); with it the base load of feahip_response_base_load along (bx by bz), which
   * needs no surface load.  It uses the locked store like (harmonic ...), with the same load errors.  After the harmonic
   * sweep feasolver_hip runs fea_transient_run.  Written by fea_deck_save only when n > 0: a deck without the section is
   * read, run and written as before.  The fields are the newest of the struct and stand in front of harmonic_count,
   * whose place (with everything behind it) the host tests pin                                                     */
  /* :sn-exponent b :sn-coefficient A :rainflow-depth d inside (transient ... :stress t), flat keys: the rainflow count of the six
   * stress components of every node over the history and Miner's sum on the S-N curve N s^b = A (s the stress amplitude),
   * 1 <= b <= 64, A > 0, on a stack of d points, 4 <= d <= FEA_RAINFLOW_MAX_DEPTH (32 where absent).  The exponent turns the
   * analysis on and needs the coefficient and :stress t; the other two are refused without it.  After the von Mises peaks
   * fea_transient_run calls feahip_response_stress_rainflow, logs the largest damage with its node, its component and its
   * cycles (and how many rows overflowed the stack, if any did) and appends "Fatigue damage (rainflow)", the largest of the
   * six components per node.  transient_sn_exponent = 0: off.  Written by fea_deck_save only when set: a deck without the
   * keys is read, run and written as before.  The three fields are the newest of the struct and stand in front of the
   * three of the next comment                                                                                          */
  double transient_sn_exponent, transient_sn_coefficient;
  int transient_rainflow_depth;
  /* :sn-exponent b :sn-coefficient A :duration T inside (random ...), flat keys as :stress t is: random-vibration fatigue of the
   * equivalent von Mises process on the S-N curve N s^b = A (s the stress amplitude), 1 <= b <= 64, A > 0, over the
   * duration T > 0 (1 where absent).  The exponent turns the analysis on and needs the coefficient; the other two are refused
   * without it.  After the RMS results fea_random_run calls feahip_response_stress_basis and
   * feahip_response_stress_fatigue on the same modes, load and grid, logs the largest Dirlik damage T D_DK with its node,
   * its nu0 and the life 1 / D_DK, and appends two $NodeData sections, "Fatigue damage (Dirlik)" (T D_DK) and
   * "Zero-upcrossing rate".  random_sn_exponent = 0: off.  Written by fea_deck_save only when set: a deck without the keys is
   * read, run and written as before.  The three fields are the newest of the struct and stand in front of the two of the
   * next comment                                                                                                       */
  double random_sn_exponent, random_sn_coefficient, random_duration;
  /* :stress t inside (harmonic ...) and (transient ...): after the displacement peaks, the largest von Mises stress of every
   * node over the sweep (over the cycle and the frequencies) or over the history, on the same modes and load
   * (feahip_response_stress_basis, then feahip_response_stress_sweep or _transient), one more log line and one more
   * $NodeData section each.  :stress nil where absent.  Written by fea_deck_save only when set: a deck without the key is
   * read, run and written as before.  The two fields are the newest of the struct and stand in front of the two of the next
   * comment, whose place (with everything behind it) the host tests pin                                                */
  int harmonic_stress, transient_stress;
  /* :stress t inside (spectrum ...) and (random ...): after the displacement result, the peak (the RMS) of the von Mises
   * stress on the same modes and load (feahip_response_stress_basis, then feahip_response_stress_spectrum or _random), one
   * more log line and one more $NodeData section each.  :stress nil where absent; with :rule abs it is refused (the von
   * Mises form needs the signs); any section but these two, (harmonic ...) and (transient ...) refuses the key.  Written by fea_deck_save only when set.  The two
   * fields are the newest of the struct and stand in front of the fields of the two sections, which the next comment
   * describes                                                                                                        */
  int spectrum_stress, random_stress;
  /* response spectrum and random vibration, optional, inside (solution ...) beside a (modal ...) with :count or :shift:
   *   (spectrum :base (bx by bz) :rule srss|cqc|abs :zeta z :static-correction t :zpa a :interp linear|loglog
   *             (points (f1 sa1) (f2 sa2) ...))
   *   (random   :base (bx by bz) :zeta z :static-correction t :interp linear|loglog :per-mode n :background n
   *             (psd (f1 s1) (f2 s2) ...))
   * f in Hz, strictly ascending and not negative, as in (harmonic ...); sa a spectral acceleration, s a one-sided PSD of the
   * load factor per Hz, both not negative; up to FEA_DECK_MAX_POINTS points.  :rule srss, :zeta 0, :static-correction t,
   * :zpa 0, :interp linear, :per-mode 32 and :background 257 where absent.  Without :base the load is the surface load of
   * the state reached; both have the load errors of (transient ...), and :zpa > 0 needs :static-correction t and a rule
   * other than abs.  After the transient run feasolver_hip runs fea_spectrum_run and fea_random_run.  Written by
   * fea_deck_save only when present: a deck without the sections is read, run and written as before.  The fields stand
   * in front of transient_steps, whose place (with everything behind it) the host tests pin                         */
  int has_spectrum, spectrum_count;
  double *spectrum_points;                    /* [spectrum_count][2] = f in Hz, sa */
  int spectrum_rule;                          /* FEAHIP_SRSS, FEAHIP_CQC, FEAHIP_ABS */
  int spectrum_static, spectrum_loglog, spectrum_has_base;
  double spectrum_zeta, spectrum_zpa, spectrum_base[3];
  int has_random, random_count;
  double *random_points;                      /* [random_count][2] = f in Hz, S per Hz */
  int random_static, random_loglog, random_per_mode, random_background, random_has_base;
  double random_zeta, random_base[3];
  int transient_steps;
  double transient_dt, transient_zeta;
  int transient_static, transient_shape;      /* FEA_SHAPE_* */
  double transient_rise;
  int transient_has_base;
  double transient_base[3];
  int harmonic_count;
  double harmonic_from, harmonic_to, harmonic_zeta;
  int harmonic_static;
  /* Rayleigh damping, optional: :damping-alpha a :damping-beta b inside (dynamics ...), both >= 0 and 0 where absent:
   * C = a M + b K_d, K_d the tangent at the reference configuration (fea_deck_create_solver calls feahip_set_damping
   * after the mass).  :scheme explicit with a non-zero :damping-beta is a load error (the explicit loop takes the
   * mass-proportional part only).  Written by fea_deck_save only when non-zero, with 17 digits: a deck without the keys
   * is read, run and written as before.  The two fields are the newest of the struct and stand in front of the contact
   * fields, whose place (with the buckling and modal ones behind them) the host tests pin                        */
  double damping_alpha, damping_beta;
  /* contact with rigid obstacles, optional: (contact :penalty e :augment k :gap-tolerance g (faces (n ...) ...)
   * (plane :point (x y z) :normal (x y z) :travel (x y z)) (sphere :center (..) :radius r :travel (..) :inside t)
   * (cylinder :point (..) :axis (..) :radius r :travel (..) :inside t) ...) inside (boundary-conditions ...), beside
   * (surface-loads ...): the faces and obstacles of feahip_set_contact, up to FEAHIP_MAX_OBSTACLES of them in deck order
   * (:augment 0, :gap-tolerance 0, :travel (0 0 0) and :inside nil where absent).  With :augment k > 0 fea_solve_steps
   * follows every converged increment by up to k multiplier updates (feahip_contact_augment), each with its own Newton
   * iterations; every finished step logs "Contact: active n, force F, max penetration p" and the .msh file gets one
   * $NodeData "Contact pressure" section per step.  Written by fea_deck_save only when there are faces and obstacles: a
   * deck without the section is read, run and written as before                                                  */
  int contact_faces_count;
  int contact_nodes_per_face;
  int *contact_nodes;           /* [count][nodes_per_face]                   */
  int contact_obstacles_count;
  int *contact_kind;            /* [count] FEAHIP_OBSTACLE_*                 */
  double *contact_geom;         /* [count][10]: point, direction, radius, travel */
  double contact_penalty;
  int contact_augment;
  double contact_gap_tolerance;
  /* linear buckling, optional: (buckling :modes N :tolerance t :max M) inside (solution ...), N in [1, 8] (:tolerance
   * 1e-8 and :max 2000 where absent).  After its last step -- and after the modal run of a deck that has both --
   * feasolver_hip calls feahip_solve_buckling at the state reached, logs one line per mode and appends one $NodeData
   * section per mode shape to the .msh file (fea_buckling_run).  It needs no density.  Written by fea_deck_save only
   * when N > 0: a deck without the section is read, run and written as before.  The three fields are the newest of the
   * struct and stand in front of the five modal ones, whose place at its end is pinned by the modal tests       */
  int buckling_modes;
  double buckling_tolerance;
  int buckling_max;
  /* modal analysis, optional: (modal :modes N :tolerance t :max M) inside (solution ...), N in [1, 8] (:tolerance 1e-8
   * and :max 1000 where absent).  After its last step feasolver_hip calls feahip_solve_modes at the state reached, logs
   * one line per mode and appends one $NodeData section per mode shape to the .msh file (fea_modal_run).  It needs the
   * density of (dynamics ... :density rho) -- :steps 0 there leaves the run static --: a deck without one is refused at
   * load.  Written by fea_deck_save only when N > 0.
   * :count N, N in [1, 64], instead of :modes (both together are refused), and :shift s, s >= 0 (written only when not
   * zero): with either key fea_modal_run calls feahip_solve_modes_locked(N, s) -- more than eight modes, and with s of
   * the order of the first elastic eigenvalue a body with rigid-body modes.  A deck without them is read, run and
   * written as before                                                                                           */
  int modal_count;
  double modal_shift;
  int modal_modes;
  double modal_tolerance;
  int modal_max;
} fea_deck;

/* sexp_data_load (sexp_loader.c:275-327).  Returns 0, or -1 with a message
 * in errbuf.  Defaults as fea_task_alloc / fea_solution_params_alloc
 * (fea_solver.c:1509-1549) and process_slae_solver (sexp_loader.c:100-103). */
int fea_deck_load(const char *path, fea_deck *deck, char *errbuf, int errlen);
void fea_deck_free(fea_deck *deck);
/* writes the same grammar (the emitter of utilities/tetgenProcessor)        */
int fea_deck_save(const char *path, const fea_deck *deck);

/* element plug-in: what solver_create_element_params_<type> +
 * solver_gauss_node_alloc produce.  weights[G], forms[G][npe],
 * dforms[G][3][npe].  Returns npe, or -1 for an unsupported pair.           */
int fea_element_tables(int ele_type, int gauss_count, double *weights,
                       double *forms, double *dforms);

/* the mass rule of an element type (exact for straight-sided elements): 4 points for TET4, 27 for TET10, 8 for
 * HEXAHEDRA8; 0 for an unknown type                                          */
int fea_mass_points(int ele_type);
/* creates the device context for a deck, its surface loads, its material table, its mass and its body force installed */
int fea_deck_create_solver(const fea_deck *deck, int device, feahip_ctx **ctx,
                           char *errbuf, int errlen);

/* solve() of the reference, calling the C ABI for every step.  Prints the
 * three quantitative log lines of the reference (fea_solver.c:212-213,224)
 * to `log` when it is not NULL.  x_steps (may be NULL) receives the node
 * coordinates after every completed load step, [steps][N][3].
 * Returns the number of completed load steps, or a negative FEAHIP_E* code. */
/* The load-increment / Newton loop itself (solve(), fea_solver.c:163-236): after every converged increment
 * `after_step(deck, ctx, step, user)` runs where the reference takes its load_step snapshot (:233-235); a
 * non-zero return aborts the loop with that code.  Returns the increments finished, or a negative FEAHIP_* code. */
typedef int (*fea_step_fn)(const fea_deck *deck, feahip_ctx *ctx, int step, void *user);
int fea_solve_steps(const fea_deck *deck, feahip_ctx *ctx, void *log /* FILE* */, fea_step_fn after_step, void *user);
int fea_solve(const fea_deck *deck, feahip_ctx *ctx, void *log /* FILE* */,
              double *x_steps, int x_steps_cap);

/* The log lines of (results :energy t) and (results :reactions t) for the state in force: "Strain energy W" (with
 * explicit_run: "Strain energy W, kinetic energy T, total W + T") and "Reactions sum rx ry rz".  Nothing is written,
 * and nothing computed, without the attributes or with a NULL log.                                              */
int fea_log_results(const fea_deck *deck, feahip_ctx *ctx, void *log /* FILE* */, int explicit_run);

/* Per-load-step snapshot (load_step of the reference, fea_solver.h:212-224):
 * node coordinates and the stress of Gauss point 0 of every element.         */
typedef struct fea_step_snapshot {
  double *nodes;      /* [nodes_count][3] */
  double *stress0;    /* [elements_count][9], stresses[e][0] */
  /* (results :nodal-stress t) only, NULL otherwise: feahip_get_nodal_stresses of all elements */
  double *nodal_stress;   /* [nodes_count][6] xx yy zz xy yz xz */
  double *von_mises;      /* [nodes_count] */
  /* a deck with (contact ...) only, NULL otherwise: the summed contact pressure of feahip_get_contact_status */
  double *contact_pressure;   /* [nodes_count] */
} fea_step_snapshot;

/* fea_solve with snapshots for the exporter: steps[cap] are allocated by the
 * callee (free with fea_snapshots_free).  Returns completed steps or <0.     */
int fea_solve_with_snapshots(const fea_deck *deck, feahip_ctx *ctx, void *log,
                             fea_step_snapshot *steps, int cap);
void fea_snapshots_free(fea_step_snapshot *steps, int n);
/* The path-following run of a deck with (arc-length :max N), N > 0, and surface
 * loads: feahip_solve_arclength with max_steps = N and lambda_max =
 * load-increments; one log line per converged step ("Arc-length step k
 * finished: load factor l, n iterations"); *last receives the final state.
 * Returns the completed steps or a negative FEAHIP_E* code.                  */
int fea_solve_arclength_with_snapshot(const fea_deck *deck, feahip_ctx *ctx, void *log,
                                      fea_step_snapshot *last);

/* The run of a deck with (dynamics :steps N ...), N > 0: feahip_solve_dynamic; one log line per completed step
 * ("Dynamic step k finished: time t, n iterations"; the explicit scheme: feahip_solve_explicit and
 * "Explicit step k finished: time t, dt h"); *last receives the final state.  Returns the completed steps
 * or a negative FEAHIP_E* code.
 * With (results :energy t) or (results :reactions t) the steps are made one call each (one call for all of them where
 * the explicit scheme estimates its own step, :dt 0: the lines then follow the last step only) and every step is
 * followed by "Strain energy W" -- on the explicit scheme "Strain energy W, kinetic energy T, total W + T" -- and
 * "Reactions sum rx ry rz", the sum of feahip_get_reactions per axis.  The static and the arc-length runs write the
 * same lines after every finished increment / at the end of the path.                                          */
int fea_solve_dynamic_with_snapshot(const fea_deck *deck, feahip_ctx *ctx, void *log, fea_step_snapshot *last);

/* solver_export_tetrahedra10_gmsh (fea_solver.c:1375-1488): Gmsh 2.0 ASCII,
 * nodes with %f, TET10 elements with local nodes 8 and 9 swapped, and per
 * load step (step 0 = zeros) NodeData "Displacements" and ElementData
 * "Stress tensor" (Gauss point 0) tagged load*0.83333333.  4-node elements
 * are written as Gmsh type 4.  A deck with a material table writes the
 * element's material as its first tag, the physical entity, numbered from 1
 * as everything in the file (material id + 1); other decks write 1.  Steps
 * whose snapshot holds a nodal stress are followed by NodeData "Nodal stress"
 * (9 components, the symmetric tensor in full) and NodeData "Von Mises".     */
int fea_export_gmsh(const char *filename, const fea_deck *deck,
                    const fea_step_snapshot *steps, int nsteps);

/* The modal analysis of a deck with (modal :modes N ...), N > 0, at the state the context is in: feahip_solve_modes
 * (feahip_solve_modes_locked and the locked store for a deck with :count or :shift),
 * one log line per mode ("Mode k: omega^2 = l, f = x Hz", f = sqrt(max(l, 0)) / 2 pi) and, with msh_path not NULL, one
 * $NodeData section "Mode k" per mode shape appended to that file, tagged with the frequency.  A solve that runs out
 * of steps is logged and its modes are written as they stand.  Returns 0, or a negative FEAHIP_E* code.        */
int fea_modal_run(const fea_deck *deck, feahip_ctx *ctx, void *log /* FILE* */, const char *msh_path);

/* The frequency sweep of a deck with (harmonic :count n ...), n > 0, right after fea_modal_run, on the locked modes that
 * run left: the load is feahip_get_surface_forces at the state reached (FEAHIP_EINVAL when it is all zero),
 * feahip_response_load with the deck's solver settings, then feahip_response_sweep over the n frequencies with the
 * deck's :damping-alpha, :damping-beta and :zeta.  Log: "Harmonic: n frequencies f0 .. f1 Hz, m modes, static correction
 * on|off" and "Harmonic peak: |u| = p at f = x Hz, node a dof j" (the largest peak of all dofs, the lowest dof among
 * equals, node from 1, dof 0-2).  With msh_path not NULL two $NodeData sections of three components per node are
 * appended: "Harmonic peak amplitude" and "Harmonic peak frequency" (Hz).  With :stress t then feahip_response_stress_basis
 * and feahip_response_stress_sweep over the same frequencies: "Harmonic peak von Mises: vm = p, node a, f = x Hz" (the
 * largest of all nodes, the lowest node among equals) and a one-component section "Harmonic peak von Mises stress";
 * fea_transient_run likewise: "Transient peak von Mises: vm = p, node a, t = x" and "Transient peak von Mises stress"
 * (feahip_response_stress_transient).  Returns 0, or a negative FEAHIP_E* code.  */
int fea_harmonic_run(const fea_deck *deck, feahip_ctx *ctx, void *log /* FILE* */, const char *msh_path);
/* The time history of a deck with (transient :steps n ...), n > 0, after fea_harmonic_run and before anything drops the
 * locked modes: feahip_response_load with the surface load of the state reached (all zero: a log line and FEAHIP_EINVAL)
 * or, with :base, feahip_response_base_load, then feahip_response_transient of the displacement with the deck's
 * :damping-alpha, :damping-beta and :zeta.  Log: "Transient: n steps of dt, shape s, m modes, static correction on|off",
 * with :base one "Effective mass: mode k, gamma g, m_eff e, cumulative fraction c of total t" line per mode, and
 * "Transient peak: |u| = p at t = x, node a dof j" (the largest peak of all dofs, the lowest dof among equals).  With
 * msh_path two $NodeData sections are appended: "Transient peak displacement" and "Transient peak time".  Returns 0, or a
 * negative FEAHIP_E* code.  */
int fea_transient_run(const fea_deck *deck, feahip_ctx *ctx, void *log /* FILE* */, const char *msh_path);
/* The design peak of a deck with (spectrum ...), after fea_transient_run and before anything drops the locked modes: the
 * load as in fea_transient_run (the surface load of the state reached, or with :base the base load), then
 * feahip_response_spectrum of the displacement with the deck's points (Hz to rad/s), :rule, :zpa, :damping-alpha,
 * :damping-beta and :zeta.  Log: "Spectrum peak: |u| = p, node a dof j, rule r, m modes" (the largest of all dofs, the
 * lowest dof among equals, node from 1, dof 0-2).  With :stress t also "Spectrum peak von Mises: vm = p, node a, rule r, m
 * modes" and a one-component section "Spectrum peak von Mises stress" (fea_random_run: "Random RMS von Mises: vm = p, node
 * a, g grid points, m modes" and "RMS von Mises stress").  With msh_path one $NodeData section "Spectrum peak displacement" is
 * appended.  Returns 0, or a negative FEAHIP_E* code.  */
int fea_spectrum_run(const fea_deck *deck, feahip_ctx *ctx, void *log /* FILE* */, const char *msh_path);
/* The RMS displacement of a deck with (random ...), after fea_spectrum_run: the load likewise, the PSD table from per Hz
 * over Hz to per rad/s over rad/s, the grid of feahip_host_random_grid over the table's band with the table's abscissae
 * as breakpoints, the PSD read there by feahip_host_psd_value, then feahip_response_random.  Log: "Random RMS: |u| = p,
 * node a dof j, n grid points, m modes".  With msh_path one $NodeData section "RMS displacement" is appended.  Returns 0,
 * or a negative FEAHIP_E* code.  */
int fea_random_run(const fea_deck *deck, feahip_ctx *ctx, void *log /* FILE* */, const char *msh_path);

/* The buckling analysis of a deck with (buckling :modes N ...), N > 0, at the state the context is in:
 * feahip_solve_buckling, one log line per mode ("Buckling mode k: factor = f, nu = v") and, with msh_path not NULL, one
 * $NodeData section "Buckling mode k" per mode shape appended to that file, tagged with the factor.  A solve that runs
 * out of steps is logged and its modes are written as they stand.  Returns 0, or a negative FEAHIP_E* code.       */
int fea_buckling_run(const fea_deck *deck, feahip_ctx *ctx, void *log /* FILE* */, const char *msh_path);

/* "<base>.msh" next to the deck, as initial_data_load builds it
 * (fea_solver.c:1681-1687); out must hold strlen(deck_path)+5 bytes.        */
void fea_export_name(const char *deck_path, char *out);

#ifdef __cplusplus
}
#endif
#endif
