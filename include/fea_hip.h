/*
 * fea_hip.h -- C ABI of the MI355X-native assembly + Newton hot path.
 *
 * One opaque context replaces the `fea_solver` object of the reference for
 * the calls that `solve()` makes inside its load-increment / Newton loops
 * (solver-large/fea_solver.c:130-242).  Every entry below names the
 * reference function it stands in for.  Plain pointers and sizes only; all
 * host arrays are copied (caller keeps ownership); getters fill caller-owned
 * host buffers in the reference's own shapes.
 *
 * Every function returns 0 on success or a negative FEAHIP_E* code, never
 * exits and never asserts (the reference's error() calls exit(),
 * fea_solver.c:57-61).  feahip_last_error() gives the message.
 * A context is single-caller (the reference is single-threaded).
 */
#ifndef FEA_HIP_H
#define FEA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct feahip_ctx feahip_ctx;

enum {
  FEAHIP_OK = 0,
  FEAHIP_EINVAL = -1,      /* bad argument / unsupported combination        */
  FEAHIP_ENODEVICE = -2,   /* no usable HIP device: the path has no CPU mode */
  FEAHIP_EHIP = -3,        /* a HIP runtime call failed                      */
  FEAHIP_ENOMEM = -4,
  FEAHIP_ESTATE = -5,      /* call order violated (e.g. restore before stash)*/
  FEAHIP_ENOTCONVERGED = -6,
  FEAHIP_ECOMM = -7        /* RCCL failure                                   */
};

/* material models, numbered as `model_type` (fea_model.h:37-40) */
enum { FEAHIP_MODEL_A5 = 0, FEAHIP_MODEL_COMPRESSIBLE_NEOHOOKEAN = 1 };
/* linear solvers, numbered as `slae_solver_type` (fea_solver.h:62-66).
 * CG = conjugate gradients started from x0 = rhs (fea_solver.c:251-256);
 * PCG_ILU and CHOLESKY have no GPU-idiomatic twin: both run diagonally
 * (3x3 block) preconditioned CG, CHOLESKY iterated to stagnation.           */
enum { FEAHIP_CG = 0, FEAHIP_PCG_ILU = 1, FEAHIP_CHOLESKY = 2 };
/* assembly strategies */
enum {
  FEAHIP_ASM_AUTO = 0,
  FEAHIP_ASM_ROWOWNER = 1, /* node-centric gather, every CSR value written
                              once, deterministic                            */
  FEAHIP_ASM_ATOMIC = 2,   /* element-parallel, FP64 atomics into the CSR    */
  FEAHIP_ASM_PATCH = 3,    /* retired (refused): element states shared through
                              LDS per 16-row chunk; 1.8x slower than STAGED   */
  FEAHIP_ASM_STAGED = 4,   /* linear tets: row-owner visits with node
                              coordinates and connectivity staged in LDS     */
  FEAHIP_ASM_PAIRED = 5,   /* retired (refused): two face-sharing elements per
                              lane; 5 % slower than STAGED                    */
  FEAHIP_ASM_PIPELINED = 6,/* retired (refused): STAGED with the next chunk's
                              loads in flight; equal to STAGED within 2 %     */
  FEAHIP_ASM_SHARED = 7,   /* 10-node tets: Gauss-point states evaluated once
                              per chunk element and shared through LDS, the
                              blocks of a (row, element, column) pair summed
                              over the Gauss points in registers              */
  FEAHIP_ASM_GATHER = 8    /* linear tets: a 1024-thread workgroup owns a run
                              of block rows; every element touching them is
                              evaluated once into an LDS record, one thread
                              per off-diagonal block then sums that block's
                              element contributions in registers.  10-node
                              tets: the same with the Gauss points as an
                              outer loop over per-element state records a
                              first kernel wrote, up to five blocks per
                              thread.  No atomics anywhere, fixed summation
                              order: bitwise reproducible                     */
};

/* ---- lifetime ----------------------------------------------------------- */

/* Stands in for fea_solver_alloc (fea_solver.c:387-456) plus
 * solver_create_element_database (:556-571): the element plug-in arrives as
 * the tables solver_gauss_node_alloc tabulates (:503-535) -- weights[G]
 * (divisor 6 already inside) and dforms[G][3][npe] -- because device code
 * cannot call the host's isoform_t/disoform_t pointers (fea_solver.h:34-40).
 * The material plug-in arrives as (model, parameters[]) of `fea_model`
 * (fea_model.h:46-57): parameters[0] = lambda, parameters[1] = mu.
 * elements: [n_elems][npe] 0-based node ids (elements_array, :132-138)
 * nodes0:   [n_nodes][3]   initial coordinates (nodes_array, :124-128)
 * presc_*:  prescribed_bnd_node fields (:142-146), deck order.              */
int feahip_create(feahip_ctx **out, int device,
                  int n_nodes, int n_elems, int npe, int gauss_count,
                  const double *gauss_weights, const double *dforms,
                  const int *elements, const double *nodes0,
                  int model, const double *model_params, int params_count,
                  int n_presc, const int *presc_node, const int *presc_type,
                  const double *presc_values);

/* fea_solver_free (fea_solver.c:459-501); frees device memory only. */
void feahip_destroy(feahip_ctx *ctx);

const char *feahip_last_error(const feahip_ctx *ctx);
/* message of the last failed feahip_create (no context exists then) */
const char *feahip_create_error(void);

/* ---- the calls of solve() ---------------------------------------------- */

/* solver_update_nodes_with_bc (fea_solver.c:1281-1284): x[c] += lambda*value
 * for every prescribed dof.                                                 */
int feahip_update_nodes_with_bc(feahip_ctx *ctx, double lambda);

/* solver_create_current_shape_gradients + solver_create_stresses
 * (fea_solver.c:831-861).  The assembly kernels recompute J, grad N, F and
 * sigma in registers, so this only invalidates the cached per-Gauss-point
 * F / sigma that feahip_get_graddefs / feahip_get_stresses serve; it also
 * returns, in *n_bad (may be NULL), the count of Gauss points whose current
 * Jacobian determinant is <= 0 as seen by the last assembly.               */
int feahip_update_state(feahip_ctx *ctx, int *n_bad);

/* solver_create_stiffness (fea_solver.c:873-883): K = sum_e (Kc + Ksigma). */
int feahip_create_stiffness(feahip_ctx *ctx);
/* solver_create_residual_forces (fea_solver.c:863-870): f = -T.            */
int feahip_create_residual_forces(feahip_ctx *ctx);
/* both in one pass over the mesh (what a full-Newton iteration needs)      */
int feahip_create_stiffness_and_residual(feahip_ctx *ctx);

/* sp_matrix_copy(global -> stiffness) (fea_solver.c:179) and
 * sp_matrix_free + sp_matrix_copy(stiffness -> global) (:194-195).         */
int feahip_stash_stiffness(feahip_ctx *ctx);
int feahip_restore_stiffness(feahip_ctx *ctx);

/* solver_apply_prescribed_bc (fea_solver.c:1200-1257): for every prescribed
 * dof c with p = lambda*value: f[r] -= K[r,c]*p, row and column c zeroed
 * keeping K[c,c], f[c] = K[c,c]*p.                                          */
int feahip_apply_prescribed_bc(feahip_ctx *ctx, double lambda);

/* solver_solve_slae (fea_solver.c:300-321): solve K u = f.  iters / resid
 * (relative residual ||f-Ku||/||f||) may be NULL.                          */
int feahip_solve_slae(feahip_ctx *ctx, int solver_type, double tolerance,
                      int max_iterations, int *iters, double *resid);

/* K [u, u2] = [f, f2]: two CG / PCG recurrences run in lockstep over ONE read
 * of the matrix per iteration.  Column 0 is exactly the system
 * feahip_solve_slae solves (the context's f, start vector u0 = f); column 1 is
 * f2, [3N] in the caller's dof order, used as given (the caller zeroes the
 * prescribed dofs), start vector f2.  Each column has its own scalars and its
 * own stop test; a column that has converged is frozen -- none of its vectors
 * is written again -- and the solve ends when both have stopped or at
 * max_iterations.  iters[2] / resid[2] per column (either may be NULL).  The
 * loop is the two-reduction textbook loop; feahip_set_pcg_variant does not
 * apply to it.  Preconditioner kind 0 and 1 as feahip_solve_slae (kind 1: one
 * W-cycle per live column and iteration); CHOLESKY means "to stagnation".
 * Returns FEAHIP_ESTATE before the first stiffness assembly, FEAHIP_EINVAL
 * under preconditioner kind 2 and on a context that has a transport, a row
 * shard, or was created by feahip_create_rank* (feahip_last_error says which),
 * FEAHIP_ENOTCONVERGED on a breakdown in either column (feahip_last_error
 * names the column).  Column 0 is read with feahip_get_solution, column 1
 * with feahip_get_solution2.                                                 */
int feahip_solve_slae2(feahip_ctx *ctx, int solver_type, double tolerance,
                       int max_iterations, const double *f2, int iters[2], double resid[2]);
/* u2 of the last feahip_solve_slae2, [3N] in the caller's dof order.         */
int feahip_get_solution2(feahip_ctx *ctx, double *u2);

/* cdot(global_forces_vct, global_solution_vct) (fea_solver.c:208-210).     */
int feahip_energy(feahip_ctx *ctx, double *tolerance);

/* solver_update_nodes_with_solution (fea_solver.c:1270-1279): x += u.
 * u == NULL uses the device-resident solution of the last solve.           */
int feahip_update_nodes_with_solution(feahip_ctx *ctx, const double *u);

/* The whole loop of solve() (fea_solver.c:163-236) run by the library.
 * tol_log[tol_log_cap] receives <u,f> of every Newton iteration, its_log
 * [load_increments] the iteration count of every step (either may be NULL).
 * *steps_done = number of completed load steps.                             */
int feahip_solve(feahip_ctx *ctx, int load_increments, int max_newton,
                 int modified_newton, double desired_tolerance,
                 int solver_type, double solver_tolerance, int solver_max_iter,
                 double *tol_log, int tol_log_cap, int *its_log,
                 int *steps_done);

/* Crisfield's cylindrical arc length on the surface loads: follows the
 * equilibrium path T(x) = lambda F(x) through limit points, where the load
 * control of feahip_solve stops converging.  F is the surface-load vector at
 * load factor 1 (constant for dead tractions, evaluated at the current nodes
 * for follower pressure); prescribed dofs stay where they are.  Every step
 * starts from a converged (x_n, lambda_n) with radius dl:
 *   predictor  K v = F; first step dl = |v| (so dlambda = 1: load control's
 *              first increment), later dlambda = s dl / |v| with
 *              s = sign(Du_prev . v); Du = dlambda v;
 *   corrector  (at most max_newton) at x_n + Du, lambda_n + Dlambda: K, R =
 *              lambda F - T and F; K [du_R, du_F] = [R, F] with the two-column
 *              solve; dlam from a dlam^2 + b dlam + c = 0, a = du_F.du_F,
 *              b = 2 (Du + du_R).du_F, c = |Du + du_R|^2 - dl^2, the root with
 *              the larger Du . (Du + du_R + dlam du_F); du = du_R + dlam du_F,
 *              Du += du, Dlambda += dlam; converged when |<du, R>| <=
 *              desired_tolerance (the energy test of fea_solver.c:208-221).
 * A negative discriminant, max_newton iterations without convergence or an
 * assembly with bad Jacobians restore (x_n, lambda_n), halve dl and retry, at
 * most 8 times per step; then FEAHIP_ENOTCONVERGED with *steps_done completed
 * steps.  dl is never grown.  Stops when lambda >= lambda_max or after
 * max_steps steps.  lambda_log[max_steps] receives the converged factor of
 * every step, its_log[max_steps] its corrector iterations, tol_log[log_cap]
 * <du, R> of every corrector iteration (any may be NULL).  The context's load
 * factor and nodes are left at the last converged point.  FEAHIP_ESTATE
 * without loaded faces; refused like feahip_solve_slae2 on sharded contexts.  */
int feahip_solve_arclength(feahip_ctx *ctx, double lambda_max, int max_steps, int max_newton,
                           double desired_tolerance, int solver_type, double solver_tolerance,
                           int solver_max_iter, double *lambda_log, double *tol_log, int log_cap,
                           int *its_log, int *steps_done);

/* ---- surface loads ------------------------------------------------------ */
/* What the reference leaves unwritten (solver_create_forces_bc, fea_solver.c:
 * 1191-1198).  A loaded face is a boundary face of exactly one element: a
 * 3-node triangle of a TET4, a 6-node triangle of a TET10 (corners, then
 * mid-side nodes), a 4-node quad of a HEX8.  Its node ids come in any order;
 * the library matches the set against the faces of the owning element and
 * takes node order and OUTWARD normal from it.  Two kinds:
 *   FEAHIP_LOAD_PRESSURE  follower pressure p on the CURRENT face,
 *                         t da = -p n da (p > 0 pushes into the body)
 *   FEAHIP_LOAD_TRACTION  dead traction t0 per REFERENCE area, t da = t0 dA
 * F_a = int N_a t da, integrated exactly for the pressure (tri3: 1 point,
 * tri6: 6-point degree-4 rule, quad4: 2 x 2 Gauss); the dead traction uses
 * the same points.  Every assembly that writes the residual then produces
 * f = lambda F_ext(x) - T(x) (feahip_apply_prescribed_bc still overwrites the
 * prescribed dofs); stiffness-only assembly is unchanged.  NO load stiffness
 * is assembled: the follower-pressure tangent is non-symmetric and the CG /
 * PCG solvers need a symmetric K, so Newton converges to the exact answer of
 * the exact residual, possibly in more iterations.  lambda is the context's
 * load factor: 0 at creation, feahip_update_nodes_with_bc(ctx, l) adds l to it
 * (deck values are per increment, as prescribed displacements), so after load
 * step s of feahip_solve the load applied is (s+1) x the values given.  With
 * no loaded faces nothing is launched and nothing changes.  Row shards and
 * in-process groups add the loads of the rows they own; a feahip_create_rank
 * context takes the whole face list and keeps the faces touching its owned
 * nodes; a feahip_create_rank_local context takes faces in LOCAL node ids.  */
enum { FEAHIP_LOAD_PRESSURE = 0, FEAHIP_LOAD_TRACTION = 1 };
/* replaces the set; n_faces = 0 clears it.  face_nodes[n_faces][nodes_per_face]
 * in the CALLER's node ids, kind[n_faces], values[n_faces][3] (pressure in [0];
 * the traction vector t0 otherwise).  A node set that is not exactly one
 * element's boundary face (interior face, unknown face, wrong node count) is
 * refused with FEAHIP_EINVAL, feahip_last_error naming the face.            */
int feahip_set_surface_loads(feahip_ctx *ctx, int n_faces, int nodes_per_face, const int *face_nodes,
                             const int *kind, const double *values);
/* lambda * F_ext at the current nodes, [3N] in the caller's dof order (test /
 * post-processing hook; authoritative on the owned rows of a shard)         */
int feahip_get_surface_forces(feahip_ctx *ctx, double *f);
int feahip_set_load_factor(feahip_ctx *ctx, double lambda);
int feahip_get_load_factor(feahip_ctx *ctx, double *lambda);

/* ---- frictionless contact with rigid obstacles -------------------------- */
/* Node-to-rigid-surface contact by a penalty with augmented-Lagrangian
 * (Uzawa) updates.  The contact NODES are the nodes of the contact faces,
 * which are given and resolved exactly as the faces of
 * feahip_set_surface_loads (same refusals, same rule for rank contexts).
 * Each contact node a carries a reference-area weight w_a, computed once on
 * the host from X0: tri3 A/3; quad4 the row sums of int N_a dA by the 2 x 2
 * rule; tri6 HRZ lumping -- the diagonal of int N_a N_b dA by the 6-point rule,
 * scaled so the six weights sum to the area (the corner functions of a tri6
 * integrate to zero, so a consistent weight would switch the corners off).
 * Up to FEAHIP_MAX_OBSTACLES obstacles; obstacle o sits at
 * c = c0 + load_factor * travel, so it moves with the load increments as the
 * prescribed displacements and the surface loads do.  With x the node:
 *   FEAHIP_OBSTACLE_PLANE            g = (x - c).a              n = a
 *   FEAHIP_OBSTACLE_SPHERE           g = |x - c| - r            n = (x - c)/|x - c|
 *   FEAHIP_OBSTACLE_SPHERE_INSIDE    g = r - |x - c|            n = -(x - c)/|x - c|
 *   FEAHIP_OBSTACLE_CYLINDER         as the sphere with q = (I - a a')(x - c) for x - c
 *   FEAHIP_OBSTACLE_CYLINDER_INSIDE  as the sphere from inside, with q
 * a is the plane's normal or the cylinder's axis (normalised by the library).
 * A node ON the sphere's centre or the cylinder's axis (rho = |x - c| or |q|
 * = 0) has no normal and is SKIPPED for that obstacle, in every kernel.
 * With the multiplier mu_ao >= 0 (0 at feahip_set_contact), the penetration
 * p = -g and the penalty eps (a pressure per length):
 *   pressure  t = max(0, mu_ao + eps p)       force  F_a += w_a t n
 *   K_aa += w_a [ eps n n' - s t (P - n n') / rho ]   (s = +1 solid, -1 inside, 0 plane;
 *                                                       P = I, or I - a a' for cylinders)
 *   potential Pi_c = sum w_a t^2 / (2 eps)    augmentation  mu_ao <- max(0, mu_ao + eps p)
 * Every assembly that writes the residual produces f = lambda F_ext - T + F_c,
 * every assembly that writes K adds K_c to the node's own diagonal block: no
 * pattern change.  feahip_get_reactions therefore sees F_c as well.  A context
 * without contact launches nothing and keeps the bits it had before.
 * feahip_solve (and the group solve) with augment_max > 0: after the Newton
 * loop of a load increment has converged, up to augment_max times -- read the
 * maximum penetration over the active pairs; stop if it is <= gap_tolerance;
 * update the multipliers; iterate again at the same load.  its_log[step] counts
 * the iterations of all passes.  Modified Newton stashes the K of the pass's
 * first assembly, contact stiffness included; with contact, full Newton is the
 * sensible choice (the active set changes inside a step).  The Newmark and the
 * explicit loops use the multipliers as they stand and never update them;
 * feahip_stable_step adds w_a eps n n' of EVERY contact pair, in contact or not,
 * to the K of the plain assembly (in place of the active pairs' own term)
 * before the Gershgorin bound, so a node entering contact between two
 * estimates cannot push the step over the bound.  feahip_solve_arclength
 * refuses a context with contact (FEAHIP_ESTATE).  Modes and buckling see the K
 * of the assembly entry, contact stiffness of the active pairs included (the
 * bilateral linearisation); nothing more is promised there.                 */
enum { FEAHIP_OBSTACLE_PLANE = 0, FEAHIP_OBSTACLE_SPHERE = 1, FEAHIP_OBSTACLE_SPHERE_INSIDE = 2,
       FEAHIP_OBSTACLE_CYLINDER = 3, FEAHIP_OBSTACLE_CYLINDER_INSIDE = 4 };
#define FEAHIP_MAX_OBSTACLES 8
/* replaces the contact; n_faces = 0 or n_obstacles = 0 clears it (multipliers
 * included) -- but a feahip_create_rank_local context given obstacles and no
 * face (its slab holds none of them) keeps the obstacles and the parameters,
 * so that its rank enters the collectives of the augmentation with the
 * others.  kind[n_obstacles]; geom[n_obstacles][10] = point (3), direction
 * (3), radius, travel (3).  FEAHIP_EINVAL with the offending index in
 * feahip_last_error: a bad face, an unknown kind, penalty <= 0, a zero
 * direction (plane, cylinders), radius <= 0 on a round kind, more than
 * FEAHIP_MAX_OBSTACLES obstacles, negative augment_max or gap_tolerance.    */
int feahip_set_contact(feahip_ctx *ctx, int n_faces, int nodes_per_face, const int *face_nodes,
                       int n_obstacles, const int *kind, const double *geom, double penalty,
                       int augment_max, double gap_tolerance);
/* the contact nodes this context owns, ascending, in the ids of its node
 * arrays, and their weights (either may be null: *n alone sizes the arrays)  */
int feahip_get_contact_nodes(feahip_ctx *ctx, int *n, int *nodes, double *weights);
/* the obstacles of the contact in force (0 without one)                     */
int feahip_get_contact_obstacles(feahip_ctx *ctx, int *n_obstacles);
/* mu[n][n_obstacles] in the node order of feahip_get_contact_nodes          */
int feahip_get_contact_multipliers(feahip_ctx *ctx, double *mu);
int feahip_set_contact_multipliers(feahip_ctx *ctx, const double *mu);
/* F_c at the current nodes, [3N], shaped like feahip_get_surface_forces     */
int feahip_get_contact_forces(feahip_ctx *ctx, double *f);
/* per node: the smallest gap over the obstacles (+inf away from the owned
 * contact nodes) and the summed pressure t (0 there); either may be null     */
int feahip_get_contact_status(feahip_ctx *ctx, double *gap, double *pressure);
/* collective, as feahip_kinetic_energy (one call on any context of an
 * in-process group drives the group; every RCCL rank calls it): out[4] = active pairs (t > 0), the
 * largest penetration over them (0 without one), sum w t, Pi_c               */
int feahip_contact_info(feahip_ctx *ctx, double *out);
/* collective: reports the largest penetration over the active pairs (a null
 * max_penetration skips that reduction), then updates the multipliers        */
int feahip_contact_augment(feahip_ctx *ctx, double *max_penetration);

/* ---- heterogeneous bodies: a table of (lambda, mu) pairs and one material id
 * per element.  feahip_set_materials replaces the context's single pair by the
 * table; n_materials = 0 returns to the pair given at creation.  At most
 * FEAHIP_MAX_MATERIALS pairs.  The MODEL stays one per context (FEAHIP_MODEL_*
 * is a compile-time parameter of the kernels): the table varies its two
 * parameters, not the law.
 * params[n_materials][2] = lambda, mu; elem_material[E] has values in
 * [0, n_materials), in the CALLER's element order: the whole mesh's on a
 * feahip_create / feahip_create_rank context (a rank context keeps the entries
 * of its own elements), the LOCAL order on a feahip_create_rank_local context.
 * On row shards and in-process groups every context gets the same call.
 * FEAHIP_EINVAL (feahip_last_error names the offending index): null arrays with
 * n_materials > 0, n_materials > FEAHIP_MAX_MATERIALS, an id outside
 * [0, n_materials), a non-finite parameter; the context is left as it was.
 * May be called at any time: the cached F and sigma are dropped, K and f are
 * what the next assembly makes them, a stashed K is left alone, and gather maps
 * built before are built again with the ids.  Strategies: GATHER, ROWOWNER and
 * ATOMIC (and AUTO, which chooses among them) assemble with a table; STAGED
 * and SHARED are refused with FEAHIP_EINVAL at the assembly.                  */
#define FEAHIP_MAX_MATERIALS 256
int feahip_set_materials(feahip_ctx *ctx, int n_materials, const double *params, const int *elem_material);
/* the table in force: *n_materials (0: the single pair), and where non-null
 * params[n][2] and elem_material (a first call with nulls sizes them).
 * elem_material always has one entry per element of THIS context, in the
 * context's own element order.  On a feahip_create_rank context that is the
 * LOCAL order of the rank's elements (feahip_rank_maps: elem_global), NOT the
 * whole-mesh order feahip_set_materials takes there: what this call returns
 * cannot be passed back to feahip_set_materials on such a context without
 * scattering it through elem_global first.  On every other context get and
 * set use the same order.                                                     */
int feahip_get_materials(feahip_ctx *ctx, int *n_materials, double *params, int *elem_material);
/* ---- implicit dynamics: consistent mass, body force, Newmark steps ---------
 * Nothing below changes a bit of K, f, u or any launch on a context that never
 * had a mass set, or whose mass was cleared again.
 *
 * feahip_set_mass: M_ab = sum_e rho_e sum_g w_g det J0_g N_a(g) N_b(g), times
 * the 3x3 identity, kept as one double per block of K's pattern (owned rows).
 * The mass rule is the caller's and separate from the stiffness rule (a
 * 1-point TET4 rule gives a rank-1 element mass): weights[mass_points] with
 * the divisor inside as gauss_weights, forms[mass_points][npe] = N_a at the
 * points, dforms[mass_points][3][npe] for det J0 (reference configuration).
 * n_rho = 1: a uniform density; n_rho = the material count in force
 * (feahip_set_materials): one density per material id, the ids in the
 * context's own element order as feahip_set_materials documents; n_rho = 0
 * clears the mass and with it the body force, velocities and accelerations.
 * A later feahip_set_materials with another count drops a per-material mass:
 * the next call that needs the mass returns FEAHIP_ESTATE.  FEAHIP_EINVAL
 * (feahip_last_error names the index or element; the context is left as it
 * was): a density that is not finite and positive, n_rho neither 1 nor the
 * table size, null arrays, det J0 <= 0 at a mass point.  Assembled on the GPU,
 * once per call, no atomics, fixed summation order.  Row shards, in-process
 * groups and rank contexts each get the same call.  Velocities, accelerations
 * are zero afterwards.                                                        */
int feahip_set_mass(feahip_ctx *ctx, int n_rho, const double *rho, int mass_points, const double *weights,
                    const double *forms, const double *dforms);
/* y = M x, host vectors [3N] in the caller's dof order (test hook;
 * authoritative on the owned rows like feahip_spmv, zero on the others)       */
int feahip_mass_spmv(feahip_ctx *ctx, const double *x, double *y);
/* An acceleration b per unit mass as the dead load F_body = M (1 (x) b),
 * computed once on the owned rows.  It is scaled by the load factor like the
 * surface loads: every assembly that writes the residual gives
 * f = lambda (F_surf(x) + F_body) - T(x), so feahip_solve ramps gravity.  NULL
 * or zeros clear it; FEAHIP_ESTATE without a mass.  feahip_solve_arclength
 * with a body force set is refused with FEAHIP_EINVAL.                       */
int feahip_set_body_force(feahip_ctx *ctx, const double b[3]);
/* Velocity and acceleration of ALL nodes of the context (halo nodes
 * included), [N][3] in the caller's node ids; the time.  FEAHIP_ESTATE without
 * a mass (the time excepted).                                                */
int feahip_set_velocities(feahip_ctx *ctx, const double *v);
int feahip_get_velocities(feahip_ctx *ctx, double *v);
int feahip_set_accelerations(feahip_ctx *ctx, const double *a);
int feahip_get_accelerations(feahip_ctx *ctx, double *a);
int feahip_get_time(feahip_ctx *ctx, double *t);
int feahip_set_time(feahip_ctx *ctx, double t);
/* Solves M a = lambda F_ext(x) - T(x) with a = 0 on the prescribed dofs into
 * the accelerations, by the ordinary solve on K := M (K is marked changed
 * afterwards).  Collective: an in-process group is driven from any of its
 * contexts, the ranks of an RCCL run all make the call.                      */
int feahip_consistent_acceleration(feahip_ctx *ctx, int solver_type, double tolerance, int max_iterations);
/* n_steps Newmark steps (displacement form, full Newton; line search and
 * modified Newton do not apply).  Per step, a0 = 1 / (beta dt^2):
 *   xt = x + dt v + dt^2 (1/2 - beta) a,  vt = v + dt (1 - gamma) a;
 *   feahip_update_nodes_with_bc(ctx, dlambda) (dlambda = 0 holds loads and
 *   supports fixed);
 *   Newton from x_n until |<u,f>| <= desired_tolerance or max_newton
 *   iterations, on K + a0 M and f = lambda F_ext - T - a0 M (x - xt);
 *   a = a0 (x - xt), v = vt + gamma dt a, t += dt on all nodes (at prescribed
 *   nodes they describe the prescribed motion).
 * A step that uses up max_newton iterations stops the loop as in feahip_solve;
 * *steps_done counts the completed steps and the state is that of the last
 * completed one.  tol_log / its_log as feahip_solve.  FEAHIP_EINVAL for
 * dt <= 0, beta <= 0 or gamma < 0; FEAHIP_ESTATE without a mass.             */
int feahip_solve_dynamic(feahip_ctx *ctx, int n_steps, double dt, double beta, double gamma, double dlambda,
                         int max_newton, double desired_tolerance, int solver_type, double solver_tolerance,
                         int solver_max_iter, double *tol_log, int tol_log_cap, int *its_log, int *steps_done);
/* ---- Rayleigh damping ------------------------------------------------------
 * feahip_set_damping gives the context the viscous damping
 *   C = alpha M + beta_k K_d.
 * M is the mass of the loop that runs: the consistent mass of feahip_set_mass
 * in feahip_solve_dynamic and feahip_consistent_acceleration, the HRZ-lumped
 * mass in feahip_solve_explicit.  It is not copied: a later feahip_set_mass is
 * followed by the alpha part.  K_d is a SNAPSHOT: the plain tangent at the x
 * of this call (no contact term, unmasked), assembled once and copied into a
 * store of its own over the owned rows -- allocated only when beta_k > 0, as
 * large as K.  After such a call K holds that plain assembly and counts as
 * changed; f, u and x are untouched.  feahip_set_materials leaves K_d alone.
 * A constant C keeps the damping linear: with K_d = K(X0), every undamped mode
 * omega gets zeta = (alpha / omega + beta_k omega) / 2.
 *   feahip_solve_dynamic: with c1 = gamma / (beta dt) and w = vt + c1 (x - xt)
 *   the residual is f - a0 M (x - xt) - C w, the matrix
 *   K + (a0 + c1 alpha) M + c1 beta_k K_d.
 *   feahip_consistent_acceleration: M a = lambda F_ext - T - C v.
 *   feahip_solve_explicit: a = (f / ml - alpha vh) / (1 + alpha dt / 2), the
 *   central-difference scheme with the centred velocity; its stability limit
 *   is 2 / omega_max for every alpha >= 0, so feahip_stable_step is unchanged.
 *   A context with beta_k > 0 is refused there (FEAHIP_EINVAL).
 * Static solves, the arc length, modes and buckling ignore the damping.
 * (0, 0) clears it and frees the store; a context without damping launches
 * nothing new.  A negative or non-finite coefficient is FEAHIP_EINVAL and
 * leaves the context as it was.  The call is per context, not collective: a
 * rank assembles its own rows (x current on its halo nodes, as for every
 * assembly).  After a change of the row shard every entry that needs K_d
 * returns FEAHIP_ESTATE until the damping is set again; alpha > 0 without a
 * mass is FEAHIP_ESTATE at the use.                                          */
int feahip_set_damping(feahip_ctx *ctx, double alpha, double beta_k);
int feahip_get_damping(feahip_ctx *ctx, double *alpha, double *beta_k);
/* y = C v, host vectors [3N] in the caller's dof order (test hook, the
 * conventions of feahip_mass_spmv).  FEAHIP_ESTATE without damping.          */
int feahip_damping_spmv(feahip_ctx *ctx, const double *v, double *y);
/* Host only: the two coefficients that give the damping ratios zeta1, zeta2 at
 * the circular frequencies omega1, omega2:
 *   alpha  = 2 w1 w2 (z1 w2 - z2 w1) / (w2^2 - w1^2),
 *   beta_k = 2 (z2 w2 - z1 w1) / (w2^2 - w1^2).
 * FEAHIP_EINVAL for equal or non-positive frequencies.  A negative result (the
 * two ratios cannot both be met with C >= 0) is returned as it is;
 * feahip_set_damping refuses it.                                             */
int feahip_host_rayleigh(double omega1, double zeta1, double omega2, double zeta2, double *alpha, double *beta_k);

/* Host-only (no device): resolve faces to (owning element, local face) exactly
 * as feahip_set_surface_loads does; returns FEAHIP_EINVAL with the index of
 * the first bad face in *bad (-1 when all resolve).  Local faces: TET4 / TET10
 * 0..3 = opposite vertex 3, 2, 1, 0; HEX8 0..5 = t = -1, t = +1, s = -1,
 * r = +1, s = +1, r = -1.                                                   */
int feahip_host_surface_faces(int n_nodes, int n_elems, int npe, const int *elements, int n_faces,
                              int nodes_per_face, const int *face_nodes, int *face_elem, int *face_local,
                              int *bad);

/* ---- multi-GPU: row-sharded operation ---------------------------------- */
/* The reference is one process; sharding is new.  Nodes (block rows of K,
 * entries of f, u, x) are owned by one rank each, in contiguous ranges; a rank
 * assembles every element touching its rows, so assembly needs no exchange.
 * The linear solve exchanges halo rows (ncclSend/ncclRecv between slab
 * neighbours) and all-reduces one to three doubles per CG step; the Newton
 * test <u,f> is all-reduced so every rank takes the same branch.
 *
 * One process per GPU: rank 0 calls feahip_comm_unique_id (128 bytes),
 * broadcasts it by any means (bench.py: torch.distributed), every rank calls
 * feahip_comm_init; after that the ordinary entries above (create_stiffness,
 * apply_prescribed_bc, solve_slae, energy, update_nodes_with_solution, solve)
 * are collective over the ranks.  A rank holds the K rows, the modified-Newton
 * copy, the assembly maps and the multigrid hierarchy of its own slab only;
 * the mesh arrays handed to feahip_create are the whole mesh on every rank
 * (DESIGN.md section 6 says what is sharded and what is not).                */
int feahip_comm_unique_id(void *out, int cap);
int feahip_comm_init(feahip_ctx *ctx, int rank, int nranks, const void *unique_id);
/* nodes with LIBRARY id in [row0, row1) are this rank's; getters are
 * authoritative there only (feahip_node_numbering maps the caller's node ids
 * to library ids: a slab of library ids is a slab of the mesh, not a range of
 * the caller's ids)                                                          */
int feahip_owned_rows(feahip_ctx *ctx, int *row0, int *row1);

/* A rank that holds only its slab.  feahip_create_rank takes the same arguments
 * as feahip_create plus (rank, nranks) and builds the context of ONE rank: the
 * nodes it owns (a slab of library ids), the elements that touch them, their
 * halo nodes -- locally indexed, owned nodes first -- with the block rows, K,
 * maps, vectors and multigrid hierarchy of that sub-mesh only, and the halo plan
 * installed.  Nothing in it is sized by the whole mesh (the reference's single
 * row-wise store, fea_solver.c:444-448, becomes nranks independent ones).  Its
 * node- and element-indexed entries speak LOCAL indices: feahip_rank_maps says
 * which nodes / elements of the caller's mesh they are; feahip_rank_counts:
 * out8 = {local nodes, owned nodes (local ids [0, owned)), local elements,
 * nodes of the whole mesh, blocks of all local rows, blocks of the owned rows,
 * rows sent per exchange, rows received}.  After feahip_comm_init (same rank,
 * nranks) or feahip_group_init the collective entries work as for row shards. */
int feahip_create_rank(feahip_ctx **out, int device, int rank, int nranks,
                       int n_nodes, int n_elems, int npe, int gauss_count,
                       const double *gauss_weights, const double *dforms,
                       const int *elements, const double *nodes0,
                       int model, const double *model_params, int params_count,
                       int n_presc, const int *presc_node, const int *presc_type,
                       const double *presc_values);
/* The same rank context from the caller's OWN slab: a caller that partitions its
 * mesh itself (every MPI code does) hands over its local nodes -- [0, n_own)
 * the nodes it owns, then the halo nodes: every other node of an element that
 * touches an owned node -- those elements in LOCAL node ids, and for every halo
 * node the rank that owns it.  No argument is sized by the whole mesh and
 * nothing of that size is allocated.  The context is a rank context in every
 * respect (feahip_rank_counts / _maps, feahip_owned_rows, feahip_comm_init,
 * feahip_group_*, multigrid, line search, surface loads).  It keeps the local
 * order it is given; the order of the owned rows is what the assembly kernels
 * see, and feahip_host_slab_order below offers a good one.
 *   n_global_nodes  nodes of the whole mesh (reports and the range of
 *                   node_global only)
 *   elements        [n_elems][npe] LOCAL node ids; every element has an owned
 *                   node, and the rank holds EVERY element touching its nodes
 *   node_global     [n_local] the caller's global id, distinct
 *   elem_global     [n_elems] or NULL (then 0..n_elems-1); reports only
 *   halo_owner      [n_local - n_own] owning rank of local node n_own + i
 * Halo plan: derived from the local elements and halo_owner.  The two ends of an
 * exchange are built in different processes and share only node_global, so the
 * rows to and from a peer travel in ascending GLOBAL node id on both sides
 * (feahip_create_rank orders them by library id).
 * Prescribed dofs: presc_node in LOCAL ids, and the caller passes the entries
 * of EVERY local node, halo nodes included: an owned row's column at a
 * prescribed halo dof is cancelled from it (feahip_apply_prescribed_bc), which
 * the rank can only do if it knows the dof is prescribed.
 * Surface loads on such a context (feahip_set_surface_loads) take faces in
 * LOCAL node ids, all of whose nodes are local; a face that touches no owned
 * node is dropped silently (another rank's), any other bad face is refused.
 * Refused with FEAHIP_EINVAL, feahip_create_error naming the offending index:
 * n_own outside [1, n_local]; an element id outside [0, n_local); an element
 * with no owned node; a halo node no element touches; halo_owner outside
 * [0, nranks) or equal to rank; node_global outside [0, n_global_nodes) or
 * repeated; a prescribed id outside [0, n_local).                            */
int feahip_create_rank_local(feahip_ctx **out, int device, int rank, int nranks,
        int n_global_nodes,
        int n_local, int n_own,
        int n_elems, int npe, int gauss_count,
        const double *gauss_weights, const double *dforms,
        const int *elements,
        const double *nodes0,          /* [n_local][3]                            */
        const int *node_global,
        const int *elem_global,
        const int *halo_owner,
        int model, const double *model_params, int params_count,
        int n_presc, const int *presc_node /* LOCAL ids */, const int *presc_type,
        const double *presc_values);
/* Host-only (no device): the halo plan feahip_create_rank_local installs, in
 * GLOBAL node ids -- counts3 = {peers, rows sent, rows received} by a sizing
 * call with null lists, then the lists as feahip_host_rank_plan gives them.
 * The same validation (without the range of node_global: no n_global_nodes
 * here), the message through feahip_create_error.                            */
int feahip_host_rank_local_plan(int rank, int nranks, int n_local, int n_own, int n_elems, int npe,
        const int *elements, const int *node_global, const int *halo_owner,
        int *counts3, int *peers, int *send_off, int *recv_off, int *send_idx, int *recv_idx);
/* Host-only (no device): a local order that suits the kernels -- the library's
 * numbering (csrc/renumber.cpp) of the LOCAL mesh, split stably into owned
 * first, halo after.  new_local_id[n_local]: the new local id of local node a
 * (owned ids stay in [0, n_own)); the caller permutes its arrays by it.
 * Returns 1 when it reorders, 0 when the order given is kept, negative on
 * error.                                                                     */
int feahip_host_slab_order(int n_local, int n_own, int n_elems, int npe, const int *elements,
        const double *nodes0, int *new_local_id);
int feahip_rank_counts(feahip_ctx *ctx, long long *out8);
int feahip_rank_maps(feahip_ctx *ctx, int *node_global, int *elem_global);
/* Host-only (no device): the same sub-mesh without a context -- counts8 =
 * {local nodes, owned nodes, local elements, blocks of the owned rows, blocks
 * of all local rows, peers, rows sent, rows received}; with non-null arrays
 * (sized by a first call): the caller's ids of the local nodes and elements,
 * and the block rows of the OWNED nodes as the rank builds them from its own
 * elements (rowptr[owned + 1], colidx = the caller's id of the column node).  */
int feahip_host_rank_mesh(int rank, int nranks, int n_nodes, int n_elems, int npe,
                          const int *elements, const double *nodes0, long long *counts8,
                          int *node_global, int *elem_global, long long *rowptr, int *colidx);

/* Host-only: that sub-mesh's halo plan in the caller's node ids -- counts3 =
 * {peers, rows sent, rows received} by a first call with null lists, then
 * peers[npeers], send_off / recv_off[npeers + 1], send_idx / recv_idx in the
 * order the rows travel.                                                      */
int feahip_host_rank_plan(int rank, int nranks, int n_nodes, int n_elems, int npe,
                          const int *elements, const double *nodes0, int *counts3, int *peers,
                          int *send_off, int *recv_off, int *send_idx, int *recv_idx);

/* In-process group: n contexts of the same mesh (on any devices) driven by one
 * host thread; halo rows move by device copies, sums on the host.  Same
 * kernels and halo plan as the RCCL path.                                    */
int feahip_group_init(feahip_ctx **ctxs, int n);
int feahip_group_solve_slae(feahip_ctx **ctxs, int n, int solver_type, double tolerance,
                            int max_iterations, int *iters, double *resid);
int feahip_group_energy(feahip_ctx **ctxs, int n, double *tolerance);
int feahip_group_update_nodes_with_solution(feahip_ctx **ctxs, int n);
int feahip_group_solve(feahip_ctx **ctxs, int n, int load_increments, int max_newton,
                       int modified_newton, double desired_tolerance, int solver_type,
                       double solver_tolerance, int solver_max_iter, double *tol_log,
                       int tol_log_cap, int *its_log, int *steps_done);
int feahip_group_solve_dynamic(feahip_ctx **ctxs, int n, int n_steps, double dt, double beta, double gamma,
                               double dlambda, int max_newton, double desired_tolerance, int solver_type,
                               double solver_tolerance, int solver_max_iter, double *tol_log, int tol_log_cap,
                               int *its_log, int *steps_done);
/* ---- explicit dynamics: central differences on a lumped mass --------------
 * The state (x, v, a, time, load factor) is the Newmark state, with the same
 * getters and setters: a caller may switch between feahip_solve_dynamic and
 * feahip_solve_explicit on one context.  All entries below return
 * FEAHIP_ESTATE without a mass (feahip_set_mass); the lumped mass is built on
 * the first of them, from the rule and the densities of the last
 * feahip_set_mass, and again when the shard or the material ids change.
 *
 * feahip_get_lumped_mass: ml[N] in the caller's node ids, HRZ-lumped per
 * element (ml_a = sum_e m_e d_a / sum_b d_b, d_a = sum_g rho w det J0 N_a^2):
 * positive on every element type, each element's mass kept.  Authoritative on
 * the owned rows of a sharded context, zero elsewhere.
 *
 * feahip_stable_step (collective like feahip_consistent_acceleration):
 * *dt_crit = 2 / sqrt(max_i sum_j |K_ij| / ml(i)), Gershgorin's bound on the
 * largest frequency of M_L^-1 K with K the tangent at the current x (assembled
 * here, not masked: K holds another matrix afterwards, as after an assembly).
 *
 * feahip_kinetic_energy (collective): 1/2 sum ml |v|^2 over the owned nodes.
 *
 * feahip_solve_explicit: n_steps of
 *   vh = v + dt/2 a;  x += dt vh  (prescribed dofs: x += dlambda * value);
 *   load factor += dlambda;  f = lambda (F_surf + F_body) - T(x);
 *   a = f / ml;  v = vh + dt/2 a;  time += dt
 * with a = 0 and v = dlambda * value / dt on the prescribed dofs.  One residual
 * assembly and two pointwise kernels per step; no stiffness assembly, no solve.
 * dt > 0: a fixed step (safety, restep ignored).  dt == 0: dt = safety *
 * feahip_stable_step, estimated before the first step and again every restep
 * steps (restep <= 0: once); 0 < safety <= 1.  dt_log (may be NULL) receives
 * the step used in each step, up to dt_log_cap entries.  Elements with
 * det J <= 0 (or NaN) at a Gauss point are counted by a pass of their own over
 * the current nodes, on every element type alike, before every estimate and
 * once after the last step; nothing is read back anywhere else.  The counts
 * of all ranks meet in a max all-reduce before anything depends on them: an
 * inversion on any rank ends the loop on every rank with
 * FEAHIP_ENOTCONVERGED, *steps_done = the steps done at the previous check,
 * and the state is left as it is -- explicit steps cannot be rolled back.
 * feahip_update_state reports that count afterwards.
 * v and a are authoritative on owned nodes only: a halo node holds
 * v = (its displacement of the step) / dt and a = 0.
 * FEAHIP_EINVAL: dt < 0, n_steps < 0, safety outside (0, 1] with dt == 0.   */
int feahip_get_lumped_mass(feahip_ctx *ctx, double *ml);
int feahip_stable_step(feahip_ctx *ctx, double *dt_crit);
int feahip_kinetic_energy(feahip_ctx *ctx, double *e);
int feahip_solve_explicit(feahip_ctx *ctx, int n_steps, double dt, double safety, int restep,
                          double dlambda, double *dt_log, int dt_log_cap, int *steps_done);
int feahip_group_solve_explicit(feahip_ctx **ctxs, int n, int n_steps, double dt, double safety,
                                int restep, double dlambda, double *dt_log, int dt_log_cap,
                                int *steps_done);
/* ---- results: nodal stress, strain energy, reactions -----------------------
 * What a load case is read by, recovered on the device from the current nodes
 * and the material table in force (nothing is cached between calls).  A context
 * that never calls these allocates and launches nothing for them.  The
 * reference has no counterpart: it exports the Gauss-point tensors only.
 *
 * feahip_get_nodal_stresses: the volume-weighted average of the Cauchy stress
 * over the selected elements at node a,
 *   sigma_a = (sum_{e at a} sum_g vol_eg sigma_eg) / (sum_{e at a} sum_g vol_eg),
 * sigma_eg and vol_eg = w_g |det J_g| those of the current configuration on the
 * stiffness rule, with the element's own (lambda, mu) under a material table.
 * sig6[N][6] in the order xx, yy, zz, xy, yz, xz (the upper entries of the
 * averaged tensor); von_mises[N] = sqrt(3/2 s:s) with s the deviator of
 * sigma_a -- the von Mises stress of the average, not the average of the von
 * Mises stresses; weight[N] = the denominator.  Any of the three may be NULL.
 * All are indexed by the caller's node ids (local ids on a rank context).
 * material = -1 selects all elements, material = m in [0, n_materials) those
 * with that id: stress is discontinuous across a material interface and an
 * average across one means nothing.  A node no selected element touches gets
 * stress 0 and weight 0.  FEAHIP_EINVAL for an id outside the table, and for
 * m >= 0 on a context without one.  On a sharded context the result is
 * authoritative on the owned rows and zero elsewhere, like
 * feahip_get_lumped_mass; no exchange is needed.
 *
 * feahip_strain_energy: W = sum_e sum_g w_g det J0_g Psi(F_eg) over the
 * stiffness rule, det J0 = det J / det F, with the potential of the model's
 * stress:  COMPRESSIBLE_NEOHOOKEAN  Psi = mu/2 (tr b - 3) - mu ln J
 *                                         + lambda/2 (ln J)^2
 *          A5                       Psi = lambda/2 (tr E)^2 + mu E:E,
 *                                   E = (F'F - I)/2.
 * Collective like feahip_kinetic_energy: an in-process group is driven from
 * any of its members, the ranks of an RCCL run all make the call.  Every node
 * of an element takes the share W_e / npe and a rank sums the shares of the
 * nodes it owns, so a ghost element is counted once.  feahip_get_nodal_energy
 * returns those shares, w_node[N] in the caller's ids, owned rows only.  No
 * inversion check is made: with det F <= 0 the NaN propagates, and
 * feahip_update_state still reports the inversions.
 *
 * feahip_get_reactions: r[3N] in the caller's dof order.  On every prescribed
 * dof c, r_c = T_c(x) - lambda (F_surf(x) + F_body)_c, minus the unmasked
 * residual at that dof (feahip_apply_prescribed_bc overwrites f there, so the
 * residual is assembled again here); zero on every other dof; authoritative on
 * the owned rows.  The inertia term of a dynamic context is NOT included: on a
 * moving body this is the internal force minus the applied loads at the
 * support, not the force the support exerts.  K, f, u, x, the cached F / sigma
 * and the count feahip_update_state reports are left exactly as they were.
 *
 * All four return FEAHIP_EINVAL on a null context or a null required output. */
int feahip_get_nodal_stresses(feahip_ctx *ctx, int material,
                              double *sig6, double *von_mises, double *weight);
int feahip_strain_energy(feahip_ctx *ctx, double *W);
int feahip_get_nodal_energy(feahip_ctx *ctx, double *w_node);
int feahip_get_reactions(feahip_ctx *ctx, double *r);

/* ---- modal analysis: the lowest natural frequencies and mode shapes ---------
 * feahip_solve_modes: the n_modes lowest eigenpairs of K(x) phi = lambda M phi
 * on the free dofs, by a blocked LOBPCG whose basis is M-orthonormalised at
 * every step.  A context that never calls the entries below allocates and
 * launches nothing for them.  The reference has no counterpart.
 *   K  the tangent at the current nodes, assembled here (feahip_create_stiffness)
 *      and masked with feahip_apply_prescribed_bc(ctx, 0.0): what the PCG and
 *      the multigrid see.  K and f hold another matrix afterwards, as after
 *      feahip_stable_step and feahip_consistent_acceleration.
 *   M  the consistent mass of feahip_set_mass, per-material densities included,
 *      used unmasked: the iteration lives in the subspace of vectors that vanish
 *      on the prescribed dofs -- every vector it builds is zero there and the
 *      M-products are zeroed there.
 * lambda[n_modes] is ascending and holds omega^2 (not its root).  The modes are
 * M-orthonormal and exactly 0 on the prescribed dofs.  The sign of a mode is
 * arbitrary but the same bits on every call: the start block is a fixed integer
 * hash of (library dof index, column) mapped to [-1, 1), no random state and no
 * clock.  The block width is FEA_MODAL_COLS = 8 and 1 <= n_modes <= 8; all eight
 * columns iterate (the surplus are guard vectors), no locking, no deflation.
 * Converged: for every M-normalised column j < n_modes, r_j = K x_j - theta_j M x_j
 * has ||r_j|| <= tolerance (||K x_j|| + |theta_j| ||M x_j||) in the 2-norm.
 * resid[n_modes] (may be NULL) receives that ratio from FRESH products K X, M X
 * at return, *iters (may be NULL) the Rayleigh-Ritz steps taken.  After
 * max_iterations steps without convergence: FEAHIP_ENOTCONVERGED, with lambda,
 * resid and the modes left as they stand.
 * Preconditioner: the context's own (feahip_set_preconditioner) -- kind 0 the
 * 3x3 block-Jacobi inverse, kind 1 one W-cycle per column and step; kind 2 is
 * refused.  warm != 0 with modes held from an earlier call on this context:
 * the solve starts from them (all eight columns, the guard columns included),
 * and a converged restart at an unchanged state returns with *iters == 0 and
 * nothing touched; warm == 0 starts from the hash.
 * FEAHIP_ESTATE: no mass, or a stale one.  FEAHIP_EINVAL: n_modes outside
 * [1, 8], tolerance <= 0, max_iterations < 0, null lambda, fewer than 24 free
 * dofs; a context with a transport, a row shard or made by feahip_create_rank*
 * (refused like feahip_solve_slae2, feahip_last_error says which).
 * A body with zero-energy modes (no or too few supports) is NOT refused and
 * nothing is promised for it: the relative test cannot be met at lambda = 0,
 * and no shift is offered.
 * Memory: nine block vectors, 9 x 192 bytes per node, plus 13 MB of partial
 * sums, allocated on the first call and kept until feahip_destroy.
 *
 * feahip_get_modes: modes [first, first + count) of the last solve (all eight
 * columns are held), phi[count][3N] in the caller's dof order.  FEAHIP_ESTATE
 * before any solve, FEAHIP_EINVAL for a range outside [0, 8] or null phi.     */
#define FEA_MODAL_COLS 8
int feahip_solve_modes(feahip_ctx *ctx, int n_modes, double tolerance, int max_iterations, int warm,
                       double *lambda /*[n_modes]*/, double *resid /*[n_modes], may be NULL*/, int *iters /*may be NULL*/);
int feahip_get_modes(feahip_ctx *ctx, int first, int count, double *phi);
/* [Y, Z] = [K X, mask(M X)] for eight columns in one pass over K's pattern,
 * host vectors [8][3N] in the caller's dof order; Z is zero on the prescribed
 * dofs (test hook for the block product of feahip_solve_modes, refused as that
 * solve is; FEAHIP_ESTATE before the first stiffness assembly; modes held from
 * a solve are dropped)                                                        */
int feahip_spmm_km(feahip_ctx *ctx, const double *x8, double *y8, double *z8);
/* feahip_solve_modes over the ranks of a sharded run: the same pencil, stop
 * test, block of eight columns and outputs, on row shards and on
 * feahip_create_rank / feahip_create_rank_local contexts that have a transport.
 * COLLECTIVE like feahip_consistent_acceleration: an in-process group
 * (feahip_group_init) is driven from any one member, the ranks of an RCCL run
 * (feahip_comm_init) all make the call.  Every rank works on the rows it owns:
 * the halo rows of a block vector travel before its product (192 bytes per
 * row, under the product of the rows that read no halo column), and the 24
 * norms and 768 Gram sums of a step are all-reduced (792 doubles) before the
 * one Rayleigh-Ritz step every rank then takes on identical numbers.  The
 * preconditioner is the rank's own: kind 0 its 3x3 block-Jacobi inverses,
 * kind 1 one W-cycle per column on its diagonal block of K.
 * lambda, resid and *iters are the same on every rank.  Afterwards
 * feahip_get_modes on each context gives the rank's own rows and zero on all
 * others (as feahip_get_lumped_mass does); the rows of all ranks together are
 * M-orthonormal over the whole mesh and 0 on the prescribed dofs.
 * The start block is the hash of feahip_solve_modes keyed by the node's
 * identity in the whole mesh (the library id on a row shard, node_global on a
 * rank context), so it does not depend on the cut; the same input on the same
 * number of ranks gives the same bits (a group sums in rank order).
 * warm: as in feahip_solve_modes, when every rank holds modes of a sharded
 * solve on its current rows.  Modes of this solve are not a start for
 * feahip_solve_modes on the same context, nor the reverse: either solve
 * drops the other's.
 * FEAHIP_EINVAL: n_modes outside [1, 8], tolerance <= 0, max_iterations < 0,
 * null lambda; a context without a transport (feahip_solve_modes is the solve
 * for it); preconditioner 2; ranks whose preconditioner kinds differ; fewer
 * than 24 free dofs over all ranks (one rank may own fewer, or none).
 * FEAHIP_ESTATE: no mass, or a stale one, on any rank.  Refusals that depend
 * on other ranks are all-reduced: every rank returns the same code.
 * Memory per rank: feahip_solve_modes' nine block vectors over the rank's
 * local nodes (owned and halo), plus 192 bytes per row sent and per row
 * received, allocated on the first call.                                     */
int feahip_solve_modes_sharded(feahip_ctx *ctx, int n_modes, double tolerance, int max_iterations, int warm,
                               double *lambda /*[n_modes]*/, double *resid /*[n_modes], may be NULL*/, int *iters /*may be NULL*/);
/* Test hook for the sharded block product, shaped like
 * feahip_group_apply_preconditioner: x8[k], y8[k], z8[k] are [8][3 N_k] in
 * context k's own dof order.  Only the owned rows of x8[k] matter: the halo
 * rows of X come by the block exchange.  y8[k] = K X and z8[k] = mask(M X) on
 * rank k's rows, zero elsewhere.  FEAHIP_ESTATE before the first stiffness
 * assembly or without a mass; modes held are dropped.                        */
int feahip_group_spmm_km(feahip_ctx **ctxs, int n, const double *const *x8, double *const *y8, double *const *z8);
/* Host-only (no device): the Rayleigh-Ritz step of feahip_solve_modes.  gram_m,
 * gram_k: S' M S and S' K S, n_dirs x n_dirs (8, 16 or 24), row-major, S = [X, W,
 * P] in blocks of eight.  Scales by diag(gram_m)^-1/2, eigendecomposes by cyclic
 * Jacobi, drops directions with eigenvalue <= 1e-12 x the largest, and returns
 * theta[8] ascending and coef[n_dirs][16]: columns 0-7 give X_new = S C_x,
 * columns 8-15 P_new = X_new - X C_x[X rows] (the part of X_new that lies in
 * [W, P]: its X rows are zero).  Returns the rank kept, or -1
 * when fewer than eight directions are left or an entry is not finite.        */
int feahip_host_modal_ritz(int n_dirs, const double *gram_m, const double *gram_k, double *theta, double *coef);

/* ---- modal analysis, more than eight modes and free bodies --------------------
 * feahip_solve_modes_locked: the n_modes lowest eigenpairs of the same pencil,
 * 1 <= n_modes <= FEA_MODAL_MAX_LOCKED, in sweeps of the eight-column block with
 * hard locking, on the shifted pencil (K + shift M, M), shift >= 0.
 *   shift  K's store holds K_s = K + shift M on the free dofs (assembled, the
 *      mass added, masked: the order of a Newmark iteration), so the products
 *      and both preconditioners see K_s.  The iteration finds theta_s = lambda +
 *      shift; lambda[] is UNSHIFTED, near 0 for the rigid-body modes of a free
 *      body.  With shift > 0 K_s is positive definite and the stop test is well
 *      posed at lambda = 0: give a shift of the order of the first elastic
 *      eigenvalue expected (no automatic choice is made).  shift == 0 is the
 *      supported body; a free body with shift == 0 behaves as under
 *      feahip_solve_modes: not refused, nothing promised.
 *   sweep  the block is deflated against the locked modes and orthonormalised
 *      on its own; it iterates as feahip_solve_modes does, with the
 *      preconditioned residuals deflated against the locked modes
 *      (W <- W - Q (MQ' W), on the device, nothing read back) before they are
 *      multiplied; it stops when its leading min(6, n_modes - locked) columns
 *      (two guard columns) pass the stop test on fresh products.  The leading
 *      converged columns, contiguous from column 0 and within n_modes, are
 *      locked; the others move to the front and the freed columns are filled
 *      from the hash with column indices not used before.  lambda[] is
 *      ascending: the pairs are sorted once more at return, because two
 *      eigenvalues equal to rounding (a degenerate pair split by the end of
 *      a sweep) can come out of two sweeps in either order.
 * Converged: ||K_s x - theta_s M x|| <= tolerance (||K_s x|| + |theta_s| ||M x||),
 * the ratio resid[] reports.  *iters: the Rayleigh-Ritz steps summed over all
 * sweeps, capped by max_iterations; *sweeps: the sweeps.  When the steps run
 * out: FEAHIP_ENOTCONVERGED, the pairs locked so far in lambda / resid (NaN
 * after them), their count in feahip_get_locked_count, their modes readable.
 * The same input gives the same bits.  Refused: what feahip_solve_modes refuses,
 * n_modes outside [1, 64], a negative or non-finite shift, fewer than
 * n_modes + 24 free dofs.  K and f hold another matrix afterwards, the block
 * of feahip_solve_modes is scratch (feahip_get_modes and warm restarts behave
 * as before any solve), and there is no warm restart of this solve.
 * Memory: 2 x ceil(n_modes / 8) block vectors and up to 8 MB of partial sums on
 * top of feahip_solve_modes', allocated on the first call for the n_modes
 * asked (a larger request later reallocates).
 * feahip_get_locked_modes: modes [first, first + count) of the locked store,
 * phi[count][3N] in the caller's dof order, M-orthonormal, 0 on the prescribed
 * dofs.  FEAHIP_ESTATE before a locked solve, FEAHIP_EINVAL outside those
 * locked.                                                                      */
#define FEA_MODAL_MAX_LOCKED 64
int feahip_solve_modes_locked(feahip_ctx *ctx, int n_modes, double shift, double tolerance, int max_iterations,
                              double *lambda /*[n_modes]*/, double *resid /*[n_modes], may be NULL*/,
                              int *iters /*may be NULL: Rayleigh-Ritz steps over all sweeps*/,
                              int *sweeps /*may be NULL*/);
int feahip_get_locked_modes(feahip_ctx *ctx, int first, int count, double *phi /*[count][3N], caller's dof order*/);
int feahip_get_locked_count(feahip_ctx *ctx, int *count);
/* lambda[count] of the modes first .. first + count - 1 held (feahip_solve_modes_locked or feahip_response_set_basis),
 * ascending and unshifted: the values the response entries use.  FEAHIP_ESTATE without modes held, FEAHIP_EINVAL for a
 * range outside them. */
int feahip_get_locked_lambda(feahip_ctx *ctx, int first, int count, double *lambda /*[count]*/);
/* Test hook for the deflation kernels: out8 = x8 - Q (MQ' x8) with MQ = mask(M Q)
 * from the block product, q[n_locked][3N], x8 and out8 [8][3N] host vectors in
 * the caller's dof order, 1 <= n_locked <= 64.  Refused where feahip_spmm_km is;
 * modes held from either solve are dropped.                                   */
int feahip_modal_deflate(feahip_ctx *ctx, int n_locked, const double *q, const double *x8, double *out8);

/* ---- frequency response by mode superposition on the locked modes -------------
 * The steady-state amplitude u(w) e^{iwt} under a harmonic load F e^{iwt}, F real,
 * from the n_locked <= 64 M-orthonormal pairs (lam_k, phi_k) the locked store
 * holds.  A context that never calls the entries below allocates and launches
 * nothing for them.
 *     q_k    = phi_k' F                                     (participation)
 *     d_k    = alpha + beta_k lam_k + 2 zeta_k sqrt(max(lam_k, 0))
 *     H_k(w) = 1 / (lam_k - w^2 + i w d_k)
 *     u(w)   = u_s + sum_k phi_k a_k(w)
 *   mode displacement (static_correction == 0):  u_s = 0,   a_k = q_k H_k
 *   mode acceleration (static_correction != 0):  K u_s = F on the free dofs,
 *                                                a_k = q_k (H_k - 1 / lam_k)
 * K is the tangent at the current nodes, masked as feahip_apply_prescribed_bc
 * with factor 0 masks it.  The three parts of d_k are additive; zeta (one ratio
 * per mode, ascending lam) may be NULL, which means zero.  With all modes of the
 * body the sum is the solution of (K - w^2 M + i w (alpha M + beta_k K)) u = F;
 * with the lowest m the correction carries the static part of the modes left
 * out, which is most of their share below the m-th frequency (DESIGN.md 21
 * has the truncation errors measured).  No system in K - w^2 M is ever solved.
 * The damping of feahip_set_damping is NOT read: its K_d is a snapshot at other
 * nodes which these modes do not diagonalise.  alpha, beta_k and zeta are the
 * caller's, per call.
 *
 * feahip_response_set_basis: installs the caller's pairs, lam[n] in any order
 * and phi[n][3N] in the caller's dof order, M-orthonormal on the caller's word
 * (no M-product is made), zeroed on the prescribed dofs, into the locked store
 * as modes of a solve with shift 0, column k of the store the k-th pair by
 * ascending lam (equal ones in the caller's order): the superposition kernels
 * sum in column order, so the order the pairs are listed in does not reach the
 * bits of any result.  feahip_get_locked_modes and feahip_get_locked_count then
 * return them, ascending in lam.  For modes kept
 * from an earlier run.  Refused: the contexts feahip_solve_modes_locked refuses
 * and a context without a mass, n outside [1, 64], a lam that is not finite.
 * The block of feahip_solve_modes is scratch, as under feahip_modal_deflate.
 *
 * feahip_response_load: q (k_response_project: one read of F and of the panels
 * in use, a fixed grid, a two-stage sum in a fixed order, no atomics) and, with
 * static_correction != 0, u_s: K assembled at the current nodes, masked with
 * factor 0, and K u_s = F solved by the context's PCG and preconditioner
 * (solver_type, tolerance, max_iterations, *iters and *resid as under
 * feahip_solve_slae; they are not read without the correction, where *iters is
 * 0).  F[3N] is in the caller's dof order; its entries on the prescribed dofs
 * are not read.  q[n_locked] (may be NULL): ascending lam.  Afterwards K, f
 * and u hold other values, as after feahip_consistent_acceleration; x, v, a,
 * the time, the load factor and the locked store are untouched.
 * FEAHIP_ESTATE without modes held.  FEAHIP_EINVAL: a correction asked for
 * when the modes come from a solve with shift > 0 or any lam_k <= 0 (a free
 * body's K is singular; such a body may still be swept without correction);
 * the contexts feahip_solve_modes_locked refuses (a transport, a row shard,
 * feahip_create_rank*, preconditioner 2); an F that is not finite; with the
 * correction an unknown solver_type or max_iterations <= 0.
 * FEAHIP_ENOTCONVERGED from the solve is passed on, and returned as well when
 * its iterations run out above the tolerance (a u_s that is not one would be
 * wrong at every frequency); no load is held then.
 * A later locked solve, feahip_response_set_basis or any entry that drops the
 * locked modes (feahip_modal_deflate, feahip_solve_buckling, the timing hooks
 * 16-17) invalidates the load: the entries below return FEAHIP_ESTATE until
 * the next load.
 * feahip_get_response_static: u_s[3N] of the load held, caller's dof order,
 * exactly 0 on the prescribed dofs (all zero without the correction).
 *
 * feahip_response_sweep: the host makes the table a_k(w_j) of all frequencies
 * (the code behind feahip_host_response_coefficients), it goes to the device
 * in one copy and ONE launch of k_response_sweep walks it: a lane owns a dof,
 * holds its n_locked mode values in registers and keeps the largest
 * |u_i(w_j)|^2 and its index.
 *   peak[i]     max_j |u_i(w_j)|
 *   peak_at[i]  the lowest j that attains it
 * both [3N], caller's dof order, exactly 0 on the prescribed dofs.  Probes:
 * n_probe <= 64 dofs (3 node + axis, caller's numbering) whose full complex
 * curves come back, probe_re / probe_im [n_probe][n_freq] (may be NULL with
 * n_probe == 0); the host sums them from the probes' rows of the store and of
 * u_s and from the same table, in the kernel's order.  omega[n_freq] are
 * circular frequencies in any order.  The same input gives the same bits.
 * FEAHIP_ESTATE without a load held for the modes held.  FEAHIP_EINVAL: n_freq
 * outside [1, FEA_RESPONSE_MAX_FREQ]; a negative or non-finite omega, alpha,
 * beta_k or zeta_k; a coefficient that is not finite (w = 0 on a zero mode,
 * w^2 = lam_k with d_k = 0); n_probe outside [0, 64]; a probe dof outside
 * [0, 3N).  Nothing of the context's state changes.
 * feahip_response_field: re[3N] and im[3N] of u(omega), caller's dof order, by
 * the field-writing instantiation of the same kernel at one frequency.
 *
 * feahip_host_response_coefficients (no device): coef[n_freq][2][64], re then
 * im, mode k of the arrays given at column k, zero past n_modes.  Returns
 * FEAHIP_EINVAL where the sweep does, and for lam_k <= 0 with the correction.
 * The corrected coefficient is evaluated as q (w^2 a - b^2 - i b lam) /
 * (lam (a^2 + b^2)), a = lam - w^2, b = w d, which has no cancellation where
 * w^2 << lam.
 * Memory: 3 x 3N doubles, 1 MB of partial sums and the 4 MB table, on top of
 * the locked store, allocated by the first load.  Not offered: sharded runs,
 * complex loads and a phase between loads, residual vectors beyond the one
 * static correction.                                                          */
#define FEA_RESPONSE_MAX_FREQ 4096
int feahip_response_set_basis(feahip_ctx *ctx, int n, const double *lam /*[n]*/, const double *phi /*[n][3N], caller's dofs*/);
int feahip_response_load(feahip_ctx *ctx, const double *F /*[3N]*/, int static_correction, int solver_type, double tolerance,
                         int max_iterations, double *q /*[n_locked], may be NULL*/, int *iters /*may be NULL*/,
                         double *resid /*may be NULL*/);
int feahip_get_response_static(feahip_ctx *ctx, double *u_s /*[3N]*/);
int feahip_response_sweep(feahip_ctx *ctx, int n_freq, const double *omega /*[n_freq]*/, double alpha, double beta_k,
                          const double *zeta /*[n_locked] or NULL*/, double *peak /*[3N]*/, int *peak_at /*[3N]*/,
                          int n_probe, const int *probe_dof /*[n_probe]*/, double *probe_re,
                          double *probe_im /*[n_probe][n_freq], may be NULL with n_probe == 0*/);
int feahip_response_field(feahip_ctx *ctx, double omega, double alpha, double beta_k, const double *zeta /*[n_locked] or NULL*/,
                          double *re /*[3N]*/, double *im /*[3N]*/);
int feahip_host_response_coefficients(int n_modes, const double *lam, const double *q, int n_freq, const double *omega,
                                      double alpha, double beta_k, const double *zeta /*[n_modes] or NULL*/,
                                      int static_correction, double *coef /*[n_freq][2][64], zero past n_modes*/);

/* ---- transient response by mode superposition, base excitation ----------------
 * The response to F g(t) from rest, F the load held (feahip_response_load or
 * feahip_response_base_load), g given at the n_steps + 1 times t_n = n dt and
 * linear in between.  Every mode held obeys
 *     q'' + d_k q' + lam_k q = q_k g(t),     d_k as above,
 * and is advanced by the exact propagator of a linear load,
 *     (q, q')_{n+1} = A_k (q, q')_n + b0_k q_k g_n + b1_k q_k g_{n+1},
 *     A_k = exp(dt [[0, 1], [-lam_k, -d_k]]),
 * so there is no stability limit on dt: a mode with omega dt = 50 is as safe as
 * one with 0.01.  A_k, b0_k and b1_k come from power series on a step
 * dt / 2^s with |lam_k| (dt / 2^s)^2 <= 1/2 and d_k dt / 2^s <= 1/2, doubled s
 * times, in long double: under-, critically and over-damped modes, lam_k = 0
 * and lam_k = +-1e-12 are no special cases.  One coefficient row per step:
 *   quantity 0  u(t_n) = u_s g_n + sum_k phi_k a_k(n), a_k = q(t_n) without the
 *               static correction (u_s = 0), a_k = q(t_n) - q_k g_n / lam_k with
 *               it (mode acceleration: the modes left out respond statically)
 *   quantity 1  v(t_n) = sum_k phi_k q'(t_n)
 *   quantity 2  a(t_n) = sum_k phi_k (q_k g_n - d_k q' - lam_k q), relative to
 *               the base under a base load
 * Velocity and acceleration carry no static term, correction or not.
 *
 * feahip_response_base_load: the load of a rigid base acceleration along dir,
 *     F = -M r on the free dofs, 0 on the prescribed ones,
 * r the translation dir on ALL dofs, the prescribed ones included (the supports
 * move with the ground; the response is relative to the base).  M r is one
 * launch of the mass product, which reads every column.  The rest is
 * feahip_response_load: the projection, with static_correction != 0 the solve
 * K u_s = F, and the load is held for sweep, field and transient alike.
 *   q[n_locked]         phi_k' F, ascending lam
 *   gamma[n_locked]     the participation factors phi_k' M r = -q_k
 *   eff_mass[n_locked]  gamma_k^2 (the modes are M-orthonormal)
 *   *total_mass         r' M r over all dofs (|dir|^2 times the body's mass)
 * Each may be NULL.  Refused where feahip_response_load is, and with
 * FEAHIP_EINVAL for a dir that is zero or not finite.
 *
 * feahip_response_transient: the host makes the rows (the code behind
 * feahip_host_transient_coefficients), FEA_TRANSIENT_CHUNK at a time; a chunk
 * and its g_n go through the coefficient buffer of the frequency sweep, so no
 * device allocation grows with n_steps, and one launch of k_transient_sweep per
 * chunk walks it: a lane owns a dof, holds its n_locked mode values in
 * registers, and keeps the largest |u_i(t_n)| and its step; every launch after
 * the first continues from what the one before left.  The host fills the next
 * chunk while one runs.
 *   peak[i]     max_n |u_i(t_n)| of the quantity asked for
 *   peak_at[i]  the lowest step n that attains it
 * both [3N], caller's dof order, exactly 0 on the prescribed dofs.  Probes:
 * n_probe <= 64 dofs whose whole histories come back, probe[n_probe][n_steps +
 * 1], summed on the host in the kernel's order.  Snapshots: n_snap <= 4096
 * steps whose field comes back, snap[n_snap][3N], one launch of the
 * field-writing instantiation each; a snapshot's value at a probe dof has the
 * bits of the probe's history at that step.  The same input gives the same
 * bits.  FEAHIP_ESTATE without modes held or without a load held for them, as
 * feahip_response_sweep.  FEAHIP_EINVAL: a row-sharded or feahip_create_rank*
 * context; n_steps outside [1, FEA_TRANSIENT_MAX_STEPS]; dt not positive or
 * not finite; a g that is not finite; quantity outside 0..2; a negative or
 * non-finite alpha, beta_k or zeta_k; n_probe outside [0, 64] or a probe dof
 * outside [0, 3N); n_snap outside [0, 4096] or a snapshot step outside [0,
 * n_steps]; a null required array; a coefficient that is not finite.  x, v, a,
 * the time, the load factor, K, f, u and the locked store are untouched; the
 * table of the last frequency sweep is gone (hook 23 of feahip_time_kernel is
 * refused until the next sweep, and hook 25 after one).
 *
 * feahip_host_transient_coefficients (no device): coef[n_steps + 1][64], mode k
 * of the arrays given at column k, zero past n_modes; the very rows the device
 * entry uses, bit for bit.  Refuses what the device entry refuses of the same
 * arguments, and lam_k <= 0 with the correction.
 * Not offered: sharded runs, several load patterns with their own histories in
 * one call, non-zero initial conditions, a static term in velocity and
 * acceleration.                                                                */
#define FEA_TRANSIENT_MAX_STEPS 1048576
#define FEA_TRANSIENT_CHUNK     8064    /* rows of a launch: 8064 x 64 coefficients and 8064 g_n fill the sweep's 4 MB table */
int feahip_response_base_load(feahip_ctx *ctx, const double *dir /*[3]*/, int static_correction, int solver_type,
                              double tolerance, int max_iterations, double *q /*[n_locked]*/, double *gamma /*[n_locked]*/,
                              double *eff_mass /*[n_locked]*/, double *total_mass, int *iters, double *resid /*each may be NULL*/);
int feahip_response_transient(feahip_ctx *ctx, int n_steps, double dt, const double *g /*[n_steps + 1]*/, double alpha,
                              double beta_k, const double *zeta /*[n_locked] or NULL*/, int quantity, double *peak /*[3N]*/,
                              int *peak_at /*[3N]*/, int n_probe, const int *probe_dof /*[n_probe]*/,
                              double *probe /*[n_probe][n_steps + 1]*/, int n_snap, const int *snap_step /*[n_snap]*/,
                              double *snap /*[n_snap][3N]*/);
int feahip_host_transient_coefficients(int n_modes, const double *lam, const double *q, int n_steps, double dt,
                                       const double *g /*[n_steps + 1]*/, double alpha, double beta_k,
                                       const double *zeta /*[n_modes] or NULL*/, int static_correction, int quantity,
                                       double *coef /*[n_steps + 1][64], zero past n_modes*/);

/* ---- response spectrum and random vibration on the locked modes ----
 * Both ask one thing of the modes and the load held: on every dof a quadratic
 * form of its own mode values x_i = (phi_i1 .. phi_im),
 *     out_i = sqrt(max(0, x_i' C x_i + 2 u_s,i (b' x_i) + s u_s,i^2)),
 * C[m][m] symmetric, b[m] and s the same for every dof and made on the host.
 * k_response_combine evaluates it in one launch: a lane owns a dof, holds its
 * mode values in registers and reads the table, folded onto its upper triangle,
 * through the scalar data cache; m (m + 1) / 2 + 2 m FMAs per dof, whatever the
 * number of frequencies behind C.  A context that never calls the entries below
 * allocates and launches nothing for them; the table is a device buffer of its
 * own (about 33 KB, made by the first call), so the tables of the last sweep
 * and of the last transient stay (hooks 23 and 25 of feahip_time_kernel).
 *
 * feahip_response_combine: the form as given.  C[n_locked][n_locked] and
 * b[n_locked] (NULL: zero) by ascending mode, `absolute` != 0 takes |phi_ik|
 * for every mode value (the ABS rule is the form C = |a||a|').  out[3N] in the
 * caller's dof order, exactly 0 on the prescribed dofs and where the form is
 * negative.  The same input gives the same bits.  FEAHIP_EINVAL: C not
 * symmetric to the bit, or C, twice an off-diagonal entry of C (the table holds
 * the upper triangle doubled), b or s not finite.
 *
 * feahip_response_random: the RMS under a one-sided PSD S(w) per rad/s of the
 * load factor g (the load is F g(t), int S dw the mean square of g), given at
 * n_freq strictly ascending omega_j.  With a(w_j) the coefficient row of
 * feahip_response_sweep (that very code), wt_j the trapezoid weights and p =
 * quantity (0 displacement, 1 velocity, 2 acceleration)
 *     C_kl = sum_j wt_j S_j w_j^(2p) Re(a_k conj(a_l))
 *     b_k  = sum_j wt_j S_j w_j^(2p) Re(a_k),   s = sum_j wt_j S_j w_j^(2p)
 * (b = 0, s = 0 for a load held without the static correction), accumulated in
 * long double: rms_i^2 is the trapezoid rule of S |(i w)^p u_i(w)|^2 over the
 * fields feahip_response_field returns.  modal_cov[n_locked][n_locked] (may be
 * NULL) receives C.  n_freq in [2, FEA_RANDOM_MAX_FREQ].
 * feahip_host_random_form is the same builder without a device; it refuses what
 * feahip_response_sweep refuses of the same arguments, an omega that is not
 * strictly ascending and an S that is negative or not finite.
 * feahip_host_random_grid: a grid that resolves every peak, the union of
 * n_background >= 2 points of linspace(w_lo, w_hi), for every mode with lam_k >
 * 0 and d_k > 0 the n_per_mode points w_k + (d_k / 2) tan(theta_i), theta_i =
 * ((i + 1/2) / n_per_mode) pi - pi / 2 (the substitution that makes a
 * Lorentzian peak flat), and the caller's breakpoints: *n_out of them at the
 * front of omega_out on entry.  Clipped to [w_lo, w_hi], sorted, duplicates
 * removed; *n_out is the count on return.  omega_out holds n_background +
 * n_modes n_per_mode + the breakpoints; NULL asks for the count alone (no
 * breakpoints then).  FEAHIP_EINVAL also for more than FEA_RANDOM_MAX_FREQ
 * points.
 * feahip_host_psd_value: the table (w[n_pts] strictly ascending, S[n_pts]) at
 * `at`, linear or (loglog != 0) linear in the logarithms, a point's own value at
 * a point, zero outside the table.  feahip_host_spectrum_value: the same with
 * the end values outside.  NaN for a table that is none.
 *
 * feahip_response_spectrum: the design peak under a response spectrum Sa(w)
 * (n_pts points, w in rad/s) with the load held; under a base load q_k =
 * -gamma_k.  sa_k = Sa(sqrt(lam_k)), a_k = q_k sa_k / lam_k the peak modal
 * displacement (times sqrt(lam_k), lam_k for quantity 1, 2: pseudo-velocity and
 * -acceleration).  rule FEAHIP_SRSS: C = diag(a_k^2).  FEAHIP_CQC: C_jk =
 * rho_jk a_j a_k,
 *     rho_jk = 8 sqrt(z_j z_k) (z_j + r z_k) r^1.5 /
 *              ((1 - r^2)^2 + 4 z_j z_k r (1 + r^2) + 4 (z_j^2 + z_k^2) r^2),
 * r = w_k / w_j, z_k = d_k / (2 w_k) (Der Kiureghian, unequal damping); rho_kk
 * = 1 exactly, a zero denominator off the diagonal gives 1, all z = 0 gives the
 * SRSS table.  FEAHIP_ABS: C = |a||a|' on |phi|.  Missing mass: with a load
 * held with the static correction, zpa > 0 and quantity 0 the rigid residual
 * zpa (u_s + sum_k phi_k c_k), c_k = -q_k / lam_k, is added by SRSS: C += zpa^2
 * c c', b = zpa^2 c, s = zpa^2.  modal_peak[n_locked] (may be NULL) receives
 * a_k.  FEAHIP_EINVAL: lam_k <= 0 for any mode, an unknown rule or quantity, a
 * negative or non-finite sa or zpa, zpa != 0 at quantity 1 or 2, without the
 * static correction or with FEAHIP_ABS (the residual needs the signed values).
 * feahip_host_spectrum_form is the builder without a device, sa[n_modes] given.
 *
 * The three device entries: FEAHIP_ESTATE without modes held or without a load
 * held for them, FEAHIP_EINVAL on a row-sharded or feahip_create_rank* context,
 * as feahip_response_transient; x, v, a, the time, the load factor, K, f, u,
 * the locked store, the load held and both coefficient tables are untouched.
 * Not offered: sharded runs, combining several excitation directions, absolute
 * (base-plus-relative) acceleration, closed-form PSD integrals, cross-spectra
 * between several loads, zero-crossing rates and fatigue counts.               */
#define FEA_RANDOM_MAX_FREQ 262144
enum { FEAHIP_SRSS = 0, FEAHIP_CQC = 1, FEAHIP_ABS = 2 };
int feahip_response_combine(feahip_ctx *ctx, const double *C /*[n_locked][n_locked]*/, const double *b /*[n_locked] or NULL*/,
                            double s, int absolute, double *out /*[3N]*/);
int feahip_response_random(feahip_ctx *ctx, int n_freq, const double *omega /*[n_freq]*/, const double *S /*[n_freq]*/,
                           double alpha, double beta_k, const double *zeta /*[n_locked] or NULL*/, int quantity,
                           double *rms /*[3N]*/, double *modal_cov /*[n_locked][n_locked] or NULL*/);
int feahip_response_spectrum(feahip_ctx *ctx, int n_pts, const double *w /*[n_pts]*/, const double *sa /*[n_pts]*/, int loglog,
                             int rule, double alpha, double beta_k, const double *zeta /*[n_locked] or NULL*/, double zpa,
                             int quantity, double *peak /*[3N]*/, double *modal_peak /*[n_locked] or NULL*/);
int feahip_host_random_form(int n_modes, const double *lam, const double *q, int n_freq, const double *omega, const double *S,
                            double alpha, double beta_k, const double *zeta /*[n_modes] or NULL*/, int static_correction,
                            int quantity, double *C /*[n_modes][n_modes]*/, double *b /*[n_modes]*/, double *s);
int feahip_host_random_grid(int n_modes, const double *lam, double alpha, double beta_k, const double *zeta /*[n_modes] or NULL*/,
                            double w_lo, double w_hi, int n_background, int n_per_mode, double *omega_out /*or NULL*/,
                            int *n_out);
double feahip_host_psd_value(int n_pts, const double *w, const double *S, int loglog, double at);
double feahip_host_spectrum_value(int n_pts, const double *w, const double *sa, int loglog, double at);
int feahip_host_spectrum_form(int n_modes, const double *lam, const double *q, const double *sa /*[n_modes]*/, double alpha,
                              double beta_k, const double *zeta /*[n_modes] or NULL*/, int rule, int static_correction,
                              double zpa, int quantity, double *C /*[n_modes][n_modes]*/, double *b /*[n_modes]*/, double *s);

/* ---- stress from mode superposition: modal stresses, RMS and peak von Mises ----
 * The linear map from a displacement increment du at the current nodes x to
 * the nodal Cauchy stress it causes.  At a Gauss point, g[a][j] = dN_a/dx_j,
 *     l_ij = sum_a du_a,i g[a][j],   d = (l + l') / 2
 *     dsigma = c : d + l sigma + sigma l' - tr(d) sigma
 * sigma the Cauchy stress of the point, c the spatial tangent of the model:
 *   Neo-Hookean  c : d = (lambda / J) tr(d) I + 2 ((mu - lambda ln J) / J) d
 *   A5, b = F F' c : d = (lambda (b : d) b + 2 mu b d b) / J
 * (the coefficients l1, m1 of the stiffness; for A5 the stiffness takes them on
 * the identity, the stress increment on b).  The nodal value keeps the weights
 * of feahip_get_nodal_stresses, held fixed,
 *     T_a = sum_e sum_g vol_g dsigma_g / sum_e sum_g vol_g,  vol_g = w_g |det J_g|
 * over all elements at the node (material = -1) or over those of one material
 * id; a node that touches no selected element returns 0.  Components xx yy zz
 * xy yz xz.  At an unstressed state this is exactly the derivative of
 * feahip_get_nodal_stresses; at a prestressed state it leaves out the variation
 * of the weights.  Two kernels (k_mstress_elements, k_mstress_nodes) work a
 * panel of eight columns at a time; no atomics, the same input gives the same
 * bits.  A context that never calls the entries below allocates and launches
 * nothing for them; the first call allocates the element records [E][6][8],
 * the [6N] outputs, the two panels of the single-vector path ([3N][8] in,
 * [6N][8] out: 72 N doubles) and, for the basis, the stress store of 6N x 8
 * doubles per panel of eight modes -- twice the locked store.
 *
 * feahip_stress_increment: the map for one vector du[3N] in the caller's dof
 * order, sig6[N][6] in the caller's node order.  Needs no modes and no mass.
 * FEAHIP_EINVAL: a material outside the table, du not finite.
 * feahip_response_stress_basis: the stress store of the modes held, at the
 * current nodes: T_k for every mode, column for column the locked store.  With
 * a load held with the static correction also T_s from u_s (bit for bit
 * feahip_stress_increment of u_s); T_s = 0 otherwise.  FEAHIP_ESTATE without
 * modes held.  Whatever invalidates the load invalidates the store: a later
 * locked solve, feahip_response_set_basis, feahip_modal_deflate,
 * feahip_solve_buckling, hooks 16-17 of feahip_time_kernel; a new load
 * invalidates T_s, and with it the entries below until the basis is built
 * again.  The store is that of the nodes at the call: it does not follow x.
 * feahip_get_modal_stresses: sig6[count][N][6] of the modes [first, first +
 * count) by ascending lam.  feahip_get_response_static_stress: T_s[N][6].
 * feahip_response_stress_field: sig6 = cs T_s + sum_k coef_k T_k (coef by
 * ascending mode, one fma per store column onto cs T_s) and vm[N], its von
 * Mises stress: the stress of one row of feahip_host_response_coefficients
 * (the real and the imaginary part each with a call of its own, cs = 1 for the
 * real part of a load held with the correction) or of
 * feahip_host_transient_coefficients (cs = g_n).
 *
 * The forms.  For a linear combination y = L T_a of the rows of a node (an
 * m-vector of mode values) and y_s = L T_s,a, with (C, b, s) as
 * feahip_response_combine takes them,
 *     q(y) = y' C y + 2 y_s (b' y) + s y_s^2
 *     out6[a][c] = sqrt(max(0, q(T_a,c)))
 *     vm[a] = sqrt(max(0, (q(xx-yy) + q(yy-zz) + q(zz-xx)) / 2
 *                          + 3 (q(xy) + q(yz) + q(xz))))
 * -- the RMS (or design peak) of the von Mises stress is a quadratic form of
 * its own in the modal covariance (Segalman et al.), not a function of the
 * component values.  k_stress_combine evaluates the nine forms of a node in one
 * launch, a lane per node, one combination in registers at a time.
 * feahip_response_stress_combine: the form as given, with the checks of
 * feahip_response_combine; vm may be NULL.  feahip_response_stress_random: the
 * form of feahip_host_random_form at quantity 0; modal_cov as
 * feahip_response_random.  feahip_response_stress_spectrum: the form of
 * feahip_host_spectrum_form at quantity 0; with FEAHIP_ABS the components take
 * |T| and peak_vm must be NULL (FEAHIP_EINVAL otherwise: the differences need
 * the signs); peak_vm may be NULL under the other rules.
 *
 * All entries but feahip_stress_increment: FEAHIP_ESTATE without modes held;
 * the entries after the basis also without a store for these modes or with a
 * load made since; the three with a form also without a load held.  Every
 * entry: FEAHIP_EINVAL on a row-sharded or feahip_create_rank* context, as
 * feahip_response_transient.  x, v, a, the time, the load factor, K, f, u, the
 * locked store, the load held and all three coefficient tables (hooks 23, 25,
 * 26) are untouched: the form table of the stresses is a buffer of its own.
 * Not offered: sharded runs (stress peaks over a whole sweep or transient in
 * one launch are feahip_response_stress_sweep and _transient below), principal
 * stresses, a signed von Mises stress, the variation of the weights at a
 * prestressed state, superconvergent recovery.                               */
int feahip_stress_increment(feahip_ctx *ctx, const double *du /*[3N]*/, int material, double *sig6 /*[N][6]*/);
int feahip_response_stress_basis(feahip_ctx *ctx, int material);
int feahip_get_modal_stresses(feahip_ctx *ctx, int first, int count, double *sig6 /*[count][N][6]*/);
int feahip_get_response_static_stress(feahip_ctx *ctx, double *sig6 /*[N][6]*/);
int feahip_response_stress_field(feahip_ctx *ctx, const double *coef /*[n_locked]*/, double cs, double *sig6 /*[N][6]*/,
                                 double *vm /*[N]*/);
int feahip_response_stress_combine(feahip_ctx *ctx, const double *C /*[n_locked][n_locked]*/, const double *b /*[n_locked] or NULL*/,
                                   double s, double *out6 /*[N][6]*/, double *vm /*[N] or NULL*/);
int feahip_response_stress_random(feahip_ctx *ctx, int n_freq, const double *omega /*[n_freq]*/, const double *S /*[n_freq]*/,
                                  double alpha, double beta_k, const double *zeta /*[n_locked] or NULL*/, double *rms6 /*[N][6]*/,
                                  double *rms_vm /*[N] or NULL*/, double *modal_cov /*[n_locked][n_locked] or NULL*/);
int feahip_response_stress_spectrum(feahip_ctx *ctx, int n_pts, const double *w /*[n_pts]*/, const double *sa /*[n_pts]*/,
                                    int loglog, int rule, double alpha, double beta_k, const double *zeta /*[n_locked] or NULL*/,
                                    double zpa, double *peak6 /*[N][6]*/, double *peak_vm /*[N] or NULL; NULL with FEAHIP_ABS*/,
                                    double *modal_peak /*[n_locked] or NULL*/);

/* ---- stress peaks over a frequency sweep or a transient, one launch each ----
 * The largest stress of every node over all rows of a coefficient table, where
 * feahip_response_stress_field gives the stress of one row.  With T_k[N][6] the
 * stress store of feahip_response_stress_basis and T_s the stress of the
 * static correction, components xx yy zz xy yz xz:
 *   sweep      a_k = coef[j][0][k] + i coef[j][1][k], the table of
 *              feahip_response_sweep:  s_c = T_s,a,c + sum_k T_k,a,c a_k
 *   transient  the rows of feahip_response_transient at quantity 0:
 *              sigma_c = T_s,a,c g_n + sum_k T_k,a,c a_k(n)
 * one fma per store column in ascending column order onto the static term,
 * the order of feahip_response_stress_field: the components of a row have the
 * bits of that entry for (coef_row, cs).
 *   peak6[a][c]    = max_j |s_c|   or   max_n |sigma_c|
 *   vm[a]          = the largest von Mises stress.  Transient: of sigma,
 *                    sqrt(1.5 (dx^2 + dy^2 + dz^2 + 2 (xy^2 + yz^2 + xz^2))) on
 *                    the deviator d = sigma - mean.  Sweep: the largest value
 *                    over the CYCLE of sigma(t) = re cos wt - im sin wt, which
 *                    is not the von Mises stress of the amplitudes: with V the
 *                    von Mises form, A = re' V re, B = im' V im, C = re' V im,
 *                      vm^2(t) = (A + B)/2 + ((A - B)/2) cos 2wt - C sin 2wt
 *                      vm_peak^2 = (A + B)/2 + sqrt(((A - B)/2)^2 + C^2)
 *                    evaluated on the deviators of re and im (the expanded form
 *                    sum p^2 - (sum p)^2 / 3 loses a nearly hydrostatic state).
 *   peak6_at, vm_at  the lowest row that attains the peak (a strict comparison).
 * All four in the caller's node ids.  Up to 64 probe nodes (caller's ids): the
 * six components of every row, probe_re / probe_im [n_probe][n_freq][6] and
 * probe [n_probe][n_steps + 1][6], summed on the host in the kernels' order:
 * bit for bit feahip_response_stress_field of that row.
 * k_stress_sweep / k_stress_transient (kernels_stress_sweep.hip): a lane owns
 * a stress row and keeps its 8 P store values in registers, a wave takes ten
 * nodes; the six lanes of a node meet across lanes for the von Mises form.
 * The transient goes FEA_TRANSIENT_CHUNK rows at a time, each launch continuing
 * from the peaks of the one before.  No LDS memory, no atomics, the same bits on
 * every call.
 * FEAHIP_EINVAL: what feahip_response_sweep and feahip_response_transient
 * refuse, for the same arguments (n_freq outside [1, FEA_RESPONSE_MAX_FREQ], a
 * negative or non-finite omega, a coefficient that is not finite, n_steps, dt,
 * g, the damping), n_probe outside [0, 64], a probe node outside [0, N); a
 * row-sharded or feahip_create_rank* context.  FEAHIP_ESTATE where
 * feahip_response_stress_random gives it: no modes, no load, no stress store for
 * them, a load made since.  A refused call leaves its outputs as they were.
 * The first call allocates a coefficient table of its own (4 MB) and the two
 * index arrays: the table of the last displacement sweep, the last chunk of the
 * last transient and both forms stay (hooks 23, 25, 26, 28), as do x, v, a, the
 * time, K, f and u.  Hooks 29 and 30 of feahip_time_kernel launch over the last
 * table again.  A context that never calls these entries allocates and launches
 * nothing for them.
 * feahip_host_harmonic_von_mises: vm_peak of one complex stress state, the
 * kernel's arithmetic on the host (no device).
 * Not offered: sharded runs, principal stresses, a signed von Mises stress,
 * stress rates (velocity, acceleration), several loads with a phase between
 * them.                                                                       */
int feahip_response_stress_sweep(feahip_ctx *ctx, int n_freq, const double *omega /*[n_freq]*/, double alpha, double beta_k,
                                 const double *zeta /*[n_locked] or NULL*/, double *peak6 /*[N][6]*/, int *peak6_at /*[N][6]*/,
                                 double *vm /*[N]*/, int *vm_at /*[N]*/, int n_probe, const int *probe_node /*[n_probe]*/,
                                 double *probe_re /*[n_probe][n_freq][6]*/, double *probe_im /*[n_probe][n_freq][6]*/);
int feahip_response_stress_transient(feahip_ctx *ctx, int n_steps, double dt, const double *g /*[n_steps + 1]*/, double alpha,
                                     double beta_k, const double *zeta /*[n_locked] or NULL*/, double *peak6 /*[N][6]*/,
                                     int *peak6_at /*[N][6]*/, double *vm /*[N]*/, int *vm_at /*[N]*/, int n_probe,
                                     const int *probe_node /*[n_probe]*/, double *probe /*[n_probe][n_steps + 1][6]*/);
double feahip_host_harmonic_von_mises(const double re6[6], const double im6[6]);

/* ---- random-vibration fatigue: spectral moments, rates and damage per node ----
 * A part under random vibration is qualified on fatigue life.  Seven stress
 * processes per node: the six components xx yy zz xy yz xz, and as the seventh
 * the equivalent von Mises process of Preumont and Piefort, whose PSD is
 * trace(V G_sigma(w)): its moments are the von Mises combination of the nine
 * forms, (q(xx-yy) + q(yy-zz) + q(zz-xx)) / 2 + 3 (q(xy) + q(yz) + q(xz)),
 * evaluated as k_stress_combine evaluates it.
 *   moments  m_n = integral of w^n G(w) dw, n = 0, 1, 2, 4, w in rad per unit
 *            time, by the trapezoid rule of feahip_host_random_form with the
 *            weight wt_j S_j w_j^n (feahip_host_moment_form: order 0, 2, 4 are
 *            that entry at quantity 0, 1, 2 bit for bit; it refuses what that
 *            entry refuses, and any other order).  A moment is max(0, form):
 *            sqrt(m0) has the bits of feahip_response_stress_random.
 *   rates    nu0 = sqrt(m2 / m0) / 2 pi (zero up-crossings) and nup =
 *            sqrt(m4 / m2) / 2 pi (peaks), cycles per unit time; 0 where a
 *            moment under the root is 0.
 *   damage   per unit time on the S-N curve N s^b = A, s the stress
 *            AMPLITUDE, 1 <= b <= 64, A > 0, by three estimators: [0] narrow
 *            band, (nu0 / A) (2 m0)^(b/2) Gamma(1 + b/2); [1] Dirlik's density
 *            in closed form; [2] Tovo and Benasciutti, [bw + (1 - bw)
 *            alpha2^(b - 1)] D_NB, with alpha1 = m1 / sqrt(m0 m2) and alpha2 =
 *            m2 / sqrt(m0 m4) clamped to [0, 1] (csrc/fatigue_point.h has every
 *            formula, one copy for the device and the host).
 *   status   bit 0: m0 = 0 or m2 = 0 (no stress: a node outside the material of
 *            the stress basis), every rate and damage 0; bit 1: 1 - alpha2 <=
 *            1e-6, the narrow-band limit, where Dirlik's parameters leave their
 *            range: the three damages are equal; bit 2: Dirlik's parameters are
 *            no density (one not finite, a negative weight, Q <= 0): [1] takes
 *            the value of [2].  No value is NaN for finite input.
 * feahip_response_stress_moments: four forms of the caller's own, C4[4][n][n],
 * b4[4][n] and s4[4] by ascending mode as feahip_response_stress_combine takes
 * one (b4, s4 NULL: zero), evaluated on the nine combinations of every node in
 * ONE launch (k_stress_moments, the form as the grid's second dimension).
 * feahip_response_stress_fatigue: the four forms of feahip_host_moment_form on
 * the load held, then k_fatigue_rates, a lane per (node, process) pair; any of
 * the four outputs may be NULL.  feahip_host_fatigue: the statistics of n sets
 * of moments in long double, rounded once (no device): the reference of the
 * kernel, and an entry for moments of the caller's own; rates, damage, status
 * may be NULL; FEAHIP_EINVAL for a moment that is negative or not finite.
 * Both device entries need what feahip_response_stress_random needs and refuse
 * what it refuses, with the same codes; FEAHIP_EINVAL for b outside [1, 64], A
 * not positive, either not finite.  K, f, u, x, v, a, the time, the tables of
 * the sweeps and both forms (hooks 26, 28) stay: the four tables are a buffer
 * of their own.  No atomics, the same bits on every call; a context that never
 * calls these entries allocates and launches nothing for them.
 * Not offered: sharded runs, a mean-stress correction, multi-slope S-N curves,
 * the expected extreme over a duration, principal or signed von Mises stress,
 * several loads with cross-spectra.                                          */
int feahip_host_moment_form(int n_modes, const double *lam, const double *q, int n_freq, const double *omega, const double *S,
                            double alpha, double beta_k, const double *zeta /*[n_modes] or NULL*/, int static_correction,
                            int order /*0, 1, 2 or 4*/, double *C /*[n_modes][n_modes]*/, double *b /*[n_modes]*/, double *s);
int feahip_host_fatigue(int n, const double *m /*[n][4]: m0, m1, m2, m4*/, double sn_b, double sn_a, double *rates /*[n][2] or NULL*/,
                        double *damage /*[n][3] or NULL*/, int *status /*[n] or NULL*/);
int feahip_response_stress_moments(feahip_ctx *ctx, const double *C4 /*[4][n_locked][n_locked]*/,
                                   const double *b4 /*[4][n_locked] or NULL*/, const double *s4 /*[4] or NULL*/,
                                   double *moments /*[N][7][4]*/);
int feahip_response_stress_fatigue(feahip_ctx *ctx, int n_freq, const double *omega /*[n_freq]*/, const double *S /*[n_freq]*/,
                                   double alpha, double beta_k, const double *zeta /*[n_locked] or NULL*/, double sn_b, double sn_a,
                                   double *moments /*[N][7][4] or NULL*/, double *rates /*[N][7][2] or NULL*/,
                                   double *damage /*[N][7][3] or NULL*/, int *status /*[N][7] or NULL*/);

/* ---- rainflow fatigue of a transient: cycles and Miner damage per node ---------
 * A part under a shock, a drop, a sine burst or any measured history is
 * qualified on the cycles it has seen.  feahip_response_stress_rainflow counts
 * them for every stress row of the transient of feahip_response_stress_transient
 * in the launches that make the history: ASTM E1049-85's three-point rule,
 * streamed a sample at a time on a bounded stack (csrc/rainflow_point.h has the
 * rule, one copy for the device and the host).
 *   processes  0..5 the six components xx yy zz xy yz xz: the very rows of
 *              feahip_response_stress_transient, same table, same fma order,
 *              the same bits.  6 + p the linear projection sum_c proj[p][c]
 *              sigma_c, n_proj <= FEA_RAINFLOW_MAX_PROJ: the normal stress on a
 *              plane of normal n is the row (nx^2, ny^2, nz^2, 2 nx ny, 2 ny nz,
 *              2 nx nz), so up to 48 planes give a critical-plane search on the
 *              normal stress.  A projection is formed on the store, one fma per
 *              component in ascending order from 0, before the time loop.
 *   damage     sum of count (range / 2)^b / A in counting order: Miner's sum on
 *              the S-N curve N s^b = A, s the stress AMPLITUDE, 1 <= b <= 64,
 *              A > 0, 1 / A made once on the host.  A whole b takes the power
 *              by squaring and multiplying, any other by pow: the two differ
 *              in the last bits.
 *   cycles     the sum of the counts, a multiple of 0.5;  max_range the largest
 *              counted range;  depth_used the most points the stack held.
 *   status     bit 0 (FEAHIP_RAINFLOW_CONSTANT): fewer than two reversals, a
 *              constant history (a node outside the material of the stress
 *              basis), everything 0.  Bit 1 (FEAHIP_RAINFLOW_OVERFLOW): the stack
 *              is a ring of `depth` points, 4 <= depth <=
 *              FEA_RAINFLOW_MAX_DEPTH; a push onto a full ring first counts the
 *              two oldest points as half a cycle and drops the oldest, the rule
 *              ASTM has for the start point and the residue.  A ring-down, whose
 *              ranges only shrink, is counted exactly at any depth; only a later
 *              range large enough to close a dropped one makes the count
 *              approximate.  No value is NaN for finite input.
 * Outputs [N][6 + n_proj] in the caller's node ids, any of them NULL.  Up to 64
 * probe nodes: their histories [n_probe][n_steps + 1][6 + n_proj], summed on the
 * host in the kernel's order, so feahip_host_rainflow of a probe's history is
 * the device's count of that row in everything but the rounding of the damage
 * sum.  k_stress_rainflow (kernels_stress_rainflow.hip) has the lane layout of
 * k_stress_transient; the stack lives in device memory as [depth][6N], depth x
 * 6N doubles allocated by the first call and grown when a larger depth is
 * asked.  A pass of launches counts six processes per node; the passes of the
 * projections reuse the state of the one before.  No atomics, the same bits on
 * every call.
 * feahip_host_rainflow (no device): the count of one history of n samples in
 * the same arithmetic with the damage sum in long double, and the list of the
 * counted cycles in counting order (range, mean, count) into arrays of
 * `capacity` entries each (any of them NULL; n is always enough); *n_counted
 * the number counted.  FEAHIP_EINVAL for n < 1, a sample that is not finite, b,
 * A or depth out of range, a list too short (*n_counted then holds the number
 * needed).
 * The device entry needs what feahip_response_stress_transient needs and refuses
 * what it refuses, with the same codes; FEAHIP_EINVAL in addition for b, A,
 * depth or n_proj out of range, a proj entry that is not finite, proj NULL with
 * n_proj > 0.  A refused call leaves its outputs as they were.  x, v, a, the
 * time, K, f, u, the locked store, the load held and every table of the other
 * entries stay (hooks 23, 25, 26, 28, 29, 30): the coefficient chunk is a buffer
 * of its own.  A context that never calls the entry allocates and launches
 * nothing for it.
 * Not offered: sharded runs, a mean-stress correction (the cycle means are in
 * the host's list only), multi-slope S-N curves, an amplitude gate or racetrack
 * filter, a range histogram per node, signed von Mises and principal stresses,
 * critical planes on shear, counting the residue as a closed repeated block.  */
#define FEA_RAINFLOW_MAX_DEPTH 1024
#define FEA_RAINFLOW_MAX_PROJ  48
#define FEAHIP_RAINFLOW_CONSTANT 1
#define FEAHIP_RAINFLOW_OVERFLOW 2
int feahip_host_rainflow(int n, const double *series /*[n]*/, double sn_b, double sn_a, int depth, double *damage, double *cycles,
                         double *max_range, int *depth_used, int *status, int capacity, int *n_counted,
                         double *range /*[capacity] or NULL*/, double *mean /*[capacity] or NULL*/, double *count /*[capacity] or NULL*/);
int feahip_response_stress_rainflow(feahip_ctx *ctx, int n_steps, double dt, const double *g /*[n_steps + 1]*/, double alpha,
                                    double beta_k, const double *zeta /*[n_locked] or NULL*/, double sn_b, double sn_a, int depth,
                                    int n_proj, const double *proj /*[n_proj][6] or NULL*/, double *damage, double *cycles,
                                    double *max_range /*[N][6 + n_proj] or NULL, all three*/, int *status,
                                    int *depth_used /*[N][6 + n_proj] or NULL, both*/, int n_probe,
                                    const int *probe_node /*[n_probe]*/, double *probe /*[n_probe][n_steps + 1][6 + n_proj]*/);

/* ---- linear buckling: load factors and modes from K and its geometric part ----
 * feahip_solve_buckling: the n_modes lowest eigenpairs of
 *     K_sigma(x) phi = nu K(x) phi          on the free dofs,
 * by the blocked LOBPCG of feahip_solve_modes on another pencil.  A context that
 * never calls the entries below allocates and launches nothing for them.
 *   K        the tangent at the current nodes, assembled and masked as
 *            feahip_solve_modes does it; positive definite at a stable
 *            equilibrium.  K and f hold another matrix afterwards.
 *   K_sigma  the geometric (initial-stress) part of that tangent as a matrix of
 *            its own: the block of a node pair is sum_g vol_g (g_a . sigma_g g_b)
 *            times the 3x3 identity, so ONE double per block of K's pattern,
 *            assembled on the GPU at every call from the current nodes and the
 *            material table in force (both models, all three element types).
 * Model: along the load path K(gamma) ~ (K - K_sigma) + gamma K_sigma with
 * gamma = 1 now; it is singular at
 *     factor = 1 - 1/nu     for nu < 0,
 *     factor = +infinity    for nu >= 0 (no buckling in this load direction),
 * and the estimated critical load is `factor` times the load applied so far.
 * At a small preload this is classical linear buckling.  The follower-pressure
 * load stiffness is not part of the pencil (the library assembles none).
 * nu[n_modes] (may be NULL) is ascending, so the finite factors come first and
 * ascend; factor[n_modes] as above.  The modes are K-orthonormal
 * (phi_i' K phi_j = delta_ij) and exactly 0 on the prescribed dofs.  The same
 * input gives the same bits (the start block is feahip_solve_modes' hash).
 * Converged: for every column j < n_modes, on fresh products at return,
 *   ||K_sigma x_j - nu_j K x_j|| <= tolerance (||K_sigma x_j|| + |nu_j| ||K x_j||),
 * the ratio resid[] (may be NULL) reports; *iters (may be NULL): the
 * Rayleigh-Ritz steps.  After max_iterations steps: FEAHIP_ENOTCONVERGED with
 * the pairs as they stand.  Preconditioner: the context's own, kind 0 or 1,
 * which approximates K^-1 -- the natural one for this pencil.
 * If x_j' K x_j of a column of the block is not positive, K is not positive
 * definite at this state: FEAHIP_ENOTCONVERGED, and feahip_last_error says so
 * and names a passed critical point as the likely reason (factor, nu, resid
 * are NaN then).
 * It needs NO mass, and a context that has one keeps it untouched.  Refused
 * (FEAHIP_EINVAL) as feahip_solve_modes refuses: a transport, a row shard, a
 * feahip_create_rank* context, preconditioner 2, fewer than 24 free dofs,
 * n_modes outside [1, 8]; also tolerance <= 0, max_iterations < 0, null factor.
 * Modes held by feahip_solve_modes / feahip_solve_modes_locked are dropped (and
 * either of those solves drops the buckling modes).  Nothing is promised for
 * an unstressed body, where all nu are of rounding size.  Not offered: more
 * than eight modes, a sharded solve, a shift, a reference state other than the
 * current one.
 * Memory: feahip_solve_modes' nine block vectors, one double per block of K,
 * and npe (npe + 1) / 2 doubles per element.
 *
 * feahip_get_buckling_modes: modes [first, first + count) of the last buckling
 * solve (all eight columns are held), phi[count][3N] in the caller's dof order.
 * FEAHIP_ESTATE before any solve, FEAHIP_EINVAL for a range outside [0, 8].    */
int feahip_solve_buckling(feahip_ctx *ctx, int n_modes, double tolerance, int max_iterations,
                          double *factor /*[n_modes]*/, double *nu /*[n_modes], may be NULL*/,
                          double *resid /*[n_modes], may be NULL*/, int *iters /*may be NULL*/);
int feahip_get_buckling_modes(feahip_ctx *ctx, int first, int count, double *phi /*[count][3N]*/);
/* Test hook: y = K_sigma(current nodes) x, unmasked, host vectors [3N] in the
 * caller's dof order.  K_sigma is assembled on each call; refused on sharded or
 * rank contexts, as feahip_spmm_km is.                                         */
int feahip_geometric_spmv(feahip_ctx *ctx, const double *x, double *y);
/* Host-only (no device): factor[i] = 1 - 1/nu[i] for nu[i] < 0, +infinity
 * otherwise (nu = 0, -0.0 and positive nu: no buckling in this direction).     */
int feahip_host_buckling_factor(int n, const double *nu, double *factor);

/* z = M^-1 r on every rank of the group at once, with the preconditioner the
 * group's PCG applies: r[k] and z[k] are rank k's [N_k][3] vectors as
 * feahip_apply_preconditioner takes them (the caller's node ids of context k;
 * z[k] covers rank k's rows, 0 elsewhere).  Under preconditioner 2 the operator
 * spans the ranks and this is how it is applied without a solve.             */
int feahip_group_apply_preconditioner(feahip_ctx **ctxs, int n, const double *const *r,
                                      double *const *z);

/* Host-only (no device): the halo plan of one rank from the element->node
 * map, in the numbering it is given (a context plans in library ids: pass
 * elements translated by feahip_host_numbering to get what it gets).  First call with null lists fills counts[5] = {npeers, nsend, nrecv,
 * row0, row1}; second call fills peers[npeers], send_off/recv_off[npeers+1],
 * send_idx[nsend], recv_idx[nrecv] (node ids, ascending per peer).           */
int feahip_shard_plan(int n_nodes, int n_elems, int npe, const int *elements, int rank,
                      int nranks, int *counts, int *peers, int *send_off, int *recv_off,
                      int *send_idx, int *recv_idx);
/* Host-only (no device is touched): what the assembly maps `rank` of `nranks`
 * builds for ITS block rows say, as one hash per row of the set of (row,
 * column, element, local row node, local column node) contributions they
 * list; rows[0..1] = the rows the rank owns, rowhash[a] = 0 for every other
 * row.  The maps of a shard are cut differently from the unsharded ones, what
 * they say about a row must not be: the hashes of all ranks add up to the
 * unsharded ones (tests/test_host.py).                                      */
int feahip_host_assembly_digest(int n_nodes, int n_elems, int npe, const int *elements, int rank, int nranks,
                                unsigned long long *rowhash, int *rows);

/* Host-only (no device): shape of the GATHER maps (npe = 4, 10 or 8) for a
 * mesh in the numbering it is given (pass library ids to see what a context
 * builds): stats[8] = {chunks, element evaluations, distinct elements, rows,
 * chunks repeating their predecessor's map words, map bytes, chunks with a
 * block list / a diagonal list longer than a thread keeps in registers};
 * rows_hist[65] (may be null) = chunks by row count.  An element is evaluated
 * once per chunk that owns one of its nodes (fea_solver.c:887-1068 visits each
 * element once): evaluations / distinct elements is what a numbering costs.  */
int feahip_host_gather_stats(int n_nodes, int n_elems, int npe, const int *elements,
                             long long *stats, int *rows_hist);

/* Host-only (no device): the chunks of the 4-node GATHER maps of a mesh of
 * linear tetrahedra, in walk order, in the numbering given (as
 * feahip_host_gather_stats).  flags[capacity] (may be null when capacity is
 * 0): bit 0 the next chunk's map words equal this chunk's (the kernel keeps
 * them in registers), bit 1 a block list, bit 2 a diagonal list longer than
 * a thread keeps in registers.  Returns the number of chunks, or negative.   */
int feahip_host_gather_chunks(int n_nodes, int n_elems, const int *elements, int capacity, int *flags);

/* Host-only (no device): the WALK of the 4-node GATHER maps of the rows
 * [row_lo, row_hi) (row_hi <= 0: all rows) of a mesh of linear tetrahedra in
 * the numbering given -- the order of the chunk records in the maps and the
 * runs of consecutive records one workgroup walks, cut for ncu compute units
 * (0: 256).  Inside a run the chunks with byte-identical map words follow one
 * another (FEAHIP_GATHER_ORDER=0: row order); the runs are cut to near-equal
 * modelled cost (FEAHIP_GATHER_BALANCE=0: to equal chunk counts;
 * FEAHIP_GATHER_RUN=n: n chunks each; FEAHIP_GATHER_NRUNS=n: n runs by cost).
 * info[8] = {chunks, runs, bytes per record, first and end byte of a record's
 * map words, bytes of all records, chunks whose predecessor holds their map
 * words, modelled cycles of a launch}.  With capacity >= chunks: walk[i] =
 * the chunk (in row order) whose record is the i-th, run_start[runs + 1],
 * cost[i] = modelled cycles of record i where it stands.  With blob_capacity
 * >= info[5]: the records.  Any of the arrays may be null.  Returns the number
 * of chunks, or negative.                                                    */
int feahip_host_gather_walk(int n_nodes, int n_elems, const int *elements, int row_lo, int row_hi, int ncu,
                            long long *info, int capacity, int *walk, int *run_start, int *cost,
                            long long blob_capacity, unsigned char *blob);

/* Host-only (no device): the edges the GATHER maps of 10-node tetrahedra or
 * 8-node bricks reach, for a mesh in the numbering it is given (library ids:
 * what a context builds), under the FEAHIP_GATHER10_ROWS / _ELEMS / _ALPHA
 * settings of the environment.  out[FEAHIP_G10_SHAPE_LEN] =
 *   0 the maps built          1 when not, the limit they ran into first:
 *                               FEAHIP_G10_LIMIT_* below
 *   2 chunks                  3 largest elements of a chunk (record slots)
 *   4 largest nodes those elements touch
 *   5 largest write-out passes  6 smallest write-out passes
 *   7 longest contribution list of a block (entries, 2 per word)
 *   8 chunks with a block list longer than the words a thread keeps in
 *     registers              9 largest words per residual lane (fdw)
 *  10 blocks of the K tile   11 chunks with the most elements a record holds
 *  12 slot of the all-zero element record
 *  13 first chunk counted in 8 (-1: none)
 *  14 when the maps do not build, the row they fail at (-1 otherwise)
 *  15 largest rows of a chunk.
 * Returns FEAHIP_OK also when the maps do not build (out[0] = 0).           */
#define FEAHIP_G10_SHAPE_LEN 16
enum {
  FEAHIP_G10_LIMIT_NONE = 0, FEAHIP_G10_LIMIT_ELEMS = 1, FEAHIP_G10_LIMIT_ROW_LENGTH = 2,
  FEAHIP_G10_LIMIT_TASKS = 3, FEAHIP_G10_LIMIT_RESIDUAL_LANES = 4, FEAHIP_G10_LIMIT_LIST_LENGTH = 5,
  FEAHIP_G10_LIMIT_PASSES = 6, FEAHIP_G10_LIMIT_OTHER = 7
};
int feahip_host_gather10_shape(int n_nodes, int n_elems, int npe, const int *elements, long long *out);

/* ---- node numbering ---------------------------------------------------- */
/* The reference keeps the nodes in deck order (sexp_loader.c:170-215) and its
 * dof index is node * 3 + axis (fea_solver.c:377-384).  The kernels here own
 * runs of consecutive block rows, so feahip_create numbers the nodes itself
 * (compact cells of 4 x 4 x 4 nodes (48 half-grid nodes for 10-node elements), cells in slabs across the longest axis;
 * a mesh that sits on no lattice: recursive coordinate bisection into leaves of up to 64 nodes, the first cuts
 * across the longest axis; csrc/renumber.cpp) and works in that numbering.  Every entry of this header
 * that takes or returns node-indexed data translates: the caller passes and
 * receives its OWN node ids and dof indices, bit-exactly -- elements,
 * prescribed node ids, coordinates, forces, solution, the Yale matrix (rows,
 * columns, sorted as the caller's ids sort), SpMV vectors.  Only the shard
 * ranges (feahip_owned_rows, feahip_shard_plan, feahip_host_assembly_digest)
 * speak of library ids.  library_id_of_node[n_nodes]: library id of the
 * caller's node a (the identity when the caller's numbering was kept).       */
int feahip_node_numbering(feahip_ctx *ctx, int *library_id_of_node);
/* Host-only (no device): the numbering feahip_create would choose for this
 * mesh; returns 1 when it is a renumbering, 0 when the caller's ids are kept
 * (the identity is written then), negative on error.                         */
int feahip_host_numbering(int n_nodes, int n_elems, int npe, const int *elements,
                          const double *nodes0, int *library_id_of_node);

/* ---- reference-shaped views -------------------------------------------- */

int feahip_set_nodes(feahip_ctx *ctx, const double *nodes);   /* nodes_p    */
int feahip_get_nodes(feahip_ctx *ctx, double *nodes);         /* [N][3]     */
int feahip_get_forces(feahip_ctx *ctx, double *f);            /* [3N]       */
int feahip_set_forces(feahip_ctx *ctx, const double *f);
int feahip_get_solution(feahip_ctx *ctx, double *u);          /* [3N]       */
/* graddefs[e][g].components / stresses[e][g].components
 * (fea_solver.h:262-269), layout [E][G][3][3]                               */
int feahip_get_graddefs(feahip_ctx *ctx, double *F);
int feahip_get_stresses(feahip_ctx *ctx, double *S);
/* shape_gradients[e][g] of the CURRENT configuration (fea_solver.h:200-205,
 * filled by solver_create_current_shape_gradients, fea_solver.c:656-722,831):
 * grads[((e*G + g)*3 + i)*npe + a] = dN_a/dx_i, detj[e*G + g] = det J.      */
int feahip_get_shape_gradients(feahip_ctx *ctx, double *grads, double *detj);

/* global_mtx in sp_matrix_yale shape (fea_solver.c:303-304): scalar CSR of
 * the full symmetric pattern, sorted columns.                               */
int feahip_matrix_nnz(feahip_ctx *ctx, long long *nnz);
int feahip_get_matrix_yale(feahip_ctx *ctx, int *offsets, int *indexes,
                           double *values);
/* The same with 64-bit offsets.  feahip_get_matrix_yale REFUSES (FEAHIP_EINVAL, feahip_last_error says why) a matrix
 * of 2^31 or more scalar non-zeros instead of wrapping its int offsets: one rank of eight of BASELINE configs[4]
 * (50M 10-node tetrahedra) already holds 2.2e9.                                */
int feahip_get_matrix_yale64(feahip_ctx *ctx, long long *offsets, int *indexes,
                             double *values);
/* y = K x with host vectors (test hook for the SpMV kernel)                 */
int feahip_spmv(feahip_ctx *ctx, const double *x, double *y);
/* [y, y2] = K [x, x2] in one pass over K, host vectors [2][3N] (test hook for
 * the two-vector product of feahip_solve_slae2; refused as that solve is)    */
int feahip_spmv2(feahip_ctx *ctx, const double *x2, double *y2);

/* ---- tuning and measurement -------------------------------------------- */

int feahip_set_assembly(feahip_ctx *ctx, int strategy);
/* Preconditioner of the PCG_ILU / CHOLESKY solves: 0 = inverse 3x3 diagonal
 * blocks (default), 1 = aggregation multigrid (rigid-body modes of every
 * aggregate, W-cycle).  In a sharded solve every rank builds the hierarchy of
 * its own diagonal block and the preconditioner is block-Jacobi over the ranks
 * with a W-cycle inside each: no communication beyond the CG's own.
 * 2 = kind 1 plus one coarse level ACROSS the ranks, added to it:
 *     M2^-1 r = M1^-1 r + Phi (Phi' K Phi)^-1 Phi' r
 * with K the matrix the PCG sees.  Every rank cuts its owned rows, in its own
 * row order, into m_r = min(m, max(1, n_r / 64)) contiguous runs (aggregates;
 * m = clamp(128 / nranks, 1, 16), or the environment's FEAHIP_COARSE_AGGS, a
 * measurement knob); Phi holds the six rigid-body modes of every aggregate
 * about the mean X0 of its nodes, prescribed dofs included.  At most 128
 * aggregates, 768 coarse unknowns.  Phi' K Phi is formed and inverted in double
 * whenever K changed.  This kind DOES communicate inside the preconditioner:
 * one vector all-reduce of the coarse matrix per numeric setup, and one of at
 * most 768 doubles per CG iteration (on the communication stream, beside the
 * cycle) -- the single-reduction loop then carries two all-reduces per
 * iteration.  A solve returns FEAHIP_ESTATE, feahip_last_error naming the
 * aggregate, when Phi' K Phi has a pivot that is not positive (below 1e-12 of
 * its diagonal entry): an unconstrained body, a degenerate aggregate.  On a
 * context without a transport kind 2 is the same formula with one rank.  Set
 * the same kind on every rank.
 * Whatever the kind, the solve runs to the requested residual, so the solution
 * is the same to that tolerance.                                              */
int feahip_set_preconditioner(feahip_ctx *ctx, int kind);
/* z = M^-1 r with the preconditioner a PCG solve (feahip_solve_slae with
 * PCG_ILU) would use now, for the current K: kind 0 the 3x3 block-Jacobi,
 * kind 1 one multigrid W-cycle, prepared as the solve prepares it.  r and z
 * are [N][3] in the caller's node ids.  On a sharded context z covers the
 * rank's rows and is 0 elsewhere.  FEAHIP_ESTATE before the first stiffness
 * assembly.  Touches only scratch that a solve overwrites at its start.  A
 * solve's multigrid cycles (and this) return FEAHIP_EHIP if the tail kernel
 * of the small levels fails to launch.
 * Under kind 2 on a context with an RCCL transport (feahip_comm_init) this
 * call is COLLECTIVE: every rank makes it, each with its own r.  A member of
 * an in-process group is refused (FEAHIP_ESTATE): one call cannot stand for
 * all ranks there, feahip_group_apply_preconditioner does.                   */
int feahip_apply_preconditioner(feahip_ctx *ctx, const double *r, double *z);
/* The coarse level of preconditioner 2 as the next solve would use it, prepared
 * here for the current K (collective like a solve: all ranks of an RCCL run
 * call it; an in-process group is prepared as a whole from any member).
 * out8: 0 aggregates over all ranks, 1 this rank's first global aggregate id,
 * 2 its aggregates, 3 coarse unknowns (6 per aggregate), 4 numeric epoch (the
 * number of numeric setups so far: it advances only when K changed), 5 owned
 * rows, 6 the cap m, 7 (row aggregate, column aggregate) pairs of its rows.
 * With non-null arrays (sized by a first call): agg_of_owned_row[owned rows]
 * the global aggregate of every owned row in the context's row order (library
 * ids [row0, row1); local ids [0, n_own) of a rank context), and
 * centroids[aggregates][3] of ALL aggregates.  FEAHIP_ESTATE unless kind 2 is
 * set (on every rank) and K was assembled.                                   */
int feahip_coarse_info(feahip_ctx *ctx, long long *out8, int *agg_of_owned_row, double *centroids);
/* A[n][n], n = out8[3]: the all-reduced Phi' K Phi, row-major, unknown 6 A + k
 * = mode k of aggregate A (k < 3 translation, else rotation about axis k - 3). */
int feahip_coarse_matrix(feahip_ctx *ctx, double *A);
/* Host-only (no device): the cut rule.  Returns m_r = min(m, max(1, n_owned / 64))
 * (negative on a bad argument) and, when non-null, first_row_of_aggregate[m_r + 1]
 * = floor(j n_owned / m_r): aggregate j is the owned rows [first[j], first[j + 1]),
 * counted from the rank's first owned row.                                    */
int feahip_host_coarse_aggregates(int n_owned, int m, int *first_row_of_aggregate);
/* Read-only view of the multigrid hierarchy (preconditioner 1 or 2) for the
 * current K; prepared here if K changed since the last solve.
 * out16: 0 levels, 1 gamma, 2 gamma_from, 3 gamma_until, 4 coarse_sweeps,
 * 5 fine_bits (level-0 smoother matrix: 16 bfloat16, 32 float, 64 K),
 * 6 coarse matrices in float, 7 fused post-smoothing, 8 tail_from (first
 * level of the one-workgroup tail, -1 none), 9 the tail's entry-level
 * product (0 no tail, 1 matrix in LDS, 2 lane-major ELL copy, 3 CSR from L2),
 * 10 the coarsest level as one dense operator, 11 bit l set: level l's
 * matrix sits in the tail's LDS, 12/13 the rank's rows [row0, row1) in
 * library ids, 14 the tail's packed blob in use.  *over: the over-correction.
 * FEAHIP_ESTATE unless preconditioner 1 or 2 is set and K was assembled.     */
int feahip_amg_info(feahip_ctx *ctx, long long *out16, double *over);
/* One level.  counts[4]: N block rows, nnzb blocks, Nc block rows of the
 * next level (0 on the coarsest), bits of the stored matrix (level 0: the
 * smoother's copy; below: 32 or 64).  *omega: the level's Jacobi damping.
 * With rowptr..type null only counts and omega are written (sizing call);
 * otherwise rowptr[N+1], colidx[nnzb], K[nnzb][3][3] (the matrix as stored,
 * widened to double), agg[N], doff[N][3], type[N] (0 translation row,
 * 1 rotation row).  agg / doff map to the next level (-1 / 0 on the
 * coarsest).  Level 0 speaks the caller's node ids, its blocks ordered as
 * feahip_get_matrix_yale orders them, and only the rank's rows carry values
 * (agg = -1 elsewhere).  Coarse levels speak the library's own aggregate ids:
 * aggregate A of level l is block rows 2A (translation) and 2A+1 (rotation)
 * of level l+1.                                                              */
int feahip_amg_level(feahip_ctx *ctx, int level, long long *counts, double *omega, int *rowptr, int *colidx,
                     double *K, int *agg, double *doff, int *type);
/* The CG / PCG loop of feahip_solve_slae.  0: the textbook loop (what the
 * reference's sp_matrix_yale_solve_cg / _pcg_ilu run, fea_solver.c:245-280):
 * two reductions per iteration (p.Kp, then r.z and r.r), halo rows exchanged
 * before the product.  1: the single-reduction form of the same recurrence
 * (Chronopoulos / Gear): p = z + beta p and s = w + beta s with w = K z kept
 * by recurrence, so that r.z, w.z and r.r of an iteration are summed together
 * -- ONE all-reduce of three doubles per iteration -- and the halo rows of z
 * travel while the rows that touch no halo column are multiplied.  Same
 * iterates in exact arithmetic; the solve runs to the same residual.  -1
 * (default): 1 for a sharded context, 0 otherwise.                            */
int feahip_set_pcg_variant(feahip_ctx *ctx, int variant);
/* Line search along every Newton step of feahip_solve / feahip_group_solve:
 * golden-section search, `max_iterations` iterations, for the step length in
 * [1/2, 1] that minimises |eta <u, R(x + eta u)>| -- what the reference's
 * prototype does (solver-prototype/cartesian3d/large/cartesian3d_large.m:
 * 85-119) and what its C solver parses as `line-search :max` and leaves unused
 * (fea_solver.c:1517, sexp_loader.c:153-159).  0 (default) = the reference's
 * solve().  Two residual assemblies per iteration.                         */
int feahip_set_line_search(feahip_ctx *ctx, int max_iterations);
/* Restricts assembly and SpMV to this rank's slab of block rows (rank of
 * nranks, contiguous row ranges of near-equal block count).  Rows are owned
 * by exactly one rank; a rank visits every element that touches its rows, so
 * assembly needs no exchange between ranks.                                  */
int feahip_set_row_shard(feahip_ctx *ctx, int rank, int nranks);
int feahip_sync(feahip_ctx *ctx);
/* Runs `iters` timed launches of one hot-path kernel after `warmup` untimed
 * ones, bracketed by HIP events on the context's own stream; *avg_ms is the
 * mean device time of one launch.  what: 0 stiffness+residual assembly,
 * 1 stiffness only, 2 residual only, 3 SpMV, 4 one PCG iteration, 5 the
 * surface-load kernels alone (refused on a context without loaded faces),
 * 6 the two-vector SpMV, 7 one two-column PCG iteration (feahip_solve_slae2;
 * both refused where that solve is), 8 K += M (k_mass_add), 9 the inertia
 * term of the residual (k_mass_residual; 8 and 9 refused without a mass),
 * 10 the two pointwise kernels of an explicit step together (they advance v
 * and a by a step of dt = 1 on the f in force), 11 k_gershgorin on the K in
 * force (10 and 11 refused without a mass), 12 the two result passes together
 * (k_result_elements, k_result_nodes) with all outputs and material = -1,
 * 13 k_spmm_km (K X and M X of eight columns in one pass), 14 k_modal_gram (both
 * 24 x 24 Gram matrices from the nine block vectors), 15 k_modal_combine (the
 * nine block vectors recombined in place), 16 k_modal_deflate_gram and 17
 * k_modal_deflate_apply (one block vector against eight panels of the locked
 * store filled with the hash; with zero coefficients, so nothing moves); 13-17
 * refused without a mass and where feahip_solve_modes is; 18 k_geom_elements
 * and 19 k_geom_blocks, the two passes of the geometric stiffness at the
 * current nodes (refused where feahip_solve_buckling is; no mass needed);
 * 20 k_contact alone, K and f (refused on a context without contact; it adds
 * K_c and F_c into the K and f in force on every launch: both are garbage
 * afterwards, assemble again); 21 k_damp_add (K += M + K_d, refused without a
 * damping with beta_k > 0) and 22 k_damp_residual on the vectors in force with
 * a0 = c1 = 1 (refused without damping; both need a mass and leave K or f
 * garbage as 8 and 9 do); 23 k_response_sweep over the coefficient table, the
 * store and the u_s the last feahip_response_sweep used, 24 k_response_project
 * on the f in force (both FEAHIP_ESTATE before a sweep; nothing but the sweep's
 * own output buffers and partial sums is written); 25 one launch of
 * k_transient_sweep over the last chunk of the last feahip_response_transient
 * (FEAHIP_ESTATE, "no transient", before one); 26 k_response_combine over the
 * form of the last feahip_response_combine, _random or _spectrum
 * (FEAHIP_ESTATE, "no form", before one); 27 k_mstress_elements and
 * k_mstress_nodes over every panel of the locked store in use at the current
 * nodes, into the scratch panel of the single-vector path: the stress store in
 * force is needed (FEAHIP_ESTATE without one) and is not written; 28 k_stress_combine over the form
 * of the last feahip_response_stress_combine, _random or _spectrum
 * (FEAHIP_ESTATE, "no stress form", before one); 29 k_stress_sweep over the
 * table of the last feahip_response_stress_sweep and 30 one launch of
 * k_stress_transient over the last chunk of the last
 * feahip_response_stress_transient, as a first and last launch (FEAHIP_ESTATE,
 * "no stress sweep" / "no stress transient", before one; only the peak buffers
 * of the stress entries are written); 31 k_stress_moments over the four forms
 * of the last feahip_response_stress_moments or _fatigue and 32 k_fatigue_rates
 * over the last moments and the S-N curve of the last
 * feahip_response_stress_fatigue (FEAHIP_ESTATE, "no stress moments" / "no
 * fatigue rates", before one; only the buffers of the fatigue entries are
 * written); 33 one launch of k_stress_rainflow over the last chunk of the last
 * feahip_response_stress_rainflow, the component pass as a first and last
 * launch (FEAHIP_ESTATE, "no stress rainflow", before one or after a new
 * filling of the store; only the buffers of that entry are written).         */
int feahip_time_kernel(feahip_ctx *ctx, int what, int warmup, int iters,
                       double *avg_ms);
/* Streaming copy of `bytes` bytes (16 bytes per lane, read + written counted)
 * on the context's device and stream: the copy bandwidth of this box, to quote
 * roofline fractions against next to the data-sheet peak.     */
int feahip_copy_bandwidth(feahip_ctx *ctx, long long bytes, double *gbytes_per_s);
/* The same measured four ways (the call above reports the best): out4[0] one
 * 16-byte load in flight per lane (grid-stride), out4[1] four independent
 * 16-byte loads in flight per lane, out4[2] hipMemcpyDtoDAsync, out4[3] as
 * [1] with non-temporal loads and stores.                                   */
int feahip_copy_bandwidth_detail(feahip_ctx *ctx, long long bytes, double *out4);
/* device addresses of K, the column indices and the two SpMV vectors (for
 * the alignment column of a bandwidth report): out4                         */
int feahip_device_layout(feahip_ctx *ctx, long long *out4);
/* sizes the roofline model needs: N, E, npe, G, block rows, blocks, and the
 * bytes of the auxiliary maps the kernels read                              */
int feahip_sizes(feahip_ctx *ctx, long long *out8);
/* What the gather strategy's maps look like on this mesh (built on first use; zeros when another strategy runs):
 * out4[0] element evaluations per element the rank touches (1.75 for a 4x4x4 brick of a Kuhn block), out4[1] gather
 * chunks, out4[2] chunks whose map words equal their predecessor's (kept in registers by the kernel), out4[3] map
 * bytes.  For reports (bench.py extras); reference has no counterpart.                                                  */
int feahip_assembly_stats(feahip_ctx *ctx, double *out4);
/* the strategy (FEAHIP_ASM_*) the most recent assembly launch ran -- what
 * FEAHIP_ASM_AUTO resolved to on this mesh; FEAHIP_ASM_AUTO before any launch */
int feahip_assembly_in_use(feahip_ctx *ctx, int *strategy);

#ifdef __cplusplus
}
#endif
#endif
