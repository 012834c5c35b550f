// kernels_buckling.hip -- linear buckling on gfx950: the geometric stiffness K_sigma as a matrix of its own, and the lowest
// eigenpairs of K_sigma phi = nu K phi on the free dofs (feahip_solve_buckling).
//
// The geometric part of a 3x3 block of the element stiffness is (g_a . sigma g_b) vol times the identity (fem_device.h:
// the term d_ij (c . g_b) without its m1 share), so K_sigma fits the storage of the consistent mass: ONE double per block
// of K's block-CSR pattern,
//   kg[q] = sum_{e holds a and b} sum_g vol_eg (g_a . sigma_eg g_b),      q = (a, b),
// at the CURRENT nodes over the stiffness rule, with the element's own (lambda, mu) under a material table.  It is
// assembled by two kernels modelled on k_mass_elements / k_mass_blocks and k_result_elements, without atomics and in a
// fixed summation order, so every call gives the same bits:
//
//   k_geom_elements  one thread per element: load_element + gp_state over the Gauss points, the element's symmetric
//                    npe x npe scalar matrix G_e[la][lb] = sum_g vol (g_la . sigma g_lb), its UPPER TRIANGLE only (10,
//                    36, 55 doubles for TET4, HEX8, TET10), element-major: rec[e T + tri(la, lb)].
//                    Why this layout: the block pass knows (e, la, lb) of a hit and wants one 8-byte load for it -- the
//                    triangle index is two integer operations, and both (a, b) and (b, a) read the SAME double, so kg is
//                    symmetric to the bit.  Element-major (and not entry-major [T][E]) because the lanes of a wave work
//                    on the blocks of a few neighbouring rows: the hits of one row fall into the same elements, so their
//                    loads share the 80 to 440 bytes of a record (one to seven cache lines) instead of touching one line
//                    per entry; the element pass pays for it with stores T doubles apart, once per solve.
//   k_geom_blocks    one lane per owned block: k_mass_blocks' walk of the chunk's (element, local node) visits in stored
//                    order, adding rec[e T + tri(la, lb)] for the elements that hold both nodes.  A row of any length
//                    works: the lanes stride over the blocks of the chunk.
//
// The driver (buckling_solve) is modal_solve's blocked LOBPCG on the pencil (K_sigma, K): it launches kernels_modal.hip's
// kernels, unchanged, with the two products of k_spmm_km swapped -- y = K X goes to the "M" slots of ModalState::d_v,
// z = mask(kg X) to the "K" slots -- so the Gram pass returns S' K S as "G_M" and S' K_sigma S as "G_K", modal_ritz
// returns nu ascending with X K-orthonormal, and k_modal_residual forms K_sigma X - nu K X and applies the
// preconditioner of K, which is the natural one for this pencil.
//
// Nothing here is allocated or launched on a context that never calls feahip_solve_buckling, feahip_geometric_spmv or
// feahip_time_kernel 18-19.
#include "feahip_internal.h"
#include "fem_device.h"
#include <cmath>

#define MC FEA_MODAL_COLS

// multigrid preconditioner (amg.hip)
int amg_prepare(feahip_ctx *c);

// position of (la, lb), la <= lb, in the row-major upper triangle of an npe x npe matrix
__host__ __device__ __forceinline__ int geom_tri(int npe, int la, int lb) { return la * npe - (la * (la - 1)) / 2 + (lb - la); }

template <int NPE, bool LINTET, bool HET>
__global__ __launch_bounds__(256)
void k_geom_elements(AsmArgs A, double *__restrict__ rec)
{
  constexpr int T = NPE * (NPE + 1) / 2;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= A.E) return;
  int nd[NPE];
  double xe[NPE][3], Xe[NPE][3];
  load_element<NPE>(A, e, nd, xe, Xe);
  const double2 lm = elem_material<HET>(A, e);
  double G[T];
#pragma unroll
  for (int k = 0; k < T; ++k) G[k] = 0.0;
  for (int gp = 0; gp < A.G; ++gp) {
    GPState<NPE> s;
    gp_state<NPE, LINTET>(xe, Xe, A.tab, gp, A.model, lm.x, lm.y, s);
#pragma unroll
    for (int b = 0; b < NPE; ++b) {
      double t[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = s.vol * (s.sig[i][0] * s.g[b][0] + s.sig[i][1] * s.g[b][1] + s.sig[i][2] * s.g[b][2]);
#pragma unroll
      for (int a = 0; a <= b; ++a) G[geom_tri(NPE, a, b)] += s.g[a][0] * t[0] + s.g[a][1] * t[1] + s.g[a][2] * t[2];
    }
  }
  double *o = rec + (size_t)e * T;
#pragma unroll
  for (int k = 0; k < T; ++k) o[k] = G[k];
}

// One wave per chunk of owned rows; lane k takes the blocks k, k + 64, ... of the chunk (k_mass_blocks).  For its block
// (a, b) the lane walks the chunk's visits in stored order, keeps those of row a whose element also holds b, and adds the
// one double of the element's record that belongs to the pair.
__global__ __launch_bounds__(64 * FEA_WAVES_PER_WG)
void k_geom_blocks(int chunk0, int nchunks, const int *__restrict__ chunk, const int *__restrict__ rowptr,
                   const int *__restrict__ colidx, const int *__restrict__ incptr, const uint32_t *__restrict__ inc,
                   const int *__restrict__ conn, int npe, const double *__restrict__ rec, double *__restrict__ kg)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int T = npe * (npe + 1) / 2;
  for (int ch = chunk0 + blockIdx.x * FEA_WAVES_PER_WG + wave; ch < chunk0 + nchunks; ch += gridDim.x * FEA_WAVES_PER_WG) {
    const int r0 = chunk[ch], r1 = chunk[ch + 1];
    const int b0 = rowptr[r0], b1 = rowptr[r1];
    const int p0 = incptr[r0], p1 = incptr[r1];
    for (int q = b0 + lane; q < b1; q += 64) {
      int a = r0;
      while (a + 1 < r1 && rowptr[a + 1] <= q) ++a;
      const int b = colidx[q];
      double acc = 0.0;
      for (int p = p0; p < p1; ++p) {
        const uint32_t w = inc[p];
        const int e = (int)(w & 0x0FFFFFFFu), la = (int)(w >> 28);
        const int *nd = conn + (size_t)e * npe;
        if (nd[la] != a) continue;
        int lb = -1;
        for (int k = 0; k < npe; ++k) lb = (nd[k] == b) ? k : lb;
        if (lb < 0) continue;
        acc += rec[(size_t)e * T + (la <= lb ? geom_tri(npe, la, lb) : geom_tri(npe, lb, la))];
      }
      kg[q] = acc;
    }
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------
static int geom_grid(const feahip_ctx *c)
{
  const int g = (c->nchunks_local + FEA_WAVES_PER_WG - 1) / FEA_WAVES_PER_WG;
  return g < FEA_RED_BLOCKS ? (g > 0 ? g : 1) : FEA_RED_BLOCKS;
}

static int geom_ensure(feahip_ctx *c)
{
  BucklingState &B = c->buckling;
  int rc;
  if ((rc = ensure_generic_maps(c))) return rc;
  if (!B.d_rec) FEA_HIP_CHECK(c, hipMalloc((void **)&B.d_rec, sizeof(double) * (size_t)c->E * (c->npe * (c->npe + 1) / 2)));
  if (!B.d_kg_base || B.kb0 != c->kb0 || B.kb1 != c->kb1) {
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    dev_free({B.d_kg_base});
    B.d_kg_base = B.d_kg = nullptr; B.kb0 = B.kb1 = -1;
    const size_t nb = (size_t)(c->kb1 - c->kb0);
    FEA_HIP_CHECK(c, hipMalloc((void **)&B.d_kg_base, sizeof(double) * (nb ? nb : 1)));
    B.d_kg = B.d_kg_base - c->kb0; B.kb0 = c->kb0; B.kb1 = c->kb1;
  }
  return FEAHIP_OK;
}

static int enq_geom_elements(feahip_ctx *c)
{
  AsmArgs A = AsmArgs();
  A.N = c->N; A.E = c->E; A.G = c->G; A.model = c->model;
  A.lambda = c->lambda; A.mu = c->mu; A.mat = c->d_mat; A.emat = c->d_elem_mat;
  A.tab = c->d_table; A.conn = c->d_conn; A.X0 = c->d_X0; A.x = c->d_x;
  const int grid = (c->E + 255) / 256;
  double *rec = c->buckling.d_rec;
  auto launch = [&](auto H) {
    if (c->npe == 4) {
      if (c->linear_tet) hipLaunchKernelGGL((k_geom_elements<4, true, H>), dim3(grid), dim3(256), 0, c->stream, A, rec);
      else hipLaunchKernelGGL((k_geom_elements<4, false, H>), dim3(grid), dim3(256), 0, c->stream, A, rec);
    } else if (c->npe == 8)
      hipLaunchKernelGGL((k_geom_elements<8, false, H>), dim3(grid), dim3(256), 0, c->stream, A, rec);
    else
      hipLaunchKernelGGL((k_geom_elements<10, false, H>), dim3(grid), dim3(256), 0, c->stream, A, rec);
  };
  if (c->n_materials) launch(std::true_type()); else launch(std::false_type());
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

static int enq_geom_blocks(feahip_ctx *c)
{
  hipLaunchKernelGGL(k_geom_blocks, dim3(geom_grid(c)), dim3(64 * FEA_WAVES_PER_WG), 0, c->stream, c->chunk0, c->nchunks_local,
                     c->d_chunk, c->d_rowptr, c->d_colidx, c->generic.d_incptr, c->generic.d_inc, c->d_conn, c->npe,
                     (const double *)c->buckling.d_rec, c->buckling.d_kg);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// kg for the rows of the shard installed now (K exists), at the current nodes and the material table in force
int geom_assemble(feahip_ctx *c)
{
  int rc;
  if ((rc = geom_ensure(c)) || (rc = enq_geom_elements(c))) return rc;
  return enq_geom_blocks(c);
}

// hooks of feahip_time_kernel 18 and 19 (geom_assemble has run once: the records the block pass reads are there)
int time_geom_kernel(feahip_ctx *c, int what) { return what == 18 ? enq_geom_elements(c) : enq_geom_blocks(c); }

// ---- the driver ------------------------------------------------------------------------------------------------------
// The shared iteration (struct Lobpcg) on the pencil (K_sigma, K): kg stands beside K in the product and the two results
// swap slots (Lobpcg::geometric).  The slots of ModalState::d_v keep their names, and hold
//   V_KX, V_KW, V_KP: mask(K_sigma S)        V_MX, V_MW, V_MP: K S
// (K is masked and S is zero on the prescribed dofs, so K S is zero there too), so the stop test is
// ||K_sigma x - nu K x|| <= tol (||K_sigma x|| + |nu| ||K x||).
int buckling_solve(feahip_ctx *c, int n_modes, double tol, int max_it, double *nu, double *resid, int *iters)
{
  int rc;
  if ((rc = ensure_modal(c))) return rc;
  ModalState &S = c->modal;
  S.have = false;                                                     // modes of either modal solve are dropped
  S.have_locked = false;
  if (S.n_free < 3 * MC) {
    c->err = "solve_buckling: " + std::to_string(S.n_free) + " free dofs, fewer than the 24 the block of eight columns needs";
    return FEAHIP_EINVAL;
  }
  // K(x), masked as the PCG sees it (K and f are another matrix from here on: k_epoch), and K_sigma(x) beside it
  if ((rc = feahip_create_stiffness(c)) || (rc = feahip_apply_prescribed_bc(c, 0.0)) || (rc = geom_assemble(c))) return rc;
  if (c->precond == 1) { if ((rc = amg_prepare(c))) return rc; }
  else enq_precond_blockjacobi(c);
  Lobpcg L({c}, nullptr, tol);
  L.geometric = true;
  // every 20 steps the products of X AND of P are made again.  modal_solve renews X's alone; on this pencil the products
  // of P, carried by recurrence from the first step on, made the step count erratic (a float64 emulation of the
  // clamped-free column: 322 to 1326 steps over four start blocks without the second product, 324 to 349 with it;
  // tests/buckling_reference.py emulates this step)
  L.renew_p = true;
  bool not_pd = false;                                // x_j' K x_j <= 0 for a column of the block: K is not positive definite
  L.veto = [&](int ns, const double *GM) {
    bool finite = true;
    for (int j = 0; j < MC; ++j) finite = finite && std::isfinite(GM[j * ns + j]);
    for (int j = 0; finite && j < MC; ++j) if (!(GM[j * ns + j] > 0.0)) not_pd = true;
    return not_pd;
  };
  int it = 0;
  if ((rc = launch_modal_hash(c, c->modal.d_v))) return rc;             // X, the first of the nine block vectors
  const int end = L.run(n_modes, max_it, &it);
  if (end < 0) return end;
  if (end == LOBPCG_BROKE) {
    c->err = not_pd ? "solve_buckling: K is not positive definite at this state (x' K x <= 0 for a column of the block): "
                      "most likely a critical point has been passed"
                    : "solve_buckling: the Rayleigh-Ritz basis lost its rank or a sum is not finite";
    return FEAHIP_ENOTCONVERGED;
  }
  S.have_buckling = true;
  for (int j = 0; j < n_modes; ++j) { nu[j] = L.theta[j]; if (resid) resid[j] = L.ratio[j]; }
  if (iters) *iters = it;
  if (end == LOBPCG_OUT_OF_STEPS) {
    c->err = "solve_buckling: not converged after " + std::to_string(it) + " Rayleigh-Ritz steps";
    return FEAHIP_ENOTCONVERGED;
  }
  return FEAHIP_OK;
}
