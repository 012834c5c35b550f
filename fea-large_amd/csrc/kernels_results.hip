// kernels_results.hip -- result recovery on gfx950: nodal stress, von Mises stress, strain energy, reactions.
//
// Two passes, modelled on k_mass_elements / k_mass_lump, run by every call of a results entry (nothing is cached: a
// result is always that of the nodes and the material table in force).  Nothing here is allocated or launched on a
// context that never calls one of them.
//
//   k_result_elements  one thread per element (its own and the ghosts of a rank): load_element + gp_state over the
//                      stiffness rule, ONE 64-byte record per element,
//                        { sum_g vol sigma (xx yy zz xy yz xz), sum_g vol, W_e },
//                      vol = w_g |det J_g| of the current configuration, W_e = sum_g w_g det J0_g Psi(F_g) with
//                      det J0 = det J / det F and Psi the potential of the model's stress (fd_constitutive):
//                        Neo-Hookean  Psi = mu/2 (tr b - 3) - mu ln J + lambda/2 (ln J)^2
//                        A5           Psi = lambda/2 (tr E)^2 + mu E:E,  E = (F'F - I)/2
//   k_result_nodes     one wave per chunk of owned rows, lane = (row, quarter of the record): 16 rows x 4 lanes.  The
//                      visits of a chunk are stored round-robin over its rows (pattern.cpp), so visit k of row r sits
//                      at  first visit of the chunk + sum_r' min(len r', k) + #{r' < r : len r' > k}:  the wave keeps
//                      the running base and finds the last term by a ballot over the row-leader lanes and a popcount
//                      of the lower ones.  Four rounds are taken at a time so that their loads are in flight together.
//                      Each lane loads 16 bytes of the record and carries two of the eight sums in visit order --
//                      no atomics, a fixed order, the same bits on every call.  sigma_a = sum / weight,
//                      von Mises of that average, w_node = sum W_e / npe; the nodal shares of the owned rows are summed
//                      by block_sum / k_reduce_final into the strain energy.
//
// The selection by material is an argument of the NODE pass (one byte of d_elem_mat per visit, read only when a
// material is selected): the element records do not depend on it.
//
// Reactions: the residual is assembled by the ordinary assembly into d_f, which is saved before and restored after with
// device copies, so the assembly kernels stay as they are and K, f, u, x, the cached state and k_epoch are untouched.
#include "feahip_internal.h"
#include "fem_device.h"
#include "reduce_device.h"

typedef double res_v2d __attribute__((ext_vector_type(2)));

template <int NPE, bool LINTET, bool HET>
__global__ __launch_bounds__(256)
void k_result_elements(AsmArgs A, res_v2d *__restrict__ rec)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= A.E) return;
  int nd[NPE];
  double xe[NPE][3], Xe[NPE][3];
  load_element<NPE>(A, e, nd, xe, Xe);
  const double2 lm = elem_material<HET>(A, e);
  double s6[6] = {0, 0, 0, 0, 0, 0}, vol = 0.0, W = 0.0;
  for (int gp = 0; gp < A.G; ++gp) {
    GPState<NPE> s;
    gp_state<NPE, LINTET>(xe, Xe, A.tab, gp, A.model, lm.x, lm.y, s);
    s6[0] += s.vol * s.sig[0][0]; s6[1] += s.vol * s.sig[1][1]; s6[2] += s.vol * s.sig[2][2];
    s6[3] += s.vol * s.sig[0][1]; s6[4] += s.vol * s.sig[1][2]; s6[5] += s.vol * s.sig[0][2];
    vol += s.vol;
    const double Jd = fd_det3(s.F);
    double psi;
    if (A.model == FEAHIP_MODEL_COMPRESSIBLE_NEOHOOKEAN) {
      double trb = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) trb += s.F[i][j] * s.F[i][j];
      const double lnJ = log(Jd);                       // det F <= 0: NaN, and it propagates
      psi = 0.5 * lm.y * (trb - 3.0) - lm.y * lnJ + 0.5 * lm.x * lnJ * lnJ;
    } else {
      double trE = 0.0, EE = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double Eij = 0.5 * (s.F[0][i] * s.F[0][j] + s.F[1][i] * s.F[1][j] + s.F[2][i] * s.F[2][j] - ((i == j) ? 1.0 : 0.0));
          EE += Eij * Eij;
          if (i == j) trE += Eij;
        }
      psi = 0.5 * lm.x * trE * trE + lm.y * EE;
    }
    W += A.tab->w[gp] * (s.detJ / Jd) * psi;
  }
  res_v2d *o = rec + (size_t)e * 4;
  res_v2d r0, r1, r2, r3;
  r0.x = s6[0]; r0.y = s6[1]; r1.x = s6[2]; r1.y = s6[3]; r2.x = s6[4]; r2.y = s6[5]; r3.x = vol; r3.y = W;
  o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
}

// See the file header.  Quarter q of a row carries: 0 (xx, yy), 1 (zz, xy), 2 (yz, xz), 3 (weight, W).
__global__ __launch_bounds__(64 * FEA_WAVES_PER_WG)
void k_result_nodes(int chunk0, int nchunks, const int *__restrict__ chunk, const int *__restrict__ incptr,
                    const uint32_t *__restrict__ inc, const res_v2d *__restrict__ rec, const uint8_t *__restrict__ emat,
                    int material, double inv_npe, res_v2d *__restrict__ sig6, double *__restrict__ vm,
                    double *__restrict__ wt, double *__restrict__ wn, double *__restrict__ part)
{
  static_assert(FEA_CHUNK_ROWS * 4 <= 64, "four lanes per row of a chunk");
  static_assert(FEA_WAVES_PER_WG == 4, "block_sum adds four waves");
  __shared__ double sh[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row = lane >> 2, q = lane & 3;
  const unsigned long long below = (1ull << (row * 4)) - 1ull;   // the leader lanes of the rows before this one
  double wsum = 0.0;
  for (int ch = chunk0 + blockIdx.x * FEA_WAVES_PER_WG + wave; ch < chunk0 + nchunks; ch += gridDim.x * FEA_WAVES_PER_WG) {
    const int r0 = chunk[ch], r1 = chunk[ch + 1];
    const int a = r0 + row;
    const bool live = a < r1;
    const int len = live ? incptr[a + 1] - incptr[a] : 0;
    int base = incptr[r0];                             // position of the first visit of round k
    res_v2d acc;
    acc.x = 0.0; acc.y = 0.0;
    // four rounds at a time: their incidence words, then their records, are independent loads in flight together; the
    // sums still take the visits in stored order
    for (int k = 0;; k += 4) {
      bool act[4];
      int pos[4];
      int nxt = base;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        act[j] = k + j < len;
        const unsigned long long lead = __ballot(act[j] && q == 0);
        pos[j] = nxt + __popcll(lead & below);
        nxt += __popcll(lead);
      }
      if (nxt == base) break;                          // no row has a visit left
      base = nxt;
      int e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = act[j] ? (int)(inc[pos[j]] & 0x0FFFFFFFu) : -1;
      if (material >= 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = (e[j] >= 0 && (int)emat[e[j]] == material) ? e[j] : -1;
      }
      res_v2d r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) if (e[j] >= 0) r[j] = rec[(size_t)e[j] * 4 + q];
#pragma unroll
      for (int j = 0; j < 4; ++j) if (e[j] >= 0) acc += r[j];
    }
    const int l0 = row * 4;
    const double wgt = __shfl(acc.x, l0 + 3, 64);
    const double inv = wgt != 0.0 ? 1.0 / wgt : 0.0;    // no selected element at this node: stress 0, weight 0
    res_v2d s = acc * inv;
    const double sxx = __shfl(s.x, l0, 64), syy = __shfl(s.y, l0, 64), szz = __shfl(s.x, l0 + 1, 64);
    const double sxy = __shfl(s.y, l0 + 1, 64), syz = __shfl(s.x, l0 + 2, 64), sxz = __shfl(s.y, l0 + 2, 64);
    if (live) {
      if (q < 3) sig6[(size_t)a * 3 + q] = s;
      else {
        const double p = (sxx + syy + szz) * (1.0 / 3.0);
        const double dx = sxx - p, dy = syy - p, dz = szz - p;
        vm[a] = sqrt(1.5 * (dx * dx + dy * dy + dz * dz + 2.0 * (sxy * sxy + syz * syz + sxz * sxz)));
        wt[a] = wgt;
        const double w = acc.y * inv_npe;
        wn[a] = w;
        wsum += w;
      }
    }
  }
  wsum = block_sum(wsum, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = wsum;
}

// r = -f on the prescribed dofs of [i0, i1) (r is zero elsewhere)
__global__ __launch_bounds__(256)
void k_reactions(int i0, int i1, const uint8_t *__restrict__ mask, const double *__restrict__ f, double *__restrict__ r)
{
  const int i = i0 + blockIdx.x * 256 + threadIdx.x;
  if (i < i1 && mask[i]) r[i] = -f[i];
}

// ---- launchers ---------------------------------------------------------------------------------------------------
static int result_grid(const feahip_ctx *c)
{
  const int g = (c->nchunks_local + FEA_WAVES_PER_WG - 1) / FEA_WAVES_PER_WG;
  return g < FEA_RED_BLOCKS ? (g > 0 ? g : 1) : FEA_RED_BLOCKS;
}

int results_ensure(feahip_ctx *c)
{
  ResultState &R = c->results;
  int rc;
  if ((rc = ensure_generic_maps(c))) return rc;
  if (R.d_rec) return FEAHIP_OK;
  const size_t N = (size_t)c->N;
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_rec, sizeof(double) * 8 * (size_t)c->E));
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_sig6, sizeof(double) * 6 * N));
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_vm, sizeof(double) * N));
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_wt, sizeof(double) * N));
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_wn, sizeof(double) * N));
  FEA_HIP_CHECK(c, hipMalloc((void **)&R.d_part, sizeof(double) * FEA_RED_BLOCKS));
  return FEAHIP_OK;
}

// both passes at the current nodes: the nodal outputs of the owned rows (zero elsewhere) into c->results, and where
// d_energy is not null the sum of the owned nodal energy shares into *d_energy
int launch_results(feahip_ctx *c, int material, double *d_energy)
{
  int rc;
  if ((rc = results_ensure(c))) return rc;
  ResultState &R = c->results;
  AsmArgs A = AsmArgs();
  A.N = c->N; A.E = c->E; A.G = c->G; A.model = c->model;
  A.lambda = c->lambda; A.mu = c->mu; A.mat = c->d_mat; A.emat = c->d_elem_mat;
  A.tab = c->d_table; A.conn = c->d_conn; A.X0 = c->d_X0; A.x = c->d_x;
  const int grid = (c->E + 255) / 256;
  res_v2d *rec = (res_v2d *)R.d_rec;
  auto launch = [&](auto H) {
    if (c->npe == 4) {
      if (c->linear_tet) hipLaunchKernelGGL((k_result_elements<4, true, H>), dim3(grid), dim3(256), 0, c->stream, A, rec);
      else hipLaunchKernelGGL((k_result_elements<4, false, H>), dim3(grid), dim3(256), 0, c->stream, A, rec);
    } else if (c->npe == 8)
      hipLaunchKernelGGL((k_result_elements<8, false, H>), dim3(grid), dim3(256), 0, c->stream, A, rec);
    else
      hipLaunchKernelGGL((k_result_elements<10, false, H>), dim3(grid), dim3(256), 0, c->stream, A, rec);
  };
  if (c->n_materials) launch(std::true_type()); else launch(std::false_type());
  FEA_HIP_CHECK(c, hipGetLastError());
  const size_t N = (size_t)c->N;
  if (c->row0 > 0 || c->row1 < c->N) {                 // the rows of other ranks read as zero
    FEA_HIP_CHECK(c, hipMemsetAsync(R.d_sig6, 0, sizeof(double) * 6 * N, c->stream));
    FEA_HIP_CHECK(c, hipMemsetAsync(R.d_vm, 0, sizeof(double) * N, c->stream));
    FEA_HIP_CHECK(c, hipMemsetAsync(R.d_wt, 0, sizeof(double) * N, c->stream));
    FEA_HIP_CHECK(c, hipMemsetAsync(R.d_wn, 0, sizeof(double) * N, c->stream));
  }
  const int g = result_grid(c);
  hipLaunchKernelGGL(k_result_nodes, dim3(g), dim3(64 * FEA_WAVES_PER_WG), 0, c->stream, c->chunk0, c->nchunks_local, c->d_chunk,
                     c->generic.d_incptr, c->generic.d_inc, (const res_v2d *)rec, (const uint8_t *)c->d_elem_mat,
                     c->n_materials ? material : -1, 1.0 / c->npe, (res_v2d *)R.d_sig6, R.d_vm, R.d_wt, R.d_wn, R.d_part);
  FEA_HIP_CHECK(c, hipGetLastError());
  if (d_energy) {
    enq_reduce_final(c, g, 1, 0, R.d_part, d_energy);
    FEA_HIP_CHECK(c, hipGetLastError());
  }
  return FEAHIP_OK;
}

// d_r[3N] (library ids) = minus the unmasked residual on the prescribed dofs of the owned rows, zero elsewhere.  The
// residual goes through d_f, which holds afterwards what it held before; so do the count of bad Gauss points and the
// record of the strategy in use, which a residual assembly may write.
int launch_reactions(feahip_ctx *c, double *d_r, double *d_save)
{
  const size_t nb = sizeof(double) * (size_t)c->ndof;
  const int last_strategy = c->last_strategy;
  int bad = 0, rc;
  FEA_HIP_CHECK(c, hipMemcpyAsync(d_save, c->d_f, nb, hipMemcpyDeviceToDevice, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(&bad, c->d_flag + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  rc = launch_assemble(c, false, true);
  c->last_strategy = last_strategy;
  if (!rc) {
    const int i0 = 3 * c->row0, i1 = 3 * c->row1;
    FEA_HIP_CHECK(c, hipMemsetAsync(d_r, 0, nb, c->stream));
    if (i1 > i0) hipLaunchKernelGGL(k_reactions, dim3((i1 - i0 + 255) / 256), dim3(256), 0, c->stream, i0, i1,
                                    (const uint8_t *)c->d_dofmask, (const double *)c->d_f, d_r);
    FEA_HIP_CHECK(c, hipGetLastError());
  }
  FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_f, d_save, nb, hipMemcpyDeviceToDevice, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_flag + 1, &bad, sizeof(int), hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return rc;
}
