// kernels_modal_stress.hip -- the linearised nodal stress on gfx950: the linear map from a displacement increment du at the
// current nodes x to the nodal Cauchy stress it causes, applied to a panel of eight columns at a time (the modes of the
// locked store, the static correction u_s, a caller's vector).
//
// At a Gauss point, with g[a][j] = dN_a/dx_j of gp_state,
//   l_ij = sum_a du_a,i g[a][j],   d = (l + l') / 2
//   dsigma = c : d + l sigma + sigma l' - tr(d) sigma                       (the Truesdell rate of the Cauchy stress)
// sigma the Cauchy stress of the point, c the spatial tangent of the model.  With l1, m1 of GPState (fd_constitutive):
//   Neo-Hookean  c : d = l1 tr(d) I + 2 m1 d,            l1 = lambda / J, m1 = (mu - lambda ln J) / J
//   A5           c : d = l1 (b : d) b + 2 m1 b d b,      l1 = lambda / J, m1 = mu / J, b = F F'
// For the Neo-Hookean model l1, m1 are the coefficients of the minor-symmetrised tangent the stiffness uses (fem_device.h);
// for A5 the stiffness takes the same two numbers on the identity instead of b, the reference's simplification, and the
// stress increment here takes the tangent of the model itself.
//
// The nodal value keeps the weights of k_result_nodes, held fixed:
//   T_a = sum_e sum_g vol_g dsigma_g / sum_e sum_g vol_g,   vol_g = w_g |det J_g| at x
// over all elements at the node or over those of one material, components xx yy zz xy yz xz.  At an unstressed state this
// is exactly the derivative of feahip_get_nodal_stresses; at a prestressed state it leaves out the variation of the weights.
//
//   k_mstress_elements  one thread per element: load_element, then gp_state ONCE per Gauss point, applied to the eight
//                       columns of the panel in two halves of four (nine l_ij per column in registers).  A node's eight
//                       columns of three dofs are 192 contiguous bytes of the [3N][8] panel: twelve 16-byte loads.  One
//                       record of [6][8] sums of vol dsigma per element and panel; the element volume once per call.
//   k_mstress_nodes     the visit lists and the round-robin order of k_result_nodes (pattern.cpp): one wave per chunk of
//                       16 rows, four lanes per row, lane q carries the columns 2q, 2q + 1 of the six components and its
//                       own copy of the weight, in visit order -- no atomics, the same bits on every call.  It writes
//                       rows 6a .. 6a + 5 of a panel [6N][8] of the stress store, the layout of superpose.h: a lane that
//                       owns row 6a + c loads it with load_mode_values.
// A single vector is a panel with one live column (k_stress_spread, k_stress_column).  Nothing here is allocated or
// launched on a context that never calls a stress entry.
#include "superpose.h"
#include "fem_device.h"

// rounds of the node pass whose loads are in flight together
#define MSTRESS_ROUNDS 2

template <int NPE, bool LINTET, bool HET>
__global__ __launch_bounds__(256)
void k_mstress_elements(AsmArgs A, const double *__restrict__ U, double *__restrict__ rec, double *__restrict__ evol)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= A.E) return;
  int nd[NPE];
  double xe[NPE][3], Xe[NPE][3];
  load_element<NPE>(A, e, nd, xe, Xe);
  const double2 lm = elem_material<HET>(A, e);
  const bool a5 = A.model != FEAHIP_MODEL_COMPRESSIBLE_NEOHOOKEAN;
  double acc[6][MC], vol = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c)
#pragma unroll
    for (int k = 0; k < MC; ++k) acc[c][k] = 0.0;
  for (int gp = 0; gp < A.G; ++gp) {
    GPState<NPE> s;
    gp_state<NPE, LINTET>(xe, Xe, A.tab, gp, A.model, lm.x, lm.y, s);
    vol += s.vol;
    double b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) b[i][j] = s.F[i][0] * s.F[j][0] + s.F[i][1] * s.F[j][1] + s.F[i][2] * s.F[j][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double l[4][3][3];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) l[k][i][j] = 0.0;
#pragma unroll
      for (int a = 0; a < NPE; ++a) {
        const mode_v2d *p = reinterpret_cast<const mode_v2d *>(U + (size_t)nd[a] * (3 * MC));
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const mode_v2d v0 = p[i * 4 + 2 * h], v1 = p[i * 4 + 2 * h + 1];
          const double du[4] = {v0.x, v0.y, v1.x, v1.y};
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) l[k][i][j] = fma(du[k], s.g[a][j], l[k][i][j]);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double d[3][3], cd[3][3], ls[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) d[i][j] = 0.5 * (l[k][i][j] + l[k][j][i]);
        const double tr = d[0][0] + d[1][1] + d[2][2];
        if (a5) {
          double bd = 0.0, t[3][3];
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              bd += b[i][j] * d[i][j];
              t[i][j] = b[i][0] * d[0][j] + b[i][1] * d[1][j] + b[i][2] * d[2][j];
            }
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
              cd[i][j] = s.l1 * bd * b[i][j] + 2.0 * s.m1 * (t[i][0] * b[0][j] + t[i][1] * b[1][j] + t[i][2] * b[2][j]);
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) cd[i][j] = 2.0 * s.m1 * d[i][j] + ((i == j) ? s.l1 * tr : 0.0);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j)
            ls[i][j] = l[k][i][0] * s.sig[0][j] + l[k][i][1] * s.sig[1][j] + l[k][i][2] * s.sig[2][j];
        const int ci[6] = {0, 1, 2, 0, 1, 0}, cj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const int i = ci[c], j = cj[c];
          const double ds = cd[i][j] + ls[i][j] + ls[j][i] - tr * s.sig[i][j];
          acc[c][4 * h + k] = fma(s.vol, ds, acc[c][4 * h + k]);
        }
      }
    }
  }
  mode_v2d *o = reinterpret_cast<mode_v2d *>(rec + (size_t)e * (6 * MC));
#pragma unroll
  for (int c = 0; c < 6; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mode_v2d r;
      r.x = acc[c][2 * k]; r.y = acc[c][2 * k + 1];
      o[c * 4 + k] = r;
    }
  if (evol) evol[e] = vol;
}

// See the file header and k_result_nodes, whose walk over the visits this is.  Lane q of a row carries the columns
// 2q, 2q + 1 of the six components and the weight.
__global__ __launch_bounds__(64 * FEA_WAVES_PER_WG)
void k_mstress_nodes(int chunk0, int nchunks, const int *__restrict__ chunk, const int *__restrict__ incptr,
                     const uint32_t *__restrict__ inc, const mode_v2d *__restrict__ rec, const double *__restrict__ evol,
                     const uint8_t *__restrict__ emat, int material, mode_v2d *__restrict__ T)
{
  static_assert(FEA_CHUNK_ROWS * 4 <= 64, "four lanes per row of a chunk");
  constexpr int R = MSTRESS_ROUNDS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row = lane >> 2, q = lane & 3;
  const unsigned long long below = (1ull << (row * 4)) - 1ull;   // the leader lanes of the rows before this one
  for (int ch = chunk0 + blockIdx.x * FEA_WAVES_PER_WG + wave; ch < chunk0 + nchunks; ch += gridDim.x * FEA_WAVES_PER_WG) {
    const int r0 = chunk[ch], r1 = chunk[ch + 1];
    const int a = r0 + row;
    const bool live = a < r1;
    const int len = live ? incptr[a + 1] - incptr[a] : 0;
    int base = incptr[r0];                             // position of the first visit of round k
    mode_v2d acc[6];
    double wgt = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) { acc[c].x = 0.0; acc[c].y = 0.0; }
    for (int k = 0;; k += R) {
      bool act[R];
      int pos[R];
      int nxt = base;
#pragma unroll
      for (int j = 0; j < R; ++j) {
        act[j] = k + j < len;
        const unsigned long long lead = __ballot(act[j] && q == 0);
        pos[j] = nxt + __popcll(lead & below);
        nxt += __popcll(lead);
      }
      if (nxt == base) break;                          // no row has a visit left
      base = nxt;
      int e[R];
#pragma unroll
      for (int j = 0; j < R; ++j) e[j] = act[j] ? (int)(inc[pos[j]] & 0x0FFFFFFFu) : -1;
      if (material >= 0) {
#pragma unroll
        for (int j = 0; j < R; ++j) e[j] = (e[j] >= 0 && (int)emat[e[j]] == material) ? e[j] : -1;
      }
      mode_v2d r[R][6];
      double w[R];
#pragma unroll
      for (int j = 0; j < R; ++j)
        if (e[j] >= 0) {
          w[j] = evol[e[j]];
#pragma unroll
          for (int c = 0; c < 6; ++c) r[j][c] = rec[(size_t)e[j] * 24 + c * 4 + q];
        }
#pragma unroll
      for (int j = 0; j < R; ++j)
        if (e[j] >= 0) {
          wgt += w[j];
#pragma unroll
          for (int c = 0; c < 6; ++c) acc[c] += r[j][c];
        }
    }
    const double inv = wgt != 0.0 ? 1.0 / wgt : 0.0;    // no selected element at this node: stress 0
    if (live) {
#pragma unroll
      for (int c = 0; c < 6; ++c) T[((size_t)a * 6 + c) * 4 + q] = acc[c] * inv;
    }
  }
}

// panel[d][0] = v[d], the other seven columns zero
__global__ __launch_bounds__(256)
void k_stress_spread(int n, const double *__restrict__ v, double *__restrict__ panel)
{
  const int i = blockIdx.x * 256 + threadIdx.x;        // one of the 8 n entries
  if (i < n * MC) panel[i] = (i & (MC - 1)) ? 0.0 : v[i >> 3];
}

// out[r] = panel[r][col]
__global__ __launch_bounds__(256)
void k_stress_column(int n, const double *__restrict__ panel, int col, double *__restrict__ out)
{
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < n) out[r] = panel[(size_t)r * MC + col];
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
int stress_ensure(feahip_ctx *c)
{
  StressState &S = c->stress;
  int rc;
  if ((rc = ensure_generic_maps(c))) return rc;
  if (S.d_rec) return FEAHIP_OK;
  const size_t N = (size_t)c->N;
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_rec, sizeof(double) * 6 * MC * (size_t)c->E));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_evol, sizeof(double) * (size_t)c->E));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_vec, sizeof(double) * 3 * N));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_in, sizeof(double) * 3 * N * MC));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_one, sizeof(double) * 6 * N * MC));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_out6, sizeof(double) * 6 * N));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_vm, sizeof(double) * N));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_ts, sizeof(double) * 6 * N));
  return FEAHIP_OK;
}

// both passes at the current nodes: the panel d_in8 [3N][8] into the panel d_out8 [6N][8]; first: the element volumes too
static int launch_stress_panel(feahip_ctx *c, const double *d_in8, int material, bool first, double *d_out8)
{
  StressState &S = c->stress;
  AsmArgs A = AsmArgs();
  A.N = c->N; A.E = c->E; A.G = c->G; A.model = c->model;
  A.lambda = c->lambda; A.mu = c->mu; A.mat = c->d_mat; A.emat = c->d_elem_mat;
  A.tab = c->d_table; A.conn = c->d_conn; A.X0 = c->d_X0; A.x = c->d_x;
  const int grid = (c->E + 255) / 256;
  double *ev = first ? S.d_evol : nullptr;
  auto launch = [&](auto H) {
    if (c->npe == 4) {
      if (c->linear_tet) hipLaunchKernelGGL((k_mstress_elements<4, true, H>), dim3(grid), dim3(256), 0, c->stream, A, d_in8, S.d_rec, ev);
      else hipLaunchKernelGGL((k_mstress_elements<4, false, H>), dim3(grid), dim3(256), 0, c->stream, A, d_in8, S.d_rec, ev);
    } else if (c->npe == 8)
      hipLaunchKernelGGL((k_mstress_elements<8, false, H>), dim3(grid), dim3(256), 0, c->stream, A, d_in8, S.d_rec, ev);
    else
      hipLaunchKernelGGL((k_mstress_elements<10, false, H>), dim3(grid), dim3(256), 0, c->stream, A, d_in8, S.d_rec, ev);
  };
  if (c->n_materials) launch(std::true_type()); else launch(std::false_type());
  FEA_HIP_CHECK(c, hipGetLastError());
  int g = (c->nchunks_local + FEA_WAVES_PER_WG - 1) / FEA_WAVES_PER_WG;
  g = g < FEA_RED_BLOCKS ? (g > 0 ? g : 1) : FEA_RED_BLOCKS;
  hipLaunchKernelGGL(k_mstress_nodes, dim3(g), dim3(64 * FEA_WAVES_PER_WG), 0, c->stream, c->chunk0, c->nchunks_local,
                     (const int *)c->d_chunk, (const int *)c->generic.d_incptr, (const uint32_t *)c->generic.d_inc,
                     (const mode_v2d *)S.d_rec, (const double *)S.d_evol, (const uint8_t *)c->d_elem_mat,
                     c->n_materials ? material : -1, (mode_v2d *)d_out8);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// d_out[6N] = the stress of the single vector d_v[3N] (library ids), through a panel with one live column
int launch_stress_vector(feahip_ctx *c, const double *d_v, int material, double *d_out)
{
  StressState &S = c->stress;
  int rc;
  if ((rc = stress_ensure(c))) return rc;
  const int n3 = c->ndof, n6 = 6 * c->N;
  hipLaunchKernelGGL(k_stress_spread, dim3((n3 * MC + 255) / 256), dim3(256), 0, c->stream, n3, d_v, S.d_in);
  FEA_HIP_CHECK(c, hipGetLastError());
  if ((rc = launch_stress_panel(c, S.d_in, material, true, S.d_one))) return rc;
  hipLaunchKernelGGL(k_stress_column, dim3((n6 + 255) / 256), dim3(256), 0, c->stream, n6, (const double *)S.d_one, 0, d_out);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

double *stress_panel(feahip_ctx *c, int panel) { return c->stress.d_store + (size_t)panel * 6 * c->N * MC; }

// the element and node passes over every panel of the locked store in use
static int launch_stress_store(feahip_ctx *c, int material)
{
  int rc;
  for (int p = 0; p < panels_of(c); ++p)
    if ((rc = launch_stress_panel(c, locked_panel(c, 0, p), material, p == 0, stress_panel(c, p)))) return rc;
  return FEAHIP_OK;
}

// the stress store of the modes held, and T_s of the u_s of the load held with the static correction (zero otherwise)
int stress_basis(feahip_ctx *c, int material)
{
  StressState &S = c->stress;
  const ResponseState &R = c->response;
  int rc;
  S.have = false;
  S.form_set = false;
  c->fatigue.drop();                                                   // (the moments were those of the old store)
  if ((rc = stress_ensure(c))) return rc;
  const int panels = panels_of(c);
  if (panels > S.store_panels) {
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    dev_free({S.d_store});
    S.d_store = nullptr; S.store_panels = 0;
    FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_store, sizeof(double) * (size_t)panels * 6 * c->N * MC));
    S.store_panels = panels;
  }
  if ((rc = launch_stress_store(c, material))) return rc;
  const bool with_us = R.loaded && R.gen == c->modal.lock_gen && R.correction;
  if (with_us) { if ((rc = launch_stress_vector(c, R.d_us, material, S.d_ts))) return rc; }
  else FEA_HIP_CHECK(c, hipMemsetAsync(S.d_ts, 0, sizeof(double) * 6 * (size_t)c->N, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  S.material = material;
  S.gen = c->modal.lock_gen;
  S.load_count = R.load_count;
  S.have = true;
  return FEAHIP_OK;
}

// d_out[6N] = column `col` of the stress store
int launch_stress_mode(feahip_ctx *c, int col, double *d_out)
{
  const int n6 = 6 * c->N;
  hipLaunchKernelGGL(k_stress_column, dim3((n6 + 255) / 256), dim3(256), 0, c->stream, n6,
                     (const double *)stress_panel(c, col / MC), col % MC, d_out);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// hook 27 of feahip_time_kernel: both passes over every panel of the locked store in use, at the current nodes, into the
// scratch panel of the single-vector path -- the stress store keeps the stresses of the nodes of its basis call
int time_stress_store(feahip_ctx *c)
{
  int rc;
  for (int p = 0; p < panels_of(c); ++p)
    if ((rc = launch_stress_panel(c, locked_panel(c, 0, p), c->stress.material, p == 0, c->stress.d_one))) return rc;
  return FEAHIP_OK;
}
