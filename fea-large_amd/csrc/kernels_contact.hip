// kernels_contact.hip -- frictionless contact of nodes with rigid planes, spheres and cylinders (include/fea_hip.h).
//
// A contact node a with the reference-area weight w_a meets obstacle o with the gap g(x), the normal n = dg/dx, the
// penetration p = -g and the pressure t = max(0, mu_ao + eps p):
//   F_a += w_a t n            K_aa += w_a [eps n n' - s t (P - n n') / rho]            Pi_c = sum w_a t^2 / (2 eps)
// (s = 0 plane, +1 solid ball or cylinder, -1 from inside; P = I or I - a a'; rho = |x - c| or |P (x - c)|).  The term
// touches the node's own rows of f and its own diagonal block of K: no pattern change, no atomics, nothing to exchange.
//
// One lane per contact node this rank owns; the obstacles are a kernel argument (at most 8, in their given order, so the
// sums of a node have one order and a second launch gives the same bits).  Bytes per contact node of k_contact<K, f>: 32
// of x (the record k_surface_faces reads), 8 of weight, 4 of node id and of the diagonal index, 8 n_obs of multipliers,
// a 72-byte read-modify-write of the diagonal block and a 24-byte one of f.  A node with rho = 0 is skipped for that
// obstacle, in every kernel.
#include "feahip_internal.h"
#include "reduce_device.h"
#include <cmath>
#include <cstring>
#include <limits>

// ---- device ---------------------------------------------------------------------------------------------------------
namespace {
struct ContactPair {
  double g, n[3], rho, s;      // gap, normal, distance from the centre / axis (planes: 1), curvature sign
  double P[3];                 // the axis a of a cylinder (P = I - a a'), zero for spheres (P = I)
  bool ok;                     // false: rho = 0, the pair is skipped
};
}

__device__ __forceinline__ ContactPair contact_pair(const ContactObstacles &O, int o, double x0, double x1, double x2)
{
  ContactPair c;
  const int kind = O.kind[o];
  const double a0 = O.a[o][0], a1 = O.a[o][1], a2 = O.a[o][2];
  double q0 = x0 - O.c[o][0], q1 = x1 - O.c[o][1], q2 = x2 - O.c[o][2];
  c.ok = true; c.rho = 1.0; c.s = 0.0; c.P[0] = c.P[1] = c.P[2] = 0.0;
  if (kind == FEAHIP_OBSTACLE_PLANE) {
    c.g = q0 * a0 + q1 * a1 + q2 * a2;
    c.n[0] = a0; c.n[1] = a1; c.n[2] = a2;
    return c;
  }
  if (kind == FEAHIP_OBSTACLE_CYLINDER || kind == FEAHIP_OBSTACLE_CYLINDER_INSIDE) {
    const double along = q0 * a0 + q1 * a1 + q2 * a2;
    q0 -= along * a0; q1 -= along * a1; q2 -= along * a2;
    c.P[0] = a0; c.P[1] = a1; c.P[2] = a2;
  }
  const double rho = sqrt(q0 * q0 + q1 * q1 + q2 * q2);
  c.rho = rho;
  if (!(rho > 0.0)) { c.ok = false; c.g = 0.0; c.n[0] = c.n[1] = c.n[2] = 0.0; return c; }
  c.s = (kind == FEAHIP_OBSTACLE_SPHERE || kind == FEAHIP_OBSTACLE_CYLINDER) ? 1.0 : -1.0;
  const double inv = c.s / rho;
  c.g = c.s * (rho - O.r[o]);
  c.n[0] = q0 * inv; c.n[1] = q1 * inv; c.n[2] = q2 * inv;
  return c;
}

__device__ __forceinline__ void contact_x(const double *__restrict__ x, int a, double &x0, double &x1, double &x2)
{
  const double2 *p = reinterpret_cast<const double2 *>(x + (size_t)a * 4);
  const double2 lo = p[0], hi = p[1];
  x0 = lo.x; x1 = lo.y; x2 = hi.x;
}

// BOUND: the stable-step variant -- w eps n n' of every pair whatever its gap, no curvature term, no force
template <bool DOK, bool DOF, bool BOUND>
__global__ __launch_bounds__(256)
void k_contact(int n0, int n1, const int *__restrict__ node, const double *__restrict__ w, const double *__restrict__ mu,
               const double *__restrict__ x, ContactObstacles O, double eps, const int *__restrict__ diag,
               double *__restrict__ K, double *__restrict__ f)
{
  const int i = n0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1) return;
  const int a = node[i];
  const double wa = w[i];
  double x0, x1, x2;
  contact_x(x, a, x0, x1, x2);
  double F[3] = {0, 0, 0}, B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool any = false;
  for (int o = 0; o < O.n; ++o) {
    const ContactPair c = contact_pair(O, o, x0, x1, x2);
    if (!c.ok) continue;
    double t = 0.0;
    if (!BOUND) {
      t = mu[(size_t)i * O.n + o] - eps * c.g;
      if (!(t > 0.0)) continue;
    }
    any = true;
    if (DOF) { F[0] += wa * t * c.n[0]; F[1] += wa * t * c.n[1]; F[2] += wa * t * c.n[2]; }
    if (DOK) {
      const double curv = BOUND ? 0.0 : c.s * t / c.rho;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double nn = c.n[r] * c.n[q];
          const double Prq = (r == q ? 1.0 : 0.0) - c.P[r] * c.P[q];
          B[r * 3 + q] += wa * (eps * nn - curv * (Prq - nn));
        }
    }
  }
  if (!any) return;
  if (DOK) {
    double *d = K + (size_t)diag[a] * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) d[k] += B[k];
  }
  if (DOF) {
    double *o = f + (size_t)a * 3;
    o[0] += F[0]; o[1] += F[1]; o[2] += F[2];
  }
}

__global__ __launch_bounds__(256)
void k_contact_augment(int n0, int n1, const int *__restrict__ node, const double *__restrict__ x, ContactObstacles O,
                       double eps, double *__restrict__ mu)
{
  const int i = n0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1) return;
  double x0, x1, x2;
  contact_x(x, node[i], x0, x1, x2);
  for (int o = 0; o < O.n; ++o) {
    const ContactPair c = contact_pair(O, o, x0, x1, x2);
    if (!c.ok) continue;
    const double t = mu[(size_t)i * O.n + o] - eps * c.g;
    mu[(size_t)i * O.n + o] = t > 0.0 ? t : 0.0;
  }
}

// per workgroup b: part[s FEA_RED_BLOCKS + b], s = 0 active pairs, 1 sum w t, 2 Pi_c, 3 the largest penetration over the
// active pairs (0 without one).  The sums in the order of block_sums; a maximum has no order
__global__ __launch_bounds__(256)
void k_contact_info(int n0, int n1, const int *__restrict__ node, const double *__restrict__ w, const double *__restrict__ mu,
                    const double *__restrict__ x, ContactObstacles O, double eps, double *__restrict__ part)
{
  __shared__ double sh[4][3];
  __shared__ double shmax[4];
  double s[3] = {0, 0, 0}, pmax = 0.0;
  for (int i = n0 + blockIdx.x * 256 + threadIdx.x; i < n1; i += gridDim.x * 256) {
    const double wa = w[i];
    double x0, x1, x2;
    contact_x(x, node[i], x0, x1, x2);
    for (int o = 0; o < O.n; ++o) {
      const ContactPair c = contact_pair(O, o, x0, x1, x2);
      if (!c.ok) continue;
      const double t = mu[(size_t)i * O.n + o] - eps * c.g;
      if (!(t > 0.0)) continue;
      s[0] += 1.0; s[1] += wa * t; s[2] += wa * t * t / (2.0 * eps);
      pmax = fmax(pmax, -c.g);
    }
  }
  const double t = block_sums<3>(s, sh);
  if (threadIdx.x < 3) part[(size_t)threadIdx.x * FEA_RED_BLOCKS + blockIdx.x] = t;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pmax = fmax(pmax, __shfl_down(pmax, off, 64));
  if ((threadIdx.x & 63) == 0) shmax[threadIdx.x >> 6] = pmax;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)3 * FEA_RED_BLOCKS + blockIdx.x] = fmax(fmax(shmax[0], shmax[1]), fmax(shmax[2], shmax[3]));
}

// out[0] = max of part[0 .. n)  (one block)
__global__ __launch_bounds__(256)
void k_contact_max_final(int n, const double *__restrict__ part, double *__restrict__ out)
{
  __shared__ double shmax[4];
  double m = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) m = fmax(m, part[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) shmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = fmax(fmax(shmax[0], shmax[1]), fmax(shmax[2], shmax[3]));
}

// the getters' kernel: the smallest gap over the obstacles and the summed pressure, at the node's place in [N] arrays
__global__ __launch_bounds__(256)
void k_contact_status(int n0, int n1, const int *__restrict__ node, const double *__restrict__ mu,
                      const double *__restrict__ x, ContactObstacles O, double eps, double *__restrict__ gap,
                      double *__restrict__ pressure)
{
  const int i = n0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1) return;
  const int a = node[i];
  double x0, x1, x2;
  contact_x(x, a, x0, x1, x2);
  double gmin = INFINITY, tsum = 0.0;
  for (int o = 0; o < O.n; ++o) {
    const ContactPair c = contact_pair(O, o, x0, x1, x2);
    if (!c.ok) continue;
    const double t = mu[(size_t)i * O.n + o] - eps * c.g;
    gmin = fmin(gmin, c.g);
    if (t > 0.0) tsum += t;
  }
  gap[a] = gmin;
  pressure[a] = tsum;
}

// ---- launchers ------------------------------------------------------------------------------------------------------
static ContactObstacles obstacles_now(const feahip_ctx *c)
{
  const ContactState &S = c->contact;
  ContactObstacles O;
  memset(&O, 0, sizeof(O));
  O.n = S.nobs;
  for (int o = 0; o < S.nobs; ++o) {
    O.kind[o] = S.kind[o];
    for (int j = 0; j < 3; ++j) {
      O.c[o][j] = S.geom[o][j] + c->load_factor * S.geom[o][7 + j];
      O.a[o][j] = S.geom[o][3 + j];
    }
    O.r[o] = S.geom[o][6];
  }
  return O;
}

// the contact nodes of the rows this rank owns (all of them unsharded)
void contact_owned(const feahip_ctx *c, int &n0, int &n1)
{
  const std::vector<int> &h = c->contact.h_node;
  n0 = (int)(std::lower_bound(h.begin(), h.end(), c->row0) - h.begin());
  n1 = (int)(std::lower_bound(h.begin(), h.end(), c->row1) - h.begin());
}

int launch_contact(feahip_ctx *c, bool doK, bool doF, double *d_fv)
{
  const ContactState &S = c->contact;
  if (S.n == 0) return FEAHIP_OK;
  int n0, n1;
  contact_owned(c, n0, n1);
  if (n1 == n0) return FEAHIP_OK;
  const ContactObstacles O = obstacles_now(c);
  const dim3 grid((n1 - n0 + 255) / 256), block(256);
  with_kf(doK, doF, [&](auto DOK, auto DOF) {
    hipLaunchKernelGGL((k_contact<decltype(DOK)::value, decltype(DOF)::value, false>), grid, block, 0, c->stream, n0, n1, S.d_node, S.d_w, S.d_mu, c->d_x, O,
                       S.penalty, c->d_diag, c->d_K, d_fv);
  });
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_contact_bound(feahip_ctx *c)
{
  const ContactState &S = c->contact;
  if (S.n == 0) return FEAHIP_OK;
  int n0, n1;
  contact_owned(c, n0, n1);
  if (n1 == n0) return FEAHIP_OK;
  hipLaunchKernelGGL((k_contact<true, false, true>), dim3((n1 - n0 + 255) / 256), dim3(256), 0, c->stream, n0, n1, S.d_node,
                     S.d_w, S.d_mu, c->d_x, obstacles_now(c), S.penalty, c->d_diag, c->d_K, (double *)nullptr);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_contact_augment(feahip_ctx *c)
{
  const ContactState &S = c->contact;
  if (S.n == 0) return FEAHIP_OK;
  int n0, n1;
  contact_owned(c, n0, n1);
  if (n1 == n0) return FEAHIP_OK;
  hipLaunchKernelGGL(k_contact_augment, dim3((n1 - n0 + 255) / 256), dim3(256), 0, c->stream, n0, n1, S.d_node, c->d_x,
                     obstacles_now(c), S.penalty, S.d_mu);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_contact_info(feahip_ctx *c)
{
  const ContactState &S = c->contact;
  int n0 = 0, n1 = 0;
  if (S.n) contact_owned(c, n0, n1);
  if (n1 == n0) {                                              // nothing of it on this rank: four zeros
    FEA_HIP_CHECK(c, hipMemsetAsync(c->d_scal + 8, 0, sizeof(double) * 4, c->stream));
    return FEAHIP_OK;
  }
  int g = (n1 - n0 + 255) / 256;
  g = g < FEA_RED_BLOCKS ? g : FEA_RED_BLOCKS;
  hipLaunchKernelGGL(k_contact_info, dim3(g), dim3(256), 0, c->stream, n0, n1, S.d_node, S.d_w, S.d_mu, c->d_x,
                     obstacles_now(c), S.penalty, S.d_part);
  enq_reduce_final(c, g, 3, FEA_RED_BLOCKS, S.d_part, c->d_scal + 8);
  hipLaunchKernelGGL(k_contact_max_final, dim3(1), dim3(256), 0, c->stream, g, S.d_part + (size_t)3 * FEA_RED_BLOCKS,
                     c->d_scal + 11);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_contact_status(feahip_ctx *c, double *d_gap, double *d_pressure)
{
  const ContactState &S = c->contact;
  if (S.n == 0) return FEAHIP_OK;
  int n0, n1;
  contact_owned(c, n0, n1);
  if (n1 == n0) return FEAHIP_OK;
  hipLaunchKernelGGL(k_contact_status, dim3((n1 - n0 + 255) / 256), dim3(256), 0, c->stream, n0, n1, S.d_node, S.d_mu, c->d_x,
                     obstacles_now(c), S.penalty, d_gap, d_pressure);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// ---- host: the contact nodes and their weights ------------------------------------------------------------------------
// w[npf] of one face from its reference nodes X[npf][3]: the rule of face_rule with dA = |X_xi x X_eta|
static void face_weights(int npf, const FaceRule &R, const double (*X)[3], double *w)
{
  double area = 0.0, lump[FEA_SURF_MAX_NPF] = {0, 0, 0, 0, 0, 0};
  for (int q = 0; q < R.npt; ++q) {
    double t1[3] = {0, 0, 0}, t2[3] = {0, 0, 0};
    for (int a = 0; a < npf; ++a)
      for (int i = 0; i < 3; ++i) { t1[i] += R.dN[q][0][a] * X[a][i]; t2[i] += R.dN[q][1][a] * X[a][i]; }
    const double n0 = t1[1] * t2[2] - t1[2] * t2[1], n1 = t1[2] * t2[0] - t1[0] * t2[2], n2 = t1[0] * t2[1] - t1[1] * t2[0];
    const double dA = R.w[q] * std::sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    area += dA;
    // tri6: the diagonal of the consistent matrix (HRZ); tri3, quad4: the row sums int N_a dA
    for (int a = 0; a < npf; ++a) lump[a] += (npf == 6 ? R.N[q][a] * R.N[q][a] : R.N[q][a]) * dA;
  }
  double sum = 0.0;
  for (int a = 0; a < npf; ++a) sum += lump[a];
  for (int a = 0; a < npf; ++a) w[a] = npf == 6 ? lump[a] * (area / sum) : lump[a];
}

int set_contact(feahip_ctx *c, int nfaces, int npf, const int *face_nodes, int n_obstacles, const int *kind,
                const double *geom, double penalty, int augment_max, double gap_tolerance)
{
  auto refuse = [c](std::string why) { c->err = "feahip_set_contact: " + std::move(why); return FEAHIP_EINVAL; };
  if (nfaces < 0 || n_obstacles < 0) return refuse("negative count");
  // (a slab of feahip_create_rank_local that holds none of the contact faces still takes the obstacles and the parameters:
  // its rank enters the collectives of the augmentation with the others)
  const bool empty_slab = c->rank_local_ids && nfaces == 0 && n_obstacles > 0;
  if (!empty_slab && (nfaces == 0 || n_obstacles == 0)) {      // cleared
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    c->contact.release();
    return FEAHIP_OK;
  }
  if ((nfaces > 0 && !face_nodes) || !kind || !geom) return refuse("null array");
  if (n_obstacles > FEAHIP_MAX_OBSTACLES)
    return refuse(std::to_string(n_obstacles) + " obstacles, at most " + std::to_string(FEAHIP_MAX_OBSTACLES));
  if (!(penalty > 0.0) || !std::isfinite(penalty)) return refuse("the penalty must be positive");
  if (augment_max < 0) return refuse("augment_max must not be negative");
  if (!(gap_tolerance >= 0.0)) return refuse("gap_tolerance must not be negative");
  ContactState S;
  for (int o = 0; o < n_obstacles; ++o) {
    const double *g = geom + (size_t)o * 10;
    const std::string who = "obstacle " + std::to_string(o);
    if (kind[o] < FEAHIP_OBSTACLE_PLANE || kind[o] > FEAHIP_OBSTACLE_CYLINDER_INSIDE) return refuse(who + ": unknown kind " + std::to_string(kind[o]));
    for (int j = 0; j < 10; ++j) if (!std::isfinite(g[j])) return refuse(who + ": a value is not finite");
    const bool sphere = kind[o] == FEAHIP_OBSTACLE_SPHERE || kind[o] == FEAHIP_OBSTACLE_SPHERE_INSIDE;
    const double len = std::sqrt(g[3] * g[3] + g[4] * g[4] + g[5] * g[5]);
    if (!sphere && !(len > 0.0)) return refuse(who + ": zero direction");
    if (kind[o] != FEAHIP_OBSTACLE_PLANE && !(g[6] > 0.0)) return refuse(who + ": the radius must be positive");
    S.kind[o] = kind[o];
    for (int j = 0; j < 10; ++j) S.geom[o][j] = g[j];
    for (int j = 3; j < 6; ++j) S.geom[o][j] = sphere ? 0.0 : g[j] / len;
  }
  std::vector<int> fn, keep;
  if (const int rc = context_surface_faces(c, nfaces, npf, face_nodes, fn, keep)) return rc;
  // weights in double from X0: the faces' shares summed per node in a fixed order (node, then face slot, ascending)
  std::vector<double> X0((size_t)c->N * 4), share(fn.size());
  FEA_HIP_CHECK(c, hipMemcpy(X0.data(), c->d_X0, sizeof(double) * X0.size(), hipMemcpyDeviceToHost));
  FaceRule R;
  face_rule(npf, R);
  for (size_t f = 0; f < keep.size(); ++f) {
    double X[FEA_SURF_MAX_NPF][3];
    for (int k = 0; k < npf; ++k)
      for (int i = 0; i < 3; ++i) X[k][i] = X0[(size_t)fn[f * npf + k] * 4 + i];
    face_weights(npf, R, X, share.data() + f * npf);
  }
  std::vector<std::pair<int, int>> inc;
  inc.reserve(fn.size());
  for (size_t s = 0; s < fn.size(); ++s) inc.emplace_back(fn[s], (int)s);
  std::sort(inc.begin(), inc.end());
  for (size_t i = 0; i < inc.size(); ++i) {
    if (i == 0 || inc[i].first != inc[i - 1].first) { S.h_node.push_back(inc[i].first); S.h_w.push_back(0.0); }
    S.h_w.back() += share[inc[i].second];
  }
  S.set = true;
  S.n = (int)S.h_node.size(); S.nobs = n_obstacles;
  S.penalty = penalty; S.augment_max = augment_max; S.gap_tolerance = gap_tolerance;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));           // no launch in flight reads the old set
  c->contact.release();
  if (S.n > 0) {                                               // (a rank that kept no face holds the parameters alone)
    auto up = [c](auto **dst, const auto *src, size_t n) -> int {
      FEA_HIP_CHECK(c, hipMalloc((void **)dst, sizeof(**dst) * n));
      FEA_HIP_CHECK(c, hipMemcpy(*dst, src, sizeof(**dst) * n, hipMemcpyHostToDevice));
      return FEAHIP_OK;
    };
    int rc;
    if ((rc = up(&S.d_node, S.h_node.data(), S.h_node.size())) || (rc = up(&S.d_w, S.h_w.data(), S.h_w.size()))) { S.release(); return rc; }
    const size_t nmu = sizeof(double) * (size_t)S.n * S.nobs;
    if (hipMalloc((void **)&S.d_mu, nmu) != hipSuccess || hipMalloc((void **)&S.d_part, sizeof(double) * 4 * FEA_RED_BLOCKS) != hipSuccess ||
        hipMemset(S.d_mu, 0, nmu) != hipSuccess) {
      S.release(); c->err = "feahip_set_contact: out of device memory"; return FEAHIP_ENOMEM;
    }
  }
  c->contact = std::move(S);
  return FEAHIP_OK;
}
