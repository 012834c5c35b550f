// kernels_surface.hip -- surface loads: follower pressure and dead traction on boundary faces.
//
// The reference leaves solver_create_forces_bc empty (fea_solver.c:1191-1198).  Here a loaded face is a boundary face
// of exactly one element -- a 3-node triangle of a TET4, a 6-node triangle of a TET10, a 4-node quad of a HEX8 --
// and contributes F_a = int N_a t da to the residual of every assembly that writes f:  f = lambda F_ext(x) - T(x).
//   pressure p (follower):  t da = -p n da on the CURRENT face, n da = x_xi x x_eta dxi deta
//   traction t0 (dead):     t da = t0 dA,  dA = |X_xi x X_eta| dxi deta on the REFERENCE face
// n da is a polynomial on the face, integrated exactly: tri3 one point, tri6 the 6-point degree-4 rule (two linear
// tangents times a quadratic N), quad4 2 x 2 Gauss.  The dead traction uses the same points (dA is not polynomial on a
// warped face, an approximation as the volume rules are).  No load stiffness is assembled.
//
// Two kernels, no atomics, a fixed summation order (bitwise reproducible, as the volume assembly):
//   k_surface_faces   one lane per face: gathers the face's nodes, writes its npf x 3 contributions (x lambda)
//   k_surface_nodes   one lane per loaded node this rank owns: sums its (face, slot) contributions, adds them to f
// Bytes per launch: a face reads npf node records (32 B each, mostly shared with its neighbours through L2) and its
// kind and values, writes npf x 24 B; a loaded node reads its incidence list and ~6 contributions and adds 24 B to f.
#include "feahip_internal.h"
#include <array>
#include <cmath>
#include <cstring>
#include <mutex>
#include <unordered_map>

// ---- local faces of the element types: node order such that (x1 - x0) x (x2 - x0) (triangles) or the quad's
// (xi, eta) parametrisation points OUT of a positively oriented element.  Tetrahedra: a face per opposite vertex;
// 10-node faces list their corners, then the mid-side nodes of (0,1) (1,2) (2,0) of the face (local order of the
// element: 4:(0,1) 5:(1,2) 6:(0,2) 7:(0,3) 8:(1,3) 9:(2,3)).  Bricks: corners of fea_elements.c, counter-clockwise seen
// from outside.
static const int kTet4Faces[4][3] = {{0, 2, 1}, {0, 1, 3}, {0, 3, 2}, {1, 2, 3}};
static const int kTet10Faces[4][6] = {{0, 2, 1, 6, 5, 4}, {0, 1, 3, 4, 8, 7}, {0, 3, 2, 7, 9, 6}, {1, 2, 3, 5, 9, 8}};
static const int kHex8Faces[6][4] = {{0, 3, 2, 1}, {4, 5, 6, 7}, {0, 1, 5, 4}, {1, 2, 6, 5}, {2, 3, 7, 6}, {3, 0, 4, 7}};

static int faces_per_element(int npe) { return npe == 8 ? 6 : 4; }
static int nodes_per_face(int npe) { return npe == 4 ? 3 : (npe == 10 ? 6 : 4); }
static int face_node(int npe, int lf, int k)
{
  return npe == 4 ? kTet4Faces[lf][k] : (npe == 10 ? kTet10Faces[lf][k] : kHex8Faces[lf][k]);
}

// ---- quadrature of a face (FaceRule, feahip_internal.h): points, weights (reference area included), N and dN/d(xi, eta)
void face_rule(int npf, FaceRule &R)
{
  memset(&R, 0, sizeof(R));
  if (npf == 4) {                                              // quad4: 2 x 2 Gauss on [-1, 1]^2
    const double g = 1.0 / std::sqrt(3.0);
    const double xa[4] = {-1, 1, 1, -1}, ea[4] = {-1, -1, 1, 1};
    const double qx[4] = {-g, g, g, -g}, qe[4] = {-g, -g, g, g};
    R.npt = 4;
    for (int q = 0; q < 4; ++q) {
      R.w[q] = 1.0;
      for (int a = 0; a < 4; ++a) {
        R.N[q][a] = 0.25 * (1 + xa[a] * qx[q]) * (1 + ea[a] * qe[q]);
        R.dN[q][0][a] = 0.25 * xa[a] * (1 + ea[a] * qe[q]);
        R.dN[q][1][a] = 0.25 * ea[a] * (1 + xa[a] * qx[q]);
      }
    }
    return;
  }
  // triangles on (xi, eta) >= 0, xi + eta <= 1: area 1/2
  double px[6], pe[6];
  if (npf == 3) {
    R.npt = 1; px[0] = pe[0] = 1.0 / 3.0; R.w[0] = 0.5;
  } else {
    // the 6-point degree-4 rule (Strang & Fix; Dunavant 1985) in closed form: points (a, a), (1 - 2a, a), (a, 1 - 2a)
    const double s10 = std::sqrt(10.0), r = std::sqrt(38.0 - 44.0 * std::sqrt(0.4));
    const double a1 = (8.0 - s10 + r) / 18.0, a2 = (8.0 - s10 - r) / 18.0;
    const double d = std::sqrt(213125.0 - 53320.0 * s10);
    const double w1 = (620.0 + d) / 3720.0, w2 = (620.0 - d) / 3720.0;   // 3 (w1 + w2) = 1
    const double a[2] = {a1, a2}, w[2] = {w1, w2};
    R.npt = 6;
    for (int k = 0; k < 2; ++k) {
      px[3 * k + 0] = a[k];             pe[3 * k + 0] = a[k];
      px[3 * k + 1] = 1.0 - 2.0 * a[k]; pe[3 * k + 1] = a[k];
      px[3 * k + 2] = a[k];             pe[3 * k + 2] = 1.0 - 2.0 * a[k];
      for (int j = 0; j < 3; ++j) R.w[3 * k + j] = 0.5 * w[k];
    }
  }
  for (int q = 0; q < R.npt; ++q) {
    const double x = px[q], e = pe[q], l = 1.0 - x - e;
    if (npf == 3) {
      R.N[q][0] = l; R.N[q][1] = x; R.N[q][2] = e;
      R.dN[q][0][0] = -1; R.dN[q][0][1] = 1; R.dN[q][0][2] = 0;
      R.dN[q][1][0] = -1; R.dN[q][1][1] = 0; R.dN[q][1][2] = 1;
    } else {                                                   // corners 0 1 2, mid-sides (0,1) (1,2) (2,0)
      R.N[q][0] = l * (2 * l - 1); R.N[q][1] = x * (2 * x - 1); R.N[q][2] = e * (2 * e - 1);
      R.N[q][3] = 4 * l * x; R.N[q][4] = 4 * x * e; R.N[q][5] = 4 * e * l;
      const double dx[6] = {-(4 * l - 1), 4 * x - 1, 0, 4 * (l - x), 4 * e, -4 * e};
      const double de[6] = {-(4 * l - 1), 0, 4 * e - 1, -4 * x, 4 * x, 4 * (l - e)};
      for (int a = 0; a < 6; ++a) { R.dN[q][0][a] = dx[a]; R.dN[q][1][a] = de[a]; }
    }
  }
}

// ---- device ---------------------------------------------------------------------------------------------------------
template <int NPF>
__global__ __launch_bounds__(256)
void k_surface_faces(int nfaces, const int *__restrict__ fnode, const int *__restrict__ kind,
                     const double *__restrict__ val, const double *__restrict__ x, const double *__restrict__ X0,
                     double lam, FaceRule R, double *__restrict__ fc)
{
  const int face = blockIdx.x * blockDim.x + threadIdx.x;
  if (face >= nfaces) return;
  const bool pressure = kind[face] == FEAHIP_LOAD_PRESSURE;
  const double *__restrict__ P = pressure ? x : X0;          // current face for the follower pressure, reference face for t0
  double xa[NPF][3];
#pragma unroll
  for (int a = 0; a < NPF; ++a) {
    const double2 *p = reinterpret_cast<const double2 *>(P + (size_t)fnode[(size_t)face * NPF + a] * 4);
    const double2 lo = p[0], hi = p[1];
    xa[a][0] = lo.x; xa[a][1] = lo.y; xa[a][2] = hi.x;
  }
  const double v0 = val[(size_t)face * 3], v1 = val[(size_t)face * 3 + 1], v2 = val[(size_t)face * 3 + 2];
  constexpr int NPT = NPF == 3 ? 1 : (NPF == 6 ? 6 : 4);    // = R.npt; a compile-time count keeps R's indices static
  double acc[NPF][3];
#pragma unroll
  for (int a = 0; a < NPF; ++a) acc[a][0] = acc[a][1] = acc[a][2] = 0.0;
#pragma unroll
  for (int q = 0; q < NPT; ++q) {
    double t1[3] = {0, 0, 0}, t2[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < NPF; ++a)
#pragma unroll
      for (int i = 0; i < 3; ++i) { t1[i] += R.dN[q][0][a] * xa[a][i]; t2[i] += R.dN[q][1][a] * xa[a][i]; }
    const double n0 = t1[1] * t2[2] - t1[2] * t2[1];
    const double n1 = t1[2] * t2[0] - t1[0] * t2[2];
    const double n2 = t1[0] * t2[1] - t1[1] * t2[0];
    double s0, s1, s2;                                         // traction times area element times weight
    if (pressure) {
      const double c = -v0 * R.w[q];
      s0 = c * n0; s1 = c * n1; s2 = c * n2;
    } else {
      const double c = R.w[q] * sqrt(n0 * n0 + n1 * n1 + n2 * n2);
      s0 = c * v0; s1 = c * v1; s2 = c * v2;
    }
#pragma unroll
    for (int a = 0; a < NPF; ++a) {
      const double Na = R.N[q][a];
      acc[a][0] += Na * s0; acc[a][1] += Na * s1; acc[a][2] += Na * s2;
    }
  }
  double *o = fc + (size_t)face * NPF * 3;
#pragma unroll
  for (int a = 0; a < NPF; ++a)
#pragma unroll
    for (int i = 0; i < 3; ++i) o[a * 3 + i] = lam * acc[a][i];
}

__global__ __launch_bounds__(256)
void k_surface_nodes(int n0, int n1, const int *__restrict__ lnode, const int *__restrict__ lptr,
                     const int *__restrict__ lslot, const double *__restrict__ fc, double *__restrict__ f)
{
  const int i = n0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n1) return;
  double s0 = 0, s1 = 0, s2 = 0;
  for (int p = lptr[i]; p < lptr[i + 1]; ++p) {              // (face, slot) ascending: a fixed order
    const double *c = fc + (size_t)lslot[p] * 3;
    s0 += c[0]; s1 += c[1]; s2 += c[2];
  }
  double *o = f + (size_t)lnode[i] * 3;
  o[0] += s0; o[1] += s1; o[2] += s2;
}

int launch_surface_loads(feahip_ctx *c, double *d_fv)
{
  const SurfaceLoads &S = c->surf;
  if (S.nfaces == 0) return FEAHIP_OK;
  // kernel 2 runs over the loaded nodes this rank owns (all of them unsharded)
  const auto lo = std::lower_bound(S.h_lnode.begin(), S.h_lnode.end(), c->row0);
  const auto hi = std::lower_bound(S.h_lnode.begin(), S.h_lnode.end(), c->row1);
  const int n0 = (int)(lo - S.h_lnode.begin()), n1 = (int)(hi - S.h_lnode.begin());
  if (n1 == n0) return FEAHIP_OK;
  FaceRule R;
  face_rule(S.npf, R);
  const int grid = (S.nfaces + 255) / 256;
  switch (S.npf) {
  case 3: hipLaunchKernelGGL(k_surface_faces<3>, dim3(grid), dim3(256), 0, c->stream, S.nfaces, S.d_fnode, S.d_kind, S.d_val, c->d_x, c->d_X0, c->load_factor, R, S.d_fc); break;
  case 6: hipLaunchKernelGGL(k_surface_faces<6>, dim3(grid), dim3(256), 0, c->stream, S.nfaces, S.d_fnode, S.d_kind, S.d_val, c->d_x, c->d_X0, c->load_factor, R, S.d_fc); break;
  default: hipLaunchKernelGGL(k_surface_faces<4>, dim3(grid), dim3(256), 0, c->stream, S.nfaces, S.d_fnode, S.d_kind, S.d_val, c->d_x, c->d_X0, c->load_factor, R, S.d_fc); break;
  }
  FEA_HIP_CHECK(c, hipGetLastError());
  hipLaunchKernelGGL(k_surface_nodes, dim3((n1 - n0 + 255) / 256), dim3(256), 0, c->stream, n0, n1, S.d_lnode, S.d_lptr,
                     S.d_lslot, S.d_fc, d_fv);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// ---- host: faces -> (element, local face) ---------------------------------------------------------------------------
namespace {
using FaceKey = std::array<int, FEA_SURF_MAX_NPF>;             // the node set, ascending, padded with -1
struct FaceKeyHash {
  size_t operator()(const FaceKey &k) const
  {
    unsigned long long h = 1469598103934665603ull;
    for (int v : k) h = (h ^ (unsigned)v) * 1099511628211ull;
    return (size_t)h;
  }
};
FaceKey make_key(const int *ids, int n)
{
  FaceKey k;
  k.fill(-1);
  for (int i = 0; i < n; ++i) k[i] = ids[i];
  std::sort(k.begin(), k.begin() + n);
  return k;
}
std::string face_text(int f, const int *ids, int n)
{
  std::string s = "surface face " + std::to_string(f) + " (nodes";
  for (int i = 0; i < n; ++i) s += " " + std::to_string(ids[i]);
  return s + ")";
}
}  // namespace

int resolve_surface_faces(int N, int E, int npe, const int *conn, int nfaces, int npf, const int *face_nodes,
                          int *face_elem, int *face_local, std::string &why)
{
  if (npe != 4 && npe != 10 && npe != 8) { why = "surface loads need 4-, 10- or 8-node elements"; return 0; }
  const int want = nodes_per_face(npe);
  if (npf != want) {
    why = face_text(0, face_nodes, std::min(npf, FEA_SURF_MAX_NPF)) + ": a face of a " + std::to_string(npe) +
          "-node element has " + std::to_string(want) + " nodes, not " + std::to_string(npf);
    return 0;
  }
  // the requested faces by node set; identical sets chain (the same face may carry several loads)
  std::unordered_map<FaceKey, int, FaceKeyHash> head;
  head.reserve((size_t)nfaces * 2);
  std::vector<int> next((size_t)nfaces, -1);
  std::vector<uint8_t> loaded((size_t)N, 0);
  for (int f = 0; f < nfaces; ++f) {
    const int *ids = face_nodes + (size_t)f * npf;
    for (int k = 0; k < npf; ++k)
      if (ids[k] < 0 || ids[k] >= N) { why = face_text(f, ids, npf) + ": node id outside [0, " + std::to_string(N) + ")"; return f; }
    const FaceKey key = make_key(ids, npf);
    for (int k = 1; k < npf; ++k)
      if (key[k] == key[k - 1]) { why = face_text(f, ids, npf) + ": a node appears twice"; return f; }
    for (int k = 0; k < npf; ++k) loaded[ids[k]] = 1;
    auto it = head.find(key);
    if (it == head.end()) head.emplace(key, f);
    else { int g = it->second; while (next[g] >= 0) g = next[g]; next[g] = f; }
    face_elem[f] = -1; face_local[f] = -1;
  }
  // every element face whose nodes are all loaded is looked up; matches are collected per thread, merged in order
  const int nlf = faces_per_element(npe);
  std::vector<std::vector<std::array<int, 3>>> found;
  std::mutex m;
  parallel_ranges(E, 1 << 16, [&](int lo, int hi) {
    std::vector<std::array<int, 3>> mine;
    for (int e = lo; e < hi; ++e) {
      const int *en = conn + (size_t)e * npe;
      for (int lf = 0; lf < nlf; ++lf) {
        int ids[FEA_SURF_MAX_NPF];
        bool all = true;
        for (int k = 0; k < npf && all; ++k) { ids[k] = en[face_node(npe, lf, k)]; all = loaded[ids[k]] != 0; }
        if (!all) continue;
        auto it = head.find(make_key(ids, npf));
        if (it != head.end()) mine.push_back({it->second, e, lf});
      }
    }
    std::lock_guard<std::mutex> g(m);
    found.push_back(std::move(mine));
  });
  std::vector<std::array<int, 3>> all;
  for (auto &v : found) all.insert(all.end(), v.begin(), v.end());
  std::sort(all.begin(), all.end());
  std::vector<int> count((size_t)nfaces, 0), other((size_t)nfaces, -1);
  for (const auto &m : all)
    for (int f = m[0]; f >= 0; f = next[f]) {
      if (count[f]++ == 0) { face_elem[f] = m[1]; face_local[f] = m[2]; }
      else other[f] = m[1];
    }
  for (int f = 0; f < nfaces; ++f) {
    const int *ids = face_nodes + (size_t)f * npf;
    if (count[f] == 0) { why = face_text(f, ids, npf) + ": not a face of any element"; return f; }
    if (count[f] > 1) {
      why = face_text(f, ids, npf) + ": an interior face (elements " + std::to_string(face_elem[f]) + " and " +
            std::to_string(other[f]) + ")";
      return f;
    }
  }
  return -1;
}

// the caller's faces in this context's node ids, each in its element's face order (outward normal): library ids; on a
// rank context, the faces touching an owned node, in local ids.  keep[i] = the caller's index of face i of fn.
int context_surface_faces(feahip_ctx *c, int nfaces, int npf, const int *face_nodes, std::vector<int> &fn, std::vector<int> &keep)
{
  // (a feahip_create_rank_local context is handed local ids: nothing to look up, nothing sized by the whole mesh)
  fn.clear(); keep.clear();
  if (nfaces > 0 && npf != nodes_per_face(c->npe)) {
    c->err = face_text(0, face_nodes, std::min(std::max(npf, 0), FEA_SURF_MAX_NPF)) + ": a face of a " + std::to_string(c->npe) +
             "-node element has " + std::to_string(nodes_per_face(c->npe)) + " nodes, not " + std::to_string(npf);
    return FEAHIP_EINVAL;
  }
  const bool global_faces = c->rank_own >= 0 && !c->rank_local_ids;
  const int nglobal = global_faces ? c->rank_n_global : c->N;
  std::vector<int> local;
  if (global_faces) {
    local.assign((size_t)nglobal, -1);
    for (int a = 0; a < c->N; ++a) local[c->rank_node_global[a]] = a;
  }
  for (int f = 0; f < nfaces; ++f) {
    const int *ids = face_nodes + (size_t)f * npf;
    bool owned = c->rank_own < 0, present = true;
    int mapped[FEA_SURF_MAX_NPF];
    for (int k = 0; k < npf; ++k) {
      if (ids[k] < 0 || ids[k] >= nglobal) { c->err = face_text(f, ids, npf) + ": node id outside [0, " + std::to_string(nglobal) + ")"; return FEAHIP_EINVAL; }
      if (c->rank_own >= 0) {
        mapped[k] = global_faces ? local[ids[k]] : ids[k];
        present = present && mapped[k] >= 0;
        owned = owned || (mapped[k] >= 0 && mapped[k] < c->rank_own);
      } else mapped[k] = c->perm.empty() ? ids[k] : c->perm[ids[k]];
    }
    if (!present || !owned) continue;      // a rank keeps the faces touching its nodes: their elements are all local
    fn.insert(fn.end(), mapped, mapped + npf);
    keep.push_back(f);
  }
  const int nf = (int)keep.size();
  std::vector<int> felem((size_t)nf), flocal((size_t)nf);
  if (nf > 0) {
    std::vector<int> conn_dl;
    const int *conn = c->h_conn.data();
    if (c->h_conn.empty()) {                                   // meshes whose maps keep no host copy of the elements
      conn_dl.resize((size_t)c->E * c->npe);
      FEA_HIP_CHECK(c, hipMemcpy(conn_dl.data(), c->d_conn, sizeof(int) * conn_dl.size(), hipMemcpyDeviceToHost));
      conn = conn_dl.data();
    }
    std::string why;
    const int bad = resolve_surface_faces(c->N, c->E, c->npe, conn, nf, npf, fn.data(), felem.data(), flocal.data(), why);
    if (bad >= 0) {                                            // say it in the caller's ids
      const int f = keep[bad];
      const size_t p = why.find(':');
      c->err = face_text(f, face_nodes + (size_t)f * npf, npf) + (p == std::string::npos ? "" : why.substr(p));
      return FEAHIP_EINVAL;
    }
    for (int f = 0; f < nf; ++f)                               // the element's order: outward normal
      for (int k = 0; k < npf; ++k) fn[(size_t)f * npf + k] = conn[(size_t)felem[f] * c->npe + face_node(c->npe, flocal[f], k)];
  }
  return FEAHIP_OK;
}

// the context's faces from the caller's: library ids in the element's face order, incidence lists, device copies
int set_surface_loads(feahip_ctx *c, int nfaces, int npf, const int *face_nodes, const int *kind, const double *values)
{
  if (nfaces < 0 || (nfaces > 0 && (!face_nodes || !kind || !values))) { c->err = "feahip_set_surface_loads: bad arrays"; return FEAHIP_EINVAL; }
  for (int f = 0; f < nfaces; ++f)
    if (kind[f] != FEAHIP_LOAD_PRESSURE && kind[f] != FEAHIP_LOAD_TRACTION) {
      c->err = "surface face " + std::to_string(f) + ": unknown load kind " + std::to_string(kind[f]); return FEAHIP_EINVAL;
    }
  std::vector<int> fn, fk, keep;
  std::vector<double> fv;
  if (const int rc = context_surface_faces(c, nfaces, npf, face_nodes, fn, keep)) return rc;
  const int nf = (int)keep.size();
  for (int f : keep) {
    fk.push_back(kind[f]);
    fv.insert(fv.end(), values + (size_t)f * 3, values + (size_t)f * 3 + 3);
  }
  // node -> (face, slot), nodes ascending, slots ascending inside a node
  std::vector<std::pair<int, int>> inc;
  inc.reserve(fn.size());
  for (size_t s = 0; s < fn.size(); ++s) inc.emplace_back(fn[s], (int)s);
  std::sort(inc.begin(), inc.end());
  std::vector<int> lnode, lptr, lslot;
  for (size_t i = 0; i < inc.size(); ++i) {
    if (i == 0 || inc[i].first != inc[i - 1].first) { lnode.push_back(inc[i].first); lptr.push_back((int)i); }
    lslot.push_back(inc[i].second);
  }
  lptr.push_back((int)inc.size());
  c->surf.release();
  if (nf == 0) return FEAHIP_OK;                               // cleared (or nothing on this rank): no launch at all
  SurfaceLoads &S = c->surf;
  auto up = [c](auto **dst, const auto *src, size_t n) -> int {
    FEA_HIP_CHECK(c, hipMalloc((void **)dst, sizeof(**dst) * n));
    FEA_HIP_CHECK(c, hipMemcpy(*dst, src, sizeof(**dst) * n, hipMemcpyHostToDevice));
    return FEAHIP_OK;
  };
  int rc;
  if ((rc = up(&S.d_fnode, fn.data(), fn.size())) || (rc = up(&S.d_kind, fk.data(), fk.size())) ||
      (rc = up(&S.d_val, fv.data(), fv.size())) || (rc = up(&S.d_lnode, lnode.data(), lnode.size())) ||
      (rc = up(&S.d_lptr, lptr.data(), lptr.size())) || (rc = up(&S.d_lslot, lslot.data(), lslot.size()))) {
    S.release(); return rc;
  }
  if (hipMalloc((void **)&S.d_fc, sizeof(double) * fn.size() * 3) != hipSuccess) { S.release(); c->err = "out of device memory"; return FEAHIP_ENOMEM; }
  S.nfaces = nf; S.npf = npf; S.h_lnode = std::move(lnode);
  return FEAHIP_OK;
}
