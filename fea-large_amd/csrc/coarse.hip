// coarse.hip -- the coarse level across the ranks of a sharded solve (coarse.h): host topology, the numeric setup
// A_c = Phi' K Phi and its inverse, and the three kernels of an application (restrict, coarse product, prolong-add).
//
// Every sum has a fixed shape: a workgroup sums a slice of one aggregate's rows (lanes stride over the rows, then
// wave shuffles, then the four waves in order), a second pass adds the slices in order.  No atomics anywhere, so a
// repeated setup or application gives identical bits.
#include "coarse.h"
#include "reduce_device.h"
#include <cmath>
#include <cstdlib>
#include <cstring>

static inline RankCoarse *RC(const feahip_ctx *c) { return static_cast<RankCoarse *>(c->coarse); }

// ------------------------------------------------------------------------
// the cut rule
// ------------------------------------------------------------------------
int coarse_cuts(int n_owned, int m, int *first)
{
  int mr = n_owned / FEA_COARSE_MIN_ROWS;
  if (mr < 1) mr = 1;
  if (mr > m) mr = m;
  if (first)
    for (int j = 0; j <= mr; ++j) first[j] = (int)((long long)j * n_owned / mr);
  return mr;
}

int coarse_default_m(int nranks)
{
  const char *e = getenv("FEAHIP_COARSE_AGGS");
  if (e && atoi(e) > 0) return atoi(e);
  int m = FEA_COARSE_MAX_AGGS / (nranks > 0 ? nranks : 1);
  return m < 1 ? 1 : (m > 16 ? 16 : m);
}

// ------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------
// rows [lo, hi) of slice s of ns of the rows [r0, r1)
__device__ __forceinline__ void slice_rows(int r0, int r1, int s, int ns, int &lo, int &hi)
{
  lo = r0 + (int)((long long)(r1 - r0) * s / ns);
  hi = r0 + (int)((long long)(r1 - r0) * (s + 1) / ns);
}
// component `comp` of (Phi e_c) at node a: t + w x (X0_a - c_A)
__device__ __forceinline__ double phi_e(int a, int comp, const int *agg, const double *cent, const double *X0, const double *ec)
{
  const int A = agg[a];
  const double *e = ec + (size_t)A * 6, *cA = cent + (size_t)A * 3, *x = X0 + (size_t)a * 4;
  const int j1 = comp == 2 ? 0 : comp + 1, j2 = comp == 0 ? 2 : comp - 1;          // (w x d)_i = w_j1 d_j2 - w_j2 d_j1
  return e[comp] + (e[3 + j1] * (x[j2] - cA[j2]) - e[3 + j2] * (x[j1] - cA[j1]));
}

// ------------------------------------------------------------------------
// numeric setup: slice s of the rows of pair p = (row aggregate A, column aggregate B) adds Phi_a' K_ab Phi_b over
// its blocks with b in B.  grid (slices, pairs); a block of K is read once over all pairs (its column has one
// aggregate), the column indices once per pair of its row aggregate.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_coarse_setup(int ns, const int *__restrict__ first, const int *__restrict__ pair, const int *__restrict__ agg,
                    const double *__restrict__ cent, const double *__restrict__ X0, const int *__restrict__ rowptr,
                    const int *__restrict__ colidx, const double *__restrict__ K, double *__restrict__ apart)
{
  __shared__ double scratch[4][36];
  const int s = blockIdx.x, p = blockIdx.y;
  const int A = pair[2 * p], B = pair[2 * p + 1];
  int lo, hi;
  slice_rows(first[A], first[A + 1], s, ns, lo, hi);
  const double *cA = cent + (size_t)agg[first[A]] * 3, *cB = cent + (size_t)B * 3;
  const double cb0 = cB[0], cb1 = cB[1], cb2 = cB[2];
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
  for (int a = lo + (int)threadIdx.x; a < hi; a += 256) {
    double Y[3][6];                                       // sum over b in B of K_ab Phi_b, in block order
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) Y[i][j] = 0.0;
    bool any = false;
    for (int q = rowptr[a]; q < rowptr[a + 1]; ++q) {
      const int b = colidx[q];
      if (agg[b] != B) continue;
      any = true;
      const double *k = K + (size_t)q * 9, *xb = X0 + (size_t)b * 4;
      const double d0 = xb[0] - cb0, d1 = xb[1] - cb1, d2 = xb[2] - cb2;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double k0 = k[3 * i], k1 = k[3 * i + 1], k2 = k[3 * i + 2];
        Y[i][0] += k0; Y[i][1] += k1; Y[i][2] += k2;
        Y[i][3] += k2 * d1 - k1 * d2;                     // K_ab W_b with W w = w x d
        Y[i][4] += k0 * d2 - k2 * d0;
        Y[i][5] += k1 * d0 - k0 * d1;
      }
    }
    if (!any) continue;
    const double *xa = X0 + (size_t)a * 4;
    const double d0 = xa[0] - cA[0], d1 = xa[1] - cA[1], d2 = xa[2] - cA[2];
#pragma unroll
    for (int j = 0; j < 6; ++j) {                         // Phi_a' Y: the rows of Y, then W_a' Y = d x (columns of Y)
      acc[j] += Y[0][j]; acc[6 + j] += Y[1][j]; acc[12 + j] += Y[2][j];
      acc[18 + j] += d1 * Y[2][j] - d2 * Y[1][j];
      acc[24 + j] += d2 * Y[0][j] - d0 * Y[2][j];
      acc[30 + j] += d0 * Y[1][j] - d1 * Y[0][j];
    }
  }
  const double r = block_sums<36>(acc, scratch);
  if (threadIdx.x < 36) apart[((size_t)p * ns + s) * 36 + threadIdx.x] = r;
}

// second pass: the slices of a pair in order, into the dense A_c (this rank's rows of it; the rest stays zero)
__global__ void k_coarse_setup_sum(int ns, int nc, const int *__restrict__ first, const int *__restrict__ pair,
                                   const int *__restrict__ agg, const double *__restrict__ apart, double *__restrict__ Ad)
{
  const int p = blockIdx.x, k = threadIdx.x;
  if (k >= 36) return;
  double v = 0;
  for (int s = 0; s < ns; ++s) v += apart[((size_t)p * ns + s) * 36 + k];
  const int gA = agg[first[pair[2 * p]]], B = pair[2 * p + 1];
  Ad[(size_t)(6 * gA + k / 6) * nc + 6 * B + k % 6] = v;
}

// ------------------------------------------------------------------------
// an application
// ------------------------------------------------------------------------
// slice sums of Phi' r: grid (slices, this rank's aggregates)
__global__ __launch_bounds__(256)
void k_coarse_restrict(int ns, const int *__restrict__ first, const int *__restrict__ agg, const double *__restrict__ cent,
                       const double *__restrict__ X0, const double *__restrict__ r, double *__restrict__ rpart)
{
  __shared__ double scratch[4][6];
  const int s = blockIdx.x, A = blockIdx.y;
  int lo, hi;
  slice_rows(first[A], first[A + 1], s, ns, lo, hi);
  const double *cA = cent + (size_t)agg[first[A]] * 3;
  const double c0 = cA[0], c1 = cA[1], c2 = cA[2];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int a = lo + (int)threadIdx.x; a < hi; a += 256) {
    const double *x = X0 + (size_t)a * 4, *v = r + (size_t)a * 3;
    const double d0 = x[0] - c0, d1 = x[1] - c1, d2 = x[2] - c2, v0 = v[0], v1 = v[1], v2 = v[2];
    acc[0] += v0; acc[1] += v1; acc[2] += v2;
    acc[3] += d1 * v2 - d2 * v1; acc[4] += d2 * v0 - d0 * v2; acc[5] += d0 * v1 - d1 * v0;
  }
  const double t = block_sums<6>(acc, scratch);
  if (threadIdx.x < 6) rpart[((size_t)A * ns + s) * 6 + threadIdx.x] = t;
}

// r_c: this rank's slots from the slice sums in order, zero in every other rank's (the all-reduce fills them)
__global__ void k_coarse_restrict_sum(int ns, int nc, int agg0, int m_loc, const double *__restrict__ rpart, double *__restrict__ rc)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  const int A = i / 6 - agg0;
  double v = 0;
  if (A >= 0 && A < m_loc)
    for (int s = 0; s < ns; ++s) v += rpart[((size_t)A * ns + s) * 6 + i % 6];
  rc[i] = v;
}

// e_c = A_c^-1 r_c with the stored inverse: one wave per row
__global__ __launch_bounds__(256)
void k_coarse_solve(int nc, const double *__restrict__ Ainv, const double *__restrict__ rc, double *__restrict__ ec)
{
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nc) return;
  const double *m = Ainv + (size_t)row * nc;
  double v = 0;
  for (int j = lane; j < nc; j += 64) v += m[j] * rc[j];
  v = wave_sum_all(v);
  if (lane == 0) ec[row] = v;
}

// z += Phi e_c on the owned rows (dofs [i0, i1))
__global__ __launch_bounds__(256)
void k_coarse_prolong_add(int i0, int i1, const int *__restrict__ agg, const double *__restrict__ cent,
                          const double *__restrict__ X0, const double *__restrict__ ec, double *__restrict__ z)
{
  for (int i = i0 + blockIdx.x * 256 + threadIdx.x; i < i1; i += gridDim.x * 256) z[i] += phi_e(i / 3, i % 3, agg, cent, X0, ec);
}

// znew = z + Phi e_c on the owned rows, partial sums of r . znew: k_copy_dot (kernels_solve.hip) with the correction
__global__ __launch_bounds__(256)
void k_coarse_copy_dot(int i0, int i1, const double *__restrict__ z, const double *__restrict__ r, double *__restrict__ znew,
                       double *__restrict__ part, const int *__restrict__ flag, const int *__restrict__ agg,
                       const double *__restrict__ cent, const double *__restrict__ X0, const double *__restrict__ ec)
{
  __shared__ double scratch[4][1];
  if (flag && flag[0] != 0) return;
  double v[1] = {0};
  for (int i = i0 + blockIdx.x * 256 + threadIdx.x; i < i1; i += gridDim.x * 256) {
    const double zi = z[i] + phi_e(i / 3, i % 3, agg, cent, X0, ec);
    znew[i] = zi; v[0] += r[i] * zi;
  }
  const double s = block_sums<1>(v, scratch);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
int ensure_comm_stream(feahip_ctx *c)
{
  if (!c->comm_stream) {                             // (the transports create the three together as well)
    FEA_HIP_CHECK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    FEA_HIP_CHECK(c, hipEventCreateWithFlags(&c->ev_packed, hipEventDisableTiming));
    FEA_HIP_CHECK(c, hipEventCreateWithFlags(&c->ev_unpacked, hipEventDisableTiming));
  }
  return FEAHIP_OK;
}

int ensure_vred(feahip_ctx *c, size_t n)
{
  if (c->vred_cap >= n) return FEAHIP_OK;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  if (c->comm_stream) FEA_HIP_CHECK(c, hipStreamSynchronize(c->comm_stream));
  if (c->d_vred) (void)hipFree(c->d_vred);
  c->d_vred = nullptr; c->vred_cap = 0;
  FEA_HIP_CHECK(c, hipMalloc((void **)&c->d_vred, sizeof(double) * n));
  c->vred_cap = n;
  return FEAHIP_OK;
}

static int to_device(feahip_ctx *c, void *dst, const void *src, size_t bytes)
{
  if (!bytes) return FEAHIP_OK;
  FEA_HIP_CHECK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}
static int to_host(feahip_ctx *c, void *dst, const void *src, size_t bytes)
{
  if (!bytes) return FEAHIP_OK;
  FEA_HIP_CHECK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

void coarse_destroy(feahip_ctx *c)
{
  RankCoarse *h = RC(c);
  if (h) {
    (void)hipSetDevice(c->device);
    dev_free({h->d_agg, h->d_first, h->d_pair, h->d_cent, h->d_apart, h->d_Ainv, h->d_rpart, h->d_ec});
    if (h->ev_r) (void)hipEventDestroy(h->ev_r);
    if (h->ev_ec) (void)hipEventDestroy(h->ev_ec);
    delete h;
    c->coarse = nullptr;
  }
  if (c->d_vred) { (void)hipFree(c->d_vred); c->d_vred = nullptr; c->vred_cap = 0; }
}

// every rank's vector v (n doubles, its own slots filled, zero elsewhere) summed over the ranks, back in v
static int host_allreduce(std::vector<feahip_ctx *> &R, Transport *T, std::vector<std::vector<double>> &v, size_t n)
{
  int rc;
  if (!T) return FEAHIP_OK;
  size_t k = 0;
  FOR_RANKS(c) { if ((rc = to_device(c, c->d_vred, v[k++].data(), sizeof(double) * n))) return rc; }
  if ((rc = T->allreduce_vec(R, n, false))) return rc;
  k = 0;
  FOR_RANKS(c) { if ((rc = to_host(c, v[k++].data(), c->d_vred, sizeof(double) * n))) return rc; }
  return FEAHIP_OK;
}

static bool topology_current(const feahip_ctx *c, Transport *T)
{
  const RankCoarse *h = RC(c);
  return h && h->row0 == c->row0 && h->row1 == c->row1 && h->tr == (const void *)T && h->nranks == (T ? c->nranks : 1) &&
         h->m == coarse_default_m(h->nranks);
}

// aggregates of every rank, centroids of all, the aggregate of every halo node: two vector all-reduces and one halo
// exchange (of p, which a solve overwrites at its start)
static int coarse_topology(std::vector<feahip_ctx *> &R, Transport *T)
{
  int rc;
  const size_t nR = R.size();
  const int nranks = T ? R[0]->nranks : 1;
  std::vector<std::vector<int>> first(nR);
  std::vector<std::vector<double>> v(nR);
  size_t k = 0;
  FOR_RANKS(c) {
    coarse_destroy(c);
    RankCoarse *h = new RankCoarse();
    c->coarse = h;
    h->row0 = c->row0; h->row1 = c->row1; h->tr = T; h->nranks = nranks; h->m = coarse_default_m(nranks);
    if (h->m * nranks > FEA_COARSE_MAX_AGGS) { c->err = "coarse level: more than 128 aggregates over the ranks (FEAHIP_COARSE_AGGS)"; return FEAHIP_EINVAL; }
    if (c->row1 <= c->row0) { c->err = "coarse level: the rank owns no row"; return FEAHIP_ESTATE; }
    first[k].resize((size_t)h->m + 1);
    h->m_loc = coarse_cuts(c->row1 - c->row0, h->m, first[k].data());
    first[k].resize((size_t)h->m_loc + 1);
    for (int &f : first[k]) f += c->row0;
    if ((rc = ensure_comm_stream(c))) return rc;
    if ((rc = ensure_vred(c, 1024))) return rc;
    FEA_HIP_CHECK(c, hipEventCreateWithFlags(&h->ev_r, hipEventDisableTiming));
    FEA_HIP_CHECK(c, hipEventCreateWithFlags(&h->ev_ec, hipEventDisableTiming));
    v[k].assign((size_t)nranks, 0.0);
    v[k][T ? c->rank : 0] = h->m_loc;
    ++k;
  }
  if ((rc = host_allreduce(R, T, v, (size_t)nranks))) return rc;
  k = 0;
  FOR_RANKS(c) {
    RankCoarse *h = RC(c);
    const int me = T ? c->rank : 0;
    h->agg0 = 0; h->nagg = 0;
    for (int s = 0; s < nranks; ++s) { if (s < me) h->agg0 += (int)v[k][s]; h->nagg += (int)v[k][s]; }
    h->nc = 6 * h->nagg;
    if ((rc = ensure_vred(c, (size_t)h->nc * h->nc))) return rc;
    // centroids of this rank's aggregates: the mean of X0 over its nodes, in row order
    std::vector<double> X0((size_t)c->N * 4);
    if ((rc = to_host(c, X0.data(), c->d_X0, sizeof(double) * X0.size()))) return rc;
    v[k].assign((size_t)3 * h->nagg, 0.0);
    h->h_agg.assign((size_t)c->N, -1);
    for (int A = 0; A < h->m_loc; ++A) {
      double s[3] = {0, 0, 0};
      for (int a = first[k][A]; a < first[k][A + 1]; ++a) {
        h->h_agg[a] = h->agg0 + A;
        for (int d = 0; d < 3; ++d) s[d] += X0[(size_t)a * 4 + d];
      }
      for (int d = 0; d < 3; ++d) v[k][(size_t)3 * (h->agg0 + A) + d] = s[d] / (first[k][A + 1] - first[k][A]);
    }
    ++k;
  }
  if ((rc = host_allreduce(R, T, v, (size_t)3 * RC(R[0])->nagg))) return rc;
  k = 0;
  FOR_RANKS(c) { RC(c)->h_cent = v[k++]; }
  if (T) {                                            // the halo nodes' aggregates: id + 1 in the x slot of p, 0 = none
    FOR_RANKS(c) {
      RankCoarse *h = RC(c);
      std::vector<double> p((size_t)c->ndof, 0.0);
      for (int a = c->row0; a < c->row1; ++a) p[(size_t)a * 3] = h->h_agg[a] + 1;
      if ((rc = to_device(c, c->d_p, p.data(), sizeof(double) * p.size()))) return rc;
    }
    if ((rc = T->exchange(R, 0))) return rc;
    FOR_RANKS(c) {
      RankCoarse *h = RC(c);
      std::vector<double> p((size_t)c->ndof);
      if ((rc = to_host(c, p.data(), c->d_p, sizeof(double) * p.size()))) return rc;
      for (int a = 0; a < c->N; ++a)
        if (a < c->row0 || a >= c->row1) {
          const int id = (int)p[(size_t)a * 3] - 1;
          h->h_agg[a] = id >= 0 && id < h->nagg ? id : -1;
        }
      FEA_HIP_CHECK(c, hipMemsetAsync(c->d_p, 0, sizeof(double) * (size_t)c->ndof, c->stream));
    }
  }
  k = 0;
  FOR_RANKS(c) {
    RankCoarse *h = RC(c);
    // (row aggregate, column aggregate) pairs of the owned rows, column aggregates ascending
    std::vector<int> pair;
    std::vector<uint8_t> seen((size_t)h->nagg);
    int rows_max = 1;
    for (int A = 0; A < h->m_loc; ++A) {
      std::fill(seen.begin(), seen.end(), 0);
      for (int q = c->h_rowptr[first[k][A]]; q < c->h_rowptr[first[k][A + 1]]; ++q) {
        const int B = h->h_agg[c->h_colidx[q]];
        if (B >= 0) seen[B] = 1;
      }
      for (int B = 0; B < h->nagg; ++B) if (seen[B]) { pair.push_back(A); pair.push_back(B); }
      rows_max = std::max(rows_max, first[k][A + 1] - first[k][A]);
    }
    h->npair = (int)pair.size() / 2;
    h->ns_a = std::min(FEA_COARSE_SLICES, std::max(1, (rows_max + 511) / 512));
    h->ns_r = std::min(FEA_COARSE_SLICES, std::max(1, (rows_max + 2047) / 2048));
    auto up = [&](auto **dst, const auto &src) -> int {
      FEA_HIP_CHECK(c, hipMalloc((void **)dst, sizeof(src[0]) * (src.size() ? src.size() : 1)));
      return to_device(c, *dst, src.data(), sizeof(src[0]) * src.size());
    };
    if ((rc = up(&h->d_agg, h->h_agg))) return rc;
    if ((rc = up(&h->d_first, first[k]))) return rc;
    if ((rc = up(&h->d_pair, pair))) return rc;
    if ((rc = up(&h->d_cent, h->h_cent))) return rc;
    FEA_HIP_CHECK(c, hipMalloc((void **)&h->d_apart, sizeof(double) * 36 * (size_t)std::max(1, h->npair) * h->ns_a));
    FEA_HIP_CHECK(c, hipMalloc((void **)&h->d_Ainv, sizeof(double) * (size_t)h->nc * h->nc));
    FEA_HIP_CHECK(c, hipMalloc((void **)&h->d_rpart, sizeof(double) * 6 * (size_t)h->m_loc * h->ns_r));
    FEA_HIP_CHECK(c, hipMalloc((void **)&h->d_ec, sizeof(double) * (size_t)h->nc));
    ++k;
  }
  return FEAHIP_OK;
}

// inv = A^-1 by Cholesky of the symmetric part of A (n x n, row-major), in double.  Returns -1, or the index of the
// first pivot that is not positive (coarse.h: FEA_COARSE_PIVOT_TOL).
static int spd_inverse(const std::vector<double> &A, int n, std::vector<double> &inv)
{
  std::vector<double> L((size_t)n * n, 0.0), U((size_t)n * n, 0.0);      // U = L' (rows of it are columns of L)
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) L[(size_t)i * n + j] = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
  for (int j = 0; j < n; ++j) {
    double *lj = L.data() + (size_t)j * n;
    const double ajj = lj[j];
    double d = ajj;
    for (int k = 0; k < j; ++k) d -= lj[k] * lj[k];
    if (!(d > FEA_COARSE_PIVOT_TOL * ajj) || !(ajj > 0)) return j;
    const double ljj = sqrt(d);
    lj[j] = ljj;
    for (int i = j + 1; i < n; ++i) {
      double *li = L.data() + (size_t)i * n;
      double s = li[j];
      for (int k = 0; k < j; ++k) s -= li[k] * lj[k];
      li[j] = s / ljj;
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) U[(size_t)j * n + i] = L[(size_t)i * n + j];
  inv.assign((size_t)n * n, 0.0);
  parallel_ranges(n, 64, [&](int lo, int hi) {               // column c of the inverse: L y = e_c, L' x = y
    std::vector<double> y((size_t)n);
    for (int c = lo; c < hi; ++c) {
      for (int i = 0; i < c; ++i) y[i] = 0.0;
      for (int i = c; i < n; ++i) {
        const double *li = L.data() + (size_t)i * n;
        double s = i == c ? 1.0 : 0.0;
        for (int k = c; k < i; ++k) s -= li[k] * y[k];
        y[i] = s / li[i];
      }
      for (int i = n - 1; i >= 0; --i) {
        const double *ui = U.data() + (size_t)i * n;
        double s = y[i];
        for (int k = i + 1; k < n; ++k) s -= ui[k] * y[k];
        y[i] = s / ui[i];
      }
      for (int i = 0; i < n; ++i) inv[(size_t)i * n + c] = y[i];
    }
  });
  return -1;
}

static int coarse_numeric(std::vector<feahip_ctx *> &R, Transport *T)
{
  int rc;
  FOR_RANKS(c) {
    RankCoarse *h = RC(c);
    h->numeric_valid = false;
    FEA_HIP_CHECK(c, hipMemsetAsync(c->d_vred, 0, sizeof(double) * (size_t)h->nc * h->nc, c->stream));
    if (h->npair > 0) {
      hipLaunchKernelGGL(k_coarse_setup, dim3(h->ns_a, h->npair), dim3(256), 0, c->stream, h->ns_a, h->d_first, h->d_pair, h->d_agg,
                         h->d_cent, c->d_X0, c->d_rowptr, c->d_colidx, c->d_K, h->d_apart);
      hipLaunchKernelGGL(k_coarse_setup_sum, dim3(h->npair), dim3(64), 0, c->stream, h->ns_a, h->nc, h->d_first, h->d_pair, h->d_agg,
                         h->d_apart, c->d_vred);
    }
    FEA_HIP_CHECK(c, hipGetLastError());
  }
  const int nc = RC(R[0])->nc;
  if (T && (rc = T->allreduce_vec(R, (size_t)nc * nc, false))) return rc;
  std::vector<double> last_A, last_inv;                 // the ranks of one process hold the same bits: inverted once
  int bad = -1;
  FOR_RANKS(c) {
    RankCoarse *h = RC(c);
    h->h_A.resize((size_t)nc * nc);
    if ((rc = to_host(c, h->h_A.data(), c->d_vred, sizeof(double) * h->h_A.size()))) return rc;
    if (last_A != h->h_A) {
      if ((bad = spd_inverse(h->h_A, nc, last_inv)) >= 0) break;
      last_A = h->h_A;
    }
    if ((rc = to_device(c, h->d_Ainv, last_inv.data(), sizeof(double) * last_inv.size()))) return rc;
    h->numeric_valid = true; h->num_epoch = c->k_epoch; h->num_bc = c->k_bc; ++h->setups;
  }
  if (bad >= 0) {
    const std::string msg = "coarse level: A_c = Phi' K Phi is not positive definite: pivot " + std::to_string(bad % 6) +
                            " of aggregate " + std::to_string(bad / 6) + " is not positive (an unconstrained body, or a degenerate aggregate)";
    for (feahip_ctx *c : R) { c->err = msg; RC(c)->numeric_valid = false; }
    return FEAHIP_ESTATE;
  }
  return FEAHIP_OK;
}

int coarse_prepare(std::vector<feahip_ctx *> &R, Transport *T)
{
  int rc;
  bool topo = true, num = true;
  for (feahip_ctx *c : R) {
    if (!c->k_valid) { c->err = "coarse level: no stiffness matrix assembled"; return FEAHIP_ESTATE; }
    if (!topology_current(c, T)) topo = false;
  }
  if (!topo && (rc = coarse_topology(R, T))) {
    for (feahip_ctx *c : R) { if (c->err.empty()) c->err = "coarse level: topology setup failed on another rank"; }
    FOR_RANKS(c) coarse_destroy(c);
    return rc;
  }
  for (feahip_ctx *c : R) {
    const RankCoarse *h = RC(c);
    if (!(h->numeric_valid && h->num_epoch == c->k_epoch && h->num_bc == c->k_bc)) num = false;
  }
  return num ? FEAHIP_OK : coarse_numeric(R, T);
}

int coarse_enq_restrict(feahip_ctx *c, const double *r)
{
  RankCoarse *h = RC(c);
  FEA_HIP_CHECK(c, hipEventRecord(h->ev_r, c->stream));
  FEA_HIP_CHECK(c, hipStreamWaitEvent(c->comm_stream, h->ev_r, 0));
  hipLaunchKernelGGL(k_coarse_restrict, dim3(h->ns_r, h->m_loc), dim3(256), 0, c->comm_stream, h->ns_r, h->d_first, h->d_agg, h->d_cent,
                     c->d_X0, r, h->d_rpart);
  hipLaunchKernelGGL(k_coarse_restrict_sum, dim3((h->nc + 255) / 256), dim3(256), 0, c->comm_stream, h->ns_r, h->nc, h->agg0, h->m_loc,
                     h->d_rpart, c->d_vred);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int coarse_allreduce_rc(std::vector<feahip_ctx *> &R, Transport *T)
{
  return T ? T->allreduce_vec(R, (size_t)RC(R[0])->nc, true) : FEAHIP_OK;
}

int coarse_enq_solve(feahip_ctx *c)
{
  RankCoarse *h = RC(c);
  hipLaunchKernelGGL(k_coarse_solve, dim3((h->nc + 3) / 4), dim3(256), 0, c->comm_stream, h->nc, h->d_Ainv, c->d_vred, h->d_ec);
  FEA_HIP_CHECK(c, hipGetLastError());
  FEA_HIP_CHECK(c, hipEventRecord(h->ev_ec, c->comm_stream));
  return FEAHIP_OK;
}

static int owned_grid(const feahip_ctx *c)
{
  const int g = (c->row1 - c->row0 + 255) / 256;             // the grid of the PCG's vector kernels (kernels_solve.hip: vgrid)
  return g < FEA_RED_BLOCKS ? (g > 0 ? g : 1) : FEA_RED_BLOCKS;
}

int coarse_enq_prolong_add(feahip_ctx *c, double *z)
{
  RankCoarse *h = RC(c);
  FEA_HIP_CHECK(c, hipStreamWaitEvent(c->stream, h->ev_ec, 0));
  hipLaunchKernelGGL(k_coarse_prolong_add, dim3(owned_grid(c)), dim3(256), 0, c->stream, 3 * c->row0, 3 * c->row1, h->d_agg, h->d_cent,
                     c->d_X0, h->d_ec, z);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int coarse_enq_copy_dot(feahip_ctx *c, const double *z, const double *r, double *znew, double *part, const int *flag)
{
  RankCoarse *h = RC(c);
  FEA_HIP_CHECK(c, hipStreamWaitEvent(c->stream, h->ev_ec, 0));
  hipLaunchKernelGGL(k_coarse_copy_dot, dim3(owned_grid(c)), dim3(256), 0, c->stream, 3 * c->row0, 3 * c->row1, z, r, znew, part, flag,
                     h->d_agg, h->d_cent, c->d_X0, h->d_ec);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int coarse_export_info(feahip_ctx *c, long long *o, int *agg_of_owned_row, double *centroids)
{
  const RankCoarse *h = RC(c);
  o[0] = h->nagg; o[1] = h->agg0; o[2] = h->m_loc; o[3] = h->nc; o[4] = h->setups; o[5] = c->row1 - c->row0; o[6] = h->m; o[7] = h->npair;
  if (agg_of_owned_row) std::copy(h->h_agg.begin() + c->row0, h->h_agg.begin() + c->row1, agg_of_owned_row);
  if (centroids) std::copy(h->h_cent.begin(), h->h_cent.end(), centroids);
  return FEAHIP_OK;
}

int coarse_export_matrix(feahip_ctx *c, double *A)
{
  const RankCoarse *h = RC(c);
  std::copy(h->h_A.begin(), h->h_A.end(), A);
  return FEAHIP_OK;
}
