// kernels_mass.hip -- consistent mass matrix, body force and the vector kernels of the Newmark steps on gfx950.
//
// M_ab = sum_e rho_e sum_g w_g det J0_g N_a(g) N_b(g), times the 3x3 identity: ONE double per block of K's block-CSR
// pattern (m[nnzb], the owned window [kb0, kb1) as for d_K).  It is assembled once per feahip_set_mass by two kernels
// without atomics on the sums: k_mass_elements evaluates rho w det J0 at the mass points of every element, and
// k_mass_blocks gives every owned block a lane that walks the (row, element) visits of its chunk (GenericMaps, the
// row-owner assembly's incidence lists) in their stored order and adds the elements that hold both nodes of the block:
// a fixed summation order, the same bits on every call.
//
// Two kernels are on the path of every Newton iteration of a dynamic step:
//   k_mass_add       K += c M on the three diagonal entries of every owned block, streamed as 16-byte pieces of K
//   k_mass_residual  f -= a0 M (x - xt), a wave per SpMV chunk like k_spmv's row loop (k_mass_product, the same body, is
//                    y = M v: feahip_mass_spmv, the body force)
// and two pointwise kernels frame a step (k_newmark_predict, k_newmark_correct: 16-byte pieces of the 32-byte node
// records).  Nothing here is launched on a context without a mass.
//
// Explicit (central-difference) steps use a DIAGONAL mass instead: ml[N], one double per node, HRZ-lumped per element
// (k_mass_lump: m_e d_a / sum_b d_b with d_a = sum_g rho w det J0 N_a^2 -- positive on every element type and the
// element's mass exactly; the row sum of a 10-node tetrahedron is <= 0 at its corners).  It is built on first use by
// lump_ensure and framed by two pointwise kernels per step, k_explicit_kick and k_explicit_finish.  A context that
// never makes an explicit call allocates and launches none of it.  The kernels of Rayleigh damping are in
// kernels_damping.hip; only the damped finish of an explicit step (k_explicit_finish<.., DAMP>) is here.
#include "feahip_internal.h"
#include "reduce_device.h"
#include <cmath>
#include <cstring>

struct MassTable {                   // the mass rule, tabulated by the host (one upload per feahip_set_mass)
  double w[FEA_MAX_GAUSS];
  double N[FEA_MAX_GAUSS][FEA_MAX_NPE];
  double dN[FEA_MAX_GAUSS][3][FEA_MAX_NPE];
};

typedef double mass_v2d __attribute__((ext_vector_type(2)));

// wdet[e][g] = rho_e w_g det J0_g; *bad = the lowest element with det J0 <= 0 (or NaN) at a mass point
__global__ __launch_bounds__(256)
void k_mass_elements(int E, int npe, int Gm, const int *__restrict__ conn, const double *__restrict__ X0,
                     const MassTable *__restrict__ tab, const double *__restrict__ rho, int n_rho,
                     const uint8_t *__restrict__ elem_mat, double *__restrict__ wdet, int *bad)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const double r = rho[n_rho > 1 ? elem_mat[e] : 0];
  for (int g = 0; g < Gm; ++g) {
    double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int k = 0; k < npe; ++k) {
      const double *X = X0 + (size_t)conn[(size_t)e * npe + k] * 4;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double d = tab->dN[g][i][k];
#pragma unroll
        for (int j = 0; j < 3; ++j) J[i][j] += d * X[j];
      }
    }
    const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                       J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    if (!(det > 0.0)) atomicMin(bad, e);
    wdet[(size_t)e * Gm + g] = r * tab->w[g] * det;
  }
}

// One wave per chunk of owned rows; lane k takes the blocks k, k + 64, ... of the chunk.  For its block (a, b) the lane
// walks the chunk's visits (element, local node) in stored order, keeps those of row a whose element also holds b, and
// adds sum_g wdet[e][g] N_la(g) N_lb(g).
__global__ __launch_bounds__(64 * FEA_WAVES_PER_WG)
void k_mass_blocks(int chunk0, int nchunks, const int *__restrict__ chunk, const int *__restrict__ rowptr,
                   const int *__restrict__ colidx, const int *__restrict__ incptr, const uint32_t *__restrict__ inc,
                   const int *__restrict__ conn, int npe, int Gm, const MassTable *__restrict__ tab,
                   const double *__restrict__ wdet, double *__restrict__ m)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
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
        const double *wd = wdet + (size_t)e * Gm;
        double s = 0.0;
        for (int g = 0; g < Gm; ++g) s += wd[g] * tab->N[g][la] * tab->N[g][lb];
        acc += s;
      }
      m[q] = acc;
    }
  }
}

// K += c M.  The owned values of K are the contiguous run [v0, v1) of GLOBAL value indices (9 per block) and even
// global indices are 16-byte aligned (feahip_internal.h): a lane takes the piece (2p, 2p + 1), adds c m[block] to the
// entries 0, 4, 8 of a block that fall into it and stores the piece only when it holds one (two pieces in three do).
__global__ __launch_bounds__(256)
void k_mass_add(long long v0, long long v1, double coef, const double *__restrict__ m, double *__restrict__ K)
{
  const long long pl = v0 >> 1, ph = (v1 + 1) >> 1;
  const long long stride = (long long)gridDim.x * 256;
  for (long long p = pl + (long long)blockIdx.x * 256 + threadIdx.x; p < ph; p += stride) {
    const long long va = 2 * p, q = va / 9;
    const int r = (int)(va - q * 9);                       // entry of block q the first value of the piece is
    const bool d0 = r == 0 || r == 4 || r == 8, d1 = r == 3 || r == 7 || r == 8;
    if (!d0 && !d1) continue;
    const long long qb = q + (r == 8 ? 1 : 0);             // block of the second value
    if (va >= v0 && va + 1 < v1) {
      mass_v2d *kp = reinterpret_cast<mass_v2d *>(K + va);
      mass_v2d k2 = *kp;
      if (d0) k2.x += coef * m[q];
      if (d1) k2.y += coef * m[qb];
      *kp = k2;
    } else {                                               // a piece that reaches over an end of the window
      if (d0 && va >= v0) K[va] += coef * m[q];
      if (d1 && va + 1 < v1) K[va + 1] += coef * m[qb];
    }
  }
}

// The row loop of k_spmv with one double per block: a wave owns a chunk, lane k takes its blocks k and k + 64, reads
// m, the column and the 32-byte node record(s) of the column as 16-byte loads, leaves m (x_b - xt_b) in LDS, and lane
// (row, i) adds its row's partial products in block order.
//   SUB: f[row] -= a0 * sum_b m_rb (x_b - xt_b)        (the inertia term of a Newton iteration)
//  !SUB: y[row]  =      sum_b m_rb x_b                 (feahip_mass_spmv, the body force)
template <bool SUB>
__device__ __forceinline__ void mass_rows_body(int chunk0, int nchunks, const int *__restrict__ chunk, const int *__restrict__ rowptr,
                 const int *__restrict__ colidx, const double *__restrict__ m, const double *__restrict__ x,
                 const double *__restrict__ xt, double a0, double *__restrict__ y)
{
  static_assert(FEA_CHUNK_ROWS * 3 <= 64, "one lane per (row, component) of a chunk");
  static_assert(FEA_CHUNK_BLOCKS <= 128, "a lane takes the blocks k and k + 64 of a chunk");
  __shared__ double sP[FEA_WAVES_PER_WG][FEA_CHUNK_BLOCKS * 3];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double *tP = sP[wave];
  auto column = [&](int q, double (&d)[3]) {
    const double mm = m[q];
    const size_t col = (size_t)colidx[q];
    const mass_v2d *xp = reinterpret_cast<const mass_v2d *>(x + col * 4);
    const mass_v2d xa = xp[0], xb = xp[1];
    d[0] = xa.x; d[1] = xa.y; d[2] = xb.x;
    if constexpr (SUB) {
      const mass_v2d *tp = reinterpret_cast<const mass_v2d *>(xt + col * 4);
      const mass_v2d ta = tp[0], tb = tp[1];
      d[0] -= ta.x; d[1] -= ta.y; d[2] -= tb.x;
    }
    d[0] *= mm; d[1] *= mm; d[2] *= mm;
  };
  for (int ch = chunk0 + blockIdx.x * FEA_WAVES_PER_WG + wave; ch < chunk0 + nchunks; ch += gridDim.x * FEA_WAVES_PER_WG) {
    const int r0 = chunk[ch], r1 = chunk[ch + 1];
    const int b0 = rowptr[r0], nb = rowptr[r1] - b0;
    if (nb > FEA_CHUNK_BLOCKS) {
      // a row longer than the tile has a chunk of its own (pattern.cpp): the lanes stride over its blocks and their
      // sums meet in a butterfly -- any length, fixed order
      double s[3] = {0, 0, 0};
      for (int k = lane; k < nb; k += 64) {
        double d[3];
        column(b0 + k, d);
        s[0] += d[0]; s[1] += d[1]; s[2] += d[2];
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        s[0] += __shfl_xor(s[0], off, 64); s[1] += __shfl_xor(s[1], off, 64); s[2] += __shfl_xor(s[2], off, 64);
      }
      if (lane < 3) {
        const double acc = lane == 0 ? s[0] : lane == 1 ? s[1] : s[2];
        if constexpr (SUB) y[(size_t)r0 * 3 + lane] -= a0 * acc; else y[(size_t)r0 * 3 + lane] = acc;
      }
      continue;
    }
    int kb = 0, ke = 0;
    if (lane < (r1 - r0) * 3) { kb = rowptr[r0 + lane / 3] - b0; ke = rowptr[r0 + lane / 3 + 1] - b0; }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k < nb) {
        double d[3];
        column(b0 + k, d);
        tP[k * 3 + 0] = d[0]; tP[k * 3 + 1] = d[1]; tP[k * 3 + 2] = d[2];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (lane < (r1 - r0) * 3) {
      const int i = lane % 3;
      double acc = 0;
      for (int k = kb; k < ke; ++k) acc += tP[k * 3 + i];
      if constexpr (SUB) y[(size_t)r0 * 3 + lane] -= a0 * acc; else y[(size_t)r0 * 3 + lane] = acc;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
}

__global__ __launch_bounds__(64 * FEA_WAVES_PER_WG)
void k_mass_residual(int chunk0, int nchunks, const int *chunk, const int *rowptr, const int *colidx, const double *m,
                     const double *x, const double *xt, double a0, double *f)
{
  mass_rows_body<true>(chunk0, nchunks, chunk, rowptr, colidx, m, x, xt, a0, f);
}

__global__ __launch_bounds__(64 * FEA_WAVES_PER_WG)
void k_mass_product(int chunk0, int nchunks, const int *chunk, const int *rowptr, const int *colidx, const double *m,
                    const double *v, double *y)
{
  mass_rows_body<false>(chunk0, nchunks, chunk, rowptr, colidx, m, v, (const double *)nullptr, 0.0, y);
}

// f += lf * body on the dofs [i0, i1)
__global__ __launch_bounds__(256)
void k_body_add(int i0, int i1, double lf, const double *__restrict__ body, double *__restrict__ f)
{
  const int i = i0 + blockIdx.x * 256 + threadIdx.x;
  if (i < i1) f[i] += lf * body[i];
}

// Newmark predictor over the n 16-byte pieces of the node records: xt = x + dt v + c a, vt = v + d a
__global__ __launch_bounds__(256)
void k_newmark_predict(size_t n, double dt, double ca, double da, const mass_v2d *__restrict__ x,
                       const mass_v2d *__restrict__ v, const mass_v2d *__restrict__ a, mass_v2d *__restrict__ xt,
                       mass_v2d *__restrict__ vt)
{
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const mass_v2d xi = x[i], vi = v[i], ai = a[i];
    xt[i] = xi + dt * vi + ca * ai;
    vt[i] = vi + da * ai;
  }
}

// Newmark corrector: a = a0 (x - xt), v = vt + gdt a
__global__ __launch_bounds__(256)
void k_newmark_correct(size_t n, double a0, double gdt, const mass_v2d *__restrict__ x, const mass_v2d *__restrict__ xt,
                       const mass_v2d *__restrict__ vt, mass_v2d *__restrict__ v, mass_v2d *__restrict__ a)
{
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const mass_v2d ai = a0 * (x[i] - xt[i]);
    a[i] = ai;
    v[i] = vt[i] + gdt * ai;
  }
}

// HRZ lumped mass.  A wave per chunk, one lane per row: the lane walks the chunk's (element, local node) visits in stored
// order, keeps those of its row and adds m_e d_la / sum_k d_k -- no atomics, a fixed order, the same bits on every call.
__global__ __launch_bounds__(64 * FEA_WAVES_PER_WG)
void k_mass_lump(int chunk0, int nchunks, const int *__restrict__ chunk, const int *__restrict__ incptr,
                 const uint32_t *__restrict__ inc, const int *__restrict__ conn, int npe, int Gm,
                 const MassTable *__restrict__ tab, const double *__restrict__ wdet, double *__restrict__ ml)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int ch = chunk0 + blockIdx.x * FEA_WAVES_PER_WG + wave; ch < chunk0 + nchunks; ch += gridDim.x * FEA_WAVES_PER_WG) {
    const int r0 = chunk[ch], r1 = chunk[ch + 1];
    const int p0 = incptr[r0], p1 = incptr[r1];
    for (int a = r0 + lane; a < r1; a += 64) {
      double acc = 0.0;
      for (int p = p0; p < p1; ++p) {
        const uint32_t w = inc[p];
        const int e = (int)(w & 0x0FFFFFFFu), la = (int)(w >> 28);
        if (conn[(size_t)e * npe + la] != a) continue;
        const double *wd = wdet + (size_t)e * Gm;
        double me = 0.0, dsum = 0.0, da = 0.0;
        for (int g = 0; g < Gm; ++g) me += wd[g];
        for (int k = 0; k < npe; ++k) {
          double d = 0.0;
          for (int g = 0; g < Gm; ++g) d += wd[g] * tab->N[g][k] * tab->N[g][k];
          dsum += d;
          da = (k == la) ? d : da;
        }
        acc += me * da / dsum;
      }
      ml[a] = acc;
    }
  }
}

// *bad = elements of the context (its own and its ghosts) with det J <= 0, or NaN, at a Gauss point of the stiffness
// rule in the CURRENT configuration x.  The check of the explicit loop: the same count on every element type and
// assembly strategy, without an assembly (the residual-only kernels do not all count) and without touching K.
__global__ __launch_bounds__(256)
void k_count_inverted(int E, int npe, int G, const int *__restrict__ conn, const double *__restrict__ x,
                      const ElemTable *__restrict__ tab, int *bad)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  bool inv = false;
  for (int g = 0; g < G; ++g) {
    double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int k = 0; k < npe; ++k) {
      const double *X = x + (size_t)conn[(size_t)e * npe + k] * 4;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double d = tab->dN[g][i][k];
#pragma unroll
        for (int j = 0; j < 3; ++j) J[i][j] += d * X[j];
      }
    }
    const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                       J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    inv = inv || !(det > 0.0);
  }
  if (inv) atomicAdd(bad, 1);
}

// Kick and drift over the 16-byte pieces of the owned node records [a0, a1): vh = v + dt/2 a, u = dt vh; both 0 on the
// prescribed dofs (k_explicit_presc then gives vh its prescribed value there)
__global__ __launch_bounds__(256)
void k_explicit_kick(int a0, int a1, double dt, const mass_v2d *__restrict__ v, const mass_v2d *__restrict__ a,
                     const uint8_t *__restrict__ mask, mass_v2d *__restrict__ vh, double *__restrict__ u)
{
  const size_t p1 = (size_t)a1 * 2, stride = (size_t)gridDim.x * 256;
  const double hdt = 0.5 * dt;
  for (size_t p = (size_t)a0 * 2 + (size_t)blockIdx.x * 256 + threadIdx.x; p < p1; p += stride) {
    const size_t d = (p >> 1) * 3 + 2 * (p & 1);               // first dof of the piece
    mass_v2d w = v[p] + hdt * a[p];
    if (mask[d]) w.x = 0.0;
    if (p & 1) w.y = 0.0;                                      // (the pad)
    else if (mask[d + 1]) w.y = 0.0;
    vh[p] = w;
    u[d] = dt * w.x;
    if (!(p & 1)) u[d + 1] = dt * w.y;
  }
}

// vh += value dlambda / dt on the prescribed dofs of the owned nodes (the kick left 0 there; a dof named twice adds up,
// as in k_nodes_bc)
__global__ __launch_bounds__(256)
void k_explicit_presc(int n_cdof, const int *__restrict__ cdof, const double *__restrict__ cval, double rate, int a0, int a1,
                      double *__restrict__ vh)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_cdof) return;
  const int c = cdof[t], node = c / 3;
  if (node < a0 || node >= a1) return;
  atomicAdd(vh + (size_t)node * 4 + c % 3, cval[t] * rate);
}

// Finish over the pieces of ALL node records.  Owned nodes: a = f / ml (0 on prescribed dofs), v = vh + dt/2 a, and the
// piece's share of 1/2 ml |v|^2 into the workgroup's partial sum.  Other nodes: v = u / dt, a = 0 -- u is what the
// exchange brought (0 on nodes that are not in the halo), so no second exchange is needed; v and a are authoritative on
// owned nodes only.  KE_ONLY: nothing is written but the partial sums of the velocities in force.
// DAMP (mass-proportional damping C = alpha M_L): M_L a = f - alpha M_L v with the END-of-step velocity v = vh + dt/2 a,
// solved pointwise: a = (f / ml - alpha vh) / (1 + alpha dt / 2).
template <bool KE_ONLY, bool DAMP>
__global__ __launch_bounds__(256)
void k_explicit_finish(int N, int a0, int a1, double dt, const double *__restrict__ f, const double *__restrict__ ml,
                       const uint8_t *__restrict__ mask, const double *__restrict__ u, const mass_v2d *__restrict__ vh,
                       mass_v2d *__restrict__ v, mass_v2d *__restrict__ a, double *__restrict__ part, double alpha)
{
  __shared__ double sh[4];
  const size_t n = (size_t)N * 2, stride = (size_t)gridDim.x * 256;
  const double hdt = 0.5 * dt;
  double ke = 0.0;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += stride) {
    const int node = (int)(p >> 1);
    const bool lo = !(p & 1);
    const size_t d = (size_t)node * 3 + (lo ? 0 : 2);
    const bool own = node >= a0 && node < a1;
    if constexpr (KE_ONLY) {
      if (own) { const mass_v2d w = v[p]; ke += 0.5 * ml[node] * (w.x * w.x + w.y * w.y); }
    } else {
      mass_v2d vv, aa;
      if (own) {
        const double m = ml[node];
        const mass_v2d wh = vh[p];
        if constexpr (DAMP) {
          const double den = 1.0 + alpha * hdt;
          aa.x = mask[d] ? 0.0 : (f[d] / m - alpha * wh.x) / den;
          aa.y = lo ? (mask[d + 1] ? 0.0 : (f[d + 1] / m - alpha * wh.y) / den) : 0.0;
        } else {
          aa.x = mask[d] ? 0.0 : f[d] / m;
          aa.y = lo ? (mask[d + 1] ? 0.0 : f[d + 1] / m) : 0.0;
        }
        vv = wh + hdt * aa;
        ke += 0.5 * m * (vv.x * vv.x + vv.y * vv.y);
      } else {
        aa.x = 0.0; aa.y = 0.0;
        vv.x = u[d] / dt; vv.y = lo ? u[d + 1] / dt : 0.0;
      }
      v[p] = vv; a[p] = aa;
    }
  }
  ke = block_sum(ke, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = ke;
}

// [N][3] -> [N][4] (the pad is written 0)
__global__ __launch_bounds__(256)
void k_vec3_to_nodes(int N, const double *__restrict__ v3, double *__restrict__ v4)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= N) return;
  mass_v2d *o = reinterpret_cast<mass_v2d *>(v4 + (size_t)a * 4);
  mass_v2d lo, hi;
  lo.x = v3[(size_t)a * 3]; lo.y = v3[(size_t)a * 3 + 1]; hi.x = v3[(size_t)a * 3 + 2]; hi.y = 0.0;
  o[0] = lo; o[1] = hi;
}

// ---- launchers ---------------------------------------------------------------------------------------------------
static int chunk_grid(const feahip_ctx *c)
{
  const int g = (c->nchunks_local + FEA_WAVES_PER_WG - 1) / FEA_WAVES_PER_WG;
  return g < FEA_RED_BLOCKS ? (g > 0 ? g : 1) : FEA_RED_BLOCKS;
}
static int piece_grid(size_t n)
{
  const size_t g = (n + 255) / 256;
  return (int)(g < (size_t)FEA_RED_BLOCKS * 4 ? (g > 0 ? g : 1) : (size_t)FEA_RED_BLOCKS * 4);
}

int launch_mass_add(feahip_ctx *c, double coef)
{
  const long long v0 = c->kb0 * 9, v1 = c->kb1 * 9;
  if (v1 <= v0) return FEAHIP_OK;
  hipLaunchKernelGGL(k_mass_add, dim3(piece_grid((size_t)((v1 - v0) / 2 + 1))), dim3(256), 0, c->stream, v0, v1, coef,
                     c->mass.d_m, c->d_K);
  FEA_HIP_CHECK(c, hipGetLastError());
  ++c->k_epoch;                                        // another matrix: the preconditioners set up again, as after an assembly
  return FEAHIP_OK;
}

int launch_mass_residual(feahip_ctx *c, double a0)
{
  hipLaunchKernelGGL(k_mass_residual, dim3(chunk_grid(c)), dim3(64 * FEA_WAVES_PER_WG), 0, c->stream, c->chunk0,
                     c->nchunks_local, c->d_chunk, c->d_rowptr, c->d_colidx, c->mass.d_m, c->d_x, c->mass.d_xt, a0, c->d_f);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_mass_product(feahip_ctx *c, const double *d_v4, double *d_y)
{
  hipLaunchKernelGGL(k_mass_product, dim3(chunk_grid(c)), dim3(64 * FEA_WAVES_PER_WG), 0, c->stream, c->chunk0,
                     c->nchunks_local, c->d_chunk, c->d_rowptr, c->d_colidx, c->mass.d_m, d_v4, d_y);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_block_product(feahip_ctx *c, const double *d_m, const double *d_v4, double *d_y)
{
  hipLaunchKernelGGL(k_mass_product, dim3(chunk_grid(c)), dim3(64 * FEA_WAVES_PER_WG), 0, c->stream, c->chunk0,
                     c->nchunks_local, c->d_chunk, c->d_rowptr, c->d_colidx, d_m, d_v4, d_y);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_body_force(feahip_ctx *c, double *d_fv)
{
  MassState &M = c->mass;
  if (M.body[0] == 0.0 && M.body[1] == 0.0 && M.body[2] == 0.0) return FEAHIP_OK;
  // F_body is M's: a mass dropped by feahip_set_materials is refused here too, and one whose ids or rows have changed
  // since is assembled again, F_body with it, before anything is added
  if (const int rc = mass_ensure(c, "residual assembly with a body force")) return rc;
  const int i0 = 3 * c->row0, i1 = 3 * c->row1;
  if (i1 <= i0) return FEAHIP_OK;
  hipLaunchKernelGGL(k_body_add, dim3((i1 - i0 + 255) / 256), dim3(256), 0, c->stream, i0, i1, c->load_factor, c->mass.d_body, d_fv);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_newmark_predict(feahip_ctx *c, double dt, double beta, double gamma)
{
  const size_t n = (size_t)c->N * 2;
  MassState &M = c->mass;
  hipLaunchKernelGGL(k_newmark_predict, dim3(piece_grid(n)), dim3(256), 0, c->stream, n, dt, dt * dt * (0.5 - beta),
                     dt * (1.0 - gamma), (const mass_v2d *)c->d_x, (const mass_v2d *)M.d_vel, (const mass_v2d *)M.d_acc,
                     (mass_v2d *)M.d_xt, (mass_v2d *)M.d_vt);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_newmark_correct(feahip_ctx *c, double dt, double beta, double gamma)
{
  const size_t n = (size_t)c->N * 2;
  MassState &M = c->mass;
  hipLaunchKernelGGL(k_newmark_correct, dim3(piece_grid(n)), dim3(256), 0, c->stream, n, 1.0 / (beta * dt * dt), gamma * dt,
                     (const mass_v2d *)c->d_x, (const mass_v2d *)M.d_xt, (const mass_v2d *)M.d_vt, (mass_v2d *)M.d_vel,
                     (mass_v2d *)M.d_acc);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_explicit_kick(feahip_ctx *c, double dt)
{
  MassState &M = c->mass;
  M.ke_parts = 0;
  if (c->row1 <= c->row0) return FEAHIP_OK;
  hipLaunchKernelGGL(k_explicit_kick, dim3(piece_grid((size_t)(c->row1 - c->row0) * 2)), dim3(256), 0, c->stream, c->row0, c->row1,
                     dt, (const mass_v2d *)M.d_vel, (const mass_v2d *)M.d_acc, (const uint8_t *)c->d_dofmask, (mass_v2d *)M.d_vt, c->d_u);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_explicit_presc(feahip_ctx *c, double dlambda, double dt)
{
  if (c->n_cdof == 0 || dlambda == 0.0) return FEAHIP_OK;
  hipLaunchKernelGGL(k_explicit_presc, dim3((c->n_cdof + 255) / 256), dim3(256), 0, c->stream, c->n_cdof, c->d_cdof, c->d_cval,
                     dlambda / dt, c->row0, c->row1, c->mass.d_vt);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_explicit_finish(feahip_ctx *c, double dt)
{
  MassState &M = c->mass;
  const int g = piece_grid((size_t)c->N * 2);
  if (c->damping.alpha > 0.0)
    hipLaunchKernelGGL((k_explicit_finish<false, true>), dim3(g), dim3(256), 0, c->stream, c->N, c->row0, c->row1, dt, c->d_f, M.d_ml,
                       (const uint8_t *)c->d_dofmask, c->d_u, (const mass_v2d *)M.d_vt, (mass_v2d *)M.d_vel, (mass_v2d *)M.d_acc, M.d_ke_part,
                       c->damping.alpha);
  else
    hipLaunchKernelGGL((k_explicit_finish<false, false>), dim3(g), dim3(256), 0, c->stream, c->N, c->row0, c->row1, dt, c->d_f, M.d_ml,
                       (const uint8_t *)c->d_dofmask, c->d_u, (const mass_v2d *)M.d_vt, (mass_v2d *)M.d_vel, (mass_v2d *)M.d_acc, M.d_ke_part, 0.0);
  FEA_HIP_CHECK(c, hipGetLastError());
  M.ke_parts = g;
  return FEAHIP_OK;
}

int launch_kinetic_energy(feahip_ctx *c, double *d_out)
{
  MassState &M = c->mass;
  if (M.ke_parts == 0) {                                   // no explicit step left the sums of these velocities
    const int g = piece_grid((size_t)c->N * 2);
    hipLaunchKernelGGL((k_explicit_finish<true, false>), dim3(g), dim3(256), 0, c->stream, c->N, c->row0, c->row1, 0.0, (const double *)nullptr,
                       M.d_ml, (const uint8_t *)nullptr, (const double *)nullptr, (const mass_v2d *)nullptr, (mass_v2d *)M.d_vel,
                       (mass_v2d *)nullptr, M.d_ke_part, 0.0);
    M.ke_parts = g;
  }
  enq_reduce_final(c, M.ke_parts, 1, 0, M.d_ke_part, d_out);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_count_inverted(feahip_ctx *c)
{
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d_flag + 1, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_count_inverted, dim3((c->E + 255) / 256), dim3(256), 0, c->stream, c->E, c->npe, c->G, c->d_conn, c->d_x,
                     (const ElemTable *)c->d_table, c->d_flag + 1);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_vec3_to_nodes(feahip_ctx *c, const double *d_v3, double *d_v4)
{
  hipLaunchKernelGGL(k_vec3_to_nodes, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->N, d_v3, d_v4);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// ---- assembly of m and of the body force -----------------------------------------------------------------------------
namespace {
struct MassScratch {
  MassTable *tab = nullptr;
  double *rho = nullptr, *wdet = nullptr, *m = nullptr;
  int *bad = nullptr;
  ~MassScratch() { dev_free({tab, rho, wdet, m, bad}); }
};
}

// m for the rows of the shard installed now (K exists), from the parameters in P; *bad_elem >= 0: an element with
// det J0 <= 0 at a mass point (nothing is returned then)
static int mass_assemble(feahip_ctx *c, const MassState &P, double **m_base, int *bad_elem)
{
  int rc;
  *bad_elem = -1; *m_base = nullptr;
  if ((rc = ensure_generic_maps(c))) return rc;
  MassScratch S;
  MassTable T;
  memset(&T, 0, sizeof(T));
  for (int g = 0; g < P.Gm; ++g) {
    T.w[g] = P.w[g];
    for (int k = 0; k < c->npe; ++k) {
      T.N[g][k] = P.N[(size_t)g * c->npe + k];
      for (int i = 0; i < 3; ++i) T.dN[g][i][k] = P.dN[((size_t)g * 3 + i) * c->npe + k];
    }
  }
  const size_t nb = (size_t)(c->kb1 - c->kb0);
  const int none = 0x7FFFFFFF;
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.tab, sizeof(T)));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.rho, sizeof(double) * P.rho.size()));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.wdet, sizeof(double) * (size_t)c->E * P.Gm));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.m, sizeof(double) * (nb ? nb : 1)));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.bad, sizeof(int)));
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.tab, &T, sizeof(T), hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.rho, P.rho.data(), sizeof(double) * P.rho.size(), hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.bad, &none, sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_mass_elements, dim3((c->E + 255) / 256), dim3(256), 0, c->stream, c->E, c->npe, P.Gm, c->d_conn,
                     c->d_X0, S.tab, S.rho, P.n_rho, c->d_elem_mat, S.wdet, S.bad);
  hipLaunchKernelGGL(k_mass_blocks, dim3(chunk_grid(c)), dim3(64 * FEA_WAVES_PER_WG), 0, c->stream, c->chunk0,
                     c->nchunks_local, c->d_chunk, c->d_rowptr, c->d_colidx, c->generic.d_incptr, c->generic.d_inc,
                     c->d_conn, c->npe, P.Gm, S.tab, S.wdet, S.m - c->kb0);
  FEA_HIP_CHECK(c, hipGetLastError());
  int bad = none;
  FEA_HIP_CHECK(c, hipMemcpyAsync(&bad, S.bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  if (bad != none) { *bad_elem = bad; return FEAHIP_OK; }
  *m_base = S.m; S.m = nullptr;
  return FEAHIP_OK;
}

// F_body = M (1 (x) b) on the owned rows, at load factor 1 (m is current)
static int body_assemble(feahip_ctx *c)
{
  MassState &M = c->mass;
  if (M.body[0] == 0.0 && M.body[1] == 0.0 && M.body[2] == 0.0) {
    dev_free({M.d_body}); M.d_body = nullptr;
    return FEAHIP_OK;
  }
  std::vector<double> ones((size_t)c->N * 4, 0.0);
  for (int a = 0; a < c->N; ++a)
    for (int j = 0; j < 3; ++j) ones[(size_t)a * 4 + j] = M.body[j];
  if (!M.d_body) FEA_HIP_CHECK(c, hipMalloc((void **)&M.d_body, sizeof(double) * (size_t)c->ndof));
  FEA_HIP_CHECK(c, hipMemsetAsync(M.d_body, 0, sizeof(double) * (size_t)c->ndof, c->stream));
  // a vector of its own, not one of the step's: the residual assembly may come here (launch_body_force)
  double *d_b4 = nullptr;
  FEA_HIP_CHECK(c, hipMalloc((void **)&d_b4, sizeof(double) * ones.size()));
  int rc = hipMemcpyAsync(d_b4, ones.data(), sizeof(double) * ones.size(), hipMemcpyHostToDevice, c->stream) == hipSuccess
               ? launch_mass_product(c, d_b4, M.d_body) : FEAHIP_EHIP;
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = FEAHIP_EHIP;
  dev_free({d_b4});
  if (rc == FEAHIP_EHIP && c->err.empty()) c->err = "feahip_set_body_force: device copy failed";
  return rc;
}

int mass_ensure(feahip_ctx *c, const char *who)
{
  MassState &M = c->mass;
  if (M.stale) { c->err = std::string(who) + ": the material count changed since feahip_set_mass gave one density per material"; return FEAHIP_ESTATE; }
  if (!M.set) { c->err = std::string(who) + ": no mass on this context (feahip_set_mass)"; return FEAHIP_ESTATE; }
  int rc;
  if ((rc = ensure_k(c))) return rc;
  if (M.d_m_base && M.kb0 == c->kb0 && M.kb1 == c->kb1) return FEAHIP_OK;
  double *m = nullptr;
  int bad = -1;
  if ((rc = mass_assemble(c, M, &m, &bad))) return rc;
  if (bad >= 0) { c->err = std::string(who) + ": det J0 <= 0 at a mass point of element " + std::to_string(bad); return FEAHIP_ESTATE; }
  M.release_m();
  M.d_m_base = m; M.d_m = m - c->kb0; M.kb0 = c->kb0; M.kb1 = c->kb1;
  return body_assemble(c);
}

// The lumped mass of the rows installed now, from the rule and the densities of the last feahip_set_mass: built on the
// first explicit call and again when the shard has changed (feahip_set_materials and feahip_set_mass drop it).
int lump_ensure(feahip_ctx *c, const char *who)
{
  int rc;
  if ((rc = mass_ensure(c, who))) return rc;
  MassState &M = c->mass;
  if (M.d_ml && M.ml_row0 == c->row0 && M.ml_row1 == c->row1) return FEAHIP_OK;
  if ((rc = ensure_generic_maps(c))) return rc;
  MassScratch S;
  MassTable T;
  memset(&T, 0, sizeof(T));
  for (int g = 0; g < M.Gm; ++g) {
    T.w[g] = M.w[g];
    for (int k = 0; k < c->npe; ++k) {
      T.N[g][k] = M.N[(size_t)g * c->npe + k];
      for (int i = 0; i < 3; ++i) T.dN[g][i][k] = M.dN[((size_t)g * 3 + i) * c->npe + k];
    }
  }
  const int none = 0x7FFFFFFF;
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.tab, sizeof(T)));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.rho, sizeof(double) * M.rho.size()));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.wdet, sizeof(double) * (size_t)c->E * M.Gm));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.bad, sizeof(int)));
  if (!M.d_ml) FEA_HIP_CHECK(c, hipMalloc((void **)&M.d_ml, sizeof(double) * (size_t)c->N));
  if (!M.d_ke_part) FEA_HIP_CHECK(c, hipMalloc((void **)&M.d_ke_part, sizeof(double) * 4 * FEA_RED_BLOCKS));
  M.ml_row0 = M.ml_row1 = -1; M.ke_parts = 0;
  FEA_HIP_CHECK(c, hipMemsetAsync(M.d_ml, 0, sizeof(double) * (size_t)c->N, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.tab, &T, sizeof(T), hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.rho, M.rho.data(), sizeof(double) * M.rho.size(), hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.bad, &none, sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_mass_elements, dim3((c->E + 255) / 256), dim3(256), 0, c->stream, c->E, c->npe, M.Gm, c->d_conn,
                     c->d_X0, S.tab, S.rho, M.n_rho, c->d_elem_mat, S.wdet, S.bad);
  hipLaunchKernelGGL(k_mass_lump, dim3(chunk_grid(c)), dim3(64 * FEA_WAVES_PER_WG), 0, c->stream, c->chunk0, c->nchunks_local,
                     c->d_chunk, c->generic.d_incptr, c->generic.d_inc, c->d_conn, c->npe, M.Gm, S.tab, S.wdet, M.d_ml);
  FEA_HIP_CHECK(c, hipGetLastError());
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));          // (the scratch is freed on return)
  M.ml_row0 = c->row0; M.ml_row1 = c->row1;
  return FEAHIP_OK;
}

int mass_set(feahip_ctx *c, int n_rho, const double *rho, int mass_points, const double *weights, const double *forms,
             const double *dforms)
{
  auto refuse = [c](std::string why) { c->err = "feahip_set_mass: " + std::move(why); return FEAHIP_EINVAL; };
  if (n_rho == 0) {
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    c->mass.release();
    return FEAHIP_OK;
  }
  const int table = c->n_materials;
  if (n_rho != 1 && !(table > 0 && n_rho == table))
    return refuse(std::to_string(n_rho) + " densities: one, or one per material (" + std::to_string(table) + " in force)");
  if (!rho || !weights || !forms || !dforms) return refuse("null array");
  if (mass_points < 1 || mass_points > FEA_MAX_GAUSS)
    return refuse(std::to_string(mass_points) + " mass points outside [1," + std::to_string(FEA_MAX_GAUSS) + "]");
  for (int i = 0; i < n_rho; ++i)
    if (!std::isfinite(rho[i]) || !(rho[i] > 0.0)) return refuse("density " + std::to_string(i) + " is not finite and positive");
  int rc;
  if ((rc = ensure_k(c))) return rc;
  MassState P;
  P.n_rho = n_rho; P.n_mat = n_rho > 1 ? table : 0; P.Gm = mass_points;
  P.rho.assign(rho, rho + n_rho);
  P.w.assign(weights, weights + mass_points);
  P.N.assign(forms, forms + (size_t)mass_points * c->npe);
  P.dN.assign(dforms, dforms + (size_t)mass_points * 3 * c->npe);
  double *m = nullptr;
  int bad = -1;
  if ((rc = mass_assemble(c, P, &m, &bad))) return rc;
  if (bad >= 0) return refuse("det J0 <= 0 at a mass point of element " + std::to_string(bad));
  MassState &M = c->mass;
  const size_t nb4 = sizeof(double) * 4 * (size_t)c->N;
  for (double **p : {&M.d_vel, &M.d_acc, &M.d_xt, &M.d_vt}) {
    if (!*p && hipMalloc((void **)p, nb4) != hipSuccess) { dev_free({m}); c->err = "feahip_set_mass: out of device memory"; return FEAHIP_ENOMEM; }
    FEA_HIP_CHECK(c, hipMemsetAsync(*p, 0, nb4, c->stream));
  }
  M.release_m();
  M.release_lump();                                          // of the mass before: built again by the next explicit call
  M.set = true; M.stale = false;
  M.n_rho = P.n_rho; M.n_mat = P.n_mat; M.Gm = P.Gm;
  M.rho.swap(P.rho); M.w.swap(P.w); M.N.swap(P.N); M.dN.swap(P.dN);
  M.d_m_base = m; M.d_m = m - c->kb0; M.kb0 = c->kb0; M.kb1 = c->kb1;
  return body_assemble(c);                                   // a body force given before: of the new mass
}

int mass_set_body_force(feahip_ctx *c, const double *b)
{
  int rc;
  if ((rc = mass_ensure(c, "feahip_set_body_force"))) return rc;
  for (int j = 0; j < 3; ++j) {
    if (b && !std::isfinite(b[j])) { c->err = "feahip_set_body_force: component " + std::to_string(j) + " is not finite"; return FEAHIP_EINVAL; }
  }
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < 3; ++j) c->mass.body[j] = b ? b[j] : 0.0;
  return body_assemble(c);
}
