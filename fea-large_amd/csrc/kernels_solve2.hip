// kernels_solve2.hip -- K [u, u2] = [f, f2]: two (preconditioned) CG recurrences in lockstep over ONE read of the
// matrix per iteration (feahip_solve_slae2; the arc-length corrector solves K du_R = R and K du_F = F_ext with it).
//
// Layout of a paired vector: the two columns interleaved per scalar dof, v2[2 k + c] for dof k and column c.  The
// three x entries a 3x3 block multiplies are then 48 contiguous bytes for both columns -- three 16-byte loads where
// two separate vectors need six 8-byte ones --, a row lane stores its two results with one 16-byte store, the
// partial products sit in LDS as 16-byte pairs, and every vector kernel reads and writes one 16-byte piece per lane.
//
// Each column has its own scalars, its own stop flag and its own partial sums; a column whose flag is set is frozen:
// nothing of it is written again (store_live).  The loop is the two-reduction loop of kernels_solve.hip
// (enq_cg_start / enq_cg_iteration); all reductions are two-stage with a fixed grid and a fixed order, no atomics.
// The single-column kernels of kernels_solve.hip are not touched.
#include "feahip_internal.h"
#include "reduce_device.h"
#include <cmath>

#ifndef FEA_SPMV_STAGED
#define FEA_SPMV_STAGED 1      // as in kernels_solve.hip: bit 0 = the double matrix is staged through LDS
#endif
#define RB FEA_RED_BLOCKS
typedef double v2d __attribute__((ext_vector_type(2)));

// multigrid preconditioner (amg.hip)
int amg_prepare(feahip_ctx *c);
double *amg_apply(feahip_ctx *c, const double *r);

// the pair, or the component of the live column alone: a frozen column's half of the 16 bytes is not written
static __device__ __forceinline__ void store_live(v2d *p, v2d v, bool l0, bool l1)
{
  if (l0 && l1) *p = v;
  else if (l0) reinterpret_cast<double *>(p)[0] = v.x;
  else if (l1) reinterpret_cast<double *>(p)[1] = v.y;
}
// partial sums in d2_part: sum s (0 p.q, 1 r.z, 2 r.r, 3 b.b) of column c at [(2 s + c) RB, (2 s + c + 1) RB)
static __host__ __device__ __forceinline__ int pslot(int s, int c) { return (2 * s + c) * RB; }

// ------------------------------------------------------------------------
// y2 = K x2 (+ the partial sums of dotwith . y2 per column).  spmv_body of kernels_solve.hip with two vectors: a lane
// loads its blocks and their column index once, gathers the x entries of both columns (16 bytes per dof) and leaves
// SIX partial products per block in LDS (128 blocks x 48 bytes = 6 KB per wave, inside the 9 KB the staged values
// take first); the row lanes sum both columns in block order -- per column the order k_spmv sums in.
// flag (may be null): the two stop flags; the product of a frozen column is not stored, with both frozen nothing runs.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_spmv2(int chunk0, int nchunks, const int *chunk, const int *rowptr, const int *colidx, const double *K,
             const v2d *x, v2d *y, const v2d *dotwith, double *part, const int *flag)
{
  constexpr int BB = 72;
  static_assert(FEA_CHUNK_ROWS * 3 <= 64, "one lane per (row, component) of a chunk");
  constexpr int NPMAX = (15 + FEA_CHUNK_BLOCKS * BB + 15) >> 4;                   // 16-byte pieces of a chunk
  constexpr bool STAGED = ((FEA_SPMV_STAGED) & 1) != 0;
  constexpr int TILE = FEA_CHUNK_BLOCKS * 6;                                      // doubles of the partial products
  constexpr int SPD = STAGED ? (2 * NPMAX > TILE ? 2 * NPMAX : TILE) : TILE;
  static_assert(SPD % 2 == 0, "every wave's tile is 16-byte aligned");
  __shared__ __attribute__((aligned(16))) double sP[FEA_WAVES_PER_WG][SPD];
  __shared__ double scratch[5];
  bool l0 = true, l1 = true;
  if (flag) { l0 = flag[0] == 0; l1 = flag[1] == 0; }
  if (!l0 && !l1) return;                    // both columns have stopped (uniform)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double *tP = sP[wave];
  v2d *tP2 = reinterpret_cast<v2d *>(tP);
  v2d dsum = {0.0, 0.0};
  for (int ch = chunk0 + blockIdx.x * FEA_WAVES_PER_WG + wave; ch < chunk0 + nchunks; ch += gridDim.x * FEA_WAVES_PER_WG) {
    const int r0 = chunk[ch], r1 = chunk[ch + 1];
    const int b0 = rowptr[r0], nb = rowptr[r1] - b0;
    if (nb > FEA_CHUNK_BLOCKS) {
      // a row longer than the tile has a chunk of its own: the lanes stride over its blocks, a butterfly per sum
      v2d a0 = {0.0, 0.0}, a1 = {0.0, 0.0}, a2 = {0.0, 0.0};
      for (int k = lane; k < nb; k += 64) {
        const double *vp = K + (size_t)(b0 + k) * 9;
        const int col = colidx[b0 + k];
        const v2d x0 = x[(size_t)col * 3], x1 = x[(size_t)col * 3 + 1], x2 = x[(size_t)col * 3 + 2];
        a0 += vp[0] * x0 + vp[1] * x1 + vp[2] * x2;
        a1 += vp[3] * x0 + vp[4] * x1 + vp[5] * x2;
        a2 += vp[6] * x0 + vp[7] * x1 + vp[8] * x2;
      }
      a0.x = wave_sum_all(a0.x); a1.x = wave_sum_all(a1.x); a2.x = wave_sum_all(a2.x);
      a0.y = wave_sum_all(a0.y); a1.y = wave_sum_all(a1.y); a2.y = wave_sum_all(a2.y);
      if (lane < 3) {
        const v2d acc = lane == 0 ? a0 : lane == 1 ? a1 : a2;
        store_live(y + (size_t)r0 * 3 + lane, acc, l0, l1);
        if (dotwith) dsum += acc * dotwith[(size_t)r0 * 3 + lane];
      }
      continue;
    }
    double v[2][9];
    v2d xv[2][3];
    int kb = 0, ke = 0;
    if (lane < (r1 - r0) * 3) { kb = rowptr[r0 + lane / 3] - b0; ke = rowptr[r0 + lane / 3 + 1] - b0; }
    if constexpr (STAGED) {
      // the chunk's values as lane-contiguous 16-byte pieces into LDS (see spmv_body)
      constexpr int NJ = (NPMAX + 63) / 64;
      const size_t s0 = (size_t)b0 * BB, a0 = s0 & ~(size_t)15;      // the array is 16-byte aligned and padded by 16 bytes
      const int sh = (int)(s0 - a0), np = (sh + nb * BB + 15) >> 4;
      const v2d *Kp = reinterpret_cast<const v2d *>(reinterpret_cast<const char *>(K) + a0);
      int col[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) { const int k = lane + 64 * h; col[h] = colidx[k < nb ? b0 + k : b0]; }
      v2d pc[NJ];
#pragma unroll
      for (int j = 0; j < NJ - 1; ++j) { const int p = lane + 64 * j; pc[j] = Kp[p < np ? p : 0]; }
      if (np > 64 * (NJ - 1)) { const int p = lane + 64 * (NJ - 1); pc[NJ - 1] = Kp[p < np ? p : 0]; }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 3; ++i) xv[h][i] = x[(size_t)col[h] * 3 + i];
#pragma unroll
      for (int j = 0; j < NJ - 1; ++j) { const int p = lane + 64 * j; if (p < np) tP2[p] = pc[j]; }
      if (np > 64 * (NJ - 1)) { const int p = lane + 64 * (NJ - 1); if (p < np) tP2[p] = pc[NJ - 1]; }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        const char *bp = reinterpret_cast<const char *>(tP) + sh + BB * (k < nb ? k : 0);
#pragma unroll
        for (int q = 0; q < 9; ++q) v[h][q] = reinterpret_cast<const double *>(bp)[q];
      }
      // (the products below overwrite the staged values: 48 bytes per block where 72 were read, and every lane has
      // read its blocks by then)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        const int kk = k < nb ? b0 + k : b0;
        const double *vp = K + (size_t)kk * 9;
#pragma unroll
        for (int q = 0; q < 9; ++q) v[h][q] = vp[q];
        const int col = colidx[kk];
#pragma unroll
        for (int i = 0; i < 3; ++i) xv[h][i] = x[(size_t)col * 3 + i];
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k < nb) {
        tP2[k * 3 + 0] = v[h][0] * xv[h][0] + v[h][1] * xv[h][1] + v[h][2] * xv[h][2];
        tP2[k * 3 + 1] = v[h][3] * xv[h][0] + v[h][4] * xv[h][1] + v[h][5] * xv[h][2];
        tP2[k * 3 + 2] = v[h][6] * xv[h][0] + v[h][7] * xv[h][1] + v[h][8] * xv[h][2];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    const int t = lane;
    if (t < (r1 - r0) * 3) {
      const int i = t % 3;
      v2d acc = {0.0, 0.0};
      for (int k = kb; k < ke; ++k) acc += tP2[k * 3 + i];
      store_live(y + (size_t)r0 * 3 + t, acc, l0, l1);
      if (dotwith) dsum += acc * dotwith[(size_t)r0 * 3 + t];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
  if (part) {
    const double s0 = block_sum(dsum.x, scratch), s1 = block_sum(dsum.y, scratch);
    if (threadIdx.x == 0) { if (l0) part[pslot(0, 0) + blockIdx.x] = s0; if (l1) part[pslot(0, 1) + blockIdx.x] = s1; }
  }
}

// ------------------------------------------------------------------------
// vector kernels.  Lane <-> scalar dof as in k_cg_update: 21 nodes per wave and step, one 16-byte piece (both
// columns of the dof) per lane and vector, row i of a node's D^-1 block as the three doubles at 3 (3a + i), the three
// residual components of a node meet by shuffles.
// ------------------------------------------------------------------------
#define FOR_DOFS2(nb, a0, a1) \
  for (long long nb = (a0) + (long long)(blockIdx.x * 4 + (threadIdx.x >> 6)) * 21; nb < (a1); nb += (long long)gridDim.x * 4 * 21)

static __device__ __forceinline__ v2d apply_minv(const double *minv, size_t k, bool on, v2d rv, int lane, int i)
{
  double m0 = 0, m1 = 0, m2 = 0;
  if (on) { const double *m = minv + 3 * k; m0 = m[0]; m1 = m[1]; m2 = m[2]; }
  v2d z;
  {
    const double r0 = __shfl(rv.x, lane - i), r1 = __shfl(rv.x, lane - i + 1), r2 = __shfl(rv.x, lane - i + 2);
    z.x = m0 * r0 + m1 * r1 + m2 * r2;
  }
  {
    const double r0 = __shfl(rv.y, lane - i), r1 = __shfl(rv.y, lane - i + 1), r2 = __shfl(rv.y, lane - i + 2);
    z.y = m0 * r0 + m1 * r1 + m2 * r2;
  }
  return z;
}

// r = b - q ; p = M r ; partial sums r.z, r.r, b.b of both columns     (q = K x0, x0 = b)
__global__ __launch_bounds__(256)
void k2_cg_init(int a0, int a1, const v2d *b, const v2d *q, const double *minv, v2d *r, v2d *p, double *part)
{
  __shared__ double scratch[5];
  v2d srz = {0.0, 0.0}, srr = {0.0, 0.0}, sbb = {0.0, 0.0};
  const int lane = threadIdx.x & 63, i = lane % 3;
  FOR_DOFS2(nb, a0, a1) {
    const bool on = lane < 63 && nb + lane / 3 < a1;
    const size_t k = (size_t)nb * 3 + lane;
    v2d rv = {0.0, 0.0}, bv = {0.0, 0.0};
    if (on) { bv = b[k]; rv = bv - q[k]; r[k] = rv; }
    v2d z = rv;
    if (minv) z = apply_minv(minv, k, on, rv, lane, i);
    if (on) { p[k] = z; srz += rv * z; srr += rv * rv; sbb += bv * bv; }
  }
  const double z0 = block_sum(srz.x, scratch), z1 = block_sum(srz.y, scratch);
  const double r0 = block_sum(srr.x, scratch), r1 = block_sum(srr.y, scratch);
  const double b0 = block_sum(sbb.x, scratch), b1 = block_sum(sbb.y, scratch);
  if (threadIdx.x == 0) {
    part[pslot(1, 0) + blockIdx.x] = z0; part[pslot(1, 1) + blockIdx.x] = z1;
    part[pslot(2, 0) + blockIdx.x] = r0; part[pslot(2, 1) + blockIdx.x] = r1;
    part[pslot(3, 0) + blockIdx.x] = b0; part[pslot(3, 1) + blockIdx.x] = b1;
  }
}

// device scalars of column c at scal + 8 c: [0],[1] r.z ping-pong, [2] b.b, [3] last r.r, [4] tolerance^2;
// flag[c] = iteration at which the column's stop test fired (0 = running, < 0 = breakdown)
__global__ __launch_bounds__(256)
void k2_cg_init_scalars(int nparts, const double *part, double *scal, double tol, int *flag)
{
  __shared__ double scratch[5];
  for (int c = 0; c < 2; ++c) {
    const double rz = reduce_partials(part + pslot(1, c), nparts, scratch);
    const double rr = reduce_partials(part + pslot(2, c), nparts, scratch);
    const double bb = reduce_partials(part + pslot(3, c), nparts, scratch);
    if (threadIdx.x == 0) {
      double *s = scal + 8 * c;
      s[0] = rz; s[1] = rz; s[2] = bb; s[3] = rr; s[4] = tol * tol;
      flag[c] = (rr <= tol * tol * bb || rz == 0.0) ? -1000000000 : 0;   // a zero right-hand side is already solved
    }
  }
}

// per live column: alpha = r.z / p.q ; x += alpha p ; r -= alpha q ; z = M r into zq (may alias q); partial sums
// r.z, r.r.  minv null (multigrid): no z, the cycle follows.
__global__ __launch_bounds__(256)
void k2_cg_update(int a0, int a1, int it, int n_pq, const v2d *p, const v2d *q, const double *minv, v2d *x, v2d *r,
                  double *part, const double *scal, const int *flag, v2d *zq)
{
  __shared__ double scratch[5];
  const bool l0 = flag[0] == 0, l1 = flag[1] == 0;
  if (!l0 && !l1) return;
  const double pq0 = reduce_partials(part + pslot(0, 0), n_pq, scratch);
  const double pq1 = reduce_partials(part + pslot(0, 1), n_pq, scratch);
  v2d alpha;
  alpha.x = l0 ? scal[it & 1] / pq0 : 0.0;
  alpha.y = l1 ? scal[8 + (it & 1)] / pq1 : 0.0;
  v2d srz = {0.0, 0.0}, srr = {0.0, 0.0};
  const int lane = threadIdx.x & 63, i = lane % 3;
  FOR_DOFS2(nb, a0, a1) {
    const bool on = lane < 63 && nb + lane / 3 < a1;
    const size_t k = (size_t)nb * 3 + lane;
    v2d rv = {0.0, 0.0};
    if (on) {
      const v2d pv = p[k], qv = q[k];
      v2d xv = x[k];
      rv = r[k];
      if (l0) { xv.x += alpha.x * pv.x; rv.x = rv.x - alpha.x * qv.x; }
      if (l1) { xv.y += alpha.y * pv.y; rv.y = rv.y - alpha.y * qv.y; }
      store_live(x + k, xv, l0, l1);
      store_live(r + k, rv, l0, l1);
    }
    v2d z = rv;
    if (minv) z = apply_minv(minv, k, on, rv, lane, i);
    if (on) { srz += rv * z; srr += rv * rv; if (zq) store_live(zq + k, z, l0, l1); }
  }
  const double z0 = block_sum(srz.x, scratch), z1 = block_sum(srz.y, scratch);
  const double r0 = block_sum(srr.x, scratch), r1 = block_sum(srr.y, scratch);
  if (threadIdx.x == 0) {
    if (l0) { part[pslot(1, 0) + blockIdx.x] = z0; part[pslot(2, 0) + blockIdx.x] = r0; }
    if (l1) { part[pslot(1, 1) + blockIdx.x] = z1; part[pslot(2, 1) + blockIdx.x] = r1; }
  }
}

// per live column: beta = r.z_new / r.z_old ; p = z + beta p ; stop test on r.r
__global__ __launch_bounds__(256)
void k2_cg_direction(int a0, int a1, int it, int nparts, const v2d *z, v2d *p, const double *part, double *scal, int *flag)
{
  __shared__ double scratch[5];
  const bool live[2] = {flag[0] == 0, flag[1] == 0};
  if (!live[0] && !live[1]) return;
  double rz_new[2], rr[2], beta[2] = {0.0, 0.0};
  bool stop[2], broke[2], go[2];
  for (int c = 0; c < 2; ++c) {
    rz_new[c] = reduce_partials(part + pslot(1, c), nparts, scratch);
    rr[c] = reduce_partials(part + pslot(2, c), nparts, scratch);
    const double *s = scal + 8 * c;
    const double rz_old = s[it & 1];
    stop[c] = rr[c] <= s[4] * s[2];
    broke[c] = !(rz_new[c] == rz_new[c]) || !(rr[c] == rr[c]) || rz_old == 0.0;
    go[c] = live[c] && !stop[c] && !broke[c];
    if (go[c]) beta[c] = rz_new[c] / rz_old;
  }
  if (go[0] || go[1]) {
    for (size_t k = (size_t)a0 * 3 + blockIdx.x * 256 + threadIdx.x; k < (size_t)a1 * 3; k += (size_t)gridDim.x * 256) {
      const v2d zv = z[k];
      v2d pv = p[k];
      if (go[0]) pv.x = zv.x + beta[0] * pv.x;
      if (go[1]) pv.y = zv.y + beta[1] * pv.y;
      store_live(p + k, pv, go[0], go[1]);
    }
  }
  // the scalars go to the other ping-pong slot; the flags are read at kernel entry only, and a block of this launch
  // that starts after a flag was set leaves that column alone, which is what stop / broke would have made it do
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int c = 0; c < 2; ++c) {
      if (!live[c]) continue;
      double *s = scal + 8 * c;
      s[(it + 1) & 1] = rz_new[c];
      s[3] = rr[c];
      if (broke[c]) flag[c] = -(it + 1);
      else if (stop[c]) flag[c] = it + 1;
    }
  }
}

// columns in and out of a paired vector
__global__ void k2_interleave(size_t n, const double *a, const double *b, v2d *out)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) { v2d v; v.x = a[k]; v.y = b[k]; out[k] = v; }
}
__global__ void k2_deinterleave(size_t n, const v2d *in, double *a, double *b)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) { const v2d v = in[k]; a[k] = v.x; b[k] = v.y; }
}
__global__ void k2_extract(size_t n, const double *in2, int col, double *out)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = in2[2 * k + col];
}
// dst2[., col] = z (a multigrid cycle's result) ; partial sums of r2[., col] . z
__global__ __launch_bounds__(256)
void k2_insert_dot(size_t n, const double *z, const double *r2, double *dst2, int col, double *part, const int *flag)
{
  __shared__ double scratch[5];
  if (flag && flag[col] != 0) return;
  double v = 0;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) {
    const double zk = z[k];
    dst2[2 * k + col] = zk;
    v += r2[2 * k + col] * zk;
  }
  v = block_sum(v, scratch);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
static int spmv2_grid(const feahip_ctx *c)
{
  const int g = (c->nchunks_local + FEA_WAVES_PER_WG - 1) / FEA_WAVES_PER_WG;
  return g < RB ? (g > 0 ? g : 1) : RB;
}
static int vgrid2(const feahip_ctx *c)
{
  const int g = (c->N + 83) / 84;              // 4 waves x 21 nodes per block and step
  return g < RB ? (g > 0 ? g : 1) : RB;
}
static inline dim3 g256(size_t n) { return dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)); }

int ensure_solve2(feahip_ctx *c)
{
  if (c->d2_f) return FEAHIP_OK;
  const size_t n2 = sizeof(double) * 2 * (size_t)c->ndof;
  double **v[] = {&c->d2_f, &c->d2_u, &c->d2_r, &c->d2_p, &c->d2_q};
  for (double **p : v) {
    FEA_HIP_CHECK(c, hipMalloc((void **)p, n2));
    FEA_HIP_CHECK(c, hipMemsetAsync(*p, 0, n2, c->stream));
  }
  FEA_HIP_CHECK(c, hipMalloc((void **)&c->d_u2, n2 / 2));
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d_u2, 0, n2 / 2, c->stream));
  FEA_HIP_CHECK(c, hipMalloc((void **)&c->d2_part, sizeof(double) * 8 * RB));
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d2_part, 0, sizeof(double) * 8 * RB, c->stream));
  FEA_HIP_CHECK(c, hipMalloc((void **)&c->d2_scal, sizeof(double) * 16));
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d2_scal, 0, sizeof(double) * 16, c->stream));
  FEA_HIP_CHECK(c, hipMalloc((void **)&c->d2_flag, sizeof(int) * 2));
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d2_flag, 0, sizeof(int) * 2, c->stream));
  return FEAHIP_OK;
}

void release_solve2(feahip_ctx *c)
{
  dev_free({c->d2_f, c->d2_u, c->d2_r, c->d2_p, c->d2_q, c->d_u2, c->d2_part, c->d2_scal, c->d2_flag});
  c->d2_f = c->d2_u = c->d2_r = c->d2_p = c->d2_q = c->d_u2 = c->d2_part = c->d2_scal = nullptr;
  c->d2_flag = nullptr;
}

// what the two-column solve refuses: anything but a whole, unsharded matrix on one context
int solve2_refused(feahip_ctx *c, const char *who)
{
  const char *why = nullptr;
  if (c->precond == 2) why = "preconditioner 2 (coarse level across the ranks) is not supported";
  else if (c->rank_own >= 0) why = "the context is one rank's sub-mesh (feahip_create_rank*)";
  else if (c->tr) why = "the context has a transport (a member of a group or of an RCCL run)";
  else if (c->nranks != 1 || c->row0 != 0 || c->row1 != c->N) why = "the context is row-sharded";
  if (!why) return FEAHIP_OK;
  c->err = std::string(who) + ": " + why;
  return FEAHIP_EINVAL;
}

static void enq_spmv2(feahip_ctx *c, const double *x2, double *y2, const double *dotwith2, double *part, const int *flag)
{
  hipLaunchKernelGGL(k_spmv2, dim3(spmv2_grid(c)), dim3(256), 0, c->stream, c->chunk0, c->nchunks_local, c->d_chunk,
                     c->d_rowptr, c->d_colidx, c->d_K, (const v2d *)x2, (v2d *)y2, (const v2d *)dotwith2, part, flag);
}

// y2 = K x2 for device vectors in the paired layout (feahip_spmv2, feahip_time_kernel(6))
int launch_spmv2(feahip_ctx *c, const double *d_x2, double *d_y2)
{
  enq_spmv2(c, d_x2, d_y2, nullptr, nullptr, nullptr);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_interleave(feahip_ctx *c, const double *a, const double *b, double *out2)
{
  hipLaunchKernelGGL(k2_interleave, g256((size_t)c->ndof), dim3(256), 0, c->stream, (size_t)c->ndof, a, b, (v2d *)out2);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
int launch_deinterleave(feahip_ctx *c, const double *in2, double *a, double *b)
{
  hipLaunchKernelGGL(k2_deinterleave, g256((size_t)c->ndof), dim3(256), 0, c->stream, (size_t)c->ndof, (const v2d *)in2, a, b);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

static inline bool use_amg2(const feahip_ctx *c, int mode) { return mode != 0 && c->precond == 1; }

// one W-cycle for column col: its residual out of the paired r, z = M^-1 r into dst2's column (the cycle's result
// buffer is reused by the next call), the partial sums of r.z of the column
static int enq_cycle2(feahip_ctx *c, int col, double *dst2, const int *flag)
{
  const size_t n = (size_t)c->ndof;
  hipLaunchKernelGGL(k2_extract, g256(n), dim3(256), 0, c->stream, n, c->d2_r, col, c->d_r);
  const double *z = amg_apply(c, c->d_r);
  if (!z) return FEAHIP_EHIP;
  hipLaunchKernelGGL(k2_insert_dot, dim3(vgrid2(c)), dim3(256), 0, c->stream, n, z, c->d2_r, dst2, col,
                     c->d2_part + pslot(1, col), flag);
  return FEAHIP_OK;
}

// u2 = f2 ; r = f2 - K u2 ; p = M r ; the columns' scalars and flags (d2_f holds both right-hand sides)
static int enq_cg2_start(feahip_ctx *c, int mode, double tol)
{
  int rc;
  const bool amg = use_amg2(c, mode);
  if (amg) { if ((rc = amg_prepare(c))) return rc; }
  else if (mode != 0) enq_precond_blockjacobi(c);              // d_minv for the current K
  FEA_HIP_CHECK(c, hipMemcpyAsync(c->d2_u, c->d2_f, sizeof(double) * 2 * (size_t)c->ndof, hipMemcpyDeviceToDevice, c->stream));
  enq_spmv2(c, c->d2_u, c->d2_q, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(k2_cg_init, dim3(vgrid2(c)), dim3(256), 0, c->stream, 0, c->N, (const v2d *)c->d2_f, (const v2d *)c->d2_q,
                     (mode != 0 && !amg) ? c->d_minv : (const double *)nullptr, (v2d *)c->d2_r, (v2d *)c->d2_p, c->d2_part);
  if (amg)
    for (int col = 0; col < 2; ++col) if ((rc = enq_cycle2(c, col, c->d2_p, nullptr))) return rc;
  hipLaunchKernelGGL(k2_cg_init_scalars, dim3(1), dim3(256), 0, c->stream, vgrid2(c), c->d2_part, c->d2_scal, tol, c->d2_flag);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// live[col]: false once the host has seen the column's flag set (its cycles are skipped; the device skips the rest)
static int enq_cg2_iteration(feahip_ctx *c, int it, int mode, const bool *live)
{
  int rc;
  const bool amg = use_amg2(c, mode);
  enq_spmv2(c, c->d2_p, c->d2_q, c->d2_p, c->d2_part, c->d2_flag);
  hipLaunchKernelGGL(k2_cg_update, dim3(vgrid2(c)), dim3(256), 0, c->stream, 0, c->N, it, spmv2_grid(c), (const v2d *)c->d2_p,
                     (const v2d *)c->d2_q, (mode != 0 && !amg) ? c->d_minv : (const double *)nullptr, (v2d *)c->d2_u,
                     (v2d *)c->d2_r, c->d2_part, c->d2_scal, c->d2_flag, amg ? (v2d *)nullptr : (v2d *)c->d2_q);
  if (amg)
    for (int col = 0; col < 2; ++col)
      if (live[col] && (rc = enq_cycle2(c, col, c->d2_q, c->d2_flag))) return rc;
  hipLaunchKernelGGL(k2_cg_direction, dim3(vgrid2(c)), dim3(256), 0, c->stream, 0, c->N, it, vgrid2(c), (const v2d *)c->d2_q,
                     (v2d *)c->d2_p, c->d2_part, c->d2_scal, c->d2_flag);
  return FEAHIP_OK;
}

// Solves K [u, u2] = d2_f by two (preconditioned) CG recurrences started from the right-hand sides; the solutions go
// to d_u (column 0) and d_u2 (column 1).  The loop of dist_solve_pcg, variant 0, per column.
int solve_pcg2(feahip_ctx *c, int type, double tol, int max_iter, int *iters, double *resid)
{
  const int mode = (type == FEAHIP_CG) ? 0 : 1;
  if (type == FEAHIP_CHOLESKY) { tol = 1e-16; if (max_iter < 100000) max_iter = 100000; }
  int rc = enq_cg2_start(c, mode, tol);
  if (rc) return rc;
  int flag[2] = {0, 0}, it = 0;
  const int batch = use_amg2(c, mode) ? 8 : 32;
  while (it < max_iter) {
    const int n = (max_iter - it < batch) ? (max_iter - it) : batch;
    const bool live[2] = {flag[0] == 0, flag[1] == 0};
    for (int k = 0; k < n; ++k)
      if ((rc = enq_cg2_iteration(c, it + k, mode, live))) return rc;
    it += n;
    FEA_HIP_CHECK(c, hipGetLastError());
    FEA_HIP_CHECK(c, hipMemcpyAsync(flag, c->d2_flag, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (flag[0] != 0 && flag[1] != 0) break;
  }
  double sc[16];
  FEA_HIP_CHECK(c, hipMemcpyAsync(sc, c->d2_scal, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
  if ((rc = launch_deinterleave(c, c->d2_u, c->d_u, c->d_u2))) return rc;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d2_flag, 0, sizeof(int) * 2, c->stream));
  bool broke[2];
  for (int col = 0; col < 2; ++col)
    broke[col] = pcg_outcome(flag[col], it, sc + 8 * col, iters ? iters + col : nullptr, resid ? resid + col : nullptr);
  for (int col = 0; col < 2; ++col)
    if (broke[col]) {
      c->err = "CG breakdown (NaN or zero curvature) in column " + std::to_string(col) + " at iteration " + std::to_string(-flag[col]);
      return FEAHIP_ENOTCONVERGED;
    }
  return FEAHIP_OK;
}

// one two-column PCG iteration, timed (feahip_time_kernel(7)): both columns carry the context's f
int time_pcg2_iteration(feahip_ctx *c, int warmup, int iters, double *avg_ms)
{
  int rc;
  if ((rc = solve2_refused(c, "time_kernel(7)")) || (rc = ensure_solve2(c))) return rc;
  if ((rc = launch_interleave(c, c->d_f, c->d_f, c->d2_f))) return rc;
  if ((rc = enq_cg2_start(c, 1, 0.0))) return rc;
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d2_flag, 0, sizeof(int) * 2, c->stream));
  const bool live[2] = {true, true};
  if ((rc = time_enqueued(c, warmup, iters, avg_ms, [&](int k) { return enq_cg2_iteration(c, k, 1, live); }))) return rc;
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d2_flag, 0, sizeof(int) * 2, c->stream));
  return FEAHIP_OK;
}
