// kernels_modal.hip -- the lowest eigenpairs of K(x) phi = lambda M phi on the free dofs (feahip_solve_modes): a blocked
// LOBPCG whose basis is M-orthonormalised at every step, on block vectors of FEA_MODAL_COLS = 8 columns.
//
// Layout of a block vector: [3N][8] doubles, the eight columns of a scalar dof contiguous (64 bytes, half a cache
// line) -- the layout of kernels_solve2.hip carried from two columns to eight.  Nine of them live in one allocation
// (ModalState::d_v): S = [X, W, P], KS = [KX, KW, KP], MS = [MX, MW, MP].
//
// Per Rayleigh-Ritz step (struct Lobpcg, below enq_residual: the one iteration of all four drivers):
//   k_modal_residual  R = KX - MX diag(theta), the three column norms |r|^2, |Kx|^2, |Mx|^2 of every column, and (kind
//                     0) W = D^-1 R with the 3x3 block-Jacobi inverse, zero on the prescribed dofs -- one pass
//   k_spmm_km         KW = K W and MW = mask(M W) over ONE read of rowptr / colidx / K / m
//   k_modal_gram      G_M = S' MS and G_K = S' KS (24 x 24 each, the block-upper triangle) from the nine arrays in one
//                     pass, fixed grid, two-stage reduction in a fixed order, no atomics
//   (one read-back: 24 norms + 768 Gram sums; the host scales, eigendecomposes G_M by cyclic Jacobi, drops directions
//   below 1e-12 of the largest, forms the M-orthonormal basis, eigendecomposes the projected K and sends back two
//   24 x 8 coefficient matrices: modal_ritz)
//   k_modal_combine   [X, P] <- S [C_x, C_p] and the same for KS and MS, in place: only W is ever multiplied by the
//                     matrices; every 20 steps and at return KX and MX are recomputed from X.
// Nothing here exists, and nothing is launched, on a context that never calls feahip_solve_modes (or the hooks
// feahip_spmm_km, feahip_time_kernel 13-15) -- or feahip_solve_buckling, whose driver (kernels_buckling.hip) runs the same
// iteration on the pencil (K_sigma, K).
//
// More than eight modes, and bodies with zero-energy modes (feahip_solve_modes_locked, modal_solve_locked below): the
// same step in sweeps of the eight-column block on the pencil (K + shift M, M).  Converged leading columns are locked
// into a store of up to 64 modes Q with their products MQ = mask(M Q), panels of eight columns in the block-vector
// layout; the block is kept in the M-complement of the store by  W <- W - Q (MQ' W):
//   k_modal_deflate_gram    the L x 8 coefficients MQ' W: one read of W and of every MQ panel in use, fixed grid
//   k_modal_deflate_reduce  their per-workgroup partial sums in a fixed order; the coefficients stay on the device
//   k_modal_deflate_apply   W -= Q C: one read of W and of every Q panel in use, one write of W
// The store exists on a context that called feahip_solve_modes_locked (or feahip_modal_deflate, feahip_time_kernel
// 16-17) and on no other.
//
// Over the ranks of a sharded run (feahip_solve_modes_sharded, modal_solve_dist at the end of this file): the same
// iteration with a transport, every rank on the rows it owns.  The sums, the combination and the residual take the owned range [row0, row1);
// the halo rows of X and W travel as rows of 192 bytes (k_block_halo_pack / k_block_halo_unpack, Transport::
// exchange_block_begin / _end) under the product of the chunks that read no halo column; the 24 + 768 sums are
// all-reduced (Transport::allreduce_vec) before the one Rayleigh-Ritz step.  The block halo buffers and the row keys
// of the start block exist on a context that called the sharded solve (or feahip_group_spmm_km) and on no other.
#include "feahip_internal.h"
#include "reduce_device.h"
#include <cmath>

#define RB FEA_RED_BLOCKS
#define MC FEA_MODAL_COLS
static_assert(MC == 8, "the kernels below are written for eight columns (four 16-byte pairs per dof)");
typedef double v2d __attribute__((ext_vector_type(2)));

// multigrid preconditioner (amg.hip)
int amg_prepare(feahip_ctx *c);
double *amg_apply(feahip_ctx *c, const double *r);

// ------------------------------------------------------------------------
// Y = K X, Z = mask(M X) for eight columns in one pass over the pattern.  k_spmv2's chunking: a wave owns a chunk of up
// to 16 rows and 128 blocks, lane k takes the blocks k and k + 64, loads their nine K doubles, their m and the 3 x 8
// x entries of their column ONCE into registers, and then walks the columns in four pairs: per pair it leaves 3 rows x
// (K pair, M pair) = 96 bytes per block in LDS (12 KB per wave; all eight columns at once would take 48 KB per wave),
// and lane (row, i) adds its row's partial products in block order into register accumulators that are stored once,
// 64 bytes per dof and matrix.  A row longer than the tile has a chunk of its own: the lanes stride over its blocks,
// a butterfly per sum, pair by pair.  mask: 1 = prescribed dof (Z is zero there).
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_spmm_km(int chunk0, int nchunks, const int *__restrict__ chunk, const int *__restrict__ rowptr,
               const int *__restrict__ colidx, const double *__restrict__ K, const double *__restrict__ m,
               const uint8_t *__restrict__ mask, const v2d *__restrict__ x, v2d *__restrict__ y, v2d *__restrict__ z)
{
  static_assert(FEA_CHUNK_ROWS * 3 <= 64, "one lane per (row, component) of a chunk");
  static_assert(FEA_CHUNK_BLOCKS <= 128, "a lane takes the blocks k and k + 64 of a chunk");
  __shared__ __attribute__((aligned(16))) double sP[FEA_WAVES_PER_WG][FEA_CHUNK_BLOCKS * 12];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  v2d *tP2 = reinterpret_cast<v2d *>(sP[wave]);      // block k, row i: K pair at [6 k + 2 i], M pair at [6 k + 2 i + 1]
  for (int ch = chunk0 + blockIdx.x * FEA_WAVES_PER_WG + wave; ch < chunk0 + nchunks; ch += gridDim.x * FEA_WAVES_PER_WG) {
    const int r0 = chunk[ch], r1 = chunk[ch + 1];
    const int b0 = rowptr[r0], nb = rowptr[r1] - b0;
    if (nb > FEA_CHUNK_BLOCKS) {
      for (int p = 0; p < 4; ++p) {
        v2d aK[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}}, aM[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
        for (int k = lane; k < nb; k += 64) {
          const double *vp = K + (size_t)(b0 + k) * 9;
          const double mm = m[b0 + k];
          const size_t col = (size_t)colidx[b0 + k];
          const v2d x0 = x[(col * 3) * 4 + p], x1 = x[(col * 3 + 1) * 4 + p], x2 = x[(col * 3 + 2) * 4 + p];
          aK[0] += vp[0] * x0 + vp[1] * x1 + vp[2] * x2;
          aK[1] += vp[3] * x0 + vp[4] * x1 + vp[5] * x2;
          aK[2] += vp[6] * x0 + vp[7] * x1 + vp[8] * x2;
          aM[0] += mm * x0; aM[1] += mm * x1; aM[2] += mm * x2;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          aK[i].x = wave_sum_all(aK[i].x); aK[i].y = wave_sum_all(aK[i].y);
          aM[i].x = wave_sum_all(aM[i].x); aM[i].y = wave_sum_all(aM[i].y);
        }
        if (lane < 3) {
          const size_t d = (size_t)r0 * 3 + lane;
          const v2d zero = {0.0, 0.0};
          y[d * 4 + p] = lane == 0 ? aK[0] : lane == 1 ? aK[1] : aK[2];
          z[d * 4 + p] = mask[d] ? zero : (lane == 0 ? aM[0] : lane == 1 ? aM[1] : aM[2]);
        }
      }
      continue;
    }
    double v[2][9], mm[2];
    v2d xv[2][3][4];
    int kb = 0, ke = 0;
    if (lane < (r1 - r0) * 3) { kb = rowptr[r0 + lane / 3] - b0; ke = rowptr[r0 + lane / 3 + 1] - b0; }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      const int kk = k < nb ? b0 + k : b0;
      const double *vp = K + (size_t)kk * 9;
#pragma unroll
      for (int q = 0; q < 9; ++q) v[h][q] = vp[q];
      mm[h] = m[kk];
      const size_t col = (size_t)colidx[kk];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int p = 0; p < 4; ++p) xv[h][i][p] = x[(col * 3 + i) * 4 + p];
    }
    v2d accK[4], accM[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      accK[p] = v2d{0.0, 0.0}; accM[p] = v2d{0.0, 0.0};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        if (k < nb) {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            tP2[k * 6 + 2 * i] = v[h][3 * i] * xv[h][0][p] + v[h][3 * i + 1] * xv[h][1][p] + v[h][3 * i + 2] * xv[h][2][p];
            tP2[k * 6 + 2 * i + 1] = mm[h] * xv[h][i][p];
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      if (lane < (r1 - r0) * 3) {
        const int i = lane % 3;
        for (int k = kb; k < ke; ++k) { accK[p] += tP2[k * 6 + 2 * i]; accM[p] += tP2[k * 6 + 2 * i + 1]; }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    if (lane < (r1 - r0) * 3) {
      const size_t d = (size_t)r0 * 3 + lane;
      const bool fixed = mask[d] != 0;
      const v2d zero = {0.0, 0.0};
#pragma unroll
      for (int p = 0; p < 4; ++p) { y[d * 4 + p] = accK[p]; z[d * 4 + p] = fixed ? zero : accM[p]; }
    }
  }
}

// ------------------------------------------------------------------------
// G_M = S' MS and G_K = S' KS from the nine arrays in one pass.  base + j stride is array j of X W P KX KW KP MX MW MP;
// np = the column blocks of S in use (1: X alone, 2: X and W, 3: all; the others count as zero and are not read).
// A workgroup stages 32 dofs x 9 arrays in LDS with coalesced loads; wave w takes eight of them, lane (a, b) keeps the
// twelve sums s_A[a] ms_B[b], s_A[a] ks_B[b] of the six block pairs A <= B.  The four waves' sums meet in LDS in wave
// order, and the 768 sums of the workgroup go to part[(24 + e) RB + block].
// ------------------------------------------------------------------------
#define GRAM_DOFS 32
__global__ __launch_bounds__(256)
void k_modal_gram(int ndof, int np, const double *__restrict__ base, size_t stride, double *__restrict__ part)
{
  __shared__ double sh[4 * 12 * 64];                   // the tile [9][32][8] first (2304 doubles), the waves' sums after
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, a = lane >> 3, b = lane & 7;
  double acc[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) acc[q] = 0.0;
  for (int j = 0; j < 9; ++j) sh[j * 256 + threadIdx.x] = 0.0;        // arrays not in use stay zero
  const int ntiles = (ndof + GRAM_DOFS - 1) / GRAM_DOFS;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t e = (size_t)tile * (GRAM_DOFS * 8) + threadIdx.x;      // element of a block vector
    const bool in = e < (size_t)ndof * 8;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 9; ++j)
      if (j % 3 < np) sh[j * 256 + threadIdx.x] = in ? base[(size_t)j * stride + e] : 0.0;
    __syncthreads();
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const int row = (wave * 8 + d) * 8;
      const double s0 = sh[row + a], s1 = sh[256 + row + a], s2 = sh[512 + row + a];
      const double k0 = sh[768 + row + b], k1 = sh[1024 + row + b], k2 = sh[1280 + row + b];
      const double m0 = sh[1536 + row + b], m1 = sh[1792 + row + b], m2 = sh[2048 + row + b];
      acc[0] += s0 * m0; acc[1] += s0 * m1; acc[2] += s0 * m2; acc[3] += s1 * m1; acc[4] += s1 * m2; acc[5] += s2 * m2;
      acc[6] += s0 * k0; acc[7] += s0 * k1; acc[8] += s0 * k2; acc[9] += s1 * k1; acc[10] += s1 * k2; acc[11] += s2 * k2;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 12; ++q) sh[(wave * 12 + q) * 64 + lane] = acc[q];
  __syncthreads();
  for (int e = threadIdx.x; e < MODAL_GRAM; e += 256)
    part[(size_t)(MODAL_NORMS + e) * RB + blockIdx.x] = ((sh[e] + sh[768 + e]) + sh[1536 + e]) + sh[2304 + e];
}

// out[e] = the sum of part[e RB .. e RB + n): n = n_norms for e < 24, n_gram after; one workgroup per sum
__global__ __launch_bounds__(256)
void k_modal_reduce(int e0, int n_norms, int n_gram, const double *__restrict__ part, double *__restrict__ out)
{
  __shared__ double scratch[5];
  const int e = e0 + blockIdx.x;
  const double v = reduce_partials(part + (size_t)e * RB, e < MODAL_NORMS ? n_norms : n_gram, scratch);
  if (threadIdx.x == 0) out[e] = v;
}

// ------------------------------------------------------------------------
// [X, P] <- S C for the three triples (blockIdx.y = 0: S, 1: KS, 2: MS), in place: a lane owns one dof, reads its np x 8
// entries, and writes the eight of X and (write_p) the eight of P.  C[24][16]: row k = direction k of S, columns 0-7
// the coefficients of X_new, 8-15 those of P_new; it is read with uniform addresses (scalar loads), the same for
// every lane.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_modal_combine(int ndof, int np, int write_p, double *__restrict__ base, size_t stride, const double *__restrict__ C)
{
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= ndof) return;
  v2d *X = reinterpret_cast<v2d *>(base + (size_t)(3 * blockIdx.y) * stride) + (size_t)d * 4;
  v2d *W = reinterpret_cast<v2d *>(base + (size_t)(3 * blockIdx.y + 1) * stride) + (size_t)d * 4;
  v2d *P = reinterpret_cast<v2d *>(base + (size_t)(3 * blockIdx.y + 2) * stride) + (size_t)d * 4;
  double xo[8], po[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) { xo[q] = 0.0; po[q] = 0.0; }
  auto add = [&](const v2d *src, int row0) {
    double s[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) { const v2d t = src[p]; s[2 * p] = t.x; s[2 * p + 1] = t.y; }
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        xo[q] += s[k] * C[(row0 + k) * 16 + q];
        po[q] += s[k] * C[(row0 + k) * 16 + 8 + q];
      }
  };
  add(X, 0);
  if (np > 1) add(W, 8);
  if (np > 2) add(P, 16);
#pragma unroll
  for (int p = 0; p < 4; ++p) X[p] = v2d{xo[2 * p], xo[2 * p + 1]};
  if (write_p) {
#pragma unroll
    for (int p = 0; p < 4; ++p) P[p] = v2d{po[2 * p], po[2 * p + 1]};
  }
}

// ------------------------------------------------------------------------
// R = KX - MX diag(theta) and the sums |r|^2, |Kx|^2, |Mx|^2 of every column; W = D^-1 R (minv: the 3x3 block-Jacobi
// inverse, row i of node a at 9 a + 3 i) or, with minv null, W = R (the multigrid cycles follow); W is zero on the
// prescribed dofs.  A lane owns (node, column): eight lanes share a node and read its D^-1 block together.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_modal_residual(int N, const double *__restrict__ KX, const double *__restrict__ MX, const double *__restrict__ theta,
                      const double *__restrict__ minv, const uint8_t *__restrict__ mask, double *__restrict__ W,
                      double *__restrict__ part)
{
  __shared__ double sh[4][MODAL_NORMS];
  const int col = threadIdx.x & 7, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double th = theta[col];
  double s[3] = {0.0, 0.0, 0.0};
  for (int a = blockIdx.x * 32 + (threadIdx.x >> 3); a < N; a += gridDim.x * 32) {
    double r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const size_t e = ((size_t)a * 3 + j) * 8 + col;
      const double kx = KX[e], mx = MX[e];
      r[j] = kx - th * mx;
      s[0] += r[j] * r[j]; s[1] += kx * kx; s[2] += mx * mx;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double w = r[i];
      if (minv) { const double *mi = minv + (size_t)a * 9 + 3 * i; w = mi[0] * r[0] + mi[1] * r[1] + mi[2] * r[2]; }
      W[((size_t)a * 3 + i) * 8 + col] = mask[(size_t)a * 3 + i] ? 0.0 : w;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int off = 32; off >= 8; off >>= 1) s[k] += __shfl_xor(s[k], off, 64);     // the lanes of one column
    if (lane < 8) sh[wave][k * 8 + lane] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < MODAL_NORMS)
    part[(size_t)threadIdx.x * RB + blockIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// the start block: a fixed integer hash of (library dof index, column) mapped to [-1, 1), zero on the prescribed dofs
__device__ __forceinline__ double modal_hash_value(uint32_t dof, uint32_t col)
{
  uint32_t h = dof * 0x9E3779B1u ^ (col + 1u) * 0x85EBCA77u;
  h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
  return (double)h * (1.0 / 2147483648.0) - 1.0;
}
__global__ __launch_bounds__(256)
void k_modal_hash(size_t n8, const uint8_t *__restrict__ mask, double *__restrict__ X)
{
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n8) return;
  X[e] = mask[e >> 3] ? 0.0 : modal_hash_value((uint32_t)(e >> 3), (uint32_t)(e & 7));
}
// the same on the owned rows of a sharded context, keyed by the node's identity in the whole mesh (key[a] for the a-th
// owned row; null: row0 + a, the library id of a row shard), so that the start block does not depend on the cut.
// mask and X point at the first owned row.
__global__ __launch_bounds__(256)
void k_modal_hash_rows(int nrows, int row0, const int *__restrict__ key, const uint8_t *__restrict__ mask, double *__restrict__ X)
{
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)nrows * 24) return;
  const int a = (int)(e / 24), j = (int)((e >> 3) % 3);
  const uint32_t node = (uint32_t)(key ? key[a] : row0 + a);
  X[e] = mask[e >> 3] ? 0.0 : modal_hash_value(node * 3u + (uint32_t)j, (uint32_t)(e & 7));
}

// ------------------------------------------------------------------------
// Halo rows of a block vector (the sharded solve).  A node's three dofs are 24 contiguous doubles of the [3N][8]
// layout: a row travels as twelve 16-byte lanes, lane t of the launch moves lane t % 12 of row t / 12, so a wave reads
// and writes runs of 192 contiguous bytes.  buf: [n][24].
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void k_block_halo_pack(int n, const int *__restrict__ idx, const v2d *__restrict__ v, v2d *__restrict__ buf)
{
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * 12) return;
  buf[t] = v[(size_t)idx[t / 12] * 12 + t % 12];
}
__global__ __launch_bounds__(256)
void k_block_halo_unpack(int n, const int *__restrict__ idx, const v2d *__restrict__ buf, v2d *__restrict__ v)
{
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * 12) return;
  v[(size_t)idx[t / 12] * 12 + t % 12] = buf[t];
}
// test knob of the in-process transport (FEAHIP_TEST_POISON_HALO): the halo rows become NaN
__global__ __launch_bounds__(256)
void k_block_halo_poison(int n, const int *__restrict__ idx, v2d *__restrict__ v)
{
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * 12) return;
  v[(size_t)idx[t / 12] * 12 + t % 12] = v2d{__builtin_nan(""), __builtin_nan("")};
}

// a column out of a block vector, and a vector (a multigrid cycle's result) into one, zero on the prescribed dofs
__global__ void k_modal_extract(size_t n, const double *__restrict__ in8, int col, double *__restrict__ out)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = in8[k * 8 + col];
}
__global__ void k_modal_insert(size_t n, const double *__restrict__ zv, const uint8_t *__restrict__ mask, int col, double *__restrict__ dst8)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) dst8[k * 8 + col] = mask[k] ? 0.0 : zv[k];
}
// eight plain vectors [8][n] (the hooks' host layout) into a block vector, or (unpack) back
__global__ void k_modal_pack(size_t n, const double *__restrict__ in, double *__restrict__ out8, int unpack)
{
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * 8) return;
  const size_t k = e >> 3, col = e & 7;
  if (unpack) out8[col * n + k] = in[e]; else out8[e] = in[col * n + k];
}

// ------------------------------------------------------------------------
// The locked store (feahip_solve_modes_locked).  Q and MQ: npanels panels [3N][8] each, pstride doubles apart; the
// columns of the last panel that hold no mode are zero.
//
// C_p = MQ_p' W for every panel p < npanels in one pass: k_modal_gram's staging -- a workgroup stages 32 dofs of W and
// of every panel in LDS with coalesced loads (W's tile once, not once per panel); wave w takes eight of the dofs, lane
// (a, b) keeps mq_p[a] w[b] for each panel.  The four waves' sums meet in LDS in wave order and go to
// part[(p 64 + a 8 + b) RB + block].  The reads of a wave are eight consecutive doubles (broadcast over the other
// index): conflict-free.
// ------------------------------------------------------------------------
#define MODAL_PANELS (FEA_MODAL_MAX_LOCKED / MC)
static_assert(MODAL_PANELS == 8, "the panel loops below are unrolled eight times");
__global__ __launch_bounds__(256)
void k_modal_deflate_gram(int ndof, int npanels, const double *__restrict__ W, const double *__restrict__ MQ, size_t pstride,
                          double *__restrict__ part)
{
  __shared__ double sh[(1 + MODAL_PANELS) * 256];      // the tile [1 + 8][32][8] first, the waves' sums [4][8][64] after
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, a = lane >> 3, b = lane & 7;
  double acc[MODAL_PANELS];
#pragma unroll
  for (int p = 0; p < MODAL_PANELS; ++p) acc[p] = 0.0;
  const int ntiles = (ndof + GRAM_DOFS - 1) / GRAM_DOFS;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t e = (size_t)tile * (GRAM_DOFS * 8) + threadIdx.x;      // element of a block vector
    const bool in = e < (size_t)ndof * 8;
    __syncthreads();
    sh[threadIdx.x] = in ? W[e] : 0.0;
#pragma unroll
    for (int p = 0; p < MODAL_PANELS; ++p)
      if (p < npanels) sh[(1 + p) * 256 + threadIdx.x] = in ? MQ[(size_t)p * pstride + e] : 0.0;
    __syncthreads();
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const int row = (wave * 8 + d) * 8;
      const double w = sh[row + b];
#pragma unroll
      for (int p = 0; p < MODAL_PANELS; ++p)
        if (p < npanels) acc[p] += sh[(1 + p) * 256 + row + a] * w;
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < MODAL_PANELS; ++p) sh[(wave * MODAL_PANELS + p) * 64 + lane] = acc[p];
  __syncthreads();
  for (int e = threadIdx.x; e < npanels * 64; e += 256)
    part[(size_t)e * RB + blockIdx.x] = ((sh[e] + sh[512 + e]) + sh[1024 + e]) + sh[1536 + e];
}

// out[e] = the sum of part[e RB .. e RB + n), one workgroup per coefficient (k_modal_reduce's order)
__global__ __launch_bounds__(256)
void k_modal_deflate_reduce(int n, const double *__restrict__ part, double *__restrict__ out)
{
  __shared__ double scratch[5];
  const double v = reduce_partials(part + (size_t)blockIdx.x * RB, n, scratch);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// W -= sum_p Q_p C_p: a lane owns one dof, reads its 64 bytes of W once and 64 bytes of every panel in use, and
// writes W once.  C[p][a][b] (mode a of panel p, column b) is read with uniform addresses, as k_modal_combine reads
// its coefficients.  Q is zero on the prescribed dofs, so W stays zero there.
__global__ __launch_bounds__(256)
void k_modal_deflate_apply(int ndof, int npanels, double *__restrict__ W, const double *__restrict__ Q, size_t pstride,
                           const double *__restrict__ C)
{
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= ndof) return;
  v2d *Wd = reinterpret_cast<v2d *>(W) + (size_t)d * 4;
  double w[8];
#pragma unroll
  for (int p = 0; p < 4; ++p) { const v2d t = Wd[p]; w[2 * p] = t.x; w[2 * p + 1] = t.y; }
  for (int p = 0; p < npanels; ++p) {
    const v2d *Qd = reinterpret_cast<const v2d *>(Q + (size_t)p * pstride) + (size_t)d * 4;
    double q[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) { const v2d t = Qd[k]; q[2 * k] = t.x; q[2 * k + 1] = t.y; }
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) w[j] -= q[k] * C[p * 64 + k * 8 + j];
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) Wd[p] = v2d{w[2 * p], w[2 * p + 1]};
}

// columns [0, count) of X and of MX into the modes [at, at + count) of the store
__global__ __launch_bounds__(256)
void k_modal_lock(int ndof, int at, int count, const double *__restrict__ X, const double *__restrict__ MX,
                  double *__restrict__ Q, double *__restrict__ MQ, size_t pstride)
{
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= ndof) return;
  for (int j = 0; j < count; ++j) {
    const size_t to = (size_t)((at + j) >> 3) * pstride + (size_t)d * 8 + ((at + j) & 7);
    Q[to] = X[(size_t)d * 8 + j];
    MQ[to] = MX[(size_t)d * 8 + j];
  }
}

// the next block of a sweep: the columns [drop, 8) of X move to the front; the columns freed are k_modal_hash's values
// for the column indices id0, id0 + 1, ... (indices no block has used before)
__global__ __launch_bounds__(256)
void k_modal_advance(int ndof, int drop, int id0, const uint8_t *__restrict__ mask, double *__restrict__ X)
{
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= ndof) return;
  double x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = X[(size_t)d * 8 + j];
  const bool fixed = mask[d] != 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) if (k == j + drop) v = x[k];
    if (j + drop >= 8) v = fixed ? 0.0 : modal_hash_value((uint32_t)d, (uint32_t)(id0 + j + drop - 8));
    X[(size_t)d * 8 + j] = v;
  }
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
static inline dim3 g256(size_t n) { return dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)); }
// The sums, the combination and the residual run on the rows the context owns, [row0, row1): all of them on an
// unsharded context, where these are the launches they always were (base pointers + 0, the same counts and grids).
static inline int own_nodes(const feahip_ctx *c) { return c->row1 - c->row0; }
static inline int own_dofs(const feahip_ctx *c) { return 3 * (c->row1 - c->row0); }
static inline size_t own_off8(const feahip_ctx *c) { return (size_t)3 * c->row0 * MC; }   // of row0 in a block vector
static int gram_grid(const feahip_ctx *c)
{
  const int g = (own_dofs(c) + GRAM_DOFS - 1) / GRAM_DOFS;
  return g < RB ? (g > 0 ? g : 1) : RB;
}
static int resid_grid(const feahip_ctx *c)
{
  const int g = (own_nodes(c) + 31) / 32;
  return g < RB ? (g > 0 ? g : 1) : RB;
}

int ensure_modal(feahip_ctx *c)
{
  ModalState &S = c->modal;
  S.have_buckling = false;                                            // every caller makes the block its own
  S.have_sharded = false;                                             // (ensure_modal_dist keeps it for the sharded solve)
  if (S.d_v) return FEAHIP_OK;
  const size_t n8 = (size_t)c->ndof * MC;
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_v, sizeof(double) * 9 * n8));
  FEA_HIP_CHECK(c, hipMemsetAsync(S.d_v, 0, sizeof(double) * 9 * n8, c->stream));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_part, sizeof(double) * (size_t)MODAL_SUMS * RB));
  FEA_HIP_CHECK(c, hipMemsetAsync(S.d_part, 0, sizeof(double) * (size_t)MODAL_SUMS * RB, c->stream));
  FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_small, sizeof(double) * MODAL_SMALL));
  FEA_HIP_CHECK(c, hipMemsetAsync(S.d_small, 0, sizeof(double) * MODAL_SMALL, c->stream));
  // the prescribed-dof mask is the context's own byte array (d_dofmask, built once from d_cdof); its free dofs
  std::vector<uint8_t> hm((size_t)c->ndof);
  FEA_HIP_CHECK(c, hipMemcpyAsync(hm.data(), c->d_dofmask, hm.size(), hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  S.n_free = 0;
  for (uint8_t b : hm) S.n_free += b ? 0 : 1;
  S.have = false;
  return FEAHIP_OK;
}

static inline double *mv(feahip_ctx *c, int j) { return c->modal.d_v + (size_t)j * c->ndof * MC; }

// the one launch of k_spmm_km: the full range, the interior and boundary ranges of a rank, either pencil.  A row's sums are
// formed by one wave in block order, so the cut of the launches changes no bit
int launch_spmm_km(feahip_ctx *c, int first, int n, const double *d_m, const double *d_x8, double *d_y8, double *d_z8)
{
  const int g = (n + FEA_WAVES_PER_WG - 1) / FEA_WAVES_PER_WG;
  hipLaunchKernelGGL(k_spmm_km, dim3(g < RB ? (g > 0 ? g : 1) : RB), dim3(256), 0, c->stream, c->chunk0 + first, n, c->d_chunk,
                     c->d_rowptr, c->d_colidx, (const double *)c->d_K, d_m, (const uint8_t *)c->d_dofmask, (const v2d *)d_x8,
                     (v2d *)d_y8, (v2d *)d_z8);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
int launch_modal_hash(feahip_ctx *c, double *d_v8)
{
  const size_t n8 = (size_t)c->ndof * MC;
  hipLaunchKernelGGL(k_modal_hash, g256(n8), dim3(256), 0, c->stream, n8, (const uint8_t *)c->d_dofmask, d_v8);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

static void enq_gram(feahip_ctx *c, int np)
{
  hipLaunchKernelGGL(k_modal_gram, dim3(gram_grid(c)), dim3(256), 0, c->stream, own_dofs(c), np,
                     (const double *)(c->modal.d_v + own_off8(c)), (size_t)c->ndof * MC, c->modal.d_part);
}
static void enq_combine(feahip_ctx *c, int np, int write_p)
{
  if (own_dofs(c) <= 0) return;                                       // (a rank without rows)
  hipLaunchKernelGGL(k_modal_combine, dim3((own_dofs(c) + 255) / 256, 3), dim3(256), 0, c->stream, own_dofs(c), np, write_p,
                     c->modal.d_v + own_off8(c), (size_t)c->ndof * MC, (const double *)(c->modal.d_small + MODAL_SUMS));
}
// hooks of feahip_time_kernel 13, 14, 15: the product on X, the Gram pass and the combination (with the identity: the
// vectors stay as they are) on all nine arrays
int time_modal_kernel(feahip_ctx *c, int what)
{
  if (what == 13) return launch_spmm_km(c, 0, c->nchunks_local, c->mass.d_m, mv(c, V_X), mv(c, V_KX), mv(c, V_MX));
  if (what == 14) enq_gram(c, 3);
  else enq_combine(c, 3, 1);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}
int time_modal_prepare(feahip_ctx *c)
{
  int rc;
  if ((rc = ensure_modal(c))) return rc;
  ModalState &S = c->modal;
  S.have = false;                                                     // the vectors are scratch from here on
  for (int j : {V_X, V_W, V_P}) if ((rc = launch_modal_hash(c, mv(c, j)))) return rc;
  S.h_C.assign(24 * 16, 0.0);
  for (int k = 0; k < 8; ++k) { S.h_C[(size_t)k * 16 + k] = 1.0; S.h_C[(size_t)(16 + k) * 16 + 8 + k] = 1.0; }   // X <- X, P <- P
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.d_small + MODAL_SUMS, S.h_C.data(), sizeof(double) * 24 * 16, hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

// [8][3N] host-ordered device vectors (library ids) to a block vector and back
int launch_modal_pack(feahip_ctx *c, const double *d_in, double *d_out, int unpack)
{
  hipLaunchKernelGGL(k_modal_pack, g256((size_t)c->ndof * MC), dim3(256), 0, c->stream, (size_t)c->ndof, d_in, d_out, unpack);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// ---- the Rayleigh-Ritz step on the host ---------------------------------------------------------------------------
// cyclic Jacobi: A (n x n, symmetric, row-major, destroyed) = V diag(w) V'; a fixed sweep order, so the same input gives
// the same bits
static void jacobi_eig(int n, double *A, double *V, double *w)
{
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int i = 0; i < n; ++i) { dia += A[i * n + i] * A[i * n + i]; for (int j = i + 1; j < n; ++j) off += A[i * n + j] * A[i * n + j]; }
    if (!(off > 1e-36 * dia)) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        const double tau = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
        for (int k = 0; k < n; ++k) {
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = cs * akp - sn * akq; A[k * n + q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = cs * apk - sn * aqk; A[q * n + k] = sn * apk + cs * aqk;
        }
        A[p * n + q] = A[q * n + p] = 0.0;
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = cs * vkp - sn * vkq; V[k * n + q] = sn * vkp + cs * vkq;
        }
      }
  }
  for (int i = 0; i < n; ++i) w[i] = A[i * n + i];
}

// GM, GK: ns x ns (ns = 8, 16 or 24), symmetric, row-major, of S = [X, W, P].  theta[m] ascending, C[ns][2 m]: columns
// 0..m-1 the coefficients of X_new = S C_x, m..2m-1 those of P_new = X_new - X C_x[X rows].  Returns the rank of the
// basis kept, or -1 when fewer than m directions are left or a sum is not finite.
int modal_ritz(int ns, const double *GM, const double *GK, int m, double *theta, double *C)
{
  if (ns < m || ns > 24 || m > MC) return -1;
  double A[24 * 24], V[24 * 24], w[24], d[24], Q[24 * 24], T[24 * 24], Z[24 * 24], t[24], GQ[24 * 24];
  for (int i = 0; i < ns * ns; ++i) if (!std::isfinite(GM[i]) || !std::isfinite(GK[i])) return -1;
  for (int i = 0; i < ns; ++i) d[i] = GM[i * ns + i] > 0.0 ? 1.0 / sqrt(GM[i * ns + i]) : 0.0;
  for (int i = 0; i < ns; ++i) for (int j = 0; j < ns; ++j) A[i * ns + j] = d[i] * GM[i * ns + j] * d[j];
  jacobi_eig(ns, A, V, w);
  double wmax = 0.0;
  for (int i = 0; i < ns; ++i) wmax = w[i] > wmax ? w[i] : wmax;
  int r = 0;
  for (int k = 0; k < ns; ++k)
    if (w[k] > 1e-12 * wmax) {
      const double s = 1.0 / sqrt(w[k]);
      for (int i = 0; i < ns; ++i) Q[i * ns + r] = d[i] * V[i * ns + k] * s;
      ++r;
    }
  if (r < m) return -1;
  for (int i = 0; i < ns; ++i)
    for (int k = 0; k < r; ++k) { double s = 0.0; for (int j = 0; j < ns; ++j) s += GK[i * ns + j] * Q[j * ns + k]; GQ[i * ns + k] = s; }
  for (int a = 0; a < r; ++a)
    for (int b = a; b < r; ++b) {
      double s1 = 0.0, s2 = 0.0;
      for (int i = 0; i < ns; ++i) { s1 += Q[i * ns + a] * GQ[i * ns + b]; s2 += Q[i * ns + b] * GQ[i * ns + a]; }
      T[a * r + b] = T[b * r + a] = 0.5 * (s1 + s2);
    }
  jacobi_eig(r, T, Z, t);
  int order[24];
  for (int k = 0; k < r; ++k) order[k] = k;
  std::stable_sort(order, order + r, [&](int x, int y) { return t[x] < t[y]; });
  for (int j = 0; j < m; ++j) {
    theta[j] = t[order[j]];
    for (int i = 0; i < ns; ++i) {
      double s = 0.0;
      for (int k = 0; k < r; ++k) s += Q[i * ns + k] * Z[k * r + order[j]];
      C[i * 2 * m + j] = s;
    }
  }
  // P_new = X_new - X C_x[X rows] = [W, P] C_x[W, P rows]: the part of the new Ritz vectors that is not X.  It spans,
  // with X_new, the same space as X_new - X (X' M X_new) does, and is formed from the small directions alone -- the
  // other form subtracts two O(1) coefficients to get one of the size of P, and the recurrences for K P and M P then
  // carry that cancellation: with all eight columns wanted it stalled at 1e-5 on a 108-dof bar and then diverged
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < ns; ++i) C[i * 2 * m + m + j] = i < m ? 0.0 : C[i * 2 * m + j];
  return r;
}

namespace {
// the Gram matrices of np column blocks out of the 768 reduced sums
void unpack_gram(const double *sums, int np, double *GM, double *GK)
{
  static const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {0, 1, 2, 1, 2, 2};
  const int ns = 8 * np;
  for (int q = 0; q < 6; ++q) {
    if (pb[q] >= np) continue;
    for (int a = 0; a < 8; ++a)
      for (int b = 0; b < 8; ++b) {
        if (pa[q] == pb[q] && b < a) continue;                          // the upper triangle of a diagonal block
        const int i = pa[q] * 8 + a, j = pb[q] * 8 + b;
        GM[i * ns + j] = GM[j * ns + i] = sums[q * 64 + a * 8 + b];
        GK[i * ns + j] = GK[j * ns + i] = sums[(6 + q) * 64 + a * 8 + b];
      }
  }
}
}

// R (and W) of the current X, KX, MX and theta; precond: W = M^-1 R with the context's preconditioner
static int enq_residual(feahip_ctx *c, bool precond)
{
  ModalState &S = c->modal;
  const bool amg = c->precond == 1;
  const size_t o8 = own_off8(c), o = (size_t)3 * c->row0;
  hipLaunchKernelGGL(k_modal_residual, dim3(resid_grid(c)), dim3(256), 0, c->stream, own_nodes(c),
                     (const double *)(mv(c, V_KX) + o8), (const double *)(mv(c, V_MX) + o8),
                     (const double *)(S.d_small + MODAL_SUMS + 24 * 16),
                     (precond && !amg) ? (const double *)(c->d_minv + 3 * o) : (const double *)nullptr,
                     (const uint8_t *)(c->d_dofmask + o), mv(c, V_W) + o8, S.d_part);
  if (precond && amg) {
    // one W-cycle per column: its residual out of the block, the cycle, its result into the block (enq_cycle2); on
    // a sharded context the cycle is the rank's own (its diagonal block of K), as in the sharded PCG
    const size_t n = (size_t)own_dofs(c);
    for (int col = 0; col < MC; ++col) {
      hipLaunchKernelGGL(k_modal_extract, g256(n), dim3(256), 0, c->stream, n, (const double *)(mv(c, V_W) + o8), col, c->d_r + o);
      const double *zv = amg_apply(c, c->d_r);
      if (!zv) return FEAHIP_EHIP;
      hipLaunchKernelGGL(k_modal_insert, g256(n), dim3(256), 0, c->stream, n, zv + o, (const uint8_t *)(c->d_dofmask + o), col,
                         mv(c, V_W) + o8);
    }
  }
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// ---- the iteration of all four drivers (struct Lobpcg, feahip_internal.h) ------------------------------------------------
// Per step on R, the ranks this process drives (one unsharded context; all members of an in-process group; the one
// context of an RCCL rank).  Every rank keeps the nine block vectors of its own context; a vector is authoritative on
// the owned rows [row0, row1) -- all rows without a transport -- and the halo rows of X and W hold what the block
// exchange last brought:
//   residual, preconditioner          owned rows; kind 1: one W-cycle per column on the rank's own diagonal block
//   (after_residual: the locked solve deflates W)
//   products of W                     without a transport ONE launch of k_spmm_km over all chunks.  With one:
//     exchange_block_begin(W)           pack on the context's stream, copies and unpack on the communication stream
//     k_spmm_km on the interior chunks  they read no halo column (install_plan), so they run under the exchange
//     exchange_block_end, k_spmm_km on the chunks before and after the interior range
//   k_modal_gram, k_modal_reduce      owned rows; 24 + 768 sums into d_small; with a transport copied into d_vred and
//   Transport::allreduce_vec          summed over the ranks (in a group the sums meet on the host in rank order)
//   (one read-back; modal_ritz once on the sums; C and theta uploaded to every rank of R)
//   k_modal_combine                   owned rows
// Every branch depends on the (all-reduced) sums alone, so all ranks take it together.
#define EACH_RANK(c) for (feahip_ctx *c : R) if (!T || hipSetDevice(c->device) == hipSuccess)   // (one context: its device is current)
Lobpcg::Lobpcg(const std::vector<feahip_ctx *> &ranks, Transport *transport, double tolerance)
  : R(ranks), T(transport), tol(tolerance), theta(ranks[0]->modal.theta)
{
  R[0]->modal.h_C.assign(24 * 16 + MC, 0.0);
}

// block vectors [jk, jm] <- [K, mask(M)] jx on the owned rows of every rank, the halo rows of jx by exchange; geometric:
// [jm, jk] <- [K, mask(K_sigma)] jx
static int block_products(std::vector<feahip_ctx *> &R, Transport *T, bool geometric, int jx, int jk, int jm)
{
  int rc;
  auto spmm = [&](feahip_ctx *c, int first, int n) {
    return launch_spmm_km(c, first, n, geometric ? c->buckling.d_kg : c->mass.d_m, mv(c, jx), mv(c, geometric ? jm : jk),
                          mv(c, geometric ? jk : jm));
  };
  if (!T) return spmm(R[0], 0, R[0]->nchunks_local);
  std::vector<double *> xs;
  for (feahip_ctx *c : R) xs.push_back(mv(c, jx));
  if ((rc = T->exchange_block_begin(R, xs))) return rc;
  FOR_RANKS(c) { if (c->ichunk_hi > c->ichunk_lo && (rc = spmm(c, c->ichunk_lo, c->ichunk_hi - c->ichunk_lo))) return rc; }
  if ((rc = T->exchange_block_end(R))) return rc;
  FOR_RANKS(c) {                                                        // (an empty range of a rank is not launched)
    if (c->ichunk_lo > 0 && (rc = spmm(c, 0, c->ichunk_lo))) return rc;
    if (c->nchunks_local > c->ichunk_hi && (rc = spmm(c, c->ichunk_hi, c->nchunks_local - c->ichunk_hi))) return rc;
  }
  return FEAHIP_OK;
}
int Lobpcg::products(int jx, int jk, int jm) { return block_products(R, T, geometric, jx, jk, jm); }

int Lobpcg::upload()                                  // (h_C is not touched again before the next read-back)
{
  std::vector<double> &h_C = R[0]->modal.h_C;
  for (int j = 0; j < MC; ++j) h_C[24 * 16 + j] = theta[j];
  EACH_RANK(c) {
    FEA_HIP_CHECK(c, hipMemcpyAsync(c->modal.d_small + MODAL_SUMS, h_C.data(), sizeof(double) * (24 * 16 + MC), hipMemcpyHostToDevice, c->stream));
  }
  return FEAHIP_OK;
}

int Lobpcg::enq_residual(bool precond)
{
  int rc;
  EACH_RANK(c) { if ((rc = ::enq_residual(c, precond))) return rc; }
  return FEAHIP_OK;
}

// every rank's sums reduced into its d_small; with a transport copied into d_vred and summed over the ranks, so that every
// rank holds, and this process reads, the same bits
int Lobpcg::read_sums(int e0, int n)
{
  int rc;
  EACH_RANK(c) {
    hipLaunchKernelGGL(k_modal_reduce, dim3(n), dim3(256), 0, c->stream, e0, resid_grid(c), gram_grid(c),
                       (const double *)c->modal.d_part, c->modal.d_small);
    FEA_HIP_CHECK(c, hipGetLastError());
    if (T) FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_vred, c->modal.d_small + e0, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  }
  if (T && (rc = T->allreduce_vec(R, (size_t)n, false))) return rc;
  feahip_ctx *c0 = R[0];
  if (T) (void)hipSetDevice(c0->device);
  FEA_HIP_CHECK(c0, hipMemcpyAsync(sums + e0, T ? c0->d_vred : c0->modal.d_small + e0, sizeof(double) * n, hipMemcpyDeviceToHost, c0->stream));
  FEA_HIP_CHECK(c0, hipStreamSynchronize(c0->stream));
  return FEAHIP_OK;
}

int Lobpcg::fresh_norms()
{
  int rc;
  if ((rc = enq_residual(false))) return rc;
  return read_sums(0, MODAL_NORMS);
}

bool Lobpcg::converged(int want)
{
  bool ok = true;
  for (int j = 0; j < MC; ++j) {
    const double den = sqrt(sums[8 + j]) + fabs(theta[j]) * sqrt(sums[16 + j]), num = sqrt(sums[j]);
    ratio[j] = den > 0.0 ? num / den : (num == 0.0 ? 0.0 : INFINITY);
    if (j < want && !(ratio[j] <= tol)) ok = false;
  }
  return ok;
}

bool Lobpcg::ritz(int np, int *rank)                  // once for all ranks of R
{
  unpack_gram(sums + MODAL_NORMS, np, GM, GK);
  if (veto && veto(8 * np, GM)) return false;
  double Cs[24 * 16];
  const int r = modal_ritz(8 * np, GM, GK, MC, theta, Cs);
  if (r < 0) return false;
  std::vector<double> &h_C = R[0]->modal.h_C;
  std::fill(h_C.begin(), h_C.begin() + 24 * 16, 0.0);
  std::copy(Cs, Cs + 8 * np * 16, h_C.begin());
  *rank = r;
  return true;
}

int Lobpcg::run(int want, int max_it, int *it)
{
  int rc;
  // X alone: fresh products, the Gram sums of X, theta ascending and X M-orthonormal again, fresh products
  auto ritz_on_x = [&]() -> int {
    int rank = 0;
    if ((rc = products(V_X, V_KX, V_MX))) return rc;
    EACH_RANK(c) enq_gram(c, 1);
    if ((rc = read_sums(MODAL_NORMS, MODAL_GRAM))) return rc;
    if (!ritz(1, &rank)) return LOBPCG_BROKE;
    if ((rc = upload())) return rc;
    EACH_RANK(c) enq_combine(c, 1, 0);
    return products(V_X, V_KX, V_MX);
  };
  if ((rc = ritz_on_x())) return rc;
  bool hasP = false, must_step = false;
  for (int its = 0;;) {                               // the renewal follows the steps of this call, max_it bounds *it
    // the recurrences cannot drift: every 20 steps the products of X, and where the driver says so of P, are made again
    if (its > 0 && its % 20 == 0 && !must_step) {
      if ((rc = products(V_X, V_KX, V_MX))) return rc;
      if (renew_p && hasP && (rc = products(V_P, V_KP, V_MP))) return rc;
    }
    const int np = hasP ? 3 : 2;
    if ((rc = upload()) || (rc = enq_residual(true))) return rc;
    if (after_residual && (rc = after_residual())) return rc;
    if ((rc = products(V_W, V_KW, V_MW))) return rc;
    EACH_RANK(c) enq_gram(c, np);
    if ((rc = read_sums(0, MODAL_SUMS))) return rc;                     // the one synchronisation of a step
    const bool stop = converged(want) && !must_step;
    must_step = false;
    if (stop || *it >= max_it) {
      // at return: X orthonormalised on its own, fresh products, and the test made on them
      if ((rc = ritz_on_x()) || (rc = upload()) || (rc = fresh_norms())) return rc;
      if (converged(want)) return LOBPCG_CONVERGED;
      if (*it >= max_it) return LOBPCG_OUT_OF_STEPS;
      must_step = true;                                                 // the recurrences had drifted: go on from the fresh products
      continue;
    }
    int rank = 0;
    if (!ritz(np, &rank)) return LOBPCG_BROKE;
    if ((rc = upload())) return rc;
    EACH_RANK(c) enq_combine(c, np, 1);
    hasP = rank == 8 * np;                                              // a rank drop restarts the recurrence without P
    ++its; ++*it;
  }
}

int modal_solve(feahip_ctx *c, int n_modes, double tol, int max_it, int warm, double *lambda, double *resid, int *iters)
{
  int rc;
  if ((rc = ensure_modal(c))) return rc;
  ModalState &S = c->modal;
  if (S.n_free < 3 * MC) {
    c->err = "solve_modes: " + std::to_string(S.n_free) + " free dofs, fewer than the 24 the block of eight columns needs";
    return FEAHIP_EINVAL;
  }
  // K(x), masked as the PCG sees it (K and f are another matrix from here on: k_epoch)
  if ((rc = feahip_create_stiffness(c)) || (rc = feahip_apply_prescribed_bc(c, 0.0))) return rc;
  if (c->precond == 1) { if ((rc = amg_prepare(c))) return rc; }
  else enq_precond_blockjacobi(c);
  Lobpcg L({c}, nullptr, tol);
  auto finish = [&](int it, int code) {
    S.have = true;
    for (int j = 0; j < n_modes; ++j) { lambda[j] = L.theta[j]; if (resid) resid[j] = L.ratio[j]; }
    if (iters) *iters = it;
    if (code == FEAHIP_ENOTCONVERGED) c->err = "solve_modes: not converged after " + std::to_string(it) + " Rayleigh-Ritz steps";
    return code;
  };
  if (warm && S.have) {
    // the modes held, their theta, against the K of now: converged already means nothing is touched
    if ((rc = L.upload()) || (rc = L.products(V_X, V_KX, V_MX)) || (rc = L.fresh_norms())) return rc;
    if (L.converged(n_modes)) return finish(0, FEAHIP_OK);
  } else if ((rc = launch_modal_hash(c, mv(c, V_X)))) return rc;
  S.have = false;
  int it = 0;
  const int end = L.run(n_modes, max_it, &it);
  if (end < 0) return end;
  if (end == LOBPCG_BROKE) {
    c->err = "solve_modes: the Rayleigh-Ritz basis lost its rank or a sum is not finite (a body with zero-energy modes is not supported)";
    return FEAHIP_ENOTCONVERGED;
  }
  return finish(it, end == LOBPCG_CONVERGED ? FEAHIP_OK : FEAHIP_ENOTCONVERGED);
}

// column col of the block vector d_v8 to the host, [3N] in library ids
static int get_column(feahip_ctx *c, const double *d_v8, int col, double *h_lib)
{
  hipLaunchKernelGGL(k_modal_extract, g256((size_t)c->ndof), dim3(256), 0, c->stream, (size_t)c->ndof, d_v8, col, c->d_q);
  FEA_HIP_CHECK(c, hipGetLastError());
  FEA_HIP_CHECK(c, hipMemcpyAsync(h_lib, c->d_q, sizeof(double) * (size_t)c->ndof, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}
int modal_get(feahip_ctx *c, int col, double *h_lib) { return get_column(c, mv(c, V_X), col, h_lib); }

// ---- more than eight modes, and a shift: sweeps of the block with hard locking ------------------------------------------
int ensure_locked(feahip_ctx *c, int n_modes)
{
  ModalState &S = c->modal;
  const int panels = (n_modes + MC - 1) / MC;
  const size_t n8 = (size_t)c->ndof * MC;
  if (panels > S.lock_panels) {
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    dev_free({S.d_lock, S.d_lpart, S.d_lcoef});
    S.d_lock = S.d_lpart = S.d_lcoef = nullptr; S.lock_panels = 0;
    FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_lock, sizeof(double) * 2 * panels * n8));
    FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_lpart, sizeof(double) * (size_t)panels * 64 * RB));
    FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_lcoef, sizeof(double) * (size_t)panels * 64));
    S.lock_panels = panels;
    FEA_HIP_CHECK(c, hipMemsetAsync(S.d_lpart, 0, sizeof(double) * (size_t)panels * 64 * RB, c->stream));
  }
  FEA_HIP_CHECK(c, hipMemsetAsync(S.d_lock, 0, sizeof(double) * 2 * S.lock_panels * n8, c->stream));
  FEA_HIP_CHECK(c, hipMemsetAsync(S.d_lcoef, 0, sizeof(double) * (size_t)S.lock_panels * 64, c->stream));
  S.n_locked = 0;
  S.have_locked = false;
  return FEAHIP_OK;
}

double *locked_panel(feahip_ctx *c, int mq, int panel)
{
  return c->modal.d_lock + ((size_t)(mq ? c->modal.lock_panels : 0) + panel) * c->ndof * MC;
}

static void enq_deflate_gram(feahip_ctx *c, const double *d_w8, int panels)
{
  hipLaunchKernelGGL(k_modal_deflate_gram, dim3(gram_grid(c)), dim3(256), 0, c->stream, c->ndof, panels, d_w8,
                     (const double *)locked_panel(c, 1, 0), (size_t)c->ndof * MC, c->modal.d_lpart);
}
static void enq_deflate_apply(feahip_ctx *c, double *d_w8, int panels)
{
  hipLaunchKernelGGL(k_modal_deflate_apply, dim3((c->ndof + 255) / 256), dim3(256), 0, c->stream, c->ndof, panels, d_w8,
                     (const double *)locked_panel(c, 0, 0), (size_t)c->ndof * MC, (const double *)c->modal.d_lcoef);
}

// W <- W - Q (MQ' W) against the panels that hold the first n_locked modes: three launches, nothing read back
int launch_deflate(feahip_ctx *c, double *d_w8, int n_locked)
{
  const int panels = (n_locked + MC - 1) / MC;
  if (panels == 0) return FEAHIP_OK;
  enq_deflate_gram(c, d_w8, panels);
  hipLaunchKernelGGL(k_modal_deflate_reduce, dim3(panels * 64), dim3(256), 0, c->stream, gram_grid(c),
                     (const double *)c->modal.d_lpart, c->modal.d_lcoef);
  enq_deflate_apply(c, d_w8, panels);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// hooks of feahip_time_kernel 16 and 17 on W against eight panels of hash; the coefficients are zero, so W stays as it is
int time_deflate_prepare(feahip_ctx *c)
{
  int rc;
  if ((rc = time_modal_prepare(c)) || (rc = ensure_locked(c, FEA_MODAL_MAX_LOCKED))) return rc;
  for (int mq = 0; mq < 2; ++mq)
    for (int p = 0; p < MODAL_PANELS; ++p) if ((rc = launch_modal_hash(c, locked_panel(c, mq, p)))) return rc;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

int time_deflate_kernel(feahip_ctx *c, int what)
{
  if (what == 16) enq_deflate_gram(c, mv(c, V_W), MODAL_PANELS);
  else enq_deflate_apply(c, mv(c, V_W), MODAL_PANELS);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// The driver.  K_s = K + shift M (masked) is in K's store; the shared iteration runs on the pencil (K_s, M), theta_s =
// lambda + shift, with W deflated against the store before its products (Lobpcg::after_residual).  A sweep: deflate X, one
// Lobpcg::run until the leading min(6, n_modes - locked) columns pass the stop test on fresh products, lock the leading
// converged columns, move the others to the front and refill from the hash.
int modal_solve_locked(feahip_ctx *c, int n_modes, double shift, double tol, int max_it, double *lambda, double *resid,
                       int *iters, int *sweeps)
{
  int rc;
  if ((rc = ensure_modal(c))) return rc;
  ModalState &S = c->modal;
  S.have = false;                                                     // the block is scratch here
  S.have_locked = false;
  if (S.n_free < n_modes + 3 * MC) {
    c->err = "solve_modes_locked: " + std::to_string(S.n_free) + " free dofs, fewer than n_modes + 24";
    return FEAHIP_EINVAL;
  }
  if ((rc = ensure_locked(c, n_modes))) return rc;
  // K(x) + shift M in the order of a Newmark iteration: assemble, add, mask (K and f are another matrix from here on)
  if ((rc = feahip_create_stiffness(c))) return rc;
  if (shift > 0.0 && (rc = launch_mass_add(c, shift))) return rc;
  if ((rc = feahip_apply_prescribed_bc(c, 0.0))) return rc;
  if (c->precond == 1) { if ((rc = amg_prepare(c))) return rc; }
  else enq_precond_blockjacobi(c);
  const size_t n8 = (size_t)c->ndof * MC;
  int locked = 0, it = 0, sweep = 0, next_id = MC;
  for (int j = 0; j < n_modes; ++j) { lambda[j] = NAN; if (resid) resid[j] = NAN; }
  Lobpcg L({c}, nullptr, tol);
  L.after_residual = [&]() { return launch_deflate(c, mv(c, V_W), locked); };
  auto done = [&](int code, const std::string &why) {
    // The store is in the order of locking.  Two eigenvalues that are equal to rounding (a degenerate pair split by the
    // end of a sweep) can come out of two sweeps in either order, so lambda is sorted once more, stably, and the modes
    // are read through the same permutation
    static_assert(sizeof(S.lock_order) / sizeof(int) == FEA_MODAL_MAX_LOCKED, "one entry per mode of the store");
    double lam[FEA_MODAL_MAX_LOCKED], res[FEA_MODAL_MAX_LOCKED];
    for (int j = 0; j < locked; ++j) { S.lock_order[j] = j; lam[j] = lambda[j]; res[j] = resid ? resid[j] : 0.0; }
    std::stable_sort(S.lock_order, S.lock_order + locked, [&](int x, int y) { return lam[x] < lam[y]; });
    for (int j = 0; j < locked; ++j) { lambda[j] = lam[S.lock_order[j]]; if (resid) resid[j] = res[S.lock_order[j]]; }
    for (int j = 0; j < locked; ++j) S.lam[j] = lambda[j];              // kept, unshifted, for the response entries
    S.shift = shift;
    ++S.lock_gen;
    S.n_locked = locked;
    S.have_locked = true;                                               // the pairs locked so far stay readable
    if (iters) *iters = it;
    if (sweeps) *sweeps = sweep;
    if (code) c->err = "solve_modes_locked: " + why + " (" + std::to_string(locked) + " of " + std::to_string(n_modes) + " modes locked)";
    return code;
  };

  if ((rc = launch_modal_hash(c, mv(c, V_X)))) return rc;
  while (locked < n_modes) {
    ++sweep;
    const int want = n_modes - locked < MC - 2 ? n_modes - locked : MC - 2;   // two guard columns
    if ((rc = launch_deflate(c, mv(c, V_X), locked))) return rc;
    const int end = L.run(want, max_it, &it);         // (the renewal follows the sweep's own steps, max_it bounds their total)
    if (end < 0) return end;
    if (end == LOBPCG_BROKE)
      return done(FEAHIP_ENOTCONVERGED, "the Rayleigh-Ritz basis lost its rank or a sum is not finite (a body with zero-energy modes needs a shift)");
    if (end == LOBPCG_OUT_OF_STEPS) return done(FEAHIP_ENOTCONVERGED, "not converged after " + std::to_string(it) + " Rayleigh-Ritz steps");
    // lock the leading converged columns, contiguous from column 0, within n_modes
    int k = 0;
    while (k < MC && locked + k < n_modes && L.ratio[k] <= tol) ++k;
    hipLaunchKernelGGL(k_modal_lock, dim3((c->ndof + 255) / 256), dim3(256), 0, c->stream, c->ndof, locked, k,
                       (const double *)mv(c, V_X), (const double *)mv(c, V_MX), locked_panel(c, 0, 0), locked_panel(c, 1, 0), n8);
    for (int j = 0; j < k; ++j) { lambda[locked + j] = L.theta[j] - shift; if (resid) resid[locked + j] = L.ratio[j]; }
    locked += k;
    if (locked < n_modes) {
      hipLaunchKernelGGL(k_modal_advance, dim3((c->ndof + 255) / 256), dim3(256), 0, c->stream, c->ndof, k, next_id,
                         (const uint8_t *)c->d_dofmask, mv(c, V_X));
      next_id += k;
    }
    FEA_HIP_CHECK(c, hipGetLastError());
  }
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return done(FEAHIP_OK, "");
}

int modal_get_locked(feahip_ctx *c, int mode, double *h_lib)           // mode of the ascending lambda
{
  const int at = c->modal.lock_order[mode];
  return get_column(c, locked_panel(c, 0, at / MC), at % MC, h_lib);
}

// ---- the base solve over the ranks of a sharded run (feahip_solve_modes_sharded) ----------------------------------------
// modal_solve on R = the ranks this process drives (all members of an in-process group, or the one context of an RCCL
// rank): the shared iteration with the run's transport, the start block keyed by the node's identity in the whole mesh.
int ensure_modal_dist(feahip_ctx *c)
{
  int rc;
  ModalState &S = c->modal;
  const bool held = S.have_sharded;
  if ((rc = ensure_modal(c))) return rc;
  S.have_sharded = held;
  if (!S.d_bsend || S.blk_nsend != c->nsend || S.blk_nrecv != c->nrecv) {
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (c->comm_stream) FEA_HIP_CHECK(c, hipStreamSynchronize(c->comm_stream));
    dev_free({S.d_bsend, S.d_brecv});
    S.d_bsend = S.d_brecv = nullptr; S.blk_nsend = S.blk_nrecv = -1;
    FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_bsend, sizeof(double) * 24 * (size_t)(c->nsend ? c->nsend : 1)));
    FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_brecv, sizeof(double) * 24 * (size_t)(c->nrecv ? c->nrecv : 1)));
    S.blk_nsend = c->nsend; S.blk_nrecv = c->nrecv;
  }
  if (S.key_row0 != c->row0 || S.key_row1 != c->row1) {
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    dev_free({S.d_key});
    S.d_key = nullptr; S.key_row0 = S.key_row1 = -1;
    S.have_sharded = false;                                             // whatever X holds, it was for other rows
    const int n = own_nodes(c);
    if (c->rank_own >= 0 && n > 0) {                                    // a rank context: the caller's id in the whole mesh
      std::vector<int> key((size_t)n);
      for (int a = 0; a < n; ++a) {
        const int lib = c->row0 + a;
        key[(size_t)a] = c->rank_node_global[(size_t)(c->iperm.empty() ? lib : c->iperm[(size_t)lib])];
      }
      FEA_HIP_CHECK(c, hipMalloc((void **)&S.d_key, sizeof(int) * (size_t)n));
      FEA_HIP_CHECK(c, hipMemcpy(S.d_key, key.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    }
    std::vector<uint8_t> hm((size_t)3 * (n > 0 ? n : 0));
    if (!hm.empty()) {
      FEA_HIP_CHECK(c, hipMemcpyAsync(hm.data(), c->d_dofmask + (size_t)3 * c->row0, hm.size(), hipMemcpyDeviceToHost, c->stream));
      FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    }
    S.n_free_own = 0;
    for (uint8_t b : hm) S.n_free_own += b ? 0 : 1;
    S.key_row0 = c->row0; S.key_row1 = c->row1;
  }
  return FEAHIP_OK;
}

void modal_enq_block_pack(feahip_ctx *c, const double *d_v8)
{
  if (c->nsend <= 0) return;
  hipLaunchKernelGGL(k_block_halo_pack, g256((size_t)c->nsend * 12), dim3(256), 0, c->stream, c->nsend,
                     (const int *)c->d_send_idx, (const v2d *)d_v8, (v2d *)c->modal.d_bsend);
}
void modal_enq_block_unpack_on(feahip_ctx *c, double *d_v8, hipStream_t stream)
{
  if (c->nrecv <= 0) return;
  hipLaunchKernelGGL(k_block_halo_unpack, g256((size_t)c->nrecv * 12), dim3(256), 0, stream, c->nrecv,
                     (const int *)c->d_recv_idx, (const v2d *)c->modal.d_brecv, (v2d *)d_v8);
}
void modal_enq_block_poison(feahip_ctx *c, double *d_v8)
{
  if (c->nrecv <= 0) return;
  hipLaunchKernelGGL(k_block_halo_poison, g256((size_t)c->nrecv * 12), dim3(256), 0, c->stream, c->nrecv,
                     (const int *)c->d_recv_idx, (v2d *)d_v8);
}

int modal_spmm_km_dist(std::vector<feahip_ctx *> &R) { return block_products(R, R[0]->tr, false, V_X, V_KX, V_MX); }

// n doubles per rank (host, rank k's at h[k n]) summed over all ranks into out: through d_vred and the transport
static int allreduce_host(std::vector<feahip_ctx *> &R, Transport *T, int n, const double *h, double *out)
{
  int rc;
  size_t k = 0;
  FOR_RANKS(c) {
    FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_vred, h + (k++) * n, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  }
  if ((rc = T->allreduce_vec(R, (size_t)n, false))) return rc;
  feahip_ctx *c0 = R[0];
  (void)hipSetDevice(c0->device);
  FEA_HIP_CHECK(c0, hipMemcpyAsync(out, c0->d_vred, sizeof(double) * n, hipMemcpyDeviceToHost, c0->stream));
  FEA_HIP_CHECK(c0, hipStreamSynchronize(c0->stream));
  return FEAHIP_OK;
}

int modal_solve_dist(std::vector<feahip_ctx *> &R, int n_modes, double tol, int max_it, int warm, double *lambda,
                     double *resid, int *iters)
{
  int rc;
  Transport *T = R[0]->tr;
  auto refuse = [&](int code, const std::string &why) { for (feahip_ctx *c : R) c->err = "solve_modes_sharded: " + why; return code; };
  // What decides a refusal is all-reduced, so that every rank of the run returns the same code: the free dofs, the
  // ranks that hold modes of a sharded solve on their current rows, the preconditioner kinds, a missing mass
  enum { Q_FREE, Q_HAVE, Q_KIND1, Q_KIND2, Q_NOMASS, Q_RANKS, Q_N };
  std::vector<double> q((size_t)Q_N * R.size(), 0.0);
  double tot[Q_N];
  std::string mass_err;
  {
    size_t k = 0;
    FOR_RANKS(c) {
      double *qk = q.data() + (k++) * Q_N;
      if ((rc = ensure_vred(c, MODAL_SUMS))) return rc;
      const int rm = mass_ensure(c, "solve_modes_sharded");
      if (rm && rm != FEAHIP_ESTATE) return rm;
      if (rm) { qk[Q_NOMASS] = 1.0; if (mass_err.empty()) mass_err = c->err; }
      else if ((rc = ensure_modal_dist(c))) return rc;
      ModalState &S = c->modal;
      qk[Q_FREE] = rm ? 0.0 : (double)S.n_free_own;
      qk[Q_HAVE] = (!rm && S.have_sharded && S.sh_row0 == c->row0 && S.sh_row1 == c->row1) ? 1.0 : 0.0;
      qk[Q_KIND1] = c->precond == 1 ? 1.0 : 0.0;
      qk[Q_KIND2] = c->precond == 2 ? 1.0 : 0.0;
      qk[Q_RANKS] = 1.0;
    }
  }
  if ((rc = allreduce_host(R, T, Q_N, q.data(), tot))) return rc;
  if (tot[Q_NOMASS] > 0.0) {
    for (feahip_ctx *c : R) c->err = !mass_err.empty() ? mass_err : "solve_modes_sharded: no mass, or a stale one, on another rank of the run (feahip_set_mass)";
    return FEAHIP_ESTATE;
  }
  if (tot[Q_KIND2] > 0.0) return refuse(FEAHIP_EINVAL, "preconditioner 2 (coarse level across the ranks) is not supported");
  if (tot[Q_KIND1] != 0.0 && tot[Q_KIND1] != tot[Q_RANKS]) return refuse(FEAHIP_EINVAL, "the ranks' preconditioner kinds differ (feahip_set_preconditioner: the same kind on every rank)");
  if (tot[Q_FREE] < 3 * MC)
    return refuse(FEAHIP_EINVAL, std::to_string((long long)tot[Q_FREE]) + " free dofs, fewer than the 24 the block of eight columns needs");
  const bool have = tot[Q_HAVE] == tot[Q_RANKS];
  for (feahip_ctx *c : R) { c->modal.have = false; c->modal.have_sharded = false; }   // the block is this solve's from here on

  // K(x), masked as the PCG sees it (K and f are another matrix from here on: k_epoch)
  FOR_RANKS(c) { if ((rc = feahip_create_stiffness(c)) || (rc = feahip_apply_prescribed_bc(c, 0.0))) return rc; }
  FOR_RANKS(c) {
    if (c->precond == 1) { if ((rc = amg_prepare(c))) return rc; }
    else enq_precond_blockjacobi(c);
  }
  Lobpcg L(R, T, tol);
  auto finish = [&](int it, int code) {
    for (feahip_ctx *c : R) {
      ModalState &S = c->modal;
      S.have_sharded = true; S.sh_row0 = c->row0; S.sh_row1 = c->row1;
      for (int j = 0; j < MC; ++j) S.theta[j] = L.theta[j];
      if (code == FEAHIP_ENOTCONVERGED) c->err = "solve_modes_sharded: not converged after " + std::to_string(it) + " Rayleigh-Ritz steps";
    }
    for (int j = 0; j < n_modes; ++j) { lambda[j] = L.theta[j]; if (resid) resid[j] = L.ratio[j]; }
    if (iters) *iters = it;
    return code;
  };

  if (warm && have) {
    // the modes held, their theta, against the K of now: converged already means nothing is touched
    if ((rc = L.upload()) || (rc = L.products(V_X, V_KX, V_MX)) || (rc = L.fresh_norms())) return rc;
    if (L.converged(n_modes)) return finish(0, FEAHIP_OK);
  } else {
    FOR_RANKS(c) {
      if (own_nodes(c) > 0)
        hipLaunchKernelGGL(k_modal_hash_rows, g256((size_t)own_nodes(c) * 24), dim3(256), 0, c->stream, own_nodes(c), c->row0,
                           (const int *)c->modal.d_key, (const uint8_t *)(c->d_dofmask + (size_t)3 * c->row0), mv(c, V_X) + own_off8(c));
    }
  }
  int it = 0;
  const int end = L.run(n_modes, max_it, &it);
  if (end < 0) return end;
  if (end == LOBPCG_BROKE)
    return refuse(FEAHIP_ENOTCONVERGED, "the Rayleigh-Ritz basis lost its rank or a sum is not finite (a body with zero-energy modes is not supported)");
  return finish(it, end == LOBPCG_CONVERGED ? FEAHIP_OK : FEAHIP_ENOTCONVERGED);
}
