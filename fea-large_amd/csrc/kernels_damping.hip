// kernels_damping.hip -- Rayleigh damping C = alpha M + beta K_d on gfx950.
//
// M is the mass of the loop that runs: the consistent m (one double per block of K's pattern) in the Newmark loop and in
// the consistent acceleration, the lumped ml in the explicit loop (k_explicit_finish<.., DAMP>, kernels_mass.hip).  K_d is
// a SNAPSHOT: the plain tangent (no contact term, unmasked) at the x of feahip_set_damping, copied into a store of its own
// that is indexed exactly as d_K over the owned window.  A constant C keeps the damping linear, so the Newton matrix of a
// Newmark step is exact.
//
// With a0 = 1 / (beta_N dt^2), c1 = gamma / (beta_N dt), d = x - xt and w = vt + c1 d (the velocity the corrector will
// assign, pointwise), a Newton iteration of a damped step runs two kernels in place of k_mass_residual / k_mass_add:
//   k_damp_residual<KD>  f_r -= sum_b [ m_rb (a0 d_b + alpha w_b) + beta Kd_rb w_b ]: a wave per SpMV chunk, d and w made
//                        on the fly from the three gathered node records, never stored
//   k_damp_add           K += cm m I + ck K_d over the 16-byte pieces of the owned values (beta > 0 only; with beta = 0
//                        the loop calls k_mass_add with another coefficient)
// k_damp_product<KD> is the body of the first without the subtraction, y = C v.  Every kernel: a fixed summation order, no
// atomics, the same bits on every call.  Nothing here is launched on a context without damping.
#include "feahip_internal.h"
#include <cmath>

typedef double damp_v2d __attribute__((ext_vector_type(2)));

// The row loop of mass_rows_body (kernels_mass.hip) with one more record, and with KD the 72-byte block of k_spmv's row
// loop beside the scalar: lane k takes the blocks k and k + 64 of its wave's chunk, leaves its three partial sums in LDS,
// and lane (row, i) adds its row's in block order.
//   SUB: d = x - xt, w = vt + c1 d;  f[row] -= sum_b m_rb (a0 d_b + alpha w_b) + beta Kd_rb w_b
//  !SUB: w = x (the vector given);   y[row]  = sum_b alpha m_rb w_b + beta Kd_rb w_b
// m may be null where alpha = 0 (feahip_damping_spmv on a context without a mass).
// KD stages the chunk's values of K_d as k_spmv does (kernels_solve.hip): they are one contiguous run, which the wave
// reads as lane-contiguous 16-byte pieces (1 KB per load instruction) into the LDS the partial sums will take afterwards,
// and every lane picks its blocks out of it.  K_d has K's 16-byte phase and K's 16 bytes of padding (damping_set).
template <bool KD, bool SUB>
__device__ __forceinline__ void damp_rows_body(int chunk0, int nchunks, const int *__restrict__ chunk, const int *__restrict__ rowptr,
                 const int *__restrict__ colidx, const double *__restrict__ m, const double *__restrict__ Kd,
                 const double *__restrict__ x, const double *__restrict__ xt, const double *__restrict__ vt, double a0,
                 double c1, double alpha, double beta, double *__restrict__ y)
{
  static_assert(FEA_CHUNK_ROWS * 3 <= 64, "one lane per (row, component) of a chunk");
  static_assert(FEA_CHUNK_BLOCKS <= 128, "a lane takes the blocks k and k + 64 of a chunk");
  constexpr int NPMAX = (15 + FEA_CHUNK_BLOCKS * 72 + 15) >> 4;            // 16-byte pieces of a chunk's values
  constexpr int NJ = (NPMAX + 63) / 64;
  constexpr int SPD = KD ? 2 * NPMAX : FEA_CHUNK_BLOCKS * 3;
  static_assert(SPD >= FEA_CHUNK_BLOCKS * 3, "the partial sums take the place of the staged values");
  __shared__ __attribute__((aligned(16))) double sP[FEA_WAVES_PER_WG][SPD];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double *tP = sP[wave];
  // the scalar part of block q into o, the vector the 72-byte block multiplies into w
  auto records = [&](int q, double (&o)[3], double (&w)[3]) {
    const double mm = m ? m[q] : 0.0;
    const size_t col = (size_t)colidx[q];
    const damp_v2d *xp = reinterpret_cast<const damp_v2d *>(x + col * 4);
    const damp_v2d xa = xp[0], xb = xp[1];
    double s[3];
    w[0] = xa.x; w[1] = xa.y; w[2] = xb.x;
    if constexpr (SUB) {
      const damp_v2d *tp = reinterpret_cast<const damp_v2d *>(xt + col * 4);
      const damp_v2d *vp = reinterpret_cast<const damp_v2d *>(vt + col * 4);
      const damp_v2d ta = tp[0], tb = tp[1], va = vp[0], vb = vp[1];
      const double d[3] = {xa.x - ta.x, xa.y - ta.y, xb.x - tb.x};
      w[0] = va.x + c1 * d[0]; w[1] = va.y + c1 * d[1]; w[2] = vb.x + c1 * d[2];
#pragma unroll
      for (int i = 0; i < 3; ++i) s[i] = a0 * d[i] + alpha * w[i];
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) s[i] = alpha * w[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = mm * s[i];
  };
  auto block = [&](const double *kp, const double (&w)[3], double (&o)[3]) {
    double v[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) v[j] = kp[j];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] += beta * (v[3 * i] * w[0] + v[3 * i + 1] * w[1] + v[3 * i + 2] * w[2]);
  };
  for (int ch = chunk0 + blockIdx.x * FEA_WAVES_PER_WG + wave; ch < chunk0 + nchunks; ch += gridDim.x * FEA_WAVES_PER_WG) {
    const int r0 = chunk[ch], r1 = chunk[ch + 1];
    const int b0 = rowptr[r0], nb = rowptr[r1] - b0;
    if (nb > FEA_CHUNK_BLOCKS) {
      // a row longer than the tile has a chunk of its own (pattern.cpp): the lanes stride over its blocks and their
      // sums meet in a butterfly -- any length, fixed order
      double s[3] = {0, 0, 0};
      for (int k = lane; k < nb; k += 64) {
        double o[3], w[3];
        records(b0 + k, o, w);
        if constexpr (KD) block(Kd + (size_t)(b0 + k) * 9, w, o);
        s[0] += o[0]; s[1] += o[1]; s[2] += o[2];
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        s[0] += __shfl_xor(s[0], off, 64); s[1] += __shfl_xor(s[1], off, 64); s[2] += __shfl_xor(s[2], off, 64);
      }
      if (lane < 3) {
        const double acc = lane == 0 ? s[0] : lane == 1 ? s[1] : s[2];
        if constexpr (SUB) y[(size_t)r0 * 3 + lane] -= acc; else y[(size_t)r0 * 3 + lane] = acc;
      }
      continue;
    }
    int kb = 0, ke = 0;
    if (lane < (r1 - r0) * 3) { kb = rowptr[r0 + lane / 3] - b0; ke = rowptr[r0 + lane / 3 + 1] - b0; }
    double o[2][3] = {{0, 0, 0}, {0, 0, 0}}, w[2][3] = {{0, 0, 0}, {0, 0, 0}};
    if constexpr (KD) {
      const size_t s0 = (size_t)b0 * 72, al = s0 & ~(size_t)15;
      const int sh = (int)(s0 - al), np = (sh + nb * 72 + 15) >> 4;
      const damp_v2d *Kp = reinterpret_cast<const damp_v2d *>(reinterpret_cast<const char *>(Kd) + al);
      damp_v2d *sW = reinterpret_cast<damp_v2d *>(tP);
      damp_v2d pc[NJ];
#pragma unroll
      for (int j = 0; j < NJ - 1; ++j) { const int p = lane + 64 * j; pc[j] = Kp[p < np ? p : 0]; }
      if (np > 64 * (NJ - 1)) { const int p = lane + 64 * (NJ - 1); pc[NJ - 1] = Kp[p < np ? p : 0]; }
#pragma unroll
      for (int h = 0; h < 2; ++h) { const int k = lane + 64 * h; if (k < nb) records(b0 + k, o[h], w[h]); }
#pragma unroll
      for (int j = 0; j < NJ - 1; ++j) { const int p = lane + 64 * j; if (p < np) sW[p] = pc[j]; }
      if (np > 64 * (NJ - 1)) { const int p = lane + 64 * (NJ - 1); if (p < np) sW[p] = pc[NJ - 1]; }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        if (k < nb) block(reinterpret_cast<const double *>(reinterpret_cast<const char *>(tP) + sh + 72 * k), w[h], o[h]);
      }
      // (the sums below overwrite the staged values: a wave's LDS operations complete in program order, and every lane
      // has read its blocks by then)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) { const int k = lane + 64 * h; if (k < nb) records(b0 + k, o[h], w[h]); }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k < nb) { tP[k * 3 + 0] = o[h][0]; tP[k * 3 + 1] = o[h][1]; tP[k * 3 + 2] = o[h][2]; }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (lane < (r1 - r0) * 3) {
      const int i = lane % 3;
      double acc = 0;
      for (int k = kb; k < ke; ++k) acc += tP[k * 3 + i];
      if constexpr (SUB) y[(size_t)r0 * 3 + lane] -= acc; else y[(size_t)r0 * 3 + lane] = acc;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
}

template <bool KD>
__global__ __launch_bounds__(64 * FEA_WAVES_PER_WG)
void k_damp_residual(int chunk0, int nchunks, const int *chunk, const int *rowptr, const int *colidx, const double *m,
                     const double *Kd, const double *x, const double *xt, const double *vt, double a0, double c1,
                     double alpha, double beta, double *f)
{
  damp_rows_body<KD, true>(chunk0, nchunks, chunk, rowptr, colidx, m, Kd, x, xt, vt, a0, c1, alpha, beta, f);
}

template <bool KD>
__global__ __launch_bounds__(64 * FEA_WAVES_PER_WG)
void k_damp_product(int chunk0, int nchunks, const int *chunk, const int *rowptr, const int *colidx, const double *m,
                    const double *Kd, const double *v, double alpha, double beta, double *y)
{
  damp_rows_body<KD, false>(chunk0, nchunks, chunk, rowptr, colidx, m, Kd, v, (const double *)nullptr, (const double *)nullptr,
                            0.0, 0.0, alpha, beta, y);
}

// K += cm m I + ck K_d in the piece scheme of k_mass_add: the owned values are the run [v0, v1) of GLOBAL value indices,
// even indices are 16-byte aligned in K and in K_d alike, and a lane takes the piece (2p, 2p + 1).  Every piece is stored.
__global__ __launch_bounds__(256)
void k_damp_add(long long v0, long long v1, double cm, double ck, const double *__restrict__ m,
                const double *__restrict__ Kd, double *__restrict__ K)
{
  const long long pl = v0 >> 1, ph = (v1 + 1) >> 1;
  const long long stride = (long long)gridDim.x * 256;
  for (long long p = pl + (long long)blockIdx.x * 256 + threadIdx.x; p < ph; p += stride) {
    const long long va = 2 * p, q = va / 9;
    const int r = (int)(va - q * 9);                       // entry of block q the first value of the piece is
    const bool d0 = r == 0 || r == 4 || r == 8, d1 = r == 3 || r == 7 || r == 8;
    const long long qb = q + (r == 8 ? 1 : 0);             // block of the second value
    if (va >= v0 && va + 1 < v1) {
      damp_v2d *kp = reinterpret_cast<damp_v2d *>(K + va);
      damp_v2d k2 = *kp;
      const damp_v2d g2 = *reinterpret_cast<const damp_v2d *>(Kd + va);
      k2.x += ck * g2.x; k2.y += ck * g2.y;
      if (d0) k2.x += cm * m[q];
      if (d1) k2.y += cm * m[qb];
      *kp = k2;
    } else {                                               // a piece that reaches over an end of the window
      if (va >= v0) K[va] += ck * Kd[va] + (d0 ? cm * m[q] : 0.0);
      if (va + 1 < v1) K[va + 1] += ck * Kd[va + 1] + (d1 ? cm * m[qb] : 0.0);
    }
  }
}

// f -= y on the dofs [i0, i1)
__global__ __launch_bounds__(256)
void k_damp_sub(int i0, int i1, const double *__restrict__ y, double *__restrict__ f)
{
  const int i = i0 + blockIdx.x * 256 + threadIdx.x;
  if (i < i1) f[i] -= y[i];
}

// ---- launchers ---------------------------------------------------------------------------------------------------
static int chunk_grid(const feahip_ctx *c)
{
  const int g = (c->nchunks_local + FEA_WAVES_PER_WG - 1) / FEA_WAVES_PER_WG;
  return g < FEA_RED_BLOCKS ? (g > 0 ? g : 1) : FEA_RED_BLOCKS;
}

int launch_damp_residual(feahip_ctx *c, double a0, double c1)
{
  const DampingState &D = c->damping;
  const MassState &M = c->mass;
  const dim3 g(chunk_grid(c)), b(64 * FEA_WAVES_PER_WG);
  if (D.beta > 0.0)
    hipLaunchKernelGGL(k_damp_residual<true>, g, b, 0, c->stream, c->chunk0, c->nchunks_local, c->d_chunk, c->d_rowptr, c->d_colidx,
                       M.d_m, D.d_Kd, c->d_x, M.d_xt, M.d_vt, a0, c1, D.alpha, D.beta, c->d_f);
  else
    hipLaunchKernelGGL(k_damp_residual<false>, g, b, 0, c->stream, c->chunk0, c->nchunks_local, c->d_chunk, c->d_rowptr, c->d_colidx,
                       M.d_m, (const double *)nullptr, c->d_x, M.d_xt, M.d_vt, a0, c1, D.alpha, 0.0, c->d_f);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_damp_product(feahip_ctx *c, const double *d_v4, double *d_y)
{
  const DampingState &D = c->damping;
  const double *m = D.alpha > 0.0 ? c->mass.d_m : nullptr;
  const dim3 g(chunk_grid(c)), b(64 * FEA_WAVES_PER_WG);
  if (D.beta > 0.0)
    hipLaunchKernelGGL(k_damp_product<true>, g, b, 0, c->stream, c->chunk0, c->nchunks_local, c->d_chunk, c->d_rowptr, c->d_colidx,
                       m, D.d_Kd, d_v4, D.alpha, D.beta, d_y);
  else
    hipLaunchKernelGGL(k_damp_product<false>, g, b, 0, c->stream, c->chunk0, c->nchunks_local, c->d_chunk, c->d_rowptr, c->d_colidx,
                       m, (const double *)nullptr, d_v4, D.alpha, 0.0, d_y);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

int launch_damp_add(feahip_ctx *c, double cm, double ck)
{
  const long long v0 = c->kb0 * 9, v1 = c->kb1 * 9;
  if (v1 <= v0) return FEAHIP_OK;
  const size_t n = (size_t)((v1 - v0) / 2 + 1), gmax = (size_t)FEA_RED_BLOCKS * 4, g = (n + 255) / 256;
  hipLaunchKernelGGL(k_damp_add, dim3((unsigned)(g < gmax ? g : gmax)), dim3(256), 0, c->stream, v0, v1, cm, ck, c->mass.d_m,
                     c->damping.d_Kd, c->d_K);
  FEA_HIP_CHECK(c, hipGetLastError());
  ++c->k_epoch;                                        // another matrix: the preconditioners set up again, as after an assembly
  return FEAHIP_OK;
}

// f -= C v with the velocities in force (the consistent acceleration); d_q is free outside a solve
int launch_damp_force(feahip_ctx *c)
{
  const int i0 = 3 * c->row0, i1 = 3 * c->row1;
  if (i1 <= i0) return FEAHIP_OK;
  if (const int rc = launch_damp_product(c, c->mass.d_vel, c->d_q)) return rc;
  hipLaunchKernelGGL(k_damp_sub, dim3((i1 - i0 + 255) / 256), dim3(256), 0, c->stream, i0, i1, c->d_q, c->d_f);
  FEA_HIP_CHECK(c, hipGetLastError());
  return FEAHIP_OK;
}

// ---- the state -----------------------------------------------------------------------------------------------------
int damping_ready(feahip_ctx *c, const char *who)
{
  const DampingState &D = c->damping;
  if (D.beta > 0.0 && (D.row0 != c->row0 || D.row1 != c->row1 || !D.d_Kd_base)) {
    c->err = std::string(who) + ": the row shard changed since feahip_set_damping took the snapshot K_d (set the damping again)";
    return FEAHIP_ESTATE;
  }
  if (D.alpha > 0.0) return mass_ensure(c, who);
  return FEAHIP_OK;
}

int damping_set(feahip_ctx *c, double alpha, double beta)
{
  if (!(alpha >= 0.0) || !(beta >= 0.0) || !std::isfinite(alpha) || !std::isfinite(beta)) {
    c->err = "feahip_set_damping: alpha and beta_k must be finite and not negative";
    return FEAHIP_EINVAL;
  }
  DampingState &D = c->damping;
  if (beta == 0.0) {                                       // no K_d: (0, 0) clears the damping altogether
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    D.release();
    D.alpha = alpha;
    return FEAHIP_OK;
  }
  int rc;
  if ((rc = ensure_k(c))) return rc;
  const size_t nb = (size_t)(c->kb1 - c->kb0);
  const bool reuse = D.d_Kd_base && D.row0 == c->row0 && D.row1 == c->row1;   // the same window: the same store
  double *alloc = reuse ? D.d_Kd_alloc : nullptr;
  if (!reuse && hipMalloc((void **)&alloc, sizeof(double) * (9 * nb + 2)) != hipSuccess) {
    c->err = "feahip_set_damping: out of device memory for K_d (" + std::to_string(72 * nb) + " bytes, as much as K)";
    return FEAHIP_ENOMEM;
  }
  // the plain tangent at the x in force: no contact term, unmasked.  K stays as this leaves it
  ++c->k_epoch; c->k_bc = false;
  if ((rc = launch_assemble(c, true, false, true))) { if (!reuse) dev_free({alloc}); return rc; }
  double *base = alloc + (c->kb0 & 1);                     // K's 16-byte phase: even GLOBAL value indices are aligned
  if (hipMemcpyAsync(base, c->d_K_base, sizeof(double) * 9 * nb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    if (!reuse) dev_free({alloc});
    c->err = "feahip_set_damping: the copy of K into K_d failed";
    return FEAHIP_EHIP;
  }
  if (!reuse) D.release();
  D.alpha = alpha; D.beta = beta;
  D.d_Kd_alloc = alloc; D.d_Kd_base = base; D.d_Kd = base - (size_t)c->kb0 * 9;
  D.row0 = c->row0; D.row1 = c->row1;
  return FEAHIP_OK;
}
