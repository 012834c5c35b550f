// superpose.h -- what the kernels that superpose the modes of the locked store share (k_response_sweep, k_transient_sweep,
// k_response_combine) and the host code around them.  The store is 8 panels of [3N][8] doubles, `pstride` doubles apart,
// the eight columns of a dof contiguous; n modes fill the first P = (n + 7) / 8 panels.  A lane owns a dof and keeps its
// 8 P mode values in registers (load_mode_values; k_response_sweep has the same loads written out, and says why); the host
// picks the instance from the panel count (panels_of, for_panels), folds a form into the table of the combine kernels
// (folded_form) and sums the probes in the kernels' order (ProbeRows).
#pragma once
#include "feahip_internal.h"
#include <cmath>
#include <type_traits>
#include <vector>

#define MC FEA_MODAL_COLS
#define ML FEA_MODAL_MAX_LOCKED
static_assert(MC == 8 && ML == 64, "the kernels are written for eight panels of eight columns");
typedef double mode_v2d __attribute__((ext_vector_type(2)));

// x[8 p + a] = Q_p[d][a] for the panels p < P (ABSX: its magnitude), zero where the dof is outside (!in): four 16-byte
// loads per panel, so a wave reads 4 KiB contiguous per panel and slice of 64 dofs of the [3N][8] layout
template <int P, bool ABSX = false>
__device__ __forceinline__ void load_mode_values(const double *__restrict__ Q, size_t pstride, int d, bool in, double (&x)[MC * P])
{
#pragma unroll
  for (int e = 0; e < MC * P; ++e) x[e] = 0.0;
  if (!in) return;                                                     // (one branch around all the loads of the dof)
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const mode_v2d *Qd = reinterpret_cast<const mode_v2d *>(Q + (size_t)p * pstride) + (size_t)d * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const mode_v2d t = Qd[k];
      x[p * MC + 2 * k] = ABSX ? fabs(t.x) : t.x; x[p * MC + 2 * k + 1] = ABSX ? fabs(t.y) : t.y;
    }
  }
}

static inline int panels_of(const feahip_ctx *c) { return (c->modal.n_locked + MC - 1) / MC; }   // the panels in use

// f(std::integral_constant<int, P>) for the panel count as a compile-time constant: 1 to 8, anything else takes 8
template <int P = 1, class F>
static inline void for_panels(int panels, F &&f)
{
  if constexpr (P == ML / MC) f(std::integral_constant<int, P>());
  else if (panels == P) f(std::integral_constant<int, P>());
  else for_panels<P + 1>(panels, f);
}

// The form (C[n][n], b[n] or null: zero, s) by ascending mode as the table the combine kernels read (k_response_combine,
// k_stress_combine), FEA_COMBINE_TABLE doubles: T[64][64] by store column with C folded onto its upper triangle -- the
// diagonal as it is, the entries above it doubled, which is exact, zero below --, then b[64], then s
static inline std::vector<double> folded_form(const ModalState &S, const double *C, const double *b, double s)
{
  const int n = S.n_locked;
  std::vector<double> T(FEA_COMBINE_TABLE, 0.0);
  for (int j = 0; j < n; ++j) {
    const int cj = S.lock_order[j];
    for (int k = j; k < n; ++k) {
      const int ck = S.lock_order[k];
      const int lo = cj < ck ? cj : ck, hi = cj < ck ? ck : cj;
      T[(size_t)lo * ML + hi] = j == k ? C[(size_t)j * n + j] : 2.0 * C[(size_t)j * n + k];
    }
    T[(size_t)ML * ML + cj] = b ? b[j] : 0.0;
  }
  T[(size_t)ML * ML + ML] = s;
  return T;
}

// The probes' rows of Q and of u_s on the host.  sum() is the kernels' sum in the kernels' order -- one fma per store
// column, ascending, onto the start value -- so a probe has the bits of the field the kernel writes for its dof
struct ProbeRows {
  int width = 0;                       // 8 panels
  std::vector<double> rows;            // [n_probe][width + 1]: the mode values by store column, then u_s
  // enqueues the copies on c->stream (probe in library dofs); the rows are there once the stream is synchronised
  int read(feahip_ctx *c, int n_probe, const int *probe)
  {
    width = panels_of(c) * MC;
    rows.resize((size_t)n_probe * (width + 1));
    for (int r = 0; r < n_probe; ++r) {
      double *row = rows.data() + (size_t)r * (width + 1);
      for (int p = 0; p * MC < width; ++p)
        FEA_HIP_CHECK(c, hipMemcpyAsync(row + p * MC, locked_panel(c, 0, p) + (size_t)probe[r] * MC, sizeof(double) * MC,
                                        hipMemcpyDeviceToHost, c->stream));
      FEA_HIP_CHECK(c, hipMemcpyAsync(row + width, c->response.d_us + probe[r], sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    return FEAHIP_OK;
  }
  double us(int r) const { return rows[(size_t)r * (width + 1) + width]; }
  double sum(int r, const double *coef, double start) const
  {
    const double *row = rows.data() + (size_t)r * (width + 1);
    for (int col = 0; col < width; ++col) start = std::fma(row[col], coef[col], start);
    return start;
  }
};
