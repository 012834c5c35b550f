// coarse.h -- one coarse level ACROSS the ranks of a sharded solve (preconditioner kind 2).
//
// The sharded multigrid (amg.h) is a W-cycle on every rank's own diagonal block: block-Jacobi over the ranks.  An
// error that is smooth across the slab boundaries -- the bending of a slender bar -- is corrected one slab per CG
// iteration.  Kind 2 adds the correction of a coarse space that spans the ranks:
//
//     M2^-1 r = M1^-1 r + Phi (Phi' K Phi)^-1 Phi' r            (M1^-1: the cycle, unchanged)
//
// Phi: every rank cuts its owned rows, in its own row order, into m_r = min(m, max(1, n_r / 64)) contiguous runs
// (aggregates; coarse_cuts below), and every aggregate carries its six rigid-body modes about its centroid -- the
// block of node a is [I | u = t + w x (X0_a - c_A)], the convention of amg.h's doff.  At most 128 aggregates, 768
// coarse unknowns.  A_c = Phi' K Phi is formed in double from the double K (never from the multigrid's rounded
// copies), all-reduced, and inverted in double on the host of every rank (identical bits everywhere); an iteration
// restricts r, all-reduces the <= 768 doubles, multiplies by the stored inverse and adds Phi e_c to the cycle's z --
// restriction, all-reduce and product on the context's communication stream, under the cycle.
#pragma once
#include "feahip_internal.h"

#define FEA_COARSE_MAX_AGGS 128        // over all ranks
#define FEA_COARSE_MIN_ROWS 64         // owned rows per aggregate, at least
#define FEA_COARSE_SLICES 64           // workgroups that share one aggregate's rows, at most (fixed-order second pass)
#define FEA_COARSE_PIVOT_TOL 1e-12     // a Cholesky pivot below this fraction of its diagonal entry is "not positive":
                                       // rounding leaves pivots of either sign and size ~ n eps A_ii in a singular A_c

// the cut rule: aggregates of n_owned rows under the cap m; first[j] = floor(j n_owned / m_r), j = 0 .. m_r (may be
// null).  Returns m_r.
int coarse_cuts(int n_owned, int m, int *first);
// m for a run of nranks ranks: clamp(128 / nranks, 1, 16), or FEAHIP_COARSE_AGGS
int coarse_default_m(int nranks);

struct RankCoarse {
  // ---- topology (once per shard)
  int row0 = -1, row1 = -1, nranks = 0;
  const void *tr = nullptr;              // the transport it was exchanged over
  int m = 0, m_loc = 0, agg0 = 0, nagg = 0, nc = 0;     // cap; this rank's aggregates, its first global id; all; 6 nagg
  int npair = 0, ns_a = 1, ns_r = 1;     // (row aggregate, column aggregate) pairs of this rank's rows; slices per aggregate
  std::vector<int> h_agg;                // [N] global aggregate of every local node (library ids), -1: none
  std::vector<double> h_cent;            // [nagg][3]
  int *d_agg = nullptr, *d_first = nullptr, *d_pair = nullptr;   // [N], [m_loc + 1] absolute first rows, [npair][2] (local A, global B)
  double *d_cent = nullptr;
  // ---- numeric part (whenever K changed)
  bool numeric_valid = false;
  unsigned long long num_epoch = 0; bool num_bc = false;
  long long setups = 0;                  // numeric setups so far (feahip_coarse_info)
  std::vector<double> h_A;               // [nc][nc] all-reduced A_c
  double *d_apart = nullptr;             // [npair][ns_a][36] slice sums of the setup kernel
  double *d_Ainv = nullptr;              // [nc][nc]
  // ---- an application
  double *d_rpart = nullptr;             // [m_loc][ns_r][6]
  double *d_ec = nullptr;                // [nc] e_c = A_c^-1 r_c
  hipEvent_t ev_r = nullptr, ev_ec = nullptr;
};

int ensure_comm_stream(feahip_ctx *c);
// collective over R: topology on first use, numeric part for the current K.  FEAHIP_ESTATE (every rank's error text
// names the aggregate) when A_c is not positive definite.
int coarse_prepare(std::vector<feahip_ctx *> &R, Transport *T);
// r_c = Phi' r of the owned rows into the context's all-reduce buffer, on the communication stream behind everything
// the context's stream holds now
int coarse_enq_restrict(feahip_ctx *c, const double *r);
int coarse_allreduce_rc(std::vector<feahip_ctx *> &R, Transport *T);
// e_c = A_c^-1 r_c (communication stream)
int coarse_enq_solve(feahip_ctx *c);
// the context's stream waits for e_c, then z += Phi e_c on the owned rows ...
int coarse_enq_prolong_add(feahip_ctx *c, double *z);
// ... or, fused with the launch that follows the cycle in the single-reduction loop: znew = z + Phi e_c, partial sums
// of r . znew (k_copy_dot's grid and summation order)
int coarse_enq_copy_dot(feahip_ctx *c, const double *z, const double *r, double *znew, double *part, const int *flag);
void coarse_destroy(feahip_ctx *c);
// views (feahip_coarse_info / _matrix); the context is prepared
int coarse_export_info(feahip_ctx *c, long long *out8, int *agg_of_owned_row, double *centroids);
int coarse_export_matrix(feahip_ctx *c, double *A);
