// feahip_api.hip -- extern "C" entry points of include/fea_hip.h.
#include "feahip_internal.h"
#include <limits>

#undef hipMalloc
hipError_t feahip_device_malloc(void **p, size_t bytes)
{
  static int fill = -1;
  if (fill < 0) { const char *e = getenv("FEAHIP_TEST_NAN_ALLOC"); fill = e && atoi(e) > 0 ? 1 : 0; }
  const hipError_t rc = hipMalloc(p, bytes);
  if (rc == hipSuccess && fill && bytes) { (void)hipMemset(*p, 0xFF, bytes); (void)hipDeviceSynchronize(); }   // (the fill lands before anything a non-blocking stream does)
  return rc;
}
#define hipMalloc(p, bytes) feahip_device_malloc((void **)(p), (bytes))
#include "amg.h"
#include "coarse.h"
#include "node_views.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <utility>

static std::string g_create_error;

extern "C" const char *feahip_create_error(void) { return g_create_error.c_str(); }
extern "C" const char *feahip_last_error(const feahip_ctx *c) { return c ? c->err.c_str() : "null context"; }

// library id of a caller's node
static inline int lib_id(const feahip_ctx *c, int a) { return c->perm.empty() ? a : c->perm[a]; }

// ---- node-ordered views: the caller's numbering on the host side, the library's on the device (node_views.h) --------
static NodeView view_of(const feahip_ctx *c, bool owned_only = false)
{
  const int *perm = c->perm.empty() ? nullptr : c->perm.data();
  return owned_only ? NodeView(perm, c->N, c->row0, c->row1) : NodeView(perm, c->N);
}

static int get_vec(feahip_ctx *c, const double *d, double *h, size_t n)
{
  if (!h) return FEAHIP_EINVAL;
  FEA_HIP_CHECK(c, hipMemcpyAsync(h, d, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

// device d[N][lib_stride] in library ids into the caller's h[N][width].  owned_only: the rows of the shard installed
// now are all that is copied, the nodes of other ranks read as +0
static int get_view(feahip_ctx *c, const double *d, double *h, int width, int lib_stride, bool owned_only = false)
{
  if (!h) return FEAHIP_EINVAL;
  const NodeView v = view_of(c, owned_only);
  if (!v.perm && width == lib_stride && v.all_rows()) return get_vec(c, d, h, (size_t)v.N * width);
  std::vector<double> tmp((size_t)v.N * lib_stride);
  const size_t lo = (size_t)v.row0 * lib_stride;
  int rc;
  if (v.row1 > v.row0 && (rc = get_vec(c, d + lo, tmp.data() + lo, (size_t)(v.row1 - v.row0) * lib_stride))) return rc;
  to_caller(v, width, lib_stride, tmp.data(), h);
  return FEAHIP_OK;
}

// the caller's h[N][width] into device d[N][lib_stride] in library ids, the pad lanes zero
static int set_view(feahip_ctx *c, double *d, const double *h, int width, int lib_stride)
{
  if (!h) return FEAHIP_EINVAL;
  const NodeView v = view_of(c);
  std::vector<double> tmp;
  if (v.perm || width != lib_stride) {
    tmp.resize((size_t)v.N * lib_stride);
    to_library(v, width, lib_stride, h, tmp.data());
    h = tmp.data();
  }
  FEA_HIP_CHECK(c, hipMemcpyAsync(d, h, sizeof(double) * (size_t)v.N * lib_stride, hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

// a device buffer of n doubles that lives for one entry point
struct DevTemp {
  double *p = nullptr;
  DevTemp() = default;
  DevTemp(const DevTemp &) = delete;
  DevTemp &operator=(const DevTemp &) = delete;
  ~DevTemp() { if (p) (void)hipFree(p); }
  int alloc(feahip_ctx *c, size_t n, bool zero = false)
  {
    FEA_HIP_CHECK(c, hipMalloc((void **)&p, sizeof(double) * n));
    return zero && hipMemsetAsync(p, 0, sizeof(double) * n, c->stream) != hipSuccess ? FEAHIP_EHIP : FEAHIP_OK;
  }
};

// Block vectors ([3N][8], kernels_modal.hip) to and from host columns [3N] in the caller's order, through the W block
// of ModalState::d_v as [8][3N] staging.  Up: columns [first, first + count) of host, count <= 8, the columns left of
// the panel zero.  Down: the first count columns; owned_only as in get_view.  One column per transfer.
// (pick: the host column of panel column k is pick[first + k] instead of first + k)
static int upload_columns(feahip_ctx *c, double *dst_block, const double *host, int first, int count, const int *pick = nullptr)
{
  const size_t n = (size_t)c->ndof;
  double *w = c->modal.d_v + n * FEA_MODAL_COLS;
  int rc;
  if (count < FEA_MODAL_COLS) FEA_HIP_CHECK(c, hipMemsetAsync(w + count * n, 0, sizeof(double) * (FEA_MODAL_COLS - count) * n, c->stream));
  for (int k = 0; k < count; ++k)
    if ((rc = set_view(c, w + k * n, host + (size_t)(pick ? pick[first + k] : first + k) * n, 3, 3))) return rc;
  return launch_modal_pack(c, w, dst_block, 0);
}

static int download_columns(feahip_ctx *c, const double *src_block, double *host, int count, bool owned_only = false)
{
  const size_t n = (size_t)c->ndof;
  double *w = c->modal.d_v + n * FEA_MODAL_COLS;
  int rc;
  if ((rc = launch_modal_pack(c, src_block, w, 1))) return rc;
  for (int k = 0; k < count; ++k)
    if ((rc = get_view(c, w + k * n, host + k * n, 3, 3, owned_only))) return rc;
  return FEAHIP_OK;
}

// the ranks a collective call made on one context drives: the members of its in-process group, or the context alone
static std::vector<feahip_ctx *> ranks_of(feahip_ctx *c)
{
  if (c->tr && c->tr->members()) return *c->tr->members();
  return std::vector<feahip_ctx *>(1, c);
}

// The one way the error text of a collective call reaches the caller: a failed call (rc != 0) whose handle `to` holds
// no message gets the first one any of the ranks R holds.  Returns rc.
static int surface_error(feahip_ctx *to, const std::vector<feahip_ctx *> &R, int rc)
{
  if (rc && to->err.empty())
    for (feahip_ctx *r : R) if (!r->err.empty()) { to->err = r->err; break; }
  return rc;
}

template <class T>
static int dev_upload(feahip_ctx *c, T **dst, const T *src, size_t n)
{
  FEA_HIP_CHECK(c, hipMalloc((void **)dst, sizeof(T) * (n ? n : 1)));
  if (n) FEA_HIP_CHECK(c, hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice));
  return FEAHIP_OK;
}

template <class T>
static int dev_zeros(feahip_ctx *c, T **dst, size_t n)
{
  FEA_HIP_CHECK(c, hipMalloc((void **)dst, sizeof(T) * (n ? n : 1)));
  FEA_HIP_CHECK(c, hipMemset(*dst, 0, sizeof(T) * (n ? n : 1)));
  return FEAHIP_OK;
}

int ensure_generic_maps(feahip_ctx *c)
{
  GenericMaps &g = c->generic;
  if (g.built()) return FEAHIP_OK;
  if (!c->h_pat) { c->err = "incidence maps unavailable"; return FEAHIP_ESTATE; }
  const HostPattern &hp = *c->h_pat;
  int rc;
  if ((rc = dev_upload(c, &g.d_incptr, hp.incptr.data(), hp.incptr.size()))) return rc;
  if ((rc = dev_upload(c, &g.d_inc, hp.inc.data(), hp.inc.size()))) return rc;
  if (!hp.incslot.empty() && (rc = dev_upload(c, &g.d_incslot, hp.incslot.data(), hp.incslot.size()))) return rc;
  g.record(MapOutcome::built, 0, c->N);
  return FEAHIP_OK;
}

// K for the rows of the shard installed now (see feahip_internal.h)
int ensure_k(feahip_ctx *c)
{
  if (c->d_K_base) return FEAHIP_OK;
  c->kb0 = c->h_rowptr[c->row0]; c->kb1 = c->h_rowptr[c->row1];
  // +2: the SpMV reads aligned 80-byte windows; +1: a shard whose first block is odd starts one double into the
  // allocation, so that EVEN global value indices are 16-byte aligned on every rank (the gather kernels pick the
  // alignment of their 16-byte row stores from the parity of the chunk's first global block)
  const size_t n = (size_t)(c->kb1 - c->kb0) * 9 + 3;
  FEA_HIP_CHECK(c, hipMalloc((void **)&c->d_K_alloc, sizeof(double) * n));
  // on the context's own (non-blocking) stream: a null-stream memset is not ordered against the kernels that follow
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d_K_alloc, 0, sizeof(double) * n, c->stream));
  c->d_K_base = c->d_K_alloc + (c->kb0 & 1);
  c->d_K = c->d_K_base - (size_t)c->kb0 * 9;
  return FEAHIP_OK;
}

void release_k(feahip_ctx *c)
{
  if (c->d_K_alloc) (void)hipFree(c->d_K_alloc);
  if (c->d_Kstash_alloc) (void)hipFree(c->d_Kstash_alloc);
  c->d_K_alloc = c->d_Kstash_alloc = c->d_K_base = c->d_Kstash_base = c->d_K = c->d_Kstash = nullptr;
  c->have_stash = false; c->k_bc = false; c->k_valid = false; ++c->k_epoch;
}

// shared-state maps of 10-node elements for the assembly chunks this rank owns
int ensure_quad(feahip_ctx *c)
{
  QuadMaps &q = c->quad;
  const int a0 = c->achunk0, a1 = c->achunk0 + c->nachunks_local;
  if (q.settled(a0, a1) || c->npe != 10 || !c->h_pat || c->h_conn.empty()) return FEAHIP_OK;
  HostQuad hq;
  build_host_quad(c->N, c->E, c->npe, c->h_conn.data(), *c->h_pat, a0, a1, hq);
  q.release();
  if (!hq.ok) { q.record(MapOutcome::failed, a0, a1); return FEAHIP_OK; }
  int rc;
  if ((rc = dev_upload(c, &q.d_desc, hq.desc.data(), hq.desc.size()))) return rc;
  if ((rc = dev_upload(c, &q.d_elem, hq.qelem.data(), hq.qelem.size()))) return rc;
  if ((rc = dev_upload(c, &q.d_pair, hq.qpair.data(), hq.qpair.size()))) return rc;
  if ((rc = dev_upload(c, &q.d_node, hq.qnode.data(), hq.qnode.size()))) return rc;
  q.nchunks = c->nachunks_local;
  q.bytes = (long long)(hq.desc.size() * sizeof(QuadDesc) + hq.qelem.size() * 4 + hq.qpair.size() * 4 + hq.qnode.size() * 4);
  q.record(MapOutcome::built, a0, a1);
  return FEAHIP_OK;
}

int ensure_visits(feahip_ctx *c)
{
  VisitMaps &v = c->visits;
  if (v.settled(0, c->N) || !c->h_pat || c->h_conn.empty()) return FEAHIP_OK;
  HostVisits hv;
  build_host_visits(c->N, c->E, c->h_conn.data(), *c->h_pat, hv);
  if (!hv.ok) { v.record(MapOutcome::failed, 0, c->N); return FEAHIP_OK; }
  int rc;
  if ((rc = dev_upload(c, &v.d_desc, hv.desc.data(), hv.desc.size()))) return rc;
  if ((rc = dev_upload(c, &v.d_node, hv.vnode.data(), hv.vnode.size()))) return rc;
  if ((rc = dev_upload(c, &v.d_rec, hv.vrec.data(), hv.vrec.size()))) return rc;
  v.nrecords = (int)(hv.vrec.size() / 2);
  v.bytes = (long long)(hv.desc.size() * sizeof(VisitDesc) + hv.vnode.size() * 4 + hv.vrec.size() * 4);
  v.record(MapOutcome::built, 0, c->N);
  return FEAHIP_OK;
}

static int create_impl(feahip_ctx *c, int device, int n_nodes, int n_elems, int npe, int gauss_count,
                       const double *gauss_weights, const double *dforms, const int *elements,
                       const double *nodes0, int model, const double *model_params,
                       int params_count, int n_presc, const int *presc_node,
                       const int *presc_type, const double *presc_values)
{
  if (n_nodes <= 0 || n_elems <= 0 || !gauss_weights || !dforms || !elements || !nodes0 || !model_params) {
    c->err = "feahip_create: null or empty input"; return FEAHIP_EINVAL;
  }
  if (npe != 4 && npe != 8 && npe != 10) { c->err = "nodes per element must be 4, 8 or 10"; return FEAHIP_EINVAL; }
  if (gauss_count < 1 || gauss_count > FEA_MAX_GAUSS) { c->err = "gauss_count out of range"; return FEAHIP_EINVAL; }
  if (model != FEAHIP_MODEL_A5 && model != FEAHIP_MODEL_COMPRESSIBLE_NEOHOOKEAN) { c->err = "unknown material model"; return FEAHIP_EINVAL; }
  if (params_count < 2) { c->err = "material needs lambda and mu"; return FEAHIP_EINVAL; }
  if (n_presc < 0 || (n_presc > 0 && (!presc_node || !presc_type || !presc_values))) { c->err = "bad prescribed-displacement arrays"; return FEAHIP_EINVAL; }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    c->err = "no HIP device visible: this path has no CPU fallback"; return FEAHIP_ENODEVICE;
  }
  if (device < 0 || device >= ndev) { c->err = "device index out of range"; return FEAHIP_EINVAL; }
  c->device = device;
  FEA_HIP_CHECK(c, hipSetDevice(device));
  FEA_HIP_CHECK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));

  c->N = n_nodes; c->E = n_elems; c->npe = npe; c->G = gauss_count; c->ndof = 3 * n_nodes;
  c->model = model; c->lambda = model_params[0]; c->mu = model_params[1];

  // ---- the library's own node numbering (renumber.cpp).  From here on `elements`, `nodes0` and `presc_node` are
  // the permuted copies; the caller's ids come back at the getters.  FEAHIP_RENUMBER=0 keeps the caller's numbering
  // (measurement knob: what the kernels make of the ids as given).
  std::vector<int> elements_p, presc_p;
  std::vector<double> nodes_p;
  {
    for (long long i = 0; i < (long long)n_elems * npe; ++i)
      if (elements[i] < 0 || elements[i] >= n_nodes) {
        c->err = "element " + std::to_string(i / npe) + " refers to node " + std::to_string(elements[i]) + " outside [0," + std::to_string(n_nodes) + ")";
        return FEAHIP_EINVAL;
      }
    const char *e = getenv("FEAHIP_RENUMBER");
    if (c->rank_own < 0 && !(e && atoi(e) == 0) && locality_numbering(n_nodes, n_elems, npe, elements, nodes0, c->perm)) {
      bool identity = true;
      for (int a = 0; a < n_nodes && identity; ++a) identity = c->perm[a] == a;
      if (identity) c->perm.clear();
    } else c->perm.clear();
    if (!c->perm.empty()) {
      c->iperm.resize((size_t)n_nodes);
      for (int a = 0; a < n_nodes; ++a) c->iperm[c->perm[a]] = a;
      elements_p.resize((size_t)n_elems * npe);
      for (size_t i = 0; i < elements_p.size(); ++i) elements_p[i] = c->perm[elements[i]];
      nodes_p.resize((size_t)n_nodes * 3);
      for (int a = 0; a < n_nodes; ++a)
        for (int j = 0; j < 3; ++j) nodes_p[(size_t)c->perm[a] * 3 + j] = nodes0[(size_t)a * 3 + j];
      presc_p.resize((size_t)n_presc);
      for (int i = 0; i < n_presc; ++i) {
        if (presc_node[i] < 0 || presc_node[i] >= n_nodes) { c->err = "prescribed node id out of range"; return FEAHIP_EINVAL; }
        presc_p[i] = c->perm[presc_node[i]];
      }
      elements = elements_p.data(); nodes0 = nodes_p.data(); presc_node = presc_p.data();
    }
  }

  memset(&c->table, 0, sizeof(c->table));
  for (int g = 0; g < gauss_count; ++g) {
    c->table.w[g] = gauss_weights[g];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < npe; ++k) c->table.dN[g][i][k] = dforms[((size_t)g * 3 + i) * npe + k];
  }
  c->linear_tet = (npe == 4);
  for (int g = 0; g < gauss_count && c->linear_tet; ++g)
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 4; ++k) {
        const double want = (k == 0) ? -1.0 : ((k - 1 == i) ? 1.0 : 0.0);
        if (c->table.dN[g][i][k] != want) c->linear_tet = false;
      }
  int rc;
  if ((rc = dev_upload(c, &c->d_table, &c->table, 1))) return rc;

  // pattern + incidence maps (host, once)
  c->h_pat = new HostPattern();
  HostPattern &hp = *c->h_pat;
  if ((rc = build_host_pattern(n_nodes, n_elems, npe, elements, hp, c->err, c->rank_own))) return rc;    // (a rank context: chunks break at its first halo row)
  c->nnzb = (int)hp.colidx.size();
  c->max_rowlen = hp.max_rowlen;
  c->nchunks = (int)hp.chunk.size() - 1;
  c->chunk0 = 0; c->nchunks_local = c->nchunks;
  c->nachunks = hp.achunk.empty() ? 0 : (int)hp.achunk.size() - 1;
  c->achunk0 = 0; c->nachunks_local = c->nachunks;
  c->h_super_achunk = hp.super_achunk;
  c->h_chunk = hp.chunk;
  if (c->rank_own >= 0) {                                   // a rank context: the chunks of the rows it owns
    c->nchunks_local = hp.break_chunk;
    if (!hp.super_achunk.empty()) c->nachunks_local = hp.super_achunk[hp.break_super];
  }
  c->row0 = 0; c->row1 = n_nodes;
  c->ichunk_lo = 0; c->ichunk_hi = c->nchunks;
  c->h_rowptr = hp.rowptr; c->h_colidx = hp.colidx;
  c->incslot_ok = !hp.incslot.empty();

  if ((rc = dev_upload(c, &c->d_conn, elements, (size_t)n_elems * npe))) return rc;
  {
    std::vector<double> pad((size_t)n_nodes * 4, 0.0);
    for (int a = 0; a < n_nodes; ++a)
      for (int j = 0; j < 3; ++j) pad[(size_t)a * 4 + j] = nodes0[(size_t)a * 3 + j];
    if ((rc = dev_upload(c, &c->d_X0, pad.data(), pad.size()))) return rc;
    if ((rc = dev_upload(c, &c->d_x, pad.data(), pad.size()))) return rc;   // nodes_p = copy of nodes0 (:400)
  }
  if ((rc = dev_upload(c, &c->d_rowptr, hp.rowptr.data(), hp.rowptr.size()))) return rc;
  if ((rc = dev_upload(c, &c->d_colidx, hp.colidx.data(), hp.colidx.size()))) return rc;
  if ((rc = dev_upload(c, &c->d_chunk, hp.chunk.data(), hp.chunk.size()))) return rc;
  if ((rc = dev_upload(c, &c->d_diag, hp.diag.data(), hp.diag.size()))) return rc;
  c->generic.bytes = (long long)(hp.incptr.size() * 4 + hp.inc.size() * 4 + hp.incslot.size() +
                             hp.chunk.size() * 4 + hp.rowptr.size() * 4 + hp.diag.size() * 4);

  const bool lin1 = c->linear_tet && gauss_count == 1;
  if (lin1) {
    // the maps of every linear-tet strategy (gather, staged visits, generic incidence lists) are
    // built the first time a launch asks for them, from these host copies -- for the rows this rank owns where
    // the strategy allows (gather)
    c->h_conn.assign(elements, elements + (size_t)n_elems * npe);
  } else if ((rc = ensure_generic_maps(c))) return rc;
  if (npe == 10 || npe == 8) c->h_conn.assign(elements, elements + (size_t)n_elems * npe);      // gather / shared-state maps: built per shard on first use
  if (!lin1 && npe != 10 && npe != 8) { delete c->h_pat; c->h_pat = nullptr; }                   // nothing is built later for these meshes
  if ((rc = dev_zeros(c, &c->d_f, (size_t)c->ndof))) return rc;
  if ((rc = dev_zeros(c, &c->d_u, (size_t)c->ndof))) return rc;
  if ((rc = dev_zeros(c, &c->d_r, (size_t)c->ndof))) return rc;
  if ((rc = dev_zeros(c, &c->d_p, (size_t)c->ndof))) return rc;
  if ((rc = dev_zeros(c, &c->d_q, (size_t)c->ndof))) return rc;
  if ((rc = dev_zeros(c, &c->d_minv, (size_t)c->N * 9))) return rc;
  if ((rc = dev_zeros(c, &c->d_part, (size_t)6 * FEA_RED_BLOCKS))) return rc;
  if ((rc = dev_zeros(c, &c->d_scal, (size_t)16))) return rc;
  if ((rc = dev_zeros(c, &c->d_flag, (size_t)4))) return rc;

  // prescribed dofs in the order solver_apply_bc_general visits them
  // (fea_solver.c:1210-1240): deck order, x then y then z of a node
  std::vector<int> cdof;
  std::vector<double> cval;
  std::vector<uint8_t> mask((size_t)c->ndof, 0);
  for (int i = 0; i < n_presc; ++i) {
    const int node = presc_node[i], type = presc_type[i];
    if (node < 0 || node >= n_nodes) { c->err = "prescribed node id out of range"; return FEAHIP_EINVAL; }
    if (type < 0 || type > 7) { c->err = "prescribed type must be a 3-bit mask"; return FEAHIP_EINVAL; }
    for (int j = 0; j < 3; ++j)
      if (type & (1 << j)) {
        cdof.push_back(node * 3 + j);
        cval.push_back(presc_values[(size_t)i * 3 + j]);
        mask[(size_t)node * 3 + j] = 1;
      }
  }
  c->n_presc = n_presc;
  c->n_cdof = (int)cdof.size();
  if ((rc = dev_upload(c, &c->d_cdof, cdof.data(), cdof.size()))) return rc;
  if ((rc = dev_upload(c, &c->d_cval, cval.data(), cval.size()))) return rc;
  if ((rc = dev_upload(c, &c->d_dofmask, mask.data(), mask.size()))) return rc;
  return FEAHIP_OK;
}

extern "C" int feahip_create(feahip_ctx **out, int device, int n_nodes, int n_elems, int npe,
                             int gauss_count, const double *gauss_weights, const double *dforms,
                             const int *elements, const double *nodes0, int model,
                             const double *model_params, int params_count, int n_presc,
                             const int *presc_node, const int *presc_type,
                             const double *presc_values)
{
  if (!out) { g_create_error = "null output pointer"; return FEAHIP_EINVAL; }
  *out = nullptr;
  feahip_ctx *c = new (std::nothrow) feahip_ctx();
  if (!c) { g_create_error = "out of host memory"; return FEAHIP_ENOMEM; }
  int rc = create_impl(c, device, n_nodes, n_elems, npe, gauss_count, gauss_weights, dforms, elements,
                       nodes0, model, model_params, params_count, n_presc, presc_node, presc_type,
                       presc_values);
  if (rc != FEAHIP_OK) {
    g_create_error = c->err;
    feahip_destroy(c);
    return rc;
  }
  *out = c;
  return FEAHIP_OK;
}

// One rank's context of a sharded run: the sub-mesh of rankmesh.cpp as an ordinary context -- locally indexed, rows
// [0, n_own) owned, the halo plan installed -- so that nothing on a rank is sized by the whole mesh.
extern "C" int feahip_create_rank(feahip_ctx **out, int device, int rank, int nranks, int n_nodes, int n_elems, int npe,
                                  int gauss_count, const double *gauss_weights, const double *dforms,
                                  const int *elements, const double *nodes0, int model,
                                  const double *model_params, int params_count, int n_presc,
                                  const int *presc_node, const int *presc_type, const double *presc_values)
{
  if (!out) { g_create_error = "null output pointer"; return FEAHIP_EINVAL; }
  *out = nullptr;
  if (n_nodes <= 0 || n_elems <= 0 || !elements || !nodes0 || (npe != 4 && npe != 8 && npe != 10) ||
      n_presc < 0 || (n_presc > 0 && (!presc_node || !presc_type || !presc_values))) {
    g_create_error = "feahip_create_rank: null or empty input"; return FEAHIP_EINVAL;
  }
  RankMesh rm;
  int rc = build_rank_mesh(rank, nranks, n_nodes, n_elems, npe, elements, nodes0, n_presc, presc_node, presc_type, presc_values, rm, g_create_error);
  if (rc) return rc;
  if (rm.elem_global.empty() || rm.n_own <= 0) { g_create_error = "this rank owns no node of the mesh (more ranks than slabs)"; return FEAHIP_EINVAL; }
  feahip_ctx *c = new (std::nothrow) feahip_ctx();
  if (!c) { g_create_error = "out of host memory"; return FEAHIP_ENOMEM; }
  c->rank_own = rm.n_own;
  rc = create_impl(c, device, (int)rm.node_global.size(), (int)rm.elem_global.size(), npe, gauss_count, gauss_weights, dforms,
                   rm.elements.data(), rm.nodes0.data(), model, model_params, params_count, (int)rm.presc_node.size(),
                   rm.presc_node.data(), rm.presc_type.data(), rm.presc_values.data());
  if (rc == FEAHIP_OK) {
    rc = install_plan(c, rm.plan);                         // rows [0, n_own), peers, halo lists, interior chunk range
  }
  if (rc != FEAHIP_OK) { g_create_error = c->err; feahip_destroy(c); return rc; }
  c->rank_node_global = rm.node_global; c->rank_elem_global = rm.elem_global; c->rank_n_global = n_nodes; c->rank_e_global = n_elems;
  *out = c;
  return FEAHIP_OK;
}

// The same context from the caller's own slab: local nodes, local elements, halo owners -- no whole mesh anywhere.  The
// local order is the caller's (feahip_host_slab_order offers one that suits the kernels).
extern "C" int feahip_create_rank_local(feahip_ctx **out, int device, int rank, int nranks, int n_global_nodes, int n_local,
                                        int n_own, int n_elems, int npe, int gauss_count, const double *gauss_weights,
                                        const double *dforms, const int *elements, const double *nodes0,
                                        const int *node_global, const int *elem_global, const int *halo_owner, int model,
                                        const double *model_params, int params_count, int n_presc, const int *presc_node,
                                        const int *presc_type, const double *presc_values)
{
  if (!out) { g_create_error = "null output pointer"; return FEAHIP_EINVAL; }
  *out = nullptr;
  if (n_local <= 0 || n_elems <= 0 || !elements || !nodes0 || !node_global || (npe != 4 && npe != 8 && npe != 10) ||
      n_presc < 0 || (n_presc > 0 && (!presc_node || !presc_type || !presc_values))) {
    g_create_error = "feahip_create_rank_local: null or empty input"; return FEAHIP_EINVAL;
  }
  RankMesh rm;
  int rc = build_rank_mesh_local(rank, nranks, n_global_nodes, n_local, n_own, n_elems, npe, elements, nodes0, node_global,
                                 elem_global, halo_owner, n_presc, presc_node, presc_type, presc_values, rm, g_create_error);
  if (rc) return rc;
  feahip_ctx *c = new (std::nothrow) feahip_ctx();
  if (!c) { g_create_error = "out of host memory"; return FEAHIP_ENOMEM; }
  c->rank_own = rm.n_own; c->rank_local_ids = true;
  rc = create_impl(c, device, n_local, n_elems, npe, gauss_count, gauss_weights, dforms, rm.elements.data(), rm.nodes0.data(),
                   model, model_params, params_count, (int)rm.presc_node.size(), rm.presc_node.data(), rm.presc_type.data(),
                   rm.presc_values.data());
  if (rc == FEAHIP_OK) rc = install_plan(c, rm.plan);
  if (rc != FEAHIP_OK) { g_create_error = c->err; feahip_destroy(c); return rc; }
  c->rank_node_global.swap(rm.node_global); c->rank_elem_global.swap(rm.elem_global); c->rank_n_global = n_global_nodes;
  *out = c;
  return FEAHIP_OK;
}

// Host-only: the plan that call installs, in GLOBAL node ids (counts[3] by a first call with null lists).
extern "C" int feahip_host_rank_local_plan(int rank, int nranks, int n_local, int n_own, int n_elems, int npe,
                                           const int *elements, const int *node_global, const int *halo_owner, int *counts,
                                           int *peers, int *send_off, int *recv_off, int *send_idx, int *recv_idx)
{
  if (!counts) return FEAHIP_EINVAL;
  RankMesh rm;
  int rc = build_rank_mesh_local(rank, nranks, -1, n_local, n_own, n_elems, npe, elements, nullptr, node_global, nullptr,
                                 halo_owner, 0, nullptr, nullptr, nullptr, rm, g_create_error);
  if (rc) return rc;
  const ShardPlan &pl = rm.plan;
  counts[0] = (int)pl.peer.size(); counts[1] = (int)pl.send_idx.size(); counts[2] = (int)pl.recv_idx.size();
  if (peers) std::copy(pl.peer.begin(), pl.peer.end(), peers);
  if (send_off) std::copy(pl.send_off.begin(), pl.send_off.end(), send_off);
  if (recv_off) std::copy(pl.recv_off.begin(), pl.recv_off.end(), recv_off);
  if (send_idx) for (size_t i = 0; i < pl.send_idx.size(); ++i) send_idx[i] = rm.node_global[pl.send_idx[i]];
  if (recv_idx) for (size_t i = 0; i < pl.recv_idx.size(); ++i) recv_idx[i] = rm.node_global[pl.recv_idx[i]];
  return FEAHIP_OK;
}

// Host-only: a local order for a slab (rankmesh.cpp slab_order); 1 when it reorders, 0 when the order given is kept.
extern "C" int feahip_host_slab_order(int n_local, int n_own, int n_elems, int npe, const int *elements, const double *nodes0,
                                      int *new_local_id)
{
  if (!elements || !nodes0 || !new_local_id || n_local <= 0 || n_elems <= 0 || n_own < 1 || n_own > n_local ||
      (npe != 4 && npe != 8 && npe != 10)) return FEAHIP_EINVAL;
  for (long long i = 0; i < (long long)n_elems * npe; ++i)
    if (elements[i] < 0 || elements[i] >= n_local) return FEAHIP_EINVAL;
  return slab_order(n_local, n_own, n_elems, npe, elements, nodes0, new_local_id);
}

extern "C" int feahip_rank_counts(feahip_ctx *c, long long *o)
{
  if (!c || !o || c->rank_own < 0) return FEAHIP_EINVAL;
  o[0] = c->N; o[1] = c->rank_own; o[2] = c->E; o[3] = c->rank_n_global; o[4] = c->nnzb;
  o[5] = (long long)c->h_rowptr[c->rank_own]; o[6] = c->nsend; o[7] = c->nrecv;
  return FEAHIP_OK;
}

extern "C" int feahip_rank_maps(feahip_ctx *c, int *node_global, int *elem_global)
{
  if (!c || c->rank_own < 0) return FEAHIP_EINVAL;
  if (node_global) std::copy(c->rank_node_global.begin(), c->rank_node_global.end(), node_global);
  if (elem_global) std::copy(c->rank_elem_global.begin(), c->rank_elem_global.end(), elem_global);
  return FEAHIP_OK;
}

// Host-only (no device): what rank `rank` of `nranks` would hold -- counts[8] = {local nodes, owned nodes, local
// elements, blocks of the owned rows, blocks of all local rows, peers, rows sent, rows received}; with non-null arrays
// (sized by a first call) the local nodes' caller ids, the local elements' caller indices, and the block rows of the
// OWNED nodes as built from the rank's own elements (rowptr[owned + 1], column = CALLER id of the column node).
extern "C" int feahip_host_rank_mesh(int rank, int nranks, int n_nodes, int n_elems, int npe, const int *elements,
                                     const double *nodes0, long long *counts, int *node_global, int *elem_global,
                                     long long *rowptr, int *colidx)
{
  if (!elements || !nodes0 || !counts || n_nodes <= 0 || n_elems <= 0) return FEAHIP_EINVAL;
  RankMesh rm;
  std::string err;
  int rc = build_rank_mesh(rank, nranks, n_nodes, n_elems, npe, elements, nodes0, 0, nullptr, nullptr, nullptr, rm, err);
  if (rc) return rc;
  HostPattern hp;
  const int nl = (int)rm.node_global.size();
  if ((rc = build_host_pattern(nl, (int)rm.elem_global.size(), npe, rm.elements.data(), hp, err, rm.n_own))) return rc;
  counts[0] = nl; counts[1] = rm.n_own; counts[2] = (long long)rm.elem_global.size();
  counts[3] = hp.rowptr[rm.n_own]; counts[4] = (long long)hp.colidx.size();
  counts[5] = (long long)rm.plan.peer.size(); counts[6] = (long long)rm.plan.send_idx.size(); counts[7] = (long long)rm.plan.recv_idx.size();
  if (node_global) std::copy(rm.node_global.begin(), rm.node_global.end(), node_global);
  if (elem_global) std::copy(rm.elem_global.begin(), rm.elem_global.end(), elem_global);
  if (rowptr && colidx) {
    for (int a = 0; a <= rm.n_own; ++a) rowptr[a] = hp.rowptr[a];
    for (int q = 0; q < hp.rowptr[rm.n_own]; ++q) colidx[q] = rm.node_global[hp.colidx[q]];
  }
  return FEAHIP_OK;
}

// Host-only: the halo plan of one rank's sub-mesh in the CALLER's node ids (counts[3] = {peers, rows sent, rows received}
// by a first call with null lists): what it sends to and receives from every peer, in the order the rows travel.
extern "C" int feahip_host_rank_plan(int rank, int nranks, int n_nodes, int n_elems, int npe, const int *elements,
                                     const double *nodes0, int *counts, int *peers, int *send_off, int *recv_off,
                                     int *send_idx, int *recv_idx)
{
  if (!elements || !nodes0 || !counts || n_nodes <= 0 || n_elems <= 0) return FEAHIP_EINVAL;
  RankMesh rm;
  std::string err;
  int rc = build_rank_mesh(rank, nranks, n_nodes, n_elems, npe, elements, nodes0, 0, nullptr, nullptr, nullptr, rm, err);
  if (rc) return rc;
  const ShardPlan &pl = rm.plan;
  counts[0] = (int)pl.peer.size(); counts[1] = (int)pl.send_idx.size(); counts[2] = (int)pl.recv_idx.size();
  if (peers) std::copy(pl.peer.begin(), pl.peer.end(), peers);
  if (send_off) std::copy(pl.send_off.begin(), pl.send_off.end(), send_off);
  if (recv_off) std::copy(pl.recv_off.begin(), pl.recv_off.end(), recv_off);
  if (send_idx) for (size_t i = 0; i < pl.send_idx.size(); ++i) send_idx[i] = rm.node_global[pl.send_idx[i]];
  if (recv_idx) for (size_t i = 0; i < pl.recv_idx.size(); ++i) recv_idx[i] = rm.node_global[pl.recv_idx[i]];
  return FEAHIP_OK;
}

extern "C" void feahip_destroy(feahip_ctx *c)
{
  if (!c) return;
  delete c->h_pat; c->h_pat = nullptr;
  c->generic.release(); c->visits.release(); c->quad.release(); c->gather.release(); c->gather10.release();
  c->surf.release();
  c->contact.release();
  c->mass.release();
  c->damping.release();
  c->results.release();
  c->modal.release();
  c->response.release();
  c->stress.release();
  c->buckling.release();
  c->fatigue.release();
  c->rainflow.release();
  void *ptrs[] = {c->d_table, c->d_conn, c->d_X0, c->d_x, c->d_rowptr, c->d_colidx, c->d_K_alloc, c->d_Kstash_alloc,
                  c->d_chunk, c->d_diag, c->d_f, c->d_u, c->d_r, c->d_p,
                  c->d_q, c->d_minv, c->d_part, c->d_scal, c->d_flag, c->d_cdof, c->d_cval,
                  c->d_dofmask, c->d_F, c->d_S, c->d_mat, c->d_elem_mat, c->d_f_discard};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  for (void *p : {(void *)c->d_send_idx, (void *)c->d_recv_idx, (void *)c->d_send_buf, (void *)c->d_recv_buf, (void *)c->d_z, (void *)c->d_w, (void *)c->d_s})
    if (p) (void)hipFree(p);
  if (c->ev_packed) (void)hipEventDestroy(c->ev_packed);
  if (c->ev_unpacked) (void)hipEventDestroy(c->ev_unpacked);
  if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
  if (c->tr && c->owns_tr) delete c->tr;
  release_solve2(c);
  amg_destroy(c);
  coarse_destroy(c);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

#define CTX_GUARD_NOK(c)                          \
  if (!(c)) return FEAHIP_EINVAL;                 \
  FEA_HIP_CHECK(c, hipSetDevice((c)->device))
// entry points that read or write K make sure it exists for the shard installed now
#define CTX_GUARD(c)                              \
  CTX_GUARD_NOK(c);                               \
  { const int _rk = ensure_k(c); if (_rk) return _rk; }

extern "C" int feahip_sync(feahip_ctx *c)
{
  CTX_GUARD_NOK(c);
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

extern "C" int feahip_set_assembly(feahip_ctx *c, int strategy)
{
  CTX_GUARD_NOK(c);
  if (strategy < FEAHIP_ASM_AUTO || strategy > FEAHIP_ASM_GATHER) { c->err = "unknown assembly strategy"; return FEAHIP_EINVAL; }
  c->strategy = strategy;
  return FEAHIP_OK;
}

extern "C" int feahip_set_preconditioner(feahip_ctx *c, int kind)
{
  CTX_GUARD(c);
  if (kind < 0 || kind > 2) { c->err = "unknown preconditioner"; return FEAHIP_EINVAL; }
  if (kind >= 1) { int rc = amg_create(c); if (rc) return rc; }
  if (kind != 2) coarse_destroy(c);                    // nothing of the coarse level outlives kind 2
  c->precond = kind;
  return FEAHIP_OK;
}

extern "C" int feahip_set_pcg_variant(feahip_ctx *c, int variant)
{
  CTX_GUARD_NOK(c);
  if (variant < -1 || variant > 1) { c->err = "unknown PCG variant"; return FEAHIP_EINVAL; }
  c->pcg_variant = variant;
  return FEAHIP_OK;
}

extern "C" int feahip_set_line_search(feahip_ctx *c, int max_iterations)
{
  CTX_GUARD_NOK(c);
  if (max_iterations < 0) { c->err = "line search iterations must be >= 0"; return FEAHIP_EINVAL; }
  c->linesearch_max = max_iterations;
  return FEAHIP_OK;
}

extern "C" int feahip_set_row_shard(feahip_ctx *c, int rank, int nranks)
{
  CTX_GUARD_NOK(c);
  return install_shard(c, rank, nranks);
}

extern "C" int feahip_update_nodes_with_bc(feahip_ctx *c, double lambda)
{
  CTX_GUARD_NOK(c);
  c->state_valid = false;
  c->load_factor += lambda;                          // one increment of the surface loads, as of the displacements
  return launch_update_nodes_bc(c, lambda);
}

extern "C" int feahip_update_state(feahip_ctx *c, int *n_bad)
{
  CTX_GUARD_NOK(c);
  c->state_valid = false;
  if (n_bad) {
    FEA_HIP_CHECK(c, hipMemcpyAsync(&c->last_bad, c->d_flag + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    *n_bad = c->last_bad;
  }
  return FEAHIP_OK;
}

extern "C" int feahip_create_stiffness(feahip_ctx *c) { CTX_GUARD(c); ++c->k_epoch; c->k_bc = false; return launch_assemble(c, true, false); }
extern "C" int feahip_create_residual_forces(feahip_ctx *c) { CTX_GUARD(c); return launch_assemble(c, false, true); }
extern "C" int feahip_create_stiffness_and_residual(feahip_ctx *c) { CTX_GUARD(c); ++c->k_epoch; c->k_bc = false; return launch_assemble(c, true, true); }

extern "C" int feahip_stash_stiffness(feahip_ctx *c)
{
  CTX_GUARD(c);
  const size_t bytes = sizeof(double) * 9 * (size_t)(c->kb1 - c->kb0);
  if (!c->d_Kstash_base) {
    FEA_HIP_CHECK(c, hipMalloc((void **)&c->d_Kstash_alloc, bytes + 8));
    c->d_Kstash_base = c->d_Kstash_alloc + (c->kb0 & 1);      // same 16-byte phase as K
    c->d_Kstash = c->d_Kstash_base - (size_t)c->kb0 * 9;
  }
  FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_Kstash_base, c->d_K_base, bytes, hipMemcpyDeviceToDevice, c->stream));
  c->have_stash = true;
  c->stash_epoch = c->k_epoch;
  return FEAHIP_OK;
}

extern "C" int feahip_restore_stiffness(feahip_ctx *c)
{
  CTX_GUARD(c);
  if (!c->have_stash) { c->err = "restore_stiffness before stash_stiffness"; return FEAHIP_ESTATE; }
  FEA_HIP_CHECK(c, hipMemcpyAsync(c->d_K_base, c->d_Kstash_base, sizeof(double) * 9 * (size_t)(c->kb1 - c->kb0),
                                  hipMemcpyDeviceToDevice, c->stream));
  c->k_epoch = c->stash_epoch; c->k_bc = false;
  return FEAHIP_OK;
}

extern "C" int feahip_apply_prescribed_bc(feahip_ctx *c, double lambda) { CTX_GUARD(c); c->k_bc = true; return launch_apply_bc(c, lambda); }

extern "C" int feahip_solve_slae(feahip_ctx *c, int type, double tol, int max_iter, int *iters, double *resid)
{
  CTX_GUARD(c);
  if (type < FEAHIP_CG || type > FEAHIP_CHOLESKY) { c->err = "unknown solver type"; return FEAHIP_EINVAL; }
  if (max_iter <= 0) { c->err = "max_iterations must be positive"; return FEAHIP_EINVAL; }
  return solve_pcg(c, type, tol, max_iter, iters, resid);    // block-Jacobi or multigrid by the context's setting
}

extern "C" int feahip_energy(feahip_ctx *c, double *tolerance)
{
  CTX_GUARD(c);
  if (!tolerance) return FEAHIP_EINVAL;
  std::vector<feahip_ctx *> R(1, c);
  return dist_energy(R, tolerance);
}

extern "C" int feahip_update_nodes_with_solution(feahip_ctx *c, const double *u)
{
  CTX_GUARD(c);
  std::vector<feahip_ctx *> R(1, c);
  std::vector<double> tmp;
  if (u && !c->perm.empty()) {
    tmp.resize((size_t)c->ndof);
    to_library(view_of(c), 3, 3, u, tmp.data());
    u = tmp.data();
  }
  return dist_update_nodes_with_solution(R, u);
}

extern "C" int feahip_solve(feahip_ctx *c, int load_increments, int max_newton, int modified_newton,
                            double desired_tolerance, int solver_type, double solver_tolerance,
                            int solver_max_iter, double *tol_log, int tol_log_cap, int *its_log,
                            int *steps_done)
{
  CTX_GUARD(c);
  std::vector<feahip_ctx *> R(1, c);
  return dist_newton(R, load_increments, max_newton, modified_newton, desired_tolerance, solver_type,
                     solver_tolerance, solver_max_iter, tol_log, tol_log_cap, its_log, steps_done);
}

// ---- surface loads (kernels_surface.hip) ------------------------------------

extern "C" int feahip_set_surface_loads(feahip_ctx *c, int n_faces, int nodes_per_face, const int *face_nodes,
                                        const int *kind, const double *values)
{
  CTX_GUARD_NOK(c);
  return set_surface_loads(c, n_faces, nodes_per_face, face_nodes, kind, values);
}

extern "C" int feahip_get_surface_forces(feahip_ctx *c, double *f)
{
  CTX_GUARD_NOK(c);
  if (!f) return FEAHIP_EINVAL;
  DevTemp d;
  int rc;
  if ((rc = d.alloc(c, (size_t)c->ndof, true)) || (rc = launch_surface_loads(c, d.p))) return rc;
  return get_view(c, d.p, f, 3, 3);
}

extern "C" int feahip_set_load_factor(feahip_ctx *c, double lambda)
{
  CTX_GUARD_NOK(c);
  c->load_factor = lambda;
  return FEAHIP_OK;
}

extern "C" int feahip_get_load_factor(feahip_ctx *c, double *lambda)
{
  if (!c || !lambda) return FEAHIP_EINVAL;
  *lambda = c->load_factor;
  return FEAHIP_OK;
}

// ---- contact with rigid obstacles (kernels_contact.hip) ----------------------
extern "C" int feahip_set_contact(feahip_ctx *c, int n_faces, int nodes_per_face, const int *face_nodes, int n_obstacles,
                                  const int *kind, const double *geom, double penalty, int augment_max, double gap_tolerance)
{
  CTX_GUARD_NOK(c);
  return set_contact(c, n_faces, nodes_per_face, face_nodes, n_obstacles, kind, geom, penalty, augment_max, gap_tolerance);
}

// the owned contact nodes in the caller's ids, ascending: (caller id, index into ContactState::h_node)
static std::vector<std::pair<int, int>> contact_order(const feahip_ctx *c)
{
  std::vector<std::pair<int, int>> order;
  if (c->contact.n == 0) return order;
  int n0, n1;
  contact_owned(c, n0, n1);
  for (int i = n0; i < n1; ++i) order.emplace_back(c->perm.empty() ? c->contact.h_node[i] : c->iperm[c->contact.h_node[i]], i);
  std::sort(order.begin(), order.end());
  return order;
}

extern "C" int feahip_get_contact_nodes(feahip_ctx *c, int *n, int *nodes, double *weights)
{
  if (!c || !n) return FEAHIP_EINVAL;
  const auto order = contact_order(c);
  *n = (int)order.size();
  for (size_t k = 0; k < order.size(); ++k) {
    if (nodes) nodes[k] = order[k].first;
    if (weights) weights[k] = c->contact.h_w[order[k].second];
  }
  return FEAHIP_OK;
}

extern "C" int feahip_get_contact_obstacles(feahip_ctx *c, int *n_obstacles)
{
  if (!c || !n_obstacles) return FEAHIP_EINVAL;
  *n_obstacles = c->contact.nobs;
  return FEAHIP_OK;
}

extern "C" int feahip_get_contact_multipliers(feahip_ctx *c, double *mu)
{
  CTX_GUARD_NOK(c);
  if (!mu) return FEAHIP_EINVAL;
  const ContactState &S = c->contact;
  if (S.n == 0) return FEAHIP_OK;
  std::vector<double> all((size_t)S.n * S.nobs);
  FEA_HIP_CHECK(c, hipMemcpyAsync(all.data(), S.d_mu, sizeof(double) * all.size(), hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  const auto order = contact_order(c);
  for (size_t k = 0; k < order.size(); ++k)
    std::copy(all.begin() + (size_t)order[k].second * S.nobs, all.begin() + (size_t)(order[k].second + 1) * S.nobs, mu + k * S.nobs);
  return FEAHIP_OK;
}

extern "C" int feahip_set_contact_multipliers(feahip_ctx *c, const double *mu)
{
  CTX_GUARD_NOK(c);
  if (!mu) return FEAHIP_EINVAL;
  const ContactState &S = c->contact;
  if (S.n == 0) return FEAHIP_OK;
  const auto order = contact_order(c);
  for (size_t k = 0; k < order.size() * S.nobs; ++k)
    if (!(mu[k] >= 0.0)) { c->err = "feahip_set_contact_multipliers: multiplier " + std::to_string(k) + " is negative or not a number"; return FEAHIP_EINVAL; }
  std::vector<double> all((size_t)S.n * S.nobs);          // the rows of other ranks keep what they hold
  FEA_HIP_CHECK(c, hipMemcpyAsync(all.data(), S.d_mu, sizeof(double) * all.size(), hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < order.size(); ++k)
    std::copy(mu + k * S.nobs, mu + (k + 1) * S.nobs, all.begin() + (size_t)order[k].second * S.nobs);
  FEA_HIP_CHECK(c, hipMemcpyAsync(S.d_mu, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

extern "C" int feahip_get_contact_forces(feahip_ctx *c, double *f)
{
  CTX_GUARD_NOK(c);
  if (!f) return FEAHIP_EINVAL;
  DevTemp d;
  int rc;
  if ((rc = d.alloc(c, (size_t)c->ndof, true)) || (rc = launch_contact(c, false, true, d.p))) return rc;
  return get_view(c, d.p, f, 3, 3);
}

extern "C" int feahip_get_contact_status(feahip_ctx *c, double *gap, double *pressure)
{
  CTX_GUARD_NOK(c);
  const size_t N = (size_t)c->N;
  std::vector<double> h(2 * N, 0.0);                                 // where no contact node is: gap +inf, pressure 0
  std::fill(h.begin(), h.begin() + N, std::numeric_limits<double>::infinity());
  DevTemp d;
  int rc;
  if ((rc = d.alloc(c, 2 * N))) return rc;
  if (hipMemcpyAsync(d.p, h.data(), sizeof(double) * 2 * N, hipMemcpyHostToDevice, c->stream) != hipSuccess) return FEAHIP_EHIP;
  if ((rc = launch_contact_status(c, d.p, d.p + N))) return rc;
  if (gap && (rc = get_view(c, d.p, gap, 1, 1))) return rc;
  if (pressure && (rc = get_view(c, d.p + N, pressure, 1, 1))) return rc;
  return FEAHIP_OK;
}

extern "C" int feahip_contact_info(feahip_ctx *c, double *out)
{
  CTX_GUARD_NOK(c);
  if (!out) return FEAHIP_EINVAL;
  std::vector<feahip_ctx *> R = ranks_of(c);
  return surface_error(c, R, dist_contact_info(R, out));
}

extern "C" int feahip_contact_augment(feahip_ctx *c, double *max_penetration)
{
  CTX_GUARD_NOK(c);
  std::vector<feahip_ctx *> R = ranks_of(c);
  return surface_error(c, R, dist_contact_augment(R, max_penetration));
}

// ---- material table (include/fea_hip.h).  Validated in full before anything of the context changes.
extern "C" int feahip_set_materials(feahip_ctx *c, int n_materials, const double *params, const int *elem_material)
{
  CTX_GUARD_NOK(c);
  auto refuse = [c](std::string why) { c->err = "feahip_set_materials: " + std::move(why); return FEAHIP_EINVAL; };
  if (n_materials < 0) return refuse("negative material count");
  if (n_materials > FEAHIP_MAX_MATERIALS)
    return refuse(std::to_string(n_materials) + " materials, at most " + std::to_string(FEAHIP_MAX_MATERIALS));
  std::vector<uint8_t> ids;
  if (n_materials > 0) {
    if (!params || !elem_material) return refuse("null array with " + std::to_string(n_materials) + " materials");
    for (int i = 0; i < 2 * n_materials; ++i)
      if (!std::isfinite(params[i]))
        return refuse(std::string(i & 1 ? "mu" : "lambda") + " of material " + std::to_string(i / 2) + " is not finite");
    // the caller's element order: the whole mesh's on a feahip_create_rank context (its own entries are kept)
    const bool whole = c->rank_own >= 0 && !c->rank_local_ids;
    const int ne = whole ? c->rank_e_global : c->E;
    for (int e = 0; e < ne; ++e)
      if (elem_material[e] < 0 || elem_material[e] >= n_materials)
        return refuse("element " + std::to_string(e) + " has material " + std::to_string(elem_material[e]) + " outside [0," +
                      std::to_string(n_materials) + ")");
    ids.resize((size_t)c->E);
    for (int e = 0; e < c->E; ++e) ids[e] = (uint8_t)elem_material[whole ? c->rank_elem_global[e] : e];
  }
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));   // no assembly in flight reads the old table
  // the new table goes to the device first: a failed allocation or copy leaves the context with the old one
  double2 *d_mat = nullptr;
  uint8_t *d_elem_mat = nullptr;
  if (n_materials > 0) {
    int rc = dev_upload(c, &d_mat, reinterpret_cast<const double2 *>(params), (size_t)n_materials);
    if (!rc) rc = dev_upload(c, &d_elem_mat, ids.data(), ids.size());
    if (rc) { dev_free({d_mat, d_elem_mat}); return rc; }
  }
  dev_free({c->d_mat, c->d_elem_mat});
  c->d_mat = d_mat; c->d_elem_mat = d_elem_mat;
  // a mass with one density per material: a table of another size drops it (the next call that needs the mass says
  // so); the same size keeps the densities and m is assembled again with the new ids on next use
  if (c->mass.set && c->mass.n_rho > 1) {
    if (n_materials != c->mass.n_mat) c->mass.stale = true;
    c->mass.release_m();
    c->mass.release_lump();
  }
  c->n_materials = n_materials;
  c->h_mat_params.assign(params, params + (n_materials ? 2 * (size_t)n_materials : 0));
  c->h_elem_mat.swap(ids);
  c->state_valid = false;
  // the 4-node gather maps carry the ids (GatherLayout::o_emat): whatever was built or declined for this shard is built
  // again by the next assembly that asks.  No other maps know the materials.
  c->gather.release();
  return FEAHIP_OK;
}

extern "C" int feahip_get_materials(feahip_ctx *c, int *n_materials, double *params, int *elem_material)
{
  CTX_GUARD_NOK(c);
  if (!n_materials) { c->err = "feahip_get_materials: null count"; return FEAHIP_EINVAL; }
  *n_materials = c->n_materials;
  if (params) std::copy(c->h_mat_params.begin(), c->h_mat_params.end(), params);
  if (elem_material) std::copy(c->h_elem_mat.begin(), c->h_elem_mat.end(), elem_material);
  return FEAHIP_OK;
}

extern "C" int feahip_host_surface_faces(int n_nodes, int n_elems, int npe, const int *elements, int n_faces,
                                         int nodes_per_face, const int *face_nodes, int *face_elem, int *face_local,
                                         int *bad)
{
  if (bad) *bad = -1;
  if (!elements || n_nodes <= 0 || n_elems <= 0 || n_faces < 0 || (n_faces > 0 && (!face_nodes || !face_elem || !face_local)))
    return FEAHIP_EINVAL;
  for (long long i = 0; i < (long long)n_elems * npe; ++i)
    if (elements[i] < 0 || elements[i] >= n_nodes) return FEAHIP_EINVAL;
  if (n_faces == 0) return FEAHIP_OK;
  std::string why;
  const int b = resolve_surface_faces(n_nodes, n_elems, npe, elements, n_faces, nodes_per_face, face_nodes, face_elem, face_local, why);
  if (b < 0) return FEAHIP_OK;
  if (bad) *bad = b;
  return FEAHIP_EINVAL;
}

// ---- sharding ------------------------------------------------------------

static void drop_transport(feahip_ctx *c)
{
  if (c->tr && c->owns_tr) delete c->tr;
  c->tr = nullptr; c->owns_tr = false;
}

extern "C" int feahip_comm_unique_id(void *out, int cap) { return rccl_unique_id(out, cap); }

extern "C" int feahip_comm_init(feahip_ctx *c, int rank, int nranks, const void *unique_id)
{
  CTX_GUARD_NOK(c);
  if (!unique_id) return FEAHIP_EINVAL;
  int rc = install_shard(c, rank, nranks);
  if (rc) return rc;
  drop_transport(c);
  c->tr = make_rccl_transport(c, rank, nranks, unique_id, c->err);
  if (!c->tr) return FEAHIP_ECOMM;
  c->owns_tr = true;
  return FEAHIP_OK;
}

extern "C" int feahip_group_init(feahip_ctx **ctxs, int n)
{
  if (!ctxs || n < 1) return FEAHIP_EINVAL;
  Transport *t = make_group_transport();
  for (int r = 0; r < n; ++r) {
    if (!ctxs[r]) { delete t; return FEAHIP_EINVAL; }
    (void)hipSetDevice(ctxs[r]->device);
    int rc = install_shard(ctxs[r], r, n);
    if (rc) { delete t; return rc; }
    drop_transport(ctxs[r]);
    ctxs[r]->tr = t;
    ctxs[r]->owns_tr = (r == 0);
  }
  t->set_members(std::vector<feahip_ctx *>(ctxs, ctxs + n));
  return FEAHIP_OK;
}

static int group_vec(feahip_ctx **ctxs, int n, std::vector<feahip_ctx *> &R)
{
  if (!ctxs || n < 1) return FEAHIP_EINVAL;
  R.assign(ctxs, ctxs + n);
  for (int r = 0; r < n; ++r)
    if (!R[r] || R[r]->nranks != n || R[r]->rank != r || !R[r]->tr) {
      if (R[0]) R[0]->err = "not a group: call feahip_group_init on these contexts first";
      return FEAHIP_ESTATE;
    }
  return FEAHIP_OK;
}

extern "C" int feahip_group_solve_slae(feahip_ctx **ctxs, int n, int type, double tol, int max_iter, int *iters, double *resid)
{
  std::vector<feahip_ctx *> R;
  int rc = group_vec(ctxs, n, R);
  if (rc) return rc;
  return surface_error(R[0], R, dist_solve_pcg(R, type, tol, max_iter, iters, resid));
}

extern "C" int feahip_group_energy(feahip_ctx **ctxs, int n, double *tolerance)
{
  std::vector<feahip_ctx *> R;
  int rc = group_vec(ctxs, n, R);
  if (rc) return rc;
  return surface_error(R[0], R, dist_energy(R, tolerance));
}

extern "C" int feahip_group_update_nodes_with_solution(feahip_ctx **ctxs, int n)
{
  std::vector<feahip_ctx *> R;
  int rc = group_vec(ctxs, n, R);
  if (rc) return rc;
  return surface_error(R[0], R, dist_update_nodes_with_solution(R, nullptr));
}

extern "C" int feahip_group_solve(feahip_ctx **ctxs, int n, int load_increments, int max_newton, int modified_newton,
                                  double desired_tolerance, int solver_type, double solver_tolerance,
                                  int solver_max_iter, double *tol_log, int tol_log_cap, int *its_log, int *steps_done)
{
  std::vector<feahip_ctx *> R;
  int rc = group_vec(ctxs, n, R);
  if (rc) return rc;
  return surface_error(R[0], R, dist_newton(R, load_increments, max_newton, modified_newton, desired_tolerance, solver_type,
                                            solver_tolerance, solver_max_iter, tol_log, tol_log_cap, its_log, steps_done));
}

extern "C" int feahip_owned_rows(feahip_ctx *c, int *row0, int *row1)
{
  if (!c || !row0 || !row1) return FEAHIP_EINVAL;
  *row0 = c->row0; *row1 = c->row1;
  return FEAHIP_OK;
}

// Host-only: the halo plan of one rank, from the element->node map alone (no
// device is touched).  Lists are written into caller buffers sized by a first
// call with null lists: counts[0] = npeers, [1] = total send, [2] = total recv,
// [3] = row0, [4] = row1.
extern "C" int feahip_shard_plan(int n_nodes, int n_elems, int npe, const int *elements, int rank, int nranks,
                                 int *counts, int *peers, int *send_off, int *recv_off, int *send_idx, int *recv_idx)
{
  if (!elements || !counts || n_nodes <= 0 || n_elems <= 0 || nranks < 1 || rank < 0 || rank >= nranks) return FEAHIP_EINVAL;
  HostPattern hp;
  std::string err;
  int rc = build_host_pattern(n_nodes, n_elems, npe, elements, hp, err);
  if (rc) return rc;
  ShardPlan plan;
  build_shard_plan(hp.rowptr, hp.colidx, hp.chunk, rank, nranks, plan);
  counts[0] = (int)plan.peer.size(); counts[1] = (int)plan.send_idx.size(); counts[2] = (int)plan.recv_idx.size();
  counts[3] = plan.row0; counts[4] = plan.row1;
  if (peers) std::copy(plan.peer.begin(), plan.peer.end(), peers);
  if (send_off) std::copy(plan.send_off.begin(), plan.send_off.end(), send_off);
  if (recv_off) std::copy(plan.recv_off.begin(), plan.recv_off.end(), recv_off);
  if (send_idx) std::copy(plan.send_idx.begin(), plan.send_idx.end(), send_idx);
  if (recv_idx) std::copy(plan.recv_idx.begin(), plan.recv_idx.end(), recv_idx);
  return FEAHIP_OK;
}

extern "C" int feahip_host_numbering(int n_nodes, int n_elems, int npe, const int *elements, const double *nodes0, int *library_id_of_node)
{
  if (!elements || !nodes0 || !library_id_of_node || n_nodes <= 0 || n_elems <= 0 || (npe != 4 && npe != 8 && npe != 10)) return FEAHIP_EINVAL;
  for (long long i = 0; i < (long long)n_elems * npe; ++i)
    if (elements[i] < 0 || elements[i] >= n_nodes) return FEAHIP_EINVAL;
  std::vector<int> perm;
  const bool any = locality_numbering(n_nodes, n_elems, npe, elements, nodes0, perm);
  bool identity = true;
  for (int a = 0; a < n_nodes; ++a) { library_id_of_node[a] = perm[a]; identity = identity && perm[a] == a; }
  return any && !identity ? 1 : 0;
}

// ---- views ---------------------------------------------------------------

extern "C" int feahip_set_nodes(feahip_ctx *c, const double *nodes)
{
  CTX_GUARD_NOK(c);
  const int rc = set_view(c, c->d_x, nodes, 3, 4);
  if (rc == FEAHIP_OK) c->state_valid = false;
  return rc;
}

extern "C" int feahip_get_nodes(feahip_ctx *c, double *nodes) { CTX_GUARD_NOK(c); return get_view(c, c->d_x, nodes, 3, 4); }
extern "C" int feahip_get_forces(feahip_ctx *c, double *f) { CTX_GUARD(c); return get_view(c, c->d_f, f, 3, 3); }
extern "C" int feahip_get_solution(feahip_ctx *c, double *u) { CTX_GUARD(c); return get_view(c, c->d_u, u, 3, 3); }
extern "C" int feahip_set_forces(feahip_ctx *c, const double *f) { CTX_GUARD(c); return set_view(c, c->d_f, f, 3, 3); }

// ---- consistent mass, body force and implicit dynamics (kernels_mass.hip, drivers.hip) ----------------------------
extern "C" int feahip_set_mass(feahip_ctx *c, int n_rho, const double *rho, int mass_points, const double *weights,
                               const double *forms, const double *dforms)
{
  CTX_GUARD_NOK(c);
  if (n_rho < 0) { c->err = "feahip_set_mass: negative density count"; return FEAHIP_EINVAL; }
  return mass_set(c, n_rho, rho, mass_points, weights, forms, dforms);
}

extern "C" int feahip_set_body_force(feahip_ctx *c, const double *b)
{
  CTX_GUARD_NOK(c);
  return mass_set_body_force(c, b);
}

#define MASS_GUARD(c, who)                                         \
  CTX_GUARD_NOK(c);                                                \
  { const int _rm = mass_ensure(c, who); if (_rm) return _rm; }

// (the kinematic vectors are node records [N][4] that carry 3)
extern "C" int feahip_set_velocities(feahip_ctx *c, const double *v) { MASS_GUARD(c, "feahip_set_velocities"); c->mass.ke_parts = 0; return set_view(c, c->mass.d_vel, v, 3, 4); }
extern "C" int feahip_get_velocities(feahip_ctx *c, double *v) { MASS_GUARD(c, "feahip_get_velocities"); return get_view(c, c->mass.d_vel, v, 3, 4); }
extern "C" int feahip_set_accelerations(feahip_ctx *c, const double *a) { MASS_GUARD(c, "feahip_set_accelerations"); return set_view(c, c->mass.d_acc, a, 3, 4); }
extern "C" int feahip_get_accelerations(feahip_ctx *c, double *a) { MASS_GUARD(c, "feahip_get_accelerations"); return get_view(c, c->mass.d_acc, a, 3, 4); }

extern "C" int feahip_get_time(feahip_ctx *c, double *t)
{
  if (!c || !t) return FEAHIP_EINVAL;
  *t = c->mass.time;
  return FEAHIP_OK;
}

extern "C" int feahip_set_time(feahip_ctx *c, double t)
{
  if (!c) return FEAHIP_EINVAL;
  c->mass.time = t;
  return FEAHIP_OK;
}

extern "C" int feahip_mass_spmv(feahip_ctx *c, const double *x, double *y)
{
  MASS_GUARD(c, "feahip_mass_spmv");
  if (!x || !y) return FEAHIP_EINVAL;
  int rc;
  if ((rc = set_view(c, c->mass.d_xt, x, 3, 4))) return rc;        // (xt is free outside a step)
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d_q, 0, sizeof(double) * (size_t)c->ndof, c->stream));   // rows of other ranks: 0
  if ((rc = launch_mass_product(c, c->mass.d_xt, c->d_q))) return rc;
  return get_view(c, c->d_q, y, 3, 3);
}

// ---- Rayleigh damping C = alpha M + beta_k K_d (kernels_damping.hip) --------------------------------------------------
extern "C" int feahip_set_damping(feahip_ctx *c, double alpha, double beta_k)
{
  CTX_GUARD_NOK(c);
  return damping_set(c, alpha, beta_k);
}

extern "C" int feahip_get_damping(feahip_ctx *c, double *alpha, double *beta_k)
{
  if (!c || !alpha || !beta_k) return FEAHIP_EINVAL;
  *alpha = c->damping.alpha; *beta_k = c->damping.beta;
  return FEAHIP_OK;
}

extern "C" int feahip_damping_spmv(feahip_ctx *c, const double *v, double *y)
{
  CTX_GUARD(c);
  if (!v || !y) return FEAHIP_EINVAL;
  if (!c->damping.on()) { c->err = "feahip_damping_spmv: no damping on this context (feahip_set_damping)"; return FEAHIP_ESTATE; }
  int rc;
  if ((rc = damping_ready(c, "feahip_damping_spmv"))) return rc;
  DevTemp v4;                                                      // (a context with beta_k alone may have no mass vectors)
  if ((rc = v4.alloc(c, 4 * (size_t)c->N)) || (rc = set_view(c, v4.p, v, 3, 4))) return rc;
  if (hipMemsetAsync(c->d_q, 0, sizeof(double) * (size_t)c->ndof, c->stream) != hipSuccess) return FEAHIP_EHIP;   // rows of other ranks: 0
  if ((rc = launch_damp_product(c, v4.p, c->d_q))) return rc;
  return get_view(c, c->d_q, y, 3, 3);                             // (synchronises)
}

extern "C" int feahip_host_rayleigh(double omega1, double zeta1, double omega2, double zeta2, double *alpha, double *beta_k)
{
  if (!alpha || !beta_k) return FEAHIP_EINVAL;
  if (!(omega1 > 0.0) || !(omega2 > 0.0) || !std::isfinite(omega1) || !std::isfinite(omega2) || omega1 == omega2) return FEAHIP_EINVAL;
  const double den = omega2 * omega2 - omega1 * omega1;
  *alpha = 2.0 * omega1 * omega2 * (zeta1 * omega2 - zeta2 * omega1) / den;
  *beta_k = 2.0 * (zeta2 * omega2 - zeta1 * omega1) / den;
  return FEAHIP_OK;
}

extern "C" int feahip_consistent_acceleration(feahip_ctx *c, int solver_type, double tol, int max_iter)
{
  CTX_GUARD(c);
  if (solver_type < FEAHIP_CG || solver_type > FEAHIP_CHOLESKY) { c->err = "unknown solver type"; return FEAHIP_EINVAL; }
  if (max_iter <= 0) { c->err = "max_iterations must be positive"; return FEAHIP_EINVAL; }
  std::vector<feahip_ctx *> R = ranks_of(c);
  return surface_error(c, R, dist_consistent_acceleration(R, solver_type, tol, max_iter));
}

static int dynamic_args(feahip_ctx *c, int n_steps, double dt, double beta, double gamma, int max_newton, int solver_type,
                        int solver_max_iter, int *steps_done)
{
  if (steps_done) *steps_done = 0;
  if (!(dt > 0.0) || !std::isfinite(dt)) { c->err = "solve_dynamic: dt must be positive"; return FEAHIP_EINVAL; }
  if (!(beta > 0.0) || !std::isfinite(beta)) { c->err = "solve_dynamic: beta must be positive"; return FEAHIP_EINVAL; }
  if (!(gamma >= 0.0) || !std::isfinite(gamma)) { c->err = "solve_dynamic: gamma must not be negative"; return FEAHIP_EINVAL; }
  if (n_steps < 0 || max_newton <= 0 || solver_max_iter <= 0) { c->err = "solve_dynamic: n_steps >= 0, max_newton and solver_max_iter positive"; return FEAHIP_EINVAL; }
  if (solver_type < FEAHIP_CG || solver_type > FEAHIP_CHOLESKY) { c->err = "unknown solver type"; return FEAHIP_EINVAL; }
  return FEAHIP_OK;
}

extern "C" int feahip_solve_dynamic(feahip_ctx *c, int n_steps, double dt, double beta, double gamma, double dlambda,
                                    int max_newton, double desired_tolerance, int solver_type, double solver_tolerance,
                                    int solver_max_iter, double *tol_log, int tol_log_cap, int *its_log, int *steps_done)
{
  CTX_GUARD(c);
  int rc;
  if ((rc = dynamic_args(c, n_steps, dt, beta, gamma, max_newton, solver_type, solver_max_iter, steps_done))) return rc;
  std::vector<feahip_ctx *> R(1, c);
  return dist_dynamic(R, n_steps, dt, beta, gamma, dlambda, max_newton, desired_tolerance, solver_type, solver_tolerance,
                      solver_max_iter, tol_log, tol_log_cap, its_log, steps_done);
}

extern "C" int feahip_group_solve_dynamic(feahip_ctx **ctxs, int n, int n_steps, double dt, double beta, double gamma,
                                          double dlambda, int max_newton, double desired_tolerance, int solver_type,
                                          double solver_tolerance, int solver_max_iter, double *tol_log, int tol_log_cap,
                                          int *its_log, int *steps_done)
{
  std::vector<feahip_ctx *> R;
  int rc = group_vec(ctxs, n, R);
  if (rc) return rc;
  if ((rc = dynamic_args(R[0], n_steps, dt, beta, gamma, max_newton, solver_type, solver_max_iter, steps_done))) return rc;
  for (feahip_ctx *c : R) { CTX_GUARD(c); }
  rc = dist_dynamic(R, n_steps, dt, beta, gamma, dlambda, max_newton, desired_tolerance, solver_type, solver_tolerance,
                    solver_max_iter, tol_log, tol_log_cap, its_log, steps_done);
  return surface_error(R[0], R, rc);
}

// ---- explicit dynamics on the lumped mass (kernels_mass.hip, kernels_solve.hip, drivers.hip) ------------------------
extern "C" int feahip_get_lumped_mass(feahip_ctx *c, double *ml)
{
  CTX_GUARD_NOK(c);
  if (!ml) return FEAHIP_EINVAL;
  int rc;
  if ((rc = lump_ensure(c, "feahip_get_lumped_mass"))) return rc;
  return get_view(c, c->mass.d_ml, ml, 1, 1);
}

extern "C" int feahip_stable_step(feahip_ctx *c, double *dt_crit)
{
  CTX_GUARD(c);
  if (!dt_crit) return FEAHIP_EINVAL;
  std::vector<feahip_ctx *> R = ranks_of(c);
  return surface_error(c, R, dist_stable_step(R, dt_crit));
}

extern "C" int feahip_kinetic_energy(feahip_ctx *c, double *e)
{
  CTX_GUARD_NOK(c);
  if (!e) return FEAHIP_EINVAL;
  std::vector<feahip_ctx *> R = ranks_of(c);
  return surface_error(c, R, dist_kinetic_energy(R, e));
}

static int explicit_args(feahip_ctx *c, int n_steps, double dt, double safety, int *steps_done)
{
  if (steps_done) *steps_done = 0;
  if (!(dt >= 0.0) || !std::isfinite(dt)) { c->err = "solve_explicit: dt must not be negative (0 asks for the stable-step estimate)"; return FEAHIP_EINVAL; }
  if (n_steps < 0) { c->err = "solve_explicit: n_steps must not be negative"; return FEAHIP_EINVAL; }
  if (dt == 0.0 && !(safety > 0.0 && safety <= 1.0)) { c->err = "solve_explicit: safety must be in (0, 1]"; return FEAHIP_EINVAL; }
  return FEAHIP_OK;
}

extern "C" int feahip_solve_explicit(feahip_ctx *c, int n_steps, double dt, double safety, int restep, double dlambda,
                                     double *dt_log, int dt_log_cap, int *steps_done)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = explicit_args(c, n_steps, dt, safety, steps_done))) return rc;
  std::vector<feahip_ctx *> R(1, c);
  return dist_explicit(R, n_steps, dt, safety, restep, dlambda, dt_log, dt_log_cap, steps_done);
}

extern "C" int feahip_group_solve_explicit(feahip_ctx **ctxs, int n, int n_steps, double dt, double safety, int restep,
                                           double dlambda, double *dt_log, int dt_log_cap, int *steps_done)
{
  std::vector<feahip_ctx *> R;
  int rc = group_vec(ctxs, n, R);
  if (rc) return rc;
  if ((rc = explicit_args(R[0], n_steps, dt, safety, steps_done))) return rc;
  for (feahip_ctx *c : R) { CTX_GUARD_NOK(c); }
  rc = dist_explicit(R, n_steps, dt, safety, restep, dlambda, dt_log, dt_log_cap, steps_done);
  return surface_error(R[0], R, rc);
}

// ---- results: nodal stress, strain energy, reactions (kernels_results.hip) ------------------------------------------
static int results_material(feahip_ctx *c, int material, const char *who)
{
  if (material == -1) return FEAHIP_OK;
  if (material < -1 || material >= c->n_materials) {
    c->err = std::string(who) + ": material " + std::to_string(material) +
             (c->n_materials ? " outside the table of " + std::to_string(c->n_materials) : " on a context without a material table");
    return FEAHIP_EINVAL;
  }
  return FEAHIP_OK;
}

extern "C" int feahip_get_nodal_stresses(feahip_ctx *c, int material, double *sig6, double *von_mises, double *weight)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = results_material(c, material, "feahip_get_nodal_stresses"))) return rc;
  if ((rc = launch_results(c, material, nullptr))) return rc;
  if (sig6 && (rc = get_view(c, c->results.d_sig6, sig6, 6, 6))) return rc;
  if (von_mises && (rc = get_view(c, c->results.d_vm, von_mises, 1, 1))) return rc;
  if (weight && (rc = get_view(c, c->results.d_wt, weight, 1, 1))) return rc;
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return FEAHIP_OK;
}

extern "C" int feahip_get_nodal_energy(feahip_ctx *c, double *w_node)
{
  CTX_GUARD_NOK(c);
  if (!w_node) return FEAHIP_EINVAL;
  int rc;
  if ((rc = launch_results(c, -1, nullptr))) return rc;
  return get_view(c, c->results.d_wn, w_node, 1, 1);
}

extern "C" int feahip_strain_energy(feahip_ctx *c, double *W)
{
  CTX_GUARD_NOK(c);
  if (!W) return FEAHIP_EINVAL;
  std::vector<feahip_ctx *> R = ranks_of(c);
  return surface_error(c, R, dist_strain_energy(R, W));
}

extern "C" int feahip_get_reactions(feahip_ctx *c, double *r)
{
  CTX_GUARD(c);
  if (!r) return FEAHIP_EINVAL;
  DevTemp d;
  int rc;
  if ((rc = d.alloc(c, 2 * (size_t)c->ndof)) || (rc = launch_reactions(c, d.p, d.p + c->ndof))) return rc;
  return get_view(c, d.p, r, 3, 3);
}

// ---- modal analysis (kernels_modal.hip) --------------------------------------
static int modal_ready(feahip_ctx *c, const char *who)
{
  int rc;
  if ((rc = solve2_refused(c, who))) return rc;
  return mass_ensure(c, who);
}

// what the four eigenvalue entries ask of their arguments: `who` the entry, `limit` the modes it can hold, `out` its
// required output array (a shift is an argument of solve_modes_locked alone)
static int eigen_args(feahip_ctx *c, const char *who, int n_modes, int limit, double tol, int max_iter, const void *out,
                      const char *out_name, double shift = 0.0)
{
  auto refuse = [c, who](const std::string &why) { c->err = std::string(who) + ": " + why; return FEAHIP_EINVAL; };
  if (n_modes < 1 || n_modes > limit) return refuse("n_modes must be in [1, " + std::to_string(limit) + "]");
  if (!(shift >= 0.0) || !std::isfinite(shift)) return refuse("shift must be finite and not negative");
  if (!(tol > 0.0) || !std::isfinite(tol)) return refuse("tolerance must be positive");
  if (max_iter < 0) return refuse("max_iterations must not be negative");
  if (!out) return refuse(std::string("null ") + out_name);
  return FEAHIP_OK;
}

// modes [first, first + count) as `get` hands them over ([3N] on the host, library ids) into phi in the caller's order
template <class Get>
static int modes_to_caller(feahip_ctx *c, const NodeView &v, int first, int count, double *phi, Get get)
{
  std::vector<double> tmp((size_t)c->ndof);
  for (int k = 0; k < count; ++k) {
    const int rc = get(c, first + k, tmp.data());
    if (rc) return rc;
    to_caller(v, 3, 3, tmp.data(), phi + (size_t)k * c->ndof);
  }
  return FEAHIP_OK;
}

extern "C" int feahip_solve_modes(feahip_ctx *c, int n_modes, double tol, int max_iter, int warm, double *lambda,
                                  double *resid, int *iters)
{
  CTX_GUARD(c);
  if (iters) *iters = 0;
  int rc;
  if ((rc = eigen_args(c, "solve_modes", n_modes, FEA_MODAL_COLS, tol, max_iter, lambda, "lambda"))) return rc;
  if ((rc = modal_ready(c, "solve_modes"))) return rc;
  return modal_solve(c, n_modes, tol, max_iter, warm, lambda, resid, iters);
}

extern "C" int feahip_get_modes(feahip_ctx *c, int first, int count, double *phi)
{
  CTX_GUARD_NOK(c);
  if (!c->modal.have && !c->modal.have_sharded) { c->err = "get_modes: no modes held (feahip_solve_modes first)"; return FEAHIP_ESTATE; }
  if (first < 0 || count < 0 || first + count > FEA_MODAL_COLS) { c->err = "get_modes: modes [first, first + count) outside the eight held"; return FEAHIP_EINVAL; }
  if (!phi) { c->err = "get_modes: null phi"; return FEAHIP_EINVAL; }
  return modes_to_caller(c, view_of(c, c->modal.have_sharded), first, count, phi, modal_get);   // a sharded solve: the rank's own rows
}

extern "C" int feahip_spmm_km(feahip_ctx *c, const double *x8, double *y8, double *z8)
{
  CTX_GUARD(c);
  if (!x8 || !y8 || !z8) return FEAHIP_EINVAL;
  int rc;
  if ((rc = modal_ready(c, "spmm_km"))) return rc;
  if (!c->k_valid) { c->err = "spmm_km: no stiffness matrix assembled"; return FEAHIP_ESTATE; }
  if ((rc = ensure_modal(c))) return rc;
  c->modal.have = false;                                             // the block vectors are scratch here
  const size_t n8 = (size_t)c->ndof * FEA_MODAL_COLS;
  double *v = c->modal.d_v;                                          // X <- the host layout, KX, MX <- the products
  if ((rc = upload_columns(c, v, x8, 0, FEA_MODAL_COLS)) || (rc = launch_spmm_km(c, 0, c->nchunks_local, c->mass.d_m, v, v + 3 * n8, v + 6 * n8))) return rc;
  if ((rc = download_columns(c, v + 3 * n8, y8, FEA_MODAL_COLS))) return rc;
  return download_columns(c, v + 6 * n8, z8, FEA_MODAL_COLS);
}

// ---- the same solve over the ranks of a sharded run (modal_solve_dist, kernels_modal.hip) ------------------------------
extern "C" int feahip_solve_modes_sharded(feahip_ctx *c, int n_modes, double tol, int max_iter, int warm, double *lambda,
                                          double *resid, int *iters)
{
  CTX_GUARD(c);
  if (iters) *iters = 0;
  { const int rc = eigen_args(c, "solve_modes_sharded", n_modes, FEA_MODAL_COLS, tol, max_iter, lambda, "lambda"); if (rc) return rc; }
  if (!c->tr) {
    c->err = "solve_modes_sharded: the context has no transport (feahip_group_init, feahip_comm_init); feahip_solve_modes solves on one context";
    return FEAHIP_EINVAL;
  }
  std::vector<feahip_ctx *> R = ranks_of(c);
  for (feahip_ctx *r : R) { CTX_GUARD(r); }
  return surface_error(c, R, modal_solve_dist(R, n_modes, tol, max_iter, warm, lambda, resid, iters));
}

extern "C" int feahip_group_spmm_km(feahip_ctx **ctxs, int n, const double *const *x8, double *const *y8, double *const *z8)
{
  std::vector<feahip_ctx *> R;
  int rc = group_vec(ctxs, n, R);
  if (rc) return rc;
  if (!x8 || !y8 || !z8) return FEAHIP_EINVAL;
  for (int k = 0; k < n; ++k) {
    feahip_ctx *c = R[k];
    if (!x8[k] || !y8[k] || !z8[k]) return FEAHIP_EINVAL;
    CTX_GUARD(c);
    if ((rc = surface_error(R[0], R, mass_ensure(c, "group_spmm_km")))) return rc;
    if (!c->k_valid) { R[0]->err = c->err = "group_spmm_km: no stiffness matrix assembled"; return FEAHIP_ESTATE; }
    if ((rc = surface_error(R[0], R, ensure_modal_dist(c)))) return rc;
    c->modal.have = c->modal.have_sharded = false;                     // the block vectors are scratch here
    if ((rc = upload_columns(c, c->modal.d_v, x8[k], 0, FEA_MODAL_COLS))) return rc;   // X <- the host layout; KX, MX <- the products
  }
  if ((rc = surface_error(R[0], R, modal_spmm_km_dist(R)))) return rc;
  for (int k = 0; k < n; ++k) {
    feahip_ctx *c = R[k];
    FEA_HIP_CHECK(c, hipSetDevice(c->device));
    const size_t n8 = (size_t)c->ndof * FEA_MODAL_COLS;
    if ((rc = download_columns(c, c->modal.d_v + 3 * n8, y8[k], FEA_MODAL_COLS, true))) return rc;
    if ((rc = download_columns(c, c->modal.d_v + 6 * n8, z8[k], FEA_MODAL_COLS, true))) return rc;
  }
  return FEAHIP_OK;
}

extern "C" int feahip_solve_modes_locked(feahip_ctx *c, int n_modes, double shift, double tol, int max_iter, double *lambda,
                                         double *resid, int *iters, int *sweeps)
{
  CTX_GUARD(c);
  if (iters) *iters = 0;
  if (sweeps) *sweeps = 0;
  int rc;
  if ((rc = eigen_args(c, "solve_modes_locked", n_modes, FEA_MODAL_MAX_LOCKED, tol, max_iter, lambda, "lambda", shift))) return rc;
  if ((rc = modal_ready(c, "solve_modes_locked"))) return rc;
  return modal_solve_locked(c, n_modes, shift, tol, max_iter, lambda, resid, iters, sweeps);
}

extern "C" int feahip_get_locked_lambda(feahip_ctx *c, int first, int count, double *lambda)
{
  CTX_GUARD_NOK(c);
  if (!lambda) return FEAHIP_EINVAL;
  if (!c->modal.have_locked) { c->err = "get_locked_lambda: no locked modes held (feahip_solve_modes_locked first)"; return FEAHIP_ESTATE; }
  if (first < 0 || count < 0 || first + count > c->modal.n_locked) { c->err = "get_locked_lambda: range outside the modes held"; return FEAHIP_EINVAL; }
  for (int k = 0; k < count; ++k) lambda[k] = c->modal.lam[first + k];
  return FEAHIP_OK;
}

extern "C" int feahip_get_locked_count(feahip_ctx *c, int *count)
{
  CTX_GUARD_NOK(c);
  if (!count) return FEAHIP_EINVAL;
  if (!c->modal.have_locked) { c->err = "get_locked_count: no locked modes held (feahip_solve_modes_locked first)"; return FEAHIP_ESTATE; }
  *count = c->modal.n_locked;
  return FEAHIP_OK;
}

extern "C" int feahip_get_locked_modes(feahip_ctx *c, int first, int count, double *phi)
{
  CTX_GUARD_NOK(c);
  if (!c->modal.have_locked) { c->err = "get_locked_modes: no locked modes held (feahip_solve_modes_locked first)"; return FEAHIP_ESTATE; }
  if (first < 0 || count < 0 || first + count > c->modal.n_locked) {
    c->err = "get_locked_modes: modes [first, first + count) outside the " + std::to_string(c->modal.n_locked) + " locked";
    return FEAHIP_EINVAL;
  }
  if (!phi) { c->err = "get_locked_modes: null phi"; return FEAHIP_EINVAL; }
  return modes_to_caller(c, view_of(c), first, count, phi, modal_get_locked);
}

extern "C" int feahip_modal_deflate(feahip_ctx *c, int n_locked, const double *q, const double *x8, double *out8)
{
  CTX_GUARD(c);
  if (!q || !x8 || !out8) return FEAHIP_EINVAL;
  if (n_locked < 1 || n_locked > FEA_MODAL_MAX_LOCKED) { c->err = "modal_deflate: n_locked must be in [1, 64]"; return FEAHIP_EINVAL; }
  int rc;
  if ((rc = modal_ready(c, "modal_deflate"))) return rc;
  if (!c->k_valid) { c->err = "modal_deflate: no stiffness matrix assembled"; return FEAHIP_ESTATE; }
  if ((rc = ensure_modal(c)) || (rc = ensure_locked(c, n_locked))) return rc;
  c->modal.have = false;                                             // the block vectors and the store are scratch here
  const size_t n8 = (size_t)c->ndof * FEA_MODAL_COLS;
  double *v = c->modal.d_v;                                          // X <- a panel of q, MX <- mask(M X)
  for (int p = 0; p * FEA_MODAL_COLS < n_locked; ++p) {
    const int first = p * FEA_MODAL_COLS;
    if ((rc = upload_columns(c, v, q, first, std::min(FEA_MODAL_COLS, n_locked - first)))) return rc;
    if ((rc = launch_spmm_km(c, 0, c->nchunks_local, c->mass.d_m, v, v + 3 * n8, v + 6 * n8))) return rc;
    FEA_HIP_CHECK(c, hipMemcpyAsync(locked_panel(c, 0, p), v, sizeof(double) * n8, hipMemcpyDeviceToDevice, c->stream));
    FEA_HIP_CHECK(c, hipMemcpyAsync(locked_panel(c, 1, p), v + 6 * n8, sizeof(double) * n8, hipMemcpyDeviceToDevice, c->stream));
  }
  if ((rc = upload_columns(c, v, x8, 0, FEA_MODAL_COLS)) || (rc = launch_deflate(c, v, n_locked))) return rc;
  return download_columns(c, v, out8, FEA_MODAL_COLS);
}

// ---- frequency response by mode superposition on the locked store (kernels_response.hip) -------------------------------
extern "C" int feahip_response_set_basis(feahip_ctx *c, int n, const double *lam, const double *phi)
{
  CTX_GUARD(c);
  if (!lam || !phi) return FEAHIP_EINVAL;
  if (n < 1 || n > FEA_MODAL_MAX_LOCKED) { c->err = "response_set_basis: n must be in [1, 64]"; return FEAHIP_EINVAL; }
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(lam[k])) { c->err = "response_set_basis: lam is not finite"; return FEAHIP_EINVAL; }
  int rc;
  if ((rc = modal_ready(c, "response_set_basis")) || (rc = ensure_modal(c)) || (rc = ensure_locked(c, n))) return rc;
  ModalState &S = c->modal;
  S.have = false;                                                    // the block vectors are scratch here
  // The pairs go into the store by ascending lam (equal ones in the caller's order), column k the k-th of them: the sums of
  // the superposition kernels run in column order, so the order the caller lists the pairs in does not reach their bits
  int pick[FEA_MODAL_MAX_LOCKED];
  for (int k = 0; k < n; ++k) pick[k] = k;
  std::stable_sort(pick, pick + n, [&](int x, int y) { return lam[x] < lam[y]; });
  double *v = S.d_v;                                                 // X <- a panel, zero on the prescribed dofs
  for (int p = 0; p * FEA_MODAL_COLS < n; ++p) {
    const int first = p * FEA_MODAL_COLS;
    if ((rc = upload_columns(c, v, phi, first, std::min(FEA_MODAL_COLS, n - first), pick)) || (rc = launch_response_mask8(c, v))) return rc;
    FEA_HIP_CHECK(c, hipMemcpyAsync(locked_panel(c, 0, p), v, sizeof(double) * (size_t)c->ndof * FEA_MODAL_COLS, hipMemcpyDeviceToDevice, c->stream));
  }
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < n; ++k) { S.lock_order[k] = k; S.lam[k] = lam[pick[k]]; }
  S.shift = 0.0;
  S.n_locked = n;
  ++S.lock_gen;
  S.have_locked = true;
  return FEAHIP_OK;
}

static int modes_held(feahip_ctx *c, const char *who)
{
  if (c->modal.have_locked) return FEAHIP_OK;
  c->err = std::string(who) + ": no modes held (feahip_solve_modes_locked or feahip_response_set_basis first)";
  return FEAHIP_ESTATE;
}

// the load held belongs to the modes held
static int response_loaded(feahip_ctx *c, const char *who)
{
  if (const int rc = modes_held(c, who)) return rc;
  if (!c->response.loaded || c->response.gen != c->modal.lock_gen) {
    c->err = std::string(who) + ": no load held for these modes (feahip_response_load first)";
    return FEAHIP_ESTATE;
  }
  return FEAHIP_OK;
}

// a load with the static correction: K u_s = F needs a solver and modes of a K that is not singular
static int static_correction_args(feahip_ctx *c, const std::string &who, int solver_type, int max_iterations)
{
  const ModalState &S = c->modal;
  if (solver_type < FEAHIP_CG || solver_type > FEAHIP_CHOLESKY) { c->err = who + ": unknown solver type"; return FEAHIP_EINVAL; }
  if (max_iterations <= 0) { c->err = who + ": max_iterations must be positive"; return FEAHIP_EINVAL; }
  if (S.shift > 0.0) { c->err = who + ": the modes come from a solve with a shift, a body whose K may be singular: no static correction"; return FEAHIP_EINVAL; }
  for (int k = 0; k < S.n_locked; ++k)
    if (!(S.lam[k] > 0.0)) { c->err = who + ": lam of mode " + std::to_string(k + 1) + " is not positive: no static correction"; return FEAHIP_EINVAL; }
  return FEAHIP_OK;
}

// the ranges of a sweep's n_freq and of a history's n_steps
static int sweep_args(feahip_ctx *c, const char *who, int n_freq)
{
  if (n_freq >= 1 && n_freq <= FEA_RESPONSE_MAX_FREQ) return FEAHIP_OK;
  c->err = std::string(who) + ": n_freq must be in [1, 4096]";
  return FEAHIP_EINVAL;
}

static int history_args(feahip_ctx *c, const char *who, int n_steps)
{
  if (n_steps >= 1 && n_steps <= FEA_TRANSIENT_MAX_STEPS) return FEAHIP_OK;
  c->err = std::string(who) + ": n_steps must be in [1, 1048576]";
  return FEAHIP_EINVAL;
}

// at most 64 probes, and none of their arrays null where there are any
template <class... A>
static int probe_args(feahip_ctx *c, const char *who, int n_probe, const A *...arrays)
{
  if (n_probe < 0 || n_probe > 64) { c->err = std::string(who) + ": n_probe must be in [0, 64]"; return FEAHIP_EINVAL; }
  if (n_probe > 0 && (... || !arrays)) { c->err = std::string(who) + ": null probe arrays"; return FEAHIP_EINVAL; }
  return FEAHIP_OK;
}

// lib[r] = the library's dof of the caller's probe_dof[r], each inside [0, 3N)
static int probe_dofs(feahip_ctx *c, const char *who, int n_probe, const int *probe_dof, int *lib)
{
  for (int r = 0; r < n_probe; ++r) {
    if (probe_dof[r] < 0 || probe_dof[r] >= c->ndof) { c->err = std::string(who) + ": probe dof outside [0, 3N)"; return FEAHIP_EINVAL; }
    lib[r] = 3 * lib_id(c, probe_dof[r] / 3) + probe_dof[r] % 3;
  }
  return FEAHIP_OK;
}

// peak [3N] and peak_at [3N] from the library's order into the caller's
static void peaks_to_caller(feahip_ctx *c, const double *lib_peak, double *peak, const int *lib_at, int *peak_at)
{
  to_caller(view_of(c), 3, 3, lib_peak, peak);
  to_caller(view_of(c), 3, 3, lib_at, peak_at);
}

extern "C" int feahip_response_load(feahip_ctx *c, const double *F, int static_correction, int solver_type, double tolerance,
                                    int max_iterations, double *q, int *iters, double *resid)
{
  CTX_GUARD(c);
  if (iters) *iters = 0;
  if (resid) *resid = 0.0;
  if (!F) { c->err = "response_load: null F"; return FEAHIP_EINVAL; }
  int rc;
  if ((rc = modal_ready(c, "response_load")) || (rc = modes_held(c, "response_load"))) return rc;
  if (static_correction && (rc = static_correction_args(c, "response_load", solver_type, max_iterations))) return rc;
  for (int i = 0; i < c->ndof; ++i)
    if (!std::isfinite(F[i])) { c->err = "response_load: F is not finite"; return FEAHIP_EINVAL; }
  std::vector<double> tmp((size_t)c->ndof);
  to_library(view_of(c), 3, 3, F, tmp.data());
  return response_load(c, tmp.data(), static_correction, solver_type, tolerance, max_iterations, q, iters, resid);
}

extern "C" int feahip_get_response_static(feahip_ctx *c, double *u_s)
{
  CTX_GUARD_NOK(c);
  if (!u_s) return FEAHIP_EINVAL;
  const int rc = response_loaded(c, "get_response_static");
  return rc ? rc : get_view(c, c->response.d_us, u_s, 3, 3);
}

extern "C" int feahip_response_sweep(feahip_ctx *c, int n_freq, const double *omega, double alpha, double beta_k,
                                     const double *zeta, double *peak, int *peak_at, int n_probe, const int *probe_dof,
                                     double *probe_re, double *probe_im)
{
  CTX_GUARD_NOK(c);
  if (!omega || !peak || !peak_at) { c->err = "response_sweep: null omega, peak or peak_at"; return FEAHIP_EINVAL; }
  int rc;
  int probe[64];
  if ((rc = response_loaded(c, "response_sweep")) || (rc = sweep_args(c, "response_sweep", n_freq)) ||
      (rc = probe_args(c, "response_sweep", n_probe, probe_dof, probe_re, probe_im)) ||
      (rc = probe_dofs(c, "response_sweep", n_probe, probe_dof, probe))) return rc;
  std::vector<double> pk((size_t)c->ndof);
  std::vector<int> at((size_t)c->ndof);
  if ((rc = response_sweep(c, false, n_freq, omega, alpha, beta_k, zeta, pk.data(), at.data(), n_probe, probe, probe_re, probe_im))) return rc;
  peaks_to_caller(c, pk.data(), peak, at.data(), peak_at);
  return FEAHIP_OK;
}

extern "C" int feahip_response_field(feahip_ctx *c, double omega, double alpha, double beta_k, const double *zeta, double *re,
                                     double *im)
{
  CTX_GUARD_NOK(c);
  if (!re || !im) { c->err = "response_field: null re or im"; return FEAHIP_EINVAL; }
  int rc;
  if ((rc = response_loaded(c, "response_field"))) return rc;
  std::vector<double> a((size_t)c->ndof), b((size_t)c->ndof);
  if ((rc = response_sweep(c, true, 1, &omega, alpha, beta_k, zeta, a.data(), b.data(), 0, nullptr, nullptr, nullptr))) return rc;
  to_caller(view_of(c), 3, 3, a.data(), re);
  to_caller(view_of(c), 3, 3, b.data(), im);
  return FEAHIP_OK;
}

extern "C" int feahip_host_response_coefficients(int n_modes, const double *lam, const double *q, int n_freq, const double *omega,
                                                 double alpha, double beta_k, const double *zeta, int static_correction,
                                                 double *coef)
{
  return response_coefficients(n_modes, lam, q, nullptr, n_freq, omega, alpha, beta_k, zeta, static_correction, coef, nullptr);
}

// ---- transient response by mode superposition, base excitation (kernels_transient.hip, transient_table.cpp) -------------
extern "C" int feahip_response_base_load(feahip_ctx *c, const double *dir, int static_correction, int solver_type,
                                         double tolerance, int max_iterations, double *q, double *gamma, double *eff_mass,
                                         double *total_mass, int *iters, double *resid)
{
  CTX_GUARD(c);
  if (iters) *iters = 0;
  if (resid) *resid = 0.0;
  if (!dir) { c->err = "response_base_load: null dir"; return FEAHIP_EINVAL; }
  int rc;
  if ((rc = modal_ready(c, "response_base_load")) || (rc = modes_held(c, "response_base_load"))) return rc;
  if (static_correction && (rc = static_correction_args(c, "response_base_load", solver_type, max_iterations))) return rc;
  if (!std::isfinite(dir[0]) || !std::isfinite(dir[1]) || !std::isfinite(dir[2])) { c->err = "response_base_load: dir is not finite"; return FEAHIP_EINVAL; }
  if (dir[0] == 0.0 && dir[1] == 0.0 && dir[2] == 0.0) { c->err = "response_base_load: dir is zero"; return FEAHIP_EINVAL; }
  // r = dir on every node, the prescribed ones included, in the node layout (xt is free outside a step); y = M r
  std::vector<double> r4(4 * (size_t)c->N), mr((size_t)c->ndof);
  for (int i = 0; i < c->N; ++i) { r4[4 * (size_t)i] = dir[0]; r4[4 * (size_t)i + 1] = dir[1]; r4[4 * (size_t)i + 2] = dir[2]; r4[4 * (size_t)i + 3] = 0.0; }
  FEA_HIP_CHECK(c, hipMemcpyAsync(c->mass.d_xt, r4.data(), sizeof(double) * r4.size(), hipMemcpyHostToDevice, c->stream));
  FEA_HIP_CHECK(c, hipMemsetAsync(c->d_q, 0, sizeof(double) * (size_t)c->ndof, c->stream));
  if ((rc = launch_mass_product(c, c->mass.d_xt, c->d_q)) || (rc = launch_base_load(c, c->d_q, c->d_f))) return rc;
  FEA_HIP_CHECK(c, hipMemcpyAsync(mr.data(), c->d_q, sizeof(double) * mr.size(), hipMemcpyDeviceToHost, c->stream));
  FEA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  long double total = 0;                                             // r' M r, the dofs in the library's order
  for (int i = 0; i < c->ndof; ++i) total += (long double)dir[i % 3] * mr[i];
  double qs[FEA_MODAL_MAX_LOCKED];
  if ((rc = response_load(c, nullptr, static_correction, solver_type, tolerance, max_iterations, qs, iters, resid))) return rc;
  for (int k = 0; k < c->modal.n_locked; ++k) {
    if (q) q[k] = qs[k];
    if (gamma) gamma[k] = -qs[k];
    if (eff_mass) eff_mass[k] = qs[k] * qs[k];
  }
  if (total_mass) *total_mass = (double)total;
  return FEAHIP_OK;
}

extern "C" int feahip_response_transient(feahip_ctx *c, int n_steps, double dt, const double *g, double alpha, double beta_k,
                                         const double *zeta, int quantity, double *peak, int *peak_at, int n_probe,
                                         const int *probe_dof, double *probe, int n_snap, const int *snap_step, double *snap)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = solve2_refused(c, "response_transient")) || (rc = response_loaded(c, "response_transient"))) return rc;
  if (!g || !peak || !peak_at) { c->err = "response_transient: null g, peak or peak_at"; return FEAHIP_EINVAL; }
  if ((rc = history_args(c, "response_transient", n_steps)) || (rc = probe_args(c, "response_transient", n_probe, probe_dof, probe))) return rc;
  if (n_snap < 0 || n_snap > 4096) { c->err = "response_transient: n_snap must be in [0, 4096]"; return FEAHIP_EINVAL; }
  if (n_snap > 0 && (!snap_step || !snap)) { c->err = "response_transient: null snapshot arrays"; return FEAHIP_EINVAL; }
  int lib_probe[64];
  if ((rc = probe_dofs(c, "response_transient", n_probe, probe_dof, lib_probe))) return rc;
  for (int s = 0; s < n_snap; ++s)
    if (snap_step[s] < 0 || snap_step[s] > n_steps) { c->err = "response_transient: snapshot step outside [0, n_steps]"; return FEAHIP_EINVAL; }
  const size_t nd = (size_t)c->ndof;
  std::vector<double> pk(nd), fields((size_t)n_snap * nd);
  std::vector<int> at(nd);
  if ((rc = response_transient(c, n_steps, dt, g, alpha, beta_k, zeta, quantity, pk.data(), at.data(), n_probe, lib_probe, probe,
                               n_snap, snap_step, fields.data()))) return rc;
  peaks_to_caller(c, pk.data(), peak, at.data(), peak_at);
  for (int s = 0; s < n_snap; ++s) to_caller(view_of(c), 3, 3, fields.data() + (size_t)s * nd, snap + (size_t)s * nd);
  return FEAHIP_OK;
}

extern "C" int feahip_host_transient_coefficients(int n_modes, const double *lam, const double *q, int n_steps, double dt,
                                                  const double *g, double alpha, double beta_k, const double *zeta,
                                                  int static_correction, int quantity, double *coef)
{
  int rc;
  if (!coef) return FEAHIP_EINVAL;
  if ((rc = transient_check(n_modes, lam, q, n_steps, dt, g, alpha, beta_k, zeta, static_correction, quantity, nullptr))) return rc;
  TransientTable *T = transient_begin(n_modes, lam, q, nullptr, n_steps, dt, alpha, beta_k, zeta, static_correction, quantity);
  rc = transient_rows(T, g, n_steps + 1, coef, nullptr);
  transient_end(T);
  return rc;
}

// ---- response spectrum and random vibration: one quadratic form per dof (kernels_combine.hip, combine_table.cpp) ---------
static int combine_ready(feahip_ctx *c, const char *who)
{
  int rc;
  if ((rc = solve2_refused(c, who))) return rc;
  return response_loaded(c, who);
}

static int combine_to_caller(feahip_ctx *c, const double *C, const double *b, double s, bool absx, double *out)
{
  std::vector<double> tmp((size_t)c->ndof);
  const int rc = response_combine(c, C, b, s, absx, tmp.data());
  if (rc) return rc;
  to_caller(view_of(c), 3, 3, tmp.data(), out);
  return FEAHIP_OK;
}

// A caller's form (C[n][n], b[n] or null, s or null): finite, C symmetric to the bit, and finite still when an entry off
// the diagonal is doubled (folded_form).  The arrays are called C, b and s with `suffix` behind them, C in the symmetry
// text `sym`
static int form_args(feahip_ctx *c, const char *who, const char *suffix, const char *sym, int n, const double *C, const double *b,
                     const double *s)
{
  auto refuse = [&](const std::string &what) { c->err = std::string(who) + ": " + what; return FEAHIP_EINVAL; };
  const std::string x = suffix;
  for (int j = 0; j < n; ++j) {
    for (int k = 0; k < n; ++k) {
      const double v = C[(size_t)j * n + k];
      if (!std::isfinite(v)) return refuse("C" + x + " is not finite");
      if (std::memcmp(&v, &C[(size_t)k * n + j], sizeof(double))) return refuse(std::string(sym) + " is not symmetric to the bit");
      if (j != k && !std::isfinite(2.0 * v)) return refuse("twice an entry of C" + x + " is not finite");
    }
    if (b && !std::isfinite(b[j])) return refuse("b" + x + " is not finite");
  }
  if (s && !std::isfinite(*s)) return refuse("s" + x + " is not finite");
  return FEAHIP_OK;
}

// The form of random vibration on the modes and the load held (random_form), handed to emit(C, b, s, absx); the modal
// covariance to the caller, if asked for, once emit is through
template <class Emit>
static int random_on_held(feahip_ctx *c, const char *who, int n_freq, const double *omega, const double *S, double alpha,
                          double beta_k, const double *zeta, int quantity, double *modal_cov, Emit emit)
{
  const int n = c->modal.n_locked;
  std::vector<double> C((size_t)n * n), b(n);
  double s = 0.0;
  std::string why;
  if (random_form(n, c->modal.lam, c->response.q, n_freq, omega, S, alpha, beta_k, zeta, c->response.correction, quantity,
                  C.data(), b.data(), &s, &why)) {
    c->err = std::string(who) + ": " + why;
    return FEAHIP_EINVAL;
  }
  if (const int rc = emit(C.data(), b.data(), s, false)) return rc;
  if (modal_cov) std::copy(C.begin(), C.end(), modal_cov);
  return FEAHIP_OK;
}

// The same for a response spectrum (spectrum_form on the spectrum's value at every mode held) and the modal peaks.  The
// stress entry passes its peak_vm: FEAHIP_ABS takes magnitudes, and the von Mises form needs the signs
template <class Emit>
static int spectrum_on_held(feahip_ctx *c, const char *who, int n_pts, const double *w, const double *sa, int loglog, int rule,
                            double alpha, double beta_k, const double *zeta, double zpa, int quantity, const double *peak_vm,
                            double *modal_peak, Emit emit)
{
  auto refuse = [&](const std::string &what) { c->err = std::string(who) + ": " + what; return FEAHIP_EINVAL; };
  if (rule == FEAHIP_ABS && peak_vm) return refuse("no von Mises peak under FEAHIP_ABS (the differences need the signs): peak_vm must be NULL");
  const int n = c->modal.n_locked;
  double sak[FEA_MODAL_MAX_LOCKED], a[FEA_MODAL_MAX_LOCKED];
  for (int k = 0; k < n; ++k) {
    if (!(c->modal.lam[k] > 0.0)) return refuse("lam of mode " + std::to_string(k + 1) + " is not positive");
    sak[k] = feahip_host_spectrum_value(n_pts, w, sa, loglog, std::sqrt(c->modal.lam[k]));
    if (std::isnan(sak[k])) return refuse("the spectrum's points must be finite, their w strictly ascending");
  }
  std::vector<double> C((size_t)n * n), b(n);
  double s = 0.0;
  std::string why;
  if (spectrum_form(n, c->modal.lam, c->response.q, sak, alpha, beta_k, zeta, rule, c->response.correction, zpa, quantity,
                    C.data(), b.data(), &s, a, &why)) return refuse(why);
  if (const int rc = emit(C.data(), b.data(), s, rule == FEAHIP_ABS)) return rc;
  if (modal_peak) std::copy_n(a, n, modal_peak);
  return FEAHIP_OK;
}

extern "C" int feahip_response_combine(feahip_ctx *c, const double *C, const double *b, double s, int absolute, double *out)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = combine_ready(c, "response_combine"))) return rc;
  if (!C || !out) { c->err = "response_combine: null C or out"; return FEAHIP_EINVAL; }
  if ((rc = form_args(c, "response_combine", "", "C", c->modal.n_locked, C, b, &s))) return rc;
  return combine_to_caller(c, C, b, s, absolute != 0, out);
}

extern "C" int feahip_response_random(feahip_ctx *c, int n_freq, const double *omega, const double *S, double alpha, double beta_k,
                                      const double *zeta, int quantity, double *rms, double *modal_cov)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = combine_ready(c, "response_random"))) return rc;
  if (!omega || !S || !rms) { c->err = "response_random: null omega, S or rms"; return FEAHIP_EINVAL; }
  return random_on_held(c, "response_random", n_freq, omega, S, alpha, beta_k, zeta, quantity, modal_cov,
                        [&](const double *C, const double *b, double s, bool absx) { return combine_to_caller(c, C, b, s, absx, rms); });
}

extern "C" int feahip_response_spectrum(feahip_ctx *c, int n_pts, const double *w, const double *sa, int loglog, int rule,
                                        double alpha, double beta_k, const double *zeta, double zpa, int quantity, double *peak,
                                        double *modal_peak)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = combine_ready(c, "response_spectrum"))) return rc;
  if (!w || !sa || !peak) { c->err = "response_spectrum: null w, sa or peak"; return FEAHIP_EINVAL; }
  return spectrum_on_held(c, "response_spectrum", n_pts, w, sa, loglog, rule, alpha, beta_k, zeta, zpa, quantity, nullptr, modal_peak,
                          [&](const double *C, const double *b, double s, bool absx) { return combine_to_caller(c, C, b, s, absx, peak); });
}

// ---- stress from mode superposition (kernels_modal_stress.hip, kernels_stress_combine.hip) -----------------------------
extern "C" int feahip_stress_increment(feahip_ctx *c, const double *du, int material, double *sig6)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = solve2_refused(c, "stress_increment")) || (rc = results_material(c, material, "stress_increment"))) return rc;
  if (!du || !sig6) { c->err = "stress_increment: null du or sig6"; return FEAHIP_EINVAL; }
  for (int i = 0; i < c->ndof; ++i)
    if (!std::isfinite(du[i])) { c->err = "stress_increment: du is not finite"; return FEAHIP_EINVAL; }
  if ((rc = stress_ensure(c)) || (rc = set_view(c, c->stress.d_vec, du, 3, 3)) ||
      (rc = launch_stress_vector(c, c->stress.d_vec, material, c->stress.d_out6))) return rc;
  return get_view(c, c->stress.d_out6, sig6, 6, 6);
}

extern "C" int feahip_response_stress_basis(feahip_ctx *c, int material)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = solve2_refused(c, "response_stress_basis")) || (rc = modes_held(c, "response_stress_basis")) ||
      (rc = results_material(c, material, "response_stress_basis"))) return rc;
  return stress_basis(c, material);
}

// the stress store belongs to the modes held, and T_s to the last load made
static int stress_ready(feahip_ctx *c, const char *who)
{
  int rc;
  if ((rc = solve2_refused(c, who)) || (rc = modes_held(c, who))) return rc;
  const StressState &S = c->stress;
  if (!S.have || S.gen != c->modal.lock_gen) {
    c->err = std::string(who) + ": no stress store for these modes (feahip_response_stress_basis first)";
    return FEAHIP_ESTATE;
  }
  if (S.load_count != c->response.load_count) {
    c->err = std::string(who) + ": a load was made after the stress store (feahip_response_stress_basis again)";
    return FEAHIP_ESTATE;
  }
  return FEAHIP_OK;
}

extern "C" int feahip_get_modal_stresses(feahip_ctx *c, int first, int count, double *sig6)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_ready(c, "get_modal_stresses"))) return rc;
  if (first < 0 || count < 0 || first + count > c->modal.n_locked) {
    c->err = "get_modal_stresses: modes [first, first + count) outside the " + std::to_string(c->modal.n_locked) + " held";
    return FEAHIP_EINVAL;
  }
  if (!sig6) { c->err = "get_modal_stresses: null sig6"; return FEAHIP_EINVAL; }
  for (int j = 0; j < count; ++j)
    if ((rc = launch_stress_mode(c, c->modal.lock_order[first + j], c->stress.d_out6)) ||
        (rc = get_view(c, c->stress.d_out6, sig6 + (size_t)j * 6 * c->N, 6, 6))) return rc;
  return FEAHIP_OK;
}

extern "C" int feahip_get_response_static_stress(feahip_ctx *c, double *sig6)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_ready(c, "get_response_static_stress"))) return rc;
  if (!sig6) { c->err = "get_response_static_stress: null sig6"; return FEAHIP_EINVAL; }
  return get_view(c, c->stress.d_ts, sig6, 6, 6);
}

extern "C" int feahip_response_stress_field(feahip_ctx *c, const double *coef, double cs, double *sig6, double *vm)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_ready(c, "response_stress_field"))) return rc;
  if (!coef || !sig6 || !vm) { c->err = "response_stress_field: null coef, sig6 or vm"; return FEAHIP_EINVAL; }
  for (int k = 0; k < c->modal.n_locked; ++k)
    if (!std::isfinite(coef[k])) { c->err = "response_stress_field: coef is not finite"; return FEAHIP_EINVAL; }
  if (!std::isfinite(cs)) { c->err = "response_stress_field: cs is not finite"; return FEAHIP_EINVAL; }
  std::vector<double> t6(6 * (size_t)c->N), tv((size_t)c->N);
  if ((rc = stress_field(c, coef, cs, t6.data(), tv.data()))) return rc;
  to_caller(view_of(c), 6, 6, t6.data(), sig6);
  to_caller(view_of(c), 1, 1, tv.data(), vm);
  return FEAHIP_OK;
}

// the form entries need the load the store was made with as well
static int stress_form_ready(feahip_ctx *c, const char *who)
{
  int rc;
  if ((rc = solve2_refused(c, who)) || (rc = response_loaded(c, who))) return rc;
  return stress_ready(c, who);
}

static int stress_to_caller(feahip_ctx *c, const double *C, const double *b, double s, bool absx, double *out6, double *vm)
{
  std::vector<double> t6(6 * (size_t)c->N), tv((size_t)c->N);
  const int rc = stress_combine(c, C, b, s, absx, t6.data(), tv.data());
  if (rc) return rc;
  to_caller(view_of(c), 6, 6, t6.data(), out6);
  if (vm) to_caller(view_of(c), 1, 1, tv.data(), vm);
  return FEAHIP_OK;
}

extern "C" int feahip_response_stress_combine(feahip_ctx *c, const double *C, const double *b, double s, double *out6, double *vm)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_form_ready(c, "response_stress_combine"))) return rc;
  if (!C || !out6) { c->err = "response_stress_combine: null C or out6"; return FEAHIP_EINVAL; }
  if ((rc = form_args(c, "response_stress_combine", "", "C", c->modal.n_locked, C, b, &s))) return rc;
  return stress_to_caller(c, C, b, s, false, out6, vm);
}

extern "C" int feahip_response_stress_random(feahip_ctx *c, int n_freq, const double *omega, const double *S, double alpha,
                                             double beta_k, const double *zeta, double *rms6, double *rms_vm, double *modal_cov)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_form_ready(c, "response_stress_random"))) return rc;
  if (!omega || !S || !rms6) { c->err = "response_stress_random: null omega, S or rms6"; return FEAHIP_EINVAL; }
  return random_on_held(c, "response_stress_random", n_freq, omega, S, alpha, beta_k, zeta, 0, modal_cov,
                        [&](const double *C, const double *b, double s, bool absx) { return stress_to_caller(c, C, b, s, absx, rms6, rms_vm); });
}

extern "C" int feahip_response_stress_spectrum(feahip_ctx *c, int n_pts, const double *w, const double *sa, int loglog, int rule,
                                               double alpha, double beta_k, const double *zeta, double zpa, double *peak6,
                                               double *peak_vm, double *modal_peak)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_form_ready(c, "response_stress_spectrum"))) return rc;
  if (!w || !sa || !peak6) { c->err = "response_stress_spectrum: null w, sa or peak6"; return FEAHIP_EINVAL; }
  return spectrum_on_held(c, "response_stress_spectrum", n_pts, w, sa, loglog, rule, alpha, beta_k, zeta, zpa, 0, peak_vm, modal_peak,
                          [&](const double *C, const double *b, double s, bool absx) { return stress_to_caller(c, C, b, s, absx, peak6, peak_vm); });
}

// ---- random-vibration fatigue on the stress store (kernels_stress_fatigue.hip) ------------------------------------------
// lib[4][N][7] (library ids) into the caller's moments[N][7][4]
static void moments_to_caller(feahip_ctx *c, const double *lib, double *moments)
{
  const NodeView v = view_of(c);
  const size_t N = (size_t)c->N;
  for (int a = 0; a < c->N; ++a) {
    const size_t la = (size_t)v.lib(a);
    for (int k = 0; k < 7; ++k)
      for (int n = 0; n < 4; ++n) moments[((size_t)a * 7 + k) * 4 + n] = lib[(n * N + la) * 7 + k];
  }
}

extern "C" int feahip_response_stress_moments(feahip_ctx *c, const double *C4, const double *b4, const double *s4, double *moments)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_form_ready(c, "response_stress_moments"))) return rc;
  if (!C4 || !moments) { c->err = "response_stress_moments: null C4 or moments"; return FEAHIP_EINVAL; }
  const int n = c->modal.n_locked;
  for (int f = 0; f < 4; ++f)
    if ((rc = form_args(c, "response_stress_moments", "4", "a form of C4", n, C4 + (size_t)f * n * n, b4 ? b4 + (size_t)f * n : nullptr,
                        s4 ? s4 + f : nullptr))) return rc;
  std::vector<double> lib(28 * (size_t)c->N);
  if ((rc = stress_moments(c, C4, b4, s4, lib.data()))) return rc;
  moments_to_caller(c, lib.data(), moments);
  return FEAHIP_OK;
}

extern "C" int feahip_response_stress_fatigue(feahip_ctx *c, int n_freq, const double *omega, const double *S, double alpha,
                                              double beta_k, const double *zeta, double sn_b, double sn_a, double *moments,
                                              double *rates, double *damage, int *status)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_form_ready(c, "response_stress_fatigue"))) return rc;
  if (!omega || !S) { c->err = "response_stress_fatigue: null omega or S"; return FEAHIP_EINVAL; }
  double k[5];
  if (fatigue_constants(sn_b, sn_a, k)) {
    c->err = "response_stress_fatigue: the S-N curve N s^b = A needs a finite b in [1, 64] and a finite A > 0";
    return FEAHIP_EINVAL;
  }
  const int n = c->modal.n_locked;
  static const int order[4] = {0, 1, 2, 4};
  std::vector<double> C4(4 * (size_t)n * n), b4(4 * (size_t)n);
  double s4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int f = 0; f < 4; ++f) {
    std::string why;
    if (moment_form(n, c->modal.lam, c->response.q, n_freq, omega, S, alpha, beta_k, zeta, c->response.correction, order[f],
                    C4.data() + (size_t)f * n * n, b4.data() + (size_t)f * n, &s4[f], &why)) {
      c->err = "response_stress_fatigue: " + why;
      return FEAHIP_EINVAL;
    }
  }
  const size_t N = (size_t)c->N;
  std::vector<double> lm(moments ? 28 * N : 0), lr(rates ? 14 * N : 0), ld(damage ? 21 * N : 0);
  std::vector<int> ls(status ? 7 * N : 0);
  if ((rc = stress_moments(c, C4.data(), b4.data(), s4, moments ? lm.data() : nullptr)) ||
      (rc = stress_fatigue_rates(c, k, rates ? lr.data() : nullptr, damage ? ld.data() : nullptr, status ? ls.data() : nullptr))) return rc;
  if (moments) moments_to_caller(c, lm.data(), moments);
  if (rates) to_caller(view_of(c), 14, 14, lr.data(), rates);
  if (damage) to_caller(view_of(c), 21, 21, ld.data(), damage);
  if (status) to_caller(view_of(c), 7, 7, ls.data(), status);
  return FEAHIP_OK;
}

// ---- stress peaks over a sweep or a transient (kernels_stress_sweep.hip) ------------------------------------------------
// lib[r] = the library's node of the caller's probe_node[r], each inside [0, N)
static int probe_nodes(feahip_ctx *c, const char *who, int n_probe, const int *probe_node, int *lib)
{
  for (int r = 0; r < n_probe; ++r) {
    if (probe_node[r] < 0 || probe_node[r] >= c->N) { c->err = std::string(who) + ": probe node outside [0, N)"; return FEAHIP_EINVAL; }
    lib[r] = lib_id(c, probe_node[r]);
  }
  return FEAHIP_OK;
}

namespace {
// the four outputs in the library's order, and their way to the caller's
struct StressPeaks {
  std::vector<double> p6, vm;
  std::vector<int> a6, avm;
  explicit StressPeaks(const feahip_ctx *c) : p6(6 * (size_t)c->N), vm((size_t)c->N), a6(6 * (size_t)c->N), avm((size_t)c->N) {}
  void to_caller_ids(feahip_ctx *c, double *peak6, int *peak6_at, double *vm_out, int *vm_at) const
  {
    to_caller(view_of(c), 6, 6, p6.data(), peak6);
    to_caller(view_of(c), 6, 6, a6.data(), peak6_at);
    to_caller(view_of(c), 1, 1, vm.data(), vm_out);
    to_caller(view_of(c), 1, 1, avm.data(), vm_at);
  }
};
}

extern "C" int feahip_response_stress_sweep(feahip_ctx *c, int n_freq, const double *omega, double alpha, double beta_k,
                                            const double *zeta, double *peak6, int *peak6_at, double *vm, int *vm_at,
                                            int n_probe, const int *probe_node, double *probe_re, double *probe_im)
{
  CTX_GUARD_NOK(c);
  if (!omega || !peak6 || !peak6_at || !vm || !vm_at) { c->err = "response_stress_sweep: null omega, peak6, peak6_at, vm or vm_at"; return FEAHIP_EINVAL; }
  int rc;
  int probe[64];
  if ((rc = stress_form_ready(c, "response_stress_sweep")) || (rc = sweep_args(c, "response_stress_sweep", n_freq)) ||
      (rc = probe_args(c, "response_stress_sweep", n_probe, probe_node, probe_re, probe_im)) ||
      (rc = probe_nodes(c, "response_stress_sweep", n_probe, probe_node, probe))) return rc;
  StressPeaks out(c);
  std::vector<double> pre((size_t)n_probe * n_freq * 6), pim(pre.size());   // (the caller's arrays stay as they are on a refusal)
  if ((rc = stress_sweep(c, n_freq, omega, alpha, beta_k, zeta, out.p6.data(), out.a6.data(), out.vm.data(), out.avm.data(), n_probe,
                         probe, pre.data(), pim.data()))) return rc;
  out.to_caller_ids(c, peak6, peak6_at, vm, vm_at);
  std::copy(pre.begin(), pre.end(), probe_re);
  std::copy(pim.begin(), pim.end(), probe_im);
  return FEAHIP_OK;
}

extern "C" int feahip_response_stress_transient(feahip_ctx *c, int n_steps, double dt, const double *g, double alpha, double beta_k,
                                                const double *zeta, double *peak6, int *peak6_at, double *vm, int *vm_at,
                                                int n_probe, const int *probe_node, double *probe)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_form_ready(c, "response_stress_transient"))) return rc;
  if (!g || !peak6 || !peak6_at || !vm || !vm_at) { c->err = "response_stress_transient: null g, peak6, peak6_at, vm or vm_at"; return FEAHIP_EINVAL; }
  int lib_probe[64];
  if ((rc = history_args(c, "response_stress_transient", n_steps)) ||
      (rc = probe_args(c, "response_stress_transient", n_probe, probe_node, probe)) ||
      (rc = probe_nodes(c, "response_stress_transient", n_probe, probe_node, lib_probe))) return rc;
  StressPeaks out(c);
  std::vector<double> hist((size_t)n_probe * ((size_t)n_steps + 1) * 6);
  if ((rc = stress_transient(c, n_steps, dt, g, alpha, beta_k, zeta, out.p6.data(), out.a6.data(), out.vm.data(), out.avm.data(),
                             n_probe, lib_probe, hist.data()))) return rc;
  out.to_caller_ids(c, peak6, peak6_at, vm, vm_at);
  std::copy(hist.begin(), hist.end(), probe);
  return FEAHIP_OK;
}

// ---- rainflow counting of a transient (kernels_stress_rainflow.hip) --------------------------------------------------------
extern "C" int feahip_response_stress_rainflow(feahip_ctx *c, int n_steps, double dt, const double *g, double alpha, double beta_k,
                                               const double *zeta, double sn_b, double sn_a, int depth, int n_proj,
                                               const double *proj, double *damage, double *cycles, double *max_range, int *status,
                                               int *depth_used, int n_probe, const int *probe_node, double *probe)
{
  CTX_GUARD_NOK(c);
  int rc;
  if ((rc = stress_form_ready(c, "response_stress_rainflow"))) return rc;
  if (!g) { c->err = "response_stress_rainflow: null g"; return FEAHIP_EINVAL; }
  if ((rc = history_args(c, "response_stress_rainflow", n_steps)) ||
      (rc = probe_args(c, "response_stress_rainflow", n_probe, probe_node, probe))) return rc;
  if (!rainflow_arguments(sn_b, sn_a, depth)) {
    c->err = "response_stress_rainflow: the S-N curve N s^b = A needs a finite b in [1, 64] and a finite A > 0, the stack a depth in [4, 1024]";
    return FEAHIP_EINVAL;
  }
  if (n_proj < 0 || n_proj > FEA_RAINFLOW_MAX_PROJ) { c->err = "response_stress_rainflow: n_proj must be in [0, 48]"; return FEAHIP_EINVAL; }
  if (n_proj > 0 && !proj) { c->err = "response_stress_rainflow: null proj"; return FEAHIP_EINVAL; }
  for (int e = 0; e < 6 * n_proj; ++e)
    if (!std::isfinite(proj[e])) { c->err = "response_stress_rainflow: proj is not finite"; return FEAHIP_EINVAL; }
  int lib_probe[64];
  if ((rc = probe_nodes(c, "response_stress_rainflow", n_probe, probe_node, lib_probe))) return rc;
  const int W = 6 + n_proj;
  const size_t NW = (size_t)c->N * W;
  std::vector<double> ld(damage ? NW : 0), lc(cycles ? NW : 0), lr(max_range ? NW : 0);
  std::vector<int> ls(status ? NW : 0), lu(depth_used ? NW : 0);
  std::vector<double> hist((size_t)n_probe * ((size_t)n_steps + 1) * W);  // (the caller's arrays stay as they are on a refusal)
  if ((rc = stress_rainflow(c, n_steps, dt, g, alpha, beta_k, zeta, sn_b, sn_a, depth, n_proj, proj, damage ? ld.data() : nullptr,
                            cycles ? lc.data() : nullptr, max_range ? lr.data() : nullptr, status ? ls.data() : nullptr,
                            depth_used ? lu.data() : nullptr, n_probe, lib_probe, hist.data()))) return rc;
  if (damage) to_caller(view_of(c), W, W, ld.data(), damage);
  if (cycles) to_caller(view_of(c), W, W, lc.data(), cycles);
  if (max_range) to_caller(view_of(c), W, W, lr.data(), max_range);
  if (status) to_caller(view_of(c), W, W, ls.data(), status);
  if (depth_used) to_caller(view_of(c), W, W, lu.data(), depth_used);
  std::copy(hist.begin(), hist.end(), probe);
  return FEAHIP_OK;
}

extern "C" double feahip_host_harmonic_von_mises(const double re6[6], const double im6[6])
{
  return harmonic_von_mises(re6, im6);
}

extern "C" int feahip_host_modal_ritz(int n_dirs,const double *gram_m, const double *gram_k, double *theta, double *coef)
{
  if (!gram_m || !gram_k || !theta || !coef || (n_dirs != 8 && n_dirs != 16 && n_dirs != 24)) return FEAHIP_EINVAL;
  return modal_ritz(n_dirs, gram_m, gram_k, FEA_MODAL_COLS, theta, coef);
}

// ---- linear buckling (kernels_buckling.hip) -----------------------------------
extern "C" int feahip_host_buckling_factor(int n, const double *nu, double *factor)
{
  if (n < 0 || (n > 0 && (!nu || !factor))) return FEAHIP_EINVAL;
  for (int i = 0; i < n; ++i) factor[i] = nu[i] < 0.0 ? 1.0 - 1.0 / nu[i] : INFINITY;   // (-0.0 and NaN: no buckling found)
  return FEAHIP_OK;
}

extern "C" int feahip_solve_buckling(feahip_ctx *c, int n_modes, double tol, int max_iter, double *factor, double *nu,
                                     double *resid, int *iters)
{
  CTX_GUARD(c);
  if (iters) *iters = 0;
  int rc;
  if ((rc = eigen_args(c, "solve_buckling", n_modes, FEA_MODAL_COLS, tol, max_iter, factor, "factor"))) return rc;
  if ((rc = solve2_refused(c, "solve_buckling"))) return rc;
  double v[FEA_MODAL_COLS];
  for (int j = 0; j < n_modes; ++j) { v[j] = NAN; factor[j] = NAN; if (nu) nu[j] = NAN; if (resid) resid[j] = NAN; }
  rc = buckling_solve(c, n_modes, tol, max_iter, v, resid, iters);
  if (c->modal.have_buckling) {                                       // converged, or the steps ran out: the pairs as they stand
    (void)feahip_host_buckling_factor(n_modes, v, factor);
    if (nu) for (int j = 0; j < n_modes; ++j) nu[j] = v[j];
  }
  return rc;
}

extern "C" int feahip_get_buckling_modes(feahip_ctx *c, int first, int count, double *phi)
{
  CTX_GUARD_NOK(c);
  if (!c->modal.have_buckling) { c->err = "get_buckling_modes: no buckling modes held (feahip_solve_buckling first)"; return FEAHIP_ESTATE; }
  if (first < 0 || count < 0 || first + count > FEA_MODAL_COLS) { c->err = "get_buckling_modes: modes [first, first + count) outside the eight held"; return FEAHIP_EINVAL; }
  if (!phi) { c->err = "get_buckling_modes: null phi"; return FEAHIP_EINVAL; }
  return modes_to_caller(c, view_of(c), first, count, phi, modal_get);
}

extern "C" int feahip_geometric_spmv(feahip_ctx *c, const double *x, double *y)
{
  CTX_GUARD(c);
  if (!x || !y) return FEAHIP_EINVAL;
  int rc;
  if ((rc = solve2_refused(c, "geometric_spmv")) || (rc = geom_assemble(c))) return rc;
  BucklingState &B = c->buckling;
  if (!B.d_x4) FEA_HIP_CHECK(c, hipMalloc((void **)&B.d_x4, sizeof(double) * 4 * (size_t)c->N));
  if ((rc = set_view(c, B.d_x4, x, 3, 4))) return rc;
  if ((rc = launch_block_product(c, B.d_kg, B.d_x4, c->d_q))) return rc;
  return get_view(c, c->d_q, y, 3, 3);
}

// ---- two-column solve (kernels_solve2.hip) ---------------------------------
static int solve2_ready(feahip_ctx *c, const char *who)
{
  int rc;
  if ((rc = solve2_refused(c, who))) return rc;
  if (!c->k_valid) { c->err = std::string(who) + ": no stiffness matrix assembled"; return FEAHIP_ESTATE; }
  return ensure_solve2(c);
}

extern "C" int feahip_solve_slae2(feahip_ctx *c, int type, double tol, int max_iter, const double *f2, int iters[2], double resid[2])
{
  CTX_GUARD(c);
  if (type < FEAHIP_CG || type > FEAHIP_CHOLESKY) { c->err = "unknown solver type"; return FEAHIP_EINVAL; }
  if (max_iter <= 0) { c->err = "max_iterations must be positive"; return FEAHIP_EINVAL; }
  if (!f2) { c->err = "solve_slae2: null second right-hand side"; return FEAHIP_EINVAL; }
  int rc;
  if ((rc = solve2_ready(c, "solve_slae2"))) return rc;
  if ((rc = set_view(c, c->d_q, f2, 3, 3))) return rc;           // (q is scratch of any solve)
  if ((rc = launch_interleave(c, c->d_f, c->d_q, c->d2_f))) return rc;
  return solve_pcg2(c, type, tol, max_iter, iters, resid);
}

extern "C" int feahip_get_solution2(feahip_ctx *c, double *u2)
{
  CTX_GUARD(c);
  if (!c->d_u2) { c->err = "get_solution2 before solve_slae2"; return FEAHIP_ESTATE; }
  return get_view(c, c->d_u2, u2, 3, 3);
}

extern "C" int feahip_spmv2(feahip_ctx *c, const double *x2, double *y2)
{
  CTX_GUARD(c);
  if (!x2 || !y2) return FEAHIP_EINVAL;
  int rc;
  if ((rc = solve2_ready(c, "spmv2"))) return rc;
  if ((rc = set_view(c, c->d_p, x2, 3, 3)) || (rc = set_view(c, c->d_q, x2 + (size_t)c->ndof, 3, 3))) return rc;
  if ((rc = launch_interleave(c, c->d_p, c->d_q, c->d2_p))) return rc;
  if ((rc = launch_spmv2(c, c->d2_p, c->d2_q))) return rc;
  if ((rc = launch_deinterleave(c, c->d2_q, c->d_p, c->d_q))) return rc;
  if ((rc = get_view(c, c->d_p, y2, 3, 3))) return rc;
  return get_view(c, c->d_q, y2 + (size_t)c->ndof, 3, 3);
}

extern "C" int feahip_solve_arclength(feahip_ctx *c, double lambda_max, int max_steps, int max_newton, double desired_tolerance,
                                      int solver_type, double solver_tolerance, int solver_max_iter, double *lambda_log,
                                      double *tol_log, int log_cap, int *its_log, int *steps_done)
{
  CTX_GUARD(c);
  if (steps_done) *steps_done = 0;
  if (solver_type < FEAHIP_CG || solver_type > FEAHIP_CHOLESKY) { c->err = "unknown solver type"; return FEAHIP_EINVAL; }
  if (max_steps <= 0 || max_newton <= 0 || solver_max_iter <= 0) { c->err = "solve_arclength: max_steps, max_newton and solver_max_iter must be positive"; return FEAHIP_EINVAL; }
  int rc;
  if ((rc = solve2_refused(c, "solve_arclength"))) return rc;
  if (c->mass.body[0] != 0.0 || c->mass.body[1] != 0.0 || c->mass.body[2] != 0.0) { c->err = "solve_arclength: a body force is set on this context (not followed by the arc length)"; return FEAHIP_EINVAL; }
  if (c->contact.set) { c->err = "solve_arclength: contact is set on this context (not followed by the arc length)"; return FEAHIP_ESTATE; }
  if (c->surf.nfaces == 0) { c->err = "solve_arclength: no surface loads on this context"; return FEAHIP_ESTATE; }
  if ((rc = ensure_solve2(c))) return rc;
  return arclength_solve(c, lambda_max, max_steps, max_newton, desired_tolerance, solver_type, solver_tolerance,
                         solver_max_iter, lambda_log, tol_log, log_cap, its_log, steps_done);
}

extern "C" int feahip_node_numbering(feahip_ctx *c, int *library_id_of_node)
{
  if (!c || !library_id_of_node) return FEAHIP_EINVAL;
  for (int a = 0; a < c->N; ++a) library_id_of_node[a] = lib_id(c, a);
  return FEAHIP_OK;
}

static int ensure_state(feahip_ctx *c)
{
  const size_t n = (size_t)c->E * c->G * 9;
  if (!c->d_F) {
    FEA_HIP_CHECK(c, hipMalloc((void **)&c->d_F, sizeof(double) * n));
    FEA_HIP_CHECK(c, hipMalloc((void **)&c->d_S, sizeof(double) * n));
  }
  if (!c->state_valid) {
    int rc = launch_state_export(c);
    if (rc) return rc;
    c->state_valid = true;
  }
  return FEAHIP_OK;
}

extern "C" int feahip_get_graddefs(feahip_ctx *c, double *F)
{
  CTX_GUARD(c);
  int rc = ensure_state(c);
  if (rc) return rc;
  return get_vec(c, c->d_F, F, (size_t)c->E * c->G * 9);
}

extern "C" int feahip_get_stresses(feahip_ctx *c, double *S)
{
  CTX_GUARD(c);
  int rc = ensure_state(c);
  if (rc) return rc;
  return get_vec(c, c->d_S, S, (size_t)c->E * c->G * 9);
}

extern "C" int feahip_get_shape_gradients(feahip_ctx *c, double *grads, double *detj)
{
  CTX_GUARD(c);
  if (!grads || !detj) return FEAHIP_EINVAL;
  int rc = ensure_state(c);                                  // allocates F / sigma (the kernel writes them too)
  if (rc) return rc;
  const size_t ng = (size_t)c->E * c->G * 3 * c->npe, nd = (size_t)c->E * c->G;
  DevTemp dg, dd;
  if ((rc = dg.alloc(c, ng))) return rc;
  if (dd.alloc(c, nd)) { c->err = "out of device memory"; return FEAHIP_ENOMEM; }
  if ((rc = launch_state_export(c, dg.p, dd.p)) || (rc = get_vec(c, dg.p, grads, ng))) return rc;
  return get_vec(c, dd.p, detj, nd);
}

extern "C" int feahip_matrix_nnz(feahip_ctx *c, long long *nnz)
{
  if (!c || !nnz) return FEAHIP_EINVAL;
  *nnz = (long long)c->nnzb * 9;
  return FEAHIP_OK;
}

template <class OFF>
static int matrix_yale(feahip_ctx *c, OFF *offsets, int *indexes, double *values)
{
  std::vector<double> K((size_t)c->nnzb * 9, 0.0);               // rows of other ranks read as zero
  int rc = get_vec(c, c->d_K_base, K.data() + (size_t)c->kb0 * 9, (size_t)(c->kb1 - c->kb0) * 9);
  if (rc) return rc;
  size_t pos = 0;
  offsets[0] = 0;
  std::vector<std::pair<int, int>> row;                           // (caller's column node, block) of one row, sorted by column
  for (int a = 0; a < c->N; ++a) {                                // a: the CALLER's node; its row lives at the library id
    const int la = lib_id(c, a);
    row.clear();
    for (int q = c->h_rowptr[la]; q < c->h_rowptr[la + 1]; ++q)
      row.emplace_back(c->iperm.empty() ? c->h_colidx[q] : c->iperm[c->h_colidx[q]], q);
    if (!c->iperm.empty()) std::sort(row.begin(), row.end());
    for (int i = 0; i < 3; ++i) {
      for (const auto &cb : row)
        for (int j = 0; j < 3; ++j) {
          indexes[pos] = 3 * cb.first + j;
          values[pos] = K[(size_t)cb.second * 9 + 3 * i + j];
          pos++;
        }
      offsets[3 * a + i + 1] = (OFF)pos;
    }
  }
  return FEAHIP_OK;
}

extern "C" int feahip_get_matrix_yale(feahip_ctx *c, int *offsets, int *indexes, double *values)
{
  CTX_GUARD(c);
  if (!offsets || !indexes || !values) return FEAHIP_EINVAL;
  if ((long long)c->nnzb * 9 > 0x7FFFFFFFLL) {                   // sp_matrix_yale keeps int offsets: refused, not wrapped
    c->err = "matrix too large for 32-bit Yale offsets (use feahip_get_matrix_yale64)";
    return FEAHIP_EINVAL;
  }
  return matrix_yale<int>(c, offsets, indexes, values);
}

extern "C" int feahip_get_matrix_yale64(feahip_ctx *c, long long *offsets, int *indexes, double *values)
{
  CTX_GUARD(c);
  if (!offsets || !indexes || !values) return FEAHIP_EINVAL;
  if ((long long)c->N * 3 > 0x7FFFFFFFLL) { c->err = "more than 2^31 dofs: column indexes do not fit"; return FEAHIP_EINVAL; }
  return matrix_yale<long long>(c, offsets, indexes, values);
}

extern "C" int feahip_spmv(feahip_ctx *c, const double *x, double *y)
{
  CTX_GUARD(c);
  if (!x || !y) return FEAHIP_EINVAL;
  int rc = set_view(c, c->d_p, x, 3, 3);
  if (rc) return rc;
  rc = launch_spmv(c, c->d_p, c->d_q);
  if (rc) return rc;
  return get_view(c, c->d_q, y, 3, 3);
}

extern "C" int feahip_apply_preconditioner(feahip_ctx *c, const double *r, double *z)
{
  CTX_GUARD(c);
  if (!r || !z) return FEAHIP_EINVAL;
  if (!c->k_valid) { c->err = "apply_preconditioner: no stiffness matrix assembled"; return FEAHIP_ESTATE; }
  int rc = set_view(c, c->d_r, r, 3, 3);
  if (rc) return rc;
  const double *dz = nullptr;
  if ((rc = precond_apply(c, c->d_r, &dz))) return rc;
  return get_view(c, dz, z, 3, 3, true);                         // rows of other ranks: 0
}

// z = M^-1 r on every rank of a group at once: what the group's PCG applies.  Under kind 2 the operator spans the
// ranks, so this is the only way to apply it in-process; kinds 0 and 1 give what the per-context entry gives.
int dist_precond_apply(std::vector<feahip_ctx *> &R, const double **z);      // kernels_solve.hip
extern "C" int feahip_group_apply_preconditioner(feahip_ctx **ctxs, int n, const double *const *r, double *const *z)
{
  std::vector<feahip_ctx *> R;
  int rc = group_vec(ctxs, n, R);
  if (rc) return rc;
  if (!r || !z) return FEAHIP_EINVAL;
  for (int k = 0; k < n; ++k) {
    feahip_ctx *c = R[k];
    if (!r[k] || !z[k]) return FEAHIP_EINVAL;
    CTX_GUARD(c);
    if (!c->k_valid) { c->err = "apply_preconditioner: no stiffness matrix assembled"; return FEAHIP_ESTATE; }
    if ((rc = set_view(c, c->d_r, r[k], 3, 3))) return rc;
  }
  std::vector<const double *> dz((size_t)n, nullptr);
  if ((rc = surface_error(R[0], R, dist_precond_apply(R, dz.data())))) return rc;
  for (int k = 0; k < n; ++k) {
    feahip_ctx *c = R[k];
    FEA_HIP_CHECK(c, hipSetDevice(c->device));
    if ((rc = get_view(c, dz[k], z[k], 3, 3, true))) return rc;  // rows of other ranks: 0
  }
  return FEAHIP_OK;
}

// ---- the coarse level across the ranks (preconditioner 2, coarse.h) -----------
// prepared for the current K as the next solve would prepare it; collective -- an in-process group is driven from
// any of its contexts, the ranks of an RCCL run all make the call
static int coarse_ready(feahip_ctx *c)
{
  if (c->precond != 2) { c->err = "coarse view: the preconditioner is not kind 2 (feahip_set_preconditioner(2))"; return FEAHIP_ESTATE; }
  std::vector<feahip_ctx *> R(1, c);
  if (c->tr && c->tr->members()) R = *c->tr->members();
  for (feahip_ctx *m : R) {
    if (m->precond != 2) { c->err = "coarse view: preconditioner 2 is not set on every rank of the group"; return FEAHIP_ESTATE; }
    CTX_GUARD(m);
  }
  const int rc = coarse_prepare(R, c->tr);
  if (rc && c->err.empty()) c->err = R[0]->err;
  FEA_HIP_CHECK(c, hipSetDevice(c->device));
  return rc;
}

extern "C" int feahip_coarse_info(feahip_ctx *c, long long *out8, int *agg_of_owned_row, double *centroids)
{
  CTX_GUARD(c);
  if (!out8) return FEAHIP_EINVAL;
  const int rc = coarse_ready(c);
  if (rc) return rc;
  return coarse_export_info(c, out8, agg_of_owned_row, centroids);
}

extern "C" int feahip_coarse_matrix(feahip_ctx *c, double *A)
{
  CTX_GUARD(c);
  if (!A) return FEAHIP_EINVAL;
  const int rc = coarse_ready(c);
  if (rc) return rc;
  return coarse_export_matrix(c, A);
}

extern "C" int feahip_host_coarse_aggregates(int n_owned, int m, int *first_row_of_aggregate)
{
  if (n_owned < 1 || m < 1) return FEAHIP_EINVAL;
  return coarse_cuts(n_owned, m, first_row_of_aggregate);
}

// the hierarchy as the next PCG solve would use it (prepared here when K changed since)
static int amg_ready(feahip_ctx *c)
{
  if (c->precond < 1) { c->err = "multigrid view: the preconditioner is not the multigrid (feahip_set_preconditioner(1))"; return FEAHIP_ESTATE; }
  if (!c->k_valid) { c->err = "multigrid view: no stiffness matrix assembled"; return FEAHIP_ESTATE; }
  return amg_prepare(c);
}

extern "C" int feahip_amg_info(feahip_ctx *c, long long *out16, double *over)
{
  CTX_GUARD(c);
  if (!out16 || !over) return FEAHIP_EINVAL;
  int rc = amg_ready(c);
  if (rc) return rc;
  return amg_export_info(c, out16, over);
}

extern "C" int feahip_amg_level(feahip_ctx *c, int level, long long *counts, double *omega, int *rowptr, int *colidx,
                                double *K, int *agg, double *doff, int *type)
{
  CTX_GUARD(c);
  if (!counts) return FEAHIP_EINVAL;
  int rc = amg_ready(c);
  if (rc) return rc;
  AmgLevelExport e;
  if ((rc = amg_export_level(c, level, e))) return rc;
  counts[0] = e.N; counts[1] = e.nnzb; counts[2] = e.Nc; counts[3] = e.bits;
  if (omega) *omega = e.omega;
  if (!rowptr || !colidx || !K || !agg || !doff || !type) return FEAHIP_OK;    // sizing call
  if (level > 0 || c->perm.empty()) {
    std::copy(e.rowptr.begin(), e.rowptr.end(), rowptr);
    std::copy(e.colidx.begin(), e.colidx.end(), colidx);
    std::copy(e.K.begin(), e.K.end(), K);
    std::copy(e.agg.begin(), e.agg.end(), agg);
    std::copy(e.doff.begin(), e.doff.end(), doff);
    std::copy(e.type.begin(), e.type.end(), type);
    return FEAHIP_OK;
  }
  // level 0 in the caller's node ids, every row's blocks sorted by the caller's column (feahip_get_matrix_yale's order)
  std::vector<std::pair<int, int>> row;
  size_t pos = 0;
  rowptr[0] = 0;
  for (int a = 0; a < c->N; ++a) {
    const int la = lib_id(c, a);
    row.clear();
    for (int q = e.rowptr[(size_t)la]; q < e.rowptr[(size_t)la + 1]; ++q) row.emplace_back(c->iperm[(size_t)e.colidx[(size_t)q]], q);
    std::sort(row.begin(), row.end());
    for (const auto &cb : row) {
      colidx[pos] = cb.first;
      for (int t = 0; t < 9; ++t) K[pos * 9 + t] = e.K[(size_t)cb.second * 9 + t];
      pos++;
    }
    rowptr[a + 1] = (int)pos;
  }
  const NodeView v = view_of(c);
  to_caller(v, 1, 1, e.agg.data(), agg);
  to_caller(v, 1, 1, e.type.data(), type);
  to_caller(v, 3, 3, e.doff.data(), doff);
  return FEAHIP_OK;
}

extern "C" int feahip_time_kernel(feahip_ctx *c, int what, int warmup, int iters, double *avg_ms)
{
  CTX_GUARD(c);
  if (!avg_ms || iters <= 0 || warmup < 0) return FEAHIP_EINVAL;
  if (what == 4) return time_pcg_iteration(c, warmup, iters, avg_ms);
  if (what == 6 || what == 7) {
    const int rk = solve2_ready(c, what == 6 ? "time_kernel(6)" : "time_kernel(7)");
    if (rk) return rk;
    if (what == 7) return time_pcg2_iteration(c, warmup, iters, avg_ms);
  }
  if (what == 8 || what == 9) {
    if (!c->mass.set || c->mass.stale) { c->err = std::string(what == 8 ? "time_kernel(8)" : "time_kernel(9)") + ": no mass on this context (feahip_set_mass)"; return FEAHIP_EINVAL; }
    const int rk = mass_ensure(c, "time_kernel");
    if (rk) return rk;
  }
  if (what == 21 || what == 22) {
    const std::string who = "time_kernel(" + std::to_string(what) + ")";
    if (!c->damping.on() || (what == 21 && !(c->damping.beta > 0.0))) {
      c->err = who + (what == 21 ? ": no damping with beta_k > 0 on this context (feahip_set_damping)" : ": no damping on this context (feahip_set_damping)");
      return FEAHIP_EINVAL;
    }
    if (!c->mass.set || c->mass.stale) { c->err = who + ": no mass on this context (feahip_set_mass)"; return FEAHIP_EINVAL; }
    int rk;
    if ((rk = mass_ensure(c, "time_kernel")) || (rk = damping_ready(c, "time_kernel"))) return rk;
  }
  if (what == 10 || what == 11) {
    if (!c->mass.set || c->mass.stale) { c->err = std::string(what == 10 ? "time_kernel(10)" : "time_kernel(11)") + ": no mass on this context (feahip_set_mass)"; return FEAHIP_EINVAL; }
    const int rk = lump_ensure(c, "time_kernel");
    if (rk) return rk;
  }
  if (what >= 13 && what <= 15) {
    const std::string who = "time_kernel(" + std::to_string(what) + ")";
    if (!c->mass.set || c->mass.stale) { c->err = who + ": no mass on this context (feahip_set_mass)"; return FEAHIP_EINVAL; }
    int rk;
    if ((rk = solve2_refused(c, who.c_str())) || (rk = mass_ensure(c, "time_kernel")) || (rk = time_modal_prepare(c))) return rk;
  }
  if (what == 16 || what == 17) {
    const std::string who = "time_kernel(" + std::to_string(what) + ")";
    if (!c->mass.set || c->mass.stale) { c->err = who + ": no mass on this context (feahip_set_mass)"; return FEAHIP_EINVAL; }
    int rk;
    if ((rk = solve2_refused(c, who.c_str())) || (rk = mass_ensure(c, "time_kernel")) || (rk = time_deflate_prepare(c))) return rk;
  }
  if (what == 18 || what == 19) {                      // one assembly first: the buffers, and the records the block pass reads
    int rk;
    if ((rk = solve2_refused(c, what == 18 ? "time_kernel(18)" : "time_kernel(19)")) || (rk = geom_assemble(c))) return rk;
  }
  if (what == 23 || what == 24) {                      // the table, the store and f as the last response_sweep left them
    const int rk = response_loaded(c, what == 23 ? "time_kernel(23)" : "time_kernel(24)");
    if (rk) return rk;
    if (c->response.swept_freq == 0) { c->err = "time_kernel: no sweep made yet (feahip_response_sweep first)"; return FEAHIP_ESTATE; }
  }
  if (what == 25) {                                    // the last chunk of the last transient, the store and u_s as it left them
    const int rk = response_loaded(c, "time_kernel(25)");
    if (rk) return rk;
    if (c->response.trans_rows == 0) { c->err = "time_kernel: no transient made yet (feahip_response_transient first)"; return FEAHIP_ESTATE; }
  }
  if (what == 26) {                                    // the form of the last combination, the store and u_s as it left them
    const int rk = response_loaded(c, "time_kernel(26)");
    if (rk) return rk;
    if (!c->response.form_set || c->response.form_gen != c->modal.lock_gen) { c->err = "time_kernel: no form set yet (feahip_response_combine, _random or _spectrum first)"; return FEAHIP_ESTATE; }
  }
  if (what == 27 || what == 28) {                      // the stress store in force; 28: the form of the last stress combination
    const int rk = what == 27 ? stress_ready(c, "time_kernel(27)") : stress_form_ready(c, "time_kernel(28)");
    if (rk) return rk;
    if (what == 28 && !c->stress.form_set) { c->err = "time_kernel: no stress form set yet (feahip_response_stress_combine, _random or _spectrum first)"; return FEAHIP_ESTATE; }
  }
  if (what == 29 || what == 30) {                      // the table of the last stress sweep / the last chunk of the last stress transient
    const int rk = stress_form_ready(c, what == 29 ? "time_kernel(29)" : "time_kernel(30)");
    if (rk) return rk;
    const bool laid = c->stress.table_gen == c->modal.lock_gen;
    if (what == 29 && !(laid && c->stress.swept_freq > 0)) { c->err = "time_kernel: no stress sweep made yet (feahip_response_stress_sweep first)"; return FEAHIP_ESTATE; }
    if (what == 30 && !(laid && c->stress.trans_rows > 0)) { c->err = "time_kernel: no stress transient made yet (feahip_response_stress_transient first)"; return FEAHIP_ESTATE; }
  }
  if (what == 31 || what == 32) {                      // the four forms of the last moments / the moments and the curve of the last rates
    const int rk = stress_form_ready(c, what == 31 ? "time_kernel(31)" : "time_kernel(32)");
    if (rk) return rk;
    if (what == 31 && !c->fatigue.forms_set) { c->err = "time_kernel: no stress moments made yet (feahip_response_stress_moments or _fatigue first)"; return FEAHIP_ESTATE; }
    if (what == 32 && !(c->fatigue.mom_set && c->fatigue.rates_set)) { c->err = "time_kernel: no fatigue rates made yet (feahip_response_stress_fatigue first)"; return FEAHIP_ESTATE; }
  }
  if (what == 33) {                                    // the last chunk of the last stress rainflow, its curve and its depth
    const int rk = stress_form_ready(c, "time_kernel(33)");
    if (rk) return rk;
    if (!(c->rainflow.table_gen == c->modal.lock_gen && c->rainflow.rows > 0 && c->rainflow.d_stack && c->rainflow.depth <= c->rainflow.depth_cap)) { c->err = "time_kernel: no stress rainflow made yet (feahip_response_stress_rainflow first)"; return FEAHIP_ESTATE; }
  }
  if (what == 12) { const int rk = launch_results(c, -1, c->d_scal + 8); if (rk) return rk; }   // (allocates on first use)
  if (what == 5 && c->surf.nfaces == 0) { c->err = "time_kernel(5): no surface loads on this context"; return FEAHIP_EINVAL; }
  if (what == 20 && c->contact.n == 0) { c->err = "time_kernel(20): no contact on this context"; return FEAHIP_EINVAL; }
  return time_enqueued(c, warmup, iters, avg_ms, [&](int) -> int {
    switch (what) {
    case 0: return launch_assemble(c, true, true);
    case 1: return launch_assemble(c, true, false);
    case 2: return launch_assemble(c, false, true);
    case 3: return launch_spmv(c, c->d_p, c->d_q);
    case 5: return launch_surface_loads(c, c->d_f);
    case 6: return launch_spmv2(c, c->d2_p, c->d2_q);
    case 8: return launch_mass_add(c, 1.0);
    case 9: return launch_mass_residual(c, 1.0);
    case 10: { const int rk = launch_explicit_kick(c, 1.0); return rk ? rk : launch_explicit_finish(c, 1.0); }
    case 11: return launch_gershgorin(c);
    case 12: return launch_results(c, -1, c->d_scal + 8);
    case 13: case 14: case 15: return time_modal_kernel(c, what);
    case 16: case 17: return time_deflate_kernel(c, what);
    case 18: case 19: return time_geom_kernel(c, what);
    case 20: return launch_contact(c, true, true, c->d_f);
    case 21: return launch_damp_add(c, 1.0, 1.0);
    case 22: return launch_damp_residual(c, 1.0, 1.0);
    case 23: case 24: return time_response_kernel(c, what);
    case 25: return time_transient_kernel(c);
    case 26: return time_combine_kernel(c);
    case 27: return time_stress_store(c);
    case 28: return time_stress_combine(c);
    case 29: case 30: return time_stress_sweep_kernel(c, what);
    case 31: return time_stress_moments(c);
    case 32: return time_fatigue_rates(c);
    case 33: return time_rainflow_kernel(c);
    default: c->err = "unknown kernel selector"; return FEAHIP_EINVAL;
    }
  });
}

// Streaming copies: the copy bandwidth of THIS box, the figure the roofline fractions can be quoted against next to the
// 8 TB/s of the data sheet (MI355X_MICROARCH.md measures 6.29 TB/s with a float4 copy).  Four ways, the
// best one is reported (feahip_copy_bandwidth) and all four are available (feahip_copy_bandwidth_detail):
//   [0] one 16-byte load in flight per lane, grid-stride (rounds 1-3);
//   [1] FOUR independent 16-byte loads in flight per lane, then their four stores -- each workgroup streams a
//       contiguous 16 KB tile per step, 16 workgroups per CU;
//   [2] hipMemcpyDtoDAsync (the runtime's blit kernel);
//   [3] as [1] with non-temporal loads and stores.
__global__ __launch_bounds__(256)
void k_copy16(const double2 *__restrict__ src, double2 *__restrict__ dst, size_t n)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

typedef double copy_v2d __attribute__((ext_vector_type(2)));
template <bool NT>
__global__ __launch_bounds__(256)
void k_copy16x4(const copy_v2d *__restrict__ src, copy_v2d *__restrict__ dst, size_t n)
{
  // tile = 4 x 256 pieces of 16 bytes; tiles dealt round-robin to the workgroups
  const size_t ntiles = n >> 10;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t i = (tile << 10) + threadIdx.x;
    copy_v2d a, b, c, d;
    if (NT) { a = __builtin_nontemporal_load(src + i); b = __builtin_nontemporal_load(src + i + 256);
              c = __builtin_nontemporal_load(src + i + 512); d = __builtin_nontemporal_load(src + i + 768); }
    else { a = src[i]; b = src[i + 256]; c = src[i + 512]; d = src[i + 768]; }
    if (NT) { __builtin_nontemporal_store(a, dst + i); __builtin_nontemporal_store(b, dst + i + 256);
              __builtin_nontemporal_store(c, dst + i + 512); __builtin_nontemporal_store(d, dst + i + 768); }
    else { dst[i] = a; dst[i + 256] = b; dst[i + 512] = c; dst[i + 768] = d; }
  }
  for (size_t i = (ntiles << 10) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

extern "C" int feahip_copy_bandwidth_detail(feahip_ctx *c, long long bytes, double *gbytes_per_s4)
{
  CTX_GUARD_NOK(c);
  if (!gbytes_per_s4 || bytes < (1 << 20)) return FEAHIP_EINVAL;
  const size_t n = (size_t)bytes / 16;
  double2 *a = nullptr, *b = nullptr;
  FEA_HIP_CHECK(c, hipMalloc((void **)&a, n * 16));
  if (hipMalloc((void **)&b, n * 16) != hipSuccess) { (void)hipFree(a); c->err = "out of device memory"; return FEAHIP_ENOMEM; }
  (void)hipMemsetAsync(a, 0x3c, n * 16, c->stream);
  const int grid = 256 * 16;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  hipError_t err = hipSuccess;
  const int reps = 10;
  for (int m = 0; m < 4; ++m) {
    auto one = [&]() {
      if (m == 0) hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(256), 0, c->stream, a, b, n);
      else if (m == 1) hipLaunchKernelGGL(k_copy16x4<false>, dim3(grid), dim3(256), 0, c->stream, (const copy_v2d *)a, (copy_v2d *)b, n);
      else if (m == 3) hipLaunchKernelGGL(k_copy16x4<true>, dim3(grid), dim3(256), 0, c->stream, (const copy_v2d *)a, (copy_v2d *)b, n);
      else (void)hipMemcpyDtoDAsync((hipDeviceptr_t)b, (hipDeviceptr_t)a, n * 16, c->stream);
    };
    for (int k = 0; k < 3; ++k) one();
    (void)hipEventRecord(e0, c->stream);
    for (int k = 0; k < reps; ++k) one();
    (void)hipEventRecord(e1, c->stream);
    const hipError_t e = hipEventSynchronize(e1);
    if (e != hipSuccess) err = e;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    gbytes_per_s4[m] = ms > 0 ? 2.0 * (double)(n * 16) * reps / ((double)ms * 1e-3) / 1e9 : 0.0;      // read + written
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  (void)hipFree(a); (void)hipFree(b);
  if (err != hipSuccess || !(gbytes_per_s4[0] > 0)) { c->err = "copy kernel failed"; return FEAHIP_EHIP; }
  return FEAHIP_OK;
}

extern "C" int feahip_copy_bandwidth(feahip_ctx *c, long long bytes, double *gbytes_per_s)
{
  double v[4] = {0, 0, 0, 0};
  if (!gbytes_per_s) return FEAHIP_EINVAL;
  const int rc = feahip_copy_bandwidth_detail(c, bytes, v);
  if (rc) return rc;
  *gbytes_per_s = std::max(std::max(v[0], v[1]), std::max(v[2], v[3]));
  return FEAHIP_OK;
}

extern "C" int feahip_assembly_stats(feahip_ctx *c, double *o)
{
  if (!c || !o) return FEAHIP_EINVAL;
  const GatherCache &g = c->gather10.built() ? (const GatherCache &)c->gather10 : c->gather;
  o[0] = g.built() ? g.evals_per_element : 0.0;
  o[1] = g.built() ? (double)g.nchunks : 0.0;
  o[2] = g.built() ? (double)g.same_words : 0.0;
  o[3] = g.built() ? (double)g.bytes : 0.0;
  return FEAHIP_OK;
}

extern "C" int feahip_assembly_in_use(feahip_ctx *c, int *strategy)
{
  if (!c || !strategy) return FEAHIP_EINVAL;
  *strategy = c->last_strategy;
  return FEAHIP_OK;
}

extern "C" int feahip_device_layout(feahip_ctx *c, long long *o)
{
  if (!c || !o) return FEAHIP_EINVAL;
  { const int rc = ensure_k(c); if (rc) return rc; }
  o[0] = (long long)(size_t)c->d_K_base; o[1] = (long long)(size_t)c->d_colidx; o[2] = (long long)(size_t)c->d_p; o[3] = (long long)(size_t)c->d_q;
  return FEAHIP_OK;
}

extern "C" int feahip_sizes(feahip_ctx *c, long long *o)
{
  if (!c || !o) return FEAHIP_EINVAL;
  o[0] = c->N; o[1] = c->E; o[2] = c->npe; o[3] = c->G; o[4] = c->nnzb; o[5] = c->nchunks;
  // bytes of the maps the default assembly kernel reads besides the algorithmic inputs
  o[6] = c->gather.built() ? c->gather.bytes
       : c->gather10.built() ? c->gather10.bytes
       : c->visits.built() ? c->visits.bytes + (long long)(c->N + 1) * 8
       : c->quad.built() ? c->quad.bytes + (long long)(c->N + 1) * 8 : c->generic.bytes;
  o[7] = c->max_rowlen;
  return FEAHIP_OK;
}
