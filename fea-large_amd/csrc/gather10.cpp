// gather10.cpp -- one-time host construction of the maps of the GATHER assembly
// of elements with several Gauss points: 10-node tetrahedra, 8-node bricks
// (kernels_gather10.hip).
//
// The reference integrates a 30x30 element matrix Gauss point by Gauss point
// and scatters it (fea_solver.c:887-1068, sp_matrix_element_add :966,1055).
// As for the 4-node element (gather.cpp) the scatter is inverted once: a chunk
// of consecutive block rows gets one record that lists
//   header   rows, CSR range, counts, the rows of every write-out pass
//   elems    its distinct elements, as indices into the rank's element list (the state kernel's output order)
//   rows     per row: first tile position, diagonal position, first residual lane
//   tpos     per thread and block slot: tile position of the block (a, b) and of its mirror (b, a) when b is a
//            row of the chunk too (one thread serves both, the mirror is the transpose)
//   flist    per visit lane a slice of ONE row's (element, local node) visits: residual and diagonal block
//   clist    per thread and block slot the (element, local row node, local column node) contributions
// Blocks are dealt to the threads longest list first, so the 64 blocks a wave works on at a time have lists of
// (nearly) the same length.  Lists are stored thread-minor: a wave reads 64 consecutive words.
#include "feahip_internal.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

#define Q_RS 0
#define Q_RD 66
#define Q_FF 130
#define Q_MAX_TASKS (FEA_Q_SLOTS * FEA_Q_THREADS)
#define Q_FENT 8                        // visits per residual lane at most (4 words)

namespace {
// ---- pass A: chunk boundaries (partition_rows, cost = element evaluations).  false: a single row does not fit, and
// out.limit / out.limit_row say which limit of pass A it exceeds first, at which row
bool partition(const int *conn, const HostPattern &hp, int npe, int row_lo, int row_hi, int L, int max_elems, int alpha,
               int tile_blocks, HostGather10 &out)
{
  const int nrows = row_hi - row_lo;
  std::vector<uint16_t> cost((size_t)nrows * L, 0xFFFFu);
  parallel_ranges(nrows, 256, [&](int lo, int hi) {
    std::vector<int> fresh;
    for (int i = lo; i < hi; ++i) {
      int nb = 0, nfl = 0;
      chunk_costs(hp, conn, npe, row_lo + i, row_hi, L, fresh, &cost[(size_t)i * L], [&](int r, int l, int nel, int ntask, const std::vector<int> &) {
        const int rowlen = hp.rowptr[r + 1] - hp.rowptr[r];
        nb += rowlen;
        nfl += std::max(1, (hp.incptr[r + 1] - hp.incptr[r] + Q_FENT - 1) / Q_FENT);
        return nel <= (l > 1 ? max_elems : FEA_Q_MAX_ELEMS) && ntask <= Q_MAX_TASKS && nfl <= FEA_Q_FLANES &&
               rowlen <= tile_blocks / 2 && nb <= (FEA_Q_MAX_PASS - 2) * tile_blocks && nb < 0xFFFF;
      });
    }
  });
  const int r = partition_rows(cost, row_lo, row_hi, L, alpha, out.first_row);
  if (r < 0) return true;
  const int ninc = hp.incptr[r + 1] - hp.incptr[r], rowlen = hp.rowptr[r + 1] - hp.rowptr[r];
  out.limit_row = r;
  out.limit = ninc > FEA_Q_MAX_ELEMS ? G10_ELEMS : rowlen > tile_blocks / 2 ? G10_ROW_LENGTH
            : rowlen - 1 > Q_MAX_TASKS ? G10_TASKS : (ninc + Q_FENT - 1) / Q_FENT > FEA_Q_FLANES ? G10_RESIDUAL_LANES
            : rowlen > (FEA_Q_MAX_PASS - 2) * tile_blocks ? G10_PASSES : G10_OTHER;
  return false;
}

struct Local {                                      // a chunk's record, before the layout is known
  Gather10Header h;
  std::vector<uint32_t> elems, tpos;
  std::vector<uint16_t> rows, flist;
  std::vector<std::vector<uint16_t>> lists;        // per task, in thread order (task i: thread i % 256, slot i / 256)
};

// ---- pass B: one chunk's record, stage by stage; one per parallel_ranges worker, its vectors reused chunk after chunk
struct ChunkBuilder {
  const int *conn;
  const HostPattern &hp;
  const std::vector<int> &elist;
  int npe, tile_blocks;
  int r0 = 0, r1 = 0, nrows = 0, b0 = 0, nb = 0, ntask = 0;
  std::vector<int> el, task_of, order;
  std::vector<uint32_t> tp;
  std::vector<std::vector<uint16_t>> lists;

  ChunkBuilder(const int *c, const HostPattern &p, const std::vector<int> &e, int n, int t)
      : conn(c), hp(p), elist(e), npe(n), tile_blocks(t) {}

  // G10_FITS, or the limit the chunk exceeds
  int build(int row0, int row1, Local &Lc)
  {
    r0 = row0; r1 = row1; nrows = r1 - r0; b0 = hp.rowptr[r0]; nb = hp.rowptr[r1] - b0;
    Gather10Header &h = Lc.h;
    memset(&h, 0, sizeof(h));
    int limit = chunk_lists(Lc);
    if (limit == G10_FITS) limit = deal(Lc);
    if (limit == G10_FITS) limit = write_out_passes(h);
    if (limit == G10_FITS) limit = residual_lanes(Lc);
    if (limit != G10_FITS) return limit;
    Lc.elems.assign(el.size(), 0);                  // index into the rank's element list = the state kernel's output order
    for (size_t i = 0; i < el.size(); ++i)
      Lc.elems[i] = (uint32_t)(std::lower_bound(elist.begin(), elist.end(), el[i]) - elist.begin());
    h.r0 = r0; h.r1 = r1; h.b0 = b0; h.nb = nb; h.nnode = 0; h.nelem = (int)el.size(); h.ntask = ntask;
    return G10_FITS;
  }

  // ---- the chunk's elements, its blocks with a thread and their contributions
  int chunk_lists(Local &Lc)
  {
    chunk_elements(hp, r0, r1, el);
    const int nelem = (int)el.size();
    if (nelem > FEA_Q_MAX_ELEMS || nrows > FEA_Q_MAX_ROWS || nb >= 0xFFFF) return nelem > FEA_Q_MAX_ELEMS ? G10_ELEMS : G10_OTHER;
    Lc.rows.assign(FEA_Q_ROWS_U16, 0);
    for (int a = r0; a < r1; ++a) {
      Lc.rows[Q_RS + (a - r0)] = (uint16_t)(hp.rowptr[a] - b0);
      Lc.rows[Q_RD + (a - r0)] = (uint16_t)(hp.diag[a] - b0);
    }
    Lc.rows[Q_RS + nrows] = (uint16_t)nb;
    chunk_block_tasks(hp, r0, r1, tp, task_of);
    ntask = (int)tp.size();
    if (ntask > Q_MAX_TASKS) return G10_TASKS;
    chunk_block_lists(hp, conn, npe, r0, r1, el, task_of, ntask, 7, 11, lists);
    return G10_FITS;
  }

  // ---- longest lists first (ties: CSR order), dealt to the waves in runs of 64 so that the 64 blocks a wave works
  // on at a time have lists of (nearly) one length; the runs go over the waves back and forth
  int deal(Local &Lc)
  {
    Gather10Header &h = Lc.h;
    order.resize((size_t)ntask);
    for (int i = 0; i < ntask; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lists[x].size() > lists[y].size(); });
    Lc.tpos.assign((size_t)Q_MAX_TASKS, 0xFFFFFFFFu);          // no block: neither position is ever in a pass
    Lc.lists.assign((size_t)Q_MAX_TASKS, std::vector<uint16_t>());
    bool too_long = false;
    for (int i = 0; i < ntask; ++i) {
      const int run = i / 64, s = run / FEA_Q_WAVES, wv = (s & 1) ? FEA_Q_WAVES - 1 - (run % FEA_Q_WAVES) : (run % FEA_Q_WAVES);
      const int slot = s * FEA_Q_THREADS + wv * 64 + (i & 63);           // thread wv*64 + i%64, block slot s
      Lc.tpos[slot] = tp[order[i]];
      Lc.lists[slot].swap(lists[order[i]]);
      const int len = (int)Lc.lists[slot].size();
      if (len > 250) too_long = true;
      h.cnt[FEA_Q_WAVES * s + wv] = (unsigned char)std::max((int)h.cnt[FEA_Q_WAVES * s + wv], std::min(len, 250));
      h.sw[s] = (unsigned char)std::max((int)h.sw[s], (std::min(len, 250) + 1) / 2);
    }
    return too_long ? G10_LIST_LENGTH : G10_FITS;
  }

  // ---- write-out passes: whole rows, as many as fit the tile
  int write_out_passes(Gather10Header &h)
  {
    int np = 0, a = 0;
    h.prow[0] = 0;
    while (a < nrows) {
      int b = a, blocks = 0;
      while (b < nrows) {
        const int len = hp.rowptr[r0 + b + 1] - hp.rowptr[r0 + b];
        if (blocks + len > tile_blocks) break;
        blocks += len; ++b;
      }
      if (b == a || np >= FEA_Q_MAX_PASS) return G10_PASSES;
      h.prow[++np] = (unsigned char)b;
      a = b;
    }
    h.npass = np;
    return G10_FITS;
  }

  // ---- residual lanes: slices of 2*fdw visits of one row
  int residual_lanes(Local &Lc)
  {
    int fdw = 1;
    for (;; ++fdw) {
      int need = 0;
      for (int a = r0; a < r1; ++a) need += std::max(1, (hp.incptr[a + 1] - hp.incptr[a] + 2 * fdw - 1) / (2 * fdw));
      if (need <= FEA_Q_FLANES) break;
      if (2 * fdw >= Q_FENT) return G10_RESIDUAL_LANES;
    }
    int nft = 0;
    for (int a = r0; a < r1; ++a) {
      Lc.rows[Q_FF + (a - r0)] = (uint16_t)nft;
      nft += std::max(1, (hp.incptr[a + 1] - hp.incptr[a] + 2 * fdw - 1) / (2 * fdw));
    }
    Lc.rows[Q_FF + nrows] = (uint16_t)nft;
    Lc.flist.assign((size_t)fdw * 2 * FEA_Q_FLANES, (uint16_t)0xFFFFu);   // no visit: the all-zero record, once its slot is known
    for (int a = r0; a < r1; ++a) {
      const int t0 = Lc.rows[Q_FF + (a - r0)];
      for (int q = hp.incptr[a], k = 0; q < hp.incptr[a + 1]; ++q, ++k) {
        const int le = (int)(std::lower_bound(el.begin(), el.end(), inc_elem(hp.inc_rows[q])) - el.begin());
        const int lane = t0 + k / (2 * fdw), j = k % (2 * fdw);
        Lc.flist[((size_t)(j / 2) * FEA_Q_FLANES + lane) * 2 + (j & 1)] = (uint16_t)(le | (inc_node(hp.inc_rows[q]) << 7));
      }
    }
    Lc.h.nft = nft; Lc.h.fdw = fdw;
    return G10_FITS;
  }
};

// ---- layout: fixed section offsets, sized by the largest chunk; the K tile takes the records' place, so the element
// records are sized by the limit the passes were cut for (elem_cap)
bool lay_out(const std::vector<Local> &loc, int elem_cap, int tile_blocks, HostGather10 &out)
{
  const int nch = (int)loc.size();
  Gather10Layout &lay = out.lay;
  memset(&lay, 0, sizeof(lay));
  for (const Local &Lc : loc) {
    lay.max_elems = std::max(lay.max_elems, Lc.h.nelem);
    int cw = 0;
    for (int s = 0; s < FEA_Q_SLOTS; ++s) cw += Lc.h.sw[s];
    lay.max_cw = std::max(lay.max_cw, cw);
    lay.max_fdw = std::max(lay.max_fdw, Lc.h.fdw);
  }
  lay.max_elems = std::max(lay.max_elems, elem_cap);
  lay.max_cw = std::max(lay.max_cw, 1);
  lay.tile_blocks = tile_blocks;
  lay.o_nodes = 0;
  lay.o_elems = (int)sizeof(Gather10Header);
  lay.o_rows = lay.o_elems + round_up(4 * (FEA_Q_MAX_ELEMS + 1), 64);
  lay.o_tpos = lay.o_rows + round_up(2 * FEA_Q_ROWS_U16, 64);
  lay.o_flist = lay.o_tpos + 4 * Q_MAX_TASKS;
  lay.o_clist = lay.o_flist + round_up(4 * lay.max_fdw * FEA_Q_FLANES, 64);
  lay.stride = round_up(lay.o_clist + 4 * lay.max_cw * FEA_Q_THREADS, 128);
  if ((long long)nch * lay.stride > 0x7FFFFFFF00LL) return false;
  out.blob.assign((size_t)nch * lay.stride, 0);
  parallel_ranges(nch, 256, [&](int lo, int hi) {
    for (int p = lo; p < hi; ++p) {
      const Local &Lc = loc[p];
      unsigned char *rec = out.blob.data() + (size_t)p * lay.stride;
      memcpy(rec, &Lc.h, sizeof(Gather10Header));
      memcpy(rec + lay.o_elems, Lc.elems.data(), Lc.elems.size() * 4);
      memcpy(rec + lay.o_rows, Lc.rows.data(), Lc.rows.size() * 2);
      memcpy(rec + lay.o_tpos, Lc.tpos.data(), Lc.tpos.size() * 4);
      uint16_t *fl = reinterpret_cast<uint16_t *>(rec + lay.o_flist);
      const uint16_t zslot = (uint16_t)lay.max_elems;                     // record max_elems of the LDS tile stays all-zero
      for (int i = 0; i < 2 * lay.max_fdw * FEA_Q_FLANES; ++i) fl[i] = zslot;
      for (size_t i = 0; i < Lc.flist.size(); ++i)
        if (Lc.flist[i] != 0xFFFFu) fl[i] = Lc.flist[i];
      // clist: sw[0] rows of 256 words for the threads' first blocks, then sw[1] rows for their second ones, ...
      uint16_t *cl = reinterpret_cast<uint16_t *>(rec + lay.o_clist);
      for (int i = 0; i < 2 * lay.max_cw * FEA_Q_THREADS; ++i) cl[i] = zslot;
      int row0 = 0;
      for (int s = 0; s < FEA_Q_SLOTS; ++s) {
        for (int t = 0; t < FEA_Q_THREADS; ++t) {
          const std::vector<uint16_t> &l = Lc.lists[(size_t)s * FEA_Q_THREADS + t];
          for (size_t k = 0; k < l.size(); ++k) cl[(((size_t)row0 + k / 2) * FEA_Q_THREADS + t) * 2 + (k & 1)] = l[k];
        }
        row0 += Lc.h.sw[s];
      }
    }
  });
  return true;
}
}  // namespace

void build_host_gather10(int N, int E, int npe, const int *conn, const HostPattern &hp, int row_lo, int row_hi, HostGather10 &out)
{
  (void)E; (void)N;
  out.ok = false; out.nchunks = 0; out.blob.clear(); out.first_row.clear(); out.npe = npe; out.tile_blocks = 0;
  out.limit = G10_OTHER; out.limit_row = -1;
  if (npe < 2 || npe > 15) return;                     // 4-bit local node ids
  if (row_lo < 0 || row_hi > N || row_lo >= row_hi) return;
  // limits of one chunk: two workgroups' records (496 bytes per element) in one CU's LDS
  int max_rows = FEA_Q_MAX_ROWS, max_elems = 127, alpha = 8;
  if (const char *e = getenv("FEAHIP_GATHER10_ROWS")) max_rows = std::max(1, std::min(FEA_Q_MAX_ROWS, atoi(e)));
  if (const char *e = getenv("FEAHIP_GATHER10_ELEMS")) max_elems = std::max(4, std::min(FEA_Q_MAX_ELEMS, atoi(e)));
  if (const char *e = getenv("FEAHIP_GATHER10_ALPHA")) alpha = std::max(0, atoi(e));
  const int tile_blocks = (max_elems * (3 * npe + 1) * 16) / 72 - 1;   // the K tile takes the records' place
  out.tile_blocks = tile_blocks;
  if (!partition(conn, hp, npe, row_lo, row_hi, max_rows, max_elems, alpha, tile_blocks, out)) return;
  const int nch = (int)out.first_row.size() - 1;

  chunk_elements(hp, row_lo, row_hi, out.elist);       // the rank's elements; the state kernel evaluates them in this order
  std::vector<Local> loc((size_t)nch);
  std::vector<char> bad((size_t)nch, 0);
  parallel_ranges(nch, 256, [&](int lo, int hi) {
    ChunkBuilder cb(conn, hp, out.elist, npe, tile_blocks);
    for (int p = lo; p < hi; ++p) bad[p] = (char)cb.build(out.first_row[p], out.first_row[p + 1], loc[p]);
  });
  for (int p = 0; p < nch; ++p)
    if (bad[p]) { out.limit = bad[p]; out.limit_row = out.first_row[p]; return; }

  if (!lay_out(loc, std::max(max_elems, 1), tile_blocks, out)) { out.limit = G10_OTHER; return; }
  out.nchunks = nch;
  out.total_evals = 0;
  for (const Local &Lc : loc) out.total_evals += Lc.h.nelem;
  out.distinct_elems = count_distinct_elems(hp, conn, npe, row_lo, row_hi);
  out.ok = true;
  out.limit = G10_FITS;
}

// Host-only (no device): the edges the 10-node / 8-node maps of a mesh reach, over all chunks (include/fea_hip.h)
extern "C" int feahip_host_gather10_shape(int n_nodes, int n_elems, int npe, const int *elements, long long *out)
{
  if (!elements || !out || n_nodes <= 0 || n_elems <= 0 || (npe != 10 && npe != 8)) return FEAHIP_EINVAL;
  HostPattern hp;
  std::string err;
  int rc = build_host_pattern(n_nodes, n_elems, npe, elements, hp, err);
  if (rc) return rc;
  HostGather10 hg;
  build_host_gather10(n_nodes, n_elems, npe, elements, hp, 0, n_nodes, hg);
  for (int i = 0; i < FEAHIP_G10_SHAPE_LEN; ++i) out[i] = 0;
  out[0] = hg.ok;
  out[1] = hg.ok ? G10_FITS : hg.limit;
  out[13] = -1;
  out[14] = hg.ok ? -1 : hg.limit_row;
  out[10] = hg.tile_blocks;
  if (!hg.ok) return FEAHIP_OK;
  const Gather10Layout &lay = hg.lay;
  std::vector<int> nodes;
  out[2] = hg.nchunks;
  out[6] = FEA_Q_MAX_PASS + 1;
  for (int p = 0; p < hg.nchunks; ++p) {
    const unsigned char *rec = hg.blob.data() + (size_t)p * lay.stride;
    const Gather10Header &h = *reinterpret_cast<const Gather10Header *>(rec);
    const uint32_t *elems = reinterpret_cast<const uint32_t *>(rec + lay.o_elems);
    nodes.clear();
    for (int i = 0; i < h.nelem; ++i)
      for (int k = 0; k < npe; ++k) nodes.push_back(elements[(size_t)hg.elist[elems[i]] * npe + k]);
    std::sort(nodes.begin(), nodes.end());
    const int nnode = (int)(std::unique(nodes.begin(), nodes.end()) - nodes.begin());
    int longest = 0, words = 0;
    for (int s = 0; s < FEA_Q_SLOTS; ++s) {
      words = std::max(words, (int)h.sw[s]);
      for (int w = 0; w < FEA_Q_WAVES; ++w) longest = std::max(longest, (int)h.cnt[FEA_Q_WAVES * s + w]);
    }
    out[3] = std::max(out[3], (long long)h.nelem);
    out[4] = std::max(out[4], (long long)nnode);
    out[5] = std::max(out[5], (long long)h.npass);
    out[6] = std::min(out[6], (long long)h.npass);
    out[7] = std::max(out[7], (long long)longest);
    if (words > FEA_Q_REGW) { ++out[8]; if (out[13] < 0) out[13] = p; }
    out[9] = std::max(out[9], (long long)h.fdw);
    out[11] += h.nelem == FEA_Q_MAX_ELEMS;
    out[15] = std::max(out[15], (long long)(h.r1 - h.r0));
  }
  out[12] = lay.max_elems;
  return FEAHIP_OK;
}
