// gather.cpp -- one-time host construction of the maps of the GATHER assembly
// (kernels_gather.hip) for linear tetrahedra.
//
// The reference scatters every element matrix into a growing sparse matrix
// (sp_matrix_element_add, fea_solver.c:966,1055).  The mesh topology never
// changes, so the scatter is inverted once, here: for every off-diagonal 3x3
// block (a, b) of the matrix the list of (element, local row node, local column
// node) triples that contribute to it, grouped by chunks of consecutive block
// rows so that one workgroup finds everything it needs in one record:
//   header   rows, CSR range, counts
//   nodes    the nodes the chunk's elements touch, owned rows first
//   elems    the distinct elements touching the rows: 4 chunk-local node ids
//   tpos     per block thread: tile position (CSR order inside the chunk) of its block (a, b) and, when b is a
//            row of the chunk too, of the mirror block (b, a) = its transpose (one thread serves both)
//   rows     per row: first tile position, diagonal position, first residual thread
//   vlist    per residual thread a slice of ONE row's (element, local node) visits
//   clist    per block thread its contributions, ascending element order
// Every list is stored thread-minor ("transposed"): word k of thread t sits at
// [k][t], so a wave reads 64 consecutive words.
#include "feahip_internal.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

// ---------------------------------------------------------------------------
// stages shared by the builders of the chunked maps (gather.cpp, gather10.cpp, visits.cpp): where the chunks of
// consecutive block rows start, and what a chunk's rows touch
// ---------------------------------------------------------------------------
int partition_rows(const std::vector<uint16_t> &cost, int row_lo, int row_hi, int L, int alpha, std::vector<int> &first_row)
{
  const int nrows = row_hi - row_lo;
  std::vector<long long> best((size_t)nrows + 1, -1);
  std::vector<unsigned char> from((size_t)nrows + 1, 0);
  best[0] = 0;
  for (int j = 1; j <= nrows; ++j) {
    long long b = -1; int bl = 0;
    for (int l = 1; l <= L && l <= j; ++l) {
      const uint16_t c = cost[(size_t)(j - l) * L + (l - 1)];
      if (c == 0xFFFFu || best[j - l] < 0) continue;
      const long long v = best[j - l] + c + alpha;
      if (b < 0 || v < b) { b = v; bl = l; }
    }
    if (b < 0) return row_lo + j - 1;               // a single row does not fit
    best[j] = b; from[j] = (unsigned char)bl;
  }
  std::vector<int> cuts;
  for (int j = nrows; j > 0; j -= from[j]) cuts.push_back(row_lo + j);
  cuts.push_back(row_lo);
  first_row.assign(cuts.rbegin(), cuts.rend());
  return -1;
}

void chunk_elements(const HostPattern &hp, int r0, int r1, std::vector<int> &el)
{
  el.clear();
  for (int q = hp.incptr[r0]; q < hp.incptr[r1]; ++q) el.push_back(inc_elem(hp.inc_rows[q]));
  std::sort(el.begin(), el.end());
  el.erase(std::unique(el.begin(), el.end()), el.end());
}

void chunk_block_tasks(const HostPattern &hp, int r0, int r1, std::vector<uint32_t> &tpos, std::vector<int> &task_of)
{
  const int b0 = hp.rowptr[r0];
  tpos.clear();
  task_of.assign((size_t)(hp.rowptr[r1] - b0), -1);
  for (int a = r0; a < r1; ++a)
    for (int q = hp.rowptr[a]; q < hp.rowptr[a + 1]; ++q) {
      const int b = hp.colidx[q];
      if (b == a || (b >= r0 && b < a)) continue;
      const uint32_t m = b > a && b < r1 ? (uint32_t)(csr_pos(hp, b, a) - b0) : 0xFFFFu;
      task_of[q - b0] = (int)tpos.size();
      tpos.push_back((uint32_t)(q - b0) | m << 16);
    }
}

void chunk_block_lists(const HostPattern &hp, const int *conn, int npe, int r0, int r1, const std::vector<int> &el,
                       const std::vector<int> &task_of, int ntask, int la_shift, int lb_shift,
                       std::vector<std::vector<uint16_t>> &lists)
{
  const int b0 = hp.rowptr[r0];
  lists.assign((size_t)ntask, std::vector<uint16_t>());
  for (int a = r0; a < r1; ++a)
    for (int q = hp.incptr[a]; q < hp.incptr[a + 1]; ++q) {
      const int e = inc_elem(hp.inc_rows[q]), la = inc_node(hp.inc_rows[q]);
      const int le = (int)(std::lower_bound(el.begin(), el.end(), e) - el.begin());
      for (int lb = 0; lb < npe; ++lb) {
        if (lb == la) continue;
        const int b = conn[(size_t)e * npe + lb];
        if (b == a) continue;                       // degenerate element (repeated node): no off-diagonal block
        const int t = task_of[csr_pos(hp, a, b) - b0];
        if (t < 0) continue;                        // served by the mirror block's thread
        lists[(size_t)t].push_back((uint16_t)(le | la << la_shift | lb << lb_shift));
      }
    }
}

long long count_distinct_elems(const HostPattern &hp, const int *conn, int npe, int r0, int r1)
{
  long long d = 0;
  for (int a = r0; a < r1; ++a)                     // counted at its lowest-numbered node inside the range
    for (int q = hp.incptr[a]; q < hp.incptr[a + 1]; ++q) d += first_visit(hp, conn, npe, hp.inc_rows[q], r0, a);
  return d;
}

// u16 offsets inside the "rows" section
#define G_RS 0                        // rstart[MAX_ROWS + 1]
#define G_RD 66                       // rdiag[MAX_ROWS]
#define G_VF 130                      // vfirst[MAX_ROWS + 1]
#define G_ROWS_U16 200
#define G_TASK_THREADS FEA_G_TASK_THREADS   // block and residual threads; the remaining waves sum the diagonal blocks
#define G_SLOT(w) ((w) & 1023u)
#define G_LA(w) (((w) >> 10) & 3)
#define G_LB(w) (((w) >> 12) & 3)
#define G_NGROUPS (FEA_G_THREADS / 16) // 16-lane groups of a workgroup's ds_read_b128

namespace {
// the 16-lane group a ds_read_b128 serves thread t in (MI355X_MICROARCH: {0-3,12-15,20-27}, {4-11,16-19,28-31}, and
// the same pattern in the upper half of the wave), numbered over the whole workgroup
inline int b128_group(int t)
{
  static const unsigned char g32[32] = {0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1};
  return (t >> 6) * 4 + ((t >> 5) & 1) * 2 + g32[t & 31];
}

// ---- pass A: chunk boundaries (partition_rows).  Limits of one chunk: its rows, its nodes, its block and residual
// threads, and the element records one CU's LDS holds (a lattice's bricks stop at the row limit with
// FEA_G_ELEMS_TARGET elements whatever the element limit is -- its partition is the same for 672 and 719, checked on
// the 31^3, 40^3 and 66^3 blocks; an unstructured mesh uses the room: 2-3 % fewer chunks)
bool partition(int N, const int *conn, const HostPattern &hp, int row_lo, int row_hi, std::vector<int> &first_row)
{
  int max_rows = FEA_G_MAX_ROWS, max_elems = FEA_G_BIG == 1 ? FEA_G_MAX_ELEMS : FEA_G_ELEMS_TARGET, alpha = 24;
  if (const char *e = getenv("FEAHIP_GATHER_ROWS")) max_rows = std::max(1, std::min(FEA_G_MAX_ROWS, atoi(e)));
  if (const char *e = getenv("FEAHIP_GATHER_ELEMS")) max_elems = std::max(8, std::min(FEA_G_MAX_ELEMS, atoi(e)));
  if (const char *e = getenv("FEAHIP_GATHER_ALPHA")) alpha = std::max(0, atoi(e));
  const int L = max_rows, nrows = row_hi - row_lo;
  std::vector<uint16_t> cost((size_t)nrows * L, 0xFFFFu);
  parallel_ranges(nrows, 4096, [&](int lo, int hi) {
    std::vector<int> nstamp((size_t)N, -1), fresh;
    for (int i = lo; i < hi; ++i) {
      const int r0 = row_lo + i;
      int nnod = 0, nvis = 0;
      chunk_costs(hp, conn, 4, r0, row_hi, L, fresh, &cost[(size_t)i * L], [&](int r, int l, int nel, int ntask, const std::vector<int> &fr) {
        if (nstamp[r] != r0) { nstamp[r] = r0; ++nnod; }
        for (int e : fr)
          for (int k = 0; k < 4; ++k) {
            const int g = conn[(size_t)e * 4 + k];
            if (nstamp[g] != r0) { nstamp[g] = r0; ++nnod; }
          }
        nvis += hp.incptr[r + 1] - hp.incptr[r];
        return nel <= (l > 1 ? max_elems : FEA_G_MAX_ELEMS) && nnod <= FEA_G_MAX_NODES && ntask <= G_TASK_THREADS &&
               nvis <= 4 * G_TASK_THREADS;
      });
    }
  });
  return partition_rows(cost, row_lo, row_hi, L, alpha, first_row) < 0;   // else no gather assembly for this mesh
}

struct Read { uint16_t set; uint8_t off; };     // one LDS read of a record: (lane group, step, kind) and its piece

void sort_unique(std::vector<Read> &rv)             // an item read twice in one set at one piece is one address (a broadcast)
{
  std::sort(rv.begin(), rv.end(), [](const Read &a, const Read &b) { return a.set != b.set ? a.set < b.set : a.off < b.off; });
  rv.erase(std::unique(rv.begin(), rv.end(), [](const Read &a, const Read &b) { return a.set == b.set && a.off == b.off; }), rv.end());
}

void most_read_first(const std::vector<std::vector<Read>> &reads, std::vector<int> &order)
{
  order.resize(reads.size());
  for (size_t i = 0; i < reads.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return reads[a].size() > reads[b].size(); });
}

// LDS slots of items read with ds_read_b128, served in groups of 16 lanes over 16 bank slots of 16 bytes: lanes of
// a group that read different addresses in one bank slot serialise.  Piece `off` of the item in LDS slot s sits in
// bank slot (off + step s) mod 16, so which reads collide is decided by s mod 16 alone: the residue of every item
// is chosen greedily against the reads already placed (items in `order`), then once more with everything in place,
// and the items of residue r take the slots r, r + 16, ... in item order.  reads[i]: the distinct reads of item i;
// cap[r]: the slots of residue r the items may take.
void bank_slots(const std::vector<std::vector<Read>> &reads, const std::vector<int> &order, int nsets, int step,
                std::vector<int> cap, std::vector<uint8_t> &occ, std::vector<int> &res, std::vector<int> &slot)
{
  const int n = (int)reads.size();
  occ.assign((size_t)nsets * 16, 0);
  res.assign((size_t)n, -1);
  auto bank = [&](const Read &rd, int r) { return (size_t)rd.set * 16 + ((rd.off + step * r) & 15); };
  for (int pass = 0; pass < 2; ++pass)
    for (int i : order) {
      if (res[i] >= 0) {
        for (const Read &rd : reads[i]) --occ[bank(rd, res[i])];
        ++cap[res[i]];
      }
      int br = -1; long bc = 0;
      for (int r = 0; r < 16; ++r) {
        if (cap[r] <= 0) continue;
        long c = 0;
        for (const Read &rd : reads[i]) c += occ[bank(rd, r)];
        if (br < 0 || c < bc) { br = r; bc = c; }
      }
      res[i] = br; --cap[br];
      for (const Read &rd : reads[i]) ++occ[bank(rd, br)];
    }
  int next[16];
  for (int r = 0; r < 16; ++r) next[r] = r;
  slot.resize((size_t)n);
  for (int i = 0; i < n; ++i) { slot[i] = next[res[i]]; next[res[i]] += 16; }
}

struct Local {                                      // a chunk's record, before the layout is known
  GatherHeader h;
  std::vector<int> nodes;
  std::vector<uint32_t> elems, tpos;
  std::vector<uint16_t> rows, vlist, clist, dlist;
  std::vector<uint8_t> emat;                        // material id per element slot (a context with a material table only)
};

// ---- pass B: one chunk's record, stage by stage; one per parallel_ranges worker, its vectors reused chunk after chunk
struct ChunkBuilder {
  const int *conn;
  const HostPattern &hp;
  const uint8_t *elem_mat;                          // [E] material ids, null without a material table
  int r0 = 0, r1 = 0, nrows = 0, b0 = 0, nb = 0, nelem = 0, nnode = 0, nslots = 0, nnslots = 0;
  int ntask = 0, wdepth[G_TASK_THREADS / 64] = {0}, dwords = 0, ddwords = 0, zslot = 0;
  std::vector<int> el, nd, task_of, thr_blk, order, res, eslot, nslot;
  std::vector<uint32_t> btpos;
  std::vector<std::vector<uint16_t>> blists, lists, dl;
  std::vector<std::vector<Read>> reads;
  std::vector<uint8_t> occ;

  ChunkBuilder(const int *c, const HostPattern &p, const uint8_t *em) : conn(c), hp(p), elem_mat(em) {}
  int lnode(int g) const { return (int)(std::lower_bound(nd.begin(), nd.end(), g) - nd.begin()); }
  int lelem(int e) const { return (int)(std::lower_bound(el.begin(), el.end(), e) - el.begin()); }

  bool build(int row0, int row1, Local &L)
  {
    r0 = row0; r1 = row1; nrows = r1 - r0; b0 = hp.rowptr[r0]; nb = hp.rowptr[r1] - b0;
    if (!chunk_lists(L)) return false;
    deal();
    bank_schedule();
    emit(L);
    return true;
  }

  // ---- the chunk's elements, nodes, blocks with a thread and their contributions, and per row the visits of its
  // diagonal block (four lanes of the last waves per row: a row's diagonal block is summed from the records like
  // any other block, K_aa = sum_e K_aa^e)
  bool chunk_lists(Local &L)
  {
    chunk_elements(hp, r0, r1, el);
    nd.clear();
    for (int a = r0; a < r1; ++a) nd.push_back(a);          // a node no element refers to still owns a (diagonal) row
    for (int e : el)
      for (int k = 0; k < 4; ++k) nd.push_back(conn[(size_t)e * 4 + k]);
    std::sort(nd.begin(), nd.end());
    nd.erase(std::unique(nd.begin(), nd.end()), nd.end());
    nnode = (int)nd.size(); nelem = (int)el.size();
    nslots = 16 * ((nelem + 1 + 15) / 16); nnslots = 16 * ((nnode + 15) / 16);
    if (nnslots > FEA_G_MAX_NODES || nslots > FEA_G_MAX_SLOTS || nrows > FEA_G_MAX_ROWS) return false;
    L.rows.assign(G_ROWS_U16, 0);
    for (int a = r0; a < r1; ++a) {
      L.rows[G_RS + (a - r0)] = (uint16_t)(hp.rowptr[a] - b0);
      L.rows[G_RD + (a - r0)] = (uint16_t)(hp.diag[a] - b0);
    }
    L.rows[G_RS + nrows] = (uint16_t)nb;
    // which THREAD serves which block is decided by deal(), once the lists are known
    chunk_block_tasks(hp, r0, r1, btpos, task_of);
    const int nblk = (int)btpos.size();
    if (nblk > G_TASK_THREADS) return false;
    chunk_block_lists(hp, conn, 4, r0, r1, el, task_of, nblk, 10, 12, blists);
    dl.assign((size_t)4 * FEA_G_MAX_ROWS, std::vector<uint16_t>());
    for (int a = r0; a < r1; ++a)
      for (int q = hp.incptr[a], kv = 0; q < hp.incptr[a + 1]; ++q, ++kv)
        dl[(size_t)4 * (a - r0) + (kv & 3)].push_back((uint16_t)(lelem(inc_elem(hp.inc_rows[q])) | (inc_node(hp.inc_rows[q]) << 10)));
    return true;
  }

  // ---- which thread serves which block.  A wave walks its lists to the depth of its LONGEST one (empty entries
  // read the all-zero record), and the gather phase lasts as long as its busiest SIMD: in CSR order every wave
  // of a Kuhn block mixes blocks of 4 and of 6 contributions and walks 6, and ten block waves over four SIMDs
  // are 3 + 3 + 2 + 2.  So (i) the blocks are sorted by list length, a wave holds lists of (nearly) one length and
  // stops at its own depth (GatherHeader::wdepth); (ii) the waves are dealt to the wave slots so that the four
  // SIMDs carry equal sums of depths -- a workgroup's waves go to the SIMDs cyclically, slot w runs on SIMD
  // (w + start) mod 4, and the slots s, s+4, s+8 of the block waves share one (longest wave first, to the
  // lightest SIMD with a free slot); (iii) inside a wave sixteen consecutive lanes (one group of the tile
  // phase's ds_write_b64) get tile positions that differ mod 16, mirrors too where possible: a block is nine
  // doubles, so two blocks meet in a bank exactly when their positions agree mod 16.
  void deal()
  {
    constexpr int NBW = G_TASK_THREADS / 64;
    const int nblk = (int)btpos.size();
    thr_blk.assign((size_t)G_TASK_THREADS, -1);
    std::fill(wdepth, wdepth + NBW, 0);
    ntask = 0;
    auto words = [&](int i) { return ((int)blists[i].size() + 1) / 2; };
    order.resize((size_t)nblk);
    for (int i = 0; i < nblk; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return words(x) > words(y); });
    // sixteens with distinct tile positions mod 16, class by class (a class = one list length in words)
    std::vector<int> seq;
    seq.reserve((size_t)nblk);
    for (size_t c0 = 0; c0 < order.size();) {
      size_t c1 = c0;
      while (c1 < order.size() && words(order[c1]) == words(order[c0])) ++c1;
      std::vector<int> bucket[16];
      for (size_t k = c0; k < c1; ++k) bucket[btpos[order[k]] & 15u].push_back(order[k]);
      size_t left = c1 - c0;
      while (left) {
        // finish the sixteen the previous class may have left open, then whole sixteens
        const int room = 16 - (int)(seq.size() & 15);
        int rs[16];
        for (int r = 0; r < 16; ++r) rs[r] = r;
        std::stable_sort(rs, rs + 16, [&](int x, int y) { return bucket[x].size() > bucket[y].size(); });
        unsigned mused = 0;
        int taken = 0;
        for (int pass = 0; pass < 2 && taken < room && left; ++pass)      // pass 1: a second block of a residue, if the sixteen would stay short
          for (int q = 0; q < 16 && taken < room && left; ++q) {
            std::vector<int> &bk = bucket[rs[q]];
            if (bk.empty()) continue;
            size_t pick = 0;                                              // prefer a mirror position not yet in the sixteen
            for (size_t c = 0; c < bk.size() && c < 8; ++c) {
              const unsigned mp = btpos[bk[c]] >> 16;
              if (mp == 0xFFFFu || !((mused >> (mp & 15u)) & 1u)) { pick = c; break; }
            }
            const unsigned mp = btpos[bk[pick]] >> 16;
            if (mp != 0xFFFFu) mused |= 1u << (mp & 15u);
            seq.push_back(bk[pick]);
            bk.erase(bk.begin() + (long)pick);
            ++taken; --left;
          }
      }
      c0 = c1;
    }
    const int nwaves = (nblk + 63) / 64;
    std::vector<int> wcost((size_t)nwaves, 0), word((size_t)nwaves);
    for (int w = 0; w < nwaves; ++w) {
      for (int l = 0; l < 64 && w * 64 + l < nblk; ++l) wcost[w] = std::max(wcost[w], words(seq[(size_t)w * 64 + l]));
      word[w] = w;
    }
    std::stable_sort(word.begin(), word.end(), [&](int x, int y) { return wcost[x] > wcost[y]; });
    int load[4] = {0, 0, 0, 0}, used[4] = {0, 0, 0, 0};
    for (int w : word) {
      int bs = -1;
      for (int sd = 0; sd < 4; ++sd)
        if (used[sd] * 4 + sd < NBW && (bs < 0 || load[sd] < load[bs])) bs = sd;
      const int slot = used[bs] * 4 + bs;
      ++used[bs]; load[bs] += wcost[w];
      wdepth[slot] = wcost[w];
      for (int l = 0; l < 64 && w * 64 + l < nblk; ++l) thr_blk[(size_t)slot * 64 + l] = seq[(size_t)w * 64 + l];
      ntask = std::max(ntask, slot * 64 + std::min(64, nblk - w * 64));
    }
    lists.assign((size_t)ntask, std::vector<uint16_t>());         // a thread without a block: empty lists
    for (int t = 0; t < ntask; ++t)
      if (thr_blk[t] >= 0) lists[t] = blists[thr_blk[t]];
    int depth = 0, ddepth = 0;
    for (auto &l : lists) depth = std::max(depth, (int)l.size());
    for (auto &l : dl) ddepth = std::max(ddepth, (int)l.size());
    dwords = (depth + 1) / 2; ddwords = (ddepth + 1) / 2;
  }

  // ---- LDS bank schedule.  A record is 13 pieces of 16 bytes (kernels_gather.hip) and every read of it is a
  // ds_read_b128: the slot of piece `off` of the record in element slot s is (13 s + off) mod 16 = (off - 3 s) mod 16,
  // most-read elements first.  PMC before: 41 % of the kernel's LDS cycles were bank conflicts.
  void bank_schedule()
  {
    reads.assign((size_t)nelem, std::vector<Read>());
    const int nsteps = std::max(2 * dwords, 2 * ddwords);
    auto add_reads = [&](int lane, int step, uint16_t w, bool diag) {
      const int le = (int)G_SLOT(w), la = G_LA(w), lb = G_LB(w);
      const int grp = b128_group(lane);
      // kinds: 0 P_a, 1 Z_a, 2 P_b, 3 Q_b, 4 Z_b, 5 VV   (diagonal visit: P_a, Z_a, Q_a, VV)
      const int offs[6] = {la, 8 + la, diag ? 4 + la : lb, diag ? -1 : 4 + lb, diag ? -1 : 8 + lb, 12};
      for (int kind = 0; kind < 6; ++kind)
        if (offs[kind] >= 0) reads[le].push_back({(uint16_t)((grp * nsteps + step) * 6 + kind), (uint8_t)offs[kind]});
    };
    for (int t = 0; t < ntask; ++t)
      for (size_t k = 0; k < lists[t].size(); ++k) add_reads(t, (int)k, lists[t][k], false);
    for (int l = 0; l < 4 * nrows; ++l)
      for (size_t k = 0; k < dl[l].size(); ++k) add_reads(G_TASK_THREADS + l, (int)k, dl[l][k], true);
    most_read_first(reads, order);
    for (auto &rv : reads) sort_unique(rv);
    std::vector<int> cap(16, nslots / 16);
    --cap[15];                                    // one slot stays empty: the all-zero record of the unused list slots
    bank_slots(reads, order, G_NGROUPS * nsteps * 6, -3, cap, occ, res, eslot);
    std::vector<char> used((size_t)nslots, 0);
    for (int e = 0; e < nelem; ++e) used[eslot[e]] = 1;
    zslot = 0;
    while (used[zslot]) ++zslot;

    // node slots: the state phase reads the four nodes of the element in slot t from lane t, again 16 lanes per
    // group over 16 slots of 16 bytes; same greedy (lane group x 4 node positions, bank slot = node slot mod 16)
    reads.assign((size_t)nnode, std::vector<Read>());
    for (int e = 0; e < nelem; ++e)
      for (int k = 0; k < 4; ++k) reads[lnode(conn[(size_t)el[e] * 4 + k])].push_back({(uint16_t)(b128_group(eslot[e]) * 4 + k), 0});
    for (auto &rv : reads) sort_unique(rv);
    most_read_first(reads, order);
    bank_slots(reads, order, G_NGROUPS * 4, 1, std::vector<int>(16, nnslots / 16), occ, res, nslot);
  }

  // ---- the record with the slots
  void emit(Local &L)
  {
    L.nodes.assign((size_t)nnslots, 0);           // unused slots: node 0 (their coordinates are loaded and never read)
    for (int i = 0; i < nnode; ++i) L.nodes[nslot[i]] = nd[i];
    L.elems.assign((size_t)nslots, 0xFFFFFFFFu);  // unused slots stay all-zero records
    for (int i = 0; i < nelem; ++i) {
      uint32_t w = 0;
      for (int k = 0; k < 4; ++k) w |= (uint32_t)nslot[lnode(conn[(size_t)el[i] * 4 + k])] << (8 * k);
      L.elems[eslot[i]] = w;
    }
    L.emat.clear();
    if (elem_mat) {                               // unused slots: material 0 (loaded, never used)
      L.emat.assign((size_t)nslots, 0);
      for (int i = 0; i < nelem; ++i) L.emat[eslot[i]] = elem_mat[el[i]];
    }
    L.tpos.assign((size_t)ntask, 0xFFFFFFFFu);    // a thread without a block: no tile position
    for (int t = 0; t < ntask; ++t)
      if (thr_blk[t] >= 0) L.tpos[t] = btpos[thr_blk[t]];
    auto reslot = [&](uint16_t w) { return (uint16_t)((w & 0xFC00u) | (uint16_t)eslot[G_SLOT(w)]); };
    L.clist.assign((size_t)dwords * 2 * FEA_G_THREADS, (uint16_t)zslot);
    for (int t = 0; t < ntask; ++t)
      for (size_t k = 0; k < lists[t].size(); ++k)
        L.clist[((size_t)(k / 2) * FEA_G_THREADS + t) * 2 + (k & 1)] = reslot(lists[t][k]);
    L.dlist.assign((size_t)ddwords * 2 * FEA_G_DIAG_LANES, (uint16_t)zslot);
    for (int l = 0; l < 4 * nrows; ++l)
      for (size_t k = 0; k < dl[l].size(); ++k)
        L.dlist[((size_t)(k / 2) * FEA_G_DIAG_LANES + l) * 2 + (k & 1)] = reslot(dl[l][k]);
    // residual threads (waves 0-2): slices of vdepth visits of one row
    int vdepth = 1;
    for (;; ++vdepth) {
      int need = 0;
      for (int a = r0; a < r1; ++a) need += (hp.incptr[a + 1] - hp.incptr[a] + vdepth - 1) / vdepth;
      if (need <= G_TASK_THREADS) break;
    }
    int nvthr = 0;
    for (int a = r0; a < r1; ++a) {
      L.rows[G_VF + (a - r0)] = (uint16_t)nvthr;
      nvthr += (hp.incptr[a + 1] - hp.incptr[a] + vdepth - 1) / vdepth;
    }
    L.rows[G_VF + nrows] = (uint16_t)nvthr;
    L.vlist.assign((size_t)vdepth * FEA_G_THREADS, (uint16_t)zslot);
    for (int a = r0; a < r1; ++a) {
      const int t0 = L.rows[G_VF + (a - r0)];
      for (int q = hp.incptr[a], k = 0; q < hp.incptr[a + 1]; ++q, ++k)
        L.vlist[(size_t)(k % vdepth) * FEA_G_THREADS + t0 + k / vdepth] = (uint16_t)(eslot[lelem(inc_elem(hp.inc_rows[q]))] | (inc_node(hp.inc_rows[q]) << 10));
    }
    GatherHeader &h = L.h;
    memset(&h, 0, sizeof(h));
    h.r0 = r0; h.r1 = r1; h.b0 = b0; h.nb = nb; h.nnode = nnslots; h.nelem = nslots; h.noffd = ntask;
    h.depth = dwords; h.nvthr = nvthr; h.vdepth = vdepth; h.ddepth = ddwords;
    for (int w = 0; w < G_TASK_THREADS / 64; ++w) h.wdepth[w >> 2] |= (unsigned)std::min(wdepth[w], 255) << (8 * (w & 3));
  }
};

// ---- layout: fixed section offsets, sized by the largest chunk; the records in walk order (walk[i]: the chunk, in row
// order, whose record is the i-th of the blob)
bool lay_out(const std::vector<Local> &loc, const std::vector<int> &walk, bool materials, HostGather &out)
{
  const int nch = (int)loc.size();
  int m_v = 0, m_c = 0, m_d = 0, g_nodes = 0, g_elems = 0, g_tile = 0;
  GatherLayout &lay = out.lay;
  memset(&lay, 0, sizeof(lay));
  for (const Local &L : loc) {
    m_v = std::max(m_v, (int)L.vlist.size() * 2); m_c = std::max(m_c, (int)L.clist.size() * 2); m_d = std::max(m_d, (int)L.dlist.size() * 2);
    g_nodes = std::max(g_nodes, L.h.nnode); g_elems = std::max(g_elems, L.h.nelem); g_tile = std::max(g_tile, L.h.nb);
    lay.max_tasks = std::max(lay.max_tasks, L.h.noffd); lay.max_depth = std::max(lay.max_depth, L.h.depth);
    lay.max_vthr = std::max(lay.max_vthr, L.h.nvthr); lay.max_vdepth = std::max(lay.max_vdepth, L.h.vdepth);
    lay.max_ddepth = std::max(lay.max_ddepth, L.h.ddepth);
  }
  lay.max_nodes = g_nodes; lay.max_elems = g_elems; lay.max_tile = g_tile;
  lay.o_nodes = 64;
  lay.o_elems = lay.o_nodes + round_up(4 * FEA_G_MAX_NODES, 64);
  lay.o_bpos = lay.o_elems + round_up(4 * FEA_G_THREADS, 64);
  lay.o_rows = lay.o_bpos + round_up(4 * FEA_G_THREADS, 64);
  lay.o_vlist = lay.o_rows + round_up(2 * G_ROWS_U16, 64);
  lay.o_dlist = lay.o_vlist + round_up(m_v, 64);
  lay.o_clist = lay.o_dlist + round_up(m_d, 64);
  lay.stride = round_up(lay.o_clist + m_c, 128);
  // the optional last section, one material id per element slot: behind everything else, so that the offsets (and,
  // without a material table, the stride and the bytes) of the other sections are what they are without it
  if (materials) { lay.o_emat = lay.stride; lay.stride += round_up(FEA_G_THREADS, 128); }   // (a byte per thread: the kernel indexes it by its thread id)
  if ((long long)nch * lay.stride > 0x7FFFFFFF00LL) return false;
  out.blob.assign((size_t)nch * lay.stride, 0);
  parallel_ranges(nch, 512, [&](int lo, int hi) {
    for (int p = lo; p < hi; ++p) {
      const Local &L = loc[walk[p]];
      unsigned char *rec = out.blob.data() + (size_t)p * lay.stride;
      memcpy(rec, &L.h, sizeof(GatherHeader));
      memcpy(rec + lay.o_nodes, L.nodes.data(), L.nodes.size() * 4);
      memcpy(rec + lay.o_elems, L.elems.data(), L.elems.size() * 4);
      memcpy(rec + lay.o_bpos, L.tpos.data(), L.tpos.size() * 4);
      memcpy(rec + lay.o_rows, L.rows.data(), L.rows.size() * 2);
      memcpy(rec + lay.o_vlist, L.vlist.data(), L.vlist.size() * 2);
      memcpy(rec + lay.o_dlist, L.dlist.data(), L.dlist.size() * 2);
      memcpy(rec + lay.o_clist, L.clist.data(), L.clist.size() * 2);
      if (lay.o_emat) memcpy(rec + lay.o_emat, L.emat.data(), L.emat.size());
    }
  });
  return true;
}

// a chunk whose successor IN WALK ORDER has the same map words (chunk-local indices only: the interior bricks of a
// structured block are all alike) says so in its header: the kernel then keeps the words in registers instead of loading them
void mark_repeats(HostGather &out, int nch)
{
  const GatherLayout &lay = out.lay;
  out.same_as_previous = 0;
  for (int p = 0; p + 1 < nch; ++p) {
    const unsigned char *r0 = out.blob.data() + (size_t)p * lay.stride, *r1 = r0 + lay.stride;
    const GatherHeader &h0 = *reinterpret_cast<const GatherHeader *>(r0), &h1 = *reinterpret_cast<const GatherHeader *>(r1);
    const bool same = h0.nelem == h1.nelem && h0.noffd == h1.noffd && h0.depth == h1.depth && h0.nvthr == h1.nvthr &&
                      h0.vdepth == h1.vdepth && h0.ddepth == h1.ddepth && h0.r1 - h0.r0 == h1.r1 - h1.r0 &&
                      memcmp(r0 + lay.o_elems, r1 + lay.o_elems, (size_t)((lay.o_emat ? lay.o_emat : lay.stride) - lay.o_elems)) == 0;   // (the material ids are no map words: the kernel loads them for every chunk)
    if (same) { reinterpret_cast<GatherHeader *>(out.blob.data() + (size_t)p * lay.stride)->flags |= 1; ++out.same_as_previous; }
  }
}
}  // namespace

// ---------------------------------------------------------------------------
// The walk: which chunks a workgroup works on, and in what order.  A workgroup walks one RUN, a contiguous range of
// the blob's records; the records are self-describing (rows, CSR range), so their place in the blob is free.
//   * runs cut by cost: the launch lasts as long as its most expensive run, and chunks are not equally expensive (the
//     face and partial bricks of a block evaluate fewer elements and write fewer blocks than an interior brick);
//   * equal chunks adjacent: inside a run the chunks with byte-identical map words follow one another, so that all
//     but the first of them run with the words their predecessor left in registers.
// Both are decided here, once; neither changes a sum (every chunk computes what it computed, whoever walks it).
// ---------------------------------------------------------------------------
// Modelled cost of one chunk in shader cycles of the K-and-f kernel, from what the builder knows: a regression of the
// in-kernel stamps' per-run totals (diagnostic build, 66 x 396 x 66 block on an MI355X; 254 equal-count runs in row order
// and 256 cost-cut grouped runs fitted together, rms residual 5 000 cycles = 0.35 % of a run; tools/gather_run_costs.py,
// DESIGN.md section 4) on the runs' sums of
//   element waves   the state phase: waves of 64 element slots
//   list words      the gather phase: the contribution words walked by the busiest SIMD's block waves (wave slots s, s + 4,
//                   s + 8 share a SIMD, GatherHeader::wdepth) and by a diagonal wave (ddepth)
//   blocks          tile writes and row write-out
//   words           a chunk whose successor cannot keep its map words requests them behind its state phase
// Rows, elements and blocks of a brick shrink together, so the coefficients predict a chunk (interior brick 13 250, face
// brick 12 500, 48-row partial brick 10 570 cycles measured; 13 210 / 12 590 / 10 640 modelled) and are NOT phase times.
// Not measured: G_COST_LONG (a list word beyond the registers is fetched inside the gather phase: DESIGN.md's "one exposed
// HBM round trip per word"), G_COST_RUN (the prologue: two dependent latencies with nothing to hide behind), and the
// diagonal words apart from the block words (every chunk of the block has three).
#ifndef G_WALK_ORDER
#define G_WALK_ORDER 1                // defaults of FEAHIP_GATHER_ORDER / FEAHIP_GATHER_BALANCE
#endif
#ifndef G_WALK_BALANCE
#define G_WALK_BALANCE 1
#endif
#define G_COST_CHUNK 4930
#define G_COST_ELEM_WAVE 103
#define G_COST_LIST_WORD 92
#define G_COST_2_BLOCKS 13
#define G_COST_WORDS 1123
#define G_COST_LONG 2000
#define G_COST_RUN 4000
int gather_chunk_cost(const GatherHeader &h, bool loads_words)
{
  int simd[4] = {0, 0, 0, 0};
  for (int w = 0; w < G_TASK_THREADS / 64; ++w) simd[w & 3] += (int)((h.wdepth[w >> 2] >> (8 * (w & 3))) & 255u);
  const int gwords = std::max(std::max(simd[0], simd[1]), std::max(simd[2], simd[3]));
  const int over = std::max(0, h.depth - FEA_G_REGW) + std::max(0, h.ddepth - FEA_G_REGW);
  return G_COST_CHUNK + G_COST_ELEM_WAVE * ((h.nelem + 63) / 64) + G_COST_LIST_WORD * (gwords + h.ddepth) + G_COST_2_BLOCKS * h.nb / 2 +
         G_COST_LONG * over + (loads_words ? G_COST_WORDS : 0);
}

namespace {
inline unsigned long long hash_words(unsigned long long h, const void *p, size_t bytes)
{
  const unsigned char *b = static_cast<const unsigned char *>(p);
  size_t i = 0;
  for (; i + 8 <= bytes; i += 8) { unsigned long long v; memcpy(&v, b + i, 8); h = (h ^ v) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; }
  for (; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
  return h;
}
// what mark_repeats compares, before the layout: the header's shape and every word section
bool same_words(const Local &a, const Local &b)
{
  return a.h.nelem == b.h.nelem && a.h.noffd == b.h.noffd && a.h.depth == b.h.depth && a.h.nvthr == b.h.nvthr && a.h.vdepth == b.h.vdepth &&
         a.h.ddepth == b.h.ddepth && a.h.r1 - a.h.r0 == b.h.r1 - b.h.r0 && a.elems == b.elems && a.tpos == b.tpos && a.rows == b.rows &&
         a.vlist == b.vlist && a.dlist == b.dlist && a.clist == b.clist;
}
// kind[p]: chunks with byte-identical map words share a number (a hash finds the candidates, the bytes decide)
void word_kinds(const std::vector<Local> &loc, std::vector<int> &kind)
{
  const int nch = (int)loc.size();
  std::vector<unsigned long long> hs((size_t)nch);
  parallel_ranges(nch, 512, [&](int lo, int hi) {
    for (int p = lo; p < hi; ++p) {
      const Local &L = loc[p];
      const int shape[7] = {L.h.nelem, L.h.noffd, L.h.depth, L.h.nvthr, L.h.vdepth, L.h.ddepth, L.h.r1 - L.h.r0};
      unsigned long long h = hash_words(0xCBF29CE484222325ull, shape, sizeof(shape));
      h = hash_words(h, L.elems.data(), L.elems.size() * 4); h = hash_words(h, L.tpos.data(), L.tpos.size() * 4);
      h = hash_words(h, L.rows.data(), L.rows.size() * 2); h = hash_words(h, L.vlist.data(), L.vlist.size() * 2);
      h = hash_words(h, L.dlist.data(), L.dlist.size() * 2); h = hash_words(h, L.clist.data(), L.clist.size() * 2);
      hs[p] = h;
    }
  });
  std::vector<int> idx((size_t)nch);
  for (int p = 0; p < nch; ++p) idx[p] = p;
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return hs[a] < hs[b]; });
  kind.assign((size_t)nch, -1);
  int nkinds = 0;
  for (int i = 0; i < nch;) {
    int j = i;
    while (j < nch && hs[idx[j]] == hs[idx[i]]) ++j;
    std::vector<int> reps;                            // one representative per kind among the chunks of this hash
    for (int q = i; q < j; ++q) {
      const int p = idx[q];
      for (int r : reps)
        if (same_words(loc[r], loc[p])) { kind[p] = kind[r]; break; }
      if (kind[p] < 0) { kind[p] = nkinds++; reps.push_back(p); }
    }
    i = j;
  }
}

struct WalkCost {                                    // the cost of a chunk where it stands in a run
  const std::vector<int> &base, &kind;
  bool grouped;                                      // the run's chunks will be grouped by kind (else: row order)
  std::vector<int> seen;                             // kind -> the last run it was met in
  WalkCost(const std::vector<int> &b, const std::vector<int> &k, bool g) : base(b), kind(k), grouped(g), seen(b.size(), -1) {}
  // chunk p joining run `run` that began at chunk s: its predecessor there requests p's words unless it holds them
  int add(int p, int s, int run)
  {
    int c = base[p];
    if (p > s && (grouped ? seen[kind[p]] != run : kind[p] != kind[p - 1])) c += G_COST_WORDS;
    seen[kind[p]] = run;
    return c;
  }
};

// runs of at most `cap` modelled cycles, greedily; returns their number
int fill_runs(const std::vector<int> &base, const std::vector<int> &kind, bool grouped, long long cap, std::vector<int> *start)
{
  const int nch = (int)base.size();
  WalkCost wc(base, kind, grouped);
  if (start) start->assign(1, 0);
  int runs = 1, s = 0;
  long long cur = 0;
  for (int p = 0; p < nch; ++p) {
    int c = wc.add(p, s, runs);
    if (p > s && cur + c > cap) {
      s = p; ++runs; cur = 0;
      c = wc.add(p, s, runs);
      if (start) start->push_back(p);
    }
    cur += c;
  }
  if (start) start->push_back(nch);
  return runs;
}

// the cost of every run of a cut, and of every chunk in it
long long run_costs(const std::vector<int> &base, const std::vector<int> &kind, bool grouped, const std::vector<int> &start,
                    std::vector<long long> &rc)
{
  WalkCost wc(base, kind, grouped);
  const int nruns = (int)start.size() - 1;
  rc.assign((size_t)nruns, 0);
  long long mx = 0;
  for (int r = 0; r < nruns; ++r) {
    for (int p = start[r]; p < start[r + 1]; ++p) rc[r] += wc.add(p, start[r], r);
    mx = std::max(mx, rc[r]);
  }
  return mx;
}

// at most nruns runs with the smallest largest cost the greedy fill finds (bisection on the cap), then the heaviest
// runs halved until there are nruns of them: no CU is left without a run while another has two chunks
void cut_by_cost(const std::vector<int> &base, const std::vector<int> &kind, bool grouped, int nruns, std::vector<int> &start)
{
  const int nch = (int)base.size();
  long long lo = 0, hi = 0;
  for (int p = 0; p < nch; ++p) { lo = std::max(lo, (long long)base[p] + G_COST_WORDS); hi += base[p] + G_COST_WORDS; }
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (fill_runs(base, kind, grouped, mid, nullptr) <= nruns) hi = mid; else lo = mid + 1;
  }
  fill_runs(base, kind, grouped, hi, &start);
  std::vector<long long> rc;
  while ((int)start.size() - 1 < nruns) {
    run_costs(base, kind, grouped, start, rc);
    int best = -1;
    for (int r = 0; r + 1 < (int)start.size(); ++r)
      if (start[r + 1] - start[r] >= 2 && (best < 0 || rc[r] > rc[best])) best = r;
    if (best < 0) break;
    long long half = 0;
    int m = start[best];
    while (m < start[best + 1] - 1 && 2 * (half + base[m]) <= rc[best]) half += base[m++];
    start.insert(start.begin() + best + 1, std::max(m, start[best] + 1));
  }
}
}  // namespace

// how long a launch of these runs lasts, in modelled cycles: one workgroup is resident per CU, workgroup b goes to
// XCD b mod 8 and walks run (b mod 8) * per + b / 8 (kernels_gather.hip); a CU that finishes a run takes its XCD's next
long long gather_launch_cost(const std::vector<long long> &run_cost, int ncu)
{
  const int nruns = (int)run_cost.size(), per = (((nruns + 7) & ~7) + 7) >> 3, cus = std::max(1, ncu / 8);
  long long span = 0;
  for (int x = 0; x < 8; ++x) {
    std::vector<long long> busy((size_t)cus, 0);
    for (int j = 0; j < per && x * per + j < nruns; ++j) {
      auto cu = std::min_element(busy.begin(), busy.end());
      *cu += G_COST_RUN + run_cost[(size_t)x * per + j];
    }
    span = std::max(span, *std::max_element(busy.begin(), busy.end()));
  }
  return span;
}

namespace {
int env_int(const char *name, int dflt) { const char *e = getenv(name); return e && *e ? atoi(e) : dflt; }

// out.walk, out.run_start and out.cost from the chunks' records (before the layout)
void plan_walk(const std::vector<Local> &loc, int ncu, HostGather &out)
{
  const int nch = (int)loc.size();
  const bool grouped = env_int("FEAHIP_GATHER_ORDER", G_WALK_ORDER) != 0, balanced = env_int("FEAHIP_GATHER_BALANCE", G_WALK_BALANCE) != 0;
  const int run_fixed = std::max(0, env_int("FEAHIP_GATHER_RUN", 0));        // a fixed run length (tuning, tests)
  const int runs_fixed = std::max(0, env_int("FEAHIP_GATHER_NRUNS", 0));     // a fixed number of cost-balanced runs (tests)
  if (ncu <= 0) ncu = 256;
  std::vector<int> base((size_t)nch), kind;
  for (int p = 0; p < nch; ++p) base[p] = gather_chunk_cost(loc[p].h, false);
  word_kinds(loc, kind);
  std::vector<int> &start = out.run_start;
  auto equal_runs = [&](int rl, std::vector<int> &st) {
    st.clear();
    for (int c = 0; c < nch; c += rl) st.push_back(c);
    st.push_back(nch);
  };
  std::vector<long long> rc;
  if (run_fixed) equal_runs(run_fixed, start);
  else if (runs_fixed) cut_by_cost(base, kind, grouped, std::min(runs_fixed, nch), start);
  else if (FEA_G_BIG != 1) equal_runs(16, start);
  else {
    // One workgroup is resident per CU: with k runs per CU a launch lasts as long as the CU with the most work.  Two runs
    // per CU leave the scheduler something to even out, one run per CU saves a round where the chunks are few (a rank
    // of eight: 14.0 chunks per CU): whichever of k = 1, 2 predicts the shorter launch is taken.  Without balancing
    // the runs are cut by count, ceil(chunks / (k CUs)) each, and the launch is counted in chunks.
    long long best = -1;
    std::vector<int> st;
    for (int k = 2; k >= 1; --k) {
      long long cost;
      if (balanced) {
        cut_by_cost(base, kind, grouped, std::min(k * ncu, nch), st);
        run_costs(base, kind, grouped, st, rc);
        cost = gather_launch_cost(rc, ncu);
      } else {
        const int rl = std::max(1, (nch + k * ncu - 1) / (k * ncu)), nr = (nch + rl - 1) / rl;
        cost = (long long)((nr + ncu - 1) / ncu) * rl;
        equal_runs(rl, st);
      }
      if (best < 0 || cost < best) { best = cost; start = st; }
    }
  }
  // inside a run: the kinds in order of first appearance, row order inside a kind
  out.walk.resize((size_t)nch);
  for (int p = 0; p < nch; ++p) out.walk[p] = p;
  if (grouped) {
    std::vector<int> first((size_t)nch, -1);          // kind -> where it first appeared in the current run
    for (size_t r = 0; r + 1 < start.size(); ++r) {
      for (int p = start[r]; p < start[r + 1]; ++p)
        if (first[kind[p]] < start[r]) first[kind[p]] = p;
      std::stable_sort(out.walk.begin() + start[r], out.walk.begin() + start[r + 1], [&](int a, int b) { return first[kind[a]] < first[kind[b]]; });
    }
  }
  out.cost.resize((size_t)nch);
  for (size_t r = 0; r + 1 < start.size(); ++r)
    for (int i = start[r]; i < start[r + 1]; ++i)
      out.cost[i] = gather_chunk_cost(loc[out.walk[i]].h, i > start[r] && kind[out.walk[i]] != kind[out.walk[i - 1]]);
}
}  // namespace

void build_host_gather(int N, int E, const int *conn, const HostPattern &hp, int row_lo, int row_hi, HostGather &out,
                       const uint8_t *elem_mat, int ncu)
{
  (void)E;
  out.ok = false; out.nchunks = 0; out.blob.clear(); out.first_row.clear(); out.walk.clear(); out.run_start.clear(); out.cost.clear();
  if (row_lo < 0 || row_hi > N || row_lo >= row_hi) return;
  if (!partition(N, conn, hp, row_lo, row_hi, out.first_row)) return;
  const int nch = (int)out.first_row.size() - 1;
  std::vector<Local> loc((size_t)nch);
  std::vector<char> bad((size_t)nch, 0);
  parallel_ranges(nch, 512, [&](int lo, int hi) {
    ChunkBuilder cb(conn, hp, elem_mat);
    for (int p = lo; p < hi; ++p) bad[p] = !cb.build(out.first_row[p], out.first_row[p + 1], loc[p]);
  });
  for (int p = 0; p < nch; ++p)
    if (bad[p]) return;
  plan_walk(loc, ncu, out);
  if (!lay_out(loc, out.walk, elem_mat != nullptr, out)) return;
  mark_repeats(out, nch);
  out.nchunks = nch;
  out.total_evals = 0;
  for (const Local &L : loc)
    for (uint32_t w : L.elems) out.total_evals += w != 0xFFFFFFFFu;
  out.distinct_elems = count_distinct_elems(hp, conn, 4, row_lo, row_hi);
  out.ok = true;
}

// ---------------------------------------------------------------------------
// Host-only digest of what the assembly maps of one rank say, row by row: for every block row a rank's maps cover,
// a hash of the set of (row, column, element nodes, local row node, local column node) contributions they list
// (mirror blocks expanded).  The maps of different shards are cut differently (the gather chunks of a rank start
// at its first row), but what they SAY about a row must not depend on the cut: tests/test_host.py checks that the
// digests of the ranks of a sharded run add up to the digest of the unsharded run.  No device is touched.
// ---------------------------------------------------------------------------
namespace {
inline unsigned long long mix(unsigned long long h, unsigned long long v)
{
  h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
  return h * 0xBF58476D1CE4E5B9ull;
}
// the contribution of the element with nodes g[npe] to block (a, b); pair: its local row and column node
// (la * 4 + lb for 4-node elements, la * 16 + lb otherwise)
inline unsigned long long contribution_hash(int a, int b, const int *g, int npe, int pair)
{
  unsigned long long h = 0x1234567ull;
  h = mix(h, (unsigned long long)a); h = mix(h, (unsigned long long)b);
  for (int k = 0; k < npe; ++k) h = mix(h, (unsigned long long)g[k]);
  return mix(h, (unsigned long long)pair);
}
// tile position -> global row of a chunk with the rows [r0, r1) and the first block b0
int row_of(const HostPattern &hp, int r0, int r1, int b0, int pos)
{
  int a = r0;
  while (a + 1 < r1 && hp.rowptr[a + 1] - b0 <= pos) ++a;
  return a;
}

void gather_row_digest(const HostGather &hg, const HostPattern &hp, unsigned long long *rowhash)
{
  const GatherLayout &lay = hg.lay;
  for (int p = 0; p < hg.nchunks; ++p) {
    const unsigned char *rec = hg.blob.data() + (size_t)p * lay.stride;
    const GatherHeader &h = *reinterpret_cast<const GatherHeader *>(rec);
    const int *nodes = reinterpret_cast<const int *>(rec + lay.o_nodes);
    const uint32_t *elems = reinterpret_cast<const uint32_t *>(rec + lay.o_elems);
    const uint32_t *tpos = reinterpret_cast<const uint32_t *>(rec + lay.o_bpos);
    const uint16_t *clist = reinterpret_cast<const uint16_t *>(rec + lay.o_clist);
    const uint16_t *dlist = reinterpret_cast<const uint16_t *>(rec + lay.o_dlist);
    auto element_nodes = [&](int slot, int g[4]) {
      for (int k = 0; k < 4; ++k) g[k] = nodes[(elems[slot] >> (8 * k)) & 255u];
    };
    for (int t = 0; t < h.noffd; ++t) {
      if (tpos[t] == 0xFFFFFFFFu) continue;             // a thread without a block
      const int bpos = (int)(tpos[t] & 0xFFFFu), mpos = (int)(tpos[t] >> 16);
      const int a = row_of(hp, h.r0, h.r1, h.b0, bpos), b = hp.colidx[h.b0 + bpos];
      for (int k = 0; k < 2 * h.depth; ++k) {
        const uint16_t w = clist[((size_t)(k / 2) * FEA_G_THREADS + t) * 2 + (k & 1)];
        const int slot = (int)G_SLOT(w), la = G_LA(w), lb = G_LB(w);
        if (elems[slot] == 0xFFFFFFFFu) continue;     // empty list slot
        int g[4];
        element_nodes(slot, g);
        rowhash[a] += contribution_hash(a, b, g, 4, la * 4 + lb);
        if (mpos != 0xFFFF) rowhash[b] += contribution_hash(b, a, g, 4, lb * 4 + la);
      }
    }
    for (int l = 0; l < 4 * (h.r1 - h.r0); ++l)
      for (int k = 0; k < 2 * h.ddepth; ++k) {
        const uint16_t w = dlist[((size_t)(k / 2) * FEA_G_DIAG_LANES + l) * 2 + (k & 1)];
        const int slot = (int)G_SLOT(w), la = G_LA(w);
        if (elems[slot] == 0xFFFFFFFFu) continue;
        int g[4];
        element_nodes(slot, g);
        const int a = h.r0 + (l >> 2);
        rowhash[a] += contribution_hash(a, a, g, 4, la * 4 + la);
      }
  }
}

void gather10_row_digest(const HostGather10 &hg, const HostPattern &hp, const int *conn, unsigned long long *rowhash)
{
  const Gather10Layout &lay = hg.lay;
  for (int p = 0; p < hg.nchunks; ++p) {
    const unsigned char *rec = hg.blob.data() + (size_t)p * lay.stride;
    const Gather10Header &h = *reinterpret_cast<const Gather10Header *>(rec);
    const uint32_t *elems = reinterpret_cast<const uint32_t *>(rec + lay.o_elems);
    const uint32_t *tpos = reinterpret_cast<const uint32_t *>(rec + lay.o_tpos);
    const uint16_t *cl = reinterpret_cast<const uint16_t *>(rec + lay.o_clist);
    int row0 = 0;
    for (int s = 0; s < FEA_Q_SLOTS; ++s) {
      for (int t = 0; t < FEA_Q_THREADS; ++t) {
        const uint32_t tw = tpos[s * FEA_Q_THREADS + t];
        if (tw == 0xFFFFFFFFu) continue;
        const int bpos = (int)(tw & 0xFFFFu), mpos = (int)(tw >> 16);
        const int a = row_of(hp, h.r0, h.r1, h.b0, bpos), b = hp.colidx[h.b0 + bpos];
        for (int k = 0; k < 2 * h.sw[s]; ++k) {
          const uint16_t w = cl[(((size_t)row0 + k / 2) * FEA_Q_THREADS + t) * 2 + (k & 1)];
          const int le = w & 127, la = (w >> 7) & 15, lb = (w >> 11) & 15;
          if (le == lay.max_elems) continue;
          int g[16];
          for (int j = 0; j < hg.npe; ++j) g[j] = conn[(size_t)hg.elist[elems[le]] * hg.npe + j];
          rowhash[a] += contribution_hash(a, b, g, hg.npe, la * 16 + lb);
          if (mpos != 0xFFFF) rowhash[b] += contribution_hash(b, a, g, hg.npe, lb * 16 + la);
        }
      }
      row0 += h.sw[s];
    }
  }
}

void quad_row_digest(const HostQuad &hq, const HostPattern &hp, unsigned long long *rowhash)
{
  for (const QuadDesc &d : hq.desc) {
    for (int p = 0; p < d.npair; ++p) {
      const uint32_t w = hq.qpair[(size_t)d.pair_off + p];
      const int eli = (int)(w & 63u), la = (int)((w >> 6) & 15u), lb = (int)((w >> 10) & 15u), pos = (int)((w >> 14) & 255u);
      const int a = d.r0 + (int)((w >> 22) & 15u), b = hp.colidx[d.b0 + pos];
      const uint32_t *we = hq.qelem.data() + ((size_t)d.elem_off + eli) * 3;
      int g[10];
      for (int k = 0; k < 10; ++k) g[k] = hq.qnode[(size_t)d.node_off + ((we[k / 4] >> (8 * (k % 4))) & 255u)];
      rowhash[a] += contribution_hash(a, b, g, 10, la * 16 + lb);
    }
  }
}
}  // namespace

extern "C" int feahip_host_assembly_digest(int n_nodes, int n_elems, int npe, const int *elements, int rank, int nranks,
                                           unsigned long long *rowhash, int *rows)
{
  if (!elements || !rowhash || !rows || n_nodes <= 0 || n_elems <= 0 || nranks < 1 || rank < 0 || rank >= nranks) return FEAHIP_EINVAL;
  HostPattern hp;
  std::string err;
  int rc = build_host_pattern(n_nodes, n_elems, npe, elements, hp, err);
  if (rc) return rc;
  int row0, row1;
  shard_row_range(hp.chunk, rank, nranks, row0, row1);
  rows[0] = row0; rows[1] = row1;
  for (int a = 0; a < n_nodes; ++a) rowhash[a] = 0;
  if (npe == 4) {
    HostGather hg;
    build_host_gather(n_nodes, n_elems, elements, hp, row0, row1, hg);
    if (!hg.ok) return FEAHIP_EINVAL;
    gather_row_digest(hg, hp, rowhash);
  } else {
    // what AUTO runs for 10-node elements (kernels_assemble.hip): the gather maps when they build and an element
    // does not fall into too many chunks (12), the shared-state maps otherwise.  Both list every off-diagonal
    // contribution (the gather maps' mirror blocks are expanded); neither digest covers the diagonal blocks.
    bool done = false;
    if (npe == 10 || npe == 8) {
      HostGather10 hg;
      build_host_gather10(n_nodes, n_elems, npe, elements, hp, row0, row1, hg);
      if (hg.ok && (double)hg.total_evals <= 12.0 * (double)hg.distinct_elems) {
        gather10_row_digest(hg, hp, elements, rowhash);
        done = true;
      }
    }
    if (!done) {
      if (hp.super_achunk.empty()) return FEAHIP_EINVAL;
      const int nchunks = (int)hp.chunk.size() - 1;
      const int nsuper = (nchunks + FEA_SUPER_CHUNKS - 1) / FEA_SUPER_CHUNKS;
      const int s0 = (int)((long long)nsuper * rank / nranks), s1 = (int)((long long)nsuper * (rank + 1) / nranks);
      HostQuad hq;
      build_host_quad(n_nodes, n_elems, npe, elements, hp, hp.super_achunk[s0], hp.super_achunk[s1], hq);
      if (!hq.ok) return FEAHIP_EINVAL;
      quad_row_digest(hq, hp, rowhash);
    }
  }
  return FEAHIP_OK;
}

// Host-only (no device): what the gather maps (4-node, or 10-node / 8-node) look like for a mesh in the numbering it is given --
// stats[0..7] = chunks, element evaluations, distinct elements, rows, chunks repeating their predecessor's words, map
// bytes, chunks with block lists / diagonal lists longer than a thread's registers hold (4-node only); rows_hist[FEA_G_MAX_ROWS + 1] (may be null) = chunks by row count.  What the numbering of an unstructured mesh
// is judged by before a device sees it (tools/gather_stats.py).
extern "C" int feahip_host_gather_stats(int n_nodes, int n_elems, int npe, const int *elements, long long *stats, int *rows_hist)
{
  if (!elements || !stats || n_nodes <= 0 || n_elems <= 0 || (npe != 4 && npe != 10 && npe != 8)) return FEAHIP_EINVAL;
  HostPattern hp;
  std::string err;
  int rc = build_host_pattern(n_nodes, n_elems, npe, elements, hp, err);
  if (rc) return rc;
  stats[6] = stats[7] = 0;
  HostGather hg;
  HostGather10 hq;
  const HostChunkMaps &m = npe == 4 ? static_cast<const HostChunkMaps &>(hg) : hq;
  if (npe == 4) build_host_gather(n_nodes, n_elems, elements, hp, 0, n_nodes, hg);
  else build_host_gather10(n_nodes, n_elems, npe, elements, hp, 0, n_nodes, hq);
  if (!m.ok) return FEAHIP_EINVAL;
  stats[0] = m.nchunks; stats[1] = m.total_evals; stats[2] = m.distinct_elems; stats[3] = n_nodes;
  stats[4] = npe == 4 ? hg.same_as_previous : 0; stats[5] = (long long)m.blob.size();
  if (npe == 4) {
    for (int p = 0; p < hg.nchunks; ++p) {            // lists longer than the words a thread keeps in registers are walked out of memory
      const GatherHeader &gh = *reinterpret_cast<const GatherHeader *>(hg.blob.data() + (size_t)p * hg.lay.stride);
      stats[6] += gh.depth > FEA_G_REGW; stats[7] += gh.ddepth > FEA_G_REGW;
    }
    if (getenv("FEAHIP_NUMBERING_VERBOSE")) {         // chunks by the words of their longest block list / diagonal list
      int hd[17] = {0}, hdd[17] = {0};
      for (int p = 0; p < hg.nchunks; ++p) {
        const GatherHeader &gh = *reinterpret_cast<const GatherHeader *>(hg.blob.data() + (size_t)p * hg.lay.stride);
        ++hd[std::min(gh.depth, 16)]; ++hdd[std::min(gh.ddepth, 16)];
      }
      for (int k = 0; k <= 16; ++k) if (hd[k] || hdd[k]) fprintf(stderr, "gather maps: %d words: %d chunks by block list, %d by diagonal list\n", k, hd[k], hdd[k]);
    }
  }
  if (rows_hist) {
    for (int l = 0; l <= FEA_G_MAX_ROWS; ++l) rows_hist[l] = 0;
    for (int p = 0; p < m.nchunks; ++p) ++rows_hist[std::min(m.first_row[p + 1] - m.first_row[p], FEA_G_MAX_ROWS)];
  }
  return FEAHIP_OK;
}

// Host-only (no device): per chunk of the 4-node gather maps, in chunk order (include/fea_hip.h)
extern "C" int feahip_host_gather_chunks(int n_nodes, int n_elems, const int *elements, int capacity, int *flags)
{
  if (!elements || n_nodes <= 0 || n_elems <= 0 || capacity < 0 || (capacity > 0 && !flags)) return FEAHIP_EINVAL;
  HostPattern hp;
  std::string err;
  int rc = build_host_pattern(n_nodes, n_elems, 4, elements, hp, err);
  if (rc) return rc;
  HostGather hg;
  build_host_gather(n_nodes, n_elems, elements, hp, 0, n_nodes, hg);
  if (!hg.ok) return FEAHIP_EINVAL;
  for (int p = 0; p < hg.nchunks && p < capacity; ++p) {
    const GatherHeader &gh = *reinterpret_cast<const GatherHeader *>(hg.blob.data() + (size_t)p * hg.lay.stride);
    flags[p] = (gh.flags & 1) | (gh.depth > FEA_G_REGW ? 2 : 0) | (gh.ddepth > FEA_G_REGW ? 4 : 0);
  }
  return hg.nchunks;
}

// Host-only (no device): the walk of the 4-node gather maps (include/fea_hip.h)
extern "C" int feahip_host_gather_walk(int n_nodes, int n_elems, const int *elements, int row_lo, int row_hi, int ncu, long long *info,
                                       int capacity, int *walk, int *run_start, int *cost, long long blob_capacity, unsigned char *blob)
{
  if (!elements || !info || n_nodes <= 0 || n_elems <= 0 || capacity < 0 || blob_capacity < 0) return FEAHIP_EINVAL;
  HostPattern hp;
  std::string err;
  int rc = build_host_pattern(n_nodes, n_elems, 4, elements, hp, err);
  if (rc) return rc;
  if (row_hi <= 0) { row_lo = 0; row_hi = n_nodes; }
  HostGather hg;
  build_host_gather(n_nodes, n_elems, elements, hp, row_lo, row_hi, hg, nullptr, ncu);
  if (!hg.ok) return FEAHIP_EINVAL;
  const int nruns = (int)hg.run_start.size() - 1;
  std::vector<long long> rcost((size_t)nruns, 0);
  for (int r = 0; r < nruns; ++r)
    for (int i = hg.run_start[r]; i < hg.run_start[r + 1]; ++i) rcost[r] += hg.cost[i];
  info[0] = hg.nchunks; info[1] = nruns; info[2] = hg.lay.stride; info[3] = hg.lay.o_elems;
  info[4] = hg.lay.o_emat ? hg.lay.o_emat : hg.lay.stride; info[5] = (long long)hg.blob.size(); info[6] = hg.same_as_previous;
  info[7] = gather_launch_cost(rcost, ncu > 0 ? ncu : 256);
  if (capacity >= hg.nchunks && walk && run_start && cost) {
    std::copy(hg.walk.begin(), hg.walk.end(), walk);
    std::copy(hg.run_start.begin(), hg.run_start.end(), run_start);
    std::copy(hg.cost.begin(), hg.cost.end(), cost);
  }
  if (blob && blob_capacity >= (long long)hg.blob.size()) memcpy(blob, hg.blob.data(), hg.blob.size());
  return hg.nchunks;
}

#ifdef FEAHIP_DEBUG
// diagnostic build only, host only: one chunk's map record and the layout, for the LDS bank model (dbg/lds_model.py)
extern "C" int feahip_debug_gather_record_host(int n_nodes, int n_elems, const int *elements, int chunk, int *layout_ints,
                                               unsigned char *record, int *nchunks)
{
  static HostGather hg;                       // cached between the sizing call and the copying call
  static int cached_n = -1, cached_e = -1;
  if (cached_n != n_nodes || cached_e != n_elems) {
    HostPattern hp;
    std::string err;
    if (build_host_pattern(n_nodes, n_elems, 4, elements, hp, err)) return FEAHIP_EINVAL;
    build_host_gather(n_nodes, n_elems, elements, hp, 0, n_nodes, hg);
    if (!hg.ok) return FEAHIP_EINVAL;
    cached_n = n_nodes; cached_e = n_elems;
  }
  if (chunk < 0) chunk = hg.nchunks / 2;
  memcpy(layout_ints, &hg.lay, sizeof(GatherLayout));
  if (nchunks) *nchunks = hg.nchunks;
  if (chunk >= hg.nchunks) return FEAHIP_EINVAL;
  const size_t at = (size_t)(std::find(hg.walk.begin(), hg.walk.end(), chunk) - hg.walk.begin());   // chunk: in row order
  if (record) memcpy(record, hg.blob.data() + at * hg.lay.stride, hg.lay.stride);
  return (int)(sizeof(GatherLayout) / sizeof(int));
}
#endif
