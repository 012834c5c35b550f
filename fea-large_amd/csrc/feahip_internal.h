// feahip_internal.h -- context layout shared by the translation units of
// libfeahip.so.  Not part of the ABI (include/fea_hip.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <initializer_list>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include "../../include/fea_hip.h"

// Every device allocation of the library goes through here.  FEAHIP_TEST_NAN_ALLOC=1 (test knob: results must not
// change) fills a fresh allocation with 0xFF bytes -- NaN as a double or a float, -1 as an integer -- so that a read of
// memory the library never wrote shows in the results instead of depending on what the allocator handed back
// (GPU AddressSanitizer is not available on the target pool).
hipError_t feahip_device_malloc(void **p, size_t bytes);
#define hipMalloc(p, bytes) feahip_device_malloc((void **)(p), (bytes))

#define FEA_MAX_NPE 10
#define FEA_MAX_GAUSS 27

// one wave owns a run of block rows ("chunk"); its 3x3 blocks are summed in
// LDS and written to HBM once.  CHUNK_BLOCKS bounds the LDS per wave.
#define FEA_CHUNK_BLOCKS 128
#define FEA_CHUNK_ROWS 16
#define FEA_WAVES_PER_WG 4
// grid used by the vector / reduction kernels: their per-block partial sums
// are re-reduced by every block of the consuming kernel.
#define FEA_RED_BLOCKS 2048

struct ElemTable {            // element plug-in, tabulated by the host
  double w[FEA_MAX_GAUSS];
  double dN[FEA_MAX_GAUSS][3][FEA_MAX_NPE];
};

#define FEA_HIP_CHECK(ctx, call)                                            \
  do {                                                                      \
    hipError_t _e = (call);                                                 \
    if (_e != hipSuccess) {                                                 \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(_e);       \
      return FEAHIP_EHIP;                                                   \
    }                                                                       \
  } while (0)

// host map construction: f(lo, hi) on equal consecutive ranges of [0, n), one thread each (up to 32); a single
// call below serial_below items
template <class F>
void parallel_ranges(int n, int serial_below, F f)
{
  unsigned hw = std::thread::hardware_concurrency();
  int nt = (int)std::min<unsigned>(hw ? hw : 4, 32);
  if (n < serial_below) nt = 1;
  if (nt <= 1) { f(0, n); return; }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t) {
    int lo = (int)((long long)n * t / nt), hi = (int)((long long)n * (t + 1) / nt);
    th.emplace_back([=] { f(lo, hi); });
  }
  for (auto &x : th) x.join();
}
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// pattern.cpp
struct HostPattern {
  std::vector<int> rowptr, colidx;       // block CSR, sorted columns
  std::vector<int> incptr;               // [N+1]
  std::vector<uint32_t> inc;             // [npe*E]
  std::vector<uint8_t> incslot;          // [npe*E*npe]
  std::vector<int> chunk;                // chunk -> first row
  std::vector<int> diag;                 // row -> index of its diagonal block
  std::vector<uint32_t> inc_rows;        // inc before the per-chunk interleave (row-sorted)
  std::vector<int> achunk;               // assembly partition of the staged kernel (4-node elements)
  std::vector<int> super_achunk;         // first achunk of every super, [nsuper+1]
  int max_rowlen = 0;
  int break_chunk = 0, break_super = 0;  // first chunk / super at or behind row_break (their counts when there is no break)
};
int build_host_pattern(int N, int E, int npe, const int *conn, HostPattern &hp,
                       std::string &err, int row_break = -1);
// an incidence word of inc / inc_rows: element | local node << 28
inline int inc_elem(uint32_t w) { return (int)(w & 0x0FFFFFFFu); }
inline int inc_node(uint32_t w) { return (int)(w >> 28); }
// CSR position of the block (a, b)
inline int csr_pos(const HostPattern &hp, int a, int b)
{
  const int *cb = hp.colidx.data() + hp.rowptr[a], *ce = hp.colidx.data() + hp.rowptr[a + 1];
  return hp.rowptr[a] + (int)(std::lower_bound(cb, ce, b) - cb);
}

// visits.cpp
// LDS-staged visit assembly (kernels_visit.hip): per chunk, the nodes its
// elements touch (owned rows first) and one 8-byte record per (row, element)
// visit: 4 chunk-local node ids (row node first) + 3 column slots.
// assembly chunks of the staged kernel are smaller than the SpMV chunks (LDS
// per wave sets the occupancy): two passes of 64 visits, 64 nodes, 80 blocks
#define FEA_VISIT_MAX_NODES 64
#define FEA_VISIT_MAX_VISITS 128
#define FEA_ACHUNK_BLOCKS 80
#define FEA_ACHUNK_ROWS 8              // rows of a staged-assembly chunk (sizes its f tile: 16 workgroups per CU fit)
#define FEA_SUPER_CHUNKS 8            // a "super" = 8 SpMV chunks; both partitions break at supers; unit of the row shard
struct VisitDesc {                   // 32 bytes, one per chunk
  int r0, r1, b0, nb;
  int node_off, nnode;               // into vnode
  int visit_off, nvisit;             // into vrec: first record, records (a multiple of 64: whole passes)
};
struct HostVisits {
  std::vector<VisitDesc> desc;
  std::vector<int> vnode;
  std::vector<uint32_t> vrec;        // [2 * visits]: ids (4 x u8), then u8 x 4: parity flag, tile positions of the 3 blocks
  bool ok = false;
};
void build_host_visits(int N, int E, const int *conn, const HostPattern &hp, HostVisits &out);
// shared-state assembly of 10-node elements (kernels_quad.hip): per chunk the
// distinct elements touching its rows and one 4-byte record per
// (row, element, column node) pair
#define FEA_QUAD_BLOCKS 256           // K tile of one workgroup (tile position: 8 bits of the pair word)
#define FEA_QUAD_PAIRS 512            // pairs of a multi-row chunk (a single row may have more)
#define FEA_QUAD_ELEMS 64             // distinct elements of a chunk (6-bit index in a pair record)
#define FEA_QUAD_NODES 126            // coordinate tile: distinct nodes of the chunk's elements
#define FEA_QUAD_VISITS 96            // (row, element) visits of a chunk: one row-vector record per visit and Gauss point of a batch
struct QuadDesc {                    // 40 bytes, one per chunk
  int r0, r1, b0, nb;
  int elem_off, nelem;               // into qelem (3 words per element)
  int pair_off, npair;               // into qpair
  int node_off, nnode;               // into qnode
};
struct HostQuad {
  std::vector<QuadDesc> desc;
  std::vector<int> qnode;            // global ids of the chunk's nodes
  std::vector<uint32_t> qelem;       // per element 12 bytes: 10 chunk-local node ids (u8), flags (bit 0: its local node 0 is a row of this chunk), 0
  std::vector<uint32_t> qpair;       // el(6) | la(4)<<6 | lb(4)<<10 | tile position(8)<<14 | local row(4)<<22 | first pair of its visit<<26
  bool ok = false;
};
void build_host_quad(int N, int E, int npe, const int *conn, const HostPattern &hp, int p_lo, int p_hi, HostQuad &out);
int ensure_quad(feahip_ctx *c);
int launch_assemble_quad(feahip_ctx *c, bool doF);

// ---- stages shared by the builders of the chunked maps (gather.cpp).  A chunk is a run of consecutive block rows
// [r0, r1); the builders pass their scratch vectors in, so that a parallel_ranges worker reuses them chunk after chunk.
// true when the element of incidence word w, visited at row r, has no other node among the rows [r0, r): it is new
// to the rows [r0, r]
inline bool first_visit(const HostPattern &hp, const int *conn, int npe, uint32_t w, int r0, int r)
{
  const int e = inc_elem(w), la = inc_node(w);
  for (int k = 0; k < npe; ++k) {
    const int g = conn[(size_t)e * npe + k];
    if (k != la && g >= r0 && g < r) return false;
  }
  return true;
}
// Pass A, the cost row of the chunks that start at row r0: cost[l-1] = distinct elements touching the rows
// [r0, r0 + l), for l = 1, 2, ... while fits(r, l, nel, ntask, fresh) says the chunk ending at row r = r0 + l - 1
// still fits (every longer one fails too; cost[] stays 0xFFFF there).  nel: its elements; ntask: its off-diagonal
// blocks with a thread of their own (a block whose column is a lower row of the chunk is its mirror's transpose);
// fresh: the elements row r adds.
template <class Fits>
void chunk_costs(const HostPattern &hp, const int *conn, int npe, int r0, int row_hi, int L, std::vector<int> &fresh,
                 uint16_t *cost, Fits fits)
{
  int nel = 0, ntask = 0;
  for (int l = 1; l <= L && r0 + l <= row_hi; ++l) {
    const int r = r0 + l - 1;
    fresh.clear();
    for (int q = hp.incptr[r]; q < hp.incptr[r + 1]; ++q)
      if (first_visit(hp, conn, npe, hp.inc_rows[q], r0, r)) fresh.push_back(inc_elem(hp.inc_rows[q]));
    nel += (int)fresh.size();
    const int *cb = hp.colidx.data() + hp.rowptr[r], *ce = hp.colidx.data() + hp.rowptr[r + 1];
    ntask += (int)(ce - cb) - 1 - (int)(std::lower_bound(cb, ce, r) - std::lower_bound(cb, ce, r0));
    if (!fits(r, l, nel, ntask, fresh)) break;
    cost[l - 1] = (uint16_t)nel;
  }
}
// Pass A, the chunk boundaries.  Every element evaluation a chunk makes is work, so the partition that minimises
// their total (plus a per-chunk overhead alpha) is found by a shortest-path recurrence over the rows; it finds the
// natural clusters of whatever numbering the mesh came with (bricks, lines) instead of cutting through them.
// cost[i * L + l - 1]: the chunk_costs of row row_lo + i.  Returns -1 and the first row of every chunk and row_hi
// in first_row, or the first row that fits no chunk (first_row is left as it was).
int partition_rows(const std::vector<uint16_t> &cost, int row_lo, int row_hi, int L, int alpha, std::vector<int> &first_row);
// the distinct elements touching the rows [r0, r1), ascending
void chunk_elements(const HostPattern &hp, int r0, int r1, std::vector<int> &el);
// the off-diagonal blocks of the rows [r0, r1) that get a thread, in CSR order (see chunk_costs): tpos[t] = tile
// position of the block of task t | tile position of its mirror (b, a) << 16 when b is a row of the chunk too,
// 0xFFFF << 16 otherwise; task_of[pos] = the task of the block at tile position pos, -1 for none
void chunk_block_tasks(const HostPattern &hp, int r0, int r1, std::vector<uint32_t> &tpos, std::vector<int> &task_of);
// per task the contributions (element, local row node la, local column node lb) to its block, row by row in
// incidence order: word = index of the element in el | la << la_shift | lb << lb_shift
void chunk_block_lists(const HostPattern &hp, const int *conn, int npe, int r0, int r1, const std::vector<int> &el,
                       const std::vector<int> &task_of, int ntask, int la_shift, int lb_shift,
                       std::vector<std::vector<uint16_t>> &lists);
// distinct elements touching the rows [r0, r1)
long long count_distinct_elems(const HostPattern &hp, const int *conn, int npe, int r0, int r1);
// what the gather maps of both families have in common
struct HostChunkMaps {
  std::vector<unsigned char> blob;   // nchunks records of lay.stride bytes
  std::vector<int> first_row;        // [nchunks+1]
  long long total_evals = 0, distinct_elems = 0;   // element evaluations of all chunks; elements touching the rows
  int nchunks = 0;
  bool ok = false;
};

// GATHER assembly (kernels_gather.hip, gather.cpp): a 256-thread workgroup owns a run of consecutive block rows.
// Per chunk the host prepares one fixed-stride record: header, the chunk's nodes (owned rows first), its distinct
// elements as 4 chunk-local node ids, and per off-diagonal block the list of (element, local row node, local
// column node) contributions that sum to it; per residual thread a slice of one row's (element, local node) visits.
#ifndef FEA_G_BIG
#define FEA_G_BIG 1
#endif
#if FEA_G_BIG == 1
#define FEA_G_THREADS 1024            // one workgroup per CU: sixteen waves share one chunk's records (see kernels_gather.hip)
#define FEA_G_TASK_THREADS 768        // block and residual threads: waves 0-11; waves 12-15 (FEA_G_DIAG_LANES) sum the diagonal blocks
#define FEA_G_MAX_ROWS 64
#define FEA_G_MAX_NODES 256           // 8-bit chunk-local node slots
#define FEA_G_MAX_ELEMS 719           // slots come in sixteens and one stays all-zero; 45 x 16 = 720 records of 208 B fill the LDS next to the coordinates
#define FEA_G_ELEMS_TARGET 672        // a 4 x 4 x 4 brick of nodes of a Kuhn block
#define FEA_G_CELL 4, 4, 4
#elif FEA_G_BIG == 2
#define FEA_G_THREADS 512             // two workgroups per CU, eight waves each
#define FEA_G_TASK_THREADS 384
#define FEA_G_MAX_ROWS 32
#define FEA_G_MAX_NODES 128
#define FEA_G_MAX_ELEMS 351           // 22 x 16 = 352 records of 208 B + the coordinates: 80 KB
#define FEA_G_ELEMS_TARGET 320        // a 4 x 3 x 2 brick of nodes of a Kuhn block touches 300 elements
#define FEA_G_CELL 4, 2, 3
#else
#define FEA_G_THREADS 256             // three workgroups per CU
#define FEA_G_TASK_THREADS 192
#define FEA_G_MAX_ROWS 16
#define FEA_G_MAX_NODES 128
#define FEA_G_MAX_ELEMS 239
#define FEA_G_ELEMS_TARGET 216        // a 4 x 2 x 2 brick
#define FEA_G_CELL 4, 2, 2
#endif
#define FEA_G_DIAG_LANES (FEA_G_THREADS - FEA_G_TASK_THREADS)
#define FEA_G_SLOT_BITS 10            // record slot inside a contribution / visit entry: slot | la << 10 | lb << 12
#define FEA_G_MAX_SLOTS 1024
#define FEA_G_REGW 6                  // contribution words a block thread keeps in registers (2 entries each).  A lattice needs 3 (six
                                      // elements around an edge at most); on the reference's TetGen deck 92 % of the chunks have a list of
                                      // 5 words and 4 % one of 6, and with 4 in registers the rest was fetched INSIDE the gather phase,
                                      // one exposed HBM round trip per word (kernels_gather.hip); the words are loaded only up to the
                                      // mesh's longest list (GatherLayout::max_depth), so a lattice issues no more loads than before
struct GatherHeader {                // 64 bytes, first thing in a chunk record
  int r0, r1, b0, nb;                // rows [r0, r1), blocks [b0, b0+nb) of the CSR
  int nnode, nelem, noffd, depth;    // depth: contribution words per block thread
  int nvthr, vdepth;                 // residual threads, visits per residual thread
  int ddepth;                        // diagonal-block words per lane of the last wave
  unsigned wdepth[3];                // contribution words the block threads of wave slot w walk (the longest list of ITS blocks), one byte per slot
  int flags;                         // bit 0: the map words of the NEXT chunk of the context (everything but header and node list) equal this chunk's
  int pad[1];
};
static_assert(sizeof(GatherHeader) == 64 && FEA_G_TASK_THREADS / 64 <= 12, "GatherHeader: 64 bytes, twelve block-wave slots");
struct GatherLayout {                // the same for every chunk of a context
  int stride;                        // bytes per chunk record
  int o_nodes, o_elems, o_bpos, o_rows, o_vlist, o_dlist, o_clist;   // byte offsets of the sections
  int max_nodes, max_elems, max_tile;                        // LDS tiles: coordinates, element records, K blocks
  int max_tasks, max_depth, max_vthr, max_vdepth, max_ddepth;   // largest chunk: block threads, contribution words, residual threads, visits, diagonal words
  int o_emat;                        // byte offset of the material ids (one byte per element slot, the last section); 0: no material table
};
struct HostGather : HostChunkMaps {
  GatherLayout lay;
  int same_as_previous = 0;          // chunks whose map words equal their predecessor's in walk order (GatherHeader::flags)
  // the walk (gather.cpp): the blob holds the records in walk order; first_row stays in row order
  std::vector<int> walk;             // [nchunks] the chunk, in row order, whose record is the i-th of the blob
  std::vector<int> run_start;        // [nruns+1] a workgroup walks the records [run_start[r], run_start[r+1]); no run is empty
  std::vector<int> cost;             // [nchunks] modelled cycles of the i-th record where it stands (gather_chunk_cost)
};
// rows [row_lo, row_hi) only: a rank builds the maps of the rows it owns
// elem_mat (may be null): material id of every element; the records then carry the optional section o_emat
// ncu: the compute units the runs are cut for (0: 256).  FEAHIP_GATHER_ORDER=0: the records in row order;
// FEAHIP_GATHER_BALANCE=0: runs of equal chunk counts; FEAHIP_GATHER_RUN=n: runs of n chunks (tuning; no result changes)
void build_host_gather(int N, int E, const int *conn, const HostPattern &hp, int row_lo, int row_hi, HostGather &out,
                       const uint8_t *elem_mat = nullptr, int ncu = 0);
// modelled shader cycles of one chunk (K-and-f kernel) from its header; loads_words: its predecessor in the run cannot
// hand it its map words.  Pure host arithmetic.
int gather_chunk_cost(const GatherHeader &h, bool loads_words);
// modelled cycles of a launch of runs of these costs on ncu compute units
long long gather_launch_cost(const std::vector<long long> &run_cost, int ncu);
int ensure_gather(feahip_ctx *c);
int launch_assemble_gather(feahip_ctx *c, bool doK, bool doF);

// GATHER assembly of 10-node tetrahedra (kernels_gather10.hip, gather10.cpp).  Same idea as the 4-node one with the
// Gauss points as an outer loop: a 256-thread workgroup owns up to 64 consecutive block rows, evaluates every
// distinct element touching them once per Gauss point into LDS records (spatial gradient g_k and traction vector
// t_k of its ten nodes), and every thread sums up to five off-diagonal blocks over all Gauss points in registers.
#ifndef FEA_Q_THREADS
#define FEA_Q_THREADS 256             // two workgroups per CU (the accumulators of five blocks per thread take the register file:
                                      // 384 threads x 4 blocks and 512 x 3 spill 240-370 bytes per lane at their register budgets)
#endif
#define FEA_Q_WAVES (FEA_Q_THREADS / 64)
#define FEA_Q_MAX_ROWS 64
#define FEA_Q_MAX_NODES 240           // 8-bit chunk-local node ids
#define FEA_Q_MAX_ELEMS 127           // 7-bit record slot; the slot after the last one in use is the all-zero record
#ifndef FEA_Q_SLOTS
#define FEA_Q_SLOTS 5                 // blocks per thread
#endif
#define FEA_Q_REGW 4                  // contribution words per block a thread keeps in registers (2 entries each)
#define FEA_Q_MAX_PASS 7              // write-out passes of one chunk through the K tile
#define FEA_Q_FLANES 128              // residual lanes (the last two waves)
#define FEA_Q_ROWS_U16 200            // rstart[65] | rdiag[64] at 66 | ffirst[65] at 130
struct Gather10Header {              // 128 bytes
  int r0, r1, b0, nb;
  int nnode, nelem, ntask, npass;
  int nft, fdw;                      // residual lanes, words per residual lane (2 visits each)
  unsigned char prow[8];             // pass p writes the rows [prow[p], prow[p+1]) of the chunk
  unsigned char cnt[40];             // contributions of the longest list among the 64 blocks wave w holds in slot s, at [FEA_Q_WAVES s + w]
  unsigned char sw[8];               // list words stored for slot s (the longest of its waves); rows of the clist section
  int pad[8];
};
static_assert(FEA_Q_SLOTS * FEA_Q_WAVES <= 40 && FEA_Q_SLOTS <= 8, "Gather10Header: cnt / sw too small");
static_assert(sizeof(Gather10Header) == 128, "Gather10Header is 128 bytes");
struct Gather10Layout {
  int stride;
  int o_nodes, o_elems, o_rows, o_tpos, o_flist, o_clist;
  int max_nodes, max_elems, max_cw, max_fdw, tile_blocks;      // max_cw: clist rows (256 words each) of the longest chunk
};
enum Gather10Limit {                 // why build_host_gather10 gave up (feahip_host_gather10_shape reports it)
  G10_FITS = FEAHIP_G10_LIMIT_NONE, G10_ELEMS = FEAHIP_G10_LIMIT_ELEMS, G10_ROW_LENGTH = FEAHIP_G10_LIMIT_ROW_LENGTH,
  G10_TASKS = FEAHIP_G10_LIMIT_TASKS, G10_RESIDUAL_LANES = FEAHIP_G10_LIMIT_RESIDUAL_LANES,
  G10_LIST_LENGTH = FEAHIP_G10_LIMIT_LIST_LENGTH, G10_PASSES = FEAHIP_G10_LIMIT_PASSES, G10_OTHER = FEAHIP_G10_LIMIT_OTHER
};
struct HostGather10 : HostChunkMaps {
  Gather10Layout lay;
  std::vector<int> elist;            // the rank's elements (touching its rows), ascending: order of the state records
  int npe = 10;
  int limit = G10_FITS;              // when !ok: the limit the maps ran into first
  int limit_row = -1;                // ... at this row (the row that fits no chunk, or the first row of the chunk that failed)
  int tile_blocks = 0;               // blocks of the K tile the chunks are cut for (set also when the maps fail)
};
void build_host_gather10(int N, int E, int npe, const int *conn, const HostPattern &hp, int row_lo, int row_hi, HostGather10 &out);
int ensure_gather10(feahip_ctx *c);
int launch_assemble_gather10(feahip_ctx *c, bool doK, bool doF);

int launch_assemble_visit(feahip_ctx *c, bool doK, bool doF);

// ---- maps of the assembly strategies.  Each family's maps are built for one key: the rows [row0, row1) of the shard
// for the gather kernels, the assembly chunks [achunk0, achunk0 + nachunks_local) for the shared-state kernel, the
// whole mesh for the staged visits and the incidence lists.  The maps and the outcome of their build are valid for
// that key only; release() frees the buffers and forgets both.
enum class MapOutcome { none, built, failed, declined };   // declined: built, looked at and dropped by AUTO
struct MapCache {
  int key0 = -1, key1 = -1;
  MapOutcome outcome = MapOutcome::none;
  long long bytes = 0;                 // device bytes of the maps
  bool built() const { return outcome == MapOutcome::built; }
  bool is(MapOutcome o, int k0, int k1) const { return outcome == o && key0 == k0 && key1 == k1; }
  // nothing to build for this key (a declined build is made again when the strategy is asked for)
  bool settled(int k0, int k1) const { return is(MapOutcome::built, k0, k1) || is(MapOutcome::failed, k0, k1); }
  void record(MapOutcome o, int k0, int k1) { outcome = o; key0 = k0; key1 = k1; }
};
inline void dev_free(std::initializer_list<void *> ptrs) { for (void *p : ptrs) if (p) (void)hipFree(p); }
struct GenericMaps : MapCache {        // node -> element incidence (row-owner and atomic assembly)
  int *d_incptr = nullptr;             // [N+1]
  uint32_t *d_inc = nullptr;           // [npe*E]  elem | local<<28
  uint8_t *d_incslot = nullptr;        // [npe*E][npe] slot of column conn[e][b] in row
  void release() { dev_free({d_incptr, d_inc, d_incslot}); *this = GenericMaps(); }
};
struct VisitMaps : MapCache {          // LDS-staged visits (linear tetrahedra)
  VisitDesc *d_desc = nullptr;
  int *d_node = nullptr;
  uint32_t *d_rec = nullptr;
  int nrecords = 0;                    // length of rec in records (whole passes per chunk)
  void release() { dev_free({d_desc, d_node, d_rec}); *this = VisitMaps(); }
};
struct QuadMaps : MapCache {           // shared-state kernel: this rank's assembly chunks
  QuadDesc *d_desc = nullptr;
  uint32_t *d_elem = nullptr, *d_pair = nullptr;
  int *d_node = nullptr;
  int nchunks = 0;
  void release() { dev_free({d_desc, d_elem, d_pair, d_node}); *this = QuadMaps(); }
};
struct GatherCache : MapCache {        // either gather kernel: one map record per chunk of the rows this rank owns
  unsigned char *d_maps = nullptr;
  int nchunks = 0;
  double evals_per_element = 0;        // element evaluations the chunks make per element the rows touch
  int same_words = 0;                  // chunks whose map words equal their predecessor's (4-node maps)
};
struct GatherMaps : GatherCache {
  GatherLayout lay{};
  int *d_run_start = nullptr;          // [nruns+1] records of the runs, in walk order (HostGather::run_start)
  int nruns = 0;
  std::vector<int> record_of;          // [nchunks] where in d_maps the record of a chunk (in row order) sits
  void release() { dev_free({d_maps, d_run_start}); *this = GatherMaps(); }
};
struct Gather10Maps : GatherCache {
  Gather10Layout lay{};
  int *d_elist = nullptr;              // this rank's elements
  double *d_state = nullptr;           // [G][elements of the rank][18]: Gauss-point state records (kernels_gather10.hip)
  int nloc = 0;
  void release() { dev_free({d_maps, d_elist, d_state}); *this = Gather10Maps(); }
};

// surface loads (kernels_surface.hip): the loaded boundary faces in library ids, each in its element's face order
// (outward normal), and the node -> (face, slot) incidence kernel 2 sums in a fixed order
struct SurfaceLoads {
  int nfaces = 0, npf = 0;             // faces; nodes per face (3, 6 or 4)
  std::vector<int> h_lnode;            // the loaded nodes, ascending (library ids)
  int *d_fnode = nullptr;              // [nfaces][npf]
  int *d_kind = nullptr;               // [nfaces] FEAHIP_LOAD_*
  double *d_val = nullptr;             // [nfaces][3]: pressure in [0], or the dead traction t0
  double *d_fc = nullptr;              // [nfaces][npf][3] contributions of kernel 1 (lambda applied)
  int *d_lnode = nullptr, *d_lptr = nullptr, *d_lslot = nullptr;   // [nloaded], [nloaded + 1], slot = face * npf + k
  void release() { dev_free({d_fnode, d_kind, d_val, d_fc, d_lnode, d_lptr, d_lslot}); *this = SurfaceLoads(); }
};

// quadrature of a boundary face (kernels_surface.hip): tri3 one point, tri6 the 6-point degree-4 rule, quad4 2 x 2 Gauss
#define FEA_SURF_MAX_PTS 6
#define FEA_SURF_MAX_NPF 6
struct FaceRule {
  int npt;
  double w[FEA_SURF_MAX_PTS];
  double N[FEA_SURF_MAX_PTS][FEA_SURF_MAX_NPF];
  double dN[FEA_SURF_MAX_PTS][2][FEA_SURF_MAX_NPF];
};
void face_rule(int npf, FaceRule &R);

// frictionless contact of nodes with rigid obstacles (kernels_contact.hip): nothing of it exists, and nothing is
// launched, until feahip_set_contact.  The obstacles travel to the kernels by value, their point already moved to
// c0 + load_factor * travel.
struct ContactObstacles {
  int n;
  int kind[FEAHIP_MAX_OBSTACLES];
  double c[FEAHIP_MAX_OBSTACLES][3];   // the point at the load factor of the launch
  double a[FEAHIP_MAX_OBSTACLES][3];   // unit normal (plane) or axis (cylinder)
  double r[FEAHIP_MAX_OBSTACLES];
};
struct ContactState {
  bool set = false;                    // feahip_set_contact was called with faces and obstacles and not cleared since
  int n = 0, nobs = 0;                 // contact nodes this context holds (a rank: those of the faces it kept); obstacles
  double penalty = 0, gap_tolerance = 0;
  int augment_max = 0;
  int kind[FEAHIP_MAX_OBSTACLES] = {0};
  double geom[FEAHIP_MAX_OBSTACLES][10] = {{0}};   // point, unit direction, radius, travel
  std::vector<int> h_node;             // the contact nodes, ascending (library ids)
  std::vector<double> h_w;             // their reference-area weights
  int *d_node = nullptr;               // [n]
  double *d_w = nullptr;               // [n]
  double *d_mu = nullptr;              // [n][nobs] multipliers
  double *d_part = nullptr;            // [4][FEA_RED_BLOCKS] per-workgroup partials of k_contact_info
  void release() { dev_free({d_node, d_w, d_mu, d_part}); *this = ContactState(); }
};

// consistent mass and the kinematic state of the Newmark steps (kernels_mass.hip).  The parameters of the last
// feahip_set_mass call stay on the host: m holds the block rows of the shard installed when it was assembled and is
// assembled again (mass_ensure) when the shard has changed since.
struct MassState {
  bool set = false;                    // feahip_set_mass was called with n_rho > 0 and not cleared since
  bool stale = false;                  // a per-material mass whose material count changed: every use is FEAHIP_ESTATE
  int n_rho = 0, n_mat = 0, Gm = 0;    // n_mat: the material count the densities were given for
  std::vector<double> rho, w, N, dN;   // [n_rho], [Gm], [Gm][npe], [Gm][3][npe]
  double *d_m_base = nullptr;          // [kb1 - kb0] one double per owned block of K's pattern
  double *d_m = nullptr;               // d_m_base - kb0: indexed by GLOBAL block number, as d_K
  long long kb0 = -1, kb1 = -1;        // the window m was assembled for
  // node vectors in the 32-byte layout of d_x ([N][4], the fourth double stays 0), all nodes of the context
  double *d_vel = nullptr, *d_acc = nullptr, *d_xt = nullptr, *d_vt = nullptr;
  double *d_body = nullptr;            // [3N] F_body = M (1 (x) b) on the owned rows, at load factor 1; null: none
  double body[3] = {0, 0, 0};
  double time = 0;
  // explicit steps (lump_ensure): nothing below exists until an explicit entry asks for it
  double *d_ml = nullptr;              // [N] HRZ lumped mass of the owned rows [ml_row0, ml_row1), zero elsewhere
  int ml_row0 = -1, ml_row1 = -1;      // the rows ml was built for
  double *d_ke_part = nullptr;         // [4 FEA_RED_BLOCKS] per-workgroup partial sums of 1/2 ml |v|^2
  int ke_parts = 0;                    // partial sums the last explicit step left for the velocities in force (0: none)
  void release_m() { dev_free({d_m_base}); d_m_base = d_m = nullptr; kb0 = kb1 = -1; }
  void release_lump() { dev_free({d_ml, d_ke_part}); d_ml = d_ke_part = nullptr; ml_row0 = ml_row1 = -1; ke_parts = 0; }
  void release() { dev_free({d_m_base, d_vel, d_acc, d_xt, d_vt, d_body, d_ml, d_ke_part}); *this = MassState(); }
};

// Rayleigh damping C = alpha M + beta K_d (kernels_damping.hip).  M is the mass of the loop that runs (it is not copied);
// K_d is a snapshot of the plain tangent at the x of feahip_set_damping, stored like d_K over the owned window of the
// shard installed then.  Nothing of it exists, and nothing of kernels_damping.hip is launched, while both are 0.
struct DampingState {
  double alpha = 0, beta = 0;
  double *d_Kd_alloc = nullptr;        // the allocation; d_Kd_base = d_Kd_alloc + (kb0 & 1), the 16-byte phase of K
  double *d_Kd_base = nullptr;         // [kb1 - kb0][3][3], null unless beta > 0
  double *d_Kd = nullptr;              // d_Kd_base - 9 kb0: indexed by GLOBAL block number, as d_K
  int row0 = -1, row1 = -1;            // the shard the snapshot was taken for
  bool on() const { return alpha > 0.0 || beta > 0.0; }
  void release() { dev_free({d_Kd_alloc}); *this = DampingState(); }
};

// result recovery (kernels_results.hip): nothing of it exists until a results entry is called
struct ResultState {
  double *d_rec = nullptr;             // [E][8] element records: sum vol sigma (6), sum vol, W_e
  double *d_sig6 = nullptr;            // [N][6] nodal stress xx yy zz xy yz xz of the owned rows, zero elsewhere (library ids)
  double *d_vm = nullptr, *d_wt = nullptr, *d_wn = nullptr;   // [N] von Mises, weight, nodal energy share
  double *d_part = nullptr;            // [FEA_RED_BLOCKS] per-workgroup partial sums of the nodal energy shares
  void release() { dev_free({d_rec, d_sig6, d_vm, d_wt, d_wn, d_part}); *this = ResultState(); }
};

// modal analysis (kernels_modal.hip): nothing of it exists until feahip_solve_modes (or one of its hooks) is called.
// Block vectors are [3N][FEA_MODAL_COLS] doubles, the columns of a dof contiguous.
// The nine block vectors of ModalState::d_v, and the sums of a step: 24 column norms (s 8 + column, s = 0 |r|^2, 1 |Kx|^2,
// 2 |Mx|^2), then 12 x 64 Gram sums (block pair q, M: 0..5, K: 6..11, the pairs (X,X) (X,W) (X,P) (W,W) (W,P) (P,P), entry
// (a, b) at 24 + q 64 + a 8 + b).  Sum e of workgroup b is at d_part[e FEA_RED_BLOCKS + b]; reduced, at d_small[e].
enum { V_X = 0, V_W = 1, V_P = 2, V_KX = 3, V_KW = 4, V_KP = 5, V_MX = 6, V_MW = 7, V_MP = 8 };
#define MODAL_NORMS 24
#define MODAL_GRAM (12 * 64)
#define MODAL_SUMS (MODAL_NORMS + MODAL_GRAM)
#define MODAL_SMALL (24 + 12 * 64 + 24 * 16 + FEA_MODAL_COLS)
static_assert(MODAL_SMALL == MODAL_SUMS + 24 * 16 + FEA_MODAL_COLS, "the layout of ModalState::d_small: sums, C[24][16], theta[8]");
struct ModalState {
  double *d_v = nullptr;               // [9][3N][8]: X W P, KX KW KP, MX MW MP
  double *d_part = nullptr;            // [24 + 768][FEA_RED_BLOCKS] per-workgroup partial sums: column norms, Gram entries
  double *d_small = nullptr;           // [MODAL_SMALL]: the reduced sums, then C[24][16] and theta[8] of the step
  std::vector<double> h_C;             // host copy of C and theta while their upload is in flight
  double theta[FEA_MODAL_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
  int n_free = 0;                      // dofs that are not prescribed
  bool have = false;                   // X holds the modes of a finished solve (feahip_get_modes, warm restarts)
  // the locked store of feahip_solve_modes_locked: nothing of it exists until that entry (or one of its hooks) is called
  double *d_lock = nullptr;            // [2][lock_panels][3N][8]: the panels of Q, then those of MQ = mask(M Q)
  double *d_lpart = nullptr;           // [lock_panels * 64][FEA_RED_BLOCKS] per-workgroup partial sums of MQ' W
  double *d_lcoef = nullptr;           // [lock_panels * 64] the coefficients MQ' W (they never visit the host)
  int lock_panels = 0;                 // panels allocated (once, for the n_modes asked; a larger request reallocates)
  int n_locked = 0;                    // modes in the store
  int lock_order[64] = {0};            // mode j of the ascending lambda is column lock_order[j] of the store
  double lam[64] = {0};                // the UNSHIFTED lambda of mode j, ascending (the response entries read it)
  double shift = 0;                    // the shift of the solve that filled the store (0: feahip_response_set_basis)
  int lock_gen = 0;                    // counts the fillings of the store: a response load belongs to one of them
  bool have_locked = false;            // the store holds the modes of a locked solve (feahip_get_locked_modes)
  bool have_buckling = false;          // X holds the buckling modes of feahip_solve_buckling (feahip_get_buckling_modes)
  // the sharded solve (feahip_solve_modes_sharded, feahip_group_spmm_km): nothing of it exists until one of them is called
  double *d_bsend = nullptr, *d_brecv = nullptr;   // [24 nsend], [24 nrecv]: halo rows of a block vector, 192 bytes each
  int *d_key = nullptr;                // [row1 - row0] the whole-mesh node of every owned row (rank contexts; null: row0 + a)
  int blk_nsend = -1, blk_nrecv = -1;  // the halo plan the buffers were allocated for
  int key_row0 = -1, key_row1 = -1;    // the rows d_key and n_free_own were built for
  int n_free_own = 0;                  // free dofs among the owned rows
  bool have_sharded = false;           // X holds, on the rows [sh_row0, sh_row1), the modes of a finished sharded solve
  int sh_row0 = -1, sh_row1 = -1;
  void release() { dev_free({d_v, d_part, d_small, d_lock, d_lpart, d_lcoef, d_bsend, d_brecv, d_key}); *this = ModalState(); }
};

// frequency response by mode superposition (kernels_response.hip): nothing of it exists until a response entry is called.
// It reads the locked store of ModalState (Q's panels, lock_order, lam, shift) and owns what one load adds to it.
struct ResponseState {
  double *d_us = nullptr;              // [3N] the static correction u_s in library ids; zero without one
  double *d_part = nullptr;            // [64][FEA_RED_BLOCKS] per-workgroup partial sums of Q' F, by store column
  double *d_q = nullptr;               // [64] Q' F by store column
  double *d_coef = nullptr;            // [FEA_RESPONSE_MAX_FREQ][2][64] the coefficient table of a sweep: re, im by store column
  double *d_out = nullptr;             // [2][3N]: peak and (as int) peak_at of a sweep, or re and im of a field
  double q[64] = {0};                  // q_k of the ascending mode k
  bool loaded = false;                 // a load is held ...
  int gen = -1;                        // ... for the filling ModalState::lock_gen == gen of the store
  int correction = 0;                  // it was made with the static correction
  int swept_freq = 0;                  // frequencies in d_coef from the last sweep (feahip_time_kernel 23)
  int trans_rows = 0;                  // rows in d_coef from the last chunk of the last transient (feahip_time_kernel 25) ...
  int trans_step0 = 0;                 // ... and the step of its first row
  double *d_form = nullptr;            // [FEA_COMBINE_TABLE] the form of the last combination, by store column: T[64][64] (C folded
                                       // onto its upper triangle), b[64], s (kernels_combine.hip); allocated by the first one
  bool form_set = false;               // d_form holds a form (feahip_time_kernel 26) ...
  bool form_abs = false;               // ... to be taken on |phi| ...
  int form_gen = -1;                   // ... laid out for the filling form_gen of the store
  int load_count = 0;                  // counts the loads made: T_s of the stress store belongs to one of them
  void release() { dev_free({d_us, d_part, d_q, d_coef, d_out, d_form}); *this = ResponseState(); }
};

// stress from mode superposition (kernels_modal_stress.hip, kernels_stress_combine.hip): nothing of it exists until a stress
// entry is called.  The store belongs to the filling `gen` of the locked store and T_s to the load number `load_count`.
struct StressState {
  double *d_rec = nullptr;             // [E][6][8] element records of one panel: sum_g vol dsigma, component by column
  double *d_evol = nullptr;            // [E] sum_g vol
  double *d_vec = nullptr;             // [3N] a single vector in library ids (feahip_stress_increment)
  double *d_in = nullptr;              // [3N][8] the panel of a single vector: column 0 live
  double *d_one = nullptr;             // [6N][8] its stress panel (and where feahip_time_kernel 27 writes)
  double *d_out6 = nullptr;            // [6N] an output of six components per node (library ids)
  double *d_vm = nullptr;              // [N] a von Mises output
  double *d_ts = nullptr;              // [6N] T_s, the stress of the static correction; zero without one
  double *d_store = nullptr;           // [store_panels][6N][8] the stress store, column for column the locked store's
  double *d_form = nullptr;            // [FEA_COMBINE_TABLE] the form of the last stress combination (feahip_time_kernel 28)
  double *d_fcoef = nullptr;           // [64 + 8] the coefficients of the last feahip_response_stress_field, then cs
  double *d_scoef = nullptr;           // [FEA_RESPONSE_MAX_FREQ][2][64] the table of the stress sweeps (kernels_stress_sweep.hip): its
                                       // own, so the tables of the displacement sweeps stay; allocated by the first one
  int *d_at6 = nullptr;                // [6N] the row index of every stress row's peak ...
  int *d_vmat = nullptr;               // [N] ... and of every node's von Mises peak
  int swept_freq = 0;                  // frequencies in d_scoef from the last stress sweep (feahip_time_kernel 29)
  int trans_rows = 0;                  // rows in d_scoef from the last chunk of the last stress transient (hook 30) ...
  int trans_step0 = 0;                 // ... and the step of its first row
  int table_gen = -1;                  // the filling of the locked store d_scoef was laid out for
  int store_panels = 0;                // panels allocated
  bool have = false;                   // the store holds the stresses of the modes held ...
  int gen = -1;                        // ... of the filling ModalState::lock_gen == gen ...
  int load_count = -1;                 // ... and T_s that of the load ResponseState::load_count == load_count ...
  int material = -1;                   // ... over the elements of this material (-1: all)
  bool form_set = false;               // d_form holds a form for this store ...
  bool form_abs = false;               // ... to be taken on |T|
  void release() { dev_free({d_rec, d_evol, d_vec, d_in, d_one, d_out6, d_vm, d_ts, d_store, d_form, d_fcoef, d_scoef, d_at6, d_vmat}); *this = StressState(); }
};

// linear buckling (kernels_buckling.hip): nothing of it exists until feahip_solve_buckling (or one of its hooks,
// feahip_geometric_spmv and feahip_time_kernel 18-19) is called.  kg is stored like MassState::d_m.
struct BucklingState {
  double *d_rec = nullptr;             // [E][npe (npe + 1) / 2] the upper triangle of every element's scalar matrix G_e
  double *d_kg_base = nullptr;         // [kb1 - kb0] one double per owned block of K's pattern
  double *d_kg = nullptr;              // d_kg_base - kb0: indexed by GLOBAL block number, as d_K
  long long kb0 = -1, kb1 = -1;        // the window kg is allocated for
  double *d_x4 = nullptr;              // [N][4] the vector of feahip_geometric_spmv in the node layout
  void release() { dev_free({d_rec, d_kg_base, d_x4}); *this = BucklingState(); }
};

// random-vibration fatigue on the stress store (kernels_stress_fatigue.hip): nothing of it exists until a fatigue entry is
// called.  It reads the stress store and T_s of StressState; a new stress basis drops what it holds (stress_basis).
struct FatigueState {
  double *d_forms = nullptr;           // [4][FEA_COMBINE_TABLE] the four forms of the last moments, folded as StressState::d_form
  double *d_mom = nullptr;             // [4][N][7] the moments of order 0, 1, 2, 4: six components, then the von Mises process
  double *d_rates = nullptr;           // [N][7][2] nu0, nup
  double *d_damage = nullptr;          // [N][7][3] narrow band, Dirlik, Tovo-Benasciutti, per unit time
  int *d_status = nullptr;             // [N][7] the bits FEA_FATIGUE_* of fatigue_point.h
  double consts[5] = {0};              // the S-N curve of the last rates (fatigue_constants)
  bool forms_set = false;              // d_forms holds four forms for the stress store in force (feahip_time_kernel 31) ...
  bool mom_set = false;                // ... d_mom their moments ...
  bool rates_set = false;              // ... and consts a curve (feahip_time_kernel 32)
  void drop() { forms_set = mom_set = rates_set = false; }
  void release() { dev_free({d_forms, d_mom, d_rates, d_damage, d_status}); *this = FatigueState(); }
};

// rainflow counting of a transient on the stress store (kernels_stress_rainflow.hip): nothing of it exists until
// feahip_response_stress_rainflow is called.  It reads the stress store and T_s of StressState and has a coefficient chunk
// of its own, so the tables of the other entries stay.
struct RainflowBuffers {
  double *d_coef = nullptr;            // [FEA_TRANSIENT_CHUNK][64] the rows of a chunk, then its g[FEA_TRANSIENT_CHUNK]
  double *d_proj = nullptr;            // [FEA_RAINFLOW_MAX_PROJ][6] the projections of the last call
  double *d_stack = nullptr;           // [depth_cap][6N] the ring of every stress row, slot by slot
  double *d_real = nullptr;            // [4][6N] per row: the last kept sample, the damage, the cycles, the largest range
  int *d_int = nullptr;                // [6][6N] per row: direction, base, count, depth used, status, seen
  int depth_cap = 0;                   // slots d_stack is allocated for
  int depth = 0;                       // the depth of the last call ...
  double sn[2] = {0, 0};               // ... its b and 1 / A ...
  int rows = 0, step0 = 0;             // ... and the rows of its last chunk in d_coef (feahip_time_kernel 33)
  int table_gen = -1;                  // the filling of the locked store d_coef was laid out for
  void release() { dev_free({d_coef, d_proj, d_stack, d_real, d_int}); *this = RainflowBuffers(); }
};

struct feahip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  // sizes
  int N = 0, E = 0, npe = 0, G = 0, ndof = 0;
  int nnzb = 0;               // 3x3 blocks in the full symmetric pattern
  int nchunks = 0;
  int chunk0 = 0, nchunks_local = 0;  // this rank's share of the chunks (row shard)
  int nachunks = 0, achunk0 = 0, nachunks_local = 0;   // same for the staged kernel's partition
  std::vector<int> h_super_achunk, h_chunk;
  // row shard of a multi-rank solve: this rank owns nodes [row0, row1)
  int rank = 0, nranks = 1, row0 = 0, row1 = 0;
  struct Transport *tr = nullptr;      // null: single rank, no exchange
  bool owns_tr = false;
  std::vector<int> peer, send_off, recv_off;   // halo plan: per peer, ranges into the index lists
  int nsend = 0, nrecv = 0;
  int *d_send_idx = nullptr, *d_recv_idx = nullptr;
  double *d_send_buf = nullptr, *d_recv_buf = nullptr;
  int max_rowlen = 0;
  bool linear_tet = false;    // npe == 4 and dN is the constant-strain table
  int model = 0;
  double lambda = 0, mu = 0;
  // material table (feahip_set_materials): n_materials = 0 is the single pair above.  h_elem_mat is in the order of
  // the context's own elements (a rank context: its local elements)
  int n_materials = 0;
  std::vector<double> h_mat_params;    // [n_materials][2] lambda, mu
  std::vector<uint8_t> h_elem_mat;     // [E]
  double2 *d_mat = nullptr;            // [n_materials] (lambda, mu)
  uint8_t *d_elem_mat = nullptr;       // [E]
  double *d_f_discard = nullptr;       // [3N] where the residual of a K-only gather assembly with a table goes (kernels_gather.hip)
  int strategy = FEAHIP_ASM_AUTO;
  int last_strategy = FEAHIP_ASM_AUTO;   // what the most recent assembly launch ran

  ElemTable table;
  ElemTable *d_table = nullptr;

  // mesh (device)
  int *d_conn = nullptr;       // [E][npe]
  double *d_X0 = nullptr;      // [N][4] padded to 32 B (two dwordx4 per node)
  double *d_x = nullptr;       // [N][4] current configuration
  // block-CSR pattern of K (built once; topology never changes)
  int *d_rowptr = nullptr;     // [N+1]
  int *d_colidx = nullptr;     // [nnzb]
  // K holds the block rows this rank owns and nothing else: blocks [kb0, kb1) = rowptr[row0] .. rowptr[row1] (all of
  // them for an unsharded context).  It is allocated on first use, for the shard installed by then, so a rank of a
  // sharded run never holds the other ranks' rows (the reference keeps one row-wise store, fea_solver.c:444-448,
  // and its modified-Newton copy, :179).  Kernels index by GLOBAL block number through d_K = d_K_base - 9 kb0.
  double *d_K = nullptr;       // [nnzb][3][3], valid for blocks [kb0, kb1) only
  double *d_Kstash = nullptr;  // modified-Newton copy (fea_solver.c:179), same window
  double *d_K_base = nullptr, *d_Kstash_base = nullptr;   // first owned value (block kb0) of each
  double *d_K_alloc = nullptr, *d_Kstash_alloc = nullptr; // the allocations: d_K_base = d_K_alloc + (kb0 & 1), so that even GLOBAL value indices are 16-byte aligned on every rank
  long long kb0 = 0, kb1 = 0;
  bool have_stash = false;
  int *d_chunk = nullptr;      // [nchunks+1] first row of every chunk
  int *d_diag = nullptr;       // [N] index of the diagonal block of every row
  // maps of the assembly strategies (MapCache), built the first time a launch asks for them
  GenericMaps generic;         // ROWOWNER, ATOMIC
  VisitMaps visits;            // STAGED
  QuadMaps quad;               // SHARED
  GatherMaps gather;           // GATHER of linear tetrahedra
  Gather10Maps gather10;       // GATHER of 10-node tetrahedra and 8-node bricks
  // vectors (3N doubles)
  double *d_f = nullptr, *d_u = nullptr;
  double *d_r = nullptr, *d_p = nullptr, *d_q = nullptr, *d_minv = nullptr;
  double *d_part = nullptr;    // reduction partials, 6 x FEA_RED_BLOCKS
  // single-reduction PCG (kernels_solve.hip): preconditioned residual z = M r and w = K z (allocated on first use);
  // pcg_variant: -1 = single-reduction when sharded, the reference-shaped two-reduction loop otherwise; 0 / 1 force
  double *d_z = nullptr, *d_w = nullptr, *d_s = nullptr;
  int pcg_variant = -1;
  // SpMV chunks [chunk0 + ichunk_lo, chunk0 + ichunk_hi) of this rank touch no halo column: they run while the halo
  // rows are in flight (everything, for an unsharded context)
  int ichunk_lo = 0, ichunk_hi = 0;
  hipStream_t comm_stream = nullptr;   // RCCL transport: halo exchange beside the interior product
  hipEvent_t ev_packed = nullptr, ev_unpacked = nullptr;
  double *d_scal = nullptr;    // device scalars of the CG recurrences
  int *d_flag = nullptr;       // [0] converged-at iteration, [1] bad Gauss pts
  // prescribed displacements
  int n_presc = 0;             // nodes in the deck
  int n_cdof = 0;              // constrained dofs, deck order x,y,z per node
  int *d_cdof = nullptr;
  double *d_cval = nullptr;    // prescribed value per constrained dof
  uint8_t *d_dofmask = nullptr;// [3N] 1 = constrained
  // cached per-Gauss-point state for the getters
  double *d_F = nullptr, *d_S = nullptr;   // [E][G][9]
  bool state_valid = false;

  // host copies needed by getters / pattern export
  std::vector<int> h_rowptr, h_colidx;
  // The maps of a strategy (gather chunks, staged visits, generic incidence lists) are built the first time it is
  // asked for, from these host copies.
  std::vector<int> h_conn;
  struct HostPattern *h_pat = nullptr;
  bool incslot_ok = false;     // the mesh has incidence slots (row length <= 255)

  int last_bad = 0;

  // library-side node numbering (renumber.cpp): everything in the context -- mesh arrays, pattern, K, vectors, shard
  // ranges -- lives in the library's numbering; the ABI translates at its boundary.  Empty = the caller's numbering.
  std::vector<int> perm, iperm;        // perm[caller id] = library id, iperm = its inverse
  // a rank context (feahip_create_rank): this context IS one rank's sub-mesh, locally indexed; its "caller ids" are the
  // local ids, rank_node_global / rank_elem_global say which nodes and elements of the whole mesh they are
  int rank_own = -1;                   // nodes it owns (local ids [0, rank_own)); -1: an ordinary context
  std::vector<int> rank_node_global, rank_elem_global;
  int rank_n_global = 0;
  int rank_e_global = 0;               // elements of the whole mesh (feahip_create_rank; 0 where the context never saw it)
  bool rank_local_ids = false;         // feahip_create_rank_local: the caller speaks local ids (surface faces included)

  // preconditioner of PCG_ILU / CHOLESKY solves: 0 = 3x3 block-Jacobi, 1 = aggregation multigrid (amg.h), 2 = the
  // multigrid plus a coarse level across the ranks (coarse.h)
  // which matrix d_K holds: bumped by every stiffness assembly, copied by stash / restore; k_bc = prescribed-dof
  // masking applied since.  Only used to skip numeric re-setup of the multigrid hierarchy for an unchanged K
  // (modified Newton restores the same matrix every iteration); a stale hierarchy would cost iterations, not accuracy.
  unsigned long long k_epoch = 0, stash_epoch = 0;
  bool k_bc = false;
  bool k_valid = false;                // a stiffness assembly has filled d_K since it was (re)allocated
  // golden-section line search along the Newton step: iterations (0 = off, the reference's solve())
  int linesearch_max = 0;
  int precond = 0;
  void *amg = nullptr;         // AmgHierarchy, built on first use
  // kind 2: the multigrid plus one coarse level across the ranks (coarse.h); nothing of it exists under kinds 0 and 1
  void *coarse = nullptr;      // RankCoarse, built on first use
  double *d_vred = nullptr;    // buffer of the vector all-reduce (Transport::allreduce_vec)
  size_t vred_cap = 0;         // its length in doubles
  // surface loads: f = load_factor * F_ext(x) - T(x) in every residual assembly; feahip_update_nodes_with_bc adds its
  // lambda to load_factor (one increment of the loads per step, as of the prescribed displacements)
  SurfaceLoads surf;
  double load_factor = 0;
  ContactState contact;
  // two-column solve (kernels_solve2.hip), allocated on first use: paired vectors [3N][2] (the two columns interleaved
  // per dof), the second column's solution as a plain vector, and the columns' partial sums, scalars and flags
  double *d2_f = nullptr, *d2_u = nullptr, *d2_r = nullptr, *d2_p = nullptr, *d2_q = nullptr;
  double *d_u2 = nullptr;      // [3N]
  double *d2_part = nullptr;   // 8 x FEA_RED_BLOCKS
  double *d2_scal = nullptr;   // 2 x 8
  int *d2_flag = nullptr;      // [2]
  // consistent mass (kernels_mass.hip): nothing of it exists, and nothing below is launched, until feahip_set_mass
  MassState mass;
  DampingState damping;
  ResultState results;
  ModalState modal;
  ResponseState response;
  StressState stress;
  BucklingState buckling;
  FatigueState fatigue;
  RainflowBuffers rainflow;
};

// calls f(std::integral_constant<bool, DOK>, std::integral_constant<bool, DOF>) for the assembly asked for: K and f,
// K alone or f alone -- the three instantiations every assembly kernel has
template <class F>
void with_kf(bool doK, bool doF, F &&f)
{
  if (doK && doF) f(std::true_type(), std::true_type());
  else if (doK)   f(std::true_type(), std::false_type());
  else            f(std::false_type(), std::true_type());
}

// launchers (kernels_assemble.hip / kernels_patch.hip / kernels_solve.hip)
// plain: without the contact term (dist_stable_step, which puts its own bound of it on top)
int launch_assemble(feahip_ctx *c, bool doK, bool doF, bool plain = false);
int launch_state_export(feahip_ctx *c, double *d_grads = nullptr, double *d_detj = nullptr);
int launch_apply_bc(feahip_ctx *c, double lambda);
int launch_update_nodes_bc(feahip_ctx *c, double lambda);
// kernels_surface.hip: adds load_factor * F_ext of the loaded faces to the owned rows of f (nothing without loads)
int launch_surface_loads(feahip_ctx *c, double *d_fv);
// kernels_surface.hip, host only: (owning element, local face) of every face, node ids in the numbering of conn;
// -1 when all resolve, else the index of the first bad face with the reason in why
int resolve_surface_faces(int N, int E, int npe, const int *conn, int nfaces, int npf, const int *face_nodes,
                          int *face_elem, int *face_local, std::string &why);
int set_surface_loads(feahip_ctx *c, int nfaces, int npf, const int *face_nodes, const int *kind, const double *values);
// kernels_surface.hip, host only: the caller's faces in the context's node ids and their elements' face order; a rank
// keeps those touching a node it owns (keep = their indices in the caller's list).  FEAHIP_EINVAL and the reason in c->err
int context_surface_faces(feahip_ctx *c, int nfaces, int npf, const int *face_nodes, std::vector<int> &fn, std::vector<int> &keep);
// kernels_contact.hip -- node-to-rigid-surface contact on the owned contact nodes (nothing to launch without contact)
int set_contact(feahip_ctx *c, int nfaces, int npf, const int *face_nodes, int n_obstacles, const int *kind,
                const double *geom, double penalty, int augment_max, double gap_tolerance);
void contact_owned(const feahip_ctx *c, int &n0, int &n1);      // the range of ContactState::h_node this rank owns
int launch_contact(feahip_ctx *c, bool doK, bool doF, double *d_fv);   // d_fv += F_c; K's diagonal blocks += K_c
int launch_contact_bound(feahip_ctx *c);                       // K's diagonal blocks += w eps n n' of EVERY pair (stable step)
int launch_contact_augment(feahip_ctx *c);                     // mu <- max(0, mu + eps p)
int launch_contact_info(feahip_ctx *c);                        // d_scal[8 .. 12) = active pairs, sum w t, Pi_c, max penetration (own rows)
int launch_contact_status(feahip_ctx *c, double *d_gap, double *d_pressure);   // [N] each, written at the owned contact nodes
// drivers.hip -- the four numbers over all ranks (out: active, max penetration, force, Pi_c); the multiplier update
int dist_contact_info(std::vector<feahip_ctx *> &R, double *out);
int dist_contact_augment(std::vector<feahip_ctx *> &R, double *max_penetration);
int ensure_generic_maps(feahip_ctx *c);
int ensure_k(feahip_ctx *c);
void release_k(feahip_ctx *c);
int ensure_visits(feahip_ctx *c);
int dist_nodes_add_scaled(std::vector<feahip_ctx *> &R, double eta, bool exchange);
int launch_update_nodes_solution(feahip_ctx *c, const double *d_u);
int launch_spmv(feahip_ctx *c, const double *d_xv, double *d_yv);
int precond_apply(feahip_ctx *c, const double *r, const double **z);   // kernels_solve.hip
int solve_pcg(feahip_ctx *c, int type, double tol, int max_iter, int *iters,
              double *resid);
int time_pcg_iteration(feahip_ctx *c, int warmup, int iters, double *avg_ms);
// host half shared by the PCG loops (kernels_solve.hip): iterations and residual from a stop flag and its scalars
bool pcg_outcome(int flag, int it, const double *scal, int *iters, double *resid);
// out[k] = sum of part[k*stride .. k*stride+n) for k < nsums, on the context's stream (k_reduce_final, reduce_device.h)
void enq_reduce_final(feahip_ctx *c, int n, int nsums, int stride, const double *part, double *out);
void enq_precond_blockjacobi(feahip_ctx *c);                            // kernels_solve.hip
// kernels_solve2.hip -- K [u, u2] = [f, f2] over one read of K per iteration; paired vectors are [3N][2]
int ensure_solve2(feahip_ctx *c);
void release_solve2(feahip_ctx *c);
int solve2_refused(feahip_ctx *c, const char *who);                     // FEAHIP_EINVAL and the reason in c->err, or OK
int launch_spmv2(feahip_ctx *c, const double *d_x2, double *d_y2);
int launch_interleave(feahip_ctx *c, const double *a, const double *b, double *out2);
int launch_deinterleave(feahip_ctx *c, const double *in2, double *a, double *b);
int solve_pcg2(feahip_ctx *c, int type, double tol, int max_iter, int *iters, double *resid);   // d2_f -> d_u, d_u2
int time_pcg2_iteration(feahip_ctx *c, int warmup, int iters, double *avg_ms);
// kernels_modal.hip -- the lowest eigenpairs of K phi = lambda M phi by a blocked LOBPCG on eight columns
int ensure_modal(feahip_ctx *c);
int modal_solve(feahip_ctx *c, int n_modes, double tol, int max_it, int warm, double *lambda, double *resid, int *iters);
int modal_get(feahip_ctx *c, int col, double *h_lib);                   // column col of X, [3N] in library ids
// Y = K X, Z = mask(m X) on the chunks [first, first + n) of the context's own (all of them: 0, nchunks_local), m one
// double per block of K's pattern (mass.d_m, buckling.d_kg); an empty range launches one idle workgroup
int launch_spmm_km(feahip_ctx *c, int first, int n, const double *d_m, const double *d_x8, double *d_y8, double *d_z8);
int launch_modal_hash(feahip_ctx *c, double *d_v8);                     // the start block into a whole block vector
int launch_modal_pack(feahip_ctx *c, const double *d_in, double *d_out, int unpack); // [8][3N] <-> [3N][8]
int time_modal_prepare(feahip_ctx *c);                                  // the nine vectors filled for feahip_time_kernel 13-15
int time_modal_kernel(feahip_ctx *c, int what);
int modal_ritz(int ns, const double *GM, const double *GK, int m, double *theta, double *C);   // host only
// the same solve over the ranks R of a sharded run (collective); the block product over the ranks for the test hook
int modal_solve_dist(std::vector<feahip_ctx *> &R, int n_modes, double tol, int max_it, int warm, double *lambda,
                     double *resid, int *iters);
int modal_spmm_km_dist(std::vector<feahip_ctx *> &R);                   // [KX, MX] <- [K X, mask(M X)] on the owned rows, X's halo rows exchanged
int ensure_modal_dist(feahip_ctx *c);                                   // ensure_modal, the block halo buffers and the row keys
// the halo rows of a block vector [3N][8], twelve 16-byte lanes per row: into ModalState::d_bsend on the context's
// stream, out of d_brecv on `stream`, and (test knob) NaN into the halo rows on the context's stream
void modal_enq_block_pack(feahip_ctx *c, const double *d_v8);
void modal_enq_block_unpack_on(feahip_ctx *c, double *d_v8, hipStream_t stream);
void modal_enq_block_poison(feahip_ctx *c, double *d_v8);
// the same pencil with a shift, in sweeps of the eight-column block with hard locking: up to FEA_MODAL_MAX_LOCKED modes
int modal_solve_locked(feahip_ctx *c, int n_modes, double shift, double tol, int max_it, double *lambda, double *resid,
                       int *iters, int *sweeps);
int modal_get_locked(feahip_ctx *c, int mode, double *h_lib);           // mode of the locked store, [3N] in library ids
int ensure_locked(feahip_ctx *c, int n_modes);                          // the store for n_modes, zeroed and empty
double *locked_panel(feahip_ctx *c, int mq, int panel);                 // panel of Q (mq = 0) or of MQ (1), [3N][8]
int launch_deflate(feahip_ctx *c, double *d_w8, int n_locked);          // W -= Q (MQ' W) against the first n_locked modes
int time_deflate_prepare(feahip_ctx *c);                                // eight panels of hash for feahip_time_kernel 16-17
int time_deflate_kernel(feahip_ctx *c, int what);
// The iteration the four eigenvalue drivers share (modal_solve, modal_solve_locked, modal_solve_dist, buckling_solve).
// A driver assembles its matrix and its preconditioner, makes its start block in X, says below what differs and calls
// run() once, or once per sweep; the ending -- error text, flags, locking, lambda and resid -- is the driver's again.
enum { LOBPCG_CONVERGED = 0, LOBPCG_OUT_OF_STEPS = 1, LOBPCG_BROKE = 2 };   // run() < 0: the code of a HIP or transport error
struct Lobpcg {
  std::vector<feahip_ctx *> R;         // the contexts driven here; the host side of a step (theta, h_C) lives on R[0]
  struct Transport *T;                 // null: R is one unsharded context -- one full-range product, the sums read straight
                                       // out of d_small.  Else every rank works on its owned rows: the halo rows of a block
                                       // exchanged under the interior product, the sums all-reduced through d_vred
  double tol;                          // of the stop test ||r_j|| <= tol (||K x_j|| + |theta_j| ||M x_j||)
  bool geometric = false;              // the pencil (K_sigma, K): buckling.d_kg stands beside K in place of mass.d_m, and the
                                       // two products swap slots (K S into the "M" slots, mask(K_sigma S) into the "K" slots)
  bool renew_p = false;                // the renewal of every 20 steps makes the products of P again as well as those of X
  std::function<int()> after_residual; // between the preconditioned residual and W's products (the locked solve deflates W)
  std::function<bool(int ns, const double *GM)> veto;   // true refuses the Gram matrix of a Rayleigh-Ritz step: the basis "broke"
  double sums[MODAL_SUMS], GM[24 * 24], GK[24 * 24], ratio[FEA_MODAL_COLS];
  double *theta;                       // R[0]->modal.theta

  Lobpcg(const std::vector<feahip_ctx *> &ranks, struct Transport *transport, double tolerance);
  int products(int jx, int jk, int jm);   // block vectors [jk, jm] <- [K, mask(M)] jx (the slots swapped when geometric)
  int upload();                        // C and theta of the host to every rank
  int enq_residual(bool precond);      // R, its norms and W from X's products and theta, on every rank
  int read_sums(int e0, int n);        // the sums [e0, e0 + n) of all ranks into sums (one synchronisation)
  int fresh_norms();                   // the norms of X's products as they stand, into sums
  bool converged(int want);            // the stop test of the leading want columns on sums[0 .. 24); fills ratio
  bool ritz(int np, int *rank);        // theta and C from the Gram sums of np column blocks; false: the basis broke
  // X orthonormalised on its own, then steps until the leading want columns pass the stop test on fresh products or *it,
  // which counts the steps over all calls, reaches max_it.  One of LOBPCG_*, or an error code
  int run(int want, int max_it, int *it);
};
// kernels_response.hip -- frequency response by mode superposition on the locked store
int launch_response_mask8(feahip_ctx *c, double *d_v8);                 // a block vector [3N][8]: zero on the prescribed dofs
// the coefficient table [n_freq][2][64] (re, im; zero past n_modes) of mode k at column order[k] (null: k); host only.
// FEAHIP_EINVAL and *why for a negative or non-finite input and for a coefficient that is not finite
int response_coefficients(int n_modes, const double *lam, const double *q, const int *order, int n_freq, const double *omega,
                          double alpha, double beta, const double *zeta, int correction, double *coef, std::string *why);
// F (library ids, host; null: f holds it already, zero on the prescribed dofs) projected on the modes held and, with
// correction, K u_s = F solved; q[n_locked] ascending
int response_load(feahip_ctx *c, const double *h_F, int correction, int solver_type, double tol, int max_it, double *q,
                  int *iters, double *resid);
// one launch of k_response_sweep over the table of n_freq frequencies: peak / peak_at, or (field, n_freq = 1) re / im,
// [3N] in library ids; the curves of the probe dofs (library ids) on the host, [n_probe][n_freq]
int response_sweep(feahip_ctx *c, bool field, int n_freq, const double *omega, double alpha, double beta, const double *zeta,
                   double *h_out0, void *h_out1, int n_probe, const int *probe, double *probe_re, double *probe_im);
int time_response_kernel(feahip_ctx *c, int what);                      // feahip_time_kernel 23 (sweep), 24 (projection)
// transient_table.cpp -- the coefficient rows of a transient, host only: the exact propagator of every mode in long double.
// transient_check: FEAHIP_EINVAL and *why for what both transient entries refuse.  transient_begin: mode k of the arrays
// at column order[k] (null: k).  transient_rows: the rows of the next `count` steps, coef[count][64], zero past the modes;
// FEAHIP_EINVAL and *why for an entry that is not finite
struct TransientTable;
int transient_check(int n_modes, const double *lam, const double *q, int n_steps, double dt, const double *g, double alpha,
                    double beta, const double *zeta, int correction, int quantity, std::string *why);
TransientTable *transient_begin(int n_modes, const double *lam, const double *q, const int *order, int n_steps, double dt,
                                double alpha, double beta, const double *zeta, int correction, int quantity);
int transient_rows(TransientTable *T, const double *g, int count, double *coef, std::string *why);
void transient_end(TransientTable *T);
// kernels_transient.hip -- transient response by mode superposition on the load held, and the base-excitation load
int launch_base_load(feahip_ctx *c, const double *d_mr, double *d_f);   // f = -(M r) on the free dofs, 0 on the prescribed
// the chunked launches of k_transient_sweep over the whole history: peak / peak_at [3N] and the snapshots [n_snap][3N] in
// library ids, the histories of the probe dofs (library ids) on the host, [n_probe][n_steps + 1]
int response_transient(feahip_ctx *c, int n_steps, double dt, const double *g, double alpha, double beta, const double *zeta,
                       int quantity, double *h_peak, int *h_at, int n_probe, const int *probe, double *h_probe, int n_snap,
                       const int *snap_step, double *h_snap);
int time_transient_kernel(feahip_ctx *c);                               // feahip_time_kernel 25
// kernels_combine.hip -- one quadratic form of the mode values per dof: response spectrum and random vibration
#define FEA_COMBINE_TABLE (66 * 64)                                     // T[64][64], b[64], s, and padding to a whole row
// C[n_locked][n_locked], b[n_locked] (null: zero) and s by ascending mode; h_out[3N] in library ids
int response_combine(feahip_ctx *c, const double *C, const double *b, double s, bool absx, double *h_out);
int time_combine_kernel(feahip_ctx *c);                                 // feahip_time_kernel 26
// kernels_modal_stress.hip -- the linearised nodal stress of a panel of eight columns: the stress store and single vectors
int stress_ensure(feahip_ctx *c);                                       // the buffers, on the first call
int launch_stress_vector(feahip_ctx *c, const double *d_v, int material, double *d_out);   // d_out[6N] from d_v[3N], library ids
int stress_basis(feahip_ctx *c, int material);                          // the store of the modes held, T_s of the load held
int launch_stress_mode(feahip_ctx *c, int col, double *d_out);          // d_out[6N] = column col of the stress store
int time_stress_store(feahip_ctx *c);                                   // feahip_time_kernel 27
// kernels_stress_combine.hip -- quadratic forms and one linear combination of the modal stresses per node
int stress_combine(feahip_ctx *c, const double *C, const double *b, double s, bool absx, double *h_out6, double *h_vm);
int stress_field(feahip_ctx *c, const double *coef, double cs, double *h_out6, double *h_vm);
int time_stress_combine(feahip_ctx *c);                                 // feahip_time_kernel 28
// kernels_stress_sweep.hip -- stress peaks over a frequency sweep or a transient: peak6 / at6 [6N], vm / vm_at [N] in library
// ids, the probes (library node ids) [n_probe][rows][6]
int stress_sweep(feahip_ctx *c, int n_freq, const double *omega, double alpha, double beta, const double *zeta, double *h_peak6,
                 int *h_at6, double *h_vm, int *h_vmat, int n_probe, const int *probe, double *probe_re, double *probe_im);
int stress_transient(feahip_ctx *c, int n_steps, double dt, const double *g, double alpha, double beta, const double *zeta,
                     double *h_peak6, int *h_at6, double *h_vm, int *h_vmat, int n_probe, const int *probe, double *h_probe);
double harmonic_von_mises(const double re6[6], const double im6[6]);    // host only: the cycle peak, the kernel's arithmetic
int time_stress_sweep_kernel(feahip_ctx *c, int what);                  // feahip_time_kernel 29 (sweep), 30 (transient)
// kernels_stress_fatigue.hip -- four forms on the nine combinations of every node in one launch, and the fatigue statistics
// of the seven processes per node; every host array in library ids, null where not wanted
int stress_moments(feahip_ctx *c, const double *C4, const double *b4, const double *s4, double *h_mom /*[4][N][7]*/);
int stress_fatigue_rates(feahip_ctx *c, const double *k /*[5] fatigue_constants*/, double *h_rates /*[N][7][2]*/,
                         double *h_damage /*[N][7][3]*/, int *h_status /*[N][7]*/);
int time_stress_moments(feahip_ctx *c);                                 // feahip_time_kernel 31
int time_fatigue_rates(feahip_ctx *c);                                  // feahip_time_kernel 32
// kernels_stress_rainflow.hip -- the rainflow count of every stress row and of n_proj projections over a transient: the five
// outputs [N][6 + n_proj] in library ids (null where not wanted), the probes (library node ids) [n_probe][rows][6 + n_proj]
int stress_rainflow(feahip_ctx *c, int n_steps, double dt, const double *g, double alpha, double beta, const double *zeta,
                    double sn_b, double sn_a, int depth, int n_proj, const double *proj, double *h_damage, double *h_cycles,
                    double *h_range, int *h_status, int *h_used, int n_probe, const int *probe, double *h_probe);
int time_rainflow_kernel(feahip_ctx *c);                                // feahip_time_kernel 33
// rainflow_table.cpp -- false for what the rainflow entries refuse of the S-N curve and the ring
bool rainflow_arguments(double sn_b, double sn_a, int depth);
// fatigue_table.cpp -- k[5] = b, 1 / A, Gamma(1 + b), Gamma(1 + b / 2), 2^(b / 2) of the S-N curve N s^b = A, made in long
// double; FEAHIP_EINVAL for b outside [1, 64], A not positive, either not finite
int fatigue_constants(double sn_b, double sn_a, double *k);
// combine_table.cpp -- the forms of a PSD and of a response spectrum, host only, in long double.  Mode k of the arrays is
// row and column k of C[n_modes][n_modes] and entry k of b; FEAHIP_EINVAL and *why for what the entries refuse
int random_form(int n_modes, const double *lam, const double *q, int n_freq, const double *omega, const double *S, double alpha,
                double beta, const double *zeta, int correction, int quantity, double *C, double *b, double *s, std::string *why);
int spectrum_form(int n_modes, const double *lam, const double *q, const double *sa, double alpha, double beta, const double *zeta,
                  int rule, int correction, double zpa, int quantity, double *C, double *b, double *s, double *a /*[n_modes] the peak
                  modal values, or null*/, std::string *why);
int moment_form(int n_modes, const double *lam, const double *q, int n_freq, const double *omega, const double *S, double alpha,
                double beta, const double *zeta, int correction, int order /*0, 1, 2 or 4*/, double *C, double *b, double *s,
                std::string *why);
// kernels_buckling.hip -- K_sigma as one double per block, and the lowest eigenpairs of K_sigma phi = nu K phi
int geom_assemble(feahip_ctx *c);                                       // buckling.d_kg at the current nodes
int buckling_solve(feahip_ctx *c, int n_modes, double tol, int max_it, double *nu, double *resid, int *iters);
int time_geom_kernel(feahip_ctx *c, int what);                          // feahip_time_kernel 18 (elements), 19 (blocks)
// kernels_mass.hip -- consistent mass, body force and the vector kernels of the Newmark steps
int mass_set(feahip_ctx *c, int n_rho, const double *rho, int mass_points, const double *weights, const double *forms,
             const double *dforms);
int mass_ensure(feahip_ctx *c, const char *who);               // FEAHIP_ESTATE without a (valid) mass; m for the shard installed now
int mass_set_body_force(feahip_ctx *c, const double *b);
int launch_body_force(feahip_ctx *c, double *d_fv);            // d_fv += load_factor * F_body on the owned rows (nothing without one)
int launch_mass_add(feahip_ctx *c, double coef);               // K += coef M on the diagonal entries of every owned block
int launch_mass_residual(feahip_ctx *c, double a0);            // f -= a0 M (x - xt) on the owned rows
int launch_mass_product(feahip_ctx *c, const double *d_v4, double *d_y);   // y = M v on the owned rows, v in the node layout
int launch_block_product(feahip_ctx *c, const double *d_m, const double *d_v4, double *d_y);   // the same with m given (one double per block, global index)
int launch_newmark_predict(feahip_ctx *c, double dt, double beta, double gamma);
int launch_newmark_correct(feahip_ctx *c, double dt, double beta, double gamma);
int launch_vec3_to_nodes(feahip_ctx *c, const double *d_v3, double *d_v4);
// kernels_mass.hip -- HRZ lumped mass and the pointwise kernels of an explicit (central-difference) step
int lump_ensure(feahip_ctx *c, const char *who);               // mass_ensure, then ml for the rows installed now
int launch_explicit_kick(feahip_ctx *c, double dt);            // vh = v + dt/2 a (d_vt), u = dt vh; 0 on prescribed dofs
int launch_explicit_presc(feahip_ctx *c, double dlambda, double dt);   // vh = prescribed increment / dt on the prescribed dofs
int launch_explicit_finish(feahip_ctx *c, double dt);          // a = f / ml, v = vh + dt/2 a; partial sums of the kinetic energy
                                                               // (damped: a = (f / ml - alpha vh) / (1 + alpha dt / 2))
// kernels_damping.hip -- Rayleigh damping C = alpha M + beta K_d
int damping_set(feahip_ctx *c, double alpha, double beta);
int damping_ready(feahip_ctx *c, const char *who);             // FEAHIP_ESTATE when K_d is of another shard, or alpha > 0 has no mass
int launch_damp_residual(feahip_ctx *c, double a0, double c1); // f -= M (a0 d + alpha w) + beta K_d w, d = x - xt, w = vt + c1 d
int launch_damp_product(feahip_ctx *c, const double *d_v4, double *d_y);   // y = C v on the owned rows, v in the node layout
int launch_damp_add(feahip_ctx *c, double cm, double ck);      // K += cm M + ck K_d on the owned values (beta > 0 only)
int launch_damp_force(feahip_ctx *c);                          // f -= C v on the owned rows (through d_q)
int launch_kinetic_energy(feahip_ctx *c, double *d_out);       // *d_out = 1/2 sum ml |v|^2 over the owned rows
int launch_count_inverted(feahip_ctx *c);                      // d_flag[1] = elements with det J <= 0 (or NaN) at a Gauss point of x
// kernels_solve.hip -- Gershgorin bound max_i sum_j |K_ij| / ml(i) over the owned rows into d_scal[8]
int launch_gershgorin(feahip_ctx *c);
// drivers.hip -- Newmark steps and the consistent acceleration over one or more ranks
int dist_dynamic(std::vector<feahip_ctx *> &R, int n_steps, double dt, double beta, double gamma, double dlambda,
                 int max_newton, double desired_tolerance, int solver_type, double solver_tolerance, int solver_max_iter,
                 double *tol_log, int tol_log_cap, int *its_log, int *steps_done);
int dist_consistent_acceleration(std::vector<feahip_ctx *> &R, int solver_type, double tol, int max_iter);
// drivers.hip -- explicit steps, the stable step and the kinetic energy over one or more ranks
int dist_explicit(std::vector<feahip_ctx *> &R, int n_steps, double dt, double safety, int restep, double dlambda,
                  double *dt_log, int dt_log_cap, int *steps_done);
int dist_stable_step(std::vector<feahip_ctx *> &R, double *dt_crit);
int dist_kinetic_energy(std::vector<feahip_ctx *> &R, double *e);
// kernels_results.hip -- nodal stress, strain energy and reactions
int launch_results(feahip_ctx *c, int material, double *d_energy);   // both passes; *d_energy (may be null) = sum of the owned nodal energy shares
int launch_reactions(feahip_ctx *c, double *d_r, double *d_save);    // d_r = -residual on the owned prescribed dofs; d_f saved in d_save and restored
// drivers.hip -- the strain energy over one or more ranks
int dist_strain_energy(std::vector<feahip_ctx *> &R, double *W);
// drivers.hip -- Crisfield's cylindrical arc length on the surface loads (one unsharded context)
int arclength_solve(feahip_ctx *c, double lambda_max, int max_steps, int max_newton, double desired_tolerance,
                    int solver_type, double solver_tolerance, int solver_max_iter, double *lambda_log, double *tol_log,
                    int log_cap, int *its_log, int *steps_done);

// renumber.cpp -- locality numbering of the nodes; false = no basis for one (identity returned)
bool locality_numbering(int N, int E, int npe, const int *conn, const double *X, std::vector<int> &new_of_old);

// shard.cpp -- host-only plan of a row-sharded solve
struct ShardPlan {
  int rank = 0, nranks = 1, row0 = 0, row1 = 0;
  std::vector<int> peer, send_off, recv_off;   // [npeer], [npeer+1], [npeer+1]
  std::vector<int> send_idx, recv_idx;         // node ids, ascending inside every peer segment
};
// rows of rank k = rows of supers [nsuper*k/n, nsuper*(k+1)/n); chunk = SpMV chunk partition
void shard_row_range(const std::vector<int> &chunk, int rank, int nranks, int &row0, int &row1);
void build_shard_plan(const std::vector<int> &rowptr, const std::vector<int> &colidx,
                      const std::vector<int> &chunk, int rank, int nranks, ShardPlan &plan);

// rankmesh.cpp -- the sub-mesh one rank of a sharded run holds, locally indexed (owned nodes first, then halo)
struct RankMesh {
  int rank = 0, nranks = 1, npe = 0;
  int n_global = 0, n_own = 0;          // nodes of the whole mesh; nodes this rank owns (local ids [0, n_own))
  int lib0 = 0, lib1 = 0;               // the library ids it owns
  std::vector<int> node_global, node_lib;   // per local node: the caller's id, the library id
  std::vector<int> elem_global;         // per local element: the caller's element index
  std::vector<int> elements;            // [local elements][npe] local node ids
  std::vector<double> nodes0;           // [local nodes][3]
  std::vector<int> presc_node, presc_type;
  std::vector<double> presc_values;
  ShardPlan plan;                       // halo plan in local ids
};
void rank_row_range(int N, int npe, int rank, int nranks, int &g0, int &g1);
int build_rank_mesh(int rank, int nranks, int N, int E, int npe, const int *elements, const double *nodes0,
                    int n_presc, const int *presc_node, const int *presc_type, const double *presc_values,
                    RankMesh &out, std::string &err);
// the part behind "local nodes known", shared by both constructors: the halo plan from the rank's OWN elements
// (out.elements, out.n_own filled) and the owner of every halo node.  key (may be null) = the order the rows to and from
// a peer travel in: ascending key[local id]; null = ascending local id.
void finish_rank_mesh(int rank, int nranks, int npe, const int *halo_owner, const int *key, RankMesh &out);
// a rank's sub-mesh from the caller's own slab (feahip_create_rank_local): validated, copied, the plan in ascending
// GLOBAL node id per peer.  nodes0 may be null (plan only); n_global < 0 skips the range check of node_global.
int build_rank_mesh_local(int rank, int nranks, int n_global, int n_local, int n_own, int E, int npe, const int *elements,
                          const double *nodes0, const int *node_global, const int *elem_global, const int *halo_owner,
                          int n_presc, const int *presc_node, const int *presc_type, const double *presc_values,
                          RankMesh &out, std::string &err);
// the library's numbering of the LOCAL mesh, split stably into owned first, halo after; true when it reorders
int slab_order(int n_local, int n_own, int E, int npe, const int *elements, const double *nodes0, int *new_local_id);
int install_plan(feahip_ctx *c, const ShardPlan &plan);      // dist.hip: halo lists to the device, interior chunk range
int ensure_vred(feahip_ctx *c, size_t n);                    // coarse.hip: d_vred holds at least n doubles

// multi-rank operations (kernels_solve.hip; the step loops in drivers.hip).  R = the ranks driven by this
// process: one context with the RCCL transport, or all contexts of an
// in-process group.
#define FOR_RANKS(c) for (feahip_ctx *c : R) if (hipSetDevice(c->device) == hipSuccess)
struct Transport {
  virtual ~Transport() {}
  // halo rows of vector `which` (0 = p, 1 = u, 2 = x, 3 = z) from their owners
  virtual int exchange(std::vector<feahip_ctx *> &R, int which) = 0;
  // the same in two halves: begin() leaves the exchange running (on a stream of its own where the transport has
  // one), end() makes the context's stream wait for the halo rows.  Work enqueued between the two must not read them.
  virtual int exchange_begin(std::vector<feahip_ctx *> &R, int which) { return exchange(R, which); }
  virtual int exchange_end(std::vector<feahip_ctx *> &R) { (void)R; return FEAHIP_OK; }
  // the halo rows of a block vector [3N][8] per context of R (d_v8[k] belongs to R[k]) from their owners, through
  // ModalState::d_bsend / d_brecv (ensure_modal_dist): the two halves of exchange_begin / exchange_end, same events
  virtual int exchange_block_begin(std::vector<feahip_ctx *> &R, const std::vector<double *> &d_v8) = 0;
  virtual int exchange_block_end(std::vector<feahip_ctx *> &R) = 0;
  // d_scal[8+slot .. 8+slot+n) summed over all ranks, result on every rank
  virtual int allreduce(std::vector<feahip_ctx *> &R, int slot, int n) = 0;
  // the same with the maximum over all ranks (order-independent: reproducible on any transport)
  virtual int allreduce_max(std::vector<feahip_ctx *> &R, int slot, int n) = 0;
  // the contexts' d_vred[0 .. n) summed over all ranks, result on every rank.  comm: the buffer is produced and
  // consumed on the contexts' communication streams (which exist), not on their own
  virtual int allreduce_vec(std::vector<feahip_ctx *> &R, size_t n, bool comm) = 0;
  // the contexts of an in-process group in rank order; null where every process drives one context
  virtual const std::vector<feahip_ctx *> *members() const { return nullptr; }
  virtual void set_members(const std::vector<feahip_ctx *> &) {}
};
Transport *make_group_transport();
Transport *make_rccl_transport(feahip_ctx *c, int rank, int nranks, const void *unique_id, std::string &err);
int rccl_unique_id(void *out, int cap);
int install_shard(feahip_ctx *c, int rank, int nranks);
int dist_solve_pcg(std::vector<feahip_ctx *> &R, int type, double tol, int max_iter, int *iters, double *resid);
int dist_energy(std::vector<feahip_ctx *> &R, double *out);
// d_scal[8 .. 8+n) reduced over the ranks (over the transport, where there is one) and read from R[0] into out
enum class RankReduce { sum, max };
int dist_read_scalars(std::vector<feahip_ctx *> &R, RankReduce how, int n, double *out);
int dist_update_nodes_with_solution(std::vector<feahip_ctx *> &R, const double *u_host);
int dist_newton(std::vector<feahip_ctx *> &R, int load_increments, int max_newton, int modified_newton,
                double desired_tolerance, int solver_type, double solver_tolerance, int solver_max_iter,
                double *tol_log, int tol_log_cap, int *its_log, int *steps_done);

// avg_ms = the mean time of one(k) for k in [warmup, warmup + iters) on the context's stream, after one(0 .. warmup);
// one(k) enqueues and returns a status.  The events are destroyed on every path.
template <class F>
int time_enqueued(feahip_ctx *c, int warmup, int iters, double *avg_ms, F one)
{
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto run = [&]() -> int {
    int rc;
    FEA_HIP_CHECK(c, hipEventCreate(&e0));
    FEA_HIP_CHECK(c, hipEventCreate(&e1));
    for (int k = 0; k < warmup; ++k) if ((rc = one(k))) return rc;
    FEA_HIP_CHECK(c, hipEventRecord(e0, c->stream));
    for (int k = 0; k < iters; ++k) if ((rc = one(warmup + k))) return rc;
    FEA_HIP_CHECK(c, hipEventRecord(e1, c->stream));
    FEA_HIP_CHECK(c, hipEventSynchronize(e1));
    float ms = 0;
    FEA_HIP_CHECK(c, hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = iters > 0 ? (double)ms / iters : 0.0;
    return FEAHIP_OK;
  };
  const int rc = run();
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}
