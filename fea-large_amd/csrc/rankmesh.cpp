// rankmesh.cpp -- what ONE rank of a sharded run holds (host, once per context).
//
// The reference keeps one row-wise store of the whole matrix (fea_solver.c:444-448) in one process.  A rank of a
// sharded run here owns a slab of nodes -- a range of LIBRARY node ids (renumber.cpp: compact cells in slabs across
// the longest axis) -- and holds nothing but its slab: the elements that touch its nodes, those elements' nodes (its
// own first, then the halo nodes in library order), the block rows of its own nodes (pattern built from its own
// elements only: every element around an owned node is local, so an owned row is complete), K and the vectors over
// its local nodes.  Everything is indexed locally; the halo plan (who sends which rows to whom) is derived on every
// rank from its own elements: rank r needs my node a exactly when a shares an element with a node r owns, which both
// sides see.  No global pattern, no global K index space: the 50M-element TET10 block of BASELINE.json configs[4]
// (1.9e9 3x3 blocks, 140 GB of values) is eight independent index spaces of 2.4e8 blocks.
#include "feahip_internal.h"
#include <algorithm>
#include <cstring>
#include <string>

// library ids [g0, g1) of rank `rank`: equal node counts, rounded to a multiple of the numbering's FULL cell (renumber.cpp:
// 4 x 4 x 4 nodes, 48 half-grid nodes for 10-node elements).  The nodes of a cell are consecutive ids, so while the cells
// before the cut are full ones the cut falls between two cells and no gather chunk is split between two ranks; behind
// the first PARTIAL cell (the last cell of every line of a block whose node count is not a multiple of four) the
// multiples no longer coincide with cell boundaries and a cut may fall inside a cell -- that costs the two ranks one
// irregular chunk each, nothing else.  Cutting at whole layers of cells instead would make the slab faces planar but
// the ranks unequal (the 10M block has 100 layers: 12 or 13 per rank of eight, 4 % of the strong-scaling efficiency).
static int rank_cut(int N, int npe, int k, int nranks)
{
  constexpr int gc[3] = {FEA_G_CELL};
  const int cell = npe == 10 ? 48 : gc[0] * gc[1] * gc[2];
  if (k <= 0) return 0;
  if (k >= nranks) return N;
  const long long t = (long long)N * k / nranks;
  const long long c = (t + cell / 2) / cell * cell;
  return (int)std::min<long long>(std::max<long long>(c, 0), N);
}
void rank_row_range(int N, int npe, int rank, int nranks, int &g0, int &g1)
{
  g0 = rank_cut(N, npe, rank, nranks); g1 = rank_cut(N, npe, rank + 1, nranks);
}

int build_rank_mesh(int rank, int nranks, int N, int E, int npe, const int *elements, const double *nodes0,
                    int n_presc, const int *presc_node, const int *presc_type, const double *presc_values,
                    RankMesh &out, std::string &err)
{
  if (nranks < 1 || rank < 0 || rank >= nranks) { err = "bad (rank, nranks)"; return FEAHIP_EINVAL; }
  for (long long i = 0; i < (long long)E * npe; ++i)
    if (elements[i] < 0 || elements[i] >= N) { err = "element refers to a node outside the mesh"; return FEAHIP_EINVAL; }
  std::vector<int> lib;                                        // library id of every caller node
  locality_numbering(N, E, npe, elements, nodes0, lib);        // (the identity where the mesh gives no basis for one)
  out.n_global = N; out.rank = rank; out.nranks = nranks; out.npe = npe;
  rank_row_range(N, npe, rank, nranks, out.lib0, out.lib1);
  const int g0 = out.lib0, g1 = out.lib1;
  std::vector<int> cuts((size_t)nranks + 1);
  for (int k = 0; k <= nranks; ++k) cuts[k] = rank_cut(N, npe, k, nranks);
  auto owner_of = [&](int libid) { return (int)(std::upper_bound(cuts.begin(), cuts.end(), libid) - cuts.begin()) - 1; };
  // local elements: every element with an owned node, in the caller's order
  out.elem_global.clear();
  std::vector<char> is_local((size_t)N, 0);
  for (int e = 0; e < E; ++e) {
    bool mine = false;
    for (int k = 0; k < npe; ++k) { const int l = lib[elements[(size_t)e * npe + k]]; if (l >= g0 && l < g1) { mine = true; break; } }
    if (!mine) continue;
    out.elem_global.push_back(e);
    for (int k = 0; k < npe; ++k) is_local[elements[(size_t)e * npe + k]] = 1;
  }
  // local nodes: owned in library order, then halo in library order
  std::vector<std::pair<int, int>> own, halo;                  // (library id, caller id)
  for (int a = 0; a < N; ++a) {
    const int l = lib[a];
    if (l >= g0 && l < g1) own.emplace_back(l, a);             // (an owned node no element touches keeps its diagonal row)
    else if (is_local[a]) halo.emplace_back(l, a);
  }
  std::sort(own.begin(), own.end()); std::sort(halo.begin(), halo.end());
  out.n_own = (int)own.size();
  const int nl = (int)(own.size() + halo.size());
  out.node_global.resize((size_t)nl); out.node_lib.resize((size_t)nl);
  std::vector<int> local_of((size_t)N, -1);
  for (int i = 0; i < nl; ++i) {
    const auto &p = i < out.n_own ? own[i] : halo[i - out.n_own];
    out.node_lib[i] = p.first; out.node_global[i] = p.second; local_of[p.second] = i;
  }
  out.elements.resize(out.elem_global.size() * (size_t)npe);
  for (size_t i = 0; i < out.elem_global.size(); ++i)
    for (int k = 0; k < npe; ++k) out.elements[i * npe + k] = local_of[elements[(size_t)out.elem_global[i] * npe + k]];
  out.nodes0.resize((size_t)nl * 3);
  for (int i = 0; i < nl; ++i)
    for (int j = 0; j < 3; ++j) out.nodes0[(size_t)i * 3 + j] = nodes0[(size_t)out.node_global[i] * 3 + j];
  out.presc_node.clear(); out.presc_type.clear(); out.presc_values.clear();
  for (int i = 0; i < n_presc; ++i) {
    if (presc_node[i] < 0 || presc_node[i] >= N) { err = "prescribed node id out of range"; return FEAHIP_EINVAL; }
    const int l = local_of[presc_node[i]];
    if (l < 0) continue;                                        // another rank's business
    out.presc_node.push_back(l); out.presc_type.push_back(presc_type[i]);
    for (int j = 0; j < 3; ++j) out.presc_values.push_back(presc_values[(size_t)i * 3 + j]);
  }
  std::vector<int> halo_owner((size_t)(nl - out.n_own));
  for (int i = out.n_own; i < nl; ++i) halo_owner[(size_t)(i - out.n_own)] = owner_of(out.node_lib[i]);
  finish_rank_mesh(rank, nranks, npe, halo_owner.data(), nullptr, out);   // rows travel in ascending library id (= local id)
  return FEAHIP_OK;
}

// halo plan in local ids.  recv: my halo nodes by owner; send: my owned nodes that share an element with a node of
// that peer (the peer's halo nodes I own: the same set, seen from its elements).  Inside a peer's segment the rows
// ascend in key (the id both ends share); null: in local id, which feahip_create_rank's local order makes the library id.
void finish_rank_mesh(int rank, int nranks, int npe, const int *halo_owner, const int *key, RankMesh &out)
{
  out.rank = rank; out.nranks = nranks; out.npe = npe;
  const int nl = (int)out.node_global.size();
  std::vector<std::vector<int>> send((size_t)nranks), recv((size_t)nranks);
  for (int i = out.n_own; i < nl; ++i) recv[(size_t)halo_owner[i - out.n_own]].push_back(i);
  {
    const size_t ne = out.elements.size() / (size_t)npe;
    for (size_t e = 0; e < ne; ++e) {
      const int *c = out.elements.data() + e * npe;
      int owners[16]; int no = 0;
      for (int k = 0; k < npe; ++k)
        if (c[k] >= out.n_own) {
          const int r = halo_owner[c[k] - out.n_own];
          bool seen = false;
          for (int q = 0; q < no; ++q) seen = seen || owners[q] == r;
          if (!seen && no < 16) owners[no++] = r;
        }
      if (!no) continue;
      for (int k = 0; k < npe; ++k)
        if (c[k] < out.n_own)
          for (int q = 0; q < no; ++q) send[(size_t)owners[q]].push_back(c[k]);
    }
    for (int r = 0; r < nranks; ++r) {
      std::sort(send[r].begin(), send[r].end());
      send[r].erase(std::unique(send[r].begin(), send[r].end()), send[r].end());
      if (key) {
        auto by_key = [key](int a, int b) { return key[a] < key[b]; };
        std::sort(send[r].begin(), send[r].end(), by_key);
        std::sort(recv[r].begin(), recv[r].end(), by_key);
      }
    }
  }
  ShardPlan &pl = out.plan;
  pl = ShardPlan();
  pl.rank = rank; pl.nranks = nranks; pl.row0 = 0; pl.row1 = out.n_own;
  pl.send_off.push_back(0); pl.recv_off.push_back(0);
  for (int r = 0; r < nranks; ++r) {
    if (r == rank || (send[r].empty() && recv[r].empty())) continue;
    pl.peer.push_back(r);
    pl.send_idx.insert(pl.send_idx.end(), send[r].begin(), send[r].end());
    pl.recv_idx.insert(pl.recv_idx.end(), recv[r].begin(), recv[r].end());
    pl.send_off.push_back((int)pl.send_idx.size()); pl.recv_off.push_back((int)pl.recv_idx.size());
  }
}

// One rank's sub-mesh as the caller cut it: local nodes [0, n_own) owned, the rest halo with their owners named.  Nothing
// here is sized by the whole mesh: node_global is checked for repeats on a sorted copy, not through a table of n_global.
int build_rank_mesh_local(int rank, int nranks, int n_global, int n_local, int n_own, int E, int npe, const int *elements,
                          const double *nodes0, const int *node_global, const int *elem_global, const int *halo_owner,
                          int n_presc, const int *presc_node, const int *presc_type, const double *presc_values,
                          RankMesh &out, std::string &err)
{
  auto S = [](long long v) { return std::to_string(v); };
  if (nranks < 1 || rank < 0 || rank >= nranks) { err = "bad (rank, nranks)"; return FEAHIP_EINVAL; }
  if (npe != 4 && npe != 8 && npe != 10) { err = "nodes per element must be 4, 8 or 10"; return FEAHIP_EINVAL; }
  if (n_local <= 0 || E <= 0 || !elements || !node_global) { err = "null or empty slab"; return FEAHIP_EINVAL; }
  if (n_own < 1 || n_own > n_local) { err = "n_own = " + S(n_own) + " outside [1, n_local = " + S(n_local) + "]"; return FEAHIP_EINVAL; }
  if (n_own < n_local && !halo_owner) { err = "halo nodes without halo_owner"; return FEAHIP_EINVAL; }
  std::vector<char> touched((size_t)n_local, 0);
  for (int e = 0; e < E; ++e) {
    bool mine = false;
    for (int k = 0; k < npe; ++k) {
      const int a = elements[(size_t)e * npe + k];
      if (a < 0 || a >= n_local) {
        err = "element " + S(e) + " refers to local node " + S(a) + " outside [0," + S(n_local) + ")"; return FEAHIP_EINVAL;
      }
      touched[(size_t)a] = 1; mine = mine || a < n_own;
    }
    if (!mine) { err = "element " + S(e) + " has no owned node: it contributes to no row of this rank"; return FEAHIP_EINVAL; }
  }
  for (int i = n_own; i < n_local; ++i) {
    if (!touched[(size_t)i]) { err = "halo node " + S(i) + " is touched by no element"; return FEAHIP_EINVAL; }
    const int o = halo_owner[i - n_own];
    if (o < 0 || o >= nranks || o == rank) {
      err = "halo_owner[" + S(i - n_own) + "] = " + S(o) + (o == rank ? ": a halo node (local " + S(i) + ") cannot be owned by this rank"
                                                                      : " outside [0," + S(nranks) + ")");
      return FEAHIP_EINVAL;
    }
  }
  {
    std::vector<std::pair<int, int>> byid((size_t)n_local);
    for (int i = 0; i < n_local; ++i) {
      if (node_global[i] < 0 || (n_global >= 0 && node_global[i] >= n_global)) {
        err = "node_global[" + S(i) + "] = " + S(node_global[i]) + " outside [0," + S(n_global) + ")"; return FEAHIP_EINVAL;
      }
      byid[(size_t)i] = {node_global[i], i};
    }
    std::sort(byid.begin(), byid.end());
    for (int i = 1; i < n_local; ++i)
      if (byid[(size_t)i].first == byid[(size_t)i - 1].first) {
        err = "node_global[" + S(byid[(size_t)i].second) + "] repeats node_global[" + S(byid[(size_t)i - 1].second) + "] = " + S(byid[(size_t)i].first);
        return FEAHIP_EINVAL;
      }
  }
  out.n_global = n_global; out.n_own = n_own; out.lib0 = 0; out.lib1 = n_own;
  out.node_global.assign(node_global, node_global + n_local);
  out.node_lib.clear();                                         // no library numbering of the whole mesh exists here
  out.elem_global.resize((size_t)E);
  for (int e = 0; e < E; ++e) out.elem_global[(size_t)e] = elem_global ? elem_global[e] : e;
  out.elements.assign(elements, elements + (size_t)E * npe);
  if (nodes0) out.nodes0.assign(nodes0, nodes0 + (size_t)n_local * 3); else out.nodes0.clear();
  out.presc_node.clear(); out.presc_type.clear(); out.presc_values.clear();
  for (int i = 0; i < n_presc; ++i) {
    if (presc_node[i] < 0 || presc_node[i] >= n_local) {
      err = "prescribed entry " + S(i) + ": local node " + S(presc_node[i]) + " outside [0," + S(n_local) + ")"; return FEAHIP_EINVAL;
    }
    out.presc_node.push_back(presc_node[i]); out.presc_type.push_back(presc_type[i]);
    for (int j = 0; j < 3; ++j) out.presc_values.push_back(presc_values[(size_t)i * 3 + j]);
  }
  // the two ends of an exchange are built in different processes and share only the global ids
  finish_rank_mesh(rank, nranks, npe, halo_owner, out.node_global.data(), out);
  return FEAHIP_OK;
}

// A local order that suits the kernels: renumber.cpp's numbering of the local mesh (compact cells; bisection leaves off
// a lattice), then the owned nodes first and the halo nodes after, each in that numbering's order.
int slab_order(int n_local, int n_own, int E, int npe, const int *elements, const double *nodes0, int *new_local_id)
{
  std::vector<int> lib;
  locality_numbering(n_local, E, npe, elements, nodes0, lib);
  std::vector<std::pair<int, int>> own, halo;                  // (library id of the local mesh, incoming local id)
  for (int a = 0; a < n_local; ++a) (a < n_own ? own : halo).emplace_back(lib[(size_t)a], a);
  std::sort(own.begin(), own.end()); std::sort(halo.begin(), halo.end());
  bool moved = false;
  for (int i = 0; i < n_local; ++i) {
    const int a = i < n_own ? own[(size_t)i].second : halo[(size_t)(i - n_own)].second;
    new_local_id[a] = i; moved = moved || a != i;
  }
  return moved ? 1 : 0;
}
