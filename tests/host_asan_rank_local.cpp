// host-only sanitizer run over the builders of a rank made from its own slab (rankmesh.cpp: build_rank_mesh_local,
// finish_rank_mesh, slab_order): slabs cut by the whole-mesh builder, handed back as a caller would hand them
#include "feahip_internal.h"
#include <cstdio>
#include <numeric>
static const int P[6][3] = {{0,1,2},{0,2,1},{1,0,2},{1,2,0},{2,0,1},{2,1,0}};
int main()
{
  for (int quad = 0; quad < 2; ++quad) {
    const int nx = quad ? 3 : 7, ny = quad ? 14 : 40, nz = quad ? 4 : 6, m = quad ? 2 : 1;
    const int gx = m * nx + 1, gy = m * ny + 1, gz = m * nz + 1;
    auto id = [&](int i, int j, int k) { return (j * gz + k) * gx + i; };
    std::vector<int> conn; std::vector<double> pos((size_t)gx * gy * gz * 3);
    for (int j = 0; j < gy; ++j) for (int k = 0; k < gz; ++k) for (int i = 0; i < gx; ++i) {
      double *p = &pos[(size_t)id(i, j, k) * 3]; p[0] = i; p[1] = j; p[2] = k; }
    static const int ED[6][2] = {{0,1},{1,2},{0,2},{0,3},{1,3},{2,3}};
    for (int j = 0; j < ny; ++j) for (int k = 0; k < nz; ++k) for (int i = 0; i < nx; ++i)
      for (int p = 0; p < 6; ++p) {
        int c[3] = {i * m, j * m, k * m}; int v[4][3];
        for (int d = 0; d < 3; ++d) v[0][d] = c[d];
        for (int s = 0; s < 3; ++s) { c[P[p][s]] += m; for (int d = 0; d < 3; ++d) v[s + 1][d] = c[d]; }
        for (int s = 0; s < 4; ++s) conn.push_back(id(v[s][0], v[s][1], v[s][2]));
        if (quad) for (auto &e : ED) conn.push_back(id((v[e[0]][0] + v[e[1]][0]) / 2, (v[e[0]][1] + v[e[1]][1]) / 2, (v[e[0]][2] + v[e[1]][2]) / 2));
      }
    const int npe = quad ? 10 : 4, N = gx * gy * gz, E = (int)conn.size() / npe, nranks = 3;
    std::string err;
    std::vector<RankMesh> whole((size_t)nranks), loc((size_t)nranks);
    std::vector<int> owner((size_t)N, -1);
    for (int r = 0; r < nranks; ++r) {
      if (build_rank_mesh(r, nranks, N, E, npe, conn.data(), pos.data(), 0, nullptr, nullptr, nullptr, whole[r], err)) { printf("%s\n", err.c_str()); return 1; }
      for (int a = 0; a < whole[r].n_own; ++a) owner[(size_t)whole[r].node_global[a]] = r;
    }
    std::vector<std::vector<int>> howner((size_t)nranks);
    for (int r = 0; r < nranks; ++r) {
      const RankMesh &w = whole[r];
      const int nl = (int)w.node_global.size();
      for (int a = w.n_own; a < nl; ++a) howner[r].push_back(owner[(size_t)w.node_global[a]]);
      const int rc = build_rank_mesh_local(r, nranks, N, nl, w.n_own, (int)w.elem_global.size(), npe, w.elements.data(), w.nodes0.data(),
                                           w.node_global.data(), w.elem_global.data(), howner[r].data(), 0, nullptr, nullptr, nullptr, loc[r], err);
      if (rc) { printf("local rank %d: %s\n", r, err.c_str()); return 2; }
    }
    bool fit = true;                       // r's rows to s are s's rows from r, in the same (global) order
    for (int r = 0; r < nranks; ++r)
      for (size_t k = 0; k < loc[r].plan.peer.size(); ++k) {
        const int s = loc[r].plan.peer[k];
        const ShardPlan &a = loc[r].plan, &b = loc[s].plan;
        size_t kb = 0;
        while (kb < b.peer.size() && b.peer[kb] != r) ++kb;
        if (kb == b.peer.size()) { fit = false; continue; }
        const int n = a.send_off[k + 1] - a.send_off[k];
        if (n != b.recv_off[kb + 1] - b.recv_off[kb]) { fit = false; continue; }
        for (int i = 0; i < n; ++i)
          fit = fit && loc[r].node_global[a.send_idx[a.send_off[k] + i]] == loc[s].node_global[b.recv_idx[b.recv_off[kb] + i]];
        fit = fit && a.peer == whole[r].plan.peer && a.send_idx.size() == whole[r].plan.send_idx.size();
      }
    printf("%s: plans fit: %d\n", quad ? "tet10" : "tet4", (int)fit);
    {                                      // every malformed slab is refused, nothing read out of bounds
      const RankMesh &w = whole[1];
      const int nl = (int)w.node_global.size(), ne = (int)w.elem_global.size();
      int refused = 0;
      RankMesh t;
      auto run = [&](int n_own, const std::vector<int> &el, const std::vector<int> &ng, const std::vector<int> &ho, int npresc, const int *pn) {
        const int pt[1] = {7}; const double pv[3] = {0, 0, 0};
        const int rc = build_rank_mesh_local(1, nranks, N, nl, n_own, ne, npe, el.data(), w.nodes0.data(), ng.data(), nullptr, ho.data(), npresc, pn, pt, pv, t, err);
        refused += rc == FEAHIP_EINVAL;
      };
      run(0, w.elements, w.node_global, howner[1], 0, nullptr);
      { auto el = w.elements; el[3] = nl; run(w.n_own, el, w.node_global, howner[1], 0, nullptr); }
      { auto el = w.elements; for (int k = 0; k < npe; ++k) el[(size_t)npe * 2 + k] = w.n_own + k; run(w.n_own, el, w.node_global, howner[1], 0, nullptr); }
      { auto ho = howner[1]; ho[0] = nranks; run(w.n_own, w.elements, w.node_global, ho, 0, nullptr); }
      { auto ho = howner[1]; ho[1] = 1; run(w.n_own, w.elements, w.node_global, ho, 0, nullptr); }
      { auto ng = w.node_global; ng[5] = ng[0]; run(w.n_own, w.elements, ng, howner[1], 0, nullptr); }
      { const int pn[1] = {nl}; run(w.n_own, w.elements, w.node_global, howner[1], 1, pn); }
      printf("  refused: %d/7\n", refused);
    }
    {
      const RankMesh &w = whole[2];
      const int nl = (int)w.node_global.size();
      std::vector<int> nw((size_t)nl, -1), seen((size_t)nl, 0);
      const int rc = slab_order(nl, w.n_own, (int)w.elem_global.size(), npe, w.elements.data(), w.nodes0.data(), nw.data());
      bool bij = rc >= 0;
      for (int a = 0; a < nl && bij; ++a) { bij = nw[a] >= 0 && nw[a] < nl && !seen[(size_t)nw[a]] && (a < w.n_own) == (nw[a] < w.n_own); if (bij) seen[(size_t)nw[a]] = 1; }
      printf("  order: bijection %d (reorders %d)\n", (int)bij, rc);
    }
  }
  return 0;
}
