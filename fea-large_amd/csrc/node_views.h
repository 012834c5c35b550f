// node_views.h -- the one translation between the caller's node numbering and the library's, for host buffers.
// The ABI speaks the caller's ids, everything behind it the library's (renumber.cpp): perm[caller id] = library id.
// Host only (no HIP): a node field is [N][width] on the caller's side and [N][lib_stride] on the library's, where
// lib_stride >= width is the stride of the device record (the node records are [N][4] and carry 3).
#pragma once
#include <cstddef>

struct NodeView {
  const int *perm;                     // null: the library kept the caller's ids
  int N;
  int row0, row1;                      // the library ids this rank owns: the rows to_caller reads
  NodeView(const int *perm_, int N_) : perm(perm_), N(N_), row0(0), row1(N_) {}
  NodeView(const int *perm_, int N_, int row0_, int row1_) : perm(perm_), N(N_), row0(row0_), row1(row1_) {}
  int lib(int a) const { return perm ? perm[a] : a; }
  bool owns(int la) const { return la >= row0 && la < row1; }
  bool all_rows() const { return row0 <= 0 && row1 >= N; }
};

// the caller's host[N][width] into lib[N][lib_stride] in library ids; the pad lanes width..lib_stride-1 are written as zero
template <class T>
void to_library(const NodeView &v, int width, int lib_stride, const T *host, T *lib)
{
  for (int a = 0; a < v.N; ++a) {
    const T *src = host + (size_t)a * width;
    T *dst = lib + (size_t)v.lib(a) * lib_stride;
    for (int j = 0; j < width; ++j) dst[j] = src[j];
    for (int j = width; j < lib_stride; ++j) dst[j] = T(0);
  }
}

// lib[N][lib_stride] in library ids into the caller's host[N][width]; a node outside [row0, row1) reads as +0 (its
// row of lib is not looked at: it need not hold anything)
template <class T>
void to_caller(const NodeView &v, int width, int lib_stride, const T *lib, T *host)
{
  for (int a = 0; a < v.N; ++a) {
    const int la = v.lib(a);
    const T *src = lib + (size_t)la * lib_stride;
    T *dst = host + (size_t)a * width;
    if (v.owns(la)) for (int j = 0; j < width; ++j) dst[j] = src[j];
    else for (int j = 0; j < width; ++j) dst[j] = T(0);
  }
}
