// Stand-alone check of csrc/node_views.h (built with -fsanitize=address,undefined by tests/test_node_views_host.py): the two
// reorderings between the caller's node ids and the library's, judged by the index formula perm[caller id] = library
// id, on buffers sized exactly so that any overrun is a sanitizer report.
#include "node_views.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

static int g_checks = 0, g_failures = 0;

static void expect(bool ok, const char *what, int N, int width, int stride, int pk, int r0, int r1)
{
  ++g_checks;
  if (ok) return;
  ++g_failures;
  std::printf("FAILED %s: N %d width %d stride %d perm %d rows [%d, %d)\n", what, N, width, stride, pk, r0, r1);
}

template <class T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// a value no reordering writes: NaN for double, a large negative for int
template <class T> static T poison();
template <> double poison<double>() { return std::numeric_limits<double>::quiet_NaN(); }
template <> int poison<int>() { return -123456789; }

template <class T> static T sample(int a, int j) { return (T)((a + 1) * 100 + j * 7) * (T)((a + j) % 2 ? -1 : 1); }

// perm kinds: 0 identity (null), 1 reversal, 2 a fixed scramble
static std::vector<int> make_perm(int kind, int N)
{
  std::vector<int> p((size_t)N);
  for (int a = 0; a < N; ++a) p[a] = kind == 1 ? N - 1 - a : (a * 3 + 2) % N;     // 3 and 7 coprime: a bijection; N = 1: 0
  return p;
}

template <class T>
static void run(int N, int width, int stride, int pk)
{
  const std::vector<int> perm = make_perm(pk, N);
  const int *pp = pk == 0 ? nullptr : perm.data();
  auto lib_of = [&](int a) { return pk == 0 ? a : perm[a]; };

  std::vector<T> x((size_t)N * width);
  for (int a = 0; a < N; ++a)
    for (int j = 0; j < width; ++j) x[(size_t)a * width + j] = sample<T>(a, j);
  if constexpr (std::is_same<T, double>::value) x[0] = -0.0;          // bit for bit: -0 stays -0

  // to_library: every lane where the formula puts it, every pad lane exactly zero over a destination full of poison
  std::vector<T> lib((size_t)N * stride, poison<T>());
  to_library(NodeView(pp, N), width, stride, x.data(), lib.data());
  bool placed = true, padded = true;
  for (int a = 0; a < N; ++a) {
    for (int j = 0; j < width; ++j) placed = placed && same_bits(lib[(size_t)lib_of(a) * stride + j], x[(size_t)a * width + j]);
    for (int j = width; j < stride; ++j) padded = padded && same_bits(lib[(size_t)lib_of(a) * stride + j], T(0));
  }
  expect(placed, "to_library places lib[perm[a] * stride + j] = host[a * width + j]", N, width, stride, pk, 0, N);
  expect(padded, "to_library writes the pad lanes as zero", N, width, stride, pk, 0, N);

  // to_caller over all rows gives the input back, bit for bit
  std::vector<T> back((size_t)N * width, poison<T>());
  to_caller(NodeView(pp, N), width, stride, lib.data(), back.data());
  expect(std::memcmp(back.data(), x.data(), sizeof(T) * x.size()) == 0, "to_caller(to_library(x)) == x", N, width, stride, pk, 0, N);

  // owned ranges: empty, all, a strict interior one, one touching each end (what N allows)
  const int ranges[][2] = {{N / 2, N / 2}, {0, N}, {2, N - 2}, {0, N / 2 + 1}, {N / 2, N}};
  for (const auto &r : ranges) {
    if (r[0] > r[1] || r[0] < 0 || r[1] > N) continue;
    // rows outside the range hold poison on the library's side: they must not reach the caller
    std::vector<T> owned_lib = lib;
    for (int la = 0; la < N; ++la)
      if (la < r[0] || la >= r[1]) for (int j = 0; j < stride; ++j) owned_lib[(size_t)la * stride + j] = poison<T>();
    std::vector<T> out((size_t)N * width, poison<T>());
    to_caller(NodeView(pp, N, r[0], r[1]), width, stride, owned_lib.data(), out.data());
    bool inside = true, outside = true;
    for (int a = 0; a < N; ++a) {
      const bool own = lib_of(a) >= r[0] && lib_of(a) < r[1];
      for (int j = 0; j < width; ++j) {
        const T got = out[(size_t)a * width + j];
        if (own) inside = inside && same_bits(got, x[(size_t)a * width + j]);
        else outside = outside && same_bits(got, T(0));                 // all bits clear: +0.0, the sign bit included
      }
    }
    expect(inside, "to_caller keeps the nodes of the owned range", N, width, stride, pk, r[0], r[1]);
    expect(outside, "to_caller gives +0 outside the owned range", N, width, stride, pk, r[0], r[1]);
  }
}

int main()
{
  const int shapes[][2] = {{1, 1}, {3, 3}, {3, 4}, {6, 6}};
  for (int N : {1, 7})
    for (int pk = 0; pk < 3; ++pk)
      for (const auto &s : shapes) {
        run<double>(N, s[0], s[1], pk);
        run<int>(N, s[0], s[1], pk);
      }
  std::printf("node views: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
