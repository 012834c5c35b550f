// The host instantiation of csrc/rainflow_point.h over rings of exactly `depth` doubles on the heap, so that a slot outside
// the ring is a sanitizer report: depths 4 and 5, series whose counts wrap the ring round, drop the start point and
// overflow, each against a plain count on a std::vector that erases from the front.  Built with -fsanitize=address,undefined
// by tests/test_rainflow_host.py and run as a program.
#include "rainflow_point.h"
#include <cstdio>
#include <cfloat>
#include <cmath>
#include <memory>
#include <vector>

struct Cycle { double range, mean, count; };

struct HeapRing {
  std::unique_ptr<double[]> p;
  int depth;
  explicit HeapRing(int d) : p(new double[d]), depth(d) {}
  double get(int slot) const { return p[slot]; }
  void set(int slot, double v) { p[slot] = v; }
};
struct Sink {
  std::vector<Cycle> list;
  void operator()(double r, double m, double c) { list.push_back({r, m, c}); }
};

// the textbook count on a vector, with the ring's overflow rule; returns overflow, the most points held in *used
static bool plain(const std::vector<double> &x, int depth, std::vector<Cycle> &out, int *used, int *starts)
{
  std::vector<double> rev;
  std::vector<double> kept;
  for (double v : x) if (kept.empty() || v != kept.back()) kept.push_back(v);
  for (size_t i = 0; i < kept.size(); ++i)
    if (i == 0 || i + 1 == kept.size() || (kept[i] - kept[i - 1] > 0) != (kept[i + 1] - kept[i] > 0)) rev.push_back(kept[i]);
  std::vector<double> s;
  bool over = false;
  *used = 0; *starts = 0;
  auto half = [&](double a, double b) { out.push_back({std::fabs(a - b), 0.5 * (a + b), 0.5}); };
  if (rev.size() < 2) return false;
  for (double v : rev) {
    if ((int)s.size() == depth) { half(s[0], s[1]); s.erase(s.begin()); over = true; }
    s.push_back(v);
    if ((int)s.size() > *used) *used = (int)s.size();
    while (s.size() >= 3) {
      const size_t n = s.size();
      const double X = std::fabs(s[n - 2] - s[n - 1]), Y = std::fabs(s[n - 3] - s[n - 2]);
      if (X < Y) break;
      if (n == 3) { half(s[0], s[1]); s.erase(s.begin()); ++*starts; }
      else { out.push_back({Y, 0.5 * (s[n - 3] + s[n - 2]), 1.0}); s.erase(s.end() - 3, s.end() - 1); }
    }
  }
  for (size_t i = 0; i + 1 < s.size(); ++i) half(s[i], s[i + 1]);
  return over;
}

static int checks = 0, failures = 0;
static void check(bool ok, const char *what, int depth, int series)
{
  ++checks;
  if (!ok) { ++failures; std::printf("FAILED: %s (depth %d, series %d)\n", what, depth, series); }
}

int main()
{
  std::vector<std::vector<double>> all;
  all.push_back({-2, 1, -3, 5, -1, 3, -4, 4, -2});                      // the standard's example
  {                                                                    // a ring-down: nothing closes, every push past the depth overflows
    std::vector<double> x;
    for (int k = 0; k < 40; ++k) x.push_back((k % 2 ? -1.0 : 1.0) * std::pow(0.9, k));
    all.push_back(x);
  }
  {                                                                    // growing, then nested, then ring-down: start-point drops, closures
    std::vector<double> x;                                             // and overflow in one series, with flat runs and ties
    for (int k = 1; k <= 9; ++k) x.push_back((k % 2 ? 1.0 : -1.0) * k);
    for (int rep = 0; rep < 6; ++rep)
      for (double v : {10.0, -8.0, 6.0, -4.0, 2.0, 2.0, -1.0, 1.5, -3.0, 5.0, -7.0, 9.0, -10.0}) x.push_back(v + 0.25 * rep);
    for (int k = 0; k < 30; ++k) x.push_back((k % 2 ? -1.0 : 1.0) * 12.0 * std::pow(0.8, k));
    x.push_back(x.back());
    all.push_back(x);
  }
  all.push_back({3.0});
  all.push_back({3.0, 3.0, 3.0});
  all.push_back({1.0, 2.0});
  int wraps = 0, overflows = 0, start_drops = 0;
  for (int depth : {4, 5}) {
    for (size_t k = 0; k < all.size(); ++k) {
      const std::vector<double> &x = all[k];
      HeapRing ring(depth);
      Sink sink;
      RainflowState<long double> s;
      const long double b = 3.0L, inv_a = 1.0L / 7.0L;
      const RainflowPower<long double> curve{b, inv_a};
      int mine = 0;
      rainflow_begin(s);
      for (double v : x) {
        rainflow_sample(s, v, depth, curve, ring, sink);
        if (s.base + s.count > depth) ++mine;                         // (the points held go round the end of the ring)
      }
      rainflow_end(s, depth, curve, ring, sink);
      std::vector<Cycle> want;
      int used = 0, starts = 0;
      const bool over = plain(x, depth, want, &used, &starts);
      bool same = want.size() == sink.list.size();
      long double damage = 0.0L;
      double cycles = 0.0, top = 0.0;
      for (size_t i = 0; same && i < want.size(); ++i)
        same = want[i].range == sink.list[i].range && want[i].mean == sink.list[i].mean && want[i].count == sink.list[i].count;
      for (const Cycle &c : want) {
        damage += (long double)c.count * powl(0.5L * c.range, b) * inv_a;
        cycles += c.count;
        if (c.range > top) top = c.range;
      }
      const bool constant = want.empty();
      check(same, "the cycle list", depth, (int)k);
      check(s.damage == damage, "the damage", depth, (int)k);
      check(s.cycles == cycles && s.max_range == top, "cycles and the largest range", depth, (int)k);
      check(s.depth_used == (constant ? 0 : used), "the depth used", depth, (int)k);
      check(s.status == (constant ? FEA_RAINFLOW_CONSTANT : (over ? FEA_RAINFLOW_OVERFLOW : 0)), "the status", depth, (int)k);
      check(s.damage == s.damage && s.count <= depth && s.base >= 0 && s.base < depth, "the ring's state", depth, (int)k);
      {                                                                // the whole exponent by squaring: the same count, the sum within rounding
        HeapRing ring2(depth);
        Sink sink2;
        RainflowState<long double> s2;
        const RainflowIntPower<long double> whole{3, inv_a};
        rainflow_begin(s2);
        for (double v : x) rainflow_sample(s2, v, depth, whole, ring2, sink2);
        rainflow_end(s2, depth, whole, ring2, sink2);
        check(s2.cycles == s.cycles && sink2.list.size() == sink.list.size() && fabsl(s2.damage - s.damage) <= 8 * LDBL_EPSILON * s.damage,
              "the whole exponent", depth, (int)k);
      }
      if (k == 2) check(mine > 0 && over && starts > 0, "the third series no longer wraps, drops its start and overflows", depth, 2);
      wraps += mine; overflows += over; start_drops += starts;
    }
  }
  // the series were chosen to exercise all three: say so if they no longer do
  check(wraps > 0, "no series wrapped the ring round", 0, -1);
  check(overflows > 0, "no series overflowed", 0, -1);
  check(start_drops > 0, "no series dropped its start point", 0, -1);
  std::printf("rainflow ring: %d checks, %d failures (wraps %d, overflowing series %d, start drops %d)\n", checks, failures, wraps,
              overflows, start_drops);
  return failures ? 1 : 0;
}
