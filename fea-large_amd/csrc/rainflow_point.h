// rainflow_point.h -- the rainflow count of ONE stress history, streamed a sample at a time: ASTM E1049-85's three-point
// rule on a bounded stack, with Miner's sum on the S-N curve N s^b = A (s the stress AMPLITUDE, range / 2).  One copy of
// the arithmetic: k_stress_rainflow (kernels_stress_rainflow.hip) runs it with the damage in double and the stack in device
// memory, feahip_host_rainflow (rainflow_table.cpp) with the damage in long double and the stack in an array -- the
// reference the device is held to.  Every comparison is taken on doubles, so the two agree in everything but the damage sum.
//   damage     count (range / 2)^b / A per counted cycle, summed in counting order (count is 1 or 0.5, so its product is exact)
//   reversals  a sample equal to the last kept one is dropped; the first sample is a reversal; a kept sample is confirmed
//              as a reversal when the next different sample moves the other way (a strict change of sign); after the last
//              sample the last kept one is pushed if the history ever moved.
//   the rule   after every push, while the stack holds three points or more: X = |p[-2] - p[-1]|, Y = |p[-3] - p[-2]|;
//              X < Y ends it; with exactly three points Y contains the start: (p[0], p[1]) is half a cycle and p[0] goes;
//              otherwise Y is one cycle and p[-3], p[-2] go.  At the end every consecutive pair left is half a cycle, from
//              the bottom up.
//   the ring   the stack is a ring of `depth` points, 4 <= depth <= FEA_RAINFLOW_MAX_DEPTH, slot (base + i) of `depth`
//              holding point i.  A push onto a full ring first counts (p[0], p[1]) as half a cycle and drops p[0], the
//              rule ASTM has for the start point and the residue, and sets FEA_RAINFLOW_OVERFLOW.  A ring-down, whose
//              ranges only shrink so that nothing closes, is counted exactly at any depth; only a later range large
//              enough to close a dropped one makes the count approximate.
// The status: FEA_RAINFLOW_CONSTANT fewer than two reversals (a constant history), everything 0; FEA_RAINFLOW_OVERFLOW.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define FEA_RF_HD __host__ __device__
#else
#define FEA_RF_HD
#endif

#define FEA_RAINFLOW_CONSTANT 1
#define FEA_RAINFLOW_OVERFLOW 2

// what a history carries from sample to sample (and a stress row from launch to launch); T the type of the damage sum
template <class T>
struct RainflowState {
  double last;                         // the last kept sample
  int dir;                             // 0 before the history has moved, then +1 / -1: the way `last` was reached
  int base, count;                     // the ring: the slot of point 0, and the points held
  T damage;                            // sum of count (range / 2)^b / A, in counting order
  double cycles, max_range;
  int depth_used, status;
  int seen;                            // 0 before the first sample
};

template <class T>
FEA_RF_HD inline void rainflow_begin(RainflowState<T> &s)
{
  s.last = 0.0; s.dir = 0; s.base = 0; s.count = 0;
  s.damage = T(0); s.cycles = 0.0; s.max_range = 0.0; s.depth_used = 0; s.status = 0; s.seen = 0;
}

// the slot of point i (0 <= i < depth) of a ring whose point 0 is at `base`
FEA_RF_HD inline int rainflow_slot(int base, int i, int depth)
{
  const int k = base + i;
  return k >= depth ? k - depth : k;
}

// The S-N curve N s^b = A as the damage of one cycle of amplitude s, s^b / A, with 1 / A made once on the host.
// RainflowPower takes any exponent through pow; RainflowIntPower a whole one by squaring and multiplying, b - 1 products at
// the most on the longest path and a handful of registers where pow needs sixty (the device picks it for a whole b).
template <class T>
struct RainflowPower {
  T b, inv_a;
  FEA_RF_HD T operator()(T s) const { using std::pow; return pow(s, b) * inv_a; }
};
template <class T>
struct RainflowIntPower {
  int b;                               // >= 1
  T inv_a;
  FEA_RF_HD T operator()(T s) const
  {
    T r = T(1);
    for (int n = b;;) {
      if (n & 1) r *= s;
      n >>= 1;
      if (!n) break;
      s *= s;
    }
    return r * inv_a;
  }
};

// one counted range between the points p and q; sink(range, mean, count) takes the cycle list (the device passes none)
template <class T, class Curve, class Sink>
FEA_RF_HD inline void rainflow_count(RainflowState<T> &s, double p, double q, double count, const Curve &curve, Sink &sink)
{
  using std::fabs;
  const double range = fabs(p - q);
  s.damage += T(count) * curve(T(0.5 * range));
  s.cycles += count;
  if (range > s.max_range) s.max_range = range;
  sink(range, 0.5 * (p + q), count);
}

// the reversal v onto the ring, then the three-point rule; Stack has get(slot) and set(slot, value)
template <class T, class Curve, class Stack, class Sink>
FEA_RF_HD inline void rainflow_push(RainflowState<T> &s, double v, int depth, const Curve &curve, Stack &stack, Sink &sink)
{
  using std::fabs;
  if (s.count == depth) {                                              // a full ring: the bottom pair as half a cycle
    const double p0 = stack.get(s.base), p1 = stack.get(rainflow_slot(s.base, 1, depth));
    rainflow_count(s, p0, p1, 0.5, curve, sink);
    s.base = rainflow_slot(s.base, 1, depth);
    s.count -= 1;
    s.status |= FEA_RAINFLOW_OVERFLOW;
  }
  stack.set(rainflow_slot(s.base, s.count, depth), v);
  s.count += 1;
  if (s.count > s.depth_used) s.depth_used = s.count;
  while (s.count >= 3) {
    const double p2 = stack.get(rainflow_slot(s.base, s.count - 2, depth));
    const double p3 = stack.get(rainflow_slot(s.base, s.count - 3, depth));
    const double X = fabs(p2 - v), Y = fabs(p3 - p2);
    if (X < Y) break;
    if (s.count == 3) {                                                // Y contains the start: p3 is p[0]
      rainflow_count(s, p3, p2, 0.5, curve, sink);
      s.base = rainflow_slot(s.base, 1, depth);
      s.count = 2;
    } else {
      rainflow_count(s, p3, p2, 1.0, curve, sink);
      s.count -= 2;
      stack.set(rainflow_slot(s.base, s.count - 1, depth), v);
    }
  }
}

// the next sample of the history
template <class T, class Curve, class Stack, class Sink>
FEA_RF_HD inline void rainflow_sample(RainflowState<T> &s, double u, int depth, const Curve &curve, Stack &stack, Sink &sink)
{
  if (!s.seen) {
    s.seen = 1; s.last = u;
    rainflow_push(s, u, depth, curve, stack, sink);
    return;
  }
  if (u == s.last) return;
  const int d = u > s.last ? 1 : -1;
  if (s.dir != 0 && d != s.dir) rainflow_push(s, s.last, depth, curve, stack, sink);
  s.dir = d;
  s.last = u;
}

// after the last sample: the final reversal, then the residue from the bottom up
template <class T, class Curve, class Stack, class Sink>
FEA_RF_HD inline void rainflow_end(RainflowState<T> &s, int depth, const Curve &curve, Stack &stack, Sink &sink)
{
  if (s.dir != 0) rainflow_push(s, s.last, depth, curve, stack, sink);
  if (s.dir == 0) {                                                    // fewer than two reversals
    s.damage = T(0); s.cycles = 0.0; s.max_range = 0.0; s.depth_used = 0;
    s.status = FEA_RAINFLOW_CONSTANT;
    return;
  }
  double p = stack.get(s.base);
  for (int i = 1; i < s.count; ++i) {
    const double q = stack.get(rainflow_slot(s.base, i, depth));
    rainflow_count(s, p, q, 0.5, curve, sink);
    p = q;
  }
}
