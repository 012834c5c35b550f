// rainflow_table.cpp -- the rainflow count of one history on the host (no HIP): rainflow_point.h with the damage sum in long
// double, rounded to double once, and the list of counted cycles in counting order -- the reference of k_stress_rainflow at
// the probes' histories, and an entry for measured histories of the caller's own.
#include "../../include/fea_hip.h"
#include "rainflow_point.h"
#include <cmath>

int fatigue_constants(double sn_b, double sn_a, double *k);            // fatigue_table.cpp: refuses what an S-N curve may not be

namespace {
struct HostRing {
  double p[FEA_RAINFLOW_MAX_DEPTH];
  double get(int slot) const { return p[slot]; }
  void set(int slot, double v) { p[slot] = v; }
};
// the cycle list into the caller's arrays while they last; n counts on
struct ListSink {
  int capacity, n = 0;
  double *range, *mean, *count;
  void operator()(double r, double m, double c)
  {
    if (n < capacity) {
      if (range) range[n] = r;
      if (mean) mean[n] = m;
      if (count) count[n] = c;
    }
    ++n;
  }
};
}

// false for what both rainflow entries refuse of the curve and the ring
bool rainflow_arguments(double sn_b, double sn_a, int depth)
{
  double k[5];
  return fatigue_constants(sn_b, sn_a, k) == FEAHIP_OK && depth >= 4 && depth <= FEA_RAINFLOW_MAX_DEPTH;
}

extern "C" int feahip_host_rainflow(int n, const double *series, double sn_b, double sn_a, int depth, double *damage, double *cycles,
                                    double *max_range, int *depth_used, int *status, int capacity, int *n_counted, double *range,
                                    double *mean, double *count)
{
  if (n < 1 || !series || capacity < 0 || !rainflow_arguments(sn_b, sn_a, depth)) return FEAHIP_EINVAL;
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(series[i])) return FEAHIP_EINVAL;
  const bool listed = range || mean || count;
  const RainflowPower<long double> curve{(long double)sn_b, 1.0L / (long double)sn_a};
  HostRing ring;
  RainflowState<long double> s;
  ListSink sink{listed ? capacity : 0, 0, range, mean, count};
  rainflow_begin(s);
  for (int i = 0; i < n; ++i) rainflow_sample(s, series[i], depth, curve, ring, sink);
  rainflow_end(s, depth, curve, ring, sink);
  if (n_counted) *n_counted = sink.n;
  if (listed && sink.n > capacity) return FEAHIP_EINVAL;               // (the number needed is in *n_counted)
  if (damage) *damage = fabsl(s.damage) <= 1.7976931348623157e308L ? (double)s.damage : HUGE_VAL;
  if (cycles) *cycles = s.cycles;
  if (max_range) *max_range = s.max_range;
  if (depth_used) *depth_used = s.depth_used;
  if (status) *status = s.status;
  return FEAHIP_OK;
}
