"""Rainflow counting restated in numpy (include/fea_hip.h, "rainflow fatigue of a transient"): ASTM E1049-85's three-point
rule on a whole series held in memory -- first every reversal, then the stack -- in float64 with Miner's sum in long double,
the variant on a ring of `depth` points, and which rows of a table of histories the rounding bounds decide.  Nothing here
calls the entries under test; csrc/rainflow_point.h streams the same count a sample at a time.

The rule.  A sample equal to the one before it is dropped.  The first and the last sample left are reversals, and every
sample between them whose two neighbours lie on the same side of it.  The reversals go onto a stack one by one; after each,
while the stack holds three points or more, X = |p[-2] - p[-1]| and Y = |p[-3] - p[-2]|: X < Y ends it; if the stack holds
exactly three points Y contains the start, (p[0], p[1]) counts as half a cycle and p[0] goes; otherwise Y counts as one cycle
and p[-3], p[-2] go.  At the end every consecutive pair left counts as half a cycle, from the bottom up.
The ring.  A push onto a stack that holds `depth` points first counts (p[0], p[1]) as half a cycle and drops p[0] (the
overflow bit): what the rule does to the start point, done early.

Deciding a row.  With e a bound on the error of every sample (e_c of tests/stress_sweep_reference.py), the device and the
restatement drop the same samples and find the same reversals where every two consecutive samples differ by more than the
sum of their bounds, and close the same cycles where every X differs from its Y by more than the bounds of the three points
in them (e[p3] + 2 e[p2] + e[p1])."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
CONSTANT, OVERFLOW = 1, 2


def reversal_indices(x):
    """The indices of the reversals of the series x, ascending; one index for a constant series."""
    x = np.asarray(x, dtype=np.float64)
    keep = np.concatenate(([True], x[1:] != x[:-1])).nonzero()[0]
    if len(keep) < 3:
        return keep
    s = np.sign(np.diff(x[keep]))
    turn = (s[1:] != s[:-1]).nonzero()[0] + 1
    return keep[np.concatenate(([0], turn, [len(keep) - 1]))]


def count_points(p, depth=None, e=None):
    """The stack over the reversals p: (cycles [(range, mean, count)] in counting order, overflowed, the most points held,
    decided).  With the bounds e of the points, decided is False once an X lies within the bounds of its Y."""
    stack, cycles, used, over, decided = [], [], 0, False, True

    def half(k0, k1):
        a, b = p[k0], p[k1]
        cycles.append((abs(a - b), 0.5 * (a + b), 0.5))
    for k in range(len(p)):
        if depth is not None and len(stack) == depth:
            half(stack[0], stack[1])
            del stack[0]
            over = True
        stack.append(k)
        used = max(used, len(stack))
        while len(stack) >= 3:
            k3, k2, k1 = stack[-3], stack[-2], stack[-1]
            X, Y = abs(p[k2] - p[k1]), abs(p[k3] - p[k2])
            if e is not None and abs(X - Y) <= e[k3] + 2 * e[k2] + e[k1]:
                decided = False
            if X < Y:
                break
            if len(stack) == 3:
                half(k3, k2)
                del stack[0]
            else:
                cycles.append((Y, 0.5 * (p[k3] + p[k2]), 1.0))
                del stack[-3:-1]
    for k0, k1 in zip(stack[:-1], stack[1:]):
        half(k0, k1)
    return cycles, over, used, decided


def damage_of(cycles, b, A):
    """Miner's sum of count (range / 2)^b / A over the list, in long double, in its order."""
    total = LD(0)
    for rng, _, cnt in cycles:
        total += LD(cnt) * (LD(rng) / LD(2)) ** LD(b) / LD(A)
    return total


def count(x, b=3.0, A=1.0, depth=None, e=None):
    """The whole count of one series as a dict: cycles, damage (long double), n_cycles (the sum of the counts), max_range,
    depth_used, status, decided, reversals (their indices)."""
    x = np.asarray(x, dtype=np.float64)
    idx = reversal_indices(x)
    if len(idx) < 2:
        return dict(cycles=[], damage=LD(0), n_cycles=0.0, max_range=0.0, depth_used=0, status=CONSTANT, decided=True,
                    reversals=idx)
    cycles, over, used, decided = count_points(x[idx].tolist(), depth, None if e is None else np.asarray(e)[idx].tolist())
    return dict(cycles=cycles, damage=damage_of(cycles, b, A), n_cycles=float(sum(c for _, _, c in cycles)),
                max_range=max(r for r, _, _ in cycles), depth_used=used, status=OVERFLOW if over else 0, decided=decided,
                reversals=idx)


def damage_tolerance(n_counted, b, k=2):
    """k (c + b + 4) EPS: c additions of the sum, and b + 4 for the halving, 1 / A and the power."""
    return k * (n_counted + b + 4) * EPS


def pairs_decided(h, e):
    """[R]: every two consecutive samples of the histories h[n][R] differ by more than the sum of their bounds e[n][R]."""
    if len(h) < 2:
        return np.zeros(h.shape[1:], dtype=bool)
    return np.all(np.abs(np.diff(h, axis=0)) > e[1:] + e[:-1], axis=0)


def count_rows(h, e=None, depth=None, rows=None):
    """The count of every row of h[n][R] (or of the rows given) as arrays: n_cycles, max_range, status, depth_used, decided
    (with e[n][R]: the pairs and every closure), and reversals, the list of the reversal indices of each row."""
    n, R = h.shape
    rows = range(R) if rows is None else rows
    out = dict(n_cycles=np.zeros(R), max_range=np.zeros(R), status=np.zeros(R, dtype=np.int32), depth_used=np.zeros(R, dtype=np.int32),
               decided=np.zeros(R, dtype=bool), reversals=[None] * R)
    sure = pairs_decided(h, e) if e is not None else np.ones(R, dtype=bool)
    for r in rows:
        got = count(h[:, r], depth=depth, e=None if e is None else e[:, r])
        out["n_cycles"][r], out["max_range"][r], out["status"][r] = got["n_cycles"], got["max_range"], got["status"]
        out["depth_used"][r], out["decided"][r] = got["depth_used"], got["decided"] and sure[r]
        out["reversals"][r] = got["reversals"]
    return out
