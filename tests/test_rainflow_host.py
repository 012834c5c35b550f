"""Rainflow counting on the host side: feahip.host_rainflow against the textbook count of tests/rainflow_reference.py -- the
standard's example, several hundred random series with ties and flat runs at depth 1024 and on rings of 4 and 8 points, a
ring-down at depth 4, the short series, every refusal -- feahip.plane_projections, the constants and the exported symbols,
the three deck keys of (transient ...) through reader and writer, and csrc/rainflow_point.h over exactly sized rings as a stand-alone program under AddressSanitizer and UBSan.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import feahip
import rainflow_reference as rr
from test_stress_reference_cpu import _deck
from test_stress_sweep_reference_cpu import TRANSIENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = rr.LD
NEW = ("feahip_host_rainflow", "feahip_response_stress_rainflow")
ASTM = [-2, 1, -3, 5, -1, 3, -4, 4, -2]


def same_count(what, got, want, b):
    """The cycle list to the bit and in order, the four numbers, and the damage within (c + b + 4) EPS of the long-double
    sum over the reference's list."""
    cyc = want["cycles"]
    assert len(got["ranges"]) == len(cyc), (what, len(got["ranges"]), len(cyc))
    if cyc:
        r, m, c = (np.array(v) for v in zip(*cyc))
        assert np.array_equal(got["ranges"], r) and np.array_equal(got["means"], m) and np.array_equal(got["counts"], c), what
    assert got["cycles"] == want["n_cycles"] and got["max_range"] == want["max_range"], what
    assert got["status"] == want["status"] and got["depth_used"] == want["depth_used"], (what, got["status"], got["depth_used"], want)
    exact = want["damage"]
    tol = rr.damage_tolerance(len(cyc), b, 1)
    err = abs(LD(got["damage"]) - exact)
    assert err <= tol * exact, (what, float(err / exact) if exact else 0.0, tol)
    assert np.isfinite(got["damage"])
    return float(err / exact) if exact else 0.0


def test_the_example_of_the_standard():
    """ASTM E1049-85, figure 6: ranges 3, 4, 6, 8, 9 with counts 0.5, 1.5, 0.5, 1.0, 0.5."""
    got = feahip.host_rainflow(ASTM, 3.0, 1.0, 1024)
    table = {}
    for r, c in zip(got["ranges"], got["counts"]):
        table[r] = table.get(r, 0.0) + c
    assert table == {3.0: 0.5, 4.0: 1.5, 6.0: 0.5, 8.0: 1.0, 9.0: 0.5}
    assert got["cycles"] == 4.0 and got["max_range"] == 9.0 and got["status"] == 0
    same_count("the standard's example", got, rr.count(ASTM, 3.0, 1.0), 3.0)
    # the one full cycle is (-1, 3), closed inside (5, -4): range 4, mean 1
    full = [(r, m) for r, m, c in zip(got["ranges"], got["means"], got["counts"]) if c == 1.0]
    assert full == [(4.0, 1.0)]


def random_series(seed, count):
    rng = np.random.default_rng(seed)
    for k in range(count):
        n = int(rng.integers(1, 401))
        x = np.round(rng.standard_normal(n) * (1 + k % 7), int(rng.integers(0, 3)))
        if k % 5 == 0:
            x = np.cumsum(x)                                             # a random walk: long excursions, deep stacks
            x = np.round(x, int(rng.integers(0, 3)))
        yield k, x


def test_random_series_with_ties_and_flat_runs():
    """400 series of 1 to 400 samples rounded to 0, 1 or 2 decimals: the list of the unbounded count at depth 1024, the list
    of the ring variant at depths 4 and 8 with its overflow bit and depth used."""
    worst, overflowed, flat, deepest = 0.0, {4: 0, 8: 0}, 0, 0
    for k, x in random_series(41, 400):
        b, A = (3.0, 1.0) if k % 2 else (5.5, 1e3)
        flat += int(len(x) > 1 and (x[1:] == x[:-1]).any())
        unbounded = rr.count(x, b, A)
        deepest = max(deepest, unbounded["depth_used"])
        assert unbounded["depth_used"] <= 1024
        worst = max(worst, same_count(f"series {k} unbounded", feahip.host_rainflow(x, b, A, 1024), unbounded, b))
        for depth in (4, 8):
            want = rr.count(x, b, A, depth)
            overflowed[depth] += want["status"] == rr.OVERFLOW
            worst = max(worst, same_count(f"series {k} depth {depth}", feahip.host_rainflow(x, b, A, depth), want, b))
    print("largest damage error / damage", worst, "; series with a flat run", flat, "; overflowed", overflowed, "; deepest stack", deepest)
    assert flat >= 100 and overflowed[4] >= 100 and 0 < overflowed[8] < overflowed[4]


def test_a_ring_down_is_exact_at_depth_4():
    """200 periods of a decaying cosine: nothing ever closes, the unbounded count holds every reversal, and the ring of four
    points gives its list with the overflow bit set."""
    t = np.arange(0, 200, 0.5)
    x = np.exp(-0.01 * t) * np.cos(2 * np.pi * t)
    unbounded = rr.count(x, 3.0, 2.0)
    assert unbounded["depth_used"] == len(x) and unbounded["status"] == 0
    got = feahip.host_rainflow(x, 3.0, 2.0, 4)
    assert got["status"] == feahip.RAINFLOW_OVERFLOW and got["depth_used"] == 4
    want = dict(unbounded, status=rr.OVERFLOW, depth_used=4)
    same_count("ring-down at depth 4", got, want, 3.0)
    same_count("ring-down at depth 1024", feahip.host_rainflow(x, 3.0, 2.0, 1024), unbounded, 3.0)


def test_short_and_constant_series():
    for x in ([2.5], [2.5, 2.5, 2.5], np.zeros(50)):
        got = feahip.host_rainflow(x, 3.0, 1.0)
        assert got["status"] == feahip.RAINFLOW_CONSTANT and got["damage"] == 0.0 and got["cycles"] == 0.0
        assert got["max_range"] == 0.0 and got["depth_used"] == 0 and len(got["ranges"]) == 0
        same_count("constant", got, rr.count(x), 3.0)
    got = feahip.host_rainflow([1.0, 3.0], 2.0, 4.0)
    assert got["status"] == 0 and got["cycles"] == 0.5 and got["max_range"] == 2.0 and got["depth_used"] == 2
    assert got["damage"] == 0.5 * 1.0 / 4.0 and got["ranges"].tolist() == [2.0] and got["means"].tolist() == [2.0]
    same_count("two samples", got, rr.count([1.0, 3.0], 2.0, 4.0), 2.0)
    same_count("a flat start", feahip.host_rainflow([1.0, 1.0, 3.0, 3.0, 2.0], 2.0, 4.0), rr.count([1.0, 1.0, 3.0, 3.0, 2.0], 2.0, 4.0), 2.0)


def _raw(series, b=3.0, A=1.0, depth=32, n=None, capacity=None, lists=True):
    x = np.ascontiguousarray(series, dtype=np.float64)
    cap = len(x) if capacity is None else capacity
    d = [C.c_double(-7.0) for _ in range(3)]
    i = [C.c_int(-7) for _ in range(3)]
    arr = [np.full(max(cap, 1), -7.0) for _ in range(3)]
    dp = C.POINTER(C.c_double)
    rc = feahip.load_library().feahip_host_rainflow(len(x) if n is None else n, x.ctypes.data_as(dp), b, A, depth, C.byref(d[0]),
                                                    C.byref(d[1]), C.byref(d[2]), C.byref(i[0]), C.byref(i[1]), cap, C.byref(i[2]),
                                                    *(a.ctypes.data_as(dp) if lists else None for a in arr))
    return rc, [v.value for v in d], [v.value for v in i], arr


def test_refusals():
    good = np.array(ASTM, dtype=np.float64)
    assert _raw(good)[0] == 0
    for kw in (dict(n=0), dict(n=-1), dict(b=0.5), dict(b=64.5), dict(b=np.nan), dict(A=0.0), dict(A=-1.0), dict(A=np.inf),
               dict(depth=3), dict(depth=1025), dict(depth=0), dict(capacity=-1)):
        rc, d, i, arr = _raw(good, **kw)
        assert rc == feahip.EINVAL, kw
        assert d == [-7.0] * 3 and i == [-7] * 3 and all((a == -7).all() for a in arr), kw
    for bad in (np.nan, np.inf, -np.inf):
        x = good.copy()
        x[4] = bad
        assert _raw(x)[0] == feahip.EINVAL
        with pytest.raises(feahip.FeaHipError):
            feahip.host_rainflow(x, 3.0, 1.0)
    # a list too short: the number needed comes back, the five numbers stay
    rc, d, i, arr = _raw(good, capacity=3)
    assert rc == feahip.EINVAL and i[2] == 7 and d == [-7.0] * 3 and i[:2] == [-7, -7]
    rc, d, i, arr = _raw(good, capacity=7)
    assert rc == 0 and i[2] == 7 and d[1] == 4.0
    rc, d, i, arr = _raw(good, capacity=0, lists=False)                  # no list wanted: any capacity
    assert rc == 0 and i[2] == 7 and d[1] == 4.0
    assert feahip.host_rainflow(good, 1.0, 1.0, 4)["cycles"] == 4.0 and feahip.host_rainflow(good, 64.0, 1e300, 1024)["damage"] >= 0.0
    for name in NEW:
        assert name in feahip.ABI
    assert (feahip.RAINFLOW_MAX_DEPTH, feahip.RAINFLOW_MAX_PROJ, feahip.RAINFLOW_CONSTANT, feahip.RAINFLOW_OVERFLOW) == (1024, 48, 1, 2)
    header = open(os.path.join(ROOT, "include", "fea_hip.h")).read()
    for text in ("#define FEA_RAINFLOW_MAX_DEPTH 1024", "#define FEA_RAINFLOW_MAX_PROJ  48"):
        assert text in header


def test_plane_projections():
    """Rows (nx^2, ny^2, nz^2, 2 nx ny, 2 ny nz, 2 nx nz) of the normalised normals: n' sigma n for sigma in the order xx yy
    zz xy yz xz."""
    rng = np.random.default_rng(5)
    normals = np.vstack([[3.0, 0.0, 0.0], [0.0, -2.0, 0.0], rng.standard_normal((20, 3))])
    P = feahip.plane_projections(normals)
    assert P.shape == (22, 6) and P.flags["C_CONTIGUOUS"]
    assert P[0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] and P[1].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    s6 = rng.standard_normal((7, 6))
    for n, row in zip(normals, P):
        u = n / np.linalg.norm(n)
        for s in s6:
            full = np.array([[s[0], s[3], s[5]], [s[3], s[1], s[4]], [s[5], s[4], s[2]]])
            assert abs(row @ s - u @ full @ u) <= 16 * rr.EPS * np.abs(s).sum()
    assert abs(P[:, :3].sum(axis=1) - 1.0).max() <= 4 * rr.EPS
    assert feahip.plane_projections([0.0, 0.0, 5.0]).tolist() == [[0.0, 0.0, 1.0, 0.0, 0.0, 0.0]]


def test_the_ring_under_sanitizers(tmp_path):
    """tests/host_rainflow_check.cpp: the host instantiation of csrc/rainflow_point.h on heap rings of exactly 4 and 5
    doubles -- wrap-around, start-point drops and overflow in one series -- built with plain g++ under AddressSanitizer and
    UBSan and run as a program; nothing is loaded into this process."""
    exe = str(tmp_path / "host_rainflow_check")
    cmd = ["g++", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
           "-I" + os.path.join(ROOT, "fea-large_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_rainflow_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    # 2 depths x 6 series x 7 checks, the third series' own check at either depth, and the three at the end
    assert "rainflow ring: %d checks, 0 failures" % (2 * 6 * 7 + 2 + 3) in r.stdout, r.stdout[-2000:]


def test_deck_round_trip_of_the_three_keys(tmp_path):
    """:sn-exponent b :sn-coefficient A :rainflow-depth d inside (transient ... :stress t) are read, written and read again;
    a deck without them is written byte for byte as before; the keys are refused without :stress t, without the exponent and
    out of range."""
    p = tmp_path / "rainflow.sexp"
    keys = dict(transient_sn_exponent=3.5, transient_sn_coefficient=2e12, transient_rainflow_depth=48)
    _deck(**TRANSIENT, transient_stress=True, **keys).save(str(p))
    text = p.read_text()
    assert text.count(":sn-exponent 3.5 :sn-coefficient 2000000000000 :rainflow-depth 48") == 1
    back = feahip.Deck.load(str(p))
    fd = back.to_struct()
    assert (fd.transient_sn_exponent, fd.transient_sn_coefficient, fd.transient_rainflow_depth) == (3.5, 2e12, 48)
    assert (back.transient_sn_exponent, back.transient_sn_coefficient, back.transient_rainflow_depth) == (3.5, 2e12, 48)
    back.save(str(p))
    assert p.read_text() == text
    _deck(**TRANSIENT, transient_stress=True).save(str(p))
    plain = p.read_text()
    assert ":sn-" not in plain and ":rainflow-depth" not in plain
    assert plain == text.replace(" :sn-exponent 3.5 :sn-coefficient 2000000000000 :rainflow-depth 48", "")
    again = feahip.Deck.load(str(p))
    assert again.transient_sn_exponent == 0.0 and again.to_struct().transient_sn_exponent == 0.0
    # the depth defaults to 32
    p.write_text(text.replace(" :rainflow-depth 48", ""))
    assert feahip.Deck.load(str(p)).transient_rainflow_depth == 32
    for old, new in ((":sn-exponent 3.5", ":sn-exponent 0.5"), (":sn-exponent 3.5", ":sn-exponent 65"), (":sn-exponent 3.5 ", ""),
                     (":sn-coefficient 2000000000000", ":sn-coefficient 0"), (":sn-coefficient 2000000000000 ", ""),
                     (":rainflow-depth 48", ":rainflow-depth 3"), (":rainflow-depth 48", ":rainflow-depth 1025"),
                     (":rainflow-depth 48", ":rainflow-depth 7.5"), (" :stress t", "")):
        assert text.count(old) == 1
        p.write_text(text.replace(old, new))
        with pytest.raises(feahip.FeaHipError):
            feahip.Deck.load(str(p))
    for kw in (dict(transient_sn_exponent=3.0, transient_sn_coefficient=1.0), dict(transient_stress=True, transient_sn_coefficient=1.0),
               dict(transient_stress=True, transient_rainflow_depth=16), dict(transient_stress=True, transient_sn_exponent=3.0),
               dict(transient_stress=True, transient_sn_exponent=3.0, transient_sn_coefficient=1.0, transient_rainflow_depth=2)):
        with pytest.raises(ValueError, match="transient_sn|transient_rainflow"):
            _deck(**TRANSIENT, **kw)
