"""The restatement of tests/fatigue_reference.py against itself: Dirlik's closed form of E[s^b] against a quadrature of his
density, the ordering of the three damage estimators, and what becomes of Dirlik's parameters towards the narrow-band
limit -- the reason the limit is taken at 1 - alpha2 <= 1e-6.  No library, no GPU."""
import numpy as np
import pytest

import fatigue_reference as fr

SHAPES = fr.shapes()


def _quadrature(y, Z):
    return float((y[1:] + y[:-1]).sum() * 0.5 * (Z[1] - Z[0]))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_closed_form_against_quadrature(name):
    """A 2 000 001-point trapezoid rule of the density on Z in [0, 60]: the expectation to 1e-12 relative for b = 3 and
    5.5, the total probability to 1e-8 (the step is 3e-5, the narrowest of the three terms about 0.1 wide)."""
    m = fr.moments_of_psd(*SHAPES[name])
    D1, D2, D3, R, Q, _, g = fr.dirlik_parameters(m)
    assert min(D1, D2, D3, Q) > 0 and 0 < g < 1
    Z = np.linspace(0.0, 60.0, 2000001)
    p = fr.dirlik_density(Z, D1, D2, D3, R, Q)
    total = _quadrature(p, Z)
    print(name, "D1 D2 D3 R Q", D1, D2, D3, R, Q, "total probability - 1", total - 1.0)
    assert abs(total - 1.0) <= 1e-8
    for b in (3.0, 5.5):
        closed, quad = float(fr.dirlik_expectation(b, D1, D2, D3, R, Q)), _quadrature(p * Z ** b, Z)
        print(name, "b", b, "closed form", closed, "quadrature", quad, "relative", abs(quad / closed - 1.0))
        assert abs(quad - closed) <= 1e-12 * closed


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("b", [1.0, 3.0, 5.5, 12.0])
def test_ordering_of_the_estimators(name, b):
    """D_TB <= D_NB always (bw <= 1 and alpha2^(b - 1) <= 1 make the factor at most 1 for b >= 1); D_DK <= D_NB on the
    three shapes."""
    m = fr.moments_of_psd(*SHAPES[name])
    rates, damage, status, near = fr.fatigue(m, b, 1e3)
    print(name, "b", b, "nu0 nup", rates, "D_DK / D_NB", damage[1] / damage[0], "D_TB / D_NB", damage[2] / damage[0])
    assert status == 0 and not near and rates[0] > 0 and rates[1] >= rates[0]
    assert 0 < damage[2] <= damage[0] and 0 < damage[1] <= damage[0]


def test_the_factor_of_tovo_and_benasciutti_is_at_most_one():
    rng = np.random.default_rng(5)
    # moments of random discrete spectra: every (alpha1, alpha2) that a PSD can give obeys alpha2 <= alpha1 <= 1
    w = rng.uniform(0.1, 50.0, (2000, 6))
    g = rng.uniform(0.0, 1.0, (2000, 6)) ** 4
    m = np.stack([(g * w ** n).sum(axis=1) for n in fr.ORDERS], axis=1)
    for b in (1.0, 2.0, 3.0, 8.0, 64.0):
        _, damage, status, _ = fr.fatigue(m, b, 1.0)
        assert np.all(np.isfinite(damage)) and np.all(damage[:, 2] <= damage[:, 0] * (1 + 1e-14)) and np.all(damage >= 0)
        assert np.all(damage[status != 0][:, 1] == damage[status != 0][:, 2])


def test_narrow_band_probe():
    """Three points at 100 (1 -+ h), S = (1, 2, 1): 1 - alpha2 falls as 0.67 h^2 and Dirlik's parameters as fast, so their
    float64 values are rounding noise long before the process is narrow in any practical sense: from h = 1e-4 on the
    float64 Q is not positive (or exactly 0) though the long-double one still is.  With the limit at 1 - alpha2 <= 1e-6
    (h = 1e-3 here) the closed form is left where Q still has three digits, and nothing is NaN beyond."""
    first_bad = None
    for h in 10.0 ** -np.arange(1, 7):
        w = np.array([100.0 * (1 - h), 100.0, 100.0 * (1 + h)])
        m = fr.moments_of_psd(w, [1.0, 2.0, 1.0])
        D1, D2, D3, R, Q, _, g = fr.dirlik_parameters(m)
        exact = fr.dirlik_parameters(fr.moments_of_psd(w, [1.0, 2.0, 1.0], fr.LD), fr.LD)
        rates, damage, status, _ = fr.fatigue(m, 3.0, 1e3)
        print(f"h {h:.0e}: 1 - alpha2 {1 - g:.3e} (long double {float(1 - exact[6]):.3e}), Q {Q:.3e} (long double {float(exact[4]):.3e}), "
              f"D1 {D1:.3e}, status {status}, damage {damage}")
        if first_bad is None and not Q > 0:
            first_bad = h
        assert np.all(np.isfinite(damage)) and np.all(damage > 0)
        assert (status == fr.NARROW) == (1 - g <= 1e-6)
        if status == fr.NARROW:
            assert damage[0] == damage[1] == damage[2]
        else:
            assert status == 0 and Q > 0 and abs(Q / float(exact[4]) - 1) < 1e-6
    assert first_bad is not None and first_bad <= 1e-4 * (1 + 1e-12)     # Q <= 0 from h = 1e-4 on
