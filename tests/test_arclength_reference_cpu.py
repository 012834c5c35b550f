"""The numpy restatement of the arc-length loop (tests/arclength_reference.py), on the CPU: it stays on the closed-form
curve of the uniaxial bar, and it follows a shallow arch through its snap-through where load control stops."""
import numpy as np

import feahip
import arclength_reference as ar
from test_oracle_closed_form import nh_closed_form
from test_surface_loads import _stretch_for, _uniaxial_bar

BAR_TRACTION = 10.0


def bar_deck():
    return _uniaxial_bar(feahip.LOAD_TRACTION, BAR_TRACTION, 4)


def test_bar_path_lies_on_the_closed_form_curve():
    deck = bar_deck()
    out = ar.arclength(deck, 4.0, 12, deck.max_newton_count, deck.desired_tolerance)
    assert out["rc"] == 0 and len(out["lam"]) >= 4 and out["lam"][-1] >= 4.0
    assert np.all(np.diff(out["lam"]) > 0)                               # no limit point on this path
    X = deck.nodes
    for lam, x in zip(out["lam"], out["x"]):
        k1 = x[X[:, 1] > 0, 1] / X[X[:, 1] > 0, 1]
        k2 = x[X[:, 0] > 0, 0] / X[X[:, 0] > 0, 0]
        assert np.ptp(k1) < 1e-10 and np.ptp(k2) < 1e-10                  # homogeneous
        # nominal stress: sigma_yy k2^2 = lambda t0 (test_uniaxial_bar_under_follower_pressure_and_dead_traction)
        want = _stretch_for(lambda k: nh_closed_form(k)[1] * nh_closed_form(k)[0] ** 2 - lam * BAR_TRACTION)
        assert abs(k1.mean() - want) < 1e-8, (lam, k1.mean(), want)
        assert abs(k2.mean() - nh_closed_form(want)[0]) < 1e-8
    # the constraint: every step has the length of the first
    steps = np.diff(np.array([deck.nodes] + out["x"]), axis=0).reshape(len(out["x"]), -1)
    assert np.abs(np.linalg.norm(steps, axis=1) / out["dl"][0] - 1.0).max() < 1e-12


def test_arch_snaps_through_and_load_control_cannot_follow():
    deck = ar.arch_deck()
    out = ar.arclength(deck, 1e9, 40, deck.max_newton_count, deck.desired_tolerance)
    lam = out["lam"]
    assert out["rc"] == 0 and len(lam) == 40
    ext = ar.extrema(lam)
    assert len(ext) == 2, (ext, lam)
    top, bottom = ext
    assert np.all(np.diff(lam[:top + 1]) > 0)                            # rises ...
    assert bottom - top >= 2 and np.all(np.diff(lam[top:bottom + 1]) < 0)   # ... falls for at least two steps ...
    assert np.all(np.diff(lam[bottom:]) > 0) and lam[-1] > lam[top]      # ... and rises again
    assert max(out["resid"]) < 1e-8                                       # every logged point is an equilibrium
    # plain load control from the same start, in increments below the first maximum: it cannot pass it -- the step
    # across the maximum fails, or lands on the snapped branch (the crown below the chord of the supports)
    n_below = int(np.floor(lam[top] / 0.5))
    factors = 0.5 * np.arange(1, n_below + 2)
    assert factors[-2] < lam[top] < factors[-1]
    done, xs = ar.load_control(deck, factors, deck.max_newton_count, deck.desired_tolerance)
    crown = np.argmax(deck.nodes[:, 1])
    assert done >= n_below                                                # the rising branch is no trouble
    assert all(x[crown, 1] > 0.5 * deck.nodes[crown, 1] for x in xs[:n_below])
    assert done < len(factors) or xs[-1][crown, 1] < 0.0, (done, xs[-1][crown, 1])
