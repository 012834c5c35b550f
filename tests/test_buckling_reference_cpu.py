"""The float64 restatement of linear buckling (tests/buckling_reference.py) on the CPU oracle: the fact the one-double-
per-block storage of K_sigma rests on, the model's behaviour under load scaling and refinement, and the emulation of the
driver's step that sizes max_iterations.  No GPU, nothing of the library under test.

Measured on the CPU oracle: K is positive definite on the three column decks; the lowest eight nu are negative on all
three (TET4 -0.0257 to -0.0085, HEX8 in degenerate pairs from -0.0392, TET10 from -0.0398); HEX8 also has 12 positive
nu.  Steps of the emulation under block-Jacobi to 1e-8 for six modes, over eight start blocks: TET4 157 to 188, HEX8 161
to 184, TET10 183 to 206 (157, 161, 183 from the start block the tests use); the clamped-free column under its traction
300 to 361, the (3, 12, 3) TET4 column 387 to 433.  Without the renewal of P's products every 20 steps the same
emulation took 159 to 452 steps on TET4 and 193 to 748 on TET10, which is why the driver renews them."""
import math

import numpy as np
import pytest

import buckling_reference as br

KINDS = ("tet4", "hex8", "tet10")
TOL, MAX_IT = 1e-8, 2000


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_ks_is_a_scalar_times_the_identity_per_node_pair(kind):
    """Exactly 0.0: the off-diagonal entries of every 3x3 block and the differences among its three diagonal entries."""
    deck, x, _ = br.column_reference(kind)
    pairs = br.element_pairs(deck, x)
    npe = deck.elements.shape[1]
    dev = max(br.identity_deviation(ks, npe) for _, ks in pairs)
    scale = max(np.abs(ks).max() for _, ks in pairs)
    print(kind, "deviation", dev, "max |Ks|", scale)
    assert scale > 0.0
    assert dev == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_columns_are_stable_and_compressed(kind):
    _, _, ref = br.column_reference(kind)
    print(kind, "min eig K", ref.min_eig_K, "nu", ref.nu[:8], "positive nu", int((ref.nu > 1e-12).sum()))
    assert len(ref.free) == 189
    assert ref.min_eig_K > 0.0
    assert np.all(ref.nu[:8] < 0.0)
    assert np.all(np.isfinite(ref.factor(8))) and np.all(np.diff(ref.factor(8)) >= 0)
    G = ref.Phi[:, :8].T @ ref.K @ ref.Phi[:, :8]
    assert np.abs(G - np.eye(8)).max() <= 1e-10
    for j in range(8):
        assert ref.residual_ratio(ref.nu[j], ref.Phi[:, j]) <= 1e-10


def test_hex8_geometric_stiffness_is_indefinite():
    _, _, ref = br.column_reference("hex8")
    assert (ref.nu > 1e-12).sum() == 12


def test_load_scaling():
    """factor x |end motion| estimates the critical end motion whatever preload it is computed at: at -0.02 and at -0.04
    the two agree within 1 % (measured: 0.09995 and 0.10036 as end strains, 0.42 % apart)."""
    a = br.column_reference("tet4", -0.02)[2].factor(1)[0] * 0.02
    b = br.column_reference("tet4", -0.04)[2].factor(1)[0] * 0.04
    print("critical end strain at -0.02:", a / 8.0, "at -0.04:", b / 8.0, "apart", abs(a - b) / a)
    assert abs(a - b) <= 0.01 * a


def test_refinement_lowers_the_critical_strain():
    """TET10 columns of size (1, 8, 1): (1, 6, 1) cells against (2, 12, 2).  Euler's clamped-clamped value
    4 pi^2 I / (A L^2) is printed beside them and not asserted: the column is stubby (measured 0.0458 and 0.0437)."""
    strain = []
    for dims in ((1, 6, 1), (2, 12, 2)):
        deck = br.column_deck("tet10", br.END_MOTION, dims=dims, size=(1.0, 8.0, 1.0))
        ref = br.BucklingReference(deck, br.newton_state(deck))
        assert ref.min_eig_K > 0.0
        strain.append(ref.factor(1)[0] * abs(br.END_MOTION) / 8.0)
    print("critical end strain", strain, "Euler clamped-clamped", 4.0 * math.pi ** 2 / (12.0 * 64.0))
    assert strain[1] < strain[0]


@pytest.mark.parametrize("kind", KINDS)
def test_emulation_of_the_step_converges(kind):
    _, _, ref = br.column_reference(kind)
    nu, ratio, steps = ref.emulate(6, TOL, MAX_IT)
    print(kind, "emulation steps", steps, "rel err", np.abs(nu - ref.nu[:6]) / np.abs(ref.nu[:6]))
    assert steps <= 1000                                    # block-Jacobi is enough on every deck (the GPU tests use it)
    assert np.all(ratio <= TOL)
    assert np.all(np.abs(nu - ref.nu[:6]) <= 1e-6 * np.abs(ref.nu[:6]))


def test_traction_column_is_a_stable_equilibrium_on_the_load_path():
    """The deck of the GPU load-path test: the reference's Newton loop under load control converges at the full
    traction with K positive definite, and the column buckles in this load direction (nu < 0)."""
    import arclength_reference as ar
    deck = br.traction_column()
    done, xs = ar.load_control(deck, [1.0], deck.max_newton_count, deck.desired_tolerance)
    assert done == 1
    ref = br.BucklingReference(deck, xs[0])
    euler = math.pi ** 2 * 250.0 / 12.0 / (4.0 * 64.0)      # E = 250 for (100, 100), I = 1/12, L = 8, clamped-free
    print("min eig K", ref.min_eig_K, "nu", ref.nu[:4], "critical traction", ref.factor(1)[0] * br.TRACTION, "Euler", euler)
    assert len(ref.free) == 216
    assert ref.min_eig_K > 0.0
    assert ref.nu[0] < 0.0 and np.isfinite(ref.factor(1)[0]) and ref.factor(1)[0] > 1.0
