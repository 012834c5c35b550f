"""Pins tests/results_reference.py, the float64 restatement the GPU result recovery is held to, without a GPU: its
energy is the potential of the oracle's residual, a homogeneous state gives the closed forms, the nodal energy shares
add up, and the (results ...) deck section makes the round trip through libfeahost.so."""
import os

import numpy as np
import pytest

import feahip
from dynamics_reference import free_block, loaded_bar
from results_reference import ResultsRestatement, cauchy, psi, smooth_field, von_mises

MODELS = {"neohookean": feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, "a5": feahip.MODEL_A5}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynamics", "explicit_bar.sexp")
# The error of the central difference is measured against |f| |delta| (f . delta itself nearly cancels for some
# directions).  It falls with h^2 down to h = 1e-6 (truncation: 1e-4 -> 1e-5 -> 1e-6 gave 2.3e-4, 2.3e-6, 2.1e-8 absolute
# on tet10 / a5), where rounding of W / h takes over.  Measured at h = 1e-6, the largest of the three directions:
# tet4 2.7e-11 / 3.3e-11, tet10 4.4e-11 / 1.05e-10, hex8 1.9e-11 / 1.7e-11 (neohookean / a5); ten times the largest
POTENTIAL_TOL = 1.05e-9


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_energy_is_the_potential_of_the_oracle_residual(kind, model):
    """Central difference of W along three random directions against -f . delta, f the oracle's unmasked residual (-T).
    Measured: see POTENTIAL_TOL."""
    deck = loaded_bar(kind, (2, 4, 2), model=MODELS[model])
    r = ResultsRestatement(deck)
    x = smooth_field(deck.nodes)
    F, _, dj = r.state(x)
    assert np.abs(F - np.eye(3)).max() >= 0.05 and np.all(dj > 0)
    f = r.internal(x)
    rng = np.random.default_rng(11)
    h = 1e-6
    worst = 0.0
    for _ in range(3):
        delta = rng.uniform(-1.0, 1.0, x.shape)
        dW = (r.energy(x + h * delta)[0] - r.energy(x - h * delta)[0]) / (2.0 * h)
        want = -float(f @ delta.ravel())
        worst = max(worst, abs(dW - want) / (np.linalg.norm(f) * np.linalg.norm(delta)))
    print(kind, model, "potential", worst)
    r.close()
    assert worst <= POTENTIAL_TOL


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_homogeneous_state_gives_the_closed_forms(kind, model):
    deck = free_block(kind, (2, 2, 2), model=MODELS[model], parameters=[120.0, 80.0])
    F = np.array([[1.10, 0.07, 0.00], [0.00, 0.95, 0.04], [0.02, 0.00, 1.05]])
    x = deck.nodes @ F.T
    r = ResultsRestatement(deck)
    sig = cauchy(F, MODELS[model], 120.0, 80.0)
    want6 = np.array([sig[0, 0], sig[1, 1], sig[2, 2], sig[0, 1], sig[1, 2], sig[0, 2]])
    sig6, vm, wt = r.nodal_stresses(x)
    scale = np.abs(sig).max()
    assert np.abs(sig6 - want6[None, :]).max() <= 1e-12 * scale
    dev = sig - np.trace(sig) / 3.0 * np.eye(3)
    vm_closed = np.sqrt(1.5 * (dev * dev).sum())
    assert np.abs(vm - vm_closed).max() <= 1e-12 * vm_closed and abs(von_mises(want6) - vm_closed) <= 1e-14 * vm_closed
    assert np.all(wt > 0) and abs(wt.sum() - deck.nodes_per_element * np.linalg.det(F)) <= 1e-12 * wt.sum()
    W, _ = r.energy(x)
    V0 = 1.0
    assert abs(W - V0 * psi(F, MODELS[model], 120.0, 80.0)) <= 1e-12 * abs(W)
    r.close()


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_nodal_shares_sum_to_the_energy(kind):
    deck = loaded_bar(kind, (2, 4, 2))
    r = ResultsRestatement(deck)
    W, wn = r.energy(smooth_field(deck.nodes))
    r.close()
    assert W > 0 and abs(wn.sum() - W) <= 1e-13 * W


def test_results_section_round_trip(tmp_path):
    deck = loaded_bar("tet4", (2, 4, 2), results=dict(nodal_stress=True, reactions=True))
    p = tmp_path / "with_results.sexp"
    deck.save(str(p))
    assert "(results :nodal-stress t :energy nil :reactions t)" in p.read_text()
    back = feahip.Deck.load(str(p))
    assert back.results == dict(nodal_stress=True, energy=False, reactions=True)
    q = tmp_path / "again.sexp"
    back.save(str(q))
    assert q.read_bytes() == p.read_bytes()
    for flags in (dict(energy=True), dict(nodal_stress=True, energy=True, reactions=True)):
        d = loaded_bar("tet4", (2, 4, 2), results=flags)
        d.save(str(q))
        assert feahip.Deck.load(str(q)).results == {k: bool(flags.get(k)) for k in ("nodal_stress", "energy", "reactions")}
    bad = tmp_path / "bad.sexp"
    bad.write_text(p.read_text().replace(":energy nil", ":energy maybe"))
    with pytest.raises(feahip.FeaHipError):
        feahip.Deck.load(str(bad))


def test_a_deck_without_the_section_saves_as_before(tmp_path):
    """The committed deck was written by fea_deck_save before the section existed: loading and saving it gives the
    same bytes, and no flag is set."""
    d = feahip.Deck.load(GOLDEN)
    assert d.results == dict(nodal_stress=False, energy=False, reactions=False)
    p = tmp_path / "explicit_bar.sexp"
    d.save(str(p))
    with open(GOLDEN, "rb") as f:
        assert p.read_bytes() == f.read()
