"""The float64 restatement of the implicit dynamics (tests/dynamics_reference.py) on the CPU: its mass matrix has the
body's mass, its Newmark loop reproduces free flight and free fall, and the deck grammar carries the two new sections."""
import os

import numpy as np
import pytest

import feahip
import mesh
from dynamics_reference import (DENSITIES, DynamicsRestatement, dense_mass, element_volumes_and_mass, free_block)
from hetero_reference import MATERIALS, scattered_ids, with_materials

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynamics", "plain_bar.sexp")


def deck_of(kind):
    if kind == "tet4":
        return mesh.jitter_permute(mesh.bar_deck(dims=(3, 4, 3)))
    if kind == "tet10":
        return mesh.bar_deck(dims=(2, 2, 2), quadratic=True)
    return mesh.bar_deck(dims=(2, 3, 2), hexa=True)


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_mass_is_symmetric_and_weighs_the_body(kind):
    deck = deck_of(kind)
    ids = scattered_ids(deck)
    V, M = element_volumes_and_mass(deck, DENSITIES[ids])
    assert np.array_equal(M, M.T) or np.abs(M - M.T).max() <= 1e-16 * np.abs(M).max()
    want = float((DENSITIES[ids] * V).sum())
    assert abs(M.sum() - want) <= 1e-13 * want
    M3 = dense_mass(deck, DENSITIES, ids)
    assert M3.shape == (3 * len(deck.nodes),) * 2 and abs(M3.sum() - 3 * want) <= 1e-13 * 3 * want


def test_free_flight_and_free_fall_are_reproduced_to_rounding():
    deck = free_block()
    v0, b, dt = np.array([1.0, -2.0, 0.5]), np.array([0.3, -9.81, 1.1]), 0.01
    r = DynamicsRestatement(deck, 2.0)
    r.v = np.tile(v0, (len(deck.nodes), 1))
    done, its, traj = r.newmark(3, dt, 0.25, 0.5, 0.0, 10, 1e-20)
    r.close()
    assert done == 3
    for k, (x, v, a) in enumerate(traj):
        t = (k + 1) * dt
        assert np.abs(x - (deck.nodes + v0 * t)).max() <= 1e-12 and np.abs(v - v0).max() <= 1e-10 and np.abs(a).max() <= 1e-8
    r = DynamicsRestatement(deck, 2.0, body=b)
    r.lam = 1.0
    r.consistent_acceleration()
    assert np.abs(r.a - b).max() <= 1e-11 * np.abs(b).max()
    done, its, traj = r.newmark(3, dt, 0.25, 0.5, 0.0, 10, 1e-20)
    r.close()
    assert done == 3
    for k, (x, v, a) in enumerate(traj):
        t = (k + 1) * dt
        assert np.abs(x - (deck.nodes + 0.5 * b * t * t)).max() <= 1e-12
        assert np.abs(v - b * t).max() <= 1e-10 and np.abs(a - b).max() <= 1e-8


def dynamic_deck():
    d = mesh.bar_deck(dims=(2, 3, 2))
    return feahip.Deck(**{k: getattr(d, k) for k in ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements",
                                                     "presc_node", "presc_type", "presc_values")},
                       density=2.5, body_force=[0.0, -9.81, 0.125], dynamics=dict(steps=7, dt=1e-3, beta=0.3025, gamma=0.6, dlambda=0.5))


def test_deck_round_trip_of_the_two_sections(tmp_path):
    d = dynamic_deck()
    p = tmp_path / "dyn.sexp"
    d.save(str(p))
    text = p.read_text()
    assert "(dynamics :steps 7 :dt 0.001 :beta 0.30249999999999999 :gamma 0.59999999999999998 :dlambda 0.5 :density 2.5)" in text
    assert "(body-force :x 0 :y -9.8100000000000005 :z 0.125)" in text
    back = feahip.Deck.load(str(p))
    assert back.density == 2.5 and np.array_equal(back.body_force, d.body_force) and back.dynamics == d.dynamics
    back.save(str(tmp_path / "again.sexp"))
    assert (tmp_path / "again.sexp").read_text() == text
    # the density alone (a static deck with gravity): steps 0 and the defaults
    s = feahip.Deck(**{**{k: getattr(d, k) for k in ("nodes", "elements", "ele_type", "gauss_nodes_count")}, "density": 1.0,
                       "body_force": [0, 0, -1.0]})
    s.save(str(p))
    back = feahip.Deck.load(str(p))
    assert back.dynamics["steps"] == 0 and back.density == 1.0 and back.body_force[2] == -1.0
    with pytest.raises(ValueError):
        feahip.Deck(nodes=d.nodes, elements=d.elements, body_force=[0, 0, 1])


def test_deck_without_the_sections_saves_as_its_golden_file(tmp_path):
    d = mesh.bar_deck(dims=(1, 2, 1))
    p = tmp_path / "plain.sexp"
    d.save(str(p))
    with open(GOLDEN) as f:
        golden = f.read()
    assert p.read_text() == golden
    back = feahip.Deck.load(GOLDEN)
    assert back.density is None and back.body_force is None and back.dynamics is None
    back.save(str(p))
    assert p.read_text() == golden


def test_parser_refuses_malformed_sections(tmp_path):
    d = dynamic_deck()
    p = tmp_path / "dyn.sexp"
    d.save(str(p))
    text = p.read_text()

    def refused(old, new, what):
        assert old in text
        q = tmp_path / "bad.sexp"
        q.write_text(text.replace(old, new))
        with pytest.raises(feahip.FeaHipError, match=what):
            feahip.Deck.load(str(q))

    refused(":steps 7", ":steps -1", "steps must be a non-negative integer")
    refused(":steps 7 ", "", "missing attribute :steps")
    refused(":dt 0.001", ":dt 0", "dt must be positive")
    refused(":dt 0.001 ", "", "missing attribute :dt")
    refused(":beta 0.30249999999999999", ":beta 0", "beta must be positive")
    refused(":gamma 0.59999999999999998", ":gamma -0.5", "gamma must not be negative")
    refused(" :density 2.5", "", "missing attribute :density")
    refused(":density 2.5", ":density -1", "density must be positive")
    refused(":z 0.125", "", "missing attribute :z")
    dyn = text[text.index("\n   (dynamics"):text.index(":density 2.5)") + len(":density 2.5)")]
    refused(dyn, "", r"\(body-force \.\.\.\) but no \(dynamics")
