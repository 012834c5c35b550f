"""The restatement the GPU explicit-dynamics tests compare against (tests/explicit_reference.py), checked on its own:
HRZ lumping, the Gershgorin step against a dense eigenvalue, momentum and energy of the central-difference loop, and
the deck grammar of the explicit scheme.  No GPU."""
import functools

import numpy as np
import pytest

import feahip
import mesh
from dynamics_reference import DENSITIES, free_block, loaded_bar
from explicit_reference import ExplicitRestatement, body_mass, gershgorin_bound, hrz_lumped_mass, hub_fan, omega_max
from hetero_reference import scattered_ids

KINDS = ["tet4", "tet10", "hex8"]
DIMS = (2, 4, 2)


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_hrz_masses_are_positive_and_keep_the_mass(kind, table):
    deck = loaded_bar(kind, DIMS)
    ids = scattered_ids(deck)
    rho = DENSITIES if table else 2.5
    ml = hrz_lumped_mass(deck, rho, ids)
    total = body_mass(deck, rho, ids)
    print(kind, table, "min ml", ml.min(), "sum", ml.sum(), "body", total)
    assert ml.min() > 0.0
    assert abs(ml.sum() - total) <= 1e-13 * total
    if not table:
        assert abs(total - 2.5 * 2.0) <= 1e-12                # the 1 x 2 x 1 bar


def test_the_row_sum_would_not_do_for_the_quadratic_tetrahedron():
    """Why HRZ: the row sum of the 10-node tetrahedron's consistent mass is not positive at the corners."""
    from dynamics_reference import element_volumes_and_mass
    deck = loaded_bar("tet10", (1, 1, 1))
    _, M = element_volumes_and_mass(deck, np.ones(len(deck.elements)))
    assert M.sum(axis=1).min() <= 1e-15


def test_hub_fan_has_a_row_longer_than_the_tile():
    deck = hub_fan()
    nb = np.zeros(len(deck.nodes), dtype=int)
    adj = [set() for _ in deck.nodes]
    for el in deck.elements:
        for a in el:
            adj[a].update(int(b) for b in el)
    nb = np.array([len(s) for s in adj])
    assert nb[0] > 128 and hrz_lumped_mass(deck, 1.0).min() > 0


@functools.lru_cache(maxsize=None)
def step_case(shape, kind):
    """(dt_G, 2 / omega_max) at the reference state and at a state stretched by 20 % -- computed once."""
    deck = free_block(kind, DIMS) if shape == "free_block" else loaded_bar(kind, DIMS)
    r = ExplicitRestatement(deck, 1.5)
    out = []
    for x in (deck.nodes, deck.nodes * np.array([1.0, 1.2, 1.0])):
        K = r.tangent(x)
        out.append((2.0 / np.sqrt(gershgorin_bound(K, r.ml)), 2.0 / omega_max(K, r.ml)))
    r.close()
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["free_block", "loaded_bar"])
def test_gershgorin_step_is_below_the_dense_limit(shape, kind):
    """A condition, not a measurement: dt_G <= 2 / omega_max.  The printed ratio dt_G omega_max / 2 is the tightness
    DESIGN.md section 13 records."""
    for state, (dt_g, dt_w) in zip(("reference", "stretched 20 %"), step_case(shape, kind)):
        print(shape, kind, state, "dt_G", dt_g, "2/omega_max", dt_w, "tightness", dt_g / dt_w)
        assert 0.0 < dt_g <= dt_w


def test_free_block_keeps_its_linear_momentum():
    deck = free_block("tet4", DIMS)
    r = ExplicitRestatement(deck, 1.5)
    rng = np.random.default_rng(3)
    r.v = 0.05 * rng.standard_normal(r.x.shape)
    p0 = (r.ml[:, None] * r.v).sum(axis=0)
    dt = 0.5 * r.stable_step()
    traj, _ = r.explicit(20, dt)
    p = (r.ml[:, None] * traj[-1][1]).sum(axis=0)
    r.close()
    scale = (r.ml[:, None] * np.abs(traj[-1][1])).sum()
    print("momentum drift", np.abs(p - p0).max() / scale)
    assert np.abs(p - p0).max() <= 1e-13 * scale              # internal forces sum to zero: rounding only


def energy_band(r, n, dt):
    """max - min over the run of E = kinetic energy - work done by the nodal forces (trapezoid per step), scaled by
    the largest kinetic energy."""
    R0 = r.residual(r.x)
    R0[r.mask] = 0.0
    r.a = (R0 / r.ml3).reshape(-1, 3)
    xs, fs, es = [r.x.copy()], [R0], [r.kinetic_energy()]
    work = 0.0
    traj, _ = r.explicit(n, dt)
    ke = [0.0]
    for x, v, a in traj:
        f = r.ml3 * a.ravel()
        work += 0.5 * float((fs[-1] + f) @ (x - xs[-1]).ravel())
        ke.append(0.5 * float((r.ml3 * v.ravel() ** 2).sum()))
        es.append(ke[-1] - work)
        xs.append(x); fs.append(f)
    return (max(es) - min(es)) / max(ke)


# observed on the (2, 4, 2) linear-tetrahedron bar released under its end traction: band(0.5 dt_G) / band(0.25 dt_G)
# = 4.0 (the scheme is second order: the energy oscillates with an amplitude of order dt^2)
BAND_RATIO = 4.0


def test_energy_stays_inside_a_band():
    deck = loaded_bar("tet4", DIMS)
    bands = []
    for frac, n in ((0.25, 400), (0.5, 200)):                 # the same span of time
        r = ExplicitRestatement(deck, 1.5)
        r.lam = 1.0
        bands.append(energy_band(r, n, frac * r.stable_step()))
        r.close()
    print("energy band at 0.25 dt_G", bands[0], "at 0.5 dt_G", bands[1], "ratio", bands[1] / bands[0])
    assert bands[1] <= 2.0 * BAND_RATIO * bands[0]
    assert bands[1] < 0.1                                     # a band, not a drift: a small part of the energy in play


# ---- the deck grammar ---------------------------------------------------------------------------------------------
def explicit_deck(**dyn):
    d = mesh.bar_deck(dims=(2, 3, 2))
    kw = dict(steps=7, dt=0.0, dlambda=0.5, scheme="explicit", safety=0.8, restep=3)
    kw.update(dyn)
    return feahip.Deck(**{k: getattr(d, k) for k in ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements",
                                                     "presc_node", "presc_type", "presc_values")},
                       density=2.5, dynamics=kw)


def test_explicit_deck_round_trip(tmp_path):
    d = explicit_deck()
    p = tmp_path / "exp.sexp"
    d.save(str(p))
    text = p.read_text()
    assert ":dlambda 0.5 :density 2.5 :scheme explicit :safety 0.80000000000000004 :restep 3)" in text
    back = feahip.Deck.load(str(p))
    assert back.dynamics == d.dynamics and back.dynamics["scheme"] == "explicit" and back.dynamics["dt"] == 0.0
    back.save(str(tmp_path / "again.sexp"))
    assert (tmp_path / "again.sexp").read_text() == text
    with pytest.raises(ValueError):
        explicit_deck(scheme="leapfrog")
    with pytest.raises(ValueError):
        feahip.Deck(nodes=d.nodes, elements=d.elements, density=1.0, dynamics=dict(steps=1, dt=0.1, safety=0.5))


def test_other_decks_save_as_before(tmp_path):
    """A Newmark deck carries none of the new attributes, and the golden decks save byte-identically."""
    d = explicit_deck()
    n = feahip.Deck(**{k: getattr(d, k) for k in ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements")},
                    density=2.5, dynamics=dict(steps=7, dt=1e-3))
    p = tmp_path / "newmark.sexp"
    n.save(str(p))
    text = p.read_text()
    assert "scheme" not in text and "safety" not in text and "restep" not in text
    assert "(dynamics :steps 7 :dt 0.001 :beta 0.25 :gamma 0.5 :dlambda 0 :density 2.5)" in text
    import os
    golden = os.path.join(os.path.dirname(__file__), "golden", "dynamics", "plain_bar.sexp")
    back = feahip.Deck.load(golden)
    back.save(str(p))
    with open(golden) as f:
        assert p.read_text() == f.read()


def test_parser_refuses_inconsistent_combinations(tmp_path):
    p = tmp_path / "exp.sexp"
    explicit_deck(dt=1e-3).save(str(p))
    text = p.read_text()

    def refused(old, new, what):
        assert old in text
        q = tmp_path / "bad.sexp"
        q.write_text(text.replace(old, new))
        with pytest.raises(feahip.FeaHipError, match=what):
            feahip.Deck.load(str(q))

    refused(":scheme explicit", ":scheme leapfrog", "scheme must be newmark or explicit")
    refused(" :scheme explicit", "", "safety and :restep need :scheme explicit")
    refused(":scheme explicit", ":scheme newmark", "safety and :restep need :scheme explicit")
    refused(":safety 0.80000000000000004", ":safety 1.5", r"safety must be in \(0, 1\]")
    refused(":safety 0.80000000000000004", ":safety 0", r"safety must be in \(0, 1\]")
    refused(":restep 3", ":restep -1", "restep must be a non-negative integer")
    refused(":dt 0.001", ":dt -0.001", "dt must not be negative")
    refused(":dt 0.001 :beta 0.25 :gamma 0.5 :dlambda 0.5 :density 2.5 :scheme explicit :safety 0.80000000000000004 :restep 3",
            ":dt 0 :beta 0.25 :gamma 0.5 :dlambda 0.5 :density 2.5", "dt must be positive")       # :dt 0 with Newmark
    q = tmp_path / "ok.sexp"                                  # :dt 0 with the explicit scheme loads
    q.write_text(text.replace(":dt 0.001", ":dt 0"))
    assert feahip.Deck.load(str(q)).dynamics["dt"] == 0.0
