"""tests/stress_reference.py against the CPU oracle, without a GPU: the Gauss-point formula of the linearised stress
against extrapolated central differences of the oracle's stresses(), the linear-elastic limit at the reference
configuration, the fixed-weight nodal average against the central difference of the nodal stresses there, and the
rank-one identity of the nine-form von Mises combination; and the :stress key of (spectrum ...) and (random ...) through the
deck reader and writer."""
import functools

import numpy as np
import pytest

import feahip
import mesh
import stress_reference as sr
from dynamics_reference import loaded_bar
from results_reference import ResultsRestatement, smooth_field, von_mises

MODELS = {"neohookean": feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, "a5": feahip.MODEL_A5}
KINDS = ("tet4", "tet10", "hex8")
GAP_STEP = 1e-5


def random_increment(deck, seed=5, size=0.1):
    return size * np.random.default_rng(seed).standard_normal(deck.nodes.size)


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("kind", KINDS)
def test_formula_against_extrapolated_central_differences(kind, model):
    """(1, 3, 1) bars moved by smooth_field(nodes, 0.12), a random du: Richardson extrapolation of the central differences
    with h = 1e-4 and h / 2.  Bound: 1e-9 of the largest |dsigma|; with this du of size 0.1 the six cases give 2.2e-11 to
    6.2e-11, a margin of 16."""
    deck = loaded_bar(kind, (1, 3, 1), model=MODELS[model])
    x = smooth_field(deck.nodes, 0.12)
    du = random_increment(deck)
    s = sr.StressRestatement(deck)
    ds, _, _ = s.gauss_points(x, du[None, :])

    def quotient(h):
        step = h * du.reshape(-1, 3)
        return (s.r.state(x + step)[1] - s.r.state(x - step)[1]) / (2 * h)

    h = 1e-4
    want = (4.0 * quotient(h / 2) - quotient(h)) / 3.0
    err, scale = np.abs(ds[0] - want).max(), np.abs(ds[0]).max()
    print(kind, model, "largest |formula - difference|", err, "largest |dsigma|", scale, "relative", err / scale)
    assert err <= 1e-9 * scale
    s.close()


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("kind", KINDS)
def test_linear_elastic_limit_at_the_reference_configuration(kind, model):
    """x = X0, du = A X: every Gauss point and every node gives lambda tr(eps) I + 2 mu eps, within the restatement's own
    rounding bound."""
    deck = loaded_bar(kind, (1, 3, 1), model=MODELS[model])
    A = np.array([[0.011, -0.004, 0.007], [0.002, -0.013, 0.005], [-0.006, 0.009, 0.003]])
    du = (deck.nodes @ A.T).ravel()
    lam, mu = deck.parameters[:2]
    eps = 0.5 * (A + A.T)
    want = lam * np.trace(eps) * np.eye(3) + 2.0 * mu * eps
    s = sr.StressRestatement(deck)
    ds, da, _ = s.gauss_points(deck.nodes, du[None, :])
    assert np.all(np.abs(ds[0] - want) <= s.bound(da[0]) + s.bound(np.abs(want)))
    T, TA = s.nodal(deck.nodes, du[None, :])
    want6 = np.array([want[i, j] for i, j in sr.SIG6])
    assert np.all(np.abs(T[0] - want6) <= s.bound(TA[0]) + s.bound(np.abs(want6)))
    s.close()


@functools.lru_cache(maxsize=None)
def difference_gap(kind, dims=(1, 3, 1)):
    """(du, the fixed-weight average T[N][6], the largest |central difference of ResultsRestatement.nodal_stresses - T|, the
    bound on it) at x = X0 with the step GAP_STEP, Neo-Hookean: the gap of the difference quotient itself, which the GPU test
    of the library's own nodal_stresses takes as its unit.  The bound: sigma(X0 +- h du) is a difference of numbers of the
    size of the moduli, so its rounding is chain eps (lambda + 2 mu), divided by h in the quotient; the truncation of the
    central difference is h^2 / 6 of a third derivative of the size |grad du|^2 |T| <= |T| for this du."""
    deck = loaded_bar(kind, dims)
    du = random_increment(deck, 9)
    s = sr.StressRestatement(deck)
    T, _ = s.nodal(deck.nodes, du[None, :])
    step = GAP_STEP * du.reshape(-1, 3)
    quot = (s.r.nodal_stresses(deck.nodes + step)[0] - s.r.nodal_stresses(deck.nodes - step)[0]) / (2 * GAP_STEP)
    lam, mu = deck.parameters[:2]
    bound = s.chain() * sr.EPS * (lam + 2 * mu) / GAP_STEP + GAP_STEP ** 2 * np.abs(T).max()
    s.close()
    return du, T[0], float(np.abs(quot - T[0]).max()), float(bound)


@pytest.mark.parametrize("kind", KINDS)
def test_fixed_weight_average_is_the_derivative_of_the_nodal_stresses_at_the_reference_configuration(kind):
    """At x = X0 the stress vanishes, so the variation of the weights drops out: the central difference with h = 1e-5 is
    the fixed-weight average within the bound difference_gap derives (7e-7, below 2e-8 of the largest |T|; the gaps are 1e-10 to
    2e-10 of it)."""
    du, T, gap, bound = difference_gap(kind)
    print(kind, "gap of the central difference", gap, "bound", bound, "largest |T|", np.abs(T).max())
    assert gap <= bound


def test_rank_one_form_is_the_von_mises_stress_of_the_combination():
    """C = a a', b = s = 0: q(y) = (a' y)^2 for every combination, so the nine-form value is von_mises(sum_k a_k T_k)."""
    rng = np.random.default_rng(12)
    m, N = 11, 37
    T, a = rng.standard_normal((m, N, 6)), rng.standard_normal(m)
    v6, b6, vvm, bvm = sr.stress_combine(T, None, np.outer(a, a))
    sig6, vm = sr.field(T, None, a)
    assert np.all(np.abs(v6 - sig6 ** 2) <= b6)
    assert np.all(np.abs(vvm - vm ** 2) <= bvm)
    assert np.all(np.abs(np.sqrt(np.maximum(vvm, 0.0)) - vm) <= 1e-12 * vm.max())


def _deck(**kw):
    d = mesh.bar_deck(dims=(1, 2, 1))
    keys = ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements", "presc_node", "presc_type", "presc_values")
    return feahip.Deck(**{k: getattr(d, k) for k in keys}, density=1.5, dynamics=dict(steps=0, dt=1.0), modal_count=12, **kw)


SPECTRUM = dict(spectrum_points=[(0.5, 1.0), (5.0, 2.0)], spectrum_rule="cqc", spectrum_zeta=0.05, spectrum_base=(1.0, 0.0, 0.0))
RANDOM = dict(random_points=[(0.0, 1.0), (2.0, 2.5), (40.0, 0.0)], random_zeta=0.02)


def test_deck_round_trip_of_the_stress_key(tmp_path):
    """:stress t is read, written and read again in either section; a deck without it is written byte for byte as before;
    any other section, and a spectrum with :rule abs, refuse it."""
    p = tmp_path / "stress.sexp"
    for kw, fields in ((dict(SPECTRUM, spectrum_stress=True), (1, 0)), (dict(RANDOM, random_stress=True), (0, 1)),
                       (dict(SPECTRUM, **RANDOM, spectrum_stress=True, random_stress=True), (1, 1))):
        _deck(**kw).save(str(p))
        text = p.read_text()
        assert text.count(":stress t") == sum(fields)
        back = feahip.Deck.load(str(p))
        fd = back.to_struct()
        assert (fd.spectrum_stress, fd.random_stress) == fields and (back.spectrum_stress, back.random_stress) == tuple(map(bool, fields))
        back.save(str(p))
        assert p.read_text() == text
        plain = {k: v for k, v in kw.items() if not k.endswith("_stress")}
        _deck(**plain).save(str(p))
        assert p.read_text() == text.replace(" :stress t", "") and ":stress" not in p.read_text()
        assert not feahip.Deck.load(str(p)).spectrum_stress and not feahip.Deck.load(str(p)).random_stress
    _deck(**SPECTRUM, **RANDOM, spectrum_stress=True).save(str(p))
    text = p.read_text()
    for old, new in ((":stress t", ":stress maybe"), ("(modal ", "(modal :stress t "), ("(slae-solver ", "(slae-solver :stress t "),
                     (":rule cqc", ":rule abs")):
        bad = text.replace(old, new, 1)
        assert bad != text, old
        p.write_text(bad)
        with pytest.raises(feahip.FeaHipError):
            feahip.Deck.load(str(p))
    p.write_text(text.replace(":stress t", ":stress nil"))
    assert not feahip.Deck.load(str(p)).spectrum_stress
    with pytest.raises(ValueError, match="spectrum_stress"):
        _deck(**dict(SPECTRUM, spectrum_rule="abs"), spectrum_stress=True)
    with pytest.raises(ValueError, match="random_stress"):
        _deck(random_stress=True)
