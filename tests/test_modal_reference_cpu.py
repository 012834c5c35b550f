"""The float64 modal reference (tests/modal_reference.py) checked on its own: M-orthonormal modes, the six zero-energy
modes of a free block, and the Gershgorin number of the explicit scheme as an upper bound of the lumped pencil's
largest eigenvalue."""
import numpy as np
import scipy.linalg

import explicit_reference as er
from dynamics_reference import free_block, loaded_bar
from modal_reference import ModalReference

RHO = 1.5


def test_reference_modes_are_m_orthonormal_and_vanish_on_the_supports():
    deck = loaded_bar("tet4", (2, 4, 2))
    ref = ModalReference(deck, RHO)
    G = ref.Phi.T @ ref.M @ ref.Phi
    assert np.abs(G - np.eye(len(G))).max() < 1e-10
    assert not ref.Phi[ref.mask].any()
    assert np.all(np.diff(ref.lam) >= 0) and ref.lam[0] > 0
    for j in range(6):
        assert ref.residual_ratio(ref.lam[j], ref.Phi[:, j]) < 1e-12


def test_free_block_has_exactly_six_zero_energy_modes():
    ref = ModalReference(free_block("tet4", (2, 2, 2)), RHO)
    assert len(ref.free) == len(ref.mask)
    assert np.count_nonzero(np.abs(ref.lam) < 1e-9 * ref.lam[6]) == 6


def test_gershgorin_number_bounds_the_lumped_pencil():
    deck = loaded_bar("tet4", (2, 4, 2))
    ref = ModalReference(deck, RHO)
    ml = er.hrz_lumped_mass(deck, RHO)
    dt_crit = 2.0 / np.sqrt(er.gershgorin_bound(ref.K_unmasked, ml))
    K = ref.K_unmasked
    lam_max = scipy.linalg.eigh(0.5 * (K + K.T), np.diag(np.repeat(ml, 3)), eigvals_only=True)[-1]
    assert 0 < lam_max <= 4.0 / dt_crit ** 2
