"""Modal analysis, the parts that need no GPU: the (modal ...) section of the deck reader / writer, the struct the
Python side shares with the C side, and the host half of feahip_solve_modes -- the Rayleigh-Ritz step
(feahip_host_modal_ritz) driving a dense numpy LOBPCG to the eigenvalues of scipy.linalg.eigh."""
import os
import re

import numpy as np
import pytest
import scipy.linalg

import feahip
from dynamics_reference import loaded_bar
from modal_reference import ModalReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _deck(**kw):
    d = loaded_bar("tet4", (1, 2, 1), end_motion=0.01)
    return feahip.Deck(nodes=d.nodes, elements=d.elements, ele_type=d.ele_type, gauss_nodes_count=d.gauss_nodes_count,
                       presc_node=d.presc_node, presc_type=d.presc_type, presc_values=d.presc_values, **kw)


def test_modal_section_round_trip(tmp_path):
    deck = _deck(density=1.5, modal_modes=5, modal_tolerance=2.5e-9, modal_max=321)
    path = str(tmp_path / "modal.sexp")
    deck.save(path)
    text = open(path).read()
    assert re.search(r"\(modal :modes 5 :tolerance 2\.5\d*e-09 :max 321\)", text), text
    back = feahip.Deck.load(path)
    assert (back.modal_modes, back.modal_tolerance, back.modal_max) == (5, 2.5e-9, 321)
    assert back.density == 1.5 and back.dynamics["steps"] == 0
    back.save(str(tmp_path / "again.sexp"))
    assert open(str(tmp_path / "again.sexp")).read() == text


def test_modal_section_defaults(tmp_path):
    path = str(tmp_path / "m.sexp")
    _deck(density=1.5, modal_modes=2).save(path)
    text = re.sub(r"\(modal [^)]*\)", "(modal :modes 3)", open(path).read())
    open(path, "w").write(text)
    back = feahip.Deck.load(path)
    assert (back.modal_modes, back.modal_tolerance, back.modal_max) == (3, 1e-8, 1000)


def test_modal_section_is_absent_without_modes(tmp_path):
    path = str(tmp_path / "plain.sexp")
    _deck(density=1.5).save(path)
    assert "(modal" not in open(path).read()
    assert feahip.Deck.load(path).modal_modes == 0
    _deck().save(path)
    assert "(modal" not in open(path).read()


def test_modal_section_without_a_density_is_refused(tmp_path):
    with pytest.raises(ValueError, match="density"):
        _deck(modal_modes=4)
    path = str(tmp_path / "m.sexp")
    _deck(density=1.5, modal_modes=4).save(path)
    text = re.sub(r"\n\s*\(dynamics [^)]*\)", "", open(path).read())
    assert "(dynamics" not in text and "(modal" in text
    open(path, "w").write(text)
    with pytest.raises(feahip.FeaHipError, match=r"\(modal \.\.\.\) but no density"):
        feahip.Deck.load(path)
    for bad in ("(modal :modes 9)", "(modal :modes 2 :tolerance 0)", "(modal :modes 2 :max -1)", "(modal :tolerance 1e-8)"):
        open(path, "w").write(re.sub(r"\(modal [^)]*\)", bad, text))
        with pytest.raises(feahip.FeaHipError):
            feahip.Deck.load(path)


def test_deck_struct_matches_the_c_side():
    """The fields of struct fea_deck in host/fea_host.h, in order, are the fields of feahip.FeaDeck; the modal ones are
    the last, and a deck travels through the C reader and writer with every field (a size mismatch would cut them)."""
    hdr = open(os.path.join(ROOT, "fea-large_amd", "host", "fea_host.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct fea_deck {"):hdr.index("} fea_deck;")], flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.replace("typedef struct fea_deck {", "").strip()
        if stmt:
            names += [re.sub(r"\[.*\]", "", n).strip(" *") for n in re.sub(r"^\s*(int|double)\s", "", stmt).split(",")]
    assert names == [n for n, _ in feahip.FeaDeck._fields_]
    assert names[-3:] == ["modal_modes", "modal_tolerance", "modal_max"]


def _lobpcg_with_the_librarys_ritz_step(K, M, mask, n_modes, tol=1e-8, max_it=400):
    """The iteration of feahip_solve_modes in dense numpy: block-Jacobi preconditioner, S = [X, W, P], the products of X
    and P kept by recurrence -- and every Rayleigh-Ritz step made by the library's own host code."""
    n, free = len(K), (~mask).astype(np.float64)
    Mm = M * free[:, None]
    minv = np.zeros_like(K)
    for a in range(n // 3):
        s = slice(3 * a, 3 * a + 3)
        minv[s, s] = np.linalg.inv(K[s, s])
    X = np.random.default_rng(1).uniform(-1, 1, size=(n, 8)) * free[:, None]
    KX, MX = K @ X, Mm @ X
    rank, th, C = feahip.host_modal_ritz(X.T @ MX, X.T @ KX)
    assert rank == 8
    X, KX, MX = X @ C[:, :8], KX @ C[:, :8], MX @ C[:, :8]
    P = KP = MP = None
    for it in range(max_it + 1):
        R = KX - MX * th
        res = np.linalg.norm(R, axis=0) / (np.linalg.norm(KX, axis=0) + np.abs(th) * np.linalg.norm(MX, axis=0))
        if np.all(res[:n_modes] <= tol):
            return th, X, it
        W = (minv @ R) * free[:, None]
        S, KS, MS = [X, W], [KX, K @ W], [MX, Mm @ W]
        if P is not None:
            S, KS, MS = S + [P], KS + [KP], MS + [MP]
        S, KS, MS = np.hstack(S), np.hstack(KS), np.hstack(MS)
        rank, th, C = feahip.host_modal_ritz(S.T @ MS, S.T @ KS)
        assert rank >= 8
        assert not C[:8, 8:].any()                         # P_new lies in [W, P]
        X, KX, MX = S @ C[:, :8], KS @ C[:, :8], MS @ C[:, :8]
        P, KP, MP = (S @ C[:, 8:], KS @ C[:, 8:], MS @ C[:, 8:]) if rank == S.shape[1] else (None, None, None)
        if it % 20 == 19:
            KX, MX = K @ X, Mm @ X
    raise AssertionError(f"not converged: {res}")


@pytest.mark.parametrize("n_modes", [1, 6, 8])
def test_ritz_step_drives_a_dense_lobpcg_to_the_eigenvalues(n_modes):
    ref = ModalReference(loaded_bar("tet4", (2, 4, 2)), 1.5)
    th, X, it = _lobpcg_with_the_librarys_ritz_step(ref.K, ref.M, ref.mask, n_modes)
    assert np.all(np.abs(th[:n_modes] - ref.lam[:n_modes]) <= 1e-6 * ref.lam[:n_modes])
    assert np.all(np.diff(th) >= 0)
    assert np.abs(X.T @ ref.M @ X - np.eye(8)).max() < 1e-10
    assert not X[ref.mask].any()


def test_ritz_step_drops_dependent_directions_and_refuses_garbage():
    rng = np.random.default_rng(3)
    B = rng.normal(size=(40, 16))
    B[:, 12:] = B[:, 8:12]                                  # four directions twice
    Kd = np.diag(np.arange(1.0, 41.0))
    rank, th, C = feahip.host_modal_ritz(B.T @ B, B.T @ Kd @ B)
    assert rank == 12
    Xn = B @ C[:, :8]
    assert np.abs(Xn.T @ Xn - np.eye(8)).max() < 1e-8
    ref = scipy.linalg.eigh(B[:, :12].T @ Kd @ B[:, :12], B[:, :12].T @ B[:, :12], eigvals_only=True)[:8]
    assert np.allclose(th, ref, rtol=1e-8)
    G = B.T @ B
    G[0, 0] = np.nan
    assert feahip.host_modal_ritz(G, B.T @ Kd @ B)[0] == -1
    Z = np.zeros((16, 16))
    Z[:4, :4] = np.eye(4)
    assert feahip.host_modal_ritz(Z, Z)[0] == -1            # fewer than eight directions left
