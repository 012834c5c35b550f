"""The locked modal solve on the MI355X (feahip_solve_modes_locked, kernels_modal.hip): more than eight modes on supported
bodies and the zero-energy modes of free ones through a shift, against scipy.linalg.eigh on the oracle's K and the float64
mass (tests/modal_reference.py); the locked store; the two deflation kernels alone against float64; what the solve
leaves of the context's state; reproducibility; the multigrid preconditioner; refusals and running out of steps."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
import mesh
from dynamics_reference import free_block, loaded_bar
from modal_reference import ModalReference

pytestmark = pytest.mark.gpu

RHO, TOL, MAX_IT = 1.5, 1e-8, 2000


def _fan_deck(m=140):
    """tests/test_gpu_modal.py's fan of tetrahedra pairs around one node: a block row of m + 3 = 143 blocks (the long-row
    path of the block product) and 143 nodes, so the last tile of 32 dofs of a block vector is not full."""
    ang = 2 * np.pi * np.arange(m) / m
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(m)], axis=1)
    nodes = np.vstack([[0.0, 0.0, 0.0], ring, [0.0, 0.0, 0.7], [0.0, 0.0, -0.7]])
    top, bot = m + 1, m + 2
    el = []
    for i in range(m):
        a, b = 1 + i, 1 + (i + 1) % m
        el.append([0, a, b, top])
        el.append([0, b, a, bot])
    return feahip.Deck(nodes=nodes, elements=np.array(el, dtype=np.int32), ele_type=feahip.TETRAHEDRA4, gauss_nodes_count=1,
                       presc_node=[top, bot, 1], presc_type=[7, 7, 2], presc_values=np.zeros((3, 3)))


DECKS = {
    "tet4": lambda: loaded_bar("tet4", (3, 8, 3)),
    "hex8": lambda: loaded_bar("hex8", (3, 8, 3)),                        # degenerate bending pairs across the lock boundaries
    "tet10": lambda: loaded_bar("tet10", (2, 4, 2)),
    "free_tet4": lambda: free_block("tet4", (3, 3, 3), parameters=[100, 100]),
    "free_hex8": lambda: free_block("hex8", (3, 4, 5), parameters=[100, 100]),
    "fan": _fan_deck,
    "amg": lambda: mesh.bar_deck(dims=(6, 36, 6)),
}
N_MODES = {"tet4": 24, "hex8": 20, "tet10": 16, "free_tet4": 14, "free_hex8": 14}
CLAMPED, FREE = ("tet4", "hex8", "tet10"), ("free_tet4", "free_hex8")


@functools.lru_cache(maxsize=None)
def reference(kind):
    ref = ModalReference(DECKS[kind](), RHO)
    for a in (ref.lam, ref.Phi, ref.K, ref.M):
        a.setflags(write=False)
    return ref


def two_digits(v):
    return float(f"{v:.1e}")


def shift_of(kind):
    """0 for the supported bodies; for the free ones the reference's seventh eigenvalue (the first elastic one) rounded to
    two digits."""
    return two_digits(reference(kind).lam[6]) if kind in FREE else 0.0


def solver(deck, rho=RHO):
    s = feahip.FeaSolver(deck)
    s.set_mass(rho)
    return s


@functools.lru_cache(maxsize=None)
def solved(kind):
    """One cold locked solve per deck, shared by the tests that read it."""
    s = solver(DECKS[kind]())
    lam, res, steps, sweeps = s.solve_modes_locked(N_MODES[kind], shift_of(kind), TOL, MAX_IT)
    phi = s.locked_modes()
    s.close()
    for a in (lam, res, phi):
        a.setflags(write=False)
    return lam, res, steps, sweeps, phi


def check_eigenvalues(lam, ref_lam, res, shift=0.0, tol=TOL):
    n = len(lam)
    err = np.abs(lam - ref_lam[:n]) / (np.abs(ref_lam[:n]) + shift)
    print("lambda", lam, "err / (|ref| + shift)", err, "resid", res)
    assert np.all(err <= 1e-6)
    assert np.all(res <= tol)
    assert np.all(np.diff(lam) >= 0)


@pytest.mark.parametrize("kind", CLAMPED)
def test_many_modes_of_supported_bodies(kind):
    """|lambda_j - ref_j| <= 1e-6 ref_j, the bound tests/test_gpu_modal.py derives, for 24, 20 and 16 modes: three sweeps
    at least, eigenvalues ascending across the sweeps and none skipped (a skipped one would fail the comparison of every
    later index).  The float64 emulation of the algorithm needed at most 324 steps."""
    lam, res, steps, sweeps, _ = solved(kind)
    print(kind, "steps", steps, "sweeps", sweeps)
    assert lam.shape == (N_MODES[kind],)
    assert 0 < steps <= MAX_IT and sweeps >= 3
    check_eigenvalues(lam, reference(kind).lam, res)


@pytest.mark.parametrize("kind", FREE)
def test_free_bodies_return_their_six_zero_modes(kind):
    """|lambda_j - ref_j| <= 1e-6 (|ref_j| + shift): the first six are zero to 1e-6 of the shift."""
    lam, res, steps, sweeps, _ = solved(kind)
    shift = shift_of(kind)
    print(kind, "shift", shift, "steps", steps, "sweeps", sweeps)
    check_eigenvalues(lam, reference(kind).lam, res, shift)
    assert np.all(np.abs(lam[:6]) <= 1e-6 * shift) and lam[6] > 0.5 * shift


def test_free_body_with_a_shift_a_hundred_times_smaller():
    kind = "free_tet4"
    shift = shift_of(kind) / 100.0
    s = solver(DECKS[kind]())
    lam, res, steps, sweeps = s.solve_modes_locked(N_MODES[kind], shift, TOL, MAX_IT)
    s.close()
    print("shift", shift, "steps", steps, "sweeps", sweeps)
    check_eigenvalues(lam, reference(kind).lam, res, shift)


@pytest.mark.parametrize("kind", CLAMPED + FREE)
def test_locked_modes_are_m_orthonormal_vanish_on_the_supports_and_satisfy_the_reference_pencil(kind):
    """Never vector against vector (degenerate pairs rotate): each mode is an eigenvector of the REFERENCE pencil -- the
    shifted one, (K + shift M, M) at lambda + shift, where a shift was given -- to ten times the tolerance."""
    lam, _, _, _, phi = solved(kind)
    ref, shift = reference(kind), shift_of(kind)
    assert phi.shape == (N_MODES[kind], len(ref.mask))
    G = phi @ ref.M @ phi.T
    print("orthonormality", np.abs(G - np.eye(len(G))).max())
    assert np.abs(G - np.eye(len(G))).max() <= 1e-10
    assert not phi[:, ref.mask].any()
    for j in range(len(phi)):
        if shift == 0.0:
            r = ref.residual_ratio(lam[j], phi[j])
        else:
            Mp = np.where(ref.mask, 0.0, ref.M @ phi[j])
            Kp = ref.K @ phi[j] + shift * Mp
            r = np.linalg.norm(Kp - (lam[j] + shift) * Mp) / (np.linalg.norm(Kp) + abs(lam[j] + shift) * np.linalg.norm(Mp))
        print("mode", j, "reference residual", r)
        assert r <= 10 * TOL


@pytest.mark.parametrize("kind", ["tet4", "fan"])
def test_deflation_kernels_against_float64(kind):
    """out = x - Q (MQ' x) for 1, 8, 9 and 64 locked vectors (one partial panel, a full one, a panel boundary, all eight
    panels); Q random, not orthonormal, zero on the prescribed dofs; one column of x zero.  MQ is the library's own
    spmm_km, so the bound holds these two kernels and not the product.  Per entry, from absolute values in float64:
    (ndof + n_locked + 4) 2^-52 (|x| + |Q| (|MQ|' |x|)) -- the fixed-order bound of an inner product of ndof terms followed
    by one of n_locked terms; it is not measured."""
    deck = DECKS[kind]()
    s = solver(deck)
    s.create_stiffness_and_residual()
    mask = reference(kind).mask
    n = s.ndof
    if kind == "fan":
        assert n % 32 != 0 and s.N % 2 == 1                               # the last tile is not full
    rng = np.random.default_rng(31)
    q_all = rng.normal(size=(64, n))
    q_all[:, mask] = 0.0
    x8 = rng.normal(size=(8, n))
    x8[:, mask] = 0.0
    x8[5] = 0.0
    mq_all = np.vstack([s.spmm_km(q_all[8 * p:8 * p + 8])[1] for p in range(8)])
    for n_locked in (1, 8, 9, 64):
        q, mq = q_all[:n_locked], mq_all[:n_locked]
        out = s.modal_deflate(q, x8)
        want = x8 - (mq @ x8.T).T @ q
        bound = (n + n_locked + 4) * 2.0 ** -52 * (np.abs(x8) + (np.abs(mq) @ np.abs(x8).T).T @ np.abs(q))
        err = np.abs(out - want)
        print(kind, n_locked, "worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound)
        assert not out[5].any()
        assert not out[:, mask].any() and out[:, ~mask].any()
        assert np.array_equal(out, s.modal_deflate(q, x8))
    s.close()


def test_locked_solve_leaves_the_state_of_the_context_alone():
    """The shifted K must not leak: a Newton solve after a locked solve with a shift gives the bits of a context that never
    ran it; mass, nodes and u are untouched; the eight-column block is scratch (modes() is refused) and solve_modes after
    it returns the bits it returns on a fresh context."""
    deck = loaded_bar("tet4", (2, 4, 2), end_motion=0.02)
    probe = np.random.default_rng(5).normal(size=3 * len(deck.nodes))

    def newton(s):
        done, its, tol_log = s.solve(load_increments=2)
        assert done == 2
        return s.nodes(), s.solution(), its, tol_log

    a, b = solver(deck), solver(deck)
    before = (b.nodes(), b.solution(), b.mass_spmv(probe), b.load_factor())
    lam, res, steps, sweeps = b.solve_modes_locked(10, 50.0, TOL, MAX_IT)
    assert steps > 0 and sweeps >= 2 and np.all(res <= TOL)
    after = (b.nodes(), b.solution(), b.mass_spmv(probe), b.load_factor())
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
    with pytest.raises(feahip.FeaHipError, match="no modes held"):
        b.modes()
    six_b = b.solve_modes(6, TOL, 1000) + (b.modes(),)
    six_a = a.solve_modes(6, TOL, 1000) + (a.modes(),)
    for u, v in zip(six_a, six_b):
        assert np.array_equal(u, v)
    b.solve_modes_locked(10, 50.0, TOL, MAX_IT)                            # K + 50 M is in K's store again
    for u, v in zip(newton(a), newton(b)):
        assert np.array_equal(u, v)
    a.close()
    b.close()


def test_two_cold_solves_give_the_same_bits():
    kind = "tet4"
    lam, res, steps, sweeps, phi = solved(kind)
    s = solver(DECKS[kind]())
    for _ in range(2):
        lam_b, res_b, steps_b, sweeps_b = s.solve_modes_locked(N_MODES[kind], 0.0, TOL, MAX_IT)
        assert (steps_b, sweeps_b) == (steps, sweeps)
        assert np.array_equal(lam, lam_b) and np.array_equal(res, res_b) and np.array_equal(phi, s.locked_modes())
    s.close()


@pytest.mark.parametrize("kind", ["tet4", "hex8"])
def test_six_modes_without_a_shift_are_the_bits_of_solve_modes(kind):
    """One sweep of the locked solve with nothing locked and no shift is the base solve: the deflation returns before any
    launch, the stop test is on the same six leading columns, the start block, the iteration and the final Ritz step on
    X are the same, the lock copies the columns verbatim, theta - 0.0 is theta and the stable sort of an ascending list
    is the identity.  Two fresh contexts under block-Jacobi: equal, not close."""
    a, b = solver(DECKS[kind]()), solver(DECKS[kind]())
    lam_l, res_l, steps_l, sweeps = a.solve_modes_locked(6, 0.0, TOL, MAX_IT)
    lam, res, steps = b.solve_modes(6, TOL, MAX_IT)
    phi_l, phi, ndof = a.locked_modes(), b.modes(0, 6), a.ndof
    a.close()
    b.close()
    print(kind, "steps", steps_l, steps, "sweeps", sweeps)
    assert sweeps == 1 and steps_l == steps > 0
    assert np.array_equal(lam_l, lam) and np.array_equal(res_l, res)
    assert phi_l.shape == phi.shape == (6, ndof) and np.array_equal(phi_l, phi)


def test_multigrid_preconditioner():
    """Preconditioner 1 (one W-cycle per column and step, the deflation after the cycles): twelve modes without a shift and
    with one of the order of the first eigenvalue, the criterion of the supported bodies.  The steps are printed."""
    ref = reference("amg")
    s = solver(DECKS["amg"]())
    s.set_preconditioner(1)
    for shift in (0.0, two_digits(ref.lam[0])):
        lam, res, steps, sweeps = s.solve_modes_locked(12, shift, TOL, MAX_IT)
        print("multigrid: shift", shift, "steps", steps, "sweeps", sweeps)
        check_eigenvalues(lam, ref.lam, res)
    s.close()


def _refused(s, code, fn):
    with pytest.raises(feahip.FeaHipError) as e:
        fn()
    prefix = f"libfeahip error {code}: "
    msg = str(e.value)
    assert msg.startswith(prefix) and len(msg) > len(prefix) + 5, msg
    return msg


def test_refusals():
    deck = DECKS["tet4"]()
    s = feahip.FeaSolver(deck)
    s.create_stiffness_and_residual()
    assert "no mass" in _refused(s, feahip.ESTATE, lambda: s.solve_modes_locked(12))
    for what in (16, 17):
        assert "no mass" in _refused(s, feahip.EINVAL, lambda: s.time_kernel(what, 1, 1))
    s.set_mass(RHO)
    for what in (16, 17):
        assert s.time_kernel(what, 1, 2) > 0
    assert "no locked modes" in _refused(s, feahip.ESTATE, lambda: s.locked_modes())
    assert "no locked modes" in _refused(s, feahip.ESTATE, lambda: s.locked_count())
    for bad in (0, 65):
        assert "n_modes" in _refused(s, feahip.EINVAL, lambda: s.solve_modes_locked(bad))
    for bad in (-1.0, float("nan"), float("inf")):
        assert "shift" in _refused(s, feahip.EINVAL, lambda: s.solve_modes_locked(12, bad))
    assert "tolerance" in _refused(s, feahip.EINVAL, lambda: s.solve_modes_locked(12, tolerance=0.0))
    assert "max_iterations" in _refused(s, feahip.EINVAL, lambda: s.solve_modes_locked(12, max_iterations=-1))
    assert s._lib.feahip_solve_modes_locked(s._ctx, 12, 0.0, 1e-8, 10, None, None, None, None) == feahip.EINVAL
    assert b"null lambda" in s._lib.feahip_last_error(s._ctx)
    assert "n_locked" in _refused(s, feahip.EINVAL, lambda: s.modal_deflate(np.zeros((0, s.ndof)), np.zeros((8, s.ndof))))
    lam, _, _, _ = s.solve_modes_locked(2, 0.0, 1e-6, 500)
    assert s.locked_count() == 2 and s.locked_modes(1, 1).shape == (1, s.ndof)
    for first, count in ((1, 2), (-1, 1), (0, 3)):
        assert "outside" in _refused(s, feahip.EINVAL, lambda: s.locked_modes(first, count))
    s.set_row_shard(0, 2)
    assert "row-sharded" in _refused(s, feahip.EINVAL, lambda: s.solve_modes_locked(12))
    s.close()
    # fewer than n_modes + 24 free dofs: 2 x 2 x 2 cells clamped on one face have 54
    s = solver(loaded_bar("tet4", (2, 2, 2)))
    assert "free dofs" in _refused(s, feahip.EINVAL, lambda: s.solve_modes_locked(31))
    s.close()
    # a member of a group, a rank context, the coarse level across the ranks
    g = feahip.FeaGroup(deck, 2)
    g.set_mass(RHO)
    m = g.ranks[0]
    assert "transport" in _refused(m, feahip.EINVAL, lambda: m.solve_modes_locked(12))
    g.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.solve_modes_locked(12))
    r.close()
    s = solver(DECKS["amg"]())
    s.set_preconditioner(2)
    assert "preconditioner 2" in _refused(s, feahip.EINVAL, lambda: s.solve_modes_locked(12))
    s.close()


def test_running_out_of_steps_leaves_the_locked_pairs_readable():
    s = solver(DECKS["tet4"]())
    with pytest.raises(feahip.FeaHipError, match=f"error {feahip.ENOTCONVERGED}"):
        s.solve_modes_locked(24, 0.0, TOL, 3)
    assert s.locked_count() == 0 and s.locked_modes().shape == (0, s.ndof)
    cap = 3 * solved("tet4")[2] // 4                                       # three quarters of the steps the whole solve takes
    lam, res, steps, sweeps, rc = s.solve_modes_locked(24, 0.0, TOL, cap, check=False)
    n = s.locked_count()
    print("cap", cap, "locked", n, "sweeps", sweeps)
    assert rc == feahip.ENOTCONVERGED and steps == cap and 0 < n < 24      # (the first of its sweeps has ended by then)
    assert np.all(np.isfinite(lam[:n])) and np.all(np.diff(lam[:n]) >= 0) and lam[0] > 0
    assert np.all(res[:n] <= TOL) and np.all(np.isnan(lam[n:])) and np.all(np.isnan(res[n:]))
    assert np.array_equal(lam[:n], solved("tet4")[0][:n])                  # the same sweeps as the whole solve, cut short
    phi = s.locked_modes()
    assert phi.shape == (n, s.ndof) and np.all(np.isfinite(phi))
    s.close()


def test_feasolver_hip_runs_the_locked_solve_for_a_deck_with_count(tmp_path):
    """(modal :count 12 :shift s): the log holds one line per mode with the eigenvalues of solve_modes_locked at the state
    reached, the .msh file one "Mode k" section per mode -- twelve, not eight."""
    deck = loaded_bar("tet4", (3, 8, 3), end_motion=0.01, density=RHO, modal_count=12, modal_shift=5.0, load_increments_count=1)
    path = tmp_path / "locked.sexp"
    deck.save(str(path))
    s = feahip.FeaSolver(feahip.Deck.load(str(path)))
    done, _, _ = s.solve()
    assert done == 1
    lam, res, steps, _ = s.solve_modes_locked(12, 5.0, deck.modal_tolerance, deck.modal_max)
    s.close()
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert re.search(r"^Modal analysis finished: 12 modes, \d+ steps$", out.stdout, re.M), out.stdout
    got = [float(v) for v in re.findall(r"^Mode \d+: omega\^2 = (\S+),", out.stdout, re.M)]
    # (the executable reaches its state by the host's Newton loop, this test by feahip_solve: equal to their tolerance)
    assert len(got) == 12 and np.all(np.abs(np.array(got) - lam) <= 1e-9 * (np.abs(lam) + 5.0))
    text = (tmp_path / "locked.msh").read_text()
    assert [int(k) for k in re.findall(r'^"Mode (\d+)"$', text, re.M)] == list(range(1, 13))
