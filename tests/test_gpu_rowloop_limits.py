"""The block-row product kernels at the limits of their tile, on the MI355X, against long-double references.

tests/rowloop_cases.py names the meshes (LIMITS) and tests/test_rowloop_cases_host.py proves on the CPU which chunk shapes
they reach: a full tile of 128 blocks at either parity of its first block, with one, several and sixteen rows, the
smallest long rows (129, 130 blocks), 64 and 65 blocks (the k + 64 half empty, or lane 0 alone), a one-block chunk, the
577th staged 16-byte piece -- also at the end of the matrix, where its upper half is the array's padding -- and the row
shard that starts at an odd block.  Here every product that runs the shared row loop is called on each of them at a
smoothly deformed state with rho = 2.5.

Bounds.  Per row, never per vector: |y_i - ref_i| <= gamma(n + 1) s_i with gamma(k) = k u / (1 - k u), u = 2^-53, n the
roundings behind the row and s_i the row's expression with every operand replaced by its absolute value, in long double.
It holds for any summation order, with or without fused multiply-adds.  The counts n:
  K x (spmv, spmv2, the K half of spmm_km), K as stored (feahip_get_matrix_yale, exact doubles): the row's 3 nb scalar
    terms;
  m x with m the device's own entries (column b is feahip_mass_spmv of a unit vector: one term and zeros, exact): the
    row's nb terms -- this holds the row loop alone;
  m x against the long-double mass restated from the deck and the element tables: rowloop_cases.mass_row_roundings, i.e.
    nb, the product, the entry's own sum ((Gm + 1) E_ab for the E_ab elements that hold the pair, the longest of the row)
    and the 14 roundings behind one term rho w det J0 N_a N_b; s_i takes det J0 with absolute values as well;
  C v = alpha m v + beta K_d v: 4 nb terms (3 of K_d, 1 of m per block), the two coefficients and their sum (3), on the
    device's own m; against the long-double mass, the mass count and 3 nb + 3;
  kg x on the device's own kg (unit vectors again): nb.  An entry of kg comes out of two 3 x 3 inversions and a logarithm
    per element: its expression in absolute values is 1e10 to 1e17 times the entry on these wedge-shaped elements, so no
    count gives a useful bound against the oracle; every entry is held to the oracle's under the bound that
    tests/test_gpu_buckling.py gives a unit vector, 1e-12 |Ksig_ab| + 1e-12 max |Ksig|, and the product of any vector to
    the oracle's under the sum of that bound over the row's blocks, times |x_b|, and the row loop's own.
  ml (k_mass_lump) and the stable step: see test_lumped_mass_and_stable_step.
The worst ratio of error to bound is printed per kernel.  The 57 cases of this file and the 39 of
tests/test_gpu_multigrid.py run in 8.5 s together on an MI355X."""
import copy
import functools

import numpy as np
import pytest

import buckling_reference as br
import feahip
import rowloop_cases as rc
from damping_reference import DampedDynamics
from explicit_reference import gershgorin_bound, hrz_lumped_mass
from rowloop_cases import LD, RHO, U, gamma
from test_gpu_damping import PAIRS
from test_gpu_dynamics import U_TOL, check_state

pytestmark = pytest.mark.gpu

SHARD = "fan126_rank1_of_2"
NAMES = list(rc.LIMITS)
WHOLE = [n for n in NAMES if n != SHARD]                      # spmv2 and geometric_spmv refuse a row shard
WORST = {}


def held(kernel, got, ref, bound, rows=None):
    """|got - ref| <= bound on the rows given (a zero bound asks for the exact value); keeps the worst ratio per kernel."""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    if rows is not None:
        err, bound = err[..., rows], bound[..., rows]
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    assert worst <= 1.0, (kernel, worst, int(np.argmax(ratio)))
    return worst


@functools.lru_cache(maxsize=None)
def case(name):
    """(deck, state, blocks per row, long-double mass, its absolute version, roundings of a mass row): computed once,
    shared, never written to."""
    deck = rc.LIMITS[name][0]()
    x = rc.limit_state(deck)
    nb, _ = rc.block_rows(deck)
    m, mabs = rc.mass_long_double(deck, RHO)
    for a in (x, nb, m, mabs):
        a.setflags(write=False)
    return deck, x, nb, m, mabs, rc.mass_row_roundings(deck)


def context(name, deck=None):
    """(solver at the deformed state with K assembled and the mass set, dofs to check): the whole mesh, or rank 1 of 2"""
    deck0, x = case(name)[:2]
    s = feahip.FeaSolver(deck0 if deck is None else deck)
    if name == SHARD:
        s.set_row_shard(1, 2)
    s.set_nodes(x)
    s.create_stiffness_and_residual()
    s.set_mass(RHO)
    own = s.owned_nodes() if name == SHARD else np.arange(s.N)
    if name == SHARD:
        assert own[0] == 113 and len(own) == 16                # chunks (14, 801, 84), (1, 885, 128), (1, 1013, 128)
    return s, (3 * np.asarray(own)[:, None] + np.arange(3)[None, :]).ravel()


def stored(s):
    """K as stored, dense in long double (exact), and the scalar terms of every row"""
    off, idx, val = s.matrix_yale()
    A = np.zeros((s.ndof, s.ndof), dtype=LD)
    A[np.repeat(np.arange(s.ndof), np.diff(off)), idx] = val
    return A, np.diff(off)


def vectors(n, seed, count=3):
    """ones, a normal vector, a normal vector scaled by 10^uniform(-6, 6) per dof, then more of the last two kinds"""
    rng = np.random.default_rng(seed)
    out = [np.ones(n)]
    while len(out) < count:
        out.append(rng.standard_normal(n))
        out.append(rng.standard_normal(n) * 10.0 ** rng.uniform(-6.0, 6.0, n))
    return out[:count]


def own_mass(s, dofs):
    """The device's own scalar mass [N][N] on the rows to check: column b is feahip_mass_spmv of a unit vector."""
    m = np.zeros((s.N, s.N), dtype=LD)
    for b in range(s.N):
        e = np.zeros(s.ndof)
        e[3 * b] = 1.0
        y = s.mass_spmv(e)
        assert not y[1::3].any() and not y[2::3].any()
        m[:, b] = y[0::3]
    return m


def product_bound(A, n, x):
    """(A x, gamma(n + 1) |A| |x|) in long double"""
    x = np.asarray(x, dtype=LD)
    return A @ x, gamma(np.asarray(n) + 1) * (np.abs(A) @ np.abs(x))


@pytest.mark.parametrize("name", NAMES)
def test_spmv_and_spmv2(name):
    _, _, nb = case(name)[:3]
    s, dofs = context(name)
    A, nterms = stored(s)
    assert np.array_equal(nterms[dofs], 3 * np.repeat(nb, 3)[dofs])
    xs = vectors(s.ndof, 41)
    refs = [product_bound(A, nterms, x) for x in xs]
    for x, (ref, bound) in zip(xs, refs):
        y = s.spmv(x)
        held("spmv", y, ref, bound, dofs)
        assert np.array_equal(s.spmv(x), y)                                # twice: the same bits
    if name != SHARD:
        for a, b in ((0, 1), (1, 2), (2, 0)):                              # two different columns
            y2 = s.spmv2(np.stack([xs[a], xs[b]]))
            held("spmv2", y2[0], *refs[a])
            held("spmv2", y2[1], *refs[b])
            assert np.array_equal(s.spmv2(np.stack([xs[a], xs[b]])), y2)
    print(name, "worst error / bound", {k: WORST[k] for k in ("spmv", "spmv2") if k in WORST})
    s.close()


@pytest.mark.parametrize("name", NAMES)
def test_mass_spmv(name):
    deck, _, nb, m, mabs, n_mass = case(name)
    s, dofs = context(name)
    nodes = dofs[0::3] // 3
    md = own_mass(s, dofs)
    # the entries: one term of the mass rule, the entry's own sum over points and elements
    _, pairs = rc.block_rows(deck)
    n_entry = rc.mass_entry_roundings(deck) + (len(rc.mass_rule(deck)[0]) + 1) * pairs
    held("k_mass_blocks", md[nodes], m[nodes], gamma(n_entry + 1)[nodes] * mabs[nodes])
    assert not md[nodes][pairs[nodes] == 0].any()
    M, Mabs, Md = rc.scalar_blocks(m), rc.scalar_blocks(mabs), rc.scalar_blocks(md)
    for x in vectors(s.ndof, 43):
        y = s.mass_spmv(x)
        xl = np.asarray(x, dtype=LD)
        held("k_mass_product (row loop)", y, *product_bound(Md, np.repeat(nb, 3), x), dofs)
        held("k_mass_product", y, M @ xl, gamma(np.repeat(n_mass, 3) + 1) * (Mabs @ np.abs(xl)), dofs)
        assert np.array_equal(s.mass_spmv(x), y)
    print(name, "worst error / bound", {k: v for k, v in WORST.items() if k.startswith("k_mass")})
    s.close()


@pytest.mark.parametrize("name", NAMES)
def test_damping_spmv(name):
    _, _, nb, m, mabs, n_mass = case(name)
    s, dofs = context(name)
    md = rc.scalar_blocks(own_mass(s, dofs))
    M, Mabs = rc.scalar_blocks(m), rc.scalar_blocks(mabs)
    nb3 = np.repeat(nb, 3)
    vs = vectors(s.ndof, 47)
    for alpha, beta in PAIRS:
        s.set_damping(alpha, beta)                                         # the snapshot at the deformed state ...
        Kd, nterms = stored(s)                                             # ... is the K it leaves behind, bit for bit
        assert np.array_equal(nterms[dofs], 3 * nb3[dofs])
        a, b = LD(alpha), LD(beta)
        for v in vs:
            vl = np.asarray(v, dtype=LD)
            y = s.damping_spmv(v)
            held("k_damp_product (row loop)", y, (a * md + b * Kd) @ vl,
                 gamma(4 * nb3 + 3 + 1) * ((a * np.abs(md) + b * np.abs(Kd)) @ np.abs(vl)), dofs)
            held("k_damp_product", y, a * (M @ vl) + b * (Kd @ vl),
                 gamma(3 * nb3 + 3 + np.repeat(n_mass, 3) + 1) * ((a * Mabs + b * np.abs(Kd)) @ np.abs(vl)), dofs)
            assert np.array_equal(s.damping_spmv(v), y)
    print(name, "worst error / bound", {k: v for k, v in WORST.items() if k.startswith("k_damp")})
    s.close()


def with_mask(deck):
    """The deck with prescribed dofs in the hub row (x and z) and in two ring rows (y; x and y) besides its own."""
    hub = int(np.bincount(np.asarray(deck.elements).ravel()).argmax())
    ring = sorted(set(int(a) for e in deck.elements if hub in e for a in e) - set([hub]) - set(int(a) for a in deck.presc_node))[:2]
    assert len(ring) == 2
    d = copy.copy(deck)
    d.presc_node = np.concatenate([deck.presc_node, [hub] + ring]).astype(np.int32)
    d.presc_type = np.concatenate([deck.presc_type, [5, 2, 3]]).astype(np.int32)
    d.presc_values = np.vstack([deck.presc_values, np.zeros((3, 3))])
    return d, hub, ring


def dof_mask(deck):
    mask = np.zeros(3 * len(deck.nodes), dtype=bool)
    for nd, ty in zip(deck.presc_node, deck.presc_type):
        for j in range(3):
            mask[3 * nd + j] |= bool(ty & (1 << j))
    return mask


def check_spmm(tag, y8, z8, x8, A, nterms, M, Mabs, n_mass3, mask, dofs):
    for c in range(8):
        xl = np.asarray(x8[c], dtype=LD)
        held("k_spmm_km K", y8[c], *product_bound(A, nterms, x8[c]), dofs)
        held("k_spmm_km M", z8[c], np.where(mask, 0, M @ xl), gamma(n_mass3 + 1) * np.where(mask, 0, Mabs @ np.abs(xl)), dofs)
    assert not z8[:, mask].any()


@pytest.mark.parametrize("name", NAMES)
def test_spmm_km(name):
    """Eight different columns; Y = K X and Z = mask(M X) column by column, against the long-double mass.  The sharded entry
    runs as FeaGroup(fan_deck(126), 2).spmm_km and is checked on the rows each rank owns, in each rank's own result."""
    deck0, x, nb, m, mabs, n_mass = case(name)
    deck, hub, ring = with_mask(deck0)
    mask = dof_mask(deck)
    assert mask[3 * hub] and not mask[3 * hub + 1] and mask[3 * ring[0] + 1] and mask[3 * ring[1]]
    M, Mabs, n_mass3 = rc.scalar_blocks(m), rc.scalar_blocks(mabs), np.repeat(n_mass, 3)
    x8 = np.stack(vectors(3 * len(deck.nodes), 53, 8))
    if name != SHARD:
        s, dofs = context(name, deck)
        A, nterms = stored(s)
        y8, z8 = s.spmm_km(x8)
        check_spmm(name, y8, z8, x8, A, nterms, M, Mabs, n_mass3, mask, dofs)
        y8b, z8b = s.spmm_km(x8)
        assert np.array_equal(y8, y8b) and np.array_equal(z8, z8b)
        s.close()
    else:
        g = feahip.FeaGroup(deck, 2)
        g.each("set_nodes", x)
        g.each("create_stiffness_and_residual")
        g.set_mass(RHO)
        y8, z8, ys, zs = g.spmm_km(x8, per_rank=True)
        assert [len(nd) for nd in g.nodes] == [113, 16]
        for rk, nd, yr, zr in zip(g.ranks, g.nodes, ys, zs):
            A, nterms = stored(rk)                                          # the rank's own rows of K, zero elsewhere
            dofs = (3 * np.asarray(nd)[:, None] + np.arange(3)[None, :]).ravel()
            check_spmm(name, yr, zr, x8, A, nterms, M, Mabs, n_mass3, mask, dofs)
            assert np.array_equal(yr[:, dofs], y8[:, dofs]) and np.array_equal(zr[:, dofs], z8[:, dofs])
        y8b, z8b = g.spmm_km(x8)
        assert np.array_equal(y8, y8b) and np.array_equal(z8, z8b)
        g.close()
    print(name, "worst error / bound", {k: v for k, v in WORST.items() if k.startswith("k_spmm")})


@functools.lru_cache(maxsize=None)
def oracle_geometric(name):
    deck, x = case(name)[:2]
    Ks = br.dense_pair(deck, x)[1]
    Ks.setflags(write=False)
    return Ks


@pytest.mark.parametrize("name", WHOLE)
def test_geometric_spmv(name):
    deck, x, nb = case(name)[:3]
    Ks = oracle_geometric(name)
    s = feahip.FeaSolver(deck)
    s.set_nodes(x)
    kg = np.zeros((s.N, s.N), dtype=LD)                                    # the device's own entries: exact
    for b in range(s.N):
        e = np.zeros(s.ndof)
        e[3 * b + 1] = 1.0
        y = s.geometric_spmv(e)
        assert not y[0::3].any() and not y[2::3].any()
        kg[:, b] = y[1::3]
    absolute = 1e-12 * np.abs(Ks).max()
    ks = np.asarray(Ks[0::3, 0::3], dtype=LD)
    assert not Ks[0::3, 1::3].any()                                        # a scalar per block, in the oracle as well
    entry = np.where(rc.block_rows(deck)[1] > 0, 1e-12 * np.abs(ks) + absolute, 0)   # that bound for a unit vector, per block
    held("k_geom_blocks", kg, ks, entry)
    Kg, KsL, entry3 = rc.scalar_blocks(kg), np.asarray(Ks, dtype=LD), rc.scalar_blocks(entry)
    for v in vectors(s.ndof, 59):
        vl = np.asarray(v, dtype=LD)
        y = s.geometric_spmv(v)
        ref, loop = product_bound(Kg, np.repeat(nb, 3), v)
        held("kg product (row loop)", y, ref, loop)
        held("kg product (oracle)", y, KsL @ vl, entry3 @ np.abs(vl) + loop)       # what the two bounds above add up to
        assert np.array_equal(s.geometric_spmv(v), y)
    print(name, "worst error / bound", {k: v for k, v in WORST.items() if k.startswith("k") and "g" in k[:3]})
    s.close()


@pytest.mark.parametrize("name", NAMES)
def test_lumped_mass_and_stable_step(name):
    """ml against explicit_reference.hrz_lumped_mass, relative per node: ml_a is a sum of positive terms m_e d_a / sum d_b
    whose three factors each carry rho w det J0 and a sum over the mass points -- rowloop_cases.lumped_roundings counts n
    and kappa = max perm |J0| / det J0, the one place where signs mix -- so kappa gamma(n + 1) for the device and as much
    again for the float64 reference.  The stable step 2 / sqrt(max_i sum_j |K_ij| / ml_i) against gershgorin_bound on
    the K that the call leaves behind (exact doubles) and the reference ml: a row of 3 nb positive terms on either side
    (2 gamma(3 nb + 1)), ml's bound, the quotient (2 u); the square root halves the sum, and root and quotient add 2 u
    on either side.  A mesh with an isolated node has a row 0 / 0: the restatement's bound is NaN, and the library
    refuses a bound that is not positive and finite.  The sharded entry runs as the group of two."""
    deck, x, nb = case(name)[:3]
    want = hrz_lumped_mass(deck, RHO)
    n_ml, kappa = rc.lumped_roundings(deck)
    ml_tol = 2 * kappa * gamma(n_ml + 1)
    isolated = want == 0
    assert int(isolated.sum()) == {"hub66_iso_hub_pole_ring": 1, "hub22_iso_hub_ring_pole": 1, "hub29_hub_ring_pole_iso2": 2}.get(name, 0)
    s = feahip.FeaGroup(deck, 2) if name == SHARD else feahip.FeaSolver(deck)
    one = s.ranks[0] if name == SHARD else s
    for rk in (s.ranks if name == SHARD else [s]):
        rk.set_nodes(x)
    s.set_mass(RHO)
    ml = s.lumped_mass()
    held("k_mass_lump", ml, np.asarray(want, dtype=LD), ml_tol * want)
    assert np.array_equal(s.lumped_mass(), ml)
    if isolated.any():
        one.create_stiffness_and_residual()
        with np.errstate(invalid="ignore"):
            assert np.isnan(gershgorin_bound(np.asarray(stored(one)[0], dtype=np.float64), want))
        with pytest.raises(feahip.FeaHipError, match="no positive finite row sum") as e:
            s.stable_step()
        assert f"error {feahip.ESTATE}:" in str(e.value)
    else:
        dt = s.stable_step()
        if name == SHARD:
            K = sum(stored(rk)[0] for rk in s.ranks)
        else:
            K = stored(one)[0]
        dt_ref = 2.0 / np.sqrt(gershgorin_bound(np.asarray(K, dtype=np.float64), want))
        tol = 0.5 * (2 * gamma(3 * nb.max() + 1) + ml_tol.max() + 2 * U) + 4 * U
        held("k_gershgorin", np.array([dt]), np.array([dt_ref], dtype=LD), np.array([tol * dt_ref]))
        assert s.stable_step() == dt
    print(name, "worst error / bound", {k: WORST[k] for k in ("k_mass_lump", "k_gershgorin") if k in WORST}, "kappa", kappa)
    s.close()


def solve_live(K, R):
    """The dense solve of the restatement on the dofs that have a row: an isolated node has none in K + a0 M (and no
    residual), and the conjugate gradients leave its increment at zero."""
    live = np.abs(K).sum(axis=1) > 0
    assert not R[~live].any()
    u = np.zeros_like(R)
    u[live] = np.linalg.solve(K[np.ix_(live, live)], R[live])
    return u


STEP_DT, NEWTON_TOL, MAX_NEWTON = 0.05, 1e-18, 30


@functools.lru_cache(maxsize=None)
def one_step(name, damped):
    """(initial velocities, Newton count, state after one Newmark step) of the restatement from the deck's own nodes.  The
    energies |<u, R>| of its four iterations fall 1e1, 5e-4, 1e-11, 1e-24: NEWTON_TOL is a factor 1e6 from either
    neighbour on both meshes, damped or not."""
    deck = case(name)[0]
    r = DampedDynamics(deck, RHO, solve=solve_live)
    if damped:
        r.set_damping(*PAIRS[2])
    v0 = np.cos(2.0 * deck.nodes[:, [2, 0, 1]] + 0.3)
    v0.ravel()[r.mask] = 0.0
    r.v = v0.copy()
    done, its, traj = r.newmark(1, STEP_DT, 0.25, 0.5, 0.0, MAX_NEWTON, NEWTON_TOL)
    r.close()
    assert done == 1
    for a in (v0,) + traj[0]:
        a.setflags(write=False)
    return v0, its[0], traj[0]


@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "damped"])
@pytest.mark.parametrize("name", ["fan126", "hub66_iso_hub_pole_ring"])
def test_one_newmark_step(name, damped):
    """One step of feahip_solve_dynamic (full Newton) from given velocities: what first runs k_mass_residual, and with
    (0.7, 0.013) k_damp_residual<true>, on a long row and on full tiles.  State against the restatement under U_TOL."""
    assert PAIRS[2] == (0.7, 0.013)
    deck = case(name)[0]
    v0, its_w, want = one_step(name, damped)
    s = feahip.FeaSolver(deck)
    s.set_mass(RHO)
    if damped:
        s.set_damping(*PAIRS[2])
    s.set_velocities(v0)
    done, its, _ = s.solve_dynamic(1, STEP_DT, 0.25, 0.5, 0.0, max_newton=MAX_NEWTON, desired_tolerance=NEWTON_TOL)
    assert done == 1 and int(its[0]) == its_w, (its, its_w)
    check_state(f"{name} {'damped' if damped else 'undamped'}", s.nodes(), s.velocities(), s.accelerations(), want, deck)
    s.close()
