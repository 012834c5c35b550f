"""The states the constitutive kernels are held to the long-double restatement at (constitutive_reference.py).

Small bodies -- mesh.kuhn_block(2, 3, 2) linear (36 nodes) and quadratic (175 nodes), mesh.hex_block(2, 3, 2) -- far
from the corner of state space the assembly tests live in (an unrotated uniaxial stretch with det F in [1, 1.05],
lambda = mu, coordinates of order 1):

  volumetric     x = J^(1/3) X0, J on both sides of fd_log's branch point 2^k / sqrt 2, exponents -3 .. 2 of its
                 argument 1/J, and the identity limit 1 -+ 1e-9
  rotated        Q diag(0.6, 1.9, 0.8), Q [[1, .9, 0], [0, 1, .7], [0, 0, 1]], and the rigid motion Q X0 + c;
                 Q turns by 2.05 rad about (1, 2, 3)
  inhomogeneous  every corner node moved by a seeded random vector, mid-side nodes following their edge and moved a
                 little on their own, so edges curve
  material       (lambda, mu) = (1e6, 1), (0, 37), and a table of (1e4, 1) and (0, 37) scattered over the elements,
                 on a rotated stretch with J = 1.0125; and (1e6, 1) on the volumetric states J = 0.7 and 1.4143, next
                 to fd_log's branch point on the side where its exponent is 1 and -1: there the stress is lambda ln J
                 and |e| ln2 is largest beside |ln J|, so an error of ln2's low part is 2.9 times as large in the
                 stress as it is in ln2 (at lambda = mu the mu (B - I) terms bury it under the 1e-13 floor)
  scale          body and state times 1e-3, times 1e3, and both translated far from the origin

A state is a State: X0 and x as float64 arrays (what the library is given and the restatement converts exactly), the
material table and the element ids.  state(kind, name, dtype=np.longdouble) builds the same state with x computed in long
double instead of rounded to float64, for the closed-form and objectivity checks of the restatement itself."""
import functools

import numpy as np

import mesh

ELEMENT_TYPES = [("tet4", 1), ("tet10", 4), ("tet10", 5), ("tet10", 27), ("hex8", 8)]
DIMS = (2, 3, 2)
CELL = np.array([0.5, 2.0, 0.5])                       # the block's cell: size (1, 6, 1) over DIMS
VOLUMETRIC_J = {"J0.25": 0.25, "J0.5": 0.5, "J0.7": 0.7, "J0.7072": 0.7072, "J1-1e-9": 1 - 1e-9, "J1+1e-9": 1 + 1e-9,
                "J1.4141": 1.4141, "J1.4143": 1.4143, "J2": 2.0, "J4": 4.0, "J8": 8.0}
AXIS, ANGLE, SHIFT = (1.0, 2.0, 3.0), 2.05, (3.0, -2.0, 5.0)
STRETCH = (0.6, 1.9, 0.8)
SHEAR = ((1.0, 0.9, 0.0), (0.0, 1.0, 0.7), (0.0, 0.0, 1.0))
MATERIAL_STRETCH = (0.9, 1.25, 0.9)
TABLE = ((1e4, 1.0), (0.0, 37.0))
# Amplitudes, in cell spacings, of the corner and the mid-side displacements of the inhomogeneous state, and the
# translation of the offset state.  0.3 and 0.05 keep every Gauss point of every element type the right way round
# (det J > 0 and det F > 0: the admission condition test_constitutive_reference_cpu.py asserts; on the linear block
# det F runs from 0.22 to 2.4, at the 27 points of the quadratic one from 0.11 to 3.3).  The translation is 1e3 for the
# linear tetrahedron: its kernels subtract an element's first node before anything else and so does its restatement
# (constitutive_reference.evaluate, local), whose float64-to-long-double gap stays at 1e-14 there.  The 10- and 8-node
# kernels, the oracle and hence their restatement sum sum_k dN_k x_k and sum_k X_k (x) g_k as the formulas stand and
# lose |x| / cell digits: at 1e3 the restatement's own gap is 2e-11 .. 3e-11 (10 nodes, all three rules) and 3.4e-12
# (brick), over the ceiling, so the amplitude is lowered 1e3, 5e2, 2e2, 1e2, 5e1, 2e1 until the restatement alone is
# admitted: 2e2 for the brick; 2e1 for the quadratic block, which is one state for its three rules -- the 27-point rule
# is admitted from 5e1 (gap 7e-13), the 4- and 5-point rules only at 2e1 (1.3e-12 .. 1.4e-12 at 5e1, K_sigma v).
INHOMOGENEOUS_AMP = {"tet4": (0.3, 0.0), "tet10": (0.3, 0.05), "hex8": (0.3, 0.0)}
OFFSET = {"tet4": 1e3, "tet10": 2e1, "hex8": 2e2}

FAMILIES = {
    "volumetric": list(VOLUMETRIC_J),
    "rotated": ["rot_stretch", "rot_shear", "rigid"],
    "inhomogeneous": ["inhomogeneous"],
    "material": ["mat_1e6_1", "mat_0_37", "mat_table", "mat_1e6_1_J0.7", "mat_1e6_1_J1.4143"],
    "scale": ["scale_1e-3", "scale_1e3", "offset"],
}
STATES = [n for names in FAMILIES.values() for n in names]
FAMILY_OF = {n: fam for fam, names in FAMILIES.items() for n in names}
NH_MODEL = 1                                           # feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN


class State:
    def __init__(self, kind, name, conn, X0, x, materials, ids):
        self.kind, self.name, self.conn, self.X0, self.x = kind, name, conn, X0, x
        self.materials = np.asarray(materials, dtype=np.float64).reshape(-1, 2)
        self.ids = np.asarray(ids, dtype=np.int32)
        self.table = len(self.materials) > 1
        self.cell = float(np.abs(X0[conn[:, 1]] - X0[conn[:, 0]]).max(axis=1).min())     # shortest cell edge (finite-difference step)


@functools.lru_cache(maxsize=None)
def block(kind):
    if kind == "hex8":
        nodes, el = mesh.hex_block(*DIMS)
    else:
        nodes, el = mesh.kuhn_block(*DIMS, quadratic=(kind == "tet10"))
    nodes.setflags(write=False); el.setflags(write=False)
    return nodes, el


def rotation(dtype):
    """Rodrigues: the rotation by ANGLE about AXIS."""
    a = np.asarray(AXIS, dtype=dtype)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=dtype)
    t = dtype(ANGLE)
    return np.eye(3, dtype=dtype) + np.sin(t) * K + (1 - np.cos(t)) * apply_m(K, K)


def apply_m(A, B):
    return (A[:, :, None] * B[None, :, :]).sum(axis=1)


def apply(A, X):
    """x_n = A X_n for every node, as plain sums in A's dtype."""
    return (X[:, None, :] * A[None, :, :]).sum(axis=-1)


def scattered(E, n):
    """hetero_reference.scattered_ids' rule for a table of n entries: id = (7 e + 3) % n."""
    return ((7 * np.arange(E) + 3) % n).astype(np.int32)


def random_displacement(kind, conn, N):
    """Seeded: corners by amp cells per axis; a mid-side node by the mean of its edge's ends plus a move of its own."""
    amp, mid = INHOMOGENEOUS_AMP[kind]
    rng = np.random.default_rng(20)
    own = 2.0 * rng.random((N, 3)) - 1.0
    if kind != "tet10":
        return amp * CELL * own
    u = np.zeros((N, 3))
    corners = np.unique(conn[:, :4])
    u[corners] = amp * CELL * own[corners]
    for k, (a, b) in enumerate(mesh._EDGES):
        m = conn[:, 4 + k]
        u[m] = 0.5 * (u[conn[:, a]] + u[conn[:, b]]) + mid * CELL * own[m]
    return u


def state(kind, name, dtype=np.float64):
    """The State `name` on the block of `kind`; with dtype=np.longdouble x (and a scaled X0) are left unrounded."""
    X0f, conn = block(kind)
    X0 = np.asarray(X0f, dtype=dtype)
    E = len(conn)
    mats, ids = [(100.0, 100.0)], np.zeros(E, dtype=np.int32)
    Q = rotation(dtype)
    diag = lambda d: np.diag(np.asarray(d, dtype=dtype))
    if name in VOLUMETRIC_J:
        x = np.cbrt(dtype(VOLUMETRIC_J[name])) * X0
    elif name.startswith("mat_1e6_1_J"):
        x = np.cbrt(dtype(VOLUMETRIC_J[name[len("mat_1e6_1_"):]])) * X0
        mats = [(1e6, 1.0)]
    elif name == "rot_stretch":
        x = apply(apply_m(Q, diag(STRETCH)), X0)
    elif name == "rot_shear":
        x = apply(apply_m(Q, np.asarray(SHEAR, dtype=dtype)), X0)
    elif name == "rigid":
        x = apply(Q, X0) + np.asarray(SHIFT, dtype=dtype)
    elif name == "inhomogeneous":
        x = X0 + np.asarray(random_displacement(kind, conn, len(X0)), dtype=dtype)
    elif name.startswith("mat_"):
        x = apply(apply_m(Q, diag(MATERIAL_STRETCH)), X0)
        if name == "mat_1e6_1":
            mats = [(1e6, 1.0)]
        elif name == "mat_0_37":
            mats = [(0.0, 37.0)]
        else:
            mats, ids = list(TABLE), scattered(E, len(TABLE))
    elif name in ("scale_1e-3", "scale_1e3"):
        c = dtype(1e-3 if name == "scale_1e-3" else 1e3)
        x = c * apply(apply_m(Q, diag(STRETCH)), X0)
        X0 = c * X0
    elif name == "offset":
        x = apply(apply_m(Q, diag(STRETCH)), X0) + dtype(OFFSET[kind])
        X0 = X0 + dtype(OFFSET[kind])
    else:
        raise KeyError(name)
    if dtype is np.float64:
        X0, x = np.ascontiguousarray(X0), np.ascontiguousarray(x)
        X0.setflags(write=False); x.setflags(write=False)
    return State(kind, name, conn, X0, x, mats, ids)


def rotated(st, dtype=np.longdouble):
    """The same state turned once more: Q x (X0 unchanged), for K(Qx) = Q K(x) Q' and f(Qx) = Q f(x)."""
    Q = rotation(dtype)
    return State(st.kind, st.name + "+Q", st.conn, st.X0, apply(Q, np.asarray(st.x, dtype=dtype)), st.materials, st.ids), Q


# ---- the restatement's runs on a case, and its own float64-to-long-double gap by every yardstick -----------------
VECTORS = 3                                            # seeded vectors K_sigma is multiplied with


def test_vectors(ndof):
    return np.random.default_rng(11).standard_normal((VECTORS, ndof))


def point_scale(s):
    """One number per Gauss point (or node) from the entrywise stress scale: its largest entry."""
    return np.abs(s).max(axis=(-2, -1), keepdims=True)


def selections(st):
    """nodal_stresses' element selections: all elements (-1), and each material of a table."""
    return [(-1, None)] + ([(m, st.ids == m) for m in range(len(st.materials))] if st.table else [])


class Case:
    """A state on an element type and a model: `st`, the long-double run `hi` (constitutive_reference.Result), the
    derived long-double references (`nodal`, `ksv`, `ksv_scale`) and `gap`: for every quantity the difference of the
    float64 run from the long-double run, by the yardstick the kernels are measured with."""


@functools.lru_cache(maxsize=4)
def reference(kind, G, model, name):
    import constitutive_reference as cr
    st = state(kind, name)
    lo, hi = (cr.run(kind, G, st.conn, st.X0, st.x, st.materials, st.ids, model, dt) for dt in (np.float64, np.longdouble))
    c = Case()
    c.kind, c.G, c.model, c.name, c.st, c.hi = kind, G, model, name, st, hi
    c.rowscale = np.abs(hi.K).reshape(hi.N, -1).max(axis=1)
    c.sig_scale = point_scale(hi.el.sscale)
    c.gap = {"K": cr.err_block_rows(lo.K, hi.K), "f": cr.err_scaled(lo.f, hi.f, hi.fscale),
             "F": cr.err_own_max(lo.el.F, hi.el.F, 2), "g": cr.err_own_max(lo.el.g, hi.el.g, 2),
             "detJ": cr.err_scaled(lo.el.detJ, hi.el.detJ, np.abs(hi.el.detJ)),
             "sigma": cr.err_scaled(lo.el.sig, hi.el.sig, c.sig_scale),
             "W": cr.err_scaled(lo.W, hi.W, hi.Wscale)}
    c.nodal = {}
    for m, sel in selections(st):
        sl, _, _ = cr.nodal_stress(lo, st.conn, sel)
        sh, sc, wt = cr.nodal_stress(hi, st.conn, sel)
        scale = np.where(wt[:, None, None] > 0, point_scale(sc), 1)
        c.nodal[m] = (sh, scale, wt)
        c.gap["nodal", m] = cr.err_scaled(sl, sh, scale)
    v = test_vectors(3 * hi.N)
    vh = np.asarray(v, dtype=np.longdouble)
    c.v = v
    c.ksv = (hi.Ksigma[None, :, :] * vh[:, None, :]).sum(axis=-1)
    c.ksv_scale = (np.abs(hi.Ksigma)[None, :, :] * np.abs(vh)[:, None, :]).sum(axis=-1)
    c.ksv_cscale = (hi.Ksscale[None, :, :] * np.abs(vh)[:, None, :]).sum(axis=-1)
    ksv_lo = (lo.Ksigma[None, :, :] * v[:, None, :]).sum(axis=-1)
    c.gap["Ksigma"] = cr.err_scaled(ksv_lo, c.ksv, c.ksv_scale)
    c.gap["Ksigma_c"] = cr.err_scaled(ksv_lo, c.ksv, c.ksv_cscale)
    detF = cr.det3(hi.el.F)
    c.detJ_min, c.detF_min, c.detF_max = float(hi.el.detJ.min()), float(detF.min()), float(detF.max())
    c.lo = lo
    return c


# K_sigma is linear in the stress, and "relative to |K_sigma| |v|" measures it against its own size: where the body is
# stress-free to rounding (the identity limit, the rigid motion) that size is the rounding of O(mu) terms, the
# restatement's own gap by this yardstick is 1e-10 .. 1 and the comparison says nothing.  These states are admitted for
# everything but that yardstick (test_constitutive_reference_cpu.py asserts that this list is exactly what fails); their
# K_sigma v is measured against the cancellation scale instead, |g_a| . s . |g_b| summed like K_sigma, times |v|
# ("Ksigma_c"): that the product is zero to rounding of what it is the difference of.
KSIGMA_NOT_ADMITTED = ("J1-1e-9", "J1+1e-9", "rigid")


# The stress of the nearly incompressible Neo-Hookean states is lambda ln J with ln J = 0.0125: an error dF in F is an
# error dF / ln J of that scale.  On the quadratic block the undifferenced sums leave dF = 1e-14 .. 2e-14 in float64, so
# the Gauss-point stress of the restatement itself is 0.8e-12 .. 2.1e-12 off, 100 x gap at or over the ceiling.  The
# states stay, and their stress is held to the ceiling, 1e-10 (the clamp of the rule): 50 to 100 times the gap.
SIGMA_OVER_CEILING = {("tet10", NH_MODEL, "mat_1e6_1"), ("tet10", NH_MODEL, "mat_table")}


def not_admitted(c):
    """The admission condition, quantity by quantity: every Gauss point the right way round in the long-double run
    (else everything fails), and 100 times the gap under the ceiling of the tolerance rule.  Returns what fails."""
    if not (c.detJ_min > 0 and c.detF_min > 0):
        return set(c.gap)
    return {k for k, g in c.gap.items() if not 100.0 * g < 1e-10}
