"""The decks of the contact tests, shared by the CPU and the GPU files: the platen on the uniaxial block, the sphere on
the clamped pad, the block dropped on a plane, and the five obstacles of the kernel-parity test."""
import numpy as np

import feahip
import mesh
import contact_reference as cr


def library_obstacles(obstacles):
    """The restatement's obstacles as FeaSolver.set_contact takes them."""
    return [(o["kind"], o["point"], o["direction"], o["radius"], o["travel"]) for o in obstacles]


# ---- a frictionless plane pressing the top face of a uniaxial block ----------------------------------------------------
PLATEN_TRAVEL, PLATEN_STEPS = 0.3, 3
# the energy tolerance at which the GPU runs of the platen are compared with the restatement iteration by iteration:
# test_contact_reference_cpu.py checks that no increment of any of the three decks hangs on a borderline comparison there
# (at 1e-12 the TET10 deck logs 2.4e-13 and 1.1e-11 in the iterations that decide)
PLATEN_TOLERANCE = 1e-8


def platen_deck(kind, **kw):
    """bar_deck(dims=(2, 3, 2), recipe="uniaxial") without the prescriptions of its top face."""
    deck = mesh.bar_deck(dims=(2, 3, 2), recipe="uniaxial", quadratic=kind == "tet10", hexa=kind == "hex8",
                         modified_newton=False, **kw)
    top = deck.nodes[:, 1] > deck.nodes[:, 1].max() - 1e-9
    keep = ~top[deck.presc_node]
    deck.presc_node = np.ascontiguousarray(deck.presc_node[keep])
    deck.presc_type = np.ascontiguousarray(deck.presc_type[keep])
    deck.presc_values = np.ascontiguousarray(deck.presc_values[keep])
    return deck


def platen_contact(deck, penalty):
    """(contact faces, the restatement's Contact): the plane y = top, normal -y, travelling 0.3 down in 3 increments."""
    faces = mesh.block_side_faces(deck.nodes, deck.elements, 1, True)
    plane = cr.obstacle(cr.PLANE, (0.0, deck.nodes[:, 1].max(), 0.0), (0.0, -1.0, 0.0),
                        travel=(0.0, -PLATEN_TRAVEL / PLATEN_STEPS, 0.0))
    return faces, cr.Contact(deck.nodes, faces, [plane], penalty)


# ---- a sphere indenting a clamped pad ------------------------------------------------------------------------------------
SPHERE_STEPS, SPHERE_PENALTY = 4, 1e4


def sphere_deck(**kw):
    """A TET4 pad of (4, 2, 4) cells, 1 x 0.5 x 1, clamped at the bottom."""
    nodes, el = mesh.kuhn_block(4, 2, 4, origin=(0.0, 0.0, 0.0), size=(1.0, 0.5, 1.0))
    bot = np.nonzero(np.abs(nodes[:, 1]) < 1e-12)[0].astype(np.int32)
    return feahip.Deck(model=feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, parameters=[100.0, 100.0], ele_type=feahip.TETRAHEDRA4,
                       gauss_nodes_count=1, nodes=nodes, elements=el, presc_node=bot, presc_type=np.full(len(bot), 7, np.int32),
                       presc_values=np.zeros((len(bot), 3)), modified_newton=False, solver_type=feahip.CG, **kw)


def sphere_contact(deck, penalty=SPHERE_PENALTY):
    """A ball of radius 0.6 touching the top centre, travelling 0.1 down in 4 increments."""
    faces = mesh.block_side_faces(deck.nodes, deck.elements, 1, True)
    ball = cr.obstacle(cr.SPHERE, (0.5, 0.5 + 0.6, 0.5), radius=0.6, travel=(0.0, -0.1 / SPHERE_STEPS, 0.0))
    return faces, cr.Contact(deck.nodes, faces, [ball], penalty)


# ---- the five kinds around the deformed block of the parity test ----------------------------------------------------------
def parity_obstacles():
    """One obstacle of each kind around mesh.deformed_state of the bar [0, 1] x [1, 7] x [0, 1] (about 0.97 x [1, 7.6] x
    0.97 then), each with contact nodes on both sides of its surface."""
    return [cr.obstacle(cr.PLANE, (0.0, 7.2, 0.0), (0.1, -1.0, 0.2), travel=(0.0, 0.2, 0.0)),
            cr.obstacle(cr.SPHERE, (0.5, 0.5, 0.5), radius=0.6, travel=(0.0, 0.2, 0.0)),
            cr.obstacle(cr.SPHERE_INSIDE, (0.5, 4.0, 0.5), radius=3.2, travel=(0.1, 0.0, 0.0)),
            cr.obstacle(cr.CYLINDER, (1.3, 0.0, 0.5), (0.05, 1.0, 0.0), radius=0.45, travel=(-0.04, 0.0, 0.0)),
            cr.obstacle(cr.CYLINDER_INSIDE, (0.5, 0.0, 0.5), (0.0, 1.0, 0.0), radius=0.6, travel=(0.0, 0.3, 0.02))]
