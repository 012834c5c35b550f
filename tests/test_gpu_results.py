"""Result recovery on the GPU against tests/results_reference.py: nodal stress, von Mises stress, weight, nodal energy
and strain energy on every element type and both models, the selection by material, the reactions, freshness after the
nodes or the table change, row shards, rank contexts and in-process groups, the explicit run, the command line and the
timing hook.  The restatement is always evaluated at the GPU context's own nodes().

Bound: 1e-12 of max|sigma| (of max|T| for the reactions, of |W| for the energy) on linear tetrahedra, the project's own
bound for sigma and f (tests/test_gpu_parity.py); 1e-11 on tet10 and hex8, where that file holds sigma to 1e-11."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
from dynamics_reference import loaded_bar
from explicit_reference import hub_fan
from hetero_reference import MATERIALS, layered_ids, scattered_ids, with_materials
from results_reference import ResultsRestatement, smooth_field

pytestmark = pytest.mark.gpu

MODELS = {"neohookean": feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, "a5": feahip.MODEL_A5}
DIMS = (2, 4, 2)
BIG = (4, 12, 4)     # 325 nodes: several chunks, and rows for every rank of two shards or three rank contexts
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynamics", "explicit_bar.sexp")


def tol_of(deck):
    return 1e-12 if deck.nodes_per_element == 4 else 1e-11


def make_deck(name, model="neohookean"):
    if name in ("tet4", "tet10", "hex8"):
        return loaded_bar(name, DIMS, model=MODELS[model])
    if name == "big":
        return loaded_bar("tet4", BIG, model=MODELS[model])
    if name == "hub":
        return hub_fan(150)
    if name.startswith("table_"):
        d = loaded_bar(name[6:], DIMS, model=MODELS[model])
        return with_materials(d, MATERIALS, scattered_ids(d))
    raise KeyError(name)


def check_fields(tag, s, r, x, tol, rows=None, material=-1, energy=True):
    """nodal stress, von Mises, weight (and nodal energy) of the context s on `rows` against the restatement at x"""
    rows = slice(None) if rows is None else rows
    sig6, vm, wt = s.nodal_stresses(material)
    w6, wvm, wwt = r.nodal_stresses(x, material)
    scale = np.abs(w6).max()
    es, ev = np.abs(sig6[rows] - w6[rows]).max() / scale, np.abs(vm[rows] - wvm[rows]).max() / scale
    ew = np.abs(wt[rows] - wwt[rows]).max() / wwt.max()
    print(tag, "sigma", es, "von Mises", ev, "weight", ew)
    assert es <= tol and ev <= tol and ew <= tol
    if energy:
        W, wn = r.energy(x)
        got = s.nodal_energy()
        en = np.abs(got[rows] - wn[rows]).max() / np.abs(wn).max()
        print(tag, "nodal energy", en)
        assert en <= tol
    return sig6, vm, wt


# ---- 1. fields and energy against the restatement ------------------------------------------------------------------
CASES = [(k, m, st) for k in ("tet4", "tet10", "hex8") for m in sorted(MODELS) for st in ("solved", "smooth")]
CASES += [("big", "neohookean", "smooth"), ("hub", "neohookean", "smooth"),
          ("table_tet4", "neohookean", "smooth"), ("table_tet10", "a5", "smooth"), ("table_hex8", "neohookean", "solved")]


@pytest.mark.parametrize("name,model,state", CASES)
def test_fields_and_energy_match_the_restatement(name, model, state):
    deck = make_deck(name, model)
    s = feahip.FeaSolver(deck)
    if state == "solved":
        done, _, _ = s.solve(load_increments=3)
        assert done == 3
    else:
        s.set_nodes(smooth_field(deck.nodes, 0.05 if name == "hub" else 0.12))
    x = s.nodes()
    r = ResultsRestatement(deck)
    tol = tol_of(deck)
    first = check_fields(f"{name} {model} {state}", s, r, x, tol)
    W, want = s.strain_energy(), r.energy(x)[0]
    print(name, model, state, "W", W, want, abs(W - want) / abs(want))
    assert abs(W - want) <= tol * abs(want)
    wn = s.nodal_energy()
    assert abs(wn.sum() - W) <= 1e-13 * abs(W) * len(wn) ** 0.5
    again = s.nodal_stresses()                                         # the same bits on every call
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    assert s.strain_energy() == W and np.array_equal(s.nodal_energy(), wn)
    r.close()
    s.close()


# ---- 2. selection by material ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tet4", "hex8"])
def test_selection_by_material(kind):
    base = loaded_bar(kind, DIMS)
    ids = layered_ids(base)
    deck = with_materials(base, MATERIALS, ids)
    s = feahip.FeaSolver(deck)
    s.set_nodes(smooth_field(deck.nodes))
    x = s.nodes()
    r = ResultsRestatement(deck)
    tol = tol_of(deck)
    for m in range(len(MATERIALS)):
        sig6, vm, wt = check_fields(f"{kind} material {m}", s, r, x, tol, material=m, energy=False)
        outside = ~np.isin(np.arange(len(deck.nodes)), deck.elements[ids == m])
        assert outside.any() and not outside.all()
        assert np.all(wt[outside] == 0.0) and np.all(sig6[outside] == 0.0) and np.all(vm[outside] == 0.0)
        assert np.all(wt[~outside] > 0.0)
    every = s.nodal_stresses(-1)
    assert all(np.array_equal(a, b) for a, b in zip(every, s.nodal_stresses()))
    check_fields(f"{kind} all materials", s, r, x, tol)
    for bad in (len(MATERIALS), -2, 1000):
        assert s._lib.feahip_get_nodal_stresses(s._ctx, bad, None, None, None) == feahip.EINVAL
    assert all(np.array_equal(a, b) for a, b in zip(every, s.nodal_stresses()))   # the context still works
    r.close()
    s.close()
    plain = feahip.FeaSolver(base)                                     # no table: only -1 is a selection
    plain.set_nodes(x)
    assert plain._lib.feahip_get_nodal_stresses(plain._ctx, 0, None, None, None) == feahip.EINVAL
    assert plain._lib.feahip_get_nodal_stresses(plain._ctx, -1, None, None, None) == 0
    assert plain._lib.feahip_strain_energy(plain._ctx, None) == feahip.EINVAL
    assert plain._lib.feahip_get_nodal_energy(plain._ctx, None) == feahip.EINVAL
    assert plain._lib.feahip_get_reactions(plain._ctx, None) == feahip.EINVAL
    assert plain._lib.feahip_get_reactions(None, None) == feahip.EINVAL
    assert plain.strain_energy() > 0.0
    plain.close()


# ---- 3. reactions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("load", ["traction", "end_motion"])
@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_reactions_match_the_restatement(kind, load):
    deck = loaded_bar(kind, DIMS) if load == "traction" else loaded_bar(kind, DIMS, end_motion=0.05)
    s = feahip.FeaSolver(deck)
    done, _, _ = s.solve(load_increments=3)
    assert done == 3
    x, lam = s.nodes(), s.load_factor()
    assert lam == 3.0
    r = ResultsRestatement(deck)
    tol = tol_of(deck)
    T = np.abs(r.internal(x)).max()
    before = (s.forces().copy(), s.matrix_yale()[2].copy(), s.solution().copy(), s.update_state())
    got = s.reactions()
    after = (s.forces(), s.matrix_yale()[2], s.solution(), s.update_state())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))    # f, K, u and the count of bad points: bit for bit
    assert np.array_equal(s.nodes(), x)
    want = r.reactions(x, lam)
    err = np.abs(got - want).max() / T
    print(kind, load, "reactions", err, "max|T|", T, "max|r|", np.abs(want).max())
    assert err <= tol and np.all(got[~r.h.mask] == 0.0) and np.abs(got).max() > 1e-3 * T
    # equilibrium of the whole body: the supports carry the applied loads
    balance = got.reshape(-1, 3).sum(axis=0) + lam * r.external(x).reshape(-1, 3).sum(axis=0)
    print(kind, load, "balance", balance)
    assert np.abs(balance).max() <= tol * T * s.ndof
    assert np.array_equal(s.reactions(), got)
    s.set_nodes(smooth_field(deck.nodes))                              # away from equilibrium: still minus the residual
    x = s.nodes()
    got, want = s.reactions(), r.reactions(x, lam)
    err = np.abs(got - want).max() / np.abs(r.internal(x)).max()
    print(kind, load, "reactions off equilibrium", err)
    assert err <= tol
    r.close()
    s.close()


# ---- 4. freshness ----------------------------------------------------------------------------------------------------
def test_results_follow_the_nodes_and_the_table():
    base = loaded_bar("tet4", DIMS)
    deck = with_materials(base, MATERIALS, scattered_ids(base))
    s = feahip.FeaSolver(deck)
    r = ResultsRestatement(deck)
    s.set_nodes(smooth_field(deck.nodes, 0.06))
    a = check_fields("first nodes", s, r, s.nodes(), 1e-12)
    Wa = s.strain_energy()
    s.set_nodes(smooth_field(deck.nodes, 0.12))
    x = s.nodes()
    b = check_fields("moved nodes", s, r, x, 1e-12)
    Wb = s.strain_energy()
    assert not np.array_equal(a[0], b[0]) and Wb > 2.0 * Wa
    assert abs(Wb - r.energy(x)[0]) <= 1e-12 * Wb
    r.close()
    other = with_materials(base, MATERIALS[::-1].copy(), layered_ids(base))
    s.set_materials(other.materials, other.element_material)
    r = ResultsRestatement(other)
    c = check_fields("new table", s, r, x, 1e-12)
    Wc = s.strain_energy()
    assert not np.array_equal(b[0], c[0]) and abs(Wc - r.energy(x)[0]) <= 1e-12 * Wc
    got, want = s.reactions(), r.reactions(x, 0.0)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(r.internal(x)).max()
    r.close()
    s.close()


# ---- 5. shards, rank contexts, groups --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_reference():
    """The unsharded context's results on the big bar at the smooth field, computed once and shared."""
    deck = loaded_bar("tet4", BIG)
    x = smooth_field(deck.nodes)
    s = feahip.FeaSolver(deck)
    s.set_nodes(x)
    r = ResultsRestatement(deck)
    check_fields("big, one context", s, r, x, 1e-12)
    out = s.nodal_stresses() + (s.nodal_energy(), s.reactions(), s.strain_energy())
    assert np.abs(out[4] - r.reactions(x, 0.0)).max() <= 1e-12 * np.abs(r.internal(x)).max()
    r.close()
    s.close()
    for a in out[:5]:
        a.setflags(write=False)
    return deck, x, out


def check_owned(tag, got, want, rows, other_zero):
    """per-node arrays: the owned rows equal the unsharded ones to 1e-12 of their scale, every other row is zero"""
    for g, w in zip(got, want):
        scale = np.abs(w).max()
        assert np.abs(g[rows] - w[rows]).max() <= 1e-12 * scale, tag
        if other_zero is not None:
            assert np.all(g[other_zero] == 0.0), tag


def test_row_shards_are_authoritative_on_their_rows():
    deck, x, (sig6, vm, wt, wn, reac, W) = big_reference()
    parts = []
    for rank in range(2):
        s = feahip.FeaSolver(deck)
        s.set_row_shard(rank, 2)
        s.set_nodes(x)
        nd = s.owned_nodes()
        other = np.setdiff1d(np.arange(len(deck.nodes)), nd)
        assert len(nd) > 0 and len(other) > 0
        check_owned(f"shard {rank}", s.nodal_stresses() + (s.nodal_energy(),), (sig6, vm, wt, wn), nd, other)
        check_owned(f"shard {rank} reactions", (s.reactions().reshape(-1, 3),), (reac.reshape(-1, 3),), nd, other)
        parts.append(s.strain_energy())                                # no transport: this shard's share
        s.close()
    print("shares", parts, W)
    assert min(parts) > 0.0 and abs(sum(parts) - W) <= 1e-12 * W       # a ghost element is counted once


def test_rank_contexts_are_authoritative_on_their_rows():
    deck, x, (sig6, vm, wt, wn, reac, W) = big_reference()
    parts = []
    for rank in range(3):
        s = feahip.RankSolver(deck, rank, 3)
        s.set_nodes(x[s.node_global])
        nd = s.node_global[:s.n_own].astype(np.int64)
        got = s.nodal_stresses() + (s.nodal_energy(), s.reactions().reshape(-1, 3))
        for a, w in zip(got, (sig6, vm, wt, wn, reac.reshape(-1, 3))):
            assert np.abs(a[:s.n_own] - w[nd]).max() <= 1e-12 * np.abs(w).max(), rank
            assert s.n_own < s.N and np.all(a[s.n_own:] == 0.0), rank
        parts.append(s.strain_energy())
        s.close()
    print("shares", parts, W)
    assert min(parts) > 0.0 and abs(sum(parts) - W) <= 1e-12 * W       # a ghost element is counted once


@pytest.mark.parametrize("form", ["group2", "ranks3"])
def test_groups_and_rank_contexts(form):
    deck, x, (sig6, vm, wt, wn, reac, W) = big_reference()
    g = feahip.FeaGroup(deck, 2) if form == "group2" else feahip.FeaGroup(deck, 3, rank_contexts=True)
    for rk in g.ranks:
        rk.set_nodes(x[rk.node_global] if g.rank_contexts else x)
    for k, (rk, nd) in enumerate(zip(g.ranks, g.nodes)):
        got = rk.nodal_stresses() + (rk.nodal_energy(), rk.reactions().reshape(-1, 3))
        want = (sig6, vm, wt, wn, reac.reshape(-1, 3))
        if g.rank_contexts:                                            # local ids: owned rows first, the halo rows zero
            for a, w in zip(got, want):
                assert np.abs(a[:rk.n_own] - w[nd]).max() <= 1e-12 * np.abs(w).max(), (form, k)
                assert np.all(a[rk.n_own:] == 0.0), (form, k)
        else:
            check_owned(f"{form} rank {k}", got, want, nd, np.setdiff1d(np.arange(len(deck.nodes)), nd))
    stitched = g.gather("nodal_stresses") + (g.gather("nodal_energy"),)
    check_owned(form, stitched, (sig6, vm, wt, wn), slice(None), None)
    assert np.abs(g.gather("reactions") - reac).max() <= 1e-12 * np.abs(reac).max()
    Wg = g.strain_energy()
    print(form, "W", Wg, W)
    assert abs(Wg - W) <= 1e-12 * W                                    # ghost elements are not counted twice
    assert abs(stitched[3].sum() - W) <= 1e-12 * W
    assert all(rk.strain_energy() == Wg for rk in g.ranks)             # driven from any member
    g.close()


# ---- 6. explicit run -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gravity", "tet4"])
def test_strain_energy_after_explicit_steps(name):
    """After the 20 explicit steps of the cases of tests/test_gpu_explicit.py, at the returned nodes.

    `tet4` (a traction ramped up on the clamped bar) strains the body: W is held to 1e-12 of |W|.

    `gravity` is the free block in free fall.  Its exact strain energy is ZERO: on linear tetrahedra the HRZ-lumped
    mass equals the row sums of the consistent one, so a = F_body / ml is the same vector b at every node and the motion
    is rigid.  Both sides then return the rounding of mu/2 (tr b - 3) - mu ln J + ..., terms of size mu V0 = 100 that
    cancel: measured on an MI355X W = 2.08e-15 against the restatement's -1.16e-16 (a negative energy: noise as well).
    A bound relative to |W| cannot be met by any evaluation in float64 there, the restatement's included, so this case is
    held to 1e-12 of the energy of the run, T + |W| (T = 0.686: 6.9e-13 allowed, 2.2e-15 measured) -- the scale an
    energy balance is read at, and three hundred times below 1e-12 of the cancelling terms."""
    from test_gpu_explicit import make_solver, reference
    dt, traj, ke = reference(name)
    s, deck, dlam, steps = make_solver(name)
    done, _ = s.solve_explicit(steps, dt, dlambda=dlam)
    assert done == steps
    x = s.nodes()
    r = ResultsRestatement(deck)
    W, want = s.strain_energy(), r.energy(x)[0]
    r.close()
    T = s.kinetic_energy()
    print(name, "strain energy", W, "restatement", want, abs(W - want), "kinetic", T, "kinetic + strain", T + W)
    assert T > 0.0
    if name == "gravity":
        assert abs(W - want) <= 1e-12 * (T + abs(want))
    else:
        assert W > 0.0 and abs(W - want) <= 1e-12 * abs(want)
    s.close()


# ---- 7. command line -------------------------------------------------------------------------------------------------
def node_data(lines, title):
    """[(values per node)] of every $NodeData section with this title"""
    out = []
    for i, ln in enumerate(lines):
        if ln == "$NodeData" and lines[i + 2] == f'"{title}"':
            n = int(lines[i + 8])
            out.append(np.array([[float(v) for v in row.split()[1:]] for row in lines[i + 9:i + 9 + n]]))
            assert lines[i + 9 + n] == "$EndNodeData"
    return out


def test_command_line_writes_the_results(tmp_path):
    with open(GOLDEN) as f:
        text = f.read()
    assert text.count(":restep 0))") == 1
    (tmp_path / "plain").mkdir()
    plain, full = tmp_path / "plain" / "explicit_bar.sexp", tmp_path / "explicit_bar.sexp"
    plain.write_text(text)
    full.write_text(text.replace(":restep 0))", ":restep 0)\n   (results :nodal-stress t :energy t :reactions t))"))
    d = feahip.Deck.load(str(full))
    assert d.results == dict(nodal_stress=True, energy=True, reactions=True)
    n = len(d.nodes)
    s = feahip.FeaSolver(d)
    done, _ = s.solve_explicit()
    assert done == 20
    u, (sig6, vm, _), W, T, reac = s.nodes() - d.nodes, s.nodal_stresses(), s.strain_energy(), s.kinetic_energy(), s.reactions()
    s.close()
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = subprocess.run([exe, str(full)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = (tmp_path / "explicit_bar.msh").read_text().splitlines()
    (stress,), (mises,), disp = node_data(lines, "Nodal stress"), node_data(lines, "Von Mises"), node_data(lines, "Displacements")
    assert stress.shape == (n, 9) and mises.shape == (n, 1) and len(disp) == 2
    full9 = sig6[:, [0, 3, 5, 3, 1, 4, 5, 4, 2]]
    assert np.abs(stress - full9).max() <= 1e-6 and np.abs(mises[:, 0] - vm).max() <= 1e-6   # the file holds six decimals
    assert np.abs(sig6).max() > 1e-2 and np.abs(disp[1] - u).max() <= 1e-6
    energy = re.findall(r"^Strain energy (\S+), kinetic energy (\S+), total (\S+)$", out.stdout, re.M)
    sums = re.findall(r"^Reactions sum (\S+) (\S+) (\S+)$", out.stdout, re.M)
    assert len(energy) == 20 and len(sums) == 20 and len(re.findall(r"^Explicit step \d+ finished", out.stdout, re.M)) == 20
    w, t, tot = (float(v) for v in energy[-1])
    assert abs(w - W) <= 1e-9 * W and abs(t - T) <= 1e-9 * T and abs(tot - (w + t)) <= 1e-12 * tot
    assert np.abs(np.array([float(v) for v in sums[-1]]) - reac.reshape(-1, 3).sum(axis=0)).max() <= 1e-9 * np.abs(reac).max()
    # the same deck without the section: the file and the log of before
    out0 = subprocess.run([exe, str(plain)], capture_output=True, text=True, timeout=120)
    assert out0.returncode == 0, out0.stderr
    assert "Strain energy" not in out0.stdout and "Reactions" not in out0.stdout
    lines0 = (tmp_path / "plain" / "explicit_bar.msh").read_text().splitlines()
    assert lines0.count("$NodeData") == 2 and not node_data(lines0, "Nodal stress") and not node_data(lines0, "Von Mises")
    at = max(i for i, ln in enumerate(lines0) if ln == "$NodeData")   # as tests/test_gpu_explicit.py reads it
    start = next(i for i in range(at, len(lines0)) if lines0[i].strip() == str(n)) + 1
    got = np.array([[float(v) for v in ln.split()[1:4]] for ln in lines0[start:start + n]])
    assert np.abs(u).max() > 1e-3 and np.abs(got - u).max() <= 1e-6
    keep = [i for i, ln in enumerate(lines) if ln == "$NodeData" and lines[i + 2] in ('"Nodal stress"', '"Von Mises"')]
    cut = [ln for i, ln in enumerate(lines) if not any(k <= i <= k + 9 + n for k in keep)]
    assert cut == lines0                                               # nothing else in the file differs


# ---- 8. timing hook --------------------------------------------------------------------------------------------------
def test_time_kernel_12():
    deck = loaded_bar("tet4", BIG)
    s = feahip.FeaSolver(deck)
    ms = s.time_kernel(12, warmup=1, iters=3)
    assert ms > 0.0
    s.close()
