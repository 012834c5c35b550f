"""Pins the oracle's leaf functions (3x3 algebra, material models).

Golden vectors: the reference's only unit test, solver-large/tests.c:17-24.
Reference results: tests/golden/leaf/reference_leaf.npz holds what the
reference's own dense_matrix.c / fea_model.c / tests.c (compiled in place as
oracle/_ref/libfearef.so, oracle/Makefile) return on random inputs, recorded
by tools/make_leaf_golden.py; the restatement must agree with them BIT FOR BIT.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_binding as ob

A = [[1, 2, 0], [2, 0, 3], [0, 2, 3]]
B = [[0, 2, 1], [1, 1, 1], [3, 2, -1]]
AB = [[2, 4, 3], [9, 10, -1], [11, 8, -1]]        # tests.c:20
AtB = [[2, 4, 3], [6, 8, 0], [12, 9, 0]]          # tests.c:21
ABt = [[4, 3, 7], [3, 5, 3], [7, 5, 1]]           # tests.c:22

# What the reference's own compiled leaf code returns on these inputs, recorded by tools/make_leaf_golden.py
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leaf", "reference_leaf.npz"))


def _call3(fn, a, b):
    r = ob.M33()
    fn(ob.m33(a), ob.m33(b), r)
    return ob.m33_np(r)


def test_matmul_golden_vectors():
    L = ob.lib()
    assert np.array_equal(_call3(L.orc_mul3x3, A, B), np.array(AB, float))
    assert np.array_equal(_call3(L.orc_tmul3x3, A, B), np.array(AtB, float))
    assert np.array_equal(_call3(L.orc_mult3x3, A, B), np.array(ABt, float))


def test_reference_self_test_passes():
    assert int(GOLD["self_test"]) == 1    # tests.c:53-56, run at fea_solver.c:76
    for key, want in (("self_mul", AB), ("self_tmul", AtB), ("self_mult", ABt)):
        assert np.array_equal(GOLD[key], np.array(want, float))


def test_dense_matrix_bit_exact_vs_reference():
    L = ob.lib()
    p = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    for k in range(len(GOLD["dense_a"])):
        a, b = GOLD["dense_a"][k], GOLD["dense_b"][k]
        for mine, theirs in ((L.orc_mul3x3, "dense_mul"), (L.orc_tmul3x3, "dense_tmul"), (L.orc_mult3x3, "dense_mult")):
            assert np.array_equal(_call3(mine, a, b), GOLD[theirs][k])
        assert L.orc_det3x3(ob.m33(a)) == GOLD["dense_det"][k]
        m1, d1 = ob.m33(a), C.c_double()
        assert L.orc_inv3x3(m1, C.byref(d1)) == GOLD["dense_inv_rc"][k]
        assert d1.value == GOLD["dense_inv_det"][k]
        assert np.array_equal(ob.m33_np(m1), GOLD["dense_inv"][k])
        v1, v2 = np.ascontiguousarray(GOLD["dense_v1"][k]), np.ascontiguousarray(GOLD["dense_v2"][k])
        assert L.orc_cdot(p(v1), p(v2), 37) == GOLD["dense_cdot"][k]


def test_singular_matrix_is_left_alone():
    L = ob.lib()
    z = [[1, 2, 3], [2, 4, 6], [0, 1, 1]]
    assert np.array_equal(GOLD["singular_in"], np.array(z, float))
    m1, d1 = ob.m33(z), C.c_double()
    assert L.orc_inv3x3(m1, C.byref(d1)) == 0 == GOLD["singular_rc"]
    assert np.array_equal(ob.m33_np(m1), np.array(z, float))
    assert np.array_equal(GOLD["singular_out"], np.array(z, float))


@pytest.mark.parametrize("model", [0, 1])
def test_material_models_bit_exact_vs_reference(model):
    L = ob.lib()
    par = (C.c_double * 10)(100.0, 37.5)                  # lambda, mu
    Fs = GOLD[f"model{model}_F"]
    assert len(Fs) > 150
    for k in range(len(Fs)):
        s1, c1 = ob.M33(), ob.C4()
        L.orc_stress(model, par, ob.m33(Fs[k]), s1)
        assert np.array_equal(ob.m33_np(s1), GOLD[f"model{model}_stress"][k])
        L.orc_ctensor(model, par, ob.m33(Fs[k]), c1)
        assert bytes(c1) == np.ascontiguousarray(GOLD[f"model{model}_ctensor"][k]).tobytes()


def test_neohookean_stress_known_values():
    """sigma = mu(B-I)/J + lambda ln J I/J on F = diag(k2,k1,k2), the
    closed form of exact-solutions/uniaxial/uniaxial_neohookean_bonet.m:20-37."""
    import math
    L = ob.lib()
    par = (C.c_double * 10)(100.0, 100.0)
    k1, k2 = 1.1, 0.97
    J = k1 * k2 * k2
    s = ob.M33()
    L.orc_stress(1, par, ob.m33(np.diag([k2, k1, k2])), s)
    S = ob.m33_np(s)
    assert S[1, 1] == pytest.approx((100 * (k1 ** 2 - 1) + 100 * math.log(J)) / J, rel=1e-14)
    assert S[0, 0] == pytest.approx((100 * (k2 ** 2 - 1) + 100 * math.log(J)) / J, rel=1e-13)
    assert S[0, 1] == 0 and S[1, 2] == 0
