#!/usr/bin/env python3
"""Golden vectors of the reference's leaf functions (dense_matrix.c, fea_model.c, tests.c).

Calls oracle/_ref/libfearef.so -- the reference's own sources compiled in place by oracle/Makefile, which
exists only where the reference tree does -- on the inputs of tests/test_oracle_leaf.py and stores inputs and
outputs in tests/golden/leaf/reference_leaf.npz, so that the tests pin the oracle's restatement bit for bit
against the reference's results on any checkout.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import oracle_binding as ob     # noqa: E402

A = [[1, 2, 0], [2, 0, 3], [0, 2, 3]]             # tests.c:17-18
B = [[0, 2, 1], [1, 1, 1], [3, 2, -1]]


def _call3(fn, a, b):
    r = ob.M33()
    fn(ob.m33(a), ob.m33(b), r)
    return ob.m33_np(r)


def main():
    if not ob.have_ref():
        sys.exit(f"{ob.REF_LIB} is not built: make -C oracle ref (needs the reference tree)")
    R = ob.ref()
    g = {"self_test": np.int32(R.do_tests()),                                  # tests.c:53-56
         "self_mul": _call3(R.matrix_mul3x3, A, B), "self_tmul": _call3(R.matrix_transpose_mul3x3, A, B),
         "self_mult": _call3(R.matrix_transpose2_mul3x3, A, B)}

    # dense_matrix.c on random inputs (the stream of test_dense_matrix_bit_exact_vs_reference)
    rng = np.random.default_rng(20251004)
    cols = {k: [] for k in ("a", "b", "mul", "tmul", "mult", "det", "inv", "inv_det", "inv_rc", "v1", "v2", "cdot")}
    p = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    for _ in range(200):
        a, b = rng.normal(size=(3, 3)), rng.normal(size=(3, 3))
        cols["a"].append(a); cols["b"].append(b)
        cols["mul"].append(_call3(R.matrix_mul3x3, a, b))
        cols["tmul"].append(_call3(R.matrix_transpose_mul3x3, a, b))
        cols["mult"].append(_call3(R.matrix_transpose2_mul3x3, a, b))
        cols["det"].append(R.det3x3(ob.m33(a)))
        m, d = ob.m33(a), C.c_double()
        cols["inv_rc"].append(R.inv3x3(m, C.byref(d)))
        cols["inv"].append(ob.m33_np(m)); cols["inv_det"].append(d.value)
        v1, v2 = rng.normal(size=37), rng.normal(size=37)
        cols["v1"].append(v1); cols["v2"].append(v2)
        cols["cdot"].append(R.cdot(p(v1), p(v2), 37))
    for k, v in cols.items():
        g["dense_" + k] = np.array(v, dtype=np.int32 if k == "inv_rc" else np.float64)

    # inv3x3 on a singular matrix: return code and the matrix it leaves behind
    z = [[1, 2, 3], [2, 4, 6], [0, 1, 1]]
    m, d = ob.m33(z), C.c_double()
    g["singular_in"] = np.array(z, float)
    g["singular_rc"] = np.int32(R.inv3x3(m, C.byref(d)))
    g["singular_out"] = ob.m33_np(m)

    # fea_model.c stress / ctensor, lambda = 100, mu = 37.5 (fea_model.c:7-23 binds them per model)
    stress_t = C.CFUNCTYPE(None, C.POINTER(ob.RefModel), ob.M33, ob.M33)
    ctens_t = C.CFUNCTYPE(None, C.POINTER(ob.RefModel), ob.M33, ob.C4)
    for model in (0, 1):
        fm = ob.RefModel()
        fm.model = model
        fm.parameters[0], fm.parameters[1] = 100.0, 37.5
        fm.parameters_count = 2
        R.fea_model_init(C.byref(fm), model)
        ref_stress, ref_ctens = stress_t(fm.stress), ctens_t(fm.ctensor)
        rng = np.random.default_rng(7 + model)
        Fs, Ss, Cs = [], [], []
        for _ in range(200):
            F = np.eye(3) + 0.3 * rng.normal(size=(3, 3))
            if np.linalg.det(F) <= 0.05:
                continue
            s, c = ob.M33(), ob.C4()
            ref_stress(C.byref(fm), ob.m33(F), s)
            ref_ctens(C.byref(fm), ob.m33(F), c)
            Fs.append(F); Ss.append(ob.m33_np(s)); Cs.append(np.frombuffer(bytes(c), dtype=np.float64).reshape(3, 3, 3, 3))
        g[f"model{model}_F"], g[f"model{model}_stress"], g[f"model{model}_ctensor"] = np.array(Fs), np.array(Ss), np.array(Cs)

    out = os.path.join(ROOT, "tests", "golden", "leaf")
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, "reference_leaf.npz"), **g)
    print("wrote", os.path.join(out, "reference_leaf.npz"), {k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
