"""The preconditions of tests/test_gpu_rainflow.py without a GPU, from the reference modes alone (T and T_s of the float64
restatement, the library's host tables): on its histories no stress row overflows a ring of 32 points and the bounds decide
at least 90 % of the rows; the step history on the damped bar overflows a ring of 4 points in at least a tenth of the rows
and not in all; and in the histories that need a second launch some row turns at the launch boundary."""
import numpy as np
import pytest

import rainflow_reference as rr
from rainflow_cases import (CASES, CHUNK, CHUNK_CASES, DEPTH, STEP_CASE, chunk_histories, count_all, histories, reference,
                            reference_rows)


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_depth_32_holds_every_row_and_the_bounds_decide_nine_in_ten(kind, m, correction):
    ref = reference(kind)
    for name, g, dt in histories(ref):
        h, e = reference_rows(kind, m, correction, g, dt)
        got = count_all(h, e, DEPTH)
        share = got["decided"].mean()
        print(f"{kind} {m} {name}: rows {h.shape[1]}, decided {share:.3f}, deepest stack {got['depth_used'].max()}, "
              f"cycles up to {got['n_cycles'].max()}")
        assert not (got["status"] & rr.OVERFLOW).any()
        assert share >= 0.9
        assert np.array_equal(got["depth_used"], count_all(h, None)["depth_used"])      # the unbounded count needs no more


def test_depth_4_overflows_in_some_rows_of_the_step_history():
    kind, m, correction = STEP_CASE
    name, g, dt = [x for x in histories(reference(kind)) if x[0] == "257 steps, step"][0]
    h, e = reference_rows(kind, m, correction, g, dt)
    got = count_all(h, e, 4)
    share = ((got["status"] & rr.OVERFLOW) != 0).mean()
    print(f"{kind} {m} {name} at depth 4: overflowed {share:.3f} of {h.shape[1]} rows, decided {got['decided'].mean():.3f}")
    assert 0.1 <= share < 1.0


@pytest.mark.parametrize("kind,m,correction", CHUNK_CASES)
def test_a_row_turns_at_the_launch_boundary(kind, m, correction):
    """A reversal at row CHUNK - 1 is confirmed by the first row of the second launch, one at row CHUNK by its second: the
    two tones have such rows on both stores.  Under the step every row has filled its ring of 32 points and dropped points
    from it before the second launch (on the fan, whose rows all turn together, none turns at the boundary itself)."""
    for name, g, dt in chunk_histories(reference(kind)):
        assert len(g) == CHUNK + 4
        h, _ = reference_rows(kind, m, correction, g, dt)
        at = [int(np.isin([CHUNK - 1, CHUNK], rr.reversal_indices(h[:, r])).any()) for r in range(h.shape[1])]
        early = count_all(h[:CHUNK], None, DEPTH)
        full = ((early["status"] & rr.OVERFLOW) != 0).mean()
        print(f"{kind} {m} {name}: {sum(at)} of {len(at)} rows turn at row {CHUNK - 1} or {CHUNK}; {full:.3f} overflow before it")
        if name == "two tones":
            assert sum(at) >= 1
        else:
            assert full == 1.0
