"""The cut rule of preconditioner 2's aggregates (feahip_host_coarse_aggregates): no device needed.

Rank r cuts its n_r owned rows into m_r = min(m, max(1, n_r // 64)) contiguous runs [floor(j n_r / m_r),
floor((j + 1) n_r / m_r))."""
import numpy as np
import pytest

import feahip


@pytest.mark.parametrize("n_owned", [1, 63, 64, 127, 128, 777, 778, 1000, 4096, 4097, 123457])
@pytest.mark.parametrize("m", [1, 3, 12, 16])
def test_cuts_are_contiguous_exhaustive_and_balanced(n_owned, m):
    first = feahip.host_coarse_aggregates(n_owned, m)
    mr = len(first) - 1
    assert mr == min(m, max(1, n_owned // 64))
    assert first[0] == 0 and first[-1] == n_owned                     # exhaustive
    sizes = np.diff(first)
    assert np.all(sizes >= 1)                                         # contiguous, none empty
    assert sizes.max() - sizes.min() <= 1                             # balanced within one row
    assert np.array_equal(first, np.arange(mr + 1) * n_owned // mr)  # the rule, restated


def test_small_slabs_get_fewer_aggregates():
    """m_r for small n_owned: one aggregate below 128 rows, then one per 64 rows up to the cap."""
    for n, want in [(1, 1), (64, 1), (127, 1), (128, 2), (191, 2), (192, 3), (64 * 16 - 1, 15), (64 * 16, 16), (10 ** 6, 16)]:
        assert len(feahip.host_coarse_aggregates(n, 16)) - 1 == want, n
    assert len(feahip.host_coarse_aggregates(10 ** 6, 128)) - 1 == 128


def test_bad_arguments_are_refused():
    for n, m in [(0, 4), (-3, 4), (100, 0)]:
        with pytest.raises(feahip.FeaHipError):
            feahip.host_coarse_aggregates(n, m)
