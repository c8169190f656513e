"""No GPU: the NumPy restatement of the SA range balancing that tests/test_gpu_balance.py holds t2p_sa_balance to
(tests/balance_ref.py) against a brute-force loop, so the reference is itself checked."""
import numpy as np
import pytest

import balance_ref as R


@pytest.mark.parametrize("n_rows,tile_rows,n_wg", [
    ([0, 0, 65, 0, 0, 0, 4224, 1, 0, 0, 64, 63, 0], 64, 5),          # zeros in runs: repeated prefixes, the FIRST index wins
    ([33, 32, 31, 0, 4224, 4224, 7], 32, 16),                        # more workgroups than objects
    ([0, 0, 0, 0], 64, 3),                                           # nothing to do: every bound but the last is 0
])
def test_restatement_equals_brute_force(n_rows, tile_rows, n_wg):
    c = np.array(n_rows, dtype=np.uint16)
    prefix, bounds = R.balance(c, tile_rows, n_wg)
    bprefix, bbounds = R.balance_brute(c, tile_rows, n_wg)
    assert prefix.dtype == np.int64 and np.array_equal(prefix, bprefix)
    assert np.array_equal(bounds, bbounds)
    assert bounds[0] == 0 and bounds[-1] == len(c) and (np.diff(bounds) >= 0).all()


def test_generated_counts_cover_the_cases():
    for kind in ("uniform", "zero", "full", "runs"):
        c = R.counts(kind, 1025)
        assert c.dtype == np.uint16 and c.shape == (1025,) and int(c.max()) <= R.MAX_ROWS
    assert R.counts("full", 3).tolist() == [R.MAX_ROWS] * 3 and not R.counts("zero", 3).any()
    runs = R.counts("runs", 8191)
    assert not runs[:8191 // 7].any() and runs.any()
    p, b = R.balance(runs, 64, 256)
    q, d = R.balance_brute(runs, 64, 256)
    assert np.array_equal(p, q) and np.array_equal(b, d)
