"""t2p_sa_balance (csrc/ws_sa.hip: k_balance, the device code of the encoder's range balancing) against the NumPy int64
restatement of its two definitions (tests/balance_ref.py, itself held to a brute-force loop by tests/test_balance_host.py).
Integers: array_equal."""
import functools

import numpy as np
import pytest
import torch

import balance_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 1023, 1025, 8191, 65000]     # below / at a wave, around the block, around one chunk of 8,192, many chunks
KINDS = ["uniform", "zero", "full", "runs"]


@functools.lru_cache(maxsize=None)
def _counts(kind, n):
    c = R.counts(kind, n)
    c.setflags(write=False)
    return c, torch.from_numpy(c.view(np.int16).copy()).to("cuda:0")


def _run(dev_counts, tile_rows, n_wg):
    from text2pos_amd import ops
    prefix, bounds = ops.sa_balance(dev_counts, tile_rows, n_wg)
    return prefix.cpu().numpy().astype(np.int64), bounds.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_balance_equals_the_restatement(n, kind):
    c, dc = _counts(kind, n)
    for tile_rows in (32, 64):
        for n_wg in (1, 7, 256, 1024):            # n < n_wg included (n = 1, 63, 64 and 1023)
            prefix, bounds = _run(dc, tile_rows, n_wg)
            wprefix, wbounds = R.balance(c, tile_rows, n_wg)
            assert np.array_equal(prefix, wprefix), (n, kind, tile_rows, n_wg)
            assert np.array_equal(bounds, wbounds), (n, kind, tile_rows, n_wg)


def test_unaligned_arrays_give_the_same_integers():
    """Counts and prefixes that do not start on a 16-byte boundary take the element-wise loads and stores."""
    from text2pos_amd import _lib as L, ops
    c, _ = _counts("runs", 8191)
    n, n_wg = len(c) - 3, 256
    buf = torch.from_numpy(c.view(np.int16).copy()).to("cuda:0")
    view = buf[3:]
    pbuf = torch.empty((n + 2,), dtype=torch.int32, device="cuda:0")
    bounds = torch.empty((n_wg + 1,), dtype=torch.int32, device="cuda:0")
    assert view.data_ptr() % 16 == 6 and pbuf[1:].data_ptr() % 16 == 4
    L.check(L.lib().t2p_sa_balance(ops._ptr(view), n, 64, n_wg, ops._ptr(pbuf[1:]), ops._ptr(bounds), ops._stream(buf.device)),
            "t2p_sa_balance")
    wprefix, wbounds = R.balance(c[3:], 64, n_wg)
    assert np.array_equal(pbuf[1:].cpu().numpy(), wprefix) and np.array_equal(bounds.cpu().numpy(), wbounds)


def test_empty_call_and_refusals():
    from text2pos_amd import _lib as L, ops
    prefix, bounds = _run(torch.empty((0,), dtype=torch.int16, device="cuda:0"), 64, 7)
    assert prefix.tolist() == [0] and bounds.tolist() == [0] * 8
    _, dc = _counts("uniform", 64)
    for tile_rows, n_wg in ((0, 4), (64, 0)):
        with pytest.raises(L.T2PError):
            ops.sa_balance(dc, tile_rows, n_wg)
