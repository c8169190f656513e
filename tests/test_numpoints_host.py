"""pointnet_numpoints at the C boundary, without a GPU: t2p_encode_cells accepts 8 to 256 points per object and refuses the rest
with a message that names the range, before it touches a device pointer or launches anything."""
import ctypes as C

import pytest

import text2pos_amd  # noqa: F401
from text2pos_amd import _lib, ops


def _call(n_pts):
    """t2p_encode_cells with a valid config for n_pts and NULL everything else: (return code, error message)."""
    L = _lib.lib()
    cfg = ops.make_cell_config(n_pts=n_pts)
    rc = L.t2p_encode_cells(None, None, None, None, None, None, 0, 1, None, C.byref(cfg), None, None, None, 0, None)
    return rc, L.t2p_last_error().decode()


@pytest.mark.parametrize("n_pts", [8, 9, 31, 64, 100, 128, 200, 255, 256])
def test_built_sizes_pass_the_config_check(n_pts):
    rc, msg = _call(n_pts)
    assert rc != 0 and "NULL argument" in msg, msg          # refused later, for the missing buffers only
    assert "not built" not in msg


@pytest.mark.parametrize("n_pts", [0, 7, 257, 512, 1024])
def test_other_sizes_are_refused_with_the_range(n_pts):
    rc, msg = _call(n_pts)
    assert rc == -3, (rc, msg)                               # T2P_E_UNSUPPORTED
    assert f"n_pts={n_pts}" in msg and "8 <= n_pts <= 256" in msg, msg


@pytest.mark.parametrize("n_pts", [8, 100, 128, 256])
def test_workspace_follows_the_point_count(n_pts):
    L = _lib.lib()
    sizes = [L.t2p_encode_cells_workspace_bytes(5000, 300, C.byref(ops.make_cell_config(n_pts=p))) for p in (n_pts, 256)]
    assert 0 < sizes[0] <= sizes[1]
