"""The rescalings of tests/guard_rescale.py on the CPU oracle: each one leaves the network's output as it is and moves exactly
the stage it names (the GPU sweep of the fp16-range guard, test_gpu_guard.py, relies on both)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_rescale as GR  # noqa: E402


@pytest.fixture(scope="module")
def base(oracle_model):
    from text2pos_amd import synthetic as S
    cells = S.make_cells(91, 6)
    out, amax = GR.activation_maxima(oracle_model, *cells)
    return cells, out, amax


@pytest.mark.parametrize("s", [2.0 ** -16, 2.0 ** 16], ids=["2^-16", "2^16"])
@pytest.mark.parametrize("row", list(GR.ROWS))
def test_rescaling_preserves_the_output_and_moves_its_stage(oracle_model, vocab, base, row, s):
    from oracle import model as OM
    (xyz, rgb, center, mean_rgb, cell_ptr), want, amax = base
    sd, rgb_s = GR.apply(oracle_model.state_dict(), rgb, row, s)
    om = OM.OracleCellRetrieval(vocab["classes"], vocab["colors"], vocab["words"], OM.default_args()).eval()
    om.load_state_dict(sd, strict=True)
    got, got_amax = GR.activation_maxima(om, xyz, rgb_s, center, mean_rgb, cell_ptr)
    assert (got - want).abs().max().item() < 1e-6, row
    assert amax[row] > 0.0
    assert got_amax[row] == amax[row] * s, (row, got_amax[row], amax[row])
    # the other stages stay where they were (up to the float32 rounding of the scaled path)
    for other, m in amax.items():
        if other != row and GR.ROWS[other].site != GR.ROWS[row].site:
            assert abs(got_amax[other] - m) <= 1e-5 * max(m, 1.0), (row, other, got_amax[other], m)
