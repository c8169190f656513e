"""The cell encoder's three entries run the same stages (csrc/cell_encoder.hip).

t2p_pointnet2_forward runs the trunk stages, t2p_encode_cells with objects_only the trunk and the object encoder, the full call
the cell head behind them.  An entry that stops early launches the same kernels with the same arguments as the longer one up to
where it stops, so what it hands back equals the longer call's trace of that stage bit for bit - no tolerance anywhere.

One cell of 33 objects (an odd count: the 32-row tiles have a ragged end), at 256 points per object (the specialised SA kernels)
and at 100 (the stream kernel), on the f16x3 and the fp32 path, with the fp16-range guard word attached: it must read 0 after
every call.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_OBJ = 33
FEATURES = ("features0", "features1", "features2")
CASES = [(256, "f16x3"), (256, "fp32"), (100, "f16x3"), (100, "fp32")]
_memo = {}


def _runs(vocab, oracle_model, n_pts, precision):
    """Every entry once on the same cell: dict(trunk, full=(out, trace), plain=out, objects, guard={call: word})."""
    if (n_pts, precision) in _memo:
        return _memo[(n_pts, precision)]
    import text2pos_amd as t2p
    from text2pos_amd import ops
    from text2pos_amd import synthetic as S
    dev = torch.device("cuda:0")
    hm = t2p.CellRetrievalNetwork(vocab["classes"], vocab["colors"], vocab["words"], S.default_args(pointnet_numpoints=n_pts),
                                  precision=precision)
    hm.load_state_dict(oracle_model.state_dict(), strict=True)
    hm = hm.to(dev).eval()
    xyz, rgb, center, mean_rgb, cell_ptr = S.make_cells(500 + n_pts, 1, fixed_n=N_OBJ, n_pts=n_pts)
    assert xyz.shape == (N_OBJ, n_pts, 3) and list(cell_ptr) == [0, N_OBJ]
    args = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xyz, rgb, center, mean_rgb)]
    pn = hm.object_encoder.pointnet.eval()
    pn.precision = precision
    r, guard = {}, {}

    def word(model):     # the sticky guard word of the call just issued (0 on the fp32 path: no word is attached)
        torch.cuda.synchronize()
        return model.overflow_detected()

    with torch.no_grad():
        r["full"] = hm.encode_objects_packed(*args, cell_ptr, want_trace=FEATURES + ("obj_emb",), check_overflow=False)
        guard["full call with trace"] = word(hm)
        r["plain"] = hm.encode_objects_packed(*args, cell_ptr, check_overflow=False)
        guard["full call"] = word(hm)
        cfg = hm._cell_config(n_pts)
        cfg.objects_only = 1
        r["objects"] = ops.encode_cells(*args, cell_ptr, torch.from_numpy(cell_ptr).to(dev), hm._cell_pack(), cfg)
        guard["objects_only"] = word(hm)
        r["trunk"] = pn.forward_packed(args[0], args[1])      # (raises on a guard code; the word is read again below)
        guard["trunk"] = word(pn)
    r["guard"] = guard
    _memo[(n_pts, precision)] = r
    return r


@pytest.mark.parametrize("n_pts,precision", CASES)
def test_trunk_entry_equals_the_encoders_trunk(vocab, oracle_model, n_pts, precision):
    r = _runs(vocab, oracle_model, n_pts, precision)
    for k in FEATURES:
        assert torch.equal(getattr(r["trunk"], k), r["full"][1][k]), f"{k} at {n_pts} points, {precision}"


@pytest.mark.parametrize("n_pts,precision", CASES)
def test_objects_only_and_traces_leave_the_stages_alone(vocab, oracle_model, n_pts, precision):
    r = _runs(vocab, oracle_model, n_pts, precision)
    assert r["objects"].shape == (N_OBJ, 256)
    assert torch.equal(r["objects"], r["full"][1]["obj_emb"]), f"obj_emb at {n_pts} points, {precision}"
    assert torch.equal(r["full"][0], r["plain"]), f"cell embedding with and without a trace at {n_pts} points, {precision}"


@pytest.mark.parametrize("n_pts,precision", CASES)
def test_guard_word_stays_clear(vocab, oracle_model, n_pts, precision):
    r = _runs(vocab, oracle_model, n_pts, precision)
    assert all(code == 0 for code in r["guard"].values()), r["guard"]
