"""The colour / position encoders at 16,384 rows and more (csrc/small_kernels.hip: k_mlp3_rows, a lane per row with the weights in
SGPRs) against the same rows encoded in pieces of fewer than 16,384 (k_mlp3_norm<8>, whose arithmetic it must repeat bit for bit)
and against the float64 oracle.  The kernel is reached through t2p_encode_cells with a single feature and objects_only, which
returns the encoder's concat slot un-merged (models/object_encoder.py:137-140)."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LARGE = 16384          # launch_mlp3_norm's threshold
N_PTS = 8              # the PointNet++ does not run without the "class" feature; its (unused) inputs stay small


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _models(feature, dim):
    """(oracle encoder in float64, HIP model) with one feature.  Both layers' folded biases are negative (Linear bias = the BN's
    running mean, BN bias < 0), so the zero vector gives an all-zero hidden layer and an all-zero output: the norm clamp."""
    import text2pos_amd as t2p
    from text2pos_amd import synthetic as S
    from oracle import model as OM
    classes, words = S.LABELS + ["pad"], S.known_words()
    kw = dict(use_features=[feature], embed_dim=dim, pointnet_numpoints=N_PTS)
    torch.manual_seed(77 + dim)
    om = OM.OracleCellRetrieval(classes, S.COLOR_NAMES, words, OM.default_args(**kw)).eval()
    OM.randomize_bn_stats(om)
    enc = om.object_encoder.color_encoder if feature == "color" else om.object_encoder.pos_encoder
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for layer in enc:
            lin, bn = layer[0], layer[1]
            lin.bias.copy_(bn.running_mean)
            bn.bias.copy_(-0.02 - 0.1 * torch.rand(bn.num_features, generator=g))
    hm = t2p.CellRetrievalNetwork(classes, S.COLOR_NAMES, words, S.default_args(**kw))
    hm.load_state_dict(om.state_dict(), strict=True)
    return copy.deepcopy(enc).double().eval(), hm.to(_dev()).eval()


@functools.lru_cache(maxsize=None)
def _rows(n):
    """[n, 3] inputs: normal values of a few sizes, row 0 and row n - 1 zero vectors."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((n, 3)) * rng.choice([0.05, 1.0, 4.0], (n, 1))).astype(np.float32)
    x[0] = 0.0
    x[n - 1] = 0.0
    x.setflags(write=False)
    return x


def _encode(hm, feature, x, chunk_objects=0):
    """ObjectEncoder.forward with the single feature `feature` on the rows x (one object per cell) -> ([n, D], profile report)."""
    from text2pos_amd import ops
    n, dev = x.shape[0], _dev()
    pts = torch.zeros((n, N_PTS, 3), device=dev)
    rows = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    other = torch.zeros((n, 3), device=dev)
    center, mean_rgb = (other, rows) if feature == "color" else (rows, other)
    cell_ptr = np.arange(n + 1, dtype=np.int32)
    cfg = hm._cell_config(N_PTS, chunk_objects=chunk_objects)
    cfg.objects_only = 1
    torch.cuda.synchronize()
    ops.profile_report()
    ops.profile_enable(True)
    try:
        with torch.no_grad():
            out = ops.encode_cells(pts, pts, center, mean_rgb, cell_ptr, torch.from_numpy(cell_ptr).to(dev), hm._cell_pack(), cfg)
    finally:
        ops.profile_enable(False)
    return out, ops.profile_report()


@pytest.mark.parametrize("feature", ["color", "position"])
@pytest.mark.parametrize("dim", [128, 256, 384])
def test_large_call_repeats_the_small_kernels_bits(dim, feature):
    enc64, hm = _models(feature, dim)
    for n in (LARGE, LARGE + 33):          # the smallest large call; one whose last block and last wave are ragged
        x = _rows(n)
        out, rep = _encode(hm, feature, x)
        assert out.shape == (n, dim) and rep["mlp3_norm"][0] == 1, rep
        pieces, prep = _encode(hm, feature, x, chunk_objects=5000)             # 4 chunks of at most 5,000 rows: k_mlp3_norm<8>
        assert prep["mlp3_norm"][0] == -(-n // 5000)
        assert torch.equal(out.view(torch.int32), pieces.view(torch.int32)), (dim, feature, n)
        # float64 oracle on 256 of the rows (both ends, the zero vectors included)
        pick = np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), np.random.default_rng(1).integers(0, n, 128)]))[:256]
        with torch.no_grad():
            xin = torch.from_numpy(x[pick]).double()
            hidden = enc64[0](xin)
            want = torch.nn.functional.normalize(enc64(xin), dim=-1)
        got = out[torch.from_numpy(pick).to(_dev())].cpu().double()
        err = (got - want).abs().max().item()
        print(f"D={dim} {feature} n={n}: max|out - float64 oracle| = {err:.2e}")
        assert err < 1e-6
        # the inputs do what they are there for: exact zeros in the hidden layer and in the outputs, and the clamp on the zero rows
        assert (hidden == 0).any() and (hidden > 0).any() and (want == 0).any() and (want > 0).any()
        assert (hidden[0] == 0).all() and (want[0] == 0).all()
        o = out.cpu()
        assert (o[0] == 0).all() and (o[n - 1] == 0).all() and (o == 0).any() and torch.isfinite(o).all()
        norms = o[1:n - 1].double().norm(dim=-1)
        assert ((norms - 1).abs() < 1e-5).logical_or(norms == 0).all()


def test_row_count_below_the_threshold_stays_on_the_small_kernel():
    """16,383 rows in one call equal the same rows in pieces too (both on k_mlp3_norm<8>): the comparison above tests the kernels,
    not the chunking."""
    _, hm = _models("color", 256)
    x = _rows(LARGE + 33)[:LARGE - 1]
    out, rep = _encode(hm, "color", x)
    pieces, _ = _encode(hm, "color", x, chunk_objects=5000)
    assert rep["mlp3_norm"][0] == 1 and torch.equal(out.view(torch.int32), pieces.view(torch.int32))
