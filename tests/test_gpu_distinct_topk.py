"""t2p_topk_distinct (csrc/distinct.hip, include/t2p_select.h) through the C ABI, against tests/distinct_ref.py (proved on its own by
tests/test_distinct_ref_host.py).  No tolerances: the decision is comparisons of one float64 subtraction each, so indices, counts,
flags and score bits are compared for equality.
  exactness          idx, n_valid, exhausted = select_ref on the pool the GPU itself ranked; the scores are the pool's bits
  the definition     for every query with exhausted == 0 the result equals full_ref on the GPU's own full ranking (k = Nc)
  non-vacuous        full_ref's depth says which queries a pool is too short for: both kinds occur, and the short ones are flagged
Cells sit on a 10 m grid, every fifth on its predecessor's centre, every seventh with its predecessor's embedding (score ties).
D = 128; nq in {1, 3, 65}; Nc in {1, 31, 33, 700}; pools from the plain ranking (with and without conflict groups) and from
t2p_sim_topk_prior (lists that end in -inf entries)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import distinct_ref as R

pytestmark = pytest.mark.gpu

DIM, CELL, MAX_K = 128, 30.0, 1024
NQS, NCS = (1, 3, 65), (1, 31, 33, 700)
N_GROUPS = 3


def _dev():
    return torch.device("cuda:0")


def _up(a):
    return torch.tensor(np.asarray(a), device=_dev())


@functools.lru_cache(maxsize=None)
def scene(nq, nc):
    """(cells fp32 [nc, D], queries fp32 [nq, D], centres float64 [nc, 2], groups int32 [nc], prior xy [nq, 2], prior radius [nq],
    boxes [nc, 4]), read-only."""
    rng = np.random.default_rng(100 * nq + nc)
    c = rng.standard_normal((nc, DIM)).astype(np.float32)
    q = rng.standard_normal((nq, DIM)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c[7::7] = c[6::7][: len(c[7::7])]                        # identical embeddings: score ties in every query
    w = int(np.ceil(np.sqrt(nc)))
    at = rng.permutation(w * w)[:nc]
    xy = np.stack([(at % w) * 10.0, (at // w) * 10.0], axis=1).astype(np.float64)
    xy[4::5] = xy[3::5][: len(xy[4::5])]                     # cells that share a centre exactly
    group = rng.integers(0, N_GROUPS, nc).astype(np.int32)
    box = np.concatenate([xy - CELL / 2, xy + CELL / 2], axis=1)
    pxy = rng.uniform(0.0, 10.0 * w, (nq, 2))
    rad = np.array([(0.0, 25.0, 60.0, np.inf)[i % 4] for i in range(nq)])
    out = (c, q, xy, group, pxy, rad, box)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ranked(nq, nc, source, n):
    """The GPU's own ranking of the first n cells per query: (idx int64 [nq, n], score float64 [nq, n]) on the device.
    source: "plain" (t2p_sim_topk) or "prior" (t2p_sim_topk_prior with the scene's priors: lists that end at -inf)."""
    from text2pos_amd import ops
    c, q, xy, group, pxy, rad, box = scene(nq, nc)
    if source == "plain":
        return ops.sim_topk(_up(q), _up(c), n)
    return ops.sim_topk_prior(_up(q), _up(c), n, query_xy=_up(pxy), query_radius=_up(rad), cell_box=_up(box))


def select(pool_idx, pool_score, xy, group, sep, k, n_cells=None, index_offset=0):
    """t2p_topk_distinct through the C ABI on device tensors -> (rc, idx, score, n_valid, exhausted) as host arrays."""
    from text2pos_amd import _lib
    nq, pool = pool_idx.shape
    n_cells = xy.shape[0] if n_cells is None else n_cells
    dev = pool_idx.device
    idx = torch.full((nq, max(k, 1)), -7, dtype=torch.int64, device=dev)
    score = torch.full((nq, max(k, 1)), 7.0, dtype=torch.float64, device=dev)
    n_valid = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    exhausted = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    rc = _lib.lib().t2p_topk_distinct(p(pool_idx), p(pool_score), nq, pool, n_cells, index_offset, p(xy), p(group), float(sep), k, p(idx),
                                      p(score), p(n_valid), p(exhausted), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), score.cpu().numpy(), n_valid.cpu().numpy(), exhausted.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def definition(nq, nc, source, grouped, sep, k):
    """full_ref on the GPU's own full ranking (nc <= 1024): the score of every cell, scattered back from the ranking at k = nc."""
    _, _, xy, group, *_ = scene(nq, nc)
    fi, fs = (t.cpu().numpy() for t in ranked(nq, nc, source, nc))
    s = np.full((nq, nc), np.nan)
    np.put_along_axis(s, fi, fs, axis=1)
    assert not np.isnan(s).any()                             # the ranking at k = nc holds every cell once
    return R.full_ref(s, xy, group if grouped else None, sep, k)


def shapes(nc):
    """(pool, k) with k in {1, 2, 10, 64, pool} and pool in {k, 63, 64, 65, 128, 1024}, capped at nc."""
    out = set()
    for pool in {min(p, nc) for p in (63, 64, 65, 128, MAX_K)}:
        out |= {(pool, k) for k in (1, 2, 10, 64, pool) if k <= pool}
    out |= {(k, k) for k in (1, 2, 10, 64) if k <= nc}
    return sorted(out)


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("nq", NQS)
def test_selection_equals_the_reference_and_the_definition(nq, nc):
    _, _, xy, group, *_ = scene(nq, nc)
    dxy, dgroup = _up(xy), _up(group)
    kinds = {"deep enough": 0, "cut short": 0}
    for source, grouped in (("plain", False), ("plain", True), ("prior", True)):
        full_i, full_s = (t.cpu().numpy() for t in ranked(nq, nc, source, nc))
        for pool, k in shapes(nc):
            pi, ps = ranked(nq, nc, source, pool)
            hpi, hps = pi.cpu().numpy(), ps.cpu().numpy()
            # (the pool is the head of the full ranking, bit for bit: what makes the definition below the pool's definition)
            assert np.array_equal(hpi, full_i[:, :pool]) and np.array_equal(bits(hps), bits(full_s[:, :pool]))
            g = group if grouped else None
            rc, idx, score, n_valid, exhausted = select(pi, ps, dxy, dgroup if grouped else None, CELL, k)
            assert rc == 0
            want = R.select_ref(hpi, hps, xy, g, CELL, k, nc)
            what = (source, grouped, pool, k)
            assert np.array_equal(idx, want[0]) and np.array_equal(bits(score), bits(want[1])), what
            assert np.array_equal(n_valid, want[2]) and np.array_equal(exhausted, want[3]), what
            where = np.full((nq, nc), -1, dtype=np.int64)    # a cell's place in the query's pool (a pool names a cell once)
            np.put_along_axis(where, hpi, np.broadcast_to(np.arange(pool), (nq, pool)), axis=1)
            for qi in range(nq):                             # the scores are the pool's bits, at the accepted entries, in pool order
                n = n_valid[qi]
                at = where[qi, idx[qi, :n]]
                assert np.array_equal(bits(score[qi, :n]), bits(hps[qi, at])) and (np.diff(at) > 0).all()
            didx, dn, depth = definition(nq, nc, source, grouped, CELL, k)
            for qi in range(nq):
                n = n_valid[qi]
                if exhausted[qi] == 0:
                    assert n == dn[qi] and np.array_equal(idx[qi, :n], didx[qi, :n]), (what, qi)
                if depth[qi] <= pool:
                    assert exhausted[qi] == 0 and n == dn[qi]
                    kinds["deep enough"] += 1
                elif pool < nc and not np.isneginf(hps[qi]).any():
                    assert exhausted[qi] == 1 and n < k, (what, qi)
                    assert (idx[qi, n:] == hpi[qi, 0]).all() and np.isneginf(score[qi, n:]).all()       # the fill rule
                    assert np.array_equal(idx[qi, :n], didx[qi, :n])                                     # a prefix of the definition
                    kinds["cut short"] += 1
    assert kinds["deep enough"] > 0
    assert kinds["cut short"] > 0 or nc == 1                 # (one cell: every pool is the database)


def test_sep_zero_is_the_ranking_and_sep_inf_one_cell_per_group():
    from text2pos_amd import ops
    nq, nc = 65, 700
    c, q, xy, group, *_ = scene(nq, nc)
    dxy, dgroup = _up(xy), _up(group)
    for k, pool in ((1, 1), (10, 64), (64, 65), (130, 700)):
        pi, ps = ranked(nq, nc, "plain", pool)
        ti, ts = ops.sim_topk(_up(q), _up(c), k)
        for g in (None, dgroup):
            rc, idx, score, n_valid, exhausted = select(pi, ps, dxy, g, 0.0, k)
            assert rc == 0 and np.array_equal(idx, ti.cpu().numpy()) and np.array_equal(bits(score), bits(ts.cpu().numpy()))
            assert (n_valid == k).all() and (exhausted == 0).all()
    pi, ps = ranked(nq, nc, "plain", 128)
    hpi = pi.cpu().numpy()
    rc, idx, score, n_valid, exhausted = select(pi, ps, dxy, dgroup, np.inf, N_GROUPS + 1)
    assert rc == 0 and (n_valid == N_GROUPS).all() and (exhausted == 1).all()       # a fourth group might lie beyond the pool
    for qi in range(nq):
        got = idx[qi, :N_GROUPS]
        assert sorted(group[got].tolist()) == list(range(N_GROUPS))
        assert got.tolist() == [hpi[qi][np.flatnonzero(group[hpi[qi]] == gg)[0]] for gg in group[got]]     # each the best of its group
        assert (idx[qi, N_GROUPS:] == hpi[qi, 0]).all() and np.isneginf(score[qi, N_GROUPS:]).all()
    rc, idx, _, n_valid, exhausted = select(pi, ps, dxy, None, np.inf, 2)           # no groups: the best cell alone
    assert rc == 0 and (n_valid == 1).all() and np.array_equal(idx[:, 0], hpi[:, 0]) and (exhausted == 1).all()
    pi, ps = ranked(nq, nc, "plain", nc)                                            # the pool is the database: never exhausted
    rc, _, _, n_valid, exhausted = select(pi, ps, dxy, None, np.inf, 2)
    assert rc == 0 and (n_valid == 1).all() and (exhausted == 0).all()


def test_index_offset_and_repeatability():
    from text2pos_amd import ops
    nq, nc, pool, k, off = 65, 700, 128, 10, 5000
    c, q, xy, group, *_ = scene(nq, nc)
    dxy, dgroup = _up(xy), _up(group)
    pi, ps = ranked(nq, nc, "plain", pool)
    oi, os_ = ops.sim_topk(_up(q), _up(c), pool, off)
    assert torch.equal(oi, pi + off)
    base = select(pi, ps, dxy, dgroup, CELL, k)
    again = select(pi, ps, dxy, dgroup, CELL, k)
    shifted = select(oi, os_, dxy, dgroup, CELL, k, index_offset=off)
    assert base[0] == 0 and shifted[0] == 0
    assert all(np.array_equal(a, b) for a, b in zip(base[1:], again[1:]))
    assert np.array_equal(shifted[1], base[1] + off) and all(np.array_equal(a, b) for a, b in zip(base[2:], shifted[2:]))
    # the Python wrappers give the same selection
    got = ops.topk_distinct(oi, os_, dxy, CELL, k, cell_group=dgroup, index_offset=off)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, shifted[1:]))
    import text2pos_amd as t2p
    got = t2p.retrieve_topk_distinct(_up(c), _up(q), k, np.array(xy), CELL, pool=pool, index_offset=off, cell_groups=np.array(group),
                                     query_groups=np.full(nq, 1, dtype=np.int32))
    gi, gs = ops.sim_topk_grouped(_up(q), _up(c), _up(np.full(nq, 1, dtype=np.int32)), dgroup, pool, off)
    want = select(gi, gs, dxy, dgroup, CELL, k, index_offset=off)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want[1:]))
    assert (group[want[1][want[3][:, None] > np.arange(k)] - off] == 1).all()      # masked cells (other groups) are never selected
    assert t2p.retrieve_topk_distinct(_up(c), _up(q), k, np.array(xy), CELL)[0].shape == (nq, k)      # default pool: min(700, 1024, 320)


def test_a_pool_index_outside_the_table_is_marked_not_read():
    from text2pos_amd import ops
    nq, nc, pool, k = 65, 700, 128, 10
    _, _, xy, group, *_ = scene(nq, nc)
    dxy, dgroup = _up(xy), _up(group)
    pi, ps = (t.clone() for t in ranked(nq, nc, "prior", pool))
    clean = select(pi, ps, dxy, dgroup, CELL, k)
    hps = ps.cpu().numpy()
    masked_q = int(np.flatnonzero(np.isneginf(hps[:, -1]) & np.isfinite(hps[:, 0]))[0])
    assert np.isfinite(hps[[7, 11, 63]]).all() and masked_q not in (7, 11, 63)      # (every fourth query's prior has r = inf)
    pi[masked_q, -1] = 1 << 40                               # at -inf: never looked up, so not an error
    pi[7, 70] = nc                                           # one past the end, behind the first chunk
    pi[63, 0] = -1
    pi[11, pool - 1] = 1 << 40                               # the last entry of the pool
    rc, idx, score, n_valid, exhausted = select(pi, ps, dxy, dgroup, CELL, k)
    assert rc == 0
    marked = [7, 11, 63]
    assert np.flatnonzero(n_valid < 0).tolist() == marked and (n_valid[marked] == -1).all() and (exhausted[marked] == 0).all()
    assert (idx[marked] == -1).all() and np.isneginf(score[marked]).all()
    rest = np.setdiff1d(np.arange(nq), marked)
    assert np.array_equal(idx[rest], clean[1][rest]) and np.array_equal(bits(score[rest]), bits(clean[2][rest]))     # the neighbours: untouched
    assert np.array_equal(n_valid[rest], clean[3][rest]) and np.array_equal(exhausted[rest], clean[4][rest])
    with pytest.raises(IndexError, match=r"query 7\b"):
        ops.topk_distinct(pi, ps, dxy, CELL, k, cell_group=dgroup)
    out = ops.topk_distinct(pi, ps, dxy, CELL, k, cell_group=dgroup, check=False)
    assert np.array_equal(out[2].cpu().numpy(), n_valid)
    with pytest.raises(IndexError, match=r"query 0\b"):                              # a table shorter than the ranking's cells
        ops.topk_distinct(*ranked(nq, nc, "plain", pool), dxy[:300].contiguous(), CELL, k)


def test_refused_arguments_name_the_argument():
    from text2pos_amd import _lib, ops
    import text2pos_amd as t2p
    nq, nc, pool = 3, 33, 33
    c, q, xy, group, *_ = scene(nq, nc)
    dxy, dgroup = _up(xy), _up(group)
    pi, ps = ranked(nq, nc, "plain", pool)
    err = lambda: _lib.lib().t2p_last_error().decode()
    for kw, word in ((dict(k=0), "k=0"), (dict(k=-3), "k=-3"), (dict(k=34), "k=34 exceeds pool=33"), (dict(sep=-0.5), "sep=-0.5"),
                     (dict(sep=float("nan")), "sep="), (dict(n_cells=0), "n_cells")):
        args = dict(sep=CELL, k=4, n_cells=None)
        args.update(kw)
        rc, idx, _, n_valid, _ = select(pi, ps, dxy, dgroup, args["sep"], args["k"], n_cells=args["n_cells"])
        assert rc == -1 and err().startswith("topk_distinct:") and word in err(), (kw, rc, err())
        assert (idx == -7).all() and (n_valid == -7).all()                           # nothing was launched
    big = torch.zeros((1, MAX_K + 1), dtype=torch.int64, device=_dev()), torch.zeros((1, MAX_K + 1), dtype=torch.float64, device=_dev())
    assert select(*big, dxy, None, CELL, 4)[0] == -1 and "pool=1025" in err()
    from text2pos_amd._lib import T2PError
    with pytest.raises(T2PError, match="k=34 exceeds pool=33"):
        ops.topk_distinct(pi, ps, dxy, CELL, 34)
    with pytest.raises(RuntimeError, match="pool_score"):
        ops.topk_distinct(pi, ps.to(torch.float32), dxy, CELL, 4)
    with pytest.raises(RuntimeError, match="expected"):
        ops.topk_distinct(pi, ps, dxy, CELL, 4, cell_group=dgroup[:5].contiguous())
    for kw, word in ((dict(sep=-1.0), "must be >= 0"), (dict(sep=float("nan")), "must be >= 0"), (dict(pool=3), r"pool=3 outside \[k"),
                     (dict(pool=34), "pool=34 outside"), (dict(k=34), "exceeds the 33 cells")):
        args = dict(k=4, sep=CELL, pool=None)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            t2p.retrieve_topk_distinct(_up(c), _up(q), args["k"], np.array(xy), args["sep"], pool=args["pool"])
    bad = xy.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match=r"cell_xy\[17\]"):
        t2p.retrieve_topk_distinct(_up(c), _up(q), 4, bad, CELL)
