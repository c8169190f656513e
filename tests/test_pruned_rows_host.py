"""SA levels 2 and 3 without an FPS of their own and without the edge rows of repeated dense points, restated in NumPy
(csrc/sample_group.hip: k_sample_group<true, true> + k_build_rows; include/t2p.h: t2p_group_rows_pruned).

The prefix rule.  Level l + 1 samples from level l's picks in pick order, starting at index 0, so its FPS picks the prefix: with k1
the first tail centroid of level 1 (c > 0, fps_idx[c] == 0; 128 when there is none), fps_idx[l][c] = c below k1 and 0 from there on
for l = 1, 2, and the centroid positions of levels 2 and 3 are the first 64 / 32 of level 1's pick positions.
The pruning.  Dense point j >= k_prev of level 2 / 3 (k_prev = k1 / min(k1, 64)) is a tail centroid of the level below: it repeats
dense point 0, and its rows leave the lists.  The repeats are a suffix of the index order, so "first 32 hits, then drop them" is
"first 32 hits among the dense points below k_prev".

Both are checked against the real FPS / ball query of profiles/tail_rows_census.py (`level`, the pinned semantics of the kernel) on
the first 96 objects of the benchmark's stream and on objects of k distinct positions repeated to 256 points.  Every comparison is
equality.  tests/test_gpu_pruned_rows.py applies the same restatement (`expected_lists`) to the kernel's own tables.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from text2pos_amd import _lib, synthetic as S  # noqa: E402

RADII = (0.2, 0.3, 0.4)
N_CENT = (128, 64, 32)
TAIL_CODE = 64
K_DISTINCT = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256]
N_STREAM = 96
SEED = 20220002


def repeated_objects():
    """xyz, rgb [13, 256, 3]: k distinct positions (and colours) repeated to 256 points, point 0 first."""
    rng = np.random.default_rng(2025)
    xs, cs = [], []
    for k in K_DISTINCT:
        x = rng.uniform(-0.5, 0.5, (256, 3)).astype(np.float32)
        c = rng.uniform(0, 1, (256, 3)).astype(np.float32)
        idx = np.arange(256) % k
        xs.append(x[idx])
        cs.append(c[idx])
    return np.stack(xs), np.stack(cs)


def stream_objects():
    xyz, rgb, _, _ = S.make_objects(SEED, 0, N_STREAM)
    return xyz.astype(np.float32), rgb.astype(np.float32)


def first_tail(fps) -> int:
    t = np.flatnonzero((np.asarray(fps) == 0) & (np.arange(len(fps)) > 0))
    return int(t[0]) if len(t) else len(fps)


def k_prev_of(level: int, k1: int) -> int:
    """Dense points of level index `level` (1, 2) from k_prev on repeat dense point 0."""
    return k1 if level == 1 else min(k1, N_CENT[1])


def repeat_flags(pos, rgb):
    """k_build_rows' repeat test (repeat_flags in csrc/sample_group.hip): a 1,024-slot table keeps the lowest index per coordinate
    hash; a point repeats when its slot holds a lower index with the same xyz and rgb bits (a slot taken by another point of the
    same hash leaves a repeat undetected)."""
    b = np.ascontiguousarray(pos, dtype=np.float32).view(np.uint32).astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    k = (b[:, 0] * np.uint64(0x9E3779B1)) & m
    k = ((k ^ (k >> np.uint64(15))) + ((b[:, 1] * np.uint64(0x85EBCA77)) & m)) & m
    k = ((k ^ (k >> np.uint64(13))) + ((b[:, 2] * np.uint64(0xC2B2AE3D)) & m)) & m
    h = ((k ^ (k >> np.uint64(16))) & np.uint64(1023)).astype(np.int64)
    slot = {}
    for i in range(len(h)):
        slot.setdefault(int(h[i]), i)
    key = np.concatenate([pos, rgb], axis=1).astype(np.float32).view(np.uint32)
    rep = np.zeros(len(h), dtype=bool)
    for i in range(len(h)):
        f = slot[int(h[i])]
        rep[i] = f != i and np.array_equal(key[f], key[i])
    return rep


def list_rows(level, hits, k1, self_loops=True, share=False, prune=True, rep=None):
    """The u16 rows of one object's list at level index `level` from its capped hits per centroid (ascending dense indices).
    Level 0: the hits on repeated points (rep) leave.  Levels 1, 2: with `prune` the hits on dense points >= k_prev leave; with
    `share` (level 1) the first tail centroid lists its hits under TAIL_CODE and the later ones keep their self-loop row only."""
    rows = []
    k_prev = k_prev_of(level, k1) if (prune and level > 0) else 1 << 30
    for c in range(len(hits)):
        tail = share and level == 1 and c >= k1
        if not tail or c == k1:
            tag = TAIL_CODE if tail else c
            rows += [(tag << 8) | int(j) for j in hits[c] if j < k_prev and not (level == 0 and rep is not None and rep[j])]
        if self_loops:
            rows.append(((c | 0x80) << 8) | c)
    return rows


def expected_lists(fps, nbr, cnt, pos, rgb, self_loops=True, share=False, prune=True):
    """[3 lists of u16 rows] of one object from its FPS indices / neighbour tables / counts (ops.sample_group's layout)."""
    k1 = first_tail(fps[0])
    rep = repeat_flags(pos, rgb)
    return [list_rows(l, [nbr[l][c, :cnt[l][c]] for c in range(N_CENT[l])], k1, self_loops, share, prune, rep) for l in range(3)]


def _hits_uncapped(pos, cpos, r):
    r2 = np.float32(r) * np.float32(r)
    d = pos - cpos
    return np.flatnonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < r2)


@pytest.fixture(scope="module")
def census():
    """Per object: (pos, [fps of the 3 levels by real FPS], [dense positions of the 3 levels])."""
    import tail_rows_census as T
    sx, _ = stream_objects()
    rx, _ = repeated_objects()
    out = []
    for pos in list(sx) + list(rx):
        fps, dense = [], []
        p = pos
        for l in range(3):
            f, _ = T.level(p, RADII[l])
            fps.append(f)
            dense.append(p)
            p = p[f]
        out.append((pos, fps, dense))
    return out


def test_the_objects_cover_the_tails(census):
    k1 = np.array([first_tail(fps[0]) for _, fps, _ in census[:N_STREAM]])
    counts = (int((k1 < 128).sum()), int((k1 < 64).sum()), int((k1 < 32).sum()))
    print("stream objects with k1 < 128 / 64 / 32:", counts)
    assert counts[0] >= 20 and counts[1] >= 10 and counts[2] >= 2, counts
    for k, (pos, fps, _) in zip(K_DISTINCT, census[N_STREAM:]):
        assert first_tail(fps[0]) == min(k, 128), f"{k} distinct positions"


def test_levels_2_and_3_pick_the_prefix(census):
    for o, (pos, fps, dense) in enumerate(census):
        k1 = first_tail(fps[0])
        for l in (1, 2):
            c = np.arange(N_CENT[l])
            assert np.array_equal(fps[l], np.where(c < k1, c, 0)), f"object {o}: fps_idx of level {l + 1}"
        p1 = pos[fps[0]]                      # level 1's pick positions, tail entries included
        assert np.array_equal(dense[1].view(np.uint32), p1.view(np.uint32))
        assert np.array_equal(dense[2].view(np.uint32), p1[:64].view(np.uint32)), f"object {o}: level-2 centroid positions"
        assert np.array_equal(dense[2][fps[2]].view(np.uint32), p1[:32].view(np.uint32)), f"object {o}: level-3 centroid positions"


def test_cap_then_drop_is_the_first_32_below_k_prev(census):
    import tail_rows_census as T
    shorter = 0
    for o, (pos, fps, dense) in enumerate(census):
        k1 = first_tail(fps[0])
        p1 = pos[fps[0]]
        today, pruned = 0, 0
        for l in (1, 2):
            kp = k_prev_of(l, k1)
            capped = T.capped_hits(dense[l], fps[l], RADII[l])
            # the lane-per-centroid form: centroids are the prefix of level 1's picks, the loop stops at k_prev
            direct = [h[h < kp][:32] for h in (_hits_uncapped(p1[:N_CENT[l - 1]], p1[c], RADII[l]) for c in range(N_CENT[l]))]
            for c in range(N_CENT[l]):
                drop = capped[c][capped[c] < kp]
                assert np.array_equal(drop, direct[c]), f"object {o} level {l + 1} centroid {c}"
                if (capped[c] >= kp).any():      # a repeat inside the cap: dense point 0, the point it repeats, is listed before it
                    assert 0 in drop, f"object {o} level {l + 1} centroid {c}: a repeat is listed without dense point 0"
            for share in (False, True):
                full = list_rows(l, capped, k1, share=share, prune=False)
                cut = list_rows(l, capped, k1, share=share, prune=True)
                assert cut == list_rows(l, direct, k1, share=share, prune=True)
                assert [r for r in full if r & 0x8000] == [r for r in cut if r & 0x8000]          # self-loop rows are never touched
                assert len(cut) <= N_CENT[l] * 33
                if share:
                    today += len(full) if l == 1 else len(list_rows(l, capped, k1, prune=False))
                    pruned += len(cut) if l == 1 else len(list_rows(l, capped, k1, prune=True))
        if k1 < 128:
            assert pruned < today, f"object {o}: k1 = {k1}, rows {today} -> {pruned}"
            shorter += 1
        else:
            assert pruned == today
    assert shorter >= 20 + sum(k < 128 for k in K_DISTINCT)


def test_repeat_flags_find_only_true_repeats():
    xyz, rgb = stream_objects()
    found = 0
    for o in range(16):
        rep = repeat_flags(xyz[o], rgb[o])
        key = np.concatenate([xyz[o], rgb[o]], axis=1).view(np.uint32)
        _, first = np.unique(key, axis=0, return_index=True)
        exact = np.ones(256, dtype=bool)
        exact[first] = False
        assert not (rep & ~exact).any()
        found += int(rep.sum())
    assert found > 16 * 50


def test_header_declares_and_binding_binds_the_export():
    assert _lib.DEFINES["T2P_TUNING_MASK"] == 0xD
    assert _lib.SYMBOLS["t2p_group_rows_pruned"] == _lib.SYMBOLS["t2p_group_rows_built"]     # the same 11 arguments
    assert len(_lib.SYMBOLS["t2p_group_rows_pruned"][1]) == 11
