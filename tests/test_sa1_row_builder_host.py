"""k_build_rows restated in NumPy (csrc/sample_group.hip): SA level 1's row list from per-centroid hit masks.

The builder takes, per centroid, the four u64 words of the point-ordered hit mask the scan published (centroids from the first
tail centroid on take centroid 0's words: the scan stops there), keeps the first 32 set bits (the cap), clears the bits of repeated
points, and lists what is left in ascending order with the self-loop row behind it.  With EXACT repeat flags the number of hit rows
is what profiles/tail_rows_census.py counts for t2p_dedup_rows (cap applied to all hits, then the hits on repeated points leave);
the kernel's hash table may miss a few repeats, which the GPU test covers by comparing against t2p_dedup_rows itself.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from text2pos_amd import _lib, synthetic as S  # noqa: E402

M64 = (1 << 64) - 1
R0 = 0.2


def lowest_set_bits(w: int, k: int) -> int:
    """The binary search of the kernel's lowest_set_bits (k < popcount(w))."""
    if k <= 0:
        return 0
    p, s = 0, 32
    while s > 0:
        if bin(w & ((1 << (p + s)) - 1)).count("1") < k:
            p += s
        s >>= 1
    return w & (((2 << p) - 1) & M64)


def scan_masks(pos):
    """fps_idx [128] and the mask words [t0][4] the scan publishes (mask mode: strided ownership makes word j = points 64 j ..
    64 j + 63; the scan stops at the first tail centroid t0)."""
    r2 = np.float32(R0) * np.float32(R0)
    mind = np.full(256, np.inf, dtype=np.float32)
    fps, words, cur = np.zeros(128, dtype=np.int64), [], 0
    for c in range(128):
        if c > 0 and cur == 0:
            break                                   # fps[c:] stay 0
        fps[c] = cur
        d = pos - pos[cur]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        hit = d2 < r2
        words.append([sum(1 << int(b) for b in np.flatnonzero(hit[64 * j:64 * j + 64])) for j in range(4)])
        mind = np.minimum(mind, d2)
        cur = int(np.argmax(mind))
    return fps, words


def build_rows(fps, words, repeat):
    """The builder: list of u16 rows."""
    repw = [sum(1 << int(b) for b in np.flatnonzero(repeat[64 * j:64 * j + 64])) for j in range(4)]
    tail = np.flatnonzero((fps == 0) & (np.arange(128) > 0))
    t0 = int(tail[0]) if len(tail) else 128
    assert len(words) == t0
    rows = []
    for c in range(128):
        w = list(words[c if c < t0 else 0])
        left = 32
        for j in range(4):
            pc = bin(w[j]).count("1")
            if pc > left:
                w[j] = lowest_set_bits(w[j], left)
                pc = left
            left -= pc
            w[j] &= ~repw[j] & M64
            x = w[j]
            while x:
                b = (x & -x).bit_length() - 1
                rows.append((c << 8) | (64 * j + b))
                x &= x - 1
        rows.append(((c | 0x80) << 8) | c)
    return rows


def test_lowest_set_bits():
    rng = np.random.default_rng(5)
    for _ in range(300):
        w = int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63)
        pc = bin(w).count("1")
        for k in range(0, pc):
            got = lowest_set_bits(w, k)
            bits = [b for b in range(64) if w >> b & 1][:k]
            assert got == sum(1 << b for b in bits)


def test_builder_counts_equal_the_census():
    import tail_rows_census as T
    xyz, rgb, _, _ = S.make_objects(20220002, 0, 64)
    with_tail = 0
    for o in range(64):
        pos, col = xyz[o].astype(np.float32), rgb[o].astype(np.float32)
        fps, words = scan_masks(pos)
        ref_fps, _ = T.level(pos, R0)
        assert np.array_equal(fps, ref_fps), f"object {o}: the tail stop changes fps_idx"
        with_tail += len(words) < 128
        _, first = np.unique(np.concatenate([pos, col], axis=1).view(np.uint32), axis=0, return_index=True)
        repeat = np.ones(256, dtype=bool)
        repeat[first] = False
        rows = build_rows(fps, words, repeat)
        hits = [r for r in rows if not r & 0x8000]
        assert len(hits) == T.dedup_hits(pos, col, fps, R0), f"object {o}"
        # order: by centroid, hits ascending, the self loop last
        cent = [(r >> 8) & 0x7F for r in rows]
        assert cent == sorted(cent)
        for c in range(128):
            mine = [r for r in rows if (r >> 8) & 0x7F == c]
            assert mine[-1] == ((c | 0x80) << 8) | c and mine[:-1] == sorted(mine[:-1]) and len(mine) <= 33
    assert with_tail >= 10, with_tail


def test_header_declares_and_binding_binds_the_export():
    assert _lib.DEFINES["T2P_TUNING_MASK"] == 0xD
    assert "t2p_group_rows_built" in _lib.SYMBOLS
    restype, argtypes = _lib.SYMBOLS["t2p_group_rows_built"]
    assert len(argtypes) == 11                     # xyz, rgb, n_obj, n_pts, radius, self_loops, share_mask, 3 tables, stream
