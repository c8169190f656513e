"""float64 reference of t2p_localize_poses (helper of tests/test_localize_host.py and tests/test_gpu_localize.py, not a test): a plain
NumPy loop over samples and slots, the exact value in rational arithmetic, and the bound the GPU test holds the kernel to.

The bound comes from the operation count, not from the kernel's output.  With u = 2^-53 and gamma(n) = n u / (1 - n u):
  * a matched slot's term t_i = fl(c_i + o_i) (the fp32 offset widens exactly): one rounding;
  * the sum of k <= M terms in ANY order (this loop adds them in slot order, the kernel in a butterfly): every term carries at most
    k - 1 further roundings;
  * one division by k.
So a computed position is sum_i (c_i + o_i)(1 + theta_i) / k with |theta_i| <= gamma(k + 1) <= gamma(M + 1), and its distance from
the exact mean is at most gamma(M + 1) * A, A = the largest |c_i + o_i| <= max|c| + max|o|.  Two such computations (this reference
and the kernel) differ by at most twice that: POS_BOUND.
The world step w = fl(b + fl(p s)) has two roundings (one, when the multiply-add is contracted into an FMA): each side is within
u |p s| + u |b + p s| (1 + u) <= 2 u (|b| + |p| |s|) (1 + u) of b + p s for ITS p, and the two p differ by at most POS_BOUND.  With
|p| <= A (1 + gamma(M + 1)):  WORLD_BOUND = |s| POS_BOUND + 4 u (|b| + A |s|) (1 + 2^-40) - the last factor covers the second-order terms.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def magnitude(center_xy, offsets) -> float:
    """A = max|c| + max|o| over everything a sample could add up."""
    c = np.abs(np.asarray(center_xy, dtype=np.float64))
    o = np.abs(np.asarray(offsets, dtype=np.float64))
    o = o[np.isfinite(o)]
    return float(c.max() if c.size else 0.0) + float(o.max() if o.size else 0.0)


def pos_bound(n_obj: int, a: float, sides: int = 2) -> float:
    """Largest distance of `sides` float64 computations of a position (sides=1: of one from the exact value)."""
    return sides * gamma(n_obj + 1) * a


def world_bound(n_obj: int, a: float, bbox_abs: float, size_abs: float, sides: int = 2) -> float:
    return size_abs * pos_bound(n_obj, a, sides) + 2 * sides * U * (bbox_abs + a * size_abs) * (1.0 + 2.0 ** -40)


def _bad(row, n_cells, m0, off, n_hints):
    return (row < 0 or row >= n_cells or bool(((m0 < -1) | (m0 >= n_hints)).any()) or bool(np.isnan(off).any()))


def poses(matches0, offsets, cell_row, n_queries, top_k, center_xy, bbox_xy, cell_size):
    """matches0 int [Q K, M], offsets fp32 [Q K, N, 2], cell_row int [Q K]; float64 tables center_xy [n_cells, M, 2], bbox_xy
    [n_cells, 2], cell_size [n_cells] -> dict(pos_mean, pos_offset, world_mean, world_offset float64 [Q, K, 2], matched int32 [Q, K],
    best int32 [Q]): t2p_localize_poses' contract (include/t2p.h), one sample and one slot at a time."""
    matches0, offsets, cell_row = np.asarray(matches0), np.asarray(offsets), np.asarray(cell_row)
    center_xy, bbox_xy, cell_size = (np.asarray(a, dtype=np.float64) for a in (center_xy, bbox_xy, cell_size))
    q_, k_, m_, n_ = int(n_queries), int(top_k), matches0.shape[1], offsets.shape[1]
    out = {name: np.full((q_, k_, 2), np.nan) for name in ("pos_mean", "pos_offset", "world_mean", "world_offset")}
    out["matched"] = np.full((q_, k_), -1, dtype=np.int32)
    out["best"] = np.full((q_,), -1, dtype=np.int32)
    for q in range(q_):
        for c in range(k_):
            s = q * k_ + c
            row = int(cell_row[s])
            if _bad(row, center_xy.shape[0], matches0[s], offsets[s], n_):
                continue
            mean, off, cnt = np.zeros(2), np.zeros(2), 0
            for i in range(m_):
                j = int(matches0[s, i])
                if j >= 0:
                    mean = mean + center_xy[row, i]
                    off = off + (center_xy[row, i] + offsets[s, j].astype(np.float64))
                    cnt += 1
            pm = mean / cnt if cnt else np.array((0.5, 0.5))
            po = off / cnt if cnt else np.array((0.5, 0.5))
            out["pos_mean"][q, c], out["pos_offset"][q, c] = pm, po
            out["world_mean"][q, c] = bbox_xy[row] + pm * cell_size[row]
            out["world_offset"][q, c] = bbox_xy[row] + po * cell_size[row]
            out["matched"][q, c] = cnt
        ok = out["matched"][q] >= 0
        if ok.any():
            out["best"][q] = int(np.argmax(np.where(ok, out["matched"][q], -1)))
    return out


def poses_exact(matches0, offsets, cell_row, n_queries, top_k, center_xy, bbox_xy, cell_size):
    """The same in rational arithmetic (fractions.Fraction of the float inputs: no rounding anywhere) for in-range samples:
    dict of object arrays [Q, K, 2] of Fractions."""
    matches0, offsets, cell_row = np.asarray(matches0), np.asarray(offsets), np.asarray(cell_row)
    q_, k_, m_ = int(n_queries), int(top_k), matches0.shape[1]
    out = {name: np.empty((q_, k_, 2), dtype=object) for name in ("pos_mean", "pos_offset", "world_mean", "world_offset")}
    half = Fraction(1, 2)
    for q in range(q_):
        for c in range(k_):
            s = q * k_ + c
            row = int(cell_row[s])
            for d in range(2):
                terms_m = [Fraction(float(center_xy[row][i][d])) for i in range(m_) if matches0[s, i] >= 0]
                terms_o = [Fraction(float(center_xy[row][i][d])) + Fraction(float(offsets[s][int(matches0[s, i])][d]))
                           for i in range(m_) if matches0[s, i] >= 0]
                pm = sum(terms_m) / len(terms_m) if terms_m else half
                po = sum(terms_o) / len(terms_o) if terms_o else half
                b, sz = Fraction(float(bbox_xy[row][d])), Fraction(float(cell_size[row]))
                out["pos_mean"][q, c, d], out["pos_offset"][q, c, d] = pm, po
                out["world_mean"][q, c, d], out["world_offset"][q, c, d] = b + pm * sz, b + po * sz
    return out
