"""NumPy int64 restatement of the SA range balancing (include/t2p.h, t2p_sa_balance) and the inputs its tests share.
  prefix[i] = sum over g < i of ceil(n_rows[g] / tile_rows), i in [0, n];  total = prefix[n]
  bounds[b] = first m in [0, n] with prefix[m] >= floor(b * total / n_wg) for b < n_wg;  bounds[n_wg] = n"""
import numpy as np

MAX_ROWS = 4224        # the longest row list of an object (128 centroids x 33 rows)


def balance(n_rows, tile_rows, n_wg):
    c = np.asarray(n_rows).astype(np.int64)
    tiles = (c + tile_rows - 1) // tile_rows
    prefix = np.zeros(len(c) + 1, dtype=np.int64)
    np.cumsum(tiles, out=prefix[1:])
    total = int(prefix[-1])
    target = np.arange(n_wg + 1, dtype=np.int64) * total // n_wg
    bounds = np.searchsorted(prefix, target, side="left")       # first index whose prefix >= target
    bounds[n_wg] = len(c)
    return prefix, bounds.astype(np.int64)


def balance_brute(n_rows, tile_rows, n_wg):
    """The two definitions as loops over Python integers."""
    n = len(n_rows)
    prefix = [0]
    for g in range(n):
        prefix.append(prefix[-1] + -(-int(n_rows[g]) // tile_rows))
    total = prefix[n]
    bounds = []
    for b in range(n_wg):
        target = (b * total) // n_wg
        m = 0
        while prefix[m] < target:
            m += 1
        bounds.append(m)
    bounds.append(n)
    return np.array(prefix, dtype=np.int64), np.array(bounds, dtype=np.int64)


def counts(kind, n, seed=0):
    """uint16 row counts: uniform in 0..MAX_ROWS, all zero, all MAX_ROWS, or long runs of zeros (repeated prefixes)."""
    rng = np.random.default_rng(1000 * seed + n)
    if kind == "uniform":
        return rng.integers(0, MAX_ROWS + 1, n).astype(np.uint16)
    if kind == "zero":
        return np.zeros(n, dtype=np.uint16)
    if kind == "full":
        return np.full(n, MAX_ROWS, dtype=np.uint16)
    if kind == "runs":
        c = rng.integers(0, MAX_ROWS + 1, n).astype(np.uint16)
        run = max(1, n // 7)
        for start in range(0, n, 2 * run):           # every other stretch of n / 7 objects is empty, the first one included
            c[start:start + run] = 0
        return c
    raise ValueError(kind)
