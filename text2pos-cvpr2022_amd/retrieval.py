"""Top-k cell retrieval: the replacement for the per-query NumPy loop of training/coarse.py:134-140.

`retrieve_topk(cell_encodings, text_encodings, k)` returns what the reference computes per query as
`np.argsort(-1.0 * (cell_encodings @ text_encodings[q]))[0:k]` -- for all queries at once, ranked in float64 on the
GPU (csrc/sim_topk.hip), ties resolved to the lower cell index.  Any k from 1 to MAX_TOP_K: up to 16 the kernel keeps
per-lane lists in registers, above it selects exactly from a float64 score tile (same score bits, same order).
"""
import numpy as np
import torch

from . import _lib, ops

MAX_TOP_K = _lib.DEFINES["T2P_SIM_TOPK_MAX_K"]   # the largest k t2p_sim_topk accepts


def check_top_k(top_k) -> int:
    """max(top_k) of an evaluation's --top_k list, or a ValueError naming the limit: callers check BEFORE they encode."""
    ks = [int(k) for k in np.atleast_1d(np.asarray(top_k)).tolist()]
    if not ks or min(ks) < 1 or max(ks) > MAX_TOP_K:
        raise ValueError(f"top_k={list(ks)}: every k must lie in [1, {MAX_TOP_K}] (the retrieval kernel's limit, include/t2p.h)")
    return max(ks)


def _as_device_f32(x, device):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    x = x.to(device=device)
    if x.dtype != torch.float32:
        # the reference stores fp32 model outputs in float64 arrays (training/coarse.py:100-116); the values are
        # still exactly representable in fp32, anything else would silently lose precision here
        x32 = x.to(torch.float32)
        if not torch.equal(x32.to(x.dtype), x):
            raise RuntimeError("retrieve_topk: encodings are not exactly representable in float32")
        x = x32
    return x.contiguous()


def _as_device_groups(g, n: int, name: str, device):
    """Integer group ids (torch or numpy, length n) as an int32 tensor on the device; values outside int32 are refused."""
    if isinstance(g, torch.Tensor):
        if g.dtype.is_floating_point or g.dtype.is_complex or g.dtype == torch.bool:
            raise TypeError(f"retrieve_topk: {name} must be integers, got {g.dtype}")
        t = g
    else:
        a = np.asarray(g)
        if a.dtype.kind not in "iu":
            raise TypeError(f"retrieve_topk: {name} must be integers, got {a.dtype}")
        if a.dtype == np.uint64:      # (torch has no unsigned 64-bit arithmetic; the range check below needs signed values)
            if a.size and int(a.max()) > 2 ** 31 - 1:
                raise ValueError(f"retrieve_topk: {name} holds values outside int32")
            a = a.astype(np.int64)
        elif a.dtype.kind == "u":
            a = a.astype(np.int64)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"retrieve_topk: {name} has shape {tuple(t.shape)}, expected ({n},)")
    if t.dtype != torch.int32:
        if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) > 2 ** 31 - 1):
            raise ValueError(f"retrieve_topk: {name} holds values outside int32")
        t = t.to(torch.int32)
    return t.to(device=device).contiguous()


def _as_device_f64(x, shape, name: str, device):
    """Float64 geometry (torch or numpy, anything array-like) of the given shape on the device; other shapes are refused."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"retrieve_topk: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.to(device=device, dtype=torch.float64).contiguous()


def _first_offender(bad: torch.Tensor):
    """Row of the first True of a [n] or [n, m] mask (one host read), or None."""
    rows = bad.reshape(bad.shape[0], -1).any(dim=1) if bad.numel() else bad.reshape(-1)
    hit = torch.nonzero(rows)
    return int(hit[0]) if hit.numel() else None


def check_prior(query_xy: torch.Tensor, query_radius: torch.Tensor, cell_boxes: torch.Tensor):
    """ValueError naming the first query whose prior is not a finite point with a radius >= 0 (inf allowed), or the first cell whose
    box holds a NaN.  The kernel would mask such pairs silently; a caller who passes one has a bug upstream."""
    q = _first_offender(~torch.isfinite(query_xy))
    if q is not None:
        raise ValueError(f"retrieve_topk: query_xy[{q}] = {query_xy[q].tolist()} is not finite")
    q = _first_offender(~(query_radius >= 0))
    if q is not None:
        raise ValueError(f"retrieve_topk: query_radius[{q}] = {float(query_radius[q])} is NaN or negative (inf = no geometric restriction)")
    c = _first_offender(torch.isnan(cell_boxes))
    if c is not None:
        raise ValueError(f"retrieve_topk: cell_boxes[{c}] = {cell_boxes[c].tolist()} holds a NaN")


def retrieve_topk(cell_encodings, text_encodings, k: int, device=None, index_offset: int = 0, cell_groups=None,
                  query_groups=None, cell_boxes=None, query_xy=None, query_radius=None, validate: bool = True):
    """cell_encodings [Nc, D], text_encodings [Nq, D] (torch or numpy) -> (indices int64 [Nq, k], scores f64 [Nq, k])
    as torch tensors on the GPU.
    cell_groups [Nc] / query_groups [Nq] (integer arrays, torch or numpy, both or neither): the group-restricted ranking
    of the street oracle (evaluation/pipeline.py:93-108) - a pair whose groups differ scores -inf, so a query retrieves
    its own group's cells first and, when those run out, masked cells at -inf by ascending index.
    cell_boxes [Nc, 4] = x0 y0 x1 y1, query_xy [Nq, 2], query_radius [Nq] (float64, all three or none): the prior of the serving
    path (t2p_sim_topk_prior) - a pair is allowed when the query's point lies within its radius of the cell's closed square
    (radius 0: the cells that contain the point; inf: every cell).  With them the groups are optional companions, and a negative
    query group means any group.  Non-finite points, NaN or negative radii and NaN boxes are refused here, by name (one host
    read of three flags; validate=False skips it for a caller that has checked its values on the host, as Localizer does)."""
    geo = (cell_boxes, query_xy, query_radius)
    if any(g is None for g in geo) != all(g is None for g in geo):
        names = ("cell_boxes", "query_xy", "query_radius")
        raise ValueError("retrieve_topk: cell_boxes, query_xy and query_radius go together (missing: "
                         f"{', '.join(n for n, g in zip(names, geo) if g is None)})")
    if (cell_groups is None) != (query_groups is None):
        raise ValueError("retrieve_topk: cell_groups and query_groups go together (got only "
                         f"{'cell_groups' if query_groups is None else 'query_groups'})")
    if device is None:
        device = cell_encodings.device if isinstance(cell_encodings, torch.Tensor) and cell_encodings.is_cuda else \
            torch.device("cuda", torch.cuda.current_device())
    c = _as_device_f32(cell_encodings, device)
    q = _as_device_f32(text_encodings, device)
    d = c.shape[1]
    if d not in (128, 256, 384):     # e.g. embed_dim 300: zero columns up to the kernel's width add exact zeros to every score
        from .packing import kernel_embed_dim
        pad = kernel_embed_dim(d) - d
        c, q = torch.nn.functional.pad(c, (0, pad)).contiguous(), torch.nn.functional.pad(q, (0, pad)).contiguous()
    cg = qg = None
    if cell_groups is not None:
        cg = _as_device_groups(cell_groups, c.shape[0], "cell_groups", device)
        qg = _as_device_groups(query_groups, q.shape[0], "query_groups", device)
    if cell_boxes is not None:
        box = _as_device_f64(cell_boxes, (c.shape[0], 4), "cell_boxes", device)
        xy = _as_device_f64(query_xy, (q.shape[0], 2), "query_xy", device)
        rad = _as_device_f64(query_radius, (q.shape[0],), "query_radius", device)
        if validate:
            check_prior(xy, rad, box)
        return ops.sim_topk_prior(q, c, int(k), index_offset, query_xy=xy, query_radius=rad, cell_box=box, query_group=qg,
                                  cell_group=cg)
    if cg is not None:
        return ops.sim_topk_grouped(q, c, qg, cg, int(k), index_offset)
    return ops.sim_topk(q, c, int(k), index_offset)


def check_distinct(sep, what: str = "retrieve_topk_distinct") -> float:
    """The separation of a distinct-candidates call as a float, or a ValueError: a number >= 0, inf allowed (one cell per group)."""
    try:
        s = float(sep)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the separation must be one number >= 0 (got {sep!r})") from None
    if not s >= 0:
        raise ValueError(f"{what}: the separation is {s}: it must be >= 0 (0: nothing conflicts, inf: one cell per group)")
    return s


def default_distinct_pool(n_cells: int, k: int) -> int:
    """min(Nc, MAX_TOP_K, max(64, 32 k)): at a separation of the cell size, 30 m cells on a 10 m stride conflict with 24 neighbours
    each, rounded up to 32.  A default, not a guarantee: `exhausted` reports the queries it was too small for."""
    return min(int(n_cells), MAX_TOP_K, max(64, 32 * int(k)))


def retrieve_topk_distinct(cell_encodings, text_encodings, k: int, cell_xy, sep: float, pool=None, device=None, index_offset: int = 0,
                           cell_groups=None, query_groups=None, cell_boxes=None, query_xy=None, query_radius=None,
                           validate: bool = True):
    """The k best cells of every query no two of which overlap: retrieve_topk with k = pool (same restriction arguments), then the
    greedy selection of ops.topk_distinct over that ordered list - a cell is accepted iff no accepted one of its group lies within
    `sep` of it in x and in y (cell_xy float64 [Nc, 2], the cells' centres).  cell_groups, when given, are the conflict groups too:
    cells of different groups never suppress each other.  pool: None = default_distinct_pool(Nc, k), or any value in
    [k, min(Nc, MAX_TOP_K)].  Returns (indices int64 [Nq, k], scores f64 [Nq, k], n_valid int32 [Nq], exhausted int32 [Nq]) on the
    GPU: n_valid accepted cells first, the columns behind them at -inf; exhausted = 1 where the pool, not the database, cut the
    list short (ask again with a larger pool).  NaN centres are refused by name (validate=False skips that host read and the
    one of the selection's marks, for a caller that has checked its table and reads n_valid itself)."""
    k, sep = check_top_k(k), check_distinct(sep)
    nc = int(cell_encodings.shape[0])
    if k > nc:
        raise ValueError(f"retrieve_topk_distinct: k={k} exceeds the {nc} cells")
    pool = default_distinct_pool(nc, k) if pool is None else int(pool)
    if not k <= pool <= min(nc, MAX_TOP_K):
        raise ValueError(f"retrieve_topk_distinct: pool={pool} outside [k, min(Nc, {MAX_TOP_K})] = [{k}, {min(nc, MAX_TOP_K)}]")
    idx, score = retrieve_topk(cell_encodings, text_encodings, pool, device=device, index_offset=index_offset, cell_groups=cell_groups,
                               query_groups=query_groups, cell_boxes=cell_boxes, query_xy=query_xy, query_radius=query_radius,
                               validate=validate)
    dev = idx.device
    xy = _as_device_f64(cell_xy, (nc, 2), "cell_xy", dev)
    if validate:
        c = _first_offender(torch.isnan(xy))
        if c is not None:
            raise ValueError(f"retrieve_topk_distinct: cell_xy[{c}] = {xy[c].tolist()} holds a NaN")
    cg = None if cell_groups is None else _as_device_groups(cell_groups, nc, "cell_groups", dev)
    return ops.topk_distinct(idx, score, xy, sep, k, cell_group=cg, index_offset=index_offset, check=validate)


def top_retrievals(cell_encodings, text_encodings, db_cell_ids, top_k):
    """{query_idx: retrieved cell ids} exactly as eval_epoch builds it (training/coarse.py:133-147)."""
    idx, _ = retrieve_topk(cell_encodings, text_encodings, int(np.max(top_k)))
    idx = idx.cpu().numpy()
    ids = np.asarray(db_cell_ids)
    return {q: ids[idx[q]] for q in range(idx.shape[0])}
