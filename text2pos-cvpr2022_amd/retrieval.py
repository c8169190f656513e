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


def retrieve_topk(cell_encodings, text_encodings, k: int, device=None, index_offset: int = 0, cell_groups=None,
                  query_groups=None):
    """cell_encodings [Nc, D], text_encodings [Nq, D] (torch or numpy) -> (indices int64 [Nq, k], scores f64 [Nq, k])
    as torch tensors on the GPU.
    cell_groups [Nc] / query_groups [Nq] (integer arrays, torch or numpy, both or neither): the group-restricted ranking
    of the street oracle (evaluation/pipeline.py:93-108) - a pair whose groups differ scores -inf, so a query retrieves
    its own group's cells first and, when those run out, masked cells at -inf by ascending index."""
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
    if cell_groups is not None:
        cg = _as_device_groups(cell_groups, c.shape[0], "cell_groups", device)
        qg = _as_device_groups(query_groups, q.shape[0], "query_groups", device)
        return ops.sim_topk_grouped(q, c, qg, cg, int(k), index_offset)
    return ops.sim_topk(q, c, int(k), index_offset)


def top_retrievals(cell_encodings, text_encodings, db_cell_ids, top_k):
    """{query_idx: retrieved cell ids} exactly as eval_epoch builds it (training/coarse.py:133-147)."""
    idx, _ = retrieve_topk(cell_encodings, text_encodings, int(np.max(top_k)))
    idx = idx.cpu().numpy()
    ids = np.asarray(db_cell_ids)
    return {q: ids[idx[q]] for q in range(idx.shape[0])}
