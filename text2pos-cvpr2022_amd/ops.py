"""Tensor-level wrappers over the C ABI (include/t2p.h): argument validation, workspace handling, stream plumbing.

PyTorch is used for device memory, streams and torch.distributed only; all arithmetic happens in libt2p_hip.so.
Shape / dtype / device / contiguity violations raise RuntimeError before anything is launched.
"""
import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L

_workspaces: Dict[tuple, torch.Tensor] = {}


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _need(t: torch.Tensor, name: str, dtype, ndim=None, device=None):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: must live on the GPU (got device {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError(f"{name}: expected {ndim} dimensions, got shape {tuple(t.shape)}")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name}: on {t.device}, expected {device}")
    return t


DEFAULT_CHUNK_OBJECTS = L.DEFINES["T2P_DEFAULT_CHUNK_OBJECTS"]


def workspace(device, nbytes: int, tag: str) -> torch.Tensor:
    """Grow-only scratch buffer per (device, tag), obtained from torch's caching allocator."""
    key = (str(device), tag)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        _workspaces[key] = None
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def release_workspaces():
    _workspaces.clear()


# ---- streams that really run side by side ----------------------------------------------------------------------
def _spin_cycles(device) -> int:
    """Argument of torch.cuda._sleep for a ~0.4 ms single-thread spin on this device (its unit is device dependent)."""
    key = str(device)
    if key not in _spin_memo:
        st = torch.cuda.current_stream(device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)             # (first launch: module load)
        torch.cuda.synchronize(device)
        cycles = 20000
        for _ in range(8):
            e0.record(st)
            torch.cuda._sleep(cycles)
            e1.record(st)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if 0.3 <= ms <= 0.8:
                break
            cycles = max(1000, int(cycles * min(8.0, 0.45 / max(ms, 1e-3))))
        _spin_memo[key] = cycles
    return _spin_memo[key]


def _measure_overlap(a: "torch.cuda.Stream", b: "torch.cuda.Stream") -> bool:
    dev = a.device
    cycles = _spin_cycles(dev)
    torch.cuda.synchronize(dev)
    start, ea, eb = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    start.record(a)
    b.wait_event(start)
    with torch.cuda.stream(a):
        torch.cuda._sleep(cycles)
        ea.record(a)
    with torch.cuda.stream(b):
        torch.cuda._sleep(cycles)
        eb.record(b)
    ea.synchronize()
    eb.synchronize()
    solo, both = start.elapsed_time(ea), max(start.elapsed_time(ea), start.elapsed_time(eb))
    return both < 1.6 * solo


def streams_overlap(a: "torch.cuda.Stream", b: "torch.cuda.Stream") -> bool:
    """True when a kernel on stream `b` runs BESIDE a kernel on stream `a`.  HIP maps a process's streams onto a handful of hardware
    queues (4 by default) in the order of their first use; two streams that share a queue serialise, and nothing in the API says which
    do.  Measured with a single-thread spin kernel (~0.45 ms) per stream behind a common start event: side by side the pair takes one
    spin time, in one queue two.  A stream keeps its queue, so a pair is measured once per process.  (A 12,000-cell encode in two parts
    loses its whole two-stream gain, ~3 %, when the second part's stream shares the text stream's queue - which depends on what the
    process did before: docs/notebook.md, round 6.)"""
    if a.cuda_stream == b.cuda_stream:
        return False
    key = (str(a.device),) + tuple(sorted((a.cuda_stream, b.cuda_stream)))
    if key not in _overlap_memo:
        _overlap_memo[key] = _measure_overlap(a, b)
    return _overlap_memo[key]


def concurrent_stream(device, beside=()) -> "torch.cuda.Stream":
    """A HIP stream that runs beside the device's current stream and beside every stream in `beside` (streams_overlap), and - as far as
    the hardware queues allow - beside the streams this function handed out before.  Streams come from a per-device set of at most
    eight that lives as long as the process (a stream's queue is fixed at its first use; a destroyed stream's slot would be handed
    out again), so two callers may get the same stream - which orders their work, never breaks it.  Cost: ~1 ms per pair of streams
    never measured before.  Plain `torch.cuda.Stream()` when the spin kernel is unavailable, under a graph capture (the probe
    synchronises the device) or with T2P_NO_STREAM_PROBE set (the switch exists for A/B measurements of this function)."""
    device = torch.device(device)
    if not hasattr(torch.cuda, "_sleep") or os.environ.get("T2P_NO_STREAM_PROBE") or torch.cuda.is_current_stream_capturing():
        return torch.cuda.Stream(device=device)
    must = [torch.cuda.current_stream(device)] + [b for b in beside if b is not None]
    kept = _stream_sets.setdefault(str(device), [])
    best, best_score, i = None, None, 0
    while i < _MAX_KEPT_STREAMS:
        if i == len(kept):
            c = torch.cuda.Stream(device=device)
            if any(c.cuda_stream == o.cuda_stream for o in kept):
                break                      # (torch's stream pool came round)
            kept.append(c)
        c, i = kept[i], i + 1
        if any(c.cuda_stream == m.cuda_stream for m in must) or not all(streams_overlap(m, c) for m in must):
            continue
        out = [o for o in kept if _handed_out.get((str(device), o.cuda_stream), 0) > 0 and all(o.cuda_stream != m.cuda_stream for m in must)]
        score = sum(_handed_out[(str(device), o.cuda_stream)] for o in out if not streams_overlap(o, c))   # (c itself included)
        if best is None or score < best_score:
            best, best_score = c, score
        if score == 0:
            break
    if best is None:
        return torch.cuda.Stream(device=device)
    _handed_out[(str(device), best.cuda_stream)] = _handed_out.get((str(device), best.cuda_stream), 0) + 1
    return best


def pick_concurrent_streams(device, beside, n: int):
    """`n` streams from concurrent_stream, each beside `beside` and beside the ones picked before it."""
    picked = []
    for _ in range(n):
        picked.append(concurrent_stream(device, list(beside) + picked))
    return picked


_MAX_KEPT_STREAMS = 8
_overlap_memo, _stream_sets, _handed_out, _spin_memo = {}, {}, {}, {}


# ---------------------------------------------------------------------------------------------------------------
def _level_geometry(n_pts: int):
    """[(n_dense, n_cent)] of the three SA levels: every level keeps ceil(n_dense / 2) centroids, the next level's points."""
    levels, nd = [], n_pts
    for _ in range(3):
        levels.append((nd, (nd + 1) // 2))
        nd = levels[-1][1]
    return levels


# per-level tables of k_sample_group and of the encoder's trace: shape from (n_obj, n_cent, level), dtype
_LEVEL_TABLES = {
    "fps_idx": (lambda n, nc, l: (n, nc), torch.uint8),
    "nbr": (lambda n, nc, l: (n, nc, 32), torch.uint8),
    "cnt": (lambda n, nc, l: (n, nc), torch.uint8),
    "rows": (lambda n, nc, l: (n, nc * 33), torch.int16),      # uint16 bits
    "n_rows": (lambda n, nc, l: (n,), torch.int16),
    "sa_out": (lambda n, nc, l: (n * nc, (64, 128, 256)[l] + 32), torch.float32),
}


def _level_tables(n_obj: int, n_pts: int, device, names, alloc=torch.empty):
    """One tensor per level for each name of _LEVEL_TABLES, and their addresses as the void*[3] arrays of the C ABI."""
    tables = {name: [alloc(_LEVEL_TABLES[name][0](n_obj, nc, l), dtype=_LEVEL_TABLES[name][1], device=device)
                     for l, (_, nc) in enumerate(_level_geometry(n_pts))] for name in names}
    return tables, {name: (C.c_void_p * 3)(*[t.data_ptr() for t in ts]) for name, ts in tables.items()}


def _radius(radius):
    return (C.c_float * 3)(*[float(v) for v in radius])


def sample_group(xyz: torch.Tensor, radius=(0.2, 0.3, 0.4)):
    """Fused FPS + ball query of the three SA levels.  xyz [n_obj, n_pts, 3] fp32.
    Returns dict(fps_idx=[3 x uint8 [n_obj, n_c]], nbr=[3 x uint8 [n_obj, n_c, 32]], cnt=[3 x uint8 [n_obj, n_c]])."""
    _need(xyz, "xyz", torch.float32, 3)
    n_obj, n_pts, three = xyz.shape
    if three != 3:
        raise RuntimeError(f"xyz: last dimension must be 3, got {three}")
    out, arr = _level_tables(n_obj, n_pts, xyz.device, ("fps_idx", "nbr", "cnt"))
    L.check(L.lib().t2p_sample_group(_ptr(xyz), n_obj, n_pts, _radius(radius), arr["fps_idx"], arr["nbr"], arr["cnt"],
                                     _stream(xyz.device)), "t2p_sample_group")
    return out


def group_edges(xyz: torch.Tensor, first_obj: torch.Tensor, radius=(0.2, 0.3, 0.4), self_loops: bool = True):
    """FPS + ball query of the three SA levels as EDGE LISTS for the training-mode path, built on the device:
    t2p_group_rows (k_sample_group's compact row lists) -> t2p_edge_counts -> prefix sum -> t2p_edge_expand.  One host
    read-back (the three edge totals) instead of the size read-backs of a nonzero / sort / bincount chain per level.
    xyz [n_obj, n_pts, 3] fp32; first_obj [n_obj] int32 (device): first object of each object's cell.
    Returns a list of three dicts: fps_idx uint8 [n_obj, n_c], src / dst int32 [E] (dense row, centroid row; sorted by dst,
    torch_geometric's self-loop rewrite applied when self_loops), cent_ptr int32 [n_obj * n_c + 1]."""
    _need(xyz, "xyz", torch.float32, 3)
    dev = xyz.device
    _need(first_obj, "first_obj", torch.int32, 1, dev)
    n_obj, n_pts, three = xyz.shape
    if three != 3 or first_obj.numel() != n_obj:
        raise RuntimeError("group_edges: xyz must be [n_obj, n_pts, 3] and first_obj [n_obj]")
    levels = _level_geometry(n_pts)
    t, arr = _level_tables(n_obj, n_pts, dev, ("fps_idx", "rows", "n_rows"))
    rows, n_rows = t["rows"], t["n_rows"]
    st = _stream(dev)
    L.check(L.lib().t2p_group_rows(_ptr(xyz), n_obj, n_pts, _radius(radius), int(bool(self_loops)), arr["fps_idx"], arr["rows"],
                                   arr["n_rows"], st), "t2p_group_rows")
    cent_ptrs = []
    for l, (nd, nc) in enumerate(levels):
        counts = torch.empty((n_obj * nc,), dtype=torch.int32, device=dev)
        L.check(L.lib().t2p_edge_counts(_ptr(rows[l]), _ptr(n_rows[l]), _ptr(first_obj), n_obj, nd, nc,
                                        int(bool(self_loops)), _ptr(counts), st), "t2p_edge_counts")
        cp = torch.zeros((n_obj * nc + 1,), dtype=torch.int32, device=dev)
        torch.cumsum(counts, 0, dtype=torch.int32, out=cp[1:])
        cent_ptrs.append(cp)
    totals = torch.stack([cp[-1] for cp in cent_ptrs]).cpu().tolist()      # the one read-back
    out = []
    for l, (nd, nc) in enumerate(levels):
        e = int(totals[l])
        src = torch.empty((e,), dtype=torch.int32, device=dev)
        dst = torch.empty((e,), dtype=torch.int32, device=dev)
        L.check(L.lib().t2p_edge_expand(_ptr(rows[l]), _ptr(n_rows[l]), _ptr(first_obj), _ptr(cent_ptrs[l]), n_obj, nd, nc,
                                        int(bool(self_loops)), _ptr(src), _ptr(dst), st), "t2p_edge_expand")
        out.append(dict(fps_idx=t["fps_idx"][l], src=src, dst=dst, cent_ptr=cent_ptrs[l], n_dense=nd, n_cent=nc))
    return out


def sa_balance(n_rows: torch.Tensor, tile_rows: int, n_wg: int):
    """The SA edge kernels' range balancing (t2p_sa_balance): n_rows int16 [n] (uint16 bits, as group_rows returns them).
    Returns (prefix int32 [n + 1]: exclusive sums of ceil(n_rows / tile_rows); bounds int32 [n_wg + 1]: workgroup b owns the
    objects [bounds[b], bounds[b + 1]))."""
    _need(n_rows, "n_rows", torch.int16, 1)
    dev, n = n_rows.device, n_rows.shape[0]
    prefix = torch.empty((n + 1,), dtype=torch.int32, device=dev)
    bounds = torch.empty((int(n_wg) + 1,), dtype=torch.int32, device=dev)
    L.check(L.lib().t2p_sa_balance(_ptr(n_rows), n, int(tile_rows), int(n_wg), _ptr(prefix), _ptr(bounds), _stream(dev)),
            "t2p_sa_balance")
    return prefix, bounds


def group_rows(xyz: torch.Tensor, radius=(0.2, 0.3, 0.4), self_loops: bool = True, share_mask: int = 0):
    """k_sample_group's compact edge-row lists of the three SA levels (t2p_group_rows_shared).  xyz [n_obj, n_pts, 3] fp32.
    share_mask: bit 1 = SA level 2 in the shared form its f16x3 kernel consumes (the hits of the centroids that repeat
    centroid 0 once, under the pseudo-centroid code 64: include/t2p.h); 0 = full lists, any n_pts.
    Returns dict(fps_idx=[3 x uint8 [n_obj, n_c]], rows=[3 x int16 [n_obj, n_c * 33]] (uint16 bits), n_rows=[3 x int16 [n_obj]])."""
    _need(xyz, "xyz", torch.float32, 3)
    dev = xyz.device
    n_obj, n_pts, three = xyz.shape
    if three != 3:
        raise RuntimeError(f"xyz: last dimension must be 3, got {three}")
    out, arr = _level_tables(n_obj, n_pts, dev, ("fps_idx", "rows", "n_rows"))
    L.check(L.lib().t2p_group_rows_shared(_ptr(xyz), n_obj, n_pts, _radius(radius), int(bool(self_loops)), int(share_mask),
                                          arr["fps_idx"], arr["rows"], arr["n_rows"], _stream(dev)), "t2p_group_rows_shared")
    return out


def group_rows_built(xyz: torch.Tensor, rgb: torch.Tensor, radius=(0.2, 0.3, 0.4), self_loops: bool = True, share_mask: int = 0,
                     prune_dup: bool = False):
    """group_rows followed by dedup_rows on level 0 (t2p_group_rows_built): the scan publishes level 0's hit masks and one
    builder kernel writes the pruned list.  xyz, rgb [n_obj, 256, 3] fp32.
    Returns the dict of group_rows, bit for bit what the two calls leave.
    prune_dup (t2p_group_rows_pruned): the lists the encoder consumes without self-loop rows - at SA levels 2 and 3 the rows whose source
    is a repeated dense point (index >= k_prev, include/t2p.h) are left out as well."""
    _need(xyz, "xyz", torch.float32, 3)
    _need(rgb, "rgb", torch.float32, 3, xyz.device)
    dev = xyz.device
    n_obj, n_pts, three = xyz.shape
    if three != 3 or tuple(rgb.shape) != tuple(xyz.shape):
        raise RuntimeError(f"group_rows_built: xyz and rgb must both be [n_obj, n_pts, 3], got {tuple(xyz.shape)} and {tuple(rgb.shape)}")
    out, arr = _level_tables(n_obj, n_pts, dev, ("fps_idx", "rows", "n_rows"))
    name = "t2p_group_rows_pruned" if prune_dup else "t2p_group_rows_built"
    L.check(getattr(L.lib(), name)(_ptr(xyz), _ptr(rgb), n_obj, n_pts, _radius(radius), int(bool(self_loops)), int(share_mask),
                                   arr["fps_idx"], arr["rows"], arr["n_rows"], _stream(dev)), name)
    return out


def dedup_rows(xyz: torch.Tensor, rgb: torch.Tensor, rows: torch.Tensor, n_rows: torch.Tensor):
    """In-place t2p_dedup_rows: rows uint16 [n_obj, (n_pts / 2) * 33] (as int16 storage), n_rows uint16 [n_obj] (int16)."""
    _need(xyz, "xyz", torch.float32, 3)
    _need(rgb, "rgb", torch.float32, 3, xyz.device)
    _need(rows, "rows", torch.int16, 2, xyz.device)
    _need(n_rows, "n_rows", torch.int16, 1, xyz.device)
    n_obj, n_pts = xyz.shape[0], xyz.shape[1]
    if rows.shape[0] != n_obj or rows.shape[1] != ((n_pts + 1) // 2) * 33 or n_rows.numel() != n_obj:
        raise RuntimeError("dedup_rows: inconsistent shapes")
    L.check(L.lib().t2p_dedup_rows(_ptr(xyz), _ptr(rgb), n_obj, n_pts, _ptr(rows), _ptr(n_rows), _stream(xyz.device)),
            "t2p_dedup_rows")


def knn(x: torch.Tensor, seg_ptr: torch.Tensor, k: int, max_seg_rows: Optional[int] = None) -> torch.Tensor:
    _need(x, "x", torch.float32, 2)
    _need(seg_ptr, "seg_ptr", torch.int32, 1, x.device)
    if max_seg_rows is None:
        sp = seg_ptr.cpu()
        max_seg_rows = int((sp[1:] - sp[:-1]).max().item()) if sp.numel() > 1 else 0
    out = torch.empty((x.shape[0], k), dtype=torch.int32, device=x.device)
    L.check(L.lib().t2p_knn(_ptr(x), x.shape[1], _ptr(seg_ptr), seg_ptr.numel() - 1, int(max_seg_rows), k, _ptr(out),
                            _stream(x.device)), "t2p_knn")
    return out


def gemm(a: torch.Tensor, w_kmajor: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False):
    """act(a @ w_kmajor + bias);  a [M, K], w_kmajor [K, N]."""
    _need(a, "a", torch.float32, 2)
    _need(w_kmajor, "w", torch.float32, 2, a.device)
    if bias is not None:
        _need(bias, "bias", torch.float32, 1, a.device)
    m, k = a.shape
    if w_kmajor.shape[0] != k:
        raise RuntimeError(f"gemm: a is [{m},{k}] but w is {tuple(w_kmajor.shape)}")
    n = w_kmajor.shape[1]
    out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    L.check(L.lib().t2p_gemm(_ptr(a), k, _ptr(w_kmajor), _ptr(bias), _ptr(out), n, 0, m, k, n, int(relu),
                             _stream(a.device)), "t2p_gemm")
    return out


def matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [M, K] @ b [K, N] on the tiled fp32-MFMA GEMM (t2p_gemm) for any sizes: K is zero-padded to a multiple of 4 and N
    to a multiple of 8 (the kernel's granules).  The training path's weight-gradient / score products go through here:
    a transposed operand is a torch copy (`x.t().contiguous()`), the arithmetic is this library's."""
    _need(a.contiguous(), "a", torch.float32, 2)
    m, k = a.shape
    if b.shape[0] != k:
        raise RuntimeError(f"matmul: a is [{m},{k}] but b is {tuple(b.shape)}")
    n = b.shape[1]
    kp, np_ = (k + 3) // 4 * 4, (n + 7) // 8 * 8
    a = a.contiguous()
    b = b.contiguous()
    if kp != k:
        a = torch.nn.functional.pad(a, (0, kp - k))
    if kp != k or np_ != n:
        b = torch.nn.functional.pad(b, (0, np_ - n, 0, kp - k))
    if m == 0 or n == 0:
        return torch.zeros((m, n), dtype=torch.float32, device=a.device)
    out = gemm(a.contiguous(), b.contiguous())
    return out if np_ == n else out[:, :n].contiguous()


def _need_span(t: torch.Tensor, name: str, rows: int, pitch: int, width: int, dtype=torch.float32, device=None, first: int = 0):
    """t is a contiguous buffer that holds `rows` rows of `width` elements at a pitch of `pitch`, the first at element `first`."""
    _need(t, name, dtype, None, device)
    if rows < 0 or width < 0 or first < 0 or pitch < first + width:
        raise RuntimeError(f"{name}: rows={rows}, width={width} at column {first} do not fit a pitch of {pitch}")
    need = 0 if rows == 0 else (rows - 1) * pitch + first + width
    if t.numel() < need:
        raise RuntimeError(f"{name}: {t.numel()} elements, but {rows} rows of {width} at pitch {pitch} (+{first}) need {need}")
    return t


def _resid_ptr(resid: Optional[torch.Tensor], ldr: int, first: int, m: int, n: int, device):
    """Address of element `first` of the residual buffer (None: no residual) after checking that m rows of n at pitch ldr fit."""
    if resid is None:
        return None
    _need(resid, "resid", torch.float32, None, device)
    if ldr < n or first < 0 or resid.numel() < (0 if m == 0 else (m - 1) * ldr + first + n):
        raise RuntimeError(f"resid: {resid.numel()} elements do not hold {m} rows of {n} at pitch {ldr} (+{first})")
    return C.c_void_p(resid.data_ptr() + 4 * first)


def gemm_residual(a: torch.Tensor, lda: int, w_kmajor: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, ldc: int,
                  c0: int, m: int, relu: bool = False, resid: Optional[torch.Tensor] = None, ldr: int = 0, resid_first: int = 0):
    """out[:m, c0 : c0 + N] (pitch ldc) = act(a[:m, :K] (pitch lda) @ w_kmajor[K, N] + bias) + resid[:m, :N] (pitch ldr, from element
    resid_first of its buffer) on t2p_gemm_residual.  a, out and resid are contiguous buffers of any shape, addressed through the
    pitches; everything of `out` outside the window stays as it is.  resid may be `out` itself (resid_first = c0, ldr = ldc)."""
    _need(w_kmajor, "w", torch.float32, 2, a.device)
    k, n = w_kmajor.shape
    _need_span(a, "a", m, lda, k)
    _need_span(out, "out", m, ldc, n, device=a.device, first=c0)
    if bias is not None and _need(bias, "bias", torch.float32, 1, a.device).numel() != n:
        raise RuntimeError(f"gemm_residual: bias has {bias.numel()} elements, n = {n}")
    r_ptr = _resid_ptr(resid, ldr, resid_first, m, n, a.device)
    L.check(L.lib().t2p_gemm_residual(_ptr(a), lda, _ptr(w_kmajor), _ptr(bias), _ptr(out), ldc, c0, m, k, n, int(relu), r_ptr, ldr,
                                      _stream(a.device)), "t2p_gemm_residual")
    return out


def gemm_x3(a: torch.Tensor, lda: int, wx: torch.Tensor, scale: float, bias: Optional[torch.Tensor], out: torch.Tensor, ldc: int,
            c0: int, m: int, k: int, n: int, relu: bool = False, resid: Optional[torch.Tensor] = None, ldr: int = 0,
            resid_first: int = 0, amax_in: Optional[torch.Tensor] = None):
    """gemm_residual on the f16x3 matrix path (t2p_gemm_x3): wx is packing.pack_gemm_x3(w_kmajor[k, n], scale) on the device,
    amax_in an optional int32 [1] guard word that the kernel raises to the bit pattern of max |a[:m, :k]|."""
    _need(wx, "wx", torch.int16, 3, a.device)
    if tuple(wx.shape) != (2, n, (k + 31) // 32 * 32):
        raise RuntimeError(f"gemm_x3: wx is {tuple(wx.shape)}, the image of a [{k}, {n}] weight is {(2, n, (k + 31) // 32 * 32)}")
    _need_span(a, "a", m, lda, k)
    _need_span(out, "out", m, ldc, n, device=a.device, first=c0)
    if bias is not None and _need(bias, "bias", torch.float32, 1, a.device).numel() != n:
        raise RuntimeError(f"gemm_x3: bias has {bias.numel()} elements, n = {n}")
    r_ptr = _resid_ptr(resid, ldr, resid_first, m, n, a.device)
    if amax_in is not None and _need(amax_in, "amax_in", torch.int32, 1, a.device).numel() != 1:
        raise RuntimeError("gemm_x3: amax_in is one int32 word")
    L.check(L.lib().t2p_gemm_x3(_ptr(a), lda, _ptr(wx), float(scale), _ptr(bias), _ptr(out), ldc, c0, m, k, n, int(relu), r_ptr, ldr,
                                _ptr(amax_in), _stream(a.device)), "t2p_gemm_x3")
    return out


def gemm_skinny(a: torch.Tensor, lda: int, w_kmajor: torch.Tensor, out: torch.Tensor, ldc: int, m: int):
    """out[:m, :N] (pitch ldc) = a[:m, :K] (pitch lda) @ w_kmajor[K, N] on the few-rows kernel of the training-mode LSTM
    (t2p_gemm_skinny)."""
    _need(w_kmajor, "w", torch.float32, 2, a.device)
    k, n = w_kmajor.shape
    _need_span(a, "a", m, lda, k)
    _need_span(out, "out", m, ldc, n, device=a.device)
    L.check(L.lib().t2p_gemm_skinny(_ptr(a), lda, _ptr(w_kmajor), _ptr(out), ldc, m, k, n, _stream(a.device)), "t2p_gemm_skinny")
    return out


def gemm_tn(a: torch.Tensor, b: torch.Tensor, k1: Optional[int] = None, n: Optional[int] = None, out: Optional[torch.Tensor] = None):
    """a[M, K1]^T @ b[M, N] -> [K1, N] (t2p_gemm_tn): rows split over the grid, partials added in a fixed order.  The
    weight-gradient products of the training-mode path (dW = dY^T X, ...): no transposed copy, no library GEMM.
    Pitches: with k1 / n the operands are the first k1 / n columns of a / b, whose row lengths are the pitches lda / ldb; with
    `out` ([K1, ldc] float32) the product goes into its first n columns and the others stay as they are."""
    _need(a, "a", torch.float32, 2)
    _need(b, "b", torch.float32, 2, a.device)
    m, lda = a.shape
    if b.shape[0] != m:
        raise RuntimeError(f"gemm_tn: a is [{m},{lda}] but b is {tuple(b.shape)}")
    ldb = b.shape[1]
    k1, n = lda if k1 is None else int(k1), ldb if n is None else int(n)
    if not (1 <= k1 <= lda and 1 <= n <= ldb):
        raise RuntimeError(f"gemm_tn: k1={k1}, n={n} do not fit the operands' rows of {lda} and {ldb}")
    if out is None:
        out = torch.empty((k1, n), dtype=torch.float32, device=a.device)
    elif _need(out, "out", torch.float32, 2, a.device).shape[0] != k1 or out.shape[1] < n:
        raise RuntimeError(f"gemm_tn: out is {tuple(out.shape)}, the product is [{k1},{n}]")
    if m == 0:
        out[:, :n] = 0
        return out
    ws = torch.empty((L.lib().t2p_gemm_tn_workspace_bytes(m, k1, n),), dtype=torch.uint8, device=a.device)
    L.check(L.lib().t2p_gemm_tn(_ptr(a), lda, _ptr(b), ldb, _ptr(out), out.shape[1], m, k1, n, _ptr(ws), ws.numel(),
                                _stream(a.device)), "t2p_gemm_tn")
    return out


def linear_wgrad(dy: torch.Tensor, x: torch.Tensor, want_colsum: bool = True, k1: Optional[int] = None, n: Optional[int] = None,
                 out: Optional[torch.Tensor] = None):
    """(dy[M, K1]^T @ x[M, N] -> [K1, N], column sums of dy [K1] or None) in one pass over the rows (t2p_linear_wgrad_f32): the
    weight and bias gradients of a Linear.  Row pitches must be multiples of 4 floats (the layers of the path are; a whole
    operand of another width is zero-padded here).  Pitches as in gemm_tn: k1 / n select the first columns of dy / x, whose row
    lengths are lda / ldb (multiples of 4 then); `out` [K1, ldc] takes the product in its first n columns."""
    _need(dy, "dy", torch.float32, 2)
    _need(x, "x", torch.float32, 2, dy.device)
    m = dy.shape[0]
    if x.shape[0] != m:
        raise RuntimeError(f"linear_wgrad: dy is [{m},{dy.shape[1]}] but x is {tuple(x.shape)}")
    pitched = k1 is not None or n is not None
    k1, n = dy.shape[1] if k1 is None else int(k1), x.shape[1] if n is None else int(n)
    if not (1 <= k1 <= dy.shape[1] and 1 <= n <= x.shape[1]):
        raise RuntimeError(f"linear_wgrad: k1={k1}, n={n} do not fit the operands' rows of {dy.shape[1]} and {x.shape[1]}")
    if pitched and (dy.shape[1] % 4 or x.shape[1] % 4):
        raise RuntimeError(f"linear_wgrad: pitches {dy.shape[1]} and {x.shape[1]} must be multiples of 4")
    if dy.shape[1] % 4:
        dy = torch.nn.functional.pad(dy, (0, (-k1) % 4)).contiguous()
    if x.shape[1] % 4:
        x = torch.nn.functional.pad(x, (0, (-n) % 4)).contiguous()
    if out is None:
        out = torch.empty((k1, n), dtype=torch.float32, device=dy.device)
    elif _need(out, "out", torch.float32, 2, dy.device).shape[0] != k1 or out.shape[1] < n:
        raise RuntimeError(f"linear_wgrad: out is {tuple(out.shape)}, the product is [{k1},{n}]")
    colsum = torch.empty((k1,), dtype=torch.float32, device=dy.device) if want_colsum else None
    ws = torch.empty((L.lib().t2p_linear_wgrad_workspace_bytes(m, k1, n),), dtype=torch.uint8, device=dy.device)
    L.check(L.lib().t2p_linear_wgrad_f32(_ptr(dy), dy.shape[1], _ptr(x), x.shape[1], _ptr(out), out.shape[1], _ptr(colsum), m, k1, n,
                                         _ptr(ws), ws.numel(), _stream(dy.device)), "t2p_linear_wgrad_f32")
    return out, colsum


def rownorm(x: torch.Tensor) -> torch.Tensor:
    _need(x, "x", torch.float32, 2)
    out = torch.empty_like(x)
    L.check(L.lib().t2p_rownorm(_ptr(x), x.shape[0], x.shape[1], _ptr(out), _stream(x.device)), "t2p_rownorm")
    return out


def _sim_topk_call(entry: str, queries: torch.Tensor, cells: torch.Tensor, k: int, index_offset: int, extra=None, skip_empty=False):
    """What sim_topk, sim_topk_grouped and sim_topk_prior share: the checks of queries / cells, the outputs, the workspace and the
    call of t2p_<entry>.  extra(nq, nc, dev) validates the wrapper's own tensors and returns them in the entry point's order (they
    follow `cells`); skip_empty: nq == 0 returns the empty outputs without the call."""
    _need(queries, "queries", torch.float32, 2)
    _need(cells, "cells", torch.float32, 2, queries.device)
    nq, dim = queries.shape
    nc = cells.shape[0]
    if cells.shape[1] != dim:
        raise RuntimeError(f"{entry}: queries have dim {dim}, cells {cells.shape[1]}")
    dev = queries.device
    more = extra(nq, nc, dev) if extra else ()
    idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
    score = torch.empty((nq, k), dtype=torch.float64, device=dev)
    if nq == 0 and skip_empty:
        return idx, score
    nbytes = L.lib().t2p_sim_topk_workspace_bytes(nq, nc, k)
    ws = workspace(dev, nbytes, "sim_topk")
    L.check(getattr(L.lib(), "t2p_" + entry)(_ptr(queries), _ptr(cells), *[_ptr(t) for t in more], nq, nc, dim, k, int(index_offset),
                                             _ptr(idx), _ptr(score), _ptr(ws), ws.numel(), _stream(dev)), "t2p_" + entry)
    return idx, score


def _need_groups(entry: str, query_group, cell_group, nq: int, nc: int, dev):
    _need(query_group, "query_group", torch.int32, 1, dev)
    _need(cell_group, "cell_group", torch.int32, 1, dev)
    if query_group.shape[0] != nq or cell_group.shape[0] != nc:
        raise RuntimeError(f"{entry}: {query_group.shape[0]} query groups for {nq} queries, "
                           f"{cell_group.shape[0]} cell groups for {nc} cells")


def sim_topk(queries: torch.Tensor, cells: torch.Tensor, k: int, index_offset: int = 0):
    """Float64 cosine scores + ordered top-k (ties -> lower index).  Returns (idx int64 [nq,k], score f64 [nq,k])."""
    return _sim_topk_call("sim_topk", queries, cells, k, index_offset)


def sim_topk_grouped(queries: torch.Tensor, cells: torch.Tensor, query_group: torch.Tensor, cell_group: torch.Tensor, k: int,
                     index_offset: int = 0):
    """sim_topk over the effective score `cell_group[c] == query_group[q] ? score : -inf` (int32 group ids, [nq] and [nc]):
    a query's own group first, then masked cells at -inf by ascending index.  Returns (idx int64 [nq,k], score f64 [nq,k])."""
    def groups(nq, nc, dev):
        _need_groups("sim_topk_grouped", query_group, cell_group, nq, nc, dev)
        return query_group, cell_group
    return _sim_topk_call("sim_topk_grouped", queries, cells, k, index_offset, groups)


def sim_topk_prior(queries: torch.Tensor, cells: torch.Tensor, k: int, index_offset: int = 0, *, query_xy=None, query_radius=None,
                   cell_box=None, query_group=None, cell_group=None):
    """sim_topk over the pairs a query's prior allows (t2p_sim_topk_prior, include/t2p_serve.h): the prior point query_xy [nq, 2]
    lies within query_radius [nq] of the cell's closed square cell_box [nc, 4] = x0 y0 x1 y1 (float64, all three or none), and
    query_group [nq] is negative or equals cell_group [nc] (int32, both or none).  Every other pair scores -inf: a query's
    allowed cells first, then masked cells at -inf by ascending index.  Returns (idx int64 [nq,k], score f64 [nq,k])."""
    def prior(nq, nc, dev):
        geo = (query_xy, query_radius, cell_box)
        if any(t is None for t in geo) != all(t is None for t in geo):
            raise RuntimeError("sim_topk_prior: query_xy, query_radius and cell_box go together")
        if (query_group is None) != (cell_group is None):
            raise RuntimeError("sim_topk_prior: query_group and cell_group go together")
        if cell_box is None and cell_group is None:
            raise RuntimeError("sim_topk_prior: neither geometry nor groups given: call sim_topk")
        if cell_box is not None:
            _need(query_xy, "query_xy", torch.float64, 2, dev)
            _need(query_radius, "query_radius", torch.float64, 1, dev)
            _need(cell_box, "cell_box", torch.float64, 2, dev)
            if tuple(query_xy.shape) != (nq, 2) or query_radius.shape[0] != nq or tuple(cell_box.shape) != (nc, 4):
                raise RuntimeError(f"sim_topk_prior: query_xy {tuple(query_xy.shape)}, query_radius {tuple(query_radius.shape)}, cell_box "
                                   f"{tuple(cell_box.shape)} for {nq} queries and {nc} cells: expected ({nq}, 2), ({nq},), ({nc}, 4)")
        if cell_group is not None:
            _need_groups("sim_topk_prior", query_group, cell_group, nq, nc, dev)
        return query_xy, query_radius, cell_box, query_group, cell_group
    # (skip_empty: an empty tensor has no address: the entry point would read a partial pointer set)
    return _sim_topk_call("sim_topk_prior", queries, cells, k, index_offset, prior, skip_empty=True)


# ---------------------------------------------------------------------------------------------------------------
def make_cell_config(n_pts=256, embed_dim=256, pointnet_features=2, use_features=("class", "color", "position"),
                     self_loops=True, knn_k=8, variation=0, radius=(0.2, 0.3, 0.4), chunk_objects=0,
                     precision="f16x3", class_idx=None, color_idx=None, objects_only=False,
                     overflow_flag=None, tuning=0) -> L.CellConfig:
    """class_idx / color_idx: int32 device tensors [n_obj] enabling the --class_embed / --color_embed ablations.
    overflow_flag: int32 device tensor [1], the sticky fp16-range guard word of the f16x3 path (include/t2p.h)."""
    cfg = L.CellConfig()
    cfg.n_pts, cfg.embed_dim, cfg.pointnet_features = int(n_pts), int(embed_dim), int(pointnet_features)
    cfg.use_class = int("class" in use_features)
    cfg.use_color = int("color" in use_features)
    cfg.use_position = int("position" in use_features)
    cfg.self_loops, cfg.knn_k, cfg.variation = int(bool(self_loops)), int(knn_k), int(variation)
    cfg.radius = (C.c_float * 3)(*[float(r) for r in radius])
    cfg.chunk_objects = int(chunk_objects)
    cfg.objects_only = int(bool(objects_only))
    if precision not in ("fp32", "f16x3"):
        raise RuntimeError(f"precision must be 'fp32' or 'f16x3', got {precision!r}")
    cfg.precision = 1 if precision == "f16x3" else 0
    for name, t in (("class", class_idx), ("color", color_idx)):
        if t is not None:
            _need(t, name + "_idx", torch.int32, 1)
            setattr(cfg, name + "_embed", 1)
            setattr(cfg, name + "_idx", t.data_ptr())
    cfg.tuning = int(tuning)
    if overflow_flag is not None:
        _need(overflow_flag, "overflow_flag", torch.int32, 1)
        cfg.overflow_flag = overflow_flag.data_ptr()
    cfg._keepalive = (class_idx, color_idx, overflow_flag)
    return cfg


def make_cell_weights(packed: Dict[str, object]) -> L.CellWeights:
    """packed: name -> tensor (or list of 3 tensors for the sa_* members), fp32 contiguous on the GPU."""
    w = L.CellWeights()
    fields = L.CellWeights._fields_   # the fp32 matrices lead the struct, up to the first split-precision image
    for name, ctype in fields[:[n for n, _ in fields].index("sa_w2_x3")]:
        if issubclass(ctype, C.Array):          # const float* name[3]: one per SA level
            ts = packed[name]
            for t in ts:
                _need(t, name, torch.float32)
            setattr(w, name, ctype(*[t.data_ptr() for t in ts]))
        else:                                   # const float* name
            t = packed.get(name)
            if t is not None:
                _need(t, name, torch.float32)
            setattr(w, name, 0 if t is None else t.data_ptr())
    for name in ("sa_w2_x3", "sa_w1_x3"):
        x3 = packed.get(name)
        if x3 is not None:
            for t in x3:
                if t is not None:
                    _need(t, name, torch.int16)
            setattr(w, name, (C.c_void_p * 3)(*[0 if t is None else t.data_ptr() for t in x3]))
    if packed.get("sa_b2_x3") is not None:
        for t in packed["sa_b2_x3"]:
            _need(t, "sa_b2_x3", torch.float32)
        w.sa_b2_x3 = (C.c_void_p * 3)(*[t.data_ptr() for t in packed["sa_b2_x3"]])
        w.sa_w2_scale = (C.c_float * 3)(*[float(v) for v in packed["sa_w2_scale"]])
    for name in ("lin1", "lin2", "merge", "pn", "g_wp", "g_wq"):
        img = packed.get(name + "_x3")
        if img is not None:
            _need(img, name + "_x3", torch.int16)
            setattr(w, name + "_x3", img.data_ptr())
            setattr(w, name + "_scale", float(packed[name + "_scale"]))
    for name in ("ga_w1_x3", "ga_w2_x3", "g_w2_x3"):
        g = packed.get(name)
        if g is not None:
            _need(g, name, torch.int16)
            setattr(w, name, g.data_ptr())
    if packed.get("ga_w1_l1") is not None:
        w.ga_w1_l1, w.ga_b1_absmax = float(packed["ga_w1_l1"]), float(packed["ga_b1_absmax"])
        w.sa_wp_l1 = (C.c_float * 3)(*[float(v) for v in packed["sa_wp_l1"]])
        w.sa_a1_l1, w.sa_b1_absmax = float(packed["sa_a1_l1"]), float(packed["sa_b1_absmax"])
    for name in ("class_embedding", "color_embedding"):
        t = packed.get(name)
        if t is not None:
            _need(t, name, torch.float32, 2)
            setattr(w, name, t.data_ptr())
    return w


HEAD_TRACE = ("head_in", "head_edge", "head_pool", "head_l1", "head_l2")   # t2p_cell_trace: the cell head's stage outputs


def encode_cells(xyz, rgb, center, mean_rgb, cell_ptr_host: np.ndarray, cell_ptr_dev, weights: L.CellWeights,
                 cfg: L.CellConfig, want_trace=False, ws_tag: str = "encode_cells"):
    """Cell branch on packed, device-resident inputs.  Returns out [n_cells, D] (and a dict of stage outputs when
    want_trace is True or names some of them; knn_idx rows are local to the internal chunk of <= chunk_objects objects)."""
    _need(xyz, "xyz", torch.float32, 3)
    dev = xyz.device
    _need(rgb, "rgb", torch.float32, 3, dev)
    _need(center, "center", torch.float32, 2, dev)
    _need(mean_rgb, "mean_rgb", torch.float32, 2, dev)
    _need(cell_ptr_dev, "cell_ptr", torch.int32, 1, dev)
    n_obj, n_pts = xyz.shape[0], xyz.shape[1]
    if tuple(rgb.shape) != tuple(xyz.shape) or xyz.shape[2] != 3:
        raise RuntimeError(f"encode_cells: xyz {tuple(xyz.shape)} / rgb {tuple(rgb.shape)} must both be [n_obj, n_pts, 3]")
    if tuple(center.shape) != (n_obj, 3) or tuple(mean_rgb.shape) != (n_obj, 3):
        raise RuntimeError("encode_cells: center / mean_rgb must be [n_obj, 3]")
    for name in ("class", "color"):
        if getattr(cfg, name + "_embed") and cfg._keepalive[0 if name == "class" else 1].numel() != n_obj:
            raise RuntimeError(f"encode_cells: {name}_idx must have one entry per object")
    if n_pts != cfg.n_pts:
        raise RuntimeError(f"encode_cells: objects have {n_pts} points, config says {cfg.n_pts}")
    cp = np.ascontiguousarray(cell_ptr_host, dtype=np.int32)
    n_cells = cp.shape[0] - 1
    if cell_ptr_dev.numel() != n_cells + 1:
        raise RuntimeError("encode_cells: host and device cell_ptr differ in length")
    D = cfg.embed_dim
    out = None if cfg.objects_only else torch.empty((n_cells, D), dtype=torch.float32, device=dev)
    trace, tr = None, None
    if cfg.objects_only:  # ObjectEncoder.forward only: the [n_obj, D] result comes back through the trace slot
        if want_trace:
            raise RuntimeError("encode_cells: objects_only returns the object embeddings only")
        tr = L.CellTrace()
        obj_emb = torch.empty((n_obj, D), dtype=torch.float32, device=dev)
        tr.obj_emb = obj_emb.data_ptr()
    elif want_trace:
        # want_trace: True = every stage output, or an iterable of names (the full set is ~130 KB per object)
        # (True keeps its meaning: the stages up to the kNN graph; the cell head's stages HEAD_TRACE are asked for by name)
        names = set(("fps_idx", "nbr", "cnt", "sa_out", "features0", "features1", "features2", "obj_emb", "knn_idx")
                    if want_trace is True else want_trace)
        unknown = names - {"fps_idx", "nbr", "cnt", "sa_out", "features0", "features1", "features2", "obj_emb", "knn_idx", *HEAD_TRACE}
        if unknown:
            raise RuntimeError(f"encode_cells: unknown trace outputs {sorted(unknown)}")
        tr = L.CellTrace()
        trace = {}
        per_level, arr = _level_tables(n_obj, n_pts, dev, [k for k in ("fps_idx", "nbr", "cnt", "sa_out") if k in names], torch.zeros)
        trace.update(per_level)
        for name in per_level:
            setattr(tr, name, arr[name])
        flat = {"features0": ((n_obj, 1024), torch.float32), "features1": ((n_obj, 512), torch.float32),
                "features2": ((n_obj, 256), torch.float32), "obj_emb": ((n_obj, D), torch.float32),
                "knn_idx": ((n_obj, cfg.knn_k), torch.int32),
                "head_in": ((n_obj, D), torch.float32), "head_edge": ((n_obj, D), torch.float32),
                "head_pool": ((n_cells, D), torch.float32), "head_l1": ((n_cells, D), torch.float32),
                "head_l2": ((n_cells, D), torch.float32)}
        for name, (shape, dt) in flat.items():
            if name in names:
                trace[name] = torch.empty(shape, dtype=dt, device=dev)
                setattr(tr, name, trace[name].data_ptr())
    nbytes = L.lib().t2p_encode_cells_workspace_bytes(n_obj, n_cells, C.byref(cfg))
    # a single cell larger than the chunk forms its own (bigger) chunk: size for it
    biggest = int((cp[1:] - cp[:-1]).max()) if n_cells > 0 else 0
    chunk = cfg.chunk_objects if cfg.chunk_objects > 0 else DEFAULT_CHUNK_OBJECTS
    if biggest > chunk:
        big_cfg = L.CellConfig.from_buffer_copy(cfg)
        big_cfg.chunk_objects = biggest
        nbytes = max(nbytes, L.lib().t2p_encode_cells_workspace_bytes(n_obj, n_cells, C.byref(big_cfg)))
    ws = workspace(dev, nbytes, ws_tag)   # (one scratch buffer per tag: concurrent calls on two streams need two tags)
    rc = L.lib().t2p_encode_cells(_ptr(xyz), _ptr(rgb), _ptr(center), _ptr(mean_rgb),
                                  cp.ctypes.data_as(C.c_void_p), _ptr(cell_ptr_dev), n_obj, n_cells, C.byref(weights),
                                  C.byref(cfg), _ptr(out) if out is not None else None,
                                  C.byref(tr) if tr is not None else None, _ptr(ws),
                                  ws.numel(), _stream(dev))
    L.check(rc, "t2p_encode_cells")
    if cfg.objects_only:
        return obj_emb
    return (out, trace) if want_trace else out


MAX_HEAD_COLUMNS = 64   # include/t2p.h: n_classes, n_colors of t2p_classifier_heads


def pointnet2_forward(xyz, rgb, weights: L.CellWeights, cfg: L.CellConfig, head_w=None, head_b=None, n_classes: int = 0,
                      n_colors: int = 0, ws_tag: str = "pointnet2"):
    """PointNet2.forward in eval mode on packed, device-resident inputs (t2p_pointnet2_forward): the whole batch is ONE cell.
    xyz / rgb [n, P, 3]; head_w [256, n_classes + n_colors] k-major and head_b, or None for the trunk alone.
    Returns dict(features0 [n, 1024], features1 [n, 512], features2 [n, 256][, class_pred [n, n_classes], color_pred])."""
    _need(xyz, "xyz", torch.float32, 3)
    dev = xyz.device
    _need(rgb, "rgb", torch.float32, 3, dev)
    n, n_pts = xyz.shape[0], xyz.shape[1]
    if tuple(rgb.shape) != tuple(xyz.shape) or xyz.shape[2] != 3:
        raise RuntimeError(f"pointnet2_forward: xyz {tuple(xyz.shape)} / rgb {tuple(rgb.shape)} must both be [n_obj, n_pts, 3]")
    if n_pts != cfg.n_pts:
        raise RuntimeError(f"pointnet2_forward: objects have {n_pts} points, config says {cfg.n_pts}")
    out = dict(features0=torch.empty((n, 1024), dtype=torch.float32, device=dev),
               features1=torch.empty((n, 512), dtype=torch.float32, device=dev),
               features2=torch.empty((n, 256), dtype=torch.float32, device=dev))
    if head_w is not None:
        _need(head_w, "head_w", torch.float32, 2, dev)
        _need(head_b, "head_b", torch.float32, 1, dev)
        if tuple(head_w.shape) != (256, n_classes + n_colors) or head_b.numel() != n_classes + n_colors:
            raise RuntimeError(f"pointnet2_forward: head_w {tuple(head_w.shape)} is not [256, {n_classes} + {n_colors}]")
        out["class_pred"] = torch.empty((n, n_classes), dtype=torch.float32, device=dev)
        out["color_pred"] = torch.empty((n, n_colors), dtype=torch.float32, device=dev)
    ws = workspace(dev, L.lib().t2p_pointnet2_workspace_bytes(n, C.byref(cfg)), ws_tag)
    rc = L.lib().t2p_pointnet2_forward(_ptr(xyz), _ptr(rgb), n, C.byref(weights), C.byref(cfg), _ptr(head_w), _ptr(head_b),
                                       int(n_classes), int(n_colors), _ptr(out["features0"]), _ptr(out["features1"]),
                                       _ptr(out["features2"]), _ptr(out.get("class_pred")), _ptr(out.get("color_pred")),
                                       _ptr(ws), ws.numel(), _stream(dev))
    L.check(rc, "t2p_pointnet2_forward")
    return out


def classifier_heads(features2, head_w, head_b, n_classes: int, n_colors: int):
    """features2 [n, 256] -> (class_pred [n, n_classes], color_pred [n, n_colors]) on t2p_classifier_heads; head_w
    [256, n_classes + n_colors] k-major (the two heads side by side), head_b [n_classes + n_colors]."""
    _need(features2, "features2", torch.float32, 2)
    dev = features2.device
    _need(head_w, "head_w", torch.float32, 2, dev)
    _need(head_b, "head_b", torch.float32, 1, dev)
    n = features2.shape[0]
    if features2.shape[1] != 256 or tuple(head_w.shape) != (256, n_classes + n_colors) or head_b.numel() != n_classes + n_colors:
        raise RuntimeError(f"classifier_heads: features2 {tuple(features2.shape)} / head_w {tuple(head_w.shape)} / head_b "
                           f"{tuple(head_b.shape)} do not fit [n, 256] x [256, {n_classes} + {n_colors}]")
    class_pred = torch.empty((n, n_classes), dtype=torch.float32, device=dev)
    color_pred = torch.empty((n, n_colors), dtype=torch.float32, device=dev)
    L.check(L.lib().t2p_classifier_heads(_ptr(features2), _ptr(head_w), _ptr(head_b), n, int(n_classes), int(n_colors),
                                         _ptr(class_pred), _ptr(color_pred), _stream(dev)), "t2p_classifier_heads")
    return class_pred, color_pred


def softmax_xent(logits: torch.Tensor, labels: torch.Tensor):
    """logits [n, C] fp32 (rows may be strided: a column slice of a wider matrix), labels int32 [n] ->
    (row_loss [n], d_logits [n, C] = d mean-loss / d logits, correct int32 [n]) of t2p_softmax_xent."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.stride(1) != 1:
        raise RuntimeError("softmax_xent: logits must be a [n, C] tensor with unit column stride")
    if not logits.is_cuda or logits.dtype != torch.float32:
        raise RuntimeError(f"softmax_xent: logits must be fp32 on the GPU (got {logits.dtype} on {logits.device}); there is no CPU path")
    dev = logits.device
    _need(labels, "labels", torch.int32, 1, dev)
    n, c = logits.shape
    if labels.numel() != n:
        raise RuntimeError(f"softmax_xent: {n} rows of logits but {labels.numel()} labels")
    if c < 1:
        raise RuntimeError("softmax_xent: no classes")
    ld = logits.stride(0) if n > 1 else c
    if ld < c:
        raise RuntimeError("softmax_xent: rows of logits overlap")
    row_loss = torch.empty((n,), dtype=torch.float32, device=dev)
    d_logits = torch.empty((n, c), dtype=torch.float32, device=dev)
    correct = torch.empty((n,), dtype=torch.int32, device=dev)
    L.check(L.lib().t2p_softmax_xent(_ptr(logits), int(ld), _ptr(labels), n, c, _ptr(row_loss), _ptr(d_logits), c, _ptr(correct),
                                     _stream(dev)), "t2p_softmax_xent")
    return row_loss, d_logits, correct


def pack_objects(raw_xyz, raw_rgb, obj_ptr, sample_idx, rot=None):
    """Device-side FixedPoints gather (+ RandomRotate about z) + NormalizeScale + per-object means.  raw_xyz/raw_rgb
    [Np,3] fp32, obj_ptr [Nobj+1] int32, sample_idx [Nobj,P] int32 (local indices), rot None or [Nobj,2] fp32 (cos, sin
    of each object's angle, data.draw_rotations).  Returns (xyz [Nobj,P,3], rgb [Nobj,P,3], center, mean_rgb)."""
    _need(raw_xyz, "raw_xyz", torch.float32, 2)
    dev = raw_xyz.device
    _need(raw_rgb, "raw_rgb", torch.float32, 2, dev)
    _need(obj_ptr, "obj_ptr", torch.int32, 1, dev)
    _need(sample_idx, "sample_idx", torch.int32, 2, dev)
    n_obj, n_pts = sample_idx.shape
    if obj_ptr.numel() != n_obj + 1 or tuple(raw_rgb.shape) != tuple(raw_xyz.shape) or raw_xyz.shape[1] != 3:
        raise RuntimeError("pack_objects: inconsistent shapes")
    if rot is not None:
        _need(rot, "rot", torch.float32, 2, dev)
        if tuple(rot.shape) != (n_obj, 2):
            raise RuntimeError("pack_objects: rot must be [n_obj, 2]")
    xyz = torch.empty((n_obj, n_pts, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((n_obj, n_pts, 3), dtype=torch.float32, device=dev)
    center = torch.empty((n_obj, 3), dtype=torch.float32, device=dev)
    mean_rgb = torch.empty((n_obj, 3), dtype=torch.float32, device=dev)
    L.check(L.lib().t2p_pack_objects(_ptr(raw_xyz), _ptr(raw_rgb), _ptr(obj_ptr), _ptr(sample_idx),
                                     _ptr(rot) if rot is not None else None, n_obj, n_pts,
                                     _ptr(xyz), _ptr(rgb), _ptr(center), _ptr(mean_rgb), _stream(dev)), "t2p_pack_objects")
    return xyz, rgb, center, mean_rgb


def pack_scene_objects(raw_xyz, raw_rgb, obj_ptr, obj_id, key, scene_center, scene_color, n_pts: int = 256, want_rgb: bool = True,
                       want_idx: bool = False):
    """The dataloader of a scene resident in HBM (t2p_pack_scene_objects, include/t2p.h): output slot s = scene object
    obj_id[s] (int32 [n_out]) resampled to n_pts points by the counter-based draw of key[s] (int64 / uint64 bit pattern
    [n_out]), NormalizeScale'd bit for bit like the host chain; centre / mean colour gathered from the scene's tables.
    Returns (xyz, rgb | None, center, mean_rgb[, sample_idx])."""
    _need(raw_xyz, "raw_xyz", torch.float32, 2)
    dev = raw_xyz.device
    _need(raw_rgb, "raw_rgb", torch.float32, 2, dev)
    _need(obj_ptr, "obj_ptr", torch.int32, 1, dev)
    _need(obj_id, "obj_id", torch.int32, 1, dev)
    _need(key, "key", torch.int64, 1, dev)
    _need(scene_center, "scene_center", torch.float32, 2, dev)
    _need(scene_color, "scene_color", torch.float32, 2, dev)
    n_out = obj_id.shape[0]
    if key.shape[0] != n_out or tuple(raw_rgb.shape) != tuple(raw_xyz.shape) or raw_xyz.shape[1] != 3 or \
            scene_center.shape[0] != obj_ptr.shape[0] - 1 or tuple(scene_color.shape) != tuple(scene_center.shape):
        raise RuntimeError("pack_scene_objects: inconsistent shapes")
    xyz = torch.empty((n_out, n_pts, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((n_out, n_pts, 3), dtype=torch.float32, device=dev) if want_rgb else None
    center = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    mean_rgb = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((n_out, n_pts), dtype=torch.int32, device=dev) if want_idx else None
    L.check(L.lib().t2p_pack_scene_objects(_ptr(raw_xyz), _ptr(raw_rgb), _ptr(obj_ptr), _ptr(obj_id), _ptr(key), _ptr(scene_center),
                                           _ptr(scene_color), n_out, n_pts, _ptr(xyz), _ptr(rgb) if want_rgb else None,
                                           _ptr(center), _ptr(mean_rgb), _ptr(idx) if want_idx else None, _stream(dev)),
            "t2p_pack_scene_objects")
    return (xyz, rgb, center, mean_rgb, idx) if want_idx else (xyz, rgb, center, mean_rgb)


def pack_scene_objects_aug(raw_xyz, raw_rgb, raw_mirror_xy, obj_ptr, obj_id, key, flip, rot, scene_center, scene_center_mirror_xy,
                           scene_color, n_pts: int = 256, want_rgb: bool = True, want_idx: bool = False):
    """pack_scene_objects with the training augmentation (t2p_pack_scene_objects_aug, include/t2p.h): flip None or uint8 [n_out]
    (bit 0 = x mirrored, bit 1 = y mirrored; needs the scene's mirror tables raw_mirror_xy [R, 2] / scene_center_mirror_xy
    [M, 2]), rot None or fp32 [n_out, 2] (cos, sin per slot, as pack_objects).  Returns what pack_scene_objects returns."""
    _need(raw_xyz, "raw_xyz", torch.float32, 2)
    dev = raw_xyz.device
    _need(raw_rgb, "raw_rgb", torch.float32, 2, dev)
    _need(obj_ptr, "obj_ptr", torch.int32, 1, dev)
    _need(obj_id, "obj_id", torch.int32, 1, dev)
    _need(key, "key", torch.int64, 1, dev)
    _need(scene_center, "scene_center", torch.float32, 2, dev)
    _need(scene_color, "scene_color", torch.float32, 2, dev)
    n_out = obj_id.shape[0]
    if key.shape[0] != n_out or tuple(raw_rgb.shape) != tuple(raw_xyz.shape) or raw_xyz.shape[1] != 3 or \
            scene_center.shape[0] != obj_ptr.shape[0] - 1 or tuple(scene_color.shape) != tuple(scene_center.shape):
        raise RuntimeError("pack_scene_objects_aug: inconsistent shapes")
    if flip is not None:
        if raw_mirror_xy is None or scene_center_mirror_xy is None:
            raise RuntimeError("pack_scene_objects_aug: flip needs the scene's mirror tables (DeviceScene(..., mirror=True))")
        _need(flip, "flip", torch.uint8, 1, dev)
        _need(raw_mirror_xy, "raw_mirror_xy", torch.float32, 2, dev)
        _need(scene_center_mirror_xy, "scene_center_mirror_xy", torch.float32, 2, dev)
        if flip.shape[0] != n_out or tuple(raw_mirror_xy.shape) != (raw_xyz.shape[0], 2) or \
                tuple(scene_center_mirror_xy.shape) != (scene_center.shape[0], 2):
            raise RuntimeError("pack_scene_objects_aug: flip must be [n_out], the mirror tables [R, 2] and [M, 2]")
    if rot is not None:
        _need(rot, "rot", torch.float32, 2, dev)
        if tuple(rot.shape) != (n_out, 2):
            raise RuntimeError("pack_scene_objects_aug: rot must be [n_out, 2]")
    xyz = torch.empty((n_out, n_pts, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((n_out, n_pts, 3), dtype=torch.float32, device=dev) if want_rgb else None
    center = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    mean_rgb = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((n_out, n_pts), dtype=torch.int32, device=dev) if want_idx else None
    opt = lambda t: _ptr(t) if t is not None else None
    L.check(L.lib().t2p_pack_scene_objects_aug(_ptr(raw_xyz), _ptr(raw_rgb), opt(raw_mirror_xy), _ptr(obj_ptr), _ptr(obj_id), _ptr(key),
                                               opt(flip), opt(rot), _ptr(scene_center), opt(scene_center_mirror_xy), _ptr(scene_color),
                                               n_out, n_pts, _ptr(xyz), opt(rgb), _ptr(center), _ptr(mean_rgb), opt(idx), _stream(dev)),
            "t2p_pack_scene_objects_aug")
    return (xyz, rgb, center, mean_rgb, idx) if want_idx else (xyz, rgb, center, mean_rgb)


def make_match_weights(packed: Dict[str, object]) -> L.MatchWeights:
    """packed: packing.pack_match_weights(...)"""
    w = L.MatchWeights()
    cross = np.ascontiguousarray(packed["cross"], dtype=np.int32)
    w.n_layers = int(cross.shape[0])
    w.cross = cross.ctypes.data_as(C.c_void_p)
    for name in ("wqkv", "bqkv", "wm", "bm", "w1", "b1", "w2", "b2", "wf", "bf", "wo1", "bo1", "wo2", "bo2"):
        t = packed[name]
        _need(t, name, torch.float32)
        setattr(w, name, t.data_ptr())
    w.bin_score = float(packed["bin_score"])
    if packed.get("wqkv_x3") is not None:   # f16x3 images of the GNN matrices
        for name, sc in (("wqkv", "qkv"), ("wm", "m"), ("w1", "1"), ("w2", "2"), ("wf", "f")):
            _need(packed[name + "_x3"], name + "_x3", torch.int16)
            setattr(w, name + "_x3", packed[name + "_x3"].data_ptr())
            setattr(w, "scale_" + sc, float(packed["scale_" + sc]))
    w._keepalive = (cross, packed)
    return w


def match(desc0, desc1, weights: L.MatchWeights, sinkhorn_iters: int, threshold: float = 0.2):
    """desc0 [B, M, D] object encodings, desc1 [B, N, D] hint encodings (fp32, L2-normalised, on the GPU).
    Returns dict(P [B, M+1, N+1], matches0 [B, M] int64, matches1 [B, N] int64, matching_scores0/1, offsets [B, N, 2])."""
    _need(desc0, "desc0", torch.float32, 3)
    dev = desc0.device
    _need(desc1, "desc1", torch.float32, 3, dev)
    b, m, d = desc0.shape
    n = desc1.shape[1]
    if desc1.shape[0] != b or desc1.shape[2] != d:
        raise RuntimeError(f"match: desc0 {tuple(desc0.shape)} / desc1 {tuple(desc1.shape)} disagree")
    out = dict(P=torch.empty((b, m + 1, n + 1), dtype=torch.float32, device=dev),
               matches0=torch.empty((b, m), dtype=torch.int64, device=dev),
               matches1=torch.empty((b, n), dtype=torch.int64, device=dev),
               matching_scores0=torch.empty((b, m), dtype=torch.float32, device=dev),
               matching_scores1=torch.empty((b, n), dtype=torch.float32, device=dev),
               offsets=torch.empty((b, n, 2), dtype=torch.float32, device=dev))
    ws = workspace(dev, L.lib().t2p_match_workspace_bytes(b, m, n, d), "match")
    rc = L.lib().t2p_match(_ptr(desc0), _ptr(desc1), b, m, n, d, C.byref(weights), int(sinkhorn_iters), float(threshold),
                           _ptr(out["P"]), _ptr(out["matches0"]), _ptr(out["matches1"]), _ptr(out["matching_scores0"]),
                           _ptr(out["matching_scores1"]), _ptr(out["offsets"]), _ptr(ws), ws.numel(), _stream(dev))
    L.check(rc, "t2p_match")
    return out


def make_text_weights(embedding, w_ih, w_hh, bias, w_hh_x3=None, w_hh_scale=0.0) -> L.TextWeights:
    """w_hh_x3 (int16 device tensor, packing.pack_text_weights(x3=True)) selects the f16x3 recurrence; None = exact fp32."""
    w = L.TextWeights()
    for n, t in (("embedding", embedding), ("w_ih", w_ih), ("w_hh", w_hh), ("bias", bias)):
        _need(t, n, torch.float32)
        setattr(w, n, t.data_ptr())
    if w_hh_x3 is not None:
        _need(w_hh_x3, "w_hh_x3", torch.int16)
        w.w_hh_x3, w.w_hh_scale = w_hh_x3.data_ptr(), float(w_hh_scale)
    return w


def encode_text(tokens: torch.Tensor, lengths: torch.Tensor, weights: L.TextWeights, vocab: int, embed_dim: int,
                want_raw: bool = False):
    """tokens [B, T] int32 right-padded with 0, lengths [B] int32 -> L2-normalised [B, D] (and the raw encoder output)."""
    _need(tokens, "tokens", torch.int32, 2)
    dev = tokens.device
    _need(lengths, "lengths", torch.int32, 1, dev)
    b, t = tokens.shape
    if lengths.numel() != b:
        raise RuntimeError("encode_text: lengths must have one entry per row of tokens")
    out = torch.empty((b, embed_dim), dtype=torch.float32, device=dev)
    raw = torch.empty((b, embed_dim), dtype=torch.float32, device=dev) if want_raw else None
    nbytes = L.lib().t2p_encode_text_workspace_bytes(b, vocab, embed_dim)
    ws = workspace(dev, nbytes, "encode_text")
    L.check(L.lib().t2p_encode_text(_ptr(tokens), _ptr(lengths), b, t, vocab, embed_dim, C.byref(weights), _ptr(raw),
                                    _ptr(out), _ptr(ws), ws.numel(), _stream(dev)), "t2p_encode_text")
    return (out, raw) if want_raw else out


def pairwise_ranking(scores: torch.Tensor, margin: float):
    """scores [B, B] fp32 -> (row_loss [B], d_scores [B, B]) of PairwiseRankingLoss (t2p_pairwise_ranking)."""
    _need(scores, "scores", torch.float32, 2)
    b = scores.shape[0]
    if scores.shape[1] != b:
        raise RuntimeError("pairwise_ranking: scores must be square")
    dev = scores.device
    row_loss = torch.empty((b,), dtype=torch.float32, device=dev)
    row_cnt = torch.empty((b,), dtype=torch.float32, device=dev)
    d_scores = torch.empty_like(scores)
    L.check(L.lib().t2p_pairwise_ranking(_ptr(scores), b, float(margin), _ptr(row_loss), _ptr(d_scores), _ptr(row_cnt),
                                         _stream(dev)), "t2p_pairwise_ranking")
    return row_loss, d_scores


def hardest_ranking(scores: torch.Tensor, margin: float):
    """scores [B, B] fp32 -> (best [2B], d_scores [B, B]) of HardestRankingLoss (t2p_hardest_ranking)."""
    _need(scores, "scores", torch.float32, 2)
    b = scores.shape[0]
    if scores.shape[1] != b:
        raise RuntimeError("hardest_ranking: scores must be square")
    dev = scores.device
    best = torch.empty((2 * b,), dtype=torch.float32, device=dev)
    where = torch.empty((2 * b,), dtype=torch.int32, device=dev)
    d_scores = torch.empty_like(scores)
    L.check(L.lib().t2p_hardest_ranking(_ptr(scores), b, float(margin), _ptr(best), _ptr(where), _ptr(d_scores), _stream(dev)),
            "t2p_hardest_ranking")
    return best, d_scores


def lstm_cell_forward(pre, table, tokens, lengths, step: int, reverse: bool, c_prev, h_prev, gates, c, h):
    """One training-mode LSTM step (t2p_lstm_cell_forward): pre [B,4D] = h_prev @ W_hh^T, table [V,4D]; writes gates
    [B,4D] (i, f, g, o), c, h [B,D] in place."""
    dev = pre.device
    for name, t in (("pre", pre), ("table", table), ("gates", gates)):
        _need(t, name, torch.float32, 2, dev)
    for name, t in (("c_prev", c_prev), ("h_prev", h_prev), ("c", c), ("h", h)):
        _need(t, name, torch.float32, 2, dev)
    _need(tokens, "tokens", torch.int32, 2, dev)
    _need(lengths, "lengths", torch.int32, 1, dev)
    b, d = c.shape
    if tuple(pre.shape) != (b, 4 * d) or tuple(gates.shape) != (b, 4 * d) or table.shape[1] != 4 * d or tokens.shape[0] != b:
        raise RuntimeError("lstm_cell_forward: inconsistent shapes")
    L.check(L.lib().t2p_lstm_cell_forward(_ptr(pre), _ptr(table), _ptr(tokens), _ptr(lengths), b, tokens.shape[1], d,
                                          int(step), int(bool(reverse)), _ptr(c_prev), _ptr(h_prev), _ptr(gates), _ptr(c),
                                          _ptr(h), _stream(dev)), "t2p_lstm_cell_forward")


def lstm_train_loops_supported(d: int) -> bool:
    """Widths the in-library time loops take (16-byte loads of the state rows)."""
    return d % 4 == 0


def lstm_train_forward(table, w_hh_k, tokens, lengths, reverse: bool, gates, cs, hs):
    """All T steps of one direction in ONE call (t2p_lstm_train_forward): table [V,4D], w_hh_k [D,4D]; fills gates [T,B,4D],
    cs / hs [T+1,B,D] (slice 0 = the initial state, left as given)."""
    dev = table.device
    _need(table, "table", torch.float32, 2, dev)
    _need(w_hh_k, "w_hh_k", torch.float32, 2, dev)
    _need(tokens, "tokens", torch.int32, 2, dev)
    _need(lengths, "lengths", torch.int32, 1, dev)
    for name, t in (("gates", gates), ("cs", cs), ("hs", hs)):
        _need(t, name, torch.float32, 3, dev)
    b, t_len = tokens.shape
    d = w_hh_k.shape[0]
    if (tuple(w_hh_k.shape) != (d, 4 * d) or table.shape[1] != 4 * d or tuple(gates.shape) != (t_len, b, 4 * d)
            or tuple(cs.shape) != (t_len + 1, b, d) or tuple(hs.shape) != (t_len + 1, b, d) or lengths.shape[0] != b):
        raise RuntimeError("lstm_train_forward: inconsistent shapes")
    pre = torch.empty((b, 4 * d), dtype=torch.float32, device=dev)
    L.check(L.lib().t2p_lstm_train_forward(_ptr(table), _ptr(w_hh_k), _ptr(tokens), _ptr(lengths), b, t_len, d,
                                           int(bool(reverse)), _ptr(gates), _ptr(cs), _ptr(hs), _ptr(pre), _stream(dev)),
            "t2p_lstm_train_forward")


def lstm_train_backward(dh_last, w_hh_t, gates, cs, lengths, d_pre):
    """The whole backward recurrence of one direction in ONE call (t2p_lstm_train_backward): dh_last [B,D] = gradient of the
    final hidden state, w_hh_t [4D,D]; fills d_pre [T,B,4D]."""
    dev = gates.device
    _need(dh_last, "dh_last", torch.float32, 2, dev)
    _need(w_hh_t, "w_hh_t", torch.float32, 2, dev)
    _need(lengths, "lengths", torch.int32, 1, dev)
    for name, t in (("gates", gates), ("cs", cs), ("d_pre", d_pre)):
        _need(t, name, torch.float32, 3, dev)
    t_len, b, d4 = gates.shape
    d = d4 // 4
    if (tuple(dh_last.shape) != (b, d) or tuple(w_hh_t.shape) != (4 * d, d) or tuple(cs.shape) != (t_len + 1, b, d)
            or tuple(d_pre.shape) != (t_len, b, 4 * d) or lengths.shape[0] != b):
        raise RuntimeError("lstm_train_backward: inconsistent shapes")
    ws = torch.empty((5, b, d), dtype=torch.float32, device=dev)
    L.check(L.lib().t2p_lstm_train_backward(_ptr(dh_last), _ptr(w_hh_t), _ptr(gates), _ptr(cs), _ptr(lengths), b, t_len, d,
                                            _ptr(d_pre), _ptr(ws), _stream(dev)), "t2p_lstm_train_backward")


def lstm_cell_backward(dh_gemm, dh_carry_in, dc_in, gates, c_prev, c, lengths, step: int, d_pre, dc_out, dh_carry_out):
    """Backward of one training-mode LSTM step (t2p_lstm_cell_backward); dh_gemm may be None (last step)."""
    dev = gates.device
    for name, t in (("dh_carry_in", dh_carry_in), ("dc_in", dc_in), ("gates", gates), ("c_prev", c_prev), ("c", c),
                    ("d_pre", d_pre), ("dc_out", dc_out), ("dh_carry_out", dh_carry_out)):
        _need(t, name, torch.float32, 2, dev)
    if dh_gemm is not None:
        _need(dh_gemm, "dh_gemm", torch.float32, 2, dev)
    _need(lengths, "lengths", torch.int32, 1, dev)
    b, d = c.shape
    if tuple(gates.shape) != (b, 4 * d) or tuple(d_pre.shape) != (b, 4 * d):
        raise RuntimeError("lstm_cell_backward: inconsistent shapes")
    L.check(L.lib().t2p_lstm_cell_backward(_ptr(dh_gemm) if dh_gemm is not None else None, _ptr(dh_carry_in), _ptr(dc_in),
                                           _ptr(gates), _ptr(c_prev), _ptr(c), _ptr(lengths), b, d, int(step), _ptr(d_pre),
                                           _ptr(dc_out), _ptr(dh_carry_out), _stream(dev)), "t2p_lstm_cell_backward")


# ---- fine stage in train() mode (csrc/match_train.hip): token rows set-major, see include/t2p.h -----------------------------
def match_attention(qkv: torch.Tensor, batch: int, n_obj: int, n_hints: int, cross: bool) -> torch.Tensor:
    """qkv [B (n_obj + n_hints), 3 D] (q | k | v of the set-major token rows) -> the heads' messages [B (n_obj + n_hints), D] of
    one GNN layer (t2p_match_attention); cross: a token attends to the other set of its sample."""
    _need(qkv, "qkv", torch.float32, 2)
    rows = int(batch) * (int(n_obj) + int(n_hints))
    if qkv.shape[0] != rows or qkv.shape[1] % 3:
        raise RuntimeError(f"match_attention: qkv is {tuple(qkv.shape)}, expected [{rows}, 3 D]")
    d = qkv.shape[1] // 3
    msg = torch.empty((rows, d), dtype=torch.float32, device=qkv.device)
    L.check(L.lib().t2p_match_attention(_ptr(qkv), int(batch), int(n_obj), int(n_hints), d, int(bool(cross)), _ptr(msg),
                                        _stream(qkv.device)), "t2p_match_attention")
    return msg


def match_head(mdesc: torch.Tensor, batch: int, n_obj: int, n_hints: int, bin_score: float, sinkhorn_iters: int,
               threshold: float = 0.2):
    """mdesc [B (n_obj + n_hints), D] (final_proj of the set-major token rows) -> dict(P [B, n_obj + 1, n_hints + 1],
    matches0 [B, n_obj] / matches1 [B, n_hints] int64, matching_scores0/1) of t2p_match_head."""
    _need(mdesc, "mdesc", torch.float32, 2)
    dev = mdesc.device
    b, m, n = int(batch), int(n_obj), int(n_hints)
    if mdesc.shape[0] != b * (m + n):
        raise RuntimeError(f"match_head: mdesc is {tuple(mdesc.shape)}, expected [{b * (m + n)}, D]")
    out = dict(P=torch.empty((b, m + 1, n + 1), dtype=torch.float32, device=dev),
               matches0=torch.empty((b, m), dtype=torch.int64, device=dev),
               matches1=torch.empty((b, n), dtype=torch.int64, device=dev),
               matching_scores0=torch.empty((b, m), dtype=torch.float32, device=dev),
               matching_scores1=torch.empty((b, n), dtype=torch.float32, device=dev))
    L.check(L.lib().t2p_match_head(_ptr(mdesc), b, m, n, mdesc.shape[1], float(bin_score), int(sinkhorn_iters), float(threshold),
                                   _ptr(out["P"]), _ptr(out["matches0"]), _ptr(out["matches1"]), _ptr(out["matching_scores0"]),
                                   _ptr(out["matching_scores1"]), _stream(dev)), "t2p_match_head")
    return out


def matching_loss(P: torch.Tensor, idx: torch.Tensor, entry_ptr: torch.Tensor):
    """P [B, n_obj + 1, n_hints + 1] fp32, idx int32 [n_entries, 2], entry_ptr int32 [B + 1] (CSR of the entries over the
    samples) -> (loss [1], sample_loss [B]) of t2p_matching_loss; a bad entry or an empty sample shows as NaN."""
    _need(P, "P", torch.float32, 3)
    dev = P.device
    _need(idx, "idx", torch.int32, 2, dev)
    _need(entry_ptr, "entry_ptr", torch.int32, 1, dev)
    b = P.shape[0]
    if idx.shape[1] != 2 or entry_ptr.numel() != b + 1:
        raise RuntimeError(f"matching_loss: idx {tuple(idx.shape)} must be [n_entries, 2] and entry_ptr [{b + 1}]")
    if b < 1 or P.shape[1] < 2 or P.shape[2] < 2:
        raise RuntimeError(f"matching_loss: P {tuple(P.shape)} must be [B >= 1, n_obj + 1, n_hints + 1]")
    sample_loss = torch.empty((b,), dtype=torch.float32, device=dev)
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    L.check(L.lib().t2p_matching_loss(_ptr(P), b, P.shape[1] - 1, P.shape[2] - 1, _ptr(idx), _ptr(entry_ptr), idx.shape[0],
                                      _ptr(sample_loss), _ptr(loss), _stream(dev)), "t2p_matching_loss")
    return loss, sample_loss


def mse_loss(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """mean((a - b)^2) of two equal-shaped fp32 tensors -> [1] (t2p_mse_loss)."""
    _need(a, "input", torch.float32)
    _need(b, "target", torch.float32, None, a.device)
    if a.shape != b.shape:
        raise RuntimeError(f"mse_loss: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    loss = torch.empty((1,), dtype=torch.float32, device=a.device)
    L.check(L.lib().t2p_mse_loss(_ptr(a), _ptr(b), a.numel(), _ptr(loss), _stream(a.device)), "t2p_mse_loss")
    return loss


def match_attention_backward(qkv: torch.Tensor, d_msg: torch.Tensor, batch: int, n_obj: int, n_hints: int, cross: bool) -> torch.Tensor:
    """Gradient of match_attention: qkv [B (n_obj + n_hints), 3 D] as the forward read it, d_msg [B (n_obj + n_hints), D] ->
    d_qkv [B (n_obj + n_hints), 3 D] (t2p_match_attention_backward; every element written once, no atomics)."""
    _need(qkv, "qkv", torch.float32, 2)
    _need(d_msg, "d_msg", torch.float32, 2, qkv.device)
    rows = int(batch) * (int(n_obj) + int(n_hints))
    if qkv.shape[0] != rows or qkv.shape[1] % 3 or tuple(d_msg.shape) != (rows, qkv.shape[1] // 3):
        raise RuntimeError(f"match_attention_backward: qkv is {tuple(qkv.shape)} and d_msg {tuple(d_msg.shape)}, expected "
                           f"[{rows}, 3 D] and [{rows}, D]")
    d_qkv = torch.empty_like(qkv)
    L.check(L.lib().t2p_match_attention_backward(_ptr(qkv), _ptr(d_msg), int(batch), int(n_obj), int(n_hints), d_msg.shape[1],
                                                 int(bool(cross)), _ptr(d_qkv), _stream(qkv.device)), "t2p_match_attention_backward")
    return d_qkv


def match_head_backward(mdesc: torch.Tensor, d_p: torch.Tensor, batch: int, n_obj: int, n_hints: int, bin_score: float,
                        sinkhorn_iters: int):
    """Gradient of match_head's couplings: mdesc [B (n_obj + n_hints), D] as the forward read it, d_p [B, n_obj + 1, n_hints + 1] ->
    (d_mdesc like mdesc, d_bin [B] float64: the per-sample gradient of bin_score) of t2p_match_head_backward."""
    _need(mdesc, "mdesc", torch.float32, 2)
    dev = mdesc.device
    b, m, n = int(batch), int(n_obj), int(n_hints)
    _need(d_p, "d_p", torch.float32, 3, dev)
    if mdesc.shape[0] != b * (m + n) or tuple(d_p.shape) != (b, m + 1, n + 1):
        raise RuntimeError(f"match_head_backward: mdesc is {tuple(mdesc.shape)} and d_p {tuple(d_p.shape)}, expected "
                           f"[{b * (m + n)}, D] and [{b}, {m + 1}, {n + 1}]")
    d_mdesc = torch.empty_like(mdesc)
    d_bin = torch.empty((b,), dtype=torch.float64, device=dev)
    ws = torch.empty((max(1, L.lib().t2p_match_head_backward_workspace_bytes(b, m, n, int(sinkhorn_iters))),), dtype=torch.uint8,
                     device=dev)
    L.check(L.lib().t2p_match_head_backward(_ptr(mdesc), _ptr(d_p), b, m, n, mdesc.shape[1], float(bin_score), int(sinkhorn_iters),
                                            _ptr(d_mdesc), _ptr(d_bin), _ptr(ws), ws.numel(), _stream(dev)),
            "t2p_match_head_backward")
    return d_mdesc, d_bin


def matching_loss_backward(P: torch.Tensor, idx: torch.Tensor, entry_ptr: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """Gradient of matching_loss with respect to P; g: the upstream gradient, one fp32 value ON THE DEVICE (nothing is read back).
    Returns the whole dP [B, n_obj + 1, n_hints + 1] (t2p_matching_loss_backward)."""
    _need(P, "P", torch.float32, 3)
    dev = P.device
    _need(idx, "idx", torch.int32, 2, dev)
    _need(entry_ptr, "entry_ptr", torch.int32, 1, dev)
    _need(g, "g", torch.float32, 1, dev)
    b = P.shape[0]
    if idx.shape[1] != 2 or entry_ptr.numel() != b + 1 or g.numel() != 1:
        raise RuntimeError(f"matching_loss_backward: idx {tuple(idx.shape)} must be [n_entries, 2], entry_ptr [{b + 1}] and g [1]")
    if b < 1 or P.shape[1] < 2 or P.shape[2] < 2:
        raise RuntimeError(f"matching_loss_backward: P {tuple(P.shape)} must be [B >= 1, n_obj + 1, n_hints + 1]")
    d_p = torch.empty_like(P)
    L.check(L.lib().t2p_matching_loss_backward(_ptr(P), b, P.shape[1] - 1, P.shape[2] - 1, _ptr(idx), _ptr(entry_ptr), idx.shape[0],
                                               _ptr(g), _ptr(d_p), _stream(dev)), "t2p_matching_loss_backward")
    return d_p


def mse_loss_backward(a: torch.Tensor, b: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """Gradient of mse_loss with respect to a: 2 g (a - b) / n; g: one fp32 value on the device (t2p_mse_loss_backward)."""
    _need(a, "input", torch.float32)
    _need(b, "target", torch.float32, None, a.device)
    _need(g, "g", torch.float32, 1, a.device)
    if a.shape != b.shape or g.numel() != 1:
        raise RuntimeError(f"mse_loss_backward: shapes {tuple(a.shape)} and {tuple(b.shape)} differ, or g is not [1]")
    da = torch.empty_like(a)
    L.check(L.lib().t2p_mse_loss_backward(_ptr(a), _ptr(b), a.numel(), _ptr(g), _ptr(da), _stream(a.device)), "t2p_mse_loss_backward")
    return da


def colsum(x: torch.Tensor) -> torch.Tensor:
    """Column sums of x [rows, cols] fp32 -> [cols], accumulated in float64 in a fixed order, rounded once (t2p_colsum)."""
    _need(x, "x", torch.float32, 2)
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise RuntimeError(f"colsum: x {tuple(x.shape)} must have rows and columns")
    out = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
    L.check(L.lib().t2p_colsum(_ptr(x), x.shape[0], x.shape[1], _ptr(out), _stream(x.device)), "t2p_colsum")
    return out


FINE_STATS_MAX_BATCH = L.DEFINES["T2P_FINE_STATS_MAX_BATCH"]


def fine_step_row(step_row: torch.Tensor) -> np.ndarray:
    """The host copy of fine_step_stats' step_row (ONE device-to-host copy of 56 bytes; it waits for the step): float64 [7] = loss,
    loss_offsets, recall, precision, pose_mid, pose_mean, pose_offsets.  A NaN recall - a ratio of counts otherwise - is the
    kernel's mark of an index it refused to read through: IndexError.  (NaN offsets of a diverged model show in pose_offsets alone.)"""
    row = step_row.cpu().numpy()
    if np.isnan(row[2]):
        raise IndexError("fine_step_stats: a pose index outside the tables, or a matches0 / matches1 / gt_hint value outside its range "
                         "(the kernel marks the sample with NaN instead of reading through it)")
    return row


def fine_step_stats(matches0: torch.Tensor, matches1: torch.Tensor, offsets: torch.Tensor, pose_idx: torch.Tensor,
                    gt_hint: torch.Tensor, pose_xy: torch.Tensor, slot_center_xy: torch.Tensor, loss: Optional[torch.Tensor] = None,
                    loss_offsets: Optional[torch.Tensor] = None, check: bool = True):
    """training/fine.py:77-112's statistics of one step on the device (t2p_fine_step_stats): matches0 int64 [B, M], matches1 int64
    [B, N], offsets fp32 [B, N, 2] (the model's outputs), pose_idx int32 [B] rows of the tables gt_hint int32 [n, M], pose_xy float64
    [n, 2], slot_center_xy float64 [n, M, 2]; loss / loss_offsets: fp32 tensors of one element, or None.
    Returns (sample_stats float64 [B, 5], step_row float64 [7]) on the device.  check (default): read step_row back and raise
    IndexError when the kernel marked a sample (fine_step_row); a loop that reads the row anyway passes check=False and calls
    fine_step_row itself."""
    _need(matches0, "matches0", torch.int64, 2)
    dev = matches0.device
    _need(matches1, "matches1", torch.int64, 2, dev)
    _need(offsets, "offsets", torch.float32, 3, dev)
    _need(pose_idx, "pose_idx", torch.int32, 1, dev)
    _need(gt_hint, "gt_hint", torch.int32, 2, dev)
    _need(pose_xy, "pose_xy", torch.float64, 2, dev)
    _need(slot_center_xy, "slot_center_xy", torch.float64, 3, dev)
    b, m = matches0.shape
    n = matches1.shape[1]
    rows = gt_hint.shape[0]
    if matches1.shape[0] != b or tuple(offsets.shape) != (b, n, 2) or pose_idx.shape[0] != b:
        raise RuntimeError(f"fine_step_stats: matches0 {tuple(matches0.shape)}, matches1 {tuple(matches1.shape)}, offsets "
                           f"{tuple(offsets.shape)} and pose_idx {tuple(pose_idx.shape)} do not describe one batch")
    if gt_hint.shape[1] != m or tuple(pose_xy.shape) != (rows, 2) or tuple(slot_center_xy.shape) != (rows, m, 2):
        raise RuntimeError(f"fine_step_stats: tables gt_hint {tuple(gt_hint.shape)}, pose_xy {tuple(pose_xy.shape)}, slot_center_xy "
                           f"{tuple(slot_center_xy.shape)} must be [n, {m}], [n, 2], [n, {m}, 2]")
    scalars = []
    for t, name in ((loss, "loss"), (loss_offsets, "loss_offsets")):
        if t is not None:
            t = _need(t.detach().reshape(-1), name, torch.float32, 1, dev)
            if t.numel() != 1:
                raise RuntimeError(f"fine_step_stats: {name} must hold one value")
        scalars.append(t)
    sample_stats = torch.empty((b, 5), dtype=torch.float64, device=dev)
    step_row = torch.empty((7,), dtype=torch.float64, device=dev)
    L.check(L.lib().t2p_fine_step_stats(_ptr(matches0), _ptr(matches1), _ptr(offsets), _ptr(pose_idx), b, m, n, _ptr(gt_hint),
                                        _ptr(pose_xy), _ptr(slot_center_xy), rows, _ptr(scalars[0]), _ptr(scalars[1]),
                                        _ptr(sample_stats), _ptr(step_row), _stream(dev)), "t2p_fine_step_stats")
    if check:
        fine_step_row(step_row)
    return sample_stats, step_row


LOCALIZE_MAX_TOP_K = L.DEFINES["T2P_LOCALIZE_MAX_TOP_K"]


def match_indexed(obj_table: torch.Tensor, hint_table: torch.Tensor, obj_row: torch.Tensor, hint_row: torch.Tensor,
                  weights: L.MatchWeights, sinkhorn_iters: int, threshold: float = 0.2):
    """match() with its inputs addressed through tables (t2p_match_indexed): obj_table fp32 [n_cells, M, D], hint_table fp32
    [n_queries, N, D], obj_row / hint_row int32 [B] on the GPU - sample b matches cell obj_row[b] against query hint_row[b].
    Returns match()'s dict, bit for bit what match() gives on the index_select'ed tables.  A row outside its table is not read
    through: that sample's P is NaN and its matches are -1 (localize_poses marks a sample whose cell row is outside the database),
    its neighbours are unaffected."""
    _need(obj_table, "obj_table", torch.float32, 3)
    dev = obj_table.device
    _need(hint_table, "hint_table", torch.float32, 3, dev)
    _need(obj_row, "obj_row", torch.int32, 1, dev)
    _need(hint_row, "hint_row", torch.int32, 1, dev)
    n_cells, m, d = obj_table.shape
    n_queries, n = hint_table.shape[0], hint_table.shape[1]
    b = obj_row.shape[0]
    if hint_table.shape[2] != d or hint_row.shape[0] != b:
        raise RuntimeError(f"match_indexed: obj_table {tuple(obj_table.shape)} / hint_table {tuple(hint_table.shape)} / obj_row "
                           f"{tuple(obj_row.shape)} / hint_row {tuple(hint_row.shape)} disagree")
    out = dict(P=torch.empty((b, m + 1, n + 1), dtype=torch.float32, device=dev),
               matches0=torch.empty((b, m), dtype=torch.int64, device=dev),
               matches1=torch.empty((b, n), dtype=torch.int64, device=dev),
               matching_scores0=torch.empty((b, m), dtype=torch.float32, device=dev),
               matching_scores1=torch.empty((b, n), dtype=torch.float32, device=dev),
               offsets=torch.empty((b, n, 2), dtype=torch.float32, device=dev))
    if b == 0:      # (empty tensors have no address to hand over; the entry point launches nothing for batch 0 either)
        return out
    ws = workspace(dev, L.lib().t2p_match_indexed_workspace_bytes(b, m, n, d), "match_indexed")
    rc = L.lib().t2p_match_indexed(_ptr(obj_table), n_cells, _ptr(hint_table), n_queries, _ptr(obj_row), _ptr(hint_row), b, m, n, d,
                                   C.byref(weights), int(sinkhorn_iters), float(threshold), _ptr(out["P"]), _ptr(out["matches0"]),
                                   _ptr(out["matches1"]), _ptr(out["matching_scores0"]), _ptr(out["matching_scores1"]),
                                   _ptr(out["offsets"]), _ptr(ws), ws.numel(), _stream(dev))
    L.check(rc, "t2p_match_indexed")
    return out


def localize_check(matched: np.ndarray, what: str = "localize_poses", query_offset: int = 0):
    """IndexError naming the first (query, candidate) the kernel marked with matched = -1 (host array [Q, K])."""
    bad = np.argwhere(np.asarray(matched) < 0)
    if len(bad):
        q, c = int(bad[0][0]), int(bad[0][1])
        raise IndexError(f"{what}: query {q + query_offset}, candidate {c}: a cell row outside the database, a matches0 value outside "
                         f"its range or a NaN offset ({len(bad)} such samples; the kernel marks them instead of reading through them)")


def localize_poses(matches0: torch.Tensor, offsets: torch.Tensor, cell_row: torch.Tensor, n_queries: int, top_k: int,
                   center_xy: torch.Tensor, bbox_xy: torch.Tensor, cell_size: torch.Tensor, check: bool = True):
    """get_pos_in_cell (models/superglue_matcher.py:139-161), the world step of evaluation._sample_hits and run_fine's argmax over
    the candidates' matched counts for n_queries x top_k samples (query-major) in one launch (t2p_localize_poses).  matches0 int64
    [Q K, M], offsets fp32 [Q K, N, 2], cell_row int32 [Q K]; float64 tables center_xy [n_cells, M, 2], bbox_xy [n_cells, 2],
    cell_size [n_cells].  Returns a dict of device tensors: pos_mean, pos_offset, world_mean, world_offset float64 [Q, K, 2],
    matched int32 [Q, K], best int32 [Q].  check (default): read `matched` back and raise IndexError when the kernel marked a
    sample (localize_check); a caller that copies the results anyway passes check=False and calls localize_check itself."""
    _need(matches0, "matches0", torch.int64, 2)
    dev = matches0.device
    _need(offsets, "offsets", torch.float32, 3, dev)
    _need(cell_row, "cell_row", torch.int32, 1, dev)
    _need(center_xy, "center_xy", torch.float64, 3, dev)
    _need(bbox_xy, "bbox_xy", torch.float64, 2, dev)
    _need(cell_size, "cell_size", torch.float64, 1, dev)
    q, k = int(n_queries), int(top_k)
    b, m = matches0.shape
    n = offsets.shape[1]
    rows = center_xy.shape[0]
    if q < 0 or k < 1 or b != q * k or tuple(offsets.shape) != (b, n, 2) or cell_row.shape[0] != b:
        raise RuntimeError(f"localize_poses: matches0 {tuple(matches0.shape)}, offsets {tuple(offsets.shape)} and cell_row "
                           f"{tuple(cell_row.shape)} do not describe {q} queries x {k} candidates")
    if tuple(center_xy.shape) != (rows, m, 2) or tuple(bbox_xy.shape) != (rows, 2) or tuple(cell_size.shape) != (rows,):
        raise RuntimeError(f"localize_poses: tables center_xy {tuple(center_xy.shape)}, bbox_xy {tuple(bbox_xy.shape)}, cell_size "
                           f"{tuple(cell_size.shape)} must be [n, {m}, 2], [n, 2], [n]")
    f64 = lambda: torch.empty((q, k, 2), dtype=torch.float64, device=dev)
    out = dict(pos_mean=f64(), pos_offset=f64(), world_mean=f64(), world_offset=f64(),
               matched=torch.empty((q, k), dtype=torch.int32, device=dev), best=torch.empty((q,), dtype=torch.int32, device=dev))
    if q == 0:
        return out
    L.check(L.lib().t2p_localize_poses(_ptr(matches0), _ptr(offsets), _ptr(cell_row), q, k, m, n, _ptr(center_xy), _ptr(bbox_xy),
                                       _ptr(cell_size), rows, _ptr(out["pos_mean"]), _ptr(out["pos_offset"]), _ptr(out["world_mean"]),
                                       _ptr(out["world_offset"]), _ptr(out["matched"]), _ptr(out["best"]), _stream(dev)),
            "t2p_localize_poses")
    if check:
        localize_check(out["matched"].cpu().numpy())
    return out


def distinct_check(n_valid: np.ndarray, what: str = "topk_distinct", query_offset: int = 0):
    """IndexError naming the first query the selection kernel marked with n_valid = -1 (host array [Q])."""
    bad = np.flatnonzero(np.asarray(n_valid) < 0)
    if len(bad):
        raise IndexError(f"{what}: query {int(bad[0]) + query_offset}: a pool index outside the cell table ({len(bad)} such queries; the "
                         "kernel marks them instead of reading through the index)")


def topk_distinct(pool_idx: torch.Tensor, pool_score: torch.Tensor, cell_xy: torch.Tensor, sep: float, k: int, cell_group=None,
                  index_offset: int = 0, check: bool = True):
    """Greedy non-overlap selection over a ranked pool (t2p_topk_distinct, include/t2p_select.h).  pool_idx int64 / pool_score
    float64 [nq, pool]: a query's cells as sim_topk* return them (score descending, ties to the lower index, -inf last, indices
    index_offset + row); cell_xy float64 [n_cells, 2]: the cells' centres; cell_group int32 [n_cells] or None.  Walks each pool from
    the front to its first -inf entry and accepts a cell iff no accepted one lies within sep of it in x AND in y (strictly, float64)
    in the same group, up to k.  sep = 0: the first k entries; inf: one cell per group; negative or NaN: refused.
    Returns (idx int64 [nq, k], scores float64 [nq, k], n_valid int32 [nq], exhausted int32 [nq]) on the GPU: the accepted entries
    first, then the first pool entry's index at -inf; exhausted = 1 where fewer than k were found only because the pool ran out
    (no -inf entry in it and pool < n_cells) - where it is 0 the result is that of the full ranking.
    check (default): read n_valid back and raise IndexError naming the first query with a pool index outside the table
    (distinct_check); a caller that copies the results anyway passes check=False and calls distinct_check itself."""
    _need(pool_idx, "pool_idx", torch.int64, 2)
    dev = pool_idx.device
    _need(pool_score, "pool_score", torch.float64, 2, dev)
    _need(cell_xy, "cell_xy", torch.float64, 2, dev)
    if cell_group is not None:
        _need(cell_group, "cell_group", torch.int32, 1, dev)
    nq, pool = pool_idx.shape
    n_cells = cell_xy.shape[0]
    if tuple(pool_score.shape) != (nq, pool) or cell_xy.shape[1] != 2 or (cell_group is not None and cell_group.shape[0] != n_cells):
        raise RuntimeError(f"topk_distinct: pool_idx {tuple(pool_idx.shape)}, pool_score {tuple(pool_score.shape)}, cell_xy "
                           f"{tuple(cell_xy.shape)}, cell_group {None if cell_group is None else tuple(cell_group.shape)}: expected "
                           f"[nq, pool] twice, [n_cells, 2] and [n_cells]")
    k = int(k)
    idx = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=dev)
    score = torch.empty((nq, max(k, 0)), dtype=torch.float64, device=dev)
    n_valid = torch.empty((nq,), dtype=torch.int32, device=dev)
    exhausted = torch.empty((nq,), dtype=torch.int32, device=dev)
    if nq == 0 and 1 <= k <= pool:       # (empty tensors have no address to hand over; the entry point launches nothing for nq 0 either)
        return idx, score, n_valid, exhausted
    L.check(L.lib().t2p_topk_distinct(_ptr(pool_idx), _ptr(pool_score), nq, pool, n_cells, int(index_offset), _ptr(cell_xy),
                                      _ptr(cell_group), float(sep), k, _ptr(idx), _ptr(score), _ptr(n_valid), _ptr(exhausted),
                                      _stream(dev)), "t2p_topk_distinct")
    if check:
        distinct_check(n_valid.cpu().numpy())
    return idx, score, n_valid, exhausted


# ---------------------------------------------------------------------------------------------------------------
def profile_enable(on: bool):
    """Bracket every kernel launch with hipEvents on its launch stream (bench.py's live per-kernel timing)."""
    L.lib().t2p_profile_enable(int(bool(on)))


def profile_repeat(scope: Optional[str], reps: int = 1):
    """Measurement hook (t2p_profile_repeat): launches reported under `scope` are issued `reps` times back to back (same
    arguments, same results) - profiles/energy_table.py holds one kernel on the chip for seconds that way.  None / 1: off."""
    L.lib().t2p_profile_repeat(scope.encode() if scope else None, int(reps))


def profile_report() -> Dict[str, tuple]:
    """{kernel name: (launches, total_ms)} of the launches recorded since the last report; waits for them."""
    buf = C.create_string_buffer(1 << 16)
    L.check(L.lib().t2p_profile_report(buf, len(buf)), "t2p_profile_report")
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split()
        out[name] = (int(cnt), float(ms))
    return out
