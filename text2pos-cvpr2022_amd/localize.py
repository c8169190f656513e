"""Text queries against a saved cell database: the serving path of Text2Pos on the MI355X.

    python -m text2pos_amd.localize build --base_path ./data/k360_30-10_scG_pd10_pc4_spY_all/ --scenes 2013_05_28_drive_0010_sync \\
        --path_coarse ./checkpoints/coarse.pth --path_fine ./checkpoints/fine.pth --out db.pt
    python -m text2pos_amd.localize query --db db.pt --path_coarse ./checkpoints/coarse.pth --path_fine ./checkpoints/fine.pth \\
        --hints "The pose is north of a gray road." "The pose is east of a green tree."
    python -m text2pos_amd.localize query ... --hints "..." --prior 1042.5 3310.0 --radius 60 --scene 2013_05_28_drive_0010_sync
    python -m text2pos_amd.localize query ... --hints "..." --distinct 30

The reference has no such path: the only code that chains text encoding, top-k, the fine matcher and the pose estimate is its
evaluation (evaluation/pipeline.py:60-137, :172-279), which needs ground-truth poses and the raw scene, and re-encodes every
candidate cell's objects per (query, candidate) sample (dataloading/kitti360pose/eval.py:117-189).  A deployed localiser's cells
are fixed, so here they are encoded ONCE:

  CellDatabase   the coarse embedding of every cell (CellRetrievalNetwork.encode_scene_cells), the fine model's object tokens of
                 every cell's padded object list (SuperGlueMatch.encode_cell_objects), and the float64 geometry the pose estimate
                 needs (object centres, cell corner, cell size); saved and reloaded without the scene.
  Localizer      hints -> encode_text -> retrieve_topk on the resident embeddings -> encode_hints once per query ->
                 t2p_match_indexed (the matcher on the database's tokens, addressed by row) -> t2p_localize_poses (get_pos_in_cell,
                 models/superglue_matcher.py:139-161, the world coordinates and the most confident candidate, on the device).
                 No raw points, no PointNet++, one device-to-host copy per call.
                 With a prior (a position and a radius in world metres, a scene name, or both) the ranking itself is restricted
                 (t2p_sim_topk_prior, include/t2p_serve.h): a cell qualifies when the prior point lies within the radius of the
                 cell's square and the cell belongs to the named scene.  Applied after an unrestricted top-k the prior would
                 return nothing whenever the k best cells of the whole database lie elsewhere.
                 With distinct_radius the top_k candidates are k different places: overlapping cells (30 m on a 10 m stride) have
                 near-duplicate embeddings, so the ranking returns a pool of cells and t2p_topk_distinct (include/t2p_select.h)
                 keeps the best top_k no two of which lie within the radius of each other in x and in y, scene by scene.

The deliberate difference from the evaluation: a database cell has ONE T.FixedPoints draw, `transform.keys(row, slot)` of its
database row, where run_fine draws once per (query, candidate) sample as the reference's dataloader does.
"""
import argparse
import hashlib
import json
import sys
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .retrieval import MAX_TOP_K, check_distinct, check_top_k, default_distinct_pool, retrieve_topk
from .superglue_matcher import MATCH_THRESHOLD

FORMAT = 1
MAX_HINTS = 63           # t2p_match's token limit
_TENSORS = ("coarse", "fine", "center_xy", "bbox_xy", "cell_size")
_RESULT_FIELDS = ("cell_rows", "cell_ids", "scores", "pos_in_cell_mean", "pos_in_cell", "world_xy_mean", "world_xy", "matched", "best",
                  "best_world_xy")


def state_hash(model) -> str:
    """sha256 over a model's state_dict: every key in sorted order with its dtype, shape and bytes."""
    h = hashlib.sha256()
    sd = model.state_dict()
    for k in sorted(sd):
        t = sd[k].detach().cpu().contiguous()
        h.update(k.encode())
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return h.hexdigest()


def model_meta(model_coarse, model_fine) -> Dict[str, object]:
    """The part of CellDatabase.meta the two models determine."""
    return dict(hash_coarse=state_hash(model_coarse), hash_fine=state_hash(model_fine),
                dim_coarse=int(model_coarse.embed_dim), dim_fine=int(model_fine.embed_dim),
                precision_coarse=str(model_coarse.precision), precision_fine=str(model_fine.precision))


def check_models(meta: Dict[str, object], model_coarse, model_fine, what: str):
    """ValueError naming the first field of `meta` the models do not match."""
    own = model_meta(model_coarse, model_fine)
    for k in ("dim_coarse", "dim_fine", "precision_coarse", "precision_fine", "hash_coarse", "hash_fine"):
        if meta.get(k) != own[k]:
            raise ValueError(f"{what}: the database was built with {k}={meta.get(k)!r}, the model has {k}={own[k]!r}")


def _check_transform(transform):
    if not all(hasattr(transform, a) for a in ("keys", "n_pts", "seed")) or getattr(transform, "rotate_degrees", None) is not None:
        raise TypeError("CellDatabase needs a pipeline.PerCellTransform without rotation: a cell's draw must depend on "
                        "(seed, database row, slot) only")


class CellDatabase:
    """coarse fp32 [Nc, D_coarse], fine fp32 [Nc, pad_size, D_fine], center_xy float64 [Nc, pad_size, 2] (the object centres of
    every cell's padded slots), bbox_xy float64 [Nc, 2], cell_size float64 [Nc], cell_ids / scene_names (lists of str), meta (plain
    values: format, seed, n_pts, pad_size, the models' dimensions, precisions and state hashes).  A plain container: it holds CPU
    or GPU tensors alike; only Localizer.localize needs them on the GPU."""

    def __init__(self, coarse, fine, center_xy, bbox_xy, cell_size, cell_ids: Sequence[str], scene_names: Sequence[str], meta: dict):
        self.coarse, self.fine, self.center_xy, self.bbox_xy, self.cell_size = coarse, fine, center_xy, bbox_xy, cell_size
        self.cell_ids, self.scene_names, self.meta = [str(c) for c in cell_ids], [str(s) for s in scene_names], dict(meta)
        n, pad = len(self.cell_ids), int(self.meta["pad_size"])
        want = dict(coarse=((n, int(self.meta["dim_coarse"])), torch.float32), fine=((n, pad, int(self.meta["dim_fine"])), torch.float32),
                    center_xy=((n, pad, 2), torch.float64), bbox_xy=((n, 2), torch.float64), cell_size=((n,), torch.float64))
        for k, (shape, dtype) in want.items():
            t = getattr(self, k)
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype:
                got = (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"CellDatabase: {k} must be {dtype} {shape} (pad_size, dim_coarse and dim_fine from meta), got {got}")
        if len(self.scene_names) != n:
            raise ValueError(f"CellDatabase: scene_names has {len(self.scene_names)} entries for {n} cells")
        if len(set(self.cell_ids)) != n:
            raise ValueError("CellDatabase: cell_ids repeat")

    def __len__(self) -> int:
        return len(self.cell_ids)

    @property
    def device(self):
        return self.coarse.device

    # ---- the tables a prior is checked against ----------------------------------------------------------------------------------
    def cell_boxes(self) -> torch.Tensor:
        """float64 [Nc, 4] on the database's device: x0, y0, x0 + cell_size, y0 + cell_size (one rounding each), the closed square
        a prior position is measured against."""
        return torch.cat([self.bbox_xy, self.bbox_xy + self.cell_size[:, None]], dim=1).contiguous()

    def cell_centers(self) -> torch.Tensor:
        """float64 [Nc, 2] on the database's device: x0 + cell_size / 2, y0 + cell_size / 2 (one rounding each), the position two
        candidates are told apart by (distinct_radius)."""
        return (self.bbox_xy + 0.5 * self.cell_size[:, None]).contiguous()

    def scene_index(self):
        """(sorted unique scene names, int32 [Nc] on the database's device: every cell's index into them)."""
        names = sorted(set(self.scene_names))
        at = {n: i for i, n in enumerate(names)}
        idx = torch.tensor([at[n] for n in self.scene_names], dtype=torch.int32)
        return names, idx.to(self.device)

    # ---- building -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _encode(model_coarse, model_fine, cells, transform, pad_size: int, cells_per_call: int, cell_offset: int):
        from .scene import DeviceScene
        scene = DeviceScene(cells, model_coarse.device, n_pad=pad_size, pad_seed=transform.seed)
        n = scene.n_cells
        with torch.no_grad():
            coarse = model_coarse.encode_scene_cells(scene, transform, 0, n, cell_offset=cell_offset, cells_per_call=cells_per_call)
            fine = [model_fine.encode_cell_objects(scene, transform, a, min(a + cells_per_call, n), pad_size, cell_offset=cell_offset)
                    for a in range(0, n, cells_per_call)]
        fine = fine[0] if len(fine) == 1 else torch.cat(fine)
        dev = model_coarse.device
        ids = scene.padded_object_ids(pad_size)
        center = torch.from_numpy(np.ascontiguousarray(scene.center64[ids][:, :, 0:2], dtype=np.float64)).to(dev)
        bbox = torch.from_numpy(np.array([np.asarray(c.bbox_w, dtype=np.float64)[0:2] for c in cells], dtype=np.float64).reshape(n, 2)).to(dev)
        size = torch.from_numpy(np.array([float(c.cell_size) for c in cells], dtype=np.float64)).to(dev)
        return coarse.contiguous(), fine.contiguous(), center, bbox, size

    @classmethod
    def build(cls, model_coarse, model_fine, cells, transform, pad_size: int = 16, cells_per_call: int = 2048) -> "CellDatabase":
        """Uploads `cells` once (scene.DeviceScene with the fine stage's padding objects, seeded with the transform's seed) and
        encodes them with both models in eval() mode; row i draws `transform.keys(i, slot)`.  cells_per_call: the memory knob (a
        call packs cells_per_call x pad_size objects for the fine model); the result does not depend on it."""
        _check_transform(transform)
        pad_size, cells_per_call = int(pad_size), max(1, int(cells_per_call))
        if not 1 <= pad_size <= MAX_HINTS:
            raise ValueError(f"CellDatabase.build: pad_size={pad_size} outside [1, {MAX_HINTS}], the matcher's token limit")
        if model_fine.embed_dim not in (64, 128, 256):
            raise ValueError(f"CellDatabase.build: dim_fine={model_fine.embed_dim} is not built (the matcher takes 64, 128, 256)")
        cells = list(cells)
        if not cells:
            raise ValueError("CellDatabase.build: no cells")
        meta = dict(format=FORMAT, seed=int(transform.seed), n_pts=int(transform.n_pts), pad_size=pad_size,
                    **model_meta(model_coarse, model_fine))
        tensors = cls._encode(model_coarse, model_fine, cells, transform, pad_size, cells_per_call, 0)
        return cls(*tensors, [c.id for c in cells], [getattr(c, "scene_name", "") for c in cells], meta)

    def extend(self, model_coarse, model_fine, new_cells, cells_per_call: int = 2048) -> "CellDatabase":
        """Appends cells (in place; returns self).  A new cell's draw index is its database row, so the result equals a fresh
        build over all cells.  The models must be the ones the database was built with; duplicate ids are refused."""
        from .pipeline import PerCellTransform
        check_models(self.meta, model_coarse, model_fine, "CellDatabase.extend")
        new_cells = list(new_cells)
        ids = [str(c.id) for c in new_cells]
        dup = sorted(set(ids) & set(self.cell_ids)) or sorted(i for i in set(ids) if ids.count(i) > 1)
        if dup:
            raise ValueError(f"CellDatabase.extend: cell_ids repeat (first: {dup[0]!r})")
        if not new_cells:
            return self
        tf = PerCellTransform(int(self.meta["n_pts"]), int(self.meta["seed"]))
        new = self._encode(model_coarse, model_fine, new_cells, tf, int(self.meta["pad_size"]), max(1, int(cells_per_call)), len(self))
        for k, t in zip(_TENSORS, new):
            setattr(self, k, torch.cat([getattr(self, k), t.to(self.device)]).contiguous())
        self.cell_ids += ids
        self.scene_names += [str(getattr(c, "scene_name", "")) for c in new_cells]
        return self

    # ---- storage ------------------------------------------------------------------------------------------------------------
    def to(self, device) -> "CellDatabase":
        return CellDatabase(*(getattr(self, k).to(device) for k in _TENSORS), self.cell_ids, self.scene_names, self.meta)

    def save(self, path: str):
        """One torch.save of tensors (moved to the host) and plain Python values: no pickled classes."""
        torch.save(dict({k: getattr(self, k).detach().cpu().contiguous() for k in _TENSORS}, cell_ids=list(self.cell_ids),
                        scene_names=list(self.scene_names), meta=dict(self.meta)), path)

    @classmethod
    def load(cls, path: str, device="cpu") -> "CellDatabase":
        d = torch.load(path, map_location="cpu", weights_only=True)
        missing = [k for k in _TENSORS + ("cell_ids", "scene_names", "meta") if k not in d]
        if missing:
            raise ValueError(f"CellDatabase.load: {path} lacks {missing}")
        if d["meta"].get("format") != FORMAT:
            raise ValueError(f"CellDatabase.load: format={d['meta'].get('format')!r}, this package reads format={FORMAT}")
        return cls(*(d[k].to(device) for k in _TENSORS), d["cell_ids"], d["scene_names"], d["meta"])


class Localization(SimpleNamespace):
    """What Localizer.localize returns, host NumPy, Q queries x K candidates (best first): cell_rows int64 [Q, K], cell_ids
    (Q lists of K ids), scores float64 [Q, K], pos_in_cell_mean / pos_in_cell float64 [Q, K, 2] (cell units: the mean of the matched
    objects' centres / of centre + offset; (0.5, 0.5) without matches), world_xy_mean / world_xy [Q, K, 2] (bbox + pos * cell_size),
    matched int32 [Q, K] (matched objects per candidate), best int32 [Q] (the candidate with the most, first on ties) and
    best_world_xy float64 [Q, 2] = world_xy[q, best[q]]; n_valid int32 [Q] and restricted (bool).
    A call with a prior (restricted) may find fewer than K cells that qualify: n_valid[q] candidates are valid, always the first
    ones; the columns behind them read cell_rows -1, cell_ids None, scores -inf, NaN positions and matched 0; best is taken over
    the valid columns only and is -1, with a NaN best_world_xy, where n_valid is 0.  Without a prior n_valid is K.
    A call with distinct_radius (distinct, restricted both set) has the same states for the candidates the selection did not find,
    and exhausted bool [Q]: True where fewer than K were found only because the pool of ranked cells ran out (ask again with a
    larger distinct_pool); where it is False the candidates are those of the whole database.  Otherwise exhausted is all False."""

    def to_json(self, q: int) -> dict:
        """One query as plain values.  Unrestricted: the fields of _RESULT_FIELDS.  Restricted: n_valid besides, every per-candidate
        list cut to its valid prefix, best and best_world_xy null when nothing qualified - no NaN or Infinity in the line."""
        out = {k: (getattr(self, k)[q].tolist() if isinstance(getattr(self, k), np.ndarray) else list(getattr(self, k)[q]))
               for k in _RESULT_FIELDS}
        if not getattr(self, "restricted", False):
            return out
        n = int(self.n_valid[q])
        for k in _RESULT_FIELDS[:-2]:
            out[k] = out[k][:n]
        if n == 0:
            out["best"] = out["best_world_xy"] = None
        out["n_valid"] = n
        if getattr(self, "distinct", False):
            out["exhausted"] = bool(self.exhausted[q])
        return out


def check_hints(hints) -> List[List[str]]:
    """The query list of Localizer.localize, checked before anything is launched."""
    if isinstance(hints, str) or not isinstance(hints, (list, tuple)):
        raise TypeError("localize: hints must be a list of queries, each a list of hint sentences")
    out = []
    for q, h in enumerate(hints):
        if isinstance(h, str) or not isinstance(h, (list, tuple)) or not all(isinstance(s, str) for s in h):
            raise TypeError(f"localize: query {q} must be a list of hint sentences (str)")
        if not 1 <= len(h) <= MAX_HINTS:
            raise ValueError(f"localize: query {q} has {len(h)} hints; a query needs 1 to {MAX_HINTS} (the matcher's token limit)")
        out.append(list(h))
    return out


def check_prior(n_queries: int, prior_xy, prior_radius, scenes, known_scenes: Sequence[str]):
    """The prior of Localizer.localize, checked on the host before anything is launched -> (xy float64 [Q, 2], radius float64 [Q],
    group int32 [Q]) with each half None where it was not given; (None, None, None) without a prior.
    prior_xy: one (x, y) or [Q, 2], finite; prior_radius: one number or [Q], >= 0, inf = no geometric restriction; the two go
    together.  scenes: None, one name, or Q entries each a name or None (None = any scene, group -1); names index known_scenes."""
    nq = int(n_queries)
    if (prior_xy is None) != (prior_radius is None):
        raise ValueError("localize: prior_xy and prior_radius go together (got only "
                         f"{'prior_xy' if prior_radius is None else 'prior_radius'})")
    xy = rad = grp = None
    if prior_xy is not None:
        try:
            xy, rad = np.asarray(prior_xy, dtype=np.float64), np.asarray(prior_radius, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"localize: prior_xy and prior_radius must be numbers ({e})") from None
        if xy.shape == (2,):
            xy = np.broadcast_to(xy, (nq, 2))
        if rad.shape == ():
            rad = np.broadcast_to(rad, (nq,))
        if xy.shape != (nq, 2) or rad.shape != (nq,):
            raise ValueError(f"localize: prior_xy has shape {tuple(np.shape(prior_xy))} and prior_radius {tuple(np.shape(prior_radius))} for "
                             f"{nq} queries: give one (x, y) or [{nq}, 2], and one radius or [{nq}]")
        xy, rad = np.ascontiguousarray(xy), np.ascontiguousarray(rad)
        bad = np.flatnonzero(~np.isfinite(xy).all(axis=1))
        if len(bad):
            raise ValueError(f"localize: prior_xy of query {bad[0]} is {xy[bad[0]].tolist()}: a prior position must be finite")
        bad = np.flatnonzero(~(rad >= 0))
        if len(bad):
            raise ValueError(f"localize: prior_radius of query {bad[0]} is {float(rad[bad[0]])}: a radius is >= 0 (inf = no restriction)")
    if scenes is not None:
        names = [scenes] * nq if isinstance(scenes, str) else list(scenes) if isinstance(scenes, (list, tuple)) else None
        if names is None or len(names) != nq or not all(n is None or isinstance(n, str) for n in names):
            raise ValueError(f"localize: scenes must be one name or {nq} entries, each a name or None (any scene)")
        at = {n: i for i, n in enumerate(known_scenes)}
        for n in names:
            if n is not None and n not in at:
                raise ValueError(f"localize: unknown scene {n!r}; the database holds {list(known_scenes)}")
        grp = np.array([-1 if n is None else at[n] for n in names], dtype=np.int32).reshape(nq)
    return xy, rad, grp


def check_distinct_args(distinct_radius, distinct_pool, top_k: int, n_cells: int):
    """The distinct-candidates arguments of Localizer.localize, checked on the host before anything is encoded -> None without a
    radius, else (radius float, pool int).  radius: one number >= 0, inf allowed; pool: None (retrieval.default_distinct_pool) or a
    whole number in [top_k, min(n_cells, MAX_TOP_K)]; a pool without a radius is refused."""
    if distinct_radius is None:
        if distinct_pool is not None:
            raise ValueError("localize: distinct_pool needs distinct_radius")
        return None
    if isinstance(distinct_radius, bool) or np.ndim(distinct_radius) != 0:
        raise ValueError(f"localize: distinct_radius must be one number >= 0 (got {distinct_radius!r})")
    radius = check_distinct(distinct_radius, "localize: distinct_radius")
    hi = min(int(n_cells), MAX_TOP_K)
    if distinct_pool is None:
        return radius, default_distinct_pool(n_cells, top_k)
    if isinstance(distinct_pool, bool) or np.ndim(distinct_pool) != 0 or int(distinct_pool) != distinct_pool or \
            not top_k <= int(distinct_pool) <= hi:
        raise ValueError(f"localize: distinct_pool={distinct_pool!r} outside [top_k, min(len(db), {MAX_TOP_K})] = [{top_k}, {hi}]")
    return radius, int(distinct_pool)


def unpack_result(res: np.ndarray, k: int, cell_ids: Sequence[str], restricted: bool, what: str = "Localizer.localize",
                  distinct: bool = False) -> Localization:
    """The packed float64 [Q, 11 K + 1] rows of Localizer._run_chunk (in the caller's order, on the host) -> Localization.
    distinct: the rows come from a call with distinct_radius and carry two more columns, the selection's n_valid (-1: a pool index
    outside the database, IndexError naming the query) and its exhausted flag; the columns it did not fill are at -inf, so the
    rest is the restricted handling.
    restricted: candidate j of a query is valid iff its score is above -inf (the masked pairs of t2p_sim_topk_prior are exactly
    -inf and come last); the invalid columns, whose rows are real cells the matcher ran on, are overwritten as Localization
    states, and best is recomputed over the valid columns (most matched objects, the first on ties, -1 without any)."""
    nq = res.shape[0]
    cut = lambda i, n=1: res[:, i * k: (i + n) * k]
    exhausted = np.zeros(nq, dtype=bool)
    if distinct:
        ops.distinct_check(res[:, 11 * k + 1], what)
        exhausted, restricted = res[:, 11 * k + 2] != 0, True
    matched = cut(10).astype(np.int32)
    ops.localize_check(matched, what)
    rows = cut(0).astype(np.int64)
    best = res[:, 11 * k].astype(np.int32)
    scores = cut(1).copy()
    pos = [cut(i, 2).reshape(nq, k, 2).copy() for i in (2, 4, 6, 8)]
    n_valid = np.full(nq, k, dtype=np.int32)
    if restricted:
        valid = scores > -np.inf
        n_valid = valid.sum(axis=1).astype(np.int32)
        rows[~valid] = -1
        scores[~valid] = -np.inf
        matched[~valid] = 0
        for p in pos:
            p[~valid] = np.nan
        ids = [[cell_ids[j] if j >= 0 else None for j in r] for r in rows.tolist()]
        best = np.where(n_valid > 0, np.argmax(np.where(valid, matched, -1), axis=1), -1).astype(np.int32) if nq else best
    else:
        ids = [[cell_ids[j] for j in r] for r in rows]
    world = pos[3]
    best_xy = world[np.arange(nq), best] if nq else np.zeros((0, 2))
    if restricted and nq:
        best_xy[best < 0] = np.nan           # (a copy: fancy indexing)
    return Localization(cell_rows=rows, cell_ids=ids, scores=scores, pos_in_cell_mean=pos[0], pos_in_cell=pos[1], world_xy_mean=pos[2],
                        world_xy=world, matched=matched, best=best, best_world_xy=best_xy, n_valid=n_valid, restricted=bool(restricted),
                        exhausted=exhausted, distinct=bool(distinct))


def group_by_hint_count(hints: List[List[str]]) -> Dict[int, List[int]]:
    """{number of hints: the queries that have it, in the caller's order}, keys ascending."""
    groups: Dict[int, List[int]] = {}
    for q, h in enumerate(hints):
        groups.setdefault(len(h), []).append(q)
    return dict(sorted(groups.items()))


class Localizer:
    def __init__(self, model_coarse, model_fine, database: CellDatabase):
        for name, m in (("model_coarse", model_coarse), ("model_fine", model_fine)):
            if m.training:
                raise NotImplementedError(f"Localizer: {name} is in train() mode; the serving path runs the folded eval() kernels: "
                                          "call .eval()")
        check_models(database.meta, model_coarse, model_fine, "Localizer")
        self.model_coarse, self.model_fine, self.database = model_coarse, model_fine, database
        self._tables = None      # (len(database), cell boxes, scene names, scene index): what a prior is checked against
        self._centers = None     # (len(database), cell centres): what distinct candidates are told apart by

    def prior_tables(self):
        """(cell_boxes, scene names, scene index) of the database, computed once and again after the database grew (extend)."""
        if self._tables is None or self._tables[0] != len(self.database):
            self._tables = (len(self.database), self.database.cell_boxes(), *self.database.scene_index())
        return self._tables[1:]

    def distinct_tables(self):
        """(cell centres float64 [Nc, 2], scene index int32 [Nc]) of the database, computed once and again after it grew."""
        if self._centers is None or self._centers[0] != len(self.database):
            self._centers = (len(self.database), self.database.cell_centers())
        return self._centers[1], self.prior_tables()[2]

    def _require_device(self):
        db = self.database
        for name, dev in (("database", db.device), ("model_coarse", self.model_coarse.device), ("model_fine", self.model_fine.device)):
            if torch.device(dev).type != "cuda":
                raise RuntimeError(f"Localizer.localize: {name} must live on the GPU (got device {dev}); there is no CPU path")
        if not (torch.device(db.device) == torch.device(self.model_coarse.device) == torch.device(self.model_fine.device)):
            raise RuntimeError("Localizer.localize: database and models are on different devices")

    def _run_chunk(self, hints: List[List[str]], top_k: int, prior=None, distinct=None) -> torch.Tensor:
        """Queries with the same number of hints -> float64 [Q, 11 K + 1] on the device: cell rows | scores | pos_mean | pos_offset |
        world_mean | world_offset (K x 2 each) | matched | best.  (Rows and counts are small integers: exact in float64.)
        prior: None, or (xy [Q, 2], radius [Q], group [Q] or None) of these queries, already on the device (localize uploads the
        whole call's prior once, before the first launch: an upload between the chunks would wait for the work in flight) - the
        ranking then runs on t2p_sim_topk_prior; a masked candidate's row is still a real cell, so the matcher and the pose
        estimate run on it as on any other.
        distinct: None, or (radius, pool): the ranking (either family) returns `pool` cells per query and t2p_topk_distinct keeps the
        best K no two of which conflict; the rows then carry two more columns, the selection's n_valid and exhausted.  A column
        it did not fill holds the query's first pool row at -inf: a real cell, as a masked candidate of the prior path is."""
        db, mc, mf = self.database, self.model_coarse, self.model_fine
        nq, k = len(hints), int(top_k)
        for m in (mc, mf):
            if m.training:
                raise NotImplementedError("Localizer.localize: a model was put into train() mode; call .eval()")
        with torch.no_grad():
            text = mc.encode_text([" ".join(h) for h in hints])                      # io.Scenes.texts (cells.py:82)
            n_rank = k if distinct is None else int(distinct[1])
            if prior is None:
                rows, scores = retrieve_topk(db.coarse, text, n_rank)
            else:
                xy, rad, grp = prior
                boxes, _, scene_idx = self.prior_tables()
                groups = {} if grp is None else dict(cell_groups=scene_idx, query_groups=grp)
                rows, scores = retrieve_topk(db.coarse, text, n_rank, cell_boxes=boxes, query_xy=xy, query_radius=rad, validate=False,
                                             **groups)
            extra = []
            if distinct is not None:
                centers, scene_idx = self.distinct_tables()
                rows, scores, n_valid, exhausted = ops.topk_distinct(rows, scores, centers, float(distinct[0]), k, cell_group=scene_idx,
                                                                     check=False)
                extra = [n_valid, exhausted]
            hint_enc = mf.encode_hints(hints).contiguous()                           # once per query, not per candidate
            obj_row = rows.reshape(-1).to(torch.int32)
            hint_row = torch.arange(nq, dtype=torch.int32, device=rows.device).repeat_interleave(k)
            out = ops.match_indexed(db.fine, hint_enc, obj_row, hint_row, mf._match_pack(), mf.sinkhorn_iters, MATCH_THRESHOLD)
            pose = ops.localize_poses(out["matches0"], out["offsets"], obj_row, nq, k, db.center_xy, db.bbox_xy, db.cell_size,
                                      check=False)
        flat = lambda t: t.reshape(nq, -1).to(torch.float64)
        return torch.cat([flat(rows), flat(scores), flat(pose["pos_mean"]), flat(pose["pos_offset"]), flat(pose["world_mean"]),
                          flat(pose["world_offset"]), flat(pose["matched"]), flat(pose["best"])] + [flat(t) for t in extra], dim=1)

    def localize(self, hints: List[List[str]], top_k: int = 10, queries_per_call: Optional[int] = None, *, prior_xy=None,
                 prior_radius=None, scenes=None, distinct_radius=None, distinct_pool=None) -> Localization:
        """hints: one list of hint sentences per query (1 to 63 each; the coarse text of a query is " ".join(hints)).  Queries are
        grouped by their number of hints, run in calls of queries_per_call (None = min(256, 4096 // top_k), evaluation.run_fine's
        device default) and returned in the caller's order.  One device-to-host copy at the end; a sample either kernel refused to
        read through (a row outside the database, a NaN offset) raises IndexError naming query and candidate there.
        prior_xy (one (x, y) or [Q, 2], world metres) with prior_radius (one number or [Q], >= 0; inf = no geometric restriction)
        and / or scenes (one name, or Q entries each a name or None = any scene) restrict the ranking to the cells within the
        radius of the position (distance to the cell's closed square: 0 keeps the cells that contain the point) and of the named
        scene; see Localization for a query with fewer than top_k such cells.  Without them: the unrestricted call, bit for bit.
        distinct_radius (metres, >= 0, inf allowed): the candidates are top_k DIFFERENT places - walking the ranking (restricted or
        not) from the best cell, a cell is taken iff no cell taken before it lies within distinct_radius of it in x and in y
        (cell centres, strictly) in the same scene.  The cell size asks for non-overlapping cells; 0 is the plain ranking; inf one
        cell per scene.  The walk sees the distinct_pool best cells (None: min(len(db), 1024, max(64, 32 top_k)); any value in
        [top_k, min(len(db), 1024)]): Localization.exhausted marks the queries it was too short for.  Without distinct_radius the
        call is the one above, bit for bit."""
        hints = check_hints(hints)
        k = check_top_k(top_k)
        if np.ndim(top_k) != 0:
            raise ValueError("localize: top_k is one number (the candidates per query)")
        if k > len(self.database):
            raise ValueError(f"localize: top_k={k} exceeds the {len(self.database)} cells of the database")
        distinct = check_distinct_args(distinct_radius, distinct_pool, k, len(self.database))
        per_call = min(256, 4096 // k) if queries_per_call is None else int(queries_per_call)
        per_call = max(1, per_call)
        nq = len(hints)
        restricted = not (prior_xy is None and prior_radius is None and scenes is None)
        prior = check_prior(nq, prior_xy, prior_radius, scenes, sorted(set(self.database.scene_names))) if restricted else None
        self._require_device()
        chunks = [qs[a: a + per_call] for _, qs in group_by_hint_count(hints).items() for a in range(0, len(qs), per_call)]
        order = [q for chunk in chunks for q in chunk]
        if restricted:      # the prior in the order the chunks run, on the device before the first launch; a chunk takes a slice
            xy, rad, grp = prior
            if xy is None:  # a scene alone: no geometric restriction
                xy, rad = np.zeros((nq, 2)), np.full(nq, np.inf)
            sel, dev = np.asarray(order, dtype=np.int64), self.database.device
            prior = tuple(None if t is None else torch.from_numpy(np.ascontiguousarray(t[sel])).to(dev) for t in (xy, rad, grp))
        parts, at = [], 0
        for chunk in chunks:
            more = {} if distinct is None else dict(distinct=distinct)
            if restricted:
                parts.append(self._run_chunk([hints[q] for q in chunk], k, tuple(None if t is None else t[at: at + len(chunk)] for t in prior),
                                             **more))
            else:
                parts.append(self._run_chunk([hints[q] for q in chunk], k, **more))
            at += len(chunk)
        width = 11 * k + (1 if distinct is None else 3)
        packed = torch.cat(parts).cpu().numpy() if parts else np.zeros((0, width))       # the call's one device-to-host copy
        res = np.empty((nq, width), dtype=np.float64)
        res[np.asarray(order, dtype=np.int64)] = packed
        if distinct is None:
            return unpack_result(res, k, self.database.cell_ids, restricted)
        return unpack_result(res, k, self.database.cell_ids, restricted, distinct=True)

    def localize_poses(self, poses, top_k: int = 10, queries_per_call: Optional[int] = None, *, prior_xy=None, prior_radius=None,
                       scenes=None, distinct_radius=None, distinct_pool=None) -> Localization:
        """localize() on the hint sentences of data.Pose objects (evaluation.create_hint_description)."""
        from .evaluation import create_hint_description
        return self.localize([create_hint_description(p) for p in poses], top_k, queries_per_call, prior_xy=prior_xy,
                             prior_radius=prior_radius, scenes=scenes, distinct_radius=distinct_radius, distinct_pool=distinct_pool)


# ---- command line ---------------------------------------------------------------------------------------------------------------
def _load_models(a, scenes=None, words=None, classes=None):
    from . import CellRetrievalNetwork, SuperGlueMatch
    from . import data as D, io as IO
    from .pipeline import _model_args, args_from_checkpoint
    dev = torch.device("cuda", 0)
    sd, ck = IO.load_reference_checkpoint(a.path_coarse, return_args=True)
    ca = args_from_checkpoint(_model_args(a.coarse_embed_dim, use_features=a.use_features), ck, "coarse")
    coarse = CellRetrievalNetwork(classes, D.COLOR_NAMES, words, ca)
    coarse.load_state_dict(sd)
    sd, ck = IO.load_reference_checkpoint(a.path_fine, return_args=True)
    fa = args_from_checkpoint(_model_args(a.fine_embed_dim, a.fine_num_layers, a.sinkhorn_iters, a.use_features), ck, "fine")
    fine = SuperGlueMatch(classes, D.COLOR_NAMES, words, fa)
    fine.load_state_dict(sd)
    return coarse.to(dev).eval(), fine.to(dev).eval(), int(getattr(ca, "pointnet_numpoints", 256))


def read_queries(hints: Optional[List[str]], queries_file: Optional[str]) -> List[List[str]]:
    """--hints: the sentences of one query; --queries_file: one query per line, its hints separated by '|'."""
    queries = []
    if hints:
        queries.append([h.strip() for h in hints])
    if queries_file:
        with open(queries_file) as f:
            for line in f:
                if line.strip():
                    queries.append([h.strip() for h in line.strip().split("|") if h.strip()])
    if not queries:
        raise ValueError("query: give --hints or --queries_file")
    return queries


def parse_args(argv: Optional[List[str]] = None):
    """The command line of `build` and `query`, parsed and checked for flags that go together; nothing is read or loaded."""
    from .pipeline import SCENE_NAMES_VAL
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    for name in ("build", "query"):
        p = sub.add_parser(name)
        p.add_argument("--path_coarse", required=True)
        p.add_argument("--path_fine", required=True)
        p.add_argument("--coarse_embed_dim", type=int, default=256)
        p.add_argument("--fine_embed_dim", type=int, default=128)
        p.add_argument("--fine_num_layers", type=int, default=6)
        p.add_argument("--sinkhorn_iters", type=int, default=50)
        p.add_argument("--use_features", nargs="+", default=["class", "color", "position"])
        if name == "build":
            p.add_argument("--base_path", required=True)
            p.add_argument("--scenes", nargs="*", default=SCENE_NAMES_VAL)
            p.add_argument("--out", required=True)
            p.add_argument("--pad_size", type=int, default=16)
            p.add_argument("--seed", type=int, default=0, help="seed of the cells' T.FixedPoints draws")
            p.add_argument("--cells_per_call", type=int, default=2048)
        else:
            p.add_argument("--db", required=True)
            p.add_argument("--hints", nargs="+", default=None, help="the hint sentences of one query")
            p.add_argument("--queries_file", default=None, help="one query per line, its hints separated by '|'")
            p.add_argument("--top_k", type=int, default=10)
            p.add_argument("--prior", type=float, nargs=2, default=None, metavar=("X", "Y"),
                           help="prior position in world metres (with --radius); applies to every query of the invocation")
            p.add_argument("--radius", type=float, default=None, help="radius of --prior in metres (0: the cells that contain it)")
            p.add_argument("--scene", default=None, help="rank only the cells of this scene; applies to every query")
            p.add_argument("--distinct", type=float, default=None, metavar="METRES",
                           help="return top_k different places: no two candidates of a scene within METRES of each other in x and in y")
            p.add_argument("--distinct_pool", type=int, default=None, metavar="N",
                           help="ranked cells per query the distinct selection walks (with --distinct; default max(64, 32 top_k))")
            p.add_argument("--vocab_base_path", default=None, help="dataset the models' vocabulary comes from (with --vocab_scenes)")
            p.add_argument("--vocab_scenes", nargs="*", default=SCENE_NAMES_VAL)
    a = ap.parse_args(argv)
    if a.command == "query" and (a.prior is None) != (a.radius is None):
        ap.error("--prior X Y and --radius R go together")
    if a.command == "query" and a.distinct_pool is not None and a.distinct is None:
        ap.error("--distinct_pool N needs --distinct METRES")
    return a


def main(argv: Optional[List[str]] = None):
    from . import data as D, io as IO
    from .pipeline import PerCellTransform
    a = parse_args(argv)
    if a.command == "build":
        scenes = IO.load_scenes(a.base_path, a.scenes)
        coarse, fine, n_pts = _load_models(a, words=scenes.get_known_words(), classes=scenes.get_known_classes())
        db = CellDatabase.build(coarse, fine, scenes.all_cells, PerCellTransform(n_pts, a.seed), a.pad_size, a.cells_per_call)
        db.meta["known_words"] = [str(w) for w in scenes.get_known_words()]     # the query command rebuilds the models' vocabulary
        db.save(a.out)
        print(json.dumps(dict(out=a.out, cells=len(db), pad_size=a.pad_size, dim_coarse=db.meta["dim_coarse"], dim_fine=db.meta["dim_fine"])))
        return db
    check_top_k(a.top_k)                                                          # before the checkpoints are read
    queries = check_hints(read_queries(a.hints, a.queries_file))
    db = CellDatabase.load(a.db)
    check_prior(len(queries), a.prior, a.radius, a.scene, sorted(set(db.scene_names)))   # before the checkpoints are read
    check_distinct_args(a.distinct, a.distinct_pool, int(a.top_k), len(db))
    if a.vocab_base_path:
        words = IO.load_scenes(a.vocab_base_path, a.vocab_scenes).get_known_words()
    elif "known_words" in db.meta:
        words = list(db.meta["known_words"])
    else:
        raise ValueError("query: the database carries no vocabulary; give --vocab_base_path")
    coarse, fine, _ = _load_models(a, words=words, classes=list(D.KNOWN_CLASSES))
    res = Localizer(coarse, fine, db.to(coarse.device)).localize(queries, a.top_k, prior_xy=a.prior, prior_radius=a.radius, scenes=a.scene,
                                                                distinct_radius=a.distinct, distinct_pool=a.distinct_pool)
    for q in range(len(queries)):
        print(json.dumps(res.to_json(q)))
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
