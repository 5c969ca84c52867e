"""Instance inventory of a semantic volume and the planning of id remaps (no reference
counterpart: the reference mints ids as num_objs++ (src/SfM_CUDA/tsdf.cu:379-383) and never
merges or retires one; its Configuration::duplicate_thresh (configuration.h:9) is read by
nothing).  The device work is semtsdf_instance_stats and semtsdf_remap_instances; everything
here is host logic on 32-entry tables."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

_INSTANCE = np.dtype([("voxels", "<u8"), ("votes", "<u8"), ("support", "<u8"), ("sum", "<u8", (3,)),
                      ("rgb_sum", "<u8", (3,)), ("min", "<u4", (3,)), ("max", "<u4", (3,))])
assert _INSTANCE.itemsize == C.sizeof(L.Instance) == 96
_SUMS = ("voxels", "votes", "support", "index_sum", "rgb_sum")


def _derive(st: dict) -> dict:
    """The f64 fields computed from the integer ones (NaN for an id without a voxel)."""
    n = st["voxels"].astype(np.float64)[:, None]
    start, voxel = st["vol_start"][None, :], st["voxel"][None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        st["centroid"] = start + st["index_sum"].astype(np.float64) / n * voxel
        st["mean_rgb"] = st["rgb_sum"].astype(np.float64) / n
    none = (st["voxels"] == 0)[:, None]
    st["bbox_world_min"] = np.where(none, np.nan, start + st["bbox_min"].astype(np.float64) * voxel)
    st["bbox_world_max"] = np.where(none, np.nan, start + st["bbox_max"].astype(np.float64) * voxel)
    return st


def stats_from_records(rec: np.ndarray, overlap, vol_start, voxel) -> dict:
    """The stats dict from 32 semtsdf_instance records (a structured array) and the overlap table."""
    st = {"voxels": rec["voxels"].copy(), "votes": rec["votes"].copy(), "support": rec["support"].copy(),
          "index_sum": np.ascontiguousarray(rec["sum"]), "rgb_sum": np.ascontiguousarray(rec["rgb_sum"]),
          "bbox_min": np.ascontiguousarray(rec["min"]), "bbox_max": np.ascontiguousarray(rec["max"]),
          "overlap": None if overlap is None else np.asarray(overlap, np.uint64).reshape(32, 32).copy(),
          "vol_start": np.asarray(vol_start, np.float64).reshape(3), "voxel": np.asarray(voxel, np.float64).reshape(3)}
    return _derive(st)


def instance_stats(vol, sdf_max: float = 0.2, min_weight: int = 1, overlap: bool = True) -> dict:
    """What `vol` (semantic) contains, per instance id (semtsdf_instance_stats: the voxels
    semtsdf_export_surface selects, labelled by their histogram's argmax).  Arrays of length 32:
    voxels, votes, support (u64), index_sum and rgb_sum [32, 3] u64, bbox_min / bbox_max [32, 3]
    u32 (voxel index; an id without a voxel has min = 2^32 - 1, max = 0), overlap [32, 32] u64
    (voxels where both bins are nonzero; None when not asked for), and in f64 centroid,
    bbox_world_min / bbox_world_max (vol_start + index * voxel) and mean_rgb (NaN without a
    voxel).  A shard reports its owned planes; merge_instance_stats adds a group's."""
    lib = L.load()
    rec = np.zeros(L.MAX_OBJECTS, _INSTANCE)
    ov = np.zeros((L.MAX_OBJECTS, L.MAX_OBJECTS), np.uint64) if overlap else None
    L.check(lib.semtsdf_instance_stats(vol.handle, float(sdf_max), int(min_weight), L.ptr(rec.view(np.uint8)),
                                       L.ptr(ov)))
    p = vol.params
    return stats_from_records(rec, ov, list(p.vol_start), list(p.voxel))


def merge_instance_stats(parts: list) -> dict:
    """The stats of the whole from those of disjoint parts (the shards of a group): sums added,
    boxes by min / max, the derived fields recomputed."""
    if not parts:
        raise ValueError("no stats to merge")
    st = {k: np.sum([np.asarray(p[k], np.uint64) for p in parts], axis=0, dtype=np.uint64) for k in _SUMS}
    st["bbox_min"] = np.min([p["bbox_min"] for p in parts], axis=0).astype(np.uint32)
    st["bbox_max"] = np.max([p["bbox_max"] for p in parts], axis=0).astype(np.uint32)
    ovs = [p.get("overlap") for p in parts]
    st["overlap"] = None if any(o is None for o in ovs) else np.sum(ovs, axis=0, dtype=np.uint64)
    st["vol_start"], st["voxel"] = parts[0]["vol_start"].copy(), parts[0]["voxel"].copy()
    return _derive(st)


def _groups(stats: dict, thresh: float) -> np.ndarray:
    """root[k]: the smallest id of k's duplicate group (k itself when it has none)."""
    ov = stats["overlap"]
    if ov is None:
        raise ValueError("duplicate detection needs the overlap table (instance_stats(overlap=True))")
    sup = np.asarray(stats["support"], np.float64)
    root = np.arange(L.MAX_OBJECTS)

    def find(k):
        while root[k] != k:
            k = root[k]
        return k

    for a in range(1, L.MAX_OBJECTS):
        for b in range(a + 1, L.MAX_OBJECTS):
            if sup[a] <= 0 or sup[b] <= 0:
                continue
            inter = float(ov[a, b])
            if inter / (sup[a] + sup[b] - inter) > thresh:
                ra, rb = find(a), find(b)
                root[max(ra, rb)] = min(ra, rb)
    return np.array([find(k) for k in range(L.MAX_OBJECTS)])


def find_duplicates(stats: dict, thresh: float) -> list:
    """Pairs (keep, drop): ids a < b, both >= 1 with support > 0, are duplicates when the IoU of
    their supports, overlap[a, b] / (support[a] + support[b] - overlap[a, b]), exceeds `thresh`;
    the groups are the connected components and every member maps to its group's smallest id."""
    root = _groups(stats, float(thresh))
    return [(int(root[k]), k) for k in range(1, L.MAX_OBJECTS) if root[k] != k]


def plan_remap(stats: dict, num_objs: int, duplicate_thresh: float | None = None, min_voxels: int = 0,
               compact: bool = True):
    """A table for semtsdf_remap_instances and the id count that goes with it: duplicates
    (find_duplicates at duplicate_thresh; None: no merging) map to their group's smallest id, then
    ids >= 1 whose merged voxel count is below min_voxels map to 0, then with `compact` the
    surviving ids below num_objs are renumbered 1..m in increasing order and the count becomes
    m + 1 (otherwise num_objs is kept).  Returns (lut u8 [32], new_num_objs)."""
    live = max(1, min(int(num_objs), L.MAX_OBJECTS))
    lut = np.arange(L.MAX_OBJECTS)
    if duplicate_thresh is not None:
        for keep, drop in find_duplicates(stats, duplicate_thresh):
            if keep < live and drop < live:
                lut[drop] = keep
    vox = np.zeros(L.MAX_OBJECTS, np.uint64)
    np.add.at(vox, lut, np.asarray(stats["voxels"], np.uint64))
    for k in range(1, live):
        if vox[lut[k]] < min_voxels:
            lut[k] = 0
    new_num = int(num_objs)
    if compact:
        keep = [k for k in range(1, live) if lut[k] == k]
        new = np.arange(L.MAX_OBJECTS)
        new[keep] = np.arange(1, len(keep) + 1)
        lut[:live] = new[lut[:live]]
        new_num = len(keep) + 1
    return lut.astype(np.uint8), new_num


__all__ = ["instance_stats", "merge_instance_stats", "find_duplicates", "plan_remap", "stats_from_records"]
