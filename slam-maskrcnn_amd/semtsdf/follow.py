"""When the volume should follow the camera, and what leaves it when it does.

Pure host code in float64 with no device access: the rule that recentres the cube on what the
camera looks at (plan_shift), the voxels a shift pushes out (leaving) and their surface points
(evicted_points, a filter over semtsdf.export.export_surface).  The move itself is
Volume.shift (semtsdf_shift); TSDF.follow ties the three together.
"""
from __future__ import annotations

import numpy as np

BRICK = 8  # voxels: the brick of the empty-space map, the unit of a shift


def plan_shift(vol_start, vol_end, voxel, E, focus_depth, trigger_bricks=2):
    """The shift (sx, sy, sz) in voxels that brings the cube's centre back to the camera's focus,
    or None while the focus is closer than `trigger_bricks` bricks to it on every axis.

    E is the volume-to-camera extrinsic (4 x 4, the one parse_frame derives: x_cam = R x + t).
    Camera origin o = -R^T t, viewing direction d = R^T (0, 0, 1), focus f = o + focus_depth * d,
    centre c = (vol_start + vol_end) / 2, b[a] = trunc((f[a] - c[a]) / (8 * voxel[a])) towards
    zero; the shift is 8 * b."""
    E = np.asarray(E, np.float64).reshape(4, 4)
    R, t = E[:3, :3], E[:3, 3]
    o = -R.T @ t
    d = R.T @ np.array([0.0, 0.0, 1.0])
    f = o + float(focus_depth) * d
    start = np.asarray(vol_start, np.float64).reshape(3)
    end = np.asarray(vol_end, np.float64).reshape(3)
    c = (start + end) / 2
    b = np.trunc((f - c) / (BRICK * np.asarray(voxel, np.float64).reshape(3))).astype(np.int64)
    if int(np.abs(b).max()) < int(trigger_bricks):
        return None
    return tuple(int(BRICK * x) for x in b)


def leaving(dim, shift):
    """A function of voxel indices [..., 3] (before the shift) returning a boolean array: True
    where the voxel leaves the volume, i.e. its new index j - shift is outside [0, dim) on some
    axis."""
    dim = np.asarray(dim, np.int64).reshape(3)
    s = np.asarray(shift, np.int64).reshape(3)

    def mask(index):
        j = np.asarray(index).astype(np.int64) - s
        return ((j < 0) | (j >= dim)).any(axis=-1)

    return mask


def evicted_points(vol, shift, sdf_max: float = 0.2, min_weight: int = 1) -> dict:
    """The surface points of `vol` (a Volume, before the shift) that `shift` pushes out: the
    dict of semtsdf.export.export_surface restricted to the leaving indices, positions from the
    placement the volume has now."""
    from .export import export_surface

    pts = export_surface(vol, sdf_max, min_weight)
    keep = leaving(list(vol.params.dim), shift)(pts["index"])
    return {k: v[keep] for k, v in pts.items()}
