"""Model maps of a view (semtsdf_render_maps, include/semtsdf.h): the fused model's hit
distance, world position, surface normal, instance id, vote count and validity byte per pixel,
and what a host does with them: the camera of a frame pose, the depth image the model predicts
for that frame, and the shaded-surface display.  The maps come from the HIP kernel; the helpers
here only post-process them on the host.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L

# name -> (dtype, channels) of each map
MAP_LAYOUT = {"t": (np.float32, 1), "point": (np.float32, 3), "normal": (np.float32, 3), "label": (np.uint8, 1),
              "votes": (np.float32, 1), "flags": (np.uint8, 1)}


def pose_camera(Kinv, E):
    """(s2w, c) of the camera whose pixel grid is that of a frame fused with extrinsic E
    (semtsdf_pose_camera): s2w = [E[:3,:3]^T Kinv[:3,:3] | o; 0 0 0 1], c = o = -E[:3,:3]^T E[:3,3]."""
    ki = L.f32(Kinv, 16)
    e = L.f32(E, 16)
    s2w = np.zeros(16, np.float32)
    c = np.zeros(3, np.float32)
    L.check(L.load().semtsdf_pose_camera(L.ptr(ki), L.ptr(e), L.ptr(s2w), L.ptr(c)))
    return s2w, c


def maps_out(want, pointers) -> L.MapsOut:
    """semtsdf_maps_out with pointers[name] for every name in want (NULL elsewhere)."""
    bad = [w for w in want if w not in MAP_LAYOUT]
    if bad:
        raise ValueError(f"unknown map {bad[0]!r} (one of {', '.join(L.MAP_NAMES)})")
    o = L.MapsOut()
    for name in want:
        p = pointers[name]
        setattr(o, name, p.ctypes.data if isinstance(p, np.ndarray) else int(p))
    return o


def z_depth(point, flags, E):
    """Camera-frame z of each hit, (E (P, 1))[2], in f64 [H, W]; NaN on misses.  With the maps of
    pose_camera(Kinv, E) this is the depth image (in metres) the model predicts for that frame."""
    e = np.asarray(E, np.float64).reshape(4, 4)
    p = np.asarray(point, np.float64)
    z = p[..., 0] * e[2, 0] + p[..., 1] * e[2, 1] + p[..., 2] * e[2, 2] + e[2, 3]
    return np.where((np.asarray(flags) & L.MAP_HIT) != 0, z, np.nan)


def shade_normals(maps, c, ambient: int = 32):
    """Grey Lambert shading of the surface towards the camera centre c: u8 [H, W, 3], the grey
    ambient + (255 - ambient) * max(0, n . l) with l the unit vector from the point to c, black
    where bit 1 of flags (MAP_NORMAL) is clear."""
    n = np.asarray(maps["normal"], np.float64)
    p = np.asarray(maps["point"], np.float64)
    ok = (np.asarray(maps["flags"]) & L.MAP_NORMAL) != 0
    l = np.asarray(c, np.float64).reshape(3) - p
    norm = np.sqrt((l * l).sum(axis=-1))
    lam = np.clip((n * l).sum(axis=-1) / np.where(norm > 0, norm, 1.0), 0.0, 1.0)
    grey = np.where(ok, np.floor(ambient + (255 - ambient) * lam), 0).astype(np.uint8)
    return np.repeat(grey[..., None], 3, axis=-1)


__all__ = ["pose_camera", "z_depth", "shade_normals", "maps_out", "MAP_LAYOUT"]
