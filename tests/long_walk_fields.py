"""Inputs of the long-walk tests (tests/test_long_walks.py, tests/test_gpu_long_walks.py): two
volumes large enough that every kernel walking the stored volume takes a second trip of its
capped grid, a second group or a second staging chunk, filled from a thin deterministic surface
band so that the NumPy restatements stay cheap; and the table of those trips, groups and chunks
as data ("Long walks"), with the maps from a voxel to its place in each.

Storage order (semtsdf_internal.h): a tile is the 1 x 8 x 32 (x, y, z) block of 256 consecutive
stored voxels, ordered (z / 4, y, z % 4) inside; tile index = x * nuy * nuz + (y / 8) * nuz + z / 32
with nuy = ceil(Y / 8), nuz = ceil(Z / 32).  Reference order: v = (x * Y + y) * Z + z."""
from collections import namedtuple

import numpy as np

TILE = 256

# name: the row; constant: its name in csrc/semtsdf_internal.h; value: what the source must say;
# per: elements one count of the constant stands for; order: "tile" (stored index, padding included),
# "ref" (reference index) or "flat" (a plain array); elems: elements a voxel contributes (3 colour
# channels); within: the row whose chunk the count restarts in; walker: the code the row is about.
Trip = namedtuple("Trip", "name constant value per order elems within walker")
TRIPS = (
    Trip("mesh_group", "kMeshGroup", 4096, TILE, "tile", 1, None,
         "k_mesh_scan's cross-group prefix (gsum) and totals, k_mesh_classify's gsum[blk / kMeshGroup]"),
    Trip("instance_trip", "kInstBlocks", 2048, 4 * TILE, "tile", 1, None,
         "k_instance_stats' persistent loop (4 waves a block)"),
    Trip("remap_trip", "kRemapBlocks", 16384, TILE, "tile", 1, None, "k_remap_instances"),
    Trip("hist_mask_trip", "kHistMaskBlocks", 16384, TILE, "tile", 1, None, "k_hist_mask after a histogram upload"),
    Trip("hist_chunk", "kHistChunk", 1 << 22, 1, "ref", 1, None, "hist_xfer's staging chunks (k_hist_to_bm with v0 > 0)"),
    Trip("color_chunk", "kColorChunk", 1 << 24, 1, "ref", 1, None,
         "color_xfer's staging chunks (k_color_from_ref with v0 > 0)"),
    Trip("vox_upload_trip", "kXferBlocks", 16384, TILE, "ref", 1, None,
         "k_vox_from_ref's grid loop (volumes below vox_xfer's 2^26 chunk)"),
    Trip("color_upload_trip", "kXferBlocks", 16384, TILE, "ref", 3, "color_chunk",
         "k_color_from_ref's grid loop inside one staging chunk"),
    Trip("export_trip", "kExportBlocks", 65536, TILE, "ref", 1, None, "k_export_surface"),
    Trip("weight_widen_trip", "kWidenBlocks", 65536, TILE, "tile", 1, None, "k_weight_widen"),
    Trip("color_widen_trip", "kWidenBlocks", 65536, TILE, "tile", 1, None, "k_color_widen"),
    Trip("min_i64_trip", "kMinBlocks", 4096, TILE, "flat", 1, None, "k_min_i64 (semtsdf_min_i64)"),
)
TRIP = {t.name: t for t in TRIPS}

GAP = ((128, 256),)
VOLUME_A = {"dims": (600, 60, 120), "flags": 0x3, "seed": 11, "gaps": GAP}
VOLUME_B = {"dims": (276, 250, 250), "flags": 0x4, "seed": 12, "gaps": GAP}


def unit(name):
    """Elements (of the row's order) in one trip, group or chunk."""
    t = TRIP[name]
    return t.value * t.per


def tiles_shape(dims):
    """(nuy, nuz): tiles along y and z."""
    return (dims[1] + 7) // 8, (dims[2] + 31) // 32


def stored_voxels(dims):
    nuy, nuz = tiles_shape(dims)
    return dims[0] * nuy * nuz * TILE


def tile_index(dims, x, y, z):
    nuy, nuz = tiles_shape(dims)
    return (np.asarray(x, np.int64) * nuy + (np.asarray(y, np.int64) >> 3)) * nuz + (np.asarray(z, np.int64) >> 5)


def stored_index(dims, x, y, z):
    y, z = np.asarray(y, np.int64), np.asarray(z, np.int64)
    return tile_index(dims, x, y, z) * TILE + ((z >> 2) & 7) * 32 + (y & 7) * 4 + (z & 3)


def ref_index(dims, x, y, z):
    return (np.asarray(x, np.int64) * dims[1] + np.asarray(y, np.int64)) * dims[2] + np.asarray(z, np.int64)


def trip_of(name, dims, x, y, z):
    """The trip, group or chunk of row `name` that handles voxel (x, y, z) of a volume of `dims`
    (for a row inside a staging chunk: the trip of the voxel's first element in its chunk)."""
    t = TRIP[name]
    if t.order == "flat":
        raise ValueError(f"{name} walks a plain array, not a volume")
    i = stored_index(dims, x, y, z) if t.order == "tile" else ref_index(dims, x, y, z)
    if t.within:
        i = i % unit(t.within)
    return i * t.elems // unit(name)


def trip_count(name, dims):
    """Trips, groups or chunks of row `name` over a whole volume of `dims` (for a row inside a
    staging chunk: over the first chunk)."""
    t = TRIP[name]
    n = stored_voxels(dims) if t.order == "tile" else dims[0] * dims[1] * dims[2]
    if t.within:
        n = min(n, unit(t.within))
    return int(-(-n * t.elems // unit(name)))


def band_field(dims, seed, gaps=(), semantic=False):
    """sdf f32, wt i32, color u8 [X, Y, Z, 3], hist u32 [X, Y, Z, 32] (None unless semantic) of a
    thin surface z = zs(x, y): d = zs - z; inside |d| < 4 sdf = clip(d / 4, -1, 1) + noise in
    +-0.05, elsewhere exactly 1.0; 90 % of the band is observed (weights 1..4), none of it for x
    in an interval [a, b) of `gaps`; an observed voxel votes for three random bins with counts
    1..8, and 50 000 single votes fall on random voxels anywhere."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    x = np.arange(X, dtype=np.float64)[:, None]
    y = np.arange(Y, dtype=np.float64)[None, :]
    zs = Z / 2.0 + Z / 4.0 * np.sin(x / 23.0) + Z / 10.0 * np.cos(y / 7.0)
    d = (zs[:, :, None] - np.arange(Z, dtype=np.float64)[None, None, :]).astype(np.float32)
    band = np.abs(d) < np.float32(4.0)
    sdf = np.ones(dims, np.float32)
    nb = int(band.sum())
    sdf[band] = np.clip(np.float32(0.25) * d[band], np.float32(-1.0), np.float32(1.0)) + rng.uniform(
        -0.05, 0.05, nb).astype(np.float32)
    obs = band.copy()
    obs[band] = rng.random(nb) < 0.9
    for a, b in gaps:
        obs[a:b] = False
    no = int(obs.sum())
    wt = np.zeros(dims, np.int32)
    wt[obs] = rng.integers(1, 5, no).astype(np.int32)
    color = rng.integers(0, 256, dims + (3,), dtype=np.uint8)
    hist = None
    if semantic:
        hist = np.zeros((X * Y * Z, 32), np.uint32)
        rows = np.flatnonzero(obs.reshape(-1))
        bins = rng.integers(0, 32, (no, 3))
        counts = rng.integers(1, 9, (no, 3)).astype(np.uint32)
        for j in range(3):  # a repeated bin keeps its last count
            hist[rows, bins[:, j]] = counts[:, j]
        np.add.at(hist, (rng.integers(0, X * Y * Z, 50000), rng.integers(0, 32, 50000)), np.uint32(1))
        hist = hist.reshape(dims + (32,))
    return sdf, wt, color, hist


def vote_rows(hist):
    """Reference indices of the voxels with a vote, ascending."""
    return np.flatnonzero(hist.reshape(-1, 32).any(axis=1))


def bin_major(hist):
    """`hist` [X, Y, Z, 32] again, equal value by value, as a view of bin-major memory: the
    restatements pass over one bin of every voxel at a time, which is contiguous here and a stride
    of 128 B in `hist`.  Built from the rows with votes."""
    h = hist.reshape(-1, 32)
    rows = vote_rows(hist)
    bm = np.zeros((32, h.shape[0]), np.uint32)
    bm[:, rows] = h[rows].T
    return np.moveaxis(bm.reshape((32,) + hist.shape[:-1]), 0, -1)
