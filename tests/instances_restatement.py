"""NumPy restatement of the instance-inventory and id-remap contracts (include/semtsdf.h,
DESIGN.md "Instance inventory"), from downloaded arrays alone: the selection of
semtsdf_export_surface, the argmax with first maximum, the twelve fields of semtsdf_instance,
the overlap table, and the histogram through a lookup table.  Shared by tests/test_instances.py
and tests/test_gpu_instances.py."""
import numpy as np

FIELDS = ("voxels", "votes", "support", "index_sum", "rgb_sum", "bbox_min", "bbox_max")

# the identity except 7 -> 3, 9 -> 0, 31 -> 4 and the cycle 5 <-> 6
HAZARD_LUT = np.arange(32, dtype=np.uint8)
HAZARD_LUT[[7, 9, 31, 5, 6]] = [3, 0, 4, 6, 5]


def restate_stats(sdf, wt, color, hist, sdf_max, min_weight, gz=None, owned=None):
    """sdf f32 [Dx, Dy, Lz], wt i32, color [Dx, Dy, Lz, 3] (u8 or i32), hist u32 [Dx, Dy, Lz, 32];
    gz [Lz]: the global z of every stored plane (None: the plane index), owned [Lz] bool: the
    planes this handle owns (None: all).  Returns the integer fields and `overlap` as arrays, and
    `label` / `selected` per voxel."""
    D = sdf.shape
    gz = np.arange(D[2]) if gz is None else np.asarray(gz)
    owned = np.ones(D[2], bool) if owned is None else np.asarray(owned, bool)
    sel = (wt >= min_weight) & (np.abs(sdf) < np.float32(sdf_max)) & owned[None, None, :]
    h = hist.reshape(D + (32,))
    label = np.zeros(D, np.int64)
    best = np.zeros(D, np.uint32)
    for k in range(32):  # first maximum, counts > 0 only
        better = h[..., k] > best
        label[better] = k
        best[better] = h[..., k][better]
    x, y, z = np.nonzero(sel)
    lab = label[x, y, z]
    idx = np.stack([x, y, gz[z]], axis=1).astype(np.uint64)
    rgb = np.clip(color.reshape(D + (3,))[x, y, z].astype(np.int64), 0, 255).astype(np.uint64)
    present = h[x, y, z] != 0  # [n, 32]
    out = {"voxels": np.bincount(lab, minlength=32).astype(np.uint64),
           "votes": np.zeros(32, np.uint64), "support": present.sum(axis=0).astype(np.uint64),
           "index_sum": np.zeros((32, 3), np.uint64), "rgb_sum": np.zeros((32, 3), np.uint64),
           "bbox_min": np.full((32, 3), 0xFFFFFFFF, np.uint32), "bbox_max": np.zeros((32, 3), np.uint32)}
    np.add.at(out["votes"], lab, best[x, y, z].astype(np.uint64))
    np.add.at(out["index_sum"], lab, idx)
    np.add.at(out["rgb_sum"], lab, rgb)
    for k in np.unique(lab):
        out["bbox_min"][k] = idx[lab == k].min(axis=0)
        out["bbox_max"][k] = idx[lab == k].max(axis=0)
    p = present.astype(np.uint64)
    out["overlap"] = p.T @ p
    out["label"], out["selected"] = label, sel
    return out


def remap_hist(hist, lut):
    """hist' [..., j] = sum of hist[..., k] over lut[k] == j, u32 modulo 2^32."""
    h = hist.reshape(-1, 32).astype(np.uint32)
    out = np.zeros_like(h)
    with np.errstate(over="ignore"):
        for k in range(32):
            out[:, int(lut[k])] += h[:, k]
    return out.reshape(hist.shape)


def assert_stats_equal(got, want, overlap=True):
    for k in FIELDS:
        assert np.array_equal(np.asarray(got[k]).astype(np.uint64), np.asarray(want[k]).astype(np.uint64)), k
    if overlap:
        assert np.array_equal(np.asarray(got["overlap"], np.uint64), np.asarray(want["overlap"], np.uint64)), "overlap"
