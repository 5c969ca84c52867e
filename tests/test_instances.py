"""Instance inventory and id remapping without a device: the NumPy restatement on the fixed
random field (counts pinned, so it cannot pass vacuously), the host planning logic
(find_duplicates, plan_remap, merge_instance_stats) on hand-made stats, and the argument errors
of both entry points."""
import numpy as np

from instances_restatement import FIELDS, HAZARD_LUT, assert_stats_equal, remap_hist, restate_stats
from mesh_restatement import random_field
from semtsdf.instances import _INSTANCE, find_duplicates, merge_instance_stats, plan_remap, stats_from_records

FIELD_DIMS = (11, 13, 37)


def _field():
    f = random_field(FIELD_DIMS)
    f["color"] = np.clip(f["color"], 0, 255).astype(np.uint8)
    return f


def _stats(voxels=None, support=None, overlap=None):
    """Hand-made stats: only what the planning reads."""
    rec = np.zeros(32, _INSTANCE)
    rec["min"] = 0xFFFFFFFF
    for k, n in (voxels or {}).items():
        rec["voxels"][k] = n
    ov = np.zeros((32, 32), np.uint64)
    for k, n in (support or {}).items():
        rec["support"][k] = n
        ov[k, k] = n
    for (a, b), n in (overlap or {}).items():
        ov[a, b] = ov[b, a] = n
    return stats_from_records(rec, ov, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def test_restatement_on_the_random_field():
    f = _field()
    r = restate_stats(f["sdf"], f["wt"], f["color"], f["hist"], 0.2, 1)
    assert int(r["selected"].sum()) == 1027 and int(r["voxels"].sum()) == 1027
    assert int(r["voxels"].min()) == 19 and int(r["voxels"].max()) == 86 and int(r["voxels"][0]) == 86
    h = f["hist"][r["selected"]]
    top = h.max(axis=1)
    assert int((((h == top[:, None]).sum(axis=1) > 1) & (top > 0)).sum()) == 155  # a tied maximum: the first wins
    assert int((top == 0).sum()) == 50                                            # no count: label 0
    assert np.array_equal(r["overlap"], r["overlap"].T)
    assert np.array_equal(np.diag(r["overlap"]), r["support"])
    assert (r["bbox_min"] <= r["bbox_max"]).all()
    r2 = restate_stats(f["sdf"], f["wt"], f["color"], f["hist"], 0.5, 3)
    assert int(r2["selected"].sum()) == 1124 and int(r2["voxels"].sum()) == 1124
    assert np.array_equal(r2["overlap"], r2["overlap"].T) and np.array_equal(np.diag(r2["overlap"]), r2["support"])


def test_remap_restatement_on_the_random_field():
    f = _field()
    new = remap_hist(f["hist"], HAZARD_LUT)
    assert int((new != f["hist"]).any(axis=-1).sum()) == 1934 and int(np.prod(FIELD_DIMS)) == 5291
    assert np.array_equal(new.sum(axis=-1), f["hist"].sum(axis=-1))  # votes move, none is lost
    assert np.array_equal(new[..., 5], f["hist"][..., 6]) and np.array_equal(new[..., 6], f["hist"][..., 5])
    assert not new[..., [7, 9, 31]].any()
    assert np.array_equal(remap_hist(f["hist"], np.arange(32)), f["hist"])


def test_find_duplicates_chain_collapses_to_the_smallest_id():
    # 3-5 and 5-9 overlap above the threshold, 3-9 do not: one group, everything to 3
    st = _stats(support={3: 100, 5: 100, 9: 100, 12: 100}, overlap={(3, 5): 80, (5, 9): 80, (3, 9): 10, (9, 12): 30})
    assert find_duplicates(st, 0.5) == [(3, 5), (3, 9)]
    assert find_duplicates(st, 0.9) == []
    # IoU exactly at the threshold is not a duplicate: 50 / (100 + 50 - 50) = 0.5
    st = _stats(support={1: 100, 2: 50}, overlap={(1, 2): 50})
    assert find_duplicates(st, 0.5) == [] and find_duplicates(st, 0.49) == [(1, 2)]
    # background and ids without support never pair
    st = _stats(support={0: 100, 4: 100}, overlap={(0, 4): 100, (4, 6): 0})
    assert find_duplicates(st, 0.1) == []


def test_plan_remap_merges_drops_and_compacts():
    st = _stats(voxels={1: 500, 2: 40, 3: 30, 4: 5, 5: 300, 6: 8},
                support={1: 500, 2: 100, 3: 100, 4: 5, 5: 300, 6: 8}, overlap={(2, 3): 90})
    ident = np.arange(32, dtype=np.uint8)
    # nothing qualifies: the identity, and compaction of ids already 1..6 keeps the count
    lut, n = plan_remap(st, 7, duplicate_thresh=0.95, min_voxels=0, compact=True)
    assert np.array_equal(lut, ident) and n == 7 and lut.dtype == np.uint8
    lut, n = plan_remap(st, 7, duplicate_thresh=None, min_voxels=0, compact=False)
    assert np.array_equal(lut, ident) and n == 7
    # min_voxels applies after merging: 2 + 3 have 70 voxels together and survive a bound of 50
    # that either alone would miss; 4 and 6 are dissolved
    lut, n = plan_remap(st, 7, duplicate_thresh=0.5, min_voxels=50, compact=False)
    want = ident.copy()
    want[[3, 4, 6]] = [2, 0, 0]
    assert np.array_equal(lut, want) and n == 7
    # compact: the survivors 1, 2, 5 become 1, 2, 3 in order; m + 1 = 4
    lut, n = plan_remap(st, 7, duplicate_thresh=0.5, min_voxels=50, compact=True)
    want = ident.copy()
    want[1:7] = [1, 2, 2, 0, 3, 0]
    assert np.array_equal(lut, want) and n == 4
    # a merged group below the bound is dissolved as a whole
    lut, n = plan_remap(st, 7, duplicate_thresh=0.5, min_voxels=100, compact=True)
    want = ident.copy()
    want[1:7] = [1, 0, 0, 0, 2, 0]
    assert np.array_equal(lut, want) and n == 3
    # the plans satisfy the entry point's rule: 1 + max lut[k < cur] <= n <= cur
    assert 1 + int(lut[:7].max()) <= n <= 7 and lut[0] == 0


def test_merge_instance_stats_of_a_split_equals_the_whole():
    f = _field()
    start, voxel = (-0.3, 0.1, 0.5), (0.011, 0.012, 0.013)

    def as_stats(r):
        rec = np.zeros(32, _INSTANCE)
        for k, name in (("voxels", "voxels"), ("votes", "votes"), ("support", "support"), ("index_sum", "sum"),
                        ("rgb_sum", "rgb_sum"), ("bbox_min", "min"), ("bbox_max", "max")):
            rec[name] = r[k]
        return stats_from_records(rec, r["overlap"], start, voxel)

    gz = np.arange(FIELD_DIMS[2])
    whole = as_stats(restate_stats(f["sdf"], f["wt"], f["color"], f["hist"], 0.2, 1))
    parts = [as_stats(restate_stats(f["sdf"], f["wt"], f["color"], f["hist"], 0.2, 1, owned=own))
             for own in (gz % 3 == 0, gz % 3 == 1, gz % 3 == 2)]
    assert all(int(p["voxels"].sum()) > 0 for p in parts)
    merged = merge_instance_stats(parts)
    assert_stats_equal(merged, whole)
    for k in ("centroid", "mean_rgb", "bbox_world_min", "bbox_world_max"):
        assert np.array_equal(merged[k], whole[k], equal_nan=True), k
    # the derived fields: the mean index in world units, boxes in world units
    k = int(np.argmax(whole["voxels"]))
    want = np.array(start) + whole["index_sum"][k] / float(whole["voxels"][k]) * np.array(voxel)
    assert np.allclose(whole["centroid"][k], want, rtol=0, atol=1e-12)
    assert np.allclose(whole["bbox_world_min"][k], np.array(start) + whole["bbox_min"][k] * np.array(voxel), atol=1e-12)
    assert set(FIELDS) <= set(merged)


def test_instance_struct_size():
    import ctypes as C

    from semtsdf import _lib as L

    assert C.sizeof(L.Instance) == 96


def test_instance_entry_points_argument_errors_without_a_device():
    """NULL handle, NULL out and NULL lut (and a bad sdf_max or table) are refused before any
    device work: the fake handle is never dereferenced."""
    import ctypes as C

    from semtsdf import _lib as L

    lib = L.load()
    out = (L.Instance * 32)()
    lut = (C.c_uint8 * 32)(*range(32))
    handle = C.c_void_p(0x1000)
    rc = lib.semtsdf_instance_stats(None, 0.2, 1, C.cast(out, C.c_void_p), None)
    assert rc == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    rc = lib.semtsdf_instance_stats(handle, 0.2, 1, None, None)
    assert rc == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    for bad in (0.0, -1.0, float("nan")):
        rc = lib.semtsdf_instance_stats(handle, bad, 1, C.cast(out, C.c_void_p), None)
        assert rc == L.ERR_INVALID and b"sdf_max" in lib.semtsdf_last_error()
    rc = lib.semtsdf_remap_instances(None, C.cast(lut, C.c_void_p), -1, None)
    assert rc == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    rc = lib.semtsdf_remap_instances(handle, None, -1, None)
    assert rc == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    lut[0] = 1
    rc = lib.semtsdf_remap_instances(handle, C.cast(lut, C.c_void_p), -1, None)
    assert rc == L.ERR_INVALID and b"lut[0]" in lib.semtsdf_last_error()
    lut[0], lut[9] = 0, 32
    rc = lib.semtsdf_remap_instances(handle, C.cast(lut, C.c_void_p), -1, None)
    assert rc == L.ERR_INVALID and b"lut[9]" in lib.semtsdf_last_error()
