"""semtsdf_instance_stats and semtsdf_remap_instances on the device against the NumPy restatement
of their contracts (tests/instances_restatement.py) applied to the downloaded volume: every
field exactly, the in-place remap with its hazards, a pipeline that continues after a remap,
shards, and TSDF.prune_instances end to end."""
import numpy as np
import pytest

from instances_restatement import HAZARD_LUT, assert_stats_equal, remap_hist, restate_stats
from mesh_restatement import random_field

KI = (520.9, 521.0, 325.1, 249.7)
FIELD_DIMS = (11, 13, 37)  # crosses the 8-row, 4-plane and 32-plane tile boundaries; padded in y and z


def _field_params(flags):
    import semtsdf

    p = semtsdf.default_params(64, KI, 640, 480)
    start, voxel = (-0.3, 0.1, 0.5), (0.011, 0.012, 0.013)
    for a in range(3):
        p.dim[a] = FIELD_DIMS[a]
        p.vol_start[a], p.voxel[a] = start[a], voxel[a]
        p.vol_end[a] = start[a] + voxel[a] * (FIELD_DIMS[a] - 1)
    p.mu = 0.05
    p.flags = flags
    return p


def _field_volume(flags):
    import semtsdf

    f = random_field(FIELD_DIMS)
    vol = semtsdf.Volume(_field_params(flags), 0)
    color = f["color"] if flags & 4 else np.clip(f["color"], 0, 255).astype(np.uint8)
    vol.upload(sdf=f["sdf"], wt=f["wt"], color=color, hist=f["hist"] if flags & 1 else None)
    return vol, f


def _restate(vol, sdf_max, min_weight, layout=None, shard=0):
    """The restatement on what the volume itself holds (download()); for a shard the owned-plane
    set and the global z of its planes come from ShardLayout."""
    out = vol.download(hist=True)
    D = tuple(vol.local_dim)
    gz = owned = None
    if layout is not None:
        gz, owned = layout.local_to_global(shard), layout.owned_local(shard)
    return restate_stats(out["sdf"].reshape(D), out["wt"].reshape(D), out["color"].reshape(D + (3,)),
                         out["hist"].reshape(D + (32,)), sdf_max, min_weight, gz, owned)


def _params_like(p, **shard):
    import semtsdf

    q = semtsdf.default_params(64, KI, 640, 480)
    for fld in ("dim", "vol_start", "vol_end", "voxel", "K", "Kinv"):
        getattr(q, fld)[:] = getattr(p, fld)[:]
    q.mu, q.flags = p.mu, p.flags
    for k, v in shard.items():
        setattr(q, k, v)
    return q


def _fused(dims, nshards, frames_used=(1, 2, 3), parse=False):
    """Synthetic frames into a volume of `dims` placed from frame 0 (test_export's configuration),
    flags 0x3: the single volume and, for nshards > 1, its z_chunk = 8 shards.  parse: through
    parse_frame (association and relabel) instead of integrate.  Returns (single, shards, frames, p)."""
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream

    st = SyntheticStream(seed=0)
    frames = [st.frame(k) for k in range(max(frames_used) + 2)]
    p = semtsdf.default_params(64, KI, 640, 480)
    p.dim[0], p.dim[1], p.dim[2] = dims
    semtsdf.place_from_frame(p, frames[0].depth, float(np.mean(frames[0].depth[frames[0].depth > 0])) / 5000.0,
                             L.PLACE_SFM)
    p.flags = 0x3
    vols = [semtsdf.Volume(p, 0)]
    for sidx in range(nshards if nshards > 1 else 0):
        vols.append(semtsdf.Volume(_params_like(p, z_nshards=nshards, z_shard=sidx, z_chunk=8), 0))
    for k in frames_used:
        fr = frames[k]
        E = (fr.w2c @ frames[0].c2w).astype(np.float32)
        for v in vols:
            if parse:
                v.parse_frame(fr.depth, fr.rgb, np.ascontiguousarray(fr.mask).copy(), E)
            else:
                v.integrate(fr.depth, fr.rgb, np.ascontiguousarray(fr.mask), E)
    return vols[0], vols[1:], frames, p


def _raw_stats(lib, vol, sdf_max, min_weight, overlap):
    from semtsdf import _lib as L

    rec = np.full(32 * 96, 0xA5, np.uint8)
    ov = np.full(32 * 32, 0xA5A5A5A5A5A5A5A5, np.uint64) if overlap else None
    assert lib.semtsdf_instance_stats(vol.handle, sdf_max, min_weight, L.ptr(rec), L.ptr(ov)) == 0
    return rec.tobytes() + (ov.tobytes() if overlap else b"")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0x3, 0x5])
def test_stats_equal_the_restatement(flags):
    """The fixed random field in a semantic u8 volume and a COLOR_I32 volume (int32 colours
    outside [0, 255]: the clamp): every field equals the restatement at two selections, with and
    without the overlap table; the voxel counts agree with semtsdf_export_surface; two calls
    return the same bytes; the volume is not modified."""
    import semtsdf

    lib = semtsdf.load()
    vol, f = _field_volume(flags)
    if flags & 4:
        assert (f["color"] > 255).any() and (f["color"] < 0).any()
    before = vol.download(hist=True)
    for (sdf_max, mw), nsel in (((0.2, 1), 1027), ((0.5, 3), 1124)):
        want = _restate(vol, sdf_max, mw)
        assert int(want["selected"].sum()) == nsel
        got = vol.instance_stats(sdf_max, mw, overlap=True)
        print(flags, sdf_max, mw, "voxels", got["voxels"].tolist(), "support", got["support"].tolist())
        assert_stats_equal(got, want)
        assert got["overlap"].dtype == np.uint64 and got["voxels"].dtype == np.uint64
        assert np.array_equal(got["overlap"], got["overlap"].T)
        assert np.array_equal(np.diag(got["overlap"]), got["support"])
        bare = vol.instance_stats(sdf_max, mw, overlap=False)
        assert bare["overlap"] is None
        assert_stats_equal(bare, want, overlap=False)
        pts = semtsdf.export_surface(vol, sdf_max, mw)
        assert int(got["voxels"].sum()) == len(pts["label"]) == nsel
        assert np.array_equal(np.bincount(pts["label"], minlength=32), got["voxels"].astype(np.int64))
        for ov in (True, False):
            assert _raw_stats(lib, vol, sdf_max, mw, ov) == _raw_stats(lib, vol, sdf_max, mw, ov)
        k = int(np.argmax(got["voxels"]))
        p = vol.params
        want_c = np.array(list(p.vol_start), np.float64) + got["index_sum"][k] / float(got["voxels"][k]) * np.array(
            list(p.voxel), np.float64)
        assert np.array_equal(got["centroid"][k], want_c)
    after = vol.download(hist=True)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    vol.close()


@pytest.mark.gpu
def test_vote_volume_is_unsupported():
    import semtsdf
    from semtsdf import _lib as L

    lib = semtsdf.load()
    vol, _ = _field_volume(0xC)
    rec = np.zeros(32 * 96, np.uint8)
    assert lib.semtsdf_instance_stats(vol.handle, 0.2, 1, L.ptr(rec), None) == L.ERR_UNSUPPORTED
    ident = np.arange(32, dtype=np.uint8)
    assert lib.semtsdf_remap_instances(vol.handle, L.ptr(ident), -1, None) == L.ERR_UNSUPPORTED
    vol.close()


@pytest.mark.gpu
def test_remap_equals_the_restatement_in_place():
    """The fixed field through a table that merges (7 -> 3, 31 -> 4), dissolves (9 -> 0) and
    swaps (5 <-> 6: plane 5 is rewritten before plane 6 would read it): 1934 of the 5291 voxels
    change, the histogram equals remap_hist, the bin mask is rebuilt (the stats after the remap
    equal the restatement of the new arrays), everything else is untouched; an identity table
    and the refused calls change nothing."""
    import semtsdf
    from semtsdf import _lib as L

    lib = semtsdf.load()
    vol, f = _field_volume(0x3)
    vol.set_state(5, 32)
    before = vol.download(hist=True)
    ident = np.arange(32, dtype=np.uint8)

    def call(lut, num_objs):
        t = np.ascontiguousarray(lut, np.uint8)
        return lib.semtsdf_remap_instances(vol.handle, L.ptr(t), num_objs, None)

    bad0 = HAZARD_LUT.copy()
    bad0[0] = 1
    bad32 = HAZARD_LUT.copy()
    bad32[9] = 32
    # HAZARD_LUT keeps id 30, so the next id must be 31 or 32 (the current one)
    for lut, n in ((bad0, -1), (bad32, -1), (HAZARD_LUT, 33), (HAZARD_LUT, 30), (HAZARD_LUT, 5), (ident, 0), (ident, -2)):
        assert call(lut, n) == L.ERR_INVALID, (lut.tolist(), n)
    for lut, n in ((ident, -1), (ident, 32)):
        assert call(lut, n) == 0
    vol.sync()
    st = vol.state()
    assert (st.n_obs, st.num_objs) == (5, 32)
    same = vol.download(hist=True)
    for k in before:
        assert before[k].tobytes() == same[k].tobytes(), k

    vol.remap_instances(HAZARD_LUT, 31)
    after = vol.download(hist=True)
    want = remap_hist(before["hist"], HAZARD_LUT)
    changed = int((after["hist"].reshape(-1, 32) != before["hist"].reshape(-1, 32)).any(axis=1).sum())
    print("voxels changed by the remap:", changed)
    assert changed == 1934 and before["hist"].size == 5291 * 32
    assert np.array_equal(after["hist"], want)
    for k in ("sdf", "wt", "color"):
        assert before[k].tobytes() == after[k].tobytes(), k
    st = vol.state()
    assert (st.n_obs, st.num_objs) == (5, 31)
    for sdf_max, mw in ((0.2, 1), (0.5, 3)):
        got = vol.instance_stats(sdf_max, mw)
        assert_stats_equal(got, _restate(vol, sdf_max, mw))
        assert not got["support"][[7, 9, 31]].any() and got["support"][5] > 0 and got["support"][6] > 0
    # the bin mask serves the label render too: the export's labels follow the new histogram
    pts = semtsdf.export_surface(vol, 0.2, 1)
    assert np.array_equal(np.bincount(pts["label"], minlength=32), vol.instance_stats(0.2, 1)["voxels"].astype(np.int64))
    # -1 keeps the next id
    swap = ident.copy()
    swap[[1, 2]] = [2, 1]
    vol.remap_instances(swap)
    assert vol.state().num_objs == 31
    assert np.array_equal(vol.download(hist=True)["hist"], remap_hist(want, swap))
    vol.close()


@pytest.mark.gpu
def test_pipeline_continues_after_a_remap():
    """Frames 1-3 through parse_frame into the 48 x 40 x 64 volume; volume A merges its two
    largest ids and compacts in place, volume B is a fresh volume given A's state before the remap
    with the histogram remapped in NumPy.  Frame 4 through parse_frame leaves both identical:
    relabelled mask, the association's table, num_objs and the full downloads."""
    import semtsdf

    semtsdf.load()
    A, _, frames, p = _fused((48, 40, 64), 1, parse=True)
    st = A.instance_stats()
    cur = int(A.state().num_objs)
    a, b = sorted(int(k) for k in np.argsort(st["voxels"][1:])[-2:] + 1)
    assert st["voxels"][a] > 0 and st["voxels"][b] > 0 and b < cur <= 32
    lut = np.arange(32, dtype=np.uint8)
    lut[b] = a
    lut[b + 1:cur] = np.arange(b, cur - 1)  # compact: the ids above b move down by one
    pre = A.download(hist=True)
    n_obs = int(A.state().n_obs)
    A.remap_instances(lut, cur - 1)
    B = semtsdf.Volume(_params_like(p), 0)
    B.upload(sdf=pre["sdf"], wt=pre["wt"], color=pre["color"], hist=remap_hist(pre["hist"], lut))
    B.set_state(n_obs, cur - 1)
    fr = frames[4]
    E = (fr.w2c @ frames[0].c2w).astype(np.float32)
    res = []
    for v in (A, B):
        m = np.ascontiguousarray(fr.mask).copy()
        s = v.parse_frame(fr.depth, fr.rgb, m, E)
        res.append((m, bytes(s.lut), int(s.num_objs), int(v.state().num_objs), v.download(hist=True)))
    (ma, la, na, sa, da), (mb, lb, nb, sb, db) = res
    assert np.array_equal(ma, mb) and la == lb and (na, sa) == (nb, sb)
    assert na >= cur - 1  # the next id never falls; it restarted from the compacted count
    for k in da:
        assert da[k].tobytes() == db[k].tobytes(), k
    assert da["hist"].any()
    for v in (A, B):
        v.close()


@pytest.mark.gpu
def test_shards_add_up_to_the_single_volume():
    """48 x 40 x 70 in 2 shards of z_chunk 8 (the last chunk partial): each handle's stats equal
    the restatement on its owned planes and the shards' merged stats equal the single volume's in
    every field; after the same remap on all three handles each histogram equals remap_hist of
    its own download before (halo planes included) and the merged stats still agree."""
    import semtsdf
    from semtsdf.shard import ShardLayout

    semtsdf.load()
    single, shards, _, _ = _fused((48, 40, 70), 2)
    layout = ShardLayout(70, 2, 8)
    cur = int(single.state().num_objs)
    assert cur >= 4 and all(int(v.state().num_objs) == cur for v in shards)
    lut = np.arange(32, dtype=np.uint8)
    lut[[1, 2, 3]] = [2, 1, 1]  # 1 <-> 2 and 3 -> 1: plane 1 is a source and a destination
    for step in range(2):
        whole = single.instance_stats()
        parts = [v.instance_stats() for v in shards]
        assert int(whole["voxels"].sum()) > 1000 and all(int(q["voxels"].sum()) > 0 for q in parts)
        assert (whole["support"][1:3] > 0).all()  # the remapped ids are populated: the remap moves counts
        assert_stats_equal(whole, _restate(single, 0.2, 1))
        for s, (v, q) in enumerate(zip(shards, parts)):
            assert_stats_equal(q, _restate(v, 0.2, 1, layout, s))
        merged = semtsdf.merge_instance_stats(parts)
        assert_stats_equal(merged, whole)
        for k in ("centroid", "mean_rgb", "bbox_world_min", "bbox_world_max"):
            assert np.array_equal(merged[k], whole[k], equal_nan=True), k
        if step:
            break
        pre = [v.download(hist=True)["hist"] for v in [single] + shards]
        for v in [single] + shards:
            v.remap_instances(lut)
        for v, h in zip([single] + shards, pre):
            now = v.download(hist=True)["hist"]
            assert np.array_equal(now, remap_hist(h, lut))
            assert not np.array_equal(now, h)
    for v in shards + [single]:
        v.close()


@pytest.mark.gpu
def test_prune_instances_merges_a_deliberate_duplicate():
    """One object fused under two ids: frames 1-6 integrated with their ground-truth ids, the
    largest object's label rewritten to the fresh id 7 on the even frames.  prune_instances (the
    configuration's duplicate_thresh, 0.5) merges exactly that pair and the next id drops by one."""
    import semtsdf
    from semtsdf import TSDF
    from semtsdf.instances import find_duplicates
    from semtsdf.synth import SyntheticStream

    semtsdf.load()
    st = SyntheticStream(seed=0)
    f0 = st.frame(0)
    t = TSDF(KI, vol_dim=64)
    t.init_vars(f0.depth, f0.rgb, f0.w2c, float(np.mean(f0.depth[f0.depth > 0])) / 5000.0)
    frames = [st.frame(k) for k in range(1, 7)]
    counts = np.bincount(frames[0].gt_ids.reshape(-1), minlength=7)[1:7]
    dup = 1 + int(np.argmax(counts))
    for k, fr in enumerate(frames, start=1):
        m = np.ascontiguousarray(fr.gt_ids).copy()
        if k % 2 == 0:
            m[m == dup] = 7
        t.vol.integrate(fr.depth, fr.rgb, m, (fr.w2c @ f0.c2w).astype(np.float32))
    t.vol.set_state(int(t.vol.state().n_obs), 8)
    stats = t.instances()
    iou = stats["overlap"][dup, 7] / float(stats["support"][dup] + stats["support"][7] - stats["overlap"][dup, 7])
    print("duplicate pair", (dup, 7), "support IoU", iou, "voxels", stats["voxels"][:8].tolist())
    assert stats["support"][dup] > 0 and stats["support"][7] > 0
    assert find_duplicates(stats, t.config.duplicate_thresh) == [(dup, 7)]
    before = t.vol.download(hist=True)["hist"]
    lut, num = t.prune_instances()
    want = np.arange(32, dtype=np.uint8)
    want[7] = dup
    assert np.array_equal(lut, want) and num == 7 and t.num_objs == 7
    after = t.vol.download(hist=True)["hist"]
    assert np.array_equal(after, remap_hist(before, want))
    now = t.instances()
    # the merged support is the union of the two
    assert now["support"][7] == 0
    assert now["support"][dup] == stats["support"][dup] + stats["support"][7] - stats["overlap"][dup, 7]
    assert find_duplicates(now, t.config.duplicate_thresh) == []
    t.close()
