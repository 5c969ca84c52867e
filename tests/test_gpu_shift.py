"""semtsdf_shift on the device against its definition (tests/shift_restatement.py): after a
shift the handle is indistinguishable through the ABI from a twin created at the shifted
placement with the NumPy-shifted download of the old state uploaded into it -- downloads,
renders, maps, association decisions and tracked poses equal, floats as bits."""
import ctypes as C

import numpy as np
import pytest

import model_maps_restatement as R
import shift_restatement as S
from mesh_restatement import random_field

pytestmark = pytest.mark.gpu

DIMS = (24, 28, 72)  # y padded by 4, z by 24, three z-tiles
SHIFTS = [(8, 0, 0), (-8, 0, 0), (0, 8, 0), (0, -8, 0), (0, 0, 8), (0, 0, -32),
          (8, -16, 24), (0, 0, 40),  # these cross a tile
          (24, 0, 0)]                # = dim: everything is vacated
MAPS = ("t", "point", "normal", "label", "votes", "flags")


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_states_equal(got, want, what=""):
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        bad = g != w
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:3].tolist())


def params_bytes(p):
    return bytes(p)


def _field_params(flags):
    import semtsdf

    p = semtsdf.default_params(64, R.KI, 640, 480)
    start, voxel = (-0.3, 0.1, 0.5), (0.011, 0.012, 0.013)
    for a in range(3):
        p.dim[a] = DIMS[a]
        p.vol_start[a], p.voxel[a] = start[a], voxel[a]
        p.vol_end[a] = start[a] + voxel[a] * (DIMS[a] - 1)
    p.mu = 0.05
    p.flags = flags
    return p


def _field_state(form):
    f = random_field(DIMS)
    narrow = np.clip(f["color"], 0, 255)
    if form == "semantic":
        return 0x3, {"sdf": f["sdf"], "wt": f["wt"], "color": narrow.astype(np.uint8), "hist": f["hist"]}
    if form == "wide_colour":
        assert (f["color"] > 255).any()
        return 0x4, {"sdf": f["sdf"], "wt": f["wt"], "color": f["color"]}
    if form == "wide_weights":
        wt = f["wt"].copy()
        wt[5, 6, 7] = 70000
        return 0x3, {"sdf": f["sdf"], "wt": wt, "color": narrow.astype(np.uint8), "hist": f["hist"]}
    rng = np.random.default_rng(11)
    return 0x8 | 0x4, {"sdf": f["sdf"], "wt": f["wt"], "color": narrow.astype(np.int32),
                       "cls": rng.integers(0, 40, DIMS).astype(np.int32),
                       "cls_cnt": rng.integers(0, 9, DIMS).astype(np.int32)}


@pytest.mark.parametrize("form", ["semantic", "wide_colour", "wide_weights", "vote"])
def test_every_storage_form_on_ragged_dims(form):
    import semtsdf

    semtsdf.load()
    flags, state = _field_state(form)
    vol = semtsdf.Volume(_field_params(flags), 0)
    for shift in SHIFTS:
        vol.upload(**state)  # the same contents before every shift (the placement keeps moving)
        before = vol.get_params()
        want = S.numpy_shift(S.full_download(vol), shift, before.mu, dims=DIMS)
        vol.shift(*shift)
        assert_states_equal(S.full_download(vol), want, (form, shift))
        after = vol.get_params()
        start, end = S.shifted_placement(before, shift)
        for a in range(3):
            assert np.float32(after.vol_start[a]).view(np.uint32) == start[a].view(np.uint32), (shift, a)
            assert np.float32(after.vol_end[a]).view(np.uint32) == end[a].view(np.uint32), (shift, a)
        for name in ("dim", "voxel"):
            assert list(getattr(after, name)) == list(getattr(before, name))
        assert after.mu == before.mu and params_bytes(vol.params) == params_bytes(after)
        if shift == (24, 0, 0):  # nothing is left
            assert (want["wt"] == 0).all() and (bits(want["sdf"]) == np.float32(before.mu).view(np.uint32)).all()
        else:
            assert (want["wt"] != 0).any()
    # the spare is released and no array changed its size: the handle owns what it owned before
    vol.upload(**state)
    b1 = vol.state().device_bytes
    vol.shift(8, 8, -8)
    assert vol.state().device_bytes == b1
    vol.close()


def _fused_volume(sc):
    import semtsdf

    vol = semtsdf.Volume(sc["p"], 0)
    for k in range(1, 4):
        fr = sc["frames"][k]
        vol.integrate(fr.depth, fr.rgb, fr.gt_ids, sc["E"][k])
    return vol


def test_twin_equivalence_on_a_fused_scene():
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    sc = R.fused_scene()
    vol, plain = _fused_volume(sc), _fused_volume(sc)
    shift = (8, 0, -8)
    vol.shift(*shift)
    tw = S.twin(plain, shift, params=vol.get_params())
    plain.close()
    assert params_bytes(tw.get_params()) == params_bytes(vol.get_params())
    assert_states_equal(S.full_download(vol), S.full_download(tw), "after the shift")
    fr = sc["frames"][3]
    for v in (vol, tw):
        v.integrate(fr.depth, fr.rgb, fr.gt_ids, sc["E"][3])
    assert (vol.state().n_obs, vol.state().num_objs) == (tw.state().n_obs, tw.state().num_objs)
    p = vol.get_params()
    views = [semtsdf.pose_camera(list(p.Kinv), sc["E"][3]), semtsdf.orbit_camera(list(p.Kinv), 0.2, sc["dist"])]
    for s2w, c in views:
        a, b = vol.render_maps(s2w, c, 1, MAPS), tw.render_maps(s2w, c, 1, MAPS)
        assert_states_equal(a, b, "maps")
        assert int((a["flags"] & 1).sum()) >= 500  # the view shows the model: equality is not vacuous
        for mode in (L.RENDER_LABEL, L.RENDER_COLOR):
            (ia, ta), (ib, tb) = vol.raycast(s2w, c, mode, want_t=True), tw.raycast(s2w, c, mode, want_t=True)
            assert np.array_equal(ia, ib) and np.array_equal(bits(ta), bits(tb))
    assert np.array_equal(vol.map_words(), tw.map_words())
    assert_states_equal(S.full_download(vol), S.full_download(tw), "after the integrate")
    vol.close()
    tw.close()


def _stats_bytes(st):
    return None if st is None else bytes(st)


def test_sequence_with_the_policy():
    import semtsdf

    semtsdf.load()
    st = S.sequence_stream()
    frames = [st.frame(k) for k in range(S.SEQ_FRAMES)]
    focus = S.sequence_focus_depth(frames[0])
    K = S.sequence_intrinsics()
    follows, twinned, still = (semtsdf.TSDF(K, S.SEQ_DIM) for _ in range(3))
    shifts, touched = [], {}
    start0 = end0 = None
    for k, fr in enumerate(frames):
        last = k == S.SEQ_FRAMES - 1
        s = follows.follow(fr.w2c, focus_depth=focus, trigger_bricks=1)
        if s is not None:
            shifts.append(s)
            new = S.twin(twinned.vol, s, params=follows.vol.get_params())
            twinned.vol.close()
            twinned.vol = new
            assert_states_equal(S.full_download(follows.vol), S.full_download(new), ("shift at frame", k))
            assert np.array_equal(follows.vol.map_words(), new.map_words()), k
            assert np.array_equal(np.asarray(follows.vol_start, np.float32),
                                  np.array(list(new.get_params().vol_start), np.float32))
        masks = [np.ascontiguousarray(fr.mask.copy()) for _ in range(3)]
        decisions = []
        for name, t, m in zip(("follows", "twinned", "still"), (follows, twinned, still), masks):
            if last and t.vol is not None and name != "twinned":
                t.vol.set_instrumentation(events=False, count=True)
                t.vol.reset_timing()
            decisions.append(_stats_bytes(t.parse_frame(fr.depth, fr.rgb, fr.w2c, focus, m)))
            if last and name != "twinned":
                touched[name] = int(t.vol.timing().touched)
        if k == 0:
            p0 = follows.vol.get_params()
            start0, end0 = list(p0.vol_start), list(p0.vol_end)
        assert decisions[0] == decisions[1], ("association decision", k)
        assert np.array_equal(masks[0], masks[1]), ("relabelled mask", k)
    assert len(shifts) >= 2 and len({a for s in shifts for a in range(3) if s[a]}) >= 2, shifts
    assert_states_equal(S.full_download(follows.vol), S.full_download(twinned.vol), "end of the sequence")
    assert np.array_equal(follows.vol.map_words(), twinned.vol.map_words())
    assert (follows.n_obs, follows.num_objs) == (twinned.n_obs, twinned.num_objs)
    depth = frames[-1].depth
    Ea, Eb = follows.track(depth), twinned.track(depth)
    assert np.array_equal(Ea.view(np.uint64), Eb.view(np.uint64))
    # the walk left the cube placed around frame 0: without follow the last frame finds less to fuse into
    c2w = frames[-1].c2w
    f = c2w[:3, 3] + focus * c2w[:3, 2]
    assert any(not (start0[a] <= f[a] <= end0[a]) for a in range(3)), f
    assert touched["still"] < touched["follows"], touched
    for t in (follows, twinned, still):
        t.close()


def _point_rows(pts, offset=(0, 0, 0)):
    idx = pts["index"].astype(np.int64) + np.asarray(offset, np.int64)
    cols = [idx[:, 0], idx[:, 1], idx[:, 2], pts["sdf"].view(np.uint32).astype(np.int64),
            pts["rgb"][:, 0].astype(np.int64), pts["rgb"][:, 1].astype(np.int64), pts["rgb"][:, 2].astype(np.int64),
            pts["label"].astype(np.int64)]
    return {tuple(r) for r in np.stack(cols, axis=1).tolist()}


def test_nothing_leaves_silently():
    import semtsdf

    semtsdf.load()
    sc = R.fused_scene()
    vol = _fused_volume(sc)
    shift = (16, 0, 0)
    before = semtsdf.export_surface(vol, 0.2, 1)
    evicted = semtsdf.evicted_points(vol, shift, 0.2, 1)
    old_start = np.array(list(vol.params.vol_start), np.float64)
    voxel = np.array(list(vol.params.voxel), np.float64)
    assert np.array_equal(evicted["xyz"], (evicted["index"].astype(np.float64) * voxel + old_start).astype(np.float32))
    vol.shift(*shift)
    after = semtsdf.export_surface(vol, 0.2, 1)
    all_rows, out_rows, kept_rows = _point_rows(before), _point_rows(evicted), _point_rows(after, shift)
    assert len(out_rows) == len(evicted["sdf"]) > 0 and len(kept_rows) == len(after["sdf"]) > 0
    assert not (out_rows & kept_rows)
    assert out_rows | kept_rows == all_rows
    assert len(all_rows) == len(before["sdf"]) == len(out_rows) + len(kept_rows)
    vol.close()


def test_checkpoint_after_a_shift(tmp_path):
    import semtsdf

    semtsdf.load()
    sc = R.fused_scene()
    fr = sc["frames"]
    t = semtsdf.TSDF(R.KI, 64)
    for k in range(4):
        t.parse_frame(fr[k].depth, fr[k].rgb, fr[k].w2c, sc["dist"], np.ascontiguousarray(fr[k].gt_ids))
    seen = []
    c2w = fr[3].c2w.copy()
    c2w[:3, 3] += (0.7, 0.0, -0.5)
    s = t.follow(np.linalg.inv(c2w), trigger_bricks=1, on_evict=seen.append)
    assert s is not None and s[0] > 0 and s[2] < 0, s
    assert len(seen) == 1 and len(seen[0]["sdf"]) > 0
    assert np.array_equal(np.asarray(t.vol_start, np.float32), np.array(list(t.vol.get_params().vol_start), np.float32))
    path = str(tmp_path / "shifted.npz")
    t.save(path)
    u = semtsdf.TSDF.load(path)
    assert params_bytes(u.vol.get_params()) == params_bytes(t.vol.get_params())
    assert np.array_equal(np.asarray(u.vol_start, np.float64), np.asarray(t.vol_start, np.float64))
    assert np.array_equal(np.asarray(u.vol_end, np.float64), np.asarray(t.vol_end, np.float64))
    assert_states_equal(S.full_download(u.vol), S.full_download(t.vol), "reloaded")
    assert (u.n_obs, u.num_objs) == (t.n_obs, t.num_objs)
    t.close()
    u.close()


def test_errors_and_the_zero_shift():
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    sc = R.fused_scene()
    vol = _fused_volume(sc)
    state, params, words = S.full_download(vol), params_bytes(vol.get_params()), vol.map_words()
    for bad in ((4, 0, 0), (8, 8, -3), (1 << 20, 0, 0)):
        with pytest.raises(semtsdf.SemTSDFError) as e:
            vol.shift(*bad)
        assert e.value.code == L.ERR_INVALID, bad
        assert params_bytes(vol.get_params()) == params
        assert_states_equal(S.full_download(vol), state, ("untouched", bad))
    # the zero shift does nothing: the maps are not even marked for a rebuild
    vol.shift(0, 0, 0)
    assert params_bytes(vol.get_params()) == params
    assert np.array_equal(vol.map_words(), words)
    assert_states_equal(S.full_download(vol), state, "zero shift")
    vol.close()
    # a Z-sharded handle is refused
    q = semtsdf.default_params(64, R.KI, 640, 480)
    for fld in ("dim", "vol_start", "vol_end", "voxel", "K", "Kinv"):
        getattr(q, fld)[:] = getattr(sc["p"], fld)[:]
    q.mu, q.flags = sc["p"].mu, sc["p"].flags
    q.z_nshards, q.z_shard, q.z_chunk = 2, 0, 8
    shard = semtsdf.Volume(q, 0)
    with pytest.raises(semtsdf.SemTSDFError) as e:
        shard.shift(8, 0, 0)
    assert e.value.code == L.ERR_STATE
    shard.close()
