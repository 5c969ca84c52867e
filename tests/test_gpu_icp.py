"""Camera tracking on the device against the NumPy restatement of its rules (tests/icp_restatement.py):
the frame maps as bits, the 32 system words, and semtsdf.track.track against the restated loop."""
import ctypes as C

import numpy as np
import pytest

import icp_restatement as I
import model_maps_restatement as R

pytestmark = pytest.mark.gpu

FRAME_NAMES = ("vertex", "normal", "flags")


def assert_same(got, want, names):
    for n in names:
        g, w = got[n], want[n]
        assert g.shape == w.shape and g.dtype == w.dtype, n
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = g != w
        assert not bad.any(), (n, int(bad.sum()), np.argwhere(bad)[:3].tolist())


@pytest.fixture(scope="module")
def tracked():
    """The tracking scene's volume on the device, integrated like the restatement's oracle state."""
    import semtsdf

    semtsdf.load()
    sc = I.tracking_scene()
    vol = semtsdf.Volume(sc["p"], 0)
    for k in (1, 2):
        fr = sc["frames"][k]
        vol.integrate(fr.depth, fr.rgb, fr.gt_ids, sc["E"][k])
    yield vol, sc
    vol.close()


@pytest.fixture(scope="module")
def field():
    """The ragged 75 x 53 field volume; no test reads the volume itself."""
    import semtsdf

    semtsdf.load()
    p, _, _, depth = I.field_case()
    vol = semtsdf.Volume(p, 0)
    yield vol, p, depth
    vol.close()


def _subsets_equal(vol, depth, full):
    for n in FRAME_NAMES:
        part = vol.frame_maps(depth, want=(n,))
        assert sorted(part) == [n] and part[n].tobytes() == full[n].tobytes(), n


def test_frame_maps_of_the_tracking_frame(tracked):
    vol, sc = tracked
    depth = sc["frames"][3].depth
    got = vol.frame_maps(depth)
    assert_same(got, sc["frame"], FRAME_NAMES)
    _subsets_equal(vol, depth, got)


def test_frame_maps_of_the_ragged_image(field):
    """75 x 53 (tile edges in x and y, cy < 0) with zero-depth holes on a tile edge and in the last row
    and column."""
    vol, p, depth = field
    got = vol.frame_maps(depth)
    want = I.restate_frame_maps(depth, list(p.Kinv), p.depth_scale)
    assert_same(got, want, FRAME_NAMES)
    assert set(np.unique(got["flags"]).tolist()) == {0, 1, 3}
    _subsets_equal(vol, depth, got)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("min_weight", [1, 0])
def test_field_system_words(field, min_weight, stride):
    """The field view's own depth against its model maps, E_cur a small offset from E_ref = identity.  At
    min_weight 1 only 4 model pixels carry a normal, so nearly every pixel is in class none and no
    offset reaches all classes (test_icp.py); at min_weight 0 each of the four classes occurs."""
    vol, p, depth = field
    model = R.field_view(0x3, min_weight)[4]
    frame = vol.frame_maps(depth)
    eye = np.eye(4, dtype=np.float32)
    want = I.restate_system(frame, model, list(p.K), eye, I.field_offset(), stride=stride, **I.FIELD_GATES)
    got = vol.icp_system(frame, model, eye, I.field_offset(), stride=stride, **I.FIELD_GATES)
    assert got.dtype == np.int64 and got.tolist() == want.tolist()
    assert int(got[28:].sum()) == int(((frame["flags"][::stride, ::stride] & 3) == 3).sum())
    if min_weight == 0:
        assert (got[28:] > 0).all(), got[28:]


def test_tracking_scene_system_words(tracked):
    """At E0 and at the restated loop's final pose; two calls agree; the volume is unchanged."""
    vol, sc = tracked
    before = vol.download(hist=True)
    E_end, _ = I.restated_track()
    for E_cur in (sc["E_ref"], E_end):
        want = I.scene_system(E_cur)
        got = vol.icp_system(sc["frame"], sc["model"], sc["E_ref"], E_cur, **I.TRACK_GATES)
        assert got.tolist() == want.tolist()
        again = vol.icp_system(sc["frame"], sc["model"], sc["E_ref"], E_cur, **I.TRACK_GATES)
        assert again.tobytes() == got.tobytes()
        assert got[28] > 200000
    after = vol.download(hist=True)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k


def test_range_gate(tracked):
    """An E_cur whose origin is 400 m away along x puts every |Pw| beyond 32 m: no inliers, every
    visited pixel in word 31, no error (against the model where it is, the projection already refuses
    the pixels).  With the reference view and the model moved along and the other gates opened as far
    as the call allows, the projection and the gates see what they see without the move, and the
    range gate alone takes the rows away: all but those whose normal lies along x within 32 / 400
    (68 pixels on the restatement), which stay in range by the rule."""
    vol, sc = tracked
    move = np.array([400.0, 0.0, 0.0], np.float32)
    E_far = sc["E_ref"].copy()
    E_far[:3, 3] -= E_far[:3, :3] @ move  # the camera centre moved by `move`
    vis = int(((sc["frame"]["flags"] & 3) == 3).sum())
    got = vol.icp_system(sc["frame"], sc["model"], sc["E_ref"], E_far, **I.TRACK_GATES)
    assert got[:31].tolist() == [0] * 31 and int(got[31]) == vis
    model = {k: sc["model"][k].copy() for k in ("point", "normal", "flags")}
    model["point"][(model["flags"] & 1) != 0] += move
    want = I.restate_system(sc["frame"], model, list(sc["p"].K), E_far, E_far, 1.0, -1.0, 1)
    got = vol.icp_system(sc["frame"], model, E_far, E_far, 1.0, -1.0, 1)
    assert got.tolist() == want.tolist()
    near = vol.icp_system(sc["frame"], sc["model"], sc["E_ref"], sc["E_ref"], 1.0, -1.0, 1)
    assert near[28] > 0.7 * vis and got[28] < near[28] // 1000
    assert got[29] == near[29] and got[30] == near[30] == 0
    assert got[31] == near[31] + near[28] - got[28]


def test_track_equals_the_restated_loop(tracked):
    """Same words, same host solve: the extrinsic bit for bit and the same counts per iteration."""
    from semtsdf.track import pose_errors, track

    vol, sc = tracked
    E_want, log_want = I.restated_track()
    E, log = track(vol, sc["frames"][3].depth, sc["E_ref"], sc["E_ref"], iters=10, eps=0.0, **I.TRACK_GATES)
    assert E.dtype == np.float32 and E.tobytes() == E_want.tobytes()
    assert len(log) == len(log_want) == 10
    for a, b in zip(log, log_want):
        assert a == b, (a, b)
    t0, r0 = pose_errors(sc["E_ref"], sc["E_true"])
    t1, r1 = pose_errors(E, sc["E_true"])
    assert t1 <= 0.25 * t0 and r1 <= 0.25 * r0


def test_tracking_lost_keeps_the_estimate(tracked):
    from semtsdf.track import TrackingLost, track

    vol, sc = tracked
    with pytest.raises(TrackingLost) as e:
        track(vol, sc["frames"][3].depth, sc["E_ref"], sc["E_ref"], iters=3, min_inliers=400000)
    assert np.array_equal(e.value.E, sc["E_ref"]) and len(e.value.log) == 1


def test_device_pointer_variants_on_a_second_stream(tracked):
    import semtsdf
    from semtsdf import _lib as L

    vol, sc = tracked
    lib = L.load()
    n = vol.W * vol.H
    depth = np.ascontiguousarray(sc["frames"][3].depth)
    want_words = I.scene_system(sc["E_ref"])
    stream = C.c_void_p()
    L.check(lib.semtsdf_stream_create(C.byref(stream)))
    sizes = {"depth": 2 * n, "vertex": 12 * n, "normal": 12 * n, "flags": n, "m_point": 12 * n, "m_normal": 12 * n,
             "m_flags": n, "words": 256}
    bufs = {k: semtsdf.DeviceBuffer(s) for k, s in sizes.items()}
    try:
        bufs["depth"].upload(depth, stream)
        for k, src in (("m_point", "point"), ("m_normal", "normal"), ("m_flags", "flags")):
            bufs[k].upload(sc["model"][src], stream)
        vol.frame_maps_dev(bufs["depth"].ptr, bufs["vertex"].ptr, bufs["normal"].ptr, bufs["flags"].ptr, stream=stream)
        ptrs = [bufs[k].ptr for k in ("vertex", "normal", "flags", "m_point", "m_normal", "m_flags")]
        vol.icp_system_dev(ptrs, sc["E_ref"], sc["E_ref"], 0.1, 0.8, 1, bufs["words"].ptr, stream=stream)
        for k in FRAME_NAMES:
            out = np.empty_like(sc["frame"][k])
            bufs[k].download(out, stream)
            L.check(lib.semtsdf_stream_sync(stream))
            assert out.tobytes() == sc["frame"][k].tobytes(), k
        words = np.zeros(32, np.int64)
        bufs["words"].download(words, stream)
        L.check(lib.semtsdf_stream_sync(stream))
        assert words.tolist() == want_words.tolist()
        # invalid arguments, each refused before any device work
        eye = np.eye(4, dtype=np.float32)
        for kw in (dict(stride=0), dict(stride=-2), dict(dist_max=0.0), dict(dist_max=1.5), dict(dist_max=float("nan")),
                   dict(cos_min=1.25), dict(cos_min=-1.5), dict(cos_min=float("nan"))):
            args = dict(dist_max=0.1, cos_min=0.8, stride=1)
            args.update(kw)
            with pytest.raises(L.SemTSDFError) as e:
                vol.icp_system_dev(ptrs, eye, eye, args["dist_max"], args["cos_min"], args["stride"],
                                   bufs["words"].ptr, stream=stream)
            assert e.value.code == L.ERR_INVALID, kw
        with pytest.raises(L.SemTSDFError) as e:
            vol.icp_system_dev(ptrs[:5] + [None], eye, eye, 0.1, 0.8, 1, bufs["words"].ptr, stream=stream)
        assert e.value.code == L.ERR_INVALID
        with pytest.raises(L.SemTSDFError) as e:
            vol.frame_maps_dev(bufs["depth"].ptr, stream=stream)
        assert e.value.code == L.ERR_INVALID
    finally:
        L.check(lib.semtsdf_stream_sync(stream))
        for b in bufs.values():
            b.free()
        L.check(lib.semtsdf_stream_destroy(stream))


def test_refusals_by_handle():
    """A Z-sharded handle: UNSUPPORTED from all four calls; an image of more than 2^19 pixels: INVALID
    from the system (the frame maps have no such bound)."""
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    p = R.field_params(0x3)
    p.z_nshards, p.z_shard, p.z_chunk = 2, 0, 8
    vol = semtsdf.Volume(p, 0)
    depth = np.ones((R.FIELD_H, R.FIELD_W), np.uint16)
    maps = {"vertex": np.zeros((R.FIELD_H, R.FIELD_W, 3), np.float32), "flags": np.zeros((R.FIELD_H, R.FIELD_W), np.uint8)}
    maps["normal"] = maps["point"] = maps["vertex"]
    eye = np.eye(4, dtype=np.float32)
    for call in (lambda: vol.frame_maps(depth), lambda: vol.frame_maps_dev(0x1000, 0x1000),
                 lambda: vol.icp_system(maps, maps, eye, eye),
                 lambda: vol.icp_system_dev([0x1000] * 6, eye, eye, 0.1, 0.8, 1, 0x1000)):
        with pytest.raises(L.SemTSDFError) as e:
            call()
        assert e.value.code == L.ERR_UNSUPPORTED
    vol.close()
    p = semtsdf.default_params(16, R.KI, 1024, 513)
    for a in range(3):
        p.voxel[a] = 0.01
    p.mu = 0.05
    vol = semtsdf.Volume(p, 0)
    with pytest.raises(L.SemTSDFError) as e:
        vol.icp_system_dev([0x1000] * 6, eye, eye, 0.1, 0.8, 1, 0x1000)
    assert e.value.code == L.ERR_INVALID
    vol.close()


def test_host_class_tracks_and_fuses():
    """TSDF.track on a default SyntheticStream: errors against the frame's own pose no larger than the
    guess's (the last fused frame's pose), and parse_frame takes the tracked extrinsic."""
    import semtsdf
    from semtsdf.synth import SyntheticStream
    from semtsdf.track import pose_errors

    st = SyntheticStream(seed=0)
    fr = [st.frame(k) for k in range(4)]
    dist = float(np.mean(fr[0].depth[fr[0].depth > 0])) / 5000.0
    t = semtsdf.TSDF(R.KI, 128)
    with pytest.raises(ValueError):
        t.track(fr[0].depth)
    for k in range(3):
        t.parse_frame(fr[k].depth, fr[k].rgb, fr[k].w2c, dist, np.ascontiguousarray(fr[k].gt_ids))
    W = t.track(fr[3].depth)
    assert W.shape == (4, 4) and W.dtype == np.float64
    t0, r0 = pose_errors(fr[2].w2c, fr[3].w2c)
    t1, r1 = pose_errors(W, fr[3].w2c)
    assert t1 <= t0 and r1 <= r0, (t0, r0, t1, r1)
    assert len(t.last_track) >= 1 and t.last_track[-1]["inliers"] > 100000
    W2 = t.track(fr[3].depth, guess=fr[2].w2c)
    assert np.array_equal(W, W2)
    n = t.n_obs
    t.parse_frame(fr[3].depth, fr[3].rgb, W, dist, np.ascontiguousarray(fr[3].gt_ids))
    assert t.n_obs == n + 1
    t.close()
