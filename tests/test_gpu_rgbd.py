"""RGB-D tracking on the device against the NumPy restatement of its rules (tests/rgbd_restatement.py):
the intensity pyramid as bits, the 64 words of the system (the first 32 against
semtsdf_icp_system_level_dev on the same buffers), and semtsdf.track.track_rgbd against the restated
loop on the textured wall."""
import ctypes as C

import numpy as np
import pytest

import icp_restatement as I
import model_maps_restatement as R
import rgbd_restatement as G
from rgbd_restatement import FIELD_GATES, field_inputs

pytestmark = pytest.mark.gpu


def assert_intensity_same(got, want):
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want)):
        assert (g["width"], g["height"]) == (w["width"], w["height"]), l
        for n in ("S", "valid"):
            assert g[n].dtype == w[n].dtype and g[n].shape == w[n].shape, (l, n)
            bad = g[n] != w[n]
            assert not bad.any(), (l, n, int(bad.sum()), np.argwhere(bad)[:3].tolist())


@pytest.fixture(scope="module")
def field():
    """The ragged 75 x 53 field volume; no test reads the volume itself."""
    import semtsdf

    semtsdf.load()
    vol = semtsdf.Volume(G.field_colour_case()[0], 0)
    yield vol
    vol.close()


@pytest.fixture(scope="module")
def wall():
    """The wall scene's volume on the device, integrated like the restatement's oracle state."""
    import semtsdf

    semtsdf.load()
    sc = G.wall_scene()
    vol = semtsdf.Volume(sc["p"], 0)
    for k in (1, 2):
        depth, rgb, ids = sc["frames"][k]
        vol.integrate(depth, rgb, ids, sc["E"][k])
    yield vol, sc
    vol.close()


class DeviceSystem:
    """The inputs of one level on the device; both system launches on the same buffers."""

    def __init__(self, vol, frame, model, f_int, m_int, level):
        import semtsdf

        self.vol, self.level = vol, level
        self.stream = C.c_void_p(vol.stream)
        self.dims = (frame["flags"].shape[1], frame["flags"].shape[0])
        arrs = {"vertex": frame["vertex"], "normal": frame["normal"], "flags": frame["flags"], "m_point": model["point"],
                "m_normal": model["normal"], "m_flags": model["flags"], "f_S": f_int["S"], "f_valid": f_int["valid"],
                "m_S": m_int["S"], "m_valid": m_int["valid"]}
        self.bufs = {k: semtsdf.DeviceBuffer(np.ascontiguousarray(a).nbytes) for k, a in arrs.items()}
        self.bufs["words"] = semtsdf.DeviceBuffer(8 * 64)
        for k, a in arrs.items():
            self.bufs[k].upload(np.ascontiguousarray(a), self.stream)
        vol.sync()
        self.maps = [self.bufs[k].ptr for k in ("vertex", "normal", "flags", "m_point", "m_normal", "m_flags")]
        self.photo = [self.bufs[k].ptr for k in ("f_S", "f_valid", "m_S", "m_valid")]

    def _read(self, n):
        words = np.zeros(n, np.int64)
        self.bufs["words"].download(words, self.stream)
        self.vol.sync()
        return words

    def rgbd(self, E_ref, E_cur, dist_max, cos_min, r_max, stride=1):
        self.vol.rgbd_system_level_dev(self.maps, self.photo, self.level, E_ref, E_cur, dist_max, cos_min, r_max, stride,
                                       self.bufs["words"].ptr)
        return self._read(64)

    def icp(self, E_ref, E_cur, dist_max, cos_min, stride=1):
        self.vol.icp_system_level_dev(self.maps, self.dims[0], self.dims[1], E_ref, E_cur, dist_max, cos_min, stride,
                                      self.bufs["words"].ptr)
        return self._read(32)

    def free(self):
        self.vol.sync()
        for b in self.bufs.values():
            b.free()


def test_ragged_intensity_pyramid_equals_the_restatement(field):
    """75 x 53 -> 37 x 26 -> 18 x 13 (-> 9 x 6): ragged tiles, odd at every halving, validity holes on a
    tile edge and in the last row and column; with and without a validity image."""
    _, _, _, m_rgb, f_rgb, f_valid, m_valid = G.field_colour_case()
    for rgb, valid in ((f_rgb, f_valid), (m_rgb, m_valid), (f_rgb, None)):
        want = G.restate_intensity_pyramid(rgb, valid, 3)
        assert [(w["width"], w["height"]) for w in want] == [(75, 53), (37, 26), (18, 13)]
        got = field.intensity_pyramid(rgb, valid, 3)
        assert_intensity_same(got, want)
        if valid is not None:
            for lv in got:
                assert set(np.unique(lv["valid"]).tolist()) == {0, 1}
    assert_intensity_same(field.intensity_pyramid(f_rgb, f_valid, 4), G.restate_intensity_pyramid(f_rgb, f_valid, 4))
    assert_intensity_same(field.intensity_pyramid(f_rgb, f_valid, 1), G.restate_intensity_pyramid(f_rgb, f_valid, 1))


def test_intensity_pyramid_of_the_wall(wall):
    """640 x 480, four levels: the frame's image without a validity image, the model's colour render
    with the model flags' validity; two calls give identical bytes and the scratch is kept."""
    vol, sc = wall
    rgb = sc["frames"][3][1]
    valid = G.model_valid(sc["model"])
    assert 0 < int(valid.sum()) < valid.size
    for img, v in ((rgb, None), (sc["m_rgb"], valid)):
        want = G.restate_intensity_pyramid(img, v, 4)
        got = vol.intensity_pyramid(img, v, 4)
        assert_intensity_same(got, want)
        again = vol.intensity_pyramid(img, v, 4)
        for a, b in zip(got, again):
            assert a["S"].tobytes() == b["S"].tobytes() and a["valid"].tobytes() == b["valid"].tobytes()
    assert_intensity_same(vol.intensity_pyramid(sc["m_rgb"], valid, 3), sc["m_int"])
    st = vol.state().device_bytes
    vol.intensity_pyramid(rgb, None, 4)
    assert vol.state().device_bytes == st


def test_device_form_agrees_with_the_host_form_on_a_second_stream(wall):
    import semtsdf
    from semtsdf import _lib as L

    vol, sc = wall
    lib = L.load()
    valid = G.model_valid(sc["model"])
    host = vol.intensity_pyramid(sc["m_rgb"], valid, 4)
    n = vol.W * vol.H
    stream = C.c_void_p()
    L.check(lib.semtsdf_stream_create(C.byref(stream)))
    bufs = {"rgb": semtsdf.DeviceBuffer(3 * n), "valid": semtsdf.DeviceBuffer(n)}
    for l, h in enumerate(host):
        bufs[f"S{l}"] = semtsdf.DeviceBuffer(4 * h["S"].size)
        bufs[f"V{l}"] = semtsdf.DeviceBuffer(h["S"].size)
    try:
        bufs["rgb"].upload(np.ascontiguousarray(sc["m_rgb"]), stream)
        bufs["valid"].upload(valid, stream)
        levels = [{"S": bufs[f"S{l}"].ptr, "valid": bufs[f"V{l}"].ptr} for l in range(4)]
        before = vol.state().device_bytes
        geo = vol.intensity_pyramid_dev(bufs["rgb"].ptr, bufs["valid"].ptr, levels, stream=stream)
        assert vol.state().device_bytes == before          # the device form allocates nothing
        for l, h in enumerate(host):
            assert (geo[l]["width"], geo[l]["height"]) == (h["width"], h["height"])
            S, V = np.empty_like(h["S"]), np.empty_like(h["valid"])
            bufs[f"S{l}"].download(S, stream)
            bufs[f"V{l}"].download(V, stream)
            L.check(lib.semtsdf_stream_sync(stream))
            assert S.tobytes() == h["S"].tobytes() and V.tobytes() == h["valid"].tobytes(), l
        # argument errors, each refused before any device work
        for kw in (dict(rgb=0), dict(levels=[]), dict(levels=levels + [levels[3]]), dict(levels=[dict(levels[0], S=0)]),
                   dict(levels=[levels[0], dict(levels[1], valid=0)])):
            args = dict(rgb=bufs["rgb"].ptr, levels=levels)
            args.update(kw)
            with pytest.raises(L.SemTSDFError) as e:
                vol.intensity_pyramid_dev(args["rgb"], None, args["levels"], stream=stream)
            assert e.value.code == L.ERR_INVALID, kw
    finally:
        L.check(lib.semtsdf_stream_sync(stream))
        for b in bufs.values():
            b.free()
        L.check(lib.semtsdf_stream_destroy(stream))


@pytest.mark.parametrize("level", [0, 1])
def test_ragged_system_words(field, level):
    """75 x 53 and 37 x 26, strides 1 and 2: 20, 6, 6 and 2 tiles, fewer than workgroups; every
    photometric class occurs."""
    p, frame, m, f_int, m_int = field_inputs(level)
    eye = np.eye(4, dtype=np.float32)
    E_cur = I.field_offset()
    dev = DeviceSystem(field, frame, m, f_int, m_int, level)
    try:
        for stride in (1, 2):
            want = G.restate_rgbd_system(frame, m, f_int, m_int, level, list(p.K), eye, E_cur, stride=stride, **FIELD_GATES)
            got = dev.rgbd(eye, E_cur, stride=stride, **FIELD_GATES)
            assert got[32:].tolist() == want[32:].tolist(), stride
            assert (got[60:] > 0).all()
            geo = dev.icp(eye, E_cur, FIELD_GATES["dist_max"], FIELD_GATES["cos_min"], stride)
            assert got[:32].tolist() == geo.tolist() == want[:32].tolist(), stride
            host = field.rgbd_system_level(frame, m, f_int, m_int, level, eye, E_cur, stride=stride, **FIELD_GATES)
            assert host.dtype == np.int64 and host.tolist() == got.tolist()
    finally:
        dev.free()


def test_wall_system_words(wall):
    """640 x 480, level 0, stride 1: 1200 tiles over at most 256 workgroups, several trips each; and the
    coarsest level of the schedule, 160 x 120."""
    vol, sc = wall
    K = list(sc["p"].K)
    for level, gates in ((0, dict(dist_max=0.1, cos_min=0.8, r_max=0.25)), (2, dict(dist_max=0.3, cos_min=0.6, r_max=0.05))):
        dev = DeviceSystem(vol, sc["pyramid"][level], sc["model"], sc["f_int"][level], sc["m_int"][level], level)
        try:
            for E_cur in (G.wall_guess(), sc["E_ref"]):
                want = G.restate_rgbd_system(sc["pyramid"][level], sc["model"], sc["f_int"][level], sc["m_int"][level],
                                             level, K, sc["E_ref"], E_cur, **gates)
                got = dev.rgbd(sc["E_ref"], E_cur, **gates)
                assert got[32:].tolist() == want[32:].tolist(), level
                geo = dev.icp(sc["E_ref"], E_cur, gates["dist_max"], gates["cos_min"])
                assert got[:32].tolist() == geo.tolist() == want[:32].tolist(), level
                assert got[28] > 10000 and got[60] > 10000
        finally:
            dev.free()


def test_track_rgbd_equals_the_restated_loop(wall):
    """Same words, same host solve: the extrinsic bit for bit and every log entry, from a guess 36 mm off
    in the plane, which point-to-plane ICP alone cannot correct; the volume's bytes are unchanged."""
    from semtsdf.track import pose_errors, track_rgbd

    vol, sc = wall
    before = vol.download(hist=True)
    E_want, log_want = G.restated_track_rgbd("wall")
    depth, rgb, _ = sc["frames"][3]
    E, log = track_rgbd(vol, depth, rgb, sc["E_ref"], G.wall_guess(), radius=0, band=G.BAND, eps=1e-5)
    assert len(log) == len(log_want)
    for a, b in zip(log, log_want):
        assert a == b, (a, b)
    assert E.dtype == np.float32 and E.tobytes() == E_want.tobytes()
    assert all(e["photo_used"] for e in log) and {e["level"] for e in log} == {0, 1, 2}
    assert pose_errors(E, sc["E_true"])[0] <= 0.005
    after = vol.download(hist=True)
    for n in before:
        assert before[n].tobytes() == after[n].tobytes(), n


def test_system_argument_errors(field):
    from semtsdf import _lib as L

    p, frame, m, f_int, m_int = field_inputs(0)
    eye = np.eye(4, dtype=np.float32)
    dev = DeviceSystem(field, frame, m, f_int, m_int, 0)
    try:
        nan = float("nan")
        bad = [dict(level=-1), dict(level=4), dict(r_max=0.0), dict(r_max=-0.1), dict(r_max=1.5), dict(r_max=nan),
               dict(stride=0), dict(dist_max=0.0), dict(dist_max=nan), dict(cos_min=nan), dict(cos_min=1.5), dict(words=0),
               dict(maps=dev.maps[:5] + [None]), dict(maps=[None] + dev.maps[1:])]
        bad += [dict(photo=dev.photo[:k] + [None] + dev.photo[k + 1:]) for k in range(4)]
        for kw in bad:
            args = dict(maps=dev.maps, photo=dev.photo, level=0, dist_max=0.1, cos_min=0.8, r_max=0.1, stride=1,
                        words=dev.bufs["words"].ptr)
            args.update(kw)
            with pytest.raises(L.SemTSDFError) as e:
                field.rgbd_system_level_dev(args["maps"], args["photo"], args["level"], eye, eye, args["dist_max"],
                                            args["cos_min"], args["r_max"], args["stride"], args["words"])
            assert e.value.code == L.ERR_INVALID, kw
        field.rgbd_system_level_dev(dev.maps, dev.photo, 0, eye, eye, 1.0, -1.0, 1.0, 1, dev.bufs["words"].ptr)  # the bounds
        field.sync()
    finally:
        dev.free()


def test_refusals_by_handle():
    """A level the image does not admit; skew; a Z-sharded handle: UNSUPPORTED from every call."""
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    eye = np.eye(4, dtype=np.float32)
    # 12 x 9: level 2 is 3 x 2, level 3 would be 1 x 1
    p = semtsdf.default_params(16, R.KI, 12, 9)
    for a in range(3):
        p.voxel[a] = 0.01
    p.mu = 0.05
    vol = semtsdf.Volume(p, 0)
    rgb = np.zeros((9, 12, 3), np.uint8)
    assert [(v["width"], v["height"]) for v in vol.intensity_pyramid(rgb, None, 3)] == [(12, 9), (6, 4), (3, 2)]
    for nl in (0, 4, 5):
        with pytest.raises(L.SemTSDFError) as e:
            vol.intensity_pyramid(rgb, None, nl)
        assert e.value.code == L.ERR_INVALID, nl
    with pytest.raises(L.SemTSDFError) as e:
        vol.rgbd_system_level_dev([0x1000] * 6, [0x1000] * 4, 3, eye, eye, 0.1, 0.8, 0.1, 1, 0x1000)
    assert e.value.code == L.ERR_INVALID
    vol.close()
    p.K[1] = 0.5                                        # skew: the level camera has none
    vol = semtsdf.Volume(p, 0)
    with pytest.raises(L.SemTSDFError) as e:
        vol.rgbd_system_level_dev([0x1000] * 6, [0x1000] * 4, 0, eye, eye, 0.1, 0.8, 0.1, 1, 0x1000)
    assert e.value.code == L.ERR_INVALID
    vol.close()
    H, W = R.FIELD_H, R.FIELD_W
    p = R.field_params(0x3)
    p.z_nshards, p.z_shard, p.z_chunk = 2, 0, 8
    vol = semtsdf.Volume(p, 0)
    maps = {"vertex": np.zeros((H, W, 3), np.float32), "flags": np.zeros((H, W), np.uint8)}
    maps["normal"] = maps["point"] = maps["vertex"]
    ints = {"S": np.zeros((H, W), np.uint32), "valid": np.zeros((H, W), np.uint8)}
    lv = [{"S": 0x1000, "valid": 0x1000}] * 3
    for call in (lambda: vol.intensity_pyramid(np.zeros((H, W, 3), np.uint8)),
                 lambda: vol.intensity_pyramid_dev(0x1000, None, lv),
                 lambda: vol.rgbd_system_level(maps, maps, ints, ints, 0, eye, eye),
                 lambda: vol.rgbd_system_level_dev([0x1000] * 6, [0x1000] * 4, 0, eye, eye, 0.1, 0.8, 0.1, 1, 0x1000)):
        with pytest.raises(L.SemTSDFError) as e:
            call()
        assert e.value.code == L.ERR_UNSUPPORTED
    vol.close()


def test_host_class_tracks_a_wall_with_rgb():
    """TSDF.track(depth, rgb=...) on the wall frames: from the last fused frame's pose (23 mm and 0.004 rad
    off, all of it in the plane) it ends nearer the frame's own pose, and parse_frame takes the result."""
    import semtsdf
    from semtsdf.track import pose_errors

    fr = [G.wall_frame(k) for k in range(4)]
    w2c = [np.linalg.inv(f[2]) for f in fr]
    ids = np.zeros((480, 640), np.uint8)
    t = semtsdf.TSDF(R.KI, 128)
    for k in range(3):
        t.parse_frame(fr[k][0], fr[k][1], w2c[k], G.WALL_Z, ids)
    W = t.track(fr[3][0], rgb=fr[3][1])
    assert W.shape == (4, 4) and W.dtype == np.float64
    t0, r0 = pose_errors(w2c[2], w2c[3])
    t1, r1 = pose_errors(W, w2c[3])
    assert t1 <= 0.25 * t0 and r1 <= 0.25 * r0, (t0, r0, t1, r1)
    assert all(e["photo_used"] for e in t.last_track) and t.last_track[-1]["photo_inliers"] > 100000
    n = t.n_obs
    t.parse_frame(fr[3][0], fr[3][1], W, G.WALL_Z, ids)
    assert t.n_obs == n + 1
    t.close()
