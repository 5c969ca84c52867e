"""The depth pyramid on the device against the NumPy restatement of its rules
(tests/pyramid_restatement.py): every level's z and maps as bits, the system of a level as words, and
semtsdf.track.track_pyramid against the restated coarse-to-fine loop."""
import ctypes as C

import numpy as np
import pytest

import icp_restatement as I
import model_maps_restatement as R
import pyramid_restatement as P

pytestmark = pytest.mark.gpu

LEVEL_NAMES = ("z", "vertex", "normal", "flags")
RAGGED = dict(sigma_r=0.02, band=0.02)   # on the ragged depth both sides of the range term and of the band occur


def assert_levels_same(got, want, names=LEVEL_NAMES):
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want)):
        assert (g["width"], g["height"]) == (w["width"], w["height"]), l
        assert g["Kinv"].dtype == np.float32 and g["Kinv"].tobytes() == w["Kinv"].tobytes(), l
        for n in names:
            a, b = g[n], w[n]
            assert a.shape == b.shape and a.dtype == b.dtype, (l, n)
            if a.dtype == np.float32:
                a, b = a.view(np.uint32), b.view(np.uint32)
            bad = a != b
            assert not bad.any(), (l, n, int(bad.sum()), np.argwhere(bad)[:3].tolist())


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


@pytest.mark.parametrize("radius", [0, 1, 3, 4])
def test_ragged_pyramid_equals_the_restatement(field, radius):
    """75 x 53 -> 37 x 26 -> 18 x 13: odd at every halving, tile edges in x and y, holes on a tile edge and
    in the last row and column."""
    vol, p, depth = field
    st = {}
    want = P.restate_pyramid(depth, list(p.K), list(p.Kinv), p.depth_scale, 3, radius, stats=st, **RAGGED)
    assert [(w["width"], w["height"]) for w in want] == [(75, 53), (37, 26), (18, 13)]
    if radius:
        assert st["filter"]["accepted"] > 0 and st["filter"]["rejected"] > 0, st
    for h in st["halve"]:
        assert h["inside"] > 0 and h["outside"] > 0, st
    got = vol.frame_pyramid(depth, 3, radius, **RAGGED)
    assert_levels_same(got, want)
    for lv in got:
        assert set(np.unique(lv["flags"]).tolist()) == {0, 1, 3}
    assert np.array_equal(got[0]["z"] == 0, depth == 0)
    assert vol.frame_levels(3)[2]["Kinv"].tobytes() == want[2]["Kinv"].tobytes()


def test_unfiltered_level_0_is_the_frame_maps(field, tracked):
    for vol, depth in ((field[0], field[2]), (tracked[0], tracked[1]["frames"][3].depth)):
        fm = vol.frame_maps(depth)
        lv = vol.frame_pyramid(depth, 1, 0, band=0.05)[0]
        for n in ("vertex", "normal", "flags"):
            assert lv[n].tobytes() == fm[n].tobytes(), n
        assert lv["z"].tobytes() == fm["vertex"][..., 2].tobytes()  # Kinv's last row is (0, 0, 1)


def test_pyramid_of_the_tracking_frame(tracked):
    """640 x 480, three levels, radius 3: every output as the restatement has it; outputs requested alone
    equal those of the full call; two calls give identical bytes."""
    vol, sc = tracked
    depth = sc["frames"][3].depth
    want = P.scene_pyramid(radius=3, sigma_r=0.05, band=0.15)
    got = vol.frame_pyramid(depth)       # the defaults: 3 levels, radius 3, sigma_r 0.05, band 3 sigma_r
    assert_levels_same(got, want)
    again = vol.frame_pyramid(depth, 3, 3, 0.05, 0.15)
    for a, b in zip(got, again):
        for n in LEVEL_NAMES:
            assert a[n].tobytes() == b[n].tobytes(), n
    for n in ("vertex", "normal", "flags"):
        part = vol.frame_pyramid(depth, want=(n,))
        for a, b in zip(part, got):
            assert sorted(a) == sorted(["width", "height", "Kinv", "z", n])
            assert a[n].tobytes() == b[n].tobytes() and a["z"].tobytes() == b["z"].tobytes(), n
    bare = vol.frame_pyramid(depth, want=())
    assert [a["z"].tobytes() for a in bare] == [b["z"].tobytes() for b in got]
    st = vol.state().device_bytes
    vol.frame_pyramid(depth)
    assert vol.state().device_bytes == st     # the host variant's scratch is kept, not taken again


def test_level_system_with_the_handles_grid_is_icp_system(tracked):
    vol, sc = tracked
    for E_cur in (sc["E_ref"], P.basin_guess(6)):
        a = vol.icp_system(sc["frame"], sc["model"], sc["E_ref"], E_cur, **I.TRACK_GATES)
        b = vol.icp_system_level(sc["frame"], sc["model"], sc["E_ref"], E_cur, **I.TRACK_GATES)
        assert a.tolist() == b.tolist() and a[28] > 0


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("level", [1, 2])
def test_level_system_words(tracked, level, stride):
    vol, sc = tracked
    lv = P.scene_pyramid()[level]
    gates = dict(dist_max=0.2, cos_min=0.7)
    for E_cur in (sc["E_ref"], P.basin_guess(6)):
        want = P.restate_system_level(lv, sc["model"], list(sc["p"].K), sc["E_ref"], E_cur, stride=stride, **gates)
        got = vol.icp_system_level(lv, sc["model"], sc["E_ref"], E_cur, stride=stride, **gates)
        assert got.dtype == np.int64 and got.tolist() == want.tolist()
        assert int(got[28:].sum()) == int(((lv["flags"][::stride, ::stride] & 3) == 3).sum())
        if E_cur is sc["E_ref"]:
            assert (want[28:] > 0).all(), want[28:]   # every class occurs on the coarse grids too


@pytest.mark.parametrize("k", [None, 11])
def test_track_pyramid_equals_the_restated_loop(tracked, k):
    """Same words, same host solve: the extrinsic bit for bit and every log entry, from E_ref and from a
    guess 270 mm off that full-resolution ICP loses; the volume's bytes are unchanged."""
    from semtsdf.track import pose_errors, track_pyramid

    vol, sc = tracked
    before = vol.download(hist=True)
    E_want, log_want = P.restated_track_pyramid(k)
    E0 = sc["E_ref"] if k is None else P.basin_guess(k)
    E, log = track_pyramid(vol, sc["frames"][3].depth, sc["E_ref"], E0, radius=0, band=P.SCENE_BAND, eps=1e-5)
    assert E.dtype == np.float32 and E.tobytes() == E_want.tobytes()
    assert len(log) == len(log_want)
    for a, b in zip(log, log_want):
        assert a == b, (a, b)
    assert {e["level"] for e in log} == {0, 1, 2}
    t, r = pose_errors(E, sc["E_true"])
    assert t <= 0.005 and r <= 0.002
    after = vol.download(hist=True)
    for n in before:
        assert before[n].tobytes() == after[n].tobytes(), n


def test_tracking_lost_carries_the_estimate(tracked):
    from semtsdf.track import TrackingLost, track_pyramid

    vol, sc = tracked
    with pytest.raises(TrackingLost) as e:
        track_pyramid(vol, sc["frames"][3].depth, sc["E_ref"], sc["E_ref"], radius=0, band=0.05, min_inliers=400000)
    assert np.array_equal(e.value.E, sc["E_ref"]) and [x["level"] for x in e.value.log] == [2]
    with pytest.raises(ValueError):
        vol.frame_pyramid(sc["frames"][3].depth, 3, 0)     # radius 0 has no sigma_r to derive the band from


def test_device_pointer_variants_on_a_second_stream(tracked):
    import semtsdf
    from semtsdf import _lib as L

    vol, sc = tracked
    lib = L.load()
    depth = np.ascontiguousarray(sc["frames"][3].depth)
    want = P.scene_pyramid(radius=3, sigma_r=0.05, band=0.15)
    n = vol.W * vol.H
    stream = C.c_void_p()
    L.check(lib.semtsdf_stream_create(C.byref(stream)))
    sizes = {"depth": 2 * n, "m_point": 12 * n, "m_normal": 12 * n, "m_flags": n, "words": 256}
    per = {"z": 4, "vertex": 12, "normal": 12, "flags": 1}
    for l, w in enumerate(want):
        sizes.update({f"{k}{l}": b * w["width"] * w["height"] for k, b in per.items()})
    bufs = {k: semtsdf.DeviceBuffer(s) for k, s in sizes.items()}
    try:
        bufs["depth"].upload(depth, stream)
        for k, src in (("m_point", "point"), ("m_normal", "normal"), ("m_flags", "flags")):
            bufs[k].upload(sc["model"][src], stream)
        levels = [{k: bufs[f"{k}{l}"].ptr for k in per} for l in range(3)]
        before = vol.state().device_bytes
        geo = vol.frame_pyramid_dev(bufs["depth"].ptr, levels, 3, 0.05, 0.15, stream=stream)
        assert vol.state().device_bytes == before          # the device variant allocates nothing
        for l, w in enumerate(want):
            assert (geo[l]["width"], geo[l]["height"]) == (w["width"], w["height"])
            assert geo[l]["Kinv"].tobytes() == w["Kinv"].tobytes()
            for k in per:
                out = np.empty_like(w[k])
                bufs[f"{k}{l}"].download(out, stream)
                L.check(lib.semtsdf_stream_sync(stream))
                assert out.tobytes() == w[k].tobytes(), (l, k)
        model = [bufs[k].ptr for k in ("m_point", "m_normal", "m_flags")]
        for l in (2, 1, 0):
            frame = [bufs[f"{k}{l}"].ptr for k in ("vertex", "normal", "flags")]
            vol.icp_system_level_dev(frame + model, want[l]["width"], want[l]["height"], sc["E_ref"], sc["E_ref"], 0.2,
                                     0.7, 1, bufs["words"].ptr, stream=stream)
            words = np.zeros(32, np.int64)
            bufs["words"].download(words, stream)
            L.check(lib.semtsdf_stream_sync(stream))
            ref = P.restate_system_level(want[l], sc["model"], list(sc["p"].K), sc["E_ref"], sc["E_ref"], 0.2, 0.7, 1)
            assert words.tolist() == ref.tolist(), l
        # argument errors, each refused before any device work
        eye = np.eye(4, dtype=np.float32)
        dptr = bufs["depth"].ptr
        nan, inf = float("nan"), float("inf")
        bad = [dict(levels=[]), dict(levels=levels + [levels[2]] * 2), dict(radius=-1), dict(radius=5),
               dict(sigma_r=0.0), dict(sigma_r=-0.05), dict(sigma_r=nan), dict(sigma_r=inf),
               dict(band=0.0), dict(band=-0.1), dict(band=nan), dict(band=inf), dict(depth=0),
               dict(levels=[levels[0], dict(levels[1], z=0), levels[2]])]
        for kw in bad:
            args = dict(depth=dptr, levels=levels, radius=3, sigma_r=0.05, band=0.15)
            args.update(kw)
            with pytest.raises(L.SemTSDFError) as e:
                vol.frame_pyramid_dev(args["depth"], args["levels"], args["radius"], args["sigma_r"], args["band"],
                                      stream=stream)
            assert e.value.code == L.ERR_INVALID, kw
        # what a radius of 0 or a single level does not read is not checked
        vol.frame_pyramid_dev(dptr, levels, 0, nan, 0.15, stream=stream)
        vol.frame_pyramid_dev(dptr, levels[:1], 3, 0.05, nan, stream=stream)
        frame = [bufs[f"{k}0"].ptr for k in ("vertex", "normal", "flags")]
        for kw in (dict(fw=0), dict(fh=-1), dict(fw=1024, fh=513), dict(stride=0), dict(dist_max=0.0),
                   dict(cos_min=float("nan")), dict(words=0), dict(ptrs=frame + model[:2] + [None])):
            args = dict(ptrs=frame + model, fw=640, fh=480, dist_max=0.1, cos_min=0.8, stride=1, words=bufs["words"].ptr)
            args.update(kw)
            with pytest.raises(L.SemTSDFError) as e:
                vol.icp_system_level_dev(args["ptrs"], args["fw"], args["fh"], eye, eye, args["dist_max"],
                                         args["cos_min"], args["stride"], args["words"], stream=stream)
            assert e.value.code == L.ERR_INVALID, kw
    finally:
        L.check(lib.semtsdf_stream_sync(stream))
        for b in bufs.values():
            b.free()
        L.check(lib.semtsdf_stream_destroy(stream))


def test_refusals_by_handle():
    """Host-variant argument errors; a coarsest level below 2 pixels; skew with more than one level; a
    Z-sharded handle: UNSUPPORTED from every call."""
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    H, W = R.FIELD_H, R.FIELD_W
    depth = np.ones((H, W), np.uint16)
    eye = np.eye(4, dtype=np.float32)
    p = R.field_params(0x3)
    vol = semtsdf.Volume(p, 0)
    for kw in (dict(nlevels=0), dict(nlevels=5), dict(radius=5), dict(radius=-1), dict(sigma_r=0.0),
               dict(sigma_r=float("nan")), dict(band=0.0), dict(band=float("inf"))):
        args = dict(nlevels=3, radius=3, sigma_r=0.05, band=0.15)
        args.update(kw)
        with pytest.raises(L.SemTSDFError) as e:
            vol.frame_pyramid(depth, **args)
        assert e.value.code == L.ERR_INVALID, kw
    assert len(vol.frame_pyramid(depth, 4)) == 4       # 75 x 53 -> 9 x 6: four levels fit
    maps = {"vertex": np.zeros((H, W, 3), np.float32), "flags": np.zeros((H, W), np.uint8)}
    maps["normal"] = maps["point"] = maps["vertex"]
    big = {"vertex": np.zeros((2 * H, W, 3), np.float32), "flags": np.zeros((2 * H, W), np.uint8)}
    big["normal"] = big["vertex"]
    with pytest.raises(L.SemTSDFError) as e:           # the host variant's scratch holds W x H frame pixels
        vol.icp_system_level(big, maps, eye, eye)
    assert e.value.code == L.ERR_INVALID
    vol.close()
    # 12 x 9: level 2 is 3 x 2, level 3 would be 1 x 1
    p = semtsdf.default_params(16, R.KI, 12, 9)
    for a in range(3):
        p.voxel[a] = 0.01
    p.mu = 0.05
    vol = semtsdf.Volume(p, 0)
    assert [(g["width"], g["height"]) for g in vol.frame_levels(3)] == [(12, 9), (6, 4), (3, 2)]
    with pytest.raises(L.SemTSDFError) as e:
        vol.frame_levels(4)
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(L.SemTSDFError) as e:
        vol.frame_pyramid(np.ones((9, 12), np.uint16), 4)
    assert e.value.code == L.ERR_INVALID
    vol.close()
    p.K[1] = 0.5                                        # skew: one level only
    vol = semtsdf.Volume(p, 0)
    assert len(vol.frame_levels(1)) == 1
    with pytest.raises(L.SemTSDFError) as e:
        vol.frame_levels(2)
    assert e.value.code == L.ERR_INVALID
    vol.close()
    p = R.field_params(0x3)
    p.z_nshards, p.z_shard, p.z_chunk = 2, 0, 8
    vol = semtsdf.Volume(p, 0)
    lv = [{"z": 0x1000}] * 3
    for call in (lambda: vol.frame_levels(3), lambda: vol.frame_pyramid(depth),
                 lambda: vol.frame_pyramid_dev(0x1000, lv), lambda: vol.icp_system_level(maps, maps, eye, eye),
                 lambda: vol.icp_system_level_dev([0x1000] * 6, W, H, eye, eye, 0.1, 0.8, 1, 0x1000)):
        with pytest.raises(L.SemTSDFError) as e:
            call()
        assert e.value.code == L.ERR_UNSUPPORTED
    vol.close()


def test_host_class_tracks_with_the_pyramid():
    """TSDF.track(pyramid=True) on a default SyntheticStream: errors against the frame's own pose no larger
    than the guess's (the last fused frame's pose), and parse_frame takes the tracked extrinsic."""
    import semtsdf
    from semtsdf.synth import SyntheticStream
    from semtsdf.track import pose_errors

    st = SyntheticStream(seed=0)
    fr = [st.frame(k) for k in range(4)]
    dist = float(np.mean(fr[0].depth[fr[0].depth > 0])) / 5000.0
    t = semtsdf.TSDF(R.KI, 128)
    for k in range(3):
        t.parse_frame(fr[k].depth, fr[k].rgb, fr[k].w2c, dist, np.ascontiguousarray(fr[k].gt_ids))
    W = t.track(fr[3].depth, pyramid=True)
    assert W.shape == (4, 4) and W.dtype == np.float64
    t0, r0 = pose_errors(fr[2].w2c, fr[3].w2c)
    t1, r1 = pose_errors(W, fr[3].w2c)
    assert t1 <= t0 and r1 <= r0, (t0, r0, t1, r1)
    assert [e["level"] for e in t.last_track][0] == 2 and t.last_track[-1]["level"] == 0
    assert t.last_track[-1]["inliers"] > 100000
    n = t.n_obs
    t.parse_frame(fr[3].depth, fr[3].rgb, W, dist, np.ascontiguousarray(fr[3].gt_ids))
    assert t.n_obs == n + 1
    t.close()
