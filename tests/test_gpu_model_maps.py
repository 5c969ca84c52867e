"""semtsdf_render_maps on the device against the NumPy restatement of its rule
(tests/model_maps_restatement.py) on the oracle's state: every output equal, floats as bits."""
import ctypes as C

import numpy as np
import pytest

import model_maps_restatement as R

pytestmark = pytest.mark.gpu

NAMES = ("t", "point", "normal", "label", "votes", "flags")


def assert_maps_equal(got, want, names):
    for n in names:
        g, w = got[n], want[n]
        assert g.shape == w.shape and g.dtype == w.dtype, n
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = g != w
        assert not bad.any(), (n, int(bad.sum()), np.argwhere(bad)[:3].tolist())


@pytest.fixture(scope="module")
def fused():
    """The fused 64^3 volume on the device, integrated like the oracle state of the restatement."""
    import semtsdf

    semtsdf.load()
    sc = R.fused_scene()
    vol = semtsdf.Volume(sc["p"], 0)
    for k in range(1, 4):
        fr = sc["frames"][k]
        vol.integrate(fr.depth, fr.rgb, fr.gt_ids, sc["E"][k])
    yield vol, sc
    vol.close()


def _field_volume(flags):
    import semtsdf

    semtsdf.load()
    p, f, s2w, c, _ = R.field_view(flags, 1)
    vol = semtsdf.Volume(p, 0)
    color = f["color"] if flags & 4 else np.clip(f["color"], 0, 255).astype(np.uint8)
    vol.upload(sdf=f["sdf"], wt=f["wt"], color=color, hist=f["hist"] if flags & 1 else None)
    return vol, s2w, c


@pytest.mark.parametrize("angle", [0.0, 0.2])
def test_fused_maps_equal_the_restatement(fused, angle):
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.export import PALETTE

    vol, sc = fused
    s2w, c = semtsdf.orbit_camera(list(sc["p"].Kinv), angle, sc["dist"])
    for mw in (1, 2):
        s2w_o, c_o, _, want = R.fused_view(angle, mw)
        assert np.array_equal(s2w, s2w_o) and np.array_equal(c, c_o)
        got = vol.render_maps(s2w, c, mw)
        assert sorted(got) == sorted(NAMES)
        assert_maps_equal(got, want, NAMES)
    img, t = vol.raycast(s2w, c, L.RENDER_LABEL, want_t=True)
    assert np.array_equal(got["t"].view(np.uint32), t.view(np.uint32))
    lab = got["label"]
    assert np.array_equal(np.where((lab > 0)[..., None], PALETTE[lab][..., ::-1], 0).astype(np.uint8), img)


@pytest.mark.parametrize("flags", [0x3, 0x4])
def test_field_maps_equal_the_restatement(flags):
    """Ragged 75 x 53 image (tile edges in x and y, cy < 0), anisotropic voxels, dims that are no
    multiple of the storage tile, samples clamped at the faces, weights 0..4."""
    from semtsdf import _lib as L

    vol, s2w, c = _field_volume(flags)
    names = NAMES if flags & 1 else ("t", "point", "normal", "flags")
    seen = set()
    for mw in (1, 3):
        want = R.field_view(flags, mw)[4]
        got = vol.render_maps(s2w, c, mw, want=names)
        assert_maps_equal(got, want, names)
        hits = got["flags"][(got["flags"] & 1) != 0]
        assert hits.size >= 500
        seen |= set(np.unique(hits).tolist())
    assert seen == {1, 3}  # both validity outcomes among the hits
    if not flags & 1:  # label, votes: refused on a volume that is not SEMANTIC
        for name in ("label", "votes"):
            with pytest.raises(L.SemTSDFError) as e:
                vol.render_maps(s2w, c, 1, want=("t", name))
            assert e.value.code == L.ERR_STATE
    vol.close()


def test_subsets_determinism_and_read_only(fused):
    """Each output requested alone, and ("point", "flags"), gives the bytes of the full call; two
    calls return identical bytes; the volume is unchanged."""
    import semtsdf

    vol, sc = fused
    s2w, c = semtsdf.orbit_camera(list(sc["p"].Kinv), 0.2, sc["dist"])
    before = vol.download(hist=True)
    full = vol.render_maps(s2w, c, 1)
    again = vol.render_maps(s2w, c, 1)
    for n in NAMES:
        assert full[n].tobytes() == again[n].tobytes(), n
    for want in [(n,) for n in NAMES] + [("point", "flags")]:
        part = vol.render_maps(s2w, c, 1, want=want)
        assert sorted(part) == sorted(want)
        for n in want:
            assert part[n].tobytes() == full[n].tobytes(), (want, n)
    after = vol.download(hist=True)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k


def test_device_pointer_variant_on_a_second_stream(fused):
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.maps import MAP_LAYOUT

    vol, sc = fused
    lib = L.load()
    s2w, c = semtsdf.orbit_camera(list(sc["p"].Kinv), 0.2, sc["dist"])
    full = vol.render_maps(s2w, c, 2)
    n = vol.W * vol.H
    stream = C.c_void_p()
    L.check(lib.semtsdf_stream_create(C.byref(stream)))
    bufs = {k: semtsdf.DeviceBuffer(n * ch * np.dtype(dt).itemsize) for k, (dt, ch) in MAP_LAYOUT.items()}
    try:
        vol.render_maps_dev(s2w, c, 2, stream=stream, **{k: b.ptr for k, b in bufs.items()})
        for k, b in bufs.items():
            out = np.empty_like(full[k])
            b.download(out, stream)
            L.check(lib.semtsdf_stream_sync(stream))
            assert out.tobytes() == full[k].tobytes(), k
    finally:
        L.check(lib.semtsdf_stream_sync(stream))
        for b in bufs.values():
            b.free()
        L.check(lib.semtsdf_stream_destroy(stream))


def test_sharded_handle_is_unsupported():
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    p = R.field_params(0x3)
    p.z_nshards, p.z_shard, p.z_chunk = 2, 0, 8
    vol = semtsdf.Volume(p, 0)
    s2w, c = R.pose_camera_def(list(p.Kinv), np.eye(4, dtype=np.float32))
    with pytest.raises(L.SemTSDFError) as e:
        vol.render_maps(s2w, c, 1, want=("t",))
    assert e.value.code == L.ERR_UNSUPPORTED
    vol.close()


def test_host_class_model_maps_and_normal_render():
    """TSDF.model_maps(extrinsic=...) and TSDF.render(angle, mode="normal"): shapes, dtypes, and the
    shaded image black exactly where bit 1 of flags is clear."""
    import semtsdf
    from semtsdf.maps import MAP_LAYOUT

    sc = R.fused_scene()
    fr = sc["frames"]
    t = semtsdf.TSDF(R.KI, 64)
    for k in range(4):
        t.parse_frame(fr[k].depth, fr[k].rgb, fr[k].w2c, sc["dist"], np.ascontiguousarray(fr[k].gt_ids))
    m = t.model_maps(extrinsic=fr[3].w2c)
    assert sorted(m) == sorted(NAMES)
    for n, (dt, ch) in MAP_LAYOUT.items():
        assert m[n].dtype == dt and m[n].shape == (480, 640) + ((3,) if ch == 3 else ()), n
    hit = (m["flags"] & 1) != 0
    assert hit.mean() > 0.5 and np.array_equal(hit, m["t"] >= 0)
    E = semtsdf.pose.relative_pose(fr[3].w2c, t.init_extrinsic_inv)
    z = semtsdf.z_depth(m["point"], m["flags"], E)
    depth = fr[3].depth / 5000.0
    both = hit & (depth > 0)
    assert (np.abs(z[both] - depth[both]) <= float(t.voxel[0])).mean() >= 0.85
    dist = float(sc["dist"])
    mo = t.model_maps(angle=0.2, dist=dist)
    img = t.render(0.2, mode="normal", dist=dist)
    assert img.shape == (480, 640, 3) and img.dtype == np.uint8
    assert np.array_equal((img != 0).any(axis=-1), (mo["flags"] & 2) != 0)
    assert ((mo["flags"] & 2) != 0).mean() > 0.2
    views = t.orbit(1, mode="normal", step=0.2)
    assert len(views) == 1 and views[0].shape == (480, 640, 3)
    with pytest.raises(ValueError):
        t.model_maps()
    t.close()
