"""One frame sequence through the four doors of the host API, on four handles: host parse_frame;
parse_frame_dev; host associate, then host integrate; associate_dev, then integrate_dev.  They share
the frame front end of semtsdf_api.cpp (first-frame label step or association, integrate, the
observation count), so after every frame the relabelled masks, n_obs and num_objs agree, and at the
end the four volumes hold the same bytes.  A 64^3 SEMANTIC volume, 75 x 53 images (no multiple of a
tile in x or y), four frames of six spheres: at most six labels a frame, so no id reaches 32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 75, 53
KI = (61.0, 61.1, 38.1, 27.6)
NFRAMES = 4


@pytest.fixture(scope="module")
def doors():
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream
    from semtsdf.volume import DeviceBuffer

    semtsdf.load()
    st = SyntheticStream(seed=0, width=W, height=H, intrinsics=KI, min_area=25)
    f0 = st.frame(0)
    frames = [st.frame(k) for k in range(1, 1 + NFRAMES)]
    p = semtsdf.default_params(64, KI, W, H)
    semtsdf.place_from_frame(p, f0.depth, float(np.mean(f0.depth[f0.depth > 0])) / 5000.0, L.PLACE_SFM)
    p.flags = L.F_SEMANTIC | L.F_GATE_COLOR
    vols = [semtsdf.Volume(p, 0) for _ in range(4)]
    n = W * H
    bufs = [{"d": DeviceBuffer(n * 2), "r": DeviceBuffer(n * 3), "m": DeviceBuffer(n)} for _ in range(2)]

    def dev_frame(vol, b, fr):
        for key, a in (("d", fr.depth), ("r", fr.rgb), ("m", fr.mask)):
            b[key].upload(a, vol.stream)

    def dev_mask(vol, b):
        out = np.zeros((H, W), np.uint8)
        b["m"].download(out, vol.stream)
        vol.sync()
        return out

    rec = []  # per frame: the four masks, the four (n_obs, num_objs), door 1's and door 3's stats
    for k, fr in enumerate(frames):
        E = (fr.w2c @ f0.c2w).astype(np.float32)
        assert 1 <= int(fr.mask.max()) <= 6
        masks, stats = [], {}
        # door 1: host parse_frame
        m = fr.mask.copy()
        stats[1] = vols[0].parse_frame(fr.depth, fr.rgb, m, E)
        masks.append(m)
        # door 2: parse_frame_dev
        dev_frame(vols[1], bufs[0], fr)
        vols[1].parse_frame_dev(bufs[0]["d"].ptr, bufs[0]["r"].ptr, bufs[0]["m"].ptr, E)
        masks.append(dev_mask(vols[1], bufs[0]))
        # door 3: host associate (from the second frame on), host integrate
        m = fr.mask.copy()
        if k > 0:
            stats[3] = vols[2].associate(m, E)
        vols[2].integrate(fr.depth, fr.rgb, m, E)
        masks.append(m)
        # door 4: associate_dev, integrate_dev
        dev_frame(vols[3], bufs[1], fr)
        if k > 0:
            vols[3].associate_dev(bufs[1]["m"].ptr, E, want_stats=True)
        vols[3].integrate_dev(bufs[1]["d"].ptr, bufs[1]["r"].ptr, bufs[1]["m"].ptr, E)
        masks.append(dev_mask(vols[3], bufs[1]))
        states = [(int(s.n_obs), int(s.num_objs)) for s in (v.state() for v in vols)]
        rec.append({"raw": fr.mask, "masks": masks, "states": states, "stats": stats})
    downloads = [v.download(hist=True) for v in vols]
    for b in bufs:
        for x in b.values():
            x.free()
    for v in vols:
        v.close()
    return rec, downloads


def test_masks_and_state_agree_after_every_frame(doors):
    rec, _ = doors
    for k, r in enumerate(rec):
        for door in (1, 2, 3):
            assert np.array_equal(r["masks"][0], r["masks"][door]), (k, door + 1)
        assert r["states"] == [r["states"][0]] * 4, (k, r["states"])
        assert r["states"][0][0] == k + 1
    assert any(not np.array_equal(r["masks"][0], r["raw"]) for r in rec[1:])  # an association relabelled something


def test_volumes_agree_at_the_end(doors):
    _, dl = doors
    assert (dl[0]["wt"] > 0).any() and dl[0]["hist"].any()
    for door in (1, 2, 3):
        assert np.array_equal(dl[0]["sdf"].view(np.uint32), dl[door]["sdf"].view(np.uint32)), door + 1
        for key in ("wt", "color", "hist"):
            assert np.array_equal(dl[0][key], dl[door][key]), (door + 1, key)


def test_parse_frame_stats(doors):
    """The first frame reports no association (identity lut, nothing assigned, num_objs = max label
    + 1); later frames report the decision host associate reports for the same frame."""
    rec, _ = doors
    st = rec[0]["stats"][1]
    assert bytes(st.lut) == bytes(range(256))
    assert list(st.assigned_prev) == [-1] * 32
    assert st.num_objs == int(rec[0]["raw"].max()) + 1 == rec[0]["states"][0][1]
    for r in rec[1:]:
        assert bytes(r["stats"][1]) == bytes(r["stats"][3])
