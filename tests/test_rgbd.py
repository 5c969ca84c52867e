"""RGB-D tracking on the host: the exports, the properties of the intensity pyramid and of the 64-word
system on the NumPy restatement of their rules (tests/rgbd_restatement.py), and what the photometric
term buys the tracker: a textured wall, where point-to-plane ICP alone has no in-plane constraint, and
no harm on the sphere scene.  No GPU."""
import numpy as np
import pytest

import icp_restatement as I
import pyramid_restatement as P
import rgbd_restatement as G
from rgbd_restatement import FIELD_GATES, field_inputs

NEW_EXPORTS = ("semtsdf_intensity_pyramid", "semtsdf_intensity_pyramid_dev", "semtsdf_rgbd_system_level",
               "semtsdf_rgbd_system_level_dev")


def test_library_exports_the_rgbd_calls():
    import ctypes as C

    from semtsdf import _lib as L

    lib = L.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert lib.semtsdf_abi_version() == 12  # exports are only added
    assert C.sizeof(L.IntensityLevel) == 8 + 16 and C.sizeof(L.RgbdIn) == 32 and L.RGBD_WORDS == 64
    lv = (L.IntensityLevel * 4)()
    buf = C.c_void_p(0x1000)
    eye = (C.c_float * 16)()
    for fn in (lib.semtsdf_intensity_pyramid, lib.semtsdf_intensity_pyramid_dev):
        assert fn(None, buf, None, 3, lv, None) == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    for fn in (lib.semtsdf_rgbd_system_level, lib.semtsdf_rgbd_system_level_dev):
        assert fn(None, C.byref(L.IcpIn()), C.byref(L.RgbdIn()), 0, eye, eye, 0.1, 0.8, 0.1, 1, buf,
                  None) == L.ERR_INVALID


def test_constant_image_gives_a_constant_pyramid():
    rgb = np.empty((53, 75, 3), np.uint8)
    rgb[:] = (200, 17, 90)
    Y = 200 + 2 * 17 + 90
    lv = G.restate_intensity_pyramid(rgb, None, 4)
    assert [(v["width"], v["height"]) for v in lv] == [(75, 53), (37, 26), (18, 13), (9, 6)]
    for l, v in enumerate(lv):
        assert v["S"].dtype == np.uint32 and (v["S"] == 16 * 4 ** l * Y).all(), l
        assert v["valid"].dtype == np.uint8 and (v["valid"] == 1).all(), l
        # the one conversion: exact, and the same intensity at every level
        assert float(np.float32(v["S"][0, 0]) * np.float32(2.0 ** -(14 + 2 * l))) == Y / 1024.0
    white = G.restate_intensity_pyramid(np.full((8, 8, 3), 255, np.uint8), None, 3)
    assert int(white[0]["S"].max()) == 16320 and int(white[2]["S"].max()) == 16320 * 16 < 2 ** 20


def test_invalid_pixels_spread_exactly_one_pixel():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    valid = np.ones((40, 56), np.uint8)
    valid[17, 23] = 0
    valid[0, 0] = 0
    valid[39, 30] = 0
    lv = G.restate_intensity_pyramid(rgb, valid, 3)
    want = np.ones((40, 56), np.uint8)
    want[16:19, 22:25] = 0
    want[0:2, 0:2] = 0
    want[38:40, 29:32] = 0
    assert np.array_equal(lv[0]["valid"], want)
    # a coarse pixel is valid iff its four are
    assert np.array_equal(lv[1]["valid"], want.reshape(20, 2, 28, 2).min(axis=(1, 3)))
    # validity does not touch the sums
    assert np.array_equal(lv[0]["S"], G.restate_intensity_pyramid(rgb, None, 1)[0]["S"])
    # the clamped border: corner pixel (0, 0) sees Y(0, 0) nine times with weights 1 2 1 x 1 2 1 folded
    c = rgb.astype(np.int64)
    Y = c[..., 0] + 2 * c[..., 1] + c[..., 2]
    assert int(lv[0]["S"][0, 0]) == 9 * Y[0, 0] + 3 * Y[0, 1] + 3 * Y[1, 0] + Y[1, 1]


def test_rgb_and_bgr_give_equal_sums():
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, (53, 75, 3), dtype=np.uint8)
    a = G.restate_intensity_pyramid(rgb, None, 3)
    b = G.restate_intensity_pyramid(rgb[..., ::-1], None, 3)
    for x, y in zip(a, b):
        assert np.array_equal(x["S"], y["S"])


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("level", [0, 1])
def test_geometric_words_are_restate_system_and_every_photometric_class_occurs(level, stride):
    p, frame, m, f_int, m_int = field_inputs(level)
    eye = np.eye(4, dtype=np.float32)
    words = G.restate_rgbd_system(frame, m, f_int, m_int, level, list(p.K), eye, I.field_offset(), stride=stride,
                                  **FIELD_GATES)
    assert words.dtype == np.int64 and words.shape == (64,)
    geo = P.restate_system_level(frame, m, list(p.K), eye, I.field_offset(), FIELD_GATES["dist_max"],
                                 FIELD_GATES["cos_min"], stride)
    assert words[:32].tolist() == geo.tolist()
    if level == 0:
        assert geo.tolist() == I.restate_system(frame, m, list(p.K), eye, I.field_offset(), FIELD_GATES["dist_max"],
                                                FIELD_GATES["cos_min"], stride).tolist()
    visited = ((frame["flags"][::stride, ::stride] & 1) != 0) & (f_int["valid"][::stride, ::stride] != 0)
    assert int(words[60:].sum()) == int(visited.sum())
    assert (words[60:] > 0).all(), words[60:]          # inliers, far, outlier, none
    assert words[59] > 0 and words[32] > 0             # sum r^2 and J0 J0 of the inliers


def test_system_from_words_scales_both_halves():
    from semtsdf.track import rgbd_system_from_words, system_from_words

    w = np.arange(64, dtype=np.int64) * (1 << 20)
    (A, b, r2, c), (Ap, bp, rp2, cp) = rgbd_system_from_words(w)
    A0, b0, r20, c0 = system_from_words(w[:32])
    assert np.array_equal(A, A0) and np.array_equal(b, b0) and r2 == r20 and c == c0
    assert Ap[0, 0] == 32.0 and Ap[0, 5] == Ap[5, 0] == 37.0 and Ap[5, 5] == 52.0
    assert bp.tolist() == [53.0, 54.0, 55.0, 56.0, 57.0, 58.0] and rp2 == 59.0
    assert cp == {"inliers": 60 << 20, "far": 61 << 20, "outlier": 62 << 20, "none": 63 << 20}


def test_photometric_term_tracks_the_wall_where_geometry_cannot():
    """A plane seen head on: J^T J of point-to-plane ICP has rank 3, so from a guess 36 mm off in the
    plane pyramid_loop raises TrackingLost with the guess's error kept.  rgbd_loop ends at 2.42 mm,
    0.00035 rad (a tenth of the 24.2 mm voxel): 14.9 times nearer.  The condition is half that factor."""
    from semtsdf.track import TrackingLost, pose_errors, pyramid_loop

    sc = G.wall_scene()
    E0 = G.wall_guess()
    t0 = pose_errors(E0, sc["E_true"])[0]
    assert 0.035 < t0 < 0.037
    try:
        E_geo, _ = pyramid_loop(G.scene_geo_system(sc), G.scene_dims(sc), E0)
    except TrackingLost as e:
        E_geo = e.E
    c2w = [np.linalg.inv(np.asarray(E, np.float64)) for E in (E_geo, sc["E_true"])]
    in_plane = float(np.linalg.norm((c2w[0] - c2w[1])[:2, 3]))
    assert in_plane >= 0.9 * t0, in_plane                  # geometry alone keeps the in-plane error
    t_geo = pose_errors(E_geo, sc["E_true"])[0]
    E, log = G.restated_track_rgbd("wall")
    t, r = pose_errors(E, sc["E_true"])
    print(f"wall: guess {t0 * 1e3:.2f} mm, geometric {t_geo * 1e3:.2f} mm, rgbd {t * 1e3:.3f} mm {r:.5f} rad, "
          f"factor {t_geo / t:.2f}")
    assert t_geo / t >= 14.9 / 2, (t_geo, t)
    assert all(e["photo_used"] for e in log) and {e["level"] for e in log} == {0, 1, 2}
    assert log[-1]["photo_inliers"] > 250000 and log[-1]["photo_rms"] < log[0]["photo_rms"]


def test_photometric_term_does_no_harm_on_the_sphere_scene():
    """The sphere scene's checker is fixed to the screen, so its photometric term argues for no motion;
    at the default weight rgbd_loop still ends within the 1.56 mm voxel floor of pyramid_loop's end."""
    from semtsdf.track import pose_errors

    sc = G.sphere_scene()
    E_geo, _ = P.restated_track_pyramid(None)
    E, log = G.restated_track_rgbd("sphere")
    t_geo, r_geo = pose_errors(E_geo, sc["E_true"])
    t, r = pose_errors(E, sc["E_true"])
    print(f"spheres: geometric {t_geo * 1e3:.3f} mm {r_geo:.5f} rad, rgbd {t * 1e3:.3f} mm {r:.5f} rad")
    assert t <= t_geo + 0.00156, (t, t_geo)
    assert r <= r_geo + 0.00063, (r, r_geo)                # the rotation floor of the same table
    assert all(e["photo_used"] for e in log)


def test_a_thin_photometric_term_is_dropped_and_logged():
    """min_inliers above the photometric inliers of a level: the iteration is geometric alone."""
    from semtsdf.track import PYRAMID_SCHEDULE, rgbd_loop, system_from_words

    sc = G.sphere_scene()
    calls = []

    def system(level, E, dist_max, cos_min, r_max):
        w = G.scene_rgbd_system(sc)(level, E, dist_max, cos_min, r_max)
        w[32:] = 0
        w[60] = 5
        calls.append(w.copy())
        return w

    E, log = rgbd_loop(system, G.scene_dims(sc), sc["E_ref"], PYRAMID_SCHEDULE[:1], eps=0.0)
    assert [e["photo_used"] for e in log] == [False] * 4 and [e["photo_inliers"] for e in log] == [5] * 4
    A, b, _, _ = system_from_words(calls[0][:32])
    assert log[0]["step"] == float(np.linalg.norm(np.linalg.solve(A, b)))
