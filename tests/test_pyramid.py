"""The depth pyramid on the host: the exports, the properties of the filter and of the level
geometry on the NumPy restatement of their rules (tests/pyramid_restatement.py), and what the pyramid
buys the tracker on the tracking scene: more inliers on noisy depth, a wider basin of convergence,
fewer full-resolution iterations.  No GPU."""
import numpy as np
import pytest

import icp_restatement as I
import pyramid_restatement as P

NEW_EXPORTS = ("semtsdf_frame_levels", "semtsdf_frame_pyramid", "semtsdf_frame_pyramid_dev",
               "semtsdf_icp_system_level", "semtsdf_icp_system_level_dev")


def test_library_exports_the_pyramid_calls():
    import ctypes as C

    from semtsdf import _lib as L

    lib = L.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert lib.semtsdf_abi_version() == 12  # exports are only added
    # semtsdf_frame_level: 2 i32 + 9 f32 (+ 4 B padding) + 4 pointers
    assert C.sizeof(L.FrameLevel) == 4 * 11 + 4 + 8 * 4
    # NULL arguments are refused before any device is touched
    lv = (L.FrameLevel * 4)()
    buf = C.c_void_p(0x1000)
    eye = (C.c_float * 16)()
    assert lib.semtsdf_frame_levels(None, 3, lv) == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    for fn in (lib.semtsdf_frame_pyramid, lib.semtsdf_frame_pyramid_dev):
        assert fn(None, buf, 3, 0.05, 0.15, 3, lv, None) == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    for fn in (lib.semtsdf_icp_system_level, lib.semtsdf_icp_system_level_dev):
        assert fn(None, C.byref(L.IcpIn()), 8, 8, eye, eye, 0.1, 0.8, 1, buf, None) == L.ERR_INVALID


def _ramp(h=40, w=56):
    """A tilted plane in raw units, 0.6 m .. 0.8 m at depth_scale 5000, with a hole."""
    y, x = np.mgrid[0:h, 0:w]
    d = (3000 + 11 * x + 9 * y).astype(np.uint16)
    d[7:12, 20:23] = 0
    return d


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_filter_returns_a_constant_image_bit_for_bit(radius):
    d = np.full((37, 45), 3217, np.uint16)
    z = P.restate_filter(d, 5000.0, radius, 0.05)
    assert z.dtype == np.float32 and z.tobytes() == (d.astype(np.float32) / np.float32(5000.0)).tobytes()


@pytest.mark.parametrize("radius", [1, 3, 4])
def test_filter_keeps_holes_and_only_holes(radius):
    d = _ramp()
    z = P.restate_filter(d, 5000.0, radius, 0.05)
    assert np.array_equal(z == 0, d == 0)
    zc = d.astype(np.float32) / np.float32(5000.0)
    assert np.abs(z - zc)[d != 0].max() < 0.01          # a mean of neighbours within 4 pixels of a gentle slope
    assert (z != zc).any()                              # and it does smooth


@pytest.mark.parametrize("radius", [1, 3, 4])
def test_filter_leaves_a_step_larger_than_sigma_r_exactly(radius):
    """Two constant halves 60 mm apart, sigma_r 50 mm: across the step u = 1 - (d / sigma_r)^2 < 0, so no
    neighbour of the other side has weight and each side is a constant image."""
    d = np.full((30, 40), 3000, np.uint16)
    d[:, 20:] = 3300
    st = {}
    z = P.restate_filter(d, 5000.0, radius, 0.05, st)
    assert z.tobytes() == (d.astype(np.float32) / np.float32(5000.0)).tobytes()
    assert st["rejected"] > 0 and st["accepted"] > 0
    # a step below sigma_r is smoothed
    d[:, 20:] = 3100
    z = P.restate_filter(d, 5000.0, radius, 0.05)
    assert (z[:, 18:22] != (d.astype(np.float32) / np.float32(5000.0))[:, 18:22]).any()


def test_spatial_term_keeps_69_of_81_taps_at_radius_4():
    assert [len(P.spatial_terms(r)) for r in (1, 2, 3, 4)] == [9, 25, 45, 69]
    t4 = P.spatial_terms(4)
    gone = sorted(set((dy, dx) for dy in range(-4, 5) for dx in range(-4, 5)) - set(t4))
    assert all(dx * dx + dy * dy >= 25 for dy, dx in gone) and len(gone) == 12
    assert t4[(0, 0)] == np.float32(1.0) and list(t4)[0] == (-4, -2) and list(t4)[-1] == (4, 2)
    # on an image with depth everywhere and a wide range term, an interior pixel takes all 68 neighbours
    d = np.full((21, 21), 3000, np.uint16)
    st = {}
    P.restate_filter(d, 5000.0, 4, 0.05, st)
    inner = sum(1 for y in range(21) for x in range(21) for dy, dx in t4
                if (dy, dx) != (0, 0) and 0 <= y + dy < 21 and 0 <= x + dx < 21)
    assert st == {"accepted": inner, "rejected": 0} and inner > 13 * 13 * 68


def test_halving_averages_inside_the_band_only():
    z = np.array([[1.0, 1.02, 0.0, 0.7, 9.0], [1.04, 1.5, 0.6, 0.8, 9.0], [2.0, 2.0, 2.0, 2.0, 9.0]], np.float32)
    st = {}
    out = P.restate_halve(z, 0.05, st)
    assert out.shape == (1, 2)
    f = np.float32
    want0 = f(1.0) + ((f(1.02) - f(1.0)) + (f(1.04) - f(1.0))) / f(3.0)   # 1.5 is out of the band
    assert out[0, 0] == want0 and out[0, 1] == 0.0                        # a hole at (2x, 2y) stays one
    assert st == {"inside": 2, "outside": 1}


@pytest.mark.parametrize("W,H", [(640, 480), (75, 53)])
def test_level_rays_are_the_means_of_their_four_fine_rays(W, H):
    """The ray of coarse pixel (x, y) through Kinv_l equals the mean of the rays of its four pixels one
    level finer, within 1e-6 (f32 rounding of the entries)."""
    if W == 640:
        p = I.tracking_scene()["p"]
    else:
        p = I.field_case()[0]
    assert (p.width, p.height) == (W, H)
    lv = P.level_geometry(list(p.K), list(p.Kinv), W, H, 3)
    assert [(w, h) for w, h, _ in lv] == [(W, H), (W >> 1, H >> 1), (W >> 2, H >> 2)]
    assert lv[0][2].tobytes() == np.asarray(list(p.Kinv), np.float32).reshape(4, 4)[:3, :3].tobytes()
    for l in (1, 2):
        w, h, ki = lv[l]
        fine = lv[l - 1][2].astype(np.float64)
        ys, xs = np.mgrid[0:h, 0:w]
        coarse = np.stack([xs, ys, np.ones_like(xs)], -1) @ ki.astype(np.float64).T
        mean = np.zeros_like(coarse)
        for oy in (0, 1):
            for ox in (0, 1):
                mean += np.stack([2 * xs + ox, 2 * ys + oy, np.ones_like(xs)], -1) @ fine.T
        assert np.abs(coarse - mean / 4.0).max() < 1e-6


def test_pyramid_loop_tags_levels_and_keeps_the_estimate_when_lost():
    from semtsdf.track import TrackingLost, pyramid_loop

    calls = []

    def system(level, E, dist_max, cos_min):
        calls.append((level, dist_max, cos_min))
        w = np.zeros(32, np.int64)
        w[:21][[0, 6, 11, 15, 18, 20]] = 1 << 32          # J^T J = I, J^T r = 0: a zero step
        w[28] = 500 if level else 3
        return w

    E0 = np.eye(4, dtype=np.float32)
    dims = [(64, 48), (32, 24), (16, 12)]
    E, log = pyramid_loop(system, dims, E0, ((2, 4, 0.3, 0.6), (1, 5, 0.2, 0.7)))
    assert np.array_equal(E, E0) and [e["level"] for e in log] == [2, 1] and log[0]["iter"] == log[1]["iter"] == 0
    assert calls == [(2, 0.3, 0.6), (1, 0.2, 0.7)]
    with pytest.raises(TrackingLost) as e:   # level 0: 3 inliers, below 1 % of 64 x 48
        pyramid_loop(system, dims, E0)
    assert np.array_equal(e.value.E, E0) and [x["level"] for x in e.value.log] == [2, 1, 0]
    E, log = pyramid_loop(system, dims, E0, min_inliers=3)
    assert [x["level"] for x in log] == [2, 1, 0]


def test_filter_recovers_inliers_and_rotation_on_noisy_depth():
    """Frame 3 with Gaussian axial noise of three times the sensor model (mean sigma 28 mm), tracked from
    E_ref at full resolution for 10 iterations, raw against filtered (radius 3, sigma_r 0.05).  Conditions:
    final inliers at least 3 x, rotation error at most 0.6 x.  Measured: inliers 18143 -> 81176 (4.47 x),
    rotation 0.00268 -> 0.00124 rad (0.46 x), translation 3.17 -> 2.19 mm."""
    from semtsdf.track import default_min_inliers, pose_errors, track_loop

    sc = I.tracking_scene()
    p = sc["p"]
    depth = P.noisy_depth()
    assert np.array_equal(depth == 0, sc["frames"][3].depth == 0)
    raw = I.restate_frame_maps(depth, list(p.Kinv), p.depth_scale)
    fil = P.scene_pyramid(radius=3, sigma_r=0.05, band=0.15, nlevels=1, noise=P.NOISE_S)[0]
    res = {}
    for name, fm in (("raw", raw), ("filtered", fil)):
        def system(E, fm=fm):
            return I.restate_system(fm, sc["model"], list(p.K), sc["E_ref"], E, **I.TRACK_GATES)

        E, log = track_loop(system, sc["E_ref"], 10, default_min_inliers(640, 480, 1), eps=0.0)
        res[name] = (log[-1]["inliers"],) + pose_errors(E, sc["E_true"])
        print(name, res[name], [e["inliers"] for e in log])
    assert res["filtered"][0] >= 3 * res["raw"][0]
    assert res["filtered"][2] <= 0.6 * res["raw"][2]


@pytest.mark.parametrize("k", [10, 11, 12, 13])
def test_pyramid_converges_where_full_resolution_icp_does_not(k):
    """Guesses 270 mm / 0.096 rad (k 10, 11) and 400 mm / 0.144 rad (k 12, 13) off, clean depth, radius 0,
    band 0.05, the default schedule, eps 1e-5.  The pyramid ends within 5 mm and 0.002 rad (measured 1.56 mm
    and 0.00047, 0.00068, 0.00063, 0.00064 rad); track_loop at full resolution (10 iterations, TRACK_GATES)
    is lost or ends more than 100 mm off (measured 555 mm, lost, lost, 584 mm)."""
    from semtsdf.track import TrackingLost, default_min_inliers, pose_errors, track_loop

    sc = I.tracking_scene()
    E, log = P.restated_track_pyramid(k)
    t, r = pose_errors(E, sc["E_true"])
    print(k, "pyramid", t, r, [(e["level"], e["inliers"]) for e in log])
    assert t <= 0.005 and r <= 0.002
    assert [e["level"] for e in log] == sorted((e["level"] for e in log), reverse=True)
    try:
        E1, _ = track_loop(I.scene_system, P.basin_guess(k), 10, default_min_inliers(640, 480, 1), eps=1e-5)
    except TrackingLost:
        print(k, "full resolution: lost")
    else:
        t1 = pose_errors(E1, sc["E_true"])[0]
        print(k, "full resolution", t1)
        assert t1 > 0.1


def test_pyramid_needs_fewer_full_resolution_iterations():
    """k = 6 (195 mm / 0.072 rad): both converge; level-0 iterations 2 against 8 measured."""
    from semtsdf.track import default_min_inliers, pose_errors, track_loop

    sc = I.tracking_scene()
    E, log = P.restated_track_pyramid(6)
    E1, log1 = track_loop(I.scene_system, P.basin_guess(6), 10, default_min_inliers(640, 480, 1), eps=1e-5)
    for e in (E, E1):
        t, r = pose_errors(e, sc["E_true"])
        assert t <= 0.005 and r <= 0.002
    fine = sum(1 for e in log if e["level"] == 0)
    print("level-0 iterations", fine, "single level", len(log1))
    assert fine < len(log1)
