"""Camera tracking on the host: the algebra of semtsdf/track.py, and the ICP loop run over the NumPy
restatement of the device rules (tests/icp_restatement.py) on the tracking scene.  No GPU."""
import numpy as np
import pytest

import icp_restatement as I


def test_system_from_words_round_trips_a_hand_made_system():
    from semtsdf.track import system_from_words

    rng = np.random.default_rng(1)
    J = rng.integers(-64, 64, (40, 6)) / 8.0   # multiples of 1/8: every product is exact in 2^-32 units
    r = rng.integers(-64, 64, 40) / 64.0
    A, b, r2 = J.T @ J, J.T @ r, float(r @ r)
    words = np.zeros(32, np.int64)
    words[:21] = np.rint(A[np.triu_indices(6)] * 2.0 ** 32).astype(np.int64)
    words[21:27] = np.rint(b * 2.0 ** 32).astype(np.int64)
    words[27] = int(round(r2 * 2.0 ** 32))
    words[28:] = (40, 3, 2, 1)
    A2, b2, r22, counts = system_from_words(words)
    assert np.array_equal(A2, A) and np.array_equal(A2, A2.T)
    assert np.array_equal(b2, b) and r22 == r2
    assert counts == {"inliers": 40, "far": 3, "angle": 2, "none": 1}


def test_se3_apply_of_a_twist_and_its_negative_is_the_identity():
    from semtsdf.track import se3_apply, se3_exp

    for xi in ([0.3, -0.2, 0.5, 0.1, 0.2, -0.3], [1e-9, 2e-9, -1e-9, 0.05, 0.0, -0.02], [0.0] * 3 + [1.0, 2.0, 3.0]):
        xi = np.asarray(xi)
        T = se3_exp(xi)
        assert np.abs(T @ se3_exp(-xi) - np.eye(4)).max() < 1e-15
        assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() < 1e-15
    # the small-angle series meets Rodrigues' formula at the branch
    xi = np.array([0.9e-2, -0.8e-2, 0.9e-2, 1.0, 1.0, 1.0])  # |omega| = 1.5e-2: Rodrigues; its half: the series
    half = se3_exp(0.5 * xi)
    assert np.abs(se3_exp(xi) - half @ half).max() < 1e-15
    # through the f32 extrinsic: back within f32 rounding of the entries
    E = I.tracking_scene()["E_ref"]
    xi = np.array([0.01, -0.02, 0.015, 0.03, -0.01, 0.02])
    back = se3_apply(-xi, se3_apply(xi, E))
    assert back.dtype == np.float32 and np.abs(back.astype(np.float64) - E).max() < 4e-7
    # a pure translation of the volume frame moves the camera centre by it
    moved = np.linalg.inv(se3_apply([0, 0, 0, 0.1, 0.2, 0.3], np.eye(4)).astype(np.float64))
    assert np.allclose(moved[:3, 3], [0.1, 0.2, 0.3], atol=1e-7)


def test_a_singular_or_non_finite_system_raises():
    from semtsdf.track import TrackingLost, solve_step, track_loop

    A = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 0.0])
    with pytest.raises(np.linalg.LinAlgError):
        solve_step(A, np.ones(6))
    with pytest.raises(np.linalg.LinAlgError):
        solve_step(np.full((6, 6), np.nan), np.ones(6))
    assert np.allclose(solve_step(2.0 * np.eye(6), np.ones(6)), 0.5)
    # the loop turns both, and too few inliers, into TrackingLost with the estimate kept
    E0 = np.eye(4, dtype=np.float32)
    words = np.zeros(32, np.int64)
    words[28] = 100
    with pytest.raises(TrackingLost) as e:
        track_loop(lambda E: words, E0, 3, min_inliers=6)
    assert np.array_equal(e.value.E, E0) and len(e.value.log) == 1
    with pytest.raises(TrackingLost):
        track_loop(lambda E: words, E0, 3, min_inliers=101)


def test_restated_frame_maps_are_a_camera_facing_surface():
    sc = I.tracking_scene()
    fm = sc["frame"]
    depth = sc["frames"][3].depth
    assert np.array_equal((fm["flags"] & 1) != 0, depth != 0)
    ok = (fm["flags"] & 2) != 0
    assert ok.mean() > 0.5 and not ok[-1].any() and not ok[:, -1].any()
    assert np.array_equal(fm["vertex"][..., 2][depth != 0], (depth[depth != 0].astype(np.float32) / np.float32(5000.0)))
    n = fm["normal"][ok].astype(np.float64)
    assert np.abs((n * n).sum(-1) - 1.0).max() < 1e-6
    assert (n[:, 2] < 0).mean() > 0.99          # towards the camera, which looks along +z
    assert not fm["normal"][~ok].any() and not fm["vertex"][depth == 0].any()


def test_restated_loop_tracks_frame_3():
    """10 iterations from the constant-pose guess (frame 2's extrinsic): both errors against the stream's
    ground truth at most a quarter of the guess's.  Measured: guess 33.5 mm, 0.01200 rad; final 1.56 mm,
    0.00063 rad (1/21, 1/19); inliers 220058, 237932, 238579, 238530, 238536, then 238535 / 238536."""
    from semtsdf.track import default_min_inliers, pose_errors, track_loop

    sc = I.tracking_scene()
    t0, r0 = pose_errors(sc["E_ref"], sc["E_true"])
    E, log = I.restated_track()
    t1, r1 = pose_errors(E, sc["E_true"])
    print(f"guess {t0 * 1e3:.2f} mm {r0:.5f} rad; final {t1 * 1e3:.2f} mm {r1:.5f} rad")
    for entry in log:
        print(entry)
    assert len(log) == 10 and E.dtype == np.float32
    assert t1 <= 0.25 * t0 and r1 <= 0.25 * r0
    for entry in log:
        assert entry["inliers"] + entry["far"] + entry["angle"] + entry["none"] == log[0]["inliers"] + log[0]["far"] \
            + log[0]["angle"] + log[0]["none"]
    assert log[-1]["rms"] < 0.25 * log[0]["rms"] and log[-1]["inliers"] > log[0]["inliers"]
    # with the default epsilon the loop stops early, at a pose that is as good
    E5, log5 = track_loop(I.scene_system, sc["E_ref"], 10, default_min_inliers(640, 480, 1), eps=1e-5)
    assert len(log5) < 10 and log5[-1]["step"] < 1e-5
    t5, r5 = pose_errors(E5, sc["E_true"])
    assert t5 <= 0.25 * t0 and r5 <= 0.25 * r0


def test_field_case_reaches_every_class_on_the_restatement():
    """The ragged field view as an ICP problem (the GPU test's case).  With the view's maps at
    min_weight 1 only 4 of its 676 hits carry a normal (48 corner weights >= 1 each, weights 0..4), so
    no small offset reaches the inlier, far and angle classes at stride 1 and 2 together; the maps at
    min_weight 0 (every hit carries one) do, with the offset and gates chosen here."""
    import model_maps_restatement as R

    p, _, m1, depth = I.field_case()
    assert int(((m1["flags"] & 2) != 0).sum()) == 4
    fm = I.restate_frame_maps(depth, list(p.Kinv), p.depth_scale)
    assert depth[-1, 10:30].max() == 0 and depth[20:30, -1].max() == 0 and depth[5:20, 16].max() == 0
    m0 = R.field_view(0x3, 0)[4]
    eye = np.eye(4, dtype=np.float32)
    for stride in (1, 2):
        w = I.restate_system(fm, m0, list(p.K), eye, I.field_offset(), stride=stride, **I.FIELD_GATES)
        assert (w[28:] > 0).all(), (stride, w[28:])
        vis = int(((fm["flags"][::stride, ::stride] & 3) == 3).sum())
        assert int(w[28:].sum()) == vis
