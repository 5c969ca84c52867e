"""Model maps on the CPU: the NumPy restatement of the rule (tests/model_maps_restatement.py) is
pinned against libm's fmaf and the C oracle's label render, the inputs of the GPU tests are shown
not to be empty, and the host helpers (pose_camera, z_depth) and the argument checks of the new
entry points are tested through the loaded library, without a device."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import model_maps_restatement as R

ANGLES = (0.0, 0.2)


def _libm_fmaf():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
    libm.fmaf.restype = C.c_float
    return libm.fmaf


def _check_fma(a, b, c):
    fmaf = _libm_fmaf()
    got = R.fma32(a, b, c)
    want = np.array([fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, a[bad[:3]], b[bad[:3]], c[bad[:3]])


def test_fma_helper_equals_libm_on_random_triples():
    rng = np.random.default_rng(1)
    n = 100000
    m = rng.uniform(-2.0, 2.0, (3, n))
    e = rng.integers(-20, 21, (3, n))
    a, b, c = (np.ldexp(m[i], e[i]).astype(np.float32) for i in range(3))
    _check_fma(a, b, c)


def test_fma_helper_equals_libm_near_cancellation_and_ties():
    """a * b + c nearly cancels (c within a few ulps of -a * b), or lands within a few f64 ulps of
    the midpoint of two neighbouring f32 values: the cases where rounding twice would differ."""
    rng = np.random.default_rng(2)
    n = 50000
    a = rng.uniform(0.5, 2.0, n).astype(np.float32)
    b = rng.uniform(0.5, 2.0, n).astype(np.float32)
    p = a.astype(np.float64) * b.astype(np.float64)
    # cancellation: c = -RN32(p) moved by -2..2 ulps
    c1 = -p.astype(np.float32)
    for _ in range(2):
        step = rng.integers(-1, 2, n)
        c1 = np.where(step > 0, np.nextafter(c1, np.float32(np.inf)),
                      np.where(step < 0, np.nextafter(c1, np.float32(-np.inf)), c1))
    # near a tie, within a fraction of an f32 ulp: the sum aims at the midpoint of f32 r and its
    # successor, c = RN32(mid - p)
    r = rng.uniform(4.0, 64.0, n).astype(np.float32)
    mid = (r.astype(np.float64) + np.nextafter(r, np.float32(np.inf)).astype(np.float64)) / 2
    c2 = (mid - p).astype(np.float32)
    # near a tie, below an f64 ulp (where rounding twice goes wrong): |c| in [2^20, 2^21) has f32
    # ulp 2^-3 and f64 ulp 2^-32; a * b = 2^-4 (1 - k 2^-23)(1 + k 2^-23) = 2^-4 - k^2 2^-50 is half an
    # f32 ulp less a sliver that the f64 sum loses for small k; k = 0 is the exact tie
    k = rng.integers(0, 64, n).astype(np.float64)
    a3 = (np.ldexp(1.0, -4) * (1.0 - k * 2.0 ** -23)).astype(np.float32)
    b3 = (1.0 + k * 2.0 ** -23).astype(np.float32)
    c3 = (np.ldexp(rng.integers(1 << 23, 1 << 24, n).astype(np.float64), -3) * rng.choice([-1.0, 1.0], n)
          ).astype(np.float32)
    assert np.array_equal(a3.astype(np.float64) * b3.astype(np.float64), 2.0 ** -4 - k * k * 2.0 ** -50)
    _check_fma(np.concatenate([a, a, a3]), np.concatenate([b, b, b3]), np.concatenate([c1, c2, c3]))


@pytest.mark.parametrize("angle", ANGLES)
def test_restatement_label_equals_the_oracle_render(angle):
    """palette[label] (black for 0) of the restatement equals oracle.render's mode-0 image at every
    pixel: pins the restatement's hit position, cell, fractions and argmax independently."""
    from semtsdf.export import PALETTE

    _, _, img, m = R.fused_view(angle)
    lab = m["label"]
    want = np.where((lab > 0)[..., None], PALETTE[lab][..., ::-1], 0).astype(np.uint8)  # the image is BGR
    assert np.array_equal(want, img), int((want != img).any(axis=-1).sum())
    assert (m["votes"][lab > 0] > 0).all() and (lab > 0).any()
    assert (m["votes"][m["flags"] == 0] == 0).all()


@pytest.mark.parametrize("angle", ANGLES)
def test_fused_inputs_are_not_empty(angle):
    """Hit share > 0.2, normal-valid share of the hits >= 0.5 at min_weight 1, and >= 0.98 of the
    valid normals face the camera (n . d < 0)."""
    s2w, c, _, m = R.fused_view(angle)
    hit = (m["flags"] & 1) != 0
    valid = (m["flags"] & 2) != 0
    assert np.array_equal(hit, m["t"] >= 0) and not (valid & ~hit).any()
    assert hit.mean() > 0.2, hit.mean()
    assert valid.sum() / hit.sum() >= 0.5, valid.sum() / hit.sum()
    _, d = R.rays(s2w, c, 640, 480)
    nd = (m["normal"].astype(np.float64) * d.astype(np.float64)).sum(axis=-1)
    assert (nd[valid] < 0).mean() >= 0.98, (nd[valid] < 0).mean()
    # misses and invalid normals hold zeros
    assert (m["normal"][~valid] == 0).all() and (m["point"][~hit] == 0).all() and (m["t"][~hit] == -1).all()


def test_field_inputs_are_not_empty():
    """The random field seen through the ragged 75 x 53 frame: at least 500 hits, and both validity
    outcomes among them.  15 % of the field's voxels are unobserved, so few hits have all 48 corners
    observed: valid normals exist at min_weight 1 only; at min_weight 3 the weight test refuses every
    hit, those included, so the two cases differ in exactly those pixels."""
    valid = {}
    for mw in (1, 3):
        _, _, _, _, m = R.field_view(0x3, mw)
        hit = (m["flags"] & 1) != 0
        valid[mw] = (m["flags"] & 2) != 0
        assert hit.sum() >= 500, int(hit.sum())
        assert (hit & ~valid[mw]).any()
    assert valid[1].any() and not valid[3].any()
    assert m["label"].any()


def test_valid_normals_have_unit_length():
    """| |n|^2 - 1 | <= 2^-20: g * (1 / sqrt(n2)) carries the roundings of n2 (three), the root, the
    reciprocal and one product per component, each 2^-24 relative, squared: about 2^-21 in all."""
    views = [R.fused_view(a)[3] for a in ANGLES] + [R.field_view(0x3, 1)[4]]
    for m in views:
        valid = (m["flags"] & 2) != 0
        n = m["normal"][valid].astype(np.float64)
        assert valid.any()
        assert np.abs((n * n).sum(axis=-1) - 1.0).max() <= 2.0 ** -20


def test_pose_camera_matches_its_definition():
    """semtsdf_pose_camera (through the library) against Rt = E[:3,:3]^T, o = -Rt E[:3,3],
    s2w = [Rt Kinv[:3,:3] | o] in f64, rounded once."""
    import semtsdf

    sc = R.fused_scene()
    rng = np.random.default_rng(3)
    cases = [(list(sc["p"].Kinv), sc["E"][k]) for k in (1, 2, 3)]
    cases.append((list(sc["p"].Kinv), np.eye(4, dtype=np.float32)))
    cases.append((rng.normal(size=(4, 4)).astype(np.float32), rng.normal(size=(4, 4)).astype(np.float32)))
    for kinv, E in cases:
        s2w, c = semtsdf.pose_camera(kinv, E)
        s2w_d, c_d = R.pose_camera_def(kinv, E)
        assert np.array_equal(s2w.view(np.uint32), s2w_d.view(np.uint32))
        assert np.array_equal(c.view(np.uint32), c_d.view(np.uint32))
        assert list(s2w[12:]) == [0.0, 0.0, 0.0, 1.0] and np.array_equal(c, s2w.reshape(4, 4)[:3, 3])
    # the definition: a world point in front of the frame's camera projects back onto its pixel
    E = sc["E"][3].astype(np.float64)
    s2w, c = semtsdf.pose_camera(list(sc["p"].Kinv), sc["E"][3])
    K = np.array(list(sc["p"].K), np.float64).reshape(4, 4)
    Pw = s2w.reshape(4, 4).astype(np.float64)[:3] @ np.array([100.0, 50.0, 1.0, 1.0])
    ray = Pw - c  # direction of pixel (100, 50) in the world
    q = E[:3, :3] @ (c + 2.0 * ray) + E[:3, 3]
    uv = K[:3, :3] @ q
    assert np.allclose(uv[:2] / uv[2], [100.0, 50.0], atol=1e-3)
    assert np.allclose(E[:3, :3] @ c + E[:3, 3], 0.0, atol=1e-5)  # c is the camera centre


def test_pose_camera_maps_align_with_the_frame_depth():
    """64^3, the pose of frame 3: the model's predicted depth (z_depth of the maps) agrees with the
    frame's depth image within one voxel on >= 0.85 of the hit pixels that have depth.  A transposed
    or uninverted pose fails it."""
    import semtsdf

    sc = R.fused_scene()
    s2w, c = semtsdf.pose_camera(list(sc["p"].Kinv), sc["E"][3])
    s2w_d, c_d, _, m = R.fused_pose_view(3)
    assert np.array_equal(s2w, s2w_d) and np.array_equal(c, c_d)
    z = semtsdf.z_depth(m["point"], m["flags"], sc["E"][3])
    hit = (m["flags"] & 1) != 0
    assert z.dtype == np.float64 and np.isnan(z[~hit]).all() and np.isfinite(z[hit]).all()
    depth = sc["frames"][3].depth.astype(np.float64) / 5000.0
    both = hit & (depth > 0)
    assert hit.mean() > 0.5 and both.sum() > 1000
    close = np.abs(z[both] - depth[both]) <= float(sc["p"].voxel[0])
    print("hit share", hit.mean(), "within one voxel", close.mean())
    assert close.mean() >= 0.85, close.mean()


def test_shade_normals_is_black_exactly_where_the_normal_is_invalid():
    import semtsdf

    s2w, c, _, m = R.fused_view(0.2)
    img = semtsdf.shade_normals(m, c)
    assert img.shape == (480, 640, 3) and img.dtype == np.uint8
    valid = (m["flags"] & 2) != 0
    assert np.array_equal((img != 0).any(axis=-1), valid)
    assert (img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all()
    assert img[valid].max() > 128  # surfaces facing the camera are lit


def test_argument_errors_without_a_device():
    """The INVALID cases of the new entry points return before any device work, with a message."""
    from semtsdf import _lib as L

    lib = L.load()
    s2w = (C.c_float * 16)()
    c = (C.c_float * 3)()
    buf = C.c_void_p(0x1000)
    out = L.MapsOut()
    out.t = 0x1000
    none = L.MapsOut()
    for fn in (lib.semtsdf_render_maps, lib.semtsdf_render_maps_dev):
        for args in ((None, s2w, c, 1, C.byref(out), None), (buf, None, c, 1, C.byref(out), None),
                     (buf, s2w, None, 1, C.byref(out), None), (buf, s2w, c, 1, None, None)):
            assert fn(*args) == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
        # all six pointers NULL: refused before the (made-up) handle is looked at
        assert fn(buf, s2w, c, 1, C.byref(none), None) == L.ERR_INVALID
        assert b"no map requested" in lib.semtsdf_last_error()
    E = (C.c_float * 16)()
    for args in ((None, E, s2w, c), (E, None, s2w, c), (E, E, None, c), (E, E, s2w, None)):
        assert lib.semtsdf_pose_camera(*args) == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    assert C.sizeof(L.MapsOut) == 6 * C.sizeof(C.c_void_p)
    assert (L.MAP_HIT, L.MAP_NORMAL) == (1, 2)
