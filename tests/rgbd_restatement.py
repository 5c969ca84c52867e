"""NumPy restatement of the RGB-D tracking rules (include/semtsdf.h, "RGB-D tracking"): the integer
intensity pyramid of a colour image and the 64 fixed-point words of one iteration, every f32 operation
once in the rule's order (fma32, dot3 of model_maps_restatement; cross of icp_restatement; words 0..31
are pyramid_restatement.restate_system_level's), plus the scenes of the tests: a textured wall whose
colour is fixed to the world, and the sphere scene of icp_restatement with its colour render.
"""
import functools
import math

import numpy as np

import icp_restatement as I
import pyramid_restatement as P
from model_maps_restatement import F, KI, _oracle, dot3, fma32, pose_camera_def, restate_maps

BAND = P.SCENE_BAND      # the depth pyramid of the scenes: radius 0, this halving band


def restate_intensity_pyramid(rgb, valid=None, nlevels=3):
    """[{width, height, S u32 [h, w], valid u8 [h, w]}] of a u8 image [H, W, 3] and an optional validity
    image [H, W] (nonzero = valid).  Integers throughout."""
    c = np.asarray(rgb, np.uint8).astype(np.int64)
    H, W = c.shape[:2]
    Y = c[..., 0] + 2 * c[..., 1] + c[..., 2]
    ok = np.ones((H, W), bool) if valid is None else np.asarray(valid).reshape(H, W) != 0
    Yp = np.pad(Y, 1, mode="edge")          # coordinates clamped to the image
    okp = np.pad(ok, 1, mode="edge")
    S = np.zeros((H, W), np.int64)
    v = np.ones((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            S += (1, 2, 1)[dy] * (1, 2, 1)[dx] * Yp[dy:dy + H, dx:dx + W]
            v &= okp[dy:dy + H, dx:dx + W]
    out = []
    for l in range(nlevels):
        if l:
            h, w = S.shape[0] >> 1, S.shape[1] >> 1
            q = [(a[0:2 * h:2, 0:2 * w:2], a[0:2 * h:2, 1:2 * w:2], a[1:2 * h:2, 0:2 * w:2], a[1:2 * h:2, 1:2 * w:2])
                 for a in (S, v)]
            S = q[0][0] + q[0][1] + q[0][2] + q[0][3]
            v = q[1][0] & q[1][1] & q[1][2] & q[1][3]
        assert S.shape == (H >> l, W >> l) and int(S.max(initial=0)) <= 16320 * 4 ** l
        out.append({"width": W >> l, "height": H >> l, "S": S.astype(np.uint32), "valid": v.astype(np.uint8)})
    return out


def level_camera(K, level):
    """(fx_l, fy_l, cx_l, cy_l) f32 of a pyramid level: formed in float64, rounded once."""
    K = np.asarray(K, np.float32).reshape(4, 4).astype(np.float64)
    s = float(1 << level)
    return (F(K[0, 0] / s), F(K[1, 1] / s), F((K[0, 2] + 0.5) / s - 0.5), F((K[1, 2] + 0.5) / s - 0.5))


def restate_photo_words(frame, model, f_int, m_int, level, K, E_ref, E_cur, dist_max, r_max, stride):
    """Words 32..63: the photometric system of frame level `level` against the model's level."""
    fH, fW = frame["flags"].shape
    H, W = model["flags"].shape
    assert (fH, fW) == (H >> level, W >> level) == f_int["S"].shape == m_int["S"].shape
    fxl, fyl, cxl, cyl = level_camera(K, level)
    Er = np.asarray(E_ref, np.float32).reshape(4, 4)
    dmax2 = F(dist_max) * F(dist_max)
    scale = F(2.0 ** -(14 + 2 * level))
    ys, xs = I.visited_grid(frame, stride)
    vis = ((frame["flags"][ys, xs] & 1) != 0) & (f_int["valid"][ys, xs] != 0)
    ys, xs = ys[vis], xs[vis]
    _, Pw, q, on, vi, ui = I.project(frame, model, K, E_ref, E_cur, ys, xs)
    mS, mV = m_int["S"], m_int["valid"]
    with np.errstate(all="ignore"):
        on = on & ((model["flags"][vi, ui] & 1) != 0)
        d = [model["point"][vi, ui, a] - Pw[a] for a in range(3)]
        far = on & (dot3(d[0], d[1], d[2], d[0], d[1], d[2]) > dmax2)
        iz = F(1.0) / q[2]
        ul = fma32(fxl, q[0] * iz, cxl)
        vl = fma32(fyl, q[1] * iz, cyl)
        x0 = np.floor(ul)
        y0 = np.floor(vl)
        inside = on & ~far & (x0 >= 0) & (x0 + F(1.0) < F(fW)) & (y0 >= 0) & (y0 + F(1.0) < F(fH))
        xi = np.where(inside, x0, 0).astype(np.int64)
        yi = np.where(inside, y0, 0).astype(np.int64)
        inside &= (mV[yi, xi] != 0) & (mV[yi, xi + 1] != 0) & (mV[yi + 1, xi] != 0) & (mV[yi + 1, xi + 1] != 0)
        xi = np.where(inside, xi, 0)
        yi = np.where(inside, yi, 0)
        ax = ul - x0
        ay = vl - y0
        m00, m10 = mS[yi, xi].astype(np.float32) * scale, mS[yi, xi + 1].astype(np.float32) * scale
        m01, m11 = mS[yi + 1, xi].astype(np.float32) * scale, mS[yi + 1, xi + 1].astype(np.float32) * scale
        dx0, dx1, dy0 = m10 - m00, m11 - m01, m01 - m00
        top = fma32(ax, dx0, m00)
        bot = fma32(ax, dx1, m01)
        Im = fma32(ay, bot - top, top)
        gx = fma32(ay, dx1 - dx0, dx0)
        gy = fma32(ax, (m11 - m10) - dy0, dy0)
        r = f_int["S"][ys, xs].astype(np.float32) * scale - Im
        outlier = inside & (np.abs(r) > F(r_max))
        a0 = (gx * fxl) * iz
        a1 = (gy * fyl) * iz
        a2 = -((a0 * q[0] + a1 * q[1]) * iz)
        aw = [dot3(Er[0, k], Er[1, k], Er[2, k], a0, a1, a2) for k in range(3)]
        J = I.cross(Pw, aw) + aw
        inl = inside & ~outlier
        for k in range(6):
            inl &= np.abs(J[k]) < F(2048.0)
    return I.pack_words(J, r, inl, far, outlier, vis.sum(), 1048576.0)


def restate_rgbd_system(frame, model, f_int, m_int, level, K, E_ref, E_cur, dist_max, cos_min, r_max, stride=1):
    """The 64 int64 words: restate_system_level's 32, then the photometric 32."""
    geo = P.restate_system_level(frame, model, K, E_ref, E_cur, dist_max, cos_min, stride)
    pho = restate_photo_words(frame, model, f_int, m_int, level, K, E_ref, E_cur, dist_max, r_max, stride)
    return np.concatenate([geo, pho])


def model_valid(model):
    """The validity image of the model's colour render: hit and normal."""
    return ((model["flags"] & 3) == 3).astype(np.uint8)


# ------------------------------------------------------------------------------------
# the textured wall: one plane, colour fixed to the world
# ------------------------------------------------------------------------------------
WALL_Z = 2.0
WALL_STEP = (0.02, 0.012, 0.0)     # camera translation per frame, in the plane
WALL_ROLL = 0.004                  # and rotation about the optical axis per frame


def wall_colour(X, Y):
    """u8 [.., 3] of the world point (X, Y, WALL_Z): sinusoids along both in-plane axes, wavelengths of
    0.4 m and more."""
    tau = 2.0 * math.pi
    a = np.sin(tau * X / 0.4) + np.sin(tau * Y / 0.5)
    b = np.sin(tau * (X + Y) / 0.9) + np.sin(tau * (X - Y) / 0.7)
    c = np.sin(tau * X / 1.3 + 1.0) + np.sin(tau * Y / 0.6 + 2.0)
    ch = [128.0 + 30.0 * a + 25.0 * b, 128.0 + 25.0 * b + 30.0 * c, 128.0 + 30.0 * c + 25.0 * a]
    return np.clip(np.rint(np.stack(ch, axis=-1)), 0, 255).astype(np.uint8)


def wall_frame(k, W=640, H=480):
    """(depth u16, rgb u8, c2w f64) of frame k: the camera slides and rolls in front of the wall."""
    fx, fy, cx, cy = KI
    a = WALL_ROLL * k
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    c2w[:3, 3] = np.asarray(WALL_STEP) * k
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    rays = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(j, dtype=np.float64)], axis=-1)
    dirs = rays @ c2w[:3, :3].T
    s = (WALL_Z - c2w[2, 3]) / dirs[..., 2]            # camera z of the hit: the rays have z = 1
    X = c2w[:3, 3] + s[..., None] * dirs
    depth = np.clip(np.rint(s * 5000.0), 0, 65535).astype(np.uint16)
    return depth, wall_colour(X[..., 0], X[..., 1]), c2w


def _scene(frames, c2ws):
    """Frames 1-2 integrated by the oracle into a 128^3 volume placed from frame 0; the model maps, the
    colour render and its intensity pyramid at frame 2's pose; the pyramids of frame 3."""
    import semtsdf
    from semtsdf import _lib as L

    O = _oracle()
    p = semtsdf.default_params(I.TRACK_DIM, KI, 640, 480)
    d0 = frames[0][0]
    semtsdf.place_from_frame(p, d0, float(np.mean(d0[d0 > 0])) / 5000.0, L.PLACE_SFM)
    p.flags = 0x3
    g = O.OGeom.from_params(p)
    D = (I.TRACK_DIM,) * 3
    ost = O.OState(list(D), p.mu, semantic=True)
    Es = [(np.linalg.inv(c) @ c2ws[0]).astype(np.float32) for c in c2ws]
    for k in (1, 2):
        depth, rgb, ids = frames[k]
        O.integrate(g, ost, list(p.K), Es[k], depth, rgb, ids, flags=0x3)
    s2w, c = pose_camera_def(list(p.Kinv), Es[2])
    img, t = O.render(g, s2w, c, p.width, p.height, 1, ost.sdf, ost.hist, ost.color)
    model = restate_maps(t, s2w, c, ost.sdf.reshape(D), ost.wt.reshape(D), None, list(p.vol_start), list(p.voxel), 1)
    depth, rgb, _ = frames[3]
    return {"p": p, "frames": frames, "E": Es, "E_ref": Es[2], "E_true": Es[3], "model": model, "m_rgb": img,
            "m_int": restate_intensity_pyramid(img, model_valid(model), 3),
            "f_int": restate_intensity_pyramid(rgb, None, 3),
            "pyramid": P.restate_pyramid(depth, list(p.K), list(p.Kinv), p.depth_scale, 3, 0, 0.05, BAND)}


@functools.lru_cache(maxsize=None)
def wall_scene():
    fr = [wall_frame(k) for k in range(4)]
    ids = np.zeros((480, 640), np.uint8)
    return _scene([(d, c, ids) for d, c, _ in fr], [c2w for _, _, c2w in fr])


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """icp_restatement.tracking_scene's frames and poses, with the colour side."""
    sc = I.tracking_scene()
    out = _scene([(f.depth, f.rgb, f.gt_ids) for f in sc["frames"]], [f.c2w for f in sc["frames"]])
    assert out["E_ref"].tobytes() == sc["E_ref"].tobytes()
    assert out["model"]["flags"].tobytes() == sc["model"]["flags"].tobytes()
    return out


def scene_rgbd_system(sc):
    """system(level, E_cur, dist_max, cos_min, r_max) of semtsdf.track.rgbd_loop over the restated words."""
    K = list(sc["p"].K)

    def system(level, E_cur, dist_max, cos_min, r_max, stride=1):
        return restate_rgbd_system(sc["pyramid"][level], sc["model"], sc["f_int"][level], sc["m_int"][level], level, K,
                                   sc["E_ref"], E_cur, dist_max, cos_min, r_max, stride)

    return system


def scene_geo_system(sc):
    """system(level, E_cur, dist_max, cos_min) of semtsdf.track.pyramid_loop on the same scene."""
    K = list(sc["p"].K)

    def system(level, E_cur, dist_max, cos_min, stride=1):
        return P.restate_system_level(sc["pyramid"][level], sc["model"], K, sc["E_ref"], E_cur, dist_max, cos_min, stride)

    return system


def scene_dims(sc):
    return [(lv["width"], lv["height"]) for lv in sc["pyramid"]]


WALL_GUESS = (0.0, 0.0, 0.0, 0.03, 0.02, 0.0)   # twist applied to the true pose: 36 mm in the plane


def wall_guess():
    from semtsdf.track import se3_apply

    return se3_apply(np.asarray(WALL_GUESS), wall_scene()["E_true"])


@functools.lru_cache(maxsize=None)
def restated_track_rgbd(scene="wall", eps=1e-5, **kw):
    """(E, log) of semtsdf.track.rgbd_loop with its defaults over the restated words: the wall from
    wall_guess(), the spheres from E_ref."""
    from semtsdf.track import rgbd_loop

    sc = wall_scene() if scene == "wall" else sphere_scene()
    E0 = wall_guess() if scene == "wall" else sc["E_ref"]
    return rgbd_loop(scene_rgbd_system(sc), scene_dims(sc), E0, eps=eps, **kw)


# ------------------------------------------------------------------------------------
# the ragged field case (icp_restatement.field_case) with a synthetic colour field
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field_colour_case():
    """field_case's params, model maps (min_weight 0, as test_icp's four-class case) and depth, with
    two u8 images [53, 75, 3]: smooth sinusoids for the model and the same pattern shifted and with
    bright patches for the frame, so that residuals fall on both sides of the gate; validity holes in
    both, on tile edges and in the last row and column.  The model's validity is synthetic like its
    colour: the view's 676 hits are too ragged for a 3 x 3 neighbourhood of them to be whole often (138
    pixels at level 0, 11 at level 1), so (m_flags & 3) == 3 would leave no class but none."""
    import model_maps_restatement as R

    p, _, _, depth = I.field_case()
    m = R.field_view(0x3, 0)[4]
    H, W = depth.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")

    def img(sx, sy):
        a = 128 + 60 * np.sin((x + sx) / 5.0) + 50 * np.cos((y + sy) / 4.0)
        return np.clip(np.rint(np.stack([a, 0.8 * a + 20, 255 - a], axis=-1)), 0, 255).astype(np.uint8)

    m_rgb, f_rgb = img(0.0, 0.0), img(1.5, -1.0)
    f_rgb[((x // 5 + y // 5) % 3) == 0] = 250
    f_valid = np.ones((H, W), np.uint8)
    f_valid[40:44, 15:17] = 0      # on a tile edge
    f_valid[-1, 30:40] = 0
    f_valid[3:9, -1] = 0
    m_valid = np.ones((H, W), np.uint8)
    m_valid[30:36, 26:31] = 0      # inside the densest hits
    m_valid[20:40, 48] = 0         # on a tile edge
    m_valid[-1, 5:25] = 0
    m_valid[10:20, -1] = 0
    return p, m, depth, m_rgb, f_rgb, f_valid, m_valid


FIELD_GATES = dict(dist_max=0.01, cos_min=0.8, r_max=0.05)


def field_inputs(level):
    """The ragged field case on pyramid level `level`: frame maps, model maps, both intensity levels."""
    p, m, depth, m_rgb, f_rgb, f_valid, m_valid = field_colour_case()
    pyr = P.restate_pyramid(depth, list(p.K), list(p.Kinv), p.depth_scale, 2, 0, 0.05, 0.02)
    f_int = restate_intensity_pyramid(f_rgb, f_valid, 2)
    m_int = restate_intensity_pyramid(m_rgb, m_valid, 2)
    return p, pyr[level], m, f_int[level], m_int[level]
