"""NumPy restatement of the depth-pyramid rules (include/semtsdf.h, "depth pyramid"): the level
geometry, the edge-preserving filter of level 0, the halving, the maps of a level and the system of
one ICP iteration with a frame grid of its own, every f32 operation once in the rule's order (fma32,
dot3 of model_maps_restatement; cross and the tracking scene of icp_restatement), plus the
coarse-to-fine loop of semtsdf.track.pyramid_loop over the restated words.
"""
import functools

import numpy as np

import icp_restatement as I
from model_maps_restatement import F, dot3, fma32, pose_camera_def

MAX_LEVELS = 4


def level_geometry(K, Kinv, W, H, nlevels):
    """[(width, height, Kinv f32 [3, 3])] of the levels: level 0 copies the handle's Kinv, the others
    are formed in float64 from K and rounded once per entry."""
    K = np.asarray(K, np.float32).reshape(4, 4).astype(np.float64)
    out = [(W, H, np.asarray(Kinv, np.float32).reshape(4, 4)[:3, :3].copy())]
    for l in range(1, nlevels):
        s = float(1 << l)
        fx, fy = K[0, 0] / s, K[1, 1] / s
        cx, cy = (K[0, 2] + 0.5) / s - 0.5, (K[1, 2] + 0.5) / s - 0.5
        m = np.array([[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]], np.float64)
        out.append((W >> l, H >> l, m.astype(np.float32)))
    return out


def spatial_terms(R):
    """{(dy, dx): us} of the taps the spatial term keeps (us > 0), in the rule's order."""
    inv_s = F(1.0) / F((R + 1) * (R + 1))
    out = {}
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            us = F(1.0) - F(dx * dx + dy * dy) * inv_s
            if us > 0:
                out[(dy, dx)] = F(us)
    return out


def restate_filter(depth, depth_scale, radius, sigma_r, stats=None):
    """Level 0 of a u16 depth image [H, W]: f32 [H, W].  stats (a dict) receives the numbers of
    neighbour visits accepted and rejected by the range term."""
    depth = np.asarray(depth, np.uint16)
    H, W = depth.shape
    zc = depth.astype(np.float32) / F(depth_scale)
    if radius == 0:
        return zc
    R = int(radius)
    inv_r = F(1.0) / F(sigma_r)
    pad = np.zeros((H + 2 * R, W + 2 * R), np.float32)   # off the image reads as raw depth 0
    pad[R:R + H, R:R + W] = zc
    has = depth != 0
    num = np.zeros((H, W), np.float32)
    den = np.zeros((H, W), np.float32)
    accepted = rejected = 0
    for (dy, dx), us in spatial_terms(R).items():
        zn = pad[R + dy:R + dy + H, R + dx:R + dx + W]
        d = zn - zc
        e = d * inv_r
        u = F(1.0) - e * e
        there = has & (zn != 0)
        take = there & (u > 0)
        w = np.where(take, (us * us) * (u * u), F(0.0)).astype(np.float32)
        num = np.where(take, fma32(w, d, num), num)
        den = np.where(take, den + w, den)
        if (dy, dx) != (0, 0):
            accepted += int(take.sum())
            rejected += int((there & ~take).sum())
    if stats is not None:
        stats.update(accepted=accepted, rejected=rejected)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(has, zc + num / den, F(0.0)).astype(np.float32)


def restate_halve(z, band, stats=None):
    """The next level of z f32 [h, w]: f32 [h >> 1, w >> 1].  stats receives the numbers of block pixels
    with depth (the first aside) inside and outside the band."""
    z = np.asarray(z, np.float32)
    h, w = z.shape[0] >> 1, z.shape[1] >> 1
    q = [z[0:2 * h:2, 0:2 * w:2], z[0:2 * h:2, 1:2 * w:2], z[1:2 * h:2, 0:2 * w:2], z[1:2 * h:2, 1:2 * w:2]]
    b = q[0]
    s = np.zeros((h, w), np.float32)
    n = np.zeros((h, w), np.float32)
    inside = outside = 0
    for k in range(4):
        d = q[k] - b
        there = (b != 0) & (q[k] != 0)
        take = there & (np.abs(d) <= F(band))
        s = np.where(take, s + d, s)
        n = np.where(take, n + F(1.0), n)
        if k:
            inside += int(take.sum())
            outside += int((there & ~take).sum())
    if stats is not None:
        stats.update(inside=inside, outside=outside)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b != 0, b + s / n, F(0.0)).astype(np.float32)


def restate_level_maps(z, Kinv3):
    """vertex, normal f32 [h, w, 3] and flags u8 [h, w] of a level: icp_restatement.restate_frame_maps'
    rule with z in place of (float)D / depth_scale and the level's 3 x 3 Kinv."""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    ki = np.asarray(Kinv3, np.float32).reshape(3, 3)
    fy, fx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    one = np.ones_like(fx)
    has = z != 0
    V = [np.where(has, dot3(ki[a, 0], ki[a, 1], ki[a, 2], fx, fy, one) * z, F(0.0)).astype(np.float32)
         for a in range(3)]
    A = [V[a][1:, :-1] - V[a][:-1, :-1] for a in range(3)]
    B = [V[a][:-1, 1:] - V[a][:-1, :-1] for a in range(3)]
    g = I.cross(A, B)
    n2 = dot3(g[0], g[1], g[2], g[0], g[1], g[2])
    ok = has[:-1, :-1] & has[1:, :-1] & has[:-1, 1:] & (n2 > 0) & np.isfinite(n2)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / np.sqrt(n2)
        n = [np.where(ok, g[a] * inv, F(0.0)).astype(np.float32) for a in range(3)]
    normal = np.zeros((H, W, 3), np.float32)
    flags = has.astype(np.uint8)
    for a in range(3):
        normal[:-1, :-1, a] = n[a]
    flags[:-1, :-1] |= ok.astype(np.uint8) << 1
    return {"vertex": np.stack(V, axis=-1), "normal": normal, "flags": flags}


def restate_pyramid(depth, K, Kinv, depth_scale, nlevels, radius, sigma_r, band, stats=None):
    """The levels of a depth image as Volume.frame_pyramid returns them: a list of dicts with width,
    height, Kinv, z, vertex, normal, flags.  stats receives the filter's and every halving's counts."""
    depth = np.asarray(depth, np.uint16)
    H, W = depth.shape
    fs, hs = {}, []
    z = restate_filter(depth, depth_scale, radius, sigma_r, fs)
    out = []
    for l, (w, h, ki) in enumerate(level_geometry(K, Kinv, W, H, nlevels)):
        if l:
            hs.append({})
            z = restate_halve(z, band, hs[-1])
        assert z.shape == (h, w)
        out.append(dict(restate_level_maps(z, ki), width=w, height=h, Kinv=ki, z=z))
    if stats is not None:
        stats.update(filter=fs, halve=hs)
    return out


restate_system_level = I.restate_system_level   # the system with a frame grid of its own: one rule, stated there


# ------------------------------------------------------------------------------------
# the tracking scene (icp_restatement.tracking_scene) through the pyramid
# ------------------------------------------------------------------------------------
SCENE_BAND = 0.05        # the halving band of the clean-depth cases (radius 0, so it has to be given)
NOISE_S = 3.0            # the noise cases: three times the sensor model


def noisy_depth(s=NOISE_S, seed=0):
    """Frame 3 of the tracking scene with Gaussian axial noise sigma(z) = s (0.0012 + 0.0019 (z - 0.4)^2)
    metres from a seeded generator, re-quantised to u16; holes stay holes."""
    sc = I.tracking_scene()
    depth = sc["frames"][3].depth
    scale = float(sc["p"].depth_scale)
    z = depth.astype(np.float64) / scale
    sigma = s * (0.0012 + 0.0019 * (z - 0.4) ** 2)
    noisy = z + np.random.default_rng(seed).standard_normal(z.shape) * sigma
    q = np.clip(np.rint(noisy * scale), 1, 65535)
    return np.where(depth != 0, q, 0).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def scene_pyramid(radius=0, sigma_r=0.05, band=SCENE_BAND, nlevels=3, noise=0.0):
    """The restated pyramid of the tracking scene's frame 3 (noise > 0: of noisy_depth(noise))."""
    sc = I.tracking_scene()
    p = sc["p"]
    depth = noisy_depth(noise) if noise else sc["frames"][3].depth
    return restate_pyramid(depth, list(p.K), list(p.Kinv), p.depth_scale, nlevels, radius, sigma_r, band)


def scene_level_system(pyramid):
    """system(level, E_cur, dist_max, cos_min) of semtsdf.track.pyramid_loop over the restated words."""
    sc = I.tracking_scene()
    K = list(sc["p"].K)

    def system(level, E_cur, dist_max, cos_min, stride=1):
        return restate_system_level(pyramid[level], sc["model"], K, sc["E_ref"], E_cur, dist_max, cos_min, stride)

    return system


def basin_guess(k):
    """Draw k of the issue's fifteen: a random twist of magnitude (2, 4, 6, 8, 12)[k // 3] times
    (0.012 rad, 33.5 mm) applied to the true extrinsic of frame 3."""
    from semtsdf.track import se3_apply

    rng = np.random.default_rng(7)
    d = [rng.standard_normal(6) for _ in range(15)]
    mag = (2, 4, 6, 8, 12)[k // 3]
    omega = d[k][:3] * 0.012 * mag / np.linalg.norm(d[k][:3])
    v = d[k][3:] * 0.0335 * mag / np.linalg.norm(d[k][3:])
    return se3_apply(np.concatenate([omega, v]), I.tracking_scene()["E_true"])


@functools.lru_cache(maxsize=None)
def restated_track_pyramid(k=None, radius=0, sigma_r=0.05, band=SCENE_BAND, eps=1e-5):
    """(E, log) of semtsdf.track.pyramid_loop with the default schedule over the restated words of the
    clean scene, from E_ref (k None) or from basin_guess(k).  TrackingLost propagates."""
    from semtsdf.track import PYRAMID_SCHEDULE, pyramid_loop

    pyr = scene_pyramid(radius, sigma_r, band)
    dims = [(lv["width"], lv["height"]) for lv in pyr]
    E0 = I.tracking_scene()["E_ref"] if k is None else basin_guess(k)
    return pyramid_loop(scene_level_system(pyr), dims, E0, PYRAMID_SCHEDULE, eps=eps)
