"""Camera tracking against the fused model: frame-to-model point-to-plane ICP.

The device does the per-pixel work (include/semtsdf.h, "camera tracking"): the model maps of a
reference view (semtsdf_render_maps_dev), the frame maps of the depth image
(semtsdf_frame_maps_dev) and, per iteration, the normal equations as 32 fixed-point int64 words
(semtsdf_icp_system_dev).  This module is the host side, NumPy float64 like pose.py: it scales the
words back, solves the 6 x 6 system and moves the pose.  track_pyramid runs the same loop coarse to
fine on the depth pyramid (include/semtsdf.h, "depth pyramid": semtsdf_frame_pyramid_dev,
semtsdf_icp_system_level_dev) against the one full-resolution render of the model, and track_rgbd
adds a photometric term between the frame's colour image and the model's colour render
(include/semtsdf.h, "RGB-D tracking": semtsdf_intensity_pyramid_dev, semtsdf_rgbd_system_level_dev),
whose row J = (Pw x aw, aw) follows the same convention: r - J xi is the intensity residual after the step.

Conventions.  E is the integrate's extrinsic: volume frame to camera, so C2W = E^-1 is the camera's
pose in the volume frame.  A step is a twist xi = (omega, v) of the volume frame:
C2W <- exp(xi) C2W.  The residual of a pixel is r = Nm . (Pm - Pw) and its row J = (Pw x Nm, Nm), so
r - J xi is the residual after the step to first order, and xi solves (J^T J) xi = J^T r.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np

from . import _lib as L

SCALE = 2.0 ** -32          # one unit of the fixed-point sums
PHOTO_SCALE = 2.0 ** -20    # one unit of the photometric sums
SMALL_ANGLE = 1e-2          # |omega| below which exp() uses its series
STEP_EPS = 1e-5             # |xi| (radians and metres together) below which the loop stops
COUNT_NAMES = ("inliers", "far", "angle", "none")
PHOTO_COUNT_NAMES = ("inliers", "far", "outlier", "none")
PHOTO_WEIGHT = 0.02         # metres per unit of intensity (the sweep that chose it)
R_MAX = 0.25                # the gate on the intensity residual, intensities in [0, 1)


class TrackingLost(RuntimeError):
    """Too few inliers to trust a step.  `E` is the estimate the loop had reached (f32 extrinsic),
    `log` its per-iteration log up to and including the failing iteration."""

    def __init__(self, msg, E, log):
        super().__init__(msg)
        self.E = E
        self.log = log


def _unpack(words, scale, names):
    """(A, b, r2, counts) of one 32-word block: the symmetric 6 x 6 A = J^T J, b = J^T r and
    r2 = sum r^2 scaled back (float64), and the four class counts as a dict of ints under `names`."""
    w = np.asarray(words, np.int64).reshape(L.ICP_WORDS)
    A = np.zeros((6, 6), np.float64)
    iu = np.triu_indices(6)  # row-major upper triangle: the word order
    A[iu] = w[:21].astype(np.float64) * scale
    A = A + np.triu(A, 1).T
    b = w[21:27].astype(np.float64) * scale
    counts = {n: int(w[28 + k]) for k, n in enumerate(names)}
    return A, b, float(w[27]) * scale, counts


def system_from_words(words):
    """(A, b, r2, counts) of the 32 int64 words: the point-to-plane system scaled back by 2^-32
    (metres), counts inliers, far, angle, none."""
    return _unpack(words, SCALE, COUNT_NAMES)


def rgbd_system_from_words(words):
    """Two (A, b, r2, counts) tuples of the 64 int64 words: the point-to-plane system as
    system_from_words returns it and the photometric one (scale 2^-20, units of intensity; counts
    inliers, far, outlier, none)."""
    w = np.asarray(words, np.int64).reshape(L.RGBD_WORDS)
    return system_from_words(w[:L.ICP_WORDS]), _unpack(w[L.ICP_WORDS:], PHOTO_SCALE, PHOTO_COUNT_NAMES)


def solve_step(A, b):
    """xi of A xi = b (np.linalg.solve); raises numpy.linalg.LinAlgError on a singular or
    non-finite system."""
    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        raise np.linalg.LinAlgError("non-finite system")
    return np.linalg.solve(A, b)


def se3_exp(xi):
    """The 4 x 4 rigid motion exp(xi) of a twist xi = (omega, v), float64: R = I + a K + b K^2 (Rodrigues)
    and t = (I + b K + c K^2) v with K = [omega]x, th = |omega|, a = sin th / th,
    b = (1 - cos th) / th^2 = 2 sin^2(th / 2) / th^2, c = (th - sin th) / th^3.  Below th = SMALL_ANGLE
    the series a = 1 - th^2/6 + th^4/120, b = 1/2 - th^2/24 + th^4/720, c = 1/6 - th^2/120 + th^4/5040,
    whose truncation error is below 2e-16 there; above it the cancellation in th - sin th costs c at most
    6 eps / th^2 < 2e-11 of its value, which reaches t only through K^2 (th^2)."""
    xi = np.asarray(xi, np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    K2 = K @ K
    th = math.sqrt(float(w @ w))
    t2 = th * th
    if th < SMALL_ANGLE:
        a = 1.0 - t2 / 6.0 + t2 * t2 / 120.0
        b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0
        c = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0
    else:
        h = math.sin(0.5 * th)
        a, b, c = math.sin(th) / th, 2.0 * h * h / t2, (th - math.sin(th)) / (t2 * th)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * K2
    T[:3, 3] = (np.eye(3) + b * K + c * K2) @ v
    return T


def se3_apply(xi, E):
    """The extrinsic after the step xi: C2W_new = exp(xi) C2W with C2W = E^-1, inverted again and
    rounded once to float32."""
    c2w = np.linalg.inv(np.asarray(E, np.float64).reshape(4, 4))
    return np.linalg.inv(se3_exp(xi) @ c2w).astype(np.float32)


def default_min_inliers(width, height, stride):
    """1 % of the pixels a stride visits at most (at least 6: the unknowns)."""
    return max(6, (((width - 1) // stride + 1) * ((height - 1) // stride + 1)) // 100)


# (level, max iterations, dist_max, cos_min), coarse first: the gates open where the smoothed coarse
# normals can bear it and close again at full resolution
PYRAMID_SCHEDULE = ((2, 4, 0.3, 0.6), (1, 5, 0.2, 0.7), (0, 10, 0.1, 0.8))


def _loop(system, schedule, need_of, E0, eps, w2=None):
    """The loop of all three trackers.  Each (level, iters, dist_max, cos_min) entry of `schedule` runs at
    most `iters` iterations from the previous entry's result, needing need_of(level) inliers:
    system(level, E_cur, dist_max, cos_min) -> words, solve, step, stop below eps.  level None: one
    untagged entry, whose log entries carry no `level` and whose TrackingLost messages no prefix.
    w2 None: 32 words; else 64, and the photometric system joins with weight w2 where it has the
    needed inliers itself."""
    E = np.asarray(E0, np.float32).reshape(4, 4).copy()
    log = []
    for level, iters, dist_max, cos_min in schedule:
        need = need_of(level)
        where = "" if level is None else f"level {level}: "
        for it in range(int(iters)):
            words = system(level, E, dist_max, cos_min)
            if w2 is None:
                A, b, r2, counts = system_from_words(words)
            else:
                (A, b, r2, counts), (Ap, bp, rp2, pc) = rgbd_system_from_words(words)
            n = counts["inliers"]
            entry = dict(counts, iter=it, rms=math.sqrt(r2 / n) if n else float("nan"), step=float("nan"))
            if level is not None:
                entry["level"] = level
            if w2 is not None:
                m = pc["inliers"]
                used = m >= need and w2 > 0.0
                entry.update(photo_inliers=m, photo_rms=math.sqrt(rp2 / m) if m else float("nan"), photo_used=used)
                if used:
                    A, b = A + w2 * Ap, b + w2 * bp
            log.append(entry)
            if n < need:
                raise TrackingLost(f"{where}iteration {it}: {n} inliers, fewer than {need}", E, log)
            try:
                xi = solve_step(A, b)
            except np.linalg.LinAlgError as e:
                raise TrackingLost(f"{where}iteration {it}: {e}", E, log) from e
            entry["step"] = float(np.linalg.norm(xi))
            E = se3_apply(xi, E)
            if entry["step"] < eps:
                break
    return E, log


def _levels(schedule, dims, stride, min_inliers):
    """(schedule with int levels, need_of) of a coarse-to-fine loop: default_min_inliers of a level's
    grid dims[level] = (width, height) unless min_inliers is given."""
    def need_of(level):
        w, h = dims[level]
        return default_min_inliers(w, h, int(stride)) if min_inliers is None else min_inliers

    return [(int(level), iters, dist_max, cos_min) for level, iters, dist_max, cos_min in schedule], need_of


def track_loop(system, E0, iters=10, min_inliers=6, eps=STEP_EPS):
    """The ICP loop over any source of the words: system(E_cur) -> 32 int64 words.  Returns
    (E, log): the f32 extrinsic after at most `iters` steps (fewer when a step's |xi| falls below
    eps) and one dict per iteration with the four counts, rms = sqrt(sum r^2 / inliers) before the
    step and step = |xi|.  Raises TrackingLost (estimate and log kept) when an iteration finds
    fewer than min_inliers inliers, or its system cannot be solved."""
    return _loop(lambda _level, E, _dist_max, _cos_min: system(E), ((None, iters, None, None),),
                 lambda _level: min_inliers, E0, eps)


def pyramid_loop(system, dims, E0, schedule=PYRAMID_SCHEDULE, stride=1, min_inliers=None, eps=STEP_EPS):
    """The coarse-to-fine loop over any source of the words: system(level, E_cur, dist_max,
    cos_min) -> 32 int64 words, `dims[level]` = (width, height) of that level's frame grid.  Each
    schedule entry runs track_loop's iterations from the previous entry's result, with
    default_min_inliers of its level's grid unless min_inliers is given.  Returns (E, log); every log
    entry carries its `level`.  TrackingLost carries the estimate reached and the log of all levels so
    far, its message the level."""
    return _loop(system, *_levels(schedule, dims, stride, min_inliers), E0, eps)


def rgbd_loop(system, dims, E0, schedule=PYRAMID_SCHEDULE, photo_weight=PHOTO_WEIGHT, r_max=R_MAX, stride=1,
              min_inliers=None, eps=STEP_EPS):
    """pyramid_loop with the photometric term: system(level, E_cur, dist_max, cos_min, r_max) -> 64
    int64 words.  Each iteration solves (A_g + w^2 A_p) xi = b_g + w^2 b_p with w = photo_weight; a
    photometric system with fewer than the level's min_inliers inliers is left out of that iteration
    (photo_used False in its log entry).  The step, the stop rule and TrackingLost (on the geometric
    inliers alone) are track_loop's.  Log entries are pyramid_loop's plus photo_inliers, photo_rms
    (intensity units, before the step) and photo_used."""
    return _loop(lambda level, E, dist_max, cos_min: system(level, E, dist_max, cos_min, r_max),
                 *_levels(schedule, dims, stride, min_inliers), E0, eps, w2=float(photo_weight) ** 2)


@contextlib.contextmanager
def _device_frame(vol, depth, E_ref, min_weight, sizes, nwords, after_model=None):
    """The device side that every tracker sets up once per frame, as a context: the buffers named in
    `sizes` (bytes) beside depth, the three model maps and `nwords` int64 words; the model maps rendered
    at pose_camera(Kinv, E_ref) (min_weight: their validity threshold); after_model(bufs, s2w, c) if
    given; the depth (u16, contiguous) uploaded.  Yields (bufs, read_words): the DeviceBuffer table and
    a function that copies the words into one host array, waits and returns it.  On the way out, also
    when an allocation fails half way, it waits for the volume's stream and frees every buffer."""
    from .maps import pose_camera
    from .volume import DeviceBuffer

    n = vol.W * vol.H
    s2w, c = pose_camera(list(vol.params.Kinv), E_ref)
    stream = C.c_void_p(vol.stream)
    sizes = dict({"depth": 2 * n, "m_point": 12 * n, "m_normal": 12 * n, "m_flags": n, "words": 8 * nwords}, **sizes)
    bufs = {}
    try:
        for k, size in sizes.items():
            bufs[k] = DeviceBuffer(size)
        vol.render_maps_dev(s2w, c, int(min_weight), point=bufs["m_point"].ptr, normal=bufs["m_normal"].ptr,
                            flags=bufs["m_flags"].ptr)
        if after_model is not None:
            after_model(bufs, s2w, c)
        bufs["depth"].upload(depth, stream)
        words = np.zeros(nwords, np.int64)

        def read_words():
            bufs["words"].download(words, stream)
            vol.sync()
            return words

        yield bufs, read_words
    finally:
        vol.sync()
        for b in bufs.values():
            b.free()


def _level_sizes(geo, per):
    """{name + level: bytes} of per-pixel buffers on every level of frame_levels' geometry."""
    return {f"{k}{l}": size * g["width"] * g["height"] for l, g in enumerate(geo) for k, size in per.items()}


def _level_pointers(bufs, names, level, keys=None):
    """The raw pointers of one level's buffers, as a list or under `keys`."""
    ptrs = [bufs[f"{k}{level}"].ptr for k in names]
    return dict(zip(keys, ptrs)) if keys else ptrs


_LEVEL_MAPS = {"z": 4, "vertex": 12, "normal": 12, "flags": 1}     # bytes per pixel of a depth-pyramid level
_LEVEL_INTENSITIES = {"fS": 4, "fV": 1, "mS": 4, "mV": 1}         # and of the two intensity pyramids' level
_MODEL = ("m_point", "m_normal", "m_flags")


def _pyramid_args(vol, schedule):
    """(schedule as tuples, number of levels its coarsest entry needs, their geometry)."""
    schedule = tuple(tuple(s) for s in schedule)
    if not schedule or min(int(s[0]) for s in schedule) < 0:
        raise ValueError("schedule: (level, iterations, dist_max, cos_min) entries with level >= 0")
    nlevels = max(int(s[0]) for s in schedule) + 1
    return schedule, nlevels, vol.frame_levels(nlevels)


def track(vol, depth, E_ref, E0, iters=10, dist_max=0.1, cos_min=0.8, stride=1, min_weight=1, min_inliers=None,
          eps=STEP_EPS):
    """Tracks the depth image (u16 [H, W]) against the model in `vol`, starting from the extrinsic
    E0.  The model maps are rendered once at pose_camera(Kinv, E_ref) (min_weight: the maps'
    validity threshold) and stay on the device, as do the frame maps; each iteration is one
    launch and a 256-byte read-back.  min_inliers defaults to default_min_inliers.  Returns
    (E, log) as track_loop does, and raises TrackingLost like it."""
    d = np.ascontiguousarray(depth, dtype=np.uint16)
    n = vol.W * vol.H
    if d.size != n:
        raise ValueError(f"depth must be {vol.H}x{vol.W} u16")
    if min_inliers is None:
        min_inliers = default_min_inliers(vol.W, vol.H, int(stride))
    E_ref = L.f32(E_ref, 16)
    with _device_frame(vol, d, E_ref, min_weight, {"vertex": 12 * n, "normal": 12 * n, "flags": n},
                       L.ICP_WORDS) as (bufs, read_words):
        vol.frame_maps_dev(bufs["depth"].ptr, bufs["vertex"].ptr, bufs["normal"].ptr, bufs["flags"].ptr)
        pointers = [bufs[k].ptr for k in ("vertex", "normal", "flags") + _MODEL]

        def system(E):
            vol.icp_system_dev(pointers, E_ref, E, dist_max, cos_min, stride, bufs["words"].ptr)
            return read_words()

        return track_loop(system, E0, iters, min_inliers, eps)


def track_pyramid(vol, depth, E_ref, E0, schedule=PYRAMID_SCHEDULE, radius=3, sigma_r=0.05, band=None, stride=1,
                  min_weight=1, min_inliers=None, eps=STEP_EPS):
    """track() coarse to fine on the depth pyramid (Volume.frame_pyramid_dev: the edge-preserving
    filter of `radius`, `sigma_r`, halvings within `band`).  The model maps are rendered once at full
    resolution and the pyramid is built once, as many levels as the schedule's coarsest entry needs;
    everything stays on the device and each iteration is one launch (icp_system_level_dev) and a
    256-byte read-back.  Returns (E, log) as pyramid_loop does, and raises TrackingLost like it."""
    d = np.ascontiguousarray(depth, dtype=np.uint16)
    if d.size != vol.W * vol.H:
        raise ValueError(f"depth must be {vol.H}x{vol.W} u16")
    schedule, nlevels, geo = _pyramid_args(vol, schedule)
    E_ref = L.f32(E_ref, 16)
    with _device_frame(vol, d, E_ref, min_weight, _level_sizes(geo, _LEVEL_MAPS), L.ICP_WORDS) as (bufs, read_words):
        vol.frame_pyramid_dev(bufs["depth"].ptr, [_level_pointers(bufs, _LEVEL_MAPS, l, _LEVEL_MAPS) for l in range(nlevels)],
                              radius, sigma_r, band)
        model = [bufs[k].ptr for k in _MODEL]

        def system(level, E, dist_max, cos_min):
            frame = _level_pointers(bufs, ("vertex", "normal", "flags"), level)
            vol.icp_system_level_dev(frame + model, geo[level]["width"], geo[level]["height"], E_ref, E, dist_max,
                                     cos_min, stride, bufs["words"].ptr)
            return read_words()

        dims = [(g["width"], g["height"]) for g in geo]
        return pyramid_loop(system, dims, E0, schedule, stride, min_inliers, eps)


def track_rgbd(vol, depth, rgb, E_ref, E0, schedule=PYRAMID_SCHEDULE, photo_weight=PHOTO_WEIGHT, r_max=R_MAX, radius=3,
               sigma_r=0.05, band=None, stride=1, min_weight=1, min_inliers=None, eps=STEP_EPS):
    """track_pyramid with a photometric term between the frame's colour image `rgb` (u8 [H, W, 3]) and
    the colour render of the model.  Once: the model maps and the colour raycast at
    pose_camera(Kinv, E_ref), the depth pyramid, and the intensity pyramids of the frame and of the
    render (valid where the model flags are 3); then per iteration one launch
    (Volume.rgbd_system_level_dev) and a 512-byte read-back.  Returns (E, log) as rgbd_loop does, and
    raises TrackingLost like it."""
    d = np.ascontiguousarray(depth, dtype=np.uint16)
    c = np.ascontiguousarray(rgb, dtype=np.uint8)
    n = vol.W * vol.H
    if d.size != n or c.size != 3 * n:
        raise ValueError(f"depth must be {vol.H}x{vol.W} u16 and rgb {vol.H}x{vol.W}x3 u8")
    schedule, nlevels, geo = _pyramid_args(vol, schedule)
    E_ref = L.f32(E_ref, 16)
    stream = C.c_void_p(vol.stream)

    m_flags = np.zeros(n, np.uint8)
    m_valid = np.zeros(n, np.uint8)   # lives as long as the call: its upload is asynchronous

    def colour_render(bufs, s2w, cam):
        vol.raycast_dev(s2w, cam, L.RENDER_COLOR, bufs["m_rgb"].ptr, stream=stream)
        bufs["m_flags"].download(m_flags, stream)   # the one read-back before the loop: valid = (m_flags & 3) == 3
        vol.sync()
        m_valid[:] = (m_flags & 3) == 3
        bufs["m_valid"].upload(m_valid, stream)

    sizes = dict({"rgb": 3 * n, "m_rgb": 3 * n, "m_valid": n}, **_level_sizes(geo, {**_LEVEL_MAPS, **_LEVEL_INTENSITIES}))
    with _device_frame(vol, d, E_ref, min_weight, sizes, L.RGBD_WORDS, colour_render) as (bufs, read_words):
        bufs["rgb"].upload(c, stream)
        vol.frame_pyramid_dev(bufs["depth"].ptr, [_level_pointers(bufs, _LEVEL_MAPS, l, _LEVEL_MAPS) for l in range(nlevels)],
                              radius, sigma_r, band)
        for image, valid, names in ((bufs["rgb"].ptr, None, ("fS", "fV")), (bufs["m_rgb"].ptr, bufs["m_valid"].ptr, ("mS", "mV"))):
            vol.intensity_pyramid_dev(image, valid, [_level_pointers(bufs, names, l, ("S", "valid")) for l in range(nlevels)])
        model = [bufs[k].ptr for k in _MODEL]

        def system(level, E, dist_max, cos_min, r_max):
            frame = _level_pointers(bufs, ("vertex", "normal", "flags"), level)
            photo = _level_pointers(bufs, _LEVEL_INTENSITIES, level)
            vol.rgbd_system_level_dev(frame + model, photo, level, E_ref, E, dist_max, cos_min, r_max, stride,
                                      bufs["words"].ptr)
            return read_words()

        dims = [(g["width"], g["height"]) for g in geo]
        return rgbd_loop(system, dims, E0, schedule, photo_weight, r_max, stride, min_inliers, eps)


def pose_errors(E, E_true):
    """(translation error in metres, rotation angle in radians) between two extrinsics, measured
    on the camera poses C2W = E^-1."""
    a = np.linalg.inv(np.asarray(E, np.float64).reshape(4, 4))
    b = np.linalg.inv(np.asarray(E_true, np.float64).reshape(4, 4))
    dR = a[:3, :3].T @ b[:3, :3]
    ang = math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1.0) / 2.0)))
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), ang


__all__ = ["TrackingLost", "system_from_words", "solve_step", "se3_exp", "se3_apply", "track_loop", "track",
           "pose_errors", "default_min_inliers", "STEP_EPS", "PYRAMID_SCHEDULE", "pyramid_loop", "track_pyramid",
           "rgbd_system_from_words", "rgbd_loop", "track_rgbd", "PHOTO_WEIGHT", "R_MAX"]
