"""NumPy restatement of the camera-tracking rules (include/semtsdf.h, "camera tracking"): the frame
maps of a depth image and the 32 fixed-point words of one ICP iteration, every f32 operation once in
the rule's order (fma32, dot3 of model_maps_restatement), plus the tracking scene of the tests: model
maps restated on oracle state, and the loop of semtsdf.track.track_loop over the restated words.
"""
import functools

import numpy as np

from model_maps_restatement import F, KI, _oracle, dot3, pose_camera_def, restate_maps

ICP_WORDS = 32


def cross(a, b):
    """Two rounded products and one subtraction per component (no fma)."""
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def restate_frame_maps(depth, Kinv, depth_scale):
    """vertex, normal f32 [H, W, 3] and flags u8 [H, W] of a u16 depth image [H, W]."""
    depth = np.asarray(depth, np.uint16)
    H, W = depth.shape
    ki = np.asarray(Kinv, np.float32).reshape(4, 4)
    fy, fx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    one = np.ones_like(fx)
    z = depth.astype(np.float32) / F(depth_scale)
    has = depth != 0
    V = [np.where(has, dot3(ki[a, 0], ki[a, 1], ki[a, 2], fx, fy, one) * z, F(0.0)).astype(np.float32)
         for a in range(3)]
    A = [V[a][1:, :-1] - V[a][:-1, :-1] for a in range(3)]
    B = [V[a][:-1, 1:] - V[a][:-1, :-1] for a in range(3)]
    g = cross(A, B)
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


def visited_grid(frame, stride):
    """(ys, xs) of the frame pixels a stride visits, as index grids."""
    fH, fW = frame["flags"].shape
    return np.meshgrid(np.arange(0, fH, stride), np.arange(0, fW, stride), indexing="ij")


def project(frame, model, K, E_ref, E_cur, ys, xs):
    """Steps 1-2 of the rule for the frame pixels (ys, xs): (Rt, Pw, q, on, vi, ui) with Rt of E_cur,
    Pw and q = E_ref Pw as lists of three arrays, `on` where q lies in front of the reference camera and
    rounds onto the model's grid, and (vi, ui) the model pixel there (0 elsewhere)."""
    H, W = model["flags"].shape
    K = np.asarray(K, np.float32).reshape(4, 4)
    Er = np.asarray(E_ref, np.float32).reshape(4, 4)
    Ec = np.asarray(E_cur, np.float32).reshape(4, 4)
    Rt = Ec[:3, :3].T
    o = pose_camera_def(np.eye(4, dtype=np.float32).reshape(-1), Ec)[1]  # -Rt t: f64 sums rounded once
    V = [frame["vertex"][ys, xs, a] for a in range(3)]
    with np.errstate(all="ignore"):
        Pw = [dot3(Rt[a, 0], Rt[a, 1], Rt[a, 2], V[0], V[1], V[2]) + o[a] for a in range(3)]
        q = [dot3(Er[a, 0], Er[a, 1], Er[a, 2], Pw[0], Pw[1], Pw[2]) + Er[a, 3] for a in range(3)]
        s = [dot3(K[a, 0], K[a, 1], K[a, 2], q[0], q[1], q[2]) for a in range(3)]
        u = np.floor(s[0] / s[2] + F(0.5))
        v = np.floor(s[1] / s[2] + F(0.5))
        on = ~(q[2] <= 0) & (u >= 0) & (u < F(W)) & (v >= 0) & (v < F(H))
    ui = np.where(on, u, 0).astype(np.int64)
    vi = np.where(on, v, 0).astype(np.int64)
    return Rt, Pw, q, on, vi, ui


def pack_words(J, r, inl, far, third, visited, scale):
    """The 32 int64 words of a system: the sums of RN(x y scale) over the inliers, x y formed in
    float64, in the order J^T J (upper triangle, row-major), J^T r, r r; then the counts of inliers, far,
    the third class (angle or outlier) and none = visited less those three."""
    words = np.zeros(ICP_WORDS, np.int64)
    t = [j[inl].astype(np.float64) for j in J] + [r[inl].astype(np.float64)]

    def fix(a, b):
        return int(np.rint(a * b * scale).astype(np.int64).sum())

    w = 0
    for i in range(6):
        for j in range(i, 6):
            words[w] = fix(t[i], t[j])
            w += 1
    for i in range(7):
        words[21 + i] = fix(t[i], t[6])
    words[28] = int(inl.sum())
    words[29] = int(far.sum())
    words[30] = int(third.sum())
    words[31] = int(visited) - int(words[28] + words[29] + words[30])
    return words


def restate_system_level(frame, model, K, E_ref, E_cur, dist_max, cos_min, stride):
    """The 32 int64 words from the frame maps, the model maps (point, normal, flags), the handle's K
    (16 values) and the two extrinsics, on two grids: the visited pixels and the frame maps' shape are
    the frame's, the projection's bounds and the looked-up maps the model's (the handle's W x H)."""
    dmax2 = F(dist_max) * F(dist_max)
    ys, xs = visited_grid(frame, stride)
    vis = (frame["flags"][ys, xs] & 3) == 3
    ys, xs = ys[vis], xs[vis]
    Rt, Pw, _, on, vi, ui = project(frame, model, K, E_ref, E_cur, ys, xs)
    n = [frame["normal"][ys, xs, a] for a in range(3)]
    with np.errstate(all="ignore"):
        Nw = [dot3(Rt[a, 0], Rt[a, 1], Rt[a, 2], n[0], n[1], n[2]) for a in range(3)]
        on = on & ((model["flags"][vi, ui] & 3) == 3)
        Pm = [model["point"][vi, ui, a] for a in range(3)]
        Nm = [model["normal"][vi, ui, a] for a in range(3)]
        d = [Pm[a] - Pw[a] for a in range(3)]
        far = on & (dot3(d[0], d[1], d[2], d[0], d[1], d[2]) > dmax2)
        angle = on & ~far & (dot3(Nm[0], Nm[1], Nm[2], Nw[0], Nw[1], Nw[2]) < F(cos_min))
        r = dot3(Nm[0], Nm[1], Nm[2], d[0], d[1], d[2])
        J = cross(Pw, Nm) + Nm
        inl = on & ~far & ~angle
        for k in range(6):
            inl &= np.abs(J[k]) < F(32.0)
    return pack_words(J, r, inl, far, angle, vis.sum(), 4294967296.0)


def restate_system(frame, model, K, E_ref, E_cur, dist_max, cos_min, stride):
    """restate_system_level with the frame maps on the model's own grid."""
    assert frame["flags"].shape == model["flags"].shape
    return restate_system_level(frame, model, K, E_ref, E_cur, dist_max, cos_min, stride)


# ------------------------------------------------------------------------------------
# the tracking scene, built once per process
# ------------------------------------------------------------------------------------
TRACK_DIM = 128
TRACK_GATES = dict(dist_max=0.1, cos_min=0.8, stride=1)


@functools.lru_cache(maxsize=None)
def tracking_scene():
    """128^3, flags 0x3, 640 x 480; SyntheticStream(seed=0) at three times its default motion, placed
    from frame 0, frames 1 and 2 integrated by the oracle; frame 3 is tracked with E_ref = E0 = frame
    2's extrinsic.  Holds the oracle state, the restated model maps of E_ref and the restated frame
    maps of frame 3."""
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream

    O = _oracle()
    st = SyntheticStream(seed=0, yaw_step=0.012, trans_step=(0.03, 0, 0.015))
    frames = [st.frame(k) for k in range(4)]
    p = semtsdf.default_params(TRACK_DIM, KI, 640, 480)
    dist = float(np.mean(frames[0].depth[frames[0].depth > 0])) / 5000.0
    semtsdf.place_from_frame(p, frames[0].depth, dist, L.PLACE_SFM)
    p.flags = 0x3
    g = O.OGeom.from_params(p)
    D = (TRACK_DIM,) * 3
    ost = O.OState(list(D), p.mu, semantic=True)
    Es = [(fr.w2c @ frames[0].c2w).astype(np.float32) for fr in frames]
    for k in (1, 2):
        fr = frames[k]
        O.integrate(g, ost, list(p.K), Es[k], fr.depth, fr.rgb, fr.gt_ids, flags=0x3)
    s2w, c = pose_camera_def(list(p.Kinv), Es[2])
    _, t = O.render(g, s2w, c, p.width, p.height, 0, ost.sdf, ost.hist)
    model = restate_maps(t, s2w, c, ost.sdf.reshape(D), ost.wt.reshape(D), None, list(p.vol_start), list(p.voxel), 1)
    frame = restate_frame_maps(frames[3].depth, list(p.Kinv), p.depth_scale)
    return {"p": p, "frames": frames, "E": Es, "E_ref": Es[2], "E_true": Es[3], "model": model, "frame": frame}


def scene_system(E_cur):
    sc = tracking_scene()
    return restate_system(sc["frame"], sc["model"], list(sc["p"].K), sc["E_ref"], E_cur, **TRACK_GATES)


@functools.lru_cache(maxsize=None)
def restated_track():
    """(E, log) of semtsdf.track.track_loop over the restated words: 10 iterations from E0 = E_ref
    (eps = 0: no early stop), with track()'s default min_inliers."""
    from semtsdf.track import default_min_inliers, track_loop

    sc = tracking_scene()
    return track_loop(scene_system, sc["E_ref"], 10, default_min_inliers(640, 480, 1), eps=0.0)


# ------------------------------------------------------------------------------------
# the ragged field view (model_maps_restatement.field_view) as an ICP problem
# ------------------------------------------------------------------------------------
FIELD_GATES = dict(dist_max=0.01, cos_min=0.8)


def field_offset():
    """E_cur of the field case: a small rotation and translation away from E_ref = identity."""
    from semtsdf.track import se3_apply

    return se3_apply([0.004, -0.006, 0.01, 0.004, -0.003, 0.006], np.eye(4, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def field_case():
    """(params, field, model maps, depth u16 [53, 75]) of field_view(0x3, 1): the depth is the view's
    own z (camera = volume frame) re-quantised to raw units, with zero-depth holes on a tile edge
    (column 16, row 32) and in the last row and column."""
    import model_maps_restatement as R

    p, f, _, _, m = R.field_view(0x3, 1)
    z = m["point"][..., 2].astype(np.float64)
    hit = (m["flags"] & 1) != 0
    depth = np.where(hit, np.rint(z * p.depth_scale), 0).astype(np.uint16)
    depth[5:20, 16] = 0
    depth[32, 40:60] = 0
    depth[-1, 10:30] = 0
    depth[20:30, -1] = 0
    return p, f, m, depth
