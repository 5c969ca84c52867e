"""NumPy restatement of the model-maps rule (include/semtsdf.h, "model maps of a view"), for the
tests: every f32 operation of the rule once, in the rule's order, on reference-layout arrays
([Dx, Dy, Dz] row-major).  The hit distance t is taken from the C oracle's render, which is bit-equal
to the device's march; everything after the march is restated here.

f32 +, -, *, /, sqrt are correctly rounded in NumPy.  The fused multiply-add is done in f64: the
product of two f32 values is exact in f64, the one f64 add is rounded, its error is recovered with
TwoSum, and where the f64 sum sits exactly on an f32 tie (the midpoint of two neighbouring f32
values) with a nonzero error, the sum is moved one f64 ulp towards the error's sign before the final
rounding to f32 -- that is the only case in which rounding twice differs from rounding once.
"""
import functools

import numpy as np

F = np.float32
KI = (520.9, 521.0, 325.1, 249.7)


def fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays (broadcast), exactly."""
    a64, b64, c64 = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a64 * b64                      # exact: 24 x 24 bits
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)  # TwoSum: p + c64 == s + err exactly
        r = s.astype(np.float32)
        d = s - r.astype(np.float64)       # exact
        toward = np.where(d > 0, np.float32(np.inf), np.float32(-np.inf))
        other = np.nextafter(r, toward).astype(np.float64)
        tie = (d != 0) & np.isfinite(s) & np.isfinite(other) & ((other - s) == d)
        fix = tie & (err != 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def dot3(a0, a1, a2, b0, b1, b2):
    return fma32(a2, b2, fma32(a1, b1, F(a0) * F(b0)))


def mix(a, b, t):
    return fma32(t, b, (F(1.0) - t) * a)


def rays(s2w, c, W, H):
    """(o [3], d [H, W, 3]) of the render camera."""
    s = np.asarray(s2w, np.float32).reshape(4, 4)
    c = np.asarray(c, np.float32).reshape(3)
    fy, fx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    one = np.ones_like(fx)
    r = [dot3(s[i, 0], s[i, 1], s[i, 2], fx, fy, one) + s[i, 3] - c[i] for i in range(3)]
    inv = F(1.0) / np.sqrt(dot3(r[0], r[1], r[2], r[0], r[1], r[2]))
    return c, np.stack([r[i] * inv for i in range(3)], axis=-1)


class Tri:
    """The clamped trilinear sample at points p [N, 3]: corner indices and fractions."""

    def __init__(self, p, start, voxel, dims):
        self.f, self.i0, self.i1 = [], [], []
        for a in range(3):
            i = (p[:, a] - F(start[a])) / F(voxel[a])
            fl = np.floor(i)
            self.f.append(i - fl)
            k = fl.astype(np.int64)
            self.i0.append(np.clip(k, 0, dims[a] - 1))
            self.i1.append(np.clip(k + 1, 0, dims[a] - 1))

    def corners(self, vol):
        """vol[x + i, y + j, z + k] as d[i][j][k], each [N]."""
        ix = (self.i0, self.i1)
        return [[[vol[ix[i][0], ix[j][1], ix[k][2]] for k in range(2)] for j in range(2)] for i in range(2)]

    def eval(self, vol):
        d = self.corners(vol)
        d = [[[np.asarray(d[i][j][k]).astype(np.float32) for k in range(2)] for j in range(2)] for i in range(2)]
        fx, fy, fz = self.f
        low = mix(mix(d[0][0][0], d[1][0][0], fx), mix(d[0][1][0], d[1][1][0], fx), fy)
        high = mix(mix(d[0][0][1], d[1][0][1], fx), mix(d[0][1][1], d[1][1][1], fx), fy)
        return mix(low, high, fz)

    def min_corner(self, vol):
        d = self.corners(vol)
        return np.minimum.reduce([d[i][j][k] for i in range(2) for j in range(2) for k in range(2)])


def restate_maps(t, s2w, c, sdf, wt, hist, start, voxel, min_weight):
    """The six maps from the hit distances t [H, W] (-1: miss) and the volume arrays sdf, wt
    [Dx, Dy, Dz], hist [Dx, Dy, Dz, 32] or None (then no label, votes)."""
    H, W = t.shape
    dims = sdf.shape
    voxel = np.asarray(voxel, np.float32)
    o, d = rays(s2w, c, W, H)
    hit = t >= 0
    out = {"t": np.where(hit, t, F(-1.0)).astype(np.float32), "point": np.zeros((H, W, 3), np.float32),
           "normal": np.zeros((H, W, 3), np.float32), "flags": hit.astype(np.uint8)}
    th = t[hit]
    P = np.stack([fma32(th, d[..., a][hit], o[a]) for a in range(3)], axis=-1)
    out["point"][hit] = P
    if hist is not None:
        tr = Tri(P, start, voxel, dims)
        votes = np.zeros(len(th), np.float32)
        label = np.zeros(len(th), np.uint8)
        for k in range(32):  # ascending bins, strict >
            hk = hist[..., k]
            if not hk.any():
                continue  # every sample of the bin is a mix of zeros: 0, never a strict maximum
            v = tr.eval(hk)
            better = v > votes
            votes = np.where(better, v, votes)
            label = np.where(better, np.uint8(k), label)
        out["votes"] = np.zeros((H, W), np.float32)
        out["label"] = np.zeros((H, W), np.uint8)
        out["votes"][hit] = votes
        out["label"][hit] = label
    wmin = np.full(len(th), np.iinfo(np.int32).max, np.int64)
    g = []
    for a in range(3):
        s = []
        for sign in (1, -1):
            Q = P.copy()
            Q[:, a] = P[:, a] + voxel[a] if sign > 0 else P[:, a] - voxel[a]
            tr = Tri(Q, start, voxel, dims)
            s.append(tr.eval(sdf))
            wmin = np.minimum(wmin, tr.min_corner(wt))
        g.append((s[0] - s[1]) / (voxel[a] + voxel[a]))
    n2 = dot3(g[0], g[1], g[2], g[0], g[1], g[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / np.sqrt(n2)
        n = np.stack([g[a] * inv for a in range(3)], axis=-1).astype(np.float32)
    out["_hit"], out["_wmin"], out["_n"], out["_n2ok"] = hit, wmin, n, (n2 > 0) & np.isfinite(n2)
    return with_min_weight(out, min_weight)


def with_min_weight(core, min_weight):
    """The maps of restate_maps' result at another min_weight (only normal and flags depend on it)."""
    out = {k: (v.copy() if k in ("normal", "flags") else v) for k, v in core.items()}
    hit = core["_hit"]
    ok = (core["_wmin"] >= min_weight) & core["_n2ok"]
    out["normal"][hit] = np.where(ok[:, None], core["_n"], F(0.0))
    out["flags"][hit] = np.uint8(1) | (ok.astype(np.uint8) << 1)
    return out


# ------------------------------------------------------------------------------------
# the two configurations of the tests, built once per process
# ------------------------------------------------------------------------------------
def _oracle():
    import oracle as O

    O.build()
    return O


@functools.lru_cache(maxsize=None)
def fused_scene():
    """64^3, SyntheticStream(seed=0) placed from frame 0, frames 1-3 integrated with gt_ids, flags 0x3,
    640 x 480 (the configuration of test_render_matches_oracle), as oracle state."""
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream

    O = _oracle()
    st = SyntheticStream(seed=0)
    frames = [st.frame(k) for k in range(4)]
    p = semtsdf.default_params(64, KI, 640, 480)
    dist = float(np.mean(frames[0].depth[frames[0].depth > 0])) / 5000.0
    semtsdf.place_from_frame(p, frames[0].depth, dist, L.PLACE_SFM)
    p.flags = 0x3
    g = O.OGeom.from_params(p)
    ost = O.OState([64, 64, 64], p.mu, semantic=True)
    Es = [None]
    for k in range(1, 4):
        fr = frames[k]
        E = (fr.w2c @ frames[0].c2w).astype(np.float32)
        Es.append(E)
        O.integrate(g, ost, list(p.K), E, fr.depth, fr.rgb, fr.gt_ids, flags=0x3)
    return {"p": p, "g": g, "ost": ost, "frames": frames, "E": Es, "dist": dist}


def fused_view(angle, min_weight=1):
    """(s2w, c, the oracle's label image, the restated maps) of the orbit view at `angle`."""
    s2w, c, img, m = _fused_view(angle)
    return s2w, c, img, with_min_weight(m, min_weight)


@functools.lru_cache(maxsize=None)
def _fused_view(angle):
    O = _oracle()
    sc = fused_scene()
    s2w, c = O.orbit_camera(list(sc["p"].Kinv), angle, sc["dist"])
    return (s2w, c) + _restate_oracle_state(sc, s2w, c, 1)


@functools.lru_cache(maxsize=None)
def fused_pose_view(k, min_weight=1):
    """The same for the pose camera of frame k (pose_camera in f64 rounded once: its definition)."""
    sc = fused_scene()
    s2w, c = pose_camera_def(list(sc["p"].Kinv), sc["E"][k])
    return (s2w, c) + _restate_oracle_state(sc, s2w, c, min_weight)


def _restate_oracle_state(sc, s2w, c, min_weight):
    O = _oracle()
    p, ost = sc["p"], sc["ost"]
    D = tuple(p.dim)
    img, t = O.render(sc["g"], s2w, c, p.width, p.height, 0, ost.sdf, ost.hist)
    m = restate_maps(t, s2w, c, ost.sdf.reshape(D), ost.wt.reshape(D), ost.hist.reshape(D + (32,)),
                     list(p.vol_start), list(p.voxel), min_weight)
    return img, m


def pose_camera_def(Kinv, E):
    """semtsdf_pose_camera by its definition: f64 products summed in ascending index, rounded once."""
    K = np.asarray(Kinv, np.float32).reshape(4, 4).astype(np.float64)
    e = np.asarray(E, np.float32).reshape(4, 4).astype(np.float64)
    s2w = np.zeros((4, 4), np.float32)
    for i in range(3):
        acc = 0.0
        for k in range(3):
            acc += e[k, i] * e[k, 3]
        s2w[i, 3] = np.float32(-acc)
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc += e[k, i] * K[k, j]
            s2w[i, j] = np.float32(acc)
    s2w[3, 3] = 1.0
    return s2w.reshape(16), s2w[:3, 3].copy()


FIELD_DIMS = (11, 13, 37)
FIELD_START, FIELD_VOXEL = (-0.3, 0.1, 0.5), (0.011, 0.012, 0.013)
FIELD_W, FIELD_H = 75, 53
FIELD_INTR = (120.0, 120.0, 77.0, -2.0)  # fx, fy, cx, cy


def field_params(flags):
    """test_gpu_mesh.py's field volume with the ragged 75 x 53 frame."""
    import semtsdf

    p = semtsdf.default_params(64, FIELD_INTR, FIELD_W, FIELD_H)
    for a in range(3):
        p.dim[a] = FIELD_DIMS[a]
        p.vol_start[a], p.voxel[a] = FIELD_START[a], FIELD_VOXEL[a]
        p.vol_end[a] = FIELD_START[a] + FIELD_VOXEL[a] * (FIELD_DIMS[a] - 1)
    p.mu = 0.05
    p.flags = flags
    return p


def field_view(flags, min_weight):
    """(params, field, s2w, c, restated maps) of the random field seen from pose_camera(Kinv, identity)."""
    p, f, s2w, c, m = _field_view(flags)
    return p, f, s2w, c, with_min_weight(m, min_weight)


@functools.lru_cache(maxsize=None)
def _field_view(flags):
    from mesh_restatement import random_field

    O = _oracle()
    p = field_params(flags)
    f = random_field(FIELD_DIMS)
    s2w, c = pose_camera_def(list(p.Kinv), np.eye(4, dtype=np.float32))
    g = O.OGeom.from_params(p)
    sem = bool(flags & 1)
    sdf = np.ascontiguousarray(f["sdf"].reshape(-1))
    hist = np.ascontiguousarray(f["hist"].reshape(-1))
    color = np.ascontiguousarray(f["color"].reshape(-1))
    _, t = O.render(g, s2w, c, FIELD_W, FIELD_H, 0 if sem else 1, sdf, hist if sem else None, color, True)
    m = restate_maps(t, s2w, c, f["sdf"], f["wt"], f["hist"] if sem else None, list(p.vol_start), list(p.voxel), 1)
    return p, f, s2w, c, m
