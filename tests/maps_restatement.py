"""The empty-space octant maps restated from their definition (plain NumPy, no GPU), and the
inputs of the map-update tests, built from the C oracle alone so that their conditions can be
checked without a GPU (tests/test_maps.py) before tests/test_gpu_map_updates.py relies on them.

Definition.  Brick b (8^3 voxels, partial at the upper edges) is skippable when every voxel of
the bricks b + {0,1}^3 that lie inside the volume holds sdf >= thr, thr = f32(voxel) / f32(2) *
f32(1 + 2^-16).  d0(b) is CAP for a skippable brick and 0 otherwise.  Byte o of b's word (bit a
of o set: negative along axis a) is min over 0 <= kx, ky, kz < CAP of max(kx, ky, kz, d0(b + s
k)), neighbours outside the volume ignored: the L-inf distance, capped, to the nearest
non-skippable brick of octant o.

numpy_maps states it with array shifts, one axis at a time; naive_maps with loops over bricks,
voxels and offsets, nothing shared with the former but the threshold."""
import itertools

import numpy as np

CAP = 16  # kBrickDistCap (SEMTSDF_BRICK_DIST_CAP)
RCP_TABLE = 1024  # kRcpTable: weights below it take the reciprocal table, the others true division
WEIGHTS = (0, 1, 2, 7, 1022, 1023, 1024, 1025, 4095, 4096)


def skip_threshold(voxel) -> np.float32:
    return np.float32(voxel) / np.float32(2.0) * np.float32(1.0 + 2.0 ** -16)


def numpy_maps(sdf_xyz: np.ndarray, voxel: float) -> np.ndarray:
    """Octant words from the definition (dims need not be multiples of 8: partial edge bricks)."""
    thr = np.float32(voxel) / np.float32(2.0) * np.float32(1.0 + 2.0 ** -16)
    X, Y, Z = sdf_xyz.shape
    nb = [(X + 7) // 8, (Y + 7) // 8, (Z + 7) // 8]
    pad = np.full((nb[0] * 8, nb[1] * 8, nb[2] * 8), np.inf, np.float32)
    pad[:X, :Y, :Z] = sdf_xyz
    plain = pad.reshape(nb[0], 8, nb[1], 8, nb[2], 8).min(axis=(1, 3, 5))
    bmin = plain.copy()
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                sh = np.full_like(plain, np.inf)
                sh[: nb[0] - dx, : nb[1] - dy, : nb[2] - dz] = plain[dx:, dy:, dz:]
                bmin = np.minimum(bmin, sh)
    d0 = np.where(bmin >= thr, CAP, 0).astype(np.int32)
    words = np.zeros(d0.shape, np.uint64)
    for o in range(8):
        d = d0.copy()
        for a in range(3):
            s = -1 if (o >> a) & 1 else 1
            out = d.copy()  # k = 0
            n = d.shape[a]
            for k in range(1, CAP):
                if k >= n:
                    break
                sh = np.full_like(d, 1 << 20)
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                if s > 0:
                    src[a], dst[a] = slice(k, n), slice(0, n - k)
                else:
                    src[a], dst[a] = slice(0, n - k), slice(k, n)
                sh[tuple(dst)] = d[tuple(src)]
                out = np.minimum(out, np.maximum(k, sh))
            d = out
        words |= d.astype(np.uint64) << np.uint64(8 * o)
    return words.reshape(-1)


def naive_maps(sdf_xyz: np.ndarray, voxel: float) -> np.ndarray:
    """The definition as loops: per brick the minimum over every voxel of the bricks b + {0,1}^3
    inside the volume, skippable iff that minimum >= thr, then per octant the minimum over the
    CAP^3 offsets of max(kx, ky, kz, d0)."""
    thr = skip_threshold(voxel)
    X, Y, Z = sdf_xyz.shape
    nbx, nby, nbz = (X + 7) // 8, (Y + 7) // 8, (Z + 7) // 8
    d0 = [[[0] * nbz for _ in range(nby)] for _ in range(nbx)]
    for bx in range(nbx):
        for by in range(nby):
            for bz in range(nbz):
                m = None
                for i, j, k in itertools.product((0, 1), repeat=3):
                    cx, cy, cz = bx + i, by + j, bz + k
                    if cx >= nbx or cy >= nby or cz >= nbz:
                        continue
                    for x in range(8 * cx, min(8 * cx + 8, X)):
                        for y in range(8 * cy, min(8 * cy + 8, Y)):
                            for z in range(8 * cz, min(8 * cz + 8, Z)):
                                v = sdf_xyz[x, y, z]
                                if m is None or v < m:
                                    m = v
                d0[bx][by][bz] = CAP if m >= thr else 0
    words = np.zeros(nbx * nby * nbz, np.uint64)
    for bx in range(nbx):
        for by in range(nby):
            for bz in range(nbz):
                w = 0
                for o in range(8):
                    sx, sy, sz = (-1 if o & 1 else 1), (-1 if o & 2 else 1), (-1 if o & 4 else 1)
                    best = CAP  # every term with a k >= CAP, and an empty set, is worth CAP at least
                    for kx in range(CAP):
                        cx = bx + sx * kx
                        if cx < 0 or cx >= nbx or kx >= best:
                            continue
                        for ky in range(CAP):
                            cy = by + sy * ky
                            if cy < 0 or cy >= nby or ky >= best:
                                continue
                            for kz in range(CAP):
                                cz = bz + sz * kz
                                if cz < 0 or cz >= nbz:
                                    continue
                                best = min(best, max(kx, ky, kz, d0[cx][cy][cz]))
                    w |= best << (8 * o)
                words[(bx * nby + by) * nbz + bz] = w
    return words


def brick_skippable(sdf_xyz: np.ndarray, voxel: float) -> np.ndarray:
    """d0 > 0 per brick, [nbx, nby, nbz] (byte 0 of a word is 0 exactly where d0 is: k = 0)."""
    X, Y, Z = sdf_xyz.shape
    nb = ((X + 7) // 8, (Y + 7) // 8, (Z + 7) // 8)
    return (numpy_maps(sdf_xyz, voxel) & np.uint64(0xFF)).reshape(nb) > 0


def brick_any(mask_xyz: np.ndarray) -> np.ndarray:
    """Per brick: does any voxel of the brick itself carry the mask."""
    X, Y, Z = mask_xyz.shape
    nb = ((X + 7) // 8, (Y + 7) // 8, (Z + 7) // 8)
    pad = np.zeros((nb[0] * 8, nb[1] * 8, nb[2] * 8), bool)
    pad[:X, :Y, :Z] = mask_xyz
    return pad.reshape(nb[0], 8, nb[1], 8, nb[2], 8).any(axis=(1, 3, 5))


# ---------------------------------------------------------------------------- input builders
def new_ostate(oracle, dims, mu, flags, lz=None):
    return oracle.OState(list(dims), mu, semantic=bool(flags & 1), color_i32=bool(flags & 4), vote=bool(flags & 8),
                         lz=lz)


def frame_labels(fr, flags):
    """(mask, cls) arguments of oracle.integrate for a frame under `flags`."""
    return (fr.gt_ids if flags & 1 else None), (fr.gt_ids.astype(np.int32) if flags & 8 else None)


def f_field(oracle, g, p, frame, E, flags, depth=None, zmap=None):
    """The frame integrated into a fresh state: (touched = wt == 1, f = sdf), flat.  With weight
    0 the oracle stores f itself (fma(sdf, 0, f) / 1)."""
    lz = None if zmap is None else len(zmap)
    ost = new_ostate(oracle, list(p.dim), p.mu, flags, lz)
    mask, cls = frame_labels(frame, flags)
    oracle.integrate(g, ost, list(p.K), E, frame.depth if depth is None else depth, frame.rgb, mask, cls, flags=flags,
                     zmap=zmap)
    return ost.wt == 1, ost.sdf.copy()


def sdf_classes(rng, n, thr, mu):
    """n sdf values drawn per voxel from: thr, nextafter(thr, +-inf) once and twice, +-0, +-2^-20,
    uniform(-1, 1), 1.0 and mu (the reset value); the first row of the table below is what a
    draw is worth at or above the threshold."""
    thr = np.float32(thr)
    inf = np.float32(np.inf)
    up1, dn1 = np.nextafter(thr, inf), np.nextafter(thr, -inf)
    table = np.array([thr, up1, np.nextafter(up1, inf), 1.0, mu, dn1, np.nextafter(dn1, -inf), 0.0, -0.0, 2.0 ** -20,
                      -2.0 ** -20], np.float32)
    k = rng.integers(0, table.size + 1, n)
    out = np.where(k < table.size, table[np.minimum(k, table.size - 1)], rng.uniform(-1.0, 1.0, n).astype(np.float32))
    return out.astype(np.float32)


def seed_aux(rng, wt, flags):
    """Colours 0..255 and, with a histogram, at most two small bins per voxel whose sum stays
    at or below the weight."""
    n = wt.size
    color = rng.integers(0, 256, n * 3).astype(np.int32 if flags & 4 else np.uint8)
    hist = None
    if flags & 1:
        hist = np.zeros((n, 32), np.uint32)
        for _ in range(2):
            b = rng.integers(0, 32, n)
            c = np.minimum(rng.integers(0, 4, n), wt // 2).astype(np.uint32)
            hist[np.arange(n), b] += c
        hist = hist.reshape(-1)
    return color, hist


def seed_state(rng, dims, thr, touched, f, mu=None, sparse_z=None, p_low=1.0 / 1024, plant=64, flags=0x3,
               free_low=False):
    """An uploadable (sdf, wt, color, hist), flat in the reference layout.

    Every voxel draws its sdf from sdf_classes and its weight from WEIGHTS on its own, so one
    lane of 4 z-consecutive voxels mixes table and division weights.  A brick flips only where
    its whole 2^3 neighbourhood sits on one side before the frame, which independent draws over
    all classes never give.  So the planes z >= sparse_z (default: the upper half) keep a draw
    below the threshold with probability p_low, and only where the frame touches the voxel with
    f >= thr; otherwise they redraw it among the classes at or above (uniform on [thr, 1] for
    the uniform class).  The planes below sparse_z keep every draw.  `plant` touched voxels with
    |f| < 1 get sdf = -f and weight 1: the numerator fma(sdf, w, f) is then exactly 0 (the
    0x1p-60 path), which no draw from the classes reaches.  free_low: every voxel the frame
    touches with f == 1 draws again, among the classes below the threshold only (the free and
    full-free units then cross upwards wherever the weight lets them)."""
    X, Y, Z = dims
    n = X * Y * Z
    thr = np.float32(thr)
    mu = np.float32(1.0 if mu is None else mu)
    touched = np.asarray(touched).reshape(-1)
    f = np.asarray(f, np.float32).reshape(-1)
    sdf = sdf_classes(rng, n, thr, mu)
    inf = np.float32(np.inf)
    high = np.array([thr, np.nextafter(thr, inf), np.nextafter(np.nextafter(thr, inf), inf), 1.0, mu], np.float32)
    k = rng.integers(0, high.size + 1, n)
    u = (thr + rng.uniform(0.0, 1.0, n) * (1.0 - float(thr))).astype(np.float32)
    redraw = np.where(k < high.size, high[np.minimum(k, high.size - 1)], np.maximum(u, thr)).astype(np.float32)
    keep = (rng.uniform(0.0, 1.0, n) < p_low) & touched & (f >= thr)
    zs = np.tile(np.arange(Z), X * Y)
    sparse = (zs >= (Z // 2 if sparse_z is None else sparse_z)) & (sdf < thr) & ~keep
    sdf = np.where(sparse, redraw, sdf).astype(np.float32)
    wt = np.asarray(WEIGHTS, np.int32)[rng.integers(0, len(WEIGHTS), n)]
    cand = np.nonzero(touched & (np.abs(f) < 1.0) & (f != 0.0))[0]
    sel = rng.choice(cand, size=min(plant, cand.size), replace=False) if cand.size else cand
    sdf[sel] = -f[sel]
    wt[sel] = 1
    if free_low:
        dn1 = np.nextafter(thr, -inf)
        low = np.array([dn1, np.nextafter(dn1, -inf), 0.0, -0.0, 2.0 ** -20, -2.0 ** -20], np.float32)
        k = rng.integers(0, low.size + 1, n)
        v = (-1.0 + rng.uniform(0.0, 1.0, n) * (1.0 + float(dn1))).astype(np.float32)
        draw = np.where(k < low.size, low[np.minimum(k, low.size - 1)], np.minimum(v, dn1)).astype(np.float32)
        sdf = np.where(touched & (f == 1.0), draw, sdf).astype(np.float32)
    color, hist = seed_aux(rng, wt, flags)
    return sdf, wt, color, hist


def crossings(sdf_before, sdf_after, thr):
    """(down, up): before >= thr > after, and before < thr <= after."""
    thr = np.float32(thr)
    b, a = np.asarray(sdf_before, np.float32), np.asarray(sdf_after, np.float32)
    return (b >= thr) & (a < thr), (b < thr) & (a >= thr)


def side(x, thr):
    """-1 below, 0 equal, 1 above the threshold."""
    thr = np.float32(thr)
    x = np.asarray(x, np.float32)
    return (x > thr).astype(np.int32) - (x < thr).astype(np.int32)


# --------------------------------------------------------------------- the cases' own inputs
KI = (520.9, 521.0, 325.1, 249.7)
W, H = 640, 480
DIMS = (44, 36, 136)  # ragged on x and y; nbz = 17: a last quad of one brick, the cap reachable along z
# The volume is placed (PLACE_SFM, frame 0) for 0.72 of the frame's mean depth: with the full mean
# depth the far wall of the synthetic scene lies at 5/8 of the z extent and no voxel of the last
# four z-bricks is ever touched; with 0.72 the wall's band falls into z-bricks 15 and 16 (the lone
# brick of the last quad), the objects' into 4..11, with free space between them.
PLACE = 0.72
SHARD_DIMS = (40, 36, 48)
SHARDS = ((2, 8), (3, 5), (3, 2))
FREE_DIMS = (96, 96, 96)
SEED_FLAGS = (0x3, 0x1, 0x4, 0xC)

_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def frames():
    from semtsdf.synth import SyntheticStream

    def build():
        st = SyntheticStream(seed=3)
        return [st.frame(k) for k in range(6)]

    return cached("frames", build)


def pose(k):
    fr = frames()
    return (fr[k].w2c @ fr[0].c2w).astype(np.float32)


def mean_depth():
    d = frames()[0].depth
    return float(np.mean(d[d > 0])) / 5000.0


def make_params(dims, flags=0x3, cull=True, place=PLACE):
    """The make / place_from_frame pattern of test_gpu_parity.py (host functions of the C ABI, no
    GPU call)."""
    import semtsdf
    from semtsdf import _lib as L

    p = semtsdf.default_params(64, KI, W, H)
    p.dim[0], p.dim[1], p.dim[2] = dims
    semtsdf.place_from_frame(p, frames()[0].depth, mean_depth() * place, L.PLACE_SFM)
    p.flags = flags | (0 if cull else L.F_NO_CULL)
    return p


def fill_holes(depth):
    d = depth.copy()
    d[d == 0] = np.uint16(d[d > 0].max())  # holes become far samples
    return d


def set_ostate(ost, seed):
    for k, v in seed.items():
        if v is not None:
            getattr(ost, k)[:] = v


def copy_ostate(oracle, dims, mu, flags, src, lz=None):
    ost = new_ostate(oracle, dims, mu, flags, lz)
    set_ostate(ost, {k: getattr(src, k) for k in ("sdf", "wt", "color", "hist", "cls", "cls_cnt")})
    return ost


def vote_seed(rng, n):
    """(cls, cls_cnt) of a vote volume: classes 0..5, counts 0..3."""
    return rng.integers(0, 6, n).astype(np.int32), rng.integers(0, 4, n).astype(np.int32)


def integrate_frame(oracle, g, p, ost, fr, E, flags, depth=None, zmap=None, x_range=None):
    mask, cls = frame_labels(fr, flags)
    return oracle.integrate(g, ost, list(p.K), E, fr.depth if depth is None else depth, fr.rgb, mask, cls,
                            flags=flags & 0xF, zmap=zmap, x_range=x_range)


class Case:
    """One seeded single-frame input: params, geometry, frame, pose, the seed (dict of flat
    arrays, reference layout) and the oracle's state after the frame."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def seeded_case(oracle, flags, dims=DIMS, frame=1, rng_seed=1, sparse_z=None, depth=None, E=None, free_low=False,
                plant=64):
    """a: the seed uploaded, then one frame.  The sdf, weights and crossings are the same for
    every flag set (colour, histogram and votes are drawn after them)."""
    def build():
        p = make_params(dims, flags)
        g = oracle.OGeom.from_params(p)
        fr = frames()[frame]
        Ek = pose(frame) if E is None else E
        thr = skip_threshold(p.voxel[0])
        touched, f = f_field(oracle, g, p, fr, Ek, flags, depth=depth)
        rng = np.random.default_rng(rng_seed)
        sdf, wt, color, hist = seed_state(rng, dims, thr, touched, f, mu=p.mu, sparse_z=sparse_z, flags=flags,
                                          free_low=free_low, plant=plant)
        seed = dict(sdf=sdf, wt=wt, color=color, hist=hist, cls=None, cls_cnt=None)
        if flags & 8:
            seed["cls"], seed["cls_cnt"] = vote_seed(rng, sdf.size)
        ost = new_ostate(oracle, dims, p.mu, flags)
        set_ostate(ost, seed)
        counts = integrate_frame(oracle, g, p, ost, fr, Ek, flags, depth=depth)
        return Case(p=p, g=g, fr=fr, E=Ek, thr=thr, dims=tuple(dims), flags=flags, touched=touched, f=f, seed=seed,
                    ost=ost, counts=counts, depth=fr.depth if depth is None else depth)

    key = ("seeded", flags, tuple(dims), frame, rng_seed, sparse_z, free_low, plant,
           None if depth is None else depth.tobytes()[:64] + bytes(str(int(depth.sum())), "ascii"),
           None if E is None else np.asarray(E).tobytes())
    return cached(key, build)


def shard_case(oracle, nshards, chunk, sidx):
    """f: the (SHARD_DIMS) seed of sequence a through shard sidx's local plane map; the local planes
    past the volume's end (the last halo plane) hold the reset state and are never integrated.  The
    whole small volume draws sparsely (sparse_z = 0), so that bricks of the local maps flip both ways."""
    from semtsdf.shard import ShardLayout

    def build():
        c = seeded_case(oracle, 0x3, dims=SHARD_DIMS, rng_seed=5, sparse_z=0)
        X, Y, Z = SHARD_DIMS
        zmap = ShardLayout(Z, nshards, chunk).local_to_global(sidx).astype(np.int32)
        inside = zmap < Z
        zc = np.minimum(zmap, Z - 1)

        def local(a, extra, fill):
            if a is None:
                return None
            out = a.reshape((X, Y, Z) + extra)[:, :, zc].copy()
            out[:, :, ~inside] = fill
            return np.ascontiguousarray(out).reshape(-1)

        seed = dict(sdf=local(c.seed["sdf"], (), np.float32(c.p.mu)), wt=local(c.seed["wt"], (), 0),
                    color=local(c.seed["color"], (3,), 0), hist=local(c.seed["hist"], (32,), 0), cls=None,
                    cls_cnt=None)
        ldims = (X, Y, int(zmap.size))
        ost = new_ostate(oracle, SHARD_DIMS, c.p.mu, 0x3, lz=zmap.size)
        set_ostate(ost, seed)
        integrate_frame(oracle, c.g, c.p, ost, c.fr, c.E, 0x3, zmap=zmap)
        return Case(p=c.p, g=c.g, fr=c.fr, E=c.E, thr=c.thr, dims=ldims, flags=0x3, seed=seed, ost=ost, zmap=zmap)

    return cached(("shard", nshards, chunk, sidx), build)


def mean_update(so, w, f):
    """The oracle's running mean fma(so, (float)w, f) / (float)(w + 1) in NumPy: the product of
    two f32 values is exact in f64; the sum is rounded to f64 and then to f32 (a double rounding
    the oracle does not have: the tests check every planted value against the oracle itself)."""
    so, f = np.asarray(so, np.float32), np.asarray(f, np.float32)
    w = np.asarray(w, np.int64)
    num = (so.astype(np.float64) * w.astype(np.float32).astype(np.float64) + f.astype(np.float64)).astype(np.float32)
    return num / (w + 1).astype(np.float32)


def solve_weight(so, f, target, wmax):
    """A weight 0 <= w <= wmax with mean_update(so, w, f) == target exactly, or -1."""
    so, f, target = np.float32(so), np.float32(f), np.float32(target)
    if so == target:
        w0 = abs(float(f) - float(so)) * 2.0 ** 32 + 16.0  # the change is below half an ulp of thr
    else:
        w0 = (float(f) - float(target)) / (float(target) - float(so))
    if not (0.0 <= w0 <= wmax):
        return -1
    step = max(1, int(np.spacing(np.float32(w0))))
    cand = np.unique(np.clip(int(w0) + step * np.arange(-48, 49), 0, wmax))
    hit = cand[mean_update(np.full(cand.size, so), cand, np.full(cand.size, f)) == target]
    return int(hit[0]) if hit.size else -1


THRESHOLD_WMAX = 1 << 27  # the planted weights of case b, apart from the lone voxels'
LONE_WMAX = 1 << 29  # the lone voxels': one ulp of thr at f == 1 takes about 2.6e8 (an eighth of INT32_MAX)


def threshold_case(oracle, rng_seed=7, per_pair=24, lone=3):
    """b: every stored sdf is thr, thr -+ 1 ulp, +0.0 or -0.0 with weights from WEIGHTS; on top,
    for every pair (before, after) of {thr - 1 ulp, thr, thr + 1 ulp}^2, up to per_pair voxels
    near a surface (|f - thr| < 0.1) get the stored value `before` and a weight solved so that
    the frame leaves `after` exactly.  `lone` bricks whose whole 2^3 neighbourhood is untouched
    or touched with f >= thr hold thr or thr + 1 ulp throughout, except one voxel with f == 1 at
    thr - 1 ulp whose weight takes it to thr: the brick's only sub-threshold voxel becomes equal
    and the brick flips to skippable.  One ulp of thr at f == 1 takes a weight of about 2.6e8
    (LONE_WMAX bounds it)."""
    def build():
        flags, dims = 0x3, DIMS
        p = make_params(dims, flags)
        g = oracle.OGeom.from_params(p)
        fr, E = frames()[1], pose(1)
        thr = skip_threshold(p.voxel[0])
        inf = np.float32(np.inf)
        up1, dn1 = np.nextafter(thr, inf), np.nextafter(thr, -inf)
        touched, f = f_field(oracle, g, p, fr, E, flags)
        rng = np.random.default_rng(rng_seed)
        n = touched.size
        X, Y, Z = dims
        sdf = np.array([thr, up1, dn1, 0.0, -0.0], np.float32)[rng.integers(0, 5, n)]
        wt = np.asarray(WEIGHTS, np.int32)[rng.integers(0, len(WEIGHTS), n)]
        reserved = np.zeros(n, bool)
        t3, f3 = touched.reshape(dims), f.reshape(dims)
        bad = brick_any(t3 & (f3 < thr))  # bricks holding a voxel the frame takes below
        nb = bad.shape
        lone_bricks = []
        order = rng.permutation(nb[0] * nb[1] * nb[2])
        idx = np.arange(n).reshape(dims)
        for br in order:
            bx, by, bz = np.unravel_index(br, nb)
            if bx + 1 >= nb[0] or by + 1 >= nb[1] or bz + 1 >= nb[2] or bad[bx:bx + 2, by:by + 2, bz:bz + 2].any():
                continue
            hood = idx[8 * bx:8 * bx + 16, 8 * by:8 * by + 16, 8 * bz:8 * bz + 16].reshape(-1)
            own = idx[8 * bx:8 * bx + 8, 8 * by:8 * by + 8, 8 * bz:8 * bz + 8].reshape(-1)
            own = own[touched[own] & (f[own] == 1.0)]
            if reserved[hood].any() or own.size == 0:
                continue
            v = int(rng.choice(own))
            w = solve_weight(dn1, 1.0, thr, LONE_WMAX)
            if w < 0:
                continue
            sdf[hood] = np.array([thr, up1], np.float32)[rng.integers(0, 2, hood.size)]
            sdf[v], wt[v] = dn1, w
            reserved[hood] = True
            lone_bricks.append(((int(bx), int(by), int(bz)), v))
            if len(lone_bricks) == lone:
                break
        planted = []
        near = np.nonzero(touched & ~reserved & (np.abs(f - thr) < 0.1) & (np.abs(f - thr) > 2.0 ** -12))[0]
        near = rng.permutation(near)
        used = 0
        for so in (dn1, thr, up1):
            for target in (dn1, thr, up1):
                got = 0
                while got < per_pair and used < near.size:
                    v = int(near[used])
                    used += 1
                    if so != target and (f[v] > so) != (target > so):
                        continue
                    w = solve_weight(so, f[v], target, THRESHOLD_WMAX)
                    if w < 0:
                        continue
                    sdf[v], wt[v] = so, w
                    planted.append((v, float(so), float(target)))
                    got += 1
        color, hist = seed_aux(rng, np.minimum(wt, 8), flags)
        seed = dict(sdf=sdf, wt=wt, color=color, hist=hist, cls=None, cls_cnt=None)
        ost = new_ostate(oracle, dims, p.mu, flags)
        set_ostate(ost, seed)
        integrate_frame(oracle, g, p, ost, fr, E, flags)
        return Case(p=p, g=g, fr=fr, E=E, thr=thr, dims=dims, flags=flags, touched=touched, f=f, seed=seed, ost=ost,
                    planted=planted, lone=lone_bricks, near3=(dn1, thr, up1), depth=fr.depth)

    return cached(("threshold", rng_seed, per_pair, lone), build)


# d: a surface appears and goes
FAR_RAW, PATCH_RAW = 20000, 10000  # 4.0 m (past the volume's end + mu) and 2.0 m (inside it)
# As the issue states it (P, P, Q, P, P, P) no brick can change: Q meets sdf 1 with weight 2 and
# (2 + f) / 3 > 1/3 stays far above the threshold (about 0.03) for every f > -1.  Three Q frames
# take the voxels behind the patch (f < -2/3) below it, (2 + 3 f) / 5 < 0, and three P frames bring
# every voxel back above, (2 + 3 f + 3) / 8 > 1/4: the surface appears and goes.
SURFACE_SEQ = "PPQQQPPP"


def surface_frames():
    P = np.full((H, W), FAR_RAW, np.uint16)
    Q = P.copy()
    Q[H // 2 - 24:H // 2 + 24, W // 2 - 24:W // 2 + 24] = PATCH_RAW
    return {"P": P, "Q": Q}


def surface_case(oracle):
    """The oracle's state after every frame of SURFACE_SEQ (E = identity, colours and ids of frame
    1), each a copy."""
    def build():
        flags = 0x3
        p = make_params(DIMS, flags)
        g = oracle.OGeom.from_params(p)
        fr = frames()[1]
        E = np.eye(4, dtype=np.float32)
        ost = new_ostate(oracle, DIMS, p.mu, flags)
        states = []
        for ch in SURFACE_SEQ:
            integrate_frame(oracle, g, p, ost, fr, E, flags, depth=surface_frames()[ch])
            states.append(copy_ostate(oracle, DIMS, p.mu, flags, ost))
        return Case(p=p, g=g, fr=fr, E=E, dims=DIMS, flags=flags, states=states, thr=skip_threshold(p.voxel[0]))

    return cached("surface", build)


# e: free and full-free units
def flip_pose():
    """The `flip` pose of test_gpu_wide_poses.py: the camera at the origin looking back (-z), the
    volume behind it: every touched voxel has qz <= 0 and f == 1."""
    c2w = np.eye(4)
    c2w[0, 0], c2w[2, 2] = -1.0, -1.0  # rot_y(pi)
    return np.linalg.inv(c2w).astype(np.float32)


def free_case(oracle, name):
    """`head_on`: frame 1 with its holes filled; `flip`: the same image under flip_pose.  The seed
    holds sdf below the threshold wherever the frame touches with f == 1."""
    fr = frames()[1]
    return seeded_case(oracle, 0x3, dims=FREE_DIMS, rng_seed=11, depth=fill_holes(fr.depth),
                       E=None if name == "head_on" else flip_pose(), free_low=True)


def whole_units(mask_xyz):
    """Per 1x8x16 unit (the integrate's work unit) inside the volume: all of its voxels carry the
    mask.  [X, Y // 8, Z // 16]."""
    X, Y, Z = mask_xyz.shape
    return mask_xyz[:, :Y // 8 * 8, :Z // 16 * 16].reshape(X, Y // 8, 8, Z // 16, 16).all(axis=(2, 4))


def orbit(p, angle):
    import semtsdf

    return semtsdf.orbit_camera(list(p.Kinv), angle, mean_depth() * PLACE)
