"""Integrate, render and association away from the head-on camera: the HIP path against the C
oracle, bit for bit (sdf and t bit patterns, integer state and images with array_equal; no
tolerance anywhere).  Every other GPU test drives the kernels from almost one viewing geometry
(yaw of 0.004 rad per frame, orbit angles up to 0.3), so these cases reach code that no other
test runs.

Which case reaches which code path
  octants 4-7 (dz < 0; the octant's map byte, brick_box towards -z):
      B test_render_all_octants at angles 1.0, pi, -1.0 (test_octant_coverage proves all 8
      octants carry hits); B association at `opposite`, `side`, `inside_back`; A
      test_render_after_flip; C renders at pi; D sharded and fused.
  qz <= 0 (voxels behind the camera still divide to a pixel and are updated with f == 1;
  unit_cull's sign-mixed wmin/wmax return, the hull of all-negative units, dmin - zmax with
  zmax < 0):
      A `inside`, `flip`, `above` (all touched voxels of `flip` and `above` are behind),
      `oblique` (units straddle sz == 0); C planes 0-7; D sharded `inside` and `flip`.
  sz == 0 exactly (+-inf saturates off the image) and the NaN pixel (0 / 0 floors to pixel 0):
      C plane gz == 8 in every depth image; `one_pixel00` touches exactly voxel (12, 12, 8),
      reached through the NaN alone.
  footprints wider than 256 px (camera inside the volume):
      A `inside`, B `inside_back`, C (the camera sits at voxel (12, 12, 8)).
  thin footprints (the volume seen along an axis, a 1x8x16 unit projecting to a strip):
      A `side`, `above`, `roll90`.
  dead units (dmax - zmin < -mu - margin): A `beyond` (everything dead), `far`.
  diff == +-mu exactly:
      C `const2048`: plane 19 has diff == +mu (f == 1.0, not gated), plane 29 has diff == -mu
      (untouched), plane 28 is the last touched one.
  zero direction components (ray_bounds and box_exit divide by them):
      C association and renders: column 320 has dx == 0 and row 240 has dy == 0 exactly.
  reverse slab order (a ray with dz < 0 visits the Z-slabs back to front):
      D test_sharded_wide_poses (angles 1.0, pi, -1.0; both exchanges) and
      test_sharded_association_opposite.
  fused association + view launch with dz < 0 in both marches: D test_fused_view_opposite.

Cull-class counters (bricks, free_units, full_units of semtsdf_timing for the pose frame alone,
flags 0x3, culling on), measured on an MI355X.  The A volume has 1400 units and the C volume
216, which is what `bricks` reads with SEMTSDF_F_NO_CULL (free_units and full_units are 0 then,
and with flags 0x1 and 0x4, where a free unit would still owe its colour or histogram):
  A (56, 40, 72)   bricks  free_units  full_units
    inside            616         227           0
    flip             1027        1018           0
    opposite          626         192           0
    roll90            629         107           0
    side              572         114           0
    above             917         910           0
    oblique           668          86           0
    far               261           0           0
    beyond              0           0           0
  C (24, 24, 40)   bricks  free_units  full_units
    const2048         144           0           0
    checker           144           0           0
    zeros              84           0           0
    one_pixel00        96           0           0
    max65535          216           0           0
    step              180           0           0
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KI = (520.9, 521.0, 325.1, 249.7)
W, H = 640, 480
NPX = W * H
ANGLES = (1.0, math.pi, -1.0)


@pytest.fixture(scope="module")
def S():
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    return semtsdf, L


@pytest.fixture(scope="module")
def stream():
    from semtsdf.synth import SyntheticStream

    st = SyntheticStream(seed=0)
    return st, [st.frame(k) for k in range(5)]


@pytest.fixture(scope="module")
def cache():
    """Oracle results shared by the tests of this module (base states, renders, marches);
    readers copy what they change."""
    return {}


# ---------------------------------------------------------------------------------- helpers
def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def extrinsic(R, t):
    """E = inv(c2w), c2w = [R | t], in f64, cast to f32."""
    c2w = np.eye(4)
    c2w[:3, :3] = R
    c2w[:3, 3] = t
    return np.linalg.inv(c2w).astype(np.float32)


def centre(p):
    return (np.array(p.vol_start[:], np.float64) + np.array(p.vol_end[:], np.float64)) / 2


def pose(name, p):
    c = centre(p)
    R, t = {
        "inside": (np.eye(3), c),
        "flip": (rot_y(math.pi), (0, 0, 0)),
        "opposite": (rot_y(math.pi), (0, 0, 2 * c[2])),
        "roll90": (rot_z(math.pi / 2), (0, 0, 0)),
        "side": (rot_y(math.pi / 2), (c[0] - c[2], 0, c[2])),
        "above": (rot_x(math.pi / 2), (0, c[1] - c[2], c[2])),
        "oblique": (rot_y(0.5) @ rot_x(0.35), (-0.9, 0.5, 0.3)),
        "far": (np.eye(3), (0, 0, -2)),
        "beyond": (np.eye(3), (0, 0, -6)),
        "inside_back": (rot_y(2.5), c),
    }[name]
    return extrinsic(R, np.asarray(t, np.float64))


def mean_depth(frames):
    d = frames[0].depth
    return float(np.mean(d[d > 0])) / 5000.0


def make_params(S, dims, frames, flags, cull=True):
    semtsdf, L = S
    p = semtsdf.default_params(64, KI, W, H)
    p.dim[0], p.dim[1], p.dim[2] = dims
    semtsdf.place_from_frame(p, frames[0].depth, mean_depth(frames), L.PLACE_SFM)
    p.flags = flags | (0 if cull else L.F_NO_CULL)
    return p


def new_ostate(oracle, dims, mu, flags):
    return oracle.OState(list(dims), mu, semantic=bool(flags & 1), color_i32=bool(flags & 4), vote=bool(flags & 8))


def copy_ostate(oracle, dims, mu, flags, src):
    ost = new_ostate(oracle, dims, mu, flags)
    for k in ("sdf", "wt", "color", "hist"):
        if getattr(src, k) is not None:
            getattr(ost, k)[:] = getattr(src, k)
    return ost


def base_frames(frames, p):
    for k in (1, 2, 3):
        fr = frames[k]
        yield fr, (fr.w2c @ frames[0].c2w).astype(np.float32), (fr.gt_ids if p.flags & 1 else None)


def oracle_base(oracle, cache, S, dims, frames, flags):
    """(p, g, a copy of the oracle state after frames 1-3 with their own poses and gt_ids)."""
    key = ("base", tuple(dims), flags)
    p = make_params(S, dims, frames, flags)
    g = oracle.OGeom.from_params(p)
    if key not in cache:
        ost = new_ostate(oracle, dims, p.mu, flags)
        for fr, E, m in base_frames(frames, p):
            oracle.integrate(g, ost, list(p.K), E, fr.depth, fr.rgb, m, flags=flags)
        cache[key] = ost
    return p, g, copy_ostate(oracle, dims, p.mu, flags, cache[key])


def make(S, oracle, cache, dims, frames, flags, cull=True):
    """A GPU volume and an oracle state, both holding the base state (frames 1-3)."""
    semtsdf, L = S
    _, g, ost = oracle_base(oracle, cache, S, dims, frames, flags)
    p = make_params(S, dims, frames, flags, cull)
    vol = semtsdf.Volume(p, 0)
    vol.set_instrumentation(events=False, count=True)
    for fr, E, m in base_frames(frames, p):
        vol.integrate(fr.depth, fr.rgb, m, E)
    return p, vol, g, ost


def assert_same(vol, ost, hist=False):
    out = vol.download(hist=hist)
    assert np.array_equal(out["sdf"].view(np.uint32), ost.sdf.view(np.uint32)), "sdf bits"
    assert np.array_equal(out["wt"], ost.wt), "weight"
    assert np.array_equal(out["color"], ost.color), "colour"
    if hist:
        assert np.array_equal(out["hist"], ost.hist), "histogram"


def _shard_handles(S, p, nshards, chunk):
    semtsdf, L = S
    shards = []
    for sidx in range(nshards):
        q = semtsdf.default_params(64, KI, W, H)
        for fld in ("dim", "vol_start", "vol_end", "voxel", "K", "Kinv"):
            getattr(q, fld)[:] = getattr(p, fld)[:]
        q.mu, q.flags = p.mu, p.flags
        q.z_nshards, q.z_shard, q.z_chunk = nshards, sidx, chunk
        shards.append(semtsdf.Volume(q, 0))
    return shards


def oracle_pose_frame(oracle, g, p, ost, E, fr, flags):
    """Integrates fr under E into ost; returns (touched, gated, touched with qz < 0): the counts of
    the oracle, and qz in f64 from E for the voxels whose weight it raised."""
    wt0 = ost.wt.copy()
    counts = oracle.integrate(g, ost, list(p.K), E, fr.depth, fr.rgb, fr.gt_ids if flags & 1 else None, flags=flags)
    dims = tuple(p.dim[:])
    vs, vx = np.array(p.vol_start[:], np.float64), np.array(p.voxel[:], np.float64)
    ax = [vs[i] + np.arange(dims[i]) * vx[i] for i in range(3)]
    E64 = np.asarray(E, np.float64).reshape(4, 4)
    qz = (E64[2, 0] * ax[0][:, None, None] + E64[2, 1] * ax[1][None, :, None] + E64[2, 2] * ax[2][None, None, :]
          + E64[2, 3])
    touched = (ost.wt != wt0).reshape(dims)
    assert int(touched.sum()) == int(counts[0])
    return int(counts[0]), int(counts[1]), int((touched & (qz < 0)).sum())


def ray_octants(s2w, c):
    """Octant (dx < 0 | dy < 0 << 1 | dz < 0 << 2) of every pixel's ray, from s2w and c as the
    render computes the direction (the sign of r = s2w (x, y, 1) - c; f32 products are exact in
    f64 and each sum is rounded to f32)."""
    s = np.asarray(s2w, np.float32).reshape(4, 4).astype(np.float64)
    cc = np.asarray(c, np.float32).astype(np.float64)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    octs = np.zeros((H, W), np.int32)
    for i in range(3):
        acc = f32(s[i, 0] * x + 0 * y)
        acc = f32(s[i, 1] * y + acc)
        acc = f32(s[i, 2] + acc)
        r = f32(f32(acc + s[i, 3]) - cc[i])
        octs |= (r < 0).astype(np.int32) << i
    return octs


def oracle_view(oracle, cache, tag, g, p, ost, angle, dist, mode):
    key = ("view", tag, angle, dist, mode)
    if key not in cache:
        s2w, c = oracle.orbit_camera(list(p.Kinv), angle, dist)
        cache[key] = (s2w, c) + oracle.render(g, s2w, c, W, H, mode, ost.sdf, ost.hist, ost.color)
    return cache[key]


def oracle_probs(oracle, cache, tag, g, p, ost, E):
    key = ("probs", tag)
    if key not in cache:
        cache[key] = oracle.march_probs(g, list(p.Kinv), E, W, H, ost.sdf, ost.hist, p.box_thresh)
    return cache[key]


# --------------------------------------------------- A. integrate under wide poses, (56, 40, 72)
DIMS_A = (56, 40, 72)
# oracle touched at least / touched behind the camera at least: about half of what the oracle
# returns for these inputs (touched, gated, behind with flags 0x3: inside 13440 948 7299; flip
# 77279 0 77279; opposite 28583 14131 0; roll90 28606 14204 0; side 28340 14029 0; above 78235 0
# 78235; oblique 26957 12469 0; far 14557 12307 0; beyond 0 0 0)
POSES_A = {"inside": (10000, 5000), "flip": (10000, 5000), "opposite": (10000, 0), "roll90": (10000, 0),
           "side": (10000, 0), "above": (10000, 5000), "oblique": (10000, 0), "far": (10000, 0), "beyond": (0, 0)}
CASES_A = [(n, 0x3, True) for n in POSES_A] + \
          [(n, fl, cu) for n in ("inside", "flip", "oblique") for fl, cu in ((0x3, False), (0x1, True), (0x4, True))]


def run_pose_case(S, oracle, cache, frames, name, flags, cull):
    p, vol, g, ost = make(S, oracle, cache, DIMS_A, frames, flags, cull)
    base_wt = ost.wt.copy()
    base_sdf = ost.sdf.copy()
    E = pose(name, p)
    fr = frames[2]
    touched, gated, behind = oracle_pose_frame(oracle, g, p, ost, E, fr, flags)
    need_touched, need_behind = POSES_A[name]
    if name == "beyond":  # everything dead: the frame changes nothing
        assert touched == 0 and np.array_equal(ost.wt, base_wt)
        assert np.array_equal(ost.sdf.view(np.uint32), base_sdf.view(np.uint32))
    else:
        assert touched >= need_touched, touched
    assert behind >= need_behind, behind
    vol.reset_timing()
    vol.integrate(fr.depth, fr.rgb, fr.gt_ids if flags & 1 else None, E)
    tm = vol.timing()
    print(f"pose {name} flags {flags:#x} cull {cull}: oracle touched {touched} gated {gated} behind {behind}; "
          f"gpu touched {tm.touched} gated {tm.gated} bricks {tm.bricks} free_units {tm.free_units} "
          f"full_units {tm.full_units}")
    assert_same(vol, ost, hist=bool(flags & 1))
    assert (tm.touched, tm.gated) == (touched, gated)
    return p, vol, g, ost, tm


@pytest.mark.parametrize("name,flags,cull", CASES_A,
                         ids=[f"{n}-{fl:#x}-{'cull' if cu else 'nocull'}" for n, fl, cu in CASES_A])
def test_integrate_wide_pose(S, oracle, stream, cache, name, flags, cull):
    """One frame (depth, colour and ids of frame 2; the image need not fit the pose, the update
    rule is what is tested) under a wide pose on top of the base state: every array and the
    touched / gated counters of that frame equal the oracle's.  Measured on an MI355X with flags
    0x3 and culling on (bricks, free_units, full_units): inside 616 227 0; flip 1027 1018 0;
    opposite 626 192 0; roll90 629 107 0; side 572 114 0; above 917 910 0; oblique 668 86 0; far
    261 0 0; beyond 0 0 0 (of 1400 units)."""
    st, frames = stream
    p, vol, g, ost, tm = run_pose_case(S, oracle, cache, frames, name, flags, cull)
    if name == "flip" and flags == 0x3 and cull:
        assert tm.free_units > 0  # every in-image voxel there has diff > mu
    vol.close()


def test_render_after_flip(S, oracle, stream, cache):
    """A render at orbit angle pi after the `flip` frame: the empty-space maps and steady flags
    it reads were refreshed from a state written through the behind-camera path."""
    st, frames = stream
    semtsdf, L = S
    p, vol, g, ost, tm = run_pose_case(S, oracle, cache, frames, "flip", 0x3, True)
    s2w, c = semtsdf.orbit_camera(list(p.Kinv), math.pi, mean_depth(frames))
    img, t = vol.raycast(s2w, c, L.RENDER_LABEL, want_t=True)
    ref, t_ref = oracle.render(g, s2w, c, W, H, 0, ost.sdf, ost.hist, ost.color)
    assert (t_ref >= 0).mean() > 0.05
    assert np.array_equal(t.view(np.uint32), t_ref.view(np.uint32))
    assert np.array_equal(img, ref)
    vol.close()


# ------------------------------------- B. marches in all eight octants, (96, 80, 112)
DIMS_B = (96, 80, 112)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("angle", ANGLES)
def test_render_all_octants(S, oracle, stream, cache, angle, mode):
    st, frames = stream
    semtsdf, L = S
    p, vol, g, ost = make(S, oracle, cache, DIMS_B, frames, 0x3)
    dist = mean_depth(frames)
    s2w_o, c_o, ref, t_ref = oracle_view(oracle, cache, "B", g, p, ost, angle, dist, mode)
    s2w, c = semtsdf.orbit_camera(list(p.Kinv), angle, dist)
    assert np.array_equal(s2w, s2w_o) and np.array_equal(c, c_o)
    img, t = vol.raycast(s2w, c, mode, want_t=True)
    assert (t_ref >= 0).mean() > 0.1
    assert np.array_equal(t.view(np.uint32), t_ref.view(np.uint32))
    assert np.array_equal(img, ref), int((img != ref).any(axis=-1).sum())
    vol.close()


def test_octant_coverage(S, oracle, stream, cache):
    """The oracle's own hits of the three render angles cover each of the 8 ray octants at least
    5 000 times (measured on the CPU: 23988, 32070, 58735, 70179, 38784, 25029, 41757, 48456),
    so test_render_all_octants compares marches in every octant."""
    st, frames = stream
    p, g, ost = oracle_base(oracle, cache, S, DIMS_B, frames, 0x3)
    hits = np.zeros(8, np.int64)
    for angle in ANGLES:
        s2w, c, _, t_ref = oracle_view(oracle, cache, "B", g, p, ost, angle, mean_depth(frames), 0)
        hits += np.bincount(ray_octants(s2w, c)[t_ref >= 0], minlength=8)
    print("oracle hits per octant:", hits.tolist())
    assert (hits >= 5000).all(), hits.tolist()


@pytest.mark.parametrize("name", ["opposite", "side", "inside_back"])
def test_association_wide_pose(S, oracle, stream, cache, name):
    """Association probabilities and box masks at poses whose rays have dz < 0 (oracle: 26 %, 41 %
    and 45 % of the pixels carry probabilities; `inside_back` marches from inside the volume)."""
    st, frames = stream
    p, vol, g, ost = make(S, oracle, cache, DIMS_B, frames, 0x3)
    E = pose(name, p)
    vol.set_state(3, 7)
    probs_o, box_o = oracle_probs(oracle, cache, ("B", name), g, p, ost, E)
    share = float((probs_o.reshape(NPX, 32) > 0).any(axis=1).mean())
    print(f"association {name}: oracle share {share:.3f}")
    assert share >= 0.1, share
    probs_g, box_g = vol.assoc_probs(E)
    assert np.array_equal(probs_g.reshape(-1).view(np.uint32), probs_o.view(np.uint32))
    assert np.array_equal(box_g.reshape(-1), box_o)
    vol.close()


def test_parse_frame_opposite(S, oracle, stream, cache):
    """A whole frame (association, relabel, integrate) at `opposite` against the oracle's
    filter_overlaps and integrate: relabelled mask, decision, object count and state."""
    st, frames = stream
    p, vol, g, ost = make(S, oracle, cache, DIMS_B, frames, 0x3)
    E = pose("opposite", p)
    vol.set_state(3, 7)
    fr = frames[4]
    probs_o, box_o = oracle_probs(oracle, cache, ("B", "opposite"), g, p, ost, E)
    m_ref, num, _, prev, _ = oracle.filter_overlaps(probs_o, box_o, fr.mask.copy(), 3, 7, p.prior_mrcnn_err_rate,
                                                    precision=0)
    m_gpu = np.ascontiguousarray(fr.mask.copy())
    stats = vol.parse_frame(fr.depth, fr.rgb, m_gpu, E)
    assert np.array_equal(m_gpu, m_ref)
    assert np.array_equal(np.array(stats.assigned_prev[:]), prev)
    assert stats.num_objs == num
    oracle.integrate(g, ost, list(p.K), E, fr.depth, fr.rgb, m_ref, flags=0x3)
    stt = vol.state()
    assert stt.n_obs == 4 and stt.num_objs == num
    assert_same(vol, ost, hist=True)
    vol.close()


# ------------------------------------- C. exactly representable geometry: the rule's boundaries
DIMS_C = (24, 24, 40)
KI_C = (512.0, 512.0, 320.0, 240.0)
# oracle (touched, gated) of each depth image into a fresh state
IMAGES_C = {"const2048": (3567, 2745), "checker": (2053, 1544), "zeros": (0, 0), "one_pixel00": (1, 0),
            "max65535": (9591, 0), "step": (4470, 2717)}


def exact_params(S, cull=True):
    """voxel 1/32, vol_start (-0.375, -0.375, -0.25), mu 5/32, depth_scale 4096, K (512, 512, 320,
    240), E = I: every product of the f32 contract is exact.  Plane gz == 8 has sz == 0, voxel
    (12, 12, 8) is the camera centre (0 / 0), planes 0-7 are behind the camera."""
    semtsdf, L = S
    p = semtsdf.default_params(24, KI_C, W, H)
    for i in range(3):
        p.dim[i] = DIMS_C[i]
        p.voxel[i] = 1.0 / 32
        p.vol_start[i] = (-0.375, -0.375, -0.25)[i]
        p.vol_end[i] = p.vol_start[i] + (DIMS_C[i] - 1) / 32.0
    p.mu = 0.15625
    p.depth_scale = 4096.0
    p.flags = 0x3 | (0 if cull else L.F_NO_CULL)
    return p


def exact_geom(oracle, p):
    return oracle.OGeom(list(p.dim), list(p.vol_start), list(p.voxel), p.mu, list(p.vol_end), depth_scale=4096.0,
                        gate=p.gate)


def exact_inputs():
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    mask = rng.integers(0, 5, (H, W)).astype(np.uint8)
    return rgb, mask


def exact_depth(name):
    d = np.zeros((H, W), np.uint16)
    if name == "const2048":
        d[:] = 2048
    elif name == "checker":
        d[(np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0] = 2048
    elif name == "one_pixel00":
        d[0, 0] = 2048
    elif name == "max65535":
        d[:] = 65535
    elif name == "step":
        d[:, :320] = 1024
        d[:, 320:] = 3072
    else:
        assert name == "zeros"
    return d


def oracle_exact_image(oracle, p, name):
    """The oracle's state and counts after one depth image, with the facts that the geometry
    fixes asserted on it (a wrong oracle cannot pass quietly)."""
    g = exact_geom(oracle, p)
    ost = oracle.OState(list(DIMS_C), p.mu, semantic=True)
    rgb, mask = exact_inputs()
    E = np.eye(4, dtype=np.float32)
    counts = oracle.integrate(g, ost, list(p.K), E, exact_depth(name), rgb, mask, flags=0x3)
    assert (int(counts[0]), int(counts[1])) == IMAGES_C[name]
    wt = ost.wt.reshape(DIMS_C)
    sdf = ost.sdf.reshape(DIMS_C)
    if name == "const2048":
        assert wt[:, :, 29:].sum() == 0  # diff == -mu on plane 29: rejected
        assert wt[:, :, 28].sum() == 456
        assert wt[:, :, :8].sum() == 231  # behind the camera
        on19 = wt[:, :, 19] > 0  # diff == +mu: f == 1.0 exactly, not gated
        assert on19.sum() > 0 and (sdf[:, :, 19][on19] == np.float32(1.0)).all()
        assert ost.hist.reshape(DIMS_C + (32,))[:, :, 19].sum() == 0
        assert ost.color.reshape(DIMS_C + (3,))[:, :, 19].sum() == 0
    if name == "one_pixel00":  # 0 / 0 floors to pixel (0, 0): the camera-centre voxel alone
        assert wt.sum() == 1 and wt[12, 12, 8] == 1 and sdf[12, 12, 8] == np.float32(1.0)
    if name == "zeros":
        fresh = oracle.OState(list(DIMS_C), p.mu, semantic=True)
        assert np.array_equal(ost.sdf.view(np.uint32), fresh.sdf.view(np.uint32)) and not ost.wt.any()
        assert not ost.hist.any() and not ost.color.any()
    return g, ost, counts


@pytest.mark.parametrize("cull", [True, False], ids=["cull", "nocull"])
@pytest.mark.parametrize("name", list(IMAGES_C))
def test_exact_geometry_image(S, oracle, name, cull):
    semtsdf, L = S
    p = exact_params(S, cull)
    g, ost, counts = oracle_exact_image(oracle, p, name)
    vol = semtsdf.Volume(p, 0)
    vol.set_instrumentation(events=False, count=True)
    rgb, mask = exact_inputs()
    vol.integrate(exact_depth(name), rgb, mask, np.eye(4, dtype=np.float32))
    tm = vol.timing()
    print(f"exact {name} cull {cull}: gpu touched {tm.touched} gated {tm.gated} bricks {tm.bricks} "
          f"free_units {tm.free_units} full_units {tm.full_units}")
    assert_same(vol, ost, hist=True)
    assert (tm.touched, tm.gated) == (int(counts[0]), int(counts[1]))
    vol.close()


def exact_combined(S, oracle, cache, gpu=True):
    """`const2048`, then `step`, into one volume."""
    semtsdf, L = S
    p = exact_params(S)
    g = exact_geom(oracle, p)
    rgb, mask = exact_inputs()
    E = np.eye(4, dtype=np.float32)
    if "exact" not in cache:
        ost = oracle.OState(list(DIMS_C), p.mu, semantic=True)
        got = [oracle.integrate(g, ost, list(p.K), E, exact_depth(n), rgb, mask, flags=0x3)[:2].tolist()
               for n in ("const2048", "step")]
        assert got == [[3567, 2745], [4470, 2717]], got
        cache["exact"] = ost
    vol = None
    if gpu:
        vol = semtsdf.Volume(p, 0)
        for n in ("const2048", "step"):
            vol.integrate(exact_depth(n), rgb, mask, E)
        vol.set_state(2, 5)
    return p, vol, g, cache["exact"]


def test_exact_geometry_association(S, oracle, cache):
    """The camera inside the volume at voxel (12, 12, 8); the rays of column 320 have dx == 0 and
    those of row 240 dy == 0 exactly (oracle: 85.5 % of the pixels carry probabilities, 472 on
    column 320, 553 on row 240)."""
    p, vol, g, ost = exact_combined(S, oracle, cache)
    E = np.eye(4, dtype=np.float32)
    probs_o, box_o = oracle_probs(oracle, cache, "exact", g, p, ost, E)
    has = (probs_o.reshape(H, W, 32) > 0).any(axis=2)
    print(f"exact association: share {has.mean():.3f} column 320 {int(has[:, 320].sum())} row 240 "
          f"{int(has[240].sum())}")
    assert has[:, 320].sum() >= 400 and has[240].sum() >= 400
    probs_g, box_g = vol.assoc_probs(E)
    assert np.array_equal(probs_g.reshape(-1).view(np.uint32), probs_o.view(np.uint32))
    assert np.array_equal(box_g.reshape(-1), box_o)
    assert_same(vol, ost, hist=True)
    vol.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("angle", [0.0, math.pi])
def test_exact_geometry_render(S, oracle, cache, angle, mode):
    """Orbit views at dist 0.5 (oracle hit share 0.855 and 0.913; 472 and 480 hits on column 320,
    whose rays have dx == 0)."""
    semtsdf, L = S
    p, vol, g, ost = exact_combined(S, oracle, cache)
    s2w_o, c_o, ref, t_ref = oracle_view(oracle, cache, "exact", g, p, ost, angle, 0.5, mode)
    print(f"exact render {angle}: share {(t_ref >= 0).mean():.3f} column 320 {int((t_ref[:, 320] >= 0).sum())}")
    assert (t_ref[:, 320] >= 0).sum() >= 400 and (t_ref >= 0).mean() >= 0.4
    s2w, c = semtsdf.orbit_camera(list(p.Kinv), angle, 0.5)
    assert np.array_equal(s2w, s2w_o) and np.array_equal(c, c_o)
    img, t = vol.raycast(s2w, c, mode, want_t=True)
    assert np.array_equal(t.view(np.uint32), t_ref.view(np.uint32))
    assert np.array_equal(img, ref), int((img != ref).any(axis=-1).sum())
    vol.close()


# ------------------------------------------------------------------ D. sharded and fused paths
DIMS_D = (48, 40, 64)


def sharded_wide(S, frames, exchange):
    from semtsdf.shard import LocalShardGroup

    semtsdf, L = S
    p = make_params(S, DIMS_D, frames, 0x3)
    vol = semtsdf.Volume(p, 0)
    shards = _shard_handles(S, p, 3, 5)
    steps = list(base_frames(frames, p)) + [(frames[2], pose(n, p), frames[2].gt_ids) for n in ("inside", "flip")]
    for fr, E, m in steps:
        for v in [vol] + shards:
            v.integrate(fr.depth, fr.rgb, m, E)
    for v in [vol] + shards:
        v.set_state(5, 7)
    return p, vol, shards, LocalShardGroup(shards, exchange=exchange)


@pytest.mark.parametrize("exchange", ["min", "allgather"])
def test_sharded_wide_poses(S, stream, exchange):
    """Three Z-slab shards of chunk 5 after the base frames and the `inside` and `flip` frames: the
    gathered planes equal the single volume, halo planes equal their owners, and the sharded
    raycast at angles whose rays cross the slabs back to front equals the single volume's."""
    from semtsdf.shard import ShardLayout

    st, frames = stream
    semtsdf, L = S
    p, vol, shards, grp = sharded_wide(S, frames, exchange)
    dims = DIMS_D
    lay = ShardLayout(dims[2], 3, 5)
    full = vol.download(hist=True)
    locs = [sh.download(hist=True) for sh in shards]
    for key, extra in (("sdf", ()), ("wt", ()), ("color", (3,)), ("hist", (32,))):
        parts = [lc[key].reshape((dims[0], dims[1], -1) + extra) for lc in locs]
        got = lay.gather(parts, dims[0], dims[1])
        ref = full[key].reshape(dims + extra)
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), key
        assert lay.check_halo(parts), key
    dist = mean_depth(frames)
    for mode in (L.RENDER_LABEL, L.RENDER_COLOR):
        for angle in ANGLES:
            s2w, c = semtsdf.orbit_camera(list(p.Kinv), angle, dist)
            img, t = vol.raycast(s2w, c, mode, want_t=True)
            simg, stt = grp.raycast(s2w, c, mode, want_t=True)
            assert (t >= 0).mean() > 0.1, angle
            assert np.array_equal(stt.view(np.uint32), t.view(np.uint32)), (mode, angle)
            assert np.array_equal(simg, img), (mode, angle)
    for sh in shards:
        sh.close()
    vol.close()


def test_sharded_association_opposite(S, stream):
    from semtsdf.volume import DeviceBuffer

    st, frames = stream
    p, vol, shards, grp = sharded_wide(S, frames, "min")
    E = pose("opposite", p)
    fr = frames[4]
    m_single = np.ascontiguousarray(fr.mask.copy())
    stats = vol.associate(m_single, E)
    assert not np.array_equal(m_single, fr.mask)  # the decision relabels something
    mbufs = [DeviceBuffer(NPX) for _ in shards]
    for mb in mbufs:
        mb.upload(fr.mask, grp.stream)
    for ss in grp.associate_dev([mb.ptr for mb in mbufs], E, want_stats=True):
        assert list(ss.assigned_prev) == list(stats.assigned_prev)
        assert ss.num_objs == stats.num_objs and bytes(ss.lut) == bytes(stats.lut)
    for mb in mbufs:
        got = np.zeros(NPX, np.uint8)
        mb.download(got, grp.stream)
        shards[0].sync()
        assert np.array_equal(got, m_single.reshape(-1))
    for sh in shards:
        sh.close()
    vol.close()


def test_fused_view_opposite(S, stream):
    """semtsdf_parse_frame_view_dev with the view at orbit angle pi and the frame at `opposite`
    (both marches of the fused launch run rays with dz < 0) equals the serial raycast,
    association and integrate: view, hit distances, relabelled mask and volume."""
    import torch

    semtsdf, L = S
    st, frames = stream
    dev = torch.device("cuda", 0)
    fr = frames[4]
    d_in = torch.from_numpy(fr.depth.reshape(-1).view(np.int16)).to(dev)
    r_in = torch.from_numpy(fr.rgb.reshape(-1)).to(dev)
    m_in = torch.from_numpy(np.ascontiguousarray(fr.mask).reshape(-1)).to(dev)
    torch.cuda.synchronize()

    def run(fused):
        p = make_params(S, (96, 96, 96), frames, 0x3)
        vol = semtsdf.Volume(p, 0)
        for f, E, m in base_frames(frames, p):
            vol.integrate(f.depth, f.rgb, m, E)
        vol.set_state(3, 7)
        E = pose("opposite", p)
        s2w, c = semtsdf.orbit_camera(list(p.Kinv), math.pi, mean_depth(frames))
        mask = m_in.clone()
        out = torch.zeros(NPX * 3, dtype=torch.uint8, device=dev)
        tt = torch.zeros(NPX, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        if fused:
            vol.parse_frame_view_dev(d_in.data_ptr(), r_in.data_ptr(), mask.data_ptr(), E, s2w, c, L.RENDER_LABEL,
                                     out.data_ptr(), tt.data_ptr())
        else:
            vol.raycast_dev(s2w, c, L.RENDER_LABEL, out.data_ptr(), tt.data_ptr())
            vol.parse_frame_dev(d_in.data_ptr(), r_in.data_ptr(), mask.data_ptr(), E)
        vol.sync()
        torch.cuda.synchronize()
        state = vol.download(hist=True)
        res = (out.cpu(), tt.cpu(), mask.cpu()), (vol.state().n_obs, vol.state().num_objs)
        vol.close()
        return res, state

    ((va, ta, ma), na), sa = run(False)
    ((vb, tb, mb), nb), sb = run(True)
    assert float((ta >= 0).float().mean()) > 0.1 and not torch.equal(ma, m_in.cpu())
    assert torch.equal(va, vb) and torch.equal(ta.view(torch.int32), tb.view(torch.int32)) and torch.equal(ma, mb)
    assert na == nb and na[0] == 4
    for key in ("sdf", "wt", "color", "hist"):
        assert np.array_equal(sa[key].view(np.uint8), sb[key].view(np.uint8)), key
