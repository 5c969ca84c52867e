"""The kernels that walk the stored volume, past their first trip, group and chunk: two volumes
(tests/long_walk_fields.py; tests/test_long_walks.py proves on the CPU that every trip, group and
chunk they reach holds compared values) filled by upload, every result compared exactly with the
NumPy restatements and the C oracle applied to the uploaded arrays, never to a download.

Why a broken second trip, group or chunk changes a compared value ("Long walks"):
  hist_chunk, vox/color_upload_trip, color_chunk: a chunk or trip written at a wrong base or with
      a wrong stride leaves voxels of the download unequal to the upload (random colours everywhere,
      votes and weights in both chunks and trips).
  hist_mask_trip: an upload leaves the bin mask all ones until k_hist_mask rewrites it; a word the
      second trip misses counts 32 present bins in `support` and `overlap`.
  instance_trip: a tile the loop misses or visits twice changes `voxels` and every sum.
  mesh_group: gsum of a wrong group, or a prefix that skips the empty groups, moves every later
      vertex and triangle base: faces index wrong vertices and the totals change.
  export_trip: a missed tail loses its selected voxels; the sorted points are compared one by one.
  remap_trip: a voxel the second trip misses keeps its old counts and its old mask word.
  weight/color_widen_trip: a voxel not converted holds whatever the new allocation held; the
      untouched voxels at x >= 256 are compared with the uploaded values.
  min_i64_trip: an element past the first 1 048 576 that is skipped keeps dst, which differs from
      the minimum wherever src is smaller."""
from concurrent.futures import ThreadPoolExecutor

import ctypes as C

import numpy as np
import pytest

import long_walk_fields as F
from instances_restatement import HAZARD_LUT, assert_stats_equal, remap_hist, restate_stats
from mesh_restatement import assert_meshes_equal, canonical, restate_mesh

pytestmark = pytest.mark.gpu

KI = (520.9, 521.0, 325.1, 249.7)
START, VOXEL = (-0.3, 0.1, 0.5), (0.011, 0.012, 0.013)  # _field_params of test_gpu_mesh.py
U16_MAX = 65535


@pytest.fixture(scope="module")
def S():
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    return semtsdf, L


def params(semtsdf, dims, flags):
    p = semtsdf.default_params(64, KI, 640, 480)
    for a in range(3):
        p.dim[a] = dims[a]
        p.vol_start[a], p.voxel[a] = START[a], VOXEL[a]
        p.vol_end[a] = START[a] + VOXEL[a] * (dims[a] - 1)
    p.mu = 0.05
    p.flags = flags
    return p


def build(S, V):
    """The volume of V, uploaded; the uploaded arrays in the shapes the restatements take."""
    semtsdf, L = S
    dims = V["dims"]
    sem = bool(V["flags"] & 1)
    sdf, wt, color, hist = F.band_field(dims, V["seed"], V["gaps"], sem)
    if V["flags"] & 4:
        color = color.astype(np.int32)  # the int32 boundary; values in [0, 255] keep byte storage
    vol = semtsdf.Volume(params(semtsdf, dims, V["flags"]), 0)
    vol.upload(sdf=sdf, wt=wt, color=color, hist=hist)
    return {"vol": vol, "dims": dims, "sdf": sdf, "wt": wt, "color": color, "hist": hist,
            "rows": F.vote_rows(hist) if sem else None, "hist_bm": F.bin_major(hist) if sem else None,
            "start": np.array(START, np.float32), "voxel": np.array(VOXEL, np.float32)}


@pytest.fixture(scope="module")
def A(S):
    a = build(S, F.VOLUME_A)
    a["vol"].set_state(5, 32)
    yield a
    a["vol"].close()


@pytest.fixture(scope="module")
def B(S):
    b = build(S, F.VOLUME_B)
    yield b
    b["vol"].close()


def assert_download_equals(vol, f, hist):
    out = vol.download(hist=hist)
    assert np.array_equal(out["sdf"].view(np.uint32), f["sdf"].reshape(-1).view(np.uint32)), "sdf bits"
    assert np.array_equal(out["wt"], f["wt"].reshape(-1)), "weight"
    assert out["color"].dtype == f["color"].dtype and np.array_equal(out["color"], f["color"].reshape(-1)), "colour"
    if hist:
        assert np.array_equal(out["hist"], f["hist"].reshape(-1)), "histogram"
    return out


def check_mesh(semtsdf, lib, f, min_weight, counts=None):
    want = restate_mesh(f["sdf"], f["wt"], f["color"], f["hist"], f["start"], f["voxel"], min_weight)
    if counts is not None:
        assert (len(want["vertices"]), len(want["faces"])) == counts
    nv, nt = C.c_uint64(), C.c_uint64()
    assert lib.semtsdf_extract_mesh(f["vol"].handle, min_weight, None, 0, None, 0, C.byref(nv), C.byref(nt)) == 0
    assert (int(nv.value), int(nt.value)) == (len(want["vertices"]), len(want["faces"]))  # the count-only call
    got = semtsdf.extract_mesh(f["vol"], min_weight=min_weight)
    assert int(got["faces"].max()) < len(got["vertices"])
    assert_meshes_equal(canonical(got), want)


def check_export(semtsdf, f, sdf_max, min_weight, hist_labels):
    """export_surface against the NumPy selection in reference order: index, sdf bits, colour, label."""
    pts = semtsdf.export_surface(f["vol"], sdf_max, min_weight)
    sel = (f["wt"] >= min_weight) & (np.abs(f["sdf"]) < np.float32(sdf_max))
    want = np.argwhere(sel).astype(np.uint32)  # sorted by (x, y, z): the reference order
    assert len(pts["index"]) == len(want)
    idx = pts["index"].astype(np.int64)
    order = np.argsort(F.ref_index(f["dims"], idx[:, 0], idx[:, 1], idx[:, 2]), kind="stable")
    assert np.array_equal(pts["index"][order], want)
    x, y, z = want[:, 0], want[:, 1], want[:, 2]
    assert np.array_equal(pts["sdf"][order].view(np.uint32), f["sdf"][x, y, z].view(np.uint32))
    assert np.array_equal(pts["rgb"][order], np.clip(f["color"][x, y, z], 0, 255).astype(np.uint8))
    assert np.array_equal(pts["label"][order], hist_labels[x, y, z].astype(np.uint8))
    trips = np.bincount(F.trip_of("export_trip", f["dims"], x, y, z), minlength=F.trip_count("export_trip", f["dims"]))
    return pts, trips


# ------------------------------------------------------------------------------------ volume A
def test_a_download_equals_the_upload(A):
    """hist_xfer's second upload chunk (k_hist_to_bm with v0 = 2^22, the boundary inside x layer 582)
    and k_vox_from_ref's second trip, against the download that the 512^3 oracle comparison covers."""
    assert_download_equals(A["vol"], A, hist=True)


@pytest.mark.parametrize("sdf_max,min_weight,overlap", [(0.5, 2, True), (0.2, 1, False)])
def test_a_instance_stats_equal_the_restatement(A, sdf_max, min_weight, overlap):
    """k_instance_stats' three trips (the last partial), and k_hist_mask's second trip: the upload
    left every mask word all ones, so a word it missed would add 32 to support."""
    want = restate_stats(A["sdf"], A["wt"], A["color"], A["hist_bm"], sdf_max, min_weight)
    got = A["vol"].instance_stats(sdf_max, min_weight, overlap=overlap)
    assert_stats_equal(got, want, overlap=overlap)
    assert int(want["voxels"].sum()) > 40000 and (want["support"] > 0).all()
    if overlap:
        A["stats"] = want


def test_a_mesh_equals_the_restatement(S, A):
    """Five scan groups, the second empty between nonzero ones and the last partial: vertex and
    triangle bases of groups 2-4 are sums over gsum of the groups before them."""
    semtsdf, L = S
    lib = semtsdf.load()
    check_mesh(semtsdf, lib, A, 1, (141027, 200042))
    check_mesh(semtsdf, lib, A, 3, (964, 800))


def test_a_export_equals_the_selection(S, A):
    """export_surface(0.5, 2) point by point, its labels the argmax of the uploaded histogram, its
    label counts the inventory's voxels."""
    semtsdf, L = S
    want = A.get("stats") or restate_stats(A["sdf"], A["wt"], A["color"], A["hist_bm"], 0.5, 2)
    pts, _ = check_export(semtsdf, A, 0.5, 2, want["label"])
    assert np.array_equal(np.bincount(pts["label"], minlength=32), want["voxels"].astype(np.int64))


def remapped(A):
    """The remap of A through HAZARD_LUT, once: the rows with votes and their restated histogram."""
    if "remap" not in A:
        h, rows = A["hist"].reshape(-1, 32), A["rows"]
        want = remap_hist(h[rows], HAZARD_LUT)
        changed = (want != h[rows]).any(axis=1)
        x, y, z = np.unravel_index(rows[changed], A["dims"])
        assert np.bincount(F.trip_of("remap_trip", A["dims"], x, y, z), minlength=2).tolist() == [72742, 16110]
        A["vol"].remap_instances(HAZARD_LUT, 31)
        A["remap"] = (rows, want)
    return A["remap"]


def test_a_remap_in_both_trips(A):
    """After every reader of A's uploaded state (it rewrites the histogram).  k_remap_instances'
    second trip: the downloaded histogram equals remap_hist of the uploaded one (restated on the
    rows with votes; no other row gains a vote), sdf, weights and colours are untouched."""
    rows, want = remapped(A)
    st = A["vol"].state()
    assert (st.n_obs, st.num_objs) == (5, 31)
    out = A["vol"].download(hist=True)
    got = out["hist"].reshape(-1, 32)
    assert np.array_equal(got[rows], want)
    assert np.count_nonzero(got) == np.count_nonzero(want)  # and nothing anywhere else
    for k in ("sdf", "wt", "color"):
        assert out[k].tobytes() == A[k].tobytes(), k


def test_a_inventory_after_the_remap(A):
    """The inventory after the remap equals the restatement of the new arrays: the mask words of
    the second trip were rebuilt (a stale word keeps the bins 7, 9 and 31 in `support`)."""
    rows, want = remapped(A)
    new = np.zeros((32, A["hist"].size // 32), np.uint32)  # bin-major, as A["hist_bm"]
    new[:, rows] = want.T
    new = np.moveaxis(new.reshape((32,) + A["dims"]), 0, -1)
    stats = A["vol"].instance_stats(0.5, 2, overlap=True)
    assert_stats_equal(stats, restate_stats(A["sdf"], A["wt"], A["color"], new, 0.5, 2))
    assert not stats["support"][[7, 9, 31]].any() and stats["support"][5] > 0 and stats["support"][6] > 0


# ------------------------------------------------------------------------------------ volume B
def test_b_download_equals_the_upload(B):
    """color_xfer's second upload chunk (int32 boundary, byte storage, the boundary inside x layer
    268) and the twelve trips of k_color_from_ref inside the first."""
    assert_download_equals(B["vol"], B, hist=False)


def test_b_export_equals_the_selection(S, B):
    """k_export_surface's second trip: 5114 of the selected voxels lie past reference voxel 2^24."""
    semtsdf, L = S
    _, trips = check_export(semtsdf, B, 0.5, 2, np.zeros(B["dims"], np.uint8))
    assert trips.tolist() == [94972, 5114]


def test_b_mesh_equals_the_restatement(S, B):
    """Eighteen scan groups, eight of them empty in a row, the last partial."""
    semtsdf, L = S
    check_mesh(semtsdf, semtsdf.load(), B, 1, (230470, 285274))


@pytest.fixture(scope="module")
def BW(B, oracle):
    """What the two widening tests share, set up after every reader of B's uploaded state (it
    integrates): the oracle's state of B after one frame on the uploaded weights 1..4 (no widening;
    the handle allocates its frame staging there, once), the observed voxels, and frame(k), which
    integrates synthetic frame k on the device and in the oracle (x slabs in a thread pool).  The
    camera stands at the origin and sees no voxel at x >= 256."""
    from semtsdf.synth import SyntheticStream

    vol, dims = B["vol"], B["dims"]
    p = vol.params
    g = oracle.OGeom.from_params(p)
    ost = oracle.OState(list(dims), p.mu, color_i32=True)
    ost.sdf[:], ost.wt[:], ost.color[:] = B["sdf"].reshape(-1), B["wt"].reshape(-1), B["color"].reshape(-1)
    st = SyntheticStream(seed=0)
    frames = {k: st.frame(k) for k in (1, 2, 3)}
    E = np.eye(4, dtype=np.float32)
    slabs = [(x, min(x + 12, dims[0])) for x in range(0, dims[0], 12)]

    def frame(k):
        fr = frames[k]
        vol.integrate(fr.depth, fr.rgb, None, E)
        with ThreadPoolExecutor(8) as ex:
            counts = list(ex.map(lambda r: oracle.integrate(g, ost, list(p.K), E, fr.depth, fr.rgb, None,
                                                            flags=0x4, x_range=r), slabs))
        return sum(int(c[0]) for c in counts)

    frame(3)
    return ost, frame, np.flatnonzero(B["wt"].reshape(-1) > 0)


def widen_step(B, BW, k, top, names):
    """Weights top, top - 1 and top - 2 on the observed voxels, uploaded; then frame k.  Returns the
    growth of device_bytes over the upload and over the frame, after comparing the arrays `names`
    with the oracle's."""
    vol, dims = B["vol"], B["dims"]
    ost, frame, obs = BW
    far = slice(256 * dims[1] * dims[2], None)  # x >= 256: the second trip of both widening kernels
    ost.wt[:] = 0
    ost.wt[obs] = (top - obs % 3).astype(np.int32)
    assert (ost.wt[far] == top).sum() > 1000
    seeded = ost.wt[far].copy()
    sizes = [int(vol.state().device_bytes)]
    vol.upload(wt=ost.wt)
    sizes.append(int(vol.state().device_bytes))
    touched = frame(k)
    sizes.append(int(vol.state().device_bytes))
    assert touched > 100000 and (ost.wt == top + 1).sum() > 1000  # the limit is crossed
    assert np.array_equal(ost.wt[far], seeded)  # untouched at x >= 256
    out = vol.download(**{n: n in names for n in ("sdf", "wt", "color")})
    for n in names:
        assert np.array_equal(out[n].view(np.uint32), getattr(ost, n).view(np.uint32)), (k, n)
    return sizes[1] - sizes[0], sizes[2] - sizes[1]


def test_b_weight_widening_in_both_trips(B, BW):
    """Weights up to 65535 on the observed voxels, x >= 256 included, keep uint16 storage; the next
    integrate could pass 65535 and widens first (k_weight_widen, two trips, the boundary at x = 256):
    exactly 2 B more per stored voxel.  Every array then equals the C oracle's, and the voxels at
    x >= 256 carry the converted values."""
    assert widen_step(B, BW, 1, U16_MAX, ("sdf", "wt", "color")) == (0, 2 * F.stored_voxels(B["dims"]))


def test_b_colour_widening_in_both_trips(B, BW):
    """Weights of 2^23 - 1: the next integrate widens the byte colours to int32 x 4 first
    (k_color_widen, two trips): exactly 12 B more per stored voxel; colours and weights equal the
    oracle's (the upload itself widens the weights when this test runs alone)."""
    assert widen_step(B, BW, 2, (1 << 23) - 1, ("wt", "color"))[1] == 12 * F.stored_voxels(B["dims"])


# ---------------------------------------------------------------------------------- stand-alone
@pytest.mark.parametrize("n", [F.unit("min_i64_trip") + 77, 307200])
def test_min_i64_past_one_trip(S, n):
    """semtsdf_min_i64 over one trip of its 4096 x 256 grid plus 77 elements, and below one trip (the
    record count of a 640 x 480 frame, shard.py's use): np.minimum, with INT64_MIN and INT64_MAX in
    both operands."""
    from semtsdf.volume import DeviceBuffer

    semtsdf, L = S
    lib = semtsdf.load()
    rng = np.random.default_rng(n)
    info = np.iinfo(np.int64)
    a = rng.integers(info.min, info.max, n, dtype=np.int64, endpoint=True)
    b = rng.integers(info.min, info.max, n, dtype=np.int64, endpoint=True)
    ext = np.array([info.min, info.max, info.min, info.max, 0, -1], np.int64)
    for arr, vals, at in ((a, ext, 0), (b, ext[[2, 3, 1, 0, -1, 4]], 0), (a, ext, n - 6), (b, ext[::-1], n - 6)):
        arr[at:at + 6] = vals
    want = np.minimum(a, b)
    assert (want[-77:] != a[-77:]).sum() > 10  # the tail changes: a skipped element would show
    da, db = DeviceBuffer(n * 8), DeviceBuffer(n * 8)
    da.upload(a)
    db.upload(b)
    L.check(lib.semtsdf_min_i64(C.c_void_p(da.ptr), C.c_void_p(db.ptr), n, None))
    got, src = np.zeros(n, np.int64), np.zeros(n, np.int64)
    da.download(got)
    db.download(src)
    L.check(lib.semtsdf_stream_sync(None))
    assert np.array_equal(got, want) and np.array_equal(src, b)
    da.free()
    db.free()
