"""Weight storage on the device: uint16 per voxel until a weight could pass 65535, int32 from then
on (a one-way switch per volume, undone only by a reset).  The int32 boundary of upload and
download, the integrate and every reader of weights give the same values in both forms: checked
against the C oracle and the restatements of tests/.

The sharded and async paths run the narrow form by default in
test_gpu_parity.py::test_sharded_handles_equal_single_volume, test_async_prepass_* and
test_gpu_bench_config.py."""
import numpy as np
import pytest

import model_maps_restatement as R
from instances_restatement import assert_stats_equal, restate_stats
from mesh_restatement import assert_meshes_equal, canonical, restate_mesh

pytestmark = pytest.mark.gpu

KI = R.KI
U16_MAX = 65535
NAMES = ("t", "point", "normal", "label", "votes", "flags")


def assert_maps_equal(got, want, names):
    for n in names:
        g, w = got[n], want[n]
        assert g.shape == w.shape and g.dtype == w.dtype, n
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = g != w
        assert not bad.any(), (n, int(bad.sum()), np.argwhere(bad)[:3].tolist())


@pytest.fixture(scope="module")
def S():
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    return semtsdf, L


@pytest.fixture(scope="module")
def frames():
    from semtsdf.synth import SyntheticStream

    st = SyntheticStream(seed=0)
    return [st.frame(k) for k in range(7)]


def placed(S, dims, frame0, flags):
    semtsdf, L = S
    p = semtsdf.default_params(64, KI, 640, 480)
    p.dim[0], p.dim[1], p.dim[2] = dims
    semtsdf.place_from_frame(p, frame0.depth, float(np.mean(frame0.depth[frame0.depth > 0])) / 5000.0, L.PLACE_SFM)
    p.flags = flags
    return p


def assert_same(vol, ost):
    out = vol.download(hist=True)
    assert np.array_equal(out["sdf"].view(np.uint32), ost.sdf.view(np.uint32)), "sdf bits"
    assert np.array_equal(out["wt"], ost.wt), "weight"
    assert np.array_equal(out["color"], ost.color), "colour"
    assert np.array_equal(out["hist"], ost.hist), "histogram"


def test_integrate_across_the_u16_limit(S, oracle, frames):
    """Two frames, then every nonzero weight set to 65533 or 65534 by an upload (still uint16
    storage), then four more frames: the first brings weights to 65535 in narrow storage, the second
    could pass it and widens first.  Every array equals the oracle's after each frame, and
    device_bytes grows by 2 B per stored voxel exactly once."""
    semtsdf, L = S
    dims = (64, 64, 64)
    p = placed(S, dims, frames[0], 0x3)
    vol = semtsdf.Volume(p, 0)
    g = oracle.OGeom.from_params(p)
    ost = oracle.OState(list(dims), p.mu, semantic=True)

    def step(k):
        fr = frames[k]
        E = (fr.w2c @ frames[0].c2w).astype(np.float32)
        vol.integrate(fr.depth, fr.rgb, fr.mask, E)
        oracle.integrate(g, ost, list(p.K), E, fr.depth, fr.rgb, fr.mask, flags=0x3)

    for k in (1, 2):
        step(k)
    assert_same(vol, ost)
    narrow_bytes = vol.state().device_bytes
    idx = np.arange(ost.wt.size, dtype=np.int64)
    ost.wt[:] = np.where(ost.wt > 0, 65533 + idx % 2, 0).astype(np.int32)
    assert (ost.wt == 65533).any() and (ost.wt == 65534).any()
    vol.upload(wt=ost.wt)
    assert vol.state().device_bytes == narrow_bytes  # 65534 fits: still uint16
    assert np.array_equal(vol.download()["wt"], ost.wt)
    sizes = [narrow_bytes]
    for k in (3, 4, 5, 6):
        step(k)
        assert_same(vol, ost)
        sizes.append(vol.state().device_bytes)
    assert int(ost.wt.max()) > U16_MAX + 1  # the crossing happened, by more than one step
    nvox = 64 * 64 * 64  # 64^3 is whole 1 x 8 x 32 tiles: every stored voxel is a voxel of the volume
    grown = [b - a for a, b in zip(sizes, sizes[1:])]
    assert grown == [0, 2 * nvox, 0, 0], grown  # bound 65534 -> 65535 fits; 65535 -> 65536 does not
    # a reset volume holds uint16 weights again
    vol.reset()
    assert vol.state().device_bytes == narrow_bytes
    assert not vol.download()["wt"].any()
    vol.close()


@pytest.mark.parametrize("case", ["fits", "negative", "65536"])
def test_upload_decides_the_form(S, frames, case):
    """Ragged dims (padding rows and planes in y and z).  Weights in [0, 65535], both ends present,
    keep uint16 storage; one negative weight or one weight of 65536 switches to int32 storage before
    the transfer.  Each round-trips exactly through download, and a later upload of small weights
    into the wide volume does too (the switch is one way)."""
    semtsdf, L = S
    dims = (33, 20, 50)
    p = placed(S, dims, frames[0], 0x1)
    vol = semtsdf.Volume(p, 0)
    n = int(np.prod(dims))
    stored = int(vol.state().device_bytes)
    rng = np.random.default_rng(5)
    wt = rng.integers(0, U16_MAX + 1, n, dtype=np.int32)
    wt[7], wt[n - 1] = 0, U16_MAX
    if case == "negative":
        wt[n // 2] = -1
    if case == "65536":
        wt[n // 3] = U16_MAX + 1
    vol.upload(wt=wt)
    grown = int(vol.state().device_bytes) - stored
    # stored voxels of the tiled layout: y padded to 8 rows, z to 32 planes
    nvox = 33 * 24 * 64
    assert grown == (0 if case == "fits" else 2 * nvox), (case, grown)
    assert np.array_equal(vol.download()["wt"], wt), case
    small = rng.integers(0, 50, n, dtype=np.int32)
    vol.upload(wt=small)
    assert int(vol.state().device_bytes) - stored == grown
    assert np.array_equal(vol.download()["wt"], small), case
    vol.close()


def test_readers_in_both_forms(S):
    """render_maps (normals and flags at a min_weight that separates voxels), extract_mesh,
    export_surface and instance_stats on the fused 64^3 state of model_maps_restatement in narrow
    form, then again after an upload that adds 70000 to every nonzero weight (wide form) with
    min_weight raised by 70000: each equals its restatement on the downloaded arrays."""
    semtsdf, L = S
    sc = R.fused_scene()
    p, ost = sc["p"], sc["ost"]
    D = (64, 64, 64)
    vol = semtsdf.Volume(p, 0)
    for k in range(1, 4):
        fr = sc["frames"][k]
        vol.integrate(fr.depth, fr.rgb, fr.gt_ids, sc["E"][k])
    s2w, c = semtsdf.orbit_camera(list(p.Kinv), 0.2, sc["dist"])
    start, voxel = np.array(list(p.vol_start), np.float32), np.array(list(p.voxel), np.float32)
    mw, sdf_max = 2, 0.5
    assert (ost.wt == 1).any() and (ost.wt >= 2).any()  # min_weight 2 separates touched voxels
    exports = []
    for shift in (0, 70000):
        if shift:
            narrow_bytes = vol.state().device_bytes  # (the readers above allocated their scratch)
            vol.upload(wt=np.where(ost.wt > 0, ost.wt + shift, 0).astype(np.int32))
            assert vol.state().device_bytes == narrow_bytes + 2 * 64 ** 3  # int32 storage now
        out = vol.download(hist=True)
        assert np.array_equal(out["wt"], np.where(ost.wt > 0, ost.wt + shift, 0))
        sdf, wt = out["sdf"].reshape(D), out["wt"].reshape(D)
        color, hist = out["color"].reshape(D + (3,)), out["hist"].reshape(D + (32,))
        m = mw + shift
        got = vol.render_maps(s2w, c, m)
        want = R.restate_maps(got["t"], s2w, c, sdf, wt, hist, start, voxel, m)
        assert_maps_equal(got, want, NAMES)
        valid = (got["flags"] & 2) != 0
        hit = (got["flags"] & 1) != 0
        assert valid.any() and (hit & ~valid).any()  # the weight test decides both ways
        mesh = semtsdf.extract_mesh(vol, min_weight=m)
        assert_meshes_equal(canonical(mesh), restate_mesh(sdf, wt, color, hist, start, voxel, m))
        stats = vol.instance_stats(sdf_max, m, overlap=True)
        assert_stats_equal(stats, restate_stats(sdf, wt, color, hist, sdf_max, m))
        pts = semtsdf.export_surface(vol, sdf_max, m)
        sel = (wt >= m) & (np.abs(sdf) < np.float32(sdf_max))
        assert len(pts["label"]) == int(sel.sum()) == int(stats["voxels"].sum())
        assert np.array_equal(np.bincount(pts["label"], minlength=32), stats["voxels"].astype(np.int64))
        exports.append(pts)
    # the same voxels pass in both forms (weights and min_weight shifted together)
    assert sorted(exports[0]) == sorted(exports[1])
    for k in exports[0]:
        assert np.array_equal(exports[0][k], exports[1][k]), k
    vol.close()
