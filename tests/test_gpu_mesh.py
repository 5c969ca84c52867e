"""semtsdf_extract_mesh on the device against the NumPy restatement of its contract
(tests/mesh_restatement.py) applied to the downloaded volume: vertices canonicalised by key,
triangles rotated to their smallest index, then everything compared exactly (positions as bits)."""
import ctypes as C

import numpy as np
import pytest

from mesh_restatement import assert_meshes_equal, canonical, random_field, restate_mesh

KI = (520.9, 521.0, 325.1, 249.7)
FIELD_DIMS = (11, 13, 37)  # crosses the 8-row, 4-plane and 32-plane tile boundaries; padded in y and z


def _field_params(flags):
    import semtsdf

    p = semtsdf.default_params(64, KI, 640, 480)
    start, voxel = (-0.3, 0.1, 0.5), (0.011, 0.012, 0.013)
    for a in range(3):
        p.dim[a] = FIELD_DIMS[a]
        p.vol_start[a], p.voxel[a] = start[a], voxel[a]
        p.vol_end[a] = start[a] + voxel[a] * (FIELD_DIMS[a] - 1)
    p.mu = 0.05
    p.flags = flags
    return p


def _restate(vol, dims, min_weight=1):
    """The restatement on what the volume itself holds (download())."""
    p = vol.params
    sem = bool(p.flags & 1)
    out = vol.download(hist=sem)
    D = tuple(dims)
    return restate_mesh(out["sdf"].reshape(D), out["wt"].reshape(D), out["color"].reshape(D + (3,)),
                        out["hist"].reshape(D + (32,)) if sem else None, np.array(list(p.vol_start), np.float32),
                        np.array(list(p.voxel), np.float32), min_weight)


def _fused(dims, nshards):
    """Synthetic frames 1-3 into a volume of `dims` placed from frame 0 (test_export's
    configuration), flags 0x3: the single volume and, for nshards > 1, its z_chunk = 8 shards."""
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream

    st = SyntheticStream(seed=0)
    frames = [st.frame(k) for k in range(4)]
    p = semtsdf.default_params(64, KI, 640, 480)
    p.dim[0], p.dim[1], p.dim[2] = dims
    semtsdf.place_from_frame(p, frames[0].depth, float(np.mean(frames[0].depth[frames[0].depth > 0])) / 5000.0,
                             L.PLACE_SFM)
    p.flags = 0x3
    vols = [semtsdf.Volume(p, 0)]
    for sidx in range(nshards if nshards > 1 else 0):
        q = semtsdf.default_params(64, KI, 640, 480)
        for fld in ("dim", "vol_start", "vol_end", "voxel", "K", "Kinv"):
            getattr(q, fld)[:] = getattr(p, fld)[:]
        q.mu, q.flags = p.mu, p.flags
        q.z_nshards, q.z_shard, q.z_chunk = nshards, sidx, 8
        vols.append(semtsdf.Volume(q, 0))
    for k in range(1, 4):
        fr = frames[k]
        E = (fr.w2c @ frames[0].c2w).astype(np.float32)
        for v in vols:
            v.integrate(fr.depth, fr.rgb, np.ascontiguousarray(fr.mask), E)
    return vols[0], vols[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0x3, 0x4, 0x5, 0xC])
def test_random_field_mesh_equals_restatement(flags):
    """The fixed random field uploaded into a semantic u8 volume, COLOR_I32 volumes (int32 colours
    outside [0, 255]: the clamp) and a vote volume (no histogram: label 0): the mesh equals the
    restatement at min_weight 1 and 3 (the weights span 1..4); without a sign change it is empty."""
    import semtsdf

    semtsdf.load()
    f = random_field(FIELD_DIMS)
    vol = semtsdf.Volume(_field_params(flags), 0)
    color = f["color"] if flags & 4 else np.clip(f["color"], 0, 255).astype(np.uint8)
    vol.upload(sdf=f["sdf"], wt=f["wt"], color=color, hist=f["hist"] if flags & 1 else None)
    for mw in (1, 3):
        want = _restate(vol, FIELD_DIMS, mw)
        got = semtsdf.extract_mesh(vol, min_weight=mw)
        assert got["vertices"].dtype == np.float32 and got["faces"].dtype == np.uint32
        assert_meshes_equal(canonical(got), want)
        if mw == 1:  # the restatement of the uploaded arrays themselves: the counts of tests/test_mesh.py
            assert (len(want["faces"]), len(want["vertices"])) == (8788, 7098)
            assert bool(want["label"].any()) == bool(flags & 1)
            if flags & 4:
                assert (f["color"] > 255).any() and (f["color"] < 0).any()
    vol.upload(sdf=np.abs(f["sdf"]) + np.float32(0.1))
    got = semtsdf.extract_mesh(vol)
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)
    vol.close()


@pytest.mark.gpu
def test_fused_volume_mesh_equals_restatement():
    """test_export's fused volume (48 x 40 x 64, frames 1-3, flags 0x3): the mesh equals the
    restatement, has more than 5000 triangles, and indexes every vertex."""
    import semtsdf

    semtsdf.load()
    vol, _ = _fused((48, 40, 64), 1)
    want = _restate(vol, (48, 40, 64))
    got = semtsdf.extract_mesh(vol)
    n = len(got["vertices"])
    assert len(got["faces"]) > 5000
    assert int(got["faces"].max()) < n
    assert np.array_equal(np.unique(got["faces"]), np.arange(n))
    assert (got["edge"] >= 1).all() and (got["edge"] <= 7).all()
    assert_meshes_equal(canonical(got), want)
    vol.close()


@pytest.mark.gpu
def test_shard_meshes_merge_to_the_single_volume_mesh():
    """48 x 40 x 70 in 2 shards of z_chunk 8 (the last chunk partial): merge_meshes of the shards'
    meshes equals the single volume's mesh, and the halo-plane vertices both shards emit carry
    identical bytes."""
    import semtsdf

    semtsdf.load()
    single, shards = _fused((48, 40, 70), 2)
    whole = semtsdf.extract_mesh(single)
    parts = [semtsdf.extract_mesh(v) for v in shards]
    assert len(whole["faces"]) > 5000 and all(len(m["faces"]) > 0 for m in parts)
    assert sum(len(m["faces"]) for m in parts) == len(whole["faces"])
    assert sum(len(m["edge"]) for m in parts) > len(whole["edge"])  # the halo-plane vertices are in both
    assert_meshes_equal(canonical(semtsdf.merge_meshes(parts)), canonical(whole))
    assert_meshes_equal(canonical(semtsdf.merge_meshes(parts[::-1])), canonical(whole))  # whichever copy is kept
    for v in shards + [single]:
        v.close()


@pytest.mark.gpu
def test_mesh_determinism_capacity_and_untouched_state():
    """Two calls return identical bytes; a count-only call agrees with the full call; short
    capacities return ERR_INVALID with the counts and leave the buffers alone; extraction does
    not modify the volume."""
    import semtsdf
    from semtsdf import _lib as L

    lib = semtsdf.load()
    f = random_field(FIELD_DIMS)
    vol = semtsdf.Volume(_field_params(0x3), 0)
    vol.upload(sdf=f["sdf"], wt=f["wt"], color=np.clip(f["color"], 0, 255).astype(np.uint8), hist=f["hist"])
    before = vol.download(hist=True)
    nv, nt = C.c_uint64(), C.c_uint64()
    assert lib.semtsdf_extract_mesh(vol.handle, 1, None, 0, None, 0, C.byref(nv), C.byref(nt)) == 0
    n, m = int(nv.value), int(nt.value)
    assert (n, m) == (7098, 8788)

    def full(vcap, tcap):
        verts = np.full(n * 32, 0xA5, np.uint8)
        tris = np.full(m * 3, 0xA5A5A5A5, np.uint32)
        a, b = C.c_uint64(), C.c_uint64()
        rc = lib.semtsdf_extract_mesh(vol.handle, 1, verts.ctypes.data, vcap, tris.ctypes.data, tcap, C.byref(a),
                                      C.byref(b))
        return rc, verts, tris, int(a.value), int(b.value)

    rc, v1, t1, a, b = full(n, m)
    assert rc == 0 and (a, b) == (n, m)
    rc, v2, t2, a, b = full(n + 5, m + 7)  # larger capacities: the same bytes
    assert rc == 0 and (a, b) == (n, m)
    assert v1.tobytes() == v2.tobytes() and t1.tobytes() == t2.tobytes()
    assert not (v1.reshape(n, 32)[:, 29:] != 0).any()  # pad = 0
    for vcap, tcap in ((n - 1, m), (n, m - 1), (0, 0)):
        rc, v3, t3, a, b = full(vcap, tcap)
        assert rc == L.ERR_INVALID and (a, b) == (n, m)
        assert (v3 == 0xA5).all() and (t3 == 0xA5A5A5A5).all()
    rc = lib.semtsdf_extract_mesh(vol.handle, 1, v1.ctypes.data, n, None, m, C.byref(nv), C.byref(nt))
    assert rc == L.ERR_INVALID
    after = vol.download(hist=True)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    vol.close()
