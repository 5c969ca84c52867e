"""Mesh export on the CPU: the mesh PLY writer and reader, merge_meshes, the properties of the
NumPy restatement of the extraction contract (tests/mesh_restatement.py) that the GPU tests
compare the device against, and the argument errors of semtsdf_extract_mesh."""
import os
import tempfile

import numpy as np

from mesh_restatement import random_field, restate_mesh

KI = (520.9, 521.0, 325.1, 249.7)


def _mesh(n, m, seed):
    rng = np.random.default_rng(seed)
    return {"vertices": rng.normal(size=(n, 3)).astype(np.float32),
            "voxel": rng.integers(0, 50, (n, 3)).astype(np.uint32), "edge": rng.integers(1, 8, n).astype(np.uint8),
            "rgb": rng.integers(0, 256, (n, 3), dtype=np.uint8), "label": rng.integers(0, 32, n).astype(np.uint8),
            "faces": rng.integers(0, max(n, 1), (m, 3)).astype(np.uint32)}


def test_mesh_ply_round_trip():
    from semtsdf.export import PALETTE, read_mesh_ply, write_mesh_ply

    mesh = _mesh(500, 900, 0)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "m.ply")
        write_mesh_ply(f, mesh)
        with open(f, "rb") as fh:
            head = fh.read(400)
        assert b"element face 900\nproperty list uchar uint vertex_indices\n" in head
        r = read_mesh_ply(f)
        assert np.array_equal(r["vertices"].view(np.uint32), mesh["vertices"].view(np.uint32))
        assert np.array_equal(r["faces"], mesh["faces"]) and r["faces"].dtype == np.uint32
        assert np.array_equal(r["rgb"], mesh["rgb"]) and np.array_equal(r["label"], mesh["label"])
        write_mesh_ply(f, mesh, color_by_label=True)
        r = read_mesh_ply(f)
        want = np.where((mesh["label"] > 0)[:, None], PALETTE[mesh["label"]], mesh["rgb"])
        assert np.array_equal(r["rgb"], want) and np.array_equal(r["faces"], mesh["faces"])
        write_mesh_ply(f, _mesh(0, 0, 0))  # empty mesh
        r = read_mesh_ply(f)
        assert r["vertices"].shape == (0, 3) and r["faces"].shape == (0, 3)


def test_merge_meshes_welds_equal_keys():
    from semtsdf.export import merge_meshes

    def make(keys, faces, tag):
        k = np.array(keys, np.uint32).reshape(-1, 4)
        n = len(k)
        return {"vertices": np.full((n, 3), tag, np.float32) + np.arange(n, dtype=np.float32)[:, None],
                "voxel": k[:, :3].copy(), "edge": k[:, 3].astype(np.uint8), "rgb": np.full((n, 3), tag, np.uint8),
                "label": np.full(n, tag, np.uint8), "faces": np.array(faces, np.uint32).reshape(-1, 3)}

    a = make([(0, 0, 7, 1), (0, 1, 7, 2), (1, 0, 8, 1), (1, 0, 8, 3)], [(0, 1, 2), (2, 1, 3)], 10)
    b = make([(1, 0, 8, 3), (2, 0, 9, 4), (1, 0, 8, 1)], [(0, 1, 2)], 20)  # shares a's vertices 3 and 2
    m = merge_meshes([a, b])
    keys = [(0, 0, 7, 1), (0, 1, 7, 2), (1, 0, 8, 1), (1, 0, 8, 3), (2, 0, 9, 4)]  # sorted, 7 -> 5 vertices
    got = [tuple(int(c) for c in v) + (int(e),) for v, e in zip(m["voxel"], m["edge"])]
    assert got == keys
    assert m["faces"].tolist() == [[0, 1, 2], [2, 1, 3], [3, 4, 2]]
    assert m["label"].tolist() == [10, 10, 10, 10, 20]  # the first occurrence is kept
    assert np.array_equal(m["vertices"][:4], a["vertices"]) and np.array_equal(m["vertices"][4], b["vertices"][1])
    c = make([(5, 5, 5, 1), (5, 5, 5, 2), (5, 5, 6, 1)], [(2, 0, 1)], 30)  # disjoint: concatenates
    m = merge_meshes([a, c])
    assert len(m["edge"]) == 7 and m["faces"].tolist() == [[0, 1, 2], [2, 1, 3], [6, 4, 5]]
    assert merge_meshes([])["faces"].shape == (0, 3)


def test_restatement_on_the_random_field():
    """The fixed 11 x 13 x 37 field: every (tet, sign case) occurs, the mesh is a manifold with
    boundary (an edge lies in 1 or 2 triangles), and the counts are pinned."""
    f = random_field()
    assert ((f["sdf"] == 0) & ~np.signbit(f["sdf"])).mean() > 0.01 and ((f["sdf"] == 0) & np.signbit(f["sdf"])).sum() > 20
    assert f["wt"].min() == 0 and f["wt"].max() == 4
    m = restate_mesh(f["sdf"], f["wt"], f["color"], f["hist"], np.array([-0.3, 0.1, 0.5], np.float32),
                     np.array([0.011, 0.012, 0.013], np.float32))
    st = m["stats"]
    assert (st["valid_cells"], len(m["faces"]), len(m["vertices"])) == (1159, 8788, 7098)
    assert st["combos"].shape == (6, 16) and st["combos"].min() >= 53
    assert (st["combos"].sum(axis=1) == 1159).all()
    assert st["t01"] == 404
    fa = m["faces"].astype(np.int64)
    e = np.sort(np.concatenate([fa[:, [0, 1]], fa[:, [1, 2]], fa[:, [2, 0]]]), axis=1)
    _, uses = np.unique(e, axis=0, return_counts=True)
    assert uses.min() == 1 and uses.max() == 2
    assert np.array_equal(np.unique(fa), np.arange(len(m["vertices"])))  # every vertex referenced
    m3 = restate_mesh(f["sdf"], f["wt"], f["color"], f["hist"], np.zeros(3, np.float32), np.ones(3, np.float32),
                      min_weight=3)
    assert 0 < len(m3["faces"]) < len(m["faces"])


def test_restatement_on_the_export_configuration(oracle):
    """The volume of test_export (48 x 40 x 64, synthetic frames 1-3, flags 0x3), fused by the CPU
    oracle: 11258 triangles on 6253 vertices, wound towards the camera side."""
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream

    O = oracle
    st = SyntheticStream(seed=0)
    frames = [st.frame(k) for k in range(4)]
    p = semtsdf.default_params(64, KI, 640, 480)
    p.dim[0], p.dim[1], p.dim[2] = 48, 40, 64
    semtsdf.place_from_frame(p, frames[0].depth, float(np.mean(frames[0].depth[frames[0].depth > 0])) / 5000.0,
                             L.PLACE_SFM)
    p.flags = 0x3
    g = O.OGeom.from_params(p)
    ost = O.OState(list(p.dim), p.mu, semantic=True)
    for k in range(1, 4):
        fr = frames[k]
        E = (fr.w2c @ frames[0].c2w).astype(np.float32)
        O.integrate(g, ost, list(p.K), E, fr.depth, fr.rgb, np.ascontiguousarray(fr.mask), flags=0x3)
    D = (48, 40, 64)
    m = restate_mesh(ost.sdf.reshape(D), ost.wt.reshape(D), ost.color.reshape(D + (3,)), ost.hist.reshape(D + (32,)),
                     np.array(list(p.vol_start), np.float32), np.array(list(p.voxel), np.float32))
    assert (len(m["faces"]), len(m["vertices"])) == (11258, 6253)
    # normals point into free space: sdf grows along them (the gradient at the owner voxel, central in x)
    v = m["vertices"].astype(np.float64)
    fa = m["faces"].astype(np.int64)
    n = np.cross(v[fa[:, 1]] - v[fa[:, 0]], v[fa[:, 2]] - v[fa[:, 0]])
    sdf = ost.sdf.reshape(D).astype(np.float64)
    grad = np.stack(np.gradient(sdf), axis=-1)
    o = m["voxel"][fa[:, 0]].astype(np.int64)
    dots = (n * grad[o[:, 0], o[:, 1], o[:, 2]]).sum(axis=1)
    assert (dots > 0).sum() > 0.9 * (dots != 0).sum()


def test_extract_mesh_argument_errors_without_a_device():
    import ctypes as C

    from semtsdf import _lib as L

    lib = L.load()
    nv, nt = C.c_uint64(), C.c_uint64()
    assert C.sizeof(L.MeshVertex) == 32
    rc = lib.semtsdf_extract_mesh(None, 1, None, 0, None, 0, C.byref(nv), C.byref(nt))
    assert rc == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    handle = C.c_void_p(0x1000)  # never dereferenced: the count pointers are checked first
    rc = lib.semtsdf_extract_mesh(handle, 1, None, 0, None, 0, None, C.byref(nt))
    assert rc == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
    rc = lib.semtsdf_extract_mesh(handle, 1, None, 0, None, 0, C.byref(nv), None)
    assert rc == L.ERR_INVALID and b"NULL" in lib.semtsdf_last_error()
