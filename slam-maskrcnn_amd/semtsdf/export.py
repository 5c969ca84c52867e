"""Surface export of a fused volume (the reference keeps no export of its
own -- its volume layout is src/TSDF_Python/tsdf.py:48-52 and the voxel position rule
src/SfM_CUDA/tsdf.cu:30): the labelled surface voxels as a point cloud, and the labelled
triangle mesh of the sdf = 0 level set (semtsdf_extract_mesh), both written as PLY."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

# the palette of the label render (viewer.cu:93-126), RGB
PALETTE = np.array([
    230, 25, 75, 60, 180, 75, 255, 225, 25, 0, 130, 200, 245, 130, 48, 145, 30, 180, 70, 240, 240, 240, 50, 230,
    210, 245, 60, 250, 190, 190, 0, 128, 128, 230, 190, 255, 170, 110, 40, 255, 250, 200, 128, 0, 0, 170, 255, 195,
    230, 25, 75, 60, 180, 75, 255, 225, 25, 0, 130, 200, 245, 130, 48, 145, 30, 180, 70, 240, 240, 240, 50, 230,
    210, 245, 60, 250, 190, 190, 0, 128, 128, 230, 190, 255, 170, 110, 40, 255, 250, 200, 128, 0, 0, 170, 255, 195,
], np.uint8).reshape(32, 3)


def export_surface(vol, sdf_max: float = 0.2, min_weight: int = 1) -> dict:
    """Surface voxels of `vol` (a Volume; a shard exports its owned planes): weight >= min_weight
    and |sdf| < sdf_max.  Returns index [n, 3] u32 (global voxel index, the reference's flat
    order), xyz [n, 3] f32 world position vol_start + index * voxel rounded once (tsdf.cu:30's
    fmaf), sdf [n] f32, rgb [n, 3] u8, label [n] u8."""
    lib = L.load()
    n = C.c_uint64()
    L.check(lib.semtsdf_export_surface(vol.handle, float(sdf_max), int(min_weight), None, 0, C.byref(n)))
    pts = (L.SurfacePoint * max(int(n.value), 1))()
    if n.value:
        L.check(lib.semtsdf_export_surface(vol.handle, float(sdf_max), int(min_weight), C.cast(pts, C.c_void_p),
                                           int(n.value), C.byref(n)))
    a = np.frombuffer(pts, dtype=np.dtype([("x", "<u4"), ("y", "<u4"), ("z", "<u4"), ("sdf", "<f4"),
                                           ("r", "u1"), ("g", "u1"), ("b", "u1"), ("label", "u1")]))[:int(n.value)]
    idx = np.stack([a["x"], a["y"], a["z"]], axis=1).astype(np.uint32)
    p = vol.params
    start = np.array(list(p.vol_start), np.float32).astype(np.float64)
    voxel = np.array(list(p.voxel), np.float32).astype(np.float64)
    # idx * voxel + start is exact in double (a 16-bit index times a 24-bit float, plus a float):
    # rounding it once to f32 is the fused multiply-add of tsdf.cu:30
    xyz = (idx.astype(np.float64) * voxel + start).astype(np.float32)
    return {"index": idx, "xyz": xyz, "sdf": a["sdf"].copy(), "rgb": np.stack([a["r"], a["g"], a["b"]], axis=1),
            "label": a["label"].copy()}


_MESH_VERTEX = np.dtype([("pos", "<f4", (3,)), ("voxel", "<u4", (3,)), ("rgb", "u1", (3,)), ("label", "u1"),
                         ("edge", "u1"), ("pad", "u1", (3,))])
_MESH_KEYS = ("vertices", "voxel", "edge", "rgb", "label")
_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                        ("label", "u1")])
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<u4", (3,))])


def _mesh_dict(rec: np.ndarray, faces: np.ndarray) -> dict:
    return {"vertices": np.ascontiguousarray(rec["pos"]), "voxel": np.ascontiguousarray(rec["voxel"]),
            "edge": rec["edge"].copy(), "rgb": np.ascontiguousarray(rec["rgb"]), "label": rec["label"].copy(),
            "faces": faces}


def extract_mesh(vol, min_weight: int = 1) -> dict:
    """The labelled triangle mesh of `vol`'s sdf = 0 level set (semtsdf_extract_mesh: marching
    tetrahedra over the cells whose 8 corners have weight >= min_weight; a shard extracts the
    cells whose min-corner plane it owns -- merge_meshes joins a group's).  Returns vertices
    [n, 3] f32, voxel [n, 3] u32 and edge [n] u8 (the vertex's key: owner voxel, global index,
    and edge class 1..7), rgb [n, 3] u8, label [n] u8, faces [m, 3] u32."""
    lib = L.load()
    nv, nt = C.c_uint64(), C.c_uint64()
    L.check(lib.semtsdf_extract_mesh(vol.handle, int(min_weight), None, 0, None, 0, C.byref(nv), C.byref(nt)))
    rec = np.zeros(int(nv.value), _MESH_VERTEX)
    faces = np.zeros((int(nt.value), 3), np.uint32)
    if nv.value:
        L.check(lib.semtsdf_extract_mesh(vol.handle, int(min_weight), rec.ctypes.data, int(nv.value), faces.ctypes.data,
                                         int(nt.value), C.byref(nv), C.byref(nt)))
    return _mesh_dict(rec, faces)


def merge_meshes(meshes: list) -> dict:
    """One mesh from several (the shards of a group): vertices with equal keys (voxel, edge) are
    welded into one -- the first occurrence is kept -- and the faces remapped.  The vertices come
    out sorted by key (x, y, z, edge), the faces in input order."""
    cat = {k: np.concatenate([np.asarray(m[k]) for m in meshes]) if meshes else None for k in _MESH_KEYS}
    if not meshes or not len(cat["edge"]):
        return _mesh_dict(np.zeros(0, _MESH_VERTEX), np.zeros((0, 3), np.uint32))
    vx = cat["voxel"].astype(np.uint64)
    key = np.stack([vx[:, 0], vx[:, 1], vx[:, 2], cat["edge"].astype(np.uint64)], axis=1)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    offs = np.cumsum([0] + [len(m["edge"]) for m in meshes])
    faces = [inverse[np.asarray(m["faces"], np.int64).reshape(-1, 3) + o] for m, o in zip(meshes, offs)]
    out = {k: np.ascontiguousarray(cat[k][first]) for k in _MESH_KEYS}
    out["faces"] = np.concatenate(faces).astype(np.uint32).reshape(-1, 3)
    return out


def write_mesh_ply(path: str, mesh: dict, color_by_label: bool = False) -> None:
    """Binary little-endian PLY of a mesh: the vertex element of write_ply (float x, y, z; uchar
    red, green, blue; uchar label) and `element face` with `property list uchar uint
    vertex_indices`.  With color_by_label the colours are the label render's palette (label 0
    keeps its colour)."""
    xyz = np.ascontiguousarray(mesh["vertices"], np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    rgb = np.ascontiguousarray(mesh["rgb"], np.uint8).reshape(n, 3)
    lab = np.ascontiguousarray(mesh["label"], np.uint8).reshape(n)
    faces = np.ascontiguousarray(mesh["faces"], np.uint32).reshape(-1, 3)
    if color_by_label:
        rgb = np.where((lab > 0)[:, None], PALETTE[lab % 32], rgb).astype(np.uint8)
    vrec = np.zeros(n, dtype=_PLY_VERTEX)
    vrec["x"], vrec["y"], vrec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    vrec["red"], vrec["green"], vrec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    vrec["label"] = lab
    frec = np.zeros(faces.shape[0], dtype=_PLY_FACE)
    frec["n"] = 3
    frec["v"] = faces
    header = ("ply\nformat binary_little_endian 1.0\ncomment semtsdf mesh export\n"
              f"element vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar label\n"
              f"element face {faces.shape[0]}\nproperty list uchar uint vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def read_mesh_ply(path: str) -> dict:
    """Reads back what write_mesh_ply writes: vertices, rgb, label, faces."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    n = int(next(ln for ln in head if ln.startswith("element vertex")).split()[-1])
    m = int(next(ln for ln in head if ln.startswith("element face")).split()[-1])
    vrec = np.frombuffer(data, dtype=_PLY_VERTEX, count=n, offset=end)
    frec = np.frombuffer(data, dtype=_PLY_FACE, count=m, offset=end + n * _PLY_VERTEX.itemsize)
    if m and not (frec["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    return {"vertices": np.stack([vrec["x"], vrec["y"], vrec["z"]], axis=1),
            "rgb": np.stack([vrec["red"], vrec["green"], vrec["blue"]], axis=1), "label": vrec["label"].copy(),
            "faces": frec["v"].copy().reshape(-1, 3)}


def write_ply(path: str, xyz: np.ndarray, rgb: np.ndarray, label: np.ndarray | None = None,
              color_by_label: bool = False) -> None:
    """Binary little-endian PLY: float x, y, z; uchar red, green, blue; uchar label.  With
    color_by_label the colours are the label render's palette (label 0 keeps its colour)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(n, 3)
    lab = np.zeros(n, np.uint8) if label is None else np.ascontiguousarray(label, np.uint8).reshape(n)
    if color_by_label:
        rgb = np.where((lab > 0)[:, None], PALETTE[lab % 32], rgb).astype(np.uint8)
    rec = np.zeros(n, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"),
                                      ("blue", "u1"), ("label", "u1")]))
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    rec["label"] = lab
    header = ("ply\nformat binary_little_endian 1.0\ncomment semtsdf surface export\n"
              f"element vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar label\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def read_ply(path: str) -> dict:
    """Reads back what write_ply writes (tests, tools)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    n = int(next(ln for ln in head if ln.startswith("element vertex")).split()[-1])
    rec = np.frombuffer(data[end:], dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"),
                                                    ("green", "u1"), ("blue", "u1"), ("label", "u1")]), count=n)
    return {"xyz": np.stack([rec["x"], rec["y"], rec["z"]], axis=1), "rgb": np.stack([rec["red"], rec["green"],
                                                                                        rec["blue"]], axis=1),
            "label": rec["label"].copy()}
