"""NumPy restatement of the mesh-extraction contract (include/semtsdf.h, DESIGN.md "Mesh
extraction"), derived from the downloaded volume arrays alone: valid cells, the six Kuhn
tetrahedra, the 1/2/3-negative rule, the winding from the midpoint rule computed geometrically,
positions in f32 NumPy operations.  Shared by tests/test_mesh.py and tests/test_gpu_mesh.py."""
from itertools import permutations

import numpy as np

PERMS = sorted(permutations(range(3)))  # xyz, xzy, yxz, yzx, zxy, zyx: the tet index


def tet_vertices(perm):
    """The 4 corner offsets of tet `perm`: v0 = 0, then one more axis of the permutation each."""
    v = np.zeros((4, 3), np.int64)
    for i, a in enumerate(perm):
        v[i + 1] = v[i]
        v[i + 1, a] += 1
    return v


def case_triangles(V, mask):
    """Triangles of the tet with vertices V whose negative vertices are the bits of `mask`: a list
    of three (i, j) tet-vertex pairs (i < j) each, wound so that with every crossing at its edge
    midpoint the right-hand normal points from the negative towards the non-negative vertices."""
    neg = [i for i in range(4) if mask >> i & 1]
    pos = [i for i in range(4) if not mask >> i & 1]
    e = lambda a, b: (min(a, b), max(a, b))
    if len(neg) in (0, 4):
        return []
    if len(neg) == 1:
        tris = [[e(neg[0], p) for p in pos]]
    elif len(neg) == 3:
        tris = [[e(pos[0], n) for n in neg]]
    else:
        (A, B), (C, D) = neg, pos
        tris = [[e(A, C), e(A, D), e(B, D)], [e(A, C), e(B, D), e(B, C)]]
    want = V[pos].mean(axis=0) - V[neg].mean(axis=0)
    out = []
    for t in tris:
        m = [(V[i] + V[j]) / 2.0 for i, j in t]
        n = np.cross(m[1] - m[0], m[2] - m[0])
        d = float(np.dot(n, want))
        assert abs(d) > 1e-9
        out.append(t if d > 0 else [t[0], t[2], t[1]])
    return out


def restate_mesh(sdf, wt, color, hist, start, voxel, min_weight=1):
    """sdf f32 [Dx,Dy,Dz], wt i32, color [Dx,Dy,Dz,3] (u8 or i32), hist u32 [Dx,Dy,Dz,32] or None,
    start/voxel f32 [3].  Returns the mesh in canonical form (canonical()) plus `stats`."""
    D = sdf.shape
    neg = sdf < np.float32(0.0)
    ok = wt >= min_weight
    valid = np.ones((D[0] - 1, D[1] - 1, D[2] - 1), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                valid &= ok[dx:D[0] - 1 + dx, dy:D[1] - 1 + dy, dz:D[2] - 1 + dz]
    cells = np.argwhere(valid).astype(np.int64)
    flat = lambda p: (p[:, 0] * D[1] + p[:, 1]) * D[2] + p[:, 2]
    tri_keys = []
    combos = np.zeros((6, 16), np.int64)
    for t, perm in enumerate(PERMS):
        V = tet_vertices(perm)
        vneg = np.stack([neg.reshape(-1)[flat(cells + V[i])] for i in range(4)], axis=1)
        mask = (vneg * (1 << np.arange(4))).sum(axis=1)
        combos[t] = np.bincount(mask, minlength=16)
        for m in range(1, 15):
            c = cells[mask == m]
            if not len(c):
                continue
            for tri in case_triangles(V, m):
                keys = []
                for i, j in tri:
                    d = V[j] - V[i]
                    cls = int(d[0] | d[1] << 1 | d[2] << 2)
                    keys.append(flat(c + V[i]) * 8 + cls)
                tri_keys.append(np.stack(keys, axis=1))
    tri_keys = np.concatenate(tri_keys) if tri_keys else np.zeros((0, 3), np.int64)
    vkeys = np.unique(tri_keys)  # sorted by (x, y, z, edge)
    faces = np.searchsorted(vkeys, tri_keys).astype(np.uint32)
    cls = (vkeys & 7).astype(np.int64)
    own = vkeys >> 3
    o = np.stack([own // (D[1] * D[2]), own // D[2] % D[1], own % D[2]], axis=1)
    d = np.stack([cls & 1, cls >> 1 & 1, cls >> 2 & 1], axis=1)
    q = o + d
    s0 = sdf.reshape(-1)[flat(o)].astype(np.float32)
    s1 = sdf.reshape(-1)[flat(q)].astype(np.float32)
    with np.errstate(all="ignore"):
        tt = (s0 / (s0 - s1)).astype(np.float32)
    start = np.asarray(start, np.float32)
    voxel = np.asarray(voxel, np.float32)
    g = o.astype(np.float32) + np.where(d > 0, tt[:, None], np.float32(0.0)).astype(np.float32)
    pos = ((g * voxel[None, :]).astype(np.float32) + start[None, :]).astype(np.float32)
    near = np.where((np.abs(s0) <= np.abs(s1))[:, None], o, q)
    nf = flat(near)
    rgb = np.clip(color.reshape(-1, 3)[nf].astype(np.int64), 0, 255).astype(np.uint8)
    lab = np.zeros(len(vkeys), np.uint8)
    if hist is not None:
        h = hist.reshape(-1, 32)[nf]
        best = np.zeros(len(vkeys), np.uint32)
        for k in range(32):  # first maximum, counts > 0 only
            better = h[:, k] > best
            lab[better] = k
            best[better] = h[better, k]
    mesh = {"vertices": pos, "voxel": o.astype(np.uint32), "edge": cls.astype(np.uint8), "rgb": rgb, "label": lab,
            "faces": faces}
    mesh = canonical(mesh)
    mesh["stats"] = {"valid_cells": int(len(cells)), "combos": combos,
                     "t01": int(((tt == 0) | (tt == 1)).sum())}
    return mesh


def canonical(mesh):
    """Vertices sorted by the key (x, y, z, edge), faces remapped, each rotated to start at its
    smallest index, rows sorted: two meshes of one surface compare equal array by array."""
    vx = mesh["voxel"].astype(np.int64)
    order = np.lexsort((mesh["edge"], vx[:, 2], vx[:, 1], vx[:, 0]))
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    f = inv[mesh["faces"].astype(np.int64)].reshape(-1, 3)
    if len(f):
        r = np.argmin(f, axis=1)
        f = np.stack([np.take_along_axis(f, ((r + k) % 3)[:, None], axis=1)[:, 0] for k in range(3)], axis=1)
        f = f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]
    out = {k: np.ascontiguousarray(mesh[k][order]) for k in ("vertices", "voxel", "edge", "rgb", "label")}
    out["faces"] = f.astype(np.uint32)
    return out


def assert_meshes_equal(got, want):
    """Exact comparison of two canonical meshes, positions as bit patterns."""
    assert got["voxel"].shape == want["voxel"].shape, (got["voxel"].shape, want["voxel"].shape)
    assert got["faces"].shape == want["faces"].shape, (got["faces"].shape, want["faces"].shape)
    assert np.array_equal(got["voxel"], want["voxel"]) and np.array_equal(got["edge"], want["edge"])
    assert np.array_equal(got["vertices"].view(np.uint32), want["vertices"].view(np.uint32))
    assert np.array_equal(got["rgb"], want["rgb"])
    assert np.array_equal(got["label"], want["label"])
    assert np.array_equal(got["faces"], want["faces"])


def random_field(dims=(11, 13, 37), seed=0):
    """The fixed random field of the mesh tests: sdf uniform in [-1, 1) with 2 % exact 0.0 and 1 %
    -0.0, 85 % of the voxels observed with weights 1..4, random colours (int32, some outside
    [0, 255]) and a sparse random histogram."""
    rng = np.random.default_rng(seed)
    sdf = rng.uniform(-1.0, 1.0, dims).astype(np.float32)
    r = rng.random(dims)
    sdf[r < 0.02] = np.float32(0.0)
    sdf[(r >= 0.02) & (r < 0.03)] = np.float32(-0.0)
    obs = rng.random(dims) < 0.85
    wt = np.where(obs, rng.integers(1, 5, dims), 0).astype(np.int32)
    color = rng.integers(-40, 300, dims + (3,)).astype(np.int32)
    hist = (rng.integers(0, 9, dims + (32,)) * (rng.random(dims + (32,)) < 0.1)).astype(np.uint32)
    return {"sdf": sdf, "wt": wt, "color": color, "hist": hist}
