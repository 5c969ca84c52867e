"""The long-walk inputs on the CPU (tests/long_walk_fields.py): the conditions under which
tests/test_gpu_long_walks.py cannot pass vacuously.  Every trip of a capped grid, every scan
group and every staging chunk that the two volumes reach holds enough compared values, the group
the gap covers holds none between groups that do, and the units of the trip table equal the
constants the launchers use.  From the fields and the restatements alone: no device, no library."""
import os
import re

import numpy as np
import pytest

import long_walk_fields as F
from instances_restatement import HAZARD_LUT, remap_hist
from mesh_restatement import restate_mesh

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slam-maskrcnn_amd", "csrc")
START, VOXEL = np.array((-0.3, 0.1, 0.5), np.float32), np.array((0.011, 0.012, 0.013), np.float32)
ENOUGH = 1000


def _field(V):
    sdf, wt, color, hist = F.band_field(V["dims"], V["seed"], V["gaps"], bool(V["flags"] & 1))
    return {"dims": V["dims"], "sdf": sdf, "wt": wt, "color": color, "hist": hist}


@pytest.fixture(scope="module")
def A():
    return _field(F.VOLUME_A)


@pytest.fixture(scope="module")
def B():
    return _field(F.VOLUME_B)


def per_trip(name, dims, mask):
    """Voxels of `mask` in every trip, group or chunk of row `name`."""
    x, y, z = np.nonzero(mask)
    return np.bincount(F.trip_of(name, dims, x, y, z), minlength=F.trip_count(name, dims)).tolist()


def vertices_per_group(f, min_weight=1):
    m = restate_mesh(f["sdf"], f["wt"], f["color"], f["hist"], START, VOXEL, min_weight)
    o = m["voxel"].astype(np.int64)  # a vertex is counted in the tile of the voxel that owns its edge
    per = np.bincount(F.trip_of("mesh_group", f["dims"], o[:, 0], o[:, 1], o[:, 2]),
                      minlength=F.trip_count("mesh_group", f["dims"])).tolist()
    return per, len(m["vertices"]), len(m["faces"])


def test_volume_shapes_and_trip_counts():
    """A: y and z ragged (4 padded rows, 8 padded planes), 19 200 tiles; B: 70 656 tiles.  The trips,
    groups and chunks each reaches, and where the reference-order boundaries fall: inside an x layer,
    not on a layer or tile edge."""
    a, b = F.VOLUME_A["dims"], F.VOLUME_B["dims"]
    assert (F.tiles_shape(a)[0] * 8 - a[1], F.tiles_shape(a)[1] * 32 - a[2]) == (4, 8)
    assert (F.stored_voxels(a) // 256, F.stored_voxels(a), int(np.prod(a))) == (19200, 4915200, 4320000)
    assert (F.stored_voxels(b) // 256, F.stored_voxels(b), int(np.prod(b))) == (70656, 18087936, 17250000)
    count = lambda dims: {t.name: F.trip_count(t.name, dims) for t in F.TRIPS if t.order != "flat"}
    ca, cb = count(a), count(b)
    assert [ca[k] for k in ("mesh_group", "instance_trip", "remap_trip", "hist_mask_trip", "hist_chunk",
                            "vox_upload_trip")] == [5, 3, 2, 2, 2, 2]
    assert [cb[k] for k in ("mesh_group", "export_trip", "color_chunk", "weight_widen_trip", "color_widen_trip",
                            "vox_upload_trip", "color_upload_trip")] == [18, 2, 2, 2, 2, 5, 12]
    # the last of each is partial
    assert F.stored_voxels(a) % F.unit("mesh_group") and F.stored_voxels(a) % F.unit("instance_trip")
    assert F.stored_voxels(b) % F.unit("mesh_group") and F.stored_voxels(b) % F.unit("weight_widen_trip")
    for dims, name, layer in ((a, "hist_chunk", 582), (b, "export_trip", 268), (b, "color_chunk", 268)):
        per_layer = dims[1] * dims[2]
        assert F.unit(name) // per_layer == layer and F.unit(name) % per_layer and F.unit(name) % dims[2], name
    assert F.unit("weight_widen_trip") == 256 * F.stored_voxels(b) // b[0]  # tile order: the boundary is x = 256
    # the maps agree with the definitions of the orders on a few voxels
    x, y, z = np.array([0, 5, 599]), np.array([0, 9, 59]), np.array([0, 37, 119])
    assert F.ref_index(a, x, y, z).tolist() == [0, (5 * 60 + 9) * 120 + 37, 4320000 - 1]
    assert F.tile_index(a, x, y, z).tolist() == [0, 5 * 32 + 1 * 4 + 1, 599 * 32 + 7 * 4 + 3]
    assert F.stored_index(a, x, y, z).tolist() == [0, (5 * 32 + 5) * 256 + 1 * 32 + 1 * 4 + 1,
                                                   (599 * 32 + 31) * 256 + 5 * 32 + 3 * 4 + 3]
    # every stored index of a volume occurs once
    d = (3, 11, 37)
    g = np.indices(d).reshape(3, -1)
    s = F.stored_index(d, *g)
    assert len(np.unique(s)) == s.size and s.max() < F.stored_voxels(d)


def test_volume_a_fills_every_trip(A):
    """Volume A: every mesh group outside the gap owns vertices and group 1 none; every instance
    trip, remap trip, histogram chunk, k_hist_mask trip and upload trip holds compared voxels."""
    dims = A["dims"]
    per, nv, nt = vertices_per_group(A)
    print("A: vertices per mesh group", per, "vertices", nv, "triangles", nt)
    assert per == [39346, 0, 39249, 37966, 24466] and (nv, nt) == (141027, 200042)
    assert per[1] == 0 and all(n >= ENOUGH for i, n in enumerate(per) if i != 1)
    per3, nv3, nt3 = vertices_per_group(A, 3)
    assert (nv3, nt3) == (964, 800) and per3[1] == 0 and all(n > 0 for i, n in enumerate(per3) if i != 1)
    sdf, wt = A["sdf"], A["wt"]
    sel = (wt >= 2) & (np.abs(sdf) < np.float32(0.5))
    per = per_trip("instance_trip", dims, sel)
    print("A: selected voxels per instance trip", per)
    assert per == [20840, 41397, 14129] and min(per) >= ENOUGH
    h = A["hist"].reshape(-1, 32)
    rows = F.vote_rows(A["hist"])
    bm = F.bin_major(A["hist"])
    assert bm.shape == A["hist"].shape and bm.strides[-1] > bm.strides[0] and np.array_equal(bm, A["hist"])
    voted = np.zeros(int(np.prod(dims)), bool)
    voted[rows] = True
    voted = voted.reshape(dims)
    for name, want in (("hist_chunk", [242070, 8865]), ("hist_mask_trip", [206240, 44695])):
        per = per_trip(name, dims, voted)
        print("A: voxels with votes per", name, per)
        assert per == want and min(per) >= ENOUGH
    assert voted[~(wt > 0)].sum() > 40000  # the single votes fall outside the band too
    changed = np.zeros(int(np.prod(dims)), bool)
    changed[rows] = (remap_hist(h[rows], HAZARD_LUT) != h[rows]).any(axis=1)
    per = per_trip("remap_trip", dims, changed.reshape(dims))
    print("A: voxels HAZARD_LUT changes per remap trip", per)
    assert per == [72742, 16110] and min(per) >= ENOUGH
    per = per_trip("vox_upload_trip", dims, wt > 0)
    assert per == [196106, 7508] and min(per) >= ENOUGH


def test_volume_b_fills_every_trip(B):
    """Volume B: mesh groups 8-15 lie in the gap and own no vertex, the ten others do; both export
    trips hold selected voxels; both colour chunks and both widen trips hold observed voxels."""
    dims = B["dims"]
    per, nv, nt = vertices_per_group(B)
    print("B: vertices per mesh group", per, "vertices", nv, "triangles", nt)
    assert per == [21874, 24942, 25872, 26751, 25254, 27603, 26382, 23187, 0, 0, 0, 0, 0, 0, 0, 0, 23728, 4877]
    assert (nv, nt) == (230470, 285274)
    assert all((n == 0) if 8 <= i < 16 else (n >= ENOUGH) for i, n in enumerate(per))
    sdf, wt = B["sdf"], B["wt"]
    sel = (wt >= 2) & (np.abs(sdf) < np.float32(0.5))
    per = per_trip("export_trip", dims, sel)
    print("B: selected voxels per export trip", per)
    assert per == [94972, 5114] and min(per) >= ENOUGH
    for name, want in (("color_chunk", [252693, 13664]), ("weight_widen_trip", [230427, 35930]),
                       ("color_widen_trip", [230427, 35930])):
        per = per_trip(name, dims, wt > 0)
        print("B: observed voxels per", name, per)
        assert per == want and min(per) >= ENOUGH
    # the upload loops inside a chunk: the last trip of each holds observed voxels (every colour is
    # compared, observed or not)
    assert per_trip("vox_upload_trip", dims, wt > 0)[-1] == 13664
    assert per_trip("color_upload_trip", dims, wt > 0)[-1] == 22266


def _constants():
    """name -> value of every `constexpr <integer type> kName = <integer expression>;` of the sources."""
    out = {}
    for fn in ("semtsdf_internal.h", "semtsdf_kernels.hip", "semtsdf_api.cpp"):
        with open(os.path.join(CSRC, fn)) as f:
            text = f.read()
        for m in re.finditer(r"constexpr\s+(?:unsigned|int|uint64_t|uint32_t|size_t)\s+(k\w+)\s*=\s*([^;]+);", text):
            expr = re.sub(r"(?<=\d)(?:ull|u|ul)\b", "", m.group(2))
            if re.fullmatch(r"[\d\s<*+()]+", expr):
                out.setdefault(m.group(1), []).append(int(eval(expr)))  # digits, shifts, products and sums only
    return out


def _body(text, signature):
    """The text of the function whose definition starts with `signature`, up to its closing brace."""
    i = text.index(signature)
    return text[i:text.index("\n}\n", i)]


# launcher -> the constant its grid cap or chunk size must come from
USES = (("semtsdf_kernels.hip", "hipError_t launch_min_i64(", "kMinBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_hist_mask(", "kHistMaskBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_hist_chunk_to_bm(", "kXferBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_hist_chunk_to_vm(", "kXferBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_vox_chunk(", "kXferBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_color_chunk(", "kXferBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_weight_widen(", "kWidenBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_color_widen(", "kWidenBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_export_surface(", "kExportBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_remap_instances(", "kRemapBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_instance_stats(", "kInstBlocks"),
        ("semtsdf_kernels.hip", "hipError_t launch_mesh_count(", "mesh_groups(g)"),
        ("semtsdf_internal.h", "inline uint64_t mesh_groups(", "kMeshGroup"),
        ("semtsdf_api.cpp", "static int hist_xfer(", "kHistChunk"),
        ("semtsdf_api.cpp", "static int color_xfer(", "kColorChunk"))


def test_trip_table_equals_the_source():
    """Every unit of the table is the value of its constant in csrc/, and every launcher takes its
    cap or chunk from that constant and from no bare number of that size."""
    consts = _constants()
    for t in F.TRIPS:
        assert len(consts.get(t.constant, ())) == 1, f"row {t.name}: {t.constant} has {consts.get(t.constant, [])} " \
                                                     "as definitions in csrc/, not one"
        assert consts[t.constant][0] == t.value, f"row {t.name}: {t.constant} is {consts[t.constant][0]} in csrc/, " \
                                                 f"{t.value} in tests/long_walk_fields.py"
    named = {t.constant for t in F.TRIPS}
    texts = {}
    for fn, sig, const in USES:
        if fn not in texts:
            with open(os.path.join(CSRC, fn)) as f:
                texts[fn] = f.read()
        body = _body(texts[fn], sig)
        assert const in body, f"{sig.split()[-1]}: does not use {const}"
        assert const in named or const == "mesh_groups(g)", const
        for lit in re.findall(r"(?<![\w.])(\d{4,}|1ull << \d+|1u << \d+)(?![\w.])", body):
            assert False, f"{sig.split()[-1]}: bare number {lit} beside {const}"
    # a tile is 256 stored voxels and a block of every walker 256 threads
    assert "mesh_blocks(const VolGeom& g) { return g.nvox / 256u; }" in texts["semtsdf_internal.h"]
    assert F.TILE == 256
