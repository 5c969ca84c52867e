"""Brick paging on the host: the library exports the two calls, the NumPy definition
(tests/bricks_restatement.py) is its own inverse, the boxes a shift vacates and uncovers are what
semtsdf.follow.leaving says per voxel, and BrickStore keeps, returns, remaps and saves records."""
import itertools

import numpy as np
import pytest

import bricks_restatement as B
from mesh_restatement import random_field

DIMS = (11, 13, 37)
MU = 0.05


def _state(flags, dims=DIMS):
    f = random_field(dims)
    st = {"sdf": f["sdf"], "wt": f["wt"]}
    st["color"] = f["color"] if flags & B.F_COLOR_I32 else np.clip(f["color"], 0, 255).astype(np.uint8)
    if flags & B.F_SEMANTIC:
        st["hist"] = f["hist"]
    if flags & B.F_VOTE:
        rng = np.random.default_rng(3)
        st["cls"] = rng.integers(0, 40, dims).astype(np.int32)
        st["cls_cnt"] = rng.integers(0, 9, dims).astype(np.int32)
    return st


def test_library_exports_both_calls():
    import ctypes as C

    from semtsdf import _lib as L

    lib = L.load()
    assert hasattr(lib, "semtsdf_pack_bricks") and hasattr(lib, "semtsdf_unpack_bricks")
    assert lib.semtsdf_abi_version() == 12
    assert C.sizeof(L.Brick) == 24 and L.BRICK_DTYPE.itemsize == 24
    assert [L.BRICK_DTYPE.fields[n][1] for n in ("b", "bins", "offset")] == [0, 12, 16]
    assert (L.Brick.b.offset, L.Brick.bins.offset, L.Brick.offset.offset) == (0, 12, 16)
    # argument errors are decided before any device work
    n = C.c_uint64(7)
    box = (C.c_int32 * 3)()
    assert lib.semtsdf_pack_bricks(None, box, box, None, 0, None, 0, C.byref(n), C.byref(n)) == L.ERR_INVALID
    assert lib.semtsdf_unpack_bricks(None, None, 0, None, 0) == L.ERR_INVALID


@pytest.mark.parametrize("flags", [0x3, 0x4, 0x8 | 0x4, 0x1 | 0x4])
def test_numpy_unpack_inverts_numpy_pack(flags):
    st = _state(flags)
    bricks, words = B.numpy_pack(st, DIMS, flags, MU)
    nb = B.brick_counts(DIMS)
    assert len(bricks) == nb[0] * nb[1] * nb[2]  # a random field occupies every brick
    off = bricks["offset"].astype(np.int64)
    sizes = np.diff(np.append(off, words.size))
    ncol = 3 if flags & B.F_COLOR_I32 else 1
    for e, n in zip(bricks, sizes):
        assert n == 512 * (2 + ncol + bin(int(e["bins"])).count("1") + (2 if flags & B.F_VOTE else 0))
    assert [tuple(b) for b in bricks["b"]] == sorted(tuple(b) for b in bricks["b"])
    back = B.numpy_unpack(B.reset_state(DIMS, flags, MU), DIMS, flags, MU, bricks, words)
    assert B.states_equal(back, st, DIMS)
    # a sub-box returns exactly its slice of the whole list, offsets restarted
    lo, hi = (0, 1, 2), (2, 2, 4)
    sub, sw = B.numpy_pack(st, DIMS, flags, MU, lo, hi)
    inside = [i for i, b in enumerate(bricks["b"]) if all(lo[a] <= b[a] < hi[a] for a in range(3))]
    assert np.array_equal(sub["b"], bricks["b"][inside]) and np.array_equal(sub["bins"], bricks["bins"][inside])
    assert np.array_equal(sw, np.concatenate([words[off[i]:off[i] + sizes[i]] for i in inside]))
    # reset bricks are skipped, and an unpack leaves every other brick alone
    holed = {k: v.copy() for k, v in B.shaped(st, DIMS).items()}
    fresh = B.reset_state(DIMS, flags, MU)
    for k in holed:
        holed[k][0:8, 8:13, 0:16] = B.shaped(fresh, DIMS)[k][0:8, 8:13, 0:16]
    hb, hw = B.numpy_pack(holed, DIMS, flags, MU)
    assert len(hb) == len(bricks) - 2 and not any(tuple(b) in ((0, 1, 0), (0, 1, 1)) for b in hb["b"])
    other = _state(flags)
    other["wt"] = other["wt"] + 1
    merged = B.numpy_unpack(other, DIMS, flags, MU, sub, sw)
    want = {k: v.copy() for k, v in B.shaped(other, DIMS).items()}
    for k in want:
        want[k][0:11, 8:13, 16:32] = B.shaped(st, DIMS)[k][0:11, 8:13, 16:32]
    assert B.states_equal(merged, want, DIMS)


def test_boxes_cover_what_leaves_and_enters():
    from semtsdf.bricks import entering_boxes, leaving_boxes
    from semtsdf.follow import leaving

    nb = (3, 4, 9)
    dim = tuple(8 * n for n in nb)
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in dim], indexing="ij"), axis=-1)
    for s in itertools.product((-16, -8, 0, 8, 16), repeat=3):
        sb = [x // 8 for x in s]
        for boxes, want in ((leaving_boxes(nb, sb), leaving(dim, s)(idx)),
                            (entering_boxes(nb, sb), leaving(dim, [-x for x in s])(idx))):
            assert len(boxes) <= 3, (s, boxes)
            count = np.zeros(dim, np.int32)
            for lo, hi in boxes:
                assert all(0 <= lo[a] < hi[a] <= nb[a] for a in range(3)), (s, lo, hi)
                count[8 * lo[0]:8 * hi[0], 8 * lo[1]:8 * hi[1], 8 * lo[2]:8 * hi[2]] += 1
            assert count.max(initial=0) <= 1, s            # disjoint
            assert np.array_equal(count == 1, want), s     # and exactly the voxels that leave / enter


def _records(n, flags=0x3, seed=0):
    """n bricks with random records in ascending order at (k, 2k, 3)."""
    rng = np.random.default_rng(seed)
    bricks = np.zeros(n, B.BRICK_DTYPE)
    parts, at = [], 0
    for k in range(n):
        bins = int(rng.integers(0, 1 << 32)) & 0x0000F00F if flags & 1 else 0
        planes = 2 + (3 if flags & 4 else 1) + bin(bins).count("1") + (2 if flags & 8 else 0)
        bricks[k] = ((k, 2 * k, 3), bins, at)
        parts.append(rng.integers(0, 1 << 32, 512 * planes, dtype=np.uint64).astype(np.uint32))
        at += parts[-1].size
    return bricks, np.concatenate(parts)


def test_store_put_take_and_origin():
    from semtsdf.bricks import BrickStore

    bricks, words = _records(5)
    s = BrickStore()
    s.put(bricks, words)
    assert len(s) == 5 and s.nbytes == words.nbytes + 16 * 5
    assert s.keys() == [(k, 2 * k, 3) for k in range(5)]
    s.origin = [2, 0, -1]  # the volume moved: local b is now world origin + b
    got, gw = s.take((-1, 2, 4), (2, 9, 5))  # world x 1..3, y 2..8, z 3
    assert [tuple(b) for b in got["b"]] == [(-1, 2, 4), (0, 4, 4), (1, 6, 4)]
    off = bricks["offset"].astype(np.int64)
    end = np.append(off[1:], words.size)
    assert np.array_equal(gw, words[off[1]:end[3]]) and list(got["offset"]) == [0, off[2] - off[1], off[3] - off[1]]
    assert np.array_equal(got["bins"], bricks["bins"][1:4])
    assert len(s) == 2 and s.keys() == [(0, 0, 3), (4, 8, 3)]
    empty, ew = s.take((-1, 2, 4), (2, 9, 5))  # taken records are gone
    assert len(empty) == 0 and ew.size == 0
    s.put(got, gw)  # put keys by the current origin: the same world bricks again
    assert s.keys() == [(k, 2 * k, 3) for k in range(5)]
    s.origin = [0, 0, 0]
    back, bw = s.take((0, 0, 0), (5, 9, 4))
    assert np.array_equal(back, bricks) and np.array_equal(bw, words) and len(s) == 0 and s.nbytes == 0
    with pytest.raises(ValueError):
        s.put(bricks, words[:-1])


def test_store_save_and_load(tmp_path):
    from semtsdf.bricks import BrickStore

    bricks, words = _records(4, seed=2)
    s = BrickStore()
    s.flags = 0x1
    s.origin = [3, -2, 7]
    s.put(bricks, words)
    path = str(tmp_path / "store.npz")
    s.save(path)
    t = BrickStore.load(path)
    assert t.origin == [3, -2, 7] and t.flags == 0x1 and t.keys() == s.keys() and t.nbytes == s.nbytes
    for k in s.keys():
        assert t.get(k)[0] == s.get(k)[0] and np.array_equal(t.get(k)[1], s.get(k)[1])
    e = BrickStore()
    e.save(str(tmp_path / "empty.npz"))
    assert len(BrickStore.load(str(tmp_path / "empty.npz"))) == 0


def test_store_remap_is_the_dense_lut_rule():
    from semtsdf.bricks import BrickStore

    rng = np.random.default_rng(5)
    dims, flags = (8, 8, 16), 0x3
    st = B.reset_state(dims, flags, MU)
    st["wt"][...] = 1  # both bricks stay occupied whatever happens to their histograms
    for k in (1, 2, 3, 5):  # brick 0 (z < 8): four sparse bins, each present
        st["hist"][:, :, :8, k] = rng.integers(1, 4, (8, 8, 8)) * (rng.random((8, 8, 8)) < 0.3)
        st["hist"][0, 0, 0, k] = 1
    st["hist"][0, 0, 0, 2] = 0xFFFFFFFF  # the merge 2 + 3 wraps modulo 2^32 in this voxel
    # brick 1 (z >= 8): bins 11 and 12 in one voxel only, and their merge wraps to 0: the plane empties
    st["hist"][1, 1, 9, 11], st["hist"][1, 1, 9, 12] = 1, 0xFFFFFFFF
    lut = np.arange(32)
    lut[1], lut[5] = 5, 1  # a cycle
    lut[3] = 2             # a merge
    lut[11] = 12           # a merge that empties its plane
    bricks, words = B.numpy_pack(st, dims, flags, MU)
    assert list(bricks["bins"]) == [0b101110, (1 << 11) | (1 << 12)]
    s = BrickStore()
    s.flags = flags
    s.put(bricks, words)
    s.remap(lut)
    want = {k: v.copy() for k, v in st.items()}
    dense = np.zeros_like(st["hist"])
    for k in range(32):
        dense[..., lut[k]] += st["hist"][..., k]  # u32: modulo 2^32
    want["hist"] = dense
    wb, ww = B.numpy_pack(want, dims, flags, MU)
    assert list(wb["bins"]) == [0b100110, 0]  # the wrapped sum emptied plane 12: dropped
    got, gw = s.take((0, 0, 0), (1, 1, 2))
    assert np.array_equal(got, wb) and np.array_equal(gw, ww)
    with pytest.raises(ValueError):
        s.remap(np.arange(32)[::-1])


def test_shift_paged_refuses_ragged_dims():
    from semtsdf.bricks import BrickStore, shift_paged

    class Ragged:
        local_dim = (24, 28, 72)

    with pytest.raises(ValueError):
        shift_paged(Ragged(), BrickStore(), (8, 0, 0))


class NumpyVolume:
    """The paging calls of a Volume on the definition alone: what shift_paged drives, without a device."""

    class _P:
        pass

    def __init__(self, state, dims, flags):
        self.local_dim, self.state = tuple(dims), B.shaped(state, dims)
        self.params = self._P()
        self.params.flags, self.params.mu = flags, MU

    def brick_counts(self):
        return B.brick_counts(self.local_dim)

    def pack_bricks(self, lo=None, hi=None):
        return B.numpy_pack(self.state, self.local_dim, self.params.flags, MU, lo, hi)

    def unpack_bricks(self, bricks, words):
        self.state = B.numpy_unpack(self.state, self.local_dim, self.params.flags, MU, bricks, words)

    def shift(self, sx, sy, sz):
        from shift_restatement import numpy_shift

        self.state = numpy_shift(self.state, (sx, sy, sz), MU, dims=self.local_dim)


def test_shift_paged_keeps_the_world_on_a_numpy_volume():
    from semtsdf.bricks import BrickStore, shift_paged

    dims, flags = (16, 24, 16), 0x3
    st = _state(flags, dims)
    holed = {k: v.copy() for k, v in B.shaped(st, dims).items()}
    for k, v in B.shaped(B.reset_state(dims, flags, MU), dims).items():
        holed[k][8:16, 0:8, :] = v[8:16, 0:8, :]  # reset bricks: they are never stored
    vol, store = NumpyVolume(holed, dims, flags), BrickStore()
    canvas = B.Canvas(holed, dims, flags, MU, margin=24)
    world0 = {k: v.copy() for k, v in canvas.world.items()}
    walk = [(8, 8, 0), (0, -16, 8), (-16, 0, 0), (8, 8, 0), (0, 0, -8)]
    assert np.sum(walk, axis=0).tolist() == [0, 0, 0]
    for k, s in enumerate(walk):
        shift_paged(vol, store, s)
        assert B.states_equal(vol.state, canvas.shift(s), dims), (k, s)
        assert (len(store) > 0) == (k < len(walk) - 1)
        items = [(key,) + store.get(key) for key in store.keys()]
        world = B.rebuild_world(vol.state, items, store.origin, dims, flags, MU, margin=24)
        assert B.states_equal(world, world0, [d + 48 for d in dims]), (k, s)
    assert store.origin == [0, 0, 0] and store.flags == flags & 0xD and B.states_equal(vol.state, holed, dims)
    shift_paged(vol, store, (0, 0, 0))  # nothing to do
    assert len(store) == 0
    shift_paged(vol, store, (16, 0, 0))  # everything leaves
    assert store.origin == [2, 0, 0] and len(store) == 2 * 3 * 2 - 2
    assert B.states_equal(vol.state, B.reset_state(dims, flags, MU), dims)
    with pytest.raises(ValueError):
        shift_paged(vol, store, (4, 0, 0))
    other = NumpyVolume(holed, dims, 0x4)
    with pytest.raises(ValueError):
        shift_paged(other, store, (8, 0, 0))  # records of another form
