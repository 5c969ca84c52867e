"""semtsdf_pack_bricks / semtsdf_unpack_bricks and the paged follow on the device against their
definition (tests/bricks_restatement.py): packed bytes equal numpy_pack's, an unpack leaves the handle
indistinguishable from a twin made by uploading numpy_unpack's state, and a volume that walks away
and returns through shift_paged finds what it left -- floats as bits throughout."""
import ctypes as C
import functools

import numpy as np
import pytest

import bricks_restatement as B
import model_maps_restatement as R
import shift_restatement as S
from mesh_restatement import random_field

pytestmark = pytest.mark.gpu

DIMS = (24, 28, 72)    # y ragged by 4, nine z-bricks across three z-tiles, z padded by 24
SMALL = (11, 13, 37)   # ragged on every axis
MU = 0.05
MAPS = ("t", "point", "normal", "flags")
# bricks of the field that hold the reset state ...
RESET = [(0, 0, 0), (0, 0, 1), (1, 2, 4), (2, 2, 8), (0, 3, 5)]
# ... and bricks that differ from it in exactly one value of one field
ONLY = {"sdf": (1, 0, 2), "hist": (1, 0, 3), "color": (2, 1, 6), "cls_cnt": (0, 2, 7)}


def _block(b, dims):
    return tuple(slice(8 * b[a], min(8 * b[a] + 8, dims[a])) for a in range(3))


@functools.lru_cache(maxsize=None)
def _field(dims, form, seed=0, holes=True):
    """(flags, state): random_field with the histogram of every brick thinned to 0-3 bins, the RESET
    bricks reset and the ONLY bricks differing from the reset state in one field each (holes=False:
    every brick keeps its random contents)."""
    f = random_field(dims, seed)
    rng = np.random.default_rng(17 + seed)
    nb = B.brick_counts(dims)
    for b in np.ndindex(*nb):
        keep = rng.choice(32, size=int(rng.integers(0, 4)), replace=False)
        drop = np.setdiff1d(np.arange(32), keep)
        f["hist"][_block(b, dims) + (drop,)] = 0
    narrow = np.clip(f["color"], 0, 255)
    if form in ("semantic", "wide_weights"):
        flags, st = 0x3, {"sdf": f["sdf"], "wt": f["wt"], "color": narrow.astype(np.uint8), "hist": f["hist"]}
    elif form == "wide_colour":
        assert (f["color"] > 255).any()
        flags, st = 0x4, {"sdf": f["sdf"], "wt": f["wt"], "color": f["color"]}
    else:
        flags, st = 0x8 | 0x4, {"sdf": f["sdf"], "wt": f["wt"], "color": narrow.astype(np.int32),
                                "cls": rng.integers(0, 40, dims).astype(np.int32),
                                "cls_cnt": rng.integers(0, 9, dims).astype(np.int32)}
    fresh = B.reset_state(dims, flags, MU)
    inside = [b for b in RESET + list(ONLY.values()) if holes and all(b[a] < nb[a] for a in range(3))]
    for b in inside:
        for k in st:
            st[k][_block(b, dims)] = fresh[k][_block(b, dims)]
    def voxel(field, x, y, z):  # a voxel of the field's ONLY brick, or None when the dims do not reach it
        b = ONLY[field]
        return (8 * b[0] + x, 8 * b[1] + y, 8 * b[2] + z) if field in st and b in inside else None

    for field, at, value in (("sdf", voxel("sdf", 1, 3, 3), np.float32(-0.0)), ("color", voxel("color", 1, 2, 5), 9),
                             ("hist", voxel("hist", 2, 0, 4), 2), ("cls_cnt", voxel("cls_cnt", 0, 3, 7), 1)):
        if at is not None:
            st[field][at + ({"color": (1,), "hist": (31,)}.get(field, ()))] = value
    if form == "wide_colour":
        st["color"][9, 9, 9, 0] = 300
    if form == "wide_weights":
        st["wt"][13, 12, 20] = 70000
    for a in st.values():
        a.setflags(write=False)
    return flags, st


def _params(flags, dims=DIMS):
    import semtsdf

    p = semtsdf.default_params(64, R.KI, 640, 480)
    start, voxel = (-0.3, 0.1, 0.5), (0.011, 0.012, 0.013)
    for a in range(3):
        p.dim[a] = dims[a]
        p.vol_start[a], p.voxel[a] = start[a], voxel[a]
        p.vol_end[a] = start[a] + voxel[a] * (dims[a] - 1)
    p.mu = MU
    p.flags = flags
    return p


def _volume(flags, state, dims=DIMS):
    import semtsdf

    semtsdf.load()
    vol = semtsdf.Volume(_params(flags, dims), 0)
    vol.upload(**state)
    return vol


def _same(got, want, what):
    gb, gw = got
    wb, ww = want
    assert gb.dtype == wb.dtype and gb.tobytes() == wb.tobytes(), (what, len(gb), len(wb))
    assert gw.dtype == ww.dtype and np.array_equal(gw, ww), (what, gw.size, ww.size)


BOXES = {"whole": (None, None), "interior": ((1, 1, 4), (2, 2, 5)), "ragged corner": ((2, 3, 8), (3, 4, 9)),
         "across a z-tile": ((0, 0, 3), (3, 4, 6)), "x-slab": ((0, 0, 0), (1, 4, 9)), "y-slab": ((0, 3, 0), (3, 4, 9)),
         "z-slab": ((0, 0, 8), (3, 4, 9)), "empty": ((1, 1, 1), (1, 3, 4)), "reset bricks": ((0, 0, 0), (1, 1, 2))}


@pytest.mark.parametrize("form", ["semantic", "wide_colour", "wide_weights", "vote"])
def test_pack_equals_the_definition(form):
    from semtsdf import _lib as L

    flags, state = _field(DIMS, form)
    vol = _volume(flags, state)
    bytes0 = vol.state().device_bytes
    nb = B.brick_counts(DIMS)
    for name, (lo, hi) in BOXES.items():
        want = B.numpy_pack(state, DIMS, flags, MU, lo, hi)
        total = int(np.prod([h - l for l, h in zip(lo or (0, 0, 0), hi or nb)]))
        if name in ("empty", "reset bricks"):
            assert len(want[0]) == 0 and (name == "empty") == (total == 0)
        elif name in ("interior", "ragged corner"):
            assert len(want[0]) == total == 1
        else:  # the expectation holds skipped and kept bricks: equality is not vacuous
            assert 0 < len(want[0]) < total, (name, len(want[0]), total)
        _same(vol.pack_bricks(lo, hi), want, (form, name))
    present = {tuple(b) for b in B.numpy_pack(state, DIMS, flags, MU)[0]["b"]}
    assert not present & set(RESET)
    fields = [k for k in ONLY if k in state]
    assert len(fields) >= 2 and all(ONLY[k] in present for k in fields)  # one differing value keeps a brick
    # the count-only call, a short capacity, a second call
    want_b, want_w = B.numpy_pack(state, DIMS, flags, MU)
    lo, hi = np.zeros(3, np.int32), np.array(nb, np.int32)
    fn = L.load().semtsdf_pack_bricks
    n, m = C.c_uint64(0), C.c_uint64(0)
    L.check(fn(vol.handle, L.ptr(lo), L.ptr(hi), None, 0, None, 0, C.byref(n), C.byref(m)))
    assert (n.value, m.value) == (len(want_b), want_w.size)
    for short in ((len(want_b) - 1, want_w.size), (len(want_b), want_w.size - 1)):
        bb, ww = np.full(len(want_b), 0x55, np.uint8).repeat(24), np.full(want_w.size, 0x55555555, np.uint32)
        n.value = m.value = 0
        rc = fn(vol.handle, L.ptr(lo), L.ptr(hi), L.ptr(bb), short[0], L.ptr(ww), short[1], C.byref(n), C.byref(m))
        assert rc == L.ERR_INVALID and (n.value, m.value) == (len(want_b), want_w.size)
        assert (bb == 0x55).all() and (ww == 0x55555555).all()
    assert fn(vol.handle, L.ptr(lo), L.ptr(hi), L.ptr(np.zeros(24, np.uint8)), 1, None, 0, C.byref(n),
              C.byref(m)) == L.ERR_INVALID  # one buffer alone
    for bad_lo, bad_hi in (((0, 0, -1), nb), ((0, 0, 0), (3, 4, 10)), ((2, 0, 0), (1, 4, 9))):
        with pytest.raises(Exception) as e:
            vol.pack_bricks(bad_lo, bad_hi)
        assert e.value.code == L.ERR_INVALID
    _same(vol.pack_bricks(), vol.pack_bricks(), (form, "twice"))
    assert vol.state().device_bytes == bytes0
    assert B.states_equal(S.full_download(vol), state, DIMS)  # the volume is not modified
    vol.close()


def test_pack_on_dims_ragged_on_every_axis():
    flags, state = _field(SMALL, "semantic")
    vol = _volume(flags, state, SMALL)
    nb = B.brick_counts(SMALL)
    want = B.numpy_pack(state, SMALL, flags, MU)
    assert 0 < len(want[0]) < nb[0] * nb[1] * nb[2]
    _same(vol.pack_bricks(), want, "whole")
    corner = tuple(n - 1 for n in nb)
    _same(vol.pack_bricks(corner, nb), B.numpy_pack(state, SMALL, flags, MU, corner, nb), "corner")
    # and back: into a volume of another state, every brick of which is then A's or its own
    _, other = _field(SMALL, "semantic", seed=1)
    b = _volume(flags, other, SMALL)
    sub = vol.pack_bricks((0, 1, 2), nb)
    b.unpack_bricks(*sub)
    assert B.states_equal(S.full_download(b), B.numpy_unpack(other, SMALL, flags, MU, *sub), SMALL)
    vol.close()
    b.close()


def _twin_check(b, want, flags, dims):
    """`b` against a twin made by uploading `want`: downloads, maps, map words, one further integrate."""
    import semtsdf

    assert B.states_equal(S.full_download(b), want, dims)
    tw = semtsdf.Volume(b.get_params(), 0)
    tw.upload(**{k: np.ascontiguousarray(v) for k, v in want.items()})
    st = b.state()
    tw.set_state(int(st.n_obs), int(st.num_objs))
    p = b.get_params()
    s2w, c = semtsdf.pose_camera(list(p.Kinv), np.eye(4, dtype=np.float32))
    names = MAPS + (("label", "votes") if flags & 1 else ())
    ma, mb = b.render_maps(s2w, c, 1, names), tw.render_maps(s2w, c, 1, names)
    for k in names:
        ga, gb = (x.view(np.uint32) if x.dtype == np.float32 else x for x in (ma[k], mb[k]))
        assert np.array_equal(ga, gb), k
    assert int((ma["flags"] & 1).sum()) >= 500  # the view shows the model
    assert np.array_equal(b.map_words(), tw.map_words())
    fr = R.fused_scene()["frames"][1]
    for v in (b, tw):
        v.integrate(fr.depth, fr.rgb, fr.gt_ids if flags & 1 else None, np.eye(4, dtype=np.float32))
    assert B.states_equal(S.full_download(b), S.full_download(tw), dims)
    tw.close()


@pytest.mark.parametrize("case", ["widens weights", "widens colour", "sub-box"])
def test_unpack_twin(case):
    from semtsdf import _lib as L

    form = "wide_colour" if case == "widens colour" else "wide_weights" if case == "widens weights" else "semantic"
    flags, a_state = _field(DIMS, form)
    _, b_state = _field(DIMS, "semantic" if flags & 1 else "wide_colour", seed=1, holes=False)
    if case == "widens colour":  # B starts with byte colours, A brings 300
        b_state = dict(b_state, color=np.clip(b_state["color"], 0, 255))
        assert a_state["color"].max() == 300 and b_state["color"].max() <= 255
    a, b = _volume(flags, a_state), _volume(flags, b_state)
    assert not B.states_equal(a_state, b_state, DIMS)
    lo, hi = ((0, 1, 2), (2, 4, 6)) if case == "sub-box" else (None, None)
    bricks, words = a.pack_bricks(lo, hi)
    _same((bricks, words), B.numpy_pack(a_state, DIMS, flags, MU, lo, hi), case)
    nb = B.brick_counts(DIMS)
    assert 0 < len(bricks) < (24 if case == "sub-box" else nb[0] * nb[1] * nb[2])
    bytes0 = b.state().device_bytes
    b.unpack_bricks(bricks, words)
    want = B.numpy_unpack(b_state, DIMS, flags, MU, bricks, words)
    if case == "widens weights":
        assert want["wt"].max() == 70000 and b.state().device_bytes == bytes0 + 2 * _stored(DIMS)
    elif case == "widens colour":
        assert want["color"].max() > 255 and b.state().device_bytes == bytes0 + 12 * _stored(DIMS)
    else:
        assert b.state().device_bytes == bytes0
        untouched = np.ones(DIMS, bool)
        untouched[0:16, 8:28, 16:48] = False
        for k, v in B.shaped(b_state, DIMS).items():
            assert np.array_equal(want[k][untouched], v[untouched])  # the expectation keeps B's other bricks
    # the reset bricks of A inside the box were not packed: B keeps its own there
    a_shaped = B.shaped(a_state, DIMS)
    assert any(any(not np.array_equal(want[k][_block(r, DIMS)], a_shaped[k][_block(r, DIMS)]) for k in want)
               for r in RESET if lo is None or all(lo[i] <= r[i] < hi[i] for i in range(3)))
    _twin_check(b, want, flags, DIMS)
    a.close()
    b.close()


def _stored(dims):
    return dims[0] * ((dims[1] + 7) // 8 * 8) * ((dims[2] + 31) // 32 * 32)


def test_unpack_refuses_bad_lists():
    from semtsdf import _lib as L

    flags, state = _field(DIMS, "semantic")
    vol = _volume(flags, state)
    bricks, words = vol.pack_bricks((0, 0, 2), (3, 4, 9))
    assert len(bricks) > 4
    other = _volume(flags, _field(DIMS, "semantic", seed=1)[1])
    before, params = S.full_download(other), bytes(other.get_params())
    words0 = other.map_words().copy()

    def refused(b, w, code=L.ERR_INVALID):
        with pytest.raises(Exception) as e:
            other.unpack_bricks(b, w)
        assert e.value.code == code, e.value
        assert B.states_equal(S.full_download(other), before, DIMS) and bytes(other.get_params()) == params

    swapped = bricks.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    refused(swapped, words)  # unsorted (the offsets then are not the running sum either)
    dup = bricks.copy()
    dup["b"][1] = dup["b"][0]
    refused(dup, words)
    off = bricks.copy()
    off["offset"][2] += 512
    refused(off, words)
    refused(bricks, words[:-512])
    refused(bricks, np.append(words, np.zeros(512, np.uint32)))
    for axis, val in ((0, 3), (1, -1), (2, 9)):
        out = bricks.copy()
        out["b"][-1][axis] = val
        refused(out, words)
    assert np.array_equal(other.map_words(), words0)
    other.unpack_bricks(bricks[:0], words[:0])  # nothing to do: nothing marked stale, nothing changed
    assert B.states_equal(S.full_download(other), before, DIMS)
    # bins on a volume without a histogram
    cflags, cstate = _field(DIMS, "wide_colour")
    plain = _volume(cflags, cstate)
    pb, pw = plain.pack_bricks((0, 0, 2), (1, 1, 4))
    assert len(pb) == 2 and not pb["bins"].any()
    pb["bins"][1] = 1
    with pytest.raises(Exception) as e:
        plain.unpack_bricks(pb, pw)
    assert e.value.code == L.ERR_INVALID
    assert B.states_equal(S.full_download(plain), cstate, DIMS)
    for v in (vol, other, plain):
        v.close()
    # a Z-sharded handle is refused by both calls
    import semtsdf

    q = _params(flags)
    q.z_nshards, q.z_shard, q.z_chunk = 2, 0, 8
    shard = semtsdf.Volume(q, 0)
    one = (bricks[:1], words[:int(bricks["offset"][1])])
    # ... whatever else is wrong with the arguments: a box outside the volume, a malformed list
    for call in (lambda: shard.pack_bricks((0, 0, 0), (1, 1, 1)), lambda: shard.unpack_bricks(*one),
                 lambda: shard.pack_bricks((0, 0, -1), (1, 1, 99)), lambda: shard.unpack_bricks(dup, words),
                 lambda: shard.unpack_bricks(bricks[:0], words[:0])):
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == L.ERR_UNSUPPORTED
    shard.close()


def _fused_volume():
    import semtsdf

    semtsdf.load()
    sc = R.fused_scene()
    vol = semtsdf.Volume(sc["p"], 0)
    for k in range(1, 4):
        fr = sc["frames"][k]
        vol.integrate(fr.depth, fr.rgb, fr.gt_ids, sc["E"][k])
    return vol


def test_round_trip_through_a_shift():
    from semtsdf.bricks import BrickStore, shift_paged

    vol, plain = _fused_volume(), _fused_volume()
    dims, mu = (64, 64, 64), float(vol.params.mu)
    home = S.full_download(vol)
    nbricks = len(B.numpy_pack(home, dims, 0x3, mu)[0])
    assert 0 < nbricks < 512  # the fused scene leaves empty bricks: occupancy matters
    store = BrickStore()
    for s in ((8, 0, -8), (-8, 0, 8)):
        shift_paged(vol, store, s)
        plain.shift(*s)
    assert store.origin == [0, 0, 0] and len(store) == 0
    assert B.states_equal(S.full_download(vol), home, dims)
    assert not B.states_equal(S.full_download(plain), home, dims)  # the plain shifts lost what left
    assert bytes(vol.get_params()) == bytes(plain.get_params())
    plain.close()
    # five shifts that sum to zero, against the canvas model after each
    canvas = B.Canvas(home, dims, 0x3, mu, margin=16)
    world0 = {k: v.copy() for k, v in canvas.world.items()}
    walk = [(8, 8, 0), (0, -16, 8), (-16, 0, 0), (8, 8, 0), (0, 0, -8)]
    assert np.sum(walk, axis=0).tolist() == [0, 0, 0]
    for k, s in enumerate(walk):
        shift_paged(vol, store, s)
        assert B.states_equal(S.full_download(vol), canvas.shift(s), dims), (k, s)
        assert (len(store) > 0) == (k < len(walk) - 1)
    assert store.origin == [0, 0, 0]
    # a walk that ends one brick away: the window is the plain shift of the original, and window and
    # store together are still the original world
    for s in ((0, 8, 0), (8, -8, 0)):
        shift_paged(vol, store, s)
    assert store.origin == [1, 0, 0]
    window = S.full_download(vol)
    assert B.states_equal(window, S.numpy_shift(home, (8, 0, 0), mu, dims=dims), dims)
    assert {k[0] for k in store.keys()} == {0} and 0 < len(store) <= 64
    items = [(k,) + store.get(k) for k in store.keys()]
    world = B.rebuild_world(window, items, store.origin, dims, 0x3, mu, margin=16)
    assert B.states_equal(world, world0, [d + 32 for d in dims])
    vol.close()


def test_follow_with_a_store():
    import semtsdf
    from semtsdf.bricks import BrickStore

    semtsdf.load()
    st = S.sequence_stream()
    frames = [st.frame(k) for k in range(4)]
    focus = S.sequence_focus_depth(frames[0])
    K = S.sequence_intrinsics()
    paged, plain = semtsdf.TSDF(K, S.SEQ_DIM), semtsdf.TSDF(K, S.SEQ_DIM)
    for t in (paged, plain):
        for fr in frames:
            t.parse_frame(fr.depth, fr.rgb, fr.w2c, focus, np.ascontiguousarray(fr.mask.copy()))
    dims, mu, flags = (S.SEQ_DIM,) * 3, float(paged.vol.params.mu), int(paged.vol.params.flags) & 0xD
    assert flags == 0x1
    home, home_params = S.full_download(paged.vol), bytes(paged.vol.get_params())
    home_valid = int((paged.model_maps(extrinsic=frames[3].w2c)["flags"] & 1).sum())
    assert home_valid >= 500
    poses = [np.linalg.inv(st.c2w(k)) for k in range(S.SEQ_FRAMES)]
    store = BrickStore()
    out = poses[4:] + poses[::-1]
    moved = 0
    for pose in out:
        s = paged.follow(pose, focus_depth=focus, trigger_bricks=1, store=store)
        assert s == plain.follow(pose, focus_depth=focus, trigger_bricks=1)
        moved += s is not None
        if pose is poses[-1]:
            far, far_bricks = list(store.origin), len(store)
    assert moved >= 4 and any(far) and far_bricks > 0 and paged.store is store and plain.store is None
    # a store that cannot page for this volume is refused before anything happens: no eviction report,
    # no shift, and it is not remembered
    alien, seen = BrickStore(), []
    alien.flags = 0x4
    before = bytes(paged.vol.get_params())
    with pytest.raises(ValueError):
        paged.follow(poses[-1], focus_depth=focus, trigger_bricks=1, store=alien, on_evict=seen.append)
    assert paged.store is store and not seen and len(alien) == 0 and bytes(paged.vol.get_params()) == before
    # window and store rebuild the world of before the walk, at the store's final origin
    items = [(k,) + store.get(k) for k in store.keys()]
    reach = [abs(o) for o in store.origin] + [max(-k[a], k[a] - 7, 0) for k in store.keys() for a in range(3)]
    margin = 8 * (max(reach) + 1)
    window = S.full_download(paged.vol)
    world = B.rebuild_world(window, items, store.origin, dims, flags, mu, margin)
    world0 = B.Canvas(home, dims, flags, mu, margin).world
    assert B.states_equal(world, world0, [d + 2 * margin for d in dims])
    valid = int((paged.model_maps(extrinsic=frames[3].w2c)["flags"] & 1).sum())
    lost = int((plain.model_maps(extrinsic=frames[3].w2c)["flags"] & 1).sum())
    assert valid > lost, (valid, lost)
    if store.origin == [0, 0, 0] and bytes(paged.vol.get_params()) == home_params:
        assert valid == home_valid and B.states_equal(window, home, dims)
    # prune_instances applies its table to the store too: out again, then dissolve every instance
    for pose in poses[4:]:
        paged.follow(pose, focus_depth=focus, trigger_bricks=1, store=store)
    kept = {k: store.get(k) for k in store.keys()}
    assert any(bins & ~1 for bins, _ in kept.values())  # the store holds instance bins to merge
    lut, _ = paged.prune_instances(min_voxels=10 ** 9)
    lut = [int(x) for x in np.asarray(lut).reshape(-1)]
    assert len(lut) == 32 and len(set(lut)) < 32  # a merging table
    for k, (bins, rec) in kept.items():
        one = np.zeros(1, B.BRICK_DTYPE)
        one["bins"] = bins
        dense = B.numpy_unpack(B.reset_state((8, 8, 8), flags, mu), (8, 8, 8), flags, mu, one, rec)
        merged = np.zeros_like(dense["hist"])
        for j in range(32):
            merged[..., lut[j]] += dense["hist"][..., j]
        dense["hist"] = merged
        wb, ww = B.numpy_pack(dense, (8, 8, 8), flags, mu)
        got = store.get(k)
        assert len(wb) == 1 and got[0] == int(wb["bins"][0]) and np.array_equal(got[1], ww), k
    assert any(store.get(k)[0] != bins for k, (bins, _) in kept.items())
    paged.close()
    plain.close()
