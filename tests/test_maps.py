"""CPU: the restatement of the empty-space maps against the definition written as loops, and the
input conditions of tests/test_gpu_map_updates.py proved from the C oracle alone (the counts
each case needs of its seed: crossings per lane and brick position, bricks that flip each way,
values within an ulp of the threshold, whole free units).  The 256^3 dirty-list case asserts
its own condition before its GPU call: its oracle frame costs as much as the test it guards."""
import math

import numpy as np
import pytest

import maps_restatement as R
from maps_restatement import CAP, naive_maps, numpy_maps


# ------------------------------------------------------------- the restatement against the loops
@pytest.mark.parametrize("dims", [(9, 17, 70), (8, 8, 8), (1, 1, 1), (136, 8, 8), (8, 136, 8), (8, 8, 136),
                                  (24, 17, 40)])
def test_numpy_maps_equal_the_loops(dims):
    """Random fields from the seed's sdf classes: `dense` draws every voxel from all classes (no
    brick skippable), `sparse` keeps one draw in 2048 below the threshold (most bricks skippable,
    distances of a few bricks), `high` none (every byte at the cap, whatever the number of bricks),
    `one_low` one voxel of brick 0 (with 17 bricks along an axis the distances 0..15 and the cap
    all occur: the cap is reached at brick 15 and exceeded at brick 16)."""
    voxel = 0.0625
    thr = R.skip_threshold(voxel)
    n = dims[0] * dims[1] * dims[2]
    rng = np.random.default_rng(n)
    draws = R.sdf_classes(rng, n, thr, 0.3125)
    hi = np.where(draws >= thr, draws, np.float32(1.0)).astype(np.float32)
    fields = {"dense": draws, "sparse": np.where(rng.uniform(0, 1, n) < 1.0 / 2048, draws, hi).astype(np.float32),
              "high": hi, "one_low": hi.copy()}
    fields["one_low"][0] = np.float32(0.0)  # brick 0 alone non-skippable: distances 0, 1, 2, ... from it
    seen = set()
    for name, fld in fields.items():
        s = fld.reshape(dims)
        a, b = numpy_maps(s, voxel), naive_maps(s, voxel)
        assert a.dtype == np.uint64 and a.shape == b.shape
        assert np.array_equal(a, b), (name, int(np.count_nonzero(a != b)))
        seen |= set(np.unique(a.view(np.uint8)).tolist())
    assert (fields["high"] >= thr).all()
    assert np.array_equal(numpy_maps(fields["high"].reshape(dims), voxel),
                          np.full(a.size, CAP * 0x0101010101010101, np.uint64))
    if max(dims) == 136:  # 17 bricks along one axis: every distance from 0 to the cap occurs
        assert seen == set(range(CAP + 1)), sorted(seen)


def test_threshold_is_the_f32_formula():
    voxel = np.float32(0.06525779)
    thr = R.skip_threshold(voxel)
    assert thr.dtype == np.float32 and thr == np.float32(np.float32(voxel / np.float32(2)) * np.float32(1 + 2.0 ** -16))
    s = np.full((8, 8, 8), thr, np.float32)
    assert (numpy_maps(s, voxel) == np.uint64(CAP * 0x0101010101010101)).all()  # >=: equal is skippable
    s[3, 4, 5] = np.nextafter(thr, np.float32(-np.inf))
    assert (numpy_maps(s, voxel) == 0).all() and (naive_maps(s, voxel) == 0).all()


# --------------------------------------------------------------------- a. seeded single frame
def seeded_counts(c):
    """The counts of the issue's conditions from the oracle's before / after sdf."""
    dims, thr, voxel = c.dims, c.thr, c.p.voxel[0]
    before, after = c.seed["sdf"], c.ost.sdf
    dn, up = R.crossings(before, after, thr)
    dn3, up3 = dn.reshape(dims), up.reshape(dims)
    z = np.arange(dims[2])
    out = {"lane": [[int(m[:, :, z % 4 == k].sum()) for k in range(4)] for m in (dn3, up3)],
           "brick": [[int(m[:, :, (z // 8) % 4 == k].sum()) for k in range(4)] for m in (dn3, up3)],
           "last_quad": int((dn3 | up3)[:, :, (dims[2] - 1) // 32 * 32:].sum())}
    s0, s1 = R.brick_skippable(before.reshape(dims), voxel), R.brick_skippable(after.reshape(dims), voxel)
    cb = R.brick_any(dn3 | up3)
    w0 = numpy_maps(before.reshape(dims), voxel).reshape(s0.shape)
    w1 = numpy_maps(after.reshape(dims), voxel).reshape(s0.shape)
    out["skip_to_not"], out["not_to_skip"] = int((s0 & ~s1).sum()), int((~s0 & s1).sum())
    out["cross_keep"] = int((cb & (s0 == s1)).sum())
    out["distance_only"] = int((~cb & (w0 != w1)).sum())
    wq, tq = c.seed["wt"].reshape(-1, 4), c.touched.reshape(-1, 4)  # z fastest: a lane's 4 voxels
    out["mixed_lanes"] = int((tq.any(1) & ((wq < R.RCP_TABLE) & tq).any(1) & ((wq >= R.RCP_TABLE) & tq).any(1)).sum())
    num = c.seed["sdf"].astype(np.float64) * c.seed["wt"] + c.f.astype(np.float64)  # exact in f64
    out["zero_numerator"] = int((c.touched & (num == 0.0) & (c.seed["wt"] > 0)).sum())
    return out


@pytest.mark.parametrize("flags", R.SEED_FLAGS, ids=[hex(f) for f in R.SEED_FLAGS])
def test_seeded_frame_conditions(oracle, flags):
    """Measured (the same for every flag set, the sdf and weight draws come first): crossings per
    lane position down 2039 2066 2134 2015, up 1320 1337 1366 1393; per brick position of a quad
    down 5163 426 255 2410, up 1462 996 1309 1649; 4904 in the lone brick of the last quad; 38
    bricks flip skippable -> not, 27 not -> skippable, 133 hold a crossing and keep their side, 76
    change their word without a crossing; 16 232 touched lanes mix table and division weights;
    64 touched voxels have a zero numerator."""
    c = R.seeded_case(oracle, flags)
    assert c.dims == (44, 36, 136) and (c.dims[2] + 7) // 8 == 17
    assert np.isfinite(c.seed["sdf"]).all() and set(np.unique(c.seed["wt"])) <= set(R.WEIGHTS)
    if c.seed["hist"] is not None:
        assert (c.seed["hist"].reshape(-1, 32).sum(axis=1) <= c.seed["wt"]).all()
    n = seeded_counts(c)
    print(flags, n)
    assert min(n["lane"][0]) >= 1 and min(n["lane"][1]) >= 1, n
    assert min(n["brick"][0]) >= 1 and min(n["brick"][1]) >= 1, n
    assert n["last_quad"] >= 1, n
    assert n["skip_to_not"] >= 20 and n["not_to_skip"] >= 20 and n["cross_keep"] >= 20, n
    assert n["distance_only"] >= 1 and n["mixed_lanes"] >= 100 and n["zero_numerator"] >= 1, n
    ref = R.seeded_case(oracle, 0x3)
    assert np.array_equal(c.seed["sdf"].view(np.uint32), ref.seed["sdf"].view(np.uint32))
    assert np.array_equal(c.ost.sdf.view(np.uint32), ref.ost.sdf.view(np.uint32))
    assert np.array_equal(c.ost.wt, ref.ost.wt)


# ------------------------------------------------------------------ b. values at the threshold
def test_threshold_case_conditions(oracle):
    """Measured: 24 voxels for each of the 9 pairs of {below, equal, above}^2 end exactly on thr or
    one ulp beside it; 3 bricks flip through their only sub-threshold voxel becoming equal."""
    c = R.threshold_case(oracle)
    dn1, thr, up1 = c.near3
    assert thr == c.thr and dn1 < thr < up1
    allowed = np.array([thr, dn1, up1, 0.0], np.float32)
    assert np.isin(c.seed["sdf"], allowed).all()  # -0.0 == 0.0
    assert (np.signbit(c.seed["sdf"]) & (c.seed["sdf"] == 0)).sum() > 1000
    v = np.array([pl[0] for pl in c.planted])
    assert (c.seed["wt"][v] <= R.THRESHOLD_WMAX).all() and c.seed["wt"].max() <= R.LONE_WMAX
    pairs = {}
    for vi, so, target in c.planted:
        assert c.seed["sdf"][vi] == np.float32(so) and c.touched[vi]
        if c.ost.sdf[vi] == np.float32(target):  # the oracle's own result, not the solver's
            key = (int(R.side(so, thr)), int(R.side(target, thr)))
            pairs[key] = pairs.get(key, 0) + 1
    print(pairs)
    assert len(pairs) == 9 and min(pairs.values()) >= 1, pairs
    s0 = R.brick_skippable(c.seed["sdf"].reshape(c.dims), c.p.voxel[0])
    s1 = R.brick_skippable(c.ost.sdf.reshape(c.dims), c.p.voxel[0])
    b3, a3 = c.seed["sdf"].reshape(c.dims), c.ost.sdf.reshape(c.dims)
    flips = 0
    for (bx, by, bz), vi in c.lone:
        hood = (slice(8 * bx, 8 * bx + 16), slice(8 * by, 8 * by + 16), slice(8 * bz, 8 * bz + 16))
        if (b3[hood] < thr).sum() == 1 and c.seed["sdf"][vi] == dn1 and c.ost.sdf[vi] == thr and \
                (a3[hood] >= thr).all() and not s0[bx, by, bz] and s1[bx, by, bz]:
            flips += 1
    print("lone bricks:", flips, [int(c.seed["wt"][vi]) for _, vi in c.lone])
    assert flips >= 1
    # equal -> equal and above -> equal keep their brick's side (>= : equal counts as above)
    dn, up = R.crossings(c.seed["sdf"], c.ost.sdf, thr)
    for vi, so, target in c.planted:
        if so >= thr and c.ost.sdf[vi] == thr:
            assert not dn[vi] and not up[vi]


# ------------------------------------------------------------------------- c. deferred updates
def test_deferred_frames_each_dirty_other_bricks(oracle):
    """Frames 1..5 of the deferred sequences: every frame after the first holds crossings, and in
    bricks the frame before it left alone (so the dirty bits of several integrates differ)."""
    p = R.make_params(R.DIMS)
    g = oracle.OGeom.from_params(p)
    ost = R.new_ostate(oracle, R.DIMS, p.mu, 0x3)
    thr = R.skip_threshold(p.voxel[0])
    prev = None
    for k in range(1, 6):
        before = ost.sdf.copy()
        R.integrate_frame(oracle, g, p, ost, R.frames()[k], R.pose(k), 0x3)
        dn, up = R.crossings(before, ost.sdf, thr)
        cb = R.brick_any((dn | up).reshape(R.DIMS))
        assert cb.sum() >= 1, k
        if prev is not None:
            assert (cb & ~prev).sum() >= 1, k
        prev = cb


# ------------------------------------------------------------- d. a surface appears and goes
def test_surface_case_conditions(oracle):
    """Measured: non-skippable bricks after each frame of P P Q Q Q P P P: 0 0 0 8 12 8 0 0 (the
    issue's P P Q P P P cannot change a brick: (2 + f) / 3 > 1/3 for every f > -1)."""
    c = R.surface_case(oracle)
    voxel = c.p.voxel[0]
    count = [int((~R.brick_skippable(s.sdf.reshape(c.dims), voxel)).sum()) for s in c.states]
    print(count)
    full = np.uint64(CAP * 0x0101010101010101)
    assert (numpy_maps(c.states[1].sdf.reshape(c.dims), voxel) == full).all()
    last_q = R.SURFACE_SEQ.rindex("Q")
    assert count[last_q] >= 4 and count[-1] == 0
    assert (numpy_maps(c.states[-1].sdf.reshape(c.dims), voxel) == full).all()


# ----------------------------------------------------------------- e. free and full-free units
@pytest.mark.parametrize("name", ["head_on", "flip"])
def test_free_case_conditions(oracle, name):
    """Measured, whole 1x8x16 units touched throughout with f == 1: head_on 787, flip 2540 (of
    6912); upward crossings inside them: head_on 55 570, flip 179 354."""
    c = R.free_case(oracle, name)
    assert max(c.dims) <= 96 and (c.depth > 0).all()
    t3, f3 = c.touched.reshape(c.dims), c.f.reshape(c.dims)
    free = R.whole_units(t3 & (f3 == 1.0))
    some = R.whole_units(~t3 | (f3 == 1.0)) & ~R.whole_units(~t3)
    dn, up = R.crossings(c.seed["sdf"], c.ost.sdf, c.thr)
    assert (c.seed["sdf"][c.touched & (c.f == 1.0)] < c.thr).all()
    X, Y, Z = c.dims
    up_in = int((up.reshape(c.dims)[:, :Y // 8 * 8, :Z // 16 * 16].reshape(X, Y // 8, 8, Z // 16, 16)
                 & free[:, :, None, :, None]).sum())
    print(name, int(free.sum()), int(some.sum()), free.size, up_in)
    assert free.sum() >= 50 and some.sum() >= free.sum() and up_in >= 1000
    if name == "flip":
        E64 = np.asarray(c.E, np.float64)
        vs, vx = np.array(c.p.vol_start[:], np.float64), np.array(c.p.voxel[:], np.float64)
        ax = [vs[i] + np.arange(c.dims[i]) * vx[i] for i in range(3)]
        qz = (E64[2, 0] * ax[0][:, None, None] + E64[2, 1] * ax[1][None, :, None] + E64[2, 2] * ax[2][None, None, :]
              + E64[2, 3])
        assert (qz[t3] <= 0).all() and (f3[t3] == 1.0).all() and t3.sum() > 10000


# ------------------------------------------------------------------------------------ f. shards
@pytest.mark.parametrize("nshards,chunk", R.SHARDS)
def test_shard_case_conditions(oracle, nshards, chunk):
    """Every shard's local seed holds crossings in both directions, and over the shards bricks of
    the local maps flip both ways; chunks of 5 and 2 planes put chunk boundaries inside bricks."""
    from semtsdf.shard import ShardLayout

    lay = ShardLayout(R.SHARD_DIMS[2], nshards, chunk)
    flips = np.zeros(2, np.int64)
    for s in range(nshards):
        c = R.shard_case(oracle, nshards, chunk, s)
        assert c.dims[2] == lay.local_planes(s) and c.seed["sdf"].size == c.dims[0] * c.dims[1] * c.dims[2]
        dn, up = R.crossings(c.seed["sdf"], c.ost.sdf, c.thr)
        assert dn.sum() >= 1 and up.sum() >= 1, (s, int(dn.sum()), int(up.sum()))
        s0 = R.brick_skippable(c.seed["sdf"].reshape(c.dims), c.p.voxel[0])
        s1 = R.brick_skippable(c.ost.sdf.reshape(c.dims), c.p.voxel[0])
        flips += (int((s0 & ~s1).sum()), int((~s0 & s1).sum()))
    print(nshards, chunk, flips.tolist())
    assert (flips >= 1).all(), flips.tolist()
    if chunk in (5, 2):
        assert (chunk + 1) % 8 != 0


# -------------------------------------------------------------- h. the views of the stream case
def test_stream_case_views_hit(oracle):
    """The two views of the caller-stream case see the surface (hit shares above 5 %)."""
    p = R.make_params(R.DIMS)
    g = oracle.OGeom.from_params(p)
    ost = R.new_ostate(oracle, R.DIMS, p.mu, 0x3)
    for k, angle in ((1, 0.2), (2, math.pi)):
        R.integrate_frame(oracle, g, p, ost, R.frames()[k], R.pose(k), 0x3)
        s2w, c = oracle.orbit_camera(list(p.Kinv), angle, R.mean_depth() * R.PLACE)
        img, t = oracle.render(g, s2w, c, R.W, R.H, 0, ost.sdf, ost.hist, ost.color)
        print(angle, float((t >= 0).mean()))
        assert (t >= 0).mean() > 0.05
