"""GPU: the incremental update of the empty-space maps (crossing detection in stage_compute, dirty
marking in stage_store, k_brick_plain over the dirty list, the list reset in k_brick_dilate, the
deferral to the first march or map query) against the map's definition.  Every assertion is
exact: np.array_equal of map_words() with maps_restatement.numpy_maps of the handle's own
downloaded sdf and, where a case says so, of the whole state with the C oracle on the same seed.
tests/test_maps.py proves on the CPU, from the oracle alone, that every input below holds the
crossings, flips and values its case is about (case g asserts its own before its GPU call).

An upload or a reset marks the whole map stale, and the next query rebuilds every brick.  So each
case that uploads a seed queries the map once before its frame: the query after the frame is
then the incremental update, from the dirty bits of that frame alone.

Which case reaches which code path
  crossing detection (sign of so - thr XOR sign of sn - thr, ORed over the lane's 4 voxels):
      a: downward and upward crossings at each of the 4 positions of a lane; b: every pair of
      {1 ulp below, equal, 1 ulp above}^2 (equal counts as above: only pairs that change side
      mark); e: upward crossings in the FREE template and in the full-free path without projection.
  dirty marking (ballot -> z-brick of the unit -> bit of the quad's word, first setter lists the quad):
      a: crossings in each of the 4 bricks of a quad and in the lone brick of the last quad
      (nbz = 17), all four flag sets (0x3, 0x1, 0x4, 0xC: the SEM / CI32 / VOTE templates), with and
      without the unit cull; f: shards, whose z-bricks are bricks of the local storage (halo planes
      included, chunks of 5 and 2 planes put chunk boundaries inside bricks).
  dirty recompute (k_brick_plain(all = 0); the stale minima of the other bricks stay on their side):
      a: bricks that flip either way, bricks that hold a crossing and keep their side, words that
      change through a neighbour alone; b: the brick whose only sub-threshold voxel becomes equal;
      d: a surface that appears in a volume at the cap and goes again; g: 4764 dirty quads, more
      than the 4096 waves of one pass (the second trip of the grid-stride loop).
  list reset and deferral (k_brick_dilate; maps_dirty / maps_stale in ensure_maps):
      c: dirty bits of 5 integrates consumed at once; a reset, an upload and a remap between the
      marking and the update; then one more frame on the map the full rebuild left.
  update on the stream of the march that needs it (order_after_map): h.
  running means at the reciprocal table's end (kRcpTable = 1024): a, e and f draw every weight from
      {0, 1, 2, 7, 1022, 1023, 1024, 1025, 4095, 4096} per voxel (lanes mix both paths), with 64
      zero numerators (the 0x1p-60 path); b holds weights up to 2.6e8.

Cull-class counters of case e (free_units, full_units of semtsdf_timing for the case's frame, flags
0x3, a (96, 96, 96) volume of 6912 units), measured on an MI355X:
            touched   gated   bricks  free_units  full_units
  head_on    304195   67575     4334        1727         552
  flip       439339       0     4256        4256        2536
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import maps_restatement as R
from instances_restatement import remap_hist
from maps_restatement import CAP, numpy_maps

pytestmark = pytest.mark.gpu

FULL = np.uint64(CAP * 0x0101010101010101)


@pytest.fixture(scope="module")
def S():
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    return semtsdf, L


# ---------------------------------------------------------------------------------- helpers
def new_volume(S, p, count=False):
    semtsdf, L = S
    vol = semtsdf.Volume(p, 0)
    vol.set_instrumentation(events=False, count=count)
    return vol


def upload_seed(vol, seed):
    vol.upload(**{k: v for k, v in seed.items() if v is not None})


def check_map(vol, voxel, tag=None):
    """map_words() against the definition on the handle's own stored sdf; returns the words."""
    wa = vol.map_words()
    assert wa is not None
    s = vol.download(wt=False, color=False)["sdf"].reshape(vol.local_dim)
    ref = numpy_maps(s, voxel)
    assert np.array_equal(wa, ref), (tag, int(np.count_nonzero(wa != ref)), int(wa.size))
    return wa


def assert_state(vol, ost, flags):
    out = vol.download(hist=bool(flags & 1), cls=bool(flags & 8))
    assert np.array_equal(out["sdf"].view(np.uint32), ost.sdf.view(np.uint32)), "sdf bits"
    assert np.array_equal(out["wt"], ost.wt), "weight"
    assert np.array_equal(out["color"], ost.color), "colour"
    if flags & 1:
        assert np.array_equal(out["hist"], ost.hist), "histogram"
    if flags & 8:
        assert np.array_equal(out["cls"], ost.cls) and np.array_equal(out["cls_cnt"], ost.cls_cnt), "vote"


def integrate(S, vol, fr, E, flags, depth=None):
    """One frame through the entry point of the flag set (vote volumes: integrate_vote_dev with
    device buffers)."""
    from semtsdf.volume import DeviceBuffer

    d = np.ascontiguousarray(fr.depth if depth is None else depth, np.uint16)
    if flags & 8:
        rgb = np.ascontiguousarray(fr.rgb, np.uint8)
        cls = np.ascontiguousarray(fr.gt_ids.astype(np.int32))
        bufs = [DeviceBuffer(a.nbytes) for a in (d, rgb, cls)]
        for b, a in zip(bufs, (d, rgb, cls)):
            b.upload(a)
        vol.sync()
        vol.integrate_vote_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, E)
        vol.sync()
        for b in bufs:
            b.free()
    else:
        vol.integrate(d, fr.rgb, fr.gt_ids if flags & 1 else None, E)


def seeded_run(S, c, p, count=False):
    """Upload c's seed, query (the full rebuild, on the seed), integrate c's frame, query (the
    incremental update), compare the state with the oracle's.  Returns (volume, timing)."""
    vol = new_volume(S, p, count)
    upload_seed(vol, c.seed)
    check_map(vol, p.voxel[0], "seed")
    vol.reset_timing()
    integrate(S, vol, c.fr, c.E, c.flags, depth=c.depth)
    tm = vol.timing()
    check_map(vol, p.voxel[0], "frame")
    assert_state(vol, c.ost, c.flags)
    return vol, tm


# --------------------------------------------------------------------- a. seeded single frame
@pytest.mark.parametrize("cull", [True, False], ids=["cull", "nocull"])
@pytest.mark.parametrize("flags", R.SEED_FLAGS, ids=[hex(f) for f in R.SEED_FLAGS])
def test_seeded_single_frame(S, oracle, flags, cull):
    c = R.seeded_case(oracle, flags)
    vol, tm = seeded_run(S, c, R.make_params(c.dims, flags, cull), count=flags == 0x3)
    if flags == 0x3:
        assert (tm.touched, tm.gated) == (int(c.counts[0]), int(c.counts[1]))
    vol.close()


# ------------------------------------------------------------------ b. values at the threshold
def test_values_at_the_threshold(S, oracle):
    c = R.threshold_case(oracle)
    vol, _ = seeded_run(S, c, R.make_params(c.dims, c.flags))
    vol.close()


# ------------------------------------------------------------------------- c. deferred updates
def oracle_frames(oracle, p, ost, ks):
    g = oracle.OGeom.from_params(p)
    for k in ks:
        R.integrate_frame(oracle, g, p, ost, R.frames()[k], R.pose(k), 0x3)
    return ost


def test_deferred_update_equals_update_per_frame(S, oracle):
    p = R.make_params(R.DIMS)
    a, b = new_volume(S, p), new_volume(S, p)
    check_map(b, p.voxel[0], "fresh")  # the later single query updates incrementally
    for k in range(1, 6):
        for v in (a, b):
            integrate(S, v, R.frames()[k], R.pose(k), 0x3)
        wa = check_map(a, p.voxel[0], k)
    wb = check_map(b, p.voxel[0], "deferred")
    assert np.array_equal(wa, wb)
    ost = oracle_frames(oracle, p, R.new_ostate(oracle, R.DIMS, p.mu, 0x3), range(1, 6))
    assert_state(b, ost, 0x3)
    assert 0 < np.count_nonzero((wb & np.uint64(0xFF)) > 0) < wb.size
    a.close()
    b.close()


@pytest.mark.parametrize("between", ["reset", "upload", "remap"])
def test_deferred_update_across(S, oracle, between):
    """integrate x2, then a reset, an upload of a seed's sdf or a remap with a merging table, then
    integrate x2 (x1 after the remap), and only then the first query since the fresh volume's; one
    more frame after it updates incrementally on that map."""
    p = R.make_params(R.DIMS)
    vol = new_volume(S, p)
    check_map(vol, p.voxel[0], "fresh")
    ost = R.new_ostate(oracle, R.DIMS, p.mu, 0x3)
    for k in (1, 2):
        integrate(S, vol, R.frames()[k], R.pose(k), 0x3)
    oracle_frames(oracle, p, ost, (1, 2))
    if between == "reset":
        vol.reset()
        ost = R.new_ostate(oracle, R.DIMS, p.mu, 0x3)
        rest = (3, 4)
    elif between == "upload":
        sdf = R.seeded_case(oracle, 0x3).seed["sdf"]
        vol.upload(sdf=sdf)
        ost.sdf[:] = sdf
        rest = (3, 4)
    else:
        lut = np.arange(32, dtype=np.uint8)
        lut[2] = 1  # id 2 merges into id 1
        assert ost.hist.reshape(-1, 32)[:, 2].sum() > 0
        vol.remap_instances(lut)
        ost.hist[:] = remap_hist(ost.hist, lut)
        rest = (3,)
    for k in rest:
        integrate(S, vol, R.frames()[k], R.pose(k), 0x3)
    oracle_frames(oracle, p, ost, rest)
    check_map(vol, p.voxel[0], between)
    assert_state(vol, ost, 0x3)
    integrate(S, vol, R.frames()[5], R.pose(5), 0x3)
    oracle_frames(oracle, p, ost, (5,))
    check_map(vol, p.voxel[0], "one more")
    assert_state(vol, ost, 0x3)
    vol.close()


# ------------------------------------------------------------- d. a surface appears and goes
def surface_views(oracle, c):
    """The oracle's label and colour renders at orbit angles 0.2 and pi and its association
    probabilities at the frames' pose, after the last Q and after the last P (computed once, on a
    thread pool: each is a 640 x 480 march)."""
    def build():
        jobs = {}
        with ThreadPoolExecutor(8) as ex:
            for at in (R.SURFACE_SEQ.rindex("Q"), len(R.SURFACE_SEQ) - 1):
                st = c.states[at]
                for angle in (0.2, math.pi):
                    s2w, cam = oracle.orbit_camera(list(c.p.Kinv), angle, R.mean_depth() * R.PLACE)
                    for mode in (0, 1):
                        jobs[(at, angle, mode)] = ex.submit(oracle.render, c.g, s2w, cam, R.W, R.H, mode, st.sdf,
                                                            st.hist, st.color)
                jobs[(at, "probs")] = ex.submit(oracle.march_probs, c.g, list(c.p.Kinv), c.E, R.W, R.H, st.sdf,
                                                st.hist, c.p.box_thresh)
            return {k: j.result() for k, j in jobs.items()}

    return R.cached("surface views", build)


def test_surface_appears_and_goes(S, oracle):
    semtsdf, L = S
    c = R.surface_case(oracle)
    ref = surface_views(oracle, c)
    last_q, last = R.SURFACE_SEQ.rindex("Q"), len(R.SURFACE_SEQ) - 1
    # the oracle sees the patch after the last Q (1115 and 4048 hit pixels) and nothing at the end
    assert (ref[(last_q, 0.2, 0)][1] >= 0).sum() >= 500 and (ref[(last_q, math.pi, 0)][1] >= 0).sum() >= 500
    assert (ref[(last_q, "probs")][0] > 0).sum() >= 500
    assert (ref[(last, 0.2, 0)][1] >= 0).sum() == 0 and (ref[(last, "probs")][0] > 0).sum() == 0
    vol = new_volume(S, c.p)
    depth = R.surface_frames()
    for i, ch in enumerate(R.SURFACE_SEQ):
        integrate(S, vol, c.fr, c.E, 0x3, depth=depth[ch])
        wa = check_map(vol, c.p.voxel[0], (i, ch))
        if i < R.SURFACE_SEQ.index("Q") or i == last:
            assert (wa == FULL).all(), i
        if i == last_q:
            assert 4 <= np.count_nonzero((wa & np.uint64(0xFF)) == 0) < wa.size
        if i in (last_q, last):
            assert_state(vol, c.states[i], 0x3)
            for angle in (0.2, math.pi):
                s2w, cam = semtsdf.orbit_camera(list(c.p.Kinv), angle, R.mean_depth() * R.PLACE)
                for mode in (L.RENDER_LABEL, L.RENDER_COLOR):
                    img, t = vol.raycast(s2w, cam, mode, want_t=True)
                    img_o, t_o = ref[(i, angle, int(mode))]
                    assert np.array_equal(t.view(np.uint32), t_o.view(np.uint32)), (i, angle, mode)
                    assert np.array_equal(img, img_o), (i, angle, mode)
            vol.set_state(i + 1, 7)
            probs, box = vol.assoc_probs(c.E)
            probs_o, box_o = ref[(i, "probs")]
            assert np.array_equal(probs.reshape(-1).view(np.uint32), probs_o.view(np.uint32)), i
            assert np.array_equal(box.reshape(-1), box_o), i
    vol.close()


# ----------------------------------------------------------------- e. free and full-free units
@pytest.mark.parametrize("name", ["head_on", "flip"])
def test_free_and_full_free_units(S, oracle, name):
    c = R.free_case(oracle, name)
    vol, tm = seeded_run(S, c, R.make_params(c.dims, c.flags), count=True)
    print(f"free case {name}: touched {tm.touched} gated {tm.gated} bricks {tm.bricks} free_units {tm.free_units} "
          f"full_units {tm.full_units}")
    assert (tm.touched, tm.gated) == (int(c.counts[0]), int(c.counts[1]))
    assert tm.free_units > 0 and tm.full_units > 0
    vol.close()


# ------------------------------------------------------------------------------------ f. shards
def shard_handles(S, p, nshards, chunk):
    """As _shard_handles of test_gpu_parity.py."""
    semtsdf, L = S
    shards = []
    for sidx in range(nshards):
        q = semtsdf.default_params(64, R.KI, R.W, R.H)
        for fld in ("dim", "vol_start", "vol_end", "voxel", "K", "Kinv"):
            getattr(q, fld)[:] = getattr(p, fld)[:]
        q.mu, q.flags = p.mu, p.flags
        q.z_nshards, q.z_shard, q.z_chunk = nshards, sidx, chunk
        shards.append(semtsdf.Volume(q, 0))
    return shards


@pytest.mark.parametrize("nshards,chunk", R.SHARDS)
def test_shards_seeded_and_deferred(S, oracle, nshards, chunk):
    from semtsdf.shard import ShardLayout

    p = R.make_params(R.SHARD_DIMS)
    lay = ShardLayout(R.SHARD_DIMS[2], nshards, chunk)
    # sequence a on every shard's local storage
    shards = shard_handles(S, p, nshards, chunk)
    for sidx, sh in enumerate(shards):
        c = R.shard_case(oracle, nshards, chunk, sidx)
        assert tuple(sh.local_dim) == c.dims and np.array_equal(lay.local_to_global(sidx), c.zmap)
        upload_seed(sh, c.seed)
        check_map(sh, p.voxel[0], ("seed", sidx))
        integrate(S, sh, c.fr, c.E, 0x3)
        check_map(sh, p.voxel[0], ("frame", sidx))
        assert_state(sh, c.ost, 0x3)
        sh.close()
    # sequence c, first variant: a query per frame against one query at the end
    a, b = shard_handles(S, p, nshards, chunk), shard_handles(S, p, nshards, chunk)
    for sh in b:
        check_map(sh, p.voxel[0], "fresh")
    for k in range(1, 6):
        for sh in a + b:
            integrate(S, sh, R.frames()[k], R.pose(k), 0x3)
        wa = [check_map(sh, p.voxel[0], (k, i)) for i, sh in enumerate(a)]
    for i, sh in enumerate(b):
        assert np.array_equal(check_map(sh, p.voxel[0], ("deferred", i)), wa[i])
    for sh in a + b:
        sh.close()


# --------------------------------------------------- g. a dirty list longer than one pass
def test_dirty_list_longer_than_one_pass(S, oracle):
    """256^3: 8192 quads, of which 4764 hold a crossing voxel (sdf 0.0 with weight 1 goes to f / 2,
    at or above the threshold wherever f >= 2 thr): k_brick_plain's list loop, launched with 4096
    waves, takes its second trip."""
    D = 256
    dims = (D, D, D)
    p = R.make_params(dims, 0x2)
    g = oracle.OGeom.from_params(p)
    fr, E = R.frames()[1], R.pose(1)
    depth = R.fill_holes(fr.depth)
    ost = R.new_ostate(oracle, dims, p.mu, 0x2)
    ost.sdf[:] = 0.0
    ost.wt[:] = 1
    before = ost.sdf.copy()
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(lambda r: R.integrate_frame(oracle, g, p, ost, fr, E, 0x2, depth=depth, x_range=r),
                    [(x, x + 32) for x in range(0, D, 32)]))
    dn, up = R.crossings(before, ost.sdf, R.skip_threshold(p.voxel[0]))
    quads = (dn | up).reshape(D // 8, 8, D // 8, 8, D // 32, 32).any(axis=(1, 3, 5))
    print("quads holding a crossing:", int(quads.sum()), "of", quads.size)
    assert quads.size == 8192 and quads.sum() > 4096
    vol = new_volume(S, p)
    vol.upload(sdf=before, wt=np.ones(before.size, np.int32))
    wa = check_map(vol, p.voxel[0], "seed")
    assert (wa == 0).all()  # sdf 0.0 throughout: nothing skippable
    integrate(S, vol, fr, E, 0x2, depth=depth)
    wa = check_map(vol, p.voxel[0], "frame")
    assert np.count_nonzero(wa) > 0
    out = vol.download(color=False)
    assert np.array_equal(out["sdf"].view(np.uint32), ost.sdf.view(np.uint32)) and np.array_equal(out["wt"], ost.wt)
    vol.close()


# ------------------------------------------------------------- h. update on a caller's stream
def test_update_on_caller_streams(S, oracle):
    """raycast_dev on a caller's stream runs the pending update there; the next integrate (on the
    volume's stream) is ordered after it, and a raycast_dev on a second caller stream updates
    again; map_words() (on the volume's stream) then equals the definition and both images the
    oracle's."""
    import torch

    semtsdf, L = S
    dev = torch.device("cuda", 0)
    p = R.make_params(R.DIMS)
    g = oracle.OGeom.from_params(p)
    ost = R.new_ostate(oracle, R.DIMS, p.mu, 0x3)
    vol = new_volume(S, p)
    check_map(vol, p.voxel[0], "fresh")
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    outs = [torch.zeros(R.W * R.H * 3, dtype=torch.uint8, device=dev) for _ in streams]
    ts = [torch.zeros(R.W * R.H, dtype=torch.float32, device=dev) for _ in streams]
    torch.cuda.synchronize()
    refs = []
    for i, (k, angle) in enumerate(((1, 0.2), (2, math.pi))):
        integrate(S, vol, R.frames()[k], R.pose(k), 0x3)
        R.integrate_frame(oracle, g, p, ost, R.frames()[k], R.pose(k), 0x3)
        s2w, cam = semtsdf.orbit_camera(list(p.Kinv), angle, R.mean_depth() * R.PLACE)
        vol.raycast_dev(s2w, cam, L.RENDER_LABEL, outs[i].data_ptr(), ts[i].data_ptr(), stream=streams[i].cuda_stream)
        refs.append(oracle.render(g, s2w, cam, R.W, R.H, 0, ost.sdf, ost.hist, ost.color))
        streams[i].synchronize()  # the view has read the volume before the next frame changes it
    check_map(vol, p.voxel[0], "after both")
    assert_state(vol, ost, 0x3)
    for i, (img_o, t_o) in enumerate(refs):
        assert (t_o >= 0).mean() > 0.05
        assert np.array_equal(ts[i].cpu().numpy().view(np.uint32), t_o.reshape(-1).view(np.uint32)), i
        assert np.array_equal(outs[i].cpu().numpy(), img_o.reshape(-1)), i
    vol.close()
