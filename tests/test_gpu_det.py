"""libsemtsdf_det.so on the device, exactly: the NMS kernels (through MR.nms_sorted) against the
reference's rule (oracle.non_max_suppression, pinned to mrcnn/utils.py by goldens) or against an
analytic expectation, at every size where the sweep takes another path, at the IoU threshold itself and
on degenerate boxes; the grouped NMS against tests/det_restatement.py's nms_grouped; detections() and
proposals() with the HIP NMS on the inputs of tests/test_det_post.py; and the ROI align (through
MR.roi_align_dev) bit for bit against the f32 restatement of include/semtsdf_det.h in fp16 and bf16."""
import numpy as np
import pytest

import det_restatement as R
import oracle as O

torch = pytest.importorskip("torch")
from semtsdf import maskrcnn as MR  # noqa: E402

pytestmark = pytest.mark.gpu

KB = 64  # boxes per mask word (csrc/semtsdf_det.hip kB)
MR_MAX_BOXES = 16384  # SEMTSDF_DET_MAX_BOXES


def dev():
    return torch.device("cuda", 0)


def run_nms(boxes, thr, max_out, groups=None):
    """-> (kept indices, count, the tail past the count) from MR.nms_sorted."""
    b = torch.from_numpy(np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)).to(dev())
    g = None if groups is None else torch.from_numpy(np.asarray(groups)).to(dev())
    # without groups: the three-argument call the proposals use
    keep, count = MR.nms_sorted(b, float(thr), int(max_out), g) if g is not None else \
        MR.nms_sorted(b, float(thr), int(max_out))
    k, c = keep.cpu().numpy(), int(count.cpu()[0])
    assert k.shape == (max_out,) and k.dtype == np.int32
    return k[:c], c, k[c:]


def assert_nms(boxes, thr, max_out, want, groups=None, what=""):
    want = np.asarray(want)[:max_out]
    got, c, tail = run_nms(boxes, thr, max_out, groups)
    assert c == len(want), (what, len(boxes), thr, max_out, c, len(want))
    np.testing.assert_array_equal(got, want, err_msg=f"{what} n={len(boxes)} thr={thr} max_out={max_out}")
    assert (tail == -1).all(), (what, len(boxes), thr, max_out)


def reference_keep(boxes_sorted, thr):
    n = len(boxes_sorted)
    if n == 0:
        return np.zeros(0, np.int32)
    return O.non_max_suppression(boxes_sorted, -np.arange(n, dtype=np.float64), thr)


# ------------------------------------------------------------------------------------- NMS
# the sweep keeps SEMTSDF_DET_MAX_BOXES / 64 / 64 = 4 accumulator words per lane: word b + 1 + lane + 64 k
# of row block b, so k = 1, 2, 3 are first entered at n = 4097 (65 words + block 0), 8257 and 12353
SIZES = (0, 1, 64, 65, 4096, 4097, 8256, 8257, 12352, 12353, 16384)
ONE_THRESHOLD = {8256: 0.3, 8257: 0.5, 12352: 0.7, 12353: 0.3, 16384: 0.5}


@pytest.mark.parametrize("n", SIZES)
def test_nms_sizes_and_cuts(n):
    """Clustered boxes at every size at which k_nms_sweep takes another accumulator word, the empty
    input and the documented maximum, each with max_out in {n, 1000, 1, 0}: count, kept prefix and the
    -1 tail against the reference rule."""
    rng = np.random.default_rng(100 + n)
    boxes = R.clustered_boxes(rng, n) if n else np.zeros((0, 4), np.float32)
    for thr in ((ONE_THRESHOLD[n],) if n in ONE_THRESHOLD else (0.3, 0.5, 0.7)):
        ref = reference_keep(boxes, thr)
        assert n == 0 or 0 < len(ref) <= n
        for max_out in (n, 1000, 1, 0):
            assert_nms(boxes, thr, max_out, ref, what="sizes")


def grid_boxes(side=128):
    """side^2 pairwise disjoint boxes, box i inside cell i of a side x side grid."""
    rng = np.random.default_rng(5)
    n = side * side
    k = np.arange(n)
    oy, ox, s = (k // side) / side, (k % side) / side, 1.0 / side
    y1, x1 = oy + rng.uniform(0.1, 0.3, n) * s, ox + rng.uniform(0.1, 0.3, n) * s
    h, w = rng.uniform(0.3, 0.6, n) * s, rng.uniform(0.3, 0.6, n) * s
    return np.stack([y1, x1, y1 + h, x1 + w], 1).astype(np.float32)


@pytest.mark.parametrize("source", ["block0", "later_block"])
def test_nms_far_reach(source):
    """16384 disjoint boxes; one box of every word w in 1..255 is overwritten with a copy of an earlier
    kept box (IoU 1): of box w % 64 of block 0, which makes block 0's sweep set a bit through every
    (k, lane) accumulator slot it has and the LDS OR of every word; or of a box of block w // 2, whose
    distance to its copy grows from 1 to 128 words.  Expected analytically: everything but the copies."""
    boxes = grid_boxes()
    n = len(boxes)
    assert n == MR_MAX_BOXES
    w = np.arange(1, n // KB)
    if source == "block0":
        dst, src = KB * w + (7 * w) % KB, w % KB
    else:  # sources on even lanes, copies on odd lanes: no source is itself a copy
        dst, src = KB * w + 2 * (w % 32) + 1, KB * (w // 2) + 2 * (w % 32)
    assert not set(dst) & set(src) and (src < dst).all() and len(set(dst)) == len(dst)
    boxes[dst] = boxes[src]
    want = np.setdiff1d(np.arange(n), dst)
    assert_nms(boxes, 0.5, n, want, what=source)
    assert_nms(boxes, 0.5, 8000, want, what=source)


@pytest.mark.parametrize("thr", [0.3, 0.5, 0.7])
def test_nms_threshold_edge(thr):
    """4096 isolated pairs (n = 8192) whose IoU is one f32 step either side of the threshold, several
    dozen exactly on it: the lower side keeps both boxes (the rule is a strict >), the upper side keeps
    the first.  Both orders inside the pair.  A kernel whose IoU is off in the last bit (a fast
    reciprocal, a contracted multiply-add) fails here."""
    p = R.near_threshold_pairs(thr, 4096, np.random.default_rng(int(thr * 10)), 64)
    assert (p["steps"] == 1).all()
    assert (p["iou_lo"] <= np.float32(thr)).all() and (p["iou_hi"] > np.float32(thr)).all()
    assert (p["iou_lo"] == np.float32(thr)).sum() > 0
    n = 2 * 4096
    for order in ("a first", "b first"):
        for side in ("lo", "hi", "mixed"):
            upper = {"lo": np.zeros(4096, bool), "hi": np.ones(4096, bool), "mixed": np.arange(4096) % 3 == 0}[side]
            b = np.where(upper[:, None], p["b_hi"], p["b_lo"])
            boxes = np.zeros((n, 4), np.float32)
            boxes[0::2], boxes[1::2] = (p["a"], b) if order == "a first" else (b, p["a"])
            want = np.sort(np.concatenate([np.arange(0, n, 2), 1 + 2 * np.nonzero(~upper)[0]]))
            assert_nms(boxes, thr, n, want, what=f"edge {side}, {order}")


def test_nms_exact_half():
    """A = s (0, 0, 1, 1) and B = s (0, 0, 1, 0.5), s a power of two: IoU is exactly 0.5 in f32.  Both
    are kept at 0.5; at the f32 just below 0.5 the second is suppressed."""
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    for s in (2.0 ** -8, 0.125, 1.0, 4.0, 1024.0):
        a, b = np.array([0, 0, s, s], np.float32), np.array([0, 0, s, 0.5 * s], np.float32)
        for pair in ((a, b), (b, a)):
            boxes = np.stack(pair)
            assert_nms(boxes, 0.5, 2, [0, 1], what=f"half s={s}")
            assert_nms(boxes, below, 2, [0], what=f"below half s={s}")


def degenerate_boxes():
    rng = np.random.default_rng(8)
    b = R.clustered_boxes(rng, 700)
    kind = np.zeros(700, np.int64)
    ix = rng.permutation(700)
    z, dz, inv, dup, touch = ix[:60], ix[60:90], ix[90:150], ix[150:200], ix[200:240]
    b[z[:20], 2] = b[z[:20], 0]            # zero height
    b[z[20:40], 3] = b[z[20:40], 1]        # zero width
    b[z[40:], 2:] = b[z[40:], :2]          # a point
    b[z[50:]] = 0.0                        # the zero rows proposals() pads with
    b[dz] = b[z[rng.integers(0, 60, 30)]]  # exact duplicates of zero-area boxes
    kind[z], kind[dz] = 1, 1
    b[inv[:20]] = b[inv[:20]][:, [2, 1, 0, 3]]
    b[inv[20:40]] = b[inv[20:40]][:, [0, 3, 2, 1]]
    b[inv[40:]] = b[inv[40:]][:, [2, 3, 0, 1]]
    kind[inv] = 2
    src = ix[240:290]
    b[dup] = b[src]                        # identical full boxes
    kind[dup] = 3
    tsrc = ix[290:330]                     # touching along an edge: b.y1 == a.y2, the same x extent
    b[touch, 0] = b[tsrc, 2]
    b[touch, 2] = b[tsrc, 2] + (b[tsrc, 2] - b[tsrc, 0])
    b[touch, 1], b[touch, 3] = b[tsrc, 1], b[tsrc, 3]
    return b, kind, dup, src


@pytest.mark.parametrize("thr", [0.3, 0.5, 0.7])
def test_nms_degenerate_boxes(thr):
    """Zero-area boxes (and exact duplicates of them: IoU 0/0, which suppresses nothing), inverted
    extents, identical full boxes (IoU 1) and boxes touching along an edge (IoU 0) among ordinary
    clustered boxes: the reference rule, and what follows from it for the zero-area boxes and the
    duplicates."""
    b, kind, dup, src = degenerate_boxes()
    ref = reference_keep(b, thr)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert set(np.nonzero((kind == 1) & (area == 0))[0]) <= set(ref.tolist())  # every zero-area box is kept
    assert (area[kind == 1] == 0).all() and (area < 0).any()
    first, second = np.minimum(dup, src), np.maximum(dup, src)
    assert not (np.isin(first, ref) & np.isin(second, ref) & (area[first] > 0)).any()  # never both of a duplicate pair
    for max_out in (len(b), 100):
        assert_nms(b, thr, max_out, ref, what="degenerate")


@pytest.mark.parametrize("n", [65, 4097, 16384])
def test_nms_grouped(n):
    """semtsdf_det_nms_grouped against nms_grouped (greedy in order, suppression inside a group only):
    clustered boxes with random groups in 0..80."""
    rng = np.random.default_rng(200 + n)
    boxes = R.clustered_boxes(rng, n)
    groups = rng.integers(0, 81, n).astype(np.int32)
    for thr in ((0.3, 0.7) if n < 16384 else (0.3,)):
        want = R.nms_grouped(boxes, groups, thr, n)
        plain = reference_keep(boxes, thr)
        assert len(want) > len(plain) or (n == 65 and thr == 0.7)  # the groups matter on this input
        for max_out in (n, 100):
            assert_nms(boxes, thr, max_out, want, groups=groups, what="grouped")
        # one group, whatever its id, and no groups at all: the ungrouped rule
        assert_nms(boxes, thr, n, plain, groups=np.full(n, 80, np.int32), what="one group")
        assert_nms(boxes, thr, n, plain, groups=None, what="no groups")
    assert_nms(boxes, 0.3, n, R.nms_grouped(boxes, groups.astype(np.int64) - 40, 0.3, n),
               groups=groups.astype(np.int64) - 40, what="int64 and negative groups")


def test_nms_grouped_threshold_edge():
    """The isolated near-threshold pairs with every box in group 80 decide as the ungrouped rule; with
    the two boxes of a pair in different groups nothing is suppressed."""
    thr = 0.3
    p = R.near_threshold_pairs(thr, 4096, np.random.default_rng(31), 64)
    assert (p["steps"] == 1).all()
    n = 2 * 4096
    upper = np.arange(4096) % 2 == 1
    boxes = np.zeros((n, 4), np.float32)
    boxes[0::2] = p["a"]
    boxes[1::2] = np.where(upper[:, None], p["b_hi"], p["b_lo"])
    want = np.sort(np.concatenate([np.arange(0, n, 2), 1 + 2 * np.nonzero(~upper)[0]]))
    assert_nms(boxes, thr, n, want, groups=np.full(n, 80, np.int32), what="group 80")
    np.testing.assert_array_equal(R.nms_grouped(boxes, np.full(n, 80), thr, n), want)
    assert_nms(boxes, thr, n, np.arange(n), groups=(np.arange(n) % 2).astype(np.int32), what="two groups")


# ------------------------------------------------------ detections() and proposals(), HIP NMS
@pytest.fixture(scope="module")
def model():
    # the box stages use no weights: the module stays on the CPU, its constants are made on the device
    return MR.MaskRCNN(MR.Config(DTYPE=torch.float32, BACKBONE="resnet50"), seed=0).eval()


def test_detections_equal_refine_detections_graph_on_device(model):
    R.check_detection_case(model, dev())


def test_detections_decide_pairs_at_the_threshold_on_device(model):
    R.check_pair_case(model, dev())


def test_proposals_equal_proposal_layer_on_device(model):
    R.check_proposal_case(model, dev())


def test_unmold_boxes_round_the_f64_product_on_device(model):
    """tests/test_det_post.py's half-pixel boxes through unmold() on the device."""
    boxes = R.half_pixel_boxes((480, 640))
    R.check_unmold_boxes(model, boxes, R.denorm_boxes(boxes, (480, 640)), dev())


# ------------------------------------------------------------------------------- ROI align
TORCH_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def run_roi_align(feats, rois, lvl, pool, dtype):
    """feats [C, H, W] f32 arrays holding values of `dtype` -> MR.roi_align_dev's output widened to f32."""
    fs = [torch.from_numpy(f)[None].to(dev(), TORCH_DT[dtype]) for f in feats]
    for f, t in zip(feats, fs):
        assert np.array_equal(t[0].float().cpu().numpy(), f)  # the maps hold exactly these values
    out = MR.roi_align_dev(torch.from_numpy(rois).to(dev()), torch.from_numpy(lvl).to(dev()), fs, pool)
    assert out.dtype == TORCH_DT[dtype] and tuple(out.shape) == (len(rois), feats[0].shape[0], pool, pool)
    return out.float().cpu().numpy()


def assert_bits_equal(got, want, what):
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} of {g.size} elements differ, first at {bad[0]}: " \
                              f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("pool", [2, 7, 14])
def test_roi_align_bits(dtype, pool):
    """Non-square maps (24, 40), (12, 20), (6, 10), (3, 5) with 5 channels, rois inside, straddling
    each border, outside, zero, clipped to exactly 0.0 and 1.0 on each side, flat and inverted, the four
    levels interleaved along n: every output element bit-equal to roi_align_f32."""
    feats, rois, lvl = R.roi_inputs(dtype)
    assert set(lvl.tolist()) == {2, 3, 4, 5}
    want = R.roi_align_f32(feats, rois, lvl, pool, dtype)
    assert (want != 0).sum() > want.size // 4
    assert_bits_equal(run_roi_align(feats, rois, lvl, pool, dtype), want, f"{dtype} pool {pool}")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_roi_align_second_trip_of_the_grid_stride_loop(dtype):
    """The launch is min(ceil(total / 256), 8192) blocks of 256 threads: 2200 rois x 5 channels x 14 x 14
    = 2,156,000 elements exceed its 2,097,152 threads, so the last elements are a thread's second trip
    (production: 12.5 M elements, always several trips)."""
    feats, base, _ = R.roi_inputs(dtype)
    rng = np.random.default_rng(9)
    n, pool = 2200, 14
    assert n * R.ROI_C * pool * pool > 8192 * 256
    rois = base[rng.integers(0, len(base), n)]
    some = rng.integers(0, n, n // 2)
    rois[some] = (rois[some] + rng.normal(0, 0.01, (len(some), 4))).astype(np.float32)
    lvl = rng.integers(2, 6, n).astype(np.int32)
    want = R.roi_align_f32(feats, rois, lvl, pool, dtype)
    got = run_roi_align(feats, rois, lvl, pool, dtype)
    first = 8192 * 256 // (R.ROI_C * pool * pool)  # the roi the second trip starts in
    assert (want[first + 1:] != 0).any()
    assert_bits_equal(got, want, f"{dtype} second trip")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("pool", [2, 7, 14])
def test_roi_align_identity(dtype, pool):
    """roi (0, 0, 1, 1) on a level with H = pool and W = 2 pool - 1: the steps are exactly 1 and 2, the
    samples fall on map elements, the output is feat[:, :, ::2] whatever the restatement says.  An H / W
    mix-up in the indexing cannot pass."""
    rng = np.random.default_rng(pool)
    for level in (2, 3, 4, 5):
        feats = [R.round_to(rng.normal(0, 1, (3, 4, 6)).astype(np.float32), dtype) for _ in range(4)]
        feats[level - 2] = R.round_to(rng.normal(0, 1, (3, pool, 2 * pool - 1)).astype(np.float32), dtype)
        rois = np.array([[0, 0, 1, 1]], np.float32)
        got = run_roi_align(feats, rois, np.array([level], np.int32), pool, dtype)
        assert_bits_equal(got[0], np.ascontiguousarray(feats[level - 2][:, :, ::2]), f"identity level {level}")


def test_roi_align_no_rois():
    feats, _, _ = R.roi_inputs("fp16")
    out = run_roi_align(feats, np.zeros((0, 4), np.float32), np.zeros(0, np.int32), 7, "fp16")
    assert out.shape == (0, R.ROI_C, 7, 7)
    torch.cuda.synchronize()
