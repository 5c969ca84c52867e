"""semtsdf_detections_to_labels on the device (pixel boxes + mini-masks -> the u8 label map, the
[H][W][N] masks never made) against the NumPy restatement of its rule (tests/paste_restatement.py), bit
for bit unless a test says otherwise: the reference-made golden, box and image shapes at every edge of
the rule, the order of the arithmetic, the three input types, the keep/rank/label edges and the argument
checks; then the Python producer (MaskRCNN.labels_from, detect_labels, GraphDetector in label mode)
against the existing unmold + semtsdf_masks_to_labels path outside the restatement's `near` band."""
import numpy as np
import pytest

import paste_restatement as PR

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SHAPES = ((7, 13), (33, 65), (96, 128))


def smooth(rng, n, mh=28, mw=28):
    """Smooth sigmoid mini-masks [n, mh, mw] f32 (low-frequency waves through a sigmoid)."""
    yy, xx = np.mgrid[0:mh, 0:mw]
    yy, xx = (yy + 0.5) / mh, (xx + 0.5) / mw
    out = np.empty((n, mh, mw), np.float32)
    for i in range(n):
        f = np.full((mh, mw), rng.uniform(0.0, 2.0))
        for _ in range(3):
            f += rng.normal(0, 1.5) * np.cos(2 * np.pi * (rng.uniform(0, 1.5) * yy + rng.uniform(0, 1.5) * xx)
                                             + rng.uniform(0, 2 * np.pi))
        out[i] = 1.0 / (1.0 + np.exp(-f))
    return out


def edge_boxes(H, W):
    return np.array([
        [0, 0, H, W],                                          # the whole image
        [2, 3, 3, 4], [1, 0, 2, W], [0, 2, H, 3],              # 1 x 1, 1 x w, h x 1
        [1, 2, 29, 30],                                        # 28 x 28: the identity, fy = fx = 0
        [2, 1, 29, 28], [0, 3, 29, 32],                        # 27 and 29 on a side
        [3, 2, 16, 11],                                        # smaller than the mini-mask
        [-5, 2, H // 2, W - 2], [H // 2, 2, H + 6, W - 3],     # over the top, the bottom,
        [1, -7, H - 1, W // 2], [1, W // 2, H - 1, W + 9],     # the left and the right side
        [-3, -4, H + 5, W + 2],                                # over all four
        [H + 1, 0, H + 9, 8], [-9, -9, 0, 0], [0, W, 5, W + 5],  # fully outside
        [3, 3, 3, 8], [3, 3, 8, 3], [5, 5, 2, 9], [5, 9, 8, 2],  # zero and negative extent
    ], np.int32)


def run(boxes, minis, shape, min_area=2000, dtype=None):
    from semtsdf.masks import detections_to_labels

    return detections_to_labels(boxes, minis, shape, min_area, dtype)


def check(oracle, boxes, minis, shape, min_area, tag, dev_minis=None, dtype=None):
    """Device == restatement: labels, kept count and areas.  dev_minis/dtype: what the device is handed
    when that is not the f32 array the restatement reads (fp16, bf16 bits)."""
    want, wk, wa = PR.detections_to_labels(oracle, boxes, minis, shape, min_area)
    got, k, areas = run(boxes, minis if dev_minis is None else dev_minis, shape, min_area, dtype)
    assert got.shape == tuple(shape) and got.dtype == np.uint8
    np.testing.assert_array_equal(areas, wa, err_msg=f"{tag}: areas")
    assert k == wk, tag
    np.testing.assert_array_equal(got, want, err_msg=f"{tag}: labels")
    return got, k, areas


def to_bf16_bits(a):
    """f32 -> bf16 bit patterns (round to nearest even), and the f32 values they stand for."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return b, (b.astype(np.uint32) << 16).view(np.float32)


# ------------------------------------------------------------------------------------ golden
def test_golden_cases_on_device():
    def single(box, mini, shape):
        lab, kept, areas = run(box[None], mini[None], shape, min_area=-1)
        assert kept == 1 and int(areas[0]) == int((lab == 1).sum())
        return lab == 1

    PR.check_golden(single, lambda b, m, s: run(b, m, s)[:2])


# ------------------------------------------------------------------------- shapes and boxes
@pytest.mark.parametrize("shape", SHAPES)
def test_box_and_image_shapes(oracle, shape):
    rng = np.random.default_rng(shape[0])
    boxes = edge_boxes(*shape)
    minis = smooth(rng, len(boxes))
    for i in range(len(boxes)):  # each box alone: every pixel of its own paste
        check(oracle, boxes[i:i + 1], minis[i:i + 1], shape, -1, f"{shape} box {boxes[i].tolist()}")
    check(oracle, boxes, minis, shape, -1, f"{shape} all boxes")  # together: the ranks among them
    check(oracle, boxes, minis, shape, 12, f"{shape} all boxes, min_area 12")


@pytest.mark.parametrize("shape", SHAPES)
def test_non_square_mini_mask_in_a_non_square_box(oracle, shape):
    H, W = shape
    rng = np.random.default_rng(9)
    boxes = np.array([[1, 2, H - 1, W - 3], [0, 0, H, W], [-2, 3, H // 2, W + 4], [2, 1, 16, 21], [0, 0, 20, 14]],
                     np.int32)
    minis = smooth(rng, len(boxes), 14, 20)
    minis[1, 3, :] = 1.0  # one bright row: swapped axes would paint a column
    minis[1, :3, :] = 0.0
    minis[1, 4:, :] = 0.0
    for i in range(len(boxes)):
        check(oracle, boxes[i:i + 1], minis[i:i + 1], shape, -1, f"{shape} 14x20 box {boxes[i].tolist()}")
    check(oracle, boxes, minis, shape, -1, f"{shape} 14x20 all")
    check(oracle, boxes[:2], smooth(rng, 2, 64, 1), shape, -1, f"{shape} 64x1")
    check(oracle, boxes[:2], smooth(rng, 2, 1, 64), shape, -1, f"{shape} 1x64")
    check(oracle, boxes[:3], smooth(rng, 3, 64, 64), shape, -1, f"{shape} 64x64")


# ------------------------------------------------------------------------- arithmetic order
def test_constant_half_mask_follows_the_written_lerp(oracle):
    """A constant 0.5 mini-mask sits on the threshold, so every rounding of v = top (1 - fy) + bot fy
    decides a pixel: another order of the operations (a fused multiply-add, a lerp written a + f (b - a))
    can give another map.  The expectation is the restatement's, not an analysis; it has pixels of both
    kinds (the rim, blended with the zero outside, is off)."""
    shape = (96, 128)
    boxes = np.array([[3, 5, 30, 32], [40, 2, 69, 31], [2, 40, 62, 120], [70, 60, 83, 69], [66, 80, 94, 127]],
                     np.int32)
    minis = np.full((len(boxes), 28, 28), 0.5, np.float32)
    for i in range(len(boxes)):
        check(oracle, boxes[i:i + 1], minis[i:i + 1], shape, -1, f"half {boxes[i].tolist()}")
    m = PR.paste_mask(minis[2], boxes[2], shape)[2:62, 40:120]
    assert m.any() and not m.all()
    # elements a few f32 steps either side of 0.5: the interior is decided by the last bit of v
    rng = np.random.default_rng(14)
    steps = rng.integers(-3, 4, minis.shape).astype(np.float32) * np.float32(2.0 ** -24)
    minis = (minis + steps).astype(np.float32)
    for i in range(len(boxes)):
        check(oracle, boxes[i:i + 1], minis[i:i + 1], shape, -1, f"half +- steps {boxes[i].tolist()}")
    m = PR.paste_mask(minis[2], boxes[2], shape)[6:58, 46:114]
    assert m.any() and not m.all()


def test_nan_and_infinite_elements(oracle):
    shape = (33, 65)
    rng = np.random.default_rng(4)
    boxes = np.array([[0, 0, 33, 65], [2, 3, 30, 31], [1, 30, 28, 64], [5, 5, 18, 14]], np.int32)
    minis = smooth(rng, len(boxes))
    for i, bad in enumerate((np.nan, np.inf, -np.inf, np.nan)):
        at = rng.integers(0, 28, (6, 2))
        minis[i, at[:, 0], at[:, 1]] = bad
    minis[3, 0, :] = np.inf  # the rim: inf times the zero weight of an outside tap's partner
    for i in range(len(boxes)):
        check(oracle, boxes[i:i + 1], minis[i:i + 1], shape, -1, f"non-finite {i}")
    check(oracle, boxes, minis, shape, -1, "non-finite all")


# ------------------------------------------------------------------------------------ dtype
def test_fp16_bf16_and_f32_inputs(oracle):
    shape = (33, 65)
    rng = np.random.default_rng(6)
    boxes = np.array([[0, 0, 33, 65], [2, 3, 31, 60], [-3, 20, 20, 70], [4, 4, 17, 13]], np.int32)
    v = smooth(rng, len(boxes))
    h = v.astype(np.float16)
    bits, b = to_bf16_bits(v)
    assert not np.array_equal(h.astype(np.float32), v) and not np.array_equal(b, v)
    check(oracle, boxes, v, shape, -1, "f32")
    check(oracle, boxes, h.astype(np.float32), shape, -1, "fp16", dev_minis=h)
    check(oracle, boxes, b, shape, -1, "bf16", dev_minis=bits, dtype=1)


# ------------------------------------------------------------------------------- rule edges
def test_equal_areas_go_to_the_lower_index(oracle):
    shape = (96, 128)
    mini = (np.float32(0.45) + np.float32(0.5) * smooth(np.random.default_rng(8), 1)[0]).astype(np.float32)  # mostly on
    boxes = np.array([[10, 10, 60, 70], [30, 40, 80, 100], [20, 25, 70, 85]], np.int32)  # one size, overlapping
    minis = np.stack([mini] * 3)
    lab, kept, areas = check(oracle, boxes, minis, shape, 0, "ties")
    assert kept == 3 and areas[0] == areas[1] == areas[2] > 0
    m = PR.paste_masks(boxes, minis, shape)
    both = m[:, :, 0] & m[:, :, 1] & m[:, :, 2]
    assert both.any() and (lab[both] == 1).all()
    assert (lab[m[:, :, 1] & m[:, :, 2] & ~m[:, :, 0]] == 2).all()


def test_min_area_boundary(oracle):
    shape = (96, 128)
    rng = np.random.default_rng(10)
    boxes = np.array([[5, 5, 70, 90], [20, 30, 60, 80]], np.int32)
    minis = smooth(rng, 2)
    A = int(PR.paste_masks(boxes, minis, shape)[:, :, 1].sum())
    assert 0 < A < int(PR.paste_masks(boxes, minis, shape)[:, :, 0].sum())
    kept = [check(oracle, boxes, minis, shape, a, f"min_area {a}")[1] for a in (A - 1, A, 10 ** 6, -1)]
    assert kept == [2, 1, 0, 2]


@pytest.mark.parametrize("n", [0, 1, 255, 256])
def test_detection_counts(oracle, n):
    shape = (33, 65)
    rng = np.random.default_rng(n)
    y, x = rng.integers(-4, 30, n), rng.integers(-4, 60, n)
    boxes = np.stack([y, x, y + rng.integers(0, 14, n), x + rng.integers(0, 18, n)], 1).astype(np.int32)
    lab, kept, _ = check(oracle, boxes, smooth(rng, n), shape, 0, f"n {n}")
    if n == 0:
        assert kept == 0 and not lab.any()


def test_argument_errors_are_refused():
    from semtsdf import _lib as L

    b = np.zeros((257, 4), np.int32)
    with pytest.raises(L.SemTSDFError):
        run(b, np.zeros((257, 28, 28), np.float32), (8, 8))
    with pytest.raises(L.SemTSDFError):
        run(b[:1], np.zeros((1, 65, 28), np.float32), (8, 8))
    with pytest.raises(L.SemTSDFError):
        run(b[:1], np.zeros((1, 28, 65), np.float32), (8, 8))
    with pytest.raises(L.SemTSDFError):
        run(b[:1], np.zeros((1, 28, 28), np.float32), (8, 8), dtype=3)
    lab, kept, _ = run(b[:1], np.ones((1, 28, 28), np.float32), (8, 8))  # the library still works afterwards
    assert kept == 0 and not lab.any()


# --------------------------------------------------------- agreement with the existing path
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model():
    from semtsdf import maskrcnn as MR

    return MR.MaskRCNN(MR.Config(DTYPE=torch.float32, BACKBONE="resnet50", NUM_CLASSES=6), seed=0).eval()


SHAPE = (120, 160)
NWIN = np.array([0.0, 0.0, 1.0, 1.0], np.float32)


def fixed_rows(seed=12, n=14):
    """Random fixed-row detector outputs, no network: det [n, 6] (normalised boxes of well separated
    sizes, class, score), rows of class 0, all-zero rows and a zero-area row among them, and smooth
    masks [n, 6, 28, 28]."""
    rng = np.random.default_rng(seed)
    det = np.zeros((n, 6), np.float32)
    side = np.linspace(0.15, 0.95, n)
    for i in range(n):
        h, w = side[i], side[(i * 7) % n]
        y, x = rng.uniform(0, 1 - h), rng.uniform(0, 1 - w)
        det[i] = [y, x, y + h, x + w, rng.integers(1, 6), 0.99 - 0.01 * i]
    det[3, 4] = 0          # a class-0 row
    det[9] = 0             # zero rows (tf.pad)
    det[13] = 0
    det[6, 2] = det[6, 0] - 1.0 / (SHAPE[0] - 1)  # zero pixel area: unmold_detections drops it
    masks = smooth(rng, n * 6).reshape(n, 6, 28, 28)
    return torch.from_numpy(det).to(dev()), torch.from_numpy(masks).to(dev())


def both_paths(model, oracle, det, masks, shape, nwin, min_area):
    """labels_from against the restatement bit for bit, and against unmold + masks_to_labels: the old
    path's masks equal the rule's outside each detection's `near` band, and where that leaves keep and
    rank alone the two label maps are equal outside the band."""
    from semtsdf.masks import masks_to_labels

    with torch.no_grad():
        new = model.labels_from(det, masks.float(), shape, (256, 256), nwin, min_area=min_area)
        old = model.unmold(det, masks.float(), shape, (256, 256), nwin, compact=False)
    torch.cuda.synchronize()
    for k in ("rois", "class_ids", "scores"):
        assert torch.equal(new[k], old[k]), k
    boxes = new["rois"].cpu().numpy()
    cls = new["class_ids"].cpu().numpy().astype(np.int64)
    minis = masks.float().cpu().numpy()[np.arange(len(cls)), cls]
    want, wk, wa = PR.detections_to_labels(oracle, boxes, minis, shape, min_area)
    lab = new["labels"].cpu().numpy()
    assert lab.shape == tuple(shape) and lab.dtype == np.uint8
    np.testing.assert_array_equal(new["areas"].cpu().numpy().view(np.uint32), wa)
    np.testing.assert_array_equal(lab, want)
    assert (wa[cls == 0] == 0).all()
    # the existing path
    om = old["masks"].cpu().numpy().astype(bool)
    rule = PR.paste_masks(boxes, minis, shape)
    near = np.zeros(shape, bool)
    for i in range(len(boxes)):
        ni = PR.near_map(boxes[i:i + 1], minis[i:i + 1], shape)
        assert not (om[:, :, i] != rule[:, :, i])[~ni].any(), i
        near |= ni
    old_lab, old_kept = masks_to_labels(om, min_area)
    oa = om.sum(axis=(0, 1))
    key = lambda a: [(int(v), i) for i, v in enumerate(a) if v > min_area]  # noqa: E731
    same_order = [i for _, i in sorted(key(oa))] == [i for _, i in sorted(key(wa))]
    print(f"kept {wk} (existing path {old_kept}), near pixels {int(near.sum())}, same keep and rank: {same_order}")
    if same_order:
        assert old_kept == wk
        assert not (old_lab != lab)[~near].any()
    return wk, int(near.sum()), same_order, wa


def test_labels_from_agrees_with_unmold_and_masks_to_labels(model, oracle):
    det, masks = fixed_rows()
    kept, near, same_order, areas = both_paths(model, oracle, det, masks, SHAPE, NWIN, 300)
    # the case's areas are well apart, so the comparison of the two label maps did take place
    a = np.sort(areas[areas > 0].astype(np.int64))
    assert np.diff(a).min() > near and np.abs(a - 300).min() > near
    assert same_order and 3 <= kept < (areas > 0).sum() and near <= 1e-3 * PR.box_pixels(
        model.unmold_boxes(det, SHAPE, NWIN)[0].cpu().numpy(), SHAPE)


def test_labels_from_is_deterministic_and_capturable(model):
    det, masks = fixed_rows(seed=13)
    from semtsdf.masks import detections_to_labels_workspace

    work = torch.empty(detections_to_labels_workspace(det.shape[0]), dtype=torch.uint8, device=dev())
    a = model.labels_from(det, masks, SHAPE, (256, 256), NWIN, min_area=300)
    b = model.labels_from(det, masks, SHAPE, (256, 256), NWIN, min_area=300, work=work)
    torch.cuda.synchronize()
    assert int(a["labels"].max()) >= 3
    for k in a:
        assert torch.equal(a[k], b[k]), k
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(side):
        model.labels_from(det, masks, SHAPE, (256, 256), NWIN, min_area=300, work=work)
    torch.cuda.current_stream(dev()).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model.labels_from(det, masks, SHAPE, (256, 256), NWIN, min_area=300, work=work)
    for _ in range(2):
        out["labels"].zero_()
        out["areas"].zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], out[k]), k


# --------------------------------------------------------------------------------- detector
def test_detector_label_mode_small_configuration(oracle):
    """The 192/256 configuration of tests/test_maskrcnn.py: one run of the network, its (det, masks) into
    both paste paths; then GraphDetector(labels=True) replays a label map that keeps the contract.  (Two
    separate runs of the network are not compared: the detector is not reproducible call to call.)"""
    from semtsdf import maskrcnn as MR

    cfg = MR.Config(IMAGE_MIN_DIM=192, IMAGE_MAX_DIM=256, PRE_NMS_LIMIT=1000, POST_NMS_ROIS_INFERENCE=200,
                    DTYPE=torch.float32, BACKBONE="resnet50")
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (120, 160, 3), dtype=np.uint8)).to(dev())
    m = MR.MaskRCNN(cfg, seed=0).to(dev()).eval()
    m.calibrate(dev(), img)
    with torch.no_grad():
        det, masks, shape, nwin = m._network(img)
    assert int((det[:, 4] > 0).sum()) > 0
    both_paths(m, oracle, det, masks, (120, 160), nwin, 50)
    g = MR.GraphDetector(m, img.shape, dev(), labels=True)
    for _ in range(2):
        out = g(img)
        torch.cuda.synchronize()
        lab, areas, cls = out["labels"].cpu().numpy(), out["areas"].cpu().numpy(), out["class_ids"].cpu().numpy()
        assert lab.shape == (120, 160) and lab.dtype == np.uint8
        assert tuple(out["rois"].shape) == (cfg.DETECTION_MAX_INSTANCES, 4)
        assert int(lab.max()) <= int((areas > 2000).sum())
        assert (areas[cls == 0] == 0).all() and (areas >= 0).all()
