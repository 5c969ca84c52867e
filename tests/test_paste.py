"""The mask paste rule of semtsdf_detections_to_labels (include/semtsdf.h) on the CPU: its NumPy
restatement (tests/paste_restatement.py) against tests/golden/paste_golden.npz, which
tests/golden/gen_paste.py made by executing the reference's own unmold_mask (scikit-image resize) and
dmask.py mask_detect.  Masks and labels are equal outside the golden's `near` map (pixels whose f64
interpolated value lies within 1e-4 of 0.5, where skimage's f32 rounding may decide the threshold the
other way); the map covers at most 0.1 % of a case's box pixels, and the recorded skimage-vs-f64
deviation stays below 1e-5, a tenth of the band.  tests/test_gpu_paste.py holds the device to the
restatement bit for bit."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import paste_restatement as PR
from paste_restatement import golden

DEV_CAP = 1e-5    # recorded |skimage - f64 restatement|; the band is 1e-4


def test_restatement_equals_the_reference_outside_the_band(oracle):
    PR.check_golden(lambda b, m, s: PR.paste_mask(m, b, s),
                    lambda b, m, s: PR.detections_to_labels(oracle, b, m, s)[:2])


def test_golden_cases_cover_the_rule():
    singles, labels, _, band = golden()
    assert band == 1e-4
    sizes = {(int(b[2] - b[0]), int(b[3] - b[1])) for b, *_ in singles}
    assert (28, 28) in sizes and any(h == 1 for h, _ in sizes) and any(w == 1 for _, w in sizes)
    assert any(h > 28 and w > 28 for h, w in sizes) and any(h < 28 and w < 28 for h, w in sizes)
    assert {m.shape for _, m, *_ in singles} >= {(28, 28), (14, 20)}  # one non-square mini-mask size
    assert [s for _, _, s, *_ in labels] == [(96, 128), (480, 640)]
    for boxes, minis, shape, lab, kept, near in labels:
        assert 0 < kept < len(boxes) and int(lab.max()) == kept
        # areas apart from one another and from the 2000-pixel rule by more than the band's pixels
        areas = np.sort(PR.paste_masks(boxes, minis, shape).sum(axis=(0, 1)).astype(np.int64))
        k = int(near.sum())
        assert np.abs(areas - 2000).min() > k and np.diff(areas[areas > 2000]).min() > k
    # the near map is the restatement's own f64 band
    boxes, minis, shape, _, _, near = labels[0]
    np.testing.assert_array_equal(PR.near_map(boxes, minis, shape, band), near)


def test_recorded_skimage_deviation_leaves_the_band_its_margin():
    dev = golden()[2]
    print(f"recorded |skimage - f64 restatement| max: {dev:.3g}")
    assert 0.0 < dev <= DEV_CAP


def test_f32_rule_differs_from_f64_only_inside_the_band():
    """The rule's own f32 rounding against the f64 values: the thresholded masks agree outside the band."""
    for box, mini, shape, _, near in golden()[0]:
        a, b = PR.paste_mask(mini, box, shape), PR.paste_mask(mini, box, shape, np.float64)
        assert not (a != b)[~near].any()


def test_restatement_clips_boxes_and_keeps_axes_apart():
    rng = np.random.default_rng(5)
    mini = rng.random((14, 20)).astype(np.float32)
    shape = (33, 65)
    whole = PR.paste_mask(mini, [-5, -9, 40, 70], (60, 90))  # the same box, shifted inside a larger image
    inside = PR.paste_mask(mini, [0, 0, 45, 79], (60, 90))
    np.testing.assert_array_equal(PR.paste_mask(mini, [-5, -9, 40, 70], shape), inside[5:38, 9:74])
    np.testing.assert_array_equal(whole[:40, :70], inside[5:45, 9:79])
    for box in ([3, 3, 3, 9], [3, 3, 9, 3], [9, 9, 3, 3], [-9, 0, 0, 9], [33, 0, 40, 9], [0, 65, 9, 70]):
        assert not PR.paste_mask(mini, box, shape).any(), box
    # a mini-mask with one bright row pastes as rows, not columns
    bar = np.zeros((14, 20), np.float32)
    bar[3] = 1.0
    m = PR.paste_mask(bar, [0, 0, 28, 40], shape)
    assert m[6:8, :40].all() and not m[:5].any() and not m[9:].any()


def test_shared_box_helper_equals_reference_denorm_boxes():
    """MaskRCNN.unmold_boxes, the box arithmetic unmold() and labels_from() share, against utils.py:875-889
    denorm_boxes as the reference executed it (denorm_480_640 of mrcnn_utils_golden.npz): window
    (0, 0, 1, 1), a 480 x 640 image, the golden's boxes as detections of class 1, a few of class 0."""
    torch = pytest.importorskip("torch")
    from semtsdf import maskrcnn as MR

    G = np.load(os.path.join(GOLDEN, "mrcnn_utils_golden.npz"))
    boxes = np.clip(G["delta_boxes"], 0, 1).astype(np.float32)
    want = G["denorm_480_640"]
    n = len(boxes)
    cls = np.ones((n, 1), np.float32)
    cls[::7] = 0
    det = torch.from_numpy(np.concatenate([boxes, cls, np.full((n, 1), 0.9, np.float32)], 1))
    m = MR.MaskRCNN(MR.Config(DTYPE=torch.float32, BACKBONE="resnet50"), seed=0)
    px, c, ok = m.unmold_boxes(det, (480, 640), np.array([0.0, 0.0, 1.0, 1.0], np.float32))
    assert px.dtype == torch.int32
    np.testing.assert_array_equal(px.numpy(), want)
    np.testing.assert_array_equal(c.numpy(), cls[:, 0].astype(np.int64))
    area = (want[:, 2] - want[:, 0]) * (want[:, 3] - want[:, 1])
    np.testing.assert_array_equal(ok.numpy(), (area > 0) & (cls[:, 0] > 0))
    assert ok.sum() > 100 and (~ok).sum() > 100


def test_argument_errors_without_a_device():
    """semtsdf_detections_to_labels refuses bad arguments with a message before any device work (the
    pointers here are made up)."""
    import ctypes as C

    from semtsdf import _lib as L

    lib = L.load()
    buf = C.c_void_p(0x1000)
    assert lib.semtsdf_detections_to_labels_workspace(100) >= 256 * 7 + 4

    def call(boxes=buf, mini=buf, dtype=2, mh=28, mw=28, n=100, w=640, h=480, labels=buf, work=buf):
        return lib.semtsdf_detections_to_labels(boxes, mini, dtype, mh, mw, n, w, h, 2000, labels, None, work, None,
                                                None)

    for kw, word in (({"labels": None}, b"labels"), ({"work": None}, b"workspace"), ({"boxes": None}, b"NULL"),
                     ({"mini": None}, b"NULL"), ({"dtype": 3}, b"dtype"), ({"dtype": -1}, b"dtype"),
                     ({"mh": 65}, b"mini-mask"), ({"mw": 0}, b"mini-mask"), ({"n": 257}, b"n=257"),
                     ({"n": -1}, b"n=-1"), ({"w": 0}, b"size"), ({"w": 1 << 15, "h": 1 << 14}, b"size")):
        assert call(**kw) == L.ERR_INVALID and word in lib.semtsdf_last_error(), kw
