"""The detector's box post-processing on the CPU against restatements of the reference's rules
(tests/det_restatement.py, from mrcnn/model.py and mrcnn/utils.py by line): MaskRCNN.detections()
against refine_detections_graph with its per-class NMS, proposals() against ProposalLayer, unmold()'s box
arithmetic against the stored denorm_boxes golden, and the two formulations of the ROI align against
one f64 interpolation of the contract's samples.  The NMS here is the oracle's (the product's runs on
the GPU only; tests/test_gpu_det.py repeats these cases with it)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import det_restatement as R
import oracle as O

torch = pytest.importorskip("torch")
from semtsdf import maskrcnn as MR  # noqa: E402

G = np.load(os.path.join(GOLDEN, "mrcnn_utils_golden.npz"))


@pytest.fixture(scope="module")
def model():
    return MR.MaskRCNN(MR.Config(DTYPE=torch.float32, BACKBONE="resnet50"), seed=0, nms=O.nms_sorted_cpu).eval()


def test_detections_equal_refine_detections_graph(model):
    """detections() against model.py:689-784 with the per-class NMS on each class's own boxes: 1000
    rois (the last 200 zero rows), 81 classes, clusters shared by the classes, score ties, background
    and below-confidence rows interleaved; every output row equal."""
    R.check_detection_case(model)


def test_detections_decide_pairs_at_the_threshold_as_the_per_class_rule(model):
    """1800 isolated pairs of classes 1, 40 and 80 whose refined boxes have an IoU one f32 step either
    side of 0.3 (and some exactly 0.3, which the strict > keeps).  IoU of class-offset boxes
    (refined + 2 * class in f32) decides several hundred of them the other way; the per-class rule of
    model.py:736-750 works on the boxes themselves."""
    R.check_pair_case(model)


def test_proposals_equal_proposal_layer(model):
    """proposals() against model.py:282-334: about 3000 anchors, the pre-NMS cut, the NMS cut at
    POST_NMS_ROIS_INFERENCE and the zero padding; equal score ties take the lower index first."""
    R.check_proposal_case(model)


def test_unmold_boxes_equal_reference_denorm_boxes(model):
    """unmold()'s boxes against utils.py:875-889 denorm_boxes as the reference executed it
    (denorm_480_640 of the golden): window (0, 0, 1, 1), a 480 x 640 image, the golden's boxes clipped
    to [0, 1] as detections of class 1.  Every row of positive pixel area equal, the dropped rows
    exactly the others (model.py:2414-2423)."""
    boxes = np.clip(G["delta_boxes"], 0, 1).astype(np.float32)
    want = G["denorm_480_640"]
    area = (want[:, 2] - want[:, 0]) * (want[:, 3] - want[:, 1])
    assert (area > 0).sum() > 200 and (area <= 0).sum() > 100  # both kinds of row are there
    R.check_unmold_boxes(model, boxes, want)


def test_unmold_boxes_round_the_f64_product(model):
    """denorm_boxes multiplies the f32 boxes by an integer array: NumPy takes that product in f64 and
    rounds it to the pixel.  Boxes whose every coordinate, times 479 or 639, sits within an f32 step of
    a half: rounding the product to f32 first moves each to the neighbouring pixel.  The expectation is
    the restated denorm_boxes, which the same test holds to the reference's executed golden."""
    np.testing.assert_array_equal(R.denorm_boxes(np.clip(G["delta_boxes"], 0, 1), (480, 640)), G["denorm_480_640"])
    boxes = R.half_pixel_boxes((480, 640))
    want = R.denorm_boxes(boxes, (480, 640))
    in32 = np.round(boxes * np.array([479, 639, 479, 639], np.float32) + np.array([0, 0, 1, 1], np.float32))
    print(f"{len(boxes)} boxes, {int((in32 != want).sum())} coordinates that an f32 product rounds the other way")
    assert len(boxes) >= 4 and (in32 != want).all()
    R.check_unmold_boxes(model, boxes, want)


# ---------------------------------------------------------------------------------- ROI align
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("pool", [2, 7, 14])
def test_roi_align_restatement_against_f64(dtype, pool):
    """roi_align_f32 (the f32 operations of include/semtsdf_det.h, one rounding to the output type T)
    against the f64 interpolation of the same samples, per element:

        |diff| <= 0.5 ulp_T(|v64|) + 8 * 2^-24 * max|corner|

    Half an ulp of T is the one conversion.  The rest is the f32 arithmetic: each lerp
    a * (1 - f) + b * f has four roundings (1 - f, two products, the sum), each at most 2^-24 of a
    value no larger than max|corner|, and the vertical lerp carries the two horizontal ones' errors
    with weights that sum to 1: 4 + 4 = 8 units of 2^-24 max|corner|.  Where that f32 error moves the
    value across a rounding boundary of T the conversion errs by half an ulp plus the move, which the
    same sum covers.  Derived, not measured."""
    feats, rois, lvl = R.roi_inputs(dtype)
    a = R.roi_align_f32(feats, rois, lvl, pool, dtype).astype(np.float64)
    b = R.roi_align_f64(feats, rois, lvl, pool)
    cmax = max(float(np.abs(f).max()) for f in feats)
    bound = 0.5 * R.ulp(b, dtype) + 8 * 2.0 ** -24 * cmax
    err = np.abs(a - b)
    print(f"{dtype} pool {pool}: max error / bound {float((err / bound).max()):.3f}, {int((b != 0).sum())} non-zero outputs")
    assert (b != 0).sum() > b.size // 4
    assert (err <= bound).all()


@pytest.mark.parametrize("pool", [2, 7, 14])
def test_grid_sample_roi_align_against_f64(model, pool):
    """The PyTorch formulation of MaskRCNN.roi_align (grid_sample of f32 maps on the CPU; the branch the
    device ROI align replaced) against roi_align_f64 on the rois of the GPU ROI-align tests, the level
    of each roi by the rule of model.py:406-413 for a 1024 x 1024 image.  Same f32 sample positions
    and inside decisions; grid_sample gets them through normalised coordinates, y / (H - 1) * 2 - 1 and
    back, which moves a position by a few f32 steps of the coordinate.  Tolerance 3e-6 * max|map|:
    measured against roi_align_f64 on these inputs the largest error is 1.45e-6 * max|map| (pool 2:
    9.4e-7, pool 7: 1.45e-6, pool 14: 1.34e-6), taken with a 2x margin."""
    feats, rois, _ = R.roi_inputs("fp16")
    lvl = R.roi_levels(rois, (1024, 1024))
    assert set(lvl.tolist()) == {2, 3, 4, 5}
    want = R.roi_align_f64(feats, rois, lvl, pool)
    with torch.no_grad():
        got = model.roi_align(torch.from_numpy(rois), [torch.from_numpy(f)[None] for f in feats], pool, (1024, 1024))
    got = got.numpy().astype(np.float64)
    cmax = max(float(np.abs(f).max()) for f in feats)
    err = float(np.abs(got - want).max()) / cmax
    print(f"pool {pool}: max error {err:.3e} of max|map|")
    assert got.shape == want.shape
    assert err <= 3e-6
