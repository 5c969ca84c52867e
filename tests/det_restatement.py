"""NumPy restatements of the detector's post-processing, written from the reference's
Mask_RCNN/mrcnn/model.py and mrcnn/utils.py (cited by line) and from the arithmetic that
include/semtsdf_det.h states for the ROI align, not from semtsdf/maskrcnn.py or the kernels; and the
seeded inputs that tests/test_det_post.py (CPU) and tests/test_gpu_det.py (GPU) share.

All box arithmetic is f32, one NumPy operation per operation of the rule, so that a result can be
compared exactly.  The log-scale columns of every delta the cases use are zero: exp(0) is exactly 1 in
every library, which leaves the shift arithmetic (IEEE add, subtract, multiply) to be compared."""
import numpy as np

import oracle as O

F = np.float32


# ------------------------------------------------------------------------------------ boxes
def apply_box_deltas(boxes, deltas):
    """model.py:219-240 apply_box_deltas_graph, f32."""
    boxes, deltas = np.asarray(boxes, F), np.asarray(deltas, F)
    height = boxes[:, 2] - boxes[:, 0]
    width = boxes[:, 3] - boxes[:, 1]
    center_y = boxes[:, 0] + F(0.5) * height
    center_x = boxes[:, 1] + F(0.5) * width
    center_y = center_y + deltas[:, 0] * height
    center_x = center_x + deltas[:, 1] * width
    height = height * np.exp(deltas[:, 2])
    width = width * np.exp(deltas[:, 3])
    y1 = center_y - F(0.5) * height
    x1 = center_x - F(0.5) * width
    return np.stack([y1, x1, y1 + height, x1 + width], axis=1)


def clip_boxes(boxes, window):
    """model.py:243-258 clip_boxes_graph: max(min(v, w2), w1) per coordinate, f32."""
    wy1, wx1, wy2, wx2 = (F(v) for v in window)
    y1 = np.maximum(np.minimum(boxes[:, 0], wy2), wy1)
    x1 = np.maximum(np.minimum(boxes[:, 1], wx2), wx1)
    y2 = np.maximum(np.minimum(boxes[:, 2], wy2), wy1)
    x2 = np.maximum(np.minimum(boxes[:, 3], wx2), wx1)
    return np.stack([y1, x1, y2, x2], axis=1)


def iou_pairs(a, b):
    """utils.py:58-76 compute_iou for the pairs (a[k], b[k]), f32, the areas as utils.py:108-109."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    y1 = np.maximum(a[:, 0], b[:, 0])
    y2 = np.minimum(a[:, 2], b[:, 2])
    x1 = np.maximum(a[:, 1], b[:, 1])
    x2 = np.minimum(a[:, 3], b[:, 3])
    inter = np.maximum(x2 - x1, F(0)) * np.maximum(y2 - y1, F(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area_a + area_b - inter)


def _nms_in_order(boxes_sorted, thr):
    """utils.py:116-150 on boxes already in their order of decreasing score (O.non_max_suppression is
    pinned to utils.py by tests/golden/mrcnn_utils_golden.npz); strictly decreasing stand-in scores
    keep the given order, which is where equal scores are decided: the lower index first, as
    tf.nn.top_k and tf.image.non_max_suppression take them."""
    n = len(boxes_sorted)
    if n == 0:
        return np.zeros(0, np.int64)
    return O.non_max_suppression(boxes_sorted, -np.arange(n, dtype=np.float64), thr).astype(np.int64)


def nms_grouped(boxes_sorted, groups, thr, max_out):
    """Greedy NMS in the given order (utils.py:116-150 with the IoU of utils.py:58-76 in f32), a box
    suppressed only by a kept box of its own group: the kept indices, at most max_out of them."""
    b = np.asarray(boxes_sorted, F)
    g = np.zeros(len(b), np.int64) if groups is None else np.asarray(groups)
    thr = F(thr)
    kept = []
    kept_by_group = {}
    for i in range(len(b)):
        if len(kept) >= max_out:
            break
        mine = kept_by_group.setdefault(int(g[i]), [])
        if mine:
            iou = iou_pairs(b[mine], np.broadcast_to(b[i], (len(mine), 4)))
            if (iou > thr).any():
                continue
        mine.append(i)
        kept.append(i)
    return np.array(kept, np.int64)


def refine_detections(rois, probs, deltas, window, cfg):
    """model.py:689-784 refine_detections_graph -> [DETECTION_MAX_INSTANCES, 6] f32
    (y1, x1, y2, x2, class_id, score), zero rows after the detections."""
    rois, probs, deltas = np.asarray(rois, F), np.asarray(probs, F), np.asarray(deltas, F)
    n = rois.shape[0]
    class_ids = probs.argmax(axis=1)                                            # :705
    class_scores = probs[np.arange(n), class_ids]                               # :707-708
    deltas_specific = deltas[np.arange(n), class_ids]                           # :710
    refined = apply_box_deltas(rois, deltas_specific * np.asarray(cfg.BBOX_STD_DEV, F))  # :713-714
    refined = clip_boxes(refined, window)                                       # :716
    keep = class_ids > 0                                                        # :721
    keep &= class_scores >= F(cfg.DETECTION_MIN_CONFIDENCE)                     # :723-727
    # the zero rows that ProposalLayer pads with (model.py:329-331) are no proposals and are no
    # candidates: the reference refines them to a zero-area box, which unmold_detections drops
    # (model.py:2414-2423)
    keep &= np.abs(rois).sum(axis=1) > 0
    keep = np.nonzero(keep)[0]
    picked = []
    for c in np.unique(class_ids[keep]):                                        # :734-757
        ixs = keep[class_ids[keep] == c]                                        # :739
        ixs = ixs[np.argsort(-class_scores[ixs], kind="stable")]
        k = _nms_in_order(refined[ixs], cfg.DETECTION_NMS_THRESHOLD)            # :741-745
        picked.append(ixs[k[:cfg.DETECTION_MAX_INSTANCES]])
    picked = np.sort(np.concatenate(picked)) if picked else np.zeros(0, np.int64)  # :760-765
    top = np.argsort(-class_scores[picked], kind="stable")[:cfg.DETECTION_MAX_INSTANCES]  # :767-771
    picked = picked[top]
    out = np.zeros((cfg.DETECTION_MAX_INSTANCES, 6), F)                         # :782-783
    out[:len(picked), :4] = refined[picked]                                     # :775-779
    out[:len(picked), 4] = class_ids[picked].astype(F)
    out[:len(picked), 5] = class_scores[picked]
    return out


def proposal_layer(logits, deltas, anchors, cfg):
    """model.py:282-334 ProposalLayer.call -> [POST_NMS_ROIS_INFERENCE, 4] f32, zero-padded.  The
    scores are the foreground softmax of the RPN logits (rpn_graph, model.py:862-864)."""
    logits, deltas, anchors = np.asarray(logits, F), np.asarray(deltas, F), np.asarray(anchors, F)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    scores = (e / e.sum(axis=1, keepdims=True))[:, 1]                           # :284
    deltas = deltas * np.asarray(cfg.RPN_BBOX_STD_DEV, F)                       # :287
    k = min(cfg.PRE_NMS_LIMIT, anchors.shape[0])                                # :293
    ix = np.argsort(-scores, kind="stable")[:k]                                 # :294 (ties: lower index)
    boxes = clip_boxes(apply_box_deltas(anchors[ix], deltas[ix]), (0, 0, 1, 1))  # :306-317
    keep = _nms_in_order(boxes, cfg.RPN_NMS_THRESHOLD)[:cfg.POST_NMS_ROIS_INFERENCE]  # :325-327
    out = np.zeros((cfg.POST_NMS_ROIS_INFERENCE, 4), F)                         # :330-331
    out[:len(keep)] = boxes[keep]
    return out


def denorm_boxes(boxes, shape):
    """utils.py:875-889 denorm_boxes: the f32 boxes times the integer scale is an f64 product in NumPy,
    np.around rounds halves to even."""
    h, w = shape
    scale = np.array([h - 1, w - 1, h - 1, w - 1])
    shift = np.array([0, 0, 1, 1])
    return np.around(np.multiply(np.asarray(boxes, F), scale) + shift).astype(np.int32)


def half_pixel_boxes(shape, seed=17, draws=2_000_000):
    """Boxes in [0, 1] whose every coordinate rounds to another pixel when the product with
    (h - 1, w - 1) is rounded to f32 before np.around than when it is taken in f64 as denorm_boxes
    takes it (the product sits within an f32 step of a half): about 1 in 80 000 seeded draws per
    coordinate, y1 and x1 from the lower third of the image and y2 and x2 from the upper, so that the
    boxes have a positive area."""
    rng = np.random.default_rng(seed)
    h, w = shape
    cols = []
    for den, sh, upper in ((h - 1, 0, False), (w - 1, 0, False), (h - 1, 1, True), (w - 1, 1, True)):
        v = rng.uniform(0.6, 1.0, draws).astype(F) if upper else rng.uniform(0.0, 0.4, draws).astype(F)
        in64 = np.around(v.astype(np.float64) * den + sh)
        in32 = np.round(v * F(den) + F(sh))
        cols.append(v[in64 != in32.astype(np.float64)])
    n = min(len(c) for c in cols)
    return np.stack([c[:n] for c in cols], axis=1)


def roi_levels(rois, image_shape):
    """model.py:406-413: level 4 + round(log2(sqrt(h w) / (224 / sqrt(image area)))) in 2..5; a roi
    without a positive area (log of 0 or of a NaN) takes level 2."""
    rois = np.asarray(rois, F)
    h = rois[:, 2] - rois[:, 0]
    w = rois[:, 3] - rois[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        lv = np.log2(np.sqrt(h * w) / F(224.0 / np.sqrt(float(image_shape[0] * image_shape[1]))))
        lv = np.clip(4 + np.round(lv), 2, 5)
    return np.where(np.isnan(lv), 2, lv).astype(np.int32)


# -------------------------------------------------------------------------------- ROI align
def round_to(v, dtype):
    """One round-to-nearest-even conversion of f32 values to fp16 or bf16, returned widened to f32."""
    v = np.ascontiguousarray(v, F)
    if dtype == "fp16":
        with np.errstate(over="ignore"):
            return v.astype(np.float16).astype(F)
    assert dtype == "bf16"
    u = v.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(F)


def _axis(p1, p2, size, pool):
    """The f32 sample positions of include/semtsdf_det.h along one axis:
    y = y1 * hm + (float)i * (((y2 - y1) * hm) / pm), inside when 0 <= y <= hm, y0 = floor(y),
    yb = min(y0 + 1, size - 1), fy = y - y0."""
    hm, pm = F(size - 1), F(pool - 1)
    i = np.arange(pool, dtype=F)
    step = ((p2 - p1) * hm) / pm
    y = (p1 * hm)[:, None] + i[None, :] * step[:, None]
    assert y.dtype == F
    inside = (y >= F(0)) & (y <= hm)
    y0f = np.floor(y)
    fy = y - y0f
    y0 = np.where(inside, y0f, 0).astype(np.int64)
    yb = np.minimum(y0 + 1, size - 1)
    return inside, y0, yb, fy


def _roi_align(feats, rois, lvl, pool, T):
    rois = np.asarray(rois, F)
    lvl = np.clip(np.asarray(lvl), 2, 5)
    n, C = rois.shape[0], feats[0].shape[0]
    out = np.zeros((n, C, pool, pool), T)
    one = T(1)
    for L in range(2, 6):
        sel = np.nonzero(lvl == L)[0]
        if sel.size == 0:
            continue
        f = np.asarray(feats[L - 2]).astype(T)  # [C, H, W], the values of the fp16 / bf16 map
        H, W = f.shape[1:]
        r = rois[sel]
        iy, y0, yb, fy = _axis(r[:, 0], r[:, 2], H, pool)
        ix, x0, xb, fx = _axis(r[:, 1], r[:, 3], W, pool)
        Y0, YB = y0[:, :, None], yb[:, :, None]
        X0, XB = x0[:, None, :], xb[:, None, :]
        v00, v01 = f[:, Y0, X0], f[:, Y0, XB]  # [C, m, pool, pool]
        v10, v11 = f[:, YB, X0], f[:, YB, XB]
        fxe, fye = fx.astype(T)[None, :, None, :], fy.astype(T)[None, :, :, None]
        top = v00 * (one - fxe) + v01 * fxe
        bot = v10 * (one - fxe) + v11 * fxe
        v = top * (one - fye) + bot * fye
        assert v.dtype == T
        inside = (iy[:, :, None] & ix[:, None, :])[None]
        out[sel] = np.where(inside, v, T(0)).transpose(1, 0, 2, 3)
    return out


def roi_align_f32(feats, rois, lvl, pool, dtype):
    """semtsdf_det_roi_align as include/semtsdf_det.h states it (PyramidROIAlign, model.py:374-452, with
    tf.image.crop_and_resize's positions): feats the four maps [C, H, W] (the values of the fp16 or bf16
    maps), every product, sum and quotient rounded to f32, the two horizontal lerps and then the
    vertical one, one conversion to `dtype` ("fp16" / "bf16"); the result widened to f32."""
    return round_to(_roi_align(feats, rois, lvl, pool, F), dtype)


def roi_align_f64(feats, rois, lvl, pool):
    """The same samples (the f32 positions and inside decisions are the contract) interpolated in f64,
    not rounded to the output type."""
    return _roi_align(feats, rois, lvl, pool, np.float64)


def ulp(v, dtype):
    """The spacing of fp16 / bf16 numbers at |v| (the subnormal spacing below the smallest normal)."""
    p, emin = {"fp16": (11, -14), "bf16": (8, -126)}[dtype]
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where(a > 0, np.maximum(e, emin), emin)
    return np.exp2(e - (p - 1))


def roi_cases(rng):
    """The rois of the ROI-align tests, [n, 4] f32: inside the image, straddling each border, fully
    outside, zero rois, clipped to exactly 0.0 and 1.0 on each side (what clip_boxes makes of a
    proposal at the border), y1 == y2 and x1 == x2, and inverted ones; shuffled."""
    def boxes(c, hw):
        return np.concatenate([c - hw / 2, c + hw / 2], axis=1)

    out = [boxes(rng.uniform(0.3, 0.7, (40, 2)), rng.uniform(0.02, 0.5, (40, 2)))]           # inside
    for side in range(4):                                                                    # straddling
        c = rng.uniform(0.2, 0.8, (8, 2))
        c[:, side % 2] = (0.0, 1.0)[side // 2] + rng.uniform(-0.05, 0.05, 8)
        out.append(boxes(c, rng.uniform(0.15, 0.4, (8, 2))))
    far = boxes(rng.uniform(0.2, 0.8, (8, 2)), rng.uniform(0.05, 0.3, (8, 2)))               # outside
    far[:4] += 1.5
    far[4:] -= 1.5
    out.append(far)
    out.append(np.zeros((6, 4)))                                                             # zero rois
    for side in range(4):                                                                    # clipped
        b = boxes(rng.uniform(0.3, 0.7, (8, 2)), rng.uniform(0.1, 0.4, (8, 2)))
        b[:, side] = (0.0, 0.0, 1.0, 1.0)[side]
        out.append(b)
    out.append(np.array([[0.0, 0.0, 1.0, 1.0], [0.0, 0.25, 1.0, 0.75], [0.5, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0],
                         [1.0, 0.0, 1.0, 1.0], [0.0, 1.0, 1.0, 1.0]]))
    flat = boxes(rng.uniform(0.3, 0.7, (8, 2)), rng.uniform(0.1, 0.4, (8, 2)))               # y1 == y2, x1 == x2
    flat[:4, 2] = flat[:4, 0]
    flat[4:, 3] = flat[4:, 1]
    out.append(flat)
    inv = boxes(rng.uniform(0.3, 0.7, (8, 2)), rng.uniform(0.1, 0.4, (8, 2)))                # inverted
    inv[:3] = inv[:3][:, [2, 1, 0, 3]]
    inv[3:6] = inv[3:6][:, [0, 3, 2, 1]]
    inv[6:] = inv[6:][:, [2, 3, 0, 1]]
    out.append(inv)
    r = np.concatenate(out).astype(F)
    return r[rng.permutation(len(r))]


# ------------------------------------------------------------------- pairs at the threshold
def near_threshold_pairs(thr, n, rng, cell, refine=None):
    """n pairs of boxes (a, b) whose IoU sits one f32 step either side of `thr`.

    Box a is random inside its own cell of a cell x cell grid over the unit square (pair k in cell k,
    so n <= cell^2; cell == 1: every pair in [0.2, 0.8]^2, the pairs then overlap one another) with
    margins that keep both boxes inside the cell: pairs do not touch one another.  Box b shares a's x1
    and has a's y extent with a small jitter; b.x2 is bisected over the f32 bit patterns between a.x1
    (IoU 0) and a.x2 (IoU > 0.8) until two adjacent floats lo, hi hold iou(lo) <= thr < iou(hi), the
    IoU in f32 as utils.py:58-76 takes it.  refine(boxes, "a" / "b"): the IoU is taken on the refined
    boxes instead (the detection head's deltas), the bisection still over b's own x2.

    Returns {"a", "b_lo", "b_hi"} [n, 4] f32 (the unrefined boxes), {"iou_lo", "iou_hi"} [n] f32 and
    "steps" [n] = hi - lo as integers, which the caller asserts to be 1 for every pair."""
    thr = F(thr)
    refine = refine or (lambda b, which: b)
    k = np.arange(n)
    if cell > 1:
        assert n <= cell * cell
        oy, ox, s = (k // cell) / cell, (k % cell) / cell, 1.0 / cell
    else:
        oy, ox, s = np.full(n, 0.2), np.full(n, 0.2), 0.6
    h, w = rng.uniform(0.3, 0.6, n) * s, rng.uniform(0.3, 0.6, n) * s
    y1, x1 = oy + rng.uniform(0.15, 0.25, n) * s, ox + rng.uniform(0.15, 0.25, n) * s
    a = np.stack([y1, x1, y1 + h, x1 + w], axis=1).astype(F)
    b = a.copy()
    b[:, 0] = (y1 + rng.uniform(-0.05, 0.05, n) * h).astype(F)
    b[:, 2] = (y1 + h + rng.uniform(-0.05, 0.05, n) * h).astype(F)
    ra = refine(a, "a")

    def iou_at(bits):
        bb = b.copy()
        bb[:, 3] = bits.astype(np.int32).view(F)
        return bb, iou_pairs(ra, refine(bb, "b"))

    lo = a[:, 1].copy().view(np.int32).astype(np.int64)
    hi = a[:, 3].copy().view(np.int32).astype(np.int64)
    assert (iou_at(lo)[1] <= thr).all() and (iou_at(hi)[1] > thr).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        above = iou_at(mid)[1] > thr
        move = hi - lo > 1
        hi = np.where(move & above, mid, hi)
        lo = np.where(move & ~above, mid, lo)
    b_lo, iou_lo = iou_at(lo)
    b_hi, iou_hi = iou_at(hi)
    return {"a": a, "b_lo": b_lo, "b_hi": b_hi, "iou_lo": iou_lo, "iou_hi": iou_hi, "steps": hi - lo}


def clustered_boxes(rng, n, spread=0.03):
    """Boxes around n / 12 cluster centres, as tests/test_maskrcnn.py's NMS cases: [n, 4] f32."""
    ctr = rng.uniform(0, 1, (max(n // 12, 1), 2))
    k = rng.integers(0, ctr.shape[0], n)
    cy, cx = ctr[k, 0] + rng.normal(0, spread, n), ctr[k, 1] + rng.normal(0, spread, n)
    h, w = rng.uniform(0.01, 0.25, n), rng.uniform(0.01, 0.25, n)
    return np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(F)


# ------------------------------------------------- inputs of detections() and proposals()
WINDOW = (0.0625, 0.03125, 0.9375, 0.96875)  # f32-exact: the window is clamped to in f32 everywhere
CLASSES = (0, 1, 2, 17, 40, 41, 63, 79, 80, 0, 1, 80)


def _probs_and_deltas(rng, cls, score, num_classes):
    n = len(cls)
    probs = rng.uniform(0.0, 0.01, (n, num_classes)).astype(F)
    probs[np.arange(n), cls] = score
    deltas = np.zeros((n, num_classes, 4), F)
    deltas[:, :, :2] = rng.normal(0, 0.5, (n, num_classes, 2))
    return probs, deltas


def detection_case(seed=11, n=1000, n_zero=200, num_classes=81):
    """rois, probs, deltas, window for refine_detections: nine cluster centres shared by all classes
    (boxes of different classes overlap as much as boxes of one), classes from CLASSES (background
    argmax rows among them), scores in [0.5, 1) (rows below DETECTION_MIN_CONFIDENCE among the
    others), exact score ties inside a class and across classes, scores exactly at the confidence
    bound, the last n_zero rois zero rows with confident classes; arbitrary shift deltas, zero
    log-scale deltas."""
    rng = np.random.default_rng(seed)
    m = n - n_zero
    ctr = rng.uniform(0.2, 0.8, (9, 2))
    k = rng.integers(0, 9, m)
    c = ctr[k] + rng.normal(0, 0.02, (m, 2))
    hw = rng.uniform(0.05, 0.25, (m, 2))
    rois = np.zeros((n, 4), F)
    rois[:m] = np.concatenate([c - hw / 2, c + hw / 2], axis=1)
    cls = np.asarray(CLASSES)[rng.integers(0, len(CLASSES), n)]
    score = rng.uniform(0.5, 1.0, n).astype(F)
    src, dst = rng.integers(0, m, 60), rng.integers(0, m, 60)
    score[dst] = score[src]                   # ties, whatever the classes
    cls[dst[:30]] = cls[src[:30]]             # half of them inside one class
    score[rng.integers(0, m, 10)] = F(0.7)    # at the bound: candidates (>=)
    score[rng.integers(0, m, 10)] = np.nextafter(F(0.7), F(0))
    probs, deltas = _probs_and_deltas(rng, cls, score, num_classes)
    return rois, probs, deltas, WINDOW


def pair_detection_case(seed=12, per_class=600, classes=(1, 40, 80), thr=0.3, num_classes=81):
    """rois, probs, deltas, window whose refined boxes are isolated pairs at the NMS threshold:
    per_class pairs for each class, the first half with b on the low side (IoU <= thr, the exact ties
    among them: both boxes are detections) and the second half on the high side (b is suppressed).
    Row 2k is a, row 2k + 1 is b, a has the higher score.  Also returns the refined pairs'
    {"iou": f32 IoU of every pair, "cls": its class, "suppressed": whether the per-class rule drops b}."""
    rng = np.random.default_rng(seed)
    npair = per_class * len(classes)
    cls_pair = np.repeat(np.asarray(classes), per_class)[rng.permutation(npair)]
    cls = np.repeat(cls_pair, 2)
    score = np.sort(rng.uniform(0.75, 1.0, 2 * npair).astype(F))[::-1].copy()
    probs, deltas = _probs_and_deltas(rng, cls, score, num_classes)
    deltas[:, :, :2] *= 0.2  # shifts of at most a few per cent of a box: the pair stays in its cell
    std = np.asarray((0.1, 0.1, 0.2, 0.2), F)
    d = deltas[np.arange(2 * npair), cls] * std

    window = (0.0, 0.0, 1.0, 1.0)  # every cell lies inside it: no box is clipped

    def refine(b, which):
        return clip_boxes(apply_box_deltas(b, d[0::2] if which == "a" else d[1::2]), window)

    p = near_threshold_pairs(thr, npair, rng, 64, refine=refine)
    assert (p["steps"] == 1).all()
    high = np.arange(npair) % 2 == 1
    rois = np.zeros((2 * npair, 4), F)
    rois[0::2] = p["a"]
    rois[1::2] = np.where(high[:, None], p["b_hi"], p["b_lo"])
    ra, rb = refine(rois[0::2], "a"), refine(rois[1::2], "b")
    iou = iou_pairs(ra, rb)
    info = {"iou": iou, "cls": cls_pair, "suppressed": iou > F(thr), "a": ra, "b": rb, "high": high}
    return (rois, probs, deltas, window), info


def proposal_case(seed=13, S=256, every=5):
    """logits, deltas, anchors for proposal_layer: every fifth anchor of the S x S pyramid (about
    3000), foreground logits a permutation of evenly spaced values (the order of the scores does not
    hang on the last bit of a softmax) with a few exact ties, arbitrary shift deltas that push boxes
    past the image's border (clipped, some to zero area), zero log-scale deltas."""
    from semtsdf import maskrcnn as MR

    rng = np.random.default_rng(seed)
    strides = [4, 8, 16, 32, 64]
    shapes = [(int(np.ceil(S / s)), int(np.ceil(S / s))) for s in strides]
    a = MR.generate_pyramid_anchors((32, 64, 128, 256, 512), (0.5, 1, 2), shapes, strides, 1)
    anchors = MR.norm_boxes(a, (S, S))[::every]
    n = anchors.shape[0]
    logits = np.zeros((n, 2), F)
    logits[:, 1] = np.linspace(-4, 4, n)[rng.permutation(n)]
    src, dst = rng.integers(0, n, 40), rng.integers(0, n, 40)
    logits[dst] = logits[src]
    deltas = np.zeros((n, 4), F)
    deltas[:, :2] = rng.normal(0, 1.5, (n, 2))
    return logits, deltas, anchors


# ------------------------------- the cases through the product, on the CPU or on the device
def _torch():
    import torch

    return torch


def run_detections(m, case, dev="cpu"):
    rois, probs, deltas, window = case
    torch = _torch()
    with torch.no_grad():
        d = m.detections(torch.from_numpy(rois).to(dev), torch.from_numpy(probs).to(dev),
                         torch.from_numpy(deltas).to(dev), window)
    return d.cpu().numpy()


def run_proposals(m, case, dev="cpu"):
    logits, deltas, anchors = case
    torch = _torch()
    with torch.no_grad():
        r = m.proposals(torch.from_numpy(logits).to(dev), torch.from_numpy(deltas).to(dev),
                        torch.from_numpy(anchors).to(dev))
    return r.cpu().numpy()


def check_detection_case(m, dev="cpu"):
    case = detection_case()
    for max_inst in (100, 30):
        m.config.DETECTION_MAX_INSTANCES = max_inst
        try:
            want = refine_detections(*case, m.config)
            got = run_detections(m, case, dev)
        finally:
            m.config.DETECTION_MAX_INSTANCES = 100
        nd = int((want[:, 4] > 0).sum())
        print(f"max {max_inst}: {nd} detections, classes {sorted(set(want[:nd, 4].astype(int)))}")
        assert got.shape == want.shape == (max_inst, 6)
        np.testing.assert_array_equal(got, want)
    # the case does what it is for: the cut and (with a wide limit) the zero rows both occur, ties and
    # scores at the bound are among the detections
    assert nd == 30
    m.config.DETECTION_MAX_INSTANCES = 1000
    try:
        want = refine_detections(*case, m.config)
        got = run_detections(m, case, dev)
    finally:
        m.config.DETECTION_MAX_INSTANCES = 100
    nd = int((want[:, 4] > 0).sum())
    s = want[:nd, 5]
    print(f"max 1000: {nd} detections, {int((np.diff(s) == 0).sum())} ties, {int((s == np.float32(0.7)).sum())} at 0.7")
    assert 100 < nd < 1000 and (np.diff(s) == 0).any() and (s == np.float32(0.7)).any()
    assert not (s < np.float32(0.7)).any()
    np.testing.assert_array_equal(got, want)


def check_pair_case(m, dev="cpu"):
    case, info = pair_detection_case()
    npair = len(info["iou"])
    thr = np.float32(0.3)
    # the input can tell the two forms apart: IoU of the boxes shifted by 2 * class (in f32) decides
    # some pairs differently from the IoU of the boxes themselves
    flips = 0
    for c in (1, 40, 80):
        sel = info["cls"] == c
        off = np.float32(2.0 * c)
        shifted = iou_pairs(info["a"][sel] + off, info["b"][sel] + off) > thr
        flips += int((shifted != info["suppressed"][sel]).sum())
    ties = int((info["iou"] == thr).sum())
    print(f"{npair} pairs, {int(info['suppressed'].sum())} suppressed, {ties} exactly at the threshold, "
          f"{flips} decided differently by class-offset boxes")
    assert flips > 0 and ties > 0
    assert info["suppressed"].any() and not info["suppressed"].all()
    m.config.DETECTION_MAX_INSTANCES = 2 * npair
    try:
        want = refine_detections(*case, m.config)
        got = run_detections(m, case, dev)
    finally:
        m.config.DETECTION_MAX_INSTANCES = 100
    # the restatement itself keeps every a and exactly the b's at or below the threshold
    assert int((want[:, 4] > 0).sum()) == 2 * npair - int(info["suppressed"].sum())
    nd_got = int((got[:, 4] > 0).sum())
    assert nd_got == 2 * npair - int(info["suppressed"].sum()), \
        f"{nd_got} detections, the per-class rule keeps {2 * npair - int(info['suppressed'].sum())}"
    np.testing.assert_array_equal(got, want)


def check_proposal_case(m, dev="cpu"):
    case = proposal_case()
    n = case[2].shape[0]
    assert 3000 <= n <= 3500
    cfg = m.config
    saved = cfg.PRE_NMS_LIMIT, cfg.POST_NMS_ROIS_INFERENCE
    try:
        for pre, post in ((1000, 200), (1000, 1000), (6000, 300)):
            cfg.PRE_NMS_LIMIT, cfg.POST_NMS_ROIS_INFERENCE = pre, post
            want = proposal_layer(*case, cfg)
            got = run_proposals(m, case, dev)
            nz = int((np.abs(want).sum(axis=1) > 0).sum())
            print(f"pre {pre} post {post}: {nz} non-zero rois")
            assert got.shape == want.shape == (post, 4)
            if post == 1000:
                assert nz < post  # zero padding
            else:
                assert (np.abs(want[-1]) > 0).any()  # the NMS was cut at `post`
            np.testing.assert_array_equal(got, want)
    finally:
        cfg.PRE_NMS_LIMIT, cfg.POST_NMS_ROIS_INFERENCE = saved


def check_unmold_boxes(m, boxes, want, dev="cpu"):
    """unmold() of `boxes` [n, 4] (normalised, inside [0, 1]) as detections of class 1 with window
    (0, 0, 1, 1) on a 480 x 640 image against `want`, the reference's pixel boxes: the rows of positive
    pixel area equal, the others dropped (model.py:2414-2423), in the compact and the fixed-row form."""
    torch = _torch()
    n = boxes.shape[0]
    score = np.linspace(0.99, 0.71, n, dtype=F)
    det = torch.from_numpy(np.concatenate([boxes.astype(F), np.ones((n, 1), F), score[:, None]], 1)).to(dev)
    masks = torch.zeros((n, m.config.NUM_CLASSES, 28, 28), device=dev)
    nwin = np.array([0.0, 0.0, 1.0, 1.0], F)
    ok = (want[:, 2] - want[:, 0]) * (want[:, 3] - want[:, 1]) > 0
    with torch.no_grad():
        out = m.unmold(det, masks, (480, 640), (1024, 1024), nwin, compact=True)
        fixed = m.unmold(det, masks, (480, 640), (1024, 1024), nwin, compact=False)
    np.testing.assert_array_equal(out["rois"].cpu().numpy(), want[ok])
    np.testing.assert_array_equal(out["scores"].cpu().numpy(), score[ok])
    np.testing.assert_array_equal(fixed["rois"].cpu().numpy(), want * ok[:, None])
    np.testing.assert_array_equal(fixed["class_ids"].cpu().numpy() > 0, ok)


ROI_MAPS = ((24, 40), (12, 20), (6, 10), (3, 5))
ROI_C = 5


def roi_inputs(dtype, seed=21):
    """Four non-square maps [C, H, W] holding fp16 / bf16 values (as f32), the rois of roi_cases and
    levels interleaved along n."""
    rng = np.random.default_rng(seed)
    feats = [round_to(rng.normal(0, 1, (ROI_C, h, w)).astype(np.float32), dtype) for h, w in ROI_MAPS]
    rois = roi_cases(rng)
    lvl = (2 + (np.arange(len(rois)) + rng.integers(0, 2, len(rois))) % 4).astype(np.int32)
    return feats, rois, lvl
