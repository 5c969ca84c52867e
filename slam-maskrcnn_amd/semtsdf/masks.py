"""Mask producer contract: Mask R-CNN detection masks -> the u8
instance-label mask the fusion consumes, on the GPU (semtsdf_masks_to_labels, restating
Mask_RCNN/dmask.py:21-59 mask_detect: filter_tiny_objects, preserve_small_objs, label
i + 1), or straight from the detector's pixel boxes and mini-masks (semtsdf_detections_to_labels:
unmold_mask of mrcnn/utils.py:565-581 evaluated per pixel, then the same rule).  The detector itself
(COCO-weight Mask R-CNN) is not part of this package: its weights are not available offline; any producer
that yields masks[H, W, N], or boxes and mini-masks, can feed it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .volume import DeviceBuffer

MIN_AREA = 2000  # dmask.py:42 (area > 2000)


def masks_to_labels_dev(masks_ptr: int, width: int, height: int, n: int, labels_ptr: int, min_area: int = MIN_AREA,
                        stream=None, want_count: bool = False):
    """Device masks [H][W][n] bytes -> device labels [H][W] u8 (async unless want_count)."""
    k = C.c_int()
    L.check(L.load().semtsdf_masks_to_labels(C.c_void_p(masks_ptr) if n else None, int(width), int(height), int(n),
                                             int(min_area), C.c_void_p(labels_ptr),
                                             C.byref(k) if want_count else None, stream))
    return k.value if want_count else None


MINI_DTYPES = {"float16": 0, "bfloat16": 1, "float32": 2}  # semtsdf_detections_to_labels' dtype codes


def detections_to_labels_workspace(n: int = 256) -> int:
    """Bytes of device workspace detections_to_labels_dev needs for n detections."""
    return int(L.load().semtsdf_detections_to_labels_workspace(int(n)))


def detections_to_labels_dev(boxes_ptr: int, mini_ptr: int, dtype: int, mh: int, mw: int, n: int, width: int,
                             height: int, labels_ptr: int, work_ptr: int, min_area: int = MIN_AREA, areas_ptr: int = 0,
                             stream=None, want_count: bool = False):
    """Device pixel boxes [n][4] int32 + mini-masks [n][mh][mw] (dtype 0 fp16, 1 bf16, 2 f32) -> device
    labels [H][W] u8 by the paste rule of include/semtsdf.h (unmold_mask, then the dmask.py rule), the
    [H][W][n] masks never made; areas_ptr (u32 [n]) optional; work_ptr: detections_to_labels_workspace(n)
    bytes.  Async unless want_count; allocates nothing (capturable in a HIP graph)."""
    k = C.c_int()
    L.check(L.load().semtsdf_detections_to_labels(
        C.c_void_p(boxes_ptr) if boxes_ptr else None, C.c_void_p(mini_ptr) if mini_ptr else None, int(dtype), int(mh),
        int(mw), int(n), int(width), int(height), int(min_area), C.c_void_p(labels_ptr) if labels_ptr else None,
        C.c_void_p(areas_ptr) if areas_ptr else None, C.c_void_p(work_ptr) if work_ptr else None,
        C.byref(k) if want_count else None, stream))
    return k.value if want_count else None


def detections_to_labels(boxes: np.ndarray, mini: np.ndarray, shape, min_area: int = MIN_AREA,
                         dtype: int | None = None):
    """Host convenience: boxes int [N, 4] (y1, x1, y2, x2) pixels, mini [N, mh, mw] float16 / float32 (or
    uint16 holding bf16 bits with dtype=1), shape (H, W) -> (labels u8 [H, W], kept detections,
    areas u32 [N])."""
    b = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    m = np.ascontiguousarray(mini)
    if m.ndim != 3 or m.shape[0] != b.shape[0]:
        raise ValueError("mini must be [N, mh, mw] with one mask per box")
    if dtype is None:
        if m.dtype.name not in MINI_DTYPES:
            raise ValueError(f"mini dtype {m.dtype} is not float16 or float32 (bf16: uint16 bits with dtype=1)")
        dtype = MINI_DTYPES[m.dtype.name]
    elif dtype in (0, 1, 2) and m.dtype.itemsize != (4 if dtype == 2 else 2):
        raise ValueError(f"mini elements of {m.dtype.itemsize} bytes do not hold dtype {dtype}")
    n, mh, mw = m.shape
    H, W = int(shape[0]), int(shape[1])
    out = np.zeros((H, W), np.uint8)
    areas = np.zeros(n, np.uint32)
    bufs = [DeviceBuffer(max(b.nbytes, 1)), DeviceBuffer(max(m.nbytes, 1)), DeviceBuffer(max(H * W, 1)),
            DeviceBuffer(max(areas.nbytes, 1)), DeviceBuffer(detections_to_labels_workspace(n))]
    bb, mb, ob, ab, wb = bufs
    try:
        if n:
            bb.upload(b)
            mb.upload(m)
        kept = detections_to_labels_dev(bb.ptr if n else 0, mb.ptr if n else 0, dtype, mh, mw, n, W, H, ob.ptr, wb.ptr,
                                        min_area, ab.ptr, want_count=True)
        ob.download(out)
        if n:
            ab.download(areas)
        L.check(L.load().semtsdf_stream_sync(None))
    finally:
        for d in bufs:
            d.free()
    return out, kept, areas


def masks_to_labels(masks: np.ndarray, min_area: int = MIN_AREA):
    """Host convenience: masks bool/u8 [H, W, N] -> (labels u8 [H, W], kept detections)."""
    m = np.ascontiguousarray(masks)
    if m.ndim != 3:
        raise ValueError("masks must be [H, W, N]")
    m = m.view(np.uint8) if m.dtype == np.bool_ else np.ascontiguousarray(m, dtype=np.uint8)
    H, W, n = m.shape
    out = np.zeros((H, W), np.uint8)
    mb = DeviceBuffer(max(m.nbytes, 1))
    ob = DeviceBuffer(H * W)
    try:
        if n:
            mb.upload(m)
        kept = masks_to_labels_dev(mb.ptr, W, H, n, ob.ptr, min_area, want_count=True)
        ob.download(out)
        L.check(L.load().semtsdf_stream_sync(None))
    finally:
        mb.free()
        ob.free()
    return out, kept
