"""Thin object wrapper over one `semtsdf_vol` handle of the C ABI.

All compute goes through libsemtsdf.so (HIP kernels for gfx950); this module only
marshals arguments.  Device buffers for resident frames (bench, multi-frame pipelines) are
allocated through the library too, so no second allocator is involved.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def default_params(dim, intrinsics, width, height) -> L.Params:
    lib = L.load()
    p = L.Params()
    intr = L.f32(intrinsics, 4)
    L.check(lib.semtsdf_params_default(C.byref(p), int(dim), L.ptr(intr), int(width), int(height)))
    return p


def place_from_frame(p: L.Params, depth: np.ndarray, mean_depth: float, mode: int) -> L.Params:
    lib = L.load()
    d = np.ascontiguousarray(depth, dtype=np.uint16)
    if d.size != p.width * p.height:
        raise ValueError("depth size does not match params")
    L.check(lib.semtsdf_place_from_frame(C.byref(p), L.ptr(d), float(mean_depth), int(mode)))
    return p


def orbit_camera(Kinv, angle: float, dist: float):
    lib = L.load()
    ki = L.f32(Kinv, 16)
    s2w = np.zeros(16, np.float32)
    c = np.zeros(3, np.float32)
    L.check(lib.semtsdf_orbit_camera(L.ptr(ki), float(angle), float(dist), L.ptr(s2w), L.ptr(c)))
    return s2w, c


class DeviceBuffer:
    """A device allocation owned by the library's allocator (hipMalloc)."""

    def __init__(self, nbytes: int):
        lib = L.load()
        self.nbytes = int(nbytes)
        self._p = C.c_void_p()
        L.check(lib.semtsdf_dev_malloc(C.byref(self._p), self.nbytes))

    @property
    def ptr(self) -> int:
        return self._p.value

    def upload(self, a: np.ndarray, stream=None, offset: int = 0):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        L.check(L.load().semtsdf_memcpy(C.c_void_p(self.ptr + offset), L.ptr(a), a.nbytes, 1, stream))

    def copy_from(self, src_ptr: int, nbytes: int, stream=None, offset: int = 0):
        """Device-to-device copy into this buffer (asynchronous on ``stream``)."""
        assert offset + nbytes <= self.nbytes
        L.check(L.load().semtsdf_memcpy(C.c_void_p(self.ptr + offset), C.c_void_p(src_ptr), int(nbytes), 3, stream))

    def download(self, out: np.ndarray, stream=None, offset: int = 0):
        assert out.flags["C_CONTIGUOUS"] and offset + out.nbytes <= self.nbytes
        L.check(L.load().semtsdf_memcpy(L.ptr(out), C.c_void_p(self.ptr + offset), out.nbytes, 2, stream))

    def free(self):
        if self._p.value:
            L.check(L.load().semtsdf_dev_free(self._p))
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Volume:
    def __init__(self, params: L.Params, device: int = 0):
        lib = L.load()
        self.params = params
        self._h = C.c_void_p()
        L.check(lib.semtsdf_create(C.byref(params), int(device), C.byref(self._h)))
        self.W, self.H = params.width, params.height
        st = self.state()
        self.local_dim = tuple(st.local_dim)
        self.nvox = int(st.local_voxels)  # reference layout (dense rows of local_dim[2] planes)

    # ---- lifecycle
    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return L.load().semtsdf_get_stream(self._h)

    def close(self):
        if self._h and self._h.value:
            L.check(L.load().semtsdf_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        L.check(L.load().semtsdf_reset(self._h, None))

    def shift(self, sx: int, sy: int, sz: int, stream=None):
        """Move the volume by whole bricks (semtsdf_shift): voxel i then holds what voxel i + s
        held, what slides in is the reset state, and vol_start / vol_end move with it.  Each
        component is a multiple of 8 voxels.  `params` is refreshed from the handle."""
        s = np.array([int(sx), int(sy), int(sz)], np.int32)
        L.check(L.load().semtsdf_shift(self._h, L.ptr(s), stream))
        self.params = self.get_params()

    def get_params(self) -> L.Params:
        p = L.Params()
        L.check(L.load().semtsdf_get_params(self._h, C.byref(p)))
        return p

    def state(self) -> L.State:
        st = L.State()
        L.check(L.load().semtsdf_get_state(self._h, C.byref(st)))
        return st

    def set_state(self, n_obs: int, num_objs: int):
        L.check(L.load().semtsdf_set_state(self._h, int(n_obs), int(num_objs)))

    def sync(self):
        L.check(L.load().semtsdf_stream_sync(C.c_void_p(self.stream)))

    # ---- frames (host pointers)
    def _frame(self, depth, rgb, mask):
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        r = np.ascontiguousarray(rgb, dtype=np.uint8)
        if d.size != self.W * self.H or r.size != self.W * self.H * 3:
            raise ValueError(f"frame must be {self.H}x{self.W} (depth u16, rgb u8x3)")
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.size != self.W * self.H:
                raise ValueError("mask must be HxW u8")
        return d, r, m

    def integrate(self, depth, rgb, mask, E):
        d, r, m = self._frame(depth, rgb, mask)
        e = L.f32(E, 16)
        L.check(L.load().semtsdf_integrate(self._h, L.ptr(d), L.ptr(r), L.ptr(m), L.ptr(e), None))

    def associate(self, mask: np.ndarray, E) -> L.AssocStats:
        """Relabels `mask` (u8, C-contiguous) in place and returns the decision."""
        assert mask.dtype == np.uint8 and mask.flags["C_CONTIGUOUS"] and mask.size == self.W * self.H
        st = L.AssocStats()
        e = L.f32(E, 16)
        L.check(L.load().semtsdf_associate(self._h, L.ptr(mask), L.ptr(e), C.byref(st), None))
        return st

    def parse_frame(self, depth, rgb, mask, E) -> L.AssocStats:
        d, r, m = self._frame(depth, rgb, None)
        st = L.AssocStats()
        e = L.f32(E, 16)
        if mask is not None:
            assert mask.dtype == np.uint8 and mask.flags["C_CONTIGUOUS"] and mask.size == self.W * self.H
        L.check(L.load().semtsdf_parse_frame(self._h, L.ptr(d), L.ptr(r), L.ptr(mask), L.ptr(e), C.byref(st), None))
        return st

    def assoc_probs(self, E):
        n = self.W * self.H * L.MAX_OBJECTS
        probs = np.zeros(n, np.float32)
        box = np.zeros(n, np.uint8)
        e = L.f32(E, 16)
        L.check(L.load().semtsdf_assoc_probs(self._h, L.ptr(e), L.ptr(probs), L.ptr(box), None))
        return probs.reshape(self.H, self.W, L.MAX_OBJECTS), box.reshape(self.H, self.W, L.MAX_OBJECTS)

    # ---- device-resident frames
    def integrate_dev(self, depth_ptr: int, rgb_ptr: int, mask_ptr: int | None, E, stream=None):
        e = L.f32(E, 16)
        L.check(L.load().semtsdf_integrate_dev(self._h, C.c_void_p(depth_ptr), C.c_void_p(rgb_ptr),
                                               C.c_void_p(mask_ptr) if mask_ptr else None, L.ptr(e), stream))

    def integrate_dev_async(self, depth_ptr: int, rgb_ptr: int, mask_ptr: int | None, E, inputs_ready=None,
                            stream=None):
        """integrate_dev with the frame prepass on the volume's prep stream, overlapping the
        previous frame's integrate; inputs_ready: a raw hipEvent_t marking the inputs complete
        (None: they already are).  The inputs must not change until this frame has run."""
        e = L.f32(E, 16)
        L.check(L.load().semtsdf_integrate_dev_async(self._h, C.c_void_p(depth_ptr), C.c_void_p(rgb_ptr),
                                                     C.c_void_p(mask_ptr) if mask_ptr else None, L.ptr(e),
                                                     C.c_void_p(inputs_ready) if inputs_ready else None, stream))

    def integrate_vote_dev(self, depth_ptr: int, rgb_ptr: int, cls_ptr: int, E, stream=None):
        e = L.f32(E, 16)
        L.check(L.load().semtsdf_integrate_vote_dev(self._h, C.c_void_p(depth_ptr), C.c_void_p(rgb_ptr),
                                                    C.c_void_p(cls_ptr), L.ptr(e), stream))

    def parse_frame_dev(self, depth_ptr: int, rgb_ptr: int, mask_ptr: int | None, E, stream=None,
                        integrate_after_event: int | None = None):
        """integrate_after_event: a raw hipEvent_t (e.g. torch.cuda.Event.cuda_event) the
        frame's integrate waits for (readers of the previous state on other streams)."""
        e = L.f32(E, 16)
        L.check(L.load().semtsdf_parse_frame_dev_after(self._h, C.c_void_p(depth_ptr), C.c_void_p(rgb_ptr),
                                                       C.c_void_p(mask_ptr) if mask_ptr else None, L.ptr(e),
                                                       C.c_void_p(integrate_after_event) if integrate_after_event
                                                       else None, stream))

    def parse_frame_view_dev(self, depth_ptr: int, rgb_ptr: int, mask_ptr: int | None, E, s2w, c, mode,
                             out_ptr: int, t_ptr: int | None = None, stream=None):
        """parse_frame_dev plus one live view of the volume as it stands before this frame (the
        view shown after the previous frame), rendered in the same launch as this frame's
        association march (semtsdf_parse_frame_view_dev)."""
        e = L.f32(E, 16)
        s = L.f32(s2w, 16)
        cc = L.f32(c, 3)
        L.check(L.load().semtsdf_parse_frame_view_dev(self._h, C.c_void_p(depth_ptr), C.c_void_p(rgb_ptr),
                                                      C.c_void_p(mask_ptr) if mask_ptr else None, L.ptr(e),
                                                      L.ptr(s), L.ptr(cc), int(mode), C.c_void_p(out_ptr),
                                                      C.c_void_p(t_ptr) if t_ptr else None, stream))

    def associate_dev(self, mask_ptr: int, E, stream=None, want_stats=False):
        e = L.f32(E, 16)
        st = L.AssocStats() if want_stats else None
        L.check(L.load().semtsdf_associate_dev(self._h, C.c_void_p(mask_ptr), L.ptr(e),
                                               C.byref(st) if st is not None else None, stream))
        return st

    # ---- render
    def raycast(self, s2w, c, mode=L.RENDER_LABEL, want_t=False):
        out = np.zeros((self.H, self.W, 3), np.uint8)
        t = np.zeros((self.H, self.W), np.float32) if want_t else None
        s = L.f32(s2w, 16)
        cc = L.f32(c, 3)
        L.check(L.load().semtsdf_raycast(self._h, L.ptr(s), L.ptr(cc), int(mode), L.ptr(out), L.ptr(t), None))
        return (out, t) if want_t else out

    def raycast_dev(self, s2w, c, mode, out_ptr: int, t_ptr: int | None = None, stream=None):
        s = L.f32(s2w, 16)
        cc = L.f32(c, 3)
        L.check(L.load().semtsdf_raycast_dev(self._h, L.ptr(s), L.ptr(cc), int(mode), C.c_void_p(out_ptr),
                                             C.c_void_p(t_ptr) if t_ptr else None, stream))

    # ---- model maps
    def render_maps(self, s2w, c, min_weight: int = 1, want=L.MAP_NAMES) -> dict:
        """The model maps of a view (semtsdf_render_maps): a dict of the maps named in `want`,
        NumPy arrays [H, W] (t, votes f32; label, flags u8) or [H, W, 3] (point, normal f32)."""
        from .maps import MAP_LAYOUT, maps_out

        want = (want,) if isinstance(want, str) else tuple(want)
        out = {}
        for name in want:
            if name not in MAP_LAYOUT:
                raise ValueError(f"unknown map {name!r} (one of {', '.join(L.MAP_NAMES)})")
            dt, ch = MAP_LAYOUT[name]
            out[name] = np.zeros((self.H, self.W) + ((ch,) if ch > 1 else ()), dt)
        o = maps_out(want, out)
        s = L.f32(s2w, 16)
        cc = L.f32(c, 3)
        L.check(L.load().semtsdf_render_maps(self._h, L.ptr(s), L.ptr(cc), int(min_weight), C.byref(o), None))
        return out

    def render_maps_dev(self, s2w, c, min_weight: int = 1, stream=None, **pointers):
        """render_maps into device buffers, asynchronous on `stream`: one raw device pointer per
        requested map, by name (t=..., point=..., normal=..., label=..., votes=..., flags=...)."""
        from .maps import maps_out

        o = maps_out([k for k, p in pointers.items() if p], pointers)
        s = L.f32(s2w, 16)
        cc = L.f32(c, 3)
        L.check(L.load().semtsdf_render_maps_dev(self._h, L.ptr(s), L.ptr(cc), int(min_weight), C.byref(o), stream))

    # ---- camera tracking (semtsdf/track.py drives these)
    def frame_maps(self, depth, want=("vertex", "normal", "flags")) -> dict:
        """The frame maps of a depth image (semtsdf_frame_maps): camera-space vertex and normal f32
        [H, W, 3] and the validity byte u8 [H, W] (bit 0: depth, bit 1: normal) named in `want`."""
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.size != self.W * self.H:
            raise ValueError(f"depth must be {self.H}x{self.W} u16")
        want = (want,) if isinstance(want, str) else tuple(want)
        shapes = {"vertex": ((self.H, self.W, 3), np.float32), "normal": ((self.H, self.W, 3), np.float32),
                  "flags": ((self.H, self.W), np.uint8)}
        bad = [w for w in want if w not in shapes]
        if bad:
            raise ValueError(f"unknown frame map {bad[0]!r} (one of {', '.join(shapes)})")
        out = {k: np.zeros(*shapes[k]) for k in want}
        L.check(L.load().semtsdf_frame_maps(self._h, L.ptr(d), L.ptr(out.get("vertex")), L.ptr(out.get("normal")),
                                            L.ptr(out.get("flags")), None))
        return out

    def frame_maps_dev(self, depth_ptr: int, vertex: int | None = None, normal: int | None = None,
                       flags: int | None = None, stream=None):
        """frame_maps from and into device buffers (raw pointers), asynchronous on `stream`."""
        L.check(L.load().semtsdf_frame_maps_dev(self._h, C.c_void_p(depth_ptr), *[C.c_void_p(p) if p else None
                                                                                    for p in (vertex, normal, flags)],
                                                stream))

    def _system(self, fn, maps, photo, grid, E_ref, E_cur, gates, stride, words_ptr=None, stream=None, sizes=None,
                error=None):
        """One call of a tracking-system entry point `fn`: `maps` the six maps in semtsdf_icp_in order
        (frame vertex, normal, flags; model point, normal, flags), `photo` the four intensity arrays
        in semtsdf_rgbd_in order or None, `grid` the integers the entry point takes between the inputs
        and the extrinsics (the frame grid or the level), `gates` its thresholds.  With `sizes` the
        host form: arrays, each of that many elements or ValueError(error), and the words are
        returned.  Without it the device form: raw pointers and `words_ptr`, nothing is read back."""
        ins = list(maps) + list(photo or ())
        words = None
        if sizes is not None:
            ins = [np.ascontiguousarray(a, t) for a, t in zip(ins, (np.float32, np.float32, np.uint8) * 2
                                                               + (np.uint32, np.uint8) * 2)]
            if any(a.size != size for a, size in zip(ins, sizes)):
                raise ValueError(error)
            words = np.zeros(L.RGBD_WORDS if photo else L.ICP_WORDS, np.int64)
            addrs, wp = [a.ctypes.data for a in ins], L.ptr(words)
        else:
            addrs, wp = [int(p) if p else None for p in ins], C.c_void_p(words_ptr) if words_ptr else None
        structs = [C.byref(L.IcpIn(*addrs[:6]))] + ([C.byref(L.RgbdIn(*addrs[6:]))] if photo else [])
        er, ec = L.f32(E_ref, 16), L.f32(E_cur, 16)
        L.check(fn(self._h, *structs, *[int(g) for g in grid], L.ptr(er), L.ptr(ec), *[float(g) for g in gates],
                   int(stride), wp, stream))
        return words

    @staticmethod
    def _maps(frame: dict, model: dict) -> list:
        return [frame["vertex"], frame["normal"], frame["flags"], model["point"], model["normal"], model["flags"]]

    def icp_system(self, frame: dict, model: dict, E_ref, E_cur, dist_max: float = 0.1, cos_min: float = 0.8,
                   stride: int = 1) -> np.ndarray:
        """The 32 int64 words of one ICP iteration's point-to-plane system (semtsdf_icp_system) from
        host arrays: `frame` as frame_maps returns it, `model` the point, normal, flags of
        render_maps at pose_camera(Kinv, E_ref)."""
        n = self.W * self.H
        return self._system(L.load().semtsdf_icp_system, self._maps(frame, model), None, (), E_ref, E_cur,
                            (dist_max, cos_min), stride, sizes=(n * 3, n * 3, n) * 2,
                            error=f"maps must be {self.H}x{self.W}")

    def icp_system_dev(self, pointers, E_ref, E_cur, dist_max, cos_min, stride, words_ptr: int, stream=None):
        """icp_system on device buffers: `pointers` the six raw pointers in semtsdf_icp_in order
        (frame vertex, normal, flags; model point, normal, flags), `words_ptr` 32 int64 on the
        device; asynchronous on `stream`, nothing is read back."""
        self._system(L.load().semtsdf_icp_system_dev, pointers, None, (), E_ref, E_cur, (dist_max, cos_min), stride,
                     words_ptr, stream)

    # ---- depth pyramid (semtsdf/track.py's track_pyramid drives these)
    @staticmethod
    def _pyramid_band(radius, sigma_r, band, nlevels):
        if band is None:
            if int(radius) == 0 and int(nlevels) > 1:
                raise ValueError("band must be given when radius is 0 (its default is 3 * sigma_r of the filter)")
            band = 3.0 * float(sigma_r)
        return float(band)

    def frame_levels(self, nlevels: int = 3) -> list:
        """Width, height and Kinv (f32 [3, 3]) of the pyramid's levels (semtsdf_frame_levels); no device work."""
        lv = (L.FrameLevel * L.PYRAMID_MAX_LEVELS)()
        L.check(L.load().semtsdf_frame_levels(self._h, int(nlevels), lv))
        return [{"width": int(v.width), "height": int(v.height),
                 "Kinv": np.array(v.Kinv[:], np.float32).reshape(3, 3)} for v in lv[:int(nlevels)]]

    def frame_pyramid(self, depth, nlevels: int = 3, radius: int = 3, sigma_r: float = 0.05, band=None,
                      want=("vertex", "normal", "flags")) -> list:
        """The depth pyramid of a depth image and the frame maps of its levels (semtsdf_frame_pyramid):
        one dict per level with width, height, Kinv, z (f32 [h, w], metres, 0 = no depth) and the
        maps named in `want` (vertex, normal f32 [h, w, 3]; flags u8 [h, w]).  Level 0 is the depth
        through the edge-preserving filter of `radius` and `sigma_r` (radius 0: unfiltered), each
        further level a halving within `band` metres, by default 3 * sigma_r (to be given when
        radius is 0)."""
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.size != self.W * self.H:
            raise ValueError(f"depth must be {self.H}x{self.W} u16")
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in ("vertex", "normal", "flags")]
        if bad:
            raise ValueError(f"unknown frame map {bad[0]!r} (one of vertex, normal, flags)")
        band = self._pyramid_band(radius, sigma_r, band, nlevels)
        out = self.frame_levels(nlevels)  # refuses a bad nlevels before anything is sized by it
        lv = (L.FrameLevel * L.PYRAMID_MAX_LEVELS)()
        for o, v in zip(out, lv):
            h, w = o["height"], o["width"]
            o["z"] = np.zeros((h, w), np.float32)
            for name in want:
                o[name] = np.zeros((h, w) if name == "flags" else (h, w, 3), np.uint8 if name == "flags" else np.float32)
            v.z = o["z"].ctypes.data
            for name in want:
                setattr(v, name, o[name].ctypes.data)
        L.check(L.load().semtsdf_frame_pyramid(self._h, L.ptr(d), int(radius), float(sigma_r), band, int(nlevels), lv,
                                               None))
        return out

    def frame_pyramid_dev(self, depth_ptr: int, levels, radius: int = 3, sigma_r: float = 0.05, band=None,
                          stream=None) -> list:
        """frame_pyramid from and into device buffers, asynchronous on `stream`: `levels` holds one
        dict per level with the raw device pointer "z" and optionally "vertex", "normal", "flags".
        Returns the levels' width, height and Kinv as frame_levels does."""
        nlevels = len(levels)
        band = self._pyramid_band(radius, sigma_r, band, nlevels)
        lv = (L.FrameLevel * max(nlevels, L.PYRAMID_MAX_LEVELS))()  # the library refuses a bad count
        for o, v in zip(levels, lv):
            for name in ("z", "vertex", "normal", "flags"):
                setattr(v, name, int(o[name]) if o.get(name) else None)
        L.check(L.load().semtsdf_frame_pyramid_dev(self._h, C.c_void_p(depth_ptr) if depth_ptr else None, int(radius),
                                                   float(sigma_r), band, nlevels, lv, stream))
        return [{"width": int(v.width), "height": int(v.height),
                 "Kinv": np.array(v.Kinv[:], np.float32).reshape(3, 3)} for v in lv[:nlevels]]

    def icp_system_level(self, frame: dict, model: dict, E_ref, E_cur, dist_max: float = 0.1, cos_min: float = 0.8,
                         stride: int = 1) -> np.ndarray:
        """icp_system with the frame maps on a grid of their own (semtsdf_icp_system_level): `frame`
        a level of frame_pyramid ([h, w] taken from its flags), `model` the full-resolution point,
        normal, flags of render_maps at pose_camera(Kinv, E_ref)."""
        fl = np.ascontiguousarray(frame["flags"], np.uint8)
        if fl.ndim != 2:
            raise ValueError("frame flags must be [h, w]")
        fh, fw = fl.shape
        m, n = fw * fh, self.W * self.H
        return self._system(L.load().semtsdf_icp_system_level, self._maps(frame, model), None, (fw, fh), E_ref, E_cur,
                            (dist_max, cos_min), stride, sizes=(m * 3, m * 3, m, n * 3, n * 3, n),
                            error=f"frame maps must be {fh}x{fw}, model maps {self.H}x{self.W}")

    def icp_system_level_dev(self, pointers, frame_width: int, frame_height: int, E_ref, E_cur, dist_max, cos_min,
                             stride, words_ptr: int, stream=None):
        """icp_system_level on device buffers: `pointers` as icp_system_dev takes them, the frame's
        three on a frame_width x frame_height grid; asynchronous on `stream`, nothing is read back."""
        self._system(L.load().semtsdf_icp_system_level_dev, pointers, None, (frame_width, frame_height), E_ref, E_cur,
                     (dist_max, cos_min), stride, words_ptr, stream)

    # ---- RGB-D tracking (semtsdf/track.py's track_rgbd drives these)
    def intensity_pyramid(self, rgb, valid=None, nlevels: int = 3) -> list:
        """The intensity pyramid of a u8 colour image [H, W, 3] (semtsdf_intensity_pyramid): one dict
        per level with width, height, S (u32 [h, w], the integer sums; the intensity is
        S * 2^-(14 + 2 l)) and valid (u8 [h, w]).  `valid` u8 [H, W], nonzero = valid; None: all valid."""
        c = np.ascontiguousarray(rgb, dtype=np.uint8)
        if c.size != self.W * self.H * 3:
            raise ValueError(f"rgb must be {self.H}x{self.W}x3 u8")
        m = None
        if valid is not None:
            m = np.ascontiguousarray(valid, dtype=np.uint8)
            if m.size != self.W * self.H:
                raise ValueError(f"valid must be {self.H}x{self.W} u8")
        nl = int(nlevels)
        lv = (L.IntensityLevel * max(nl, L.PYRAMID_MAX_LEVELS))()
        out = []
        for l in range(max(0, min(nl, L.PYRAMID_MAX_LEVELS))):  # the library refuses a bad count
            h, w = self.H >> l, self.W >> l
            out.append({"width": w, "height": h, "S": np.zeros((h, w), np.uint32), "valid": np.zeros((h, w), np.uint8)})
            lv[l].S = out[l]["S"].ctypes.data
            lv[l].valid = out[l]["valid"].ctypes.data
        L.check(L.load().semtsdf_intensity_pyramid(self._h, L.ptr(c), L.ptr(m), nl, lv, None))
        return out

    def intensity_pyramid_dev(self, rgb_ptr: int, valid_ptr, levels, stream=None) -> list:
        """intensity_pyramid from and into device buffers, one launch, asynchronous on `stream`:
        `levels` holds one dict per level with the raw device pointers "S" and "valid"; valid_ptr may
        be None.  Returns the levels' width and height."""
        nl = len(levels)
        lv = (L.IntensityLevel * max(nl, L.PYRAMID_MAX_LEVELS))()
        for o, v in zip(levels, lv):
            v.S = int(o["S"]) if o.get("S") else None
            v.valid = int(o["valid"]) if o.get("valid") else None
        L.check(L.load().semtsdf_intensity_pyramid_dev(self._h, C.c_void_p(rgb_ptr) if rgb_ptr else None,
                                                       C.c_void_p(valid_ptr) if valid_ptr else None, nl, lv, stream))
        return [{"width": int(v.width), "height": int(v.height)} for v in lv[:nl]]

    def rgbd_system_level(self, frame: dict, model: dict, f_int: dict, m_int: dict, level: int, E_ref, E_cur,
                          dist_max: float = 0.1, cos_min: float = 0.8, r_max: float = 0.1, stride: int = 1) -> np.ndarray:
        """The 64 int64 words of one RGB-D iteration on pyramid level `level`
        (semtsdf_rgbd_system_level) from host arrays: `frame` and `model` as icp_system_level takes
        them (the frame maps of that level), `f_int` and `m_int` that level of intensity_pyramid of the
        frame's colour image and of the model's colour render (dicts with S and valid)."""
        fh, fw = self.H >> int(level), self.W >> int(level)
        m, n = fw * fh, self.W * self.H
        return self._system(L.load().semtsdf_rgbd_system_level, self._maps(frame, model),
                            [f_int["S"], f_int["valid"], m_int["S"], m_int["valid"]], (level,), E_ref, E_cur,
                            (dist_max, cos_min, r_max), stride, sizes=(m * 3, m * 3, m, n * 3, n * 3, n) + (m,) * 4,
                            error=f"frame maps and intensities must be {fh}x{fw}, model maps {self.H}x{self.W}")

    def rgbd_system_level_dev(self, pointers, photo, level: int, E_ref, E_cur, dist_max, cos_min, r_max, stride,
                              words_ptr: int, stream=None):
        """rgbd_system_level on device buffers: `pointers` as icp_system_level_dev takes them, `photo`
        the four raw pointers in semtsdf_rgbd_in order (frame S, valid; model S, valid), `words_ptr`
        64 int64 on the device; asynchronous on `stream`, nothing is read back."""
        self._system(L.load().semtsdf_rgbd_system_level_dev, pointers, photo, (level,), E_ref, E_cur,
                     (dist_max, cos_min, r_max), stride, words_ptr, stream)

    # ---- state transfer (reference layouts)
    def download(self, sdf=True, wt=True, color=True, hist=False, cls=False):
        n = self.nvox
        ci32 = bool(self.params.flags & L.F_COLOR_I32)
        out = {}
        a_sdf = np.zeros(n, np.float32) if sdf else None
        a_wt = np.zeros(n, np.int32) if wt else None
        a_col = np.zeros(n * 3, np.int32 if ci32 else np.uint8) if color else None
        a_hist = np.zeros(n * L.MAX_OBJECTS, np.uint32) if hist else None
        a_cls = np.zeros(n, np.int32) if cls else None
        a_cnt = np.zeros(n, np.int32) if cls else None
        L.check(L.load().semtsdf_download(self._h, L.ptr(a_sdf), L.ptr(a_wt), L.ptr(a_col), L.ptr(a_hist),
                                          L.ptr(a_cls), L.ptr(a_cnt)))
        for k, v in (("sdf", a_sdf), ("wt", a_wt), ("color", a_col), ("hist", a_hist), ("cls", a_cls),
                     ("cls_cnt", a_cnt)):
            if v is not None:
                out[k] = v
        return out

    def download_slab(self, x0: int, x1: int, sdf=True, wt=True, color=True, hist=False, cls=False):
        """The x-planes [x0, x1) of download() (semtsdf_download_slab)."""
        n = (int(x1) - int(x0)) * int(self.local_dim[1]) * int(self.local_dim[2])
        ci32 = bool(self.params.flags & L.F_COLOR_I32)
        arrs = {"sdf": np.zeros(n, np.float32) if sdf else None, "wt": np.zeros(n, np.int32) if wt else None,
                "color": np.zeros(n * 3, np.int32 if ci32 else np.uint8) if color else None,
                "hist": np.zeros(n * L.MAX_OBJECTS, np.uint32) if hist else None,
                "cls": np.zeros(n, np.int32) if cls else None, "cls_cnt": np.zeros(n, np.int32) if cls else None}
        L.check(L.load().semtsdf_download_slab(self._h, int(x0), int(x1), *[L.ptr(arrs[k]) for k in
                                                                             ("sdf", "wt", "color", "hist", "cls",
                                                                              "cls_cnt")]))
        return {k: v for k, v in arrs.items() if v is not None}

    def upload(self, sdf=None, wt=None, color=None, hist=None, cls=None, cls_cnt=None):
        ci32 = bool(self.params.flags & L.F_COLOR_I32)

        def c(a, dt):
            return None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(-1)

        arrs = [c(sdf, np.float32), c(wt, np.int32), c(color, np.int32 if ci32 else np.uint8), c(hist, np.uint32),
                c(cls, np.int32), c(cls_cnt, np.int32)]
        L.check(L.load().semtsdf_upload(self._h, *[L.ptr(a) for a in arrs]))

    # ---- brick paging (semtsdf/bricks.py drives these)
    def brick_counts(self):
        """(nbx, nby, nbz): the 8^3 bricks per axis, ceil(dim / 8)."""
        return tuple((int(d) + 7) // 8 for d in self.local_dim)

    def pack_bricks(self, lo=None, hi=None):
        """The occupied bricks of the brick box lo <= b < hi (default: the whole volume) as
        (bricks, words): a structured array (b i32 x 3, bins u32, offset u64) in ascending
        (bx, by, bz) order and the u32 words of their records back to back (semtsdf_pack_bricks:
        a count call, then a fill call)."""
        lo = np.array([0, 0, 0] if lo is None else lo, np.int32).reshape(3)
        hi = np.array(self.brick_counts() if hi is None else hi, np.int32).reshape(3)
        nb, nw = C.c_uint64(0), C.c_uint64(0)
        fn = L.load().semtsdf_pack_bricks
        L.check(fn(self._h, L.ptr(lo), L.ptr(hi), None, 0, None, 0, C.byref(nb), C.byref(nw)))
        bricks = np.zeros(nb.value, L.BRICK_DTYPE)
        words = np.zeros(nw.value, np.uint32)
        if nb.value:
            L.check(fn(self._h, L.ptr(lo), L.ptr(hi), C.c_void_p(bricks.ctypes.data), nb.value,
                       C.c_void_p(words.ctypes.data), nw.value, C.byref(nb), C.byref(nw)))
        return bricks, words

    def unpack_bricks(self, bricks, words):
        """Overwrites the listed bricks with their records (semtsdf_unpack_bricks): `bricks` and
        `words` as pack_bricks returns them, of this volume or of one with the same flags."""
        bricks = np.ascontiguousarray(bricks, L.BRICK_DTYPE).reshape(-1)
        words = np.ascontiguousarray(words, np.uint32).reshape(-1)
        L.check(L.load().semtsdf_unpack_bricks(self._h, C.c_void_p(bricks.ctypes.data) if bricks.size else None,
                                               bricks.size, C.c_void_p(words.ctypes.data) if words.size else None,
                                               words.size))

    # ---- instance inventory and id remapping
    def instance_stats(self, sdf_max: float = 0.2, min_weight: int = 1, overlap: bool = True) -> dict:
        """Per-instance voxel counts, votes, supports, index and colour sums, boxes and the
        overlap table of this (semantic) volume: semtsdf.instances.instance_stats."""
        from .instances import instance_stats

        return instance_stats(self, sdf_max, min_weight, overlap)

    def remap_instances(self, lut, num_objs: int = -1, stream=None):
        """The histogram through `lut` (32 ids; lut[0] == 0) in place, merging, dropping or
        renumbering ids; num_objs (-1: unchanged) becomes the next id (semtsdf_remap_instances;
        queued on `stream`, None: the volume's own)."""
        t = np.ascontiguousarray(np.asarray(lut).reshape(-1))
        if t.size != L.MAX_OBJECTS or (t < 0).any() or (t > 255).any():
            raise ValueError(f"lut must hold {L.MAX_OBJECTS} ids")
        t = t.astype(np.uint8)
        L.check(L.load().semtsdf_remap_instances(self._h, L.ptr(t), int(num_objs), stream))

    # ---- instrumentation
    def set_instrumentation(self, events: bool = True, count: bool = False, force_exact: bool = False):
        """events: HIP-event kernel timing; count: touched/gated voxel counters; force_exact: every
        association row decided from its exact f32 pixel-order sums (tests, cost measurement)."""
        flags = (1 if events else 0) | (2 if count else 0) | (4 if force_exact else 0)
        L.check(L.load().semtsdf_set_instrumentation(self._h, flags))

    def map_words(self):
        """The octant distance map of the current state (numpy uint64 per 8^3 brick, x-major, z
        fastest; byte o = octant o's distance in bricks), or None without octant maps."""
        import numpy as np
        n = C.c_uint64(0)
        L.check(L.load().semtsdf_map_words(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros(n.value, dtype=np.uint64)
        L.check(L.load().semtsdf_map_words(self._h, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out

    def filter_overlaps_dev(self, probs_ptr: int, box_ptr: int, mask_ptr: int, stream=None) -> L.AssocStats:
        """TSDF::filter_overlaps (tsdf.cu:304-416) on device arrays: probs f32 [H*W][32], box u8
        [H*W][32], mask u8 [H*W] relabelled in place; uses this handle's n_obs and num_objs."""
        st = L.AssocStats()
        L.check(L.load().semtsdf_filter_overlaps_dev(self._h, C.c_void_p(probs_ptr), C.c_void_p(box_ptr),
                                                     C.c_void_p(mask_ptr), C.byref(st), stream))
        return st

    def timing(self) -> L.Timing:
        t = L.Timing()
        L.check(L.load().semtsdf_get_timing(self._h, C.byref(t)))
        return t

    def reset_timing(self):
        L.check(L.load().semtsdf_reset_timing(self._h))
