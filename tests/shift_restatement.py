"""The definition semtsdf_shift is held to, in NumPy on the reference layouts.

numpy_shift: voxel i of the result holds what voxel i + s held, and the reset state where i + s
lies outside the volume: slices and a fill, nothing else.  twin: the handle a shifted volume must
be indistinguishable from through the ABI: created at the shifted placement, the NumPy-shifted
download of the old state uploaded into it, the counters set."""
import numpy as np

KEYS = ("sdf", "wt", "color", "hist", "cls", "cls_cnt")
CHANNELS = {"sdf": 1, "wt": 1, "color": 3, "hist": 32, "cls": 1, "cls_cnt": 1}


def numpy_shift(state, shift, mu, dims=None):
    """`state`: a dict of arrays in the reference layout (x-major, z fastest; colour 3 and
    histogram 32 values per voxel), flat as Volume.download returns them or shaped.  `dims`
    defaults to the shape of a 3-D state["sdf"].  Returns arrays of the input's shapes and dtypes."""
    dims = tuple(int(d) for d in (dims if dims is not None else np.asarray(state["sdf"]).shape))
    assert len(dims) == 3
    s = [int(x) for x in shift]
    dst, src = [], []
    for a in range(3):
        lo, hi = max(0, -s[a]), min(dims[a], dims[a] - s[a])  # destination indices with a source inside
        dst.append(slice(lo, max(lo, hi)))
        src.append(slice(lo + s[a], max(lo, hi) + s[a]))
    out = {}
    for k, a in state.items():
        a = np.asarray(a)
        v = a.reshape(dims + (CHANNELS[k],))
        r = np.zeros_like(v)
        if k == "sdf":
            r[...] = np.float32(mu)
        r[dst[0], dst[1], dst[2]] = v[src[0], src[1], src[2]]
        out[k] = r.reshape(a.shape)
    return out


def shifted_placement(params, shift):
    """(vol_start, vol_end) after the shift: rounded once from float64."""
    start = [np.float32(np.float64(params.vol_start[a]) + np.float64(shift[a]) * np.float64(params.voxel[a]))
             for a in range(3)]
    end = [np.float32(np.float64(params.vol_end[a]) + np.float64(shift[a]) * np.float64(params.voxel[a]))
           for a in range(3)]
    return start, end


# ------------------------------------------------------------------------------------
# the walking sequence of the follow tests: a camera that leaves the cube placed around frame 0.
# Half-size frames (320 x 240, halved intrinsics) keep the host-side synthesis short.
# ------------------------------------------------------------------------------------
SEQ_FRAMES = 20
SEQ_DIM = 64
SEQ_W, SEQ_H = 320, 240
# Metres per frame.  The cube placed around frame 0 reaches 1.79 m in x, so a step of 0.06 m would
# leave the last focus (1.14 m) inside it; 0.1 m carries it to 1.9 m, outside, which the tests assert.
SEQ_STEP = (0.1, 0, 0.035)


def sequence_intrinsics():
    from semtsdf.config import TUM_INTRINSICS

    return tuple(float(x) / 2 for x in TUM_INTRINSICS)


def sequence_stream():
    from semtsdf.synth import SyntheticStream

    return SyntheticStream(seed=0, width=SEQ_W, height=SEQ_H, intrinsics=sequence_intrinsics(), min_area=500,
                           yaw_step=0, trans_step=SEQ_STEP)


def sequence_focus_depth(frame0):
    """The mean depth of frame 0 in metres: the focus depth of every follow call of the sequence."""
    return float(np.mean(frame0.depth[frame0.depth > 0])) / 5000.0


def plan_sequence(stream, frame0):
    """The shifts the policy plans along the sequence, on the host alone: the volume placed from
    frame 0 (semtsdf_place_from_frame), follow(pose, focus, trigger_bricks=1) before every frame
    k >= 1, the placement moved by the float64 rule.  Returns (params of frame 0, [(k, shift)])."""
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.follow import plan_shift

    focus = sequence_focus_depth(frame0)
    p = semtsdf.default_params(SEQ_DIM, sequence_intrinsics(), SEQ_W, SEQ_H)
    semtsdf.place_from_frame(p, frame0.depth, focus, L.PLACE_SFM)
    start, end, voxel = list(p.vol_start), list(p.vol_end), list(p.voxel)
    c2w0 = stream.c2w(0)
    shifts = []
    for k in range(1, SEQ_FRAMES):
        E = (np.linalg.inv(stream.c2w(k)) @ c2w0).astype(np.float32)
        s = plan_shift(start, end, voxel, E, focus, trigger_bricks=1)
        if s is None:
            continue
        shifts.append((k, s))
        start = [float(np.float32(np.float64(start[a]) + np.float64(s[a]) * np.float64(voxel[a]))) for a in range(3)]
        end = [float(np.float32(np.float64(end[a]) + np.float64(s[a]) * np.float64(voxel[a]))) for a in range(3)]
    return p, shifts


def full_download(vol):
    from semtsdf import _lib as L

    return vol.download(hist=bool(vol.params.flags & L.F_SEMANTIC), cls=bool(vol.params.flags & L.F_VOTE))


def twin(vol, shift, params=None, device=0):
    """The upload-made twin of `vol` (not yet shifted) after `shift`.  `params`: the parameter
    block of the shifted handle (get_params()); by default that of `vol` with the placement moved
    by the float64 rule."""
    import ctypes as C

    import semtsdf
    from semtsdf import _lib as L

    old = vol.get_params()
    if params is None:
        params = L.Params()
        C.memmove(C.byref(params), C.byref(old), C.sizeof(L.Params))
        start, end = shifted_placement(old, shift)
        for a in range(3):
            params.vol_start[a], params.vol_end[a] = float(start[a]), float(end[a])
    st = vol.state()
    moved = numpy_shift(full_download(vol), shift, old.mu, dims=tuple(old.dim))
    tw = semtsdf.Volume(params, device)
    tw.upload(**moved)
    tw.set_state(int(st.n_obs), int(st.num_objs))
    return tw
