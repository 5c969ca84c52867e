"""The handle's device-memory accounting (semtsdf_state.device_bytes) around the calls that allocate
on first use, swap a buffer for one of another size, or take scratch for the call only: exact
deltas on the first use, none on the second, none from call scratch on success or failure, and the
same figure again for a volume destroyed and created anew.  One 64^3 SEMANTIC|GATE volume at
640x480; no kernel or shape beyond what the rest of the suite runs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 640, 480
NPX = W * H
KI = (520.9, 521.0, 325.1, 249.7)
NVOX = 64 ** 3  # 64^3 is whole 1 x 8 x 32 tiles: every stored voxel is a voxel of the volume


@pytest.fixture(scope="module")
def S():
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    return semtsdf, L


@pytest.fixture(scope="module")
def scene(S):
    from semtsdf.synth import SyntheticStream

    semtsdf, L = S
    st = SyntheticStream(seed=0)
    frames = [st.frame(k) for k in range(4)]
    p = semtsdf.default_params(64, KI, W, H)
    d0 = frames[0].depth
    semtsdf.place_from_frame(p, d0, float(np.mean(d0[d0 > 0])) / 5000.0, L.PLACE_SFM)
    p.flags = L.F_SEMANTIC | L.F_GATE_COLOR
    Es = [(fr.w2c @ frames[0].c2w).astype(np.float32) for fr in frames]
    dist = p.vol_start[2] + 0.5 * (p.vol_end[2] - p.vol_start[2])
    s2w, c = semtsdf.orbit_camera(list(p.Kinv), 0.3, dist)
    return {"p": p, "frames": frames, "E": Es, "s2w": s2w, "c": c}


def nbytes(vol):
    return int(vol.state().device_bytes)


def fused(S, scene, nframes=2):
    semtsdf, _ = S
    vol = semtsdf.Volume(scene["p"], 0)
    for k in range(1, 1 + nframes):
        fr = scene["frames"][k]
        vol.integrate(fr.depth, fr.rgb, fr.mask, scene["E"][k])
    return vol


def test_first_use_of_each_lazy_buffer(S, scene):
    """Each host-pointer variant allocates its device staging on the first call and never again."""
    from semtsdf.volume import DeviceBuffer

    semtsdf, L = S
    vol = fused(S, scene)
    s2w, c = scene["s2w"], scene["c"]
    fr = scene["frames"][3]

    def deltas(call):
        a = nbytes(vol)
        call()
        b = nbytes(vol)
        call()
        return b - a, nbytes(vol) - b

    assert deltas(lambda: vol.raycast(s2w, c, L.RENDER_LABEL)) == (7 * NPX, 0)
    assert deltas(lambda: vol.raycast(s2w, c, L.RENDER_LABEL, want_t=True)) == (0, 0)  # the pair came together
    assert deltas(lambda: vol.render_maps(s2w, c, 1)) == (34 * NPX, 0)
    maps = {}

    def track():
        maps["frame"] = vol.frame_maps(fr.depth)

    assert deltas(track) == (52 * NPX + 8 * 32, 0)
    model = vol.render_maps(s2w, c, 1, want=("point", "normal", "flags"))
    E = scene["E"][3]
    assert deltas(lambda: vol.icp_system(maps["frame"], model, E, E)) == (0, 0)  # shares the frame maps' scratch
    assert deltas(lambda: vol.assoc_probs(E)) == (160 * NPX, 0)

    # the launch order of the fused view + association march: two u32 per 16x16 tile of mask plus view
    d_b, r_b, m_b, out_b = DeviceBuffer(NPX * 2), DeviceBuffer(NPX * 3), DeviceBuffer(NPX), DeviceBuffer(NPX * 3)
    d_b.upload(fr.depth, vol.stream)
    r_b.upload(fr.rgb, vol.stream)

    def view_frame():
        m_b.upload(fr.mask, vol.stream)
        vol.parse_frame_view_dev(d_b.ptr, r_b.ptr, m_b.ptr, E, s2w, c, L.RENDER_LABEL, out_b.ptr)
        vol.sync()

    tiles = 2 * ((W + 15) // 16) * ((H + 15) // 16)
    assert deltas(view_frame) == (2 * 4 * tiles, 0)
    for b in (d_b, r_b, m_b, out_b):
        b.free()
    vol.close()


def test_icp_system_first_allocates_the_tracking_scratch(S, scene):
    """icp_system before any frame_maps call takes the same scratch."""
    semtsdf, L = S
    vol = fused(S, scene, 1)
    n = NPX
    frame = {"vertex": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32),
             "flags": np.zeros(n, np.uint8)}
    model = {"point": frame["vertex"], "normal": frame["normal"], "flags": frame["flags"]}
    E = scene["E"][1]
    a = nbytes(vol)
    vol.icp_system(frame, model, E, E)
    b = nbytes(vol)
    vol.frame_maps(scene["frames"][1].depth)
    assert (b - a, nbytes(vol) - b) == (52 * NPX + 8 * 32, 0)
    vol.close()


def test_weight_storage_cycle_and_recreate(S, scene):
    """An upload with a weight of 70000 adds 2 B per stored voxel, reset() removes it again; a
    volume destroyed and created again starts at the first handle's initial figure."""
    semtsdf, L = S
    vol = semtsdf.Volume(scene["p"], 0)
    initial = nbytes(vol)
    wt = np.ones(NVOX, np.int32)
    wt[12345] = 70000
    vol.upload(wt=wt)
    assert nbytes(vol) == initial + 2 * NVOX
    assert np.array_equal(vol.download(sdf=False, color=False)["wt"], wt)
    assert nbytes(vol) == initial + 2 * NVOX  # the transfers' staging is scratch of the call
    vol.reset()
    assert nbytes(vol) == initial
    vol.upload(wt=wt)  # and once more round the cycle
    assert nbytes(vol) == initial + 2 * NVOX
    vol.reset()
    assert nbytes(vol) == initial
    vol.close()
    again = semtsdf.Volume(scene["p"], 0)
    assert nbytes(again) == initial
    again.close()


def test_call_scratch_leaves_the_count_alone(S, scene):
    """extract_mesh with capacities below the counted sizes returns ERR_INVALID and leaves
    device_bytes unchanged; the same call with enough capacity then succeeds, also unchanged."""
    semtsdf, L = S
    lib = semtsdf.load()
    vol = fused(S, scene)
    before = nbytes(vol)
    nv, nt = C.c_uint64(), C.c_uint64()
    assert lib.semtsdf_extract_mesh(vol.handle, 1, None, 0, None, 0, C.byref(nv), C.byref(nt)) == 0
    n, m = int(nv.value), int(nt.value)
    assert n > 0 and m > 0
    assert nbytes(vol) == before
    verts = np.zeros(n * 32, np.uint8)
    tris = np.zeros(m * 3, np.uint32)

    def full(vcap, tcap):
        a, b = C.c_uint64(), C.c_uint64()
        rc = lib.semtsdf_extract_mesh(vol.handle, 1, verts.ctypes.data, vcap, tris.ctypes.data, tcap, C.byref(a),
                                      C.byref(b))
        return rc, int(a.value), int(b.value)

    for vcap, tcap in ((n - 1, m), (n, m - 1)):
        assert full(vcap, tcap) == (L.ERR_INVALID, n, m)
        assert nbytes(vol) == before
    assert full(n, m) == (0, n, m)
    assert nbytes(vol) == before
    assert verts.any() and tris.any()  # the mesh was written
    vol.instance_stats(0.2, 1, overlap=True)
    semtsdf.export_surface(vol, 0.2, 1)
    assert nbytes(vol) == before
    vol.close()
