"""GPU: the empty-space octant maps the marches skip with (k_brick_plain, k_brick_dilate,
k_brick_oct_axis x3) equal, after every frame, a NumPy restatement of the map's definition from
the downloaded sdf: brick b is skippable when every voxel of the bricks b + {0,1}^3 (inside the
volume) holds sdf >= voxel/2 (1 + 2^-16); byte o of b's word is the L-inf distance, capped, to
the nearest non-skippable brick of octant o (bit a of o set: negative along axis a), i.e. min
over 0 <= k < cap per axis of max(k, d0(b + s k e))."""
import numpy as np
import pytest

from maps_restatement import CAP, numpy_maps  # noqa: F401

pytestmark = pytest.mark.gpu

KI = (520.9, 521.0, 325.1, 249.7)


@pytest.fixture(scope="module")
def S():
    import semtsdf
    from semtsdf import _lib as L

    semtsdf.load()
    return semtsdf, L


@pytest.fixture(scope="module")
def stream():
    from semtsdf.synth import SyntheticStream

    st = SyntheticStream(seed=3)
    return st, [st.frame(k) for k in range(5)]


@pytest.mark.parametrize("dims", [(96, 96, 96), (120, 88, 136), (64, 160, 40)])
def test_maps_equal_definition_at_every_frame(S, stream, dims):
    semtsdf, L = S
    st, frames = stream
    p = semtsdf.default_params(64, KI, 640, 480)
    p.dim[0], p.dim[1], p.dim[2] = dims
    semtsdf.place_from_frame(p, frames[0].depth, float(np.mean(frames[0].depth[frames[0].depth > 0])) / 5000.0,
                             L.PLACE_SFM)
    p.flags = L.F_SEMANTIC | L.F_GATE_COLOR
    v = semtsdf.Volume(p, 0)
    v.set_instrumentation(events=False)
    voxel = float(p.voxel[0])
    skippable = []
    for k, fr in enumerate(frames):
        E = (fr.w2c @ frames[0].c2w).astype(np.float32)
        v.integrate(fr.depth, fr.rgb, np.ascontiguousarray(fr.mask), E)
        wa = v.map_words()
        assert wa is not None
        s = v.download(wt=False, color=False)["sdf"].reshape(dims)
        ref = numpy_maps(s, voxel)
        assert np.array_equal(wa, ref), (dims, k, int(np.count_nonzero(wa != ref)))
        skippable.append(float(np.mean((wa & np.uint64(0xFF)) > 0)))
    v.close()
    # the maps are not trivial: some bricks skippable, some not
    assert 0.0 < skippable[-1] < 1.0, skippable
