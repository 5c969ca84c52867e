"""The host side of the moving volume: the policy that decides when the cube follows the camera
(semtsdf.follow.plan_shift) on hand-computed cases, the set of voxels a shift pushes out
(semtsdf.follow.leaving) and the NumPy definition of a shift (tests/shift_restatement.py) against
plain loops, the walking sequence of the GPU test, and the argument checks of semtsdf_shift that
need no device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import shift_restatement as S

START, END = (-1.0, -1.0, 1.0), (1.0, 1.0, 3.0)   # centre (0, 0, 2)
VOXEL = (0.03125,) * 3                             # a brick is 0.25 m


def w2c(origin, c2w_rot=np.eye(3)):
    m = np.eye(4)
    m[:3, :3] = c2w_rot.T
    m[:3, 3] = -c2w_rot.T @ np.asarray(origin, np.float64)
    return m


@pytest.mark.parametrize("origin, focus, trigger, want", [
    ((0, 0, 0), 2.0, 2, None),                      # focus at the centre
    ((0, 0, 0), 2.4990234375, 2, None),             # 1.996 bricks: just under the trigger
    ((0, 0, 0), 2.5, 2, (0, 0, 16)),                # exactly 2 bricks: at the trigger
    ((0, 0, 0), 2.25, 1, (0, 0, 8)),                # trigger of one brick
    ((0, 0, 0), 1.3, 2, (0, 0, -16)),               # -2.8 bricks truncates towards zero (floor: -24)
    ((0.8, -0.3, 0), 2.0, 2, (24, -8, 0)),          # 3.2 and -1.2 bricks
    ((-0.49, 0.49, 0), 2.0, 2, None),               # -1.96 and 1.96 bricks
])
def test_plan_shift_hand_cases(origin, focus, trigger, want):
    from semtsdf.follow import plan_shift

    assert plan_shift(START, END, VOXEL, w2c(origin), focus, trigger) == want


def test_plan_shift_rotated_camera():
    from semtsdf.follow import plan_shift

    # the camera at (0, 0, 2) looks along world +x: its z axis is the third column of the rotation
    rot = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    assert plan_shift(START, END, VOXEL, w2c((0, 0, 2), rot), 1.0, 2) == (32, 0, 0)
    assert plan_shift(START, END, VOXEL, w2c((0, 0, 2), rot), 0.3, 2) is None
    # looking along world -y from (0, 0.1, 2): focus (0, -0.9, 2), -3.6 bricks
    rot = np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    assert plan_shift(START, END, VOXEL, w2c((0, 0.1, 2), rot), 1.0, 2) == (0, -24, 0)


def test_plan_shift_anisotropic_voxels():
    from semtsdf.follow import plan_shift

    voxel = (0.03125, 0.0625, 0.125)  # bricks of 0.25, 0.5 and 1 m
    # focus - centre = (0.8, -1.2, 1.0): 3.2, -2.4 and 1 bricks
    assert plan_shift(START, END, voxel, w2c((0.8, -1.2, 0)), 3.0, 2) == (24, -16, 8)
    assert plan_shift(START, END, voxel, w2c((0.2, -0.9, 0)), 3.9, 2) is None  # 0.8, -1.8, 1.9


@pytest.mark.parametrize("shift", [(8, 0, 0), (0, -8, 0), (0, 0, 32), (-8, 8, -8), (24, 0, 0), (0, 0, 0), (0, 32, -80)])
def test_leaving_equals_a_loop(shift):
    from semtsdf.follow import leaving

    dim = (24, 28, 72)
    idx = np.array(list(itertools.product(*[range(d) for d in dim])), np.uint32)
    got = leaving(dim, shift)(idx)
    want = np.zeros(len(idx), bool)
    for n, j in enumerate(idx.tolist()):
        want[n] = any(not (0 <= j[a] - shift[a] < dim[a]) for a in range(3))
    assert got.dtype == bool and np.array_equal(got, want)
    # what leaves is what has no destination: the rest maps one to one onto the destinations with a source
    stays = int((~want).sum())
    assert stays == int(np.prod([max(0, dim[a] - abs(shift[a])) for a in range(3)]))


@pytest.mark.parametrize("shift", [(8, 0, 0), (0, -8, 0), (0, 0, 32), (-8, 8, -8), (16, 0, 0)])
def test_numpy_shift_equals_a_triple_loop(shift):
    dims = (16, 12, 40)
    rng = np.random.default_rng(5)
    mu = np.float32(0.125)
    state = {"sdf": rng.uniform(-1, 1, dims).astype(np.float32), "wt": rng.integers(1, 9, dims).astype(np.int32),
             "color": rng.integers(1, 256, dims + (3,)).astype(np.uint8),
             "hist": rng.integers(1, 9, dims + (32,)).astype(np.uint32),
             "cls": rng.integers(1, 9, dims).astype(np.int32), "cls_cnt": rng.integers(1, 9, dims).astype(np.int32)}
    got = S.numpy_shift(state, shift, mu)
    want = {k: np.zeros_like(v) for k, v in state.items()}
    want["sdf"][...] = mu
    for x in range(dims[0]):
        for y in range(dims[1]):
            for z in range(dims[2]):
                u = (x + shift[0], y + shift[1], z + shift[2])
                if all(0 <= u[a] < dims[a] for a in range(3)):
                    for k in state:
                        want[k][x, y, z] = state[k][u]
    for k in state:
        assert got[k].shape == state[k].shape and got[k].dtype == state[k].dtype, k
        assert np.array_equal(got[k].view(np.uint32) if k == "sdf" else got[k],
                              want[k].view(np.uint32) if k == "sdf" else want[k]), k
    # flat arrays, as Volume.download returns them
    flat = S.numpy_shift({k: v.reshape(-1) for k, v in state.items()}, shift, mu, dims=dims)
    for k in state:
        assert flat[k].ndim == 1 and np.array_equal(flat[k], got[k].reshape(-1)), k


def test_sequence_plans_shifts_on_two_axes():
    """The walking sequence of tests/test_gpu_shift.py, planned on the host: at least two shifts on
    two different axes, and a last focus outside the cube placed around frame 0."""
    import semtsdf

    semtsdf.load()
    st = S.sequence_stream()
    f0 = st.frame(0)
    p, shifts = S.plan_sequence(st, f0)
    assert len(shifts) >= 2, shifts
    axes = {a for _, s in shifts for a in range(3) if s[a]}
    assert len(axes) >= 2, shifts
    assert all(c % 8 == 0 for _, s in shifts for c in s)
    c2w = st.c2w(S.SEQ_FRAMES - 1)
    focus = c2w[:3, 3] + S.sequence_focus_depth(f0) * c2w[:3, 2]
    assert any(not (p.vol_start[a] <= focus[a] <= p.vol_end[a]) for a in range(3)), focus


def test_shift_is_exported_and_checks_its_arguments_without_a_device():
    from semtsdf import _lib as L

    lib = L.load()
    assert "semtsdf_shift" in L.SIGNATURES and hasattr(lib, "semtsdf_shift")
    assert lib.semtsdf_abi_version() == 12
    ok = (C.c_int32 * 3)(8, 0, -8)
    assert lib.semtsdf_shift(None, ok, None) == L.ERR_INVALID
    # the shift itself is checked before the handle is looked at: any non-null pointer will do
    fake = C.create_string_buffer(1 << 16)
    assert lib.semtsdf_shift(fake, None, None) == L.ERR_INVALID
    for bad in ((4, 0, 0), (0, -12, 0), (8, 8, 1), (1 << 20, 0, 0), (0, -(1 << 20), 0), (0, 0, (1 << 30))):
        assert lib.semtsdf_shift(fake, (C.c_int32 * 3)(*bad), None) == L.ERR_INVALID, bad
        assert lib.semtsdf_last_error()
