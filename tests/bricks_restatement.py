"""The definition semtsdf_pack_bricks / semtsdf_unpack_bricks and the paged follow are held to, in
NumPy on the reference layouts.

numpy_pack: the occupied bricks of a brick box and their records, by slicing: a brick is the
8 x 8 x 8 block of the arrays padded with the reset state, a record its planes flattened in C order
(place w = 64 x + 8 y + z).  numpy_unpack: the inverse, writing real voxels only.  Canvas: the model
of paging -- the volume is a window on a larger array that keeps what leaves."""
import numpy as np

F_SEMANTIC, F_COLOR_I32, F_VOTE = 0x1, 0x4, 0x8
BRICK_DTYPE = np.dtype([("b", np.int32, 3), ("bins", np.uint32), ("offset", np.uint64)])
CHANNELS = {"sdf": 1, "wt": 1, "color": 3, "hist": 32, "cls": 1, "cls_cnt": 1}
KEYS = ("sdf", "wt", "color", "hist", "cls", "cls_cnt")


def mu_bits(mu):
    return np.float32(mu).view(np.uint32)


def shaped(state, dims):
    """The arrays of `state` (flat, as Volume.download returns them, or shaped) as [dims + (channels,)]."""
    dims = tuple(int(d) for d in dims)
    return {k: np.asarray(a).reshape(dims + (CHANNELS[k],)) for k, a in state.items()}


def reset_state(dims, flags, mu):
    dims = tuple(int(d) for d in dims)
    s = {"sdf": np.full(dims, np.float32(mu), np.float32), "wt": np.zeros(dims, np.int32),
         "color": np.zeros(dims + (3,), np.int32 if flags & F_COLOR_I32 else np.uint8)}
    if flags & F_SEMANTIC:
        s["hist"] = np.zeros(dims + (32,), np.uint32)
    if flags & F_VOTE:
        s["cls"] = np.zeros(dims, np.int32)
        s["cls_cnt"] = np.zeros(dims, np.int32)
    return s


def brick_counts(dims):
    return tuple((int(d) + 7) // 8 for d in dims)


def _planes(st, flags, sl):
    """(planes before the histogram, histogram [8, 8, 8, 32] or None, planes after it) of the block sl, as u32."""
    head = [st["sdf"][sl][..., 0].view(np.uint32), st["wt"][sl][..., 0].astype(np.int32).view(np.uint32)]
    c = st["color"][sl]
    if flags & F_COLOR_I32:
        head += [c[..., i].astype(np.int32).view(np.uint32) for i in range(3)]
    else:
        c = c.astype(np.uint32)
        head.append(c[..., 0] | c[..., 1] << 8 | c[..., 2] << 16)
    hist = st["hist"][sl] if flags & F_SEMANTIC else None
    tail = [st[k][sl][..., 0].astype(np.int32).view(np.uint32) for k in ("cls", "cls_cnt")] if flags & F_VOTE else []
    return head, hist, tail


def _padded(state, dims, flags, mu):
    """The shaped state padded with the reset state to whole bricks."""
    nb = brick_counts(dims)
    full = reset_state([8 * n for n in nb], flags, mu)
    st = shaped(state, dims)
    for k in full:
        full[k] = full[k].reshape(full[k].shape[:3] + (CHANNELS[k],))
        full[k][:dims[0], :dims[1], :dims[2]] = st[k]
    return full


def numpy_pack(state, dims, flags, mu, lo=None, hi=None):
    """(bricks, words) of the brick box lo <= b < hi (default: the whole volume) of `state`."""
    dims = tuple(int(d) for d in dims)
    nb = brick_counts(dims)
    lo = (0, 0, 0) if lo is None else tuple(int(x) for x in lo)
    hi = nb if hi is None else tuple(int(x) for x in hi)
    full = _padded(state, dims, flags, mu)
    bricks, parts, at = [], [], 0
    for bx in range(lo[0], hi[0]):
        for by in range(lo[1], hi[1]):
            for bz in range(lo[2], hi[2]):
                sl = (slice(8 * bx, 8 * bx + 8), slice(8 * by, 8 * by + 8), slice(8 * bz, 8 * bz + 8))
                head, hist, tail = _planes(full, flags, sl)
                occupied = (head[0] != mu_bits(mu)).any() or any(p.any() for p in head[1:] + tail)
                bins, hp = 0, []
                if hist is not None:
                    for k in range(32):
                        if hist[..., k].any():
                            bins |= 1 << k
                            hp.append(hist[..., k])
                    occupied = occupied or bins != 0
                if not occupied:
                    continue
                rec = np.concatenate([p.reshape(-1) for p in head + hp + tail]).astype(np.uint32)
                bricks.append(((bx, by, bz), bins, at))
                parts.append(rec)
                at += rec.size
    b = np.zeros(len(bricks), BRICK_DTYPE)
    for i, e in enumerate(bricks):
        b[i] = e
    return b, (np.concatenate(parts) if parts else np.zeros(0, np.uint32))


def numpy_unpack(state, dims, flags, mu, bricks, words, inplace=False):
    """`state` with the real voxels of the listed bricks overwritten by their records: a new dict of
    shaped arrays, the input left unchanged (inplace: the shaped input arrays themselves)."""
    dims = tuple(int(d) for d in dims)
    out = {k: a if inplace else a.copy() for k, a in shaped(state, dims).items()}
    ncol = 3 if flags & F_COLOR_I32 else 1
    for e in np.asarray(bricks).reshape(-1):
        bx, by, bz = (int(x) for x in e["b"])
        bins, at = int(e["bins"]), int(e["offset"])
        nx, ny, nz = (min(8, dims[a] - 8 * b) for a, b in enumerate((bx, by, bz)))
        dst = (slice(8 * bx, 8 * bx + nx), slice(8 * by, 8 * by + ny), slice(8 * bz, 8 * bz + nz))

        def plane(i):
            return words[at + 512 * i: at + 512 * (i + 1)].reshape(8, 8, 8)[:nx, :ny, :nz]

        out["sdf"][dst + (0,)] = plane(0).view(np.float32)
        out["wt"][dst + (0,)] = plane(1).view(np.int32)
        if flags & F_COLOR_I32:
            for i in range(3):
                out["color"][dst + (i,)] = plane(2 + i).view(np.int32)
        else:
            for i in range(3):
                out["color"][dst + (i,)] = (plane(2) >> (8 * i)) & 0xFF
        i = 2 + ncol
        if flags & F_SEMANTIC:
            for k in range(32):
                if bins >> k & 1:
                    out["hist"][dst + (k,)] = plane(i)
                    i += 1
                else:
                    out["hist"][dst + (k,)] = 0
        if flags & F_VOTE:
            out["cls"][dst + (0,)] = plane(i).view(np.int32)
            out["cls_cnt"][dst + (0,)] = plane(i + 1).view(np.int32)
    return out


def states_equal(a, b, dims):
    a, b = shaped(a, dims), shaped(b, dims)
    if sorted(a) != sorted(b):
        return False
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in a)


class Canvas:
    """The model of paging.  The world is an array of dims + 2 * margin voxels per axis, the reset state
    outside what was ever seen; the volume is the window of `dims` voxels at margin + 8 * origin.  A
    shift writes the window back into the world and moves it: nothing that leaves is lost."""

    def __init__(self, state, dims, flags, mu, margin=32):
        self.dims, self.flags, self.mu, self.margin = tuple(int(d) for d in dims), flags, mu, int(margin)
        self.world = reset_state([d + 2 * self.margin for d in self.dims], flags, mu)
        self.world = shaped(self.world, [d + 2 * self.margin for d in self.dims])
        self.origin = [0, 0, 0]  # bricks
        self.write(state)

    def _slices(self):
        return tuple(slice(self.margin + 8 * o, self.margin + 8 * o + d) for o, d in zip(self.origin, self.dims))

    def write(self, state):
        sl = self._slices()
        for k, a in shaped(state, self.dims).items():
            self.world[k][sl] = a

    def window(self):
        sl = self._slices()
        return {k: a[sl].copy() for k, a in self.world.items()}

    def shift(self, shift, state=None):
        """Moves the window by `shift` voxels; `state`, if given, is what the window holds now."""
        if state is not None:
            self.write(state)
        self.origin = [o + int(s) // 8 for o, s in zip(self.origin, shift)]
        assert all(0 <= self.margin + 8 * o and self.margin + 8 * o + d <= d + 2 * self.margin
                   for o, d in zip(self.origin, self.dims)), "the walk leaves the canvas"
        return self.window()


def rebuild_world(window, store_items, origin, dims, flags, mu, margin=32):
    """The world a window and a store stand for: the reset state, the store's records at their world
    bricks, the window at `origin` (bricks).  store_items: (world brick, bins, record) triples."""
    dims = tuple(int(d) for d in dims)
    wd = [d + 2 * margin for d in dims]
    world = shaped(reset_state(wd, flags, mu), wd)
    for key, bins, rec in store_items:
        b = np.zeros(1, BRICK_DTYPE)
        b[0] = ([margin // 8 + int(k) for k in key], bins, 0)
        numpy_unpack(world, wd, flags, mu, b, rec, inplace=True)
    sl = tuple(slice(margin + 8 * o, margin + 8 * o + d) for o, d in zip(origin, dims))
    for k, a in shaped(window, dims).items():
        world[k][sl] = a
    return world
