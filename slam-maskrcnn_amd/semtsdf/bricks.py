"""Paging bricks: what a shift pushes out of the volume is kept on the host and put back when the
camera returns.

Host code only.  Volume.pack_bricks / unpack_bricks (semtsdf_pack_bricks, semtsdf_unpack_bricks) move
the occupied 8^3 bricks of a box between the device and their records; BrickStore keeps records
under integer world brick coordinates; leaving_boxes / entering_boxes name the brick boxes a shift
vacates and uncovers; shift_paged ties them to Volume.shift.  World coordinates are integers kept
here (the sum of all shifts, in bricks): never derived from the f32 vol_start, which rounds once
per shift.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L

BRICK = 8
PLANE = L.BRICK_VOXELS  # words of one plane of a record


def popcount(bins: int) -> int:
    return bin(int(bins) & 0xFFFFFFFF).count("1")


def record_planes(flags: int, bins: int) -> int:
    """Planes of a record: sdf, weight, colour (1, or 3 for COLOR_I32), one per bin, cls and cls_cnt (VOTE)."""
    return 2 + (3 if flags & L.F_COLOR_I32 else 1) + popcount(bins) + (2 if flags & L.F_VOTE else 0)


def _axis_ranges(n: int, s: int):
    """(leave, keep): the brick ranges [a, b) of an axis of n bricks that a shift of s bricks vacates and keeps."""
    if s > 0:
        m = min(s, n)
        return (0, m), (m, n)
    if s < 0:
        m = max(n + s, 0)
        return (m, n), (0, m)
    return (0, 0), (0, n)


def leaving_boxes(nb, sb):
    """At most three disjoint brick boxes [(lo, hi)] covering the bricks that a shift of `sb` bricks
    pushes out of a volume of `nb` bricks: b leaves iff b - sb lies outside [0, nb) on some axis
    (semtsdf.follow.leaving, per brick)."""
    r = [_axis_ranges(int(nb[a]), int(sb[a])) for a in range(3)]
    (lx, kx), (ly, ky), (lz, _) = r
    whole = [(0, int(nb[a])) for a in range(3)]
    boxes = [(lx, whole[1], whole[2]), (kx, ly, whole[2]), (kx, ky, lz)]
    out = []
    for box in boxes:
        if all(b > a for a, b in box):
            out.append((tuple(a for a, _ in box), tuple(b for _, b in box)))
    return out


def entering_boxes(nb, sb):
    """The boxes of the shifted volume that hold nothing of the old one (the reset state): the mirror
    of leaving_boxes, b enters iff b + sb lies outside [0, nb) on some axis."""
    return leaving_boxes(nb, [-int(s) for s in sb])


class BrickStore:
    """Records of bricks outside the volume, keyed by world brick (origin + b).

    origin: three ints, the sum of all shifts so far divided by 8 (shift_paged advances it), so that
    the local brick b of the volume is the world brick origin + b."""

    def __init__(self):
        self.origin = [0, 0, 0]
        self.flags = None  # F_SEMANTIC | F_COLOR_I32 | F_VOTE of the volume the records came from (shift_paged)
        self._d = {}       # (wx, wy, wz) -> (bins, record u32 [planes * 512])

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        return tuple(int(k) for k in key) in self._d

    def keys(self):
        return sorted(self._d)

    def get(self, key):
        """(bins, record) of a world brick, or None."""
        return self._d.get(tuple(int(k) for k in key))

    @property
    def nbytes(self) -> int:
        """Host bytes held: the records, and 16 for the key and bins of each."""
        return sum(rec.nbytes + 16 for _, rec in self._d.values())

    def put(self, bricks, words):
        """Keeps the records of `bricks` (local coordinates, as Volume.pack_bricks returns them with
        `words`) under origin + b; a record already kept for a brick is replaced."""
        bricks = np.asarray(bricks, L.BRICK_DTYPE).reshape(-1)
        words = np.asarray(words, np.uint32).reshape(-1)
        if not bricks.size:
            return
        off = bricks["offset"].astype(np.int64)
        end = np.append(off[1:], words.size)
        if off[0] != 0 or (end < off).any() or ((end - off) % PLANE).any():
            raise ValueError("offsets are not the running sum of whole planes")
        o = np.asarray(self.origin, np.int64)
        for k in range(bricks.size):
            key = tuple(int(x) for x in o + bricks["b"][k])
            self._d[key] = (int(bricks["bins"][k]), words[off[k]:end[k]].copy())

    def take(self, lo, hi):
        """Removes and returns, as (bricks, words) in ascending local order, the kept records of the
        local brick box lo <= b < hi."""
        o = np.asarray(self.origin, np.int64)
        wlo, whi = o + np.asarray(lo, np.int64), o + np.asarray(hi, np.int64)
        found = sorted(k for k in self._d if all(wlo[a] <= k[a] < whi[a] for a in range(3)))
        bricks = np.zeros(len(found), L.BRICK_DTYPE)
        parts, at = [], 0
        for i, key in enumerate(found):
            bins, rec = self._d.pop(key)
            bricks[i] = (np.asarray(key, np.int64) - o, bins, at)
            parts.append(rec)
            at += rec.size
        return bricks, (np.concatenate(parts) if parts else np.zeros(0, np.uint32))

    def remap(self, lut):
        """The kept histograms through `lut` under the rule of semtsdf_remap_instances:
        hist'[j] = sum of hist[k] over lut[k] == j (modulo 2^32), bins recomputed, planes that
        become empty dropped."""
        lut = np.asarray(lut, np.int64).reshape(-1)
        if lut.size != L.MAX_OBJECTS or lut[0] != 0 or (lut < 0).any() or (lut >= L.MAX_OBJECTS).any():
            raise ValueError(f"lut must hold {L.MAX_OBJECTS} ids below {L.MAX_OBJECTS} with lut[0] == 0")
        for key, (bins, rec) in list(self._d.items()):
            if not bins:
                continue
            ks = [k for k in range(L.MAX_OBJECTS) if bins >> k & 1]
            planes = rec.reshape(-1, PLANE)
            tail = 2 if (self.flags or 0) & L.F_VOTE else 0
            h0 = planes.shape[0] - tail - len(ks)  # the histogram planes follow the colour
            new = {}
            for i, k in enumerate(ks):
                j = int(lut[k])
                new[j] = planes[h0 + i] + new[j] if j in new else planes[h0 + i].copy()  # u32: wraps
            kept = [j for j in sorted(new) if new[j].any()]
            nbins = sum(1 << j for j in kept)
            rows = [planes[:h0]] + [new[j][None] for j in kept] + [planes[planes.shape[0] - tail:]]
            self._d[key] = (nbins, np.concatenate(rows).reshape(-1).astype(np.uint32))

    def save(self, path: str):
        keys = self.keys()
        recs = [self._d[k] for k in keys]
        np.savez_compressed(path, origin=np.asarray(self.origin, np.int64),
                            flags=np.int64(-1 if self.flags is None else self.flags),
                            keys=np.asarray(keys, np.int64).reshape(-1, 3),
                            bins=np.asarray([b for b, _ in recs], np.uint32),
                            sizes=np.asarray([r.size for _, r in recs], np.int64),
                            words=np.concatenate([r for _, r in recs]) if recs else np.zeros(0, np.uint32))

    @classmethod
    def load(cls, path: str) -> "BrickStore":
        z = np.load(path if str(path).endswith(".npz") else str(path) + ".npz", allow_pickle=False)
        s = cls()
        s.origin = [int(x) for x in z["origin"]]
        s.flags = None if int(z["flags"]) < 0 else int(z["flags"])
        at = 0
        for key, bins, n in zip(z["keys"], z["bins"], z["sizes"]):
            s._d[tuple(int(x) for x in key)] = (int(bins), z["words"][at:at + int(n)].astype(np.uint32))
            at += int(n)
        return s


_FORM = L.F_SEMANTIC | L.F_COLOR_I32 | L.F_VOTE


def check_paged(vol, store: BrickStore) -> int:
    """Whether `vol` can page into `store`, before anything is touched: ValueError for dims that are not
    multiples of 8 or a store that holds records of another form.  Returns the volume's form flags."""
    dim = [int(d) for d in vol.local_dim]
    if any(d % BRICK for d in dim):
        raise ValueError(f"paging needs dims that are multiples of {BRICK} (a partial edge brick cannot hold a whole "
                         f"returning brick), got {tuple(dim)}")
    form = int(vol.params.flags) & _FORM
    if store.flags is not None and store.flags != form:
        raise ValueError("the store holds records of a volume of another form (semantic / colour / vote flags)")
    return form


def shift_paged(vol, store: BrickStore, shift):
    """Volume.shift with paging: the occupied bricks the shift pushes out go into `store`, and the
    bricks of the store that the shifted volume covers again come back.  In this order: pack the
    leaving boxes, put them, shift, advance store.origin, take the entering boxes, unpack them."""
    form = check_paged(vol, store)
    shift = [int(s) for s in shift]
    if any(s % BRICK for s in shift):
        raise ValueError(f"shift {tuple(shift)} is not a multiple of {BRICK} voxels")
    store.flags = form
    if not any(shift):
        return
    sb = [s // BRICK for s in shift]
    nb = vol.brick_counts()
    for lo, hi in leaving_boxes(nb, sb):
        store.put(*vol.pack_bricks(lo, hi))
    vol.shift(*shift)
    store.origin = [store.origin[a] + sb[a] for a in range(3)]
    for lo, hi in entering_boxes(nb, sb):
        bricks, words = store.take(lo, hi)
        if bricks.size:
            vol.unpack_bricks(bricks, words)
