// The index rule of semtsdf_shift: which stored line a destination line of the tiled layout is
// gathered from when the volume moves by whole 8^3 bricks, and which voxels of it are kept.
//
// A line is the 1 x 8 x 4 (x, y, z) voxels that tile_index (semtsdf_internal.h) stores as 32
// consecutive elements: x, the y-group gy = y >> 3 and the z-quad q = z >> 2 name it, and line
// l = (x * nuy + gy) * nq + q starts at element 32 l (nq = 8 * nuz quads per column).  Inside a
// line voxel w = 4 (y & 7) + (z & 3).  A shift by multiples of 8 voxels moves y by whole groups and
// z by whole quads, so every voxel keeps its place w and the source of a destination line is one
// line, or nothing.
//
// Device code under HIP; plain C++ otherwise (`SEMTSDF_HD` is then empty), so the CPU test
// (tests/test_shift_index.py) compiles this header with g++.
#pragma once
#include <stdint.h>

#ifndef SEMTSDF_HD
#if defined(__HIPCC__)
#define SEMTSDF_HD __device__
#else
#define SEMTSDF_HD
#endif
#endif

namespace semtsdf {

constexpr int kShiftBrick = 8;         // shifts are multiples of the empty-space map's brick
constexpr int kShiftLimit = 1 << 20;   // |shift| stays below this on every axis
constexpr int kLineVoxels = 32;        // voxels of a line

struct ShiftGeom {
    int dimx, dimy, dimz;  // real voxels per axis (z: the stored planes of an unsharded handle)
    int nuy, nq;           // y-groups and z-quads per column of the storage, padding included
    int sx, sy, sz;        // the shift in voxels: destination i holds what source i + s held
};

struct ShiftLine {
    int x, gy, q;
};

SEMTSDF_HD inline ShiftLine shift_line_coords(const ShiftGeom& g, uint32_t line) {
    ShiftLine c;
    c.q = (int)(line % (uint32_t)g.nq);
    const uint32_t col = line / (uint32_t)g.nq;
    c.gy = (int)(col % (uint32_t)g.nuy);
    c.x = (int)(col / (uint32_t)g.nuy);
    return c;
}

// The source line of destination line c, or -1 ("outside"): no voxel of the destination line has
// a source inside the volume, so the whole line takes the fill value.
SEMTSDF_HD inline int64_t shift_source_line(const ShiftGeom& g, const ShiftLine& c) {
    const int x = c.x + g.sx, gy = c.gy + g.sy / kShiftBrick, q = c.q + g.sz / 4;
    if (x < 0 || x >= g.dimx || gy < 0 || gy >= g.nuy || q < 0 || q >= g.nq) return -1;
    // lines that hold nothing but z padding, on either side
    if (c.q * 4 >= g.dimz || q * 4 >= g.dimz) return -1;
    return ((int64_t)x * g.nuy + gy) * g.nq + q;
}

// Voxel w of destination line c (whose source line exists) keeps the source's value iff it is a
// real voxel and so is its source; otherwise it takes the fill value (the last y-group and the
// last z-tile mix real and padding voxels when the dims are ragged).
SEMTSDF_HD inline bool shift_voxel_kept(const ShiftGeom& g, const ShiftLine& c, int w) {
    const int y = c.gy * 8 + (w >> 2), z = c.q * 4 + (w & 3);
    return y < g.dimy && z < g.dimz && y + g.sy >= 0 && y + g.sy < g.dimy && z + g.sz >= 0 && z + g.sz < g.dimz;
}

// Every voxel of destination line c is kept: the line is copied as it is.
SEMTSDF_HD inline bool shift_line_whole(const ShiftGeom& g, const ShiftLine& c) {
    return shift_voxel_kept(g, c, 0) && shift_voxel_kept(g, c, kLineVoxels - 1);
}

}  // namespace semtsdf
