// The index rule of semtsdf_pack_bricks / semtsdf_unpack_bricks: where the 8^3 voxels of a brick
// lie in the tiled layout, which of them are real, and how many words its record has.
//
// Brick b = (bx, by, bz) holds the voxels 8 b[a] <= i[a] < 8 b[a] + 8.  In the tiled layout
// (tile_index, semtsdf_internal.h) it is 8 runs, one per x, of 64 consecutive elements each: the
// y-group of the brick is by, and its z-quads 2 bz and 2 bz + 1 are adjacent inside z-tile bz >> 2.
// Run x starts at element (8 bx + x) * tx + by * ty + (bz >> 2) * 256 + (bz & 3) * 64, and element e
// of it is the voxel (x, y, z) = (x, (e >> 2) & 7, 4 (e >> 5) + (e & 3)) of the brick, whose place in
// the brick's record is w = 64 x + 8 y + z.  The permutation from e to w stays inside the 64 words
// (256 B) of the run.
//
// Host and device code under HIP (the host validates an unpack with the words-per-record rule);
// plain C++ otherwise (`SEMTSDF_BHD` is then empty), so the CPU test
// (tests/test_bricks_index.py) compiles this header with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SEMTSDF_BHD __host__ __device__
#else
#define SEMTSDF_BHD
#endif

namespace semtsdf {

constexpr int kBrick = 8;             // voxels per axis of a brick
constexpr int kBrickRuns = 8;         // runs of a brick: one per x
constexpr int kBrickRunVoxels = 64;   // elements of a run
constexpr int kBrickVoxels = 512;     // words of one plane of a record

struct BrickGeom {
    int dimx, dimy, dimz;  // real voxels per axis (z: the stored planes of an unsharded handle)
    uint32_t tx, ty;       // VolGeom::tx, ty
};

// First element of run x (0..7) of brick (bx, by, bz).  The run exists iff 8 bx + x < dimx: the
// storage has no x layers past the last real one, while y and z are padded to whole tiles.
SEMTSDF_BHD inline uint32_t brick_run_start(const BrickGeom& g, int bx, int by, int bz, int x) {
    return (uint32_t)(kBrick * bx + x) * g.tx + (uint32_t)by * g.ty + (uint32_t)(bz >> 2) * 256u +
           (uint32_t)(bz & 3) * 64u;
}
SEMTSDF_BHD inline bool brick_run_exists(const BrickGeom& g, int bx, int x) { return kBrick * bx + x < g.dimx; }

// Element e (0..63) of a run: its voxel inside the brick, and its place in the record.
SEMTSDF_BHD inline int brick_elem_y(int e) { return (e >> 2) & 7; }
SEMTSDF_BHD inline int brick_elem_z(int e) { return 4 * (e >> 5) + (e & 3); }
SEMTSDF_BHD inline int brick_place(int x, int e) { return 64 * x + 8 * brick_elem_y(e) + brick_elem_z(e); }

// The brick reaches past a dim: some of its voxels are not real (padding, or a run that does not exist).
SEMTSDF_BHD inline bool brick_ragged(const BrickGeom& g, int bx, int by, int bz) {
    return kBrick * bx + kBrick > g.dimx || kBrick * by + kBrick > g.dimy || kBrick * bz + kBrick > g.dimz;
}

// Element e of run x of the brick is a real voxel.
SEMTSDF_BHD inline bool brick_voxel_real(const BrickGeom& g, int bx, int by, int bz, int x, int e) {
    return kBrick * bx + x < g.dimx && kBrick * by + brick_elem_y(e) < g.dimy && kBrick * bz + brick_elem_z(e) < g.dimz;
}

// Planes of a record: sdf, weight, colour (1 packed, or 3 for a COLOR_I32 volume), one per set bit of
// bins, cls and cls_cnt for a VOTE volume.  A record has 512 words per plane.
SEMTSDF_BHD inline int brick_record_planes(bool color_i32, bool vote, uint32_t bins) {
    int n = 0;
    for (uint32_t m = bins; m; m &= m - 1) ++n;
    return 2 + (color_i32 ? 3 : 1) + n + (vote ? 2 : 0);
}
SEMTSDF_BHD inline uint64_t brick_record_words(bool color_i32, bool vote, uint32_t bins) {
    return (uint64_t)kBrickVoxels * (uint64_t)brick_record_planes(color_i32, vote, bins);
}

}  // namespace semtsdf
