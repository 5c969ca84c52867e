// Stand-alone check of the index rule of the brick paging calls (csrc/semtsdf_bricks.h): the runs of
// a brick, the place of a run's elements in the record and the real-voxel mask, expanded per voxel
// against tile_index's formula (restated here) and the definition -- place w = 64 (x & 7) +
// 8 (y & 7) + (z & 7), a voxel is real iff its index is below the dim on every axis -- on an
// exact-size heap array (so a sanitizer build sees any access outside the stored voxels), with every
// place of every brick named exactly once and every real voxel reached by exactly one brick.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../slam-maskrcnn_amd/csrc/semtsdf_bricks.h"

using namespace semtsdf;

// tile_index of semtsdf_internal.h in plain integer arithmetic
static uint32_t tile_index(uint32_t nuy, uint32_t nuz, int x, int y, int z) {
    const uint32_t ty = nuz * 256u, tx = nuy * ty;
    return (uint32_t)x * tx + (uint32_t)(y >> 3) * ty + (uint32_t)(y & 7) * 4u + (uint32_t)(z >> 5) * 256u +
           (uint32_t)((z >> 2) & 7) * 32u + (uint32_t)(z & 3);
}

int main() {
    const int dxs[] = {8, 11, 24}, dyz[] = {8, 12, 28, 32, 40, 72};
    long cases = 0, bricks = 0, voxels = 0, bad = 0, real = 0, masked = 0, ragged = 0;
    for (int dx : dxs) for (int dy : dyz) for (int dz : dyz) {
        const uint32_t nuy = (uint32_t)(dy + 7) / 8, nuz = (uint32_t)(dz + 31) / 32;
        const size_t nvox = (size_t)dx * nuy * nuz * 256u;
        const BrickGeom g{dx, dy, dz, nuy * nuz * 256u, nuz * 256u};
        std::vector<uint32_t> seen(nvox, 0u);  // times a stored element was named by a real voxel
        const int nb[3] = {(dx + 7) / 8, (dy + 7) / 8, (dz + 7) / 8};
        ++cases;
        for (int bx = 0; bx < nb[0]; ++bx) for (int by = 0; by < nb[1]; ++by) for (int bz = 0; bz < nb[2]; ++bz) {
            ++bricks;
            const bool rag = brick_ragged(g, bx, by, bz);
            ragged += rag;
            bool all_real = true;
            std::vector<int> place(kBrickVoxels, 0);
            for (int x = 0; x < kBrickRuns; ++x) {
                const bool exists = brick_run_exists(g, bx, x);
                if (exists != (8 * bx + x < dx)) ++bad;
                for (int e = 0; e < kBrickRunVoxels; ++e) {
                    ++voxels;
                    const int vx = 8 * bx + x, vy = 8 * by + brick_elem_y(e), vz = 8 * bz + brick_elem_z(e);
                    const int w = brick_place(x, e);
                    if (w < 0 || w >= kBrickVoxels) { ++bad; continue; }
                    ++place[w];
                    if (w != 64 * (vx & 7) + 8 * (vy & 7) + (vz & 7)) ++bad;
                    if (w / 64 != x) ++bad;  // the permutation stays inside the run's 64 words
                    const bool want_real = vx < dx && vy < dy && vz < dz;
                    if (brick_voxel_real(g, bx, by, bz, x, e) != want_real) ++bad;
                    all_real = all_real && want_real;
                    (want_real ? real : masked) += 1;
                    if (!exists) continue;  // no such run in the storage: never addressed
                    const uint32_t t = brick_run_start(g, bx, by, bz, x) + (uint32_t)e;
                    if (t != tile_index(nuy, nuz, vx, vy, vz)) ++bad;
                    if (want_real) ++seen.at(t);
                    else (void)seen.at(t);  // padding of an existing run is stored
                }
            }
            for (int c : place)
                if (c != 1) ++bad;
            if (rag == all_real) ++bad;  // ragged iff some voxel is not real
            if (brick_record_words(false, false, 0u) != 3u * 512u || brick_record_words(true, false, 0x80000001u) != 7u * 512u ||
                brick_record_words(true, true, 0u) != 7u * 512u || brick_record_words(false, false, 0xFFFFFFFFu) != 35u * 512u)
                ++bad;
        }
        for (int x = 0; x < dx; ++x) for (int y = 0; y < dy; ++y) for (int z = 0; z < dz; ++z)
            if (seen.at(tile_index(nuy, nuz, x, y, z)) != 1u) ++bad;
        long named = 0;
        for (uint32_t s : seen) named += s;
        if (named != (long)dx * dy * dz) ++bad;
    }
    printf("bricks %ld %ld %ld %ld %ld %ld %ld\n", cases, bricks, voxels, bad, real, masked, ragged);
    return bad ? 1 : 0;
}
