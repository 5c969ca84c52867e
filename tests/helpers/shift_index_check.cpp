// Stand-alone check of the index rule of semtsdf_shift (csrc/semtsdf_shift.h): the destination-line
// -> source-line rule and its per-voxel mask, expanded per voxel through tile_index's formula
// (restated here), against the per-voxel definition -- voxel i holds what voxel i + s held, the
// reset state where i + s is outside the volume, and padding voxels hold the reset state -- on
// exact-size heap arrays (so a sanitizer build sees any access outside the stored voxels), with
// every stored index written exactly once.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../slam-maskrcnn_amd/csrc/semtsdf_shift.h"

using namespace semtsdf;

// tile_index of semtsdf_internal.h in plain integer arithmetic
static uint32_t tile_index(uint32_t nuy, uint32_t nuz, int x, int y, int z) {
    const uint32_t ty = nuz * 256u, tx = nuy * ty;
    return (uint32_t)x * tx + (uint32_t)(y >> 3) * ty + (uint32_t)(y & 7) * 4u + (uint32_t)(z >> 5) * 256u +
           (uint32_t)((z >> 2) & 7) * 32u + (uint32_t)(z & 3);
}

int main() {
    const int dxs[] = {8, 11, 24}, dys[] = {8, 13, 28}, dzs[] = {32, 37, 72};
    const int sh[] = {0, 8, -8, 16, -16, 32, -32, 80, -80};
    const uint32_t kFill = 0xFFFFFFFFu;
    long cases = 0, lines = 0, voxels = 0, bad = 0, copied = 0, masked = 0;
    for (int dx : dxs) for (int dy : dys) for (int dz : dzs) {
        const uint32_t nuy = (uint32_t)(dy + 7) / 8, nuz = (uint32_t)(dz + 31) / 32;
        const uint32_t nlines = (uint32_t)dx * nuy * nuz * 8u;
        const size_t nvox = (size_t)nlines * kLineVoxels;
        // the source: a distinct value per real voxel, the reset state in the padding
        std::vector<uint32_t> src(nvox, kFill), dst(nvox), written(nvox);
        for (int x = 0; x < dx; ++x) for (int y = 0; y < dy; ++y) for (int z = 0; z < dz; ++z) {
            const uint32_t t = tile_index(nuy, nuz, x, y, z);
            src.at(t) = t;
        }
        for (int sx : sh) for (int sy : sh) for (int sz : sh) {
            const ShiftGeom g{dx, dy, dz, (int)nuy, (int)nuz * 8, sx, sy, sz};
            std::fill(written.begin(), written.end(), 0u);
            ++cases;
            for (uint32_t l = 0; l < nlines; ++l) {
                const ShiftLine c = shift_line_coords(g, l);
                const int64_t sl = shift_source_line(g, c);
                const bool whole = sl >= 0 && shift_line_whole(g, c);
                ++lines;
                if (sl >= (int64_t)nlines) { ++bad; continue; }
                for (int w = 0; w < kLineVoxels; ++w) {
                    // the rule: what the kernel stores at element 32 l + w
                    const bool kept = sl >= 0 && (whole || shift_voxel_kept(g, c, w));
                    const uint32_t got = kept ? src.at((size_t)sl * kLineVoxels + w) : kFill;
                    // the definition, through tile_index
                    const int x = c.x, y = c.gy * 8 + (w >> 2), z = c.q * 4 + (w & 3);
                    const uint32_t t = tile_index(nuy, nuz, x, y, z);
                    if (t != l * kLineVoxels + (uint32_t)w) ++bad;
                    const bool real = x < dx && y < dy && z < dz;
                    const int ux = x + sx, uy = y + sy, uz = z + sz;
                    const bool inside = ux >= 0 && ux < dx && uy >= 0 && uy < dy && uz >= 0 && uz < dz;
                    const uint32_t want = real && inside ? tile_index(nuy, nuz, ux, uy, uz) : kFill;
                    if (got != want) ++bad;
                    if (whole && !(real && inside)) ++bad;
                    dst.at(t) = got;
                    ++written.at(t);
                    ++voxels;
                    (kept ? copied : masked) += 1;
                }
            }
            for (uint32_t wr : written)
                if (wr != 1u) ++bad;
        }
    }
    printf("shift %ld %ld %ld %ld %ld %ld\n", cases, lines, voxels, bad, copied, masked);
    return bad ? 1 : 0;
}
