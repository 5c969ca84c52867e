// Stand-alone check of the host-side weight scan of semtsdf_upload (csrc/semtsdf_wscan.h): the
// upper bound and the uint16 decision against a plain restatement, on exact-size heap arrays (so a
// sanitizer build sees any read outside [0, n)), n = 0 included, at the int32 extremes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../slam-maskrcnn_amd/csrc/semtsdf_wscan.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

int main() {
    const int32_t edge[] = {0, 1, 65534, 65535, 65536, 65537, -1, INT32_MIN, INT32_MAX, 1 << 23};
    long cases = 0, bad = 0, narrow = 0, wide = 0;
    for (int n = 0; n <= 70; ++n) {
        for (int rep = 0; rep < 300; ++rep) {
            std::vector<int32_t> w((size_t)n);
            const int mode = rep % 3;  // 0: all in range, 1: one edge value somewhere, 2: anything
            for (auto& x : w) x = (int32_t)(mode == 2 ? rnd() : rnd() % 65536u);
            if (mode == 1 && n > 0) w[rnd() % (uint32_t)n] = edge[rnd() % (sizeof(edge) / sizeof(edge[0]))];
            int64_t wmax = 0;
            bool fits = true;
            for (int32_t x : w) {
                if ((int64_t)x > wmax) wmax = x;
                if (x < 0 || x > 65535) fits = false;
            }
            const semtsdf::WeightScan r = semtsdf::scan_weights(n ? w.data() : nullptr, (uint64_t)n);
            ++cases;
            if (r.wmax != wmax || r.fits_u16 != fits) ++bad;
            (fits ? narrow : wide) += 1;
        }
    }
    printf("scan %ld %ld %ld %ld\n", cases, bad, narrow, wide);
    return bad ? 1 : 0;
}
