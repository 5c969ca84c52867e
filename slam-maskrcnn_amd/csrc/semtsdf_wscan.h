// Host-side scan of uploaded weights (semtsdf_upload): their upper bound and whether uint16
// storage holds every value.  No device dependency, so it can be built and run on its own.
#pragma once
#include <stdint.h>

namespace semtsdf {

constexpr int64_t kNarrowWeightMax = 65535;  // largest weight uint16 storage holds

struct WeightScan {
    int64_t wmax;   // max(0, every value): the upper bound integrate_impl counts on from
    bool fits_u16;  // every value lies in [0, kNarrowWeightMax]
};

inline WeightScan scan_weights(const int32_t* wt, uint64_t n) {
    WeightScan r{0, true};
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t w = wt[i];
        if (w > r.wmax) r.wmax = w;
        if (w < 0 || w > kNarrowWeightMax) r.fits_u16 = false;
    }
    return r;
}

}  // namespace semtsdf
