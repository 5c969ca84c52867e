// The marches' repeated `t += step`, done in O(1) per binade of t and bit-identical to the
// single additions.  The hit position of a ray depends on the exact sequence of rounded
// additions, and the sharded march replays sample positions from counts alone, so every
// place that advances t by more than one sample goes through the one routine below.
//
// Device code under HIP; plain C++ otherwise (`SEMTSDF_HD` is then empty), so the CPU test
// (tests/test_march_steps.py) compiles this header with g++.  Requires -ffp-contract=off.
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__)
#define SEMTSDF_HD __device__
#else
#define SEMTSDF_HD
#endif

// Estimate of 1 / d for the closed form's count.  Only an estimate: the count is fixed up
// exactly in both directions, so the result does not depend on it (the test biases it).
#ifndef SEMTSDF_STEPS_RCP
#if defined(__HIPCC__)
#define SEMTSDF_STEPS_RCP(d) __builtin_amdgcn_rcpf(d)
#else
#define SEMTSDF_STEPS_RCP(d) (1.0f / (d))
#endif
#endif

namespace semtsdf {

// Up to nmax additions of step to t (t > 0, step > 0) while t < tend; BOUNDED = false: no
// count limit (nmax is ignored and costs nothing).  Returns the number of additions; after
// one or more, t_prev is the value before the last one (else it is left alone).
//
// Inside a binade [2^e, 2^(e+1)) every t is a multiple of its ulp, so RN(t + step) = t + d
// with the same d = RN_ulp(step) for every t there (unless step is an exact tie between two
// multiples of the ulp, which takes single steps), and t + m d is exact while it stays below
// 2^(e+1).  The addition that crosses into the next binade is done singly.
template <bool BOUNDED>
SEMTSDF_HD inline int skip_steps(float& t, float& t_prev, float step, float tend, int nmax = 0) {
    int n = 0;
    while (t < tend && (!BOUNDED || n < nmax)) {
        const float t1 = t + step;
        // one more sample ends the run: a shortcut of the march's (the general path below takes
        // the same single step; the replays have no end and do without the extra exit)
        if (!BOUNDED && !(t1 < tend)) {
            t_prev = t;
            t = t1;
            ++n;
            break;
        }
        uint32_t tb;
        memcpy(&tb, &t, 4);
        const uint32_t eb = tb & 0x7F800000u, ub = eb - (23u << 23), pb = eb + (1u << 23);
        float ulp, top;
        memcpy(&ulp, &ub, 4);
        memcpy(&top, &pb, 4);
        const float d = t1 - t;  // exact (t1 within a factor 2 of t)
        const float lim = fminf(tend, top);
        int m = 0;  // additions of the closed form (0: a single step)
        if (fabsf(step - d) * 2.0f != ulp && t1 < top) {
            const int cap = BOUNDED ? nmax - n : 0;
            m = (int)((lim - t) * SEMTSDF_STEPS_RCP(d));  // estimate, fixed up exactly below
            m = m < 1 ? 1 : m;
            if (BOUNDED) m = m < cap ? m : cap;
            while (m > 1 && !(t + (float)m * d < lim)) --m;
            while ((!BOUNDED || m < cap) && t + (float)(m + 1) * d < lim) ++m;
        }
        if (m <= 1) {  // a tie, or the next addition leaves the binade: single step
            t_prev = t;
            t = t1;
            ++n;
            continue;
        }
        t_prev = t + (float)(m - 1) * d;
        t = t + (float)m * d;
        n += m;
    }
    return n;
}

// Sample position of the sharded march: t0 + vx added ncoarse times, then vx / 4 added nfine
// times (counts <= 0 add nothing), with the same rounded additions as the single-volume march.
SEMTSDF_HD inline float replay_t(float t, int ncoarse, int nfine, float vx) {
    float tp;
    skip_steps<true>(t, tp, vx, INFINITY, ncoarse);
    skip_steps<true>(t, tp, vx / 4.0f, INFINITY, nfine);
    return t;
}

}  // namespace semtsdf
