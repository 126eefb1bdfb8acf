// The fp8 (e4m3) weight quantisation rule, stated once for every packer that applies it (conv_q8.hip, conv_q8_sparse.hip,
// wpack.hip).
#pragma once
#include "common.h"

// a = max |w * mask| of a filter, (m, x) = frexp(a): e = 9 - x if m <= 0.875 else 8 - x, so that a 2^e lies in (224, 448];
// e = 0 for an all-zero filter.  Integer steps only: the host emulation cannot disagree at a power of two.
__device__ __forceinline__ int q8_filter_exponent(float amax) {
    int e = 0;
    if (amax > 0.f) {
        int x;
        const float m = frexpf(amax, &x);
        e = m <= 0.875f ? 9 - x : 8 - x;
    }
    return e;
}

// the value whose e4m3 rounding is the weight's code: w * mask scaled by the filter's exponent, clamped to the format's range
// (the conversion returns NaN above its maximum)
__device__ __forceinline__ float q8_weight_scaled(float wm, int e) { return fminf(fmaxf(ldexpf(wm, e), -448.f), 448.f); }
