// The 4-bit (e2m1 codes + group shifts) weight quantisation rule of the fp8 engine, stated once for every pass that applies it
// (conv_q8_w4.hip: the engine's packer; wpack.hip: the "w4" payload of a compressed model file).
#pragma once
#include "common.h"
#include "q8_exp.h"

// e4_f of a filter from max |w * mask|: the fp8 packers' exponent minus one, 0 for an all-zero filter
__device__ __forceinline__ int w4_filter_exponent(float amax) { return amax > 0.f ? q8_filter_exponent(amax) - 1 : 0; }

// Smallest integer g with amax <= 6 * 2^g for amax > 0 (0 for amax == 0), integer steps as q8_filter_exponent: (m, x) =
// frexp(amax), 6 * 2^g = 0.75 * 2^(g + 3), so g = x - 3 if m <= 0.75 else x - 2.  Unclamped: under it nothing saturates in
// w4_code.  The MXFP4 activation cast (conv_q4_mx.hip) uses it as it stands: g in [-11, 7] for e4m3 inputs.
__device__ __forceinline__ int w4_group_shift_free(float amax) {
    if (!(amax > 0.f)) return 0;
    int x;
    const float m = frexpf(amax, &x);
    return m <= 0.75f ? x - 3 : x - 2;
}

// ... clamped to the weight format's [-5, 6] (-5 for amax == 0)
__device__ __forceinline__ int w4_group_shift(float amax) {
    if (!(amax > 0.f)) return -5;
    const int g = w4_group_shift_free(amax);
    return g < -5 ? -5 : g > 6 ? 6 : g;
}

// s (the scaled weight) -> its 4-bit code under shift g: round to nearest onto the e2m1 grid, ties to the even mantissa bit
// (rintf on 2 v / v / v / 2: an even integer there is a code with mantissa bit 0); above 6 saturates; a zero magnitude
// carries no sign bit.
__device__ __forceinline__ unsigned w4_code(float s, int g) {
    const float v = fminf(ldexpf(fabsf(s), -g), 6.f);
    unsigned c;
    if (v < 2.f) c = (unsigned)rintf(2.f * v);               // 0, 0.5, 1, 1.5, (2)
    else if (v < 4.f) c = (unsigned)rintf(v) + 2u;           // 2, 3, (4)
    else c = (unsigned)rintf(0.5f * v) + 4u;                 // 4, 6
    return (c != 0u && s < 0.f) ? (c | 8u) : c;
}

// the grid magnitude of a code's low three bits: {0, 0.5, 1, 1.5} = m / 2, {2, 3, 4, 6} = (2 + m % 2) << (m - 4) / 2
__device__ __forceinline__ float w4_grid(unsigned m) {
    return m < 4u ? 0.5f * (float)m : (float)((2u + (m & 1u)) << ((m - 4u) >> 1));
}

// the value of an e4m3 byte's low seven bits, for the MXFP4 activation cast (the pass of conv_q4_mx.hip and the store of
// conv_epi.h); the NaN pattern 0x7f continues the format to 480 (mcamd.h)
__device__ __forceinline__ float a4_mag(unsigned b) {
    const unsigned e = (b >> 3) & 15u, m = b & 7u;
    return e ? ldexpf((float)(8u + m), (int)e - 10) : ldexpf((float)m, -9);
}
