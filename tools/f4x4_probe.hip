// Probe of the gfx950 block-scaled MFMA with e2m1 (MX-FP4) operands on BOTH sides -- DESIGN.md 3zj (tools only; not part of
// libmcamd.so).  tools/f4_probe.hip pinned the 4-bit A operand; csrc/conv_q4_mx.hip depends on the same questions for B
// (blgp:4, four registers) with a per-lane B scale:
//  1. operand packing: is element e of B's lane (c, h) the nibble at bits [4 e, 4 e + 4) of its four registers (low nibble of
//     byte e / 2 first), and is it k = 32 h + e -- so that group h of A meets group h of B in one lane?  Scored against the exact
//     products of random e2m1 x e2m1 codes, both nibble orders of B.
//  2. scales: is B's e8m0 scale byte 0 of the lane's scale register (op_sel 0, bytes 1-3 ignored), one per (row, 32 k), applied
//     beside A's -- with DIFFERENT bytes per (row, half) on both sides?
// build + run:  hipcc --offload-arch=gfx950 -O3 -o tools/f4x4_probe tools/f4x4_probe.hip && ./tools/f4x4_probe
// measured (MI355X, one box): 1. B's lane (c, h) holds k = 32 h + e, low nibble first, as A's -- 0 mismatches of 1 024; with the
// high nibble first 1 023.  2. holds: with different scale bytes per (row, half) on both sides 0 mismatches (1 022 with the
// high nibble first).  Group h of A meets group h of B in one lane.  
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

// one wave: C[r][c] = sum_h 2^(SA[r][h] - 127) 2^(SB[c][h] - 127) sum_e A[r][32 h + e] B[c][32 h + e]; A, B: [32 rows][2 halves][16
// bytes] of e2m1 nibbles, SA, SB: [32 rows][2 halves] e8m0 bytes
__global__ void mfma4x4_kernel(const unsigned char* A, const unsigned char* B, const unsigned char* SA, const unsigned char* SB, float* C) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const i32x4_t a = *(const i32x4_t*)(A + (r * 2 + h) * 16);
    const i32x4_t b = *(const i32x4_t*)(B + (r * 2 + h) * 16);
    const int sa = SA[r * 2 + h] | 0x55aa3300;     // bytes 1-3 must not matter with op_sel 0
    const int sb = SB[r * 2 + h] | 0x33cc5500;
    f32x16_t acc;
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    asm volatile("s_nop 1\n\tv_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4 blgp:4\n\ts_nop 15\n\ts_nop 15"
                 : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(sb));
    for (int i = 0; i < 16; ++i) C[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[i];
}

static const float GRID[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
static float e2m1(int c) { return (c & 8) ? -GRID[c & 7] : GRID[c & 7]; }

int main() {
    // exact products (halves and small integers, 64 terms of at most 36: every partial sum is an fp32 number)
    std::vector<int> ca(32 * 64), cb(32 * 64);
    std::vector<unsigned char> pa(32 * 32), pb(32 * 32), sa(64), sb(64);
    srand(7);
    for (int i = 0; i < 32 * 64; ++i) {
        ca[i] = rand() % 16, cb[i] = rand() % 16;
        if (ca[i] == 8) ca[i] = 0;
        if (cb[i] == 8) cb[i] = 0;
    }
    for (int i = 0; i < 32 * 32; ++i) {                    // low nibble = the even element, on both sides
        pa[i] = (unsigned char)(ca[2 * i] | ca[2 * i + 1] << 4);
        pb[i] = (unsigned char)(cb[2 * i] | cb[2 * i + 1] << 4);
    }
    unsigned char *dA, *dB, *dSA, *dSB;
    float* dC;
    CK(hipMalloc(&dA, pa.size())); CK(hipMalloc(&dB, pb.size())); CK(hipMalloc(&dSA, 64)); CK(hipMalloc(&dSB, 64)); CK(hipMalloc(&dC, 4096));
    CK(hipMemcpy(dA, pa.data(), pa.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, pb.data(), pb.size(), hipMemcpyHostToDevice));
    for (int mode = 0; mode < 2; ++mode) {
        for (int i = 0; i < 64; ++i) {                     // (a narrow range: the instruction drops products far below the largest)
            sa[i] = (unsigned char)(mode ? 125 + rand() % 5 : 127);
            sb[i] = (unsigned char)(mode ? 124 + rand() % 5 : 127);
        }
        CK(hipMemcpy(dSA, sa.data(), 64, hipMemcpyHostToDevice));
        CK(hipMemcpy(dSB, sb.data(), 64, hipMemcpyHostToDevice));
        mfma4x4_kernel<<<1, 64>>>(dA, dB, dSA, dSB, dC);
        std::vector<float> C(1024);
        CK(hipMemcpy(C.data(), dC, 4096, hipMemcpyDeviceToHost));
        int bad[2] = {0, 0};
        for (int swap = 0; swap < 2; ++swap)               // B's nibble order -- 0: low nibble first (as packed), 1: high nibble first
            for (int r = 0; r < 32; ++r)
                for (int c = 0; c < 32; ++c) {
                    double s = 0.0;
                    for (int h = 0; h < 2; ++h) {
                        double sh = 0.0;
                        for (int e = 0; e < 32; ++e) sh += (double)e2m1(ca[r * 64 + 32 * h + e]) * e2m1(cb[c * 64 + 32 * h + (e ^ swap)]);
                        s += ldexp(sh, sa[r * 2 + h] - 127 + sb[c * 2 + h] - 127);
                    }
                    if (C[r * 32 + c] != (float)s) ++bad[swap];
                }
        printf("e2m1 x e2m1 32x32x64, B lane (c, h) = k [32 h, 32 h + 32), %s scales: mismatches of 1024 -- B low nibble first %d, high "
               "nibble first %d (C[0][0] = %g, C[5][7] = %g)\n", mode ? "per-(row, half) A and B" : "uniform (127)", bad[0], bad[1], C[0],
               C[5 * 32 + 7]);
    }
    return 0;
}
