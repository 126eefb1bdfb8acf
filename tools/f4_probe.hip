// Probe of the gfx950 block-scaled MFMA with an e2m1 (MX-FP4) A operand against an e4m3 B operand -- DESIGN.md 3zg (tools
// only; not part of libmcamd.so).  Questions csrc/conv_q8_w4_mx.hip depends on:
//  1. operand packing: with cbsz:4 the A operand is four registers; is element e of lane (r, h) the nibble at bits
//     [4 e, 4 e + 4) (low nibble of byte e / 2 first), and which k is it -- against which k of the fp8 operand's eight
//     registers?  Scored against the exact products: both nibble orders, with the fp8 lane (c, h) loaded with the bytes
//     [16 h, 16 h + 16) and [32 + 16 h, + 16) of its row (SPLIT, what conv_q8_kernel reads) or with [32 h, 32 h + 32).
//  2. scales: is A's e8m0 scale byte 0 of the lane's scale register (op_sel 0, bytes 1-3 ignored), one per (row, 32 k)?
//  3. issue rate of the mixed fp4 x fp8 form against fp8 x fp8 and fp4 x fp4.
// build + run:  hipcc --offload-arch=gfx950 -O3 -o tools/f4_probe tools/f4_probe.hip && ./tools/f4_probe
// measured (MI355X, one box): 1. the fp4 lane (r, h) holds k = 32 h + e, low nibble first, and meets the SPLIT fp8 read -- 0
// mismatches of 1 024; with the fp8 lane holding [32 h, 32 h + 32) both nibble orders miss in > 1 020 (k [16, 32) and [32, 48)
// trade places).  2. holds.  3. e4m3 x e4m3 4 911, e2m1 x e4m3 4 974, e2m1 x e2m1 7 766 TFLOP/s: the mixed form runs at the
// fp8 rate.  
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

// one wave: C[32][32] = sum_k 2^(SA[r][k / 32] - 127) A[r][k] B[c][k]; A: [32 rows][2 halves][16 bytes] of e2m1 nibbles,
// B: [32 rows][64 bytes] e4m3, SA: [32 rows][2 halves] e8m0 bytes
__global__ void mfma4_kernel(const unsigned char* A, const unsigned char* B, const unsigned char* SA, float* C, int split) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const i32x4_t a = *(const i32x4_t*)(A + (r * 2 + h) * 16);
    const i32x4_t b0 = *(const i32x4_t*)(B + r * 64 + (split ? 16 * h : 32 * h));
    const i32x4_t b1 = *(const i32x4_t*)(B + r * 64 + (split ? 32 + 16 * h : 32 * h + 16));
    const i32x8_t b = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
    const int sa = SA[r * 2 + h] | 0x55aa3300;     // bytes 1-3 must not matter with op_sel 0
    const int sb = 127 * 0x01010101;
    f32x16_t acc;
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    asm volatile("s_nop 1\n\tv_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4\n\ts_nop 15\n\ts_nop 15"
                 : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(sb));
    for (int i = 0; i < 16; ++i) C[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[i];
}

// FMT 0: e4m3 x e4m3, 1: e2m1 x e4m3, 2: e2m1 x e2m1 (all 32x32x64 scaled); the operands are whole 8-register tuples, of which
// the instruction reads what its format needs
template <int FMT>
__global__ __launch_bounds__(256) void rate_kernel(float* out, int iters, int sa, int sb) {
    f32x16_t acc[4];
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    i32x8_t a, b;
    for (int i = 0; i < 8; ++i) { a[i] = 0x22222222 + (threadIdx.x & 1) * 0x11111111; b[i] = 0x30303030 + i; }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (FMT == 2) acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc[j], 4, 4, 0, sa, 0, sb);
            else if (FMT == 1) acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc[j], 4, 0, 0, sa, 0, sb);
            else acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc[j], 0, 0, 0, sa, 0, sb);
        }
    }
    float s = 0.f;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 16; ++i) s += acc[j][i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

static const float GRID[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
static float e2m1(int c) { return (c & 8) ? -GRID[c & 7] : GRID[c & 7]; }
static float e4m3(int b) {      // e4m3fn, finite codes only
    const int e = (b >> 3) & 15, m = b & 7;
    const float x = e == 0 ? ldexpf(m / 8.f, -6) : ldexpf(1.f + m / 8.f, e - 7);
    return (b & 0x80) ? -x : x;
}

int main() {
    // 1 + 2: exact products (small integers and halves: every partial sum is an fp32 number) with per-(row, half) scales
    const int bcodes[8] = {0x00, 0x38, 0xb8, 0x40, 0x44, 0xc8, 0x30, 0x4c};      // 0, 1, -1, 2, 3, -4, 0.5, 5
    std::vector<int> ca(32 * 64), cb(32 * 64);
    std::vector<unsigned char> pa(32 * 32), pb(32 * 64), sa(64);
    srand(4);
    for (int i = 0; i < 32 * 64; ++i) {
        ca[i] = rand() % 16;
        if (ca[i] == 8) ca[i] = 0;
        cb[i] = bcodes[rand() % 8];
        pb[i] = (unsigned char)cb[i];
    }
    for (int i = 0; i < 32 * 32; ++i) pa[i] = (unsigned char)(ca[2 * i] | ca[2 * i + 1] << 4);      // low nibble = the even element
    unsigned char *dA, *dB, *dSA;
    float* dC;
    CK(hipMalloc(&dA, pa.size())); CK(hipMalloc(&dB, pb.size())); CK(hipMalloc(&dSA, 64)); CK(hipMalloc(&dC, 4096));
    CK(hipMemcpy(dA, pa.data(), pa.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, pb.data(), pb.size(), hipMemcpyHostToDevice));
    for (int mode = 0; mode < 4; ++mode) {
        const int uniform = !(mode & 1), split = mode < 2;
        for (int i = 0; i < 64; ++i) sa[i] = (unsigned char)(uniform ? 127 : 125 + rand() % 5);       // (a narrow range: the
                                                                                       // instruction drops products far below the largest)
        CK(hipMemcpy(dSA, sa.data(), 64, hipMemcpyHostToDevice));
        mfma4_kernel<<<1, 64>>>(dA, dB, dSA, dC, split);
        std::vector<float> C(1024);
        CK(hipMemcpy(C.data(), dC, 4096, hipMemcpyDeviceToHost));
        int bad[2] = {0, 0};
        for (int swap = 0; swap < 2; ++swap)       // 0: low nibble first (as packed), 1: high nibble first
            for (int r = 0; r < 32; ++r)
                for (int c = 0; c < 32; ++c) {
                    double s = 0.0;
                    for (int h = 0; h < 2; ++h) {
                        double sh = 0.0;
                        for (int e = 0; e < 32; ++e) sh += (double)e2m1(ca[r * 64 + 32 * h + (e ^ swap)]) * e4m3(cb[c * 64 + 32 * h + e]);
                        s += ldexp(sh, sa[r * 2 + h] - 127);
                    }
                    if (C[r * 32 + c] != (float)s) ++bad[swap];
                }
        printf("e2m1 x e4m3 32x32x64, fp8 lane %s, %s A scales: mismatches of 1024 -- low nibble first %d, high nibble first %d (C[0][0] = %g, C[5][7] = %g)\n",
               split ? "split" : "contiguous", uniform ? "uniform (127)" : "per-(row, half)", bad[0], bad[1], C[0], C[5 * 32 + 7]);
    }

    // 3. issue rate: 1024 workgroups of 4 waves (4 per CU), 4 independent accumulators per wave
    float* dO;
    CK(hipMalloc(&dO, 1024 * 256 * 4));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const int iters = 20000;
    const char* names[3] = {"e4m3 x e4m3", "e2m1 x e4m3", "e2m1 x e2m1"};
    for (int fmt = 0; fmt < 3; ++fmt)
        for (int rep = 0; rep < 2; ++rep) {
            CK(hipEventRecord(e0));
            if (fmt == 2) rate_kernel<2><<<1024, 256>>>(dO, iters, 127 * 0x01010101, 126 * 0x01010101);
            else if (fmt == 1) rate_kernel<1><<<1024, 256>>>(dO, iters, 127 * 0x01010101, 122 * 0x01010101);
            else rate_kernel<0><<<1024, 256>>>(dO, iters, 115 * 0x01010101, 122 * 0x01010101);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            const double flop = 1024.0 * 4 * iters * 4 * 2.0 * 32 * 32 * 64;
            if (rep) printf("rate %s scaled 32x32x64: %.3f ms, %.1f TFLOP/s\n", names[fmt], ms, flop / ms * 1e-9);
        }
    return 0;
}
