// Probe of the gfx950 2:4 sparse fp8 MFMA for the sparse fp8 forward (tools only; not part of libmcamd.so):
//  1. operand and index layout of v_smfmac_f32_32x32x64_fp8_fp8.  Hypothesis checked exactly on integer data, lane
//     l = (r, h), r = l & 31, h = l >> 5:
//     A (sparse, 4 VGPRs): row r, the dense k range [32 h, 32 h + 32) compressed to 16 kept bytes; kept byte j lies in the
//       group of 4 k's [32 h + 4 (j / 2), +4) at offset bits [2 j, 2 j + 2) of the 32-bit index VGPR;
//     B (dense, 8 VGPRs): column r, byte e = k 32 (e >> 4) + 16 h + (e & 15) -- the B fragment of the dense 32x32x64 form;
//     C: the 32x32 accumulator of the dense form.
//     Then a one-hot dump prints which B byte each (kept byte, index) pair meets, so that another layout can be read off.
//  2. what the instruction keeps of small products beside a large one (the experiment of DESIGN.md 3i): one product of
//     2^16 in kept slot 0 of row 0, cancelled by the accumulator input, and ONE product 2^j in kept slot s; per slot the
//     smallest j that still arrives whole.  Slots that stop early share the large product's group; 16 - j_min + 1 is the
//     number of bits kept below the group's largest product.
//  3. issue rate against v_smfmac_f32_32x32x32_f16 and the dense block-scaled fp8 MFMA (dense-equivalent FLOP).
// build + run:  hipcc --offload-arch=gfx950 -O3 -o tools/smfmac_f8_probe tools/smfmac_f8_probe.hip && ./tools/smfmac_f8_probe
// measured (MI355X): layout as stated, 0 mismatches; beside 2^16 a product in kept slots 1-7 arrives whole down
// to 2^3 and is gone at 2^2, in slots 8-15 down to 2^-8 (fp32's own limit beside 2^16), in the other lane half down to 2^-12
// (the smallest tried); of 31 products 2^j, 31 arrive for j >= 3 and 24 below: groups of 8 products, 14 bits kept below the
// group's largest -- as the dense fp8 MFMAs.  8 484 TFLOP/s dense-equivalent (~38 cycles per instruction) against 3 740
// (~43) for the fp16 sparse form and 4 847 (~66) for the dense block-scaled fp8 form on constant data
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <vector>

typedef _Float16 half_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(8))) _Float16 h8_t;
typedef __attribute__((ext_vector_type(16))) _Float16 h16_t;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

// one wave.  Ac: [64 lanes][16] kept bytes, Bl: [64 lanes][32] bytes, idx: [64] index VGPRs, Cin / C: [32][32]
__global__ void smfmac_kernel(const unsigned char* Ac, const unsigned char* Bl, const int* idx, const float* Cin, float* C) {
    const int lane = threadIdx.x, h = lane >> 5;
    const i32x4_t a = *(const i32x4_t*)(Ac + lane * 16);
    const i32x4_t b0 = *(const i32x4_t*)(Bl + lane * 32), b1 = *(const i32x4_t*)(Bl + lane * 32 + 16);
    const i32x8_t b = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
    f32x16_t acc;
    for (int i = 0; i < 16; ++i) acc[i] = Cin[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + (lane & 31)];
    acc = __builtin_amdgcn_smfmac_f32_32x32x64_fp8_fp8(a, b, acc, idx[lane], 0, 0);
    for (int i = 0; i < 16; ++i) C[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + (lane & 31)] = acc[i];
}

template <int KIND>
__global__ __launch_bounds__(256) void rate_kernel(float* out, int iters) {
    f32x16_t acc[4];
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    i32x4_t a4;
    i32x8_t a8, b8;
    for (int i = 0; i < 4; ++i) a4[i] = 0x38383838 + threadIdx.x;
    for (int i = 0; i < 8; ++i) { a8[i] = 0x38383838 + threadIdx.x; b8[i] = 0x30303030 + i; }
    h8_t ha;
    h16_t hb16;
    for (int i = 0; i < 8; ++i) ha[i] = (half_t)(0.001f * (threadIdx.x + i));
    for (int i = 0; i < 16; ++i) hb16[i] = (half_t)(0.25f + i);
    const int id = 0x4e4e4e4e;
    const int sc = 127 * 0x01010101;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (KIND == 0) acc[j] = __builtin_amdgcn_smfmac_f32_32x32x32_f16(ha, hb16, acc[j], id, 0, 0);
            else if (KIND == 1) acc[j] = __builtin_amdgcn_smfmac_f32_32x32x64_fp8_fp8(a4, b8, acc[j], id, 0, 0);
            else acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc[j], 0, 0, 0, sc, 0, sc);
        }
    }
    float s = 0.f;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 16; ++i) s += acc[j][i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

static float e4m3_decode(unsigned char v) {
    int s = v >> 7, e = (v >> 3) & 15, m = v & 7;
    float x;
    if (e == 15 && m == 7) return NAN;
    if (e == 0) x = ldexpf((float)m, -9);
    else x = ldexpf(1.f + m / 8.f, e - 7);
    return s ? -x : x;
}
static unsigned char e4m3_encode_exact(float v) {      // v must be an e4m3 value
    for (int b = 0; b < 256; ++b)
        if (b != 0x80 && e4m3_decode((unsigned char)b) == v) return (unsigned char)b;
    printf("not an e4m3 value: %g\n", v);
    exit(1);
}

static unsigned char *dA, *dB;
static int* dI;
static float *dCin, *dC;

static std::vector<float> run(const std::vector<unsigned char>& a, const std::vector<unsigned char>& b, const std::vector<int>& iv,
                              const std::vector<float>& cin) {
    CK(hipMemcpy(dA, a.data(), 64 * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, b.data(), 64 * 32, hipMemcpyHostToDevice));
    CK(hipMemcpy(dI, iv.data(), 256, hipMemcpyHostToDevice));
    CK(hipMemcpy(dCin, cin.data(), 4096, hipMemcpyHostToDevice));
    smfmac_kernel<<<1, 64>>>(dA, dB, dI, dCin, dC);
    CK(hipGetLastError());
    std::vector<float> c(1024);
    CK(hipMemcpy(c.data(), dC, 4096, hipMemcpyDeviceToHost));
    return c;
}

int main() {
    CK(hipMalloc(&dA, 64 * 16)); CK(hipMalloc(&dB, 64 * 32)); CK(hipMalloc(&dI, 256)); CK(hipMalloc(&dCin, 4096)); CK(hipMalloc(&dC, 4096));
    const std::vector<float> zeroC(1024, 0.f);
    // 1a. exactness on random integer data under the layout stated above
    srand(7);
    {
        std::vector<int> Ad(32 * 64, 0), Bd(64 * 32);          // dense A[row][k], B[k][col]
        std::vector<unsigned char> Ac(64 * 16), Bl(64 * 32);
        std::vector<int> idx(64);
        for (int i = 0; i < 64 * 32; ++i) Bd[i] = rand() % 9 - 4;
        for (int lane = 0; lane < 64; ++lane) {
            const int r = lane & 31, h = lane >> 5;
            unsigned field = 0;
            for (int g = 0; g < 8; ++g) {
                int p0 = rand() % 4, p1 = rand() % 4;
                while (p1 == p0) p1 = rand() % 4;
                if (p0 > p1) { int t = p0; p0 = p1; p1 = t; }
                const int v0 = rand() % 9 - 4, v1 = rand() % 9 - 4;
                Ad[r * 64 + 32 * h + 4 * g + p0] = v0;
                Ad[r * 64 + 32 * h + 4 * g + p1] = v1;
                Ac[lane * 16 + 2 * g] = e4m3_encode_exact((float)v0);
                Ac[lane * 16 + 2 * g + 1] = e4m3_encode_exact((float)v1);
                field |= (unsigned)p0 << (4 * g) | (unsigned)p1 << (4 * g + 2);
            }
            idx[lane] = (int)field;
        }
        for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 32; ++e)
                Bl[lane * 32 + e] = e4m3_encode_exact((float)Bd[(32 * (e >> 4) + 16 * (lane >> 5) + (e & 15)) * 32 + (lane & 31)]);
        const std::vector<float> C = run(Ac, Bl, idx, zeroC);
        int bad = 0;
        for (int r = 0; r < 32; ++r)
            for (int c = 0; c < 32; ++c) {
                int s = 0;
                for (int k = 0; k < 64; ++k) s += Ad[r * 64 + k] * Bd[k * 32 + c];
                if (C[r * 32 + c] != (float)s) ++bad;
            }
        printf("layout (hypothesis): mismatches %d of 1024\n", bad);
    }
    // 1b. one-hot dump: A = 1 in kept slot j of the lanes of half h only; B byte e of the lanes of half hb carries the
    //     number f = e + 32 hb in two runs (1 + (f & 7), then 1 + (f >> 3): both e4m3 values); all 16 index fields = p.
    printf("one-hot: B byte met (e + 32 * lane half; -1 = none) by kept slot j of the lanes of half h, all index fields = p\n");
    for (int h = 0; h < 2; ++h)
        for (int p = 0; p < 4; ++p) {
            printf("  h=%d p=%d:", h, p);
            for (int j = 0; j < 16; ++j) {
                std::vector<unsigned char> a(64 * 16, 0), b(64 * 32);
                for (int l = 32 * h; l < 32 * h + 32; ++l) a[l * 16 + j] = 0x38;                   // 1.0
                std::vector<int> iv(64, (int)(0x55555555u * (unsigned)p));
                int f = 0;
                for (int part = 0; part < 2; ++part) {
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 32; ++e) {
                            const int ff = e + 32 * (l >> 5);
                            b[l * 32 + e] = e4m3_encode_exact((float)(1 + (part ? ff >> 3 : ff & 7)));
                        }
                    const float c00 = run(a, b, iv, zeroC)[0];
                    if (c00 == 0.f) { f = -1; break; }
                    f += part ? ((int)c00 - 1) << 3 : (int)c00 - 1;
                }
                printf(" %2d", f);
            }
            printf("\n");
        }

    // 2. truncation: big product 2^8 * 2^8 in kept slot 0 (lane 0, index 0 -> its B byte), accumulator input -2^16; one
    //    small product 2^j = 2^ja * 2^jb in kept slot s (lanes 0 / 32 of row 0).  B column 0 holds 2^jb in every byte but
    //    the one the big product meets.  Also the same without the big product (reference).
    printf("truncation: per kept slot s of row 0 (s < 16: lane 0, else lane 32), smallest j with 2^j arriving whole beside 2^16\n");
    for (int with_big = 1; with_big >= 0; --with_big) {
        printf("  %s:", with_big ? "beside 2^16" : "alone      ");
        for (int s = with_big ? 1 : 0; s < 32; ++s) {
            int jmin = 99;
            float first_bad = 0.f;
            for (int j = 8; j >= -12; --j) {
                const int ja = j / 2, jb = j - ja;
                std::vector<unsigned char> a(64 * 16, 0), b(64 * 32, 0);
                std::vector<int> iv(64, 0x44444444);           // every group: offsets 0 and 1
                std::vector<float> cin(1024, 0.f);
                for (int l = 0; l < 64; l += 32)
                    for (int e = 0; e < 32; ++e) b[l * 32 + e] = e4m3_encode_exact(ldexpf(1.f, jb));
                a[(s >> 4) * 32 * 16 + (s & 15)] = e4m3_encode_exact(ldexpf(1.f, ja));
                if (with_big) {
                    a[0] = e4m3_encode_exact(256.f);
                    b[0] = e4m3_encode_exact(256.f);           // hypothesis 1: kept slot 0 / offset 0 of lane 0 meets B byte 0 of lane 0
                    cin[0] = -65536.f;
                }
                const float c00 = run(a, b, iv, cin)[0];
                if (c00 == ldexpf(1.f, j)) jmin = j;
                else { first_bad = c00; break; }
            }
            printf(" %d", jmin);
            if (jmin > -12 && s == 1) printf("(then %g)", first_bad);
        }
        printf("\n");
    }
    // 2b. the experiment as DESIGN.md 3i ran it: all 31 other kept slots carry 2^j; how many arrive
    printf("truncation, 31 products 2^j beside 2^16 (arrived = C / 2^j):");
    for (int j = 8; j >= -8; --j) {
        const int ja = j / 2, jb = j - ja;
        std::vector<unsigned char> a(64 * 16, 0), b(64 * 32, 0);
        std::vector<int> iv(64, 0x44444444);
        std::vector<float> cin(1024, 0.f);
        for (int l = 0; l < 64; l += 32) {
            for (int e = 0; e < 32; ++e) b[l * 32 + e] = e4m3_encode_exact(ldexpf(1.f, jb));
            for (int e = 0; e < 16; ++e) a[l * 16 + e] = e4m3_encode_exact(ldexpf(1.f, ja));
        }
        a[0] = e4m3_encode_exact(256.f);
        b[0] = e4m3_encode_exact(256.f);
        cin[0] = -65536.f;
        printf(" j=%d:%g", j, run(a, b, iv, cin)[0] / ldexpf(1.f, j));
    }
    printf("\n");

    // 3. issue rate: 1024 workgroups of 4 waves, 4 independent accumulators per wave
    float* dO; CK(hipMalloc(&dO, 1024 * 256 * 4));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int iters = 20000;
    const char* names[3] = {"smfmac f16 32x32x32", "smfmac fp8 32x32x64", "mfma scale f8f6f4 32x32x64"};
    for (int kind = 0; kind < 3; ++kind) {
        for (int rep = 0; rep < 2; ++rep) {
            CK(hipEventRecord(e0));
            if (kind == 0) rate_kernel<0><<<1024, 256>>>(dO, iters);
            else if (kind == 1) rate_kernel<1><<<1024, 256>>>(dO, iters);
            else rate_kernel<2><<<1024, 256>>>(dO, iters);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            const double per = kind == 0 ? 32.0 : 64.0;   // dense-equivalent K per instruction
            const double flop = 1024.0 * 4 * iters * 4 * 2.0 * 32 * 32 * per;
            const double cyc = ms * 1e-3 * 2.4e9 / (iters * 4.0 * 4.0);
            if (rep) printf("rate %s: %.3f ms, %.1f TFLOP/s (dense-equivalent), ~%.1f cycles per instruction at 2.4 GHz\n", names[kind], ms,
                            flop / ms * 1e-9, cyc);
        }
    }
    return 0;
}
