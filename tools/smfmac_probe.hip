// Probe of the gfx950 2:4 sparse fp16 MFMA for the sparse forward (tools only; not part of libmcamd.so):
//  1. operand and index layout of v_smfmac_f32_32x32x32_f16.  Lane l = (r, h), r = l & 31, h = l >> 5:
//     A (sparse, 4 VGPRs): row r, the dense k range [16 h, 16 h + 16) compressed to 8 kept fp16 values; kept value j lies
//       in the group of 4 k's [16 h + 4 (j / 2), +4) at offset idx_j = bits [2 j, 2 j + 2) of the 16-bit index field that
//       `abid` picks out of the index VGPR (abid 0: bits 0-15, abid 1: bits 16-31);
//     B (dense, 8 VGPRs): column r, element e = k 16 (e >> 3) + 8 h + (e & 7) -- the two fragments of the dense
//       32x32x16 MFMA (k [8 h, 8 h + 8) of each k16 half) concatenated;
//     C: the 32x32 accumulator of the dense form.
//     Checked exactly on integer-valued data; then a one-hot dump prints which B element each (kept value, index)
//     pair meets (how the layout above was read off).
// measured (MI355X): both abid forms exact (0 mismatches); one-hot table as stated; 4 049 TFLOP/s dense-equivalent against
// 2 121 for the dense fp16 form on constant data -- the same ~38-40 cycles per instruction for twice the k
//  2. issue rate against v_mfma_f32_32x32x16_f16 (dense-equivalent FLOP: 2 * 32 * 32 * 32 per smfmac).
// build + run:  hipcc --offload-arch=gfx950 -O3 -o tools/smfmac_probe tools/smfmac_probe.hip && ./tools/smfmac_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef _Float16 half_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(8))) _Float16 h8_t;
typedef __attribute__((ext_vector_type(16))) _Float16 h16_t;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

// one wave.  Ac: [64 lanes][8] kept values, Bl: [64 lanes][16], idx: [64] index VGPRs; C[32][32]
template <int ABID>
__global__ void smfmac_kernel(const half_t* Ac, const half_t* Bl, const int* idx, float* C) {
    const int lane = threadIdx.x, h = lane >> 5;
    h8_t a;
    h16_t b;
    for (int i = 0; i < 8; ++i) a[i] = Ac[lane * 8 + i];
    for (int i = 0; i < 16; ++i) b[i] = Bl[lane * 16 + i];
    f32x16_t acc;
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    acc = __builtin_amdgcn_smfmac_f32_32x32x32_f16(a, b, acc, idx[lane], 0, ABID);
    for (int i = 0; i < 16; ++i) {
        int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        C[row * 32 + (lane & 31)] = acc[i];
    }
}

template <int SPARSE>
__global__ __launch_bounds__(256) void rate_kernel(float* out, int iters) {
    f32x16_t acc[4];
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    h8_t ha, hb;
    h16_t hb16;
    for (int i = 0; i < 8; ++i) { ha[i] = (half_t)(0.001f * (threadIdx.x + i)); hb[i] = (half_t)(0.5f + i); }
    for (int i = 0; i < 16; ++i) hb16[i] = (half_t)(0.25f + i);
    const int id = 0x4e4e + threadIdx.x;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (SPARSE) acc[j] = __builtin_amdgcn_smfmac_f32_32x32x32_f16(ha, hb16, acc[j], id, 0, 0);
            else acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ha, hb, acc[j], 0, 0, 0);
        }
    }
    float s = 0.f;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 16; ++i) s += acc[j][i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

int main() {
    half_t *dA, *dB; int* dI; float* dC;
    CK(hipMalloc(&dA, 64 * 8 * 2)); CK(hipMalloc(&dB, 64 * 16 * 2)); CK(hipMalloc(&dI, 64 * 4)); CK(hipMalloc(&dC, 4096));
    // 1a. exactness on random integer data under the layout stated above
    srand(7);
    std::vector<int> Ad(32 * 32, 0), Bd(32 * 32);          // dense A[row][k], B[k][col]; k = 16 h + e
    std::vector<half_t> Ac(64 * 8), Bl(64 * 16);
    std::vector<int> idx(64);
    for (int i = 0; i < 32 * 32; ++i) Bd[i] = rand() % 9 - 4;
    for (int lane = 0; lane < 64; ++lane) {
        const int r = lane & 31, h = lane >> 5;
        unsigned field = 0;
        for (int g = 0; g < 4; ++g) {
            int p0 = rand() % 4, p1 = rand() % 4;
            while (p1 == p0) p1 = rand() % 4;
            if (p0 > p1) { int t = p0; p0 = p1; p1 = t; }
            const int v0 = rand() % 9 - 4, v1 = rand() % 9 - 4;
            Ad[r * 32 + 16 * h + 4 * g + p0] = v0;
            Ad[r * 32 + 16 * h + 4 * g + p1] = v1;
            Ac[lane * 8 + 2 * g] = (half_t)v0;
            Ac[lane * 8 + 2 * g + 1] = (half_t)v1;
            field |= (unsigned)p0 << (4 * g) | (unsigned)p1 << (4 * g + 2);
        }
        idx[lane] = (int)field;
    }
    for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 16; ++e) Bl[lane * 16 + e] = (half_t)Bd[(16 * (e >> 3) + 8 * (lane >> 5) + (e & 7)) * 32 + (lane & 31)];
    CK(hipMemcpy(dA, Ac.data(), 64 * 8 * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, Bl.data(), 64 * 16 * 2, hipMemcpyHostToDevice));
    for (int abid = 0; abid < 2; ++abid) {
        std::vector<int> iv(64);
        for (int l = 0; l < 64; ++l) iv[l] = abid ? (int)(((unsigned)idx[l] << 16) | 0x1234u) : (int)((unsigned)idx[l] | 0xbeef0000u);
        CK(hipMemcpy(dI, iv.data(), 256, hipMemcpyHostToDevice));
        if (abid) smfmac_kernel<1><<<1, 64>>>(dA, dB, dI, dC);
        else smfmac_kernel<0><<<1, 64>>>(dA, dB, dI, dC);
        CK(hipGetLastError());
        std::vector<float> C(1024);
        CK(hipMemcpy(C.data(), dC, 4096, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int r = 0; r < 32; ++r)
            for (int c = 0; c < 32; ++c) {
                int s = 0;
                for (int k = 0; k < 32; ++k) s += Ad[r * 32 + k] * Bd[k * 32 + c];
                if (C[r * 32 + c] != (float)s) ++bad;
            }
        printf("layout abid=%d: mismatches %d of 1024\n", abid, bad);
    }
    // 1b. one-hot dump: A = 1 in kept slot j of the lanes of K half h only, B element e of every lane = 1 + e + 16 h,
    //     index field = the same 2-bit value p in all 8 positions; C[0][0] names the B element met (0 = none)
    printf("one-hot: value = 1 + (B element) + 16 * (K half) met by kept slot j with all index fields = p\n");
    for (int h = 0; h < 2; ++h)
        for (int p = 0; p < 4; ++p) {
            printf("  h=%d p=%d:", h, p);
            for (int j = 0; j < 8; ++j) {
                std::vector<half_t> a(64 * 8, (half_t)0.f), b(64 * 16);
                for (int l = 32 * h; l < 32 * h + 32; ++l) a[l * 8 + j] = (half_t)1.f;
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 16; ++e) b[l * 16 + e] = (half_t)(float)(1 + e + 16 * (l >> 5));
                std::vector<int> iv(64, (int)(0x5555u * (unsigned)p));
                CK(hipMemcpy(dA, a.data(), 64 * 8 * 2, hipMemcpyHostToDevice));
                CK(hipMemcpy(dB, b.data(), 64 * 16 * 2, hipMemcpyHostToDevice));
                CK(hipMemcpy(dI, iv.data(), 256, hipMemcpyHostToDevice));
                smfmac_kernel<0><<<1, 64>>>(dA, dB, dI, dC);
                float c00;
                CK(hipMemcpy(&c00, dC, 4, hipMemcpyDeviceToHost));
                printf(" %3g", c00);
            }
            printf("\n");
        }

    // 2. issue rate: 1024 workgroups of 4 waves, 4 independent accumulators per wave
    float* dO; CK(hipMalloc(&dO, 1024 * 256 * 4));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int iters = 20000;
    for (int sp = 0; sp < 2; ++sp) {
        for (int rep = 0; rep < 2; ++rep) {
            CK(hipEventRecord(e0));
            if (sp) rate_kernel<1><<<1024, 256>>>(dO, iters);
            else rate_kernel<0><<<1024, 256>>>(dO, iters);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            const double per = sp ? 32.0 : 16.0;   // dense-equivalent K per instruction
            double flop = 1024.0 * 4 * iters * 4 * 2.0 * 32 * 32 * per;
            const double cyc = ms * 1e-3 * 2.4e9 / (iters * 4.0 * 4.0);   // 4 waves per SIMD x 4 instructions per iteration
            if (rep) printf("rate %s: %.3f ms, %.1f TFLOP/s (dense-equivalent), ~%.1f cycles per instruction at 2.4 GHz\n",
                            sp ? "smfmac f16 32x32x32" : "mfma f16 32x32x16", ms, flop / ms * 1e-9, cyc);
        }
    }
    return 0;
}
