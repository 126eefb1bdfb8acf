// 2:4-sparse fp8 (OCP e4m3) implicit-GEMM convolution forward for gfx950 (MI355X), inference epilogue (an addition beyond
// the reference: the nm_prune masks on the fp8 engine, Darknet.precision = "fp8-2:4").
//
//   S[n][m] = sum_{tap, c} W8[n][kpos(tap, c)] * X8[pixel(m) + tap][c]        (W8 2:4 along c; fp32 accumulation)
//   v       = leaky(scale[n] * 2^-(e[n] + 1) * S + shift[n])
//
// The byte buffers, the K loop around the matrix step and the epilogue are conv_q8_loop.h's; the weights are conv_q8.hip's
// packed rows with every group of 4 consecutive k reduced to its 2 kept bytes (mcamd_pack_q8_sparse24 below), multiplied on
// the sparse MFMA with the weights as the (sparse) A operand as in conv_sparse.hip.
//
// One K chunk = 64 dense k: per weight row 32 kept bytes + 8 index bytes (Q8HalfRowsA), per pixel one 64-byte row.  Lane
// (r, h), r = lane & 31, h = lane >> 5, holds
//   A: the 16 kept bytes of dense k [32 h, 32 h + 32) of row r, and index word h of the row's chunk: kept byte j lies in
//      group j / 2 of those 32 k at offset bits [2 j, 2 j + 2);
//   B: bytes [16 h, 16 h + 16) and [32 + 16 h, 32 + 16 h + 16) of pixel row r
// which IS the operand layout of v_smfmac_f32_32x32x64_fp8_fp8 (tools/smfmac_f8_probe.hip): MCAMD_Q8_MFMA=1 issues one per
// 32x32 block and chunk.  The default form converts the bytes to fp16 in registers and issues two
// v_smfmac_f32_32x32x32_f16 (layout: conv_sparse.hip); step s takes, of the same registers,
//   A: kept bytes [4 s, 4 s + 4) and [8 + 4 s, 8 + 4 s + 4) with their index bits [8 s, 8 s + 8) and [16 + 8 s, 16 + 8 s + 8),
//   B: bytes [8 s, 8 s + 8) of each of the lane's two 16-byte pieces,
// a k permutation common to both operands under which that instruction's lanes (A: k [16 h, 16 h + 16), B: k 16 (e >> 3) +
// 8 h + (e & 7)) meet exactly the registers above.  Its products are exact and its sum is an fp32 sum: the byte contract.
#include "conv_q8_loop.h"
#include "q8_exp.h"

typedef _Float16 h16_t __attribute__((ext_vector_type(16)));

template <class T>
using Q8SparseRowsA = Q8HalfRowsA<T, 8>;         // 32 kept bytes + two index words per row and chunk

// F8MFMA as in q8_mma: false = fp16 sparse MFMAs on converted bytes (byte-exact), true = the fp8 sparse MFMA, which like the
// dense fp8 MFMAs sums groups of 8 products on a grid 14 bits below the group's largest.
template <class T, bool F8MFMA>
__global__ __launch_bounds__(T::NT) void conv_q8_sparse_kernel(IgemmArgs a, const unsigned* __restrict__ idx, int npad,
                                                               const int* __restrict__ wexp, int y_f8, int y2_f8) {
    using A = Q8SparseRowsA<T>;
    constexpr int TM = T::TM, TN = T::TN;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Q8Wave w = q8_wave<T>();
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    A aop;
    aop.setup(a, idx, npad, nt, w.tid);
    f32x16_t acc[TM][TN];
    q8_zero(acc);
    const Q8Lane<T> ln(w);
    int ip[TM];                                    // the lane's index word in a stage's band
#pragma unroll
    for (int i = 0; i < TM; ++i) ip[i] = ln.arow[i] * 8 + ln.hh * 4;
    q8_ring<T>(a, aop, Q8SeqDense{a.ktot / T::BK}, mt, smem, w, [&](const char* sa, const char* sb) {
        i32x4_t af[TM];
        int ix[TM];
        i32x8_t bf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            af[i] = *(const i32x4_t*)(sa + ln.ahalf[i]);
            ix[i] = *(const int*)(A::band(sa) + ip[i]);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = q8_row_frag(sb, ln.b[j]);
        if constexpr (F8MFMA) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_smfmac_f32_32x32x64_fp8_fp8(af[i], bf[j], acc[i][j], ix[i], 0, 0);
        } else {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                h8_t a16[TM];
                int i16[TM];
                h16_t b16[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    a16[i] = q8_to_f16(af[i][s], af[i][2 + s]);
                    const unsigned x = (unsigned)ix[i];
                    i16[i] = (int)(((x >> (8 * s)) & 0xffu) | (((x >> (16 + 8 * s)) & 0xffu) << 8));
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const h8_t lo = q8_to_f16(bf[j][2 * s], bf[j][2 * s + 1]), hi = q8_to_f16(bf[j][4 + 2 * s], bf[j][4 + 2 * s + 1]);
                    b16[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_smfmac_f32_32x32x32_f16(a16[i], b16[j], acc[i][j], i16[i], 0, 0);
            }
        }
    });
    __syncthreads();                               // every wave is done with the stage buffers
    q8_infer_epilogue<T>(a, acc, wexp, y_f8, y2_f8, smem, mt, nt, w);
}

template <class T, bool F8MFMA>
static int conv_q8_sparse_launch_t(IgemmArgs& a, const Q8Choice& c, const unsigned* idx, int npad, const int* wexp, int y_f8, int y2_f8,
                                   hipStream_t st) {
    constexpr int RING = Q8SparseRowsA<T>::RING;
    auto kern = conv_q8_sparse_kernel<T, F8MFMA>;
    MCAMD_LDS_OPT_IN(kern, q8_infer_lds_max(RING, T::TILE_BYTES));
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(T::NT), q8_infer_lds(RING, T::TILE_BYTES, a, y_f8, y2_f8), st, a, idx, npad, wexp, y_f8,
                       y2_f8);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_sparse24");
    return MCAMD_OK;
}

// The tile is mcamd_q8_choice's (conv_q8.hip: 256 channels x 128 pixels from 256 filters with the fp8 MFMA, 128 x 128 from
// 128, 64 x 128 below); a 3-deep ring (54 / 39 / 33 KB).
// MCAMD_Q8_MFMA: 0 = fp16 sparse MFMAs on converted bytes, 1 = the fp8 sparse MFMA.
int mcamd_conv_q8_sparse_launch(IgemmArgs& a, const void* idx, const void* wexp, int y_f8, int y2_f8, hipStream_t st) {
    const int npad = round_up_int(a.N, 256);
    const Q8Choice c = mcamd_q8_choice(a.M, a.N, MCAMD_Q8_FORM_SPARSE);
    return q8_dispatch(c, "conv_fwd_q8_sparse24", [&](auto t, auto f8) {
        return conv_q8_sparse_launch_t<decltype(t), decltype(f8)::value>(a, c, (const unsigned*)idx, npad, (const int*)wexp, y_f8, y2_f8, st);
    });
}

// ---------------------------------------------------------------------------------------
// packer: fp32 OIHW master * mask -> kept e4m3 bytes [Npad][ktot / 2] + index words [ktot / 64][Npad][2] + exponents
// ---------------------------------------------------------------------------------------
// One workgroup per row n < Npad.  The exponent is pack_q8_kernel's (max |w * mask| of the whole filter, integer steps).
// Then one thread per 32 dense k of the packed order [cb][tap][64]: 8 groups of 4 consecutive input channels at one tap ->
// 16 kept bytes and one index word.  The kept entries of a group are pack_sparse24_kernel's: the non-zeros of the fp32
// w * mask in channel order (the first two when the mask does not conform); a group with fewer gets distinct ascending
// indices with zero values.  Pad rows: zero bytes, e = 0.
__global__ __launch_bounds__(256) void pack_q8_sparse24_kernel(const float* __restrict__ w, const float* __restrict__ mask,
                                                               char* __restrict__ wq, unsigned* __restrict__ idx,
                                                               int* __restrict__ wexp, int cout, int cin, int ntaps, int npad) {
    __shared__ float red[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int ktot = cin * ntaps;
    float amax = 0.f;
    if (n < cout)
        for (int o = tid; o < ktot; o += 256) {
            const long long s = (long long)n * ktot + o;
            amax = fmaxf(amax, fabsf(w[s] * (mask ? mask[s] : 1.f)));
        }
    red[tid] = amax;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    amax = red[0];
    const int e = q8_filter_exponent(amax);
    if (tid == 0) wexp[n] = e;
    for (int u = tid; u < ktot / 32; u += 256) {
        i32x4_t kept;
        unsigned field = 0;
#pragma unroll
        for (int g2 = 0; g2 < 4; ++g2) {           // two groups -> four kept bytes -> one 32-bit word
            float kv[4];
#pragma unroll
            for (int gg = 0; gg < 2; ++gg) {
                const int g = 2 * g2 + gg;
                const int kp = 32 * u + 4 * g;                       // first k of the group in the packed order
                const int cb = kp / (ntaps * 64), r = kp - cb * ntaps * 64;
                const int tap = r / 64, c0 = cb * 64 + (r - tap * 64);
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = 0.f;
                    if (n < cout) {
                        const long long s = ((long long)n * cin + c0 + i) * ntaps + tap;
                        v[i] = w[s] * (mask ? mask[s] : 1.f);
                    }
                }
                int p[2], np = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (v[i] != 0.f && np < 2) p[np++] = i;
                if (np == 0) { p[0] = 0; p[1] = 1; }
                else if (np == 1) { if (p[0] == 0) p[1] = 1; else { p[1] = p[0]; p[0] = 0; } }
                float k0 = 0.f, k1 = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {      // (selects, not indexed reads: v stays in registers)
                    k0 = p[0] == i ? v[i] : k0;
                    k1 = p[1] == i ? v[i] : k1;
                }
                kv[2 * gg] = q8_weight_scaled(k0, e);
                kv[2 * gg + 1] = q8_weight_scaled(k1, e);
                field |= (unsigned)p[0] << (4 * g) | (unsigned)p[1] << (4 * g + 2);
            }
            int b = __builtin_amdgcn_cvt_pk_fp8_f32(kv[0], kv[1], 0, false);
            b = __builtin_amdgcn_cvt_pk_fp8_f32(kv[2], kv[3], b, true);
            kept[g2] = b;
        }
        *(i32x4_t*)(wq + (long long)n * (ktot / 2) + 16 * u) = kept;
        idx[((long long)(u >> 1) * npad + n) * 2 + (u & 1)] = field;
    }
}

int mcamd_pack_q8_sparse24_launch(const float* w, const float* mask, void* wq, void* idx, void* wexp, int cout, int cin,
                                  int ntaps, hipStream_t st) {
    const int npad = round_up_int(cout, 256);
    hipLaunchKernelGGL(pack_q8_sparse24_kernel, dim3(npad), dim3(256), 0, st, w, mask, (char*)wq, (unsigned*)idx, (int*)wexp, cout,
                       cin, ntaps, npad);
    MCAMD_LAUNCH_CHECK("pack_q8_sparse24");
    return MCAMD_OK;
}
