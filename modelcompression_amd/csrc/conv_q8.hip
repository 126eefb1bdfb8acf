// fp8 (OCP e4m3) implicit-GEMM convolution forward for gfx950 (MI355X), inference epilogue (an addition beyond the
// reference: post-training quantised inference, Darknet.precision = "fp8") -- and, for quantisation-aware
// training (Darknet.precision = "fp8-qat"), the same kernel with a raw fp32 epilogue + BatchNorm partial sums,
// the fake quantisation of the weights and the training form of the cast pass.
//
//   S[n][m] = sum_{tap, c} W8[n][kpos(tap, c)] * X8[pixel(m) + tap][c]        (fp32 accumulation of exact products)
//   v       = leaky(scale[n] * 2^-(e[n] + 1) * S + shift[n])
//
// X8 = e4m3(2 x) bytes in a padded NHWC BYTE buffer (halo bytes 0x00), W8 = e4m3(w * 2^e[n]) with one exponent per
// filter (mcamd_pack_q8 below).  The MFMA: by default v_mfma_f32_32x32x16_f16 on the bytes converted to fp16 in registers
// (byte-exact against the contract), or the block-scaled fp8 MFMA with both e8m0 scales 1.0 (MCAMD_Q8_MFMA=1: half the MFMA
// time, not byte-exact; conv_q8_loop.h: q8_mma).  The power of two goes into the epilogue's per-filter scale (exact).
// As in conv_sparse.hip the weights are the A operand (rows = output channels) and the pixels the columns, so that a lane's
// four accumulator rows are four consecutive channels of one pixel: one 32-bit word of output bytes.
//
// The K loop (operand form, LDS-DMA staging, ring, fragments, both MFMA forms) and the inference epilogue are
// conv_q8_loop.h's, here over all K chunks of 64-byte weight rows.  MaxPool of bytes is taken on the order-preserving key of
// the code (q is monotone: the maximum of the bytes is the byte of the maximum; -0 sorts below +0).
#include "conv_q8_loop.h"
#include "q8_exp.h"

// RAW (training, Darknet.precision = "fp8-qat"): the same main loop with the MCAMD_EPI_RAW_F32 epilogue --
// y[m][n] = 2^-(e[n] + 1) * S as fp32 [M][y_ld] (the power of two is exact) plus, per channel, the sum and the sum of squares
// of those fp32 values over the workgroup's pixel tile: slab row = the pixel tile mt, every row written, fixed order, no
// atomics (conv_epi.h: store_raw32_ch_tile, shared with conv_q8_w4.hip's training kernel).
//
// BORDER (slim models; conv_q8_border_kernel below): the epilogue adds the fp32 table entry of the pixel's
// border class to the raw value 2^-(e[n] + 1) * S in front of the affine step (conv_epi.h: Q8Border).
template <class T, bool F8MFMA, bool RAW, bool BORDER>
__device__ __forceinline__ void conv_q8_block(const IgemmArgs& __restrict__ a, const int* __restrict__ wexp, int y_f8, int y2_f8,
                                              const float* __restrict__ border, int border_ld) {
    using A = Q8RowsA<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Q8Wave w = q8_wave<T>();
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    A aop;
    aop.setup(a, nt, w.tid);                       // rows < Npad = round_up(N, 256)
    f32x16_t acc[T::TM][T::TN];
    q8_zero(acc);
    const Q8Lane<T> ln(w);
    q8_ring<T>(a, aop, Q8SeqDense{a.ktot / T::BK}, mt, smem, w, [&](const char* sa, const char* sb) {
        q8_dense_step<T, F8MFMA, false>(acc, sb, ln, [&](int i) { return q8_row_frag(sa, ln.a[i]); });
    });
    q8_mma_drain<F8MFMA>();
    __syncthreads();                               // every wave is done with the stage buffers
    if constexpr (RAW) {
        static_assert(raw32_ch_lds_bytes(T::BMW, T::BNP, T::WM, T::WN) <= A::RING, "raw epilogue inside the ring");
        store_raw32_ch_tile<T::BMW, T::BNP, T::WM, T::WN>(a, acc, wexp, smem, mt, nt, w.wm, w.wn, w.wave, w.lane, w.tid);   // (conv_epi.h)
    } else if constexpr (BORDER) {
        q8_infer_epilogue<T>(a, acc, wexp, y_f8, y2_f8, smem, mt, nt, w, Q8Border{border, wexp, border_ld, mt * T::BNP});
    } else {
        q8_infer_epilogue<T>(a, acc, wexp, y_f8, y2_f8, smem, mt, nt, w);
    }
}

template <class T, bool F8MFMA, bool RAW>
__global__ __launch_bounds__(T::NT) void conv_q8_kernel(IgemmArgs a, const int* __restrict__ wexp, int y_f8, int y2_f8) {
    conv_q8_block<T, F8MFMA, RAW, false>(a, wexp, y_f8, y2_f8, nullptr, 0);
}

// ... with a border table (inference epilogue only)
template <class T, bool F8MFMA>
__global__ __launch_bounds__(T::NT) void conv_q8_border_kernel(IgemmArgs a, const int* __restrict__ wexp, int y_f8, int y2_f8,
                                                               const float* __restrict__ border, int border_ld) {
    conv_q8_block<T, F8MFMA, false, true>(a, wexp, y_f8, y2_f8, border, border_ld);
}

template <class T, bool F8MFMA, bool RAW>
static int conv_q8_launch_t(IgemmArgs& a, const Q8Choice& c, const int* wexp, int y_f8, int y2_f8, hipStream_t st, const float* border,
                            int border_ld) {
    constexpr int RING = Q8RowsA<T>::RING, LDS = q8_infer_lds_max(RING, T::TILE_BYTES);
    const int lds = q8_infer_lds(RING, T::TILE_BYTES, a, y_f8, y2_f8);   // (RAW: y_f8 = y2_f8 = 0, its tiles lie inside the ring)
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    if constexpr (!RAW) {
        if (border) {                              // (the same tile, ring and LDS as the launch without a table)
            auto kern = conv_q8_border_kernel<T, F8MFMA>;
            MCAMD_LDS_OPT_IN(kern, LDS);
            hipLaunchKernelGGL(kern, dim3(c.grid), dim3(T::NT), lds, st, a, wexp, y_f8, y2_f8, border, border_ld);
            MCAMD_LAUNCH_CHECK("conv_fwd_q8_slim");
            return MCAMD_OK;
        }
    }
    auto kern = conv_q8_kernel<T, F8MFMA, RAW>;
    MCAMD_LDS_OPT_IN(kern, LDS);
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(T::NT), lds, st, a, wexp, y_f8, y2_f8);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8");
    return MCAMD_OK;
}

// Tiles as conv_sparse.hip's: 256 channels x 128 pixels (8 waves of 64 x 64) from 256 filters, 128 x 128 (4 waves) from
// 128, 64 x 128 below; a 3-deep ring of 64-byte rows (72 / 48 / 36 KB: two workgroups per CU).  The same rule in all four
// forms (inference, raw fp32, border table, 2:4 -- `form` is there so that a form can get a rule of its own).
// MCAMD_Q8_MFMA: 0 = fp16 MFMAs on converted bytes, 1 = the (block-scaled / sparse) fp8 MFMA: faster, not
// byte-exact (see the kernels' comments).
// No 256-channel tile in the default form: with the converted fragments it needs 136 registers (133 with 2:4 weights), one
// workgroup per CU, and measured 0.87-0.92 x the fp16 kernels on the 256- and 512-filter layers (2:4: 0.73-0.84 x the
// 128 x 128 tile there, 0.94 x over the whole forward).
// The grid is whole rounds of 8 pixel tiles (q8_choice_grid).
Q8Choice mcamd_q8_choice(long long M, int N, int form) {
    (void)form;
    Q8Choice c;
    c.f8mfma = MCAMD_ENV_INT("MCAMD_Q8_MFMA", 0) ? 1 : 0;
    c.bnp = 128;
    c.stages = 3;
    if (c.f8mfma && N >= 256) c.bmw = 256;
    else c.bmw = N >= 128 ? 128 : 64;
    q8_choice_grid(c, M, N);
    return c;
}

// `border` (mcamd_conv_fwd_q8_slim; inference epilogue only): fp32 [16][border_ld] table added by pixel class, or NULL.
int mcamd_conv_q8_launch(IgemmArgs& a, const void* wexp, int y_f8, int y2_f8, hipStream_t st, const float* border, int border_ld) {
    const int* we = (const int*)wexp;
    const bool raw = a.mode == MCAMD_EPI_RAW_F32;  // training: fp32 y + statistics, the same tile per filter count
    const Q8Choice c = mcamd_q8_choice(a.M, a.N, raw ? MCAMD_Q8_FORM_RAW : border ? MCAMD_Q8_FORM_BORDER : MCAMD_Q8_FORM_INFER);
    return q8_dispatch(c, "conv_fwd_q8", [&](auto t, auto f8) {
        if (raw) return conv_q8_launch_t<decltype(t), decltype(f8)::value, true>(a, c, we, 0, 0, st, nullptr, 0);
        return conv_q8_launch_t<decltype(t), decltype(f8)::value, false>(a, c, we, y_f8, y2_f8, st, border, border_ld);
    });
}

// ---------------------------------------------------------------------------------------
// packer: fp32 OIHW master * mask -> e4m3 bytes [Npad][ktot] in the kernel's K order + one exponent per filter
// ---------------------------------------------------------------------------------------
// One workgroup per row n < Npad.  a = max |w * mask| of the filter, (m, x) = frexp(a), e = 9 - x if m <= 0.875 else 8 - x
// (a 2^e in (224, 448]; e = 0 for an all-zero filter): integer steps only, so the host emulation cannot disagree at a
// power of two.  Then w8 = e4m3(clamp(ldexp(w * mask, e))), four k per thread and store.  Pad rows: zero bytes, e = 0.
// PITCH (mcamd_pack_q8_slim): cin % 8 == 0 only; the row is laid out for cin_pad = round_up(cin, 64) channels
// and the bytes of the channels [cin, cin_pad) are 0x00 -- the exponent comes from the real weights.
template <bool PITCH>
__device__ __forceinline__ void pack_q8_row(const float* __restrict__ w, const float* __restrict__ mask, char* __restrict__ wq,
                                            int* __restrict__ wexp, int cout, int cin, int ntaps) {
    __shared__ float red[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int ktot = cin * ntaps;
    const int cin_pad = PITCH ? (cin + 63) / 64 * 64 : cin, kpad = cin_pad * ntaps;
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
    for (int k4 = tid; k4 < kpad / 4; k4 += 256) {
        const int kp = 4 * k4;                                   // position in the packed order [cb][tap][64]
        const int cb = kp / (ntaps * 64), r = kp - cb * ntaps * 64;
        const int tap = r / 64, c0 = cb * 64 + (r - tap * 64);
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = 0.f;
            if (n < cout && (!PITCH || c0 < cin)) {              // (cin % 4 == 0: all four channels or none)
                const long long s = ((long long)n * cin + c0 + i) * ntaps + tap;
                v[i] = q8_weight_scaled(w[s] * (mask ? mask[s] : 1.f), e);
            }
        }
        int b = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        b = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], b, true);
        *(int*)(wq + (long long)n * kpad + kp) = b;
    }
}

__global__ __launch_bounds__(256) void pack_q8_kernel(const float* __restrict__ w, const float* __restrict__ mask,
                                                      char* __restrict__ wq, int* __restrict__ wexp, int cout, int cin,
                                                      int ntaps) {
    pack_q8_row<false>(w, mask, wq, wexp, cout, cin, ntaps);
}

__global__ __launch_bounds__(256) void pack_q8_slim_kernel(const float* __restrict__ w, const float* __restrict__ mask,
                                                           char* __restrict__ wq, int* __restrict__ wexp, int cout, int cin,
                                                           int ntaps) {
    pack_q8_row<true>(w, mask, wq, wexp, cout, cin, ntaps);
}

int mcamd_pack_q8_slim_launch(const float* w, const float* mask, void* wq, void* wexp, int cout, int cin, int ntaps, hipStream_t st) {
    hipLaunchKernelGGL(pack_q8_slim_kernel, dim3(round_up_int(cout, 256)), dim3(256), 0, st, w, mask, (char*)wq, (int*)wexp, cout,
                       cin, ntaps);
    MCAMD_LAUNCH_CHECK("pack_q8_slim");
    return MCAMD_OK;
}

int mcamd_pack_q8_launch(const float* w, const float* mask, void* wq, void* wexp, int cout, int cin, int ntaps, hipStream_t st) {
    hipLaunchKernelGGL(pack_q8_kernel, dim3(round_up_int(cout, 256)), dim3(256), 0, st, w, mask, (char*)wq, (int*)wexp, cout,
                       cin, ntaps);
    MCAMD_LAUNCH_CHECK("pack_q8");
    return MCAMD_OK;
}

// ---------------------------------------------------------------------------------------
// cast pass of an fp16 -> fp8 edge: fp16 [pixels][src_ld] channels [src_choff, +C) -> e4m3(2 x) bytes [pixels][dst_ld]
// channels [dst_choff, +C), halo pixels included (0 -> 0x00).  8 channels per thread.
// ---------------------------------------------------------------------------------------
// BACK (training): the values the codes stand for, deq(code) / 2 (exact in fp16), are written back over the
// fp16 source, so that the consumer's weight gradient multiplies what its forward multiplied.
template <bool BACK>
__global__ __launch_bounds__(256) void cast_q8_kernel(half_t* __restrict__ src, long long pixels, int src_ld, int src_choff,
                                                      int C, char* __restrict__ dst, int dst_ld, int dst_choff) {
    const int c8 = C / 8;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= pixels * c8) return;
    const long long p = t / c8;
    const int c = (int)(t - p * c8) * 8;
    const h8_t h = *(const h8_t*)(src + p * src_ld + src_choff + c);
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
    i32x2_t o;
    o[0] = e4m3_bytes4(v), o[1] = e4m3_bytes4(v + 4);
    *(i32x2_t*)(dst + p * dst_ld + dst_choff + c) = o;
    if (BACK) {
        h8_t r = q8_to_f16(o[0], o[1]);
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = r[i] * (half_t)0.5f;
        *(h8_t*)(src + p * src_ld + src_choff + c) = r;
    }
}

int mcamd_cast_q8_launch(const void* src, long long pixels, int src_ld, int src_choff, int C, void* dst, int dst_ld,
                         int dst_choff, int back, hipStream_t st) {
    const long long total = pixels * (C / 8);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (back) hipLaunchKernelGGL(cast_q8_kernel<true>, grid, dim3(256), 0, st, (half_t*)src, pixels, src_ld, src_choff, C, (char*)dst, dst_ld, dst_choff);
    else hipLaunchKernelGGL(cast_q8_kernel<false>, grid, dim3(256), 0, st, (half_t*)src, pixels, src_ld, src_choff, C, (char*)dst, dst_ld, dst_choff);
    MCAMD_LAUNCH_CHECK("cast_q8");
    return MCAMD_OK;
}

// ---------------------------------------------------------------------------------------
// fake quantisation of the weights (training): w_q = deq(e4m3(clamp(w * mask * 2^e))) * 2^-e as fp32 OIHW, e =
// the exponent table pack_q8_kernel wrote for the same weights -- the values the forward's weight bytes stand for.  The fp16
// packers build the dgrad operand from it.  Four consecutive weights per thread (cin * taps is a multiple of 64).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fakequant_q8_kernel(const float* __restrict__ w, const float* __restrict__ mask,
                                                           const int* __restrict__ wexp, float* __restrict__ out,
                                                           long long total4, int per_filter) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total4) return;
    const long long s = 4 * t;
    const int e = wexp[s / per_filter];
    f32x4_t v = *(const f32x4_t*)(w + s);
    if (mask) {
        const f32x4_t m = *(const f32x4_t*)(mask + s);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] *= m[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = fminf(fmaxf(ldexpf(v[i], e), -448.f), 448.f);
    int b = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
    b = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], b, true);
    f32x4_t r;
    r[0] = ldexpf(__builtin_amdgcn_cvt_f32_fp8(b, 0), -e), r[1] = ldexpf(__builtin_amdgcn_cvt_f32_fp8(b, 1), -e);
    r[2] = ldexpf(__builtin_amdgcn_cvt_f32_fp8(b, 2), -e), r[3] = ldexpf(__builtin_amdgcn_cvt_f32_fp8(b, 3), -e);
    *(f32x4_t*)(out + s) = r;
}

int mcamd_fakequant_q8_launch(const float* w, const float* mask, const void* wexp, float* out, int cout, int cin, int ntaps,
                              hipStream_t st) {
    const long long total4 = (long long)cout * cin * ntaps / 4;
    hipLaunchKernelGGL(fakequant_q8_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, w, mask, (const int*)wexp, out,
                       total4, cin * ntaps);
    MCAMD_LAUNCH_CHECK("fakequant_q8");
    return MCAMD_OK;
}
