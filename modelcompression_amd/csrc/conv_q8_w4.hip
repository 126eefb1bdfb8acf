// 4-bit weight inference on the fp8 engine (an addition beyond the reference: Darknet.precision = "fp8-w4") --
// and its training form (Darknet.precision = "fp8-w4-qat"; DESIGN.md 3x: the raw fp32 epilogue + the fake quantisation below):
// conv_q8_loop.h's K loop and epilogue with the weight operand held as e2m1 codes + one shift per group of 32 input channels,
// staged as nibbles and expanded to e4m3 bytes IN REGISTERS in front of the MFMAs.
//
//   S[n][m] = sum_{tap, c} W8x[n][kpos(tap, c)] * X8[pixel(m) + tap][c]       (fp32 accumulation of exact products)
//   v       = leaky(scale[n] * 2^-(e4[n] + 1) * S + shift[n])
//
// The format, per filter f of w = weight * mask (mcamd.h states it in full): e4_f = e_f - 1 with e_f mcamd_pack_q8's exponent
// (0 for an all-zero filter), s = w 2^e4_f; per group -- the 32 consecutive input channels [32 j, 32 j + 32) at one tap -- the
// smallest shift g in [-5, 6] with max |s| <= 6 * 2^g; a code = sign + |s| / 2^g rounded to nearest (ties to the even
// mantissa bit) onto {0, 0.5, 1, 1.5, 2, 3, 4, 6}.  Every value grid[code] * 2^g is an e4m3 number (one mantissa bit, 2^-6
// <= |value| <= 384), so W8x, the byte of that value, is exact, and this kernel is conv_q8_kernel on a restricted set of weight
// bytes: the decoded fragment of lane (r, h) holds the bytes [16 h, 16 h + 16) and [32 + 16 h, +16) of row r's chunk, as
// conv_q8_kernel's does, and both kernels hand their fragments to the same step function (q8_dense_step) in both MFMA forms
// (MCAMD_Q8_MFMA).
//
// One K chunk = 64 k: per weight row 32 code bytes (half of conv_q8.hip's A traffic) + 2 shift bytes (Q8HalfRowsA: the shift
// bytes of a tile's chunk are one wave-wide DMA), per pixel one 64-byte row.
//
// Decode (w4_decode): code dword d of a lane's 16 bytes holds the lane's k 8 d .. 8 d + 7 -- byte b: low nibble k 8 d + b,
// high nibble k 8 d + 4 + b -- so `x & 0x0f0f0f0f` and `(x >> 4) & 0x0f0f0f0f` are the four codes of two output dwords.  The
// magnitude byte comes from an 8-entry table by v_perm_b32 (entry c: 0 for c = 0, else the e4m3 magnitude of grid[c] 2^g --
// the group's table is the g = -5 one, {0x00, 0x08, 0x10, 0x14, 0x18, 0x1c, 0x20, 0x24}, plus (g + 5) << 3 on its non-zero
// entries: two additions per group and lane), the sign bit is moved up from bit 3.  A lane's first 16 k lie in the chunk's
// first group, its second 16 in the second.
#include "conv_q8_loop.h"
#include "q8_exp.h"
#include "w4_quant.h"

template <class T>
using Q8W4RowsA = Q8HalfRowsA<T, 2>;             // 32 code bytes + the two group shifts per row and chunk

// e4m3 magnitudes of the grid {0, 0.5, 1, 1.5, 2, 3, 4, 6} * 2^-5: entries 0-3 (v_perm's second source), 4-7 (its first)
constexpr unsigned W4_TLO = 0x14100800u, W4_THI = 0x24201c18u;

struct W4Table {
    unsigned lo, hi;
};

// the table of a group with shift byte G = g + 5: every non-zero entry's exponent field raised by G (no carry: <= 0x7c)
__device__ __forceinline__ W4Table w4_table(unsigned G) {
    W4Table t;
    t.lo = W4_TLO + (G << 3) * 0x01010100u;
    t.hi = W4_THI + (G << 3) * 0x01010101u;
    return t;
}

// four codes, one per byte (bits 0-2 magnitude, bit 3 sign) -> their four e4m3 bytes
__device__ __forceinline__ int w4_bytes4(unsigned c4, const W4Table& t) {
    const unsigned mag = __builtin_amdgcn_perm(t.hi, t.lo, c4 & 0x07070707u);
    return (int)(((c4 & 0x08080808u) << 4) | mag);
}

// a lane's 16 code bytes + the two shift bytes of its row's chunk -> its 32 e4m3 weight bytes (conv_q8_kernel's fragment)
__device__ __forceinline__ i32x8_t w4_decode(i32x4_t codes, unsigned shifts) {
    const W4Table t0 = w4_table(shifts & 0xffu), t1 = w4_table((shifts >> 8) & 0xffu);
    i32x8_t o;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned x = (unsigned)codes[d];
        o[2 * d] = w4_bytes4(x & 0x0f0f0f0fu, d < 2 ? t0 : t1);
        o[2 * d + 1] = w4_bytes4((x >> 4) & 0x0f0f0f0fu, d < 2 ? t0 : t1);
    }
    return o;
}

// RAW (training, Darknet.precision = "fp8-w4-qat"): the same K loop -- staging, register decode, both MFMA forms
// and their s_nop spacing -- with the MCAMD_EPI_RAW_F32 epilogue conv_q8_block uses (conv_epi.h: store_raw32_ch_tile): y[m][n] =
// 2^-(e4[n] + 1) * S as fp32 [M][y_ld] and, with a.stats, the per-channel sums and sums of squares of those values, slab row =
// the pixel tile.  That epilogue's LDS need (72 / 36 / 19 KB) is not the ring's (51 / 39 / 33 KB -- the code rows are half the
// fp8 kernel's): the launch asks for the larger of the two.
template <class T, bool F8MFMA, bool RAW>
__device__ __forceinline__ void conv_q8_w4_block(const IgemmArgs& __restrict__ a, const char* __restrict__ gshift, int npad,
                                                 const int* __restrict__ wexp, int y_f8, int y2_f8) {
    using A = Q8W4RowsA<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Q8Wave w = q8_wave<T>();
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    A aop;
    aop.setup(a, gshift, npad, nt, w.tid);
    f32x16_t acc[T::TM][T::TN];
    q8_zero(acc);
    const Q8Lane<T> ln(w);
    // the shared MFMA sequence on the decoded bytes; the A fragment was just written by VALU instructions (VALU_A)
    q8_ring<T>(a, aop, Q8SeqDense{a.ktot / T::BK}, mt, smem, w, [&](const char* sa, const char* sb) {
        q8_dense_step<T, F8MFMA, true>(acc, sb, ln, [&](int i) {
            return w4_decode(*(const i32x4_t*)(sa + ln.ahalf[i]), *(const unsigned short*)(A::band(sa) + ln.arow[i] * 2));
        });
    });
    q8_mma_drain<F8MFMA>();
    __syncthreads();                               // every wave is done with the stage buffers
    // the shared epilogues, e4_f in place of e_f (RAW: the launch requested raw32_ch_lds_bytes() or the ring, whichever is larger)
    if constexpr (RAW) store_raw32_ch_tile<T::BMW, T::BNP, T::WM, T::WN>(a, acc, wexp, smem, mt, nt, w.wm, w.wn, w.wave, w.lane, w.tid);
    else q8_infer_epilogue<T>(a, acc, wexp, y_f8, y2_f8, smem, mt, nt, w);
}

template <class T, bool F8MFMA>
__global__ __launch_bounds__(T::NT) void conv_q8_w4_kernel(IgemmArgs a, const char* __restrict__ gshift, int npad,
                                                           const int* __restrict__ wexp, int y_f8, int y2_f8) {
    conv_q8_w4_block<T, F8MFMA, false>(a, gshift, npad, wexp, y_f8, y2_f8);
}

// ... with the raw fp32 epilogue + statistics (training)
template <class T, bool F8MFMA>
__global__ __launch_bounds__(T::NT) void conv_q8_w4_raw_kernel(IgemmArgs a, const char* __restrict__ gshift, int npad,
                                                               const int* __restrict__ wexp) {
    conv_q8_w4_block<T, F8MFMA, true>(a, gshift, npad, wexp, 0, 0);
}

template <class T, bool F8MFMA>
static int conv_q8_w4_raw_launch_t(IgemmArgs& a, const Q8Choice& c, const char* gshift, int npad, const int* wexp, hipStream_t st) {
    constexpr int RING = Q8W4RowsA<T>::RING;
    constexpr int EPI = raw32_ch_lds_bytes(T::BMW, T::BNP, T::WM, T::WN);
    constexpr int LDS = RING > EPI ? RING : EPI;   // (256 x 128: the epilogue's 72 KB over a 51 KB ring)
    static_assert(EPI <= LDS && RING <= LDS && LDS <= 160 * 1024, "raw epilogue and ring inside the requested LDS");
    auto kern = conv_q8_w4_raw_kernel<T, F8MFMA>;
    MCAMD_LDS_OPT_IN(kern, LDS);
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(T::NT), LDS, st, a, gshift, npad, wexp);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_w4_raw");
    return MCAMD_OK;
}

template <class T, bool F8MFMA>
static int conv_q8_w4_launch_t(IgemmArgs& a, const Q8Choice& c, const char* gshift, int npad, const int* wexp, int y_f8, int y2_f8,
                               hipStream_t st) {
    constexpr int RING = Q8W4RowsA<T>::RING;
    auto kern = conv_q8_w4_kernel<T, F8MFMA>;
    MCAMD_LDS_OPT_IN(kern, q8_infer_lds_max(RING, T::TILE_BYTES));
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(T::NT), q8_infer_lds(RING, T::TILE_BYTES, a, y_f8, y2_f8), st, a, gshift, npad, wexp, y_f8,
                       y2_f8);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_w4");
    return MCAMD_OK;
}

// The tile is mcamd_q8_choice's for the fp8 block (conv_q8.hip: 256 filters x 128 pixels from 256 filters with the fp8 MFMA,
// 128 x 128 from 128, 64 x 128 below; 3 stages): every one of the five instances compiles without scratch memory
// (profiles/q8_w4_resources.txt), so none is left out.
Q8Choice mcamd_q8_w4_choice(long long M, int N) { return mcamd_q8_choice(M, N, MCAMD_Q8_FORM_INFER); }

int mcamd_conv_q8_w4_launch(IgemmArgs& a, const void* gshift, const void* wexp, int y_f8, int y2_f8, hipStream_t st) {
    const int npad = round_up_int(a.N, 256);
    const Q8Choice c = mcamd_q8_w4_choice(a.M, a.N);
    return q8_dispatch(c, "conv_fwd_q8_w4", [&](auto t, auto f8) {
        return conv_q8_w4_launch_t<decltype(t), decltype(f8)::value>(a, c, (const char*)gshift, npad, (const int*)wexp, y_f8, y2_f8, st);
    });
}

// The training launch: the same tile per filter count (mcamd_q8_choice's for the raw fp8 block, as the engine's statistics
// slab and mcamd_conv_fwd_q8_stats_rows assume).
int mcamd_conv_q8_w4_raw_launch(IgemmArgs& a, const void* gshift, const void* wexp, hipStream_t st) {
    const int npad = round_up_int(a.N, 256);
    const Q8Choice c = mcamd_q8_choice(a.M, a.N, MCAMD_Q8_FORM_RAW);
    return q8_dispatch(c, "conv_fwd_q8_w4_raw", [&](auto t, auto f8) {
        return conv_q8_w4_raw_launch_t<decltype(t), decltype(f8)::value>(a, c, (const char*)gshift, npad, (const int*)wexp, st);
    });
}

// ---------------------------------------------------------------------------------------
// packer: fp32 OIHW master * mask -> codes [Npad][ktot / 2] + shift bytes [ktot / 64][Npad][2] + exponents [Npad]
// ---------------------------------------------------------------------------------------
// the lane-local order of a chunk's k: piece h (16 code bytes), t in [0, 32) -> position in the 64-k chunk
__device__ __forceinline__ int w4_kk(int h, int t) { return t < 16 ? 16 * h + t : 32 + 16 * h + (t - 16); }

// (the shift rule w4_group_shift and the round-to-grid step w4_code: w4_quant.h, shared with wpack.hip)

// One workgroup per row n < Npad.  The exponent is pack_q8_kernel's minus one (0 for an all-zero filter).  Then the row is
// walked four chunks at a time, every weight read once: thread t stages the scaled w * mask of position t of the 256 (packed
// order [cb][tap][64]) in LDS; eight threads take the maxima and shifts of the eight groups; 128 threads write one code byte
// (two weights) each.  Pad rows: zero codes, shift byte 0, exponent 0.
__global__ __launch_bounds__(256) void pack_q8_w4_kernel(const float* __restrict__ w, const float* __restrict__ mask,
                                                         char* __restrict__ codes, char* __restrict__ gshift,
                                                         int* __restrict__ wexp, int cout, int cin, int ntaps, int npad) {
    __shared__ float red[256];
    __shared__ float sv[256];                                    // scaled weights of four chunks
    __shared__ int sg[8];                                        // their group shifts
    const int n = blockIdx.x, tid = threadIdx.x;
    const int ktot = cin * ntaps, nchunks = ktot / 64;
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
    const int e4 = w4_filter_exponent(amax);
    if (tid == 0) wexp[n] = e4;
    for (int q0 = 0; q0 < nchunks; q0 += 4) {                    // (uniform over the workgroup: the barriers below)
        {
            const int q = q0 + tid / 64, kk = tid % 64;
            float v = 0.f;
            if (n < cout && q < nchunks) {
                const int cb = q / ntaps, tap = q - cb * ntaps;
                const long long s = ((long long)n * cin + cb * 64 + kk) * ntaps + tap;
                v = ldexpf(w[s] * (mask ? mask[s] : 1.f), e4);   // exact: a power of two
            }
            sv[tid] = v;
        }
        __syncthreads();
        if (tid < 8) {                                           // group tid % 2 of chunk q0 + tid / 2
            float m = 0.f;
            for (int k = 0; k < 32; ++k) m = fmaxf(m, fabsf(sv[tid * 32 + k]));
            const int g = w4_group_shift(m);
            sg[tid] = g;
            const int q = q0 + tid / 2;
            if (q < nchunks) gshift[((long long)q * npad + n) * 2 + (tid & 1)] = (char)(n < cout ? g + 5 : 0);
        }
        __syncthreads();
        if (tid < 128) {                                         // code byte i of chunk q0 + tid / 32
            const int c = tid / 32, i = tid % 32, q = q0 + c;
            const int h = i / 16, d = (i % 16) / 4, b = i % 4;
            const int g = sg[2 * c + (d >= 2)];
            const unsigned lo = w4_code(sv[c * 64 + w4_kk(h, 8 * d + b)], g), hi = w4_code(sv[c * 64 + w4_kk(h, 8 * d + 4 + b)], g);
            if (q < nchunks) codes[(long long)n * (ktot / 2) + (long long)q * 32 + i] = (char)(lo | hi << 4);
        }
        __syncthreads();                                         // before the next four chunks overwrite sv / sg
    }
}

int mcamd_pack_q8_w4_launch(const float* w, const float* mask, void* codes, void* gshift, void* wexp, int cout, int cin, int ntaps,
                            hipStream_t st) {
    const int npad = round_up_int(cout, 256);
    hipLaunchKernelGGL(pack_q8_w4_kernel, dim3(npad), dim3(256), 0, st, w, mask, (char*)codes, (char*)gshift, (int*)wexp, cout, cin,
                       ntaps, npad);
    MCAMD_LAUNCH_CHECK("pack_q8_w4");
    return MCAMD_OK;
}

// ---------------------------------------------------------------------------------------
// expander: codes + shift bytes -> the e4m3 bytes [Npad][ktot] in mcamd_pack_q8's layout (the forward's own decode)
// ---------------------------------------------------------------------------------------
// One thread per (row, chunk, piece): 16 code bytes -> the two 16-byte runs [16 h, +16) and [32 + 16 h, +16) of the chunk.
__global__ __launch_bounds__(256) void unpack_q8_w4_kernel(const char* __restrict__ codes, const char* __restrict__ gshift,
                                                           char* __restrict__ wq, long long total, int ktot, int npad) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int upr = ktot / 32;                                   // pieces per row
    const long long n = t / upr;
    const int u = (int)(t - n * upr), q = u >> 1, h = u & 1;
    const i32x4_t c = *(const i32x4_t*)(codes + n * (ktot / 2) + 16 * u);
    const unsigned char* gp = (const unsigned char*)gshift + ((long long)q * npad + n) * 2;
    const i32x8_t o = w4_decode(c, (unsigned)gp[0] | (unsigned)gp[1] << 8);
    i32x4_t lo, hi;
#pragma unroll
    for (int i = 0; i < 4; ++i) lo[i] = o[i], hi[i] = o[4 + i];
    char* row = wq + n * ktot + (long long)q * 64;
    *(i32x4_t*)(row + 16 * h) = lo;
    *(i32x4_t*)(row + 32 + 16 * h) = hi;
}

int mcamd_unpack_q8_w4_launch(const void* codes, const void* gshift, void* wq, int cout, int cin, int ntaps, hipStream_t st) {
    const int npad = round_up_int(cout, 256), ktot = cin * ntaps;
    const long long total = (long long)npad * (ktot / 32);
    hipLaunchKernelGGL(unpack_q8_w4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const char*)codes,
                       (const char*)gshift, (char*)wq, total, ktot, npad);
    MCAMD_LAUNCH_CHECK("unpack_q8_w4");
    return MCAMD_OK;
}

// ---------------------------------------------------------------------------------------
// fake quantisation (training): codes + shift bytes + exponents -> fp32 OIHW w_q = grid[code] * 2^g * 2^-e4_f, the
// values the forward's decoded bytes stand for, read back through the documented layout.  The fp16 packers build the dgrad
// operand from it.  One thread per weight (the stores are contiguous; a code byte is shared by two threads, a shift byte by 32).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fakequant_q8_w4_kernel(const unsigned char* __restrict__ codes,
                                                              const unsigned char* __restrict__ gshift, const int* __restrict__ wexp,
                                                              float* __restrict__ out, long long total, int cin, int ntaps, int npad) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;         // OIHW: ((n * cin + c) * ntaps + tap)
    if (s >= total) return;
    const int tap = (int)(s % ntaps);
    const long long nc = s / ntaps;
    const int c = (int)(nc % cin), n = (int)(nc / cin);
    const int q = (c / 64) * ntaps + tap, kk = c % 64;                     // chunk and position in it (mcamd_pack_q8's order)
    const int j = kk >> 5, h = (kk >> 4) & 1, t = (kk & 15) + 16 * j;      // group, piece, t: kk = w4_kk(h, t)
    const int d = t >> 3, r = t & 7;                                       // byte i = 4 d + r % 4, high nibble for r >= 4
    const unsigned byte = codes[(long long)n * (cin * ntaps / 2) + (long long)q * 32 + 16 * h + 4 * d + (r & 3)];
    const unsigned code = r >= 4 ? byte >> 4 : byte & 15u;
    const int g = (int)gshift[((long long)q * npad + n) * 2 + j] - 5;
    const unsigned m = code & 7u;
    const float v = ldexpf(w4_grid(m), g - wexp[n]);                       // exact: a power of two
    out[s] = m == 0u ? 0.f : ((code & 8u) ? -v : v);
}

int mcamd_fakequant_q8_w4_launch(const void* codes, const void* gshift, const void* wexp, float* out, int cout, int cin, int ntaps,
                                 hipStream_t st) {
    const long long total = (long long)cout * cin * ntaps;
    hipLaunchKernelGGL(fakequant_q8_w4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const unsigned char*)codes,
                       (const unsigned char*)gshift, (const int*)wexp, out, total, cin, ntaps, round_up_int(cout, 256));
    MCAMD_LAUNCH_CHECK("fakequant_q8_w4");
    return MCAMD_OK;
}
