// MXFP4 activations x MXFP4 weights (an addition beyond the reference: Darknet.precision = "fp4-mx"): the
// "fp8-w4-mx" block with its PIXEL operand in 4 bits too -- v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz:4 AND blgp:4, four
// registers and one e8m0 scale byte per lane on both sides, the form tools/f4_probe.hip measured at 1.56x the fp8 issue rate.
// Two kernels: the cast pass that writes the activation format, and the implicit-GEMM forward that reads it.
//
//   S[n][m] = sum_{groups} 2^g[n] 2^s[m] * sum_{k in group} grid[wcode[n][k]] * grid[acode[pixel(m) + tap][c]]
//   v       = leaky(scale[n] * 2^-(e4[n] + 1) * S + shift[n])                              (q8_infer_epilogue, unchanged)
//
// Activation format (mcamd.h states it; mcamd_cast_a4_mx writes it from the engine's padded e4m3 buffer, whose bytes stand for
// 2 x): per buffer row -- a padded pixel -- and group of 32 consecutive channels the smallest s with max |value| <= 6 * 2^s
// (w4_quant.h's rule, unclamped: s in [-11, 7]) and w4_code(value, s) per channel:
//   codes   [rows][cin / 2] bytes, the even channel in the low nibble: channels [64 b + 32 h, + 32) of a row are the 16 bytes
//           at 32 b + 16 h -- one lane's four B registers (tools/f4x4_probe.hip: B's lane (c, h) holds k = 32 h + e, low nibble
//           first, as A's)
//   scales  [rows][cin / 64] 32-bit words: byte h = 127 + s of group h of the 64-channel block, bytes 2-3 zero.  A word, not a
//           byte pair, because it is staged by a 4-byte LDS-DMA per pixel and chunk: one aligned piece whatever cin / 64 is.
// Every (code, scale) pair stands for an e4m3 number (the inputs are multiples of 2^-9 and nothing saturates) but one: +-448 =
// 3.5 * 2^7 is a tie and goes to 4 * 2^7 = 512.  Elsewhere this block is the "fp8-w4-mx" block on a restricted set of
// activation bytes.
//
// The forward.  Weight side: conv_q8_w4_mx.hip's operands and half-row staging (Q8HalfRowsA<T, 2>), unchanged.  Pixel side, per
// 64-k chunk and workgroup of 128 pixels:
//   staging  256 code pieces of 16 bytes -- four wave-wide DMA instructions where the byte kernels issue eight -- and 128 scale
//            words, two 4-byte DMA instructions.  Piece (pixel p, half h) lands in slot h * 128 + p: two PLANES of 128 x 16
//            bytes, not 32-byte rows.
//   banks    lane (r, h) of a block reads slot h * 128 + p0 + r with one ds_read_b128: the 16 lanes of a ds_read_b128 group
//            (common.h, swz) share h and read 16 CONSECUTIVE slots, 256 contiguous bytes = every one of the 64 banks once.
//            Rows of 32 bytes read as (r * 2 + h) * 16 are contiguous over the WAVE but not over a group: lanes r and r + 8 of
//            a group lie 256 bytes apart, a 2-way conflict by that model -- hence the planes.  No swizzle either way.
//   scales   behind the planes, one word per pixel: lane (r, h) reads byte 4 (p0 + r) + h with ds_read_u8 into byte 0 of its
//            scale register (op_sel 0), as the weight side does.
//   ring     a stage is 4 608 pixel bytes (the byte kernels: 8 192) + the weight half rows; FOUR stages where the family has
//            three fit the LDS the epilogue's tiles need anyway in every instance (profiles/q4_mx_resources.txt), so two
//            chunks stay in flight across each barrier.  One 64-k step per stage: cin % 128 != 0 is common (conv3, conv5, the
//            3 x 3 blocks' nine taps) and a two-step stage would need a tail form.
//   step     per 32 x 32 block four A registers, four B registers, one scale byte a side, then the MFMA in place (inline
//            assembly, `s_nop 1` in front as conv_q8_loop.h pads its strings, q8_mma_drain() behind the loop).  No VALU
//            instruction between the LDS reads and the MFMA.
// The instruction drops products far below the largest of their group as the fp8 form does: not byte-exact
// against a float64 sum on Gaussian operands, exact on operands whose partial sums are fp32 numbers (the tests' integer draws).
#include "conv_q8_loop.h"
#include "w4_quant.h"

// ---------------------------------------------------------------------------------------
// cast pass: e4m3 bytes [rows][ld], channels [choff, choff + cin) -> codes + scale words
// ---------------------------------------------------------------------------------------
// (a4_mag, the value of an e4m3 byte's low seven bits: w4_quant.h)
// One thread per 16 channels: one 16-byte load, the group maximum from the pair's other lane (DPP quad_perm [1, 0, 3, 2]; e4m3
// is monotone in its low seven bits, so the maximum is taken on them), 8 code bytes stored; lane 0 of a quad -- 64 channels --
// takes group 1's scale byte from lane 2 (quad_perm [2, 2, 2, 2]) and stores the block's scale word.  cin % 64 == 0: a quad
// never straddles a row or the end of the grid.
__global__ __launch_bounds__(256) void cast_a4_mx_kernel(const char* __restrict__ src, long long rows, int ld, int choff, int cin,
                                                         char* __restrict__ codes, int* __restrict__ scales) {
    const int ppr = cin / 16;                                    // pieces per row
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * ppr) return;
    const long long row = t / ppr;
    const int piece = (int)(t - row * ppr);
    const i32x4_t in = *(const i32x4_t*)(src + row * ld + choff + piece * 16);
    unsigned top = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned m7 = (unsigned)in[d] & 0x7f7f7f7fu;
        top = max(max(top, m7 & 0xffu), max((m7 >> 8) & 0xffu, max((m7 >> 16) & 0xffu, m7 >> 24)));
    }
    top = max(top, (unsigned)__builtin_amdgcn_update_dpp(0, (int)top, 0xb1, 0xf, 0xf, true));
    const int s = w4_group_shift_free(a4_mag(top));
    i32x2_t out;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        unsigned word = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned b = ((unsigned)in[2 * d + e / 4] >> (8 * (e & 3))) & 0xffu;
            const float v = a4_mag(b);
            word |= w4_code((b & 0x80u) ? -v : v, s) << (4 * e);
        }
        out[d] = (int)word;
    }
    *(i32x2_t*)(codes + row * (cin / 2) + piece * 8) = out;
    const int sb = 127 + s;
    const int sb1 = __builtin_amdgcn_update_dpp(0, sb, 0xaa, 0xf, 0xf, true);
    if ((piece & 3) == 0) scales[row * (cin / 64) + piece / 4] = sb | sb1 << 8;
}

int mcamd_cast_a4_mx_launch(const void* x8, long long rows, int ld, int choff, int cin, void* codes, void* scales, hipStream_t st) {
    const long long total = rows * (cin / 16);
    hipLaunchKernelGGL(cast_a4_mx_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const char*)x8, rows, ld, choff, cin,
                       (char*)codes, (int*)scales);
    MCAMD_LAUNCH_CHECK("cast_a4_mx");
    return MCAMD_OK;
}

// ---------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------
// conv_q8_loop.h's tile constants for the epilogue and the weight staging + this kernel's pixel stage and ring depth
template <int BMW_, int BNP_, int WM_, int WN_>
struct Q4Tile : Q8Tile<BMW_, BNP_, WM_, WN_, 3> {
    using Base = Q8Tile<BMW_, BNP_, WM_, WN_, 3>;
    static constexpr int RING_STAGES = 4;
    static constexpr int B4_CODE = BNP_ * 32, B4_BYTES = B4_CODE + BNP_ * 4;       // two planes of 16-byte pieces + the scale words
    static constexpr int NW = Base::NT / 64, CODE_WAVES = BNP_ * 2 / 64, SCALE_WAVES = BNP_ / 64;
    static_assert(CODE_WAVES <= NW && SCALE_WAVES <= NW && BNP_ % 64 == 0, "whole waves per DMA instruction");
    static_assert(((NW - SCALE_WAVES) * 64) % BNP_ == 0, "a scale wave's lanes name the pixels tid % BNP");
};

// B: thread tid stages the code piece (pixel tid % BNP, half (tid / BNP) % 2) -- waves [0, CODE_WAVES) -- and the scale word
// of pixel tid % BNP -- the last SCALE_WAVES waves.  `a` addresses buffer ROWS (x_ld 1, x_off 0: tile_x_base and tap_off
// count padded pixels); a row is cin / 2 code bytes and cin / 16 scale bytes.
template <class T>
struct Q4PixelsB {
    static constexpr int DMIN = T::CODE_WAVES >= T::NW ? 1 : 0;   // DMA instructions EVERY wave issues per stage
    long long cbase, sbase;
    const char* xs;
    int crow, srow;
    __device__ __forceinline__ void setup(const IgemmArgs& __restrict__ a, const void* xscales, int mt, int tid) {
        crow = a.cin_tap / 2, srow = a.cin_tap / 16;
        const long long prow = tile_x_base(a, a.dst_mode != 0, mt * T::BNP + tid % T::BNP);
        cbase = prow * crow + ((tid / T::BNP) & 1) * 16;
        sbase = prow * srow;
        xs = (const char*)xscales;
    }
    __device__ __forceinline__ void issue(const IgemmArgs& __restrict__ a, int q, char* sb, int wave) const {
        const int cb = q / a.ntaps, tap = q - cb * a.ntaps;      // one chunk per tap of a 64-channel block
        const long long trow = a.tap_off[tap];
        if (wave < T::CODE_WAVES) glds16((const char*)a.x + cbase + trow * crow + cb * 32, sb + wave * 1024);
        if (wave >= T::NW - T::SCALE_WAVES)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xs + sbase + trow * srow + cb * 4),
                                             (__attribute__((address_space(3))) void*)(sb + T::B4_CODE + (wave - (T::NW - T::SCALE_WAVES)) * 256),
                                             4, 0, 0);
    }
};

// conv_q8_loop.h's q8_ring at this kernel's depth and with its pixel operand: body(sa, sb) once per chunk, in order; chunks
// i+1 .. i+RING_STAGES-2 stay in flight across the barrier (a wave that issues more than DMIN per stage waits for more:
// in-order completion).  Fewer chunks than the ring is deep fill part of the prologue.
template <class T, class A, class Body>
__device__ __forceinline__ void q4_ring(const IgemmArgs& __restrict__ a, const A& aop, const Q4PixelsB<T>& bop, int n, char* smem,
                                        const Q8Wave& w, Body body) {
    constexpr int NS = T::RING_STAGES, STAGE_BYTES = A::BYTES + T::B4_BYTES, DMIN = A::DMIN + Q4PixelsB<T>::DMIN;
    static_assert(NS == 4 && DMIN >= 1, "the counted waits below");
    auto stage = [&](int q, int buf) {
        char* sa = smem + buf * STAGE_BYTES;
        aop.issue(a, q, sa, w.wave);
        bop.issue(a, q, sa + A::BYTES, w.wave);
    };
#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
        if (p < n) stage(p, p);
    int sidx = 0;
    for (int i = 0; i < n; ++i) {
        int issued = i + NS - 1;
        if (issued > n) issued = n;
        const int inflight = issued - i - 1;
        if (inflight >= 2) wait_vmcnt<2 * DMIN>();
        else if (inflight == 1) wait_vmcnt<DMIN>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();              // chunk i landed for every wave; every wave is done with chunk i-1
        if (i + NS - 1 < n) stage(i + NS - 1, (sidx + NS - 1) % NS);
        const char* sa = smem + sidx * STAGE_BYTES;
        sidx = sidx + 1 == NS ? 0 : sidx + 1;
        body(sa, sa + A::BYTES);
    }
}

template <class T>
using Q4RowsA = Q8HalfRowsA<T, 2>;               // conv_q8_w4_mx.hip's weight stage: 32 code bytes + two e8m0 bytes per row

// a lane's fragment addresses, taken once in front of the K loop (offsets into a stage's A region / B region)
template <class T>
struct Q4Lane {
    int a[T::TM], asc[T::TM], b[T::TN], bsc[T::TN];
    __device__ __forceinline__ explicit Q4Lane(const Q8Wave& w) {
        const int hh = w.lane >> 5;
#pragma unroll
        for (int i = 0; i < T::TM; ++i) {
            const int row = w.wm * T::WM + i * 32 + (w.lane & 31);
            a[i] = (row * 2 + hh) * 16;
            asc[i] = Q4RowsA<T>::SLOTS * 16 + row * 2 + hh;
        }
#pragma unroll
        for (int j = 0; j < T::TN; ++j) {
            const int p = w.wn * T::WN + j * 32 + (w.lane & 31);
            b[j] = (hh * T::BNP + p) * 16;
            bsc[j] = T::B4_CODE + p * 4 + hh;
        }
    }
};

// acc += A(e2m1, 4 registers, scale byte 0 of sa) x B(e2m1, 4 registers, scale byte 0 of sb); accumulates in place
#define Q4_MX_MFMA "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4 blgp:4"
template <class T>
__device__ __forceinline__ void q4mx_step(f32x16_t (&acc)[T::TM][T::TN], const char* sa, const char* sb, const Q4Lane<T>& ln) {
    i32x4_t af[T::TM], bf[T::TN];
    int as[T::TM], bs[T::TN];
#pragma unroll
    for (int i = 0; i < T::TM; ++i) {
        af[i] = *(const i32x4_t*)(sa + ln.a[i]);
        as[i] = *(const unsigned char*)(sa + ln.asc[i]);
    }
#pragma unroll
    for (int j = 0; j < T::TN; ++j) {
        bf[j] = *(const i32x4_t*)(sb + ln.b[j]);
        bs[j] = *(const unsigned char*)(sb + ln.bsc[j]);
    }
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j)
            asm volatile("s_nop 1\n\t" Q4_MX_MFMA : "+v"(acc[i][j]) : "v"(af[i]), "v"(bf[j]), "v"(as[i]), "v"(bs[j]));
}

template <class T>
__global__ __launch_bounds__(T::NT) void conv_q4_mx_kernel(IgemmArgs a, const char* __restrict__ wscales, int npad,
                                                           const int* __restrict__ wexp, const char* __restrict__ xscales, int y_f8,
                                                           int y2_f8) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Q8Wave w = q8_wave<T>();
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    Q4RowsA<T> aop;
    aop.setup(a, wscales, npad, nt, w.tid);
    Q4PixelsB<T> bop;
    bop.setup(a, xscales, mt, w.tid);
    f32x16_t acc[T::TM][T::TN];
    q8_zero(acc);
    const Q4Lane<T> ln(w);
    q4_ring<T>(a, aop, bop, a.ktot / T::BK, smem, w, [&](const char* sa, const char* sb) { q4mx_step<T>(acc, sa, sb, ln); });
    q8_mma_drain<true>();
    __syncthreads();                               // every wave is done with the stage buffers
    q8_infer_epilogue<T>(a, acc, wexp, y_f8, y2_f8, smem, mt, nt, w);
}

template <class T>
static int conv_q4_mx_launch_t(IgemmArgs& a, const Q8Choice& c, const char* wscales, int npad, const int* wexp, const char* xscales,
                               int y_f8, int y2_f8, hipStream_t st) {
    constexpr int RING = T::RING_STAGES * (Q4RowsA<T>::BYTES + T::B4_BYTES);
    auto kern = conv_q4_mx_kernel<T>;
    MCAMD_LDS_OPT_IN(kern, q8_infer_lds_max(RING, T::TILE_BYTES));
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(T::NT), q8_infer_lds(RING, T::TILE_BYTES, a, y_f8, y2_f8), st, a, wscales, npad, wexp,
                       xscales, y_f8, y2_f8);
    MCAMD_LAUNCH_CHECK("conv_fwd_q4_mx");
    return MCAMD_OK;
}

// The same kernel with MXFP4 destinations (mcamd_conv_fwd_q4_mx_a4): conv_q4_mx_kernel's K loop, then the
// epilogue whose store quantises the byte tile on its way out (conv_epi.h store_pad_tile_a4) -- its consumer reads the codes
// and scale words with no cast pass.  fy / fy2: MCAMD_FMT_* per destination.  A kernel of its own, so that every instance
// above stays what it was.
template <class T>
__global__ __launch_bounds__(T::NT) void conv_q4_mx_a4_kernel(IgemmArgs a, const char* __restrict__ wscales, int npad,
                                                              const int* __restrict__ wexp, const char* __restrict__ xscales, int fy,
                                                              int fy2, A4Dst d, A4Dst d2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Q8Wave w = q8_wave<T>();
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    Q4RowsA<T> aop;
    aop.setup(a, wscales, npad, nt, w.tid);
    Q4PixelsB<T> bop;
    bop.setup(a, xscales, mt, w.tid);
    f32x16_t acc[T::TM][T::TN];
    q8_zero(acc);
    const Q4Lane<T> ln(w);
    q4_ring<T>(a, aop, bop, a.ktot / T::BK, smem, w, [&](const char* sa, const char* sb) { q4mx_step<T>(acc, sa, sb, ln); });
    q8_mma_drain<true>();
    __syncthreads();                               // every wave is done with the stage buffers
    q8_infer_epilogue_a4<T>(a, acc, wexp, fy, fy2, d, d2, smem, mt, nt, w);
}

template <class T>
static int conv_q4_mx_a4_launch_t(IgemmArgs& a, const Q8Choice& c, const char* wscales, int npad, const int* wexp, const char* xscales,
                                  int fy, int fy2, const A4Dst& d, const A4Dst& d2, hipStream_t st) {
    constexpr int RING = T::RING_STAGES * (Q4RowsA<T>::BYTES + T::B4_BYTES);
    auto kern = conv_q4_mx_a4_kernel<T>;
    MCAMD_LDS_OPT_IN(kern, q8_infer_lds_max(RING, T::TILE_BYTES));
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    // (an MXFP4 destination is quantised from the byte tile: sized as an e4m3 one; the kernel sees an MXFP4 copy in d2 alone)
    const int lds = q8_infer_lds(RING, T::TILE_BYTES, a, fy != MCAMD_FMT_F16, fy2 != MCAMD_FMT_F16);
    if (fy2 == MCAMD_FMT_A4) a.y2 = nullptr;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(T::NT), lds, st, a, wscales, npad, wexp, xscales, fy, fy2, d, d2);
    MCAMD_LAUNCH_CHECK("conv_fwd_q4_mx_a4");
    return MCAMD_OK;
}

int mcamd_conv_q4_mx_a4_launch(IgemmArgs& a, const void* xscales, const void* wscales, const void* wexp, int fy, int fy2,
                               const A4Dst& d, const A4Dst& d2, hipStream_t st) {
    const int npad = round_up_int(a.N, 256);
    const Q8Choice c = mcamd_q4_mx_choice(a.M, a.N);
    const char *ws = (const char*)wscales, *xs = (const char*)xscales;
    const int* we = (const int*)wexp;
    if (c.bmw == 256) return conv_q4_mx_a4_launch_t<Q4Tile<256, 128, 64, 64>>(a, c, ws, npad, we, xs, fy, fy2, d, d2, st);
    if (c.bmw == 128) return conv_q4_mx_a4_launch_t<Q4Tile<128, 128, 64, 64>>(a, c, ws, npad, we, xs, fy, fy2, d, d2, st);
    return conv_q4_mx_a4_launch_t<Q4Tile<64, 128, 32, 64>>(a, c, ws, npad, we, xs, fy, fy2, d, d2, st);
}

// mcamd_q8_w4_mx_choice's three tiles (256 / 128 / 64 filters x 128 pixels) on a four-stage ring.  Every instance compiles
// without scratch memory (profiles/q4_mx_resources.txt).
Q8Choice mcamd_q4_mx_choice(long long M, int N) {
    Q8Choice c = mcamd_q8_w4_mx_choice(M, N);
    c.stages = 4;
    return c;
}

// a: geometry in buffer rows (x_ld 1, x_off 0), a.x = the activation codes, a.w = the weight codes
int mcamd_conv_q4_mx_launch(IgemmArgs& a, const void* xscales, const void* wscales, const void* wexp, int y_f8, int y2_f8,
                            hipStream_t st) {
    const int npad = round_up_int(a.N, 256);
    const Q8Choice c = mcamd_q4_mx_choice(a.M, a.N);
    const char *ws = (const char*)wscales, *xs = (const char*)xscales;
    const int* we = (const int*)wexp;
    if (c.bmw == 256) return conv_q4_mx_launch_t<Q4Tile<256, 128, 64, 64>>(a, c, ws, npad, we, xs, y_f8, y2_f8, st);
    if (c.bmw == 128) return conv_q4_mx_launch_t<Q4Tile<128, 128, 64, 64>>(a, c, ws, npad, we, xs, y_f8, y2_f8, st);
    return conv_q4_mx_launch_t<Q4Tile<64, 128, 32, 64>>(a, c, ws, npad, we, xs, y_f8, y2_f8, st);
}
