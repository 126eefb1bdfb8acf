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
// (byte-exact against the contract), or v_mfma_scale_f32_32x32x64_f8f6f4 with both e8m0 scales 1.0 (MCAMD_Q8_MFMA=1: half
// the MFMA time, not byte-exact; see conv_q8_kernel).  The power of two goes into the epilogue's per-filter scale (exact).
// As in conv_sparse.hip the weights are the A operand (rows = output channels)
// and the pixels the columns, so that a lane's four accumulator rows are four consecutive channels of one pixel: one
// 32-bit word of output bytes.
//
// Operand form: K order [channel block of 64][tap][64 channels]; one K chunk = 64 k = one 64-byte LDS row per weight row /
// pixel, staged by global_load_lds_dwordx4 (source address swizzled as in conv_igemm.hip).  Lane (r, h) of an MFMA reads
// bytes [16 h, 16 h + 16) and [32 + 16 h, 32 + 16 h + 16) of row r for BOTH operands: a k permutation common to A and B
// (tools/f8_probe.hip; the F8 phase of conv_igemm_pp.hip reads the same way).  Against the fp16 kernels a chunk carries
// twice the k per staged byte (and, with the fp8 MFMA, per MFMA cycle).
//
// Epilogue: the tile is laid down in LDS as [pixel][channel] in the format of each destination -- e4m3(2 v) bytes for a
// destination an fp8 block reads (ONE rounding from fp32), fp16 otherwise (conv_epi.h: write_ch_tile) -- and stored PLAIN /
// POOL (+ the optional full-resolution copy y2) / REORG by the store every forward implicit-GEMM kernel uses
// (store_pad_tile).  MaxPool of bytes is taken on the order-preserving key of the code (q is monotone: the maximum of the
// bytes is the byte of the maximum; -0 sorts below +0).
#include "kernels.h"
#include "conv_epi.h"
#include "q8_exp.h"

// F8MFMA = false (the default): the staged bytes are converted to fp16 in registers and multiplied by
// v_mfma_f32_32x32x16_f16, whose sum of the (exact) products is an fp32 sum -- the arithmetic of the contract, byte for
// byte.  F8MFMA = true (MCAMD_Q8_MFMA=1): one v_mfma_scale_f32_32x32x64_f8f6f4 per block and chunk, half the MFMA time --
// but that instruction (and the non-scaled fp8 one) drops products more than ~14 bits below the largest of their group
// of 8, which flips ~6e-4 of the output bytes to the adjacent code.
//
// RAW (training, Darknet.precision = "fp8-qat"): the same main loop with the MCAMD_EPI_RAW_F32 epilogue --
// y[m][n] = 2^-(e[n] + 1) * S as fp32 [M][y_ld] (the power of two is exact) plus, per channel, the sum and the sum of squares
// of those fp32 values over the workgroup's pixel tile: slab row = the pixel tile mt, every row written, fixed order, no
// atomics (conv_epi.h: store_raw32_ch_tile, shared with conv_q8_w4.hip's training kernel).
//
// BORDER (slim models; conv_q8_border_kernel below): the epilogue adds the fp32 table entry of the pixel's
// border class to the raw value 2^-(e[n] + 1) * S in front of the affine step (conv_epi.h: Q8Border).
template <int BMW, int BNP, int WM, int WN, int NSTAGE, bool F8MFMA, bool RAW, bool BORDER>
__device__ __forceinline__ void conv_q8_block(const IgemmArgs& __restrict__ a, const int* __restrict__ wexp, int y_f8, int y2_f8,
                                              const float* __restrict__ border, int border_ld) {
    constexpr int WAVES_N = BNP / WN;
    constexpr int NT = (BMW / WM) * (BNP / WN) * 64;
    constexpr int BK = 64, CPR = 4;                // 64 e4m3 k per 64-byte LDS row: four 16-byte chunks
    constexpr int A_SLOTS = BMW * CPR, B_SLOTS = BNP * CPR;
    constexpr int A_IT = A_SLOTS / NT, B_IT = B_SLOTS / NT;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int STAGE_BYTES = (A_SLOTS + B_SLOTS) * 16;
    constexpr int DPS = A_IT + B_IT;               // DMA instructions per stage and wave
    static_assert(A_SLOTS % NT == 0 && B_SLOTS % NT == 0, "whole workgroups per DMA round");
    static_assert(NSTAGE >= 2 && NSTAGE <= 3, "LDS ring depth");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    const int nchunks = a.ktot / BK;
    const char* xg = (const char*)a.x;             // byte operands: every stride of `a` counts bytes
    const char* wg = (const char*)a.w;

    long long wbase[A_IT];
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPR, phys = slot % CPR;
        wbase[it] = (long long)(nt * BMW + row) * a.ktot + (phys ^ swz<CPR>(row)) * 16;   // rows < Npad = round_up(N, 256)
    }
    long long xbase[B_IT];
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPR, phys = slot % CPR;
        xbase[it] = tile_x_base(a, a.dst_mode != 0, mt * BNP + row) + (phys ^ swz<CPR>(row)) * 16;
    }

    f32x16_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto stage = [&](int q, int buf) {
        const int cb = q / a.ntaps, tap = q - cb * a.ntaps;      // one chunk per tap of a 64-channel block
        const int koff = a.tap_off[tap] + cb * BK;
        char* sa = smem + buf * STAGE_BYTES;
        char* sb = sa + A_SLOTS * 16;
#pragma unroll
        for (int it = 0; it < A_IT; ++it) glds16(wg + wbase[it] + (long long)q * BK, sa + (it * NT + wave * 64) * 16);
#pragma unroll
        for (int it = 0; it < B_IT; ++it) glds16(xg + xbase[it] + koff, sb + (it * NT + wave * 64) * 16);
    };

    // fragment addresses: row = block row + (lane & 31), 16-byte chunks h and 2 + h of the row (swizzled)
    const int lrow = lane & 31, hh = lane >> 5;
    const int SC = 127 * 0x01010101;               // e8m0 1.0 in all four scale bytes

#pragma unroll
    for (int p = 0; p < NSTAGE - 1; ++p)
        if (p < nchunks) stage(p, p);
    int sidx = 0;
    for (int q = 0; q < nchunks; ++q) {
        int issued = q + NSTAGE - 1;
        if (issued > nchunks) issued = nchunks;
        const int inflight = issued - q - 1;
        if (NSTAGE == 2 || inflight == 0) wait_vmcnt<0>();
        else wait_vmcnt<DPS>();
        __builtin_amdgcn_s_barrier();              // chunk q landed for every wave; every wave is done with chunk q-1
        if (q + NSTAGE - 1 < nchunks) {
            int ns = sidx + NSTAGE - 1;
            if (ns >= NSTAGE) ns -= NSTAGE;
            stage(q + NSTAGE - 1, ns);
        }
        const char* sa = smem + sidx * STAGE_BYTES;
        const char* sb = sa + A_SLOTS * 16;
        sidx = sidx + 1 == NSTAGE ? 0 : sidx + 1;
        i32x8_t af[TM], bf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = wm * WM + i * 32 + lrow;
            const i32x4_t lo = *(const i32x4_t*)(sa + (row * CPR + (hh ^ swz<CPR>(row))) * 16);
            const i32x4_t hi = *(const i32x4_t*)(sa + (row * CPR + ((2 + hh) ^ swz<CPR>(row))) * 16);
            af[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int row = wn * WN + j * 32 + lrow;
            const i32x4_t lo = *(const i32x4_t*)(sb + (row * CPR + (hh ^ swz<CPR>(row))) * 16);
            const i32x4_t hi = *(const i32x4_t*)(sb + (row * CPR + ((2 + hh) ^ swz<CPR>(row))) * 16);
            bf[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
        // Inline assembly as in conv_igemm_pp.hip (through the builtin hipcc does not accumulate in place).  The operands
        // come from LDS reads the compiler waits for; the blocks are independent; the epilogue's reads are padded below.
        if constexpr (F8MFMA) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    asm volatile("v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
                                 : "+v"(acc[i][j])
                                 : "v"(af[i]), "v"(bf[j]), "v"(SC), "v"(SC));
        } else {
            // four 16-k steps: 8-byte piece s of the lane's 32 bytes of both operands (lanes h = 0 / 1 hold disjoint k)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                h8_t a16[TM], b16[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a16[i] = q8_to_f16(af[i][2 * s4], af[i][2 * s4 + 1]);
#pragma unroll
                for (int j = 0; j < TN; ++j) b16[j] = q8_to_f16(bf[j][2 * s4], bf[j][2 * s4 + 1]);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a16[i], b16[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    if constexpr (F8MFMA) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // last (assembly) MFMA -> VALU reads of the accumulators

    // ------------------------------- epilogue -------------------------------
    __syncthreads();                               // every wave is done with the stage buffers
    if constexpr (RAW) {
        static_assert(raw32_ch_lds_bytes(BMW, BNP, WM, WN) <= NSTAGE * STAGE_BYTES, "raw epilogue inside the ring");
        store_raw32_ch_tile<BMW, BNP, WM, WN>(a, acc, wexp, smem, mt, nt, wm, wn, wave, lane, tid);   // (conv_epi.h)
        return;
    }
    const bool has2 = a.y2 != nullptr;
    const bool need_b = y_f8 || (has2 && y2_f8), need_h = !y_f8 || (has2 && !y2_f8);
    // tile rows are PB = BMW + 8 elements apart: the 32 pixels of a wave's write then fall on 32 different LDS banks (a
    // pitch of BMW puts them all on one or two)
    constexpr int PB = BMW + 8;
    char* bt = smem;                               // [BNP][PB] e4m3 tile
    half_t* ht = (half_t*)(smem + (need_b ? BNP * PB : 0));   // [BNP][PB] fp16 tile
    // the per-filter scale with the power of two of the packed weights and of the 2 x activations taken back (exact)
    const float* scale = a.scale;
    bool sat;
    if constexpr (BORDER)
        sat = write_ch_tile<BMW, PB, WM, WN>(a, acc, [scale](int n) { return scale ? scale[n] : 1.f; }, need_b, need_h, bt, ht, nt, wm,
                                             wn, lane, Q8Border{border, wexp, border_ld, mt * BNP});
    else
        sat = write_ch_tile<BMW, PB, WM, WN>(a, acc, [scale, wexp](int n) { return ldexpf(scale ? scale[n] : 1.f, -(wexp[n] + 1)); },
                                             need_b, need_h, bt, ht, nt, wm, wn, lane);
    __syncthreads();
    store_pad_tile<BNP, BMW, PB, NT>(a, bt, ht, y_f8 != 0, y2_f8 != 0, mt, nt, tid);
    if (sat && a.overflow) atomicOr(a.overflow, 1);
}

template <int BMW, int BNP, int WM, int WN, int NSTAGE, bool F8MFMA, bool RAW>
__global__ __launch_bounds__((BMW / WM) * (BNP / WN) * 64)
void conv_q8_kernel(IgemmArgs a, const int* __restrict__ wexp, int y_f8, int y2_f8) {
    conv_q8_block<BMW, BNP, WM, WN, NSTAGE, F8MFMA, RAW, false>(a, wexp, y_f8, y2_f8, nullptr, 0);
}

// ... with a border table (inference epilogue only)
template <int BMW, int BNP, int WM, int WN, int NSTAGE, bool F8MFMA>
__global__ __launch_bounds__((BMW / WM) * (BNP / WN) * 64)
void conv_q8_border_kernel(IgemmArgs a, const int* __restrict__ wexp, int y_f8, int y2_f8, const float* __restrict__ border,
                           int border_ld) {
    conv_q8_block<BMW, BNP, WM, WN, NSTAGE, F8MFMA, false, true>(a, wexp, y_f8, y2_f8, border, border_ld);
}

template <int BMW, int BNP, int WM, int WN, int NSTAGE, bool F8MFMA, bool RAW = false>
static int conv_q8_launch_t(IgemmArgs& a, const Q8Choice& c, const int* wexp, int y_f8, int y2_f8, hipStream_t st,
                            const float* border = nullptr, int border_ld = 0) {
    constexpr int NT = (BMW / WM) * (BNP / WN) * 64;
    constexpr int RING = NSTAGE * (BMW + BNP) * 64;
    constexpr int PB = BMW + 8;                    // tile row pitch (conv_q8_kernel)
    constexpr int TILES = BNP * PB * 3;            // a byte and an fp16 tile (destinations of both formats)
    constexpr int LDS = RING > TILES ? RING : TILES;
    const bool has2 = a.y2 != nullptr;
    const bool mixed = (y_f8 || (has2 && y2_f8)) && (!y_f8 || (has2 && !y2_f8));
    const int lds = (mixed && !RAW) ? LDS : (RING > BNP * PB * 2 ? RING : BNP * PB * 2);   // (RAW: its tiles lie inside the ring)
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    if constexpr (!RAW) {
        if (border) {                              // (the same tile, ring and LDS as the launch without a table)
            auto kern = conv_q8_border_kernel<BMW, BNP, WM, WN, NSTAGE, F8MFMA>;
            MCAMD_LDS_OPT_IN(kern, LDS);
            hipLaunchKernelGGL(kern, dim3(c.grid), dim3(NT), lds, st, a, wexp, y_f8, y2_f8, border, border_ld);
            MCAMD_LAUNCH_CHECK("conv_fwd_q8_slim");
            return MCAMD_OK;
        }
    }
    auto kern = conv_q8_kernel<BMW, BNP, WM, WN, NSTAGE, F8MFMA, RAW>;
    MCAMD_LDS_OPT_IN(kern, LDS);
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(NT), lds, st, a, wexp, y_f8, y2_f8);
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
// The grid is whole rounds of 8 pixel tiles (xcd_tile).
Q8Choice mcamd_q8_choice(long long M, int N, int form) {
    (void)form;
    Q8Choice c;
    c.f8mfma = MCAMD_ENV_INT("MCAMD_Q8_MFMA", 0) ? 1 : 0;
    c.bnp = 128;
    c.stages = 3;
    if (c.f8mfma && N >= 256) c.bmw = 256;
    else c.bmw = N >= 128 ? 128 : 64;
    c.mtiles = (int)((M + c.bnp - 1) / c.bnp);
    c.ntiles = (N + c.bmw - 1) / c.bmw;
    c.grid = (c.mtiles + 7) / 8 * 8 * c.ntiles;
    return c;
}

// `border` (mcamd_conv_fwd_q8_slim; inference epilogue only): fp32 [16][border_ld] table added by pixel class, or NULL.
int mcamd_conv_q8_launch(IgemmArgs& a, const void* wexp, int y_f8, int y2_f8, hipStream_t st, const float* border, int border_ld) {
    const int* we = (const int*)wexp;
    const bool raw = a.mode == MCAMD_EPI_RAW_F32;  // training: fp32 y + statistics, the same tile per filter count
    const Q8Choice c = mcamd_q8_choice(a.M, a.N, raw ? MCAMD_Q8_FORM_RAW : border ? MCAMD_Q8_FORM_BORDER : MCAMD_Q8_FORM_INFER);
    if (c.bnp == 128 && c.stages == 3) {
        if (raw) {
            if (c.f8mfma && c.bmw == 256) return conv_q8_launch_t<256, 128, 64, 64, 3, true, true>(a, c, we, 0, 0, st);
            if (c.f8mfma && c.bmw == 128) return conv_q8_launch_t<128, 128, 64, 64, 3, true, true>(a, c, we, 0, 0, st);
            if (c.f8mfma && c.bmw == 64) return conv_q8_launch_t<64, 128, 32, 64, 3, true, true>(a, c, we, 0, 0, st);
            if (!c.f8mfma && c.bmw == 128) return conv_q8_launch_t<128, 128, 64, 64, 3, false, true>(a, c, we, 0, 0, st);
            if (!c.f8mfma && c.bmw == 64) return conv_q8_launch_t<64, 128, 32, 64, 3, false, true>(a, c, we, 0, 0, st);
        } else {
            if (c.f8mfma && c.bmw == 256) return conv_q8_launch_t<256, 128, 64, 64, 3, true>(a, c, we, y_f8, y2_f8, st, border, border_ld);
            if (c.f8mfma && c.bmw == 128) return conv_q8_launch_t<128, 128, 64, 64, 3, true>(a, c, we, y_f8, y2_f8, st, border, border_ld);
            if (c.f8mfma && c.bmw == 64) return conv_q8_launch_t<64, 128, 32, 64, 3, true>(a, c, we, y_f8, y2_f8, st, border, border_ld);
            if (!c.f8mfma && c.bmw == 128) return conv_q8_launch_t<128, 128, 64, 64, 3, false>(a, c, we, y_f8, y2_f8, st, border, border_ld);
            if (!c.f8mfma && c.bmw == 64) return conv_q8_launch_t<64, 128, 32, 64, 3, false>(a, c, we, y_f8, y2_f8, st, border, border_ld);
        }
    }
    mcamd_set_error("conv_fwd_q8: no kernel instance %d x %d, fp8 MFMA %d, %d stages", c.bmw, c.bnp, c.f8mfma, c.stages);
    return MCAMD_EINVAL;
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
