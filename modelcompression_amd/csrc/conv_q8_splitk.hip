// Split-K forward for low-batch fp8 inference (Darknet.precision = "fp8-splitk"): the byte K loop of
// conv_q8.hip with the K axis cut into S slices, by the launch design of conv_splitk.hip -- for the layers whose M = B*H*W
// pixels give conv_q8_kernel a handful of 128 x 128 tiles that each walk the whole K axis alone (YOLOv2's 13x13 layers at
// B = 1: 16 working workgroups on 256 CUs, 144-180 dependent K chunks).
//
//   launch 1, q8_splitk_partial_kernel<F8MFMA>: workgroup (tile, slice s) multiplies the K chunks
//       [floor(s n / S), floor((s+1) n / S)) of the tile's n = ktot / 64 chunks -- the operands, the staging, the fragment
//       mapping and the MFMA order inside a chunk of conv_q8_block, in either MFMA form (MCAMD_Q8_MFMA) -- and stores its
//       fp32 accumulators, unrounded, to slab s of the workspace [S][Mpad][Npad] (pixels x channels, whole tiles).
//   launch 2, q8_splitk_finish_kernel: a 16-pixel x 64-channel tile per workgroup sums the S slabs of each element in slice
//       order 0 .. S-1 in fp32, applies the fp8 epilogue expression of write_ch_tile (conv_epi.h), lays the tile down in
//       LDS once per needed format (e4m3(2 v) bytes / saturated fp16) and calls store_pad_tile.
//
// The reduction is the launch boundary, for the reasons DESIGN.md 3p gives: no workgroup waits for, polls or counts another,
// there are no arrival counters and no fences, and the result is a function of the operands, the MFMA form and S only.  With
// S = 1 the pair computes what conv_q8_kernel computes, code for code: an element's accumulator sees the same instruction
// sequence whatever the tile, and the epilogue expression is the same one, contracted the same way (this file is compiled
// with conv_q8.hip's flags).
#include "kernels.h"
#include "conv_epi.h"

struct Q8SplitkArgs {
    IgemmArgs a;            // byte operands: every stride counts bytes (mcamd_conv_fwd_q8)
    const int* wexp;        // per-filter exponents of the packed weights
    float* ws;              // [slices][slab_elems]
    long long slab_elems;   // mtiles * 64 * npad
    int slices;
    int npad;               // ntiles * 64: floats per slab row
    int mtiles, ntiles;
    int y_f8, y2_f8;
};

constexpr int QSK_BMW = 64, QSK_BNP = 64;    // partial tile: 64 filters x 64 pixels, 4 waves of 32 x 32
constexpr int QSK_FR = 16, QSK_FC = 64;      // finish tile: 16 pixels x 64 channels

template <bool F8MFMA>
__global__ __launch_bounds__(256) void q8_splitk_partial_kernel(Q8SplitkArgs p) {
    constexpr int BMW = QSK_BMW, BNP = QSK_BNP, NT = 256, WAVES_N = 2, NSTAGE = 3;
    constexpr int BK = 64, CPR = 4;                // 64 e4m3 k per 64-byte LDS row: four 16-byte chunks
    constexpr int A_SLOTS = BMW * CPR, B_SLOTS = BNP * CPR;
    constexpr int STAGE_BYTES = (A_SLOTS + B_SLOTS) * 16;
    constexpr int DPS = 2;                         // DMA instructions per stage and wave: one weight piece, one pixel piece
    static_assert(A_SLOTS == NT && B_SLOTS == NT, "one DMA piece of each operand per thread and chunk");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const IgemmArgs& a = p.a;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    // the pixel tiles of one (filter tile, slice) on one XCD: they stage the same weight chunks
    int mt, grp;
    if (!xcd_tile(p.mtiles, p.ntiles * p.slices, mt, grp)) return;
    const int s = grp / p.ntiles, nt = grp - s * p.ntiles;
    const int nchunks = a.ktot / BK;
    const int q0 = (int)((long long)s * nchunks / p.slices), q1 = (int)((long long)(s + 1) * nchunks / p.slices);
    const int nloc = q1 - q0;
    const char* xg = (const char*)a.x;
    const char* wg = (const char*)a.w;

    const int srow = tid / CPR, sphys = tid % CPR;
    // (weight rows < round_up(N, 64) <= Npad = round_up(N, 256) exist: zero bytes behind the last filter)
    const long long wbase = (long long)(nt * BMW + srow) * a.ktot + (sphys ^ swz<CPR>(srow)) * 16;
    const long long xbase = tile_x_base(a, a.dst_mode != 0, mt * BNP + srow) + (sphys ^ swz<CPR>(srow)) * 16;

    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    auto stage = [&](int q, int buf) {
        const int cb = q / a.ntaps, tap = q - cb * a.ntaps;      // one chunk per tap of a 64-channel block
        const int koff = a.tap_off[tap] + cb * BK;
        char* sa = smem + buf * STAGE_BYTES;
        char* sb = sa + A_SLOTS * 16;
        glds16(wg + wbase + (long long)q * BK, sa + wave * 64 * 16);
        glds16(xg + xbase + koff, sb + wave * 64 * 16);
    };

    // fragment addresses: row = block row + (lane & 31), 16-byte chunks h and 2 + h of the row (swizzled)
    const int lrow = lane & 31, hh = lane >> 5;
    const int SC = 127 * 0x01010101;               // e8m0 1.0 in all four scale bytes

#pragma unroll
    for (int i = 0; i < NSTAGE - 1; ++i)
        if (i < nloc) stage(q0 + i, i);
    int sidx = 0;
    for (int i = 0; i < nloc; ++i) {
        int issued = i + NSTAGE - 1;
        if (issued > nloc) issued = nloc;
        const int inflight = issued - i - 1;
        if (inflight == 0) wait_vmcnt<0>();
        else wait_vmcnt<DPS>();
        __builtin_amdgcn_s_barrier();              // chunk i landed for every wave; every wave is done with chunk i-1
        if (i + NSTAGE - 1 < nloc) {
            int ns = sidx + NSTAGE - 1;
            if (ns >= NSTAGE) ns -= NSTAGE;
            stage(q0 + i + NSTAGE - 1, ns);
        }
        const char* sa = smem + sidx * STAGE_BYTES;
        const char* sb = sa + A_SLOTS * 16;
        sidx = sidx + 1 == NSTAGE ? 0 : sidx + 1;
        i32x8_t af, bf;
        {
            const int row = wm * 32 + lrow;
            const i32x4_t lo = *(const i32x4_t*)(sa + (row * CPR + (hh ^ swz<CPR>(row))) * 16);
            const i32x4_t hi = *(const i32x4_t*)(sa + (row * CPR + ((2 + hh) ^ swz<CPR>(row))) * 16);
            af = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
        {
            const int row = wn * 32 + lrow;
            const i32x4_t lo = *(const i32x4_t*)(sb + (row * CPR + (hh ^ swz<CPR>(row))) * 16);
            const i32x4_t hi = *(const i32x4_t*)(sb + (row * CPR + ((2 + hh) ^ swz<CPR>(row))) * 16);
            bf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
        // conv_q8_block's order inside a chunk (inline assembly for the fp8 MFMA as there: through the builtin hipcc does
        // not accumulate in place; the operands come from LDS reads the compiler waits for)
        if constexpr (F8MFMA) {
            asm volatile("v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
                         : "+v"(acc)
                         : "v"(af), "v"(bf), "v"(SC), "v"(SC));
        } else {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const h8_t a16 = q8_to_f16(af[2 * s4], af[2 * s4 + 1]);
                const h8_t b16 = q8_to_f16(bf[2 * s4], bf[2 * s4 + 1]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a16, b16, acc, 0, 0, 0);
            }
        }
    }
    if constexpr (F8MFMA) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // last (assembly) MFMA -> VALU reads of the accumulators

    // a lane's accumulator rows 4 g .. 4 g + 3 are four consecutive channels of one pixel: one 16-byte store per g; the four
    // stores of a wave fill whole 128-byte lines (32 channels of a pixel).  The slab is padded to whole tiles, so pixels past
    // the last one and channels past the last filter are stored too (never read back as results: the finish kernel's stores
    // mask them).
    float* slab = p.ws + (long long)s * p.slab_elems;
    const long long prow = (long long)(mt * BNP + wn * 32 + lrow) * p.npad + nt * BMW + wm * 32 + 4 * hh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[4 * g + e];
        *(f32x4_t*)(slab + prow + 8 * g) = v;
    }
}

__global__ __launch_bounds__(256) void q8_splitk_finish_kernel(Q8SplitkArgs p) {
    constexpr int NT = 256, PITCH = QSK_FC;
    __shared__ __attribute__((aligned(16))) char bt[QSK_FR * PITCH];       // [pixel][channel] e4m3 tile
    __shared__ __attribute__((aligned(16))) half_t ht[QSK_FR * PITCH];     // [pixel][channel] fp16 tile
    const IgemmArgs& a = p.a;
    const int tid = threadIdx.x;
    const int nt = blockIdx.x % p.ntiles, mt = blockIdx.x / p.ntiles;
    const int row = tid / (QSK_FC / 4), c4 = (tid % (QSK_FC / 4)) * 4;
    const int n0 = nt * QSK_FC + c4;
    // (rows up to round_up(M, 16) <= Mpad and columns up to Npad exist in every slab)
    const float* src = p.ws + (long long)(mt * QSK_FR + row) * p.npad + n0;
    f32x4_t acc = *(const f32x4_t*)src;
    for (int s = 1; s < p.slices; ++s) {           // slice order: the sum does not depend on scheduling
        const f32x4_t u = *(const f32x4_t*)(src + (long long)s * p.slab_elems);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += u[e];
    }
    const bool has2 = a.y2 != nullptr;
    const bool need_b = p.y_f8 || (has2 && p.y2_f8), need_h = !p.y_f8 || (has2 && !p.y2_f8);
    // write_ch_tile's expression: the per-filter scale with the power of two of the packed weights and of the 2 x
    // activations taken back (exact), then the affine step and the leaky slope
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int n = n0 + e;
        float sc = 1.f, sh = 0.f;
        if (n < a.N) {
            sc = ldexpf(a.scale ? a.scale[n] : 1.f, -(p.wexp[n] + 1));
            if (a.shift) sh = a.shift[n];
        }
        v[e] = acc[e] * sc + sh;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * a.slope;
    bool sat = false;
    if (need_b) *(int*)(bt + row * PITCH + c4) = e4m3_bytes4(v);
    if (need_h) {
        h4_t hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sat |= fabsf(v[e]) > 65504.f && mt * QSK_FR + row < a.M && n0 + e < a.N;
            hv[e] = (half_t)fminf(fmaxf(v[e], -65504.f), 65504.f);   // saturate, never inf
        }
        *(h4_t*)(ht + row * PITCH + c4) = hv;
    }
    __syncthreads();
    store_pad_tile<QSK_FR, QSK_FC, PITCH, NT>(a, bt, ht, p.y_f8 != 0, p.y2_f8 != 0, mt, nt, tid);
    if (sat && a.overflow) atomicOr(a.overflow, 1);
}

// a.* geometry and epilogue fields filled by the caller (mode MCAMD_EPI_PAD_F16, byte strides); p: mcamd_splitk_plan with
// 64-wide chunks (cin % 64 == 0); ws: p.slices * p.slab_elems floats.  The MFMA form is mcamd_q8_choice's (MCAMD_Q8_MFMA).
int mcamd_q8_splitk_launch(const IgemmArgs& a, const SplitkPlan& p, const void* wexp, int y_f8, int y2_f8, float* ws, hipStream_t st) {
    if (p.bk != 64 || p.bm != QSK_BNP || p.bn != QSK_BMW || a.cin_tap % 64 != 0 || a.ktot % 64 != 0 || p.slices < 1 ||
        p.slices > p.chunks) {
        mcamd_set_error("conv_fwd_q8_splitk: K per tap %d / slices %d do not fit %d chunks of %d", a.cin_tap, p.slices, p.chunks, p.bk);
        return MCAMD_EINVAL;
    }
    Q8SplitkArgs k;
    k.a = a;
    k.wexp = (const int*)wexp;
    k.ws = ws;
    k.slab_elems = p.slab_elems;
    k.slices = p.slices;
    k.npad = p.ntiles * QSK_BMW;
    k.mtiles = p.mtiles, k.ntiles = p.ntiles;
    k.y_f8 = y_f8, k.y2_f8 = y2_f8;
    const int groups = p.ntiles * p.slices;
    const dim3 grid((unsigned)(round_up_int(groups, 8) * p.mtiles));
    const int lds = 3 * (QSK_BMW + QSK_BNP) * 64;
    if (mcamd_q8_choice(a.M, a.N, MCAMD_Q8_FORM_INFER).f8mfma) hipLaunchKernelGGL(q8_splitk_partial_kernel<true>, grid, dim3(256), lds, st, k);
    else hipLaunchKernelGGL(q8_splitk_partial_kernel<false>, grid, dim3(256), lds, st, k);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_splitk (partial)");
    const dim3 fgrid((unsigned)(((a.M + QSK_FR - 1) / QSK_FR) * p.ntiles));
    hipLaunchKernelGGL(q8_splitk_finish_kernel, fgrid, dim3(256), 0, st, k);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_splitk (finish)");
    return MCAMD_OK;
}
