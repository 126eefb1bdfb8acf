// Split-K forward for low-batch fp8 inference (Darknet.precision = "fp8-splitk"): the byte K loop of
// conv_q8_loop.h with the K axis cut into S slices, by the launch design of conv_splitk.hip -- for the layers whose M = B*H*W
// pixels give conv_q8_kernel a handful of 128 x 128 tiles that each walk the whole K axis alone (YOLOv2's 13x13 layers at
// B = 1: 16 working workgroups on 256 CUs, 144-180 dependent K chunks).
//
//   launch 1, q8_splitk_partial_kernel<F8MFMA>: workgroup (tile, slice s) runs the shared loop over the K chunks
//       [floor(s n / S), floor((s+1) n / S)) of the tile's n = ktot / 64 chunks, in either MFMA form (MCAMD_Q8_MFMA), and
//       stores its fp32 accumulators, unrounded, to slab s of the workspace [S][Mpad][Npad] (pixels x channels, whole tiles).
//   launch 2, q8_splitk_finish_kernel: a 16-pixel x 64-channel tile per workgroup sums the S slabs of each element in slice
//       order 0 .. S-1 in fp32, applies the fp8 epilogue expression of write_ch_tile (conv_epi.h), lays the tile down in
//       LDS once per needed format (e4m3(2 v) bytes / saturated fp16) and calls store_pad_tile.
//
// The reduction is the launch boundary, for the reasons DESIGN.md 3p gives: no workgroup waits for, polls or counts another,
// there are no arrival counters and no fences, and the result is a function of the operands, the MFMA form and S only.  With
// S = 1 the pair computes what conv_q8_kernel computes, code for code: an element's accumulator sees the same instruction
// sequence whatever the tile (the same step function per chunk, in chunk order), and the finish kernel's epilogue
// expression is write_ch_tile's, contracted the same way (this file is compiled with conv_q8.hip's flags, build.py).
#include "conv_q8_loop.h"

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

using QskTile = Q8Tile<64, 64, 32, 32, 3>;   // partial tile: 64 filters x 64 pixels, 4 waves of 32 x 32
constexpr int QSK_BMW = QskTile::BMW, QSK_BNP = QskTile::BNP;
constexpr int QSK_FR = 16, QSK_FC = 64;      // finish tile: 16 pixels x 64 channels

template <bool F8MFMA>
__global__ __launch_bounds__(QskTile::NT) void q8_splitk_partial_kernel(Q8SplitkArgs p) {
    using T = QskTile;
    static_assert(T::TM == 1 && T::TN == 1, "one accumulator block per wave (the slab store below)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const IgemmArgs& a = p.a;
    const Q8Wave w = q8_wave<T>();
    // the pixel tiles of one (filter tile, slice) on one XCD: they stage the same weight chunks
    int mt, grp;
    if (!xcd_tile(p.mtiles, p.ntiles * p.slices, mt, grp)) return;
    const int s = grp / p.ntiles, nt = grp - s * p.ntiles;
    const int nchunks = a.ktot / T::BK;
    const int q0 = (int)((long long)s * nchunks / p.slices), q1 = (int)((long long)(s + 1) * nchunks / p.slices);
    Q8RowsA<T> aop;
    aop.setup(a, nt, w.tid);
    f32x16_t acc[1][1];
    q8_zero(acc);
    const Q8Lane<T> ln(w);
    q8_ring<T>(a, aop, Q8SeqSlice{q1 - q0, q0}, mt, smem, w, [&](const char* sa, const char* sb) {
        q8_dense_step<T, F8MFMA, false>(acc, sb, ln, [&](int i) { return q8_row_frag(sa, ln.a[i]); });
    });
    q8_mma_drain<F8MFMA>();

    // a lane's accumulator rows 4 g .. 4 g + 3 are four consecutive channels of one pixel: one 16-byte store per g; the four
    // stores of a wave fill whole 128-byte lines (32 channels of a pixel).  The slab is padded to whole tiles, so pixels past
    // the last one and channels past the last filter are stored too (never read back as results: the finish kernel's stores
    // mask them).
    float* slab = p.ws + (long long)s * p.slab_elems;
    const int lrow = w.lane & 31, hh = w.lane >> 5;
    const long long prow = (long long)(mt * T::BNP + w.wn * 32 + lrow) * p.npad + nt * T::BMW + w.wm * 32 + 4 * hh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[0][0][4 * g + e];
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
    const int lds = Q8RowsA<QskTile>::RING;
    if (mcamd_q8_choice(a.M, a.N, MCAMD_Q8_FORM_INFER).f8mfma) hipLaunchKernelGGL(q8_splitk_partial_kernel<true>, grid, dim3(256), lds, st, k);
    else hipLaunchKernelGGL(q8_splitk_partial_kernel<false>, grid, dim3(256), lds, st, k);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_splitk (partial)");
    const dim3 fgrid((unsigned)(((a.M + QSK_FR - 1) / QSK_FR) * p.ntiles));
    hipLaunchKernelGGL(q8_splitk_finish_kernel, fgrid, dim3(256), 0, st, k);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_splitk (finish)");
    return MCAMD_OK;
}
