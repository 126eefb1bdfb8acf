// 4-bit weights fed to the block-scaled MFMA AS fp4 (an addition beyond the reference: Darknet.precision = "fp8-w4-mx";
// DESIGN.md 3zg): conv_q8_loop.h's ring, pixel staging, half-row weight staging and inference epilogue around a matrix step
// of its own -- v_mfma_scale_f32_32x32x64_f8f6f4 with an e2m1 A operand (cbsz:4, four registers) against the e4m3 pixels,
// the group shift as the lane's e8m0 scale.  conv_q8_w4.hip's register decode (a v_perm_b32 table, sign moves, two
// additions per group and lane in front of every chunk's MFMAs) is gone: nothing but LDS reads stands in front of the MFMA.
//
//   S[n][m] = sum_{groups} 2^g * sum_{k in group} grid[code[n][k]] * X8[pixel(m) + tap][c]     (the instruction's arithmetic)
//   v       = leaky(scale[n] * 2^-(e4[n] + 1) * S + shift[n])                                  (q8_infer_epilogue, e4_f)
//
// The quantisation is mcamd_pack_q8_w4's (w4_quant.h: e4_f, group shifts g in [-5, 6], codes and rounding); the grid {0, 0.5,
// 1, 1.5, 2, 3, 4, 6} with the sign in bit 3 IS OCP e2m1, a group of 32 input channels at one tap IS one lane's half of a
// 64-k chunk, and 2^g IS the e8m0 byte 127 + g.  Only the layout differs (mcamd.h states it; tools/f4_probe.hip measured it):
//
//   codes   [Npad][ktot / 2]: chunk q of row n = 32 bytes, piece h = 16 bytes = group h = positions [32 h, 32 h + 32) of
//           mcamd_pack_q8's k order; byte i of piece h: low nibble position 32 h + 2 i, high nibble 32 h + 2 i + 1
//   scales  [ktot / 64][Npad][2]: byte 127 + g per group (pad rows 127) -- gshift's shape: one wave-wide DMA per chunk
//
// Per 64-k chunk and 32 x 32 block, lane (r, h), r = lane & 31, h = lane >> 5:
//   A      one ds_read_b128 of piece h of weight row r, straight into the instruction's four A registers
//   scale  one ds_read_u8 of byte h of row r's staged pair: byte 0 of the scale register, which op_sel 0 selects (bytes 1-3
//          are zero and unused) -- no VALU instruction and no per-lane op_sel
//   B      q8_row_frag's 16-byte pieces h and 2 + h of pixel row r, as conv_q8_kernel reads them.  That is NOT a free
//          permutation of k: measured (tools/f4_probe.hip, and the one-hot test with the other read), the instruction's k
//          of an 8-bit operand is 16 h + e for the lane's elements e < 16 (registers 0-3) and 32 + 16 h + (e - 16) above
//          (registers 4-7), while a 4-bit operand's lane holds the 32 CONSECUTIVE k [32 h, 32 h + 32) in its four
//          registers.  So A's group h -- one lane, one scale -- meets B's bytes [32 h, 32 h + 32) spread over both half-waves,
//          and reading B as bytes [32 h, 32 h + 32) per lane swaps k [16, 32) with [32, 48).  Banks: piece c of row p sits
//          in 16-byte slot 4 (p & 3) + (c ^ ((p >> 2) & 3)) of the 16 slots that span the 64 banks; the 16 lanes of a
//          ds_read_b128 group share h, hence c, and their 16 rows give 4 x 4 distinct ((p & 3), (p >> 2) & 3) pairs: 16
//          distinct slots -- conflict-free with the ring's swizzle as it is.
// No VALU instruction stands between the fragment reads and the MFMA.  The compiler does re-materialise B's constant scale
// register with a v_mov_b32 right in front of the first MFMA in the loop's tail copy (seen in the ISA of all three
// instances), and hipcc pads no hazard in front of inline assembly: every string opens with conv_q8_loop.h's `s_nop 1` (issued
// while the matrix pipe is busy with the MFMA before it); q8_mma_drain() pads the other end.  The instruction's fp8-side
// truncation is conv_q8_loop.h's F8MFMA one (~6e-4 of the bytes one code off): "fp8-w4-mx" is not byte-exact.
#include "conv_q8_loop.h"
#include "w4_quant.h"

template <class T>
using Q8W4MxRowsA = Q8HalfRowsA<T, 2>;           // 32 code bytes + the two e8m0 group scales per row and chunk

// a lane's fragment addresses, taken once in front of the K loop (offsets into a stage's A region / B region)
template <class T>
struct W4MxLane {
    int a[T::TM], sc[T::TM];
    Q8RowOff b[T::TN];
    __device__ __forceinline__ explicit W4MxLane(const Q8Wave& w) {
        const int hh = w.lane >> 5;
#pragma unroll
        for (int i = 0; i < T::TM; ++i) {
            const int row = w.wm * T::WM + i * 32 + (w.lane & 31);
            a[i] = (row * 2 + hh) * 16;
            sc[i] = Q8W4MxRowsA<T>::SLOTS * 16 + row * 2 + hh;
        }
#pragma unroll
        for (int j = 0; j < T::TN; ++j) b[j] = q8_row_off(w.wn * T::WN + j * 32 + (w.lane & 31), hh);
    }
};

// acc += A(e2m1, 4 registers, scale byte 0 of sa) x B(e4m3, 8 registers, scale 1.0); accumulates in place (inline assembly,
// as Q8_F8_MFMA: through the builtin hipcc does not)
#define Q8_W4MX_MFMA "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4"
template <class T>
__device__ __forceinline__ void w4mx_step(f32x16_t (&acc)[T::TM][T::TN], const char* sa, const char* sb, const W4MxLane<T>& ln) {
    const int SC = 127 * 0x01010101;             // e8m0 1.0 in all four scale bytes of B
    i32x4_t af[T::TM];
    int as[T::TM];
    i32x8_t bf[T::TN];
#pragma unroll
    for (int i = 0; i < T::TM; ++i) {
        af[i] = *(const i32x4_t*)(sa + ln.a[i]);
        as[i] = *(const unsigned char*)(sa + ln.sc[i]);
    }
#pragma unroll
    for (int j = 0; j < T::TN; ++j) bf[j] = q8_row_frag(sb, ln.b[j]);
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j)
            asm volatile("s_nop 1\n\t" Q8_W4MX_MFMA : "+v"(acc[i][j]) : "v"(af[i]), "v"(bf[j]), "v"(as[i]), "v"(SC));
}

template <class T>
__global__ __launch_bounds__(T::NT) void conv_q8_w4_mx_kernel(IgemmArgs a, const char* __restrict__ scales, int npad,
                                                              const int* __restrict__ wexp, int y_f8, int y2_f8) {
    using A = Q8W4MxRowsA<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Q8Wave w = q8_wave<T>();
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    A aop;
    aop.setup(a, scales, npad, nt, w.tid);
    f32x16_t acc[T::TM][T::TN];
    q8_zero(acc);
    const W4MxLane<T> ln(w);
    q8_ring<T>(a, aop, Q8SeqDense{a.ktot / T::BK}, mt, smem, w, [&](const char* sa, const char* sb) { w4mx_step<T>(acc, sa, sb, ln); });
    q8_mma_drain<true>();
    __syncthreads();                               // every wave is done with the stage buffers
    q8_infer_epilogue<T>(a, acc, wexp, y_f8, y2_f8, smem, mt, nt, w);
}

template <class T>
static int conv_q8_w4_mx_launch_t(IgemmArgs& a, const Q8Choice& c, const char* scales, int npad, const int* wexp, int y_f8, int y2_f8,
                                  hipStream_t st) {
    constexpr int RING = Q8W4MxRowsA<T>::RING;
    auto kern = conv_q8_w4_mx_kernel<T>;
    MCAMD_LDS_OPT_IN(kern, q8_infer_lds_max(RING, T::TILE_BYTES));
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(T::NT), q8_infer_lds(RING, T::TILE_BYTES, a, y_f8, y2_f8), st, a, scales, npad, wexp, y_f8,
                       y2_f8);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_w4_mx");
    return MCAMD_OK;
}

// The three fp8-MFMA tiles of mcamd_q8_choice (256 filters x 128 pixels from 256 filters, 128 x 128 from 128, 64 x 128 below;
// 3 stages), whatever MCAMD_Q8_MFMA says: this kernel has one matrix instruction and no fp16-MFMA form.  Every instance
// compiles without scratch memory (profiles/q8_w4_mx_resources.txt).
Q8Choice mcamd_q8_w4_mx_choice(long long M, int N) {
    Q8Choice c;
    c.f8mfma = 1;
    c.bnp = 128;
    c.stages = 3;
    c.bmw = N >= 256 ? 256 : N >= 128 ? 128 : 64;
    q8_choice_grid(c, M, N);
    return c;
}

int mcamd_conv_q8_w4_mx_launch(IgemmArgs& a, const void* scales, const void* wexp, int y_f8, int y2_f8, hipStream_t st) {
    const int npad = round_up_int(a.N, 256);
    const Q8Choice c = mcamd_q8_w4_mx_choice(a.M, a.N);
    const char* sc = (const char*)scales;
    const int* we = (const int*)wexp;
    if (c.bmw == 256) return conv_q8_w4_mx_launch_t<Q8Tile<256, 128, 64, 64, 3>>(a, c, sc, npad, we, y_f8, y2_f8, st);
    if (c.bmw == 128) return conv_q8_w4_mx_launch_t<Q8Tile<128, 128, 64, 64, 3>>(a, c, sc, npad, we, y_f8, y2_f8, st);
    return conv_q8_w4_mx_launch_t<Q8Tile<64, 128, 32, 64, 3>>(a, c, sc, npad, we, y_f8, y2_f8, st);
}

// The same kernel with MXFP4 destinations (mcamd_conv_fwd_q8_w4_mx_a4): the producer in front of an fp4 x fp4
// block where the engine's e4m3 activations end (Darknet.fp4_skip).  conv_q8_w4_mx_kernel's K loop, then the epilogue whose
// store quantises the byte tile on its way out (conv_epi.h store_pad_tile_a4); fy / fy2: MCAMD_FMT_* per destination.
template <class T>
__global__ __launch_bounds__(T::NT) void conv_q8_w4_mx_a4_kernel(IgemmArgs a, const char* __restrict__ scales, int npad,
                                                                 const int* __restrict__ wexp, int fy, int fy2, A4Dst d, A4Dst d2) {
    using A = Q8W4MxRowsA<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Q8Wave w = q8_wave<T>();
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    A aop;
    aop.setup(a, scales, npad, nt, w.tid);
    f32x16_t acc[T::TM][T::TN];
    q8_zero(acc);
    const W4MxLane<T> ln(w);
    q8_ring<T>(a, aop, Q8SeqDense{a.ktot / T::BK}, mt, smem, w, [&](const char* sa, const char* sb) { w4mx_step<T>(acc, sa, sb, ln); });
    q8_mma_drain<true>();
    __syncthreads();                               // every wave is done with the stage buffers
    q8_infer_epilogue_a4<T>(a, acc, wexp, fy, fy2, d, d2, smem, mt, nt, w);
}

template <class T>
static int conv_q8_w4_mx_a4_launch_t(IgemmArgs& a, const Q8Choice& c, const char* scales, int npad, const int* wexp, int fy, int fy2,
                                     const A4Dst& d, const A4Dst& d2, hipStream_t st) {
    constexpr int RING = Q8W4MxRowsA<T>::RING;
    auto kern = conv_q8_w4_mx_a4_kernel<T>;
    MCAMD_LDS_OPT_IN(kern, q8_infer_lds_max(RING, T::TILE_BYTES));
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    // (an MXFP4 destination is quantised from the byte tile: sized as an e4m3 one; the kernel sees an MXFP4 copy in d2 alone)
    const int lds = q8_infer_lds(RING, T::TILE_BYTES, a, fy != MCAMD_FMT_F16, fy2 != MCAMD_FMT_F16);
    if (fy2 == MCAMD_FMT_A4) a.y2 = nullptr;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(T::NT), lds, st, a, scales, npad, wexp, fy, fy2, d, d2);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_w4_mx_a4");
    return MCAMD_OK;
}

int mcamd_conv_q8_w4_mx_a4_launch(IgemmArgs& a, const void* scales, const void* wexp, int fy, int fy2, const A4Dst& d, const A4Dst& d2,
                                  hipStream_t st) {
    const int npad = round_up_int(a.N, 256);
    const Q8Choice c = mcamd_q8_w4_mx_choice(a.M, a.N);
    const char* sc = (const char*)scales;
    const int* we = (const int*)wexp;
    if (c.bmw == 256) return conv_q8_w4_mx_a4_launch_t<Q8Tile<256, 128, 64, 64, 3>>(a, c, sc, npad, we, fy, fy2, d, d2, st);
    if (c.bmw == 128) return conv_q8_w4_mx_a4_launch_t<Q8Tile<128, 128, 64, 64, 3>>(a, c, sc, npad, we, fy, fy2, d, d2, st);
    return conv_q8_w4_mx_a4_launch_t<Q8Tile<64, 128, 32, 64, 3>>(a, c, sc, npad, we, fy, fy2, d, d2, st);
}

// ---------------------------------------------------------------------------------------
// split-K partial kernel for low-batch inference (Darknet.precision = "fp8-w4-mx-splitk")
// ---------------------------------------------------------------------------------------
// conv_q8_splitk.hip's launch design on this file's operands and matrix step.  Workgroup (pixel tile, filter tile, slice s) of
// a 64-filter x 64-pixel tile -- four waves, one 32 x 32 accumulator block each -- runs the chunks [floor(s n / S),
// floor((s + 1) n / S)) of the n = ktot / 64 chunks through the ring and stores its fp32 accumulators, unrounded, to slab s of
// the workspace [S][Mpad][Npad]; q8_splitk_finish_kernel (conv_q8_splitk.hip, unchanged) sums the slabs in slice order and
// applies the epilogue.  No workgroup waits for another: the launch boundary is the reduction.
//   staging  per chunk and workgroup: 64 rows x 32 code bytes (waves 0 and 1: one DMA instruction each), the tile's 128 scale
//            bytes of plane q of [ktot / 64][Npad][2] (wave 0: one more; the 64 lanes repeat the 8 pieces) and 64 pixel rows
//            x 64 bytes (every wave: one) -- 7 KB a stage, 21 KB for the three.  Half the weight bytes of the byte kernel
//            in the regime where every workgroup of a (filter tile, slice) waits for the same weight chunks: xcd_tile puts
//            the pixel tiles of one (filter tile, slice) on one XCD, so they stage those chunks out of one L2.
//   step     w4mx_step<T> with TM = TN = 1: one ds_read_b128 (A), one ds_read_u8 (scale), two ds_read_b128 (B), one MFMA.
//   store    a lane's accumulator rows 4 g .. 4 g + 3 are four consecutive channels of one pixel: one 16-byte store per g,
//            whole 128-byte lines per wave; the slab is padded to whole tiles, so nothing is masked (the finish kernel's
//            stores are).
struct W4MxSplitkArgs {
    IgemmArgs a;            // byte operands, a.w = the codes
    const char* scales;     // [ktot / 64][wnpad][2]
    float* ws;              // [slices][slab_elems]
    long long slab_elems;   // mtiles * 64 * npad
    int slices;
    int wnpad;              // rows of a scale plane: round_up(N, 256)
    int npad;               // ntiles * 64: floats per slab row
    int mtiles, ntiles;
};

using W4SkTile = Q8Tile<64, 64, 32, 32, 3>;

__global__ __launch_bounds__(W4SkTile::NT) void q8_w4_mx_splitk_partial_kernel(W4MxSplitkArgs p) {
    using T = W4SkTile;
    static_assert(T::TM == 1 && T::TN == 1, "one accumulator block per wave (the slab store below)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const IgemmArgs& a = p.a;
    const Q8Wave w = q8_wave<T>();
    int mt, grp;
    if (!xcd_tile(p.mtiles, p.ntiles * p.slices, mt, grp)) return;
    const int s = grp / p.ntiles, nt = grp - s * p.ntiles;
    const int nchunks = a.ktot / T::BK;
    const int q0 = (int)((long long)s * nchunks / p.slices), q1 = (int)((long long)(s + 1) * nchunks / p.slices);
    Q8W4MxRowsA<T> aop;
    aop.setup(a, p.scales, p.wnpad, nt, w.tid);
    f32x16_t acc[1][1];
    q8_zero(acc);
    const W4MxLane<T> ln(w);
    q8_ring<T>(a, aop, Q8SeqSlice{q1 - q0, q0}, mt, smem, w, [&](const char* sa, const char* sb) { w4mx_step<T>(acc, sa, sb, ln); });
    q8_mma_drain<true>();

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

// a.* geometry and epilogue fields filled by the caller (mode MCAMD_EPI_PAD_F16, byte strides, a.w = the codes); p:
// mcamd_splitk_plan with 64-wide chunks (cin % 64 == 0); ws: p.slices * p.slab_elems floats
int mcamd_q8_w4_mx_splitk_launch(const IgemmArgs& a, const SplitkPlan& p, const void* scales, const void* wexp, int y_f8, int y2_f8,
                                 float* ws, hipStream_t st) {
    if (p.bk != 64 || p.bm != W4SkTile::BNP || p.bn != W4SkTile::BMW || a.cin_tap % 64 != 0 || a.ktot % 64 != 0 || p.slices < 1 ||
        p.slices > p.chunks) {
        mcamd_set_error("conv_fwd_q8_w4_mx_splitk: K per tap %d / slices %d do not fit %d chunks of %d", a.cin_tap, p.slices, p.chunks,
                        p.bk);
        return MCAMD_EINVAL;
    }
    W4MxSplitkArgs k;
    k.a = a;
    k.scales = (const char*)scales;
    k.ws = ws;
    k.slab_elems = p.slab_elems;
    k.slices = p.slices;
    k.wnpad = round_up_int(a.N, 256);
    k.npad = p.ntiles * W4SkTile::BMW;
    k.mtiles = p.mtiles, k.ntiles = p.ntiles;
    const dim3 grid((unsigned)(round_up_int(p.ntiles * p.slices, 8) * p.mtiles));
    hipLaunchKernelGGL(q8_w4_mx_splitk_partial_kernel, grid, dim3(W4SkTile::NT), Q8W4MxRowsA<W4SkTile>::RING, st, k);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_w4_mx_splitk (partial)");
    return mcamd_q8_splitk_finish_launch(a, p, wexp, y_f8, y2_f8, ws, st, "conv_fwd_q8_w4_mx_splitk (finish)");
}

// ---------------------------------------------------------------------------------------
// packer: fp32 OIHW master * mask -> codes [Npad][ktot / 2] + e8m0 scales [ktot / 64][Npad][2] + exponents [Npad]
// ---------------------------------------------------------------------------------------
// pack_q8_w4_kernel's steps in its order (one workgroup per row n < Npad, four chunks at a time, every weight read once; the
// exponent, shift and code rules are w4_quant.h's) with this file's layout: code byte i of a chunk holds positions 2 i (low
// nibble) and 2 i + 1 (high nibble), the scale byte is 127 + g.  Pad rows: zero codes, scale 127, exponent 0.
__global__ __launch_bounds__(256) void pack_q8_w4_mx_kernel(const float* __restrict__ w, const float* __restrict__ mask,
                                                            char* __restrict__ codes, char* __restrict__ scales,
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
            if (q < nchunks) scales[((long long)q * npad + n) * 2 + (tid & 1)] = (char)(n < cout ? 127 + g : 127);
        }
        __syncthreads();
        if (tid < 128) {                                         // code byte i of chunk q0 + tid / 32: positions 2 i, 2 i + 1
            const int c = tid / 32, i = tid % 32, q = q0 + c;
            const int g = sg[2 * c + i / 16];
            const unsigned lo = w4_code(sv[c * 64 + 2 * i], g), hi = w4_code(sv[c * 64 + 2 * i + 1], g);
            if (q < nchunks) codes[(long long)n * (ktot / 2) + (long long)q * 32 + i] = (char)(lo | hi << 4);
        }
        __syncthreads();                                         // before the next four chunks overwrite sv / sg
    }
}

int mcamd_pack_q8_w4_mx_launch(const float* w, const float* mask, void* codes, void* scales, void* wexp, int cout, int cin, int ntaps,
                               hipStream_t st) {
    const int npad = round_up_int(cout, 256);
    hipLaunchKernelGGL(pack_q8_w4_mx_kernel, dim3(npad), dim3(256), 0, st, w, mask, (char*)codes, (char*)scales, (int*)wexp, cout, cin,
                       ntaps, npad);
    MCAMD_LAUNCH_CHECK("pack_q8_w4_mx");
    return MCAMD_OK;
}

// ---------------------------------------------------------------------------------------
// expander: codes + scales -> the e4m3 bytes [Npad][ktot] in mcamd_pack_q8's layout (what the instruction multiplies)
// ---------------------------------------------------------------------------------------
// the e4m3 byte of grid[code & 7] * 2^g, sign from bit 3: exponent field and mantissa bit of the g = -5 magnitudes {0, 2^-6,
// 2^-5, 1.5 2^-5, 2^-4, 1.5 2^-4, 2^-3, 1.5 2^-3}, the exponent field raised by g + 5 on a non-zero entry (<= 0x7c: no carry)
__device__ __forceinline__ unsigned w4mx_byte(unsigned code, int g) {
    const unsigned m = code & 7u;
    const unsigned mag = (unsigned)(0x24201c1814100800ull >> (8 * m)) & 0xffu;
    return m == 0u ? 0u : ((code & 8u) << 4) | (mag + ((unsigned)(g + 5) << 3));
}

// One thread per (row, chunk, piece): 16 code bytes -> the 32 bytes [32 h, 32 h + 32) of the chunk.
__global__ __launch_bounds__(256) void unpack_q8_w4_mx_kernel(const char* __restrict__ codes, const char* __restrict__ scales,
                                                              char* __restrict__ wq, long long total, int ktot, int npad) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int upr = ktot / 32;                                   // pieces per row
    const long long n = t / upr;
    const int u = (int)(t - n * upr), q = u >> 1, h = u & 1;
    const i32x4_t c = *(const i32x4_t*)(codes + n * (ktot / 2) + 16 * u);
    const int g = (int)((const unsigned char*)scales)[((long long)q * npad + n) * 2 + h] - 127;
    i32x8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {                                // output dword j: code bytes 2 j and 2 j + 1
        const unsigned two = ((unsigned)c[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        o[j] = (int)(w4mx_byte(two & 15u, g) | w4mx_byte((two >> 4) & 15u, g) << 8 | w4mx_byte((two >> 8) & 15u, g) << 16 |
                     w4mx_byte(two >> 12, g) << 24);
    }
    *(i32x8_t*)(wq + n * ktot + (long long)q * 64 + 32 * h) = o;
}

int mcamd_unpack_q8_w4_mx_launch(const void* codes, const void* scales, void* wq, int cout, int cin, int ntaps, hipStream_t st) {
    const int npad = round_up_int(cout, 256), ktot = cin * ntaps;
    const long long total = (long long)npad * (ktot / 32);
    hipLaunchKernelGGL(unpack_q8_w4_mx_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const char*)codes,
                       (const char*)scales, (char*)wq, total, ktot, npad);
    MCAMD_LAUNCH_CHECK("unpack_q8_w4_mx");
    return MCAMD_OK;
}
