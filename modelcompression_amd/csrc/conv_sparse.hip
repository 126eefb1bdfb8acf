// 2:4-sparse implicit-GEMM convolution forward for gfx950 (MI355X), inference epilogue (an addition beyond the reference:
// it runs the 2:4 weight masks of nm_prune at the sparse MFMA rate).
//
//   D[n][m] = sum_{tap, c} Wsp[n][kpos(tap, c)] * X[pixel(m) + tap][c]
//
// v_smfmac_f32_32x32x32_f16 takes its SPARSE operand as A (the M rows of the 32x32 product), so here the weights are A
// (n = output channel) and the activations are the dense B operand (m = pixel, the columns) -- the transpose of
// conv_igemm.hip.  Operand layout (tools/smfmac_probe.hip, exact on integer data): lane (r, h), r = lane & 31, h = lane >> 5,
//   A: row r, dense k [16 h, 16 h + 16) as 8 kept fp16 values; kept value j lies in group j / 2 (4 consecutive k) at
//      offset bits [2 j, 2 j + 2) of the lane's 16-bit index (abid 0: the low half of the index VGPR);
//   B: column r, element e = k 16 (e >> 3) + 8 h + (e & 7): two 16-byte pieces of the pixel's K row.
// A packed weight row (mcamd_pack_sparse24) is therefore simply the dense packed row (K order [channel block][tap][kb],
// include/mcamd.h) with every group of 4 k reduced to its 2 kept values: ktot / 2 fp16, and its indices one 16-bit word
// per 16 k, stored K32-chunk-major [ktot / 32][Npad][2] so that the indices of a workgroup's rows for one K chunk are one
// contiguous run (one LDS-DMA instruction).
//
// Staging per K chunk of BK (= the channel block, 64 or 32) k: BMW weight rows of BK / 2 fp16, their indices, BNP pixel
// rows of BK fp16 -- all by global_load_lds_dwordx4 (DMA source address swizzled as in conv_igemm.hip).  Against the
// dense kernel the weight bytes and the MFMA count halve; the activation bytes do not change.
//
// Epilogue: MCAMD_EPI_PAD_F16 (leaky(acc * scale + shift), the inference form of mcamd_conv_fwd mode 2), the tile laid
// down in LDS as [pixel][channel] (conv_epi.h: write_ch_tile) and stored PLAIN / POOL / REORG by the store every forward
// implicit-GEMM kernel uses (store_pad_tile).
#include "kernels.h"
#include "conv_epi.h"

typedef _Float16 h16_t __attribute__((ext_vector_type(16)));

template <int BMW, int BNP, int WM, int WN, int BK, int NSTAGE>
__global__ __launch_bounds__((BMW / WM) * (BNP / WN) * 64)
void sparse24_kernel(IgemmArgs a, const unsigned short* __restrict__ idx, int npad) {
    constexpr int WAVES_N = BNP / WN;
    constexpr int NT = (BMW / WM) * (BNP / WN) * 64;
    constexpr int CPRA = BK / 16;                  // 16-byte chunks per compressed weight row
    constexpr int CPRB = BK / 8;                   // per pixel row
    constexpr int A_SLOTS = BMW * CPRA, B_SLOTS = BNP * CPRB;
    constexpr int A_IT = (A_SLOTS + NT - 1) / NT, B_IT = (B_SLOTS + NT - 1) / NT;
    constexpr int KSUB = BK / 32;                  // smfmac k-steps per chunk
    constexpr int I_BYTES = KSUB * BMW * 4 > 1024 ? KSUB * BMW * 4 : 1024;   // index region: whole wave-wide DMAs
    constexpr int I_WAVES = I_BYTES / 1024;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int STAGE_BYTES = (A_SLOTS + B_SLOTS) * 16 + I_BYTES;
    constexpr int DMIN = A_SLOTS / NT + B_SLOTS / NT;
    static_assert(A_SLOTS % 64 == 0 && B_SLOTS % 64 == 0, "whole waves per DMA instruction");
    static_assert(I_BYTES % 1024 == 0 && I_WAVES <= NT / 64, "index region");
    static_assert(NSTAGE >= 2 && NSTAGE <= 3, "LDS ring depth");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    const int nchunks = a.ktot / BK;
    const int krow = a.ktot / 2;                   // compressed row length (fp16)

    long long wbase[A_IT];
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPRA, phys = slot % CPRA;
        const int logical = CPRA == 4 ? (phys ^ swz<4>(row)) : phys;
        wbase[it] = (long long)(nt * BMW + row) * krow + logical * 8;
    }
    long long xbase[B_IT];
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPRB, phys = slot % CPRB;
        const int logical = phys ^ swz<CPRB>(row);
        xbase[it] = tile_x_base(a, a.dst_mode != 0, mt * BNP + row) + logical * 8;
    }
    // index DMA (waves 0 .. I_WAVES-1): slot l fetches 16 bytes = 4 rows of K32 step s = l / (BMW / 4) of the chunk
    const int islot = wave * 64 + lane;
    const int is = islot / (BMW / 4) < KSUB ? islot / (BMW / 4) : KSUB - 1;
    const long long ibase = ((long long)is * npad + nt * BMW + 4 * (islot % (BMW / 4))) * 2;

    f32x16_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto stage = [&](int q, int buf) {
        const int per_block = a.ntaps;             // one chunk per tap of a channel block (BK == kb)
        const int cb = q / per_block, tap = q - cb * per_block;
        const int koff = a.tap_off[tap] + cb * BK;
        char* sa = smem + buf * STAGE_BYTES;
        char* si = sa + A_SLOTS * 16;
        char* sb = si + I_BYTES;
#pragma unroll
        for (int it = 0; it < A_IT; ++it) {
            const int wslot = it * NT + wave * 64;
            if (wslot < A_SLOTS) glds16(a.w + wbase[it] + (long long)q * (BK / 2), sa + wslot * 16);
        }
        if (wave < I_WAVES) glds16(idx + ibase + (long long)q * KSUB * npad * 2, si + wave * 1024);
#pragma unroll
        for (int it = 0; it < B_IT; ++it) {
            const int wslot = it * NT + wave * 64;
            if (wslot < B_SLOTS) glds16(a.x + xbase[it] + koff, sb + wslot * 16);
        }
    };

#pragma unroll
    for (int p = 0; p < NSTAGE - 1; ++p)
        if (p < nchunks) stage(p, p);
    int sidx = 0;
    for (int q = 0; q < nchunks; ++q) {
        int issued = q + NSTAGE - 1;
        if (issued > nchunks) issued = nchunks;
        const int inflight = issued - q - 1;
        if (NSTAGE == 2 || inflight == 0) wait_vmcnt<0>();
        else wait_vmcnt<DMIN>();
        __builtin_amdgcn_s_barrier();              // chunk q landed for every wave; every wave is done with chunk q-1
        if (q + NSTAGE - 1 < nchunks) {
            int ns = sidx + NSTAGE - 1;
            if (ns >= NSTAGE) ns -= NSTAGE;
            stage(q + NSTAGE - 1, ns);
        }
        const char* sa = smem + sidx * STAGE_BYTES;
        const char* si = sa + A_SLOTS * 16;
        const char* sb = si + I_BYTES;
        sidx = sidx + 1 == NSTAGE ? 0 : sidx + 1;
#pragma unroll
        for (int s = 0; s < KSUB; ++s) {
            h8_t af[TM];
            int ix[TM];
            h16_t bf[TN];
            const int hh = lane >> 5;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm * WM + i * 32 + (lane & 31);
                const int c = 2 * s + hh;
                const int phys = CPRA == 4 ? (c ^ swz<4>(row)) : c;
                af[i] = *(const h8_t*)(sa + (row * CPRA + phys) * 16);
                ix[i] = *(const unsigned short*)(si + s * BMW * 4 + row * 4 + hh * 2);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wn * WN + j * 32 + (lane & 31);
                const h8_t lo = *(const h8_t*)(sb + (row * CPRB + ((4 * s + hh) ^ swz<CPRB>(row))) * 16);
                const h8_t hi = *(const h8_t*)(sb + (row * CPRB + ((4 * s + 2 + hh) ^ swz<CPRB>(row))) * 16);
                bf[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_smfmac_f32_32x32x32_f16(af[i], bf[j], acc[i][j], ix[i], 0, 0);
        }
    }

    // ------------------------------- epilogue -------------------------------
    __syncthreads();                               // every wave is done with the stage buffers
    half_t* ct = (half_t*)smem;                    // [BNP][BMW] fp16 output tile: pixel rows, channel columns
    const float* scale = a.scale;
    const bool sat = write_ch_tile<BMW, BMW, WM, WN>(a, acc, [scale](int n) { return scale ? scale[n] : 1.f; }, false, true, nullptr,
                                                     ct, nt, wm, wn, lane);
    __syncthreads();
    store_pad_tile<BNP, BMW, BMW, NT>(a, nullptr, ct, false, false, mt, nt, tid);
    if (sat && a.overflow) atomicOr(a.overflow, 1);
}

template <int BMW, int BNP, int WM, int WN, int BK, int NSTAGE>
static int sparse24_launch_t(IgemmArgs& a, const Sparse24Choice& c, const unsigned short* idx, int npad, hipStream_t st) {
    constexpr int NT = (BMW / WM) * (BNP / WN) * 64;
    constexpr int I_BYTES = (BK / 32) * BMW * 4 > 1024 ? (BK / 32) * BMW * 4 : 1024;
    constexpr int STAGE_BYTES = (BMW * (BK / 16) + BNP * (BK / 8)) * 16 + I_BYTES;
    constexpr int LDS = NSTAGE * STAGE_BYTES > BNP * BMW * 2 ? NSTAGE * STAGE_BYTES : BNP * BMW * 2;   // ring / epilogue tile
    auto kern = sparse24_kernel<BMW, BNP, WM, WN, BK, NSTAGE>;
    MCAMD_LDS_OPT_IN(kern, LDS);
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(NT), LDS, st, a, idx, npad);
    MCAMD_LAUNCH_CHECK("conv_fwd_sparse24");
    return MCAMD_OK;
}

// Tile: 256 channels x 128 pixels (8 waves of 64 x 64) for layers with >= 256 filters and 64-channel blocks -- the weight
// half of a staged chunk is cheap with 2:4, so the taller tile halves the activation bytes per MFMA --, 128 x 128 (4 waves)
// for >= 128 filters, 64 x 128 below.  MCAMD_SPARSE_WIDE=0: no 256-channel tile (A/B switch).  K chunks of
// the channel block kb, two ring stages.  The grid is whole rounds of 8 pixel tiles (xcd_tile).
Sparse24Choice mcamd_sparse24_choice(long long M, int N, int kb) {
    Sparse24Choice c;
    c.bk = kb == 64 ? 64 : 32;
    c.bnp = 128;
    c.stages = 2;
    if (c.bk == 64 && N >= 256 && MCAMD_ENV_INT("MCAMD_SPARSE_WIDE", 1)) c.bmw = 256;
    else c.bmw = N >= 128 ? 128 : 64;
    c.mtiles = (int)((M + c.bnp - 1) / c.bnp);
    c.ntiles = (N + c.bmw - 1) / c.bmw;
    c.grid = (c.mtiles + 7) / 8 * 8 * c.ntiles;
    return c;
}

int mcamd_sparse24_launch(IgemmArgs& a, const void* idx, hipStream_t st) {
    const unsigned short* ix = (const unsigned short*)idx;
    const int npad = round_up_int(a.N, 256);
    const Sparse24Choice c = mcamd_sparse24_choice(a.M, a.N, a.kb);
    if (c.bnp == 128 && c.stages == 2) {
        if (c.bmw == 256 && c.bk == 64) return sparse24_launch_t<256, 128, 64, 64, 64, 2>(a, c, ix, npad, st);
        if (c.bmw == 128 && c.bk == 64) return sparse24_launch_t<128, 128, 64, 64, 64, 2>(a, c, ix, npad, st);
        if (c.bmw == 64 && c.bk == 64) return sparse24_launch_t<64, 128, 32, 64, 64, 2>(a, c, ix, npad, st);
        if (c.bmw == 128 && c.bk == 32) return sparse24_launch_t<128, 128, 64, 64, 32, 2>(a, c, ix, npad, st);
        if (c.bmw == 64 && c.bk == 32) return sparse24_launch_t<64, 128, 32, 64, 32, 2>(a, c, ix, npad, st);
    }
    mcamd_set_error("conv_fwd_sparse24: no kernel instance %d x %d, K %d, %d stages", c.bmw, c.bnp, c.bk, c.stages);
    return MCAMD_EINVAL;
}

// ---------------------------------------------------------------------------------------
// packer: fp32 OIHW master * mask -> kept fp16 values [Npad][ktot / 2] + indices [ktot / 32][Npad][2]
// ---------------------------------------------------------------------------------------
// One thread per (row n < Npad, 16-k unit u): the 16 dense k's of the packed K order, 4 groups of 4 consecutive input
// channels at one tap.  The kept entries of a group are its non-zeros of w * mask in channel order (at most 2 when the
// mask conforms, mcamd_nm_violations); a group with fewer gets distinct indices with zero values, ascending.
__global__ void pack_sparse24_kernel(const float* __restrict__ w, const float* __restrict__ mask, half_t* __restrict__ vals,
                                     unsigned short* __restrict__ idx, int cout, int cin, int ntaps, int cin_tap, int kb,
                                     int npad, int units) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)npad * units) return;
    const int n = (int)(t / units), u = (int)(t - (long long)n * units);
    h8_t kept;
    unsigned field = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int kp = 16 * u + 4 * g;                       // first k of the group in the packed order
        const int cb = kp / (ntaps * kb), r = kp - cb * ntaps * kb;
        const int tap = r / kb, c0 = cb * kb + (r - tap * kb);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = c0 + e;
            v[e] = 0.f;
            if (n < cout && c < cin) {
                const long long o = ((long long)n * cin + c) * ntaps + tap;
                v[e] = w[o] * (mask ? mask[o] : 1.f);
            }
        }
        int p[2], np = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v[e] != 0.f && np < 2) p[np++] = e;
        if (np == 0) { p[0] = 0; p[1] = 1; }
        else if (np == 1) { if (p[0] == 0) p[1] = 1; else { p[1] = p[0]; p[0] = 0; } }
        kept[2 * g] = (half_t)v[p[0]];
        kept[2 * g + 1] = (half_t)v[p[1]];
        field |= (unsigned)p[0] << (4 * g) | (unsigned)p[1] << (4 * g + 2);
    }
    *(h8_t*)(vals + (long long)n * (units * 8) + 8 * u) = kept;
    idx[((long long)(u >> 1) * npad + n) * 2 + (u & 1)] = (unsigned short)field;
}

int mcamd_pack_sparse24_launch(const float* w, const float* mask, void* vals, void* idx, int cout, int cin, int ntaps,
                               int cin_tap, int kb, hipStream_t st) {
    const int npad = round_up_int(cout, 256);
    const int units = ntaps * cin_tap / 16;
    const long long total = (long long)npad * units;
    hipLaunchKernelGGL(pack_sparse24_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, mask, (half_t*)vals,
                       (unsigned short*)idx, cout, cin, ntaps, cin_tap, kb, npad, units);
    MCAMD_LAUNCH_CHECK("pack_sparse24");
    return MCAMD_OK;
}
