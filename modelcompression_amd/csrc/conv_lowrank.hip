// Low-rank (factored) convolution forward for fp16 inference (Darknet.lowrank): a k x k convolution Cin -> r
// followed by a 1 x 1 convolution r -> Cout, both GEMMs in ONE launch with the r-channel intermediate kept in LDS.
//
//   H[m][j] = sat_half( fp32 sum over (tap, c) of X[pixel(m) + tap][c] * U[j][kpos(tap, c)] )        j < r
//   Y[m][n] = epilogue( fp32 sum over j < r of H[m][j] * V[n][j] )
//
// which is what mcamd_conv_fwd (MCAMD_EPI_RAW_F16, r filters) followed by mcamd_conv_fwd (MCAMD_EPI_PAD_F16, 1 x 1) computes,
// without the round trip of H through global memory and without the second launch.
//
// Work split: one workgroup of 256 threads (4 waves) owns LR_BM = 64 pixels -- in pooled order for the POOL / REORG
// destinations -- and ALL R = round_up(r, 64) intermediate columns of them (U is packed for round_up(r, 256) filters: rows
// r .. R-1 are zeros).  No workgroup waits for another and nothing is atomic but the overflow flag.
//
// Phase 1 is igemm_kernel's implicit GEMM on a 64 x R tile: activation rows and U chunks of 32 K values arrive by LDS-DMA
// into a 3-stage swizzled ring with counted vmcnt waits, the waves sit R % 128 ? 2 x 2 : 1 x 4 over (pixels, columns) and
// multiply with v_mfma_f32_32x32x16_f16 (R = 256: 64 accumulator registers per lane).
//
// Hand-over: the accumulators are rounded with sat_half and laid down as the r / 32 K chunks of an operand tile,
// [chunk q][64 pixels][4 pieces of 16 bytes] with the ring's XOR swizzle of the pieces, so phase 2 reads its fragments of H
// with the same conflict-free ds_read_b128 the ring's tiles are read with.
//
// Phase 2 walks the (N tile of LR_BN = 128 filters, K chunk of H) pairs as ONE sequence through the same ring (now 128 rows
// of V per stage), so the DMA stays ahead across the N tiles' epilogues.  V is the A operand there -- accumulator rows are
// filters, columns pixels, waves 2 x 2 of 64 filters x 32 pixels in the registers phase 1 has released -- which makes the
// epilogue the one of the weights-as-A kernels: write_ch_tile (leaky(acc * scale + shift), saturating fp16, 8-byte LDS
// writes) and store_pad_tile (PLAIN / POOL (+ y2) / REORG), once per N tile.
#include "kernels.h"
#include "conv_epi.h"

constexpr int LR_BM = 64, LR_BN = 128, LR_BK = 32, LR_NS = 3;
constexpr int LR_PITCH = LR_BN + 8;   // halfs between the pixel rows of the output tile: 8-byte writes of 16 pixels on 16 bank pairs

__host__ __device__ constexpr int lr_h_bytes(int R) { return LR_BM * R * 2; }
__host__ __device__ constexpr int lr_ring1_bytes(int R) { return LR_NS * (LR_BM + R) * (LR_BK / 8) * 16; }
__host__ __device__ constexpr int lr_ring2_bytes() { return LR_NS * LR_BN * (LR_BK / 8) * 16; }
__host__ __device__ constexpr int lr_ct_bytes() { return LR_BM * LR_PITCH * 2; }
// H tile + the larger of phase 1's ring and phase 2's ring with the output tile behind it
__host__ __device__ constexpr int lr_lds_bytes(int R) {
    return lr_h_bytes(R) + (lr_ring1_bytes(R) > lr_ring2_bytes() + lr_ct_bytes() ? lr_ring1_bytes(R) : lr_ring2_bytes() + lr_ct_bytes());
}

struct LowrankArgs {
    IgemmArgs a;       // x, w = U, geometry of the k x k part (N = cout: the epilogue's channel count), epilogue
    const half_t* v;   // [round_up(cout, 256)][r]
    int r;             // rank: multiple of 32
    int mtiles, ntiles;
};

template <int R>
__global__ __launch_bounds__(256) void lowrank_kernel(LowrankArgs p) {
    constexpr int BM = LR_BM, BK = LR_BK, NT = 256, CPR = BK / 8, NS = LR_NS;
    constexpr int WAVES_N = R % 128 == 0 ? 4 : 2, WAVES_M = 4 / WAVES_N;
    constexpr int WM = BM / WAVES_M, WN = R / WAVES_N, TM = WM / 32, TN = WN / 32;
    constexpr int A_SLOTS = BM * CPR, B_SLOTS = R * CPR, B_IT = B_SLOTS / NT;
    constexpr int STAGE1 = (A_SLOTS + B_SLOTS) * 16;
    constexpr int D1 = 1 + B_IT;                      // DMA instructions every wave issues per K chunk of phase 1
    constexpr int V_IT = LR_BN * CPR / NT, STAGE2 = LR_BN * CPR * 16, D2 = V_IT;
    static_assert(A_SLOTS == NT && B_SLOTS % NT == 0 && (LR_BN * CPR) % NT == 0, "every wave issues the same DMA pieces");
    static_assert(R % 64 == 0 && R >= 64 && R <= 256 && WN % 32 == 0 && WM % 32 == 0, "wave tiles of 32 x 32 blocks");
    static_assert(NS == 3 && D1 < 64, "vmcnt immediate range");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* hs = smem;                                  // H tile
    char* ring = smem + lr_h_bytes(R);
    half_t* ct = (half_t*)(ring + lr_ring2_bytes());  // [BM][LR_PITCH] output tile of phase 2

    const IgemmArgs& a = p.a;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: no waterfall around the LDS-DMA
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    // consecutive pixel tiles go round the XCDs and walk U in step: every XCD's L2 serves its tiles one copy of each chunk
    int nt_unused, mt;
    if (!xcd_tile(1, p.mtiles, nt_unused, mt)) return;
    const bool pooled = a.dst_mode != 0;
    bool sat = false;

    // ------------------------------- phase 1: H = X * U^T -------------------------------
    const int nchunks = a.ktot / BK;
    long long abase, bbase[B_IT];
    {
        const int row = tid / CPR, phys = tid % CPR;
        abase = tile_x_base(a, pooled, mt * BM + row) + (phys ^ swz<CPR>(row)) * 8;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPR, phys = slot % CPR;
        bbase[it] = (long long)row * a.ktot + (phys ^ swz<CPR>(row)) * 8;
    }

    {
        f32x16_t acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

        auto stage = [&](int q, int buf) {
            // packed K order [channel block of a.kb][tap][a.kb channels]: chunk q -> (block, tap, sub-chunk)
            const int sub = a.kb / BK, per_block = a.ntaps * sub;
            const int cb = q / per_block, rr = q - cb * per_block;
            const int tap = rr / sub;
            const int koff = a.tap_off[tap] + cb * a.kb + (rr - tap * sub) * BK;
            char* sa = ring + buf * STAGE1;
            char* sb = sa + A_SLOTS * 16;
            glds16(a.x + abase + koff, sa + wave * 64 * 16);
#pragma unroll
            for (int it = 0; it < B_IT; ++it) glds16(a.w + bbase[it] + (long long)q * BK, sb + (it * NT + wave * 64) * 16);
        };

#pragma unroll
        for (int i = 0; i < NS - 1; ++i)
            if (i < nchunks) stage(i, i);
        int sidx = 0;
        for (int q = 0; q < nchunks; ++q) {
            if (q + 1 < nchunks) wait_vmcnt<D1>();   // chunk q + 1 may still be in flight
            else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();            // chunk q landed for every wave; every wave is done reading chunk q - 1
            if (q + NS - 1 < nchunks) {
                int ns = sidx + NS - 1;
                if (ns >= NS) ns -= NS;
                stage(q + NS - 1, ns);
            }
            const char* sa = ring + sidx * STAGE1;
            const char* sb = sa + A_SLOTS * 16;
            sidx = sidx + 1 == NS ? 0 : sidx + 1;
#pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
                const int chunk = 2 * s + (lane >> 5);
                h8_t af[TM], bf[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int row = wm * WM + i * 32 + (lane & 31);
                    af[i] = *(const h8_t*)(sa + (row * CPR + (chunk ^ swz<CPR>(row))) * 16);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int row = wn * WN + j * 32 + (lane & 31);
                    bf[j] = *(const h8_t*)(sb + (row * CPR + (chunk ^ swz<CPR>(row))) * 16);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }

        // ------------------------------- hand-over -------------------------------
        // H as phase 2's K chunks: half (row, col) at chunk col / 32, piece ((col % 32) / 8) ^ swz(row) of that chunk's row
        half_t* hh = (half_t*)hs;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = wn * WN + j * 32 + (lane & 31);
            const int q = col >> 5, piece = (col & 31) >> 3, e = col & 7;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int row = wm * WM + i * 32 + mfma32_row(g, lane);
                    const float v = acc[i][j][g];
                    sat |= fabsf(v) > 65504.f;
                    hh[((q * BM + row) * CPR + (piece ^ swz<CPR>(row))) * 8 + e] = sat_half(v);
                }
        }
    }

    // ------------------------------- phase 2: Y = H * V^T -------------------------------
    const int kc2 = p.r / BK, total2 = p.ntiles * kc2;
    const int wm2 = wave >> 1, wn2 = wave & 1;       // 64 filters x 32 pixels per wave
    long long vbase[V_IT];
#pragma unroll
    for (int it = 0; it < V_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPR, phys = slot % CPR;
        vbase[it] = (long long)row * p.r + (phys ^ swz<CPR>(row)) * 8;
    }
    auto stage2 = [&](int i, int buf) {
        const int nt = i / kc2, q = i - nt * kc2;
        char* sb = ring + buf * STAGE2;
#pragma unroll
        for (int it = 0; it < V_IT; ++it)
            glds16(p.v + vbase[it] + (long long)nt * LR_BN * p.r + q * BK, sb + (it * NT + wave * 64) * 16);
    };

    __syncthreads();   // H is down and every wave is done with phase 1's ring
#pragma unroll
    for (int i = 0; i < NS - 1; ++i)
        if (i < total2) stage2(i, i);

    f32x16_t acc2[2][1];
    const float* scale = a.scale;
    int sidx = 0, q = 0, nt = 0;
    for (int i = 0; i < total2; ++i) {
        if (i + 1 < total2) wait_vmcnt<D2>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();   // item i landed for every wave; every wave is done with item i - 1 (and the tile before)
        if (i + NS - 1 < total2) {
            int ns = sidx + NS - 1;
            if (ns >= NS) ns -= NS;
            stage2(i + NS - 1, ns);
        }
        const char* sb = ring + sidx * STAGE2;
        sidx = sidx + 1 == NS ? 0 : sidx + 1;
        if (q == 0) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc2[t][0][e] = 0.f;
        }
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            const int chunk = 2 * s + (lane >> 5);
            const int hrow = wn2 * 32 + (lane & 31);
            const h8_t hf = *(const h8_t*)(hs + ((q * BM + hrow) * CPR + (chunk ^ swz<CPR>(hrow))) * 16);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int vrow = wm2 * 64 + t * 32 + (lane & 31);
                const h8_t vf = *(const h8_t*)(sb + (vrow * CPR + (chunk ^ swz<CPR>(vrow))) * 16);
                acc2[t][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, hf, acc2[t][0], 0, 0, 0);
            }
        }
        if (++q == kc2) {
            // the output tile lies behind the ring: the DMAs in flight do not touch it, and the barrier at the head of the next
            // item separates this tile's reads from the next tile's writes
            sat |= write_ch_tile<LR_BN, LR_PITCH, 64, 32>(a, acc2, [scale](int n) { return scale ? scale[n] : 1.f; }, false, true,
                                                          nullptr, ct, nt, wm2, wn2, lane);
            __syncthreads();
            store_pad_tile<LR_BM, LR_BN, LR_PITCH, NT>(a, nullptr, ct, false, false, mt, nt, tid);
            q = 0;
            ++nt;
        }
    }
    if (sat && a.overflow) atomicOr(a.overflow, 1);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
LowrankChoice mcamd_lowrank_choice(long long M, int n, int rank) {
    LowrankChoice c;
    c.rp = round_up_int(rank, 64);
    c.bm = LR_BM, c.bn = LR_BN, c.bk = LR_BK, c.stages = LR_NS;
    c.mtiles = (int)((M + LR_BM - 1) / LR_BM);
    c.ntiles = (n + LR_BN - 1) / LR_BN;
    c.grid = round_up_int(c.mtiles, 8);
    c.lds_bytes = c.rp == 64 ? lr_lds_bytes(64) : c.rp == 128 ? lr_lds_bytes(128) : c.rp == 192 ? lr_lds_bytes(192) : lr_lds_bytes(256);
    return c;
}

template <int R>
static int lowrank_launch_t(const LowrankArgs& k, const LowrankChoice& c, hipStream_t st) {
    constexpr int LDS = lr_lds_bytes(R);
    if (LDS > 64 * 1024) MCAMD_LDS_OPT_IN((lowrank_kernel<R>), LDS);
    hipLaunchKernelGGL((lowrank_kernel<R>), dim3(c.grid), dim3(256), LDS, st, k);
    MCAMD_LAUNCH_CHECK("conv_fwd_lowrank");
    return MCAMD_OK;
}

// a.* geometry and epilogue fields filled by the caller (mode MCAMD_EPI_PAD_F16; a.w = the packed U, a.N = cout)
int mcamd_lowrank_launch(const IgemmArgs& a, const void* vp, int rank, hipStream_t st) {
    if (rank < 32 || rank > 256 || rank % 32 != 0 || a.cin_tap % LR_BK != 0 || a.kb % LR_BK != 0) {
        mcamd_set_error("conv_fwd_lowrank: rank %d / K per tap %d have no kernel instance", rank, a.cin_tap);
        return MCAMD_EINVAL;
    }
    const LowrankChoice c = mcamd_lowrank_choice(a.M, a.N, rank);
    LowrankArgs k;
    k.a = a;
    k.v = (const half_t*)vp;
    k.r = rank;
    k.mtiles = c.mtiles, k.ntiles = c.ntiles;
    switch (c.rp) {
        case 64: return lowrank_launch_t<64>(k, c, st);
        case 128: return lowrank_launch_t<128>(k, c, st);
        case 192: return lowrank_launch_t<192>(k, c, st);
        default: return lowrank_launch_t<256>(k, c, st);
    }
}
