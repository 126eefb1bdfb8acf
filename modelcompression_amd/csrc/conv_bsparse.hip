// Block-sparse fp16 forward (inference; forward and dgrad in training) for gfx950 (MI355X): the implicit GEMM of conv_igemm.hip
// on 64-filter N tiles that takes its K chunks from a list instead of 0 .. nchunks-1 (an addition beyond the reference;
// Darknet.sparse = "block"; Darknet.sparse_train = "block").
//
//   D[m][n] = sum_{q in list[n / 64]} sum_{k in chunk q} X[pixel(m) + tap(q)][c(q, k)] * Wp[n][q kb + k]
//
// The packed K axis runs [channel block][tap][kb channels] (include/mcamd.h), so chunk q of kb = 64 (32 when the padded
// channel count is no multiple of 64) columns is one (channel block, tap) pair: the grain of block_prune's masks.  A chunk
// whose 64 x kb weights of the N tile are all zero adds x * (+-0) = +-0 to accumulators that start at +0 and therefore never
// hold -0: leaving it out changes no bit of the result (finite activations: the fp16 forwards saturate, never inf).  The
// lists come from the packed weights themselves (bsparse_lists_kernel), so any mask works -- an unstructured one just gives
// full lists -- and no second weight format exists.
//
// Operands, LDS-DMA staging with swizzled source addresses, the NSTAGE ring with counted vmcnt waits and the
// v_mfma_f32_32x32x16_f16 walk in K order are igemm_kernel's; the epilogue is its MCAMD_EPI_PAD_F16 branch with the shared
// stores of conv_epi.h.  With full lists every accumulator sees igemm_kernel's MFMA sequence.
//
// The training form (Darknet.sparse_train = "block") is the same K loop with igemm_kernel's MCAMD_EPI_RAW_F16
// branch: the tile to y[M][y_ld] through store_raw_tile and, with a.stats, the BatchNorm partial sums of the stored values to
// one slab row per pixel tile through store_stats_slab.  It serves the forward GEMM and the dgrad GEMM alike -- the dgrad
// packing [Cpad][kpos(t, n)] has the same K order over cout_p, so its chunk q is one (cout block, flipped tap) pair and
// bsparse_lists_kernel reads its lists from it unchanged.
#include "kernels.h"
#include "conv_epi.h"

constexpr int BS_BN = 64;   // N tile = the pruning grain (filters per block of block_prune)

// count[ntiles], list[ntiles][nchunks]: entries [0, count[nt]) of row nt are the tile's chunk indices, ascending.
// EPI: MCAMD_EPI_PAD_F16 (inference) or MCAMD_EPI_RAW_F16 (the training form, forward and dgrad: DESIGN.md 3zc)
template <int BM, int BK, int NSTAGE, int EPI>
__global__ __launch_bounds__(256) void bsparse_kernel(IgemmArgs a, const int* __restrict__ count, const int* __restrict__ list) {
    constexpr int BN = BS_BN, NT = 256, WAVES_N = 2;
    constexpr int WM = BM / 2, WN = BN / WAVES_N;      // 2 x 2 waves of (BM / 2) x 32
    constexpr int TM = WM / 32;
    constexpr int CPR = BK / 8;
    constexpr int A_SLOTS = BM * CPR, B_SLOTS = BN * CPR;
    constexpr int A_IT = A_SLOTS / NT, B_IT = B_SLOTS / NT;
    constexpr int STAGE_BYTES = (A_SLOTS + B_SLOTS) * 16;
    constexpr int DMIN = A_IT + B_IT;   // DMA instructions every wave issues per K chunk
    static_assert(WN == 32 && A_SLOTS % NT == 0 && B_SLOTS % NT == 0, "every wave issues the same DMA pieces");
    static_assert(NSTAGE >= 2 && NSTAGE <= 4 && DMIN * (NSTAGE - 2) < 64, "vmcnt immediate range");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: no waterfall around the LDS-DMA
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    const int nchunks = a.ktot / BK;
    // the tile's list: wave-uniform addresses (scalar loads).  A count or an index outside its range is clamped, so a
    // list this library did not build cannot send a DMA out of the operands.
    const int* lst = list + (long long)nt * nchunks;
    int cnt = count[nt];
    cnt = cnt < 0 ? 0 : (cnt > nchunks ? nchunks : cnt);
    auto chunk_at = [&](int i) {
        const int q = lst[i];
        return q < 0 ? 0 : (q >= nchunks ? nchunks - 1 : q);
    };

    long long abase[A_IT], bbase[B_IT];
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPR, phys = slot % CPR;
        // (pooled order when the epilogue pools: four consecutive rows = one 2x2 window)
        abase[it] = tile_x_base(a, EPI == MCAMD_EPI_PAD_F16 && a.dst_mode != 0, mt * BM + row) + (phys ^ swz<CPR>(row)) * 8;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPR, phys = slot % CPR;
        bbase[it] = (long long)(nt * BN + row) * a.ktot + (phys ^ swz<CPR>(row)) * 8;
    }

    f32x16_t acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    auto stage = [&](int q, int buf) {
        // packed K order [channel block of BK][tap][BK channels] (BK == a.kb): chunk q -> (block, tap)
        const int cb = q / a.ntaps, tap = q - cb * a.ntaps;
        const int koff = a.tap_off[tap] + cb * BK;
        char* sa = smem + buf * STAGE_BYTES;
        char* sb = sa + A_SLOTS * 16;
#pragma unroll
        for (int it = 0; it < A_IT; ++it) glds16(a.x + abase[it] + koff, sa + (it * NT + wave * 64) * 16);
#pragma unroll
        for (int it = 0; it < B_IT; ++it) glds16(a.w + bbase[it] + (long long)q * BK, sb + (it * NT + wave * 64) * 16);
    };

    // NSTAGE-deep LDS ring with counted waits, as igemm_kernel: list entries i+1 .. i+NSTAGE-2 stay in flight across the
    // barrier.  cnt < NSTAGE - 1 fills part of the prologue; cnt == 0 runs neither loop and the accumulators stay zero.
#pragma unroll
    for (int i = 0; i < NSTAGE - 1; ++i)
        if (i < cnt) stage(chunk_at(i), i);
    int sidx = 0;
    for (int i = 0; i < cnt; ++i) {
        int issued = i + NSTAGE - 1;
        if (issued > cnt) issued = cnt;
        const int inflight = issued - i - 1;
        if (NSTAGE == 2 || inflight == 0) wait_vmcnt<0>();
        else if (inflight == 1) wait_vmcnt<DMIN>();
        else wait_vmcnt<(NSTAGE > 3 ? 2 * DMIN : DMIN)>();
        __builtin_amdgcn_s_barrier();   // entry i landed for every wave; every wave is done reading entry i-1
        if (i + NSTAGE - 1 < cnt) {
            int ns = sidx + NSTAGE - 1;
            if (ns >= NSTAGE) ns -= NSTAGE;
            stage(chunk_at(i + NSTAGE - 1), ns);
        }
        const char* sa = smem + sidx * STAGE_BYTES;
        const char* sb = sa + A_SLOTS * 16;
        sidx = sidx + 1 == NSTAGE ? 0 : sidx + 1;
        constexpr int KS = BK / 16;
        h8_t af[KS][TM], bf[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int chunk = 2 * k + (lane >> 5);
            const int rb = wn * WN + (lane & 31);
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                const int ra = wm * WM + t * 32 + (lane & 31);
                af[k][t] = *(const h8_t*)(sa + (ra * CPR + (chunk ^ swz<CPR>(ra))) * 16);
            }
            bf[k] = *(const h8_t*)(sb + (rb * CPR + (chunk ^ swz<CPR>(rb))) * 16);
        }
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int t = 0; t < TM; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[k][t], bf[k], acc[t], 0, 0, 0);
    }

    // ------------------------------- epilogue (igemm_kernel's MCAMD_EPI_PAD_F16 / MCAMD_EPI_RAW_F16 branches) -------------------------------
    __syncthreads();   // every wave is done with the stage buffers
    half_t* ct = (half_t*)smem;   // [BM][BN] fp16 output tile
    bool sat = false;
    if constexpr (EPI == MCAMD_EPI_PAD_F16) {
        const int col = wn * WN + (lane & 31);
        const int n = nt * BN + col;
        float sc = 1.f, sh = 0.f;
        if (n < a.N) {
            if (a.scale) sc = a.scale[n];
            if (a.shift) sh = a.shift[n];
        }
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * WM + t * 32 + mfma32_row(r, lane);
                float v = acc[t][r] * sc + sh;
                v = v > 0.f ? v : v * a.slope;
                ct[row * BN + col] = (half_t)fminf(fmaxf(v, -65504.f), 65504.f);   // saturate, never inf
                sat |= fabsf(v) > 65504.f;
            }
        __syncthreads();
        store_pad_tile<BM, BN, BN, NT>(a, nullptr, ct, false, false, mt, nt, tid);
        if (sat && a.overflow) atomicOr(a.overflow, 1);
    } else {
        // the raw tile to y[M][y_ld], and (a.stats) the BatchNorm partial sums of the values AS STORED -- fp16, saturated, rows
        // past the last pixel as zeros: igemm_kernel's convention -- to the slab row of this pixel tile (the grid is not
        // persistent: one row per M tile).  An empty list leaves the accumulators zero: zeros stored, zero sums.
        static_assert(EPI == MCAMD_EPI_RAW_F16, "bsparse_kernel: epilogue modes 0 and 2");
        float s1[1] = {0.f}, s2[1] = {0.f};
        const int col = wn * WN + (lane & 31);
        const int mlim = a.M - mt * BM;   // rows of this tile that are real pixels
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * WM + t * 32 + mfma32_row(r, lane);
                const float v = acc[t][r];
                const half_t hv = (half_t)fminf(fmaxf(v, -65504.f), 65504.f);   // saturate, never inf
                sat |= fabsf(v) > 65504.f;
                ct[row * BN + col] = hv;
                if (a.stats) {
                    const float fv = row < mlim ? (float)hv : 0.f;
                    s1[0] += fv;
                    s2[0] += fv * fv;
                }
            }
        __syncthreads();
        store_raw_tile<BM, BN, NT>(a, ct, mt, nt, tid);
        if (sat && a.overflow) atomicOr(a.overflow, 1);
        if (a.stats) store_stats_slab<BM, BN, WM, WN, NT>(a, smem, s1, s2, mt, nt, wm, wn, lane, tid);   // (uniform; its barrier ends the tile's use)
    }
}

// ---------------------------------------------------------------------------------------
// chunk lists from the packed forward weights [Npad][ktot]
// ---------------------------------------------------------------------------------------
// One workgroup per N tile.  Pass 1: wave v takes the chunks q = v, v + waves, ...; its lanes read the 64 x kb halfs of
// (tile, q) in 16-byte pieces and ONE ballot says whether any of them is non-zero (by value: the sign bit is masked off,
// w * 0 = -0 for a negative w is a zero); the flag goes to LDS.  Pass 2: wave 0 walks the flags 64 at a time in ascending q,
// a kept chunk's position = kept chunks before this group + kept chunks below its lane in the group's ballot.  No atomics,
// no host synchronisation: the lists are a function of the weights alone.
constexpr int BSL_NT = 1024;
__global__ __launch_bounds__(BSL_NT) void bsparse_lists_kernel(const half_t* __restrict__ w, int ktot, int kb, int nchunks,
                                                               int* __restrict__ count, int* __restrict__ list) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* flags = (int*)smem;   // [nchunks]
    const int nt = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cpr = kb / 8, pieces = BS_BN * cpr;   // 16-byte pieces of one (tile, chunk): 256 or 512
    for (int q = wave; q < nchunks; q += BSL_NT / 64) {
        unsigned any = 0;
        for (int p = lane; p < pieces; p += 64) {
            const int row = p / cpr, c = p - row * cpr;
            const i32x4_t v = *(const i32x4_t*)(w + (long long)(nt * BS_BN + row) * ktot + (long long)q * kb + c * 8);
            any |= ((unsigned)(v[0] | v[1] | v[2] | v[3])) & 0x7fff7fffu;
        }
        const unsigned long long b = __ballot(any != 0);
        if (lane == 0) flags[q] = b != 0 ? 1 : 0;
    }
    __syncthreads();
    if (wave != 0) return;
    int kept = 0;
    int* row = list + (long long)nt * nchunks;
    for (int base = 0; base < nchunks; base += 64) {
        const int q = base + lane;
        const bool f = q < nchunks && flags[q] != 0;
        const unsigned long long b = __ballot(f);
        if (f) row[kept + __popcll(b & ((1ull << lane) - 1ull))] = q;
        kept += __popcll(b);
    }
    // entries behind the kept ones: a valid index, so a reader that ignored the count would still stay inside the operands
    for (int i = kept + lane; i < nchunks; i += 64) row[i] = 0;
    if (lane == 0) count[nt] = kept;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
int mcamd_bsparse_lists_launch(const void* wp, int cout, int cin_tap, int ntaps, int* count, int* list, hipStream_t st) {
    const int kb = cin_tap % 64 == 0 ? 64 : 32, ktot = ntaps * cin_tap, nchunks = ktot / kb;
    const int ntiles = (cout + BS_BN - 1) / BS_BN;
    if (nchunks > 8192) {
        mcamd_set_error("bsparse_lists: %d K chunks exceed the 8192 the list kernel holds flags for", nchunks);
        return MCAMD_EINVAL;
    }
    hipLaunchKernelGGL(bsparse_lists_kernel, dim3(ntiles), dim3(BSL_NT), (size_t)nchunks * sizeof(int), st, (const half_t*)wp, ktot,
                       kb, nchunks, count, list);
    MCAMD_LAUNCH_CHECK("bsparse_lists");
    return MCAMD_OK;
}

template <int BM, int BK, int NSTAGE, int EPI>
static int bsparse_launch_e(IgemmArgs& a, const BsparseChoice& c, const int* count, const int* list, hipStream_t st) {
    constexpr int STAGE_BYTES = (BM + BS_BN) * (BK / 8) * 16;
    // ring / epilogue tile (the statistics reduction of the raw form, 2 x 2 x 64 floats, fits either)
    constexpr int LDS = NSTAGE * STAGE_BYTES > BM * BS_BN * 2 ? NSTAGE * STAGE_BYTES : BM * BS_BN * 2;
    auto kern = bsparse_kernel<BM, BK, NSTAGE, EPI>;
    if (LDS > 64 * 1024) MCAMD_LDS_OPT_IN(kern, LDS);
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    hipLaunchKernelGGL(kern, dim3(c.grid), dim3(256), LDS, st, a, count, list);
    // (the raw form serves mcamd_conv_fwd_bsparse_raw and mcamd_conv_dgrad_bsparse)
    MCAMD_LAUNCH_CHECK(EPI == MCAMD_EPI_RAW_F16 ? "conv_fwd_bsparse_raw / conv_dgrad_bsparse" : "conv_fwd_bsparse");
    return MCAMD_OK;
}

template <int BM, int BK, int NSTAGE>
static int bsparse_launch_t(IgemmArgs& a, const BsparseChoice& c, const int* count, const int* list, hipStream_t st) {
    if (a.mode == MCAMD_EPI_RAW_F16) return bsparse_launch_e<BM, BK, NSTAGE, MCAMD_EPI_RAW_F16>(a, c, count, list, st);
    return bsparse_launch_e<BM, BK, NSTAGE, MCAMD_EPI_PAD_F16>(a, c, count, list, st);
}

// The instance, in one place.  M tile: MCAMD_BSPARSE_BM_DEFAULT rows (MCAMD_BSPARSE_BM = 64 selects 64, anything else 128:
// A/B switch of tools/bsparse_bench.py); K chunk = the channel block kb, 3 ring stages of 64 or 4 of 32
BsparseChoice mcamd_bsparse_choice(long long M, int N, int kb) {
    BsparseChoice c;
    c.bm = MCAMD_ENV_INT("MCAMD_BSPARSE_BM", MCAMD_BSPARSE_BM_DEFAULT) == 64 ? 64 : 128;
    c.bn = BS_BN;
    c.bk = kb == 64 ? 64 : 32;
    c.stages = c.bk == 64 ? 3 : 4;
    c.mtiles = (int)((M + c.bm - 1) / c.bm);
    c.ntiles = (N + BS_BN - 1) / BS_BN;
    c.grid = (c.mtiles + 7) / 8 * 8 * c.ntiles;
    return c;
}

int mcamd_bsparse_launch(IgemmArgs& a, const int* count, const int* list, hipStream_t st) {
    const BsparseChoice c = mcamd_bsparse_choice(a.M, a.N, a.kb);
    if (c.bk == 64) return c.bm == 64 ? bsparse_launch_t<64, 64, 3>(a, c, count, list, st) : bsparse_launch_t<128, 64, 3>(a, c, count, list, st);
    return c.bm == 64 ? bsparse_launch_t<64, 32, 4>(a, c, count, list, st) : bsparse_launch_t<128, 32, 4>(a, c, count, list, st);
}
