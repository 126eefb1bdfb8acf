// Block-sparse fp8 inference forward for gfx950 (MI355X) (Darknet.precision = "fp8-block"): the byte K loop of
// conv_q8.hip on its 64-filter x 128-pixel tile, taking the K chunks of each N tile from a list instead of 0 .. nchunks-1 --
// what conv_bsparse.hip does to igemm_kernel's loop, done to conv_q8_block's.
//
//   S[n][m] = sum_{q in list[n / 64]} sum_{k in chunk q} W8[n][64 q + k] * X8[pixel(m) + tap(q)][c(q, k)]
//   v       = leaky(scale[n] * 2^-(e[n] + 1) * S + shift[n])
//
// The fp8 K order runs [channel block of 64][tap][64 channels], so one 64-byte chunk of one 64-filter tile is one
// (filter block, channel block, tap) block of block_prune's masks.  A chunk whose 64 x 64 weight bytes are all zero codes
// (0x00 / 0x80) contributes products +-0 to accumulators that start at +0 and therefore never hold -0: in the default MFMA
// form leaving it out changes no bit (finite activations: e4m3 bytes from the cast pass and the epilogues are never NaN).
// The lists come from the packed bytes themselves (q8_bsparse_lists_kernel), so any mask works, a kept weight that rounds
// to a zero byte is skipped too, and no second weight format exists.
//
// Operands, LDS-DMA staging with swizzled source addresses, the 3-stage ring with counted vmcnt waits, the fragment mapping,
// the MFMA order inside a chunk in both forms (MCAMD_Q8_MFMA) and the epilogue (write_ch_tile + store_pad_tile) are
// conv_q8_block's for <64, 128, 32, 64, 3>; with full lists every accumulator sees conv_q8_kernel's instruction sequence
// whatever that kernel's tile (conv_q8_splitk.hip's argument).  This file is compiled with conv_q8.hip's flags, so the
// epilogue expression contracts the same way.
#include "kernels.h"
#include "conv_epi.h"

constexpr int QBS_BMW = 64, QBS_BNP = 128;   // tile: 64 filters (the pruning grain) x 128 pixels, 4 waves of 32 x 64

// count[ntiles], list[ntiles][nchunks]: entries [0, count[nt]) of row nt are the tile's chunk indices, ascending
template <bool F8MFMA>
__global__ __launch_bounds__(256) void conv_q8_bsparse_kernel(IgemmArgs a, const int* __restrict__ wexp, const int* __restrict__ count,
                                                              const int* __restrict__ list, int y_f8, int y2_f8) {
    constexpr int BMW = QBS_BMW, BNP = QBS_BNP, WM = 32, WN = 64, NSTAGE = 3;
    constexpr int WAVES_N = BNP / WN;
    constexpr int NT = (BMW / WM) * (BNP / WN) * 64;
    constexpr int BK = 64, CPR = 4;                // 64 e4m3 k per 64-byte LDS row: four 16-byte chunks
    constexpr int A_SLOTS = BMW * CPR, B_SLOTS = BNP * CPR;
    constexpr int A_IT = A_SLOTS / NT, B_IT = B_SLOTS / NT;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int STAGE_BYTES = (A_SLOTS + B_SLOTS) * 16;
    constexpr int DPS = A_IT + B_IT;               // DMA instructions per stage and wave
    static_assert(NT == 256 && A_SLOTS % NT == 0 && B_SLOTS % NT == 0, "whole workgroups per DMA round");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    const int nchunks = a.ktot / BK;
    // the tile's list: wave-uniform addresses (scalar loads).  A count or an index outside its range is clamped, so a list
    // this library did not build cannot send a DMA out of the operands.
    const int* lst = list + (long long)nt * nchunks;
    int cnt = count[nt];
    cnt = cnt < 0 ? 0 : (cnt > nchunks ? nchunks : cnt);
    auto chunk_at = [&](int i) {
        const int q = lst[i];
        return q < 0 ? 0 : (q >= nchunks ? nchunks - 1 : q);
    };
    const char* xg = (const char*)a.x;             // byte operands: every stride of `a` counts bytes
    const char* wg = (const char*)a.w;

    long long wbase[A_IT];
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPR, phys = slot % CPR;
        wbase[it] = (long long)(nt * BMW + row) * a.ktot + (phys ^ swz<CPR>(row)) * 16;   // rows < round_up(N, 64) <= Npad
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

    // conv_q8_block's ring over the list: entries i+1, i+2 stay in flight across the barrier.  cnt < 2 fills part of the
    // prologue; cnt == 0 runs neither loop, the accumulators stay zero and the epilogue writes leaky(shift).
#pragma unroll
    for (int p = 0; p < NSTAGE - 1; ++p)
        if (p < cnt) stage(chunk_at(p), p);
    int sidx = 0;
    for (int i = 0; i < cnt; ++i) {
        int issued = i + NSTAGE - 1;
        if (issued > cnt) issued = cnt;
        const int inflight = issued - i - 1;
        if (inflight == 0) wait_vmcnt<0>();
        else wait_vmcnt<DPS>();
        __builtin_amdgcn_s_barrier();              // entry i landed for every wave; every wave is done with entry i-1
        if (i + NSTAGE - 1 < cnt) {
            int ns = sidx + NSTAGE - 1;
            if (ns >= NSTAGE) ns -= NSTAGE;
            stage(chunk_at(i + NSTAGE - 1), ns);
        }
        const char* sa = smem + sidx * STAGE_BYTES;
        const char* sb = sa + A_SLOTS * 16;
        sidx = sidx + 1 == NSTAGE ? 0 : sidx + 1;
        i32x8_t af[TM], bf[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            const int row = wm * WM + t * 32 + lrow;
            const i32x4_t lo = *(const i32x4_t*)(sa + (row * CPR + (hh ^ swz<CPR>(row))) * 16);
            const i32x4_t hi = *(const i32x4_t*)(sa + (row * CPR + ((2 + hh) ^ swz<CPR>(row))) * 16);
            af[t] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int row = wn * WN + j * 32 + lrow;
            const i32x4_t lo = *(const i32x4_t*)(sb + (row * CPR + (hh ^ swz<CPR>(row))) * 16);
            const i32x4_t hi = *(const i32x4_t*)(sb + (row * CPR + ((2 + hh) ^ swz<CPR>(row))) * 16);
            bf[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
        // conv_q8_block's order inside a chunk (inline assembly for the fp8 MFMA as there: through the builtin hipcc does
        // not accumulate in place; the operands come from LDS reads the compiler waits for)
        if constexpr (F8MFMA) {
#pragma unroll
            for (int t = 0; t < TM; ++t)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    asm volatile("v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
                                 : "+v"(acc[t][j])
                                 : "v"(af[t]), "v"(bf[j]), "v"(SC), "v"(SC));
        } else {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                h8_t a16[TM], b16[TN];
#pragma unroll
                for (int t = 0; t < TM; ++t) a16[t] = q8_to_f16(af[t][2 * s4], af[t][2 * s4 + 1]);
#pragma unroll
                for (int j = 0; j < TN; ++j) b16[j] = q8_to_f16(bf[j][2 * s4], bf[j][2 * s4 + 1]);
#pragma unroll
                for (int t = 0; t < TM; ++t)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[t][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a16[t], b16[j], acc[t][j], 0, 0, 0);
            }
        }
    }
    // last (assembly) MFMA -> VALU reads of the accumulators; unconditional, so also in front of a cnt == 0 epilogue
    if constexpr (F8MFMA) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");

    // ------------------------------- epilogue (conv_q8_block) -------------------------------
    __syncthreads();                               // every wave is done with the stage buffers
    const bool has2 = a.y2 != nullptr;
    const bool need_b = y_f8 || (has2 && y2_f8), need_h = !y_f8 || (has2 && !y2_f8);
    constexpr int PB = BMW + 8;                    // tile row pitch (conv_q8_block)
    static_assert(BNP * PB * 3 <= NSTAGE * STAGE_BYTES, "both epilogue tiles inside the ring");
    char* bt = smem;                               // [BNP][PB] e4m3 tile
    half_t* ht = (half_t*)(smem + (need_b ? BNP * PB : 0));   // [BNP][PB] fp16 tile
    const float* scale = a.scale;
    const bool sat = write_ch_tile<BMW, PB, WM, WN>(a, acc, [scale, wexp](int n) { return ldexpf(scale ? scale[n] : 1.f, -(wexp[n] + 1)); },
                                                    need_b, need_h, bt, ht, nt, wm, wn, lane);
    __syncthreads();
    store_pad_tile<BNP, BMW, PB, NT>(a, bt, ht, y_f8 != 0, y2_f8 != 0, mt, nt, tid);
    if (sat && a.overflow) atomicOr(a.overflow, 1);
}

// ---------------------------------------------------------------------------------------
// chunk lists from the packed weight bytes [Npad][ktot] (mcamd_pack_q8)
// ---------------------------------------------------------------------------------------
// bsparse_lists_kernel on bytes.  One workgroup per N tile.  Pass 1: wave v takes the chunks q = v, v + waves, ...; its lanes
// read the 64 x 64 bytes of (tile, q) in 16-byte pieces and ONE ballot says whether any byte is a non-zero code (the sign
// bit is masked off: 0x80 = -0 is a zero); the flag goes to LDS.  Pass 2: wave 0 walks the flags 64 at a time in ascending q,
// a kept chunk's position = kept chunks before this group + kept chunks below its lane in the group's ballot.  No atomics,
// no host synchronisation: the lists are a function of the bytes alone.
constexpr int QBL_NT = 1024;
__global__ __launch_bounds__(QBL_NT) void q8_bsparse_lists_kernel(const char* __restrict__ wq, int ktot, int nchunks,
                                                                  int* __restrict__ count, int* __restrict__ list) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* flags = (int*)smem;   // [nchunks]
    const int nt = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int CPR = 4, PIECES = QBS_BMW * CPR;   // 16-byte pieces of one (tile, chunk): 256
    for (int q = wave; q < nchunks; q += QBL_NT / 64) {
        unsigned any = 0;
        for (int p = lane; p < PIECES; p += 64) {
            const int row = p / CPR, c = p - row * CPR;
            // (rows < round_up(N, 64) <= Npad exist: zero bytes behind the last filter)
            const i32x4_t v = *(const i32x4_t*)(wq + (long long)(nt * QBS_BMW + row) * ktot + (long long)q * 64 + c * 16);
            any |= ((unsigned)(v[0] | v[1] | v[2] | v[3])) & 0x7f7f7f7fu;
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
int mcamd_q8_bsparse_lists_launch(const void* wq, int cout, int cin, int ntaps, int* count, int* list, hipStream_t st) {
    const int ktot = ntaps * cin, nchunks = ktot / 64;
    const int ntiles = (cout + QBS_BMW - 1) / QBS_BMW;
    if (nchunks > 8192) {
        mcamd_set_error("q8_bsparse_lists: %d K chunks exceed the 8192 the list kernel holds flags for", nchunks);
        return MCAMD_EINVAL;
    }
    hipLaunchKernelGGL(q8_bsparse_lists_kernel, dim3(ntiles), dim3(QBL_NT), (size_t)nchunks * sizeof(int), st, (const char*)wq, ktot,
                       nchunks, count, list);
    MCAMD_LAUNCH_CHECK("q8_bsparse_lists");
    return MCAMD_OK;
}

// always the 64 x 128 tile, 3 stages; the MFMA form is mcamd_q8_choice's (MCAMD_Q8_MFMA); whole rounds of 8 pixel tiles
Q8Choice mcamd_q8_bsparse_choice(long long M, int N) {
    Q8Choice c = mcamd_q8_choice(M, N, MCAMD_Q8_FORM_INFER);
    c.bmw = QBS_BMW, c.bnp = QBS_BNP, c.stages = 3;
    c.mtiles = (int)((M + c.bnp - 1) / c.bnp);
    c.ntiles = (N + c.bmw - 1) / c.bmw;
    c.grid = (c.mtiles + 7) / 8 * 8 * c.ntiles;
    return c;
}

int mcamd_conv_q8_bsparse_launch(IgemmArgs& a, const void* wexp, const int* count, const int* list, int y_f8, int y2_f8, hipStream_t st) {
    const Q8Choice c = mcamd_q8_bsparse_choice(a.M, a.N);
    constexpr int LDS = 3 * (QBS_BMW + QBS_BNP) * 64;   // the ring (36 KB); the epilogue's tiles lie inside it
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    if (c.f8mfma) hipLaunchKernelGGL(conv_q8_bsparse_kernel<true>, dim3(c.grid), dim3(256), LDS, st, a, (const int*)wexp, count, list, y_f8, y2_f8);
    else hipLaunchKernelGGL(conv_q8_bsparse_kernel<false>, dim3(c.grid), dim3(256), LDS, st, a, (const int*)wexp, count, list, y_f8, y2_f8);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_bsparse");
    return MCAMD_OK;
}
