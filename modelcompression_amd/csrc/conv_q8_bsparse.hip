// Block-sparse fp8 inference forward for gfx950 (MI355X) (Darknet.precision = "fp8-block"): the byte K loop of
// conv_q8_loop.h on a 64-filter x 128-pixel tile, taking the K chunks of each N tile from a list instead of 0 .. nchunks-1 --
// what conv_bsparse.hip does to igemm_kernel's loop.
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
// With full lists every accumulator sees conv_q8_kernel's instruction sequence whatever that kernel's tile: both run
// conv_q8_loop.h's step per chunk, in chunk order, and its epilogue.
#include "conv_q8_loop.h"

using QbsTile = Q8Tile<64, 128, 32, 64, 3>;   // 64 filters (the pruning grain) x 128 pixels, 4 waves of 32 x 64
constexpr int QBS_BMW = QbsTile::BMW;
static_assert(3 * QbsTile::TILE_BYTES <= Q8RowsA<QbsTile>::RING, "both epilogue tiles inside the ring");

// count[ntiles], list[ntiles][nchunks]: entries [0, count[nt]) of row nt are the tile's chunk indices, ascending.  count == 0:
// the accumulators stay zero and the epilogue writes leaky(shift).
template <bool F8MFMA>
__global__ __launch_bounds__(QbsTile::NT) void conv_q8_bsparse_kernel(IgemmArgs a, const int* __restrict__ wexp,
                                                                      const int* __restrict__ count, const int* __restrict__ list,
                                                                      int y_f8, int y2_f8) {
    using T = QbsTile;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Q8Wave w = q8_wave<T>();
    int nt, mt;
    if (!xcd_tile(a.num_ntiles, a.num_mtiles, nt, mt)) return;
    const int nchunks = a.ktot / T::BK;
    Q8RowsA<T> aop;
    aop.setup(a, nt, w.tid);
    f32x16_t acc[T::TM][T::TN];
    q8_zero(acc);
    const Q8Lane<T> ln(w);
    q8_ring<T>(a, aop, Q8SeqList(list + (long long)nt * nchunks, count[nt], nchunks), mt, smem, w, [&](const char* sa, const char* sb) {
        q8_dense_step<T, F8MFMA, false>(acc, sb, ln, [&](int i) { return q8_row_frag(sa, ln.a[i]); });
    });
    q8_mma_drain<F8MFMA>();
    __syncthreads();                               // every wave is done with the stage buffers
    q8_infer_epilogue<T>(a, acc, wexp, y_f8, y2_f8, smem, mt, nt, w);
}

// ---------------------------------------------------------------------------------------
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
    c.bmw = QbsTile::BMW, c.bnp = QbsTile::BNP, c.stages = QbsTile::NSTAGE;
    q8_choice_grid(c, M, N);
    return c;
}

int mcamd_conv_q8_bsparse_launch(IgemmArgs& a, const void* wexp, const int* count, const int* list, int y_f8, int y2_f8, hipStream_t st) {
    const Q8Choice c = mcamd_q8_bsparse_choice(a.M, a.N);
    const int lds = q8_infer_lds(Q8RowsA<QbsTile>::RING, QbsTile::TILE_BYTES, a, y_f8, y2_f8);   // the ring (36 KB): the tiles lie inside it
    a.num_mtiles = c.mtiles;
    a.num_ntiles = c.ntiles;
    if (c.f8mfma) hipLaunchKernelGGL(conv_q8_bsparse_kernel<true>, dim3(c.grid), dim3(QbsTile::NT), lds, st, a, (const int*)wexp, count, list, y_f8, y2_f8);
    else hipLaunchKernelGGL(conv_q8_bsparse_kernel<false>, dim3(c.grid), dim3(QbsTile::NT), lds, st, a, (const int*)wexp, count, list, y_f8, y2_f8);
    MCAMD_LAUNCH_CHECK("conv_fwd_q8_bsparse");
    return MCAMD_OK;
}
