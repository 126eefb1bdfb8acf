// The byte K loop and the inference epilogue of the fp8 (e4m3) forward family, each part once: conv_q8.hip (dense, raw fp32,
// border table), conv_q8_bsparse.hip (chunk lists), conv_q8_splitk.hip (K slices), conv_q8_w4.hip (4-bit codes) and
// conv_q8_sparse.hip (2:4) are this loop with their own chunk sequence, weight fragment and last step.  Every "bit-equal to
// conv_q8_kernel" statement between those files holds because the same functions run (the files are compiled with equal
// flags, build.py, so that the epilogue expression contracts the same way in each).
//
// Operand form: K order [channel block of 64][tap][64 channels]; one K chunk = 64 k.  The pixels (B operand) are one 64-byte
// LDS row each, staged by global_load_lds_dwordx4 with the source address swizzled as in conv_igemm.hip.  Lane (r, h) of an
// MFMA, r = lane & 31, h = lane >> 5, reads bytes [16 h, 16 h + 16) and [32 + 16 h, 32 + 16 h + 16) of row r for BOTH operands:
// a k permutation common to A and B (tools/f8_probe.hip; the F8 phase of conv_igemm_pp.hip reads the same way).  The weights
// (A operand, rows = output channels) come in two staging shapes: whole 64-byte rows of bytes (Q8RowsA) or 32-byte rows plus
// a side band per row (Q8HalfRowsA: conv_q8_w4.hip's shifts, conv_q8_sparse.hip's index words).
#pragma once
#include <type_traits>

#include "kernels.h"
#include "conv_epi.h"

// ---------------------------------------------------------------------------------------
// tile constants: BMW filters x BNP pixels per workgroup, WM x WN per wave, an NSTAGE-deep LDS ring
// ---------------------------------------------------------------------------------------
template <int BMW_, int BNP_, int WM_, int WN_, int NSTAGE_>
struct Q8Tile {
    static constexpr int BMW = BMW_, BNP = BNP_, WM = WM_, WN = WN_, NSTAGE = NSTAGE_;
    static constexpr int BK = 64, CPR = 4;         // 64 e4m3 k per 64-byte LDS row: four 16-byte chunks
    static constexpr int WAVES_N = BNP / WN, NT = (BMW / WM) * WAVES_N * 64;
    static constexpr int TM = WM / 32, TN = WN / 32;
    static constexpr int B_SLOTS = BNP * CPR, B_IT = B_SLOTS / NT, B_BYTES = B_SLOTS * 16;
    // epilogue tile rows are PB = BMW + 8 elements apart: the 32 pixels of a wave's write then fall on 32 different LDS
    // banks (a pitch of BMW puts them all on one or two)
    static constexpr int PB = BMW + 8;
    static constexpr int TILE_BYTES = BNP * PB;    // the [BNP][PB] e4m3 tile; the fp16 tile is twice that
    static_assert(B_SLOTS % NT == 0, "whole workgroups per DMA round");
    static_assert(NSTAGE >= 2 && NSTAGE <= 3, "LDS ring depth");
};

struct Q8Wave {
    int tid, lane, wave, wm, wn;
};
template <class T>
__device__ __forceinline__ Q8Wave q8_wave() {
    Q8Wave w;
    w.tid = threadIdx.x;
    w.lane = w.tid & 63;
    w.wave = __builtin_amdgcn_readfirstlane(w.tid >> 6);
    w.wm = w.wave / T::WAVES_N, w.wn = w.wave % T::WAVES_N;
    return w;
}

template <int TM, int TN>
__device__ __forceinline__ void q8_zero(f32x16_t (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// the 32 bytes lane (row, hh) holds of a swizzled 64-byte LDS row: 16-byte chunks hh and 2 + hh
struct Q8RowOff {
    int lo, hi;
};
__device__ __forceinline__ Q8RowOff q8_row_off(int row, int hh) {
    return {(row * 4 + (hh ^ swz<4>(row))) * 16, (row * 4 + ((2 + hh) ^ swz<4>(row))) * 16};
}
__device__ __forceinline__ i32x8_t q8_row_frag(const char* s, const Q8RowOff& o) {
    const i32x4_t lo = *(const i32x4_t*)(s + o.lo), hi = *(const i32x4_t*)(s + o.hi);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// a lane's fragment addresses, taken once in front of the K loop: lane (r, h), r = lane & 31, h = lane >> 5, reads weight row
// arow[i] for block i -- a[i]: its pieces in swizzled 64-byte rows, ahalf[i]: its 16 bytes in 32-byte rows -- and the
// pixel-row pieces b[j] for block j
template <class T>
struct Q8Lane {
    int hh, arow[T::TM], ahalf[T::TM];
    Q8RowOff a[T::TM], b[T::TN];
    __device__ __forceinline__ explicit Q8Lane(const Q8Wave& w) {
        hh = w.lane >> 5;
#pragma unroll
        for (int i = 0; i < T::TM; ++i) {
            arow[i] = w.wm * T::WM + i * 32 + (w.lane & 31);
            a[i] = q8_row_off(arow[i], hh);
            ahalf[i] = (arow[i] * 2 + hh) * 16;
        }
#pragma unroll
        for (int j = 0; j < T::TN; ++j) b[j] = q8_row_off(w.wn * T::WN + j * 32 + (w.lane & 31), hh);
    }
};

// ---------------------------------------------------------------------------------------
// operands: source addresses per thread (setup), the DMA of one chunk into a stage (issue), the layout of the stage
// ---------------------------------------------------------------------------------------
// B: the tile's BNP pixels (byte operands: every stride of `a` counts bytes)
template <class T>
struct Q8PixelsB {
    long long base[T::B_IT];
    __device__ __forceinline__ void setup(const IgemmArgs& __restrict__ a, int mt, int tid) {
#pragma unroll
        for (int it = 0; it < T::B_IT; ++it) {
            const int slot = it * T::NT + tid;
            const int row = slot / T::CPR, phys = slot % T::CPR;
            base[it] = tile_x_base(a, a.dst_mode != 0, mt * T::BNP + row) + (phys ^ swz<T::CPR>(row)) * 16;
        }
    }
    __device__ __forceinline__ void issue(const IgemmArgs& __restrict__ a, int q, char* sb, int wave) const {
        const int cb = q / a.ntaps, tap = q - cb * a.ntaps;      // one chunk per tap of a 64-channel block
        const int koff = a.tap_off[tap] + cb * T::BK;
#pragma unroll
        for (int it = 0; it < T::B_IT; ++it) glds16((const char*)a.x + base[it] + koff, sb + (it * T::NT + wave * 64) * 16);
    }
};

// A, 64-byte swizzled rows of e4m3 bytes [rows][ktot] (mcamd_pack_q8; rows < round_up(N, BMW) <= Npad exist)
template <class T>
struct Q8RowsA {
    static constexpr int SLOTS = T::BMW * T::CPR, IT = SLOTS / T::NT;
    static constexpr int BYTES = SLOTS * 16;       // of a stage
    static constexpr int DMIN = IT;                // DMA instructions every wave issues per stage
    static constexpr int RING = T::NSTAGE * (BYTES + T::B_BYTES);
    static_assert(SLOTS % T::NT == 0, "whole workgroups per DMA round");
    long long base[IT];
    __device__ __forceinline__ void setup(const IgemmArgs& __restrict__ a, int nt, int tid) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int slot = it * T::NT + tid;
            const int row = slot / T::CPR, phys = slot % T::CPR;
            base[it] = (long long)(nt * T::BMW + row) * a.ktot + (phys ^ swz<T::CPR>(row)) * 16;
        }
    }
    __device__ __forceinline__ void issue(const IgemmArgs& __restrict__ a, int q, char* sa, int wave) const {
#pragma unroll
        for (int it = 0; it < IT; ++it)
            glds16((const char*)a.w + base[it] + (long long)q * T::BK, sa + (it * T::NT + wave * 64) * 16);
    }
};

// A, 32-byte rows [rows][ktot / 2] (read 16 bytes per lane, contiguously over the wave: no swizzle) + a side band of
// BAND_ROW bytes per row and chunk, [ktot / 64][npad][BAND_ROW], staged behind the rows by whole wave-wide DMAs (lanes past
// the tile's rows repeat).  Rows < Npad = round_up(N, 256) exist.
template <class T, int BAND_ROW>
struct Q8HalfRowsA {
    static constexpr int CPR = 2, SLOTS = T::BMW * CPR, IT = (SLOTS + T::NT - 1) / T::NT;
    static constexpr int BAND = T::BMW * BAND_ROW > 1024 ? T::BMW * BAND_ROW : 1024, BAND_WAVES = BAND / 1024;
    static constexpr int BAND_PIECES = T::BMW * BAND_ROW / 16;
    static constexpr int BYTES = SLOTS * 16 + BAND;
    static constexpr int DMIN = SLOTS / T::NT;     // (a wave past SLOTS issues nothing; the band's waves issue one more)
    static constexpr int RING = T::NSTAGE * (BYTES + T::B_BYTES);
    static_assert(SLOTS % 64 == 0, "whole waves per DMA instruction");
    static_assert(BAND_PIECES >= 1 && BAND_WAVES <= T::NT / 64, "band region");
    long long base[IT], bbase;
    const char* band_g;
    int npad;
    __device__ __forceinline__ void setup(const IgemmArgs& __restrict__ a, const void* band, int npad_, int nt, int tid) {
        const int krow = a.ktot / 2;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int slot = (it * T::NT + tid) % SLOTS;
            base[it] = (long long)(nt * T::BMW + slot / CPR) * krow + (slot % CPR) * 16;
        }
        bbase = (long long)nt * T::BMW * BAND_ROW + (tid % BAND_PIECES) * 16;
        band_g = (const char*)band;
        npad = npad_;
    }
    __device__ __forceinline__ void issue(const IgemmArgs& __restrict__ a, int q, char* sa, int wave) const {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int wslot = it * T::NT + wave * 64;
            if (wslot < SLOTS) glds16((const char*)a.w + base[it] + (long long)q * (T::BK / 2), sa + wslot * 16);
        }
        if (wave < BAND_WAVES) glds16(band_g + bbase + (long long)q * npad * BAND_ROW, sa + SLOTS * 16 + wave * 1024);
    }
    // row 0 of the staged band
    static __device__ __forceinline__ const char* band(const char* sa) { return sa + SLOTS * 16; }
};

// ---------------------------------------------------------------------------------------
// chunk sequences: entry i of `count`
// ---------------------------------------------------------------------------------------
struct Q8SeqDense {     // 0 .. count-1
    int count;
    __device__ __forceinline__ int at(int i) const { return i; }
};
struct Q8SeqSlice {     // q0 .. q0 + count-1
    int count, q0;
    __device__ __forceinline__ int at(int i) const { return q0 + i; }
};
// lst[0 .. count-1] (wave-uniform addresses: scalar loads).  A count or an index outside its range is clamped, so a list
// this library did not build cannot send a DMA out of the operands.
struct Q8SeqList {
    int count;
    const int* lst;
    int nchunks;
    __device__ __forceinline__ Q8SeqList(const int* lst_, int cnt, int nchunks_)
        : count(cnt < 0 ? 0 : (cnt > nchunks_ ? nchunks_ : cnt)), lst(lst_), nchunks(nchunks_) {}
    __device__ __forceinline__ int at(int i) const {
        const int q = lst[i];
        return q < 0 ? 0 : (q >= nchunks ? nchunks - 1 : q);
    }
};

// ---------------------------------------------------------------------------------------
// ring driver: body(sa, sb) is called once per entry of `seq`, in order, with the LDS addresses of its landed A and B
// regions; entries i+1 .. i+NSTAGE-2 stay in flight across the barrier.  A short sequence fills part of the prologue; an
// empty one runs neither loop.
// ---------------------------------------------------------------------------------------
template <class T, class A, class Seq, class Body>
__device__ __forceinline__ void q8_ring(const IgemmArgs& __restrict__ a, const A& aop, const Seq& seq, int mt, char* smem, const Q8Wave& w,
                                        Body body) {
    constexpr int NSTAGE = T::NSTAGE, STAGE_BYTES = A::BYTES + T::B_BYTES;
    // (a wave that issues more than DMIN per stage waits for more: in-order completion)
    constexpr int DMIN = A::DMIN + T::B_IT;
    Q8PixelsB<T> bop;
    bop.setup(a, mt, w.tid);
    auto stage = [&](int q, int buf) {
        char* sa = smem + buf * STAGE_BYTES;
        aop.issue(a, q, sa, w.wave);
        bop.issue(a, q, sa + A::BYTES, w.wave);
    };
    const int n = seq.count;
#pragma unroll
    for (int p = 0; p < NSTAGE - 1; ++p)
        if (p < n) stage(seq.at(p), p);
    int sidx = 0;
    for (int i = 0; i < n; ++i) {
        int issued = i + NSTAGE - 1;
        if (issued > n) issued = n;
        const int inflight = issued - i - 1;
        if (NSTAGE == 2 || inflight == 0) wait_vmcnt<0>();
        else wait_vmcnt<DMIN>();
        __builtin_amdgcn_s_barrier();              // entry i landed for every wave; every wave is done with entry i-1
        if (i + NSTAGE - 1 < n) {
            int ns = sidx + NSTAGE - 1;
            if (ns >= NSTAGE) ns -= NSTAGE;
            stage(seq.at(i + NSTAGE - 1), ns);
        }
        const char* sa = smem + sidx * STAGE_BYTES;
        sidx = sidx + 1 == NSTAGE ? 0 : sidx + 1;
        body(sa, sa + A::BYTES);
    }
}

// ---------------------------------------------------------------------------------------
// dense matrix step of one chunk: acc[i][j] += af[i] x bf[j], i outer, j inner
// ---------------------------------------------------------------------------------------
// F8MFMA = false (the default): the bytes are converted to fp16 in registers and multiplied by v_mfma_f32_32x32x16_f16, whose
// sum of the (exact) products is an fp32 sum -- the arithmetic of the contract, byte for byte.  F8MFMA = true
// (MCAMD_Q8_MFMA=1): one block-scaled fp8 MFMA with both e8m0 scales 1.0 per block and chunk, half the MFMA time -- but that
// instruction (and the non-scaled fp8 one) drops products more than ~14 bits below the largest of their group of 8, which
// flips ~6e-4 of the output bytes to the adjacent code.  Inline assembly as in conv_igemm_pp.hip (through the
// builtin hipcc does not accumulate in place); the blocks are independent.  hipcc pads no hazard in front of inline assembly:
// operands that come from LDS reads are waited for, but where VALU instructions just wrote the A fragment (VALU_A:
// conv_q8_w4.hip's decode) every string opens with `s_nop 1`, the two wait states a VALU write of an MFMA source operand
// needs on gfx950 -- and q8_mma_drain() pads the other end.
#define Q8_F8_MFMA "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
template <bool F8MFMA, bool VALU_A, int TM, int TN>
__device__ __forceinline__ void q8_mma(f32x16_t (&acc)[TM][TN], const i32x8_t (&af)[TM], const i32x8_t (&bf)[TN]) {
    if constexpr (F8MFMA) {
        const int SC = 127 * 0x01010101;           // e8m0 1.0 in all four scale bytes
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if constexpr (VALU_A)
                    asm volatile("s_nop 1\n\t" Q8_F8_MFMA : "+v"(acc[i][j]) : "v"(af[i]), "v"(bf[j]), "v"(SC), "v"(SC));
                else
                    asm volatile(Q8_F8_MFMA : "+v"(acc[i][j]) : "v"(af[i]), "v"(bf[j]), "v"(SC), "v"(SC));
            }
    } else {
        // four 16-k steps: 8-byte piece s4 of the lane's 32 bytes of both operands (lanes h = 0 / 1 hold disjoint k)
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

// behind the K loop: last (assembly) MFMA -> VALU reads of the accumulators.  Unconditional, so also behind an empty sequence.
template <bool F8MFMA>
__device__ __forceinline__ void q8_mma_drain() {
    if constexpr (F8MFMA) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
}

// the step of a kernel whose A fragment is 32 e4m3 bytes: a_frag(i) -> i32x8_t of block i
template <class T, bool F8MFMA, bool VALU_A, class AFrag>
__device__ __forceinline__ void q8_dense_step(f32x16_t (&acc)[T::TM][T::TN], const char* sb, const Q8Lane<T>& ln, AFrag a_frag) {
    i32x8_t af[T::TM], bf[T::TN];
#pragma unroll
    for (int i = 0; i < T::TM; ++i) af[i] = a_frag(i);
#pragma unroll
    for (int j = 0; j < T::TN; ++j) bf[j] = q8_row_frag(sb, ln.b[j]);
    q8_mma<F8MFMA, VALU_A>(acc, af, bf);
}

// ---------------------------------------------------------------------------------------
// inference epilogue, behind a barrier that ends the K loop's use of `smem`:  v = leaky(scale[n] * 2^-(e[n] + 1) * S + shift[n])
// ---------------------------------------------------------------------------------------
// The tile is laid down in LDS as [pixel][channel] in the format of each destination -- e4m3(2 v) bytes for a destination an
// fp8 block reads (ONE rounding from fp32), fp16 otherwise (conv_epi.h: write_ch_tile) -- and stored PLAIN / POOL (+ the
// optional full-resolution copy y2) / REORG by the store every forward implicit-GEMM kernel uses (store_pad_tile).  With a
// Q8Border (slim models) the fp32 table entry of the pixel's border class joins the raw value
// 2^-(e[n] + 1) * S in front of the affine step.
template <class T, class BorderOf = NoBorder>
__device__ __forceinline__ void q8_infer_epilogue(const IgemmArgs& __restrict__ a, const f32x16_t (&acc)[T::TM][T::TN],
                                                  const int* __restrict__ wexp, int y_f8, int y2_f8, char* smem, int mt, int nt,
                                                  const Q8Wave& w, BorderOf border_of = BorderOf()) {
    const bool has2 = a.y2 != nullptr;
    const bool need_b = y_f8 || (has2 && y2_f8), need_h = !y_f8 || (has2 && !y2_f8);
    char* bt = smem;                               // [BNP][PB] e4m3 tile
    half_t* ht = (half_t*)(smem + (need_b ? T::TILE_BYTES : 0));   // [BNP][PB] fp16 tile
    // the per-filter scale with the power of two of the packed weights and of the 2 x activations taken back (exact)
    const float* scale = a.scale;
    bool sat;
    if constexpr (BorderOf::on)
        sat = write_ch_tile<T::BMW, T::PB, T::WM, T::WN>(a, acc, [scale](int n) { return scale ? scale[n] : 1.f; }, need_b, need_h, bt,
                                                         ht, nt, w.wm, w.wn, w.lane, border_of);
    else
        sat = write_ch_tile<T::BMW, T::PB, T::WM, T::WN>(a, acc, [scale, wexp](int n) { return ldexpf(scale ? scale[n] : 1.f, -(wexp[n] + 1)); },
                                                         need_b, need_h, bt, ht, nt, w.wm, w.wn, w.lane);
    __syncthreads();
    store_pad_tile<T::BNP, T::BMW, T::PB, T::NT>(a, bt, ht, y_f8 != 0, y2_f8 != 0, mt, nt, w.tid);
    if (sat && a.overflow) atomicOr(a.overflow, 1);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// dynamic LDS of an inference launch: the ring, or the epilogue's tiles where they are larger -- a byte and an fp16 tile when
// the destinations y / y2 take both formats, else room for the fp16 one
constexpr int q8_infer_lds_max(int ring, int tile) { return ring > 3 * tile ? ring : 3 * tile; }
static inline int q8_infer_lds(int ring, int tile, const IgemmArgs& a, int y_f8, int y2_f8) {
    const bool has2 = a.y2 != nullptr;
    const bool mixed = (y_f8 || (has2 && y2_f8)) && (!y_f8 || (has2 && !y2_f8));
    const int tiles = (mixed ? 3 : 2) * tile;
    return ring > tiles ? ring : tiles;
}

// pixel / filter tiles of a choice's (bmw, bnp) and its grid: whole rounds of 8 pixel tiles (xcd_tile)
static inline void q8_choice_grid(Q8Choice& c, long long M, int N) {
    c.mtiles = (int)((M + c.bnp - 1) / c.bnp);
    c.ntiles = (N + c.bmw - 1) / c.bmw;
    c.grid = (c.mtiles + 7) / 8 * 8 * c.ntiles;
}

// the five instances a Q8Choice of mcamd_q8_choice can name: launch(tile, f8mfma) with a Q8Tile and a std::bool_constant
template <class Launch>
static int q8_dispatch(const Q8Choice& c, const char* what, Launch launch) {
    if (c.bnp == 128 && c.stages == 3) {
        if (c.f8mfma && c.bmw == 256) return launch(Q8Tile<256, 128, 64, 64, 3>(), std::true_type());
        if (c.f8mfma && c.bmw == 128) return launch(Q8Tile<128, 128, 64, 64, 3>(), std::true_type());
        if (c.f8mfma && c.bmw == 64) return launch(Q8Tile<64, 128, 32, 64, 3>(), std::true_type());
        if (!c.f8mfma && c.bmw == 128) return launch(Q8Tile<128, 128, 64, 64, 3>(), std::false_type());
        if (!c.f8mfma && c.bmw == 64) return launch(Q8Tile<64, 128, 32, 64, 3>(), std::false_type());
    }
    mcamd_set_error("%s: no kernel instance %d x %d, fp8 MFMA %d, %d stages", what, c.bmw, c.bnp, c.f8mfma, c.stages);
    return MCAMD_EINVAL;
}
