// BatchNorm + LeakyReLU of a PLAIN block fused into the split-operand forward of the 1x1 convolution that follows it
// (mcamd_bn_act_conv1x1_fwd, include/mcamd.h).
//
// A 1x1 convolution has no taps: the A operand of output pixel m is pixel m of its input.  The two-kernel route writes
// that input as hi | lo planes (bn_act_fwd_kernel, 4 bytes per activation) and reads it back (igemm_kernel over
// [x_hi | x_lo | x_hi] x [w_hi | w_hi | w_lo]).  Here a workgroup loads the producer's fp32 raw output y of its 128 pixels
// once, applies leaky(y * scale + shift), splits into hi and lo in registers (conv_epi.h: the activation pass's own
// expressions), stores the hi plane -- the backward pass reads it -- and lays the K chunks down in the swizzled LDS rows
// igemm_kernel's fragment reads expect; the lo plane never exists in memory.  The weights (B) stay on LDS-DMA.
//
// Bit-equal to the two launches it replaces: every 32 x 32 accumulator block receives the same 32x32x16 f16 MFMAs in the
// same K order ([64-channel block][channel] within a part, parts hi, lo, hi), the M tiles are 128 pixels in wave rows of
// 64 dealt to the same persistent slots, and the epilogue is conv_epi.h's (MCAMD_EPI_RAW_F32): same y, same statistics slab.
//
// Workgroup: 128 pixels x BN (64 or 128) channels, 2 x (BN / 32) waves of 64 x 32.  A thread owns one 8-channel piece
// position j8 of the 64-channel blocks and the rows rsub + rg * (NT / 8): CB * RG pieces, hi and lo packed in 8 registers
// each (64 at most), kept across the three parts so that y is read once.
//
// Replaces nn.BatchNorm2d + nn.LeakyReLU + F.conv2d (reference src/nets.py:802-809, src/pruning/weightPruning/layers.py:60-64)
// for such a pair.
#include "kernels.h"
#include "conv_epi.h"

template <int BN, int CB>
__global__ __launch_bounds__(4 * BN, BN >= 128 ? 2 : 3)
void bn_conv1x1_kernel(IgemmArgs a, const float* __restrict__ py, int py_ld, int py_choff) {
    constexpr int BM = 128, WM = 64, WN = 32, BK = 64, CPR = BK / 8;
    constexpr int WAVES_N = BN / WN;
    constexpr int NT = (BM / WM) * WAVES_N * 64;
    constexpr int RSTEP = NT / 8;              // rows between a thread's pieces
    constexpr int RG = BM / RSTEP;             // row groups: pieces per thread and 64-channel block
    constexpr int KP = CB * RG;                // pieces per thread
    constexpr int A_SLOTS = BM * CPR, B_SLOTS = BN * CPR;
    constexpr int B_IT = B_SLOTS / NT;
    constexpr int STAGE_BYTES = (A_SLOTS + B_SLOTS) * 16;
    constexpr int NCH = 3 * CB;                // K chunks: hi, lo, hi
    constexpr int TM = WM / 32, TN = WN / 32;
    static_assert(KP <= 8, "hi and lo of a thread's pieces stay in 64 registers");
    static_assert(B_SLOTS % NT == 0 && RSTEP * RG == BM, "whole waves per DMA instruction, whole pieces per thread");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    int nt, pslot;
    if (!xcd_tile(1, a.num_pslots, nt, pslot)) return;   // one column tile: nt = 0
    const int j8 = tid & 7, rsub = tid >> 3;

    long long bbase[B_IT];
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
        int slot = it * NT + tid;
        int row = slot / CPR, phys = slot % CPR;
        bbase[it] = (long long)row * a.ktot + (phys ^ swz<CPR>(row)) * 8;
    }

    float s1[TN], s2[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) s1[j] = s2[j] = 0.f;

    for (int mt = pslot; mt < a.num_mtiles; mt += a.num_pslots) {
        // ---- the thread's pieces of the producer's raw output (rows past the last pixel re-read it: masked below) ----
        f32x4_t raw[KP][2];
        half_t* hdst[RG];
        bool real[RG];
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) {
            const int m = mt * BM + rg * RSTEP + rsub;
            const int mc = m < a.M ? m : a.M - 1;
            real[rg] = m < a.M;
            hdst[rg] = (half_t*)a.x + tile_x_base(a, false, m) + a.tap_off[0] + j8 * 8;   // pixel m, channel j8 * 8 of the hi plane
            const float* src = py + (long long)mc * py_ld + py_choff + j8 * 8;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                raw[cb * RG + rg][0] = *(const f32x4_t*)(src + cb * 64);
                raw[cb * RG + rg][1] = *(const f32x4_t*)(src + cb * 64 + 4);
            }
        }
        h8_t hi[KP], lo[KP];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            const float *scp = pin_here(a.scale) + cb * 64 + j8 * 8, *shp = pin_here(a.shift) + cb * 64 + j8 * 8;
            const f32x4_t sc0 = *(const f32x4_t*)scp, sc1 = *(const f32x4_t*)(scp + 4);
            const f32x4_t sh0 = *(const f32x4_t*)shp, sh1 = *(const f32x4_t*)(shp + 4);
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) {
                const int k = cb * RG + rg;
                float v[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = bn_leaky(raw[k][0][i], sc0[i], sh0[i], a.slope);
                    v[4 + i] = bn_leaky(raw[k][1][i], sc1[i], sh1[i], a.slope);
                }
                split_hi_lo(v, hi[k], lo[k]);
                if (real[rg]) *(h8_t*)(hdst[rg] + cb * 64) = hi[k];
            }
        }

        f32x16_t acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        // chunk q: part q / CB (hi, lo, hi), 64-channel block q % CB -- A from the registers, B by LDS-DMA
        auto stage = [&](int q, int buf) {
            char* sa = smem + buf * STAGE_BYTES;
            char* sb = sa + A_SLOTS * 16;
#pragma unroll
            for (int it = 0; it < B_IT; ++it)
                glds16(a.w + bbase[it] + (long long)q * BK, sb + (it * NT + wave * 64) * 16);
            const int part = q / CB, cb = q - part * CB;
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) {
                const int row = rg * RSTEP + rsub;
                *(h8_t*)(sa + (row * CPR + (j8 ^ swz<CPR>(row))) * 16) = part == 1 ? lo[cb * RG + rg] : hi[cb * RG + rg];
            }
        };

        __syncthreads();  // previous tile's last chunk has been read
        stage(0, 0);
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
            __syncthreads();  // chunk q is in LDS (DMA and ds_write drained); every wave is done reading chunk q - 1
            if (q + 1 < NCH) stage(q + 1, (q + 1) & 1);
            const char* sa = smem + (q & 1) * STAGE_BYTES;
            const char* sb = sa + A_SLOTS * 16;
            // igemm_kernel's sub-steps: the ds_reads of k16 sub-step s + 1 are issued before the MFMAs of sub-step s
            constexpr int KS = BK / 16;
            h8_t af[2][TM], bf[2][TN];
            auto load_frags = [&](int s, int set) {
                const int chunk = 2 * s + (lane >> 5);
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    int row = wm * WM + i * 32 + (lane & 31);
                    af[set][i] = *(const h8_t*)(sa + (row * CPR + (chunk ^ swz<CPR>(row))) * 16);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    int row = wn * WN + j * 32 + (lane & 31);
                    bf[set][j] = *(const h8_t*)(sb + (row * CPR + (chunk ^ swz<CPR>(row))) * 16);
                }
            };
            load_frags(0, 0);
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (s + 1 < KS) load_frags(s + 1, (s + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[s & 1][i], bf[s & 1][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        store_raw32_tile<BM, BN, WM, WN>(a, acc, mt, nt, wm, wn, lane, s1, s2);
    }
    if (a.stats) store_stats_slab<BM, BN, WM, WN, NT>(a, smem, s1, s2, pslot, nt, wm, wn, lane, tid);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// The shapes with a kernel instance: P input channels in blocks of 64, cout in one column tile of 64 or 128, and a thread's
// converted pieces within 64 registers (P <= 2 x the column tile).
bool mcamd_bn_conv1x1_shape_ok(int P, int cout) {
    if (P <= 0 || P % 64 != 0 || cout <= 0 || cout > 128 || cout % 8 != 0) return false;
    return P <= 2 * (cout <= 64 ? 64 : 128);
}

// The instance a pair takes and its launch dimensions: the launch and mcamd_bn_act_conv1x1_info both ask here.  The column
// tile is the narrower one that holds cout; the grid is the persistent slots (statistics rows) rounded up to the 8 XCDs
// plus one workgroup per XCD (xcd_tile); LDS: two stages of A and B rows of 64 halfs (>= the statistics scratch).
bool mcamd_bn_conv1x1_choice(int P, int cout, long long M, int rows, BnConv1x1Choice* c) {
    if (!mcamd_bn_conv1x1_shape_ok(P, cout) || M <= 0 || rows <= 0) return false;
    c->bn = cout <= 64 ? 64 : 128;
    c->cb = P / 64;
    c->threads = 4 * c->bn;
    c->rows = rows;
    c->num_mtiles = (int)((M + 127) / 128);
    c->grid = round_up_int(rows, 8) + 8;
    c->lds_bytes = 2 * (128 + c->bn) * 8 * 16;
    return true;
}

template <int BN, int CB>
static void launch_bc(const IgemmArgs& a, const BnConv1x1Choice& c, const float* py, int py_ld, int py_choff, hipStream_t st) {
    if (c.lds_bytes > 64 * 1024) MCAMD_LDS_OPT_IN((bn_conv1x1_kernel<BN, CB>), c.lds_bytes);
    hipLaunchKernelGGL((bn_conv1x1_kernel<BN, CB>), dim3(c.grid), dim3(c.threads), c.lds_bytes, st, a, py, py_ld, py_choff);
}

// a: filled as for the consumer's igemm launch (x = the consumer's padded input, whose hi plane is written), plus the
// producer's scale / shift / slope; P = the producer's channels; rows = persistent workgroups (statistics slab rows)
int mcamd_bn_conv1x1_launch(IgemmArgs& a, const float* py, int py_ld, int py_choff, int P, int rows, hipStream_t st) {
    BnConv1x1Choice c;
    if (a.ktot != 3 * P || !mcamd_bn_conv1x1_choice(P, a.N, a.M, rows, &c)) {
        mcamd_set_error("bn_act_conv1x1: no kernel instance for %d -> %d channels", P, a.N);
        return MCAMD_EINVAL;
    }
    a.num_mtiles = c.num_mtiles;
    a.num_pslots = c.rows;
    a.num_ntiles = 1;
    a.xcd_order = 1;
    switch (c.bn * 8 + c.cb) {
    case 64 * 8 + 1: launch_bc<64, 1>(a, c, py, py_ld, py_choff, st); break;
    case 64 * 8 + 2: launch_bc<64, 2>(a, c, py, py_ld, py_choff, st); break;
    case 128 * 8 + 1: launch_bc<128, 1>(a, c, py, py_ld, py_choff, st); break;
    case 128 * 8 + 2: launch_bc<128, 2>(a, c, py, py_ld, py_choff, st); break;
    case 128 * 8 + 3: launch_bc<128, 3>(a, c, py, py_ld, py_choff, st); break;
    case 128 * 8 + 4: launch_bc<128, 4>(a, c, py, py_ld, py_choff, st); break;
    default:
        mcamd_set_error("bn_act_conv1x1: no kernel instance <%d, %d>", c.bn, c.cb);
        return MCAMD_EINVAL;
    }
    MCAMD_LAUNCH_CHECK("bn_act_conv1x1");
    return MCAMD_OK;
}
