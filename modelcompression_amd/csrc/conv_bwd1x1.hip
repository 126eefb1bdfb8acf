// The whole backward of a dense 1x1 convolution in one launch, for gfx950 (MI355X):
//
//   G[p][c]   = sum_n dY[p][n] W[n][c]          (input gradient, fp16, saturated like mcamd_conv_dgrad)
//   dW[n][c] += sum_p dY[p][n] X[p][c]          (weight gradient, one fp32 slab per workgroup)
//   the BatchNorm-backward sums of the block that produced X, from G as stored and X (mcamd_dgrad_sums)
//
// The narrow 1x1 blocks of the early layers (conv4: 128 -> 64 at 104 x 104, conv7: 256 -> 128 at 52 x 52) are bound by
// HBM, and the dgrad launch (reads dY and X, writes G) and the wgrad launch (reads X and dY again) move X and dY twice.
// Here a persistent workgroup (8 waves, one per CU) brings a tile of P pixels of dY and of X on chip ONCE:
//
//   global -> registers (the loads of tile t + 1 are in flight while tile t is worked on) -> LDS, rows swizzled for the
//   transposing reads of tr_frag.h;
//   G^T tile = W^T dY^T with W^T as the A operand, resident in LDS for the whole launch (the dgrad packing [cin][cout], rows
//   swizzled): a lane then holds four consecutive channels of one pixel, one 8-byte LDS write each;
//   the G tile leaves LDS in 16-byte pieces, and the thread that stores a piece adds its eight channels' BatchNorm sums
//   with the X piece of the same pixel, which is in LDS already;
//   dW accumulators += dY^T X from the same staged tiles, both operands gathered with ds_read_b64_tr_b16.
//
// After its last tile the workgroup writes its accumulators as split `blockIdx.x` of the slab layout
// [nsplit][rows_pad][ktot] that wgrad_finish_vec_kernel sums, and its BatchNorm sums as row `blockIdx.x` of the slab
// bn_bwd_finalize_kernel reads.  The grid and the tile -> workgroup map are functions of the geometry alone, no workgroup
// waits for another, nothing is accumulated with atomics: two runs give the same bits.  A workgroup without a tile writes
// zeros.
#include "conv_epi.h"
#include "tr_frag.h"
#include <string.h>

struct Bwd1x1Args {
    const half_t* dy;    // padded NHWC, pixel (0,0,0) of the form `pw`
    const half_t* x;     // the same form
    const half_t* w;     // dgrad packing [CIN][COUT]
    half_t* g;           // raw [M][g_ld]
    float* slab;         // [grid][COUT][CIN]
    int* overflow;
    int dy_ld, dy_choff, x_ld, x_choff, g_ld, g_choff;
    int H, W, HW, M, pw;
    int ntiles;
    DgradSums bsum;      // slab == NULL: no sums.  act / act_ld / act_choff / act_pw are not read: the activation is x
};

// pixel of GEMM row m0 + r, from the (wave-uniform) pixel of row m0: r < 128, so the carries are a few steps
__device__ __forceinline__ void step_pixel(int b0, int h0, int w0, int r, int H, int W, int& b, int& h, int& w) {
    b = b0, h = h0, w = w0 + r;
    while (w >= W) w -= W, ++h;
    while (h >= H) h -= H, ++b;
}

template <int COUT, int CIN, int P>
__global__ __launch_bounds__(512, 1) void bwd1x1_kernel(Bwd1x1Args a) {
    constexpr int NT = 512;
    constexpr int A_CH = COUT / 8, B_CH = CIN / 8;              // 16-byte pieces per pixel of dY / X
    constexpr int A_IT = P * A_CH / NT, B_IT = P * B_CH / NT;   // pieces per thread and tile
    constexpr int A_RS = NT / A_CH, B_RS = NT / B_CH;           // rows between a thread's pieces
    constexpr int RBA = COUT * 2;                               // bytes per dY row in LDS
    constexpr int NH = CIN / 128;                               // X lies in LDS as NH planes [P][128 channels] (256-byte rows)
    constexpr int XPLANE = P * 256;
    constexpr int GP = CIN + 4;                                 // G tile pitch (fp16): the 8-byte column writes spread over the banks
    constexpr int SA = 0, SX = P * RBA, SG = SX + NH * XPLANE, SW = SG + P * GP * 2;
    constexpr int KS = COUT / 16;                               // k16 steps of the G product
    constexpr int NCB = CIN / 32;                               // 32-channel blocks of G
    constexpr int PBW = (P / 32) / (8 / NCB);                   // pixel blocks of G per wave
    constexpr int DI = COUT / 64, DJ = CIN / 128;               // dW: 2 x 4 waves, DI x DJ blocks of 32 x 32 each
    static_assert(RBA == 256 || RBA == 128, "dY rows of 64 or 128 filters");
    static_assert(CIN % 128 == 0 && NCB <= 8 && PBW >= 1 && A_IT >= 1 && B_IT >= 1, "tile shape");
    static_assert(P * A_CH % NT == 0 && P * B_CH % NT == 0 && NT % B_CH == 0 && CIN * A_CH % NT == 0, "whole pieces per thread");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // this workgroup's tiles: a contiguous, balanced range
    const int t0 = (int)((long long)blockIdx.x * a.ntiles / gridDim.x);
    const int t1 = (int)((long long)(blockIdx.x + 1) * a.ntiles / gridDim.x);

    // ---- W^T, resident in LDS for the whole launch as [c][k] rows with their 16-byte pieces XOR-swizzled by the row: the A
    // fragment of k16 step s is lane's W[k = 16 s + 8 (lane >> 5) + j][c = 32 cb + (lane & 31)], one 16-byte read
    // (in registers the 128 x 256 instance went 17 registers over its budget)
    const int cb = wave % NCB, pb0 = (wave / NCB) * PBW;
#pragma unroll
    for (int it = 0; it < CIN * A_CH / NT; ++it) {
        const int piece = it * NT + tid, c = piece / A_CH, ch = piece % A_CH;
        *(h8_t*)(smem + SW + c * RBA + ((ch ^ (c & (A_CH - 1))) << 4)) = *(const h8_t*)(a.w + c * COUT + ch * 8);
    }
    const int wrow = cb * 32 + (lane & 31);
    const char* wlane = smem + SW + wrow * RBA;      // (first read behind the tile loop's first barrier)

    // ---- BatchNorm sums: a thread keeps the same eight channels for every piece it stores
    const bool SUMS = a.bsum.slab != nullptr;
    const int sch = tid % B_CH, srow0 = tid / B_CH;
    const int sc0 = sch * 8 - a.bsum.ch_lo;                      // producer channel of this thread's first column
    const bool live = SUMS && sc0 >= 0 && sc0 < a.bsum.C;
    float sb[8], sg[8], off[8], mul[8];
    bool usey[8];
    bool need_y = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) sb[i] = sg[i] = 0.f, off[i] = 0.f, mul[i] = 0.f, usey[i] = false;
    if (live) {
        float sc[8], sh[8], mu[8], is[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            sc[i] = a.bsum.scale[sc0 + i], sh[i] = a.bsum.shift[sc0 + i], mu[i] = a.bsum.mean[sc0 + i], is[i] = a.bsum.invstd[sc0 + i];
        need_y = act_xhat_source(sc, sh, mu, is, a.bsum.y != nullptr, off, mul, usey);
#pragma unroll
        for (int i = 0; i < 8; ++i) mul[i] = usey[i] ? 0.f : mul[i];   // (those channels' xhat sums: behind the tile loop)
    }
    const float slope = a.bsum.slope, inv_slope = SUMS ? 1.0f / slope : 1.f;

    f32x16_t dw[DI][DJ];
#pragma unroll
    for (int i = 0; i < DI; ++i)
#pragma unroll
        for (int j = 0; j < DJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) dw[i][j][r] = 0.f;
    bool sat = false;

    // ---- staging: global -> registers (always loaded, from the last pixel for rows past it: a conditional load makes the
    // compiler wait for the loads before it), registers -> LDS at the swizzled places the transposing reads expect, zeros
    // for the rows past the last pixel (their dY adds nothing to dW, their G is not stored)
    h8_t ra[A_IT], rb[B_IT];
    auto load_tile = [&](int t) {
        const int m0 = t * P;
        int b0, h0, w0;
        split_pixel(m0, a.HW, a.W, b0, h0, w0);
#pragma unroll
        for (int it = 0; it < A_IT; ++it) {
            const int row = tid / A_CH + it * A_RS, ch = tid % A_CH;
            int b, h, w;
            step_pixel(b0, h0, w0, m0 + row < a.M ? row : a.M - 1 - m0, a.H, a.W, b, h, w);
            ra[it] = *(const h8_t*)(a.dy + pad_off(b, h, w, a.H, a.W, a.dy_ld, a.pw) + a.dy_choff + ch * 8);
        }
#pragma unroll
        for (int it = 0; it < B_IT; ++it) {
            const int row = tid / B_CH + it * B_RS, ch = tid % B_CH;
            int b, h, w;
            step_pixel(b0, h0, w0, m0 + row < a.M ? row : a.M - 1 - m0, a.H, a.W, b, h, w);
            rb[it] = *(const h8_t*)(a.x + pad_off(b, h, w, a.H, a.W, a.x_ld, a.pw) + a.x_choff + ch * 8);
        }
    };
    auto put_tile = [&](int t) {
        const int mlim = a.M - t * P;
        const h8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int it = 0; it < A_IT; ++it) {
            const int row = tid / A_CH + it * A_RS, ch = tid % A_CH;
            *(h8_t*)(smem + SA + row * RBA + ((ch ^ tr_swz<RBA>(row)) << 4)) = row < mlim ? ra[it] : zero;
        }
#pragma unroll
        for (int it = 0; it < B_IT; ++it) {
            const int row = tid / B_CH + it * B_RS, ch = tid % B_CH;
            *(h8_t*)(smem + SX + (ch >> 4) * XPLANE + row * 256 + (((ch & 15) ^ tr_swz<256>(row)) << 4)) = row < mlim ? rb[it] : zero;
        }
    };

    if (t0 < t1) load_tile(t0);
    for (int t = t0; t < t1; ++t) {
        put_tile(t);
        __syncthreads();
        if (t + 1 < t1) load_tile(t + 1);          // in flight until the top of the next iteration

        // ---- G^T = W^T dY^T: rows = channels 32 cb .., columns = pixels
        {
            f32x16_t g[PBW];
#pragma unroll
            for (int q = 0; q < PBW; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) g[q][r] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const h8_t wfs = *(const h8_t*)(wlane + (((2 * s + (lane >> 5)) ^ (wrow & (A_CH - 1))) << 4));
#pragma unroll
                for (int q = 0; q < PBW; ++q) {
                    const int row = (pb0 + q) * 32 + (lane & 31), ch = 2 * s + (lane >> 5);
                    const h8_t df = *(const h8_t*)(smem + SA + row * RBA + ((ch ^ tr_swz<RBA>(row)) << 4));
                    g[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wfs, df, g[q], 0, 0, 0);
                }
            }
            half_t* gt = (half_t*)(smem + SG);
#pragma unroll
            for (int q = 0; q < PBW; ++q) {
                const int row = (pb0 + q) * 32 + (lane & 31);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    h4_t hv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float f = g[q][4 * v + e];
                        sat |= fabsf(f) > 65504.f;
                        hv[e] = (half_t)fminf(fmaxf(f, -65504.f), 65504.f);   // saturate, never inf
                    }
                    *(h4_t*)(gt + row * GP + cb * 32 + 8 * v + 4 * (lane >> 5)) = hv;
                }
            }
        }
        __syncthreads();

        // ---- the G tile out, 16 bytes per thread and piece, and the sums of its eight channels
        {
            const half_t* gt = (const half_t*)(smem + SG);
#pragma unroll
            for (int k = 0; k < B_IT; ++k) {
                const int row = srow0 + k * B_RS, m = t * P + row;
                if (m >= a.M) continue;
                const h4_t g0 = *(const h4_t*)(gt + row * GP + sch * 8), g1 = *(const h4_t*)(gt + row * GP + sch * 8 + 4);
                const h8_t gq = __builtin_shufflevector(g0, g1, 0, 1, 2, 3, 4, 5, 6, 7);
                *(h8_t*)(a.g + (long long)m * a.g_ld + a.g_choff + sch * 8) = gq;
                if (!live) continue;
                const h8_t av8 = *(const h8_t*)(smem + SX + (sch >> 4) * XPLANE + row * 256 + (((sch & 15) ^ tr_swz<256>(row)) << 4));
                float z[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float av = (float)av8[i];
                    z[i] = av > 0.f ? av : av * inv_slope;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float gv = (float)gq[i];
                    const float gz = (float)av8[i] > 0.f ? gv : gv * slope;
                    sb[i] += gz;
                    sg[i] += gz * ((z[i] - off[i]) * mul[i]);
                }
            }
        }

        // ---- dW += dY^T X: wave (wave >> 2, wave & 3) owns DI x DJ blocks
#pragma unroll
        for (int s = 0; s < P / 16; ++s) {
            h8_t af[DI], bf[DJ];
#pragma unroll
            for (int i = 0; i < DI; ++i) af[i] = tr_frag_rows_builtin<RBA>(smem + SA, 16 * s, ((wave >> 2) * DI + i) * 32, lane);
#pragma unroll
            for (int j = 0; j < DJ; ++j) {
                const int col = ((wave & 3) * DJ + j) * 32;
                bf[j] = tr_frag_rows_builtin<256>(smem + SX + (col >> 7) * XPLANE, 16 * s, col & 127, lane);
            }
#pragma unroll
            for (int i = 0; i < DI; ++i)
#pragma unroll
                for (int j = 0; j < DJ; ++j) dw[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], dw[i][j], 0, 0, 0);
        }
        __syncthreads();   // every wave is done with the staged tiles and the G tile
    }

    // ---- ill-conditioned channels (rare): xhat comes from the saved fp32 y, not from the activation.  The tile loop has
    // added nothing for them (mul = 0; a load under a condition there would make every piece wait for the next tile's
    // loads); the thread goes over its own pieces again -- the G it stored itself, x and y from memory.
    if (need_y) {
        float sc[8], sh[8], mu[8], is[8], off2[8], mul2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            sc[i] = a.bsum.scale[sc0 + i], sh[i] = a.bsum.shift[sc0 + i], mu[i] = a.bsum.mean[sc0 + i], is[i] = a.bsum.invstd[sc0 + i];
        act_xhat_source(sc, sh, mu, is, true, off2, mul2, usey);
        for (int t = t0; t < t1; ++t)
            for (int k = 0; k < B_IT; ++k) {
                const int m = t * P + srow0 + k * B_RS;
                if (m >= a.M) continue;
                int b, h, w;
                split_pixel(m, a.HW, a.W, b, h, w);
                const h8_t gq = *(const h8_t*)(a.g + (long long)m * a.g_ld + a.g_choff + sch * 8);
                const h8_t av8 = *(const h8_t*)(a.x + pad_off(b, h, w, a.H, a.W, a.x_ld, a.pw) + a.x_choff + sch * 8);
                const float* yp = a.bsum.y + (long long)m * a.bsum.y_ld + a.bsum.y_choff + sc0;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float gv = (float)gq[i];
                    const float gz = (float)av8[i] > 0.f ? gv : gv * slope;
                    if (usey[i]) sg[i] += gz * ((yp[i] - off2[i]) * mul2[i]);
                }
            }
    }

    if (sat && a.overflow) atomicOr(a.overflow, 1);

    // ---- this workgroup's split of the dW slab
    float* out = a.slab + (long long)blockIdx.x * COUT * CIN;
#pragma unroll
    for (int i = 0; i < DI; ++i)
#pragma unroll
        for (int j = 0; j < DJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = ((wave >> 2) * DI + i) * 32 + mfma32_row(r, lane);
                const int k = ((wave & 3) * DJ + j) * 32 + (lane & 31);
                out[n * CIN + k] = dw[i][j][r];
            }

    // ---- ... and its row of the sums slab: the B_RS threads that share a channel, in order
    if (SUMS) {
        constexpr int PITCH = NT + 8;
        float* red = (float*)smem;               // [16 values][NT threads]
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            red[i * PITCH + tid] = sb[i];
            red[(8 + i) * PITCH + tid] = sg[i];
        }
        __syncthreads();
        for (int e = tid; e < 2 * CIN; e += NT) {
            const int which = e / CIN, col = e - which * CIN;
            const int c = col - a.bsum.ch_lo;
            if (c < 0 || c >= a.bsum.C) continue;
            const int v = which * 8 + (col & 7), chq = col >> 3;
            float s = 0.f;
            for (int r = 0; r < B_RS; ++r) s += red[v * PITCH + r * B_CH + chq];
            a.bsum.slab[((long long)blockIdx.x * 2 + which) * a.bsum.ld + c] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Instances: (Cout, Cin) and the pixels per tile; the staged tiles take 48 KB and the G tile 33 KB of LDS in both, W 16 / 64 KB.
#define BWD1X1_INSTANCES(X) X(64, 128, 128) X(128, 256, 64)

const char* mcamd_bwd1x1_refusal(int ksize, int stem, int x_wrap, int x_f8, int cout, int cin) {
    if (ksize != 1) return "ksize must be 1";
    if (stem || x_wrap != 0 || x_f8 != 0) return "dense geometry only (no stem / x_wrap / x_f8 form)";
    if (cout % 8 != 0 || cin % 8 != 0) return "cout and cin must be multiples of 8";
#define B_OK(CO_, CI_, P_) \
    if (cout == CO_ && cin == CI_) return nullptr;
    BWD1X1_INSTANCES(B_OK)
#undef B_OK
    return "no kernel instance for this (cout, cin): (64, 128) and (128, 256) exist";
}

int mcamd_bwd1x1_launch(const Bwd1x1Launch& q, hipStream_t st) {
    Bwd1x1Args a;
    memset(&a, 0, sizeof(a));
    a.dy = q.dy, a.x = q.x, a.w = q.w, a.g = q.g, a.slab = q.slab, a.overflow = q.overflow;
    a.dy_ld = q.dy_ld, a.dy_choff = q.dy_choff, a.x_ld = q.x_ld, a.x_choff = q.x_choff, a.g_ld = q.g_ld, a.g_choff = q.g_choff;
    a.H = q.H, a.W = q.W, a.HW = q.H * q.W, a.M = q.M, a.pw = q.pw;
    a.bsum = q.bsum;
    bool done = false;
#define B_CASE(CO_, CI_, P_)                                                                        \
    if (!done && q.cout == CO_ && q.cin == CI_) {                                                   \
        constexpr size_t lds = (size_t)P_ * CO_ * 2 + (size_t)P_ * CI_ * 2 + (size_t)P_ * (CI_ + 4) * 2 + (size_t)CO_ * CI_ * 2; \
        static_assert(lds >= 16 * (512 + 8) * sizeof(float), "the sums reduction reuses the tiles");  \
        a.ntiles = (q.M + P_ - 1) / P_;                                                             \
        MCAMD_LDS_OPT_IN((bwd1x1_kernel<CO_, CI_, P_>), lds);                                       \
        hipLaunchKernelGGL((bwd1x1_kernel<CO_, CI_, P_>), dim3(MCAMD_BWD1X1_GRID), dim3(512), lds, st, a); \
        done = true;                                                                                \
    }
    BWD1X1_INSTANCES(B_CASE)
#undef B_CASE
    if (!done) {
        mcamd_set_error("conv_bwd1x1: no kernel instance for cout %d cin %d", q.cout, q.cin);
        return MCAMD_EINVAL;
    }
    MCAMD_LAUNCH_CHECK("conv_bwd1x1");
    return MCAMD_OK;
}
