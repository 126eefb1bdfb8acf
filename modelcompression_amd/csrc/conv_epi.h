// Addressing and epilogues shared by the forward implicit-GEMM kernels (conv_igemm.hip, conv_igemm_pp.hip,
// conv_sparse.hip, conv_q8.hip, conv_q8_w4.hip): GEMM row -> pixel, the store of a finished LDS tile into the consumer's padded
// buffer, the accumulators -> LDS tile step of the weights-as-A kernels, and the raw fp32 epilogue + BatchNorm partial sums of
// the byte kernels' training forms.
//
// Inference blocks whose activation pass is fused with MaxPool(2,2) / Reorg(2) (reference src/nets.py:802-821 conv ->
// BatchNorm -> LeakyReLU -> MaxPool, nets.py:648-667 Reorg): the conv epilogue has applied leaky(acc * scale + shift) and
// laid the tile [pixel][channel] down in LDS; with the M tile enumerated in POOLED order -- m = 4 * pooled pixel +
// (dy * 2 + dx) -- four consecutive rows are one 2x2 window, so the pooled output (or the reorg'ed one, or the pooled one
// plus a full-resolution copy for the route that reads conv13 beside its pool) is written straight into the consumer's
// padded buffer: the raw output never exists and no activation pass runs.
#pragma once
#include "kernels.h"

// row-major pixel index p of images of HW = H * W pixels -> (image b, pixel hw of it) -> (b, h, w)
__device__ __forceinline__ void split_image(int p, int HW, int& b, int& hw) {
    b = p / HW;
    hw = p - b * HW;
}
__device__ __forceinline__ void split_pixel(int p, int HW, int W, int& b, int& h, int& w) {
    int r;
    split_image(p, HW, b, r);
    h = r / W;
    w = r - h * W;
}

// pixel of GEMM row m: row-major, or in pooled order (four consecutive rows = one 2x2 window)
__device__ __forceinline__ void tile_pixel(const IgemmArgs& __restrict__ a, bool pooled, int m, int& b, int& h, int& w) {
    if (pooled) {
        const int Wo = a.W >> 1, q = m & 3;
        int ho, wo;
        split_pixel(m >> 2, (a.H >> 1) * Wo, Wo, b, ho, wo);
        h = 2 * ho + (q >> 1);
        w = 2 * wo + (q & 1);
    } else {
        split_pixel(m, a.HW, a.W, b, h, w);
    }
}

// offset in x (in the units of a's strides) of the top-left tap of GEMM row m; rows past the last pixel re-read it
// (their results are masked or not stored)
__device__ __forceinline__ long long tile_x_base(const IgemmArgs& __restrict__ a, bool pooled, int m) {
    if (m > a.M - 1) m = a.M - 1;
    int b, h, w;
    tile_pixel(a, pooled, m, b, h, w);
    return (long long)b * a.x_img_stride + (long long)h * a.x_row_stride + (long long)w * a.x_ld + a.x_off;
}

// All channel tiles of a pixel tile (or of a persistent M slot) on one XCD -- its activation rows stay in that XCD's
// L2: blocks are dealt round-robin to the 8 XCDs.  False for the blocks that pad the grid.
__device__ __forceinline__ bool xcd_tile(int num_ntiles, int num_slots, int& nt, int& slot) {
    const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    nt = jb % num_ntiles;
    slot = (jb / num_ntiles) * 8 + xcd;
    return slot < num_slots;
}

// ---------------------------------------------------------------------------------------
// Destinations in either format: fp16, or the e4m3 bytes an fp8 block reads
// ---------------------------------------------------------------------------------------
// e4m3(2 v) of four values, clamped to +-448 first (the conversion returns NaN above the format's maximum)
__device__ __forceinline__ int e4m3_bytes4(const float* v) {
    float c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = fminf(fmaxf(v[e] * 2.f, -448.f), 448.f);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], 0, false);
    return __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], w, true);
}

// ... and back: eight e4m3 codes -> eight fp16 values (exact: every e4m3 value is an fp16 value)
__device__ __forceinline__ h8_t q8_to_f16(int lo, int hi) {
    const h2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false), p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true);
    const h2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false), p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true);
    const h4_t a = __builtin_shufflevector(p0, p1, 0, 1, 2, 3), b = __builtin_shufflevector(p2, p3, 0, 1, 2, 3);
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// order-preserving key of four e4m3 codes (unsigned byte order = value order, -0 below +0) and back: MaxPool of bytes is
// taken on the key (e4m3 is monotone: the maximum of the bytes is the byte of the maximum)
__device__ __forceinline__ unsigned e4m3_key(unsigned b) { return b ^ ((((b >> 7) & 0x01010101u) * 0xffu) | 0x80808080u); }
__device__ __forceinline__ unsigned e4m3_unkey(unsigned k) { return k ^ ((((~k >> 7) & 0x01010101u) * 0xffu) | 0x80808080u); }
__device__ __forceinline__ unsigned e4m3_max4(unsigned a, unsigned b) {
    unsigned r = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned x = (a >> (8 * e)) & 0xffu, y = (b >> (8 * e)) & 0xffu;
        r |= (x > y ? x : y) << (8 * e);
    }
    return r;
}

// 8 channels of one tile row to one destination in its format: bytes from the byte tile or fp16 from the fp16 tile
__device__ __forceinline__ void put8(void* y, bool f8, long long off, const char* bt, const half_t* ht, int tile_off) {
    if (f8) *(i32x2_t*)((char*)y + off) = *(const i32x2_t*)(bt + tile_off);
    else *(h8_t*)((half_t*)y + off) = *(const h8_t*)(ht + tile_off);
}

// ---------------------------------------------------------------------------------------
// The store of a finished tile (MCAMD_EPI_PAD_F16): ROWS pixels x COLS channels in LDS, rows PITCH elements apart, as
// fp16 (ht) and / or e4m3 bytes (bt), into the padded NHWC destination(s) -- PLAIN, POOL (+ the optional full-resolution
// copy y2) or REORG by a.dst_mode, each destination in its own format (y_f8 / y2_f8: bytes; the fp16 kernels pass
// nullptr, false, false and those branches fold away).  Nothing outside the interior pixels x [choff, choff + N) is
// written.
// ---------------------------------------------------------------------------------------
template <int ROWS, int COLS, int PITCH, int NT>
__device__ __forceinline__ void store_pad_tile(const IgemmArgs& __restrict__ a, const char* bt, const half_t* ht, bool y_f8, bool y2_f8,
                                               int mt, int nt, int tid) {
    constexpr int CH = COLS / 8;   // 8-channel pieces per tile row
    if (a.dst_mode == MCAMD_DST_PLAIN) {
        for (int slot = tid; slot < ROWS * CH; slot += NT) {
            const int row = slot / CH, ch = slot - row * CH;
            const int m = mt * ROWS + row;
            const int n0 = nt * COLS + ch * 8;
            if (m < a.M && n0 < a.N) {
                int b, h, w;
                split_pixel(m, a.HW, a.W, b, h, w);
                put8(a.y, y_f8, pad_off(b, h, w, a.H, a.W, a.y_ld) + a.y_choff + n0, bt, ht, row * PITCH + ch * 8);
            }
        }
        return;
    }
    const int Wo = a.W >> 1, Ho = a.H >> 1, HWo = Ho * Wo;
    if (a.dst_mode == MCAMD_DST_POOL) {
        const bool has2 = a.y2 != nullptr;
        for (int slot = tid; slot < (ROWS / 4) * CH; slot += NT) {
            const int pr = slot / CH, ch = slot - pr * CH;
            const int idx = mt * (ROWS / 4) + pr;   // pooled pixel
            const int n0 = nt * COLS + ch * 8;
            if (4 * idx < a.M && n0 < a.N) {
                int b, ho, wo;
                split_pixel(idx, HWo, Wo, b, ho, wo);
                const long long off = pad_off(b, ho, wo, Ho, Wo, a.y_ld) + a.y_choff + n0;
                if (y_f8) {
                    unsigned k0 = 0, k1 = 0;       // keys >= 0x00: the first window pixel always replaces them
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const i32x2_t v = *(const i32x2_t*)(bt + (4 * pr + q) * PITCH + ch * 8);
                        k0 = e4m3_max4(k0, e4m3_key((unsigned)v[0]));
                        k1 = e4m3_max4(k1, e4m3_key((unsigned)v[1]));
                    }
                    i32x2_t mx;
                    mx[0] = (int)e4m3_unkey(k0), mx[1] = (int)e4m3_unkey(k1);
                    *(i32x2_t*)((char*)a.y + off) = mx;
                } else {
                    h8_t v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = *(const h8_t*)(ht + (4 * pr + q) * PITCH + ch * 8);
                    h8_t mx;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const half_t m01 = v[0][e] > v[1][e] ? v[0][e] : v[1][e], m23 = v[2][e] > v[3][e] ? v[2][e] : v[3][e];
                        mx[e] = m01 > m23 ? m01 : m23;
                    }
                    *(h8_t*)((half_t*)a.y + off) = mx;
                }
                if (has2) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        put8(a.y2, y2_f8, pad_off(b, 2 * ho + (q >> 1), 2 * wo + (q & 1), a.H, a.W, a.y2_ld) + a.y2_choff + n0,
                             bt, ht, (4 * pr + q) * PITCH + ch * 8);
                }
            }
        }
    } else {   // MCAMD_DST_REORG: out channel = (dy * 2 + dx) * N + n at the pooled pixel
        for (int slot = tid; slot < ROWS * CH; slot += NT) {
            const int row = slot / CH, ch = slot - row * CH;
            const int m = mt * ROWS + row;
            const int n0 = nt * COLS + ch * 8;
            if (m < a.M && n0 < a.N) {
                int b, ho, wo;
                split_pixel(m >> 2, HWo, Wo, b, ho, wo);
                put8(a.y, y_f8, pad_off(b, ho, wo, Ho, Wo, a.y_ld) + a.y_choff + (m & 3) * a.N + n0, bt, ht, row * PITCH + ch * 8);
            }
        }
    }
}

// The sibling for MCAMD_EPI_RAW_F16: the fp16 tile [ROWS][COLS] to the raw output [M][y_ld].
template <int ROWS, int COLS, int NT>
__device__ __forceinline__ void store_raw_tile(const IgemmArgs& __restrict__ a, const half_t* ct, int mt, int nt, int tid) {
    constexpr int CH = COLS / 8;   // 16-byte chunks per output row
    half_t* y = (half_t*)a.y;
    for (int slot = tid; slot < ROWS * CH; slot += NT) {
        const int row = slot / CH, ch = slot - row * CH;
        const int m = mt * ROWS + row;
        const int n0 = nt * COLS + ch * 8;
        if (m < a.M && n0 < a.N) *(h8_t*)(y + (long long)m * a.y_ld + a.y_choff + n0) = *(const h8_t*)(ct + row * COLS + ch * 8);
    }
}

// ---------------------------------------------------------------------------------------
// MCAMD_EPI_RAW_F32 of the kernels whose waves hold (WM / 32) x (WN / 32) accumulator blocks of 32 x 32 (igemm_kernel,
// bn_conv1x1_kernel): the unrounded accumulators to fp32 [M][y_ld] -- a store instruction writes two rows x 32
// consecutive floats, whole 128-byte lines straight from the registers -- and the BatchNorm partial sums of the lane's
// column taken from the same fp32 values (rows >= M contribute nothing).
// ---------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void store_raw32_tile(const IgemmArgs& __restrict__ a, const f32x16_t (&acc)[WM / 32][WN / 32], int mt, int nt,
                                                 int wm, int wn, int lane, float (&s1)[WN / 32], float (&s2)[WN / 32]) {
    constexpr int TM = WM / 32, TN = WN / 32;
    float* y = (float*)a.y;
    const int mlim = a.M - mt * BM;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = nt * BN + wn * WN + j * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * WM + i * 32 + mfma32_row(r, lane);
                const float v = acc[i][j][r];
                if (row < mlim) {
                    if (n < a.N) y[(long long)(mt * BM + row) * a.y_ld + a.y_choff + n] = v;
                    s1[j] += v;
                    s2[j] += v * v;
                }
            }
    }
}

// ... and a persistent workgroup's sums to its slab row [2][stats_ld] once its M tiles are done: the two lane halves, then
// the BM / WM wave rows in order (deterministic).  `smem`: (BM / WM) * 2 * BN floats.
template <int BM, int BN, int WM, int WN, int NT>
__device__ __forceinline__ void store_stats_slab(const IgemmArgs& __restrict__ a, char* smem, float (&s1)[WN / 32], float (&s2)[WN / 32],
                                                 int pslot, int nt, int wm, int wn, int lane, int tid) {
    constexpr int TN = WN / 32;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        s1[j] += __shfl_xor(s1[j], 32);
        s2[j] += __shfl_xor(s2[j], 32);
    }
    __syncthreads();
    float* red = (float*)smem;  // [BM/WM][2][BN]
    if (lane < 32) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            red[(wm * 2 + 0) * BN + wn * WN + j * 32 + lane] = s1[j];
            red[(wm * 2 + 1) * BN + wn * WN + j * 32 + lane] = s2[j];
        }
    }
    __syncthreads();
    for (int t = tid; t < 2 * BN; t += NT) {
        int which = t / BN, col = t - which * BN;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < BM / WM; ++k) v += red[(k * 2 + which) * BN + col];
        a.stats[((long long)pslot * 2 + which) * a.stats_ld + nt * BN + col] = v;
    }
}

// ---------------------------------------------------------------------------------------
// BatchNorm + LeakyReLU of one raw value, and the split storage of an activation v: hi = fp16(v) saturated (never inf:
// inf * 0 = NaN downstream), lo = fp16(v - hi) -- exact difference, one rounding; |lo| <= ulp(hi) / 2.  The activation pass
// (bn_act.hip) and the fused 1x1 forward (bn_conv1x1.hip) share these expressions, so they produce the same bits.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float bn_leaky(float y, float sc, float sh, float slope) {
    const float z = y * sc + sh;
    return z > 0.f ? z : z * slope;
}
__device__ __forceinline__ half_t sat_half(float v) {
    return (half_t)fminf(fmaxf(v, -65504.f), 65504.f);
}
__device__ __forceinline__ void split_hi_lo(const float* v, h8_t& hi, h8_t& lo) {
#pragma unroll
    for (int i = 0; i < 8; ++i) hi[i] = sat_half(v[i]);
#pragma unroll
    for (int i = 0; i < 8; ++i) lo[i] = (half_t)(v[i] - (float)hi[i]);
}

// ---------------------------------------------------------------------------------------
// store_raw_tile for a dgrad launch whose output is the gradient G of a PLAIN BatchNorm + LeakyReLU block (a.bsum,
// MCAMD_EPI_RAW_F16_SUMS instances): while the tile goes out, pass 0 of that block's BatchNorm backward
// (bn_plain_bwd_kernel<0, BN_SRC_ACT>, bn_act.hip) is taken on it -- per producer channel sum g_z and sum g_z xhat, from G AS
// STORED (fp16, saturated: what pass 1 reads) and the 16 bytes of the producer's stored activation at the same pixel and
// channels.  Same element formulas, same ill-conditioned-channel rule (act_xhat_source: only threads that hold such a
// channel read the saved fp32 y).  Rows >= M and columns outside [ch_lo, ch_lo + C) contribute nothing.
//
// NT % (COLS / 8) == 0: a thread keeps the same 8 channels for all its slots, so the hoisted per-channel values are
// computed once per tile, and its pixels advance by NT / CH rows (stepped, no division per slot).  The threads' partials
// are reduced over the NT / CH threads that share a channel through LDS in a fixed order (layout of
// block_partials_to_slab, bn_act.hip) into tot[]: ONE register per thread and value (2 COLS values on NT threads) lives
// across the K loops of a persistent slot's M tiles; store_tile_sums_slab writes it to the slot's slab row at the end.  No
// atomics: the sums do not depend on scheduling.
//
// The coefficient pointers are taken through an empty volatile asm: inlined without it, hipcc hoists the coefficient
// loads and the address arithmetic above the K loop and every instance goes over its register budget.
// `smem`: the tile ct = [ROWS][COLS] fp16 at its start; at least 16 (NT + 8) floats long (sums_lds_bytes).
// ---------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ const T* pin_here(const T* p) {
    asm volatile("" : "+s"(p));
    return p;
}
__host__ __device__ constexpr int sums_vals(int cols, int nt) { return (2 * cols + nt - 1) / nt; }
__host__ __device__ constexpr size_t sums_lds_bytes(int nt) { return (size_t)16 * (nt + 8) * sizeof(float); }

__host__ __device__ constexpr int sums_slots(int rows, int cols, int nt) { return rows * (cols / 8) / nt; }
// ... of which this many are fetched early: all, except in the 256 x 256 ping-pong tile, whose 128 accumulator registers
// leave room for 8 of its 16 pieces (all 16: 192 bytes of scratch per lane)
__host__ __device__ constexpr int sums_early(int rows, int cols, int nt) {
    return rows * cols >= 256 * 256 && sums_slots(rows, cols, nt) > 8 ? 8 : sums_slots(rows, cols, nt);
}

// Step 1, BEFORE the accumulators go to LDS: the thread's activation pieces of the tile, all in flight while the tile is
// transposed (issued slot by slot next to the stores they cost about what the pass they replace cost: the early 1x1 dgrads
// are store-bound and the ping-pong dgrads run one tile per CU with nothing else to hide a load behind).
template <int ROWS, int COLS, int NT>
__device__ __forceinline__ void sums_prefetch(const IgemmArgs& __restrict__ a, int mt, int nt, int tid,
                                              h8_t (&aq)[sums_early(ROWS, COLS, NT)]) {
    constexpr int CH = COLS / 8, RSTEP = NT / CH, NSLOT = sums_early(ROWS, COLS, NT);
    static_assert(NT % CH == 0 && (ROWS * CH) % NT == 0, "a thread keeps its 8 channels for all its slots");
    const int ch = tid % CH, row0 = tid / CH;
    const int n0 = nt * COLS + ch * 8;
    const int c = n0 - a.bsum.ch_lo;                        // producer channel of this thread's first column
    const bool live = n0 < a.N && c >= 0 && c < a.bsum.C;   // (ch_lo and C are multiples of 8: all 8 channels or none)
    const half_t* act = pin_here(a.bsum.act) + a.bsum.act_choff + c;
    // pixel of this thread's first row, and the step of RSTEP rows (no division per slot)
    int m = mt * ROWS + row0;
    int b, h, w;
    split_pixel(m, a.HW, a.W, b, h, w);
    const int sb_ = RSTEP / a.HW, srem = RSTEP - sb_ * a.HW;
    const int sh_ = srem / a.W, sw_ = srem - sh_ * a.W;
#pragma unroll
    for (int k = 0; k < NSLOT; ++k) {
#pragma unroll
        for (int i = 0; i < 8; ++i) aq[k][i] = (half_t)0.f;
        if (live && m < a.M) aq[k] = *(const h8_t*)(act + pad_off(b, h, w, a.H, a.W, a.bsum.act_ld, a.bsum.act_pw));
        m += RSTEP;
        w += sw_;
        if (w >= a.W) w -= a.W, ++h;
        h += sh_;
        if (h >= a.H) h -= a.H, ++b;
        b += sb_;
    }
}

// Step 2, with the tile in LDS: store it and accumulate.
template <int ROWS, int COLS, int NT>
__device__ __forceinline__ void store_raw_tile_sums(const IgemmArgs& __restrict__ a, char* smem, int mt, int nt, int tid,
                                                    const h8_t (&aq)[sums_early(ROWS, COLS, NT)],
                                                    float (&tot)[sums_vals(COLS, NT)]) {
    constexpr int CH = COLS / 8, RSTEP = NT / CH, NSLOT = sums_slots(ROWS, COLS, NT), PITCH = NT + 8;
    constexpr int EARLY = sums_early(ROWS, COLS, NT);
    const half_t* ct = (const half_t*)smem;
    half_t* y = (half_t*)a.y;
    const int ch = tid % CH, row0 = tid / CH;
    const int n0 = nt * COLS + ch * 8;
    const int c = n0 - a.bsum.ch_lo;
    const bool col_ok = n0 < a.N;
    const bool live = col_ok && c >= 0 && c < a.bsum.C;
    float sb[8], sg[8], off[8], mul[8];
    bool usey[8];
    bool need_y = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) sb[i] = sg[i] = 0.f, off[i] = 0.f, mul[i] = 0.f, usey[i] = false;
    if (live) {
        const float *scp = pin_here(a.bsum.scale) + c, *shp = pin_here(a.bsum.shift) + c;
        const float *mup = pin_here(a.bsum.mean) + c, *isp = pin_here(a.bsum.invstd) + c;
        float sc[8], sh[8], mu[8], is[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) sc[i] = scp[i], sh[i] = shp[i], mu[i] = mup[i], is[i] = isp[i];
        need_y = act_xhat_source(sc, sh, mu, is, a.bsum.y != nullptr, off, mul, usey);
    }
    const float slope = a.bsum.slope, inv_slope = 1.0f / slope;
#pragma unroll
    for (int k = 0; k < NSLOT; ++k) {
        const int row = row0 + k * RSTEP, m = mt * ROWS + row;
        if (!col_ok || m >= a.M) continue;
        const h8_t gq = *(const h8_t*)(ct + row * COLS + ch * 8);
        *(h8_t*)(y + (long long)m * a.y_ld + a.y_choff + n0) = gq;
        if (!live) continue;
        h8_t av8;
        if (k < EARLY) {
            av8 = aq[k];
        } else {   // (the late pieces of the 256 x 256 tile)
            int b, h, w;
            split_pixel(m, a.HW, a.W, b, h, w);
            av8 = *(const h8_t*)(a.bsum.act + pad_off(b, h, w, a.H, a.W, a.bsum.act_ld, a.bsum.act_pw) + a.bsum.act_choff + c);
        }
        float z[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float av = (float)av8[i];
            z[i] = av > 0.f ? av : av * inv_slope;
        }
        if (need_y) {                                // ill-conditioned channels: the saved y in place of z
            const float* yp = a.bsum.y + (long long)m * a.bsum.y_ld + a.bsum.y_choff + c;
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = usey[i] ? yp[i] : z[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float gv = (float)gq[i];
            const float gz = (float)av8[i] > 0.f ? gv : gv * slope;
            sb[i] += gz;
            sg[i] += gz * ((z[i] - off[i]) * mul[i]);
        }
    }
    __syncthreads();   // every thread is done with the tile: its LDS takes the partials, [16 values][NT threads]
    float* red = (float*)smem;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        red[i * PITCH + tid] = sb[i];
        red[(8 + i) * PITCH + tid] = sg[i];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < sums_vals(COLS, NT); ++k) {
        const int t = tid + k * NT;
        if (t < 2 * COLS) {
            const int which = t / COLS, col = t - which * COLS;
            const int v = which * 8 + (col & 7), chq = col >> 3;
            float s = 0.f;
            for (int r = 0; r < RSTEP; ++r) s += red[v * PITCH + r * CH + chq];   // the threads r CH + chq, in order
            tot[k] += s;
        }
    }
    // (the next tile's K loop, or nothing that touches LDS, follows behind the kernels' own barrier)
}

// ... and the slot's sums to its slab row [2][ld] once its M tiles are done
template <int COLS, int NT>
__device__ __forceinline__ void store_tile_sums_slab(const IgemmArgs& __restrict__ a, int pslot, int nt, int tid,
                                                     const float (&tot)[sums_vals(COLS, NT)]) {
#pragma unroll
    for (int k = 0; k < sums_vals(COLS, NT); ++k) {
        const int t = tid + k * NT;
        if (t < 2 * COLS) {
            const int which = t / COLS, col = t - which * COLS;
            const int n = nt * COLS + col, c = n - a.bsum.ch_lo;
            if (n < a.N && c >= 0 && c < a.bsum.C) a.bsum.slab[((long long)pslot * 2 + which) * a.bsum.ld + c] = tot[k];
        }
    }
}

// ---------------------------------------------------------------------------------------
// Accumulators -> LDS tile of the weights-as-A kernels (conv_sparse.hip, conv_q8.hip): there the rows of a 32x32 block
// are output channels and the columns pixels, so a lane's accumulator rows 4 g .. 4 g + 3 are four consecutive channels
// of one pixel.  leaky(acc * scale_of(n) + shift[n]) goes down as [pixel][channel], rows PITCH elements apart, as e4m3(2 v)
// bytes (need_b) and / or saturated fp16 (need_h).  Returns whether an fp16 value was clamped.
//
// BorderOf (slim models; NoBorder: none, the code below is what it was): a per-pixel-class constant joins the
// raw value in front of the affine step, leaky((acc * pre(n) + table[cls][n]) * scale_of(n) + shift[n]) -- pre(n) = the
// power of two that scale_of(n) carries for the other kernels.  The class of an accumulator column is taken ONCE per
// column (TN registers), from the pixel the launch's enumeration gives it (tile_pixel: each pixel of a POOL / REORG
// window has its own); a lane then reads one 16-byte table piece per (pixel, four channels).
// ---------------------------------------------------------------------------------------
struct NoBorder {
    static constexpr bool on = false;
};
// table: fp32 [16][ld], class bits: 0 top row, 1 bottom row, 2 left column, 3 right column (bn_act.hip border_class);
// wexp: the per-filter exponents of the packed fp8 weights; m0: GEMM row (pixel) of the tile's first column
struct Q8Border {
    static constexpr bool on = true;
    const float* table;
    const int* wexp;
    int ld, m0;
    __device__ __forceinline__ int cls(const IgemmArgs& __restrict__ a, int pix) const {
        int m = m0 + pix, b, h, w;
        if (m > a.M - 1) m = a.M - 1;              // (columns past the last pixel are not stored)
        tile_pixel(a, a.dst_mode != 0, m, b, h, w);
        return (h == 0 ? 1 : 0) | (h == a.H - 1 ? 2 : 0) | (w == 0 ? 4 : 0) | (w == a.W - 1 ? 8 : 0);
    }
    __device__ __forceinline__ float pre(int n) const { return ldexpf(1.f, -(wexp[n] + 1)); }
    __device__ __forceinline__ f32x4_t row(int c, int n0) const { return *(const f32x4_t*)(table + c * ld + n0); }
};

template <int BMW, int PITCH, int WM, int WN, int TM, int TN, class ScaleOf, class BorderOf = NoBorder>
__device__ __forceinline__ bool write_ch_tile(const IgemmArgs& __restrict__ a, const f32x16_t (&acc)[TM][TN], ScaleOf scale_of, bool need_b,
                                              bool need_h, char* bt, half_t* ht, int nt, int wm, int wn, int lane,
                                              BorderOf border_of = BorderOf()) {
    bool sat = false;
    int cls[BorderOf::on ? TN : 1];
    if constexpr (BorderOf::on) {
#pragma unroll
        for (int j = 0; j < TN; ++j) cls[j] = border_of.cls(a, wn * WN + j * 32 + (lane & 31));
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch0 = wm * WM + i * 32 + 8 * g + 4 * (lane >> 5);
            float sc[4], sh[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = nt * BMW + ch0 + e;
                sc[e] = 1.f, sh[e] = 0.f;
                if (n < a.N) {
                    sc[e] = scale_of(n);
                    if (a.shift) sh[e] = a.shift[n];
                }
            }
            float pre[BorderOf::on ? 4 : 1];
            if constexpr (BorderOf::on) {
#pragma unroll
                for (int e = 0; e < 4; ++e) pre[e] = nt * BMW + ch0 + e < a.N ? border_of.pre(nt * BMW + ch0 + e) : 1.f;
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int pix = wn * WN + j * 32 + (lane & 31);
                float v[4];
                if constexpr (BorderOf::on) {
                    f32x4_t bb = {0.f, 0.f, 0.f, 0.f};
                    if (nt * BMW + ch0 < a.N) bb = border_of.row(cls[j], nt * BMW + ch0);   // (N % 4 == 0: all four or none)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (acc[i][j][4 * g + e] * pre[e] + bb[e]) * sc[e] + sh[e];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e] * sc[e] + sh[e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * a.slope;
                if (need_b) *(int*)(bt + pix * PITCH + ch0) = e4m3_bytes4(v);
                if (need_h) {
                    h4_t hv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        sat |= fabsf(v[e]) > 65504.f;
                        hv[e] = (half_t)fminf(fmaxf(v[e], -65504.f), 65504.f);   // saturate, never inf
                    }
                    *(h4_t*)(ht + pix * PITCH + ch0) = hv;
                }
            }
        }
    }
    return sat;
}

// ---------------------------------------------------------------------------------------
// MCAMD_EPI_RAW_F32 of the byte weights-as-A kernels (conv_q8.hip, conv_q8_w4.hip; training): y[m][n] =
// 2^-(wexp[n] + 1) * acc as fp32 [M][y_ld] (the power of two is exact) plus, with a.stats, per channel the sum and the sum of
// squares of those fp32 values over the workgroup's pixel tile: slab row = the pixel tile mt, every row written, fixed order,
// no atomics.  Each wave transposes its accumulators through a private LDS region, 32 pixels at a time ([pixel][channel], rows
// WM + 4 floats apart: the 16-byte writes of 8 pixels fall on 8 different bank slots), stores whole channel runs and adds the
// 32 rows of a column in order; pixels past M go down as zeros and are not stored.  Every wave of the workgroup calls it, behind
// a barrier that ends the K loop's use of `smem`, of which it uses the first raw32_ch_lds_bytes().
// ---------------------------------------------------------------------------------------
__host__ __device__ constexpr int raw32_ch_lds_bytes(int bmw, int bnp, int wm, int wn) {
    return (bmw / wm) * (bnp / wn) * 32 * (wm + 4) * 4 + (bnp / wn) * bmw * 2 * 4;
}

template <int BMW, int BNP, int WM, int WN, int TM, int TN>
__device__ __forceinline__ void store_raw32_ch_tile(const IgemmArgs& __restrict__ a, const f32x16_t (&acc)[TM][TN],
                                                    const int* __restrict__ wexp, char* smem, int mt, int nt, int wm, int wn, int wave,
                                                    int lane, int tid) {
    constexpr int WAVES_N = BNP / WN, NWAVES = (BMW / WM) * WAVES_N;
    constexpr int PF = WM + 4, C4 = WM / 4;    // floats between the pixel rows of a wave's region; float4 pieces per row
    constexpr int REGION = 32 * PF;            // floats per wave
    float* tile = (float*)smem + wave * REGION;
    float* comb = (float*)smem + NWAVES * REGION;             // [WAVES_N][BMW][2] partial sums of the pixel waves
    float* y = (float*)a.y;
    float s1 = 0.f, s2 = 0.f;                  // lane c < WM: channel wm * WM + c over this wave's WN pixels
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int m0 = mt * BNP + wn * WN + j * 32;
        const bool live = m0 + (lane & 31) < a.M;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch0 = i * 32 + 8 * g + 4 * (lane >> 5);
                f32x4_t v;
#pragma unroll
                for (int e = 0; e < 4; ++e)    // (rows up to Npad = round_up(N, 256) exist: zero bytes, exponent 0)
                    v[e] = live ? ldexpf(acc[i][j][4 * g + e], -(wexp[nt * BMW + wm * WM + ch0 + e] + 1)) : 0.f;
                *(f32x4_t*)(tile + (lane & 31) * PF + ch0) = v;
            }
        __syncthreads();
        for (int slot = lane; slot < 32 * C4; slot += 64) {
            const int row = slot / C4, c4 = slot - row * C4;
            const int m = m0 + row, n0 = nt * BMW + wm * WM + c4 * 4;
            if (m < a.M && n0 < a.N) *(f32x4_t*)(y + (long long)m * a.y_ld + a.y_choff + n0) = *(const f32x4_t*)(tile + row * PF + c4 * 4);
        }
        if (a.stats && lane < WM) {
#pragma unroll 8
            for (int p = 0; p < 32; ++p) {
                const float v = tile[p * PF + lane];
                s1 += v;
                s2 += v * v;
            }
        }
        __syncthreads();
    }
    if (a.stats) {                             // (wave-uniform)
        if (lane < WM) {
            comb[(wn * BMW + wm * WM + lane) * 2] = s1;
            comb[(wn * BMW + wm * WM + lane) * 2 + 1] = s2;
        }
        __syncthreads();
        if (tid < BMW) {
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int k = 0; k < WAVES_N; ++k) {
                t1 += comb[(k * BMW + tid) * 2];
                t2 += comb[(k * BMW + tid) * 2 + 1];
            }
            // channels in [N, round_up(N, BMW)) come out as zeros: stats_ld >= round_up(N, 256) holds them
            a.stats[((long long)mt * 2 + 0) * a.stats_ld + nt * BMW + tid] = t1;
            a.stats[((long long)mt * 2 + 1) * a.stats_ld + nt * BMW + tid] = t2;
        }
    }
}
