// BatchNorm2d + LeakyReLU + MaxPool2d(2,2) / Reorg(2) / route, fused around the conv kernels.
// HBM-bound streaming kernels: 16 bytes (8 fp16 channels) per lane, channel-fastest thread
// mapping so every wave touches whole contiguous pixel rows.
//
// Reference ops replaced: nn.BatchNorm2d (nets.py:802, torch defaults eps 1e-5 / momentum 0.1),
// nn.LeakyReLU(0.1) (nets.py:809), nn.MaxPool2d(2,2) (nets.py:821), Reorg (nets.py:648-667),
// torch.cat route (nets.py:738-746), and their autograd backward.
#include "common.h"
#include "conv_epi.h"   // e4m3_bytes4 / q8_to_f16: the byte destinations of the fp8 quantisation-aware training blocks

// ------------------------------------------------------------------------------------
// batch statistics -> affine coefficients
// ------------------------------------------------------------------------------------
// Slab reductions.  One block per 8 channels (the early layers have 32-64 channels and up to 2048 slab rows: a
// block per 32 channels was one or two CUs reading 0.5 MB each, 25-29 us), 128 row groups x 8 channels per block:
// rows are summed in double per thread, then over the 8 row groups of a wave by shuffles, then over the 16 waves
// through LDS -- a fixed order, so the result does not depend on scheduling.
constexpr int RED_CPB = 8, RED_RG = 128;

__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, m);
    hi = __shfl_xor(hi, m);
    return __hiloint2double(hi, lo);
}

// returns (for threads of wave 0 .. any) the block total in threads with ry == 0: call from all 1024 threads
__device__ __forceinline__ void block_reduce2(double& a, double& b, double (*red)[16][RED_CPB]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cx = threadIdx.x & (RED_CPB - 1);
#pragma unroll
    for (int m = RED_CPB; m < 64; m <<= 1) {   // lanes cx, cx+8, ..., cx+56 hold the same channel
        a += shfl_xor_f64(a, m);
        b += shfl_xor_f64(b, m);
    }
    if (lane < RED_CPB) {
        red[0][wave][cx] = a;
        red[1][wave][cx] = b;
    }
    __syncthreads();
    if (threadIdx.x < RED_CPB) {
        a = b = 0.0;
        for (int w = 0; w < 16; ++w) {
            a += red[0][w][cx];
            b += red[1][w][cx];
        }
    }
}

__global__ __launch_bounds__(1024) void bn_coeffs_kernel(const float* stats, int rows, int ld, int C, double count,
                                                         const float* gamma, const float* beta, float* rmean,
                                                         float* rvar, float momentum, float eps, int training,
                                                         float* scale, float* shift, float* save_mean,
                                                         float* save_invstd, const int* perm, int ones_channel) {
    __shared__ double red[2][16][RED_CPB];
    const int cx = threadIdx.x & (RED_CPB - 1), ry = threadIdx.x / RED_CPB;
    const int c = blockIdx.x * RED_CPB + cx;
    double s1 = 0.0, s2 = 0.0;
    if (training && c < C) {
        for (int p = ry; p < rows; p += RED_RG) {
            s1 += (double)stats[((long long)p * 2 + 0) * ld + c];
            s2 += (double)stats[((long long)p * 2 + 1) * ld + c];
        }
    }
    block_reduce2(s1, s2, red);
    if (ry != 0 || c >= C) return;
    // `perm` (optional): the statistics / coefficient vectors are in the kernels' PHYSICAL channel order
    // (kept filters first, engine.py filter compaction); the module's parameter vectors are in the
    // reference's order.  pc = this physical channel's index into gamma/beta/running_*.
    const int pc = perm ? perm[c] : c;
    double mean, var;
    if (training) {
        mean = s1 / count;
        var = s2 / count - mean * mean;  // biased variance (normalisation)
        if (var < 0.0) var = 0.0;
        double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        rmean[pc] = (float)((1.0 - momentum) * (double)rmean[pc] + (double)momentum * mean);
        rvar[pc] = (float)((1.0 - momentum) * (double)rvar[pc] + (double)momentum * unbiased);
    } else {
        mean = rmean[pc];
        var = rvar[pc];
    }
    double invstd = 1.0 / sqrt(var + (double)eps);
    float sc = (float)((double)gamma[pc] * invstd);
    scale[c] = sc;
    shift[c] = (float)((double)beta[pc] - mean * (double)sc);
    if (c == ones_channel) scale[c] = 0.f, shift[c] = 1.f;      // the activation pass writes ones here (fold.hip)
    if (save_mean) save_mean[c] = (float)mean;
    if (save_invstd) save_invstd[c] = (float)invstd;
}

// ------------------------------------------------------------------------------------
// forward: y(raw fp16) -> leaky(y*scale+shift) -> {plain | 2x2 max pool | reorg} -> padded NHWC
// ------------------------------------------------------------------------------------
struct ActArgs {
    const void* y;       // fp16 or fp32 (template parameter Y32) raw conv output
    const float* scale;
    const float* shift;
    half_t* dst;
    half_t* dst2;
    int B, H, W, C;
    int y_ld, y_choff, dst_ld, dst_choff, dst2_ld, dst2_choff;
    float slope;
    long long items;
    const float* border;  // optional [16][C]: added to the raw conv output by border class (slim models)
    int dst_plane, dst2_plane;  // plane strides of the split (hi | lo | hi) storage, PL == 3
    int dst_pw, dst2_pw;        // halo pixels per row / rows per image of dst, dst2: 2 (padded form) or 1 (shared-halo form)
    int dst2_pl;                // storage form of dst2 (mcamd_act_desc.planes2)
    half_t* pool_act;           // optional (pool): full-resolution fp16 activation for the backward pass (mcamd_act_desc.pool_act)
    int pool_act_ld, pool_act_pw;
    char* dst_q8;               // optional (kernel form Q8): BYTE twins of dst / dst2, same geometry (mcamd_act_desc.dst_q8)
    char* dst2_q8;
};

__device__ __forceinline__ void load8(const half_t* p, float* v) {
    h8_t h = *(const h8_t*)p;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
}
// (sat_half, bn_leaky, split_hi_lo: conv_epi.h -- shared with the fused 1x1 forward, bn_conv1x1.hip)
__device__ __forceinline__ void store8(half_t* p, const float* v) {
    h8_t h;
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = sat_half(v[i]);
    *(h8_t*)p = h;
}
__device__ __forceinline__ void loadf8(const float* p, float* v) {
    f32x4_t a = *(const f32x4_t*)p, b = *(const f32x4_t*)(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = a[i];
        v[4 + i] = b[i];
    }
}
// raw conv output, fp16 or fp32 storage
template <bool Y32>
__device__ __forceinline__ void load_y(const void* y, long long idx, float* v) {
    if (Y32) loadf8((const float*)y + idx, v);
    else load8((const half_t*)y + idx, v);
}
// activation store: one fp16 plane, or the split form of the "fp16x3" precision mode (include/mcamd.h,
// mcamd_act_desc.planes): hi = fp16(v), lo = fp16(v - hi), and hi again, `plane` channels apart
// PL == 4 (round 4): hi = fp16(v) and, `plane` fp16 units further, the e4m3 correction bytes of the consumer with
// mcamd_conv_geom.x_f8: [lo8 = e4m3((v - hi) * 2^12) : plane bytes | x8 = e4m3(v * 2) : plane bytes] (common.h); `ci` =
// channel of v[0] in the buffer (the consumer's slice starts at channel 0: a concat member writes at its offset inside the
// e4m3 strings too).  The conversion instruction returns NaN above 448: clamped first.
template <int PL>
__device__ __forceinline__ void store_act(half_t* p, int plane, const float* v, int ci = 0) {
    h8_t hi, lo;
    split_hi_lo(v, hi, lo);
    *(h8_t*)p = hi;
    if (PL == 4) {
        float ql[8], q8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ql[i] = fminf(fmaxf((v[i] - (float)hi[i]) * (float)(1 << MCAMD_F8_SXL), -448.f), 448.f);
            q8[i] = fminf(fmaxf(v[i] * (float)(1 << MCAMD_F8_SX8), -448.f), 448.f);
        }
        int wl[2], w8[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            wl[i] = __builtin_amdgcn_cvt_pk_fp8_f32(ql[4 * i], ql[4 * i + 1], 0, false);
            wl[i] = __builtin_amdgcn_cvt_pk_fp8_f32(ql[4 * i + 2], ql[4 * i + 3], wl[i], true);
            w8[i] = __builtin_amdgcn_cvt_pk_fp8_f32(q8[4 * i], q8[4 * i + 1], 0, false);
            w8[i] = __builtin_amdgcn_cvt_pk_fp8_f32(q8[4 * i + 2], q8[4 * i + 3], w8[i], true);
        }
        char* b = (char*)(p - ci + plane) + ci;      // byte ci of the e4m3 region
        typedef int i32x2_t __attribute__((ext_vector_type(2)));
        *(i32x2_t*)b = i32x2_t{wl[0], wl[1]};
        *(i32x2_t*)(b + plane) = i32x2_t{w8[0], w8[1]};
    } else if (PL >= 2) {
        *(h8_t*)(p + plane) = lo;
        if (PL == 3) *(h8_t*)(p + 2 * plane) = hi;      // (PL == 2: the consumer wraps its third K part onto the hi plane)
    }
}
// One destination of an fp8 quantisation-aware training block (mcamd_act_desc.dst_q8): with a byte twin `q`
// of the buffer, the codes e4m3(2 v) -- one rounding from fp32 -- go there and the fp16 buffer receives their values / 2
// (exact in fp16), so that the backward pass multiplies what the consumer's forward multiplied; without one, fp16(v).
__device__ __forceinline__ void store_act_q8(half_t* p, char* q, long long off, const float* v) {
    if (!q) {
        store_act<1>(p + off, 0, v);
        return;
    }
    i32x2_t o;
    o[0] = e4m3_bytes4(v), o[1] = e4m3_bytes4(v + 4);
    *(i32x2_t*)(q + off) = o;
    h8_t h = q8_to_f16(o[0], o[1]);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = h[i] * (half_t)0.5f;
    *(h8_t*)(p + off) = h;
}
// the largest fp16 value below h (bit pattern; h finite, not the most negative value)
__device__ __forceinline__ unsigned short half_prev_bits(unsigned short b) {
    if (b == 0x0000 || b == 0x8000) return 0x8001;          // +-0 -> the smallest negative subnormal
    return (b & 0x8000) ? (unsigned short)(b + 1) : (unsigned short)(b - 1);
}
// dst2 may be stored in another form than dst (its consumer is another convolution): wave-uniform switch
template <int PL>
__device__ __forceinline__ void store_act2(int pl2, half_t* p, int plane, const float* v, int ci) {
    if (PL < 2 || pl2 == PL) store_act<PL>(p, plane, v, ci);
    else if (pl2 == 4) store_act<4>(p, plane, v, ci);
    else if (pl2 == 3) store_act<3>(p, plane, v, ci);
    else if (pl2 == 2) store_act<2>(p, plane, v, ci);
    else store_act<1>(p, plane, v, ci);
}

// Border class of pixel (h, w): which 3x3 taps fall into the zero padding (bit 0 top, 1 bottom, 2 left, 3 right).
__device__ __forceinline__ int border_class(int h, int w, int H, int W) {
    return (h == 0 ? 1 : 0) | (h == H - 1 ? 2 : 0) | (w == 0 ? 4 : 0) | (w == W - 1 ? 8 : 0);
}

// FIXED: C/8 divides 256, so a thread keeps one channel group for the whole grid-stride loop and its BN
// coefficients stay in registers.  !FIXED: any C % 8 == 0 (slim models), coefficients re-read per item (L1/L2 hits).
// Q8 (fp32 y, one plane): the destinations may have byte twins (store_act_q8).
template <int MODE, bool FIXED, bool Y32, int PL, bool Q8 = false>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(ActArgs a) {
    const int CH = a.C >> 3;
    int c8 = (threadIdx.x % CH) * 8;
    float sc[8], sh[8];
    if (FIXED) {
        loadf8(a.scale + c8, sc);
        loadf8(a.shift + c8, sh);
    }
    const int Ho = a.H >> 1, Wo = a.W >> 1;
    for (long long item = (long long)blockIdx.x * 256 + threadIdx.x; item < a.items; item += (long long)gridDim.x * 256) {
        long long pix = item / CH;
        if (!FIXED) {
            c8 = (int)(item - pix * CH) * 8;
            loadf8(a.scale + c8, sc);
            loadf8(a.shift + c8, sh);
        }
        if (MODE == MCAMD_DST_PLAIN) {
            int b = (int)(pix / (a.H * a.W));
            int rem = (int)(pix - (long long)b * a.H * a.W);
            int h = rem / a.W, w = rem - h * a.W;
            float v[8];
            load_y<Y32>(a.y, pix * a.y_ld + a.y_choff + c8, v);
            if (a.border) {
                float bb[8];
                loadf8(a.border + border_class(h, w, a.H, a.W) * a.C + c8, bb);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] += bb[i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = bn_leaky(v[i], sc[i], sh[i], a.slope);
            if (Q8) store_act_q8(a.dst, a.dst_q8, pad_off(b, h, w, a.H, a.W, a.dst_ld, a.dst_pw) + a.dst_choff + c8, v);
            else store_act<PL>(a.dst + pad_off(b, h, w, a.H, a.W, a.dst_ld, a.dst_pw) + a.dst_choff + c8, a.dst_plane, v, a.dst_choff + c8);
        } else {
            int b = (int)(pix / (Ho * Wo));
            int rem = (int)(pix - (long long)b * Ho * Wo);
            int ho = rem / Wo, wo = rem - ho * Wo;
            float act[4][8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int h = 2 * ho + (k >> 1), w = 2 * wo + (k & 1);
                long long sp = ((long long)b * a.H + h) * a.W + w;
                load_y<Y32>(a.y, sp * a.y_ld + a.y_choff + c8, act[k]);
                if (a.border) {
                    float bb[8];
                    loadf8(a.border + border_class(h, w, a.H, a.W) * a.C + c8, bb);
#pragma unroll
                    for (int i = 0; i < 8; ++i) act[k][i] += bb[i];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) act[k][i] = bn_leaky(act[k][i], sc[i], sh[i], a.slope);
                if (Q8) {
                    if (a.dst2) store_act_q8(a.dst2, a.dst2_q8, pad_off(b, h, w, a.H, a.W, a.dst2_ld, a.dst2_pw) + a.dst2_choff + c8, act[k]);
                } else if (a.dst2) store_act2<PL>(a.dst2_pl, a.dst2 + pad_off(b, h, w, a.H, a.W, a.dst2_ld, a.dst2_pw) + a.dst2_choff + c8, a.dst2_plane, act[k], a.dst2_choff + c8);
            }
            long long dp = pad_off(b, ho, wo, Ho, Wo, a.dst_ld, a.dst_pw) + a.dst_choff;
            if (MODE == MCAMD_DST_POOL) {
                float m[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) m[i] = fmaxf(fmaxf(act[0][i], act[1][i]), fmaxf(act[2][i], act[3][i]));
                if (Q8) store_act_q8(a.dst, a.dst_q8, dp + c8, m);      // e4m3 of the window maximum
                else store_act<PL>(a.dst + dp + c8, a.dst_plane, m, a.dst_choff + c8);
                if (!Q8 && a.pool_act) {
                    // the four activations rounded to fp16, with the window's argmax (first maximum of the UNROUNDED values,
                    // what was just pooled) as their strict maximum: a neighbour that rounds to the same fp16 value is stored
                    // one step lower, so the backward pass finds the argmax the forward pass took from the stored values alone
                    typedef unsigned short us8_t __attribute__((ext_vector_type(8)));
                    us8_t hb[4];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        int arg = 0;
                        float best = act[0][i];
#pragma unroll
                        for (int k = 1; k < 4; ++k) {
                            const bool gt = act[k][i] > best;
                            best = gt ? act[k][i] : best, arg = gt ? k : arg;
                        }
                        const unsigned short top = __builtin_bit_cast(unsigned short, sat_half(best));
                        const unsigned short below = half_prev_bits(top);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const unsigned short hk = __builtin_bit_cast(unsigned short, sat_half(act[k][i]));
                            hb[k][i] = (k != arg && hk == top) ? below : hk;
                        }
                    }
                    half_t* q0 = a.pool_act + pad_off(b, 2 * ho, 2 * wo, a.H, a.W, a.pool_act_ld, a.pool_act_pw) + c8;
                    const long long qrow = (long long)(a.W + a.pool_act_pw) * a.pool_act_ld;
                    *(us8_t*)q0 = hb[0];
                    *(us8_t*)(q0 + a.pool_act_ld) = hb[1];
                    *(us8_t*)(q0 + qrow) = hb[2];
                    *(us8_t*)(q0 + qrow + a.pool_act_ld) = hb[3];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (Q8) store_act_q8(a.dst, a.dst_q8, dp + k * a.C + c8, act[k]);
                    else store_act<PL>(a.dst + dp + k * a.C + c8, a.dst_plane, act[k], a.dst_choff + k * a.C + c8);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------
struct ActBwdArgs {
    const void* y;       // fp16 or fp32 (template parameter Y32) saved raw conv output
    const float* scale;
    const float* shift;
    const float* mean;
    const float* invstd;
    const half_t* g;
    const half_t* g2;
    half_t* dy;
    float* slab;         // [nblocks][2][C]
    const float* coef;   // [2][C]: c1 = sum(gz)/count, c2 = sum(gz*xhat)/count
    const float* dy_keep;  // optional [C]: 0 for fully pruned filters (their dY is not needed and is zeroed)
    int* overflow;         // optional: set to 1 when a dY value was clamped to +-65504
    int B, H, W, C;
    int y_ld, y_choff, g_ld, g_choff, g2_ld, g2_choff, dy_ld, dy_choff;
    float slope;
    long long items;
    int dy_pw;             // 2: dy in the padded form, 1: shared-halo form
    const half_t* act;     // optional (source BN_SRC_ACT): the block's stored activation, padded NHWC fp16
    int act_ld, act_choff, act_pw;
    const half_t* pool_out;  // optional (bn_pool_sums_kernel): the block's POOLED activation, padded NHWC fp16 at H/2 x W/2
    int pool_out_ld, pool_out_choff, pool_out_pw;
};

// PHASE 0: per-channel sums of g_z and g_z*xhat -> slab.  PHASE 1: dy -> padded NHWC.
// Pass 0 of the BatchNorm backward kernels: every thread holds partial sums sb[8] / sg[8] of its 8 channels; threads t and
// t + CH (+ 2 CH ...) hold the same channel group.  The block's sums go to slab rows (2 block, 2 block + 1) in a fixed
// order (deterministic).  LDS scratch [16 values][256 threads] with a row pitch of 264 floats: writes are lane-consecutive
// and the reads of 64 consecutive channels (8 groups x 8 values) hit 64 distinct banks ((8 value + group) mod 64).  The
// layout of rounds 1-2, red[thread][16], put the 64 lanes of a store on 4 banks: SQ_LDS_BANK_CONFLICT 443 M cycles per 16
// launches of bn_plain_bwd_kernel<0>, the largest count in the profile (profiles/r02c_pmc_per_kernel.json); the slab
// stores were 4-byte pieces at a 32-byte stride and are whole lines now.
__device__ __forceinline__ void block_partials_to_slab(const float (&sb)[8], const float (&sg)[8], int CH, float* slab, int C) {
    constexpr int PITCH = 264;
    __shared__ float red[16 * PITCH];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        red[i * PITCH + threadIdx.x] = sb[i];
        red[(8 + i) * PITCH + threadIdx.x] = sg[i];
    }
    __syncthreads();
    const int reps = 256 / CH;
    for (int o = threadIdx.x; o < 16 * CH; o += 256) {
        const int which = o / (8 * CH), c = o - which * 8 * CH;      // c = channel inside the block's C = 8 CH channels
        const int ch = c >> 3, v = which * 8 + (c & 7);
        float s = 0.f;
        for (int k = 0; k < reps; ++k) s += red[v * PITCH + k * CH + ch];
        slab[((long long)blockIdx.x * 2 + which) * C + c] = s;
    }
}

// The end of every backward kernel: pass 1 reports a clamped dY, pass 0 hands the thread's sums to the slab.
template <int PHASE>
__device__ __forceinline__ void bn_bwd_finish(const ActBwdArgs& a, const float (&sb)[8], const float (&sg)[8], bool overflowed, int CH) {
    if (PHASE == 1 && overflowed && a.overflow) atomicOr(a.overflow, 1);
    if (PHASE == 0) block_partials_to_slab(sb, sg, CH, a.slab, a.C);
}

// The shared pieces of the backward kernels: one prologue (BnBwdChan), one position type (PixPos), the 2x2 window
// load / store, and the source parameter SRC of the specialised kernels -- where an element's value `u` in the linear
// term, its LeakyReLU side and (MaxPool) its argmax key come from:
//   BN_SRC_Y16 / BN_SRC_Y32: the saved raw conv output y, fp16 / fp32.  u = y, side = sign of z = y scale + shift, key =
//                            leaky(z) as the forward pass stored it (compared as fp16 / as fp32: unrounded with the split
//                            hi | lo storage that goes with an fp32 y).
//   BN_SRC_ACT:              the activation the forward pass stored (fp16).  u = z = a > 0 ? a : a / slope -- or the saved
//                            fp32 y on an ill-conditioned channel, below -- side = sign of a, key = a.
enum { BN_SRC_Y16 = 0, BN_SRC_Y32 = 1, BN_SRC_ACT = 2 };

// The constants of a thread's 8 channels, filled once per thread (bn_bwd_chan).  xhat = (u - off) mul:
//   a y source: off = mean, mul = invstd, no channel `usey` (nothing to choose);
//   the stored activation: act_xhat_source (common.h) -- off = beta, mul = 1 / gamma, and on the ILL-CONDITIONED
//   channels, |gamma| < BN_ACT_T max(|beta|, 1), the y form again with usey set (need_y: the thread holds one).
// Pass 1, with dm = scale (0 where dy_keep says the filter is pruned: its dY is not needed and is zeroed):
//     out = dm (g_z - c1 - xhat c2) = dm g_z - (P u + Q),   P = dm c2 mul,  Q = dm c1 - P off     (per channel, hoisted)
// The generic kernel takes the first form from c1 / c2 (it rounds differently), the specialised kernels the second.
typedef float f32x8_t __attribute__((ext_vector_type(8)));
struct BnBwdChan {
    float sc[8], sh[8], mu[8], is[8];
    float off[8], mul[8];
    bool usey[8], need_y;
    float c1[8], c2[8];                          // pass 1 only, and so are dm, P, Q
    // The three constants of pass 1's element loop are 8-wide vector values, not arrays: the compiler splits a struct's
    // arrays into 24 scalars and then pairs them for the packed fp32 instructions inside the loop (8-9 more VGPRs and
    // an occupancy step in bn_plain_bwd_kernel<1, BN_SRC_Y16 | BN_SRC_Y32>); as vectors every instance keeps the
    // registers it had with per-kernel arrays (profiles/bn_bwd_shared_pieces.txt).  Elements are read and written as [i].
    f32x8_t dm, P, Q;
};
template <int PHASE, bool FROM_ACT>
__device__ __forceinline__ void bn_bwd_chan(const ActBwdArgs& a, int c8, BnBwdChan& ch) {
    loadf8(a.scale + c8, ch.sc);
    loadf8(a.shift + c8, ch.sh);
    loadf8(a.mean + c8, ch.mu);
    loadf8(a.invstd + c8, ch.is);
    if (FROM_ACT) {
        ch.need_y = act_xhat_source(ch.sc, ch.sh, ch.mu, ch.is, a.y != nullptr, ch.off, ch.mul, ch.usey);
    } else {
        ch.need_y = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) ch.off[i] = ch.mu[i], ch.mul[i] = ch.is[i], ch.usey[i] = false;
    }
    if (PHASE == 1) {
        loadf8(a.coef + c8, ch.c1);
        loadf8(a.coef + a.C + c8, ch.c2);
        if (a.dy_keep) {
            float kp[8];
            loadf8(a.dy_keep + c8, kp);
#pragma unroll
            for (int i = 0; i < 8; ++i) ch.dm[i] = kp[i] != 0.f ? ch.sc[i] : 0.f;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) ch.dm[i] = ch.sc[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ch.P[i] = ch.dm[i] * ch.c2[i] * ch.mul[i];
            ch.Q[i] = ch.dm[i] * ch.c1[i] - ch.P[i] * ch.off[i];
        }
    }
}

// (b, h, w) of the 32-bit pixel index `pix` of a [B][H][W] tensor (full resolution, or H/2 x W/2 for the windows of a
// MaxPool block), stepped without a division: the specialised kernels decompose their start and their grid stride once.
struct PixPos {
    unsigned pix;
    int b, h, w;
};
__device__ __forceinline__ PixPos pix_pos(unsigned pix, int H, int W) {
    const int HW = H * W;
    PixPos p;
    p.pix = pix;
    p.b = (int)(pix / (unsigned)HW);
    const int rem = (int)(pix - (unsigned)p.b * (unsigned)HW);
    p.h = rem / W, p.w = rem - p.h * W;
    return p;
}
// p += s (s.pix pixels, decomposed once), with carries
__device__ __forceinline__ void pix_pos_step(PixPos& p, const PixPos& s, int H, int W) {
    p.pix += s.pix;
    p.w += s.w;
    if (p.w >= W) p.w -= W, ++p.h;
    p.h += s.h;
    if (p.h >= H) p.h -= H, ++p.b;
    p.b += s.b;
}

// The 2x2 window of 8-channel groups whose first pixel is element `i0` of `base` (fp32 or fp16), `ld` elements per pixel
// and `row` per image row, in (h, w) scan order; and its fp16 store.
template <bool F32>
__device__ __forceinline__ void load_win(const void* base, long long i0, long long ld, long long row, float (&v)[4][8]) {
    typedef typename std::conditional<F32, float, half_t>::type elem_t;
    const elem_t* p = (const elem_t*)base + i0;
    load_y<F32>(p, 0, v[0]);
    load_y<F32>(p + ld, 0, v[1]);
    load_y<F32>(p + row, 0, v[2]);
    load_y<F32>(p + row + ld, 0, v[3]);
}
__device__ __forceinline__ void store_win(half_t* p, long long ld, long long row, const float (&v)[4][8]) {
    store8(p, v[0]);
    store8(p + ld, v[1]);
    store8(p + row, v[2]);
    store8(p + row + ld, v[3]);
}

template <int MODE, int PHASE, bool Y32>
__global__ __launch_bounds__(256) void bn_act_bwd_kernel(ActBwdArgs a) {
    constexpr int NP = MODE == MCAMD_DST_PLAIN ? 1 : 4;
    const int CH = a.C >> 3;
    const int c8 = (threadIdx.x % CH) * 8;
    BnBwdChan ch;
    bn_bwd_chan<PHASE, false>(a, c8, ch);
    const auto &sc = ch.sc, &sh = ch.sh, &mu = ch.mu, &is = ch.is, &c1 = ch.c1, &c2 = ch.c2;
    const f32x8_t& dm = ch.dm;
    float sb[8], sg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sb[i] = sg[i] = 0.f;
    const int Ho = a.H >> 1, Wo = a.W >> 1;
    bool sat = false;

    for (long long item = (long long)blockIdx.x * 256 + threadIdx.x; item < a.items; item += (long long)gridDim.x * 256) {
        long long pix = item / CH;
        int b, hh[NP], ww[NP];
        long long gp;  // pixel index into g
        if (MODE == MCAMD_DST_PLAIN) {
            b = (int)(pix / (a.H * a.W));
            int rem = (int)(pix - (long long)b * a.H * a.W);
            hh[0] = rem / a.W;
            ww[0] = rem - hh[0] * a.W;
            gp = pix;
        } else {
            b = (int)(pix / (Ho * Wo));
            int rem = (int)(pix - (long long)b * Ho * Wo);
            int ho = rem / Wo, wo = rem - ho * Wo;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                hh[k] = 2 * ho + (k >> 1);
                ww[k] = 2 * wo + (k & 1);
            }
            gp = pix;
        }
        float yv[NP][8], zz[NP][8];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            long long sp = ((long long)b * a.H + hh[k]) * a.W + ww[k];
            load_y<Y32>(a.y, sp * a.y_ld + a.y_choff + c8, yv[k]);
#pragma unroll
            for (int i = 0; i < 8; ++i) zz[k][i] = yv[k][i] * sc[i] + sh[i];
        }
        float ga[NP][8];
        if (MODE == MCAMD_DST_PLAIN) {
            load8(a.g + gp * a.g_ld + a.g_choff + c8, ga[0]);
        } else if (MODE == MCAMD_DST_POOL) {
            float gv[8];
            load8(a.g + gp * a.g_ld + a.g_choff + c8, gv);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                // argmax over the window of the activation AS STORED by the forward pass (fp16; unrounded with the
                // split hi | lo storage that goes with an fp32 y), first maximum in (h, w) scan order -- torch's
                // max_pool2d tie rule on those values
                auto stored = [&](float z) {
                    const float av = z > 0.f ? z : z * a.slope;
                    return Y32 ? av : (float)(half_t)av;
                };
                float best = stored(zz[0][i]);
                int arg = 0;
#pragma unroll
                for (int k = 1; k < NP; ++k) {
                    float av = stored(zz[k][i]);
                    if (av > best) {
                        best = av;
                        arg = k;
                    }
                }
#pragma unroll
                for (int k = 0; k < NP; ++k) ga[k][i] = (k == arg) ? gv[i] : 0.f;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NP; ++k) load8(a.g + gp * a.g_ld + a.g_choff + k * a.C + c8, ga[k]);
        }
        if (a.g2) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                long long sp = ((long long)b * a.H + hh[k]) * a.W + ww[k];
                float t[8];
                load8(a.g2 + sp * a.g2_ld + a.g2_choff + c8, t);
#pragma unroll
                for (int i = 0; i < 8; ++i) ga[k][i] += t[i];
            }
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            float out[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float gz = zz[k][i] > 0.f ? ga[k][i] : ga[k][i] * a.slope;
                float xh = (yv[k][i] - mu[i]) * is[i];
                if (PHASE == 0) {
                    sb[i] += gz;
                    sg[i] += gz * xh;
                } else {
                    out[i] = dm[i] * (gz - c1[i] - xh * c2[i]);
                }
            }
            if (PHASE == 1) {
                store8(a.dy + pad_off(b, hh[k], ww[k], a.H, a.W, a.dy_ld, a.dy_pw) + a.dy_choff + c8, out);
#pragma unroll
                for (int i = 0; i < 8; ++i) sat |= fabsf(out[i]) > 65504.f;
            }
        }
    }
    bn_bwd_finish<PHASE>(a, sb, sg, sat, CH);
}

// PLAIN blocks (16 of YOLOv2's 21 BatchNorm blocks) without a second gradient: the hoisted form out = dm g_z - (P u + Q)
// (BnBwdChan), and no position arithmetic beyond one incremental (b, h, w) for the padded addresses.  The generic kernel's
// two 64-bit divisions per 48-byte item made its loop 450-640 instructions long; on the 13x13 layers (5 items per thread,
// 4 waves per SIMD) that is ~17 us of pure instruction issue for a pass that moves 44 MB -- 14.7 us measured against
// 9 us for the forward pass over the same bytes.
//
// SRC == BN_SRC_ACT: the same two passes WITHOUT the saved raw output.  LeakyReLU is invertible, so a PLAIN block's
// pre-activation is recovered from the activation the forward pass stored for the consumer (fp16, the hi plane of split
// storage): z = a > 0 ? a : a / slope, xhat = (z - beta) / gamma.  With the split-operand precisions the saved y is fp32:
// the two passes read 2 instead of 4 bytes per element for it (0.89 -> 0.65 ms per "mixed" B=64 step), at the operand
// precision every backward pass has anyway (G and dY are fp16).  With dm = gamma invstd (0 for a pruned filter):
//     out = dm g_z - (P z + Q),   P = dm c2 / gamma,  Q = dm c1 - P beta     (per channel, hoisted)
// The stored activation carries an fp16 rounding of up to 2^-11 |z|, so xhat = (z - beta) / gamma is off by up to
// 2^-11 (|xhat| + |beta / gamma|): useless where |gamma| << |beta| (at gamma = 1e-4, beta = 1 every z rounds to beta); on
// the other channels that is at most 2^-11 (1 / BN_ACT_T + |xhat|).  A channel is ILL-CONDITIONED when |gamma| <
// BN_ACT_T max(|beta|, 1); with |gamma| = |scale| / invstd the test is |scale| < BN_ACT_T max(|beta|, 1) invstd (gamma == 0
// always included).  (BN_ACT_T and act_xhat_source: common.h -- the dgrad epilogue that takes a PLAIN block's sums
// applies the same rule.)  Those channels take xhat = (y - mu) invstd from the saved fp32 y in BOTH passes instead, with
// the y sources' P = dm c2 invstd, Q = dm c1 - P mu; the LeakyReLU side stays the sign of the stored activation.  Only the
// threads that hold such a channel read y: a healthy network's backward pass reads what it read without the rule.
// y = NULL: those channels use the activation as every other channel does (gamma == 0: xhat 0, so dgamma 0; dY is 0 there
// either way, dm = 0).
template <int PHASE, int SRC>
__global__ __launch_bounds__(256) void bn_plain_bwd_kernel(ActBwdArgs a) {
    constexpr bool ACT = SRC == BN_SRC_ACT;
    const int CH = a.C >> 3, lg = __ffs(CH) - 1;        // C / 8 is a power of two (check_c)
    const int c8 = (threadIdx.x & (CH - 1)) * 8;
    BnBwdChan ch;
    bn_bwd_chan<PHASE, ACT>(a, c8, ch);
    float sb[8], sg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sb[i] = sg[i] = 0.f;
    float satmax = 0.f;
    const float inv_slope = 1.0f / a.slope;
    const unsigned npix = (unsigned)(a.items >> lg);
    const unsigned stride = (gridDim.x * 256u) >> lg;                      // pixels per grid stride
    PixPos p = pix_pos((blockIdx.x * 256u + threadIdx.x) >> lg, a.H, a.W);
    const PixPos step = pix_pos(stride, a.H, a.W);
    for (; p.pix < npix; pix_pos_step(p, step, a.H, a.W)) {
        float sv[8], gv[8], u[8];                        // sv: the source's value, y or the stored activation
        if (ACT) load8(a.act + pad_off(p.b, p.h, p.w, a.H, a.W, a.act_ld, a.act_pw) + a.act_choff + c8, sv);
        else load_y<SRC == BN_SRC_Y32>(a.y, (long long)p.pix * a.y_ld + a.y_choff + c8, sv);
        load8(a.g + (long long)p.pix * a.g_ld + a.g_choff + c8, gv);
#pragma unroll
        for (int i = 0; i < 8; ++i) u[i] = !ACT ? sv[i] : sv[i] > 0.f ? sv[i] : sv[i] * inv_slope;
        if (ACT && ch.need_y) {                          // ill-conditioned channels: the saved y in place of z
            float yv[8];
            load_y<true>(a.y, (long long)p.pix * a.y_ld + a.y_choff + c8, yv);
#pragma unroll
            for (int i = 0; i < 8; ++i) u[i] = ch.usey[i] ? yv[i] : u[i];
        }
        float out[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float side = ACT ? sv[i] : sv[i] * ch.sc[i] + ch.sh[i];
            const float gz = side > 0.f ? gv[i] : gv[i] * a.slope;
            if (PHASE == 0) {
                sb[i] += gz;
                sg[i] += gz * ((u[i] - ch.off[i]) * ch.mul[i]);
            } else {
                const float o = ch.dm[i] * gz - (ch.P[i] * u[i] + ch.Q[i]);
                out[i] = o;
                satmax = fmaxf(satmax, fabsf(o));
            }
        }
        if (PHASE == 1) store8(a.dy + pad_off(p.b, p.h, p.w, a.H, a.W, a.dy_ld, a.dy_pw) + a.dy_choff + c8, out);
    }
    bn_bwd_finish<PHASE>(a, sb, sg, satmax > 65504.f, CH);
}

// MaxPool blocks (conv2 / conv5 / conv8 / conv13 of YOLOv2: 0.7 of the 1.5 ms of BatchNorm backward).
// The generic kernel above spends ~1 300 instructions per item there (SQ_ACTIVE_INST_ANY 0.62 of the wave cycles, 3.6 TB/s:
// it is issue-bound, not HBM-bound) because it treats the four window pixels as four full backward elements.  Only the
// argmax pixel receives a gradient, so with  out = dm (g_z - c1 - xhat c2),  xhat = (u - off) mul:
//     out_k = [k == arg] dm g_z  -  (P u_k + Q)       (P, Q per channel, hoisted: BnBwdChan)
// i.e. one multiply-add per non-argmax element; the sums of pass 0 need the argmax element only.  The argmax itself is
// taken exactly as the generic kernel takes it (first maximum of the activations AS STORED by the forward pass; a y16
// source compares them as fp16 values instead of converting them back).  32-bit positions stepped incrementally (no
// division in the loop).
// G2: a second gradient at full resolution (the route that reads conv13 beside its pool) is added to every window pixel,
// so every pixel has a g_z -- still without the generic kernel's per-pixel xhat / select chains.
//
// SRC == BN_SRC_ACT: MaxPool blocks WITHOUT the saved raw output.  As a PLAIN block's pre-activation is recovered from the
// stored activation (bn_plain_bwd_kernel), a MaxPool block's comes from a FULL-RESOLUTION fp16 copy of its activation (the
// forward pass writes one beside the pooled output: mcamd_act_desc.pool_act).  z = a > 0 ? a : a / slope, xhat =
// (z - beta) / gamma; the window's argmax is the maximum of the four STORED values -- the forward pass stores them so that
// the element it pooled (first maximum of the unrounded activations) is their strict maximum -- and the LeakyReLU side of
// every element is the sign of its stored value (rounding keeps the sign).  Split-operand engines save y as fp32: the two
// passes read 2 instead of 4 bytes per element (conv2 / 5 / 8 / 13 at B = 64: 0.66 GB less per step) for 2 bytes more
// written by the forward pass where the copy did not exist.  Ill-conditioned channels (act_xhat_source) take u_k from the
// saved fp32 y in both passes, as in the PLAIN kernel, while the argmax and the LeakyReLU sides still come from the stored
// activation.
template <int PHASE, int SRC, bool G2>
__global__ __launch_bounds__(256) void bn_pool_bwd_kernel(ActBwdArgs a) {
    constexpr bool ACT = SRC == BN_SRC_ACT;
    const int CH = a.C >> 3, lg = __ffs(CH) - 1;        // C / 8 is a power of two (check_c)
    const int c8 = (threadIdx.x & (CH - 1)) * 8;
    BnBwdChan ch;
    bn_bwd_chan<PHASE, ACT>(a, c8, ch);
    float sb[8], sg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sb[i] = sg[i] = 0.f;
    float satmax = 0.f;
    const float inv_slope = 1.0f / a.slope;
    const int Ho = a.H >> 1, Wo = a.W >> 1;
    const unsigned npix = (unsigned)(a.items >> lg);                       // pooled pixels
    const unsigned stride = (gridDim.x * 256u) >> lg;                      // pooled pixels per grid stride
    PixPos p = pix_pos((blockIdx.x * 256u + threadIdx.x) >> lg, Ho, Wo);
    const PixPos step = pix_pos(stride, Ho, Wo);
    // elements per image row: y and g2 are unpadded, the activation copy and dY padded
    const long long yrow = (long long)a.W * a.y_ld, g2row = (long long)a.W * a.g2_ld;
    const long long arow = (long long)(a.W + a.act_pw) * a.act_ld, drow = (long long)(a.W + a.dy_pw) * a.dy_ld;
    for (; p.pix < npix; pix_pos_step(p, step, Ho, Wo)) {
        const long long fp = ((long long)p.b * a.H + 2 * p.h) * a.W + 2 * p.w;   // the window's first pixel, unpadded
        float sv[4][8], gv[8], g2v[4][8], u[4][8];       // sv: the source's values, y or the stored activation
        if (ACT) load_win<false>(a.act, pad_off(p.b, 2 * p.h, 2 * p.w, a.H, a.W, a.act_ld, a.act_pw) + a.act_choff + c8, a.act_ld, arow, sv);
        else load_win<SRC == BN_SRC_Y32>(a.y, fp * a.y_ld + a.y_choff + c8, a.y_ld, yrow, sv);
        load8(a.g + (long long)p.pix * a.g_ld + a.g_choff + c8, gv);
        if (G2) load_win<false>(a.g2, fp * a.g2_ld + a.g2_choff + c8, a.g2_ld, g2row, g2v);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < 8; ++i) u[k][i] = !ACT ? sv[k][i] : sv[k][i] > 0.f ? sv[k][i] : sv[k][i] * inv_slope;
        if (ACT && ch.need_y) {                          // ill-conditioned channels: the saved y in place of z
            float yv[4][8];
            load_win<true>(a.y, fp * a.y_ld + a.y_choff + c8, a.y_ld, yrow, yv);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int i = 0; i < 8; ++i) u[k][i] = ch.usey[i] ? yv[k][i] : u[k][i];
        }
        float out[4][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float side[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) side[k] = ACT ? sv[k][i] : sv[k][i] * ch.sc[i] + ch.sh[i];
            // the activation of element k as the forward pass stored it
            auto key = [&](int k) {
                if constexpr (ACT) return side[k];
                else if constexpr (SRC == BN_SRC_Y32) return side[k] > 0.f ? side[k] : side[k] * a.slope;
                else return (half_t)(side[k] > 0.f ? side[k] : side[k] * a.slope);
            };
            // first maximum in (h, w) scan order; ss, us: side and u of that element
            int arg = 0;
            auto best = key(0);
            float ss = side[0], us = u[0][i];
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const auto av = key(k);
                const bool gt = av > best;
                best = gt ? av : best, arg = gt ? k : arg, ss = gt ? side[k] : ss, us = gt ? u[k][i] : us;
            }
            if (G2) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float ga = (k == arg ? gv[i] : 0.f) + g2v[k][i];
                    const float gzk = side[k] > 0.f ? ga : ga * a.slope;
                    if (PHASE == 0) {
                        sb[i] += gzk;
                        sg[i] += gzk * ((u[k][i] - ch.off[i]) * ch.mul[i]);
                    } else {
                        const float o = ch.dm[i] * gzk - (ch.P[i] * u[k][i] + ch.Q[i]);
                        out[k][i] = o;
                        satmax = fmaxf(satmax, fabsf(o));
                    }
                }
            } else {
                const float gz = ss > 0.f ? gv[i] : gv[i] * a.slope;
                if (PHASE == 0) {
                    sb[i] += gz;
                    sg[i] += gz * ((us - ch.off[i]) * ch.mul[i]);
                } else {
                    const float t = ch.dm[i] * gz;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float o = (k == arg ? t : 0.f) - (ch.P[i] * u[k][i] + ch.Q[i]);
                        out[k][i] = o;
                        satmax = fmaxf(satmax, fabsf(o));
                    }
                }
            }
        }
        if (PHASE == 1) store_win(a.dy + pad_off(p.b, 2 * p.h, 2 * p.w, a.H, a.W, a.dy_ld, a.dy_pw) + a.dy_choff + c8, a.dy_ld, drow, out);
    }
    bn_bwd_finish<PHASE>(a, sb, sg, satmax > 65504.f, CH);
}

// Pass 0 of a MaxPool block without a second gradient, from the POOLED tensors (mcamd_act_bwd_desc.pool_out).  Only the
// pooled element of a window has a g_z, so the two sums need that element's activation and nothing of the other three.
// bn_act_fwd_kernel writes it twice: as the pooled output, sat_half(max of the four unrounded activations), and into the
// full-resolution copy as the window's strict maximum, sat_half of the same value.  The maximum of the four stored values
// in bn_pool_bwd_kernel<0, BN_SRC_ACT, false> is therefore the pooled value bit for bit (tests/test_bn_pool_sums_gpu.py
// pins it), and this pass reads pooled G + pooled activation, 4 bytes per window and channel, where that one reads 10.
// The terms are the same fp32 values and a thread adds them in the same order (its windows pix, pix + stride, ...; two per
// loop trip, four 16-byte loads in flight), so at the same grid the slab is bit-equal to that pass's.  conv2 / 5 / 8 at
// B = 64: 61 -> 22 us per launch, FETCH_SIZE 2.5 : 1.
// Threads that hold an ill-conditioned channel (act_xhat_source) need z from the saved fp32 y AT THE ARGMAX, which the
// pooled tensor does not locate: they load the window of the copy and of y as the other kernel does, one window per
// trip.  A healthy network has no such thread.
// ACT == false: an engine without the copy (filter compaction) -- pass 0 read the four fp32 y values of a window, 18 bytes
// with G.  The pooled activation gives xhat = (z - beta) / gamma at fp16 accuracy, the trade the PLAIN blocks' activation
// source made; the ill-conditioned channels take the argmax from the unrounded activations of y, as
// bn_pool_bwd_kernel<., BN_SRC_Y32, .>.

// z of the argmax element from the saved y, for the ill-conditioned channels of one window (one image row of the window at
// a time: 32 values in flight)
template <bool ACT>
__device__ __forceinline__ void pool_sums_z_from_y(const ActBwdArgs& a, const PixPos& p, int c8, const bool (&usey)[8],
                                                   const float (&sc)[8], const float (&sh)[8], float (&z)[8]) {
    const half_t* ap = ACT ? a.act + pad_off(p.b, 2 * p.h, 2 * p.w, a.H, a.W, a.act_ld, a.act_pw) + a.act_choff + c8 : nullptr;
    const long long arow = (long long)(a.W + a.act_pw) * a.act_ld;
    const float* yf = (const float*)a.y + (((long long)p.b * a.H + 2 * p.h) * a.W + 2 * p.w) * a.y_ld + a.y_choff + c8;
    const long long yrow = (long long)a.W * a.y_ld;
    float best[8], ys[8];
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
        float av[2][8], yv[2][8];
        loadf8(yf + r * yrow, yv[0]);
        loadf8(yf + r * yrow + a.y_ld, yv[1]);
        if (ACT) {
            load8(ap + r * arow, av[0]);
            load8(ap + r * arow + a.act_ld, av[1]);
        } else {                                         // no copy: the unrounded activations, as the BN_SRC_Y32 source
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float zk = yv[k][i] * sc[i] + sh[i];
                    av[k][i] = zk > 0.f ? zk : zk * a.slope;
                }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // first maximum in (h, w) scan order of the activations as the forward pass stored them
            if (r == 0) best[i] = av[0][i], ys[i] = yv[0][i];
#pragma unroll
            for (int k = r == 0 ? 1 : 0; k < 2; ++k) {
                const bool gt = av[k][i] > best[i];
                best[i] = gt ? av[k][i] : best[i], ys[i] = gt ? yv[k][i] : ys[i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = usey[i] ? ys[i] : z[i];
}
template <bool ACT>
__global__ __launch_bounds__(256) void bn_pool_sums_kernel(ActBwdArgs a) {
    const int CH = a.C >> 3, lg = __ffs(CH) - 1;        // C / 8 is a power of two (check_c)
    const int c8 = (threadIdx.x & (CH - 1)) * 8;
    BnBwdChan ch;
    bn_bwd_chan<0, true>(a, c8, ch);                     // xhat from the pooled activation, with or without the copy
    float sb[8], sg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sb[i] = sg[i] = 0.f;
    const float inv_slope = 1.0f / a.slope;
    const int Ho = a.H >> 1, Wo = a.W >> 1;
    const unsigned npix = (unsigned)(a.items >> lg);                       // pooled pixels
    const unsigned stride = (gridDim.x * 256u) >> lg;                      // pooled pixels per grid stride
    PixPos p0 = pix_pos((blockIdx.x * 256u + threadIdx.x) >> lg, Ho, Wo);
    const half_t* pout = a.pool_out + a.pool_out_choff + c8;
    const half_t* gp = a.g + a.g_choff + c8;
    auto add = [&](const float (&z)[8], const float (&pv)[8], const float (&gv)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float gz = pv[i] > 0.f ? gv[i] : gv[i] * a.slope;
            sb[i] += gz;
            sg[i] += gz * ((z[i] - ch.off[i]) * ch.mul[i]);
        }
    };
    auto window = [&](const PixPos& p, float (&pv)[8], float (&gv)[8]) {
        load8(pout + pad_off(p.b, p.h, p.w, Ho, Wo, a.pool_out_ld, a.pool_out_pw), pv);
        load8(gp + (long long)p.pix * a.g_ld, gv);
    };
    auto z_of = [&](const float (&pv)[8], float (&z)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = pv[i] > 0.f ? pv[i] : pv[i] * inv_slope;
    };
    if (ch.need_y) {                                     // a thread with an ill-conditioned channel: one window per trip
        const PixPos step = pix_pos(stride, Ho, Wo);
        for (; p0.pix < npix; pix_pos_step(p0, step, Ho, Wo)) {
            float pv[8], gv[8], z[8];
            window(p0, pv, gv);
            z_of(pv, z);
            pool_sums_z_from_y<ACT>(a, p0, c8, ch.usey, ch.sc, ch.sh, z);
            add(z, pv, gv);
        }
    } else {
        const PixPos step2 = pix_pos(2u * stride, Ho, Wo);
        PixPos p1 = pix_pos(p0.pix + stride, Ho, Wo);
        for (; p1.pix < npix; pix_pos_step(p0, step2, Ho, Wo), pix_pos_step(p1, step2, Ho, Wo)) {
            float pv0[8], gv0[8], pv1[8], gv1[8], z[8];
            window(p0, pv0, gv0);
            window(p1, pv1, gv1);
            z_of(pv0, z);
            add(z, pv0, gv0);
            z_of(pv1, z);
            add(z, pv1, gv1);
        }
        if (p0.pix < npix) {
            float pv[8], gv[8], z[8];
            window(p0, pv, gv);
            z_of(pv, z);
            add(z, pv, gv);
        }
    }
    bn_bwd_finish<0>(a, sb, sg, false, CH);
}

__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(const float* slab, int nblocks, int ld, int C, double count,
                                                               float inv_scale, float* dgamma, float* dbeta,
                                                               float* coef, const int* perm, int skip_from) {
    __shared__ double red[2][16][RED_CPB];
    const int cx = threadIdx.x & (RED_CPB - 1), ry = threadIdx.x / RED_CPB;
    const int c = blockIdx.x * RED_CPB + cx;
    double sb = 0.0, sg = 0.0;
    if (c < C) {
        for (int p = ry; p < nblocks; p += RED_RG) {
            sb += (double)slab[((long long)p * 2 + 0) * ld + c];
            sg += (double)slab[((long long)p * 2 + 1) * ld + c];
        }
    }
    block_reduce2(sb, sg, red);
    if (ry != 0 || c >= C) return;
    const int pc = perm ? perm[c] : c;   // parameter-order index of this physical channel
    const bool skip = skip_from > 0 && c >= skip_from;   // a folded dead channel: its consumer delivers these gradients (fold.hip)
    if (dbeta && !skip) dbeta[pc] = (float)(sb * inv_scale);
    if (dgamma && !skip) dgamma[pc] = (float)(sg * inv_scale);
    coef[c] = (float)(sb / count);
    coef[C + c] = (float)(sg / count);
}

// ------------------------------------------------------------------------------------
// NCHW fp32 -> padded NHWC fp16 (model boundary)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* src, int B, int C, int H, int W, float mul,
                                                           half_t* dst, int ld, int choff, int cgroups, int* overflow,
                                                           int plane, int pw) {
    bool sat = false;
    // item = (pixel, channel group of up to 8); consecutive threads -> consecutive pixels (coalesced NCHW reads)
    const long long HW = (long long)H * W;
    const long long items = (long long)B * HW * cgroups;
    for (long long item = (long long)blockIdx.x * 256 + threadIdx.x; item < items; item += (long long)gridDim.x * 256) {
        long long pg = item / ((long long)B * HW);  // channel group slowest
        long long pix = item - pg * (long long)B * HW;
        int b = (int)(pix / HW);
        int rem = (int)(pix - (long long)b * HW);
        int h = rem / W, w = rem - h * W;
        int c0 = (int)pg * 8;
        half_t* d = dst + pad_off(b, h, w, H, W, ld, pw) + choff + c0;
        const float* s = src + ((long long)b * C + c0) * HW + rem;
        int nc = C - c0 < 8 ? C - c0 : 8;
        // not "|v| > 65504": that is false for a NaN, which sat_half turns into -65504 -- a finite gradient without a flag
        if (overflow)
            for (int i = 0; i < nc; ++i) sat |= !(fabsf(s[i * HW] * mul) <= 65504.f);
        if (plane > 0) {  // split storage: hi | lo | hi planes, `plane` channels apart (mcamd_act_desc.planes)
            for (int i = 0; i < nc; ++i) {
                const float v = s[i * HW] * mul;
                const half_t hi = sat_half(v);
                d[i] = hi;
                d[plane + i] = (half_t)(v - (float)hi);
                d[2 * plane + i] = hi;
            }
        } else if (ld == 4) {  // stem image: 3 channels + one zero, one 8-byte store per pixel
            h4_t q;
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = (i < nc) ? sat_half(s[i * HW] * mul) : (half_t)0.f;
            *(h4_t*)d = q;
        } else if (nc == 8) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = s[i * HW] * mul;
            store8(d, v);
        } else {
            for (int i = 0; i < nc; ++i) d[i] = sat_half(s[i * HW] * mul);
        }
    }
    if (sat && overflow) atomicOr(overflow, 1);
}

// ------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------
static int stream_grid(long long items) {
    long long g = (items + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

extern "C" int mcamd_bn_coeffs_ex(const float* stats, int32_t stats_rows, int32_t stats_ld, int32_t C, int64_t count,
                                  const float* gamma, const float* beta, float* running_mean, float* running_var,
                                  float momentum, float eps, int32_t training, float* scale, float* shift,
                                  float* save_mean, float* save_invstd, const int32_t* chan_perm, int32_t ones_channel,
                                  void* stream) {
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* s) {
            return mcamd_bn_coeffs_ex(stats, stats_rows, stats_ld, C, count, gamma, beta, running_mean, running_var, momentum, eps,
                                      training, scale, shift, save_mean, save_invstd, chan_perm, ones_channel, s);
        });
    MCAMD_REQUIRE(C > 0 && gamma && beta && running_mean && running_var && scale && shift, "bn_coeffs: null argument");
    MCAMD_REQUIRE(!training || (stats && stats_rows > 0 && stats_ld >= C && count > 0), "bn_coeffs: bad statistics slab");
    MCAMD_REQUIRE(ones_channel < C, "bn_coeffs: ones_channel %d outside the %d channels", ones_channel, C);
    hipLaunchKernelGGL(bn_coeffs_kernel, dim3((C + RED_CPB - 1) / RED_CPB), dim3(1024), 0, (hipStream_t)stream, stats, stats_rows,
                       stats_ld, C, (double)count, gamma, beta, running_mean, running_var, momentum, eps, training,
                       scale, shift, save_mean, save_invstd, (const int*)chan_perm, ones_channel < 0 ? -1 : ones_channel);
    MCAMD_LAUNCH_CHECK("bn_coeffs");
    return MCAMD_OK;
}

extern "C" int mcamd_bn_coeffs(const float* stats, int32_t stats_rows, int32_t stats_ld, int32_t C, int64_t count,
                               const float* gamma, const float* beta, float* running_mean, float* running_var,
                               float momentum, float eps, int32_t training, float* scale, float* shift,
                               float* save_mean, float* save_invstd, const int32_t* chan_perm, void* stream) {
    return mcamd_bn_coeffs_ex(stats, stats_rows, stats_ld, C, count, gamma, beta, running_mean, running_var, momentum, eps,
                              training, scale, shift, save_mean, save_invstd, chan_perm, -1, stream);
}

static int check_c(int C, const char* what) {
    int CH = C / 8;
    if (C <= 0 || C % 8 != 0 || CH > 256 || 256 % CH != 0) {
        mcamd_set_error("%s: channel count %d must be 8 * (a power of two <= 256)", what, C);
        return MCAMD_EINVAL;
    }
    return MCAMD_OK;
}

// Which bn_act_fwd_kernel<MODE, FIXED, Y32, PL, Q8> instance a descriptor gets, its grid and its arguments: the ONE place
// that validates a descriptor and decides, for the launch and for the host-only query mcamd_bn_act_fwd_instance (what
// the exact per-instance tests ask), so the two cannot disagree.
static int act_route(const mcamd_act_desc* d, ActArgs* out, mcamd_act_instance* r) {
    MCAMD_REQUIRE(d && d->y && d->dst && d->scale && d->shift, "bn_act_fwd: null argument");
    MCAMD_REQUIRE(d->C > 0 && d->C % 8 == 0, "bn_act_fwd: channel count %d must be a positive multiple of 8", d->C);
    MCAMD_REQUIRE(d->y_ld % 8 == 0 && d->y_choff % 8 == 0 && d->dst_ld % 8 == 0 && d->dst_choff % 8 == 0 &&
                      d->dst2_ld % 8 == 0 && d->dst2_choff % 8 == 0,
                  "bn_act_fwd: leading dimensions / channel offsets must be multiples of 8");
    MCAMD_REQUIRE(d->mode == MCAMD_DST_PLAIN || (d->H % 2 == 0 && d->W % 2 == 0), "bn_act_fwd: pool/reorg need even H, W");
    MCAMD_REQUIRE(d->mode != MCAMD_DST_PLAIN || !d->dst2, "bn_act_fwd: dst2 only with pool/reorg");
    MCAMD_REQUIRE(d->y_dtype == 0 || d->y_dtype == 1, "bn_act_fwd: y_dtype %d (0 = fp16, 1 = fp32)", d->y_dtype);
    const int planes = d->planes == 0 ? 1 : d->planes;
    const int planes2 = d->planes2 == 0 ? planes : d->planes2;
    MCAMD_REQUIRE(planes >= 1 && planes <= 4 && planes2 >= 1 && planes2 <= 4 && (planes == 1) == (planes2 == 1),
                  "bn_act_fwd: planes / planes2 must be 1, or both of 2, 3, 4 (got %d, %d)", d->planes, d->planes2);
    if (planes >= 2) {
        const int span = d->mode == MCAMD_DST_REORG ? 4 * d->C : d->C;
        // (4: the e4m3 region is one plane stride of fp16 units, like a lo plane)
        MCAMD_REQUIRE(d->dst_plane % 8 == 0 && d->dst_plane >= span &&
                          d->dst_choff + (planes == 4 ? 2 * d->dst_plane : (planes - 1) * d->dst_plane + span) <= d->dst_ld,
                      "bn_act_fwd: %d planes of stride %d (+ offset %d, %d channels) do not fit dst_ld %d", planes, d->dst_plane,
                      d->dst_choff, span, d->dst_ld);
        MCAMD_REQUIRE(!d->dst2 || (d->dst2_plane % 8 == 0 && d->dst2_plane >= d->C &&
                                   d->dst2_choff + (planes2 == 4 ? 2 * d->dst2_plane : (planes2 - 1) * d->dst2_plane + d->C) <= d->dst2_ld),
                      "bn_act_fwd: %d planes of stride %d do not fit dst2_ld %d", planes2, d->dst2_plane, d->dst2_ld);
    }
    ActArgs a;
    a.dst2_pl = planes2;
    a.dst_plane = d->dst_plane, a.dst2_plane = d->dst2_plane;
    MCAMD_REQUIRE((d->dst_pad == 0 || d->dst_pad == 1) && (d->dst2_pad == 0 || d->dst2_pad == 1), "bn_act_fwd: dst_pad / dst2_pad must be 0 or 1");
    a.dst_pw = d->dst_pad ? 1 : 2, a.dst2_pw = d->dst2_pad ? 1 : 2;
    a.y = d->y;
    a.scale = d->scale;
    a.shift = d->shift;
    a.dst = (half_t*)d->dst;
    a.dst2 = (half_t*)d->dst2;
    a.B = d->B, a.H = d->H, a.W = d->W, a.C = d->C;
    a.y_ld = d->y_ld, a.y_choff = d->y_choff, a.dst_ld = d->dst_ld, a.dst_choff = d->dst_choff;
    a.dst2_ld = d->dst2_ld, a.dst2_choff = d->dst2_choff;
    a.slope = d->slope;
    long long pixels = (long long)d->B * d->H * d->W;
    if (d->mode != MCAMD_DST_PLAIN) pixels /= 4;
    a.items = pixels * (d->C / 8);
    a.border = d->border;
    MCAMD_REQUIRE(!d->pool_act || (d->mode == MCAMD_DST_POOL && d->pool_act_ld % 8 == 0 && d->pool_act_ld >= d->C &&
                                   (d->pool_act_pad == 0 || d->pool_act_pad == 1)),
                  "bn_act_fwd: pool_act goes with mode pool, pool_act_ld (%d) a multiple of 8 >= C, pool_act_pad 0 or 1", d->pool_act_ld);
    a.pool_act = (half_t*)d->pool_act;
    a.pool_act_ld = d->pool_act_ld, a.pool_act_pw = d->pool_act_pad ? 1 : 2;
    const int CH = d->C / 8;
    const bool fixed = CH <= 256 && 256 % CH == 0;
    const bool y32 = d->y_dtype == 1;
    MCAMD_REQUIRE(planes != 4 || y32, "bn_act_fwd: planes 4 (e4m3 corrections) goes with an fp32 y");
    const bool q8 = d->dst_q8 || d->dst2_q8;
    MCAMD_REQUIRE(!q8 || (y32 && planes == 1 && planes2 == 1 && !d->pool_act && (!d->dst2_q8 || d->dst2)),
                  "bn_act_fwd: byte destinations (dst_q8 / dst2_q8) go with an fp32 y, one plane, no pool_act, and dst2_q8 with dst2");
    a.dst_q8 = (char*)d->dst_q8, a.dst2_q8 = (char*)d->dst2_q8;
    MCAMD_REQUIRE(d->mode == MCAMD_DST_PLAIN || d->mode == MCAMD_DST_POOL || d->mode == MCAMD_DST_REORG, "bn_act_fwd: bad mode %d", d->mode);
    r->mode = d->mode, r->fixed = fixed, r->y32 = y32, r->planes = planes, r->planes2 = planes2, r->q8 = q8;
    r->items = a.items, r->grid = stream_grid(a.items);
    if (out) *out = a;
    return MCAMD_OK;
}

extern "C" int mcamd_bn_act_fwd_instance(const mcamd_act_desc* d, mcamd_act_instance* out) {
    MCAMD_REQUIRE(out, "bn_act_fwd_instance: null output");
    return act_route(d, nullptr, out);
}

extern "C" int mcamd_bn_act_fwd(const mcamd_act_desc* d, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(d, "bn_act_fwd: null descriptor");
        const mcamd_act_desc d_ = *d;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_bn_act_fwd(&d_, s); });
    }
    ActArgs a;
    mcamd_act_instance r;
    if (int rc = act_route(d, &a, &r)) return rc;
    const int grid = r.grid, planes = r.planes;
    const bool fixed = r.fixed, y32 = r.y32, q8 = r.q8;
    hipStream_t st = (hipStream_t)stream;
#define ACT_INST(MODE_, FIXED_)                                                                                         \
    do {                                                                                                                \
        if (q8) hipLaunchKernelGGL((bn_act_fwd_kernel<MODE_, FIXED_, true, 1, true>), dim3(grid), dim3(256), 0, st, a);                 \
        else if (y32 && planes == 4) hipLaunchKernelGGL((bn_act_fwd_kernel<MODE_, FIXED_, true, 4>), dim3(grid), dim3(256), 0, st, a);       \
        else if (y32 && planes == 3) hipLaunchKernelGGL((bn_act_fwd_kernel<MODE_, FIXED_, true, 3>), dim3(grid), dim3(256), 0, st, a);  \
        else if (y32 && planes == 2) hipLaunchKernelGGL((bn_act_fwd_kernel<MODE_, FIXED_, true, 2>), dim3(grid), dim3(256), 0, st, a);  \
        else if (y32) hipLaunchKernelGGL((bn_act_fwd_kernel<MODE_, FIXED_, true, 1>), dim3(grid), dim3(256), 0, st, a);                 \
        else if (planes == 3) hipLaunchKernelGGL((bn_act_fwd_kernel<MODE_, FIXED_, false, 3>), dim3(grid), dim3(256), 0, st, a);        \
        else if (planes == 2) hipLaunchKernelGGL((bn_act_fwd_kernel<MODE_, FIXED_, false, 2>), dim3(grid), dim3(256), 0, st, a);        \
        else hipLaunchKernelGGL((bn_act_fwd_kernel<MODE_, FIXED_, false, 1>), dim3(grid), dim3(256), 0, st, a);                         \
    } while (0)
#define ACT_CASE(MODE_)                   \
    do {                                  \
        if (fixed) ACT_INST(MODE_, true); \
        else ACT_INST(MODE_, false);      \
    } while (0)
    if (d->mode == MCAMD_DST_PLAIN) ACT_CASE(MCAMD_DST_PLAIN);
    else if (d->mode == MCAMD_DST_POOL) ACT_CASE(MCAMD_DST_POOL);
    else ACT_CASE(MCAMD_DST_REORG);
#undef ACT_CASE
#undef ACT_INST
    MCAMD_LAUNCH_CHECK("bn_act_fwd");
    return MCAMD_OK;
}

static const int kBwdBlocks = 1024;

extern "C" size_t mcamd_bn_act_bwd_workspace_bytes(const mcamd_act_bwd_desc* d) {
    return ((size_t)kBwdBlocks * 2 * d->C + 2 * (size_t)d->C) * sizeof(float);
}

// Which kernel runs pass 0 (the sums) and pass 1 (dY) of a backward call: the ONE place that decides.  pool_fast /
// plain_fast: the specialised kernels apply (the mode, no second gradient for PLAIN, 32-bit positions, the environment
// switches); otherwise the generic kernel of the mode, nullptr for a mode that does not exist.  pool_out: pass 0 of a
// MaxPool block from the pooled tensors.
typedef void (*BwdKernel)(ActBwdArgs);
struct BwdRoute {
    BwdKernel pass0, pass1;
};
static BwdRoute bwd_route(int mode, bool y32, bool act, bool g2, bool pool_out, bool pool_fast, bool plain_fast) {
    auto pass = [&](auto phase) -> BwdKernel {
        constexpr int PH = decltype(phase)::value;
        if (pool_fast) {
            if (act) return g2 ? bn_pool_bwd_kernel<PH, BN_SRC_ACT, true> : bn_pool_bwd_kernel<PH, BN_SRC_ACT, false>;
            if (y32) return g2 ? bn_pool_bwd_kernel<PH, BN_SRC_Y32, true> : bn_pool_bwd_kernel<PH, BN_SRC_Y32, false>;
            return g2 ? bn_pool_bwd_kernel<PH, BN_SRC_Y16, true> : bn_pool_bwd_kernel<PH, BN_SRC_Y16, false>;
        }
        if (plain_fast)
            return act ? bn_plain_bwd_kernel<PH, BN_SRC_ACT> : y32 ? bn_plain_bwd_kernel<PH, BN_SRC_Y32> : bn_plain_bwd_kernel<PH, BN_SRC_Y16>;
        if (mode == MCAMD_DST_PLAIN) return y32 ? bn_act_bwd_kernel<MCAMD_DST_PLAIN, PH, true> : bn_act_bwd_kernel<MCAMD_DST_PLAIN, PH, false>;
        if (mode == MCAMD_DST_POOL) return y32 ? bn_act_bwd_kernel<MCAMD_DST_POOL, PH, true> : bn_act_bwd_kernel<MCAMD_DST_POOL, PH, false>;
        if (mode == MCAMD_DST_REORG) return y32 ? bn_act_bwd_kernel<MCAMD_DST_REORG, PH, true> : bn_act_bwd_kernel<MCAMD_DST_REORG, PH, false>;
        return nullptr;
    };
    BwdRoute r = {pass(std::integral_constant<int, 0>()), pass(std::integral_constant<int, 1>())};
    if (pool_fast && pool_out) r.pass0 = act ? bn_pool_sums_kernel<true> : bn_pool_sums_kernel<false>;
    return r;
}

extern "C" int mcamd_bn_act_bwd(const mcamd_act_bwd_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(d, "bn_act_bwd: null descriptor");
        const mcamd_act_bwd_desc d_ = *d;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_bn_act_bwd(&d_, workspace, workspace_bytes, s); });
    }
    MCAMD_REQUIRE(d && (d->y || d->act) && d->g && d->dy && d->scale && d->shift && d->mean && d->invstd && workspace,
                  "bn_act_bwd: null argument");
    if (check_c(d->C, "bn_act_bwd")) return MCAMD_EINVAL;
    if (workspace_bytes < mcamd_bn_act_bwd_workspace_bytes(d)) {
        mcamd_set_error("bn_act_bwd: workspace %zu < %zu bytes", workspace_bytes, mcamd_bn_act_bwd_workspace_bytes(d));
        return MCAMD_EWORKSPACE;
    }
    MCAMD_REQUIRE(d->y_ld % 8 == 0 && d->y_choff % 8 == 0 && d->g_ld % 8 == 0 && d->g_choff % 8 == 0 &&
                      d->g2_ld % 8 == 0 && d->g2_choff % 8 == 0 && d->dy_ld % 8 == 0 && d->dy_choff % 8 == 0,
                  "bn_act_bwd: leading dimensions / channel offsets must be multiples of 8");
    MCAMD_REQUIRE(d->mode == MCAMD_DST_PLAIN || (d->H % 2 == 0 && d->W % 2 == 0), "bn_act_bwd: pool/reorg need even H, W");
    MCAMD_REQUIRE(d->grad_scale > 0.f, "bn_act_bwd: grad_scale must be positive");
    MCAMD_REQUIRE(d->y_dtype == 0 || d->y_dtype == 1, "bn_act_bwd: y_dtype %d (0 = fp16, 1 = fp32)", d->y_dtype);
    const bool y32 = d->y_dtype == 1;
    ActBwdArgs a;
    a.y = d->y;
    a.scale = d->scale, a.shift = d->shift, a.mean = d->mean, a.invstd = d->invstd;
    a.g = (const half_t*)d->g;
    a.g2 = (const half_t*)d->g2;
    a.dy = (half_t*)d->dy;
    a.slab = (float*)workspace;
    float* coef = (float*)workspace + (size_t)kBwdBlocks * 2 * d->C;
    a.coef = coef;
    a.dy_keep = d->dy_keep;
    a.overflow = (int*)d->overflow;
    a.B = d->B, a.H = d->H, a.W = d->W, a.C = d->C;
    a.y_ld = d->y_ld, a.y_choff = d->y_choff, a.g_ld = d->g_ld, a.g_choff = d->g_choff;
    a.g2_ld = d->g2_ld, a.g2_choff = d->g2_choff, a.dy_ld = d->dy_ld, a.dy_choff = d->dy_choff;
    MCAMD_REQUIRE(d->dy_pad == 0 || d->dy_pad == 1, "bn_act_bwd: dy_pad must be 0 or 1");
    a.dy_pw = d->dy_pad ? 1 : 2;
    a.slope = d->slope;
    a.act = (const half_t*)d->act;
    a.act_ld = d->act_ld, a.act_choff = d->act_choff;
    a.act_pw = d->act_pad ? 1 : 2;
    if (d->act) {
        MCAMD_REQUIRE((d->mode == MCAMD_DST_PLAIN && !d->g2) || d->mode == MCAMD_DST_POOL,
                      "bn_act_bwd: `act` (backward from the stored activation) is for PLAIN blocks without a second gradient "
                      "and for MaxPool blocks (a full-resolution copy of the activation)");
        MCAMD_REQUIRE(d->act_ld % 8 == 0 && d->act_choff % 8 == 0 && d->act_choff + d->C <= d->act_ld &&
                          (d->act_pad == 0 || d->act_pad == 1),
                      "bn_act_bwd: activation slice [%d, %d) does not fit act_ld %d", d->act_choff, d->act_choff + d->C, d->act_ld);
        MCAMD_REQUIRE(d->slope > 0.f, "bn_act_bwd: `act` needs an invertible activation (slope > 0)");
        MCAMD_REQUIRE(!d->y || d->y_dtype == 1, "bn_act_bwd: with `act`, `y` is NULL or the fp32 raw output (read for the "
                                                "channels with |gamma| < %g max(|beta|, 1) only)", (double)BN_ACT_T);
    }
    // MCAMD_BN_POOL_SUMS_POOLED=0: the sums of a MaxPool block from the full-resolution copy although pool_out is given
    a.pool_out = MCAMD_ENV_INT("MCAMD_BN_POOL_SUMS_POOLED", 1) != 0 ? (const half_t*)d->pool_out : nullptr;
    a.pool_out_ld = d->pool_out_ld, a.pool_out_choff = d->pool_out_choff;
    a.pool_out_pw = d->pool_out_pad ? 1 : 2;
    if (d->pool_out) {
        MCAMD_REQUIRE(d->mode == MCAMD_DST_POOL && !d->g2 && (d->act || (d->y && y32)) && d->slope > 0.f,
                      "bn_act_bwd: `pool_out` (sums from the pooled activation) is for MaxPool blocks without a second gradient, "
                      "with `act` or an fp32 `y`, and an invertible activation (slope > 0)");
        MCAMD_REQUIRE(d->pool_out_ld % 8 == 0 && d->pool_out_choff % 8 == 0 && d->pool_out_choff + d->C <= d->pool_out_ld &&
                          (d->pool_out_pad == 0 || d->pool_out_pad == 1),
                      "bn_act_bwd: pooled activation slice [%d, %d) does not fit pool_out_ld %d", d->pool_out_choff,
                      d->pool_out_choff + d->C, d->pool_out_ld);
    }
    long long pixels = (long long)d->B * d->H * d->W;
    double count = (double)pixels;
    if (d->mode != MCAMD_DST_PLAIN) pixels /= 4;
    a.items = pixels * (d->C / 8);
    int grid = stream_grid(a.items);
    // MCAMD_BN_BWD_BLOCKS: fewer workgroups than the slab has rows (tests: the same sums in another summation order)
    const int max_blocks = MCAMD_ENV_INT("MCAMD_BN_BWD_BLOCKS", kBwdBlocks);
    if (grid > kBwdBlocks) grid = kBwdBlocks;
    if (max_blocks >= 1 && grid > max_blocks) grid = max_blocks;
    hipStream_t st = (hipStream_t)stream;
    // MaxPool blocks: the argmax form (bn_pool_bwd_kernel); MCAMD_BN_POOL_FAST=0: generic kernel
    const bool pool_fast_on = MCAMD_ENV_INT("MCAMD_BN_POOL_FAST", 1) != 0;
    const bool pool_fast = pool_fast_on && d->mode == MCAMD_DST_POOL && a.items < (1ll << 31) &&
                           (unsigned long long)grid * 256ull < (1ull << 31);
    // PLAIN blocks without a second gradient: bn_plain_bwd_kernel (MCAMD_BN_PLAIN_FAST=0: generic kernel)
    const bool plain_fast = MCAMD_ENV_INT("MCAMD_BN_PLAIN_FAST", 1) != 0 &&
                            d->mode == MCAMD_DST_PLAIN && !d->g2 && a.items < (1ll << 31) &&
                            (unsigned long long)grid * 256ull < (1ull << 31);
    MCAMD_REQUIRE(!d->act || plain_fast || pool_fast, "bn_act_bwd: `act` needs the plain / pool fast path (fewer than 2^31 items, "
                                                      "MCAMD_BN_POOL_FAST / MCAMD_BN_PLAIN_FAST not 0)");
    // sums already taken (mcamd_act_bwd_desc.sums: the dgrad launch that wrote G formed them, mcamd_conv_dgrad_sums): no pass 0
    const float* fin_slab = (const float*)a.slab;
    int fin_rows = grid, fin_ld = d->C;
    if (d->sums) {
        MCAMD_REQUIRE(plain_fast && a.act, "bn_act_bwd: `sums` is for PLAIN blocks without a second gradient, with `act`");
        MCAMD_REQUIRE(d->sums_rows > 0 && d->sums_ld >= d->C, "bn_act_bwd: sums_rows (%d) must be positive and sums_ld (%d) >= C",
                      d->sums_rows, d->sums_ld);
        fin_slab = d->sums, fin_rows = d->sums_rows, fin_ld = d->sums_ld;
    }
    const BwdRoute route = bwd_route(d->mode, y32, a.act != nullptr, d->g2 != nullptr, a.pool_out != nullptr, pool_fast, plain_fast);
    MCAMD_REQUIRE(route.pass0 && route.pass1, "bn_act_bwd: bad mode %d", d->mode);
    if (!d->sums) hipLaunchKernelGGL(route.pass0, dim3(grid), dim3(256), 0, st, a);   // (`sums`: pass 0 ran in that dgrad's epilogue)
    MCAMD_LAUNCH_CHECK("bn_act_bwd reduce");
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((d->C + RED_CPB - 1) / RED_CPB), dim3(1024), 0, st, fin_slab, fin_rows, fin_ld, d->C,
                       count, 1.0f / d->grad_scale, d->dgamma, d->dbeta, coef, (const int*)d->chan_perm,
                       d->skip_dead_param_grads);
    MCAMD_LAUNCH_CHECK("bn_act_bwd finalize");
    hipLaunchKernelGGL(route.pass1, dim3(grid), dim3(256), 0, st, a);
    MCAMD_LAUNCH_CHECK("bn_act_bwd apply");
    return MCAMD_OK;
}

extern "C" int mcamd_nchw_f32_to_padded_nhwc_f16(const float* src, int32_t B, int32_t C, int32_t H, int32_t W, float mul,
                                                 void* dst, int32_t dst_ld, int32_t dst_choff, int32_t* overflow,
                                                 void* stream) {
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* s) {
            return mcamd_nchw_f32_to_padded_nhwc_f16(src, B, C, H, W, mul, dst, dst_ld, dst_choff, overflow, s);
        });
    MCAMD_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0, "nchw_to_nhwc: bad argument");
    MCAMD_REQUIRE(dst_choff + C <= dst_ld || dst_ld == 4, "nchw_to_nhwc: channel slice exceeds ld");
    MCAMD_REQUIRE((C >= 8) ? (dst_ld % 8 == 0 && dst_choff % 8 == 0) : true, "nchw_to_nhwc: alignment");
    int cgroups = (C + 7) / 8;
    long long items = (long long)B * H * W * cgroups;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(stream_grid(items)), dim3(256), 0, (hipStream_t)stream, src, B, C, H, W,
                       mul, (half_t*)dst, dst_ld, dst_choff, cgroups, (int*)overflow, 0, 2);
    MCAMD_LAUNCH_CHECK("nchw_to_nhwc");
    return MCAMD_OK;
}

extern "C" int mcamd_nchw_f32_to_padded_nhwc_f16_pad(const float* src, int32_t B, int32_t C, int32_t H, int32_t W, float mul,
                                                     void* dst, int32_t dst_ld, int32_t dst_choff, int32_t pad,
                                                     int32_t* overflow, void* stream) {
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* s) {
            return mcamd_nchw_f32_to_padded_nhwc_f16_pad(src, B, C, H, W, mul, dst, dst_ld, dst_choff, pad, overflow, s);
        });
    MCAMD_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && (pad == 0 || pad == 1), "nchw_to_nhwc_pad: bad argument");
    MCAMD_REQUIRE(dst_choff + C <= dst_ld && dst_ld != 4, "nchw_to_nhwc_pad: channel slice exceeds ld (and not the stem image)");
    MCAMD_REQUIRE((C >= 8) ? (dst_ld % 8 == 0 && dst_choff % 8 == 0) : true, "nchw_to_nhwc_pad: alignment");
    int cgroups = (C + 7) / 8;
    long long items = (long long)B * H * W * cgroups;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(stream_grid(items)), dim3(256), 0, (hipStream_t)stream, src, B, C, H, W,
                       mul, (half_t*)dst, dst_ld, dst_choff, cgroups, (int*)overflow, 0, pad ? 1 : 2);
    MCAMD_LAUNCH_CHECK("nchw_to_nhwc_pad");
    return MCAMD_OK;
}

extern "C" int mcamd_nchw_f32_to_padded_nhwc_f16_split(const float* src, int32_t B, int32_t C, int32_t H, int32_t W,
                                                       void* dst, int32_t dst_ld, int32_t dst_choff, int32_t plane,
                                                       void* stream) {
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* s) {
            return mcamd_nchw_f32_to_padded_nhwc_f16_split(src, B, C, H, W, dst, dst_ld, dst_choff, plane, s);
        });
    MCAMD_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0, "nchw_to_nhwc_split: bad argument");
    MCAMD_REQUIRE(plane >= C && dst_choff + 2 * plane + C <= dst_ld, "nchw_to_nhwc_split: three planes of %d channels, %d apart, exceed ld %d",
                  C, plane, dst_ld);
    int cgroups = (C + 7) / 8;
    long long items = (long long)B * H * W * cgroups;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(stream_grid(items)), dim3(256), 0, (hipStream_t)stream, src, B, C, H, W,
                       1.0f, (half_t*)dst, dst_ld, dst_choff, cgroups, (int*)nullptr, plane, 2);
    MCAMD_LAUNCH_CHECK("nchw_to_nhwc_split");
    return MCAMD_OK;
}
