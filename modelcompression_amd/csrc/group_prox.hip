// Proximal group lasso (sparsify.GroupLasso, include/mcamd.h) for gfx950, wave64: the shrink-or-zero step
// behind optimizer.step() for every block of every conv weight and every BatchNorm gate of a model, in ONE launch over a
// segment table.
//
// Workgroups of 512 threads; a segment owns a run of them (mcamd_gprox_seg.wg0):
//   block items   one per (filter block, channel block) pair of a BLOCK segment, over all taps.  The filter rows of the pair
//                 (kb * khw consecutive floats each) are read with coalesced loads into REGISTERS, all loads issued up front;
//                 then rounds of 8 rows (64 when khw = 1) go through LDS, where wave v sums the squares of taps v and v + 8 in
//                 the header's lane order (lane stride khw words: 1 or 9, conflict-free).  When the last round is summed the
//                 nine scales go through LDS and every thread writes its registers back scaled: one read and one write of each
//                 weight, no second pass over HBM.  A 64 x 64 x 9 pair is 144 KiB, more than a workgroup's LDS; it is 72
//                 registers per thread.
//                 khw other than 1 and 9 takes the direct form: wave v sums tap v, v + 8, ... from memory and rewrites it.
//   gate items    one per 512 channels of a GATE segment
// No atomics: every weight, gamma and flag has one owner, so the result depends on the operands only.  The arithmetic is
// pinned in the header (-ffp-contract=off).  Plain C++ loads and stores, 4-byte alignment; a pair's base is a 64-bit element
// offset, the elements behind it take 32-bit ones (64 filter rows stay below 2^31 weights: checked on the host).
#include "common.h"

namespace {
constexpr int GP_T = 512;
constexpr int GP_WAVES = GP_T / 64;
constexpr int GP_TAPS = 2;              // taps one wave sums in the staged form: khw <= 16
constexpr int GP_GATE = GP_T;            // channels per gate item

__host__ __device__ inline long long gp_items(const mcamd_gprox_seg& g) {
    if (g.kind == MCAMD_GPROX_GATE) return ((long long)g.cout + GP_GATE - 1) / GP_GATE;
    return (long long)((g.cout + 63) / 64) * (g.cin / (g.cin % 64 == 0 ? 64 : 32));
}

__device__ __forceinline__ double gp_butterfly(double s) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

// The scale of one block from its sum of squares; < 0 stands for "every element becomes +0.0f" (s itself is never negative:
// thr2 / n2 <= 1 there and the float64 square root is correctly rounded, so it does not exceed 1; a NaN is not < 0 either).
__device__ __forceinline__ double gp_scale(double n2, double tau2, int n_g) {
    const double thr2 = tau2 * (double)n_g;
    if (n2 <= thr2) return -1.0;
    return 1.0 - sqrt(thr2 / n2);
}

__device__ __forceinline__ float gp_apply(float w, double s) { return s < 0.0 ? 0.0f : (float)((double)w * s); }

// The staged form.  KB channels, KHW taps (at most 16: two per wave), R rows per round; R * KB is a multiple of 64.
template <int KB, int KHW, int R>
__device__ void gp_block_item(const mcamd_gprox_seg& g, int pair, double tau2, float* lds, double* sc) {
    constexpr int ROWLEN = KB * KHW;                   // consecutive floats of one filter row inside the pair
    constexpr int CHUNK = R * ROWLEN;
    constexpr int PER = (CHUNK + GP_T - 1) / GP_T;     // registers one round fills
    constexpr int ROUNDS = 64 / R;
    constexpr int STEPS = R * KB / 64;                 // lane steps (e += 64) one round of rows covers
    static_assert(KHW <= GP_WAVES * GP_TAPS && (R * KB) % 64 == 0 && 64 % R == 0, "gp_block_item: shape");
    const int cin = g.cin, cout = g.cout;
    const int ncb = cin / KB;
    const int fb = pair / ncb, cb = pair - fb * ncb;
    const int rows = cout - 64 * fb < 64 ? cout - 64 * fb : 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row_stride = cin * KHW;                  // 63 of them fit an int: checked on the host
    // element (r = 0, c = 0, tap = 0) of the pair; everything behind it is addressed with 32-bit offsets
    float* __restrict__ w = (float*)g.w + ((long long)(64 * fb) * cin + (long long)cb * KB) * KHW;
    float v[ROUNDS * PER];
    double s[GP_TAPS] = {0.0, 0.0};
    // every load of the pair is issued before the first sum: the whole pair (up to 144 KiB) is in flight at once, and the rounds
    // below start as their rows arrive
#pragma unroll
    for (int q = 0; q < ROUNDS; ++q) {
        const int row0 = q * R;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + j * GP_T;
            const int r = i / ROWLEN;
            v[q * PER + j] = (i < CHUNK && row0 + r < rows) ? w[(row0 + r) * row_stride + (i - r * ROWLEN)] : 0.f;
        }
    }
    // two LDS images, one barrier per round: round q + 1 writes the image round q - 1 was summed from, and everybody has
    // left that sum before anybody passes round q's barrier
#pragma unroll
    for (int q = 0; q < ROUNDS; ++q) {
        const int row0 = q * R;
        if (row0 < rows) {                             // uniform over the workgroup
            float* img = lds + (ROUNDS > 1 ? (q & 1) * CHUNK : 0);
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int i = tid + j * GP_T;
                if (i < CHUNK) img[i] = v[q * PER + j];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < STEPS; ++j) {
                const int el = lane + 64 * j;          // e - row0 * KB
                const int r = el / KB, c = el - r * KB;
                if (row0 + r < rows) {
#pragma unroll
                    for (int t = 0; t < GP_TAPS; ++t) {
                        const int tap = wave + GP_WAVES * t;
                        if (tap < KHW) {
                            const double x = (double)img[r * ROWLEN + c * KHW + tap];
                            s[t] += x * x;
                        }
                    }
                }
            }
        }
    }
    int* nz = (int*)g.nz;
#pragma unroll
    for (int t = 0; t < GP_TAPS; ++t) {
        const int tap = wave + GP_WAVES * t;
        if (tap < KHW) {                               // wave-uniform
            const double scale = gp_scale(gp_butterfly(s[t]), tau2, rows * KB);
            if (lane == 0) {
                sc[tap] = scale;
                if (nz) nz[(long long)pair * KHW + tap] = scale < 0.0 ? 0 : 1;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ROUNDS; ++q) {
        const int row0 = q * R;
        if (row0 < rows) {
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int i = tid + j * GP_T;
                const int r = i / ROWLEN;
                if (i < CHUNK && row0 + r < rows) {
                    const int off = i - r * ROWLEN;
                    w[(row0 + r) * row_stride + off] = gp_apply(v[q * PER + j], sc[off % KHW]);
                }
            }
        }
    }
}

// The direct form, any khw: every element belongs to one tap, so a tap's wave is the only reader and writer of its block.
__device__ void gp_block_direct(const mcamd_gprox_seg& g, int pair, double tau2) {
    float* w = (float*)g.w;
    int* nz = (int*)g.nz;
    const int cin = g.cin, khw = g.khw, cout = g.cout;
    const int kb = cin % 64 == 0 ? 64 : 32, ncb = cin / kb;
    const int fb = pair / ncb, cb = pair - fb * ncb;
    const int rows = cout - 64 * fb < 64 ? cout - 64 * fb : 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row_stride = (long long)cin * khw;
    const long long base = ((long long)(64 * fb) * cin + (long long)cb * kb) * khw;
    const int n = rows * kb;
    for (int tap = wave; tap < khw; tap += GP_WAVES) {
        double s = 0.0;
        for (int e = lane; e < n; e += 64) {
            const int r = e / kb, c = e - r * kb;
            const double x = (double)w[base + r * row_stride + (long long)c * khw + tap];
            s += x * x;
        }
        const double scale = gp_scale(gp_butterfly(s), tau2, n);
        for (int e = lane; e < n; e += 64) {
            const int r = e / kb, c = e - r * kb;
            const long long idx = base + r * row_stride + (long long)c * khw + tap;
            w[idx] = gp_apply(w[idx], scale);
        }
        if (lane == 0 && nz) nz[(long long)pair * khw + tap] = scale < 0.0 ? 0 : 1;
    }
}

__device__ void gp_gate_item(const mcamd_gprox_seg& g, long long item, float tau_gate) {
    const long long c = item * GP_GATE + threadIdx.x;
    if (c >= g.cout) return;
    float* gamma = (float*)g.w;
    int* nz = (int*)g.nz;
    const float x = gamma[c];
    const float a = fabsf(x) - tau_gate;
    int flag = 1;                                      // a NaN gamma is left alone: it is not zero
    if (a > 0.f) {
        gamma[c] = copysignf(a, x);
    } else if (a <= 0.f) {
        gamma[c] = 0.0f;
        flag = 0;
    }
    if (nz) nz[c] = flag;
}

constexpr int GP_LDS = 2 * 8 * 64 * 9;                 // floats: two images of the largest round, 8 rows x 64 x 9 (64 rows x 64 x 1 is 4096)

__global__ __launch_bounds__(GP_T) void group_prox_kernel(const mcamd_gprox_seg* __restrict__ segs, int nseg, double tau2,
                                                          float tau_gate, const float* __restrict__ skip) {
    __shared__ float lds[GP_LDS];
    __shared__ double sc[GP_WAVES * GP_TAPS];
    if (skip && *skip != 0.f) return;                  // uniform over the grid: nobody writes *skip
    const long long b = blockIdx.x;
    int si = 0;
    while (si + 1 < nseg && b >= segs[si + 1].wg0) ++si;
    const mcamd_gprox_seg g = segs[si];
    const long long item = b - g.wg0;
    if (item >= gp_items(g)) return;
    if (g.kind == MCAMD_GPROX_GATE) {
        gp_gate_item(g, item, tau_gate);
        return;
    }
    const bool wide = g.cin % 64 == 0;
    if (g.khw == 9) {
        if (wide) gp_block_item<64, 9, 8>(g, (int)item, tau2, lds, sc);
        else gp_block_item<32, 9, 8>(g, (int)item, tau2, lds, sc);
    } else if (g.khw == 1) {
        if (wide) gp_block_item<64, 1, 64>(g, (int)item, tau2, lds, sc);
        else gp_block_item<32, 1, 64>(g, (int)item, tau2, lds, sc);
    } else {
        gp_block_direct(g, (int)item, tau2);
    }
}

inline bool gp_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
}  // namespace

extern "C" int64_t mcamd_gprox_seg_workgroups(const mcamd_gprox_seg* seg) {
    if (!seg || seg->cout <= 0 || seg->cin <= 0 || seg->khw <= 0) return 0;
    if (seg->kind != MCAMD_GPROX_BLOCK && seg->kind != MCAMD_GPROX_GATE) return 0;
    if (seg->kind == MCAMD_GPROX_BLOCK && seg->cin % 32 != 0) return 0;
    if (seg->kind == MCAMD_GPROX_GATE && (seg->cin != 1 || seg->khw != 1)) return 0;
    return gp_items(*seg);
}

extern "C" int mcamd_group_prox(const mcamd_gprox_seg* segs, const mcamd_gprox_seg* segs_dev, int32_t nseg, double tau2,
                                float tau_gate, const float* skip, void* stream) {
    MCAMD_REQUIRE(segs && segs_dev && nseg > 0, "group_prox: null argument");
    MCAMD_REQUIRE(gp_aligned(segs_dev, 8) && gp_aligned(skip, 4), "group_prox: misaligned argument");
    MCAMD_REQUIRE(tau2 >= 0.0 && tau2 <= 1.7976931348623157e308, "group_prox: tau2 must be finite and not negative (got %g)", tau2);
    MCAMD_REQUIRE(tau_gate >= 0.f && tau_gate <= 3.4028234663852886e38f,
                  "group_prox: tau_gate must be finite and not negative (got %g)", (double)tau_gate);
    long long wgs = 0;
    for (int s = 0; s < nseg; ++s) {
        const mcamd_gprox_seg& g = segs[s];
        MCAMD_REQUIRE(g.kind == MCAMD_GPROX_BLOCK || g.kind == MCAMD_GPROX_GATE, "group_prox: segment %d: unknown kind %d", s, g.kind);
        MCAMD_REQUIRE(g.cout > 0 && g.cin > 0 && g.khw > 0, "group_prox: segment %d: bad shape [%d][%d][%d]", s, g.cout, g.cin, g.khw);
        MCAMD_REQUIRE(g.w, "group_prox: segment %d: null tensor", s);
        MCAMD_REQUIRE(gp_aligned(g.w, 4) && gp_aligned(g.nz, 4), "group_prox: segment %d: arrays must be 4-byte aligned", s);
        if (g.kind == MCAMD_GPROX_GATE) {
            MCAMD_REQUIRE(g.cin == 1 && g.khw == 1, "group_prox: segment %d: a gate is [C][1][1]", s);
        } else {
            MCAMD_REQUIRE(g.cin % 32 == 0, "group_prox: segment %d: blocks need cin %% 32 == 0 (cin %d)", s, g.cin);
            MCAMD_REQUIRE((long long)g.cout * g.cin * g.khw < (1ll << 40), "group_prox: segment %d: too many weights", s);
            MCAMD_REQUIRE(64ll * g.cin * g.khw < (1ll << 31), "group_prox: segment %d: 64 filter rows must stay below 2^31 weights", s);
        }
        MCAMD_REQUIRE(g.wg0 == wgs, "group_prox: segment %d: wg0 %lld is not the running sum %lld", s, (long long)g.wg0, wgs);
        wgs += gp_items(g);
        MCAMD_REQUIRE(wgs < (1ll << 31), "group_prox: too many workgroups");
    }
    const dim3 grid((unsigned)wgs);
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* st) {
            hipLaunchKernelGGL(group_prox_kernel, grid, dim3(GP_T), 0, (hipStream_t)st, segs_dev, nseg, tau2, tau_gate, skip);
            return MCAMD_OK;
        });
    hipLaunchKernelGGL(group_prox_kernel, grid, dim3(GP_T), 0, (hipStream_t)stream, segs_dev, nseg, tau2, tau_gate, skip);
    MCAMD_LAUNCH_CHECK("group_prox");
    return MCAMD_OK;
}
