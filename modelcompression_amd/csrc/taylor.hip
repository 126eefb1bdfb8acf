// First-order Taylor importance (taylor_prune, include/mcamd.h) for gfx950, wave64: the per-step accumulation
// of (g w)^2 per weight, (sum over a block of g w)^2 per block and per filter, and (gamma dgamma + beta dbeta)^2 per BatchNorm
// channel, for every layer of a model in ONE launch over a segment table.
//
// Workgroups of 256 threads; a segment owns a run of them (mcamd_taylor_seg.wg0), in this order:
//   block items    one per (filter block, channel block) pair of a conv segment with acc_b.  Four filter rows of the pair
//                  (kb * khw consecutive floats each) are read with coalesced loads, p = g * w goes to LDS and -- with acc_w --
//                  acc_w is updated on the way; then wave v sums taps v, v + 4, v + 8 from LDS in the header's lane order
//                  (lane stride khw words: 1 or 9, conflict-free).  khw > 9 takes the direct form of block_scores_kernel.
//   element items  one per 2048 weights of a conv segment with acc_w and without acc_b
//   filter items   one per 4 filters of a conv segment with acc_f, one wave per filter
//   gate items     one per 256 channels of a gate segment
// No atomics: every accumulator entry has one owner, so the result depends on the operands only.  The arithmetic is pinned
// in the header (-ffp-contract=off).  Plain C++ loads and stores; fp32 pointers need 4-byte alignment only, because a
// gradient is a view into the engine's flat buffer.  64-bit element offsets.
#include "common.h"

namespace {
constexpr int TY_T = 256;
constexpr int TY_ELEMS = 2048;          // weights per element item
constexpr int TY_ROWS = 4;              // filter rows staged per round of a block item: 4 * kb is a multiple of 64
constexpr int TY_FAST_KHW = 9;          // taps the staged form holds (3 per wave)
constexpr int TY_GATE = 256;            // channels per gate item

struct TyCounts {
    long long blocks, elems, filters, gates;
    long long total() const { return blocks + elems + filters + gates; }
};

__host__ __device__ inline TyCounts ty_counts(const mcamd_taylor_seg& g) {
    TyCounts c = {0, 0, 0, 0};
    if (g.kind == MCAMD_TAYLOR_GATE) {
        c.gates = ((long long)g.cout + TY_GATE - 1) / TY_GATE;
        return c;
    }
    const long long n = (long long)g.cout * g.cin * g.khw;
    if (g.acc_b) c.blocks = (long long)((g.cout + 63) / 64) * (g.cin / (g.cin % 64 == 0 ? 64 : 32));
    else if (g.acc_w) c.elems = (n + TY_ELEMS - 1) / TY_ELEMS;
    if (g.acc_f) c.filters = ((long long)g.cout + 3) / 4;
    return c;
}

__device__ __forceinline__ double ty_butterfly(double s) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

__device__ void ty_block_item(const mcamd_taylor_seg& g, int pair, float* lds) {
    const float* __restrict__ w = (const float*)g.w;
    const float* __restrict__ gr = (const float*)g.g;
    float* acc_w = (float*)g.acc_w;
    double* acc_b = (double*)g.acc_b;
    const int cin = g.cin, khw = g.khw, cout = g.cout;
    const int kb = cin % 64 == 0 ? 64 : 32, ncb = cin / kb;
    const int fb = pair / ncb, cb = pair - fb * ncb;
    const int rows = cout - 64 * fb < 64 ? cout - 64 * fb : 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row_stride = (long long)cin * khw;
    const long long base = ((long long)(64 * fb) * cin + (long long)cb * kb) * khw;      // element (r = 0, c = 0, tap = 0)
    if (khw > TY_FAST_KHW) {
        // direct form: wave v takes taps v, v + 4, ...; every element belongs to one tap, so acc_w has one writer too
        const int n = rows * kb;
        for (int tap = wave; tap < khw; tap += 4) {
            double s = 0.0;
            for (int e = lane; e < n; e += 64) {
                const int r = e / kb, c = e - r * kb;
                const long long idx = base + r * row_stride + (long long)c * khw + tap;
                const float p = gr[idx] * w[idx];
                if (acc_w) acc_w[idx] = acc_w[idx] + p * p;
                s += (double)p;
            }
            s = ty_butterfly(s);
            if (lane == 0) {
                const long long b = (long long)pair * khw + tap;
                acc_b[b] = acc_b[b] + s * s;
            }
        }
        return;
    }
    const int rowlen = kb * khw;                       // consecutive floats of one filter row inside the pair
    const int chunk = TY_ROWS * rowlen;                // <= 4 * 64 * 9 floats of LDS
    const int per_round = TY_ROWS * kb / 64;           // lane steps (e += 64) one round of rows covers: 4 or 2
    double s[3] = {0.0, 0.0, 0.0};
    for (int row0 = 0; row0 < rows; row0 += TY_ROWS) {
        for (int i = tid; i < chunk; i += TY_T) {
            const int r = (i >= rowlen) + (i >= 2 * rowlen) + (i >= 3 * rowlen);
            if (row0 + r < rows) {
                const long long idx = base + (row0 + r) * row_stride + (i - r * rowlen);
                const float p = gr[idx] * w[idx];
                if (acc_w) acc_w[idx] = acc_w[idx] + p * p;
                lds[i] = p;
            }
        }
        __syncthreads();
        for (int j = 0; j < per_round; ++j) {
            const int el = lane + 64 * j;              // e - row0 * kb
            const int r = el / kb, c = el - r * kb;
            if (row0 + r < rows) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int tap = wave + 4 * t;
                    if (tap < khw) s[t] += (double)lds[r * rowlen + c * khw + tap];
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int tap = wave + 4 * t;
        if (tap < khw) {                               // wave-uniform
            const double S = ty_butterfly(s[t]);
            if (lane == 0) {
                const long long b = (long long)pair * khw + tap;
                acc_b[b] = acc_b[b] + S * S;
            }
        }
    }
}

__device__ void ty_elem_item(const mcamd_taylor_seg& g, long long item) {
    const float* __restrict__ w = (const float*)g.w;
    const float* __restrict__ gr = (const float*)g.g;
    float* acc_w = (float*)g.acc_w;
    const long long n = (long long)g.cout * g.cin * g.khw;
    const long long i0 = item * TY_ELEMS + threadIdx.x;
#pragma unroll
    for (int j = 0; j < TY_ELEMS / TY_T; ++j) {
        const long long i = i0 + j * TY_T;
        if (i < n) {
            const float p = gr[i] * w[i];
            acc_w[i] = acc_w[i] + p * p;
        }
    }
}

__device__ void ty_filter_item(const mcamd_taylor_seg& g, long long item) {
    const int lane = threadIdx.x & 63;
    const long long f = item * 4 + (threadIdx.x >> 6);
    if (f >= g.cout) return;                           // wave-uniform
    const long long n = (long long)g.cin * g.khw;
    const float* __restrict__ w = (const float*)g.w + f * n;
    const float* __restrict__ gr = (const float*)g.g + f * n;
    double s = 0.0;
    for (long long e = lane; e < n; e += 64) {
        const float p = gr[e] * w[e];
        s += (double)p;
    }
    s = ty_butterfly(s);
    if (lane == 0) {
        if (g.bias) {
            const float pb = ((const float*)g.gbias)[f] * ((const float*)g.bias)[f];
            s += (double)pb;
        }
        double* acc_f = (double*)g.acc_f;
        acc_f[f] = acc_f[f] + s * s;
    }
}

__device__ void ty_gate_item(const mcamd_taylor_seg& g, long long item) {
    const long long c = item * TY_GATE + threadIdx.x;
    if (c >= g.cout) return;
    const double ga = (double)((const float*)g.w)[c], dga = (double)((const float*)g.g)[c];
    const double be = (double)((const float*)g.bias)[c], dbe = (double)((const float*)g.gbias)[c];
    const double a = ga * dga, b = be * dbe;           // exact: 24-bit x 24-bit
    const double t = a + b;
    double* acc_f = (double*)g.acc_f;
    acc_f[c] = acc_f[c] + t * t;
}

__global__ __launch_bounds__(TY_T) void taylor_accum_kernel(const mcamd_taylor_seg* __restrict__ segs, int nseg,
                                                            const float* __restrict__ skip, int* steps) {
    __shared__ float lds[TY_ROWS * 64 * TY_FAST_KHW];
    if (skip && *skip != 0.f) return;                  // uniform over the grid: nobody writes *skip
    const long long b = blockIdx.x;
    if (b == 0 && threadIdx.x == 0) *steps = *steps + 1;
    int si = 0;
    while (si + 1 < nseg && b >= segs[si + 1].wg0) ++si;
    const mcamd_taylor_seg g = segs[si];
    const TyCounts c = ty_counts(g);
    long long item = b - g.wg0;
    if (g.kind == MCAMD_TAYLOR_GATE) {
        if (item < c.gates) ty_gate_item(g, item);
        return;
    }
    if (item < c.blocks) {
        ty_block_item(g, (int)item, lds);
        return;
    }
    item -= c.blocks;
    if (item < c.elems) {
        ty_elem_item(g, item);
        return;
    }
    item -= c.elems;
    if (item < c.filters) ty_filter_item(g, item);
}

inline bool ty_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
}  // namespace

extern "C" int64_t mcamd_taylor_seg_workgroups(const mcamd_taylor_seg* seg) {
    if (!seg || seg->cout <= 0 || seg->cin <= 0 || seg->khw <= 0) return 0;
    if (seg->kind != MCAMD_TAYLOR_CONV && seg->kind != MCAMD_TAYLOR_GATE) return 0;
    if (seg->kind == MCAMD_TAYLOR_CONV && seg->acc_b && seg->cin % 32 != 0) return 0;
    return ty_counts(*seg).total();
}

extern "C" int mcamd_taylor_accum(const mcamd_taylor_seg* segs, const mcamd_taylor_seg* segs_dev, int32_t nseg, const float* skip,
                                  int32_t* steps, void* stream) {
    MCAMD_REQUIRE(segs && segs_dev && nseg > 0 && steps, "taylor_accum: null argument");
    MCAMD_REQUIRE(ty_aligned(segs_dev, 8) && ty_aligned(skip, 4) && ty_aligned(steps, 4), "taylor_accum: misaligned argument");
    long long wgs = 0;
    for (int s = 0; s < nseg; ++s) {
        const mcamd_taylor_seg& g = segs[s];
        MCAMD_REQUIRE(g.kind == MCAMD_TAYLOR_CONV || g.kind == MCAMD_TAYLOR_GATE, "taylor_accum: segment %d: unknown kind %d", s, g.kind);
        MCAMD_REQUIRE(g.cout > 0 && g.cin > 0 && g.khw > 0, "taylor_accum: segment %d: bad shape [%d][%d][%d]", s, g.cout, g.cin, g.khw);
        MCAMD_REQUIRE(g.w && g.g, "taylor_accum: segment %d: null tensor", s);
        MCAMD_REQUIRE(ty_aligned(g.w, 4) && ty_aligned(g.g, 4) && ty_aligned(g.bias, 4) && ty_aligned(g.gbias, 4) &&
                          ty_aligned(g.acc_w, 4) && ty_aligned(g.acc_b, 8) && ty_aligned(g.acc_f, 8),
                      "taylor_accum: segment %d: fp32 arrays must be 4-byte aligned, float64 arrays 8-byte aligned", s);
        if (g.kind == MCAMD_TAYLOR_GATE) {
            MCAMD_REQUIRE(g.bias && g.gbias && g.acc_f, "taylor_accum: segment %d: a gate needs beta, dbeta and acc_f", s);
            MCAMD_REQUIRE(!g.acc_w && !g.acc_b && g.cin == 1 && g.khw == 1,
                          "taylor_accum: segment %d: a gate is [C][1][1] and has filter scores only", s);
        } else {
            MCAMD_REQUIRE((g.bias != nullptr) == (g.gbias != nullptr), "taylor_accum: segment %d: a bias and its gradient go together", s);
            MCAMD_REQUIRE(g.acc_w || g.acc_b || g.acc_f, "taylor_accum: segment %d: no output", s);
            MCAMD_REQUIRE(!g.acc_b || g.cin % 32 == 0, "taylor_accum: segment %d: block scores need cin %% 32 == 0 (cin %d)", s, g.cin);
            MCAMD_REQUIRE((long long)g.cout * g.cin * g.khw < (1ll << 40), "taylor_accum: segment %d: too many weights", s);
        }
        MCAMD_REQUIRE(g.wg0 == wgs, "taylor_accum: segment %d: wg0 %lld is not the running sum %lld", s, (long long)g.wg0, wgs);
        wgs += ty_counts(g).total();
        MCAMD_REQUIRE(wgs < (1ll << 31), "taylor_accum: too many workgroups");
    }
    const dim3 grid((unsigned)wgs);
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* st) {
            hipLaunchKernelGGL(taylor_accum_kernel, grid, dim3(TY_T), 0, (hipStream_t)st, segs_dev, nseg, skip, steps);
            return MCAMD_OK;
        });
    hipLaunchKernelGGL(taylor_accum_kernel, grid, dim3(TY_T), 0, (hipStream_t)stream, segs_dev, nseg, skip, steps);
    MCAMD_LAUNCH_CHECK("taylor_accum");
    return MCAMD_OK;
}
