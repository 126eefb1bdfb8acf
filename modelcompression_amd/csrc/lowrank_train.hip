// Factor SGD (lowrank.FactorSGD, include/mcamd.h) for gfx950, wave64: behind optimizer.step() the dense weight
// gradient G of every factored block goes onto its factors (aU = V^T G, aV = G U^T), the factors take a momentum-SGD step and
// W = V U is recomposed -- three launches over one segment table, each grouped over all blocks by a tile map.
//
// One fp32 GEMM core (lt_gemm) serves the three products.  A workgroup of 256 threads owns a 64 x 64 output tile; each of its
// four waves owns a 32 x 32 accumulator of v_mfma_f32_32x32x2_f32 (16 VGPRs).  The reduction is staged through LDS in chunks
// of 32 steps, two stages (32 KiB): 16-byte global loads of chunk i + 1 are issued into registers in front of the 16 MFMAs of
// chunk i and written to the other stage behind them, one barrier per chunk.  Every reduction length here (cout, r, a K slice)
// is a multiple of 32, so a chunk is never ragged; M and N are multiples of 32, rows past them are staged as zeros and not
// stored.
//
// LDS layout of an operand stage: [k][64] floats, element (k, m) at  k * 64 + (((m + 8 (k >> 2)) & 63) ^ ((k & 1) << 5)).
//   read   lanes 0-31 of a wave read 32 consecutive m of row k = 2 kk, lanes 32-63 the same m of row 2 kk + 1: the rotation is
//          equal for both rows, the XOR sends the second row to the other 32 banks -- 64 lanes, 64 banks.
//   write  the two staging variants differ only here.  An operand that is contiguous along m / n (V^T, G as B, U as B) is
//          loaded as rows of k and written with one ds_write_b128 per load (the rotation is a multiple of 8, the XOR of 32: four
//          consecutive m stay consecutive).  An operand that is contiguous along k (G as A, U^T, V) is loaded as float4 along k
//          and written as four ds_write_b32 to rows 4 kq .. 4 kq + 3: the 8 kq of a wave are rotated to 8 different groups of
//          8 banks, its 8 rows m fill a group -- 64 lanes, 64 banks again.
//
//   product  A (m, k)             B (k, n)            reduction
//   aU       V^T, along m         G, along n          cout          epilogue: gU, MU (U itself is left to the update launch:
//   aV       G, along k           U^T, along k        a slice of K            other tiles still read the old U and V)
//   W        V, along k           U, along n          r
// aV's output is small and its reduction long: K is cut into slices of MCAMD_LRSGD_SLICE, each tile writes its slab, and the
// update launch sums the slabs in slice order in front of the SGD arithmetic.  No atomics anywhere.
//
// Workgroups are dealt round-robin to the 8 XCDs; lt_logical hands XCD x the x-th eighth of the tile list, in order, and the
// tile lists run fastest over the tiles that share a panel of G (aU: the r tiles of a column panel; aV: the r tiles of a row
// panel of a slice), so a panel of G is read from HBM by one XCD, once.
#include "common.h"

namespace {
constexpr int LT_T = 256;
constexpr int LT_TILE = MCAMD_LRSGD_TILE;            // 64: also the row length of an LDS stage
constexpr int LT_BK = 32;
constexpr int LT_STAGE = LT_BK * LT_TILE;            // floats of one operand stage
constexpr int LT_LDS = 4 * LT_STAGE;                 // A and B, two stages
constexpr int LT_S = MCAMD_LRSGD_SLICE;
constexpr int LT_ITEM = MCAMD_LRSGD_ITEM;
static_assert(LT_TILE == 64 && LT_S % LT_BK == 0 && LT_ITEM == 4 * LT_T, "lowrank_train: tile constants");

__host__ __device__ inline int lt_div(int a, int b) { return (a + b - 1) / b; }

struct LtCounts { int slices, gu, grad, update, compose; long long ws; };
__host__ __device__ inline LtCounts lt_counts(int cout, int K, int r) {
    LtCounts c;
    const int ct = lt_div(cout, LT_TILE), kt = lt_div(K, LT_TILE), rt = lt_div(r, LT_TILE);
    c.slices = lt_div(K, LT_S);
    c.gu = rt * kt;
    c.grad = c.gu + ct * rt * c.slices;
    c.update = (r * K + cout * r) / LT_ITEM;           // both are multiples of 1024: r, K and cout are multiples of 32
    c.compose = ct * kt;
    c.ws = (long long)c.slices * cout * r;
    return c;
}

__device__ __forceinline__ int lt_idx(int k, int m) { return k * LT_TILE + (((m + 8 * (k >> 2)) & 63) ^ ((k & 1) << 5)); }

__device__ __forceinline__ float4 lt_ld4(const float* __restrict__ p, bool vec) {
    if (vec) return *(const float4*)p;
    return make_float4(p[0], p[1], p[2], p[3]);
}

// One chunk of an operand into registers: 64 rows (m or n) from row0, of which `rows` exist, x 32 reduction steps from k0.
// KC: element (m, k) is p[m * ld + k]; otherwise p[k * ld + m].
template <bool KC>
__device__ __forceinline__ void lt_load(const float* __restrict__ p, int ld, int row0, int rows, int k0, bool vec, float4 (&reg)[2]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (KC) {
            const int m = (t >> 3) + 32 * q, kq = t & 7;
            reg[q] = m < rows ? lt_ld4(p + (long long)(row0 + m) * ld + k0 + 4 * kq, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const int k = (t >> 4) + 16 * q, mq = t & 15;
            reg[q] = 4 * mq < rows ? lt_ld4(p + (long long)(k0 + k) * ld + row0 + 4 * mq, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

template <bool KC>
__device__ __forceinline__ void lt_store(float* __restrict__ stage, const float4 (&reg)[2]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (KC) {
            const int m = (t >> 3) + 32 * q, k = 4 * (t & 7);
            stage[lt_idx(k, m)] = reg[q].x;
            stage[lt_idx(k + 1, m)] = reg[q].y;
            stage[lt_idx(k + 2, m)] = reg[q].z;
            stage[lt_idx(k + 3, m)] = reg[q].w;
        } else {
            const int k = (t >> 4) + 16 * q, mq = t & 15;
            *(float4*)&stage[lt_idx(k, 4 * mq)] = reg[q];
        }
    }
}

// acc (this wave's 32 x 32 of the tile at (m0, n0)) = sum over `chunks` chunks of 32 steps from k0 of A (m, k) B (k, n).
template <bool AKC, bool BKC>
__device__ __forceinline__ f32x16_t lt_gemm(const float* __restrict__ A, int lda, bool avec, int m0, int M,
                                            const float* __restrict__ B, int ldb, bool bvec, int n0, int N,
                                            int k0, int chunks, float* __restrict__ lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int am = (wave & 1) * 32 + (lane & 31), bn = (wave >> 1) * 32 + (lane & 31), kh = lane >> 5;
    f32x16_t acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 ra[2], rb[2];
    lt_load<AKC>(A, lda, m0, M - m0, k0, avec, ra);
    lt_load<BKC>(B, ldb, n0, N - n0, k0, bvec, rb);
    lt_store<AKC>(lds, ra);
    lt_store<BKC>(lds + LT_STAGE, rb);
    __syncthreads();
    for (int c = 0; c < chunks; ++c) {
        const float* cur = lds + (c & 1) * 2 * LT_STAGE;
        float* nxt = lds + ((c + 1) & 1) * 2 * LT_STAGE;
        const bool more = c + 1 < chunks;              // uniform over the workgroup
        if (more) {                                    // in flight over the MFMAs below
            lt_load<AKC>(A, lda, m0, M - m0, k0 + (c + 1) * LT_BK, avec, ra);
            lt_load<BKC>(B, ldb, n0, N - n0, k0 + (c + 1) * LT_BK, bvec, rb);
        }
#pragma unroll
        for (int kk = 0; kk < LT_BK / 2; ++kk) {
            const int k = 2 * kk + kh;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[lt_idx(k, am)], cur[LT_STAGE + lt_idx(k, bn)], acc, 0, 0, 0);
        }
        if (more) {
            // the stage chunk c - 1 was read from: everybody left it before passing the barrier that ended chunk c - 1
            lt_store<AKC>(nxt, ra);
            lt_store<BKC>(nxt + LT_STAGE, rb);
        }
        __syncthreads();
    }
    return acc;
}

// XCD x takes the x-th eighth of the `total` tiles, in order.  False for the workgroups that pad the grid to a multiple of 8.
__device__ __forceinline__ bool lt_logical(int total, int& tile) {
    const int per = lt_div(total, 8);
    tile = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    return (int)(blockIdx.x >> 3) < per && tile < total;
}

template <int WHICH>   // 0: tile0_grad, 1: tile0_update, 2: tile0_compose
__device__ __forceinline__ mcamd_lrsgd_seg lt_find(const mcamd_lrsgd_seg* __restrict__ segs, int nseg, int tile, int& local) {
    auto first = [&](int i) { return WHICH == 0 ? segs[i].tile0_grad : WHICH == 1 ? segs[i].tile0_update : segs[i].tile0_compose; };
    int si = 0;
    while (si + 1 < nseg && tile >= first(si + 1)) ++si;
    local = tile - first(si);
    return segs[si];
}

__device__ __forceinline__ bool lt_vec(const void* p) { return ((uintptr_t)p & 15) == 0; }

// this lane's element `reg` of the wave's accumulator: row and column inside the tile
__device__ __forceinline__ int lt_row(int reg) { return ((threadIdx.x >> 6) & 1) * 32 + mfma32_row(reg, threadIdx.x & 63); }
__device__ __forceinline__ int lt_col() { return (threadIdx.x >> 7) * 32 + (threadIdx.x & 31); }

__global__ __launch_bounds__(LT_T) void lowrank_sgd_grad_kernel(const mcamd_lrsgd_seg* __restrict__ segs, int nseg, int total,
                                                                 float mom, float wd, const float* __restrict__ skip,
                                                                 float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float lds[LT_LDS];
    if (skip && *skip != 0.f) return;                  // uniform over the grid: nobody writes *skip
    int tile, t;
    if (!lt_logical(total, tile)) return;
    const mcamd_lrsgd_seg s = lt_find<0>(segs, nseg, tile, t);
    const int cout = s.cout, K = s.K, r = s.r;
    const int rt = lt_div(r, LT_TILE), ct = lt_div(cout, LT_TILE);
    const float* G = (const float*)s.g;
    const bool gvec = lt_vec(G);
    const int ngu = rt * lt_div(K, LT_TILE);
    if (t < ngu) {
        // aU [r][K] = V^T G; the r tiles of one column panel of G are neighbours
        const int m0 = (t % rt) * LT_TILE, n0 = (t / rt) * LT_TILE;
        const f32x16_t acc = lt_gemm<false, false>((const float*)s.v, r, true, m0, r, G, K, gvec, n0, K, 0, cout / LT_BK, lds);
        const float* __restrict__ U = (const float*)s.u;
        float* __restrict__ MU = (float*)s.mu;
        const int col = n0 + lt_col();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = m0 + lt_row(i);
            if (row < r && col < K) {
                const int e = row * K + col;
                MU[e] = __fmaf_rn(mom, MU[e], __fmaf_rn(wd, U[e], acc[i]));
            }
        }
    } else {
        // one slab of aV [cout][r] = G U^T; the r tiles of one row panel of a slice of G are neighbours
        t -= ngu;
        const int n0 = (t % rt) * LT_TILE;
        t /= rt;
        const int m0 = (t % ct) * LT_TILE, sl = t / ct;
        const int k0 = sl * LT_S, len = K - k0 < LT_S ? K - k0 : LT_S;
        const f32x16_t acc = lt_gemm<true, true>(G, K, gvec, m0, cout, (const float*)s.u, K, true, n0, r, k0, len / LT_BK, lds);
        float* __restrict__ slab = ws + s.ws0 + (long long)sl * cout * r;
        const int col = n0 + lt_col();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = m0 + lt_row(i);
            if (row < cout && col < r) slab[row * r + col] = acc[i];
        }
    }
}

__device__ __forceinline__ float4 lt_fma4(float a, float4 x, float4 y) {
    return make_float4(__fmaf_rn(a, x.x, y.x), __fmaf_rn(a, x.y, y.y), __fmaf_rn(a, x.z, y.z), __fmaf_rn(a, x.w, y.w));
}

// One item is 1024 consecutive elements of U (first) or of V; a thread owns four.
__global__ __launch_bounds__(LT_T) void lowrank_sgd_update_kernel(const mcamd_lrsgd_seg* __restrict__ segs, int nseg, float lr,
                                                                   float mom, float wd, const float* __restrict__ skip,
                                                                   const float* __restrict__ ws) {
    if (skip && *skip != 0.f) return;
    int t;
    const mcamd_lrsgd_seg s = lt_find<1>(segs, nseg, (int)blockIdx.x, t);
    const int nu = s.r * s.K / LT_ITEM;
    if (t < nu) {
        const int e = t * LT_ITEM + 4 * threadIdx.x;
        float4* U = (float4*)((float*)s.u + e);
        *U = lt_fma4(-lr, *(const float4*)((const float*)s.mu + e), *U);
    } else {
        const int e = (t - nu) * LT_ITEM + 4 * threadIdx.x;
        const int n = s.cout * s.r, slices = lt_div(s.K, LT_S);
        const float* slab = ws + s.ws0 + e;
        float4 a = *(const float4*)slab;
        for (int sl = 1; sl < slices; ++sl) {
            const float4 b = *(const float4*)(slab + (long long)sl * n);
            a = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        }
        float4* V = (float4*)((float*)s.v + e);
        float4* MV = (float4*)((float*)s.mv + e);
        const float4 v = *V;
        const float4 m = lt_fma4(mom, *MV, lt_fma4(wd, v, a));
        *MV = m;
        *V = lt_fma4(-lr, m, v);
    }
}

__global__ __launch_bounds__(LT_T) void lowrank_sgd_compose_kernel(const mcamd_lrsgd_seg* __restrict__ segs, int nseg, int total,
                                                                    const float* __restrict__ skip) {
    __shared__ __attribute__((aligned(16))) float lds[LT_LDS];
    if (skip && *skip != 0.f) return;
    int tile, t;
    if (!lt_logical(total, tile)) return;
    const mcamd_lrsgd_seg s = lt_find<2>(segs, nseg, tile, t);
    const int cout = s.cout, K = s.K, r = s.r;
    const int ct = lt_div(cout, LT_TILE);
    // W [cout][K] = V U; the cout tiles of one column panel of U are neighbours
    const int m0 = (t % ct) * LT_TILE, n0 = (t / ct) * LT_TILE;
    const f32x16_t acc = lt_gemm<true, false>((const float*)s.v, r, true, m0, cout, (const float*)s.u, K, true, n0, K, 0, r / LT_BK, lds);
    float* __restrict__ W = (float*)s.w;
    const int col = n0 + lt_col();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = m0 + lt_row(i);
        if (row < cout && col < K) W[row * K + col] = acc[i];
    }
}

inline bool lt_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// MCAMD_OK when the shape is accepted, else the refusal, the dimension by name
int lt_refuse(int cout, int K, int r) {
    MCAMD_REQUIRE(r >= 32 && r <= 256 && r % 32 == 0, "lowrank_sgd: rank r must be a multiple of 32 in [32, 256] (r %d)", r);
    MCAMD_REQUIRE(cout > 0 && cout % 32 == 0, "lowrank_sgd: Cout must be a positive multiple of 32 (Cout %d)", cout);
    MCAMD_REQUIRE(K > 0 && K % 32 == 0, "lowrank_sgd: K = Cin k k must be a positive multiple of 32 (K %d)", K);
    MCAMD_REQUIRE((long long)cout * K < (1ll << 31), "lowrank_sgd: Cout K must stay below 2^31 (Cout %d, K %d)", cout, K);
    return MCAMD_OK;
}
}  // namespace

extern "C" int32_t mcamd_lowrank_sgd_ok(int32_t cout, int32_t K, int32_t r) { return lt_refuse(cout, K, r) == MCAMD_OK ? 1 : 0; }

extern "C" int mcamd_lowrank_sgd_info(int32_t cout, int32_t K, int32_t r, mcamd_lrsgd_info* info) {
    MCAMD_REQUIRE(info, "lowrank_sgd: null argument");
    const int rc = lt_refuse(cout, K, r);
    if (rc != MCAMD_OK) return rc;
    const LtCounts c = lt_counts(cout, K, r);
    *info = mcamd_lrsgd_info{LT_TILE, LT_BK, LT_S, c.slices, LT_T, (int32_t)(LT_LDS * sizeof(float)),
                             c.grad, c.update, c.compose, 0, c.ws * (long long)sizeof(float)};
    return MCAMD_OK;
}

extern "C" int mcamd_lowrank_sgd(const mcamd_lrsgd_seg* segs, const mcamd_lrsgd_seg* segs_dev, int32_t nseg, float lr, float mom,
                                 float wd, const float* skip, void* workspace, size_t workspace_bytes, void* stream) {
    MCAMD_REQUIRE(segs && segs_dev && nseg > 0 && workspace, "lowrank_sgd: null argument");
    MCAMD_REQUIRE(lt_aligned(segs_dev, 8) && lt_aligned(skip, 4) && lt_aligned(workspace, 16), "lowrank_sgd: misaligned argument");
    MCAMD_REQUIRE(lr - lr == 0.f && mom - mom == 0.f && wd - wd == 0.f, "lowrank_sgd: lr, mom and wd must be finite (got %g, %g, %g)",
                  (double)lr, (double)mom, (double)wd);
    long long grad = 0, update = 0, compose = 0, ws = 0;
    for (int i = 0; i < nseg; ++i) {
        const mcamd_lrsgd_seg& s = segs[i];
        const int rc = lt_refuse(s.cout, s.K, s.r);
        if (rc != MCAMD_OK) return rc;
        MCAMD_REQUIRE(s.g && s.u && s.v && s.mu && s.mv && s.w, "lowrank_sgd: segment %d: null tensor", i);
        MCAMD_REQUIRE(lt_aligned(s.g, 4) && lt_aligned(s.u, 16) && lt_aligned(s.v, 16) && lt_aligned(s.mu, 16) && lt_aligned(s.mv, 16) &&
                      lt_aligned(s.w, 16), "lowrank_sgd: segment %d: g must be 4-byte aligned, every other tensor 16-byte aligned", i);
        MCAMD_REQUIRE(s.tile0_grad == grad && s.tile0_update == update && s.tile0_compose == compose && s.ws0 == ws,
                      "lowrank_sgd: segment %d: offsets (%d, %d, %d, %lld) are not the running sums (%lld, %lld, %lld, %lld)", i,
                      s.tile0_grad, s.tile0_update, s.tile0_compose, (long long)s.ws0, grad, update, compose, ws);
        const LtCounts c = lt_counts(s.cout, s.K, s.r);
        grad += c.grad, update += c.update, compose += c.compose, ws += c.ws;
        MCAMD_REQUIRE(grad < (1ll << 30) && update < (1ll << 30) && compose < (1ll << 30), "lowrank_sgd: too many workgroups");
    }
    MCAMD_REQUIRE((unsigned long long)ws * sizeof(float) <= workspace_bytes, "lowrank_sgd: workspace of %zu bytes, %lld needed",
                  workspace_bytes, ws * (long long)sizeof(float));
    const int tg = (int)grad, tu = (int)update, tc = (int)compose;
    float* wsp = (float*)workspace;
    auto launch = [=](void* st) {
        hipLaunchKernelGGL(lowrank_sgd_grad_kernel, dim3(round_up_int(tg, 8)), dim3(LT_T), 0, (hipStream_t)st, segs_dev, nseg, tg, mom, wd,
                           skip, wsp);
        hipLaunchKernelGGL(lowrank_sgd_update_kernel, dim3(tu), dim3(LT_T), 0, (hipStream_t)st, segs_dev, nseg, lr, mom, wd, skip, wsp);
        hipLaunchKernelGGL(lowrank_sgd_compose_kernel, dim3(round_up_int(tc, 8)), dim3(LT_T), 0, (hipStream_t)st, segs_dev, nseg, tc, skip);
        return MCAMD_OK;
    };
    if (mcamd_recording()) return mcamd_rec_push(stream, launch);
    launch(stream);
    MCAMD_LAUNCH_CHECK("lowrank_sgd");
    return MCAMD_OK;
}
