// Weight sharing (trained quantisation by k-means, include/mcamd.h) for gfx950, wave64: the Lloyd rounds over
// every layer of a model and the projection that keeps the weights tied during retraining.
//
// All layers go through one segment table.  A workgroup (256 threads) owns one slab of MCAMD_WS_SLAB consecutive weights
// of one layer: it reads them with 16-byte loads, stages (code, value) pairs in LDS, and thread k of sub-slab s adds the
// members of cluster k of that sub-slab in index order (a wave reads one LDS address at a time: a broadcast).  The slab
// sums go to the workspace and are added in slab order by one thread per cluster.  No atomics anywhere, so every result
// depends on the inputs only.  The arithmetic is pinned in the header: float64, no contraction (-ffp-contract=off).
// Plain C++ loads and stores throughout; 64-bit element offsets.
#include "common.h"

constexpr int WS_SLAB = MCAMD_WS_SLAB;
constexpr int WS_T = 256;
constexpr int WS_PER = WS_SLAB / WS_T;            // weights per thread
constexpr int WS_NONE = 256;                      // the staged code of a weight that is not kept (a code is < 256)
static_assert(WS_SLAB % (4 * WS_T) == 0, "a thread loads whole groups of 4 weights");

struct WsWork {          // the workspace (mcamd_ws_workspace_bytes)
    double* psum;        // [parts]      slab sums, layer by layer: [slab][K]
    float* range;        // [2 nslabs]   slab minimum and maximum of the kept weights
    unsigned* pcnt;      // [parts]      slab counts
};

static WsWork ws_work(void* ws, long long nslabs, long long parts) {
    WsWork k;
    k.psum = (double*)ws;
    k.range = (float*)(k.psum + parts);
    k.pcnt = (unsigned*)(k.range + 2 * nslabs);
    return k;
}

extern "C" size_t mcamd_ws_workspace_bytes(int64_t nslabs, int64_t parts, int32_t nseg) {
    if (nslabs < 0 || parts < 0 || nseg < 0) return 0;
    return (size_t)parts * (sizeof(double) + sizeof(unsigned)) + (size_t)nslabs * 2 * sizeof(float) + 16;
}

// the layer slab `b` belongs to (slab0 ascends; a few dozen entries, uniform)
__device__ __forceinline__ int ws_seg_of_slab(const mcamd_ws_seg* segs, int nseg, int b) {
    int s = 0;
    while (s + 1 < nseg && b >= segs[s + 1].slab0) ++s;
    return s;
}

// the number of mid[j] < w over the K - 1 non-decreasing midpoints, by bisection (K a power of two)
__device__ __forceinline__ int ws_bisect(const double* mid, int K, float w) {
    const double x = (double)w;
    int lo = 0;
    for (int st = K >> 1; st >= 1; st >>= 1)
        if (mid[lo + st - 1] < x) lo += st;
    return lo;
}

// ---------------------------------------------------------------------------------------
// range + linear initialisation
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(WS_T) void ws_range_kernel(const mcamd_ws_seg* __restrict__ segs, int nseg, float* __restrict__ range) {
    __shared__ float rlo[WS_T], rhi[WS_T];
    const int b = blockIdx.x, tid = threadIdx.x;
    const mcamd_ws_seg g = segs[ws_seg_of_slab(segs, nseg, b)];
    const float* w = (const float*)g.w;
    const float* m = (const float*)g.mask;
    const long long base = (long long)(b - g.slab0) * WS_SLAB;
    float lo = INFINITY, hi = -INFINITY;
    for (int j = 0; j < WS_PER; ++j) {
        const long long i = base + j * WS_T + tid;
        if (i < g.n && (!m || m[i] != 0.f)) {
            const float v = w[i];
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    rlo[tid] = lo, rhi[tid] = hi;
    __syncthreads();
    for (int h = WS_T / 2; h > 0; h >>= 1) {
        if (tid < h) rlo[tid] = fminf(rlo[tid], rlo[tid + h]), rhi[tid] = fmaxf(rhi[tid], rhi[tid + h]);
        __syncthreads();
    }
    if (tid == 0) range[2 * (long long)b] = rlo[0], range[2 * (long long)b + 1] = rhi[0];
}

// one workgroup per layer
__global__ __launch_bounds__(WS_T) void ws_init_kernel(const mcamd_ws_seg* __restrict__ segs, const float* __restrict__ range,
                                                       float* __restrict__ codebook) {
    __shared__ float rlo[WS_T], rhi[WS_T];
    const int tid = threadIdx.x;
    const mcamd_ws_seg g = segs[blockIdx.x];
    const long long nsl = (g.n + WS_SLAB - 1) / WS_SLAB;
    float lo = INFINITY, hi = -INFINITY;
    for (long long s = tid; s < nsl; s += WS_T) {
        lo = fminf(lo, range[2 * (g.slab0 + s)]);
        hi = fmaxf(hi, range[2 * (g.slab0 + s) + 1]);
    }
    rlo[tid] = lo, rhi[tid] = hi;
    __syncthreads();
    for (int h = WS_T / 2; h > 0; h >>= 1) {
        if (tid < h) rlo[tid] = fminf(rlo[tid], rlo[tid + h]), rhi[tid] = fmaxf(rhi[tid], rhi[tid + h]);
        __syncthreads();
    }
    if (tid < g.K) {
        const double dlo = (double)rlo[0], dhi = (double)rhi[0];
        float c = 0.f;                                              // no kept weight: a codebook of zeros
        if (rlo[0] <= rhi[0]) c = (float)(dlo + ((dhi - dlo) * (double)tid) / (double)(g.K - 1));
        codebook[g.cb0 + tid] = c;
    }
}

// ---------------------------------------------------------------------------------------
// assign / slab sums
// ---------------------------------------------------------------------------------------
enum { WS_ASSIGN = 0, WS_ASSIGN_SUM = 1, WS_SUM = 2 };

template <int MODE>
__global__ __launch_bounds__(WS_T) void ws_slab_kernel(const mcamd_ws_seg* __restrict__ segs, int nseg, const float* __restrict__ codebook,
                                                       double* __restrict__ psum, unsigned* __restrict__ pcnt) {
    __shared__ float lv[WS_SLAB];
    __shared__ unsigned short lc[WS_SLAB];
    __shared__ double mid[WS_T];
    __shared__ double ssum[WS_T];
    __shared__ unsigned scnt[WS_T];
    const int b = blockIdx.x, tid = threadIdx.x;
    const mcamd_ws_seg g = segs[ws_seg_of_slab(segs, nseg, b)];
    const int K = g.K;
    const float* w = (const float*)g.w;
    const float* m = (const float*)g.mask;
    unsigned char* codes = (unsigned char*)g.codes;
    const long long base = (long long)(b - g.slab0) * WS_SLAB;
    if (MODE != WS_SUM) {
        if (tid < K - 1) mid[tid] = ((double)codebook[g.cb0 + tid] + (double)codebook[g.cb0 + tid + 1]) / 2.0;
        __syncthreads();
    }
    for (int j = 0; j < WS_PER / 4; ++j) {
        const int idx = j * (4 * WS_T) + 4 * tid;                 // in the slab; base and idx are multiples of 4
        const long long i = base + idx;
        float v[4] = {0.f, 0.f, 0.f, 0.f}, k[4] = {1.f, 1.f, 1.f, 1.f};
        unsigned c[4] = {0u, 0u, 0u, 0u};
        const bool full = i + 3 < g.n;
        if (full) {
            const f32x4_t q = *(const f32x4_t*)(w + i);           // 16-byte aligned: w is, base + idx is a multiple of 4
            v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
            if (m) {
                const f32x4_t r = *(const f32x4_t*)(m + i);
                k[0] = r[0], k[1] = r[1], k[2] = r[2], k[3] = r[3];
            }
            if (MODE == WS_SUM) {
                const unsigned p = *(const unsigned*)(codes + i);
                c[0] = p & 0xffu, c[1] = (p >> 8) & 0xffu, c[2] = (p >> 16) & 0xffu, c[3] = p >> 24;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                k[e] = 0.f;
                if (i + e < g.n) {
                    v[e] = w[i + e];
                    k[e] = m ? m[i + e] : 1.f;
                    if (MODE == WS_SUM) c[e] = codes[i + e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool kept = k[e] != 0.f;
            if (MODE != WS_SUM) c[e] = kept ? (unsigned)ws_bisect(mid, K, v[e]) : 0u;
            else c[e] = min(c[e], (unsigned)(K - 1));
            lv[idx + e] = v[e];
            lc[idx + e] = (unsigned short)(kept ? c[e] : (unsigned)WS_NONE);
        }
        if (MODE != WS_SUM) {
            if (full) {
                *(unsigned*)(codes + i) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i + e < g.n) codes[i + e] = (unsigned char)c[e];
            }
        }
    }
    if (MODE == WS_ASSIGN) return;
    __syncthreads();
    // thread k of sub-slab s: the members of cluster k among the sub-slab's weights, in index order
    const int S = WS_T / K, len = WS_SLAB / S;
    const int kk = tid & (K - 1), s = tid / K;
    double sum = 0.0;
    unsigned cnt = 0u;
    for (int t = s * len; t < (s + 1) * len; ++t) {
        if ((int)lc[t] == kk) {
            sum += (double)lv[t];
            ++cnt;
        }
    }
    ssum[tid] = sum, scnt[tid] = cnt;
    __syncthreads();
    if (tid < K) {
        double total = 0.0;
        unsigned n = 0u;
        for (int t = 0; t < S; ++t) total += ssum[t * K + tid], n += scnt[t * K + tid];
        const long long o = g.part0 + (long long)(b - g.slab0) * K + tid;
        psum[o] = total, pcnt[o] = n;
    }
}

// One workgroup per layer, thread k: the slab sums of cluster k in slab order, then the centroid.  The layer's slab sums lie
// as [slab][K]: all 256 threads bring WS_UT of them (WS_UT / K whole slabs) into LDS at a time, thread k adds its column.
constexpr int WS_UT = 2048;
__global__ __launch_bounds__(WS_T) void ws_update_kernel(const mcamd_ws_seg* __restrict__ segs, const double* __restrict__ psum,
                                                         const unsigned* __restrict__ pcnt, float* __restrict__ codebook,
                                                         double* __restrict__ sums, long long* __restrict__ counts) {
    __shared__ double ts[WS_UT];
    __shared__ unsigned tc[WS_UT];
    const int tid = threadIdx.x;
    const mcamd_ws_seg g = segs[blockIdx.x];
    const int K = g.K;
    const long long total = (g.n + WS_SLAB - 1) / WS_SLAB * K;
    const double* p = psum + g.part0;
    const unsigned* q = pcnt + g.part0;
    double sum = 0.0;
    long long cnt = 0;
    for (long long base = 0; base < total; base += WS_UT) {                    // (uniform)
        const int m = (int)(total - base < WS_UT ? total - base : WS_UT);      // a multiple of K
        for (int t = tid; t < m; t += WS_T) ts[t] = p[base + t], tc[t] = q[base + t];
        __syncthreads();
        if (tid < K)
            for (int r = tid; r < m; r += K) sum += ts[r], cnt += (long long)tc[r];
        __syncthreads();
    }
    if (tid >= K) return;
    sums[g.cb0 + tid] = sum, counts[g.cb0 + tid] = cnt;
    if (cnt > 0) codebook[g.cb0 + tid] = (float)(sum / (double)cnt);          // an empty cluster keeps its centroid
}

// w = codebook[code] on kept weights; ZERO: +0 elsewhere, otherwise the other weights are not written
template <bool ZERO>
__global__ __launch_bounds__(WS_T) void ws_write_kernel(const mcamd_ws_seg* __restrict__ segs, int nseg, const float* __restrict__ codebook) {
    __shared__ float cb[WS_T];
    const int b = blockIdx.x, tid = threadIdx.x;
    const mcamd_ws_seg g = segs[ws_seg_of_slab(segs, nseg, b)];
    if (tid < g.K) cb[tid] = codebook[g.cb0 + tid];
    __syncthreads();
    float* w = (float*)g.w;
    const float* m = (const float*)g.mask;
    const unsigned char* codes = (const unsigned char*)g.codes;
    const long long base = (long long)(b - g.slab0) * WS_SLAB;
    for (int j = 0; j < WS_PER; ++j) {
        const long long i = base + j * WS_T + tid;
        if (i >= g.n) break;
        if (!m || m[i] != 0.f) w[i] = cb[min((int)codes[i], g.K - 1)];
        else if (ZERO) w[i] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------
struct WsTotals {
    long long slabs, parts, cb;
};

static int ws_check_table(const char* what, const mcamd_ws_seg* segs, int nseg, long long cb_cap, bool need_codes, WsTotals* t) {
    long long slabs = 0, parts = 0, cb = 0;
    for (int s = 0; s < nseg; ++s) {
        const mcamd_ws_seg& g = segs[s];
        MCAMD_REQUIRE(g.w && g.n > 0, "%s: segment %d: bad tensor (n %lld)", what, s, (long long)g.n);
        MCAMD_REQUIRE(g.K >= 2 && g.K <= 256 && (g.K & (g.K - 1)) == 0, "%s: segment %d: K %d is not 2^bits with bits in 1..8", what, s,
                      g.K);
        MCAMD_REQUIRE(!need_codes || g.codes, "%s: segment %d: null codes", what, s);
        MCAMD_REQUIRE(((uintptr_t)g.w & 15) == 0 && ((uintptr_t)g.mask & 15) == 0 && ((uintptr_t)g.codes & 3) == 0,
                      "%s: segment %d: w and mask must be 16-byte aligned, codes 4-byte aligned", what, s);
        MCAMD_REQUIRE(g.slab0 == slabs, "%s: segment %d: slab0 %d is not the running sum %lld", what, s, g.slab0, slabs);
        MCAMD_REQUIRE(g.cb0 == cb, "%s: segment %d: cb0 %d is not the running sum %lld", what, s, g.cb0, cb);
        MCAMD_REQUIRE(g.part0 == parts, "%s: segment %d: part0 %lld is not the running sum %lld", what, s, (long long)g.part0, parts);
        const long long nsl = (g.n + WS_SLAB - 1) / WS_SLAB;
        slabs += nsl, parts += nsl * g.K, cb += g.K;
        MCAMD_REQUIRE(slabs < (1ll << 31) && cb < (1ll << 31), "%s: too many weights", what);
    }
    MCAMD_REQUIRE(cb <= cb_cap, "%s: %lld codebook entries needed, room for %lld", what, cb, cb_cap);
    t->slabs = slabs, t->parts = parts, t->cb = cb;
    return MCAMD_OK;
}

#define WS_ENTER(what, need_codes, extra)                                                              \
    MCAMD_REQUIRE(!mcamd_recording(), what ": not recordable into a launch plan");                     \
    MCAMD_REQUIRE(segs && segs_dev && nseg > 0 && codebook && (extra), what ": null argument");        \
    WsTotals t;                                                                                        \
    {                                                                                                  \
        const int rc_ = ws_check_table(what, segs, nseg, cb_cap, need_codes, &t);                      \
        if (rc_) return rc_;                                                                           \
    }                                                                                                  \
    hipStream_t st = (hipStream_t)stream

#define WS_WORKSPACE(what)                                                                             \
    MCAMD_REQUIRE(((uintptr_t)workspace & 7) == 0, what ": the workspace must be 8-byte aligned");     \
    if (workspace_bytes < mcamd_ws_workspace_bytes(t.slabs, t.parts, nseg)) {                          \
        mcamd_set_error(what ": workspace too small");                                                 \
        return MCAMD_EWORKSPACE;                                                                       \
    }                                                                                                  \
    const WsWork k = ws_work(workspace, t.slabs, t.parts)

extern "C" int mcamd_ws_init(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, float* codebook, int64_t cb_cap,
                             void* workspace, size_t workspace_bytes, void* stream) {
    WS_ENTER("ws_init", false, workspace != nullptr);
    WS_WORKSPACE("ws_init");
    hipLaunchKernelGGL(ws_range_kernel, dim3((int)t.slabs), dim3(WS_T), 0, st, segs_dev, nseg, k.range);
    hipLaunchKernelGGL(ws_init_kernel, dim3(nseg), dim3(WS_T), 0, st, segs_dev, (const float*)k.range, codebook);
    MCAMD_LAUNCH_CHECK("ws_init");
    return MCAMD_OK;
}

extern "C" int mcamd_ws_iterate(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, float* codebook, int64_t cb_cap,
                                double* sums, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    WS_ENTER("ws_iterate", true, sums && counts && workspace);
    WS_WORKSPACE("ws_iterate");
    hipLaunchKernelGGL(ws_slab_kernel<WS_ASSIGN_SUM>, dim3((int)t.slabs), dim3(WS_T), 0, st, segs_dev, nseg, (const float*)codebook, k.psum,
                       k.pcnt);
    hipLaunchKernelGGL(ws_update_kernel, dim3(nseg), dim3(WS_T), 0, st, segs_dev, (const double*)k.psum, (const unsigned*)k.pcnt, codebook,
                       sums, (long long*)counts);
    MCAMD_LAUNCH_CHECK("ws_iterate");
    return MCAMD_OK;
}

extern "C" int mcamd_ws_assign(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, const float* codebook,
                               int64_t cb_cap, void* stream) {
    WS_ENTER("ws_assign", true, true);
    hipLaunchKernelGGL(ws_slab_kernel<WS_ASSIGN>, dim3((int)t.slabs), dim3(WS_T), 0, st, segs_dev, nseg, codebook, (double*)nullptr,
                       (unsigned*)nullptr);
    MCAMD_LAUNCH_CHECK("ws_assign");
    return MCAMD_OK;
}

extern "C" int mcamd_ws_project(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, float* codebook, int64_t cb_cap,
                                double* sums, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    WS_ENTER("ws_project", true, sums && counts && workspace);
    WS_WORKSPACE("ws_project");
    hipLaunchKernelGGL(ws_slab_kernel<WS_SUM>, dim3((int)t.slabs), dim3(WS_T), 0, st, segs_dev, nseg, (const float*)codebook, k.psum, k.pcnt);
    hipLaunchKernelGGL(ws_update_kernel, dim3(nseg), dim3(WS_T), 0, st, segs_dev, (const double*)k.psum, (const unsigned*)k.pcnt, codebook,
                       sums, (long long*)counts);
    hipLaunchKernelGGL(ws_write_kernel<false>, dim3((int)t.slabs), dim3(WS_T), 0, st, segs_dev, nseg, (const float*)codebook);
    MCAMD_LAUNCH_CHECK("ws_project");
    return MCAMD_OK;
}

extern "C" int mcamd_ws_expand(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, const float* codebook,
                               int64_t cb_cap, void* stream) {
    WS_ENTER("ws_expand", true, true);
    hipLaunchKernelGGL(ws_write_kernel<true>, dim3((int)t.slabs), dim3(WS_T), 0, st, segs_dev, nseg, codebook);
    MCAMD_LAUNCH_CHECK("ws_expand");
    return MCAMD_OK;
}
