// Split-K forward for low-batch fp16 inference (Darknet.splitk): the implicit GEMM of conv_igemm.hip with the
// K axis cut into S slices, for layers whose M = B*H*W pixels give the unsplit launch a handful of workgroups that each
// walk the whole K axis alone (YOLOv2's 13x13 layers at B = 1: 32 workgroups on 256 CUs, 144-180 dependent K chunks).
//
//   launch 1, splitk_partial_kernel: workgroup (tile, slice s) multiplies the K chunks [floor(s n / S), floor((s+1) n / S))
//       of the tile's n = ktot / BK chunks -- same operands, same staging, same v_mfma_f32_32x32x16_f16 walk in K order as
//       igemm_kernel -- and stores its fp32 accumulators, unrounded, to slab s of the workspace [S][Mpad][Npad].
//   launch 2, splitk_finish_kernel: a 16-pixel x 64-channel tile per workgroup sums the S slabs of each element in slice
//       order 0 .. S-1 in fp32, applies the epilogue arithmetic of the fp16 kernels (leaky(acc * scale + shift), saturating
//       fp16, overflow flag), lays the tile down in LDS and calls the shared stores of conv_epi.h.
//
// The reduction is a launch boundary on purpose: no workgroup waits for, polls or counts another, there are no arrival
// counters and no fences, and the result is a function of the operands and S only.  With S = 1 the pair computes what
// igemm_kernel computes, bit for bit (every element's accumulator sees the same MFMA sequence, whatever the tile).
#include "kernels.h"
#include "conv_epi.h"

struct SplitkArgs {
    IgemmArgs a;
    float* ws;              // [slices][slab_elems]
    long long slab_elems;   // mtiles * BM * npad
    int slices;
    int npad;               // ntiles * BN: floats per slab row
    int mtiles, ntiles;
};

constexpr int SK_BM = 64, SK_BN = 64;    // partial tile: 4 waves of 32 x 32 (3 M tiles for 169 pixels, not 2 x 128 rows)
constexpr int SK_FR = 16, SK_FC = 64;    // finish tile

template <int BK, int NSTAGE>
__global__ __launch_bounds__(256) void splitk_partial_kernel(SplitkArgs p) {
    constexpr int BM = SK_BM, BN = SK_BN, NT = 256, WAVES_N = 2;
    constexpr int CPR = BK / 8;
    constexpr int A_SLOTS = BM * CPR, B_SLOTS = BN * CPR;
    constexpr int A_IT = A_SLOTS / NT, B_IT = B_SLOTS / NT;
    constexpr int STAGE_BYTES = (A_SLOTS + B_SLOTS) * 16;
    constexpr int DMIN = A_IT + B_IT;   // DMA instructions every wave issues per K chunk
    static_assert(A_SLOTS % NT == 0 && B_SLOTS % NT == 0, "every wave issues the same DMA pieces");
    static_assert(NSTAGE >= 2 && NSTAGE <= 4 && DMIN * (NSTAGE - 2) < 64, "vmcnt immediate range");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const IgemmArgs& a = p.a;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: no waterfall around the LDS-DMA
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    // the M tiles of one (N tile, slice) on one XCD: they stage the same weight chunks
    int mt, grp;
    if (!xcd_tile(p.mtiles, p.ntiles * p.slices, mt, grp)) return;
    const int s = grp / p.ntiles, nt = grp - s * p.ntiles;
    const int nchunks = a.ktot / BK;
    const int q0 = (int)((long long)s * nchunks / p.slices), q1 = (int)((long long)(s + 1) * nchunks / p.slices);
    const int nloc = q1 - q0;
    const bool pooled = a.mode == MCAMD_EPI_PAD_F16 && a.dst_mode != 0;

    long long abase[A_IT], bbase[B_IT];
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPR, phys = slot % CPR;
        abase[it] = tile_x_base(a, pooled, mt * BM + row) + (phys ^ swz<CPR>(row)) * 8;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
        const int slot = it * NT + tid;
        const int row = slot / CPR, phys = slot % CPR;
        bbase[it] = (long long)(nt * BN + row) * a.ktot + (phys ^ swz<CPR>(row)) * 8;
    }

    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    auto stage = [&](int q, int buf) {
        // packed K order [channel block of a.kb][tap][a.kb channels]: chunk q -> (block, tap, sub-chunk)
        const int sub = a.kb / BK > 0 ? a.kb / BK : 1, per_block = a.ntaps * sub;
        const int cb = q / per_block, r = q - cb * per_block;
        const int tap = r / sub;
        const int koff = a.tap_off[tap] + cb * a.kb + (r - tap * sub) * BK;
        char* sa = smem + buf * STAGE_BYTES;
        char* sb = sa + A_SLOTS * 16;
#pragma unroll
        for (int it = 0; it < A_IT; ++it) glds16(a.x + abase[it] + koff, sa + (it * NT + wave * 64) * 16);
#pragma unroll
        for (int it = 0; it < B_IT; ++it) glds16(a.w + bbase[it] + (long long)q * BK, sb + (it * NT + wave * 64) * 16);
    };

    // NSTAGE-deep LDS ring with counted waits, as igemm_kernel: chunks i+1 .. i+NSTAGE-2 stay in flight across the barrier
#pragma unroll
    for (int i = 0; i < NSTAGE - 1; ++i)
        if (i < nloc) stage(q0 + i, i);
    int sidx = 0;
    for (int i = 0; i < nloc; ++i) {
        int issued = i + NSTAGE - 1;
        if (issued > nloc) issued = nloc;
        const int inflight = issued - i - 1;
        if (NSTAGE == 2 || inflight == 0) wait_vmcnt<0>();
        else if (inflight == 1) wait_vmcnt<DMIN>();
        else wait_vmcnt<(NSTAGE > 3 ? 2 * DMIN : DMIN)>();
        __builtin_amdgcn_s_barrier();   // chunk i landed for every wave; every wave is done reading chunk i-1
        if (i + NSTAGE - 1 < nloc) {
            int ns = sidx + NSTAGE - 1;
            if (ns >= NSTAGE) ns -= NSTAGE;
            stage(q0 + i + NSTAGE - 1, ns);
        }
        const char* sa = smem + sidx * STAGE_BYTES;
        const char* sb = sa + A_SLOTS * 16;
        sidx = sidx + 1 == NSTAGE ? 0 : sidx + 1;
        constexpr int KS = BK / 16;
        h8_t af[KS], bf[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int chunk = 2 * k + (lane >> 5);
            const int ra = wm * 32 + (lane & 31), rb = wn * 32 + (lane & 31);
            af[k] = *(const h8_t*)(sa + (ra * CPR + (chunk ^ swz<CPR>(ra))) * 16);
            bf[k] = *(const h8_t*)(sb + (rb * CPR + (chunk ^ swz<CPR>(rb))) * 16);
        }
#pragma unroll
        for (int k = 0; k < KS; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[k], bf[k], acc, 0, 0, 0);
    }

    // a store instruction writes two rows x 32 consecutive floats of the slab (whole 128-byte lines); the slab is padded
    // to whole tiles, so rows past the last pixel and columns past the last channel are stored too (never read back as
    // results: the finish kernel's stores mask them)
    float* slab = p.ws + (long long)s * p.slab_elems;
    const int col = nt * BN + wn * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = mt * BM + wm * 32 + mfma32_row(r, lane);
        slab[(long long)row * p.npad + col] = acc[r];
    }
}

template <int EPI>
__global__ __launch_bounds__(256) void splitk_finish_kernel(SplitkArgs p) {
    constexpr int NT = 256;
    __shared__ __attribute__((aligned(16))) half_t ct[SK_FR * SK_FC];
    const IgemmArgs& a = p.a;
    const int tid = threadIdx.x;
    const int nt = blockIdx.x % p.ntiles, mt = blockIdx.x / p.ntiles;
    const int row = tid / (SK_FC / 4), c4 = (tid % (SK_FC / 4)) * 4;
    const int n0 = nt * SK_FC + c4;
    // (rows up to round_up(M, 16) <= Mpad and columns up to Npad exist in every slab)
    const float* src = p.ws + (long long)(mt * SK_FR + row) * p.npad + n0;
    f32x4_t v = *(const f32x4_t*)src;
    for (int s = 1; s < p.slices; ++s) {   // slice order: the sum does not depend on scheduling
        const f32x4_t u = *(const f32x4_t*)(src + (long long)s * p.slab_elems);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += u[e];
    }
    bool sat = false;
    h4_t hv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = v[e];
        if constexpr (EPI == MCAMD_EPI_PAD_F16) {
            float sc = 1.f, sh = 0.f;
            if (n0 + e < a.N) {
                if (a.scale) sc = a.scale[n0 + e];
                if (a.shift) sh = a.shift[n0 + e];
            }
            x = x * sc + sh;
            x = x > 0.f ? x : x * a.slope;
        }
        hv[e] = (half_t)fminf(fmaxf(x, -65504.f), 65504.f);   // saturate, never inf
        sat |= fabsf(x) > 65504.f && mt * SK_FR + row < a.M && n0 + e < a.N;
    }
    *(h4_t*)(ct + row * SK_FC + c4) = hv;
    __syncthreads();
    if constexpr (EPI == MCAMD_EPI_PAD_F16) store_pad_tile<SK_FR, SK_FC, SK_FC, NT>(a, nullptr, ct, false, false, mt, nt, tid);
    else store_raw_tile<SK_FR, SK_FC, NT>(a, ct, mt, nt, tid);
    if (sat && a.overflow) atomicOr(a.overflow, 1);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// The policy, in one place.  Split only when the unsplit launch leaves most CUs idle: the largest S <= CUS / tiles that
// leaves every slice at least MIN_CHUNKS chunks, clamped to [1, 16]; S = 1: do not split (cdna_hip_programming.md,
// "decomposition first": tiles x S about half to once the CU count).
//
// MCAMD_SPLITK_MIN_CHUNKS = 8, MCAMD_SPLITK_CUS = 256.  Measured (tools/latency_bench.py, B = 1, us unsplit -> split,
// profiles/latency_bench_splitk.json): every layer these values split is faster split --
//   conv14 / 16 / 18 (48 tiles, S = 5)   50.8 -> 19.6      conv19 / 20 (48 tiles, S = 5)   93.6 -> 24.9
//   conv22 (48 tiles, S = 5)            114.6 -> 28.0      conv9 / 11 / 13 (88 tiles, S = 2) 33.2 -> 21.6
//   conv15 / 17 (24 tiles, S = 2: slices of exactly 8 chunks)  17.5 -> 15.7
// -- the gain is down to 9-14 % at 8 chunks per slice, so 8 stays (shorter slices were not tried); 512 was not A/B-ed.
#define MCAMD_SPLITK_MIN_CHUNKS_DEFAULT 8
#define MCAMD_SPLITK_CUS_DEFAULT 256
#define MCAMD_SPLITK_MAX_SLICES 16

SplitkPlan mcamd_splitk_plan(long long M, int n, int cin_tap, int ktot, int forced) {
    SplitkPlan p;
    p.bm = SK_BM, p.bn = SK_BN;
    p.bk = cin_tap % 64 == 0 ? 64 : 32;
    p.stages = p.bk == 64 ? 3 : 4;   // splitk_partial_kernel<64, 3> / <32, 4>
    p.fr = SK_FR, p.fc = SK_FC;
    p.chunks = ktot / p.bk;
    p.mtiles = (int)((M + SK_BM - 1) / SK_BM);
    p.ntiles = (n + SK_BN - 1) / SK_BN;
    p.tiles = p.mtiles * p.ntiles;
    if (forced > 0) {
        p.slices = forced;
    } else {
        int min_chunks = MCAMD_ENV_INT("MCAMD_SPLITK_MIN_CHUNKS", MCAMD_SPLITK_MIN_CHUNKS_DEFAULT);
        const int cus = MCAMD_ENV_INT("MCAMD_SPLITK_CUS", MCAMD_SPLITK_CUS_DEFAULT);
        if (min_chunks < 1) min_chunks = 1;
        long long s = cus / (long long)p.tiles;
        if (s > p.chunks / min_chunks) s = p.chunks / min_chunks;
        if (s > MCAMD_SPLITK_MAX_SLICES) s = MCAMD_SPLITK_MAX_SLICES;
        if (s < 1) s = 1;
        p.slices = (int)s;
    }
    p.slab_elems = (long long)p.mtiles * SK_BM * p.ntiles * SK_BN;
    return p;
}

// a.* geometry and epilogue fields filled by the caller (mode MCAMD_EPI_PAD_F16 or MCAMD_EPI_RAW_F16 without statistics);
// ws: p.slices * p.slab_elems floats
int mcamd_splitk_launch(const IgemmArgs& a, const SplitkPlan& p, float* ws, hipStream_t st) {
    if (a.cin_tap % p.bk != 0 || a.ktot % p.bk != 0 || p.slices < 1 || p.slices > p.chunks) {
        mcamd_set_error("conv_fwd_splitk: K per tap %d / slices %d do not fit %d chunks of %d", a.cin_tap, p.slices, p.chunks, p.bk);
        return MCAMD_EINVAL;
    }
    SplitkArgs k;
    k.a = a;
    k.ws = ws;
    k.slab_elems = p.slab_elems;
    k.slices = p.slices;
    k.npad = p.ntiles * SK_BN;
    k.mtiles = p.mtiles, k.ntiles = p.ntiles;
    const int groups = p.ntiles * p.slices;
    const dim3 grid((unsigned)(round_up_int(groups, 8) * p.mtiles));
    if (p.bk == 64 && p.stages == 3) hipLaunchKernelGGL((splitk_partial_kernel<64, 3>), grid, dim3(256), 3 * (SK_BM + SK_BN) * 8 * 16, st, k);
    else if (p.bk == 32 && p.stages == 4) hipLaunchKernelGGL((splitk_partial_kernel<32, 4>), grid, dim3(256), 4 * (SK_BM + SK_BN) * 4 * 16, st, k);
    else {
        mcamd_set_error("conv_fwd_splitk: no partial kernel instance for chunks of %d with %d stages", p.bk, p.stages);
        return MCAMD_EINVAL;
    }
    MCAMD_LAUNCH_CHECK("conv_fwd_splitk (partial)");
    const dim3 fgrid((unsigned)(((a.M + p.fr - 1) / p.fr) * p.ntiles));
    if (a.mode == MCAMD_EPI_PAD_F16) hipLaunchKernelGGL((splitk_finish_kernel<MCAMD_EPI_PAD_F16>), fgrid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL((splitk_finish_kernel<MCAMD_EPI_RAW_F16>), fgrid, dim3(256), 0, st, k);
    MCAMD_LAUNCH_CHECK("conv_fwd_splitk (finish)");
    return MCAMD_OK;
}
