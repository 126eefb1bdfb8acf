// The two device passes around a compressed model file (.mcz, include/mcamd.h) for gfx950, wave64.
//
// pack    fp32 OIHW masters (* masks) of ALL layers, one segment table -> bit words, kept counts, fp8 / 4-bit exponents, 4-bit
//         group shifts and the compacted values in the file's own layout.  Launches: [exponents + shifts] -> words +
//         workgroup counts -> scan -> scatter.
// unpack  bit words + compacted values (+ exponents, shifts) -> fp32 OIHW weights and, optionally, the fp32 0/1 masks.
//         Launches: workgroup counts -> scan -> expand.  The words, exponents, shifts and values are read where the caller
//         has them (word0 / exp0 / shift0 / val0 are offsets it gives), so a whole file uploaded once serves as every array.
//
// One wave handles one word of 64 consecutive weights: each lane converts its weight, the wave ballot of "my code is
// non-zero" IS the word, and a lane's rank among the kept values of the word is the population count of the word below the
// lane.  A workgroup (4 waves) owns MCAMD_WZ_BLOCK_WORDS consecutive words of one segment; the position of a workgroup's
// first kept value comes from an exclusive scan of the workgroup counts inside the segment (one wave, 64 counts per step, a
// 64-bit carry).  Nothing is decided by an atomic, so the output bytes depend on the inputs only.  Plain C++ loads and stores
// throughout; 64-bit element offsets.
#include "common.h"
#include "q8_exp.h"
#include "w4_quant.h"

constexpr int WZ_BW = MCAMD_WZ_BLOCK_WORDS;      // words per workgroup
constexpr int WZ_WAVES = 4;                      // 256 threads
constexpr int WZ_WPW = WZ_BW / WZ_WAVES;         // words per wave
static_assert(WZ_BW == 64, "the scatter / expand kernels load a workgroup's words with one wave");

typedef unsigned long long u64;

struct WzWork {          // the workspace (mcamd_wz_workspace_bytes)
    u64* blockoff;       // [nblocks] kept values of the segment in front of the workgroup
    u64* segbase;        // [nseg]    pack: byte offset of the segment's values
    unsigned* blocksum;  // [nblocks] kept values of the workgroup
    int* dense;          // [nseg]    pack: the segment is stored without bit words
};

static WzWork wz_work(void* ws, long long nblocks, int nseg) {
    WzWork k;
    k.blockoff = (u64*)ws;
    k.segbase = k.blockoff + nblocks;
    k.blocksum = (unsigned*)(k.segbase + nseg);
    k.dense = (int*)(k.blocksum + nblocks);
    return k;
}

extern "C" size_t mcamd_wz_workspace_bytes(int64_t nblocks, int32_t nseg) {
    if (nblocks < 0 || nseg < 0) return 0;
    return (size_t)nblocks * (sizeof(u64) + sizeof(unsigned)) + (size_t)nseg * (sizeof(u64) + sizeof(int)) + 16;
}

// an MCAMD_WZ_W4 segment's kind carries its taps (MCAMD_WZ_W4_KIND): take them off, leaving the bare kind in the copy
__device__ __forceinline__ int wz_taps(mcamd_wz_seg& g) {
    const int taps = g.kind >> 8;
    g.kind &= 0xff;
    return taps;
}

// MCAMD_WZ_W4: the group of weight i in the order [cout][cin / 32][kh][kw] (per = cin * taps weights per filter)
__device__ __forceinline__ long long wz_w4_group(long long i, long long per, int taps) {
    const long long f = i / per, r = i - f * per, c = r / taps, tap = r - c * taps;
    return f * (per / 32) + (c >> 5) * taps + tap;
}

__device__ __forceinline__ int wz_elem(int kind) { return kind == MCAMD_WZ_FP32 ? 4 : kind == MCAMD_WZ_FP16 ? 2 : 1; }

// the code of weight * mask in the segment's value kind (e: the filter's exponent, fp8 only)
__device__ __forceinline__ unsigned wz_code(int kind, float wm, int e) {
    if (kind == MCAMD_WZ_FP32) return __float_as_uint(wm);
    if (kind == MCAMD_WZ_FP16) {
        const half_t h = (half_t)wm;                       // round to nearest even, the fp16 packers' conversion
        return (unsigned)__builtin_bit_cast(unsigned short, h);
    }
    return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(q8_weight_scaled(wm, e), 0.f, 0, false) & 0xffu;
}

// kept: any bit outside the sign bit
__device__ __forceinline__ bool wz_kept(int kind, unsigned code) {
    return (code & (kind == MCAMD_WZ_FP32 ? 0x7fffffffu : kind == MCAMD_WZ_FP16 ? 0x7fffu : kind == MCAMD_WZ_W4 ? 0x7u : 0x7fu)) != 0u;
}

__device__ __forceinline__ float wz_value(int kind, unsigned code, int e) {
    if (kind == MCAMD_WZ_FP32) return __uint_as_float(code);
    if (kind == MCAMD_WZ_FP16) return (float)__builtin_bit_cast(half_t, (unsigned short)code);
    return ldexpf(__builtin_amdgcn_cvt_f32_fp8((int)code, 0), -e);
}

__device__ __forceinline__ void wz_store(void* base, int kind, long long i, unsigned code) {
    if (kind == MCAMD_WZ_FP32) ((unsigned*)base)[i] = code;
    else if (kind == MCAMD_WZ_FP16) ((unsigned short*)base)[i] = (unsigned short)code;
    else ((unsigned char*)base)[i] = (unsigned char)code;
}

__device__ __forceinline__ unsigned wz_load(const void* base, int kind, long long i) {
    if (kind == MCAMD_WZ_FP32) return ((const unsigned*)base)[i];
    if (kind == MCAMD_WZ_FP16) return ((const unsigned short*)base)[i];
    return ((const unsigned char*)base)[i];
}

// the segment workgroup `b` belongs to (block0 ascends; <= a few dozen entries, uniform)
__device__ __forceinline__ int wz_seg_of_block(const mcamd_wz_seg* segs, int nseg, int b) {
    int s = 0;
    while (s + 1 < nseg && b >= segs[s + 1].block0) ++s;
    return s;
}

__device__ __forceinline__ float wz_masked(const mcamd_wz_seg& g, long long i) {
    const float* m = (const float*)g.mask;
    return ((const float*)g.w)[i] * (m ? m[i] : 1.f);
}

// the exponent of weight i's filter (MCAMD_WZ_FP8, MCAMD_WZ_W4) and the shift byte of its group (MCAMD_WZ_W4); 0 otherwise
__device__ __forceinline__ void wz_scales(const mcamd_wz_seg& g, int taps, long long per, long long i, const int* __restrict__ exps,
                                          const unsigned char* __restrict__ shifts, int* e, int* sh) {
    const bool w4 = g.kind == MCAMD_WZ_W4;
    *e = (w4 || g.kind == MCAMD_WZ_FP8) ? exps[g.exp0 + (int)(i / per)] : 0;
    *sh = w4 ? (int)shifts[8ll * g.shift0 + wz_w4_group(i, per, taps)] : 0;
}

// pack: the stored code of weight i and whether it is kept.  MCAMD_WZ_CODE: the byte at w[i], kept by the MASK (a shared
// value may be exactly 0); every other kind: the code of weight * mask, kept iff it is non-zero.  MCAMD_WZ_W4: pack_q8_w4_kernel's
// code of the weight scaled by its filter's e4_f under its group's shift byte `sh`
__device__ __forceinline__ unsigned wz_pack_code(const mcamd_wz_seg& g, long long i, int e, int sh, bool* keep) {
    if (g.kind == MCAMD_WZ_CODE) {
        const float* m = (const float*)g.mask;
        *keep = !m || m[i] != 0.f;
        return ((const unsigned char*)g.w)[i];
    }
    const unsigned code = g.kind == MCAMD_WZ_W4 ? w4_code(ldexpf(wz_masked(g, i), e), sh - 5) : wz_code(g.kind, wz_masked(g, i), e);
    *keep = wz_kept(g.kind, code);
    return code;
}

// ---------------------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------------------
// One workgroup per filter of the MCAMD_WZ_FP8 and MCAMD_WZ_W4 segments: exps[f] = the packers' exponent of max |w * mask|
// (fp8: e_f; 4-bit: e4_f).  MCAMD_WZ_W4: then one thread per group of 32 input channels at one tap (32 weights strided by the
// taps in OIHW): the maximum of the scaled magnitudes and from it the shift byte, pack_q8_w4_kernel's steps in its order.
__global__ __launch_bounds__(256) void wz_exponent_kernel(const mcamd_wz_seg* __restrict__ segs, int nseg, int* __restrict__ exps,
                                                          unsigned char* __restrict__ shifts) {
    __shared__ float red[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    int s = -1;
    for (int t = 0; t < nseg; ++t) {
        const int kind = segs[t].kind & 0xff;
        if ((kind == MCAMD_WZ_FP8 || kind == MCAMD_WZ_W4) && f >= segs[t].exp0 && f < segs[t].exp0 + segs[t].cout) s = t;
    }
    if (s < 0) return;                                   // (uniform; the host sizes the grid to the fp8 and 4-bit filters)
    mcamd_wz_seg g = segs[s];
    const int taps = wz_taps(g);
    const long long per = g.n / g.cout, first = (long long)(f - g.exp0) * per;
    float amax = 0.f;
    for (long long o = tid; o < per; o += 256) amax = fmaxf(amax, fabsf(wz_masked(g, first + o)));
    red[tid] = amax;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] = fmaxf(red[tid], red[tid + h]);
        __syncthreads();
    }
    if (g.kind == MCAMD_WZ_FP8) {
        if (tid == 0) exps[f] = q8_filter_exponent(red[0]);
        return;
    }
    const int e4 = w4_filter_exponent(red[0]);
    if (tid == 0) exps[f] = e4;
    const int ngrp = (int)(per / 32);                    // groups of the filter, [cin / 32][taps]
    unsigned char* out = shifts + 8ll * g.shift0 + (long long)(f - g.exp0) * ngrp;
    for (int q = tid; q < ngrp; q += 256) {
        const int j = q / taps, tap = q - j * taps;
        const long long base = first + (long long)j * 32 * taps + tap;
        float m = 0.f;
        for (int k = 0; k < 32; ++k) m = fmaxf(m, fabsf(ldexpf(wz_masked(g, base + (long long)k * taps), e4)));
        out[q] = (unsigned char)(w4_group_shift(m) + 5);
    }
}

__global__ __launch_bounds__(256) void wz_words_kernel(const mcamd_wz_seg* __restrict__ segs, int nseg, const int* __restrict__ exps,
                                                       const unsigned char* __restrict__ shifts, u64* __restrict__ words,
                                                       unsigned* __restrict__ blocksum) {
    __shared__ unsigned cnt[WZ_WAVES];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    mcamd_wz_seg g = segs[wz_seg_of_block(segs, nseg, b)];
    const int taps = wz_taps(g);
    const long long nwords = (g.n + 63) / 64, per = g.n / g.cout;
    const long long w0 = (long long)(b - g.block0) * WZ_BW + wave * WZ_WPW;
    unsigned c = 0;
    for (int j = 0; j < WZ_WPW; ++j) {
        const long long wi = w0 + j;
        if (wi >= nwords) break;                          // wave-uniform
        const long long i = wi * 64 + lane;
        bool keep = false;
        if (i < g.n) {
            int e, sh;
            wz_scales(g, taps, per, i, exps, shifts, &e, &sh);
            (void)wz_pack_code(g, i, e, sh, &keep);
        }
        const u64 word = __ballot(keep);
        if (lane == 0) words[g.word0 + wi] = word;
        c += (unsigned)__popcll(word);
    }
    if (lane == 0) cnt[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) blocksum[b] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// One wave.  Per segment: exclusive scan of its workgroup counts (64 per step), then (PACK) its kept count, whether it is
// stored with bit words, and the byte offset of its values.
template <bool PACK>
__global__ __launch_bounds__(64) void wz_scan_kernel(const mcamd_wz_seg* __restrict__ segs, int nseg,
                                                     const unsigned* __restrict__ blocksum, u64* __restrict__ blockoff,
                                                     u64* __restrict__ counts, u64* __restrict__ segbase, int* __restrict__ dense) {
    const int lane = threadIdx.x;
    u64 vb = 0;
    for (int s = 0; s < nseg; ++s) {
        mcamd_wz_seg g = segs[s];
        (void)wz_taps(g);
        const long long nwords = (g.n + 63) / 64;
        const int nb = (int)((nwords + WZ_BW - 1) / WZ_BW);
        u64 carry = 0;
        for (int base = 0; base < nb; base += 64) {
            const int idx = base + lane;
            const unsigned v = idx < nb ? blocksum[g.block0 + idx] : 0u;
            unsigned x = v;                               // <= 64 * 4096: no overflow
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned y = __shfl_up(x, d);
                if (lane >= d) x += y;
            }
            if (idx < nb) blockoff[g.block0 + idx] = carry + x - v;
            carry += (u64)__shfl(x, 63);
        }
        if (PACK) {
            const u64 elem = (u64)wz_elem(g.kind);
            // (MCAMD_WZ_W4: the rule counts the file's nibbles, the pass stores one byte per code)
            const bool bits = g.kind == MCAMD_WZ_CODE ? carry < (u64)g.n
                            : g.kind == MCAMD_WZ_W4   ? 8ull * (u64)nwords + (carry + 1ull) / 2ull < ((u64)g.n + 1ull) / 2ull
                                                      : 8ull * (u64)nwords + carry * elem < (u64)g.n * elem;
            if (lane == 0) {
                counts[s] = carry;
                dense[s] = bits ? 0 : 1;
                segbase[s] = vb;
            }
            const u64 bytes = (bits ? carry : (u64)g.n) * elem;
            vb += (bytes + 7ull) & ~7ull;
        }
    }
}

// the words of the workgroup and the exclusive scan of their population counts, in LDS
__device__ __forceinline__ void wz_block_words(const u64* __restrict__ words, bool have, long long word0, long long first,
                                               long long nwords, u64 (&wsh)[WZ_BW], unsigned (&osh)[WZ_BW]) {
    const int tid = threadIdx.x;
    if (tid < WZ_BW) {                                    // wave 0, all 64 lanes
        const u64 word = (have && first + tid < nwords) ? words[word0 + first + tid] : 0ull;
        const unsigned v = (unsigned)__popcll(word);
        unsigned x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            if (tid >= d) x += y;
        }
        wsh[tid] = word;
        osh[tid] = x - v;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void wz_scatter_kernel(const mcamd_wz_seg* __restrict__ segs, int nseg, const int* __restrict__ exps,
                                                         const unsigned char* __restrict__ shifts,
                                                         const u64* __restrict__ words, const u64* __restrict__ blockoff,
                                                         const u64* __restrict__ segbase, const int* __restrict__ dense,
                                                         char* __restrict__ values) {
    __shared__ u64 wsh[WZ_BW];
    __shared__ unsigned osh[WZ_BW];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = wz_seg_of_block(segs, nseg, b);
    mcamd_wz_seg g = segs[s];
    const int taps = wz_taps(g);
    const long long nwords = (g.n + 63) / 64, per = g.n / g.cout;
    const long long first = (long long)(b - g.block0) * WZ_BW;
    wz_block_words(words, true, g.word0, first, nwords, wsh, osh);
    const bool all = dense[s] != 0;
    void* base = values + segbase[s];
    const u64 boff = blockoff[b];
    for (int j = 0; j < WZ_WPW; ++j) {
        const int k = wave * WZ_WPW + j;
        const long long wi = first + k;
        if (wi >= nwords) break;
        const long long i = wi * 64 + lane;
        if (i >= g.n) continue;
        const u64 word = wsh[k];
        const bool bit = (word >> lane) & 1ull;
        if (!bit && !all) continue;
        unsigned code = 0u;
        if (bit) {
            int e, sh;
            wz_scales(g, taps, per, i, exps, shifts, &e, &sh);
            bool keep;
            code = wz_pack_code(g, i, e, sh, &keep);
        }
        const long long pos = all ? i : (long long)(boff + osh[k] + (u64)__popcll(word & ((1ull << lane) - 1ull)));
        wz_store(base, g.kind, pos, code);
    }
}

// ---------------------------------------------------------------------------------------
// unpack
// ---------------------------------------------------------------------------------------
// One wave per workgroup of words (WZ_BW == 64): the kept values of the workgroup.
__global__ __launch_bounds__(64) void wz_popc_kernel(const mcamd_wz_seg* __restrict__ segs, int nseg, const u64* __restrict__ words,
                                                     unsigned* __restrict__ blocksum) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const mcamd_wz_seg g = segs[wz_seg_of_block(segs, nseg, b)];      // (kind is not read)
    const long long nwords = (g.n + 63) / 64, first = (long long)(b - g.block0) * WZ_BW;
    unsigned c = (!g.dense && first + lane < nwords) ? (unsigned)__popcll(words[g.word0 + first + lane]) : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if (lane == 0) blocksum[b] = c;
}

__global__ __launch_bounds__(256) void wz_expand_kernel(const mcamd_wz_seg* __restrict__ segs, int nseg, const int* __restrict__ exps,
                                                        const unsigned char* __restrict__ shifts,
                                                        const u64* __restrict__ words, const u64* __restrict__ blockoff,
                                                        const char* __restrict__ values) {
    __shared__ u64 wsh[WZ_BW];
    __shared__ unsigned osh[WZ_BW];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    mcamd_wz_seg g = segs[wz_seg_of_block(segs, nseg, b)];
    const int taps = wz_taps(g);
    const long long nwords = (g.n + 63) / 64, per = g.n / g.cout;
    const long long first = (long long)(b - g.block0) * WZ_BW;
    wz_block_words(words, !g.dense, g.word0, first, nwords, wsh, osh);
    const void* base = values + g.val0;
    const u64 boff = blockoff[b];
    float* w = (float*)g.w;
    float* mask = (float*)g.mask;
    for (int j = 0; j < WZ_WPW; ++j) {
        const int k = wave * WZ_WPW + j;
        const long long wi = first + k;
        if (wi >= nwords) break;
        const long long i = wi * 64 + lane;
        if (i >= g.n) continue;
        const u64 word = wsh[k];
        bool bit = g.dense || ((word >> lane) & 1ull);
        unsigned code = 0u;
        if (g.dense) {
            code = wz_load(base, g.kind, i);
        } else if (bit) {
            const u64 pos = boff + osh[k] + (u64)__popcll(word & ((1ull << lane) - 1ull));
            if (pos < (u64)g.kept) code = wz_load(base, g.kind, (long long)pos);      // a damaged file reads as +0
        }
        if (g.kind == MCAMD_WZ_CODE) {                    // the codes themselves; the caller expands them (mcamd_ws_expand)
            ((unsigned char*)g.w)[i] = bit ? (unsigned char)code : (unsigned char)0;
            if (mask) mask[i] = bit ? 1.f : 0.f;
            continue;
        }
        float v = 0.f;
        if (wz_kept(g.kind, code)) {
            int e, sh;
            wz_scales(g, taps, per, i, exps, shifts, &e, &sh);
            if (g.kind != MCAMD_WZ_W4) {
                v = wz_value(g.kind, code, e);
            } else if (sh <= 11) {                        // (a damaged file's shift byte reads as +0)
                v = ldexpf(w4_grid(code & 7u), sh - 5 - e);
                if (code & 8u) v = -v;
            }
        }
        w[i] = v;
        if (mask) mask[i] = bit ? 1.f : 0.f;
    }
}

// ---------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------
struct WzTotals {
    long long blocks, words, exps, shifts, cap_bytes;     // (shifts: in units of 8 bytes)
};

// `shifts_cap` < 0: the entry point takes no shift bytes and refuses an MCAMD_WZ_W4 segment
static int wz_check_table(const char* what, const mcamd_wz_seg* segs, int nseg, bool unpack, long long words_cap, long long exps_cap,
                          long long shifts_cap, long long values_bytes, WzTotals* t) {
    long long blocks = 0, words = 0, exps = 0, shifts = 0, cap = 0;
    for (int s = 0; s < nseg; ++s) {
        const mcamd_wz_seg& g = segs[s];
        MCAMD_REQUIRE(g.w && g.n > 0 && g.cout > 0 && g.n % g.cout == 0, "%s: segment %d: bad tensor (n %lld, cout %d)", what, s,
                      (long long)g.n, g.cout);
        const bool w4 = (g.kind & 0xff) == MCAMD_WZ_W4 && g.kind >= 0;
        MCAMD_REQUIRE(g.kind == MCAMD_WZ_FP32 || g.kind == MCAMD_WZ_FP16 || g.kind == MCAMD_WZ_FP8 || g.kind == MCAMD_WZ_CODE || w4,
                      "%s: segment %d: bad value kind %d", what, s, g.kind);
        const bool scaled = w4 || g.kind == MCAMD_WZ_FP8;  // one exponent per filter
        if (w4) {
            const long long taps = g.kind >> 8, per = g.n / g.cout;
            MCAMD_REQUIRE(shifts_cap >= 0, "%s: segment %d: an MCAMD_WZ_W4 segment goes through %s_w4", what, s, what);
            MCAMD_REQUIRE(taps > 0 && per % taps == 0 && (per / taps) % 32 == 0,
                          "%s: segment %d: MCAMD_WZ_W4 needs cin %% 32 == 0 (%lld weights per filter, %lld taps)", what, s, per, taps);
        }
        const long long elem = g.kind == MCAMD_WZ_FP32 ? 4 : g.kind == MCAMD_WZ_FP16 ? 2 : 1;
        const long long nwords = (g.n + 63) / 64;
        MCAMD_REQUIRE(g.block0 == blocks, "%s: segment %d: block0 %d is not the running sum %lld", what, s, g.block0, blocks);
        if (!unpack) {                                    // pack lays the arrays out itself: running sums
            MCAMD_REQUIRE(g.word0 == words, "%s: segment %d: word0 %lld is not the running sum %lld", what, s, (long long)g.word0, words);
            words += nwords;
            if (scaled) {
                MCAMD_REQUIRE(g.exp0 == exps, "%s: segment %d: exp0 %d is not the running sum %lld", what, s, g.exp0, exps);
                exps += g.cout;
            }
            if (w4) {
                MCAMD_REQUIRE(g.shift0 == shifts, "%s: segment %d: shift0 %d is not the running sum %lld", what, s, g.shift0, shifts);
                shifts += (g.n / 32 + 7) / 8;
            }
        } else {                                          // unpack reads them where the caller has them
            MCAMD_REQUIRE(g.dense == 1 || (g.word0 >= 0 && g.word0 + nwords <= words_cap),
                          "%s: segment %d: bit words [%lld, +%lld) outside the %lld given", what, s, (long long)g.word0, nwords, words_cap);
            MCAMD_REQUIRE(!scaled || (g.exp0 >= 0 && (long long)g.exp0 + g.cout <= exps_cap),
                          "%s: segment %d: exponents [%d, +%d) outside the %lld given", what, s, g.exp0, g.cout, exps_cap);
            MCAMD_REQUIRE(!w4 || (g.shift0 >= 0 && 8ll * g.shift0 + g.n / 32 <= shifts_cap),
                          "%s: segment %d: shift bytes [%lld, +%lld) outside the %lld given", what, s, 8ll * g.shift0,
                          (long long)(g.n / 32), shifts_cap);
        }
        if (unpack) {
            MCAMD_REQUIRE(g.dense == 0 || g.dense == 1, "%s: segment %d: bad dense flag", what, s);
            MCAMD_REQUIRE(g.kept >= 0 && g.kept <= g.n, "%s: segment %d: kept %lld of %lld weights", what, s, (long long)g.kept,
                          (long long)g.n);
            const long long stored = (g.dense ? g.n : g.kept) * elem;
            MCAMD_REQUIRE(g.val0 >= 0 && g.val0 % 8 == 0 && g.val0 + stored <= values_bytes,
                          "%s: segment %d: values [%lld, +%lld) outside the %lld bytes given", what, s, (long long)g.val0, stored,
                          values_bytes);
        }
        cap += (g.n * elem + 7) / 8 * 8;
        blocks += (nwords + WZ_BW - 1) / WZ_BW;
        MCAMD_REQUIRE(blocks < (1ll << 31) && exps < (1ll << 31) && shifts < (1ll << 31), "%s: too many weights", what);
    }
    t->blocks = blocks, t->words = words, t->exps = exps, t->shifts = shifts, t->cap_bytes = cap;
    return MCAMD_OK;
}

// (shifts_cap < 0: mcamd_wz_pack, which has no shift bytes)
static int wz_pack_impl(const char* what, const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, uint64_t* words,
                        int64_t words_cap, uint64_t* counts, int32_t* exps, int64_t exps_cap, void* values, int64_t values_bytes,
                        void* workspace, size_t workspace_bytes, void* stream, uint8_t* shifts, int64_t shifts_cap) {
    MCAMD_REQUIRE(!mcamd_recording(), "%s: not recordable into a launch plan", what);
    MCAMD_REQUIRE(segs && segs_dev && nseg > 0 && words && counts && values && workspace, "%s: null argument", what);
    WzTotals t;
    const int rc = wz_check_table(what, segs, nseg, false, words_cap, exps_cap, shifts_cap, values_bytes, &t);
    if (rc) return rc;
    MCAMD_REQUIRE(words_cap >= t.words, "%s: %lld bit words needed, room for %lld", what, t.words, (long long)words_cap);
    MCAMD_REQUIRE(t.exps == 0 || (exps && exps_cap >= t.exps), "%s: %lld exponents needed, room for %lld", what, t.exps,
                  exps ? (long long)exps_cap : 0ll);
    MCAMD_REQUIRE(t.shifts == 0 || (shifts && shifts_cap >= 8 * t.shifts), "%s: %lld shift bytes needed, room for %lld", what,
                  8 * t.shifts, shifts ? (long long)shifts_cap : 0ll);
    MCAMD_REQUIRE(values_bytes >= t.cap_bytes, "%s: values need room for %lld bytes (every weight kept), got %lld", what, t.cap_bytes,
                  (long long)values_bytes);
    if (workspace_bytes < mcamd_wz_workspace_bytes(t.blocks, nseg)) {
        mcamd_set_error("%s: workspace too small", what);
        return MCAMD_EWORKSPACE;
    }
    const WzWork k = wz_work(workspace, t.blocks, nseg);
    hipStream_t st = (hipStream_t)stream;
    if (t.exps) hipLaunchKernelGGL(wz_exponent_kernel, dim3((int)t.exps), dim3(256), 0, st, segs_dev, nseg, exps, (unsigned char*)shifts);
    hipLaunchKernelGGL(wz_words_kernel, dim3((int)t.blocks), dim3(256), 0, st, segs_dev, nseg, (const int*)exps,
                       (const unsigned char*)shifts, (u64*)words, k.blocksum);
    hipLaunchKernelGGL(wz_scan_kernel<true>, dim3(1), dim3(64), 0, st, segs_dev, nseg, (const unsigned*)k.blocksum, k.blockoff,
                       (u64*)counts, k.segbase, k.dense);
    hipLaunchKernelGGL(wz_scatter_kernel, dim3((int)t.blocks), dim3(256), 0, st, segs_dev, nseg, (const int*)exps,
                       (const unsigned char*)shifts, (const u64*)words, (const u64*)k.blockoff, (const u64*)k.segbase,
                       (const int*)k.dense, (char*)values);
    MCAMD_LAUNCH_CHECK(what);
    return MCAMD_OK;
}

static int wz_unpack_impl(const char* what, const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, const uint64_t* words,
                          int64_t words_cap, const int32_t* exps, int64_t exps_cap, const void* values, int64_t values_bytes,
                          void* workspace, size_t workspace_bytes, void* stream, const uint8_t* shifts, int64_t shifts_cap) {
    MCAMD_REQUIRE(!mcamd_recording(), "%s: not recordable into a launch plan", what);
    MCAMD_REQUIRE(segs && segs_dev && nseg > 0 && values && values_bytes >= 0 && workspace, "%s: null argument", what);
    WzTotals t;
    const int rc = wz_check_table(what, segs, nseg, true, words ? words_cap : 0, exps ? exps_cap : 0,
                                  shifts_cap < 0 ? -1 : shifts ? shifts_cap : 0, values_bytes, &t);
    if (rc) return rc;
    if (workspace_bytes < mcamd_wz_workspace_bytes(t.blocks, nseg)) {
        mcamd_set_error("%s: workspace too small", what);
        return MCAMD_EWORKSPACE;
    }
    const WzWork k = wz_work(workspace, t.blocks, nseg);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(wz_popc_kernel, dim3((int)t.blocks), dim3(64), 0, st, segs_dev, nseg, (const u64*)words, k.blocksum);
    hipLaunchKernelGGL(wz_scan_kernel<false>, dim3(1), dim3(64), 0, st, segs_dev, nseg, (const unsigned*)k.blocksum, k.blockoff,
                       (u64*)nullptr, (u64*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(wz_expand_kernel, dim3((int)t.blocks), dim3(256), 0, st, segs_dev, nseg, (const int*)exps,
                       (const unsigned char*)shifts, (const u64*)words, (const u64*)k.blockoff, (const char*)values);
    MCAMD_LAUNCH_CHECK(what);
    return MCAMD_OK;
}

extern "C" int mcamd_wz_pack(const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, uint64_t* words, int64_t words_cap,
                             uint64_t* counts, int32_t* exps, int64_t exps_cap, void* values, int64_t values_bytes, void* workspace,
                             size_t workspace_bytes, void* stream) {
    return wz_pack_impl("wz_pack", segs, segs_dev, nseg, words, words_cap, counts, exps, exps_cap, values, values_bytes, workspace,
                        workspace_bytes, stream, nullptr, -1);
}

extern "C" int mcamd_wz_unpack(const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, const uint64_t* words,
                               int64_t words_cap, const int32_t* exps, int64_t exps_cap, const void* values, int64_t values_bytes,
                               void* workspace, size_t workspace_bytes, void* stream) {
    return wz_unpack_impl("wz_unpack", segs, segs_dev, nseg, words, words_cap, exps, exps_cap, values, values_bytes, workspace,
                          workspace_bytes, stream, nullptr, -1);
}

extern "C" int mcamd_wz_pack_w4(const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, uint64_t* words,
                                int64_t words_cap, uint64_t* counts, int32_t* exps, int64_t exps_cap, void* values,
                                int64_t values_bytes, void* workspace, size_t workspace_bytes, void* stream, uint8_t* shifts,
                                int64_t shifts_cap) {
    MCAMD_REQUIRE(shifts_cap >= 0, "wz_pack_w4: negative shifts_cap");
    return wz_pack_impl("wz_pack_w4", segs, segs_dev, nseg, words, words_cap, counts, exps, exps_cap, values, values_bytes, workspace,
                        workspace_bytes, stream, shifts, shifts_cap);
}

extern "C" int mcamd_wz_unpack_w4(const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, const uint64_t* words,
                                  int64_t words_cap, const int32_t* exps, int64_t exps_cap, const void* values, int64_t values_bytes,
                                  void* workspace, size_t workspace_bytes, void* stream, const uint8_t* shifts, int64_t shifts_cap) {
    MCAMD_REQUIRE(shifts_cap >= 0, "wz_unpack_w4: negative shifts_cap");
    return wz_unpack_impl("wz_unpack_w4", segs, segs_dev, nseg, words, words_cap, exps, exps_cap, values, values_bytes, workspace,
                          workspace_bytes, stream, shifts, shifts_cap);
}
