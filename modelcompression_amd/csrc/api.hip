// C-ABI entry points of libmcamd.so (see include/mcamd.h): argument validation, geometry ->
// launch descriptors, weight packing.  No allocation, no synchronisation.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "kernels.h"

static thread_local char g_err[512] = "";

void mcamd_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int g_mcamd_env_generation = 0;
int McamdEnvSlot::get(const char* name, int dflt) {
    const int g = __atomic_load_n(&g_mcamd_env_generation, __ATOMIC_ACQUIRE);
    if (gen != g) {       // (a race between host threads re-reads the same variable twice: harmless)
        const char* s = getenv(name);
        has = s && *s ? 1 : 0;
        val = has ? atoi(s) : 0;
        __atomic_store_n(&gen, g, __ATOMIC_RELEASE);
    }
    return has ? val : dflt;
}
extern "C" void mcamd_reload_config(void) { __atomic_add_fetch(&g_mcamd_env_generation, 1, __ATOMIC_ACQ_REL); }

extern "C" int mcamd_version(void) { return 101; }
extern "C" const char* mcamd_arch(void) { return "gfx950"; }
extern "C" const char* mcamd_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------------------
// geometry helpers
// ---------------------------------------------------------------------------------------
static int cin_tap_of(const mcamd_conv_geom* g) { return g->stem ? 32 : round_up_int(g->cin, 32); }
static int ntaps_of(const mcamd_conv_geom* g) { return g->stem ? 3 : g->ksize * g->ksize; }
static int cout_p_of(const mcamd_conv_geom* g) { return round_up_int(g->cout, 32); }
// padded pixels per row / rows per image of the operands (2: zero halo on every side; 1: shared-halo form, mcamd.h), and
// the number of padded pixels the 9-tap weight gradient enumerates
static int pw_of(const mcamd_conv_geom* g) { return g->pad ? 1 : 2; }
static long long padded_pixels(const mcamd_conv_geom* g) {
    const int pw = pw_of(g);
    return (long long)g->B * (g->H + pw) * (g->W + pw) + (pw == 1 ? g->W + 2 : 0);
}

static int check_geom(const mcamd_conv_geom* g, const char* what) {
    MCAMD_REQUIRE(g, "%s: null geometry", what);
    MCAMD_REQUIRE(g->B > 0 && g->H > 0 && g->W > 0 && g->cin > 0 && g->cout > 0, "%s: non-positive dimension", what);
    MCAMD_REQUIRE(g->ksize == 1 || g->ksize == 3, "%s: ksize %d unsupported (1 or 3)", what, g->ksize);
    MCAMD_REQUIRE((long long)g->B * g->H * g->W < (1ll << 31), "%s: more than 2^31 output pixels", what);
    MCAMD_REQUIRE(g->pad == 0 || (g->pad == 1 && !g->stem), "%s: pad must be 0 or 1 (and 0 for the stem layer)", what);
    if (g->stem) {
        MCAMD_REQUIRE(g->cin == 3 && g->ksize == 3 && g->x_ld == 4 && g->x_choff == 0,
                      "%s: stem form needs cin=3, ksize=3, x_ld=4, x_choff=0", what);
    } else {
        MCAMD_REQUIRE(g->x_ld % 8 == 0 && g->x_choff % 8 == 0, "%s: x_ld / x_choff must be multiples of 8", what);
        const int span = g->x_wrap > 0 ? g->x_wrap : cin_tap_of(g);
        MCAMD_REQUIRE(g->x_choff + span <= g->x_ld, "%s: x channel slice [%d, %d) exceeds x_ld %d", what,
                      g->x_choff, g->x_choff + span, g->x_ld);
    }
    if (g->x_f8 != 0) {
        MCAMD_REQUIRE(!g->stem && g->x_wrap == 0 && g->x_f8 > 0 && g->x_f8 % 64 == 0 && g->cin == 2 * g->x_f8 && g->x_choff == 0,
                      "%s: x_f8 %d needs cin = 2 P with P %% 64 == 0, no x_wrap, x_choff 0 (cin %d, x_choff %d)", what, g->x_f8, g->cin,
                      g->x_choff);
        MCAMD_REQUIRE(g->x_f8_wexp >= -24 && g->x_f8_wexp <= 40, "%s: x_f8_wexp %d outside [-24, 40]", what, g->x_f8_wexp);
    }
    if (g->x_wrap != 0) {
        const int ct = cin_tap_of(g), kb = ct % 64 == 0 ? 64 : 32;   // kblock_of(ct)
        MCAMD_REQUIRE(!g->stem && g->x_wrap > 0 && g->x_wrap % 64 == 0 && g->x_wrap % kb == 0 && g->cin == g->x_wrap / 2 * 3 && ct == g->cin,
                      "%s: x_wrap %d needs cin = 3 P, x_wrap = 2 P, P %% 32 == 0 (cin %d)", what, g->x_wrap, g->cin);
    }
    return MCAMD_OK;
}

// tap table relative to the row base = padded pixel (h, w) of output pixel (h, w), i.e. the
// top-left corner of its 3x3 window.
static void fill_taps(int ksize, int stem, int row_stride, int ld, int* taps) {
    if (stem) {
        for (int ty = 0; ty < 3; ++ty) taps[ty] = ty * row_stride;
    } else if (ksize == 3) {
        for (int ty = 0; ty < 3; ++ty)
            for (int tx = 0; tx < 3; ++tx) taps[ty * 3 + tx] = ty * row_stride + tx * ld;
    } else {
        taps[0] = row_stride + ld;  // centre pixel
    }
}

extern "C" int64_t mcamd_packed_elems_fwd(const mcamd_conv_geom* g) {
    if (!g) return 0;
    return (int64_t)round_up_int(g->cout, 256) * ntaps_of(g) * cin_tap_of(g);
}
extern "C" int64_t mcamd_packed_elems_dgrad(const mcamd_conv_geom* g) {
    if (!g || g->stem) return 0;
    return (int64_t)round_up_int(g->cin, 256) * g->ksize * g->ksize * cout_p_of(g);
}

// ---------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int round_up_dev(int v, int m) { return (v + m - 1) / m * m; }
// K order of the packed matrices: [channel block][tap][channel inside the block].  All taps of a 64-channel
// block are consecutive K chunks, so the nine shifted reads of the same activation lines follow each other
// closely and hit L2 instead of streaming the whole activation tile nine times from the Infinity Cache.
__host__ __device__ __forceinline__ int kblock_of(int ch_padded) { return ch_padded % 64 == 0 ? 64 : 32; }
// position of (tap t, channel c) inside one packed row of `taps` taps x `chp` padded channels
__host__ __device__ __forceinline__ int kpos(int t, int c, int taps, int chp) {
    const int kb = kblock_of(chp);
    return (c / kb) * taps * kb + t * kb + c % kb;
}

// `wlo` (may be NULL): the residual fp16(v - fp16(v)) of every entry in the same layout -- the lo half of split operands
__global__ __launch_bounds__(256) void pack_fwd_kernel(const float* w, const float* mask, half_t* wp, int Cout, int Cin,
                                                       int ks, int cin_tap, int stem, long long total, int ktot,
                                                       const int* rmap, const int* cmap, half_t* wlo = nullptr) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        int n = (int)(idx / ktot);
        int k = (int)(idx - (long long)n * ktot);
        float v = 0.f;
        if (n < Cout) {
            int c, ty, tx;
            bool ok;
            if (stem) {
                ty = k >> 5;
                int r = k & 31;
                tx = r >> 2;
                c = r & 3;
                ok = tx < 3 && c < 3;
            } else {
                const int kb = kblock_of(cin_tap), blk = ks * ks * kb;
                const int cb = k / blk, r = k - cb * blk;
                const int t = r / kb;
                c = cb * kb + (r - t * kb);
                ty = t / ks;
                tx = t - ty * ks;
                ok = c < Cin;
            }
            if (ok) {
                const int ns = rmap ? rmap[n] : n, cs = cmap ? cmap[c] : c;
                long long src = (((long long)ns * Cin + cs) * ks + ty) * ks + tx;
                v = w[src];
                if (mask) v *= mask[src];
            }
        }
        const half_t hv = (half_t)v;
        wp[idx] = hv;
        if (wlo) wlo[idx] = (half_t)(v - (float)hv);
    }
}

__global__ __launch_bounds__(256) void pack_dgrad_kernel(const float* w, const float* mask, half_t* wp, int Cout, int Cin,
                                                         int ks, int cout_p, long long total, int ktot,
                                                         const int* rmap, const int* cmap) {
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        int c = (int)(idx / ktot);
        int k = (int)(idx - (long long)c * ktot);
        const int kb = kblock_of(cout_p), blk = ks * ks * kb;
        const int nb = k / blk, r = k - nb * blk;
        int t = r / kb;
        int n = nb * kb + (r - t * kb);
        float v = 0.f;
        if (c < Cin && n < Cout) {
            int ty = t / ks, tx = t - ty * ks;
            const int ns = rmap ? rmap[n] : n, cs = cmap ? cmap[c] : c;
            long long src = (((long long)ns * Cin + cs) * ks + (ks - 1 - ty)) * ks + (ks - 1 - tx);
            v = w[src];
            if (mask) v *= mask[src];
        }
        wp[idx] = (half_t)v;
    }
}

extern "C" int mcamd_pack_weights(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw,
                                  const mcamd_chan_map* map, void* wp_fwd, void* wp_dgrad, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "pack_weights: null geometry");
        const mcamd_conv_geom g_ = *g;
        const bool has_map = map != nullptr;
        const mcamd_chan_map m_ = has_map ? *map : mcamd_chan_map{nullptr, nullptr};
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_pack_weights(&g_, w_oihw, mask_oihw, has_map ? &m_ : nullptr, wp_fwd, wp_dgrad, s); });
    }
    if (check_geom(g, "pack_weights")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(w_oihw, "pack_weights: null weights");
    const int* rmap = map ? (const int*)map->rows : nullptr;
    const int* cmap = map ? (const int*)map->cols : nullptr;
    MCAMD_REQUIRE(!(g->stem && cmap), "pack_weights: the stem layer takes no input-channel map");
    hipStream_t st = (hipStream_t)stream;
    if (wp_fwd) {
        int ktot = ntaps_of(g) * cin_tap_of(g);
        long long total = mcamd_packed_elems_fwd(g);
        long long grid = (total + 256 * 4 - 1) / (256 * 4);
        if (grid > 4096) grid = 4096;
        hipLaunchKernelGGL(pack_fwd_kernel, dim3((int)grid), dim3(256), 0, st, w_oihw, mask_oihw, (half_t*)wp_fwd, g->cout,
                           g->cin, g->ksize, cin_tap_of(g), g->stem, total, ktot, rmap, cmap);
    }
    if (wp_dgrad) {
        MCAMD_REQUIRE(!g->stem, "pack_weights: the stem layer has no dgrad packing");
        int ktot = g->ksize * g->ksize * cout_p_of(g);
        long long total = mcamd_packed_elems_dgrad(g);
        long long grid = (total + 256 * 4 - 1) / (256 * 4);
        if (grid > 4096) grid = 4096;
        hipLaunchKernelGGL(pack_dgrad_kernel, dim3((int)grid), dim3(256), 0, st, w_oihw, mask_oihw, (half_t*)wp_dgrad,
                           g->cout, g->cin, g->ksize, cout_p_of(g), total, ktot, rmap, cmap);
    }
    MCAMD_LAUNCH_CHECK("pack_weights");
    return MCAMD_OK;
}

extern "C" int mcamd_pack_stem_split(const float* w_oihw, const float* mask_oihw, int32_t cout, void* wp_hi, void* wp_lo,
                                     void* stream) {
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_pack_stem_split(w_oihw, mask_oihw, cout, wp_hi, wp_lo, s); });
    MCAMD_REQUIRE(w_oihw && wp_hi && wp_lo && cout > 0, "pack_stem_split: bad argument");
    mcamd_conv_geom g = {};
    g.B = 1, g.H = 2, g.W = 32, g.ksize = 3, g.cin = 3, g.cout = cout, g.x_ld = 4, g.stem = 1;
    const int ktot = ntaps_of(&g) * cin_tap_of(&g);
    const long long total = mcamd_packed_elems_fwd(&g);
    long long grid = (total + 256 * 4 - 1) / (256 * 4);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(pack_fwd_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, w_oihw, mask_oihw, (half_t*)wp_hi,
                       cout, 3, 3, cin_tap_of(&g), 1, total, ktot, (const int*)nullptr, (const int*)nullptr, (half_t*)wp_lo);
    MCAMD_LAUNCH_CHECK("pack_stem_split");
    return MCAMD_OK;
}

// All layers in one launch: a workgroup packs a 32-filter x 32-channel tile of one layer into both layouts.
// Wide accesses on both sides: a tile row (32 channels x k*k taps of one filter) is one contiguous run of the OIHW master
// and is read as float4s; both fp16 layouts keep 8 consecutive channels (forward) / 8 consecutive filters (dgrad) of one
// tap adjacent, so a lane writes 16 bytes.  (2-byte stores and nine 4-byte loads per lane: 164 us for the 405 MB of a
// YOLOv2 re-pack = 2.5 TB/s, the instruction count being the bound.)
__global__ __launch_bounds__(256) void pack_tiles_kernel(const mcamd_pack_job* jobs, int njobs, long long total) {
    constexpr int TS = 32, LDW = TS * 9 + 1;           // row stride of the LDS tile (odd: column reads spread over banks)
    __shared__ float tile[TS * LDW];                    // [n][c * kk + t], 37 KB
    for (long long item = blockIdx.x; item < total; item += gridDim.x) {
        int lo = 0, hi = njobs - 1;                     // last job whose first_tile <= item
        while (lo < hi) {
            int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].first_tile <= item) lo = mid;
            else hi = mid - 1;
        }
        const mcamd_pack_job j = jobs[lo];
        const int ks = j.ksize, kk = ks * ks;
        const int ctiles = (j.cin + TS - 1) / TS;
        const int r = (int)(item - j.first_tile);
        const int n0 = (r / ctiles) * TS, c0 = (r - (r / ctiles) * ctiles) * TS;
        __syncthreads();                                // the previous item's readers are done with the tile
        // 1. gather.  Without an input-channel map a full tile row is TS * kk contiguous floats of the master
        const bool rows_contig = !j.cols && c0 + TS <= j.cin && ((long long)j.cin * kk) % 4 == 0 && (c0 * kk) % 4 == 0;
        if (rows_contig) {
            const int q4 = TS * kk / 4;                 // float4s per row (72 or 8)
            for (int e = threadIdx.x; e < TS * q4; e += 256) {
                const int nl = e / q4, q = (e - nl * q4) * 4;
                const int n = n0 + nl;
                f32x4_t v = {0.f, 0.f, 0.f, 0.f};
                if (n < j.cout) {
                    const int ns = j.rows ? j.rows[n] : n;
                    const long long src = ((long long)ns * j.cin + c0) * kk + q;
                    v = *(const f32x4_t*)(j.w + src);
                    if (j.mask) {
                        const f32x4_t m = *(const f32x4_t*)(j.mask + src);
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = v[i] * m[i];
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) tile[nl * LDW + q + i] = v[i];
            }
        } else {
            // thread -> (n, c) pairs, c fastest: the k*k taps of a pair are one contiguous run
            for (int pair = threadIdx.x; pair < TS * TS; pair += 256) {
                const int nl = pair / TS, cl = pair - nl * TS;
                const int n = n0 + nl, c = c0 + cl;
                float v[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) v[t] = 0.f;
                if (n < j.cout && c < j.cin) {
                    const int ns = j.rows ? j.rows[n] : n, cs = j.cols ? j.cols[c] : c;
                    const long long src = ((long long)ns * j.cin + cs) * kk;
#pragma unroll
                    for (int t = 0; t < 9; ++t)
                        if (t < kk) v[t] = j.mask ? j.w[src + t] * j.mask[src + t] : j.w[src + t];
                }
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    if (t < kk) tile[nl * LDW + cl * kk + t] = v[t];
            }
        }
        __syncthreads();
        // 2. forward layout [n][kpos(t, c)]: 8 consecutive channels of one (filter, tap) per lane = one 16-byte store.
        // j.split: the split-operand packing [w_hi | w_hi | w_lo] along the input channels (w_hi = fp16(w * mask),
        // w_lo = fp16(w * mask - w_hi)), i.e. channel c is written at c, cin + c and 2 cin + c of a 3 cin wide row.
        if (j.dst_fwd && j.split == 2) {
            // fp8 correction packing (mcamd_conv_geom.x_f8): a row of 2 cin fp16 units per tap = [w_hi: cin fp16 | w8: cin
            // e4m3 bytes | wlo8: cin bytes], the byte string cut into the same [channel block][tap][64] K order as the
            // activations' [x_hi | lo8 | x8].  cin % 64 == 0 (host-checked).
            half_t* dst = (half_t*)j.dst_fwd;
            const int cin_tap = 2 * j.cin;
            for (int e = threadIdx.x; e < TS * kk * (TS / 8); e += 256) {
                const int g8 = e % (TS / 8), t = (e / (TS / 8)) % kk, nl = e / ((TS / 8) * kk);
                const int n = n0 + nl, c = c0 + g8 * 8;
                if (n >= j.cout || c >= j.cin) continue;
                const float* src = tile + nl * LDW + (g8 * 8) * kk + t;
                half_t* row = dst + (long long)n * kk * cin_tap;
                h8_t h;
                float q8[8], ql[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float v = src[i * kk];
                    h[i] = (half_t)v;
                    q8[i] = fminf(fmaxf(ldexpf((float)h[i], j.f8_wexp), -448.f), 448.f);
                    ql[i] = fminf(fmaxf(ldexpf(v - (float)h[i], j.f8_wexp + 11), -448.f), 448.f);
                }
                *(h8_t*)(row + kpos(t, c, kk, cin_tap)) = h;
                int w8[2], wl[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    w8[i] = __builtin_amdgcn_cvt_pk_fp8_f32(q8[4 * i], q8[4 * i + 1], 0, false);
                    w8[i] = __builtin_amdgcn_cvt_pk_fp8_f32(q8[4 * i + 2], q8[4 * i + 3], w8[i], true);
                    wl[i] = __builtin_amdgcn_cvt_pk_fp8_f32(ql[4 * i], ql[4 * i + 1], 0, false);
                    wl[i] = __builtin_amdgcn_cvt_pk_fp8_f32(ql[4 * i + 2], ql[4 * i + 3], wl[i], true);
                }
                // e4m3 element e of the tap's [w8 | wlo8] string lives in byte (e & 1) of fp16 unit cin + e / 2
                int* d8 = (int*)(row + kpos(t, j.cin + c / 2, kk, cin_tap));
                d8[0] = w8[0], d8[1] = w8[1];
                int* dl = (int*)(row + kpos(t, j.cin + (j.cin + c) / 2, kk, cin_tap));
                dl[0] = wl[0], dl[1] = wl[1];
            }
        } else if (j.dst_fwd) {
            half_t* dst = (half_t*)j.dst_fwd;
            const int parts = j.split ? 3 : 1;
            const int cin_tap = round_up_dev(j.cin * parts, 32);
            const bool vec_ok = parts == 1 || j.cin % 8 == 0;
            for (int e = threadIdx.x; e < TS * kk * (TS / 8); e += 256) {
                const int g8 = e % (TS / 8), t = (e / (TS / 8)) % kk, nl = e / ((TS / 8) * kk);
                const int n = n0 + nl, c = c0 + g8 * 8;
                if (n >= j.cout || c >= j.cin) continue;
                const float* src = tile + nl * LDW + (g8 * 8) * kk + t;
                const int lim = c + 8 <= j.cin ? 8 : j.cin - c;
                for (int part = 0; part < parts; ++part) {
                    half_t* d = dst + (long long)n * kk * cin_tap + kpos(t, c + part * j.cin, kk, cin_tap);
                    h8_t h;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float v = i < lim ? src[i * kk] : 0.f;
                        const half_t hi = (half_t)v;
                        h[i] = part < 2 ? hi : (half_t)(v - (float)hi);
                    }
                    if (lim == 8 && vec_ok) {
                        *(h8_t*)d = h;
                    } else {
                        for (int i = 0; i < lim; ++i) dst[(long long)n * kk * cin_tap + kpos(t, c + i + part * j.cin, kk, cin_tap)] = h[i];
                    }
                }
            }
        }
        // 3. dgrad layout [c][kpos(t', n)], flipped taps: 8 consecutive filters of one (channel, tap) per lane
        if (j.dst_dgrad) {
            half_t* dst = (half_t*)j.dst_dgrad;
            const int cout_p = round_up_dev(j.cout, 32);
            for (int e = threadIdx.x; e < TS * kk * (TS / 8); e += 256) {
                const int g8 = e % (TS / 8), t = (e / (TS / 8)) % kk, cl = e / ((TS / 8) * kk);
                const int n = n0 + g8 * 8, c = c0 + cl;
                if (n >= j.cout || c >= j.cin) continue;
                half_t* d = dst + (long long)c * kk * cout_p + kpos(t, n, kk, cout_p);
                const float* src = tile + (g8 * 8) * LDW + cl * kk + (kk - 1 - t);
                if (n + 8 <= j.cout) {
                    h8_t h;
#pragma unroll
                    for (int i = 0; i < 8; ++i) h[i] = (half_t)src[i * LDW];
                    *(h8_t*)d = h;
                } else {
                    for (int i = 0; n + i < j.cout; ++i) d[i] = (half_t)src[i * LDW];
                }
            }
        }
    }
}

extern "C" int mcamd_pack_weights_many(const mcamd_pack_job* jobs_dev, int32_t njobs, int64_t total_tiles, void* stream) {
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_pack_weights_many(jobs_dev, njobs, total_tiles, s); });
    MCAMD_REQUIRE(jobs_dev && njobs > 0 && total_tiles > 0, "pack_weights_many: empty job table");
    long long grid = total_tiles;
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(pack_tiles_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, jobs_dev, njobs,
                       (long long)total_tiles);
    MCAMD_LAUNCH_CHECK("pack_weights_many");
    return MCAMD_OK;
}

// ---------------------------------------------------------------------------------------
// forward / dgrad
// ---------------------------------------------------------------------------------------
// The operand side of a launch descriptor, shared by forward, 2:4 forward and dgrad: a padded NHWC operand `x` (`ld` elements per
// pixel, slice at channel `choff`) with `ch_tap` channels per tap on the K side, `n` output columns.  No x_wrap / x_f8.
static void fill_operand(IgemmArgs& a, const mcamd_conv_geom* g, const void* x, const void* w, int ld, int choff, int n,
                         int ch_tap, int stem) {
    memset(&a, 0, sizeof(a));
    a.x = (const half_t*)x;
    a.w = (const half_t*)w;
    a.x_ld = ld;
    a.x_row_stride = (g->W + pw_of(g)) * ld;
    a.x_img_stride = (long long)(g->H + pw_of(g)) * a.x_row_stride;
    a.x_off = choff;
    a.H = g->H, a.W = g->W, a.HW = g->H * g->W;
    a.M = g->B * g->H * g->W;
    a.N = n;
    a.cin_tap = ch_tap;
    a.ntaps = stem ? 3 : g->ksize * g->ksize;
    a.kb = kblock_of(ch_tap);
    a.ktot = a.ntaps * ch_tap;
    fill_taps(g->ksize, stem, a.x_row_stride, ld, a.tap_off);
    a.wrap = 0x7fffffff;
    a.f8_from = 0x7fffffff;
}

// `rows`: the statistics rows of the kernel the launch takes (ConvRoute.rows)
static int fill_epilogue(IgemmArgs& a, const mcamd_conv_epilogue* e, int n_out, const char* what, int rows) {
    MCAMD_REQUIRE(e && e->y, "%s: null output", what);
    a.y = e->y;
    a.mode = e->mode;
    a.bias = nullptr;
    a.stats = nullptr;
    a.scale = nullptr;
    a.shift = nullptr;
    a.slope = 1.f;
    a.y_ld = e->y_ld;
    a.y_choff = e->y_choff;
    a.stats_ld = 0;
    a.overflow = (int*)e->overflow;
    if (e->mode == MCAMD_EPI_NCHW_F32) {
        a.bias = e->bias;
    } else if (e->mode == MCAMD_EPI_RAW_F16 || e->mode == MCAMD_EPI_PAD_F16) {
        MCAMD_REQUIRE(n_out % 8 == 0, "%s: fp16 output needs a channel count that is a multiple of 8 (got %d)", what, n_out);
        MCAMD_REQUIRE(e->y_ld % 8 == 0 && e->y_choff % 8 == 0 && e->y_choff + n_out <= e->y_ld,
                      "%s: output slice [%d, %d) does not fit y_ld %d", what, e->y_choff, e->y_choff + n_out, e->y_ld);
        if (e->mode == MCAMD_EPI_RAW_F16 && e->stats) {
            MCAMD_REQUIRE(e->stats_rows == rows, "%s: stats_rows must be mcamd_conv_stats_rows() = %d (got %d)", what, rows,
                          e->stats_rows);
            MCAMD_REQUIRE(e->stats_ld >= round_up_int(n_out, 256), "%s: stats_ld must be >= %d", what,
                          round_up_int(n_out, 256));
            a.stats = e->stats;
            a.stats_ld = e->stats_ld;
        }
        if (e->mode == MCAMD_EPI_PAD_F16) {
            a.scale = e->scale;
            a.shift = e->shift;
            a.slope = e->slope;
            MCAMD_REQUIRE(e->dst_mode == MCAMD_DST_PLAIN || e->dst_mode == MCAMD_DST_POOL || e->dst_mode == MCAMD_DST_REORG,
                          "%s: bad dst_mode %d", what, e->dst_mode);
            if (e->dst_mode != MCAMD_DST_PLAIN) {
                MCAMD_REQUIRE(a.H % 2 == 0 && a.W % 2 == 0 && a.ntaps > 0 && !a.stats, "%s: pooled / reorg epilogue needs even H and W", what);
                const int span = e->dst_mode == MCAMD_DST_REORG ? 4 * n_out : n_out;
                MCAMD_REQUIRE(e->y_choff + span <= e->y_ld, "%s: pooled output slice [%d, %d) does not fit y_ld %d", what, e->y_choff,
                              e->y_choff + span, e->y_ld);
                MCAMD_REQUIRE(!e->y2 || (e->dst_mode == MCAMD_DST_POOL && e->y2_ld % 8 == 0 && e->y2_choff % 8 == 0 &&
                                         e->y2_choff + n_out <= e->y2_ld),
                              "%s: y2 (full-resolution copy) needs dst_mode POOL and a fitting slice", what);
                a.dst_mode = e->dst_mode;
                a.y2 = e->y2;
                a.y2_ld = e->y2_ld, a.y2_choff = e->y2_choff;
            }
        } else {
            MCAMD_REQUIRE(e->dst_mode == 0 && !e->y2, "%s: dst_mode / y2 belong to epilogue mode 2 (MCAMD_EPI_PAD_F16)", what);
        }
    } else if (e->mode == MCAMD_EPI_RAW_F32) {
        MCAMD_REQUIRE(e->y_ld % 4 == 0 && e->y_choff % 4 == 0 && e->y_choff + n_out <= e->y_ld,
                      "%s: fp32 output slice [%d, %d) does not fit y_ld %d", what, e->y_choff, e->y_choff + n_out, e->y_ld);
        if (e->stats) {
            MCAMD_REQUIRE(e->stats_rows == rows, "%s: stats_rows must be %d, what the row query of this launch returns (got %d)", what,
                          rows, e->stats_rows);
            MCAMD_REQUIRE(e->stats_ld >= round_up_int(n_out, 256), "%s: stats_ld must be >= %d", what,
                          round_up_int(n_out, 256));
            a.stats = e->stats;
            a.stats_ld = e->stats_ld;
        }
    } else {
        MCAMD_REQUIRE(false, "%s: bad epilogue mode %d", what, e->mode);
    }
    return MCAMD_OK;
}

// The one place that decides which kernel a geometry takes, with which tile, and how many statistics rows it writes: the
// size queries, mcamd_conv_tile_info and the launches all ask here, so they cannot disagree.  `dir` = the `dgrad` argument
// of mcamd_conv_tile_info; `stats`: the epilogue writes BatchNorm partial sums.
enum { DIR_FWD = 0, DIR_DGRAD = 1, DIR_DGRAD_CONCURRENT = 2 };
static ConvRoute conv_route(const mcamd_conv_geom* g, int dir, int mode, int dst_mode, bool stats) {
    const long long M = (long long)g->B * g->H * g->W;
    const bool fwd = dir == DIR_FWD;
    const int n = fwd ? g->cout : g->cin;
    int ct = fwd ? cin_tap_of(g) : cout_p_of(g), ktot = (fwd ? ntaps_of(g) : g->ksize * g->ksize) * ct;
    if (fwd && mcamd_stem_direct_ok(g->stem, n, mode))   // conv_stem.hip: weights in registers, image fragments straight from global memory
        return {ROUTE_STEM, 32, n, 48, mcamd_stem_rows(M)};
    if (fwd && dst_mode == MCAMD_DST_PLAIN && g->pad == 0 && g->x_f8 == 0 &&
        mcamd_wres_ok(g->ksize, g->stem, n, ct, ktot, g->B, g->H, g->W, mode))   // conv_wres.hip: weights resident in registers
        return {ROUTE_WRES, 128, 128, 64, mcamd_wres_rows(n, g->B, g->H, g->W)};
    if (fwd && g->pad == 0 && !g->stem && g->x_choff == 0 && g->x_f8 == 0 &&
        mcamd_small3x3_split_ok(M, n, ct, ktot, g->x_wrap, mode))   // conv_small.hip: weights resident, split operands
        return {ROUTE_SMALL3X3_SPLIT, 32, round_up_int(n, 32), ct, mcamd_small3x3_rows(M)};
    if (mcamd_win3x3_ok(mode, stats, M, n, ct, ktot, g->H, g->W))   // conv2 dgrad: rolling LDS window (conv_win.hip)
        return {ROUTE_WIN3X3, 32, round_up_int(n, 16), 64, 0};
    // (the fp8 correction form, mcamd_conv_geom.x_f8: K is 2/3 of the three-product problem's; the tile is chosen for that
    // problem, so that a layer takes the same tile -- and the same statistics slab -- in either form)
    if (fwd && g->x_f8 > 0 && mode == MCAMD_EPI_RAW_F32) ct = ct / 2 * 3, ktot = ktot / 2 * 3;   // (x_f8 launches with mode 3 only)
    return mcamd_igemm_route(M, n, ct, ktot, mode == MCAMD_EPI_RAW_F16, dir == DIR_DGRAD_CONCURRENT);   // stats slabs only exist with RAW
}

static int launch_route(IgemmArgs& a, const ConvRoute& r, const mcamd_conv_geom* g, hipStream_t st) {
    switch (r.kernel) {
    case ROUTE_STEM: {
        StemArgs q;
        q.x = a.x, q.w = a.w, q.y = (half_t*)a.y, q.stats = a.stats;
        q.y_ld = a.y_ld, q.y_choff = a.y_choff, q.stats_ld = a.stats_ld;
        q.H = g->H, q.W = g->W, q.HW = a.HW, q.M = a.M;
        return mcamd_stem_launch(q, g->cout, r.rows, st);
    }
    case ROUTE_WRES: return mcamd_wres_launch(a, g->B, r.rows, st);
    case ROUTE_SMALL3X3_SPLIT: return mcamd_small3x3_split_launch(a, r.rows, st);
    case ROUTE_SMALL3X3: return mcamd_small3x3_launch(a, r.rows, st);
    case ROUTE_WIN3X3: return mcamd_win3x3_launch(a, st);
    default: return mcamd_igemm_launch(a, r, st);   // ROUTE_IGEMM, ROUTE_PP
    }
}

extern "C" int32_t mcamd_conv_stats_rows_mode(const mcamd_conv_geom* g, int32_t mode) {
    if (!g) return 0;
    return conv_route(g, DIR_FWD, mode == MCAMD_EPI_RAW_F32 ? MCAMD_EPI_RAW_F32 : MCAMD_EPI_RAW_F16, MCAMD_DST_PLAIN, true).rows;
}

extern "C" int32_t mcamd_conv_stats_rows(const mcamd_conv_geom* g) { return mcamd_conv_stats_rows_mode(g, MCAMD_EPI_RAW_F16); }

extern "C" int32_t mcamd_conv_fwd_f8_ok(const mcamd_conv_geom* g) {
    if (!g || g->x_f8 <= 0 || g->x_f8 % 64 != 0 || g->cin != 2 * g->x_f8 || g->stem || g->x_wrap != 0 || g->x_choff != 0) return 0;
    return conv_route(g, DIR_FWD, MCAMD_EPI_RAW_F32, MCAMD_DST_PLAIN, true).kernel == ROUTE_PP ? 1 : 0;   // the three-product problem takes the ping-pong tile
}

// forward: with statistics, fp32 epilogue (mode 3) for the x_wrap / x_f8 forms, which only exist with it; dgrad: mode 0
extern "C" int mcamd_conv_tile_info(const mcamd_conv_geom* g, int32_t dgrad, int32_t out[4]) {
    if (check_geom(g, "conv_tile_info")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(out, "conv_tile_info: null output");
    const bool f32 = !dgrad && (g->x_wrap > 0 || g->x_f8 > 0);
    const ConvRoute r = conv_route(g, dgrad, f32 ? MCAMD_EPI_RAW_F32 : MCAMD_EPI_RAW_F16, MCAMD_DST_PLAIN, !dgrad);
    out[0] = r.bm, out[1] = r.bn, out[2] = r.bk, out[3] = r.kernel;
    return MCAMD_OK;
}

// conv_route()'s answer for any (direction, epilogue mode, destination form, statistics) a launch can have
extern "C" int mcamd_conv_route_info(const mcamd_conv_geom* g, int32_t dir, int32_t mode, int32_t dst_mode, int32_t stats,
                                     int32_t out[5]) {
    if (check_geom(g, "conv_route_info")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(out, "conv_route_info: null output");
    MCAMD_REQUIRE(dir == DIR_FWD || dir == DIR_DGRAD || dir == DIR_DGRAD_CONCURRENT, "conv_route_info: bad direction %d", dir);
    MCAMD_REQUIRE(mode >= MCAMD_EPI_RAW_F16 && mode <= MCAMD_EPI_RAW_F32, "conv_route_info: bad epilogue mode %d", mode);
    MCAMD_REQUIRE(dst_mode == MCAMD_DST_PLAIN || dst_mode == MCAMD_DST_POOL || dst_mode == MCAMD_DST_REORG,
                  "conv_route_info: bad dst_mode %d", dst_mode);
    const ConvRoute r = conv_route(g, dir, mode, dst_mode, stats != 0);
    out[0] = r.bm, out[1] = r.bn, out[2] = r.bk, out[3] = r.kernel, out[4] = r.rows;
    return MCAMD_OK;
}

extern "C" int mcamd_conv_fwd(const mcamd_conv_geom* g, const void* x, const void* wp_fwd, const mcamd_conv_epilogue* epi,
                              void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd(&g_, x, wp_fwd, &e_, s); });
    }
    if (check_geom(g, "conv_fwd")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(x && wp_fwd && epi, "conv_fwd: null input / epilogue");
    IgemmArgs a;
    fill_operand(a, g, x, wp_fwd, g->x_ld, g->x_choff, g->cout, cin_tap_of(g), g->stem);
    MCAMD_REQUIRE(g->x_wrap == 0 || epi->mode == MCAMD_EPI_RAW_F32 || epi->mode == MCAMD_EPI_NCHW_F32,
                  "conv_fwd: x_wrap goes with the fp32 epilogues (modes 3 and 1)");
    if (g->x_wrap > 0) a.wrap = g->x_wrap;
    // x_f8: channel blocks [P, 2 P) of the slice are e4m3 bytes; K order [channel block][tap][kb] -> the fp8 chunks are the tail
    if (g->x_f8 > 0) a.f8_from = (g->x_f8 / a.kb) * a.ntaps * (a.kb / 32);
    a.f8_sb = (127 - (MCAMD_F8_SXL + g->x_f8_wexp)) * 0x01010101;
    const ConvRoute r = conv_route(g, DIR_FWD, epi->mode, epi->dst_mode, epi->stats != nullptr);
    if (g->x_f8 > 0) {
        MCAMD_REQUIRE(epi->mode == MCAMD_EPI_RAW_F32, "conv_fwd: x_f8 goes with the fp32 epilogue (mode 3)");
        MCAMD_REQUIRE(r.kernel == ROUTE_PP, "conv_fwd: no fp8-correction kernel for this shape (mcamd_conv_fwd_f8_ok)");
    }
    if (fill_epilogue(a, epi, g->cout, "conv_fwd", r.rows)) return MCAMD_EINVAL;
    return launch_route(a, r, g, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// BatchNorm + LeakyReLU fused into the 1x1 split-operand forward behind it (bn_conv1x1.hip)
// ---------------------------------------------------------------------------------------
// Host logic only.  NULL = the pair (activation pass `d`, consumer forward `g`) has a fused launch; else why not.  *r: the
// route of the consumer's own forward, whose persistent slots (statistics rows) the fused launch keeps.
static const char* bn_conv1x1_refusal(const mcamd_act_desc* d, const mcamd_conv_geom* g, ConvRoute* r) {
    if (!d || !g) return "null descriptor";
    if (check_geom(g, "bn_act_conv1x1")) return mcamd_last_error();
    if (g->ksize != 1 || g->stem) return "the consumer is not a 1x1 convolution";
    if (g->x_f8 != 0) return "fp8 correction operands (x_f8)";
    if (g->pad != 0 || d->dst_pad != 0) return "shared-halo destination";
    const int P = g->x_wrap / 2;
    if (g->x_wrap <= 0 || g->cin != 3 * P) return "the consumer does not multiply split operands on two planes (x_wrap)";
    if (P % 64 != 0) return "input channels must be a multiple of 64";
    if (!mcamd_bn_conv1x1_shape_ok(P, g->cout)) return "no kernel instance: cout <= 128 in steps of 8, cin <= 128 (cout <= 64) or 256";
    if (d->mode != MCAMD_DST_PLAIN || d->dst2 || d->pool_act || d->dst_q8 || d->dst2_q8) return "the producer is not a PLAIN block with one destination";
    if (d->border) return "border table";
    if (d->B != g->B || d->H != g->H || d->W != g->W) return "producer and consumer differ in B x H x W";
    if (d->C != P || d->planes != 2 || d->dst_plane != P || d->dst_ld != g->x_ld || d->dst_choff != g->x_choff)
        return "the producer's hi | lo planes are not the consumer's input slice";
    if (d->y_dtype != 1 || d->y_ld % 4 != 0 || d->y_choff % 4 != 0 || d->y_choff + P > d->y_ld) return "the raw output must be an fp32 slice in steps of 4 channels";
    *r = conv_route(g, DIR_FWD, MCAMD_EPI_RAW_F32, MCAMD_DST_PLAIN, true);
    // (igemm_kernel's 32-column tile has wave rows of 32 pixels, the wider ones of 64: another order of the partial sums)
    if (r->kernel != ROUTE_IGEMM || r->bm != 128 || r->bn < 64) return "the consumer's own forward does not take 128-pixel igemm tiles in wave rows of 64";
    return nullptr;
}

extern "C" int32_t mcamd_bn_act_conv1x1_ok(const mcamd_act_desc* d, const mcamd_conv_geom* g) {
    ConvRoute r;
    return bn_conv1x1_refusal(d, g, &r) ? 0 : 1;
}

extern "C" int32_t mcamd_bn_act_conv1x1_stats_rows(const mcamd_act_desc* d, const mcamd_conv_geom* g) {
    ConvRoute r;
    return bn_conv1x1_refusal(d, g, &r) ? 0 : r.rows;
}

// what the launch below will choose: the same refusal function, the same choice function (bn_conv1x1.hip)
extern "C" int mcamd_bn_act_conv1x1_info(const mcamd_act_desc* d, const mcamd_conv_geom* g, mcamd_bn_conv1x1_instance* out) {
    ConvRoute r;
    const char* why = bn_conv1x1_refusal(d, g, &r);
    if (why) {
        const std::string w(why);   // (may be the error buffer itself)
        mcamd_set_error("bn_act_conv1x1_info: %s (mcamd_bn_act_conv1x1_ok)", w.c_str());
        return MCAMD_EINVAL;
    }
    MCAMD_REQUIRE(out, "bn_act_conv1x1_info: null output");
    BnConv1x1Choice c;
    MCAMD_REQUIRE(mcamd_bn_conv1x1_choice(g->x_wrap / 2, g->cout, (long long)g->B * g->H * g->W, r.rows, &c),
                  "bn_act_conv1x1_info: no kernel instance for %d -> %d channels", g->x_wrap / 2, g->cout);
    out->bn = c.bn, out->cb = c.cb, out->threads = c.threads, out->rows = c.rows;
    out->num_mtiles = c.num_mtiles, out->grid = c.grid, out->lds_bytes = c.lds_bytes;
    return MCAMD_OK;
}

extern "C" int mcamd_bn_act_conv1x1_fwd(const mcamd_act_desc* d, const mcamd_conv_geom* g, const void* wp_fwd,
                                        const mcamd_conv_epilogue* epi, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(d && g && epi, "bn_act_conv1x1_fwd: null descriptor / geometry / epilogue");
        const mcamd_act_desc d_ = *d;
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_bn_act_conv1x1_fwd(&d_, &g_, wp_fwd, &e_, s); });
    }
    ConvRoute r;
    const char* why = bn_conv1x1_refusal(d, g, &r);
    if (why) {
        const std::string w(why);   // (may be the error buffer itself)
        mcamd_set_error("bn_act_conv1x1_fwd: %s (mcamd_bn_act_conv1x1_ok)", w.c_str());
        return MCAMD_EINVAL;
    }
    MCAMD_REQUIRE(d->y && d->scale && d->shift && d->dst && wp_fwd && epi, "bn_act_conv1x1_fwd: null input / epilogue");
    MCAMD_REQUIRE(epi->mode == MCAMD_EPI_RAW_F32, "bn_act_conv1x1_fwd: epilogue mode 3 (MCAMD_EPI_RAW_F32) only");
    IgemmArgs a;
    fill_operand(a, g, d->dst, wp_fwd, g->x_ld, g->x_choff, g->cout, cin_tap_of(g), 0);
    a.wrap = g->x_wrap;
    if (fill_epilogue(a, epi, g->cout, "bn_act_conv1x1_fwd", r.rows)) return MCAMD_EINVAL;
    a.scale = d->scale, a.shift = d->shift, a.slope = d->slope;
    return mcamd_bn_conv1x1_launch(a, (const float*)d->y, d->y_ld, d->y_choff, g->x_wrap / 2, r.rows, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// 2:4 structured sparsity (conv_sparse.hip; an addition beyond the reference)
// ---------------------------------------------------------------------------------------
extern "C" int32_t mcamd_conv_fwd_sparse24_ok(const mcamd_conv_geom* g) {
    if (!g || g->stem || g->x_wrap != 0 || g->x_f8 != 0 || (g->ksize != 1 && g->ksize != 3)) return 0;
    if (g->B <= 0 || g->H <= 0 || g->W <= 0 || g->cin <= 0 || g->cout <= 0) return 0;
    if (g->cin % 4 != 0 || g->cout % 8 != 0 || (long long)g->B * g->H * g->W >= (1ll << 31)) return 0;
    if (g->pad != 0 && g->pad != 1) return 0;
    if (g->x_ld % 8 != 0 || g->x_choff % 8 != 0 || g->x_choff + cin_tap_of(g) > g->x_ld) return 0;
    return 1;
}

extern "C" int mcamd_sparse24_elems(const mcamd_conv_geom* g, int64_t out[2]) {
    MCAMD_REQUIRE(g && out, "sparse24_elems: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_sparse24_ok(g), "sparse24_elems: geometry has no 2:4 form (mcamd_conv_fwd_sparse24_ok)");
    const long long npad = round_up_int(g->cout, 256), ktot = (long long)ntaps_of(g) * cin_tap_of(g);
    out[0] = npad * ktot / 2;      // kept fp16 values
    out[1] = npad * ktot / 16;     // 16-bit index words
    return MCAMD_OK;
}

// mcamd_sparse24_choice()'s answer: what mcamd_conv_fwd_sparse24 launches for this geometry (host logic only)
extern "C" int mcamd_conv_fwd_sparse24_info(const mcamd_conv_geom* g, int32_t out[7]) {
    MCAMD_REQUIRE(g && out, "conv_fwd_sparse24_info: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_sparse24_ok(g), "conv_fwd_sparse24_info: geometry has no 2:4 form (mcamd_conv_fwd_sparse24_ok)");
    const Sparse24Choice c = mcamd_sparse24_choice((long long)g->B * g->H * g->W, g->cout, kblock_of(cin_tap_of(g)));
    out[0] = c.bmw, out[1] = c.bnp, out[2] = c.bk, out[3] = c.stages, out[4] = c.mtiles, out[5] = c.ntiles, out[6] = c.grid;
    return MCAMD_OK;
}

extern "C" int mcamd_pack_sparse24(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* wsp, void* idx,
                                   void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "pack_sparse24: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_pack_sparse24(&g_, w_oihw, mask_oihw, wsp, idx, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_sparse24_ok(g), "pack_sparse24: geometry has no 2:4 form (mcamd_conv_fwd_sparse24_ok)");
    MCAMD_REQUIRE(w_oihw && wsp && idx, "pack_sparse24: null pointer");
    const int ct = cin_tap_of(g);
    return mcamd_pack_sparse24_launch(w_oihw, mask_oihw, wsp, idx, g->cout, g->cin, ntaps_of(g), ct, kblock_of(ct),
                                      (hipStream_t)stream);
}

extern "C" int mcamd_conv_fwd_sparse24(const mcamd_conv_geom* g, const void* x, const void* wsp, const void* idx,
                                       const mcamd_conv_epilogue* epi, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_sparse24: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_sparse24(&g_, x, wsp, idx, &e_, s); });
    }
    if (check_geom(g, "conv_fwd_sparse24")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_fwd_sparse24_ok(g), "conv_fwd_sparse24: geometry has no 2:4 form (mcamd_conv_fwd_sparse24_ok)");
    MCAMD_REQUIRE(x && wsp && idx, "conv_fwd_sparse24: null input");
    MCAMD_REQUIRE(epi && epi->mode == MCAMD_EPI_PAD_F16, "conv_fwd_sparse24: epilogue mode 2 (MCAMD_EPI_PAD_F16) only");
    IgemmArgs a;
    fill_operand(a, g, x, wsp, g->x_ld, g->x_choff, g->cout, cin_tap_of(g), 0);
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_sparse24", 0)) return MCAMD_EINVAL;   // (mode 2: no statistics)
    return mcamd_sparse24_launch(a, idx, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// block sparsity (conv_bsparse.hip; an addition beyond the reference)
// ---------------------------------------------------------------------------------------
extern "C" int32_t mcamd_conv_fwd_bsparse_ok(const mcamd_conv_geom* g) {
    if (!g || g->stem || g->x_wrap != 0 || g->x_f8 != 0 || (g->ksize != 1 && g->ksize != 3)) return 0;
    if (g->B <= 0 || g->H <= 0 || g->W <= 0 || g->cin <= 0 || g->cout <= 0) return 0;
    if (g->cin % 32 != 0 || g->cout % 8 != 0 || (long long)g->B * g->H * g->W >= (1ll << 31)) return 0;
    if (g->pad != 0 && g->pad != 1) return 0;
    if (g->x_ld % 8 != 0 || g->x_choff % 8 != 0 || g->x_choff + g->cin > g->x_ld) return 0;
    return 1;
}

extern "C" int mcamd_bsparse_elems(const mcamd_conv_geom* g, int64_t out[2]) {
    MCAMD_REQUIRE(g && out, "bsparse_elems: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_bsparse_ok(g), "bsparse_elems: geometry has no block-sparse form (mcamd_conv_fwd_bsparse_ok)");
    const int ct = cin_tap_of(g);
    const long long ntiles = (g->cout + 63) / 64, nchunks = (long long)ntaps_of(g) * ct / kblock_of(ct);
    out[0] = ntiles;             // counts
    out[1] = ntiles * nchunks;   // list entries
    return MCAMD_OK;
}

extern "C" int mcamd_bsparse_lists(const mcamd_conv_geom* g, const void* wp_fwd, int32_t* count, int32_t* list, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "bsparse_lists: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_bsparse_lists(&g_, wp_fwd, count, list, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_bsparse_ok(g), "bsparse_lists: geometry has no block-sparse form (mcamd_conv_fwd_bsparse_ok)");
    MCAMD_REQUIRE(wp_fwd && count && list, "bsparse_lists: null pointer");
    MCAMD_REQUIRE(((uintptr_t)wp_fwd & 15) == 0, "bsparse_lists: packed weights must be 16-byte aligned");
    return mcamd_bsparse_lists_launch(wp_fwd, g->cout, cin_tap_of(g), ntaps_of(g), count, list, (hipStream_t)stream);
}

extern "C" int mcamd_conv_fwd_bsparse(const mcamd_conv_geom* g, const void* x, const void* wp_fwd, const int32_t* count,
                                      const int32_t* list, const mcamd_conv_epilogue* epi, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_bsparse: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_bsparse(&g_, x, wp_fwd, count, list, &e_, s); });
    }
    if (check_geom(g, "conv_fwd_bsparse")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_fwd_bsparse_ok(g), "conv_fwd_bsparse: geometry has no block-sparse form (mcamd_conv_fwd_bsparse_ok)");
    MCAMD_REQUIRE(x && wp_fwd && count && list, "conv_fwd_bsparse: null input");
    MCAMD_REQUIRE(epi && epi->mode == MCAMD_EPI_PAD_F16, "conv_fwd_bsparse: epilogue mode 2 (MCAMD_EPI_PAD_F16) only");
    IgemmArgs a;
    fill_operand(a, g, x, wp_fwd, g->x_ld, g->x_choff, g->cout, cin_tap_of(g), 0);
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_bsparse", 0)) return MCAMD_EINVAL;   // (mode 2: no statistics)
    return mcamd_bsparse_launch(a, count, list, (hipStream_t)stream);
}

// mcamd_bsparse_choice()'s answer: what mcamd_conv_fwd_bsparse launches for this geometry (host logic only)
extern "C" int mcamd_conv_fwd_bsparse_info(const mcamd_conv_geom* g, int32_t out[7]) {
    MCAMD_REQUIRE(g && out, "conv_fwd_bsparse_info: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_bsparse_ok(g), "conv_fwd_bsparse_info: geometry has no block-sparse form (mcamd_conv_fwd_bsparse_ok)");
    const BsparseChoice c = mcamd_bsparse_choice((long long)g->B * g->H * g->W, g->cout, kblock_of(cin_tap_of(g)));
    out[0] = c.bm, out[1] = c.bn, out[2] = c.bk, out[3] = c.stages, out[4] = c.mtiles, out[5] = c.ntiles, out[6] = c.grid;
    return MCAMD_OK;
}

// ... and its training form (Darknet.sparse_train = "block"): the raw fp16 epilogue, for the forward GEMM and
// for the dgrad GEMM -- N = cin, K = k*k * cout_p over the dgrad packing [Cpad][kpos(t, n)], whose K order is the forward's
// [channel block][tap][kb] over cout_p, so a K chunk is one (cout block, flipped tap) pair there too.
extern "C" int32_t mcamd_conv_bsparse_train_ok(const mcamd_conv_geom* g, int32_t dgrad) {
    if (!dgrad) return mcamd_conv_fwd_bsparse_ok(g);   // (refuses stem, x_wrap and x_f8)
    if (!g || g->stem || g->x_wrap != 0 || g->x_f8 != 0 || (g->ksize != 1 && g->ksize != 3)) return 0;
    if (g->B <= 0 || g->H <= 0 || g->W <= 0 || g->cin <= 0 || g->cout <= 0) return 0;
    if (g->cin % 8 != 0 || (long long)g->B * g->H * g->W >= (1ll << 31)) return 0;
    if (g->pad != 0 && g->pad != 1) return 0;
    return 1;   // (the slice of dy inside dy_ld: checked by the launch, which is given them)
}

// the launch's own choice for either direction
static BsparseChoice bsparse_train_choice(const mcamd_conv_geom* g, int dgrad) {
    const long long M = (long long)g->B * g->H * g->W;
    return dgrad ? mcamd_bsparse_choice(M, g->cin, kblock_of(cout_p_of(g))) : mcamd_bsparse_choice(M, g->cout, kblock_of(cin_tap_of(g)));
}

extern "C" int mcamd_conv_bsparse_train_info(const mcamd_conv_geom* g, int32_t dgrad, int32_t out[7]) {
    MCAMD_REQUIRE(g && out, "conv_bsparse_train_info: null argument");
    MCAMD_REQUIRE(mcamd_conv_bsparse_train_ok(g, dgrad), "conv_bsparse_train_info: geometry has no block-sparse training form (mcamd_conv_bsparse_train_ok)");
    const BsparseChoice c = bsparse_train_choice(g, dgrad);
    out[0] = c.bm, out[1] = c.bn, out[2] = c.bk, out[3] = c.stages, out[4] = c.mtiles, out[5] = c.ntiles, out[6] = c.grid;
    return MCAMD_OK;
}

extern "C" int32_t mcamd_conv_bsparse_raw_stats_rows(const mcamd_conv_geom* g, int32_t dgrad) {
    if (!g || !mcamd_conv_bsparse_train_ok(g, dgrad)) return 0;
    return bsparse_train_choice(g, dgrad).mtiles;   // one row per pixel tile: the grid is not persistent
}

extern "C" int mcamd_bsparse_elems_dgrad(const mcamd_conv_geom* g, int64_t out[2]) {
    MCAMD_REQUIRE(g && out, "bsparse_elems_dgrad: null argument");
    MCAMD_REQUIRE(mcamd_conv_bsparse_train_ok(g, 1), "bsparse_elems_dgrad: geometry has no block-sparse dgrad (mcamd_conv_bsparse_train_ok)");
    const int cp = cout_p_of(g);
    const long long ntiles = (g->cin + 63) / 64, nchunks = (long long)g->ksize * g->ksize * cp / kblock_of(cp);
    out[0] = ntiles;             // counts
    out[1] = ntiles * nchunks;   // list entries
    return MCAMD_OK;
}

extern "C" int mcamd_bsparse_lists_dgrad(const mcamd_conv_geom* g, const void* wp_dgrad, int32_t* count, int32_t* list, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "bsparse_lists_dgrad: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_bsparse_lists_dgrad(&g_, wp_dgrad, count, list, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_bsparse_train_ok(g, 1), "bsparse_lists_dgrad: geometry has no block-sparse dgrad (mcamd_conv_bsparse_train_ok)");
    MCAMD_REQUIRE(wp_dgrad && count && list, "bsparse_lists_dgrad: null pointer");
    MCAMD_REQUIRE(((uintptr_t)wp_dgrad & 15) == 0, "bsparse_lists_dgrad: packed weights must be 16-byte aligned");
    return mcamd_bsparse_lists_launch(wp_dgrad, g->cin, cout_p_of(g), g->ksize * g->ksize, count, list, (hipStream_t)stream);
}

extern "C" int mcamd_conv_fwd_bsparse_raw(const mcamd_conv_geom* g, const void* x, const void* wp_fwd, const int32_t* count,
                                          const int32_t* list, const mcamd_conv_epilogue* epi, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_bsparse_raw: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_bsparse_raw(&g_, x, wp_fwd, count, list, &e_, s); });
    }
    if (check_geom(g, "conv_fwd_bsparse_raw")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_bsparse_train_ok(g, 0), "conv_fwd_bsparse_raw: geometry has no block-sparse training form (mcamd_conv_bsparse_train_ok)");
    MCAMD_REQUIRE(x && wp_fwd && count && list, "conv_fwd_bsparse_raw: null input");
    MCAMD_REQUIRE(epi && epi->mode == MCAMD_EPI_RAW_F16, "conv_fwd_bsparse_raw: epilogue mode 0 (MCAMD_EPI_RAW_F16) only");
    IgemmArgs a;
    fill_operand(a, g, x, wp_fwd, g->x_ld, g->x_choff, g->cout, cin_tap_of(g), 0);
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_bsparse_raw", bsparse_train_choice(g, 0).mtiles)) return MCAMD_EINVAL;
    return mcamd_bsparse_launch(a, count, list, (hipStream_t)stream);
}

extern "C" int mcamd_conv_dgrad_bsparse(const mcamd_conv_geom* g, const void* dy, int32_t dy_ld, int32_t dy_choff, const void* wp_dgrad,
                                        const int32_t* count, const int32_t* list, const mcamd_conv_epilogue* epi, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_dgrad_bsparse: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_dgrad_bsparse(&g_, dy, dy_ld, dy_choff, wp_dgrad, count, list, &e_, s); });
    }
    if (check_geom(g, "conv_dgrad_bsparse")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_bsparse_train_ok(g, 1), "conv_dgrad_bsparse: geometry has no block-sparse dgrad (mcamd_conv_bsparse_train_ok)");
    MCAMD_REQUIRE(dy && wp_dgrad && count && list, "conv_dgrad_bsparse: null input");
    const int cout_p = cout_p_of(g);
    MCAMD_REQUIRE(dy_ld % 8 == 0 && dy_choff % 8 == 0 && dy_choff >= 0 && dy_choff + cout_p <= dy_ld,
                  "conv_dgrad_bsparse: dy slice [%d, %d) does not fit dy_ld %d", dy_choff, dy_choff + cout_p, dy_ld);
    MCAMD_REQUIRE(epi && epi->mode == MCAMD_EPI_RAW_F16 && !epi->stats && epi->dst_mode == 0 && !epi->y2,
                  "conv_dgrad_bsparse: epilogue mode 0 (MCAMD_EPI_RAW_F16) without statistics only");
    IgemmArgs a;
    fill_operand(a, g, dy, wp_dgrad, dy_ld, dy_choff, g->cin, cout_p, 0);   // (the set-up of mcamd_conv_dgrad; one tile shape:
    if (fill_epilogue(a, epi, g->cin, "conv_dgrad_bsparse", 0)) return MCAMD_EINVAL;   //  epilogue.concurrent changes nothing)
    return mcamd_bsparse_launch(a, count, list, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// split-K forward for low-batch inference (conv_splitk.hip; an addition beyond the reference)
// ---------------------------------------------------------------------------------------
// what both entries refuse, then the plan for `slices` (0 = the policy)
static int splitk_plan_for(const mcamd_conv_geom* g, int mode, int dst_mode, int slices, const char* what, SplitkPlan* p) {
    MCAMD_REQUIRE(g, "%s: null geometry", what);
    MCAMD_REQUIRE(g->stem == 0, "%s: stem %d: the first layer has no split-K form", what, g->stem);
    MCAMD_REQUIRE(g->pad == 0, "%s: pad %d: the shared-halo form is not accepted (pad must be 0)", what, g->pad);
    MCAMD_REQUIRE(g->x_wrap == 0, "%s: x_wrap %d: split operands have no split-K form", what, g->x_wrap);
    MCAMD_REQUIRE(g->x_f8 == 0, "%s: x_f8 %d: the fp8 correction form has no split-K form", what, g->x_f8);
    if (check_geom(g, what)) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mode == MCAMD_EPI_PAD_F16 || mode == MCAMD_EPI_RAW_F16,
                  "%s: epilogue mode %d: modes 2 (MCAMD_EPI_PAD_F16) and 0 (MCAMD_EPI_RAW_F16) only", what, mode);
    MCAMD_REQUIRE(dst_mode == MCAMD_DST_PLAIN || (mode == MCAMD_EPI_PAD_F16 && (dst_mode == MCAMD_DST_POOL || dst_mode == MCAMD_DST_REORG)),
                  "%s: bad dst_mode %d for epilogue mode %d", what, dst_mode, mode);
    MCAMD_REQUIRE(slices >= 0, "%s: slices %d is negative", what, slices);
    const int ct = cin_tap_of(g);
    *p = mcamd_splitk_plan((long long)g->B * g->H * g->W, g->cout, ct, ntaps_of(g) * ct, slices);
    MCAMD_REQUIRE(p->slices >= 1 && p->slices <= p->chunks, "%s: slices %d outside [1, chunks = %d]", what, p->slices, p->chunks);
    return MCAMD_OK;
}

static void splitk_info_of(const SplitkPlan& p, mcamd_splitk_info* out) {
    out->slices = p.slices;
    out->bm = p.bm, out->bn = p.bn, out->bk = p.bk;
    out->chunks = p.chunks;
    out->tiles = p.tiles;
    out->workspace_bytes = (int64_t)p.slices * p.slab_elems * (int64_t)sizeof(float);
    out->stages = p.stages;
    out->mtiles = p.mtiles, out->ntiles = p.ntiles;
    out->finish_rows = p.fr, out->finish_cols = p.fc;
}

extern "C" int mcamd_conv_fwd_splitk_info(const mcamd_conv_geom* g, int32_t mode, int32_t dst_mode, int32_t slices,
                                          mcamd_splitk_info* out) {
    MCAMD_REQUIRE(out, "conv_fwd_splitk_info: null output");
    SplitkPlan p;
    if (splitk_plan_for(g, mode, dst_mode, slices, "conv_fwd_splitk_info", &p)) return MCAMD_EINVAL;
    splitk_info_of(p, out);
    return MCAMD_OK;
}

extern "C" int mcamd_conv_fwd_splitk(const mcamd_conv_geom* g, const void* x, const void* wp_fwd, const mcamd_conv_epilogue* epi,
                                     int32_t slices, void* workspace, size_t workspace_bytes, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_splitk: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_splitk(&g_, x, wp_fwd, &e_, slices, workspace, workspace_bytes, s); });
    }
    MCAMD_REQUIRE(g, "conv_fwd_splitk: null geometry");
    MCAMD_REQUIRE(epi, "conv_fwd_splitk: null epilogue");
    SplitkPlan p;
    if (splitk_plan_for(g, epi->mode, epi->dst_mode, slices, "conv_fwd_splitk", &p)) return MCAMD_EINVAL;
    MCAMD_REQUIRE(epi->stats == nullptr, "conv_fwd_splitk: stats must be NULL (no statistics slab in the split-K form)");
    MCAMD_REQUIRE(x && wp_fwd, "conv_fwd_splitk: null input");
    const size_t need = (size_t)p.slices * (size_t)p.slab_elems * sizeof(float);
    MCAMD_REQUIRE(workspace, "conv_fwd_splitk: null workspace (%zu bytes needed)", need);
    MCAMD_REQUIRE(workspace_bytes >= need, "conv_fwd_splitk: workspace_bytes %zu is short of the %zu bytes %d slices need",
                  workspace_bytes, need, p.slices);
    MCAMD_REQUIRE(((uintptr_t)workspace & 15) == 0, "conv_fwd_splitk: workspace must be 16-byte aligned");
    IgemmArgs a;
    fill_operand(a, g, x, wp_fwd, g->x_ld, g->x_choff, g->cout, cin_tap_of(g), 0);
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_splitk", 0)) return MCAMD_EINVAL;
    return mcamd_splitk_launch(a, p, (float*)workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// fp8 (e4m3) quantised inference (conv_q8.hip; an addition beyond the reference)
// ---------------------------------------------------------------------------------------
extern "C" int32_t mcamd_conv_fwd_q8_ok(const mcamd_conv_geom* g) {
    if (!g || g->stem || g->x_wrap != 0 || g->x_f8 != 0 || (g->ksize != 1 && g->ksize != 3)) return 0;
    if (g->B <= 0 || g->H <= 0 || g->W <= 0 || g->cin <= 0 || g->cout <= 0) return 0;
    if (g->cin % 64 != 0 || g->cout % 8 != 0 || (long long)g->B * g->H * g->W >= (1ll << 31)) return 0;
    if (g->pad != 0 && g->pad != 1) return 0;
    if (g->x_ld % 16 != 0 || g->x_choff % 16 != 0 || g->x_choff < 0 || g->x_choff + g->cin > g->x_ld) return 0;
    return 1;
}

extern "C" int mcamd_q8_elems(const mcamd_conv_geom* g, int64_t out[2]) {
    MCAMD_REQUIRE(g && out, "q8_elems: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_ok(g), "q8_elems: geometry has no fp8 form (mcamd_conv_fwd_q8_ok)");
    const long long npad = round_up_int(g->cout, 256);
    out[0] = npad * ntaps_of(g) * g->cin;
    out[1] = npad;
    return MCAMD_OK;
}

extern "C" int mcamd_pack_q8(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* wq, int32_t* wexp,
                             void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "pack_q8: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_pack_q8(&g_, w_oihw, mask_oihw, wq, wexp, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_q8_ok(g), "pack_q8: geometry has no fp8 form (mcamd_conv_fwd_q8_ok)");
    MCAMD_REQUIRE(w_oihw && wq && wexp, "pack_q8: null pointer");
    return mcamd_pack_q8_launch(w_oihw, mask_oihw, wq, wexp, g->cout, g->cin, ntaps_of(g), (hipStream_t)stream);
}

extern "C" int mcamd_conv_fwd_q8(const mcamd_conv_geom* g, const void* x8, const void* wq, const int32_t* wexp,
                                 const mcamd_conv_epilogue* epi, int32_t y_f8, int32_t y2_f8, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_q8: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_q8(&g_, x8, wq, wexp, &e_, y_f8, y2_f8, s); });
    }
    if (check_geom(g, "conv_fwd_q8")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_ok(g), "conv_fwd_q8: geometry has no fp8 form (mcamd_conv_fwd_q8_ok)");
    MCAMD_REQUIRE(x8 && wq && wexp, "conv_fwd_q8: null input");
    MCAMD_REQUIRE(epi && (epi->mode == MCAMD_EPI_PAD_F16 || epi->mode == MCAMD_EPI_RAW_F32),
                  "conv_fwd_q8: epilogue modes 2 (MCAMD_EPI_PAD_F16) and 3 (MCAMD_EPI_RAW_F32) only");
    IgemmArgs a;
    fill_operand(a, g, x8, wq, g->x_ld, g->x_choff, g->cout, g->cin, 0);   // (strides in elements = bytes)
    // (mode 2: no statistics; mode 3, the training form: one slab row per pixel tile)
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_q8", epi->mode == MCAMD_EPI_RAW_F32 ? mcamd_conv_fwd_q8_stats_rows(g) : 0))
        return MCAMD_EINVAL;
    return mcamd_conv_q8_launch(a, wexp, y_f8 != 0, y2_f8 != 0, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// block-sparse fp8 forward (conv_q8_bsparse.hip; Darknet.precision = "fp8-block")
// ---------------------------------------------------------------------------------------
extern "C" int32_t mcamd_conv_fwd_q8_bsparse_ok(const mcamd_conv_geom* g) {
    return mcamd_conv_fwd_q8_ok(g) && g->cin % 64 == 0 && g->pad == 0;
}

extern "C" int mcamd_q8_bsparse_elems(const mcamd_conv_geom* g, int64_t out[2]) {
    MCAMD_REQUIRE(g && out, "q8_bsparse_elems: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_bsparse_ok(g), "q8_bsparse_elems: geometry has no block-sparse fp8 form (mcamd_conv_fwd_q8_bsparse_ok)");
    const long long ntiles = (g->cout + 63) / 64, nchunks = (long long)ntaps_of(g) * g->cin / 64;
    out[0] = ntiles;             // counts
    out[1] = ntiles * nchunks;   // list entries
    return MCAMD_OK;
}

extern "C" int mcamd_q8_bsparse_lists(const mcamd_conv_geom* g, const void* wq, int32_t* count, int32_t* list, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "q8_bsparse_lists: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_q8_bsparse_lists(&g_, wq, count, list, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_q8_bsparse_ok(g), "q8_bsparse_lists: geometry has no block-sparse fp8 form (mcamd_conv_fwd_q8_bsparse_ok)");
    MCAMD_REQUIRE(wq && count && list, "q8_bsparse_lists: null pointer");
    MCAMD_REQUIRE(((uintptr_t)wq & 15) == 0, "q8_bsparse_lists: packed weights must be 16-byte aligned");
    return mcamd_q8_bsparse_lists_launch(wq, g->cout, g->cin, ntaps_of(g), count, list, (hipStream_t)stream);
}

extern "C" int mcamd_conv_fwd_q8_bsparse(const mcamd_conv_geom* g, const void* x8, const void* wq, const int32_t* wexp,
                                         const int32_t* count, const int32_t* list, const mcamd_conv_epilogue* epi, int32_t y_f8,
                                         int32_t y2_f8, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_q8_bsparse: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_q8_bsparse(&g_, x8, wq, wexp, count, list, &e_, y_f8, y2_f8, s); });
    }
    if (check_geom(g, "conv_fwd_q8_bsparse")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_bsparse_ok(g), "conv_fwd_q8_bsparse: geometry has no block-sparse fp8 form (mcamd_conv_fwd_q8_bsparse_ok)");
    MCAMD_REQUIRE(x8 && wq && wexp && count && list, "conv_fwd_q8_bsparse: null input");
    MCAMD_REQUIRE(epi && epi->mode == MCAMD_EPI_PAD_F16, "conv_fwd_q8_bsparse: epilogue mode 2 (MCAMD_EPI_PAD_F16) only");
    IgemmArgs a;
    fill_operand(a, g, x8, wq, g->x_ld, g->x_choff, g->cout, g->cin, 0);   // (strides in elements = bytes)
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_q8_bsparse", 0)) return MCAMD_EINVAL;   // (mode 2: no statistics)
    return mcamd_conv_q8_bsparse_launch(a, wexp, count, list, y_f8 != 0, y2_f8 != 0, (hipStream_t)stream);
}

// mcamd_q8_bsparse_choice()'s answer: what mcamd_conv_fwd_q8_bsparse launches for this geometry (host logic only)
extern "C" int mcamd_conv_fwd_q8_bsparse_info(const mcamd_conv_geom* g, int32_t out[7]) {
    MCAMD_REQUIRE(g && out, "conv_fwd_q8_bsparse_info: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_bsparse_ok(g), "conv_fwd_q8_bsparse_info: geometry has no block-sparse fp8 form (mcamd_conv_fwd_q8_bsparse_ok)");
    const Q8Choice c = mcamd_q8_bsparse_choice((long long)g->B * g->H * g->W, g->cout);
    out[0] = c.bmw, out[1] = c.bnp, out[2] = c.f8mfma, out[3] = c.stages, out[4] = c.mtiles, out[5] = c.ntiles, out[6] = c.grid;
    return MCAMD_OK;
}

// ---------------------------------------------------------------------------------------
// split-K fp8 forward for low-batch inference (conv_q8_splitk.hip; Darknet.precision = "fp8-splitk")
// ---------------------------------------------------------------------------------------
// what both entries refuse, then the plan for `slices` (0 = the policy: mcamd_splitk_plan, the fp16 pair's, on 64-byte chunks)
static int q8_splitk_plan_for(const mcamd_conv_geom* g, int dst_mode, int slices, const char* what, SplitkPlan* p) {
    MCAMD_REQUIRE(g, "%s: null geometry", what);
    MCAMD_REQUIRE(g->stem == 0, "%s: stem %d: the first layer has no fp8 split-K form", what, g->stem);
    MCAMD_REQUIRE(g->pad == 0, "%s: pad %d: the shared-halo form is not accepted (pad must be 0)", what, g->pad);
    MCAMD_REQUIRE(g->cin > 0 && g->cin % 64 == 0, "%s: cin %d: the byte K loop needs cin %% 64 == 0", what, g->cin);
    if (check_geom(g, what)) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_ok(g), "%s: geometry has no fp8 form (mcamd_conv_fwd_q8_ok)", what);
    MCAMD_REQUIRE(dst_mode == MCAMD_DST_PLAIN || dst_mode == MCAMD_DST_POOL || dst_mode == MCAMD_DST_REORG, "%s: bad dst_mode %d", what,
                  dst_mode);
    MCAMD_REQUIRE(slices >= 0, "%s: slices %d is negative", what, slices);
    *p = mcamd_splitk_plan((long long)g->B * g->H * g->W, g->cout, g->cin, ntaps_of(g) * g->cin, slices);
    MCAMD_REQUIRE(p->slices >= 1 && p->slices <= p->chunks, "%s: slices %d outside [1, chunks = %d]", what, p->slices, p->chunks);
    return MCAMD_OK;
}

extern "C" int mcamd_conv_fwd_q8_splitk_info(const mcamd_conv_geom* g, int32_t dst_mode, int32_t slices, mcamd_splitk_info* out) {
    MCAMD_REQUIRE(out, "conv_fwd_q8_splitk_info: null output");
    SplitkPlan p;
    if (q8_splitk_plan_for(g, dst_mode, slices, "conv_fwd_q8_splitk_info", &p)) return MCAMD_EINVAL;
    splitk_info_of(p, out);
    return MCAMD_OK;
}

extern "C" int mcamd_conv_fwd_q8_splitk(const mcamd_conv_geom* g, const void* x8, const void* wq, const int32_t* wexp,
                                        const mcamd_conv_epilogue* epi, int32_t y_f8, int32_t y2_f8, int32_t slices, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_q8_splitk: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) {
            return mcamd_conv_fwd_q8_splitk(&g_, x8, wq, wexp, &e_, y_f8, y2_f8, slices, workspace, workspace_bytes, s);
        });
    }
    MCAMD_REQUIRE(g, "conv_fwd_q8_splitk: null geometry");
    MCAMD_REQUIRE(epi, "conv_fwd_q8_splitk: null epilogue");
    MCAMD_REQUIRE(epi->mode == MCAMD_EPI_PAD_F16, "conv_fwd_q8_splitk: epilogue mode %d: mode 2 (MCAMD_EPI_PAD_F16) only", epi->mode);
    SplitkPlan p;
    if (q8_splitk_plan_for(g, epi->dst_mode, slices, "conv_fwd_q8_splitk", &p)) return MCAMD_EINVAL;
    MCAMD_REQUIRE(epi->stats == nullptr, "conv_fwd_q8_splitk: stats must be NULL (no statistics slab in the split-K form)");
    MCAMD_REQUIRE(x8 && wq && wexp, "conv_fwd_q8_splitk: null input");
    const size_t need = (size_t)p.slices * (size_t)p.slab_elems * sizeof(float);
    MCAMD_REQUIRE(workspace, "conv_fwd_q8_splitk: null workspace (%zu bytes needed)", need);
    MCAMD_REQUIRE(workspace_bytes >= need, "conv_fwd_q8_splitk: workspace_bytes %zu is short of the %zu bytes %d slices need",
                  workspace_bytes, need, p.slices);
    MCAMD_REQUIRE(((uintptr_t)workspace & 15) == 0, "conv_fwd_q8_splitk: workspace must be 16-byte aligned (%zu bytes needed)", need);
    IgemmArgs a;
    fill_operand(a, g, x8, wq, g->x_ld, g->x_choff, g->cout, g->cin, 0);   // (strides in elements = bytes)
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_q8_splitk", 0)) return MCAMD_EINVAL;
    return mcamd_q8_splitk_launch(a, p, wexp, y_f8 != 0, y2_f8 != 0, (float*)workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// fp8 inference of slim_export models: cin a multiple of 8 on zero-padded weight rows, border tables
// ---------------------------------------------------------------------------------------
extern "C" int32_t mcamd_conv_fwd_q8_slim_ok(const mcamd_conv_geom* g) {
    if (!g || g->stem || g->x_wrap != 0 || g->x_f8 != 0 || (g->ksize != 1 && g->ksize != 3)) return 0;
    if (g->B <= 0 || g->H <= 0 || g->W <= 0 || g->cin <= 0 || g->cout <= 0) return 0;
    if (g->cin % 8 != 0 || g->cout % 8 != 0 || (long long)g->B * g->H * g->W >= (1ll << 31)) return 0;
    if (g->pad != 0 && g->pad != 1) return 0;
    // the K loop reads round_up(cin, 64) channels of every pixel: they must lie inside the pixel's row
    if (g->x_ld % 16 != 0 || g->x_choff % 16 != 0 || g->x_choff < 0 || (long long)g->x_choff + round_up_int(g->cin, 64) > g->x_ld) return 0;
    return 1;
}

extern "C" int mcamd_q8_slim_elems(const mcamd_conv_geom* g, int64_t out[2]) {
    MCAMD_REQUIRE(g && out, "q8_slim_elems: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_slim_ok(g), "q8_slim_elems: geometry has no slim fp8 form (mcamd_conv_fwd_q8_slim_ok)");
    const long long npad = round_up_int(g->cout, 256);
    out[0] = npad * ntaps_of(g) * round_up_int(g->cin, 64);
    out[1] = npad;
    return MCAMD_OK;
}

extern "C" int mcamd_pack_q8_slim(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* wq, int32_t* wexp,
                                  void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "pack_q8_slim: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_pack_q8_slim(&g_, w_oihw, mask_oihw, wq, wexp, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_q8_slim_ok(g), "pack_q8_slim: geometry has no slim fp8 form (mcamd_conv_fwd_q8_slim_ok)");
    MCAMD_REQUIRE(w_oihw && wq && wexp, "pack_q8_slim: null pointer");
    return mcamd_pack_q8_slim_launch(w_oihw, mask_oihw, wq, wexp, g->cout, g->cin, ntaps_of(g), (hipStream_t)stream);
}

extern "C" int mcamd_conv_fwd_q8_slim(const mcamd_conv_geom* g, const void* x8, const void* wq, const int32_t* wexp,
                                      const mcamd_conv_epilogue* epi, const float* border, int32_t border_ld, int32_t y_f8,
                                      int32_t y2_f8, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_q8_slim: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_q8_slim(&g_, x8, wq, wexp, &e_, border, border_ld, y_f8, y2_f8, s); });
    }
    if (check_geom(g, "conv_fwd_q8_slim")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_slim_ok(g), "conv_fwd_q8_slim: geometry has no slim fp8 form (mcamd_conv_fwd_q8_slim_ok)");
    MCAMD_REQUIRE(x8 && wq && wexp, "conv_fwd_q8_slim: null input");
    MCAMD_REQUIRE(epi && epi->mode == MCAMD_EPI_PAD_F16, "conv_fwd_q8_slim: epilogue mode 2 (MCAMD_EPI_PAD_F16) only");
    MCAMD_REQUIRE(!border || (border_ld >= g->cout && border_ld % 4 == 0),
                  "conv_fwd_q8_slim: border_ld %d must be a multiple of 4 and >= cout %d", border_ld, g->cout);
    IgemmArgs a;
    // the unchanged K loop over round_up(cin, 64) channels per tap: the weight bytes of the extra ones are 0x00
    fill_operand(a, g, x8, wq, g->x_ld, g->x_choff, g->cout, round_up_int(g->cin, 64), 0);   // (strides in elements = bytes)
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_q8_slim", 0)) return MCAMD_EINVAL;           // (mode 2: no statistics)
    return mcamd_conv_q8_launch(a, wexp, y_f8 != 0, y2_f8 != 0, (hipStream_t)stream, border, border ? border_ld : 0);
}

extern "C" int32_t mcamd_conv_fwd_q8_stats_rows(const mcamd_conv_geom* g) {
    if (!mcamd_conv_fwd_q8_ok(g)) return 0;
    return (int32_t)(((long long)g->B * g->H * g->W + MCAMD_Q8_TILE_M - 1) / MCAMD_Q8_TILE_M);
}

extern "C" int mcamd_fakequant_q8(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, const int32_t* wexp,
                                  float* wq_oihw, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "fakequant_q8: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_fakequant_q8(&g_, w_oihw, mask_oihw, wexp, wq_oihw, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_q8_ok(g), "fakequant_q8: geometry has no fp8 form (mcamd_conv_fwd_q8_ok)");
    MCAMD_REQUIRE(w_oihw && wexp && wq_oihw, "fakequant_q8: null pointer");
    return mcamd_fakequant_q8_launch(w_oihw, mask_oihw, wexp, wq_oihw, g->cout, g->cin, ntaps_of(g), (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// 2:4-sparse fp8 quantised inference (conv_q8_sparse.hip; an addition beyond the reference)
// ---------------------------------------------------------------------------------------
extern "C" int32_t mcamd_conv_fwd_q8_sparse24_ok(const mcamd_conv_geom* g) {
    return mcamd_conv_fwd_q8_ok(g);                // (cin % 64 == 0: whole groups of 4)
}

extern "C" int mcamd_q8_sparse24_elems(const mcamd_conv_geom* g, int64_t out[3]) {
    MCAMD_REQUIRE(g && out, "q8_sparse24_elems: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_sparse24_ok(g), "q8_sparse24_elems: geometry has no 2:4 fp8 form (mcamd_conv_fwd_q8_sparse24_ok)");
    const long long npad = round_up_int(g->cout, 256), ktot = (long long)ntaps_of(g) * g->cin;
    out[0] = npad * ktot / 2;      // kept bytes
    out[1] = npad * ktot / 32;     // 32-bit index words
    out[2] = npad;                 // int32 exponents
    return MCAMD_OK;
}

extern "C" int mcamd_pack_q8_sparse24(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* wq, void* idx,
                                      int32_t* wexp, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "pack_q8_sparse24: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_pack_q8_sparse24(&g_, w_oihw, mask_oihw, wq, idx, wexp, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_q8_sparse24_ok(g), "pack_q8_sparse24: geometry has no 2:4 fp8 form (mcamd_conv_fwd_q8_sparse24_ok)");
    MCAMD_REQUIRE(w_oihw && wq && idx && wexp, "pack_q8_sparse24: null pointer");
    return mcamd_pack_q8_sparse24_launch(w_oihw, mask_oihw, wq, idx, wexp, g->cout, g->cin, ntaps_of(g), (hipStream_t)stream);
}

extern "C" int mcamd_conv_fwd_q8_sparse24(const mcamd_conv_geom* g, const void* x8, const void* wq, const void* idx,
                                          const int32_t* wexp, const mcamd_conv_epilogue* epi, int32_t y_f8, int32_t y2_f8,
                                          void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_q8_sparse24: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_q8_sparse24(&g_, x8, wq, idx, wexp, &e_, y_f8, y2_f8, s); });
    }
    if (check_geom(g, "conv_fwd_q8_sparse24")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_sparse24_ok(g), "conv_fwd_q8_sparse24: geometry has no 2:4 fp8 form (mcamd_conv_fwd_q8_sparse24_ok)");
    MCAMD_REQUIRE(x8 && wq && idx && wexp, "conv_fwd_q8_sparse24: null input");
    MCAMD_REQUIRE(epi && epi->mode == MCAMD_EPI_PAD_F16, "conv_fwd_q8_sparse24: epilogue mode 2 (MCAMD_EPI_PAD_F16) only");
    IgemmArgs a;
    fill_operand(a, g, x8, wq, g->x_ld, g->x_choff, g->cout, g->cin, 0);   // (strides in elements = bytes)
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_q8_sparse24", 0)) return MCAMD_EINVAL;   // (mode 2: no statistics)
    return mcamd_conv_q8_sparse_launch(a, idx, wexp, y_f8 != 0, y2_f8 != 0, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// 4-bit weight inference on the fp8 engine (conv_q8_w4.hip; Darknet.precision = "fp8-w4")
// ---------------------------------------------------------------------------------------
extern "C" int32_t mcamd_conv_fwd_q8_w4_ok(const mcamd_conv_geom* g) {
    return mcamd_conv_fwd_q8_ok(g);                // (cin % 64 == 0: two whole groups of 32 per chunk)
}

extern "C" int mcamd_q8_w4_elems(const mcamd_conv_geom* g, int64_t out[3]) {
    MCAMD_REQUIRE(g && out, "q8_w4_elems: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_w4_ok(g), "q8_w4_elems: geometry has no 4-bit fp8 form (mcamd_conv_fwd_q8_w4_ok)");
    const long long npad = round_up_int(g->cout, 256), ktot = (long long)ntaps_of(g) * g->cin;
    out[0] = npad * ktot / 2;      // code bytes
    out[1] = npad * ktot / 32;     // shift bytes
    out[2] = npad;                 // int32 exponents
    return MCAMD_OK;
}

extern "C" int mcamd_pack_q8_w4(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* codes, void* gshift,
                                int32_t* wexp, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "pack_q8_w4: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_pack_q8_w4(&g_, w_oihw, mask_oihw, codes, gshift, wexp, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_q8_w4_ok(g), "pack_q8_w4: geometry has no 4-bit fp8 form (mcamd_conv_fwd_q8_w4_ok)");
    MCAMD_REQUIRE(w_oihw && codes && gshift && wexp, "pack_q8_w4: null pointer");
    return mcamd_pack_q8_w4_launch(w_oihw, mask_oihw, codes, gshift, wexp, g->cout, g->cin, ntaps_of(g), (hipStream_t)stream);
}

extern "C" int mcamd_unpack_q8_w4(const mcamd_conv_geom* g, const void* codes, const void* gshift, void* wq, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "unpack_q8_w4: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_unpack_q8_w4(&g_, codes, gshift, wq, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_q8_w4_ok(g), "unpack_q8_w4: geometry has no 4-bit fp8 form (mcamd_conv_fwd_q8_w4_ok)");
    MCAMD_REQUIRE(codes && gshift && wq, "unpack_q8_w4: null pointer");
    return mcamd_unpack_q8_w4_launch(codes, gshift, wq, g->cout, g->cin, ntaps_of(g), (hipStream_t)stream);
}

extern "C" int mcamd_conv_fwd_q8_w4(const mcamd_conv_geom* g, const void* x8, const void* codes, const void* gshift,
                                    const int32_t* wexp, const mcamd_conv_epilogue* epi, int32_t y_f8, int32_t y2_f8,
                                    void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_q8_w4: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_q8_w4(&g_, x8, codes, gshift, wexp, &e_, y_f8, y2_f8, s); });
    }
    if (check_geom(g, "conv_fwd_q8_w4")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_w4_ok(g), "conv_fwd_q8_w4: geometry has no 4-bit fp8 form (mcamd_conv_fwd_q8_w4_ok)");
    MCAMD_REQUIRE(x8 && codes && gshift && wexp, "conv_fwd_q8_w4: null input");
    MCAMD_REQUIRE(epi && epi->mode == MCAMD_EPI_PAD_F16, "conv_fwd_q8_w4: epilogue mode 2 (MCAMD_EPI_PAD_F16) only");
    IgemmArgs a;
    fill_operand(a, g, x8, codes, g->x_ld, g->x_choff, g->cout, g->cin, 0);   // (strides in elements = bytes)
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_q8_w4", 0)) return MCAMD_EINVAL;   // (mode 2: no statistics)
    return mcamd_conv_q8_w4_launch(a, gshift, wexp, y_f8 != 0, y2_f8 != 0, (hipStream_t)stream);
}

// the training form (Darknet.precision = "fp8-w4-qat"): raw fp32 output + statistics, and the values the codes
// stand for
extern "C" int mcamd_conv_fwd_q8_w4_raw(const mcamd_conv_geom* g, const void* x8, const void* codes, const void* gshift,
                                        const int32_t* wexp, const mcamd_conv_epilogue* epi, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_fwd_q8_w4_raw: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_fwd_q8_w4_raw(&g_, x8, codes, gshift, wexp, &e_, s); });
    }
    if (check_geom(g, "conv_fwd_q8_w4_raw")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_w4_ok(g), "conv_fwd_q8_w4_raw: geometry has no 4-bit fp8 form (mcamd_conv_fwd_q8_w4_ok)");
    MCAMD_REQUIRE(x8 && codes && gshift && wexp, "conv_fwd_q8_w4_raw: null input");
    MCAMD_REQUIRE(epi && epi->mode == MCAMD_EPI_RAW_F32, "conv_fwd_q8_w4_raw: epilogue mode 3 (MCAMD_EPI_RAW_F32) only");
    IgemmArgs a;
    fill_operand(a, g, x8, codes, g->x_ld, g->x_choff, g->cout, g->cin, 0);   // (strides in elements = bytes)
    if (fill_epilogue(a, epi, g->cout, "conv_fwd_q8_w4_raw", mcamd_conv_fwd_q8_stats_rows(g))) return MCAMD_EINVAL;
    return mcamd_conv_q8_w4_raw_launch(a, gshift, wexp, (hipStream_t)stream);
}

extern "C" int mcamd_fakequant_q8_w4(const mcamd_conv_geom* g, const void* codes, const void* gshift, const int32_t* wexp,
                                     float* wq_oihw, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "fakequant_q8_w4: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_fakequant_q8_w4(&g_, codes, gshift, wexp, wq_oihw, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_fwd_q8_w4_ok(g), "fakequant_q8_w4: geometry has no 4-bit fp8 form (mcamd_conv_fwd_q8_w4_ok)");
    MCAMD_REQUIRE(codes && gshift && wexp && wq_oihw, "fakequant_q8_w4: null pointer");
    return mcamd_fakequant_q8_w4_launch(codes, gshift, wexp, wq_oihw, g->cout, g->cin, ntaps_of(g), (hipStream_t)stream);
}

// mcamd_q8_w4_choice()'s answer: what mcamd_conv_fwd_q8_w4 launches for this geometry (host logic only)
extern "C" int mcamd_conv_fwd_q8_w4_info(const mcamd_conv_geom* g, int32_t out[7]) {
    MCAMD_REQUIRE(g && out, "conv_fwd_q8_w4_info: null argument");
    MCAMD_REQUIRE(mcamd_conv_fwd_q8_w4_ok(g), "conv_fwd_q8_w4_info: geometry has no 4-bit fp8 form (mcamd_conv_fwd_q8_w4_ok)");
    const Q8Choice c = mcamd_q8_w4_choice((long long)g->B * g->H * g->W, g->cout);
    out[0] = c.bmw, out[1] = c.bnp, out[2] = c.f8mfma, out[3] = c.stages, out[4] = c.mtiles, out[5] = c.ntiles, out[6] = c.grid;
    return MCAMD_OK;
}

// mcamd_q8_choice()'s answer: what mcamd_conv_fwd_q8 (forms 0, 1), mcamd_conv_fwd_q8_slim (form 2) and
// mcamd_conv_fwd_q8_sparse24 (form 3) launch for this geometry (host logic only)
extern "C" int mcamd_conv_fwd_q8_info(const mcamd_conv_geom* g, int32_t form, int32_t out[7]) {
    MCAMD_REQUIRE(g && out, "conv_fwd_q8_info: null argument");
    MCAMD_REQUIRE(form >= MCAMD_Q8_FORM_INFER && form <= MCAMD_Q8_FORM_SPARSE, "conv_fwd_q8_info: form %d is none of 0 .. 3", form);
    MCAMD_REQUIRE(form == MCAMD_Q8_FORM_BORDER ? mcamd_conv_fwd_q8_slim_ok(g) : mcamd_conv_fwd_q8_ok(g),
                  "conv_fwd_q8_info: geometry has no fp8 form of this kind (mcamd_conv_fwd_q8_ok / mcamd_conv_fwd_q8_slim_ok)");
    const Q8Choice c = mcamd_q8_choice((long long)g->B * g->H * g->W, g->cout, form);
    out[0] = c.bmw, out[1] = c.bnp, out[2] = c.f8mfma, out[3] = c.stages, out[4] = c.mtiles, out[5] = c.ntiles, out[6] = c.grid;
    return MCAMD_OK;
}

static int cast_q8_any(const void* src, int64_t pixels, int32_t src_ld, int32_t src_choff, int32_t C, void* dst, int32_t dst_ld,
                       int32_t dst_choff, int back, void* stream) {
    MCAMD_REQUIRE(src && dst && pixels > 0 && C > 0, "cast_q8: null pointer / empty");
    MCAMD_REQUIRE(C % 8 == 0 && src_ld % 8 == 0 && src_choff % 8 == 0 && dst_ld % 8 == 0 && dst_choff % 8 == 0 &&
                      src_choff >= 0 && dst_choff >= 0 && src_choff + C <= src_ld && dst_choff + C <= dst_ld,
                  "cast_q8: channel slices must be multiples of 8 inside their leading dimensions");
    return mcamd_cast_q8_launch(src, pixels, src_ld, src_choff, C, dst, dst_ld, dst_choff, back, (hipStream_t)stream);
}

extern "C" int mcamd_cast_q8(const void* src, int64_t pixels, int32_t src_ld, int32_t src_choff, int32_t C, void* dst,
                             int32_t dst_ld, int32_t dst_choff, void* stream) {
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_cast_q8(src, pixels, src_ld, src_choff, C, dst, dst_ld, dst_choff, s); });
    return cast_q8_any(src, pixels, src_ld, src_choff, C, dst, dst_ld, dst_choff, 0, stream);
}

extern "C" int mcamd_cast_q8_train(void* src, int64_t pixels, int32_t src_ld, int32_t src_choff, int32_t C, void* dst,
                                   int32_t dst_ld, int32_t dst_choff, void* stream) {
    if (mcamd_recording())
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_cast_q8_train(src, pixels, src_ld, src_choff, C, dst, dst_ld, dst_choff, s); });
    return cast_q8_any(src, pixels, src_ld, src_choff, C, dst, dst_ld, dst_choff, 1, stream);
}

// dgrad: the route of a launch with epilogue mode `mode` (0 or 1)
static ConvRoute dgrad_route(const mcamd_conv_geom* g, bool concurrent, int mode) {
    return conv_route(g, concurrent ? DIR_DGRAD_CONCURRENT : DIR_DGRAD, mode, MCAMD_DST_PLAIN, false);
}

extern "C" int32_t mcamd_conv_dgrad_sums_rows(const mcamd_conv_geom* g, int32_t concurrent) {
    if (!g || g->stem) return 0;
    const ConvRoute r = dgrad_route(g, concurrent != 0, MCAMD_EPI_RAW_F16);
    return mcamd_igemm_sums_ok(r) ? r.rows : 0;
}

extern "C" int mcamd_conv_dgrad_sums(const mcamd_conv_geom* g, const void* dy, int32_t dy_ld, int32_t dy_choff,
                                     const void* wp_dgrad, const mcamd_conv_epilogue* epi, const mcamd_dgrad_sums* sums,
                                     void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g && epi, "conv_dgrad: null geometry / epilogue");
        const mcamd_conv_geom g_ = *g;
        const mcamd_conv_epilogue e_ = *epi;
        if (!sums) return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_dgrad_sums(&g_, dy, dy_ld, dy_choff, wp_dgrad, &e_, nullptr, s); });
        const mcamd_dgrad_sums s_ = *sums;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_conv_dgrad_sums(&g_, dy, dy_ld, dy_choff, wp_dgrad, &e_, &s_, s); });
    }
    if (check_geom(g, "conv_dgrad")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(g->x_wrap == 0 && g->x_f8 == 0, "conv_dgrad: x_wrap / x_f8 are forward-only fields");
    MCAMD_REQUIRE(!g->stem, "conv_dgrad: the stem layer has no input gradient");
    MCAMD_REQUIRE(dy && wp_dgrad, "conv_dgrad: null input");
    int cout_p = cout_p_of(g);
    MCAMD_REQUIRE(dy_ld % 8 == 0 && dy_choff % 8 == 0 && dy_choff + cout_p <= dy_ld,
                  "conv_dgrad: dy slice [%d, %d) does not fit dy_ld %d", dy_choff, dy_choff + cout_p, dy_ld);
    IgemmArgs a;
    fill_operand(a, g, dy, wp_dgrad, dy_ld, dy_choff, g->cin, cout_p, 0);
    MCAMD_REQUIRE(epi && epi->mode != MCAMD_EPI_PAD_F16 && !epi->stats && epi->dst_mode == 0 && !epi->y2,
                  "conv_dgrad: epilogue must be mode 0 (no stats) or 1");
    a.concurrent = epi->concurrent != 0;
    const ConvRoute r = dgrad_route(g, a.concurrent, epi->mode);
    if (fill_epilogue(a, epi, g->cin, "conv_dgrad", r.rows)) return MCAMD_EINVAL;
    if (sums && sums->slab) {
        const mcamd_dgrad_sums* s = sums;
        MCAMD_REQUIRE(epi->mode == MCAMD_EPI_RAW_F16, "conv_dgrad: producer sums go with epilogue mode 0");
        MCAMD_REQUIRE(mcamd_igemm_sums_ok(r) && s->rows == r.rows,
                      "conv_dgrad: sums.rows must be mcamd_conv_dgrad_sums_rows() = %d (got %d; 0: this launch cannot take sums)",
                      mcamd_igemm_sums_ok(r) ? r.rows : 0, s->rows);
        MCAMD_REQUIRE(s->act && s->scale && s->shift && s->mean && s->invstd, "conv_dgrad: sums: null argument");
        MCAMD_REQUIRE(s->C > 0 && s->C % 8 == 0 && s->ch_lo >= 0 && s->ch_lo % 8 == 0 && s->ch_lo + s->C <= g->cin,
                      "conv_dgrad: sums: producer columns [%d, %d) must be whole groups of 8 inside the %d channels of G",
                      s->ch_lo, s->ch_lo + s->C, g->cin);
        MCAMD_REQUIRE(s->ld >= s->C, "conv_dgrad: sums.ld (%d) must be >= C (%d)", s->ld, s->C);
        MCAMD_REQUIRE(s->act_ld % 8 == 0 && s->act_choff % 8 == 0 && s->act_choff >= 0 && s->act_choff + s->C <= s->act_ld &&
                          (s->act_pad == 0 || s->act_pad == 1),
                      "conv_dgrad: sums: activation slice [%d, %d) does not fit act_ld %d", s->act_choff, s->act_choff + s->C, s->act_ld);
        MCAMD_REQUIRE(!s->y || (s->y_ld % 4 == 0 && s->y_choff % 4 == 0 && s->y_choff >= 0 && s->y_choff + s->C <= s->y_ld),
                      "conv_dgrad: sums: fp32 y slice [%d, %d) does not fit y_ld %d", s->y_choff, s->y_choff + s->C, s->y_ld);
        MCAMD_REQUIRE(s->slope > 0.f, "conv_dgrad: sums need an invertible activation (slope > 0)");
        a.bsum.slab = s->slab, a.bsum.ld = s->ld;
        a.bsum.act = (const half_t*)s->act, a.bsum.act_ld = s->act_ld, a.bsum.act_choff = s->act_choff, a.bsum.act_pw = s->act_pad ? 1 : 2;
        a.bsum.scale = s->scale, a.bsum.shift = s->shift, a.bsum.mean = s->mean, a.bsum.invstd = s->invstd;
        a.bsum.y = s->y, a.bsum.y_ld = s->y_ld, a.bsum.y_choff = s->y_choff;
        a.bsum.ch_lo = s->ch_lo, a.bsum.C = s->C;
        a.bsum.slope = s->slope;
    }
    return launch_route(a, r, g, (hipStream_t)stream);
}

extern "C" int mcamd_conv_dgrad(const mcamd_conv_geom* g, const void* dy, int32_t dy_ld, int32_t dy_choff,
                                const void* wp_dgrad, const mcamd_conv_epilogue* epi, void* stream) {
    return mcamd_conv_dgrad_sums(g, dy, dy_ld, dy_choff, wp_dgrad, epi, nullptr, stream);
}

// ---------------------------------------------------------------------------------------
// wgrad
// ---------------------------------------------------------------------------------------
static WgradPlan wgrad_plan_for(const mcamd_conv_geom* g) {
    if (mcamd_wgrad_stem_ok(g->stem, g->cout, g->W, (long long)g->B * g->H * g->W))
        return mcamd_wgrad_stem_plan((long long)g->B * g->H * g->W);
    if (mcamd_wgrad_win_ok(g->ksize, g->stem, g->cout, cin_tap_of(g), g->W, (long long)g->B * g->H * g->W))
        return mcamd_wgrad_win_plan((long long)g->B * g->H * g->W, g->cout);
    if (mcamd_wgrad_use9(g->ksize, g->stem, g->cout, cin_tap_of(g), g->W))
        return mcamd_wgrad_plan9(padded_pixels(g), g->cout, cin_tap_of(g), g->W, g->W + pw_of(g), g->B);
    return mcamd_wgrad_plan((long long)g->B * g->H * g->W, g->cout, cin_tap_of(g), ntaps_of(g));
}

extern "C" size_t mcamd_conv_wgrad_workspace_bytes(const mcamd_conv_geom* g) {
    if (!g) return 0;
    return wgrad_plan_for(g).bytes;
}

// out: see include/mcamd.h.  The plan, the ring depth and the finish kernel come from the functions the launch calls.
extern "C" int mcamd_conv_wgrad_plan_info(const mcamd_conv_geom* g, int32_t has_cmap, int32_t out[MCAMD_WGRAD_PLAN_INFO_N]) {
    if (check_geom(g, "conv_wgrad_plan_info")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(out, "conv_wgrad_plan_info: null output");
    MCAMD_REQUIRE(!(g->stem && has_cmap), "conv_wgrad_plan_info: the stem layer takes no input-channel map");
    const WgradPlan p = wgrad_plan_for(g);
    const WgradFinish f = mcamd_wgrad_finish_pick(p.nsplit, g->stem, g->cin, g->ksize, has_cmap != 0);
    const int tiles = p.n_otiles * p.n_tapgroups * p.n_ctiles;
    out[0] = p.nine == 2 ? MCAMD_WGRAD_NINE_WIDE : p.nine ? MCAMD_WGRAD_NINE : p.stemw == 1 ? MCAMD_WGRAD_STEM
             : p.stemw == 2 ? MCAMD_WGRAD_WIN : MCAMD_WGRAD_GENERIC;
    out[1] = p.tmo, out[2] = p.tnc, out[3] = p.taps, out[4] = p.kp, out[5] = p.ns;
    out[6] = p.nsplit, out[7] = p.pix_per_split, out[8] = p.rows_pad;
    out[9] = f.kernel, out[10] = f.sg;
    out[11] = tiles;
    out[12] = p.stemw ? p.nsplit : round_up_int(tiles * p.nsplit, 8);
    return MCAMD_OK;
}

extern "C" int32_t mcamd_wgrad_generic_instances(int32_t* out, int32_t cap) {
    static_assert(sizeof(int32_t) == sizeof(int), "instance tuples are copied as int");
    return mcamd_wgrad_instances((int (*)[4])out, out ? cap : 0);
}

// the operands of a weight-gradient launch as the compute kernels address them (mcamd_conv_wgrad and its list form)
static WgradArgs wgrad_args_of(const mcamd_conv_geom* g, const void* x, const void* dy, int dy_ld, int dy_choff, void* workspace) {
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.x = (const half_t*)x;
    a.dy = (const half_t*)dy;
    a.slab = (float*)workspace;
    a.x_ld = g->x_ld;
    a.x_row_stride = (g->W + pw_of(g)) * g->x_ld;
    a.x_img_stride = (long long)(g->H + pw_of(g)) * a.x_row_stride;
    a.x_off = g->x_choff;
    a.dy_ld = dy_ld;
    a.dy_row_stride = (g->W + pw_of(g)) * dy_ld;
    a.dy_img_stride = (long long)(g->H + pw_of(g)) * a.dy_row_stride;
    a.dy_off = dy_choff + a.dy_row_stride + dy_ld;
    a.dy_zero_off = dy_choff;
    a.H = g->H, a.W = g->W, a.HW = g->H * g->W;
    a.M = (int)((long long)g->B * g->H * g->W);
    a.cin_tap = cin_tap_of(g);
    a.ntaps = ntaps_of(g);
    a.ktot = a.ntaps * a.cin_tap;
    fill_taps(g->ksize, g->stem, a.x_row_stride, g->x_ld, a.tap_off);
    return a;
}

extern "C" int mcamd_conv_wgrad(const mcamd_conv_geom* g, const void* x, const void* dy, int32_t dy_ld, int32_t dy_choff,
                                const float* mask_oihw, const mcamd_chan_map* map, float grad_scale, float* dw_oihw,
                                float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "conv_wgrad: null geometry");
        const mcamd_conv_geom g_ = *g;
        const bool has_map = map != nullptr;
        const mcamd_chan_map m_ = has_map ? *map : mcamd_chan_map{nullptr, nullptr};
        return mcamd_rec_push(stream, [=](void* s) {
            return mcamd_conv_wgrad(&g_, x, dy, dy_ld, dy_choff, mask_oihw, has_map ? &m_ : nullptr, grad_scale, dw_oihw, dbias,
                                    workspace, workspace_bytes, s);
        });
    }
    if (check_geom(g, "conv_wgrad")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(g->x_wrap == 0 && g->x_f8 == 0, "conv_wgrad: x_wrap / x_f8 are forward-only fields");
    MCAMD_REQUIRE(x && dy && dw_oihw && workspace, "conv_wgrad: null argument");
    MCAMD_REQUIRE(grad_scale > 0.f, "conv_wgrad: grad_scale must be positive");
    const int* rmap = map ? (const int*)map->rows : nullptr;
    const int* cmap = map ? (const int*)map->cols : nullptr;
    MCAMD_REQUIRE(!(g->stem && cmap), "conv_wgrad: the stem layer takes no input-channel map");
    const int cin_tap = cin_tap_of(g), ntaps = ntaps_of(g);
    const long long M = (long long)g->B * g->H * g->W;
    WgradPlan p = wgrad_plan_for(g);
    MCAMD_REQUIRE(dy_ld % 8 == 0 && dy_choff % 8 == 0 && dy_choff + p.rows_pad <= dy_ld,
                  "conv_wgrad: dy slice [%d, %d) does not fit dy_ld %d", dy_choff, dy_choff + p.rows_pad, dy_ld);
    if (workspace_bytes < p.bytes) {
        mcamd_set_error("conv_wgrad: workspace %zu < %zu bytes", workspace_bytes, p.bytes);
        return MCAMD_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    WgradArgs a = wgrad_args_of(g, x, dy, dy_ld, dy_choff, workspace);
    int rc = p.nine    ? mcamd_wgrad9_launch(a, p, g->W + pw_of(g), padded_pixels(g), st)
             : p.stemw == 1 ? mcamd_wgrad_stem_launch(a, p, st)
             : p.stemw == 2 ? mcamd_wgrad_win_launch(a, p, st)
                       : mcamd_wgrad_launch(a, p, st);
    if (rc) return rc;
    rc = mcamd_wgrad_finish_launch((const float*)workspace, p, a.ktot, cin_tap, g->stem, g->cout, g->cin, g->ksize,
                                   mask_oihw, 1.0f / grad_scale, dw_oihw, rmap, cmap, st);
    if (rc) return rc;
    if (dbias) {
        long long rows = padded_pixels(g);
        // (the split-K slabs are consumed by the finish pass enqueued above: the workspace is free again, in stream order)
        rc = mcamd_colsum_launch((const half_t*)dy, rows, dy_ld, dy_choff, g->cout, 1.0f / grad_scale, dbias, st, workspace,
                                 workspace_bytes);
    }
    return rc;
}

// ---------------------------------------------------------------------------------------
// the list launch of the weight gradient (conv_wgrad.hip; Darknet.sparse_train = "block-wgrad")
// ---------------------------------------------------------------------------------------
extern "C" int32_t mcamd_conv_wgrad_bsparse_ok(const mcamd_conv_geom* g) {
    if (!g || g->B <= 0 || g->H <= 0 || g->W <= 0 || g->cin <= 0 || g->cout <= 0) return 0;
    if (g->x_wrap || g->x_f8 || (g->pad != 0 && g->pad != 1)) return 0;
    if (g->x_choff < 0 || g->x_choff % 8 || g->x_choff + g->cin > g->x_ld) return 0;
    return mcamd_wgrad_bsparse_ok(g->ksize, g->stem, g->cout, g->cin, g->W) ? 1 : 0;
}

extern "C" int mcamd_wgrad_bsparse_elems(const mcamd_conv_geom* g, int64_t out[2]) {
    MCAMD_REQUIRE(g && out, "wgrad_bsparse_elems: null argument");
    MCAMD_REQUIRE(mcamd_conv_wgrad_bsparse_ok(g), "wgrad_bsparse_elems: geometry has no list weight gradient (mcamd_conv_wgrad_bsparse_ok)");
    const int64_t nt = (int64_t)(g->cout / 64) * (g->cin / 64);
    out[0] = nt;
    out[1] = 2 * nt;
    return MCAMD_OK;
}

extern "C" int mcamd_wgrad_bsparse_lists(const mcamd_conv_geom* g, const float* mask_oihw, int32_t* tiles, int32_t* words,
                                         int32_t* counts, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "wgrad_bsparse_lists: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) { return mcamd_wgrad_bsparse_lists(&g_, mask_oihw, tiles, words, counts, s); });
    }
    MCAMD_REQUIRE(g && mcamd_conv_wgrad_bsparse_ok(g), "wgrad_bsparse_lists: geometry has no list weight gradient (mcamd_conv_wgrad_bsparse_ok)");
    MCAMD_REQUIRE(mask_oihw && tiles && words && counts, "wgrad_bsparse_lists: null pointer");
    return mcamd_wgrad_bsparse_lists_launch(mask_oihw, g->cout, g->cin, ntaps_of(g), tiles, words, counts, (hipStream_t)stream);
}

static WgradPlan wgrad_bsparse_plan_for(const mcamd_conv_geom* g, int kept_tiles, int nsplit) {
    return mcamd_wgrad_bsparse_plan(g->ksize, (long long)g->B * g->H * g->W, padded_pixels(g), g->cout, g->cin, g->W + pw_of(g),
                                    kept_tiles, nsplit);
}

extern "C" int mcamd_conv_wgrad_bsparse_plan(const mcamd_conv_geom* g, int32_t kept_tiles, int64_t out[MCAMD_WGRAD_BSPARSE_PLAN_N]) {
    if (check_geom(g, "conv_wgrad_bsparse_plan")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(out, "conv_wgrad_bsparse_plan: null output");
    MCAMD_REQUIRE(mcamd_conv_wgrad_bsparse_ok(g), "conv_wgrad_bsparse_plan: geometry has no list weight gradient (mcamd_conv_wgrad_bsparse_ok)");
    MCAMD_REQUIRE(kept_tiles >= 0 && kept_tiles <= (g->cout / 64) * (g->cin / 64),
                  "conv_wgrad_bsparse_plan: %d kept tiles of %d", kept_tiles, (g->cout / 64) * (g->cin / 64));
    const WgradPlan p = wgrad_bsparse_plan_for(g, kept_tiles, 0);
    const WgradFinish f = mcamd_wgrad_finish_pick(p.nsplit, 0, g->cin, g->ksize, false);
    out[0] = p.nine ? MCAMD_WGRAD_NINE : MCAMD_WGRAD_GENERIC;
    out[1] = p.kp, out[2] = p.ns, out[3] = p.nsplit, out[4] = p.pix_per_split;
    out[5] = f.kernel, out[6] = f.sg;
    out[7] = (int64_t)p.bytes;
    return MCAMD_OK;
}

extern "C" int mcamd_conv_wgrad_bsparse(const mcamd_conv_geom* g, const void* x, const void* dy, int32_t dy_ld, int32_t dy_choff,
                                        const float* mask_oihw, const int32_t* tiles, const int32_t* words, int32_t ntiles,
                                        int32_t nsplit, float grad_scale, float* dw_oihw, float* dbias, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "conv_wgrad_bsparse: null geometry");
        const mcamd_conv_geom g_ = *g;
        return mcamd_rec_push(stream, [=](void* s) {
            return mcamd_conv_wgrad_bsparse(&g_, x, dy, dy_ld, dy_choff, mask_oihw, tiles, words, ntiles, nsplit, grad_scale, dw_oihw,
                                            dbias, workspace, workspace_bytes, s);
        });
    }
    if (check_geom(g, "conv_wgrad_bsparse")) return MCAMD_EINVAL;
    MCAMD_REQUIRE(mcamd_conv_wgrad_bsparse_ok(g), "conv_wgrad_bsparse: geometry has no list weight gradient (mcamd_conv_wgrad_bsparse_ok)");
    MCAMD_REQUIRE(x && dy && mask_oihw && dw_oihw && workspace, "conv_wgrad_bsparse: null argument");
    MCAMD_REQUIRE(grad_scale > 0.f, "conv_wgrad_bsparse: grad_scale must be positive");
    const int all_tiles = (g->cout / 64) * (g->cin / 64);
    MCAMD_REQUIRE(ntiles >= 0 && ntiles <= all_tiles, "conv_wgrad_bsparse: %d listed tiles of %d", ntiles, all_tiles);
    MCAMD_REQUIRE(ntiles == 0 || (tiles && (words || g->ksize == 1)), "conv_wgrad_bsparse: null list");
    // (a split holds at least one step of the kernel: more splits than steps would only sum slabs of zeros)
    const long long max_split = g->ksize == 3 ? (padded_pixels(g) + 31) / 32 : ((long long)g->B * g->H * g->W + 63) / 64;
    MCAMD_REQUIRE(nsplit >= 1 && nsplit <= max_split, "conv_wgrad_bsparse: nsplit %d outside [1, %lld]", nsplit, max_split);
    const WgradPlan p = wgrad_bsparse_plan_for(g, ntiles, nsplit);
    MCAMD_REQUIRE(dy_ld % 8 == 0 && dy_choff % 8 == 0 && dy_choff + p.rows_pad <= dy_ld,
                  "conv_wgrad_bsparse: dy slice [%d, %d) does not fit dy_ld %d", dy_choff, dy_choff + p.rows_pad, dy_ld);
    if (workspace_bytes < p.bytes) {
        mcamd_set_error("conv_wgrad_bsparse: workspace %zu < %zu bytes", workspace_bytes, p.bytes);
        return MCAMD_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    WgradArgs a = wgrad_args_of(g, x, dy, dy_ld, dy_choff, workspace);
    int rc = MCAMD_OK;
    if (ntiles > 0) rc = mcamd_wgrad_bsparse_launch(a, p, g->W + pw_of(g), padded_pixels(g), tiles, words, ntiles, st);
    if (rc) return rc;
    rc = mcamd_wgrad_finish_launch((const float*)workspace, p, a.ktot, a.cin_tap, 0, g->cout, g->cin, g->ksize, mask_oihw,
                                   1.0f / grad_scale, dw_oihw, nullptr, nullptr, st, true);
    if (rc) return rc;
    if (dbias)     // (as mcamd_conv_wgrad: the slabs are consumed, the workspace is free again in stream order)
        rc = mcamd_colsum_launch((const half_t*)dy, padded_pixels(g), dy_ld, dy_choff, g->cout, 1.0f / grad_scale, dbias, st,
                                 workspace, workspace_bytes);
    return rc;
}

// ---------------------------------------------------------------------------------------
// dgrad + producer sums + wgrad of a dense 1x1 block in one launch (conv_bwd1x1.hip)
// ---------------------------------------------------------------------------------------
static const char* bwd1x1_refusal(const mcamd_conv_geom* g) {
    if (!g) return "null geometry";
    if (g->pad != 0 && g->pad != 1) return "pad must be 0 or 1";
    const char* why = mcamd_bwd1x1_refusal(g->ksize, g->stem, g->x_wrap, g->x_f8, g->cout, g->cin);
    if (why) return why;
    if (g->x_ld % 8 != 0 || g->x_choff % 8 != 0 || g->x_choff < 0 || g->x_choff + g->cin > g->x_ld)
        return "x channel slice must be whole groups of 8 inside x_ld";
    if (g->B <= 0 || g->H <= 0 || g->W <= 0 || (long long)g->B * g->H * g->W >= (1ll << 31)) return "pixel count out of range";
    return nullptr;
}

extern "C" int32_t mcamd_conv_bwd1x1_ok(const mcamd_conv_geom* g, const char** reason) {
    const char* why = bwd1x1_refusal(g);
    if (reason) *reason = why;
    return why ? 0 : 1;
}

extern "C" int32_t mcamd_conv_bwd1x1_sums_rows(const mcamd_conv_geom* g) { return bwd1x1_refusal(g) ? 0 : MCAMD_BWD1X1_GRID; }
extern "C" int32_t mcamd_conv_bwd1x1_wgrad_splits(const mcamd_conv_geom* g) { return bwd1x1_refusal(g) ? 0 : MCAMD_BWD1X1_GRID; }
extern "C" size_t mcamd_conv_bwd1x1_workspace_bytes(const mcamd_conv_geom* g) {
    return bwd1x1_refusal(g) ? 0 : (size_t)MCAMD_BWD1X1_GRID * g->cout * g->cin * sizeof(float);
}

extern "C" int mcamd_conv_bwd1x1(const mcamd_conv_geom* g, const void* x, const void* dy, int32_t dy_ld, int32_t dy_choff,
                                 const void* wp_dgrad, void* gin, int32_t g_ld, int32_t g_choff, int32_t* overflow,
                                 const mcamd_dgrad_sums* sums, const float* mask_oihw, float grad_scale, float* dw_oihw,
                                 float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    if (mcamd_recording()) {
        MCAMD_REQUIRE(g, "conv_bwd1x1: null geometry");
        const mcamd_conv_geom g_ = *g;
        const bool has_sums = sums != nullptr;
        const mcamd_dgrad_sums s_ = has_sums ? *sums : mcamd_dgrad_sums{};
        return mcamd_rec_push(stream, [=](void* s) {
            return mcamd_conv_bwd1x1(&g_, x, dy, dy_ld, dy_choff, wp_dgrad, gin, g_ld, g_choff, overflow, has_sums ? &s_ : nullptr,
                                     mask_oihw, grad_scale, dw_oihw, dbias, workspace, workspace_bytes, s);
        });
    }
    const char* why = bwd1x1_refusal(g);
    MCAMD_REQUIRE(!why, "conv_bwd1x1: %s", why);
    MCAMD_REQUIRE(x && dy && wp_dgrad && gin && dw_oihw && workspace, "conv_bwd1x1: null argument");
    MCAMD_REQUIRE(grad_scale > 0.f, "conv_bwd1x1: grad_scale must be positive");
    MCAMD_REQUIRE(dy_ld % 8 == 0 && dy_choff % 8 == 0 && dy_choff >= 0 && dy_choff + g->cout <= dy_ld,
                  "conv_bwd1x1: dy slice [%d, %d) does not fit dy_ld %d", dy_choff, dy_choff + g->cout, dy_ld);
    MCAMD_REQUIRE(g_ld % 8 == 0 && g_choff % 8 == 0 && g_choff >= 0 && g_choff + g->cin <= g_ld,
                  "conv_bwd1x1: G slice [%d, %d) does not fit g_ld %d", g_choff, g_choff + g->cin, g_ld);
    const size_t need = mcamd_conv_bwd1x1_workspace_bytes(g);
    if (workspace_bytes < need) {
        mcamd_set_error("conv_bwd1x1: workspace %zu < %zu bytes", workspace_bytes, need);
        return MCAMD_EWORKSPACE;
    }
    Bwd1x1Launch q;
    memset(&q, 0, sizeof(q));
    q.dy = (const half_t*)dy, q.x = (const half_t*)x, q.w = (const half_t*)wp_dgrad, q.g = (half_t*)gin;
    q.slab = (float*)workspace, q.overflow = (int*)overflow;
    q.dy_ld = dy_ld, q.dy_choff = dy_choff, q.x_ld = g->x_ld, q.x_choff = g->x_choff, q.g_ld = g_ld, q.g_choff = g_choff;
    q.H = g->H, q.W = g->W, q.M = g->B * g->H * g->W, q.pw = pw_of(g), q.cout = g->cout, q.cin = g->cin;
    if (sums && sums->slab) {
        const mcamd_dgrad_sums* s = sums;
        MCAMD_REQUIRE(s->rows == MCAMD_BWD1X1_GRID, "conv_bwd1x1: sums.rows must be mcamd_conv_bwd1x1_sums_rows() = %d (got %d)",
                      MCAMD_BWD1X1_GRID, s->rows);
        MCAMD_REQUIRE(s->scale && s->shift && s->mean && s->invstd, "conv_bwd1x1: sums: null argument");
        MCAMD_REQUIRE(s->C > 0 && s->C % 8 == 0 && s->ch_lo >= 0 && s->ch_lo % 8 == 0 && s->ch_lo + s->C <= g->cin,
                      "conv_bwd1x1: sums: producer columns [%d, %d) must be whole groups of 8 inside the %d channels of G",
                      s->ch_lo, s->ch_lo + s->C, g->cin);
        MCAMD_REQUIRE(s->ld >= s->C, "conv_bwd1x1: sums.ld (%d) must be >= C (%d)", s->ld, s->C);
        // the producer's stored activation IS this block's input: the launch takes it from the X tile it has staged
        MCAMD_REQUIRE(s->act == x && s->act_ld == g->x_ld && s->act_choff == g->x_choff + s->ch_lo && (s->act_pad != 0) == (g->pad != 0),
                      "conv_bwd1x1: sums: the producer's activation must be the block's input x (same buffer, ld, form; act_choff = "
                      "x_choff + ch_lo)");
        MCAMD_REQUIRE(!s->y || (s->y_ld % 4 == 0 && s->y_choff % 4 == 0 && s->y_choff >= 0 && s->y_choff + s->C <= s->y_ld),
                      "conv_bwd1x1: sums: fp32 y slice [%d, %d) does not fit y_ld %d", s->y_choff, s->y_choff + s->C, s->y_ld);
        MCAMD_REQUIRE(s->slope > 0.f, "conv_bwd1x1: sums need an invertible activation (slope > 0)");
        q.bsum.slab = s->slab, q.bsum.ld = s->ld;
        q.bsum.scale = s->scale, q.bsum.shift = s->shift, q.bsum.mean = s->mean, q.bsum.invstd = s->invstd;
        q.bsum.y = s->y, q.bsum.y_ld = s->y_ld, q.bsum.y_choff = s->y_choff;
        q.bsum.ch_lo = s->ch_lo, q.bsum.C = s->C;
        q.bsum.slope = s->slope;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = mcamd_bwd1x1_launch(q, st);
    if (rc) return rc;
    // the workgroups' accumulators are the splits of the weight gradient's slab layout: the same finish pass
    WgradPlan p;
    memset(&p, 0, sizeof(p));
    p.nsplit = MCAMD_BWD1X1_GRID, p.rows_pad = g->cout;
    rc = mcamd_wgrad_finish_launch((const float*)workspace, p, g->cin, g->cin, 0, g->cout, g->cin, 1, mask_oihw, 1.0f / grad_scale,
                                   dw_oihw, nullptr, nullptr, st);
    if (rc) return rc;
    if (dbias)
        rc = mcamd_colsum_launch((const half_t*)dy, padded_pixels(g), dy_ld, dy_choff, g->cout, 1.0f / grad_scale, dbias, st, workspace,
                                 workspace_bytes);
    return rc;
}
