// The device passes around a Huffman-coded model file ("MCZH", include/mcamd.h) for gfx950, wave64.
//
// histogram  uint8 symbols of ALL streams, one segment table -> uint64 hist[nseg][256].  One workgroup per group of
//            MCAMD_HZ_GROUP chunks counts into its own LDS counters and stores them; a second launch adds the workgroups'
//            counters of a stream in workgroup order.  Integer counts, fixed order: a function of the input only.
// encode     symbols + code lengths -> chunk_bit0 and the code bits.  Launches: per-chunk bit sums (into chunk_bit0) ->
//            per-stream exclusive scan in place, which is the file's index table, and the canonical codes -> the bits.  A
//            workgroup ORs its chunk's codes into zeroed LDS words and stores them; the first and the last 32-bit word of
//            a chunk, which a neighbouring chunk may share, go out by an integer atomic OR into the zeroed output.
//            Nothing floating-point, nothing that depends on an order.
// decode     code lengths + chunk_bit0 + bits -> symbols.  One lane per chunk, 64 chunks per workgroup, through a 2^12
//            entry table of the stream in LDS (8 KB): 12 bits at the reading position give the symbol and its length.
//            A lane never takes a bit at or past the end of its chunk (the next chunk's chunk_bit0, nbits for the last),
//            never loads a word behind the stream's last and never stores outside its chunk's symbols; what does not
//            fit raises the stream's flag.  A last launch counts the set bits of the streams that are bit words.
//
// A code's bits go most significant first into successive positions, position p = bit p % 64 of word p / 64: read from
// the low end of a word the code arrives bit-reversed, so both sides keep the codes reversed.  Plain C++ loads and stores
// and integer atomics; 64-bit byte offsets.
#include "common.h"

typedef unsigned long long u64;

constexpr int HZ_CHUNK = MCAMD_HZ_CHUNK;          // symbols per chunk
constexpr int HZ_GROUP = MCAMD_HZ_GROUP;          // chunks per workgroup of the histogram and decode passes
constexpr int HZ_MAXLEN = MCAMD_HZ_MAXLEN;
constexpr int HZ_TABLE = 1 << HZ_MAXLEN;
constexpr int HZ_LDS_WORDS = HZ_CHUNK * HZ_MAXLEN / 32 + 8;      // a chunk's bits from any start inside a 32-bit word
static_assert(HZ_CHUNK == 1024 && HZ_GROUP == 64 && HZ_MAXLEN == 12, "the kernels below are written for these");

extern "C" size_t mcamd_hz_workspace_bytes(int64_t nblocks, int32_t nseg) {
    if (nblocks < 0 || nseg < 0) return 0;
    return (size_t)nblocks * 256 * sizeof(unsigned) + (size_t)nseg * 256 * sizeof(unsigned short) + 16;
}

__device__ __forceinline__ long long hz_chunks(long long nsym) { return (nsym + HZ_CHUNK - 1) / HZ_CHUNK; }

// the segment workgroup `b` belongs to, by block0 (groups of chunks) or by chunk0 (chunks); both ascend
template <bool BY_CHUNK>
__device__ __forceinline__ int hz_seg_of(const mcamd_hz_seg* segs, int nseg, long long b) {
    int s = 0;
    while (s + 1 < nseg && b >= (BY_CHUNK ? segs[s + 1].chunk0 : (long long)segs[s + 1].block0)) ++s;
    return s;
}

// the length of symbol `sym` of a stream of alphabet A: 0 = absent (also what a length above the limit reads as)
__device__ __forceinline__ unsigned hz_len(const unsigned char* __restrict__ len, int A, unsigned sym) {
    const unsigned l = (int)sym < A ? len[sym] : 0u;
    return l <= (unsigned)HZ_MAXLEN ? l : 0u;
}

// ---------------------------------------------------------------------------------------
// histogram
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hz_hist_kernel(const mcamd_hz_seg* __restrict__ segs, int nseg,
                                                      const unsigned char* __restrict__ syms, long long syms_bytes,
                                                      const long long* __restrict__ dyn, unsigned* __restrict__ partial) {
    __shared__ unsigned h[4][256];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    for (int j = 0; j < 4; ++j) h[j][tid] = 0u;
    __syncthreads();
    const int s = hz_seg_of<false>(segs, nseg, b);
    const mcamd_hz_seg g = segs[s];
    long long off = g.sym0, n = g.nsym;
    if (dyn) {       // where the stream is and how long was decided on the device: inside the capacity and the buffer, or empty
        const long long o = dyn[2 * s], m = dyn[2 * s + 1];
        const bool ok = o >= 0 && (o & 7) == 0 && m >= 0 && m <= g.nsym && o + m <= syms_bytes;
        off = ok ? o : 0;
        n = ok ? m : 0;
    }
    const long long first = (long long)(b - g.block0) * HZ_GROUP * HZ_CHUNK;
    const unsigned char* src = syms + off;
    for (int k = 0; k < HZ_GROUP * HZ_CHUNK / 1024; ++k) {
        const long long i = first + 4ll * (tid + 256 * k);
        if (i + 4 <= n) {
            const unsigned v = *(const unsigned*)(src + i);
            atomicAdd(&h[wave][v & 0xffu], 1u);
            atomicAdd(&h[wave][(v >> 8) & 0xffu], 1u);
            atomicAdd(&h[wave][(v >> 16) & 0xffu], 1u);
            atomicAdd(&h[wave][v >> 24], 1u);
        } else {
            for (long long j = i; j < n; ++j) atomicAdd(&h[wave][src[j]], 1u);
        }
    }
    __syncthreads();
    partial[(long long)b * 256 + tid] = h[0][tid] + h[1][tid] + h[2][tid] + h[3][tid];
}

// one workgroup per stream: thread t adds the workgroups' counts of symbol t in workgroup order
__global__ __launch_bounds__(256) void hz_hist_sum_kernel(const mcamd_hz_seg* __restrict__ segs, const unsigned* __restrict__ partial,
                                                          u64* __restrict__ hist) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const mcamd_hz_seg g = segs[s];
    const long long nb = (hz_chunks(g.nsym) + HZ_GROUP - 1) / HZ_GROUP;
    u64 c = 0;
    for (long long j = 0; j < nb; ++j) c += partial[(g.block0 + j) * 256 + tid];
    hist[(long long)s * 256 + tid] = c;
}

// ---------------------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------------------
// the (up to) four symbols of thread `tid` in chunk `c` of the stream at `src` with `n` symbols; returns how many
__device__ __forceinline__ int hz_four(const unsigned char* __restrict__ src, long long n, long long c, int tid, unsigned (&sym)[4]) {
    const long long i = c * HZ_CHUNK + 4ll * tid;
    if (i + 4 <= n) {
        const unsigned v = *(const unsigned*)(src + i);
        sym[0] = v & 0xffu, sym[1] = (v >> 8) & 0xffu, sym[2] = (v >> 16) & 0xffu, sym[3] = v >> 24;
        return 4;
    }
    int m = 0;
    for (long long j = i; j < n; ++j) sym[m++] = src[j];
    return m;
}

// one workgroup per chunk: the sum of its symbols' code lengths, stored where the scan turns it into chunk_bit0
__global__ __launch_bounds__(256) void hz_chunk_bits_kernel(const mcamd_hz_seg* __restrict__ segs, int nseg,
                                                            const unsigned char* __restrict__ syms,
                                                            const unsigned char* __restrict__ length, unsigned* __restrict__ ctab) {
    __shared__ unsigned char lens[256];
    __shared__ unsigned wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = hz_seg_of<true>(segs, nseg, blockIdx.x);
    const mcamd_hz_seg g = segs[s];
    lens[tid] = (unsigned char)hz_len(length + 256ll * s, g.A, (unsigned)tid);
    __syncthreads();
    unsigned sym[4];
    const int m = hz_four(syms + g.sym0, g.nsym, (long long)blockIdx.x - g.chunk0, tid, sym);
    unsigned t = 0;
    for (int j = 0; j < m; ++j) t += lens[sym[j]];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d);
    if (lane == 0) wsum[wave] = t;
    __syncthreads();
    if (tid == 0) ctab[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one wave per stream: the exclusive scan of its chunks' bit sums, in place (64 per step, each step loads before it
// stores), and the stream's canonical codes, bit-reversed: symbols in (length, symbol) order take increasing values
__global__ __launch_bounds__(64) void hz_scan_kernel(const mcamd_hz_seg* __restrict__ segs, const unsigned char* __restrict__ length,
                                                     unsigned* __restrict__ ctab, unsigned short* __restrict__ codes) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const mcamd_hz_seg g = segs[s];
    if (lane == 0) {
        const unsigned char* len = length + 256ll * s;
        unsigned cnt[HZ_MAXLEN + 2], next[HZ_MAXLEN + 2];
        for (int l = 0; l <= HZ_MAXLEN + 1; ++l) cnt[l] = 0u;
        for (int a = 0; a < 256; ++a) ++cnt[hz_len(len, g.A, (unsigned)a)];
        cnt[0] = 0u;
        unsigned code = 0u;
        for (int l = 1; l <= HZ_MAXLEN; ++l) {
            code = (code + cnt[l - 1]) << 1;
            next[l] = code;
        }
        for (int a = 0; a < 256; ++a) {
            const unsigned l = hz_len(len, g.A, (unsigned)a);
            codes[256ll * s + a] = l ? (unsigned short)((__brev(next[l]++) >> (32 - l)) & (unsigned)(HZ_TABLE - 1)) : (unsigned short)0;
        }
    }
    const long long nc = hz_chunks(g.nsym);
    unsigned carry = 0u;
    for (long long base = 0; base < nc; base += 64) {
        const long long idx = base + lane;
        const unsigned v = idx < nc ? ctab[g.chunk0 + idx] : 0u;
        unsigned x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (idx < nc) ctab[g.chunk0 + idx] = carry + x - v;
        carry += __shfl(x, 63);
    }
}

// one workgroup per chunk: the bits
__global__ __launch_bounds__(256) void hz_bits_kernel(const mcamd_hz_seg* __restrict__ segs, int nseg,
                                                      const unsigned char* __restrict__ syms, const unsigned char* __restrict__ length,
                                                      const unsigned short* __restrict__ codes, const unsigned* __restrict__ ctab,
                                                      unsigned* __restrict__ bits32) {
    __shared__ unsigned short rev[256];
    __shared__ unsigned char lens[256];
    __shared__ unsigned img[HZ_LDS_WORDS];
    __shared__ unsigned wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = hz_seg_of<true>(segs, nseg, blockIdx.x);
    const mcamd_hz_seg g = segs[s];
    lens[tid] = (unsigned char)hz_len(length + 256ll * s, g.A, (unsigned)tid);
    rev[tid] = codes[256ll * s + tid];
    for (int j = tid; j < HZ_LDS_WORDS; j += 256) img[j] = 0u;
    __syncthreads();
    unsigned sym[4];
    const int m = hz_four(syms + g.sym0, g.nsym, (long long)blockIdx.x - g.chunk0, tid, sym);
    u64 acc = 0ull;                                       // the thread's codes, the first one lowest: at most 48 bits
    unsigned t = 0;
    for (int j = 0; j < m; ++j) {
        acc |= (u64)rev[sym[j]] << t;
        t += lens[sym[j]];
    }
    unsigned x = t;                                       // inclusive scan over the workgroup
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    unsigned before = 0u, total = 0u;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    const unsigned bit0 = ctab[blockIdx.x];
    const unsigned p = (bit0 & 31u) + before + x - t;     // relative to the chunk's first 32-bit word
    const unsigned w0 = p >> 5, sh = p & 31u;
    const u64 lo = acc << sh;
    const unsigned hi = sh ? (unsigned)(acc >> (64u - sh)) : 0u;
    if ((unsigned)lo) atomicOr(&img[w0], (unsigned)lo);
    if ((unsigned)(lo >> 32)) atomicOr(&img[w0 + 1], (unsigned)(lo >> 32));
    if (hi) atomicOr(&img[w0 + 2], hi);
    __syncthreads();
    const unsigned nw = ((bit0 & 31u) + total + 31u) >> 5;
    const u64 limit = 2ull * (((u64)g.nbits + 63ull) / 64ull);      // the stream's 32-bit words: nothing is stored past them
    unsigned* dst = bits32 + 2ll * g.word0;
    for (unsigned j = tid; j < nw; j += 256) {
        const u64 idx = (u64)(bit0 >> 5) + j;
        if (idx >= limit) break;
        const unsigned v = img[j];
        if (j == 0 || j == nw - 1) {                      // a neighbouring chunk may own bits of this word
            if (v) atomicOr(&dst[idx], v);
        } else {
            dst[idx] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hz_decode_kernel(const mcamd_hz_seg* __restrict__ segs, int nseg,
                                                       const unsigned char* __restrict__ length, const unsigned* __restrict__ ctab,
                                                       const u64* __restrict__ bits, unsigned char* __restrict__ out,
                                                       u64* __restrict__ stats) {
    __shared__ unsigned short table[HZ_TABLE];            // 12 bits at the reading position -> symbol | length << 8; 0 = unassigned
    __shared__ unsigned char sorted[256];                 // the symbols in (length, symbol) order
    __shared__ unsigned first[HZ_MAXLEN + 1], offs[HZ_MAXLEN + 1], cnt[HZ_MAXLEN + 2];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int s = hz_seg_of<false>(segs, nseg, b);
    const mcamd_hz_seg g = segs[s];
    const unsigned char* len = length + 256ll * s;
    if (lane == 0) {
        for (int l = 0; l <= HZ_MAXLEN + 1; ++l) cnt[l] = 0u;
        for (int a = 0; a < 256; ++a) ++cnt[hz_len(len, g.A, (unsigned)a)];
        cnt[0] = 0u;
        unsigned code = 0u, o = 0u, fill[HZ_MAXLEN + 1];
        for (int l = 1; l <= HZ_MAXLEN; ++l) {
            code = (code + cnt[l - 1]) << 1;
            first[l] = code;
            offs[l] = fill[l] = o;
            o += cnt[l];
        }
        for (int a = 0; a < 256; ++a) {
            const unsigned l = hz_len(len, g.A, (unsigned)a);
            if (l) sorted[fill[l]++] = (unsigned char)a;
        }
    }
    __syncthreads();
    for (int k = 0; k < HZ_TABLE / 64; ++k) {
        const unsigned idx = (unsigned)(lane + 64 * k);
        const unsigned v = __brev(idx) >> (32 - HZ_MAXLEN);    // the 12 bits in code order
        unsigned entry = 0u;
        for (int l = 1; l <= HZ_MAXLEN; ++l) {
            const unsigned pre = v >> (HZ_MAXLEN - l);
            if (pre >= first[l] && pre - first[l] < cnt[l]) {
                entry = (unsigned)sorted[offs[l] + pre - first[l]] | (unsigned)l << 8;
                break;
            }
        }
        table[idx] = (unsigned short)entry;
    }
    __syncthreads();
    const long long nc = hz_chunks(g.nsym);
    const long long c = (long long)(b - g.block0) * HZ_GROUP + lane;
    if (c >= nc) return;
    const u64 nbits = (u64)g.nbits;
    const u64 start = ctab[g.chunk0 + c];
    const u64 end = c + 1 < nc ? (u64)ctab[g.chunk0 + c + 1] : nbits;
    const long long rest = g.nsym - c * HZ_CHUNK;
    const int count = rest < HZ_CHUNK ? (int)rest : HZ_CHUNK;
    bool bad = start > end || end > nbits;
    if (!bad) {
        const unsigned* w32 = (const unsigned*)(bits + g.word0);
        const u64 nw32 = 2ull * ((nbits + 63ull) / 64ull);     // no word behind the stream's last is loaded
        unsigned char* dst = out + g.sym0 + c * HZ_CHUNK;
        u64 p = start, k = start >> 5;
        u64 buf = (k < nw32 ? (u64)w32[k] : 0ull) >> (start & 31ull);
        int avail = 32 - (int)(start & 31ull);
        ++k;
        unsigned word = 0u;
        int i = 0;
        for (; i < count; ++i) {
            if (avail < HZ_MAXLEN) {
                buf |= (k < nw32 ? (u64)w32[k] : 0ull) << avail;
                avail += 32;
                ++k;
            }
            const unsigned e = table[(unsigned)buf & (unsigned)(HZ_TABLE - 1)];
            const unsigned l = e >> 8;
            if (l == 0u || p + l > end) {                 // an unassigned code, or a code that runs into the next chunk
                bad = true;
                break;
            }
            word |= (e & 0xffu) << (8 * (i & 3));
            if ((i & 3) == 3) {
                *(unsigned*)(dst + i - 3) = word;
                word = 0u;
            }
            buf >>= l;
            avail -= (int)l;
            p += l;
        }
        for (int j = i & ~3; j < i; ++j) dst[j] = (unsigned char)(word >> (8 * (j & 3)));      // the symbols of a last, partial group
        if (p != end) bad = true;
    }
    if (bad) atomicOr(&stats[2ll * s], 1ull);
}

// one workgroup per stream whose symbols are bit words (popc_bits > 0): the set bits among the first popc_bits, and a
// flag for a set bit behind them
__global__ __launch_bounds__(256) void hz_popc_kernel(const mcamd_hz_seg* __restrict__ segs, const unsigned char* __restrict__ out,
                                                      u64* __restrict__ stats) {
    __shared__ u64 part[4];
    __shared__ int tail[4];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const mcamd_hz_seg g = segs[s];
    if (g.popc_bits <= 0) return;                         // (uniform)
    const u64* words = (const u64*)(out + g.sym0);
    const long long nw = g.nsym / 8;
    u64 ones = 0ull;
    int past = 0;
    for (long long j = tid; j < nw; j += 256) {
        const u64 w = words[j];
        const long long valid = g.popc_bits - 64 * j;     // bits of this word that stand for a weight
        const u64 keep = valid >= 64 ? ~0ull : valid <= 0 ? 0ull : (1ull << valid) - 1ull;
        ones += (u64)__popcll(w & keep);
        past |= (w & ~keep) != 0ull;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        ones += __shfl_xor(ones, d);
        past |= __shfl_xor(past, d);
    }
    if (lane == 0) part[wave] = ones, tail[wave] = past;
    __syncthreads();
    if (tid == 0) {
        stats[2ll * s + 1] = part[0] + part[1] + part[2] + part[3];
        if (tail[0] | tail[1] | tail[2] | tail[3]) atomicOr(&stats[2ll * s], 2ull);
    }
}

// ---------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------
enum { HZ_HIST, HZ_ENCODE, HZ_DECODE };

struct HzTotals {
    long long blocks, chunks;
};

static int hz_check_table(const char* what, int pass, const mcamd_hz_seg* segs, int nseg, long long syms_bytes, bool dyn,
                          long long chunk_cap, long long bits_cap, HzTotals* t) {
    long long blocks = 0, chunks = 0;
    for (int s = 0; s < nseg; ++s) {
        const mcamd_hz_seg& g = segs[s];
        MCAMD_REQUIRE(g.nsym >= 0 && g.A >= 1 && g.A <= 256, "%s: segment %d: bad stream (nsym %lld, alphabet %d)", what, s,
                      (long long)g.nsym, g.A);
        const long long nc = (g.nsym + HZ_CHUNK - 1) / HZ_CHUNK;
        MCAMD_REQUIRE(g.block0 == blocks, "%s: segment %d: block0 %d is not the running sum %lld", what, s, g.block0, blocks);
        if (!(pass == HZ_HIST && dyn))
            MCAMD_REQUIRE(g.sym0 >= 0 && g.sym0 % 8 == 0 && g.sym0 + g.nsym <= syms_bytes,
                          "%s: segment %d: symbols [%lld, +%lld) outside the %lld bytes given", what, s, (long long)g.sym0,
                          (long long)g.nsym, syms_bytes);
        if (pass != HZ_HIST) {
            MCAMD_REQUIRE(g.nbits >= 0 && g.nbits < (1ll << 32) && g.nbits <= (long long)HZ_MAXLEN * g.nsym,
                          "%s: segment %d: nbits %lld for %lld symbols (< 2^32, at most %d a symbol)", what, s, (long long)g.nbits,
                          (long long)g.nsym, HZ_MAXLEN);
            const long long nwords = (g.nbits + 63) / 64;
            MCAMD_REQUIRE(g.word0 >= 0 && g.word0 + nwords <= bits_cap, "%s: segment %d: code words [%lld, +%lld) outside the %lld given",
                          what, s, (long long)g.word0, nwords, bits_cap);
            if (pass == HZ_ENCODE)
                MCAMD_REQUIRE(g.chunk0 == chunks, "%s: segment %d: chunk0 %lld is not the running sum %lld", what, s,
                              (long long)g.chunk0, chunks);
            MCAMD_REQUIRE(g.chunk0 >= 0 && g.chunk0 + nc <= chunk_cap, "%s: segment %d: chunk_bit0 [%lld, +%lld) outside the %lld given",
                          what, s, (long long)g.chunk0, nc, chunk_cap);
        }
        if (pass == HZ_DECODE)
            MCAMD_REQUIRE(g.popc_bits >= 0 && (g.popc_bits == 0 || (g.nsym % 8 == 0 && g.popc_bits <= 8 * g.nsym)),
                          "%s: segment %d: popc_bits %lld with %lld symbols", what, s, (long long)g.popc_bits, (long long)g.nsym);
        chunks += nc;
        blocks += (nc + HZ_GROUP - 1) / HZ_GROUP;
        MCAMD_REQUIRE(blocks < (1ll << 31) && chunks < (1ll << 31), "%s: too many symbols", what);
    }
    t->blocks = blocks, t->chunks = chunks;
    return MCAMD_OK;
}

static int hz_workspace_ok(const char* what, size_t have, long long blocks, int nseg) {
    if (have < mcamd_hz_workspace_bytes(blocks, nseg)) {
        mcamd_set_error("%s: workspace too small", what);
        return MCAMD_EWORKSPACE;
    }
    return MCAMD_OK;
}

extern "C" int mcamd_hz_histogram(const mcamd_hz_seg* segs, const mcamd_hz_seg* segs_dev, int32_t nseg, const uint8_t* syms,
                                  int64_t syms_bytes, const int64_t* dyn, uint64_t* hist, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    const char* what = "hz_histogram";
    MCAMD_REQUIRE(!mcamd_recording(), "%s: not recordable into a launch plan", what);
    MCAMD_REQUIRE(segs && segs_dev && nseg > 0 && syms && syms_bytes >= 0 && hist && workspace, "%s: null argument", what);
    HzTotals t;
    int rc = hz_check_table(what, HZ_HIST, segs, nseg, syms_bytes, dyn != nullptr, 0, 0, &t);
    if (rc) return rc;
    if ((rc = hz_workspace_ok(what, workspace_bytes, t.blocks, nseg))) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned* partial = (unsigned*)workspace;
    if (t.blocks)
        hipLaunchKernelGGL(hz_hist_kernel, dim3((int)t.blocks), dim3(256), 0, st, segs_dev, nseg, (const unsigned char*)syms,
                           (long long)syms_bytes, (const long long*)dyn, partial);
    hipLaunchKernelGGL(hz_hist_sum_kernel, dim3(nseg), dim3(256), 0, st, segs_dev, (const unsigned*)partial, (u64*)hist);
    MCAMD_LAUNCH_CHECK(what);
    return MCAMD_OK;
}

extern "C" int mcamd_hz_encode(const mcamd_hz_seg* segs, const mcamd_hz_seg* segs_dev, int32_t nseg, const uint8_t* syms,
                               int64_t syms_bytes, const uint8_t* length, uint32_t* chunk_bit0, int64_t chunk_cap, uint64_t* bits,
                               int64_t bits_cap, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "hz_encode";
    MCAMD_REQUIRE(!mcamd_recording(), "%s: not recordable into a launch plan", what);
    MCAMD_REQUIRE(segs && segs_dev && nseg > 0 && syms && syms_bytes >= 0 && length && chunk_bit0 && bits && workspace,
                  "%s: null argument", what);
    HzTotals t;
    int rc = hz_check_table(what, HZ_ENCODE, segs, nseg, syms_bytes, false, chunk_cap, bits_cap, &t);
    if (rc) return rc;
    if ((rc = hz_workspace_ok(what, workspace_bytes, t.blocks, nseg))) return rc;
    if (t.chunks == 0) return MCAMD_OK;
    hipStream_t st = (hipStream_t)stream;
    unsigned short* codes = (unsigned short*)workspace;
    hipLaunchKernelGGL(hz_chunk_bits_kernel, dim3((int)t.chunks), dim3(256), 0, st, segs_dev, nseg, (const unsigned char*)syms,
                       (const unsigned char*)length, (unsigned*)chunk_bit0);
    hipLaunchKernelGGL(hz_scan_kernel, dim3(nseg), dim3(64), 0, st, segs_dev, (const unsigned char*)length, (unsigned*)chunk_bit0, codes);
    hipLaunchKernelGGL(hz_bits_kernel, dim3((int)t.chunks), dim3(256), 0, st, segs_dev, nseg, (const unsigned char*)syms,
                       (const unsigned char*)length, (const unsigned short*)codes, (const unsigned*)chunk_bit0, (unsigned*)bits);
    MCAMD_LAUNCH_CHECK(what);
    return MCAMD_OK;
}

extern "C" int mcamd_hz_decode(const mcamd_hz_seg* segs, const mcamd_hz_seg* segs_dev, int32_t nseg, const uint8_t* length,
                               const uint32_t* chunk_bit0, int64_t chunk_cap, const uint64_t* bits, int64_t bits_cap, uint8_t* out,
                               int64_t out_bytes, uint64_t* stats, void* stream) {
    const char* what = "hz_decode";
    MCAMD_REQUIRE(!mcamd_recording(), "%s: not recordable into a launch plan", what);
    MCAMD_REQUIRE(segs && segs_dev && nseg > 0 && length && chunk_bit0 && bits && out && out_bytes >= 0 && stats, "%s: null argument",
                  what);
    HzTotals t;
    const int rc = hz_check_table(what, HZ_DECODE, segs, nseg, out_bytes, false, chunk_cap, bits_cap, &t);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, (size_t)nseg * 2 * sizeof(u64), st) != hipSuccess) {
        mcamd_set_error("%s: clearing the stream flags failed", what);
        return MCAMD_ELAUNCH;
    }
    if (t.blocks)
        hipLaunchKernelGGL(hz_decode_kernel, dim3((int)t.blocks), dim3(64), 0, st, segs_dev, nseg, (const unsigned char*)length,
                           (const unsigned*)chunk_bit0, (const u64*)bits, (unsigned char*)out, (u64*)stats);
    hipLaunchKernelGGL(hz_popc_kernel, dim3(nseg), dim3(256), 0, st, segs_dev, (const unsigned char*)out, (u64*)stats);
    MCAMD_LAUNCH_CHECK(what);
    return MCAMD_OK;
}
