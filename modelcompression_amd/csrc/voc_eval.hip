// VOC07 evaluation of the eval path on the device (reference src/predict.py:250-437: voc_eval's greedy matching of
// detections to ground truth and voc_ap's 11-point metric), fed by what mcamd_detect leaves on the device.
//
// The file path formats every fp32 score and coordinate with "%f" and parses the text back as a double.  That rounding is
// q(v) = rint((double)v * 1e6) / 1e6 exactly: v * 1e6 is exact in a double (24 + 14 significant bits), rint is then the
// correctly rounded six-decimal value that the C library prints, and the division is the double that float() parses.
//
// mcamd_voc_match: one workgroup per image, the image's ground truth in LDS as doubles.  Each wave takes classes in turn:
// it gathers the class's emitted rows, sorts their 31-bit (1e6 - q(score) * 1e6, row) keys in its own LDS slice (a
// bitonic network inside the wave: no workgroup barrier, the waves' trip counts differ), then walks them in order with
// one lane per ground-truth object: IoU in fp64 term by term as voc_eval writes it, a wave maximum, the lowest lane
// among the maxima (np.argmax), and the matched set as a 64-bit mask.  Matching is sequential only inside one
// (image, class) pair.  Every loop is bounded by N, G or C: nothing here waits on data.
//
// mcamd_voc_ap: one workgroup per class over the records sorted by key: binary search of the class's segment, a scan of
// the tp / fp flags with a carry, the eleven maxima of precision at recall >= i * 0.1, and one thread that adds the
// eleven terms in order.
//
// Built with -ffp-contract=off: every float64 result is compared with == against numpy's.
#include <float.h>

#include "common.h"

namespace {
constexpr int MAXN = 2048, MAXC = 80, MAXG = 64, NWAVE = 4, NTHR = NWAVE * 64, AP_THR = 1024;
constexpr int R_BITS = 11, IMG_SHIFT = 11, IMG_BITS = 25, SCORE_SHIFT = 36, CLASS_SHIFT = 56;
static_assert((1 << R_BITS) == MAXN && IMG_SHIFT + IMG_BITS == SCORE_SHIFT && SCORE_SHIFT + 20 == CLASS_SHIFT,
              "key layout of include/mcamd.h");
static_assert(1000000 < (1 << 20) && MAXC <= 128, "the score field holds 0 .. 1e6, bit 63 stays clear");

struct MatchLds {
    double gt[MAXG][4];
    unsigned char gcls[MAXG], gdiff[MAXG];
    unsigned int key[NWAVE][MAXN];    // per wave: (1e6 - score6) << 11 | row, sorted ascending
    double bb[NWAVE][64][4];          // per wave: the rounded corners of the 64 records being walked
};

// LDS written by some lanes of a wave is read by others: order the accesses (the hardware runs a wave's LDS operations
// in order; this keeps the compiler from moving them).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double q6(float v) { return rint((double)v * 1e6) / 1e6; }

__device__ __forceinline__ double wave_max(double v) {
    for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(NTHR) void voc_match_kernel(mcamd_voc_match_desc a) {
    __shared__ MatchLds s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ng = min(max(a.gt_count[b], 0), a.G);          // <= MAXG
    const int nk = min(max(a.nkept[b], 0), a.N);             // <= MAXN; rows at or beyond it are never read
    if (tid < MAXG) {
        const bool v = tid < ng;
        const long long g = (long long)b * a.G + tid;
        for (int k = 0; k < 4; ++k) s.gt[tid][k] = v ? (double)a.gt_box[g * 4 + k] : 0.;
        s.gcls[tid] = v ? a.gt_cls[g] : 255;
        s.gdiff[tid] = v ? a.gt_difficult[g] : 0;
    }
    __syncthreads();
    if (nk == 0) return;                                     // uniform over the workgroup
    const float Wf = (float)a.image_size[2 * b], Hf = (float)a.image_size[2 * b + 1];
    const float* rows = a.rows + (long long)b * a.N * 8;
    const float* probs = a.probs + (long long)b * a.N * a.C;
    const unsigned long long image = (unsigned long long)(a.first_image + b);
    unsigned int* key = s.key[wv];
    double(*bb)[4] = s.bb[wv];
    for (int c = wv; c < a.C; c += NWAVE) {                  // everything below is uniform over the wave
        int m = 0;
        for (int r0 = 0; r0 < nk; r0 += 64) {
            const int r = r0 + lane;
            bool emit = false;
            unsigned int k = 0;
            if (r < nk) {
                const float p = probs[(long long)r * a.C + c];
                emit = p > a.conf_thresh || c == (int)rows[r * 8 + 6];
                const double s6 = fmin(fmax(rint((double)p * 1e6), 0.), 1e6);      // q(p) * 1e6, an integer
                k = ((unsigned int)(1000000 - (int)s6) << R_BITS) | (unsigned int)r;
            }
            const unsigned long long mask = __ballot(emit);
            if (emit) key[m + __popcll(mask & ((1ull << lane) - 1))] = k;          // emitted rows before r: <= r < MAXN
            m += __popcll(mask);
        }
        if (m == 0) continue;
        int P = 1;
        while (P < m) P <<= 1;                               // <= MAXN
        for (int i = m + lane; i < P; i += 64) key[i] = ~0u;
        wave_sync();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < (P >> 1); t += 64) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;    // hi < P
                    const unsigned int x = key[lo], y = key[hi];
                    if ((x > y) == ((lo & k) == 0)) key[lo] = y, key[hi] = x;
                }
                wave_sync();
            }
        }
        unsigned int base_lo = 0, base_hi = 0;
        if (lane == 0) {
            const unsigned long long base = atomicAdd((unsigned long long*)a.counters, (unsigned long long)m);
            base_lo = (unsigned int)base, base_hi = (unsigned int)(base >> 32);
        }
        const unsigned long long base = ((unsigned long long)(unsigned int)__shfl((int)base_hi, 0) << 32) |
                                        (unsigned int)__shfl((int)base_lo, 0);
        // lane j = ground-truth object j, in annotation order
        const bool mine = lane < ng && s.gcls[lane] == c;
        const double g0 = s.gt[lane][0], g1 = s.gt[lane][1], g2 = s.gt[lane][2], g3 = s.gt[lane][3];
        const double garea = (g2 - g0 + 1.) * (g3 - g1 + 1.);
        const unsigned long long difficult = __ballot(mine && s.gdiff[lane]);
        unsigned long long matched = 0;
        for (int i0 = 0; i0 < m; i0 += 64) {
            const int i = i0 + lane;
            unsigned int kmine = 0;
            if (i < m) {
                kmine = key[i];
                const float* o = rows + (int)(kmine & (MAXN - 1)) * 8;               // a row below nk
                const float x = o[0], y = o[1], w = o[2], h = o[3];
                bb[lane][0] = q6((x - w / 2.0f) * Wf), bb[lane][1] = q6((y - h / 2.0f) * Hf);
                bb[lane][2] = q6((x + w / 2.0f) * Wf), bb[lane][3] = q6((y + h / 2.0f) * Hf);
            }
            wave_sync();
            int myflag = 0;
            const int cnt = min(64, m - i0);
            for (int j = 0; j < cnt; ++j) {
                const double b0 = bb[j][0], b1 = bb[j][1], b2 = bb[j][2], b3 = bb[j][3];
                double ov = -INFINITY;                       // no object of the class: ovmax = -inf
                if (mine) {
                    const double iw = fmax((fmin(g2, b2) - fmax(g0, b0)) + 1., 0.);
                    const double ih = fmax((fmin(g3, b3) - fmax(g1, b1)) + 1., 0.);
                    const double inters = iw * ih;
                    const double uni = ((b2 - b0 + 1.) * (b3 - b1 + 1.) + garea) - inters;
                    ov = inters / uni;
                }
                const double ovmax = wave_max(ov);
                int flag = 2;                                // fp
                if (ovmax > a.ovthresh) {
                    const unsigned long long at = __ballot(mine && ov == ovmax);
                    if (at) {
                        const unsigned long long bit = at & (~at + 1);               // the first maximum
                        if (difficult & bit) flag = 0;
                        else if (!(matched & bit)) flag = 1, matched |= bit;
                    }
                }
                if (lane == j) myflag = flag;
            }
            const unsigned long long slot = base + (unsigned long long)i;
            const bool full = i < m && slot >= (unsigned long long)a.capacity;
            if (i < m && !full) {
                a.keys[slot] = ((unsigned long long)c << CLASS_SHIFT) | ((unsigned long long)(kmine >> R_BITS) << SCORE_SHIFT) |
                               (image << IMG_SHIFT) | (kmine & (MAXN - 1));
                a.flags[slot] = (unsigned char)myflag;
            }
            const unsigned long long lost = __ballot(full);
            if (lane == 0 && lost) atomicAdd((unsigned long long*)a.counters + 1, (unsigned long long)__popcll(lost));
            wave_sync();                                     // bb is rewritten by the next 64
        }
    }
}

struct ApArgs {
    const unsigned long long* keys;
    const unsigned char* flags;
    const unsigned long long* counters;
    long long capacity;
    const int* npos;
    double *ap, *rec, *prec;
};

__global__ __launch_bounds__(AP_THR) void voc_ap_kernel(ApArgs a) {
    __shared__ int wtp[AP_THR / 64], wfp[AP_THR / 64];
    __shared__ double wmax[AP_THR / 64][11];
    __shared__ long long seg[2];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long n = (long long)min(a.counters[0], (unsigned long long)a.capacity);
    if (tid < 2) {                                           // first position whose key is of class >= c + tid
        const unsigned long long target = (unsigned long long)(c + tid) << CLASS_SHIFT;
        long long lo = 0, hi = n;
        while (lo < hi) {                                    // <= 63 steps
            const long long mid = lo + ((hi - lo) >> 1);
            if (a.keys[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        seg[tid] = lo;
    }
    __syncthreads();
    const long long lo = seg[0], hi = seg[1];
    const double npos = (double)max(a.npos[c], 1);
    long long carry_tp = 0, carry_fp = 0;
    double pmax[11];
    for (int k = 0; k < 11; ++k) pmax[k] = 0.;
    for (long long base = lo; base < hi; base += AP_THR) {   // uniform over the workgroup
        const long long i = base + tid;
        const int f = i < hi ? a.flags[i] : 0;
        int tp = f == 1, fp = f == 2;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(tp, d), u = __shfl_up(fp, d);
            if (lane >= d) tp += t, fp += u;
        }
        if (lane == 63) wtp[wv] = tp, wfp[wv] = fp;
        __syncthreads();
        long long ctp = carry_tp + tp, cfp = carry_fp + fp;
        for (int w = 0; w < AP_THR / 64; ++w) {
            if (w < wv) ctp += wtp[w], cfp += wfp[w];
            carry_tp += wtp[w], carry_fp += wfp[w];
        }
        if (i < hi) {
            const double rec = (double)ctp / npos;
            const double prec = (double)ctp / fmax((double)ctp + (double)cfp, DBL_EPSILON);
            if (a.rec) a.rec[i] = rec;
            if (a.prec) a.prec[i] = prec;
            for (int k = 0; k < 11; ++k)
                if (rec >= (double)k * 0.1) pmax[k] = fmax(pmax[k], prec);
        }
        __syncthreads();                                     // wtp / wfp are rewritten by the next round
    }
    for (int k = 0; k < 11; ++k) {
        const double v = wave_max(pmax[k]);
        if (lane == 0) wmax[wv][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double ap = 0.;
        for (int k = 0; k < 11; ++k) {
            double p = 0.;
            for (int w = 0; w < AP_THR / 64; ++w) p = fmax(p, wmax[w][k]);
            ap = ap + p / 11.;
        }
        a.ap[c] = ap;
    }
}
}  // namespace

extern "C" int mcamd_voc_match(const mcamd_voc_match_desc* d, void* stream) {
    MCAMD_REQUIRE(d && d->rows && d->probs && d->nkept && d->gt_box && d->gt_cls && d->gt_difficult && d->gt_count &&
                      d->image_size && d->keys && d->flags && d->counters,
                  "voc_match: null argument");
    MCAMD_REQUIRE(d->B > 0 && d->N > 0 && d->C > 0 && d->G > 0, "voc_match: bad shape (B %d, N %d, C %d, G %d)", d->B, d->N,
                  d->C, d->G);
    MCAMD_REQUIRE(d->N <= MAXN, "voc_match: %d rows per image, at most %d", d->N, MAXN);
    MCAMD_REQUIRE(d->C <= MAXC, "voc_match: %d classes, at most %d", d->C, MAXC);
    MCAMD_REQUIRE(d->G <= MAXG, "voc_match: %d ground-truth objects per image, at most %d", d->G, MAXG);
    MCAMD_REQUIRE(d->capacity > 0, "voc_match: capacity %lld", (long long)d->capacity);
    MCAMD_REQUIRE(d->first_image >= 0 && (long long)d->first_image + d->B <= (1ll << IMG_BITS),
                  "voc_match: images %d .. %lld, the key holds %d bits", d->first_image, (long long)d->first_image + d->B - 1,
                  IMG_BITS);
    hipLaunchKernelGGL(voc_match_kernel, dim3(d->B), dim3(NTHR), 0, (hipStream_t)stream, *d);
    MCAMD_LAUNCH_CHECK("voc_match");
    return MCAMD_OK;
}

extern "C" int mcamd_voc_ap(const uint64_t* keys, const uint8_t* flags, const uint64_t* counters, int64_t capacity,
                            const int32_t* npos, int32_t C, double* ap, double* rec, double* prec, void* stream) {
    MCAMD_REQUIRE(keys && flags && counters && npos && ap, "voc_ap: null argument");
    MCAMD_REQUIRE(C > 0, "voc_ap: bad shape (C %d)", C);
    MCAMD_REQUIRE(C <= MAXC, "voc_ap: %d classes, at most %d", C, MAXC);
    MCAMD_REQUIRE(capacity > 0, "voc_ap: capacity %lld", (long long)capacity);
    ApArgs a;
    a.keys = (const unsigned long long*)keys, a.flags = flags, a.counters = (const unsigned long long*)counters;
    a.capacity = capacity, a.npos = npos, a.ap = ap, a.rec = rec, a.prec = prec;
    hipLaunchKernelGGL(voc_ap_kernel, dim3(C), dim3(AP_THR), 0, (hipStream_t)stream, a);
    MCAMD_LAUNCH_CHECK("voc_ap");
    return MCAMD_OK;
}
