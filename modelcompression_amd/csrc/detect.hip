// Detection post-processing of the eval path (reference src/nets2_utils.py:141-259 get_region_boxes + nms, as
// predict.py:148-173 chains them): region decode, confidence threshold, the reference's sort by 1 - box_conf, greedy
// NMS and the compaction of the kept rows, in ONE launch per batch with no host round trip.
//
// modelcompression_amd/nets2_utils.py restates that chain as batched torch operations (region_boxes_tensors,
// nms_tensors, detections: ~20 small launches, a [16, n, n] IoU tensor per chunk of images and a host synchronisation per
// four sweeps of its fixed-point iteration).  Those functions stay: they are what these kernels are checked against.
//
// One workgroup per image.  LDS holds the decoded boxes of all N = H W A rows and one 64-bit (key bits, row) pair per
// candidate; the pairs are sorted with a bitonic network over the next power of two, which gives the reference's stable
// order (ascending fp32 key 1 - conf, ties by lower row) whatever order the candidates were appended in.  Suppression
// walks the sorted list in blocks of 64: all waves compute which earlier entries of the block overlap which, wave 0 then
// resolves the block without a workgroup barrier (lane l holds the bit mask of the earlier lanes that overlap it, a
// 64-step ballot loop decides the lanes in order), after which all threads apply the block's survivors to the later
// candidates.  Three barriers per block instead of one per candidate.
// Every loop is bounded by N (or by 64): nothing here waits on data.
//
// Built with -ffp-contract=off: the suppression decisions are comparisons of fp32 expressions that the tests reproduce
// operation by operation on the host, and mcamd_detect's decode is bit-equal to mcamd_region_decode's because both call
// decode_row().
#include "common.h"

namespace {
constexpr int NTHR = 1024, MAXN = 2048, MAXC = 80;
static_assert(NTHR / 64 * 4 == 64, "suppress_sorted: every wave takes 4 of a block's 64 entries");

struct DetArgs {
    const float* out;      // [B][A*(5+C)][H][W]
    float* head;           // [B][N][7] or NULL
    float* cls;            // [B][N][C] or NULL
    float* rows;           // [B][N][8]  (mcamd_detect)
    float* probs;          // [B][N][C]  (mcamd_detect)
    int* nkept;            // [B]        (mcamd_detect)
    int B, A, C, H, W;
    float aw[8], ah[8];
    float conf_thresh, nms_thresh;
};

struct Head {
    float x, y, w, h, conf, cmax;
    int cid;
};

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// One row of region_boxes_tensors (nets2_utils.py:141-190): anchor `an` at cell r = cy W + cx of image b.
// cls_row (may be NULL) receives the C softmax confidences, prob_row (may be NULL) box_conf * each of them.
__device__ __forceinline__ Head decode_row(const DetArgs& a, int b, int an, int r, float* cls_row, float* prob_row) {
    const int HW = a.H * a.W, K = 5 + a.C, j = r / a.W, i = r - j * a.W;
    const float* p = a.out + ((long long)b * a.A * K + (long long)an * K) * HW + r;
    Head h;
    h.x = (sigmoidf_(p[0]) + (float)i) / (float)a.W;
    h.y = (sigmoidf_(p[HW]) + (float)j) / (float)a.H;
    h.w = expf(p[2 * HW]) * a.aw[an] / (float)a.W;
    h.h = expf(p[3 * HW]) * a.ah[an] / (float)a.H;
    h.conf = sigmoidf_(p[4 * HW]);
    const float* q = p + 5 * HW;
    float mx = q[0];
    for (int c = 1; c < a.C; ++c) mx = fmaxf(mx, q[c * HW]);
    float se = 0.f;
    for (int c = 0; c < a.C; ++c) se += expf(q[c * HW] - mx);
    h.cmax = -1.f, h.cid = 0;
    for (int c = 0; c < a.C; ++c) {
        const float v = expf(q[c * HW] - mx) / se;
        if (cls_row) cls_row[c] = v;
        if (prob_row) prob_row[c] = h.conf * v;
        if (v > h.cmax) h.cmax = v, h.cid = c;           // the first maximum wins (torch.max)
    }
    return h;
}

// _iou_matrix_cwh of nets2_utils.py = bbox_iou(x1y1x2y2=False), nets2_utils.py:63-98, term by term (region_loss.hip iou_cwh).
// Symmetric in its two boxes bit for bit.
__device__ __forceinline__ float iou_cwh(const float4 p, const float4 q) {
    const float mx = fminf(p.x - p.z / 2.0f, q.x - q.z / 2.0f), Mx = fmaxf(p.x + p.z / 2.0f, q.x + q.z / 2.0f);
    const float my = fminf(p.y - p.w / 2.0f, q.y - q.w / 2.0f), My = fmaxf(p.y + p.w / 2.0f, q.y + q.w / 2.0f);
    const float cw = p.z + q.z - (Mx - mx), ch = p.w + q.w - (My - my);
    if (cw <= 0.f || ch <= 0.f) return 0.f;
    const float carea = cw * ch;
    const float uarea = p.z * p.w + q.z * q.w - carea;
    return carea / uarea;
}

// fp32 -> 32 bits whose unsigned order is the order of the floats (-0 sorts below +0; 1 - conf never yields -0)
__device__ __forceinline__ unsigned int key_bits(float v) {
    const unsigned int u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct Lds {
    float4 box[MAXN];                 // by row
    unsigned long long key[MAXN];     // (key bits << 32) | row, sorted ascending; entries [M, P) are all ones
    unsigned char alive[MAXN];        // by sorted position
    unsigned long long keptmask[MAXN / 64];
    int blockbase[MAXN / 64];         // kept entries before the block
    float4 sbox[64];                  // boxes of the current block's survivors, in order
    unsigned char over4[NTHR / 64][64];   // 4 bits each: entries 4g .. 4g+3 of the block overlap lane l's box
    int count;
};

__device__ __forceinline__ int pow2_at_least(int m) {
    int p = 1;
    while (p < m) p <<= 1;            // m <= MAXN: at most 11 steps
    return p;
}

// Bitonic sort of s.key[0, P), P a power of two <= MAXN.  Every index is < P.  Ends with a barrier.
__device__ __forceinline__ void sort_keys(Lds& s, int P, int tid) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += NTHR) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;      // bit j clear / set; hi < P
                const unsigned long long x = s.key[lo], y = s.key[hi];
                if ((x > y) == ((lo & k) == 0)) s.key[lo] = y, s.key[hi] = x;
            }
            __syncthreads();
        }
    }
}

// Greedy suppression (nets2_utils.py:236-259) over the sorted entries [0, M), M <= MAXN: on entry alive[i] tells whether
// entry i is a candidate, on return whether it is kept; keptmask / blockbase describe the kept set per block of 64 and
// the return value is its size.  alive[] must be visible (barrier) before the call; ends with a barrier.
// Per block of 64 sorted entries, three barriers:
//   1. all 16 waves: wave g tests lane l's box against entries 4g .. 4g+3 of the block (those before l) -> over4[g][l]
//   2. wave 0: lane l gathers its 64-bit mask of overlapping earlier lanes; 64 ballot steps decide the lanes in order
//      (lane q is decided at step q, when every earlier lane is final); the survivors' boxes are compacted into sbox[]
//   3. all threads: later candidates are tested against the block's survivors
__device__ __forceinline__ int suppress_sorted(Lds& s, int M, float thresh, int tid) {
    const int nblk = (M + 63) >> 6;   // <= MAXN / 64
    const int lane = tid & 63, grp = tid >> 6;        // NTHR / 64 = 16 groups of 4 entries = the 64 of a block
    int running = 0;                  // wave 0 only
    for (int k = 0; k < nblk; ++k) {
        const int base = k << 6, nq = min(64, M - base);
        {
            const bool valid = lane < nq;
            const float4 mine = s.box[valid ? (int)(unsigned int)s.key[base + lane] : 0];
            unsigned int bits = 0;
            for (int qq = 0; qq < 4; ++qq) {
                const int q = 4 * grp + qq;           // < 64
                if (valid && q < lane && iou_cwh(s.box[(int)(unsigned int)s.key[base + q]], mine) > thresh) bits |= 1u << qq;
            }                                         // q < lane < nq: base + q < M
            s.over4[grp][lane] = (unsigned char)bits;
        }
        __syncthreads();
        if (tid < 64) {
            const int i = base + tid;
            const bool valid = tid < nq;
            const bool cand = valid && s.alive[i];
            unsigned long long over = 0;              // earlier lanes of the block whose box overlaps mine
            for (int g = 0; g < NTHR / 64; ++g) over |= (unsigned long long)s.over4[g][tid] << (4 * g);
            unsigned long long kept = 0;
            for (int q = 0; q < 64; ++q) {
                const unsigned long long ok = __ballot(cand && !(over & kept));
                kept |= ok & (1ull << q);
            }
            const bool mine_kept = (kept >> tid) & 1;
            if (valid) s.alive[i] = mine_kept;
            if (mine_kept) s.sbox[__popcll(kept & ((1ull << tid) - 1))] = s.box[(int)(unsigned int)s.key[i]];   // < 64
            if (tid == 0) s.keptmask[k] = kept, s.blockbase[k] = running;
            running += __popcll(kept);
        }
        __syncthreads();
        const int nsurv = __popcll(s.keptmask[k]);    // <= 64
        for (int jx = base + 64 + tid; jx < M; jx += NTHR) {
            if (!s.alive[jx]) continue;
            const float4 mine = s.box[(int)(unsigned int)s.key[jx]];
            for (int q = 0; q < nsurv; ++q) {
                if (iou_cwh(s.sbox[q], mine) > thresh) {
                    s.alive[jx] = 0;
                    break;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) s.count = running;
    __syncthreads();
    return s.count;
}

__global__ __launch_bounds__(NTHR) void region_decode_kernel(DetArgs a) {
    const int b = blockIdx.x, HW = a.H * a.W, N = HW * a.A;
    for (int t = threadIdx.x; t < N; t += NTHR) {        // threads along w: the channel-plane reads coalesce
        const int an = t / HW, r = t - an * HW, n = r * a.A + an;
        const long long row = (long long)b * N + n;
        const Head h = decode_row(a, b, an, r, a.cls ? a.cls + row * a.C : nullptr, nullptr);
        float* o = a.head + row * 7;
        o[0] = h.x, o[1] = h.y, o[2] = h.w, o[3] = h.h, o[4] = h.conf, o[5] = h.cmax, o[6] = (float)h.cid;
    }
}

__global__ __launch_bounds__(NTHR) void nms_kernel(const float* boxes, const float* conf, int n, float thresh, int* order,
                                                   unsigned char* kept) {
    __shared__ Lds s;
    const int b = blockIdx.x, tid = threadIdx.x, P = pow2_at_least(n);
    const float4* bx = (const float4*)boxes + (long long)b * n;
    const float* cf = conf + (long long)b * n;
    for (int i = tid; i < P; i += NTHR) {
        if (i < n) {
            s.box[i] = bx[i];
            s.key[i] = ((unsigned long long)key_bits(1.0f - cf[i]) << 32) | (unsigned int)i;
        } else {
            s.key[i] = ~0ull;
        }
    }
    __syncthreads();
    sort_keys(s, P, tid);
    for (int i = tid; i < n; i += NTHR) {
        const int src = (int)(unsigned int)s.key[i];
        order[(long long)b * n + i] = src;
        s.alive[i] = cf[src] > 0.f;
    }
    __syncthreads();
    suppress_sorted(s, n, thresh, tid);
    for (int i = tid; i < n; i += NTHR) kept[(long long)b * n + i] = s.alive[i];
}

__global__ __launch_bounds__(NTHR) void detect_kernel(DetArgs a) {
    __shared__ Lds s;
    const int b = blockIdx.x, tid = threadIdx.x, HW = a.H * a.W, N = HW * a.A;
    if (tid == 0) s.count = 0;
    __syncthreads();
    for (int t = tid; t < N; t += NTHR) {
        const int an = t / HW, r = t - an * HW, n = r * a.A + an;
        const long long row = (long long)b * N + n;
        const Head h = decode_row(a, b, an, r, a.cls ? a.cls + row * a.C : nullptr, nullptr);
        if (a.head) {
            float* o = a.head + row * 7;
            o[0] = h.x, o[1] = h.y, o[2] = h.w, o[3] = h.h, o[4] = h.conf, o[5] = h.cmax, o[6] = (float)h.cid;
        }
        s.box[n] = make_float4(h.x, h.y, h.w, h.h);
        if (h.conf * h.cmax > a.conf_thresh) {
            const int slot = atomicAdd(&s.count, 1);     // < N: one slot per row at most
            s.key[slot] = ((unsigned long long)key_bits(1.0f - h.conf) << 32) | (unsigned int)n;
        }
    }
    __syncthreads();
    const int M = s.count;
    if (M == 0) {                                        // uniform over the workgroup
        if (tid == 0) a.nkept[b] = 0;
        return;
    }
    const int P = pow2_at_least(M);
    for (int i = M + tid; i < P; i += NTHR) s.key[i] = ~0ull;
    for (int i = tid; i < M; i += NTHR) s.alive[i] = 1;
    __syncthreads();
    sort_keys(s, P, tid);
    const int total = suppress_sorted(s, M, a.nms_thresh, tid);
    if (tid == 0) a.nkept[b] = total;
    // kept rows in sorted order; head and class probabilities are recomputed by the decode they came from
    for (int i = tid; i < M; i += NTHR) {
        if (!s.alive[i]) continue;
        const int n = (int)(unsigned int)s.key[i], r = n / a.A, an = n - r * a.A;
        const int pos = s.blockbase[i >> 6] + __popcll(s.keptmask[i >> 6] & ((1ull << (i & 63)) - 1));   // < total <= M
        const long long row = (long long)b * N + pos;
        const Head h = decode_row(a, b, an, r, nullptr, a.probs + row * a.C);
        float* o = a.rows + row * 8;
        o[0] = h.x, o[1] = h.y, o[2] = h.w, o[3] = h.h, o[4] = h.conf, o[5] = h.cmax, o[6] = (float)h.cid, o[7] = (float)n;
    }
}

int fill_args(const mcamd_detect_desc* d, const char* what, DetArgs* a) {
    MCAMD_REQUIRE(d && d->output, "%s: null argument", what);
    MCAMD_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->num_anchors > 0 && d->num_anchors <= 8 && d->num_classes > 0 &&
                      d->num_classes <= MAXC,
                  "%s: bad shape (B %d, %d x %d, %d anchors <= 8, %d classes <= %d)", what, d->B, d->H, d->W, d->num_anchors,
                  d->num_classes, MAXC);
    MCAMD_REQUIRE((long long)d->H * d->W * d->num_anchors <= MAXN, "%s: %lld rows per image, at most %d", what,
                  (long long)d->H * d->W * d->num_anchors, MAXN);
    a->out = d->output, a->head = nullptr, a->cls = nullptr, a->rows = nullptr, a->probs = nullptr, a->nkept = nullptr;
    a->B = d->B, a->A = d->num_anchors, a->C = d->num_classes, a->H = d->H, a->W = d->W;
    for (int n = 0; n < 8; ++n)
        a->aw[n] = n < d->num_anchors ? d->anchors[2 * n] : 1.f, a->ah[n] = n < d->num_anchors ? d->anchors[2 * n + 1] : 1.f;
    a->conf_thresh = d->conf_thresh, a->nms_thresh = d->nms_thresh;
    return MCAMD_OK;
}
}  // namespace

extern "C" int mcamd_region_decode(const mcamd_detect_desc* d, float* head, float* cls_conf, void* stream) {
    DetArgs a;
    if (int rc = fill_args(d, "region_decode", &a)) return rc;
    MCAMD_REQUIRE(head && cls_conf, "region_decode: null argument");
    a.head = head, a.cls = cls_conf;
    hipLaunchKernelGGL(region_decode_kernel, dim3(d->B), dim3(NTHR), 0, (hipStream_t)stream, a);
    MCAMD_LAUNCH_CHECK("region_decode");
    return MCAMD_OK;
}

extern "C" int mcamd_nms(const float* boxes, const float* conf, int32_t B, int32_t n, float nms_thresh, int32_t* order,
                         uint8_t* kept, void* stream) {
    MCAMD_REQUIRE(boxes && conf && order && kept, "nms: null argument");
    MCAMD_REQUIRE(B > 0 && n > 0, "nms: bad shape (B %d, n %d)", B, n);
    MCAMD_REQUIRE(n <= MAXN, "nms: %d boxes per image, at most %d", n, MAXN);
    MCAMD_REQUIRE(((uintptr_t)boxes & 15) == 0, "nms: boxes must be 16-byte aligned");
    hipLaunchKernelGGL(nms_kernel, dim3(B), dim3(NTHR), 0, (hipStream_t)stream, boxes, conf, n, nms_thresh, order, kept);
    MCAMD_LAUNCH_CHECK("nms");
    return MCAMD_OK;
}

extern "C" int mcamd_detect(const mcamd_detect_desc* d, float* rows, float* probs, int32_t* nkept, float* head_out,
                            float* cls_out, void* stream) {
    DetArgs a;
    if (int rc = fill_args(d, "detect", &a)) return rc;
    MCAMD_REQUIRE(rows && probs && nkept, "detect: null argument");
    a.rows = rows, a.probs = probs, a.nkept = nkept, a.head = head_out, a.cls = cls_out;
    hipLaunchKernelGGL(detect_kernel, dim3(d->B), dim3(NTHR), 0, (hipStream_t)stream, a);
    MCAMD_LAUNCH_CHECK("detect");
    return MCAMD_OK;
}
