// Training augmentation of the reference's VOC loader (src/dataloader.py:148-178 + ToTensor()) for gfx950:
// crop -> Pillow bicubic resize -> flip -> Pillow HSV distortion -> u8 / 255.f, bit-equal to the PIL chain.
//
// Compiled with -ffp-contract=off: the HSV conversions restate Pillow's Convert.c float / double arithmetic
// operation by operation, and a contracted FMA would change a rounding.
//
// Two launches per batch (include/mcamd.h):
//   augment_hpass_kernel  crop + horizontal resampling pass, uint8 RGBX rows into the workspace (Pillow rounds and
//                         clips to uint8 between its two passes, so the intermediate is uint8 by definition);
//   augment_vpass_kernel  vertical pass + flip + RGB->HSV -> LUTs -> HSV->RGB, one coalesced fp32 store per channel.
// The resampling tables and LUTs come from the host (modelcompression_amd/augment.py) or from
//   augment_tables_kernel  augment.resample_table and augment.point_luts restated in float64, operation by operation,
//                          one block per (image, axis) and one per image's LUTs (mcamd_augment_tables);
// the pixel kernels clamp every table entry to the crop, so a corrupt table can give wrong pixels but never an
// out-of-bounds access.  A descriptor with lut_off == -1 has no HSV step: the resampled pixel is stored as u8 / 255.f
// (Image.resize + ToTensor(), the evaluation loader).
#include "common.h"

namespace {

constexpr int NTHR = 256;
constexpr int HROWS = 8;     // workspace rows per horizontal-pass block (a thread keeps its column's table row)
constexpr int PREC = 22;     // Pillow's PRECISION_BITS for 8-bit images

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> PREC, 0), 255); }

// The workspace holds one 32-bit word per pixel, R | G << 8 | B << 16 (Pillow's own 4-byte RGB layout): one coalesced
// store per pixel here and one load per tap in the vertical pass, instead of three byte accesses each.
__global__ __launch_bounds__(NTHR) void augment_hpass_kernel(const mcamd_augment_desc* __restrict__ descs,
                                                             const uint8_t* __restrict__ src,
                                                             const int32_t* __restrict__ coef, uint32_t* __restrict__ tmp,
                                                             int W) {
    const mcamd_augment_desc d = descs[blockIdx.z];
    const int r0 = blockIdx.y * HROWS;
    const int x = blockIdx.x * NTHR + threadIdx.x;
    if (r0 >= d.crop_h || x >= W) return;
    const int r1 = min(r0 + HROWS, d.crop_h);
    const int32_t* k = coef + d.hcoef_off + (long long)x * (d.hk + 2);
    const int first = min(max(k[0], 0), d.crop_w);
    const int cnt = min(max(k[1], 0), min(d.hk, d.crop_w - first));
    const uint8_t* s = src + d.src_off;
    uint32_t* t = tmp + d.tmp_off / 4;
    for (int r = r0; r < r1; ++r) {
        int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
        const int sy = d.crop_y + r;
        if (sy >= 0 && sy < d.src_h) {          // rows outside the source are black (PIL's crop)
            const uint8_t* row = s + (long long)sy * d.src_w * 3;
            // branch-free taps: a column outside the source reads column 0 with weight 0
#pragma unroll 8
            for (int j = 0; j < cnt; ++j) {
                const int sx = d.crop_x + first + j;
                const bool in = (unsigned)sx < (unsigned)d.src_w;
                const uint8_t* p = row + (in ? sx : 0) * 3;
                const int c = in ? k[2 + j] : 0;
                a0 += (int)p[0] * c, a1 += (int)p[1] * c, a2 += (int)p[2] * c;
            }
        }
        t[(long long)r * W + x] = (uint32_t)clip8(a0) | (uint32_t)clip8(a1) << 8 | (uint32_t)clip8(a2) << 16;
    }
}

// Pillow Convert.c rgb2hsv_row: float arithmetic where Pillow has floats, double where its constants promote.
__device__ __forceinline__ void rgb2hsv(int r, int g, int b, int& uh, int& us, int& uv) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    uv = maxc;
    if (minc == maxc) {
        uh = 0, us = 0;
        return;
    }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc)
        h = bc - gc;
    else if (g == maxc)
        h = (float)(2.0 + (double)rc - (double)bc);
    else
        h = (float)(4.0 + (double)gc - (double)rc);
    const double hd = (double)h / 6.0 + 1.0;      // in [5/6, 11/6): fmod(hd, 1.0) is exactly this subtraction
    h = (float)(hd >= 1.0 ? hd - 1.0 : hd);
    uh = min(max((int)((double)h * 255.0), 0), 255);
    us = min(max((int)((double)s * 255.0), 0), 255);
}

// Pillow Convert.c hsv2rgb (fs * f is a float product there; the other products promote to double).
__device__ __forceinline__ void hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
    if (s == 0) {
        r = g = b = v;
        return;
    }
    const double hf = (double)(float)h * 6.0 / 255.0;
    const int i = (int)floor(hf);
    const float f = (float)(hf - (double)(float)i);
    const float fs = (float)((double)(float)s / 255.0);
    const double vv = (double)(float)v;
    const int p = min(max((int)round(vv * (1.0 - (double)fs)), 0), 255);
    const int q = min(max((int)round(vv * (1.0 - (double)(fs * f))), 0), 255);
    const int t = min(max((int)round(vv * (1.0 - (double)fs * (1.0 - (double)f))), 0), 255);
    switch (i % 6) {
        case 0: r = v, g = t, b = p; break;
        case 1: r = q, g = v, b = p; break;
        case 2: r = p, g = v, b = t; break;
        case 3: r = p, g = q, b = v; break;
        case 4: r = t, g = p, b = v; break;
        default: r = v, g = p, b = q; break;
    }
}

// One block per (output row, image): the row's vertical table is block-uniform (scalar loads).
__global__ __launch_bounds__(NTHR) void augment_vpass_kernel(const mcamd_augment_desc* __restrict__ descs,
                                                             const int32_t* __restrict__ coef,
                                                             const uint8_t* __restrict__ lut,
                                                             const uint32_t* __restrict__ tmp, float* __restrict__ out,
                                                             int H, int W) {
    __shared__ uint8_t L[768];
    const int b = blockIdx.y, y = blockIdx.x;
    const mcamd_augment_desc d = descs[b];
    const bool distort = d.lut_off >= 0;         // block-uniform: one block per (row, image)
    if (distort) {
        for (int i = threadIdx.x; i < 768; i += NTHR) L[i] = lut[d.lut_off + i];
        __syncthreads();
    }
    const int32_t* k = coef + d.vcoef_off + (long long)y * (d.vk + 2);
    const int first = min(max(k[0], 0), d.crop_h);
    const int cnt = min(max(k[1], 0), min(d.vk, d.crop_h - first));
    const uint32_t* col0 = tmp + d.tmp_off / 4 + (long long)first * W;
    const long long plane = (long long)H * W;
    float* o = out + (long long)b * 3 * plane + (long long)y * W;
    for (int x = threadIdx.x; x < W; x += NTHR) {
        const uint32_t* col = col0 + (d.flip ? W - 1 - x : x);
        int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
#pragma unroll 8
        for (int j = 0; j < cnt; ++j) {
            const uint32_t p = col[(long long)j * W];
            const int c = k[2 + j];
            a0 += (int)(p & 255) * c, a1 += (int)((p >> 8) & 255) * c, a2 += (int)((p >> 16) & 255) * c;
        }
        int r = clip8(a0), g = clip8(a1), bl = clip8(a2);
        if (distort) {
            int h, s, v;
            rgb2hsv(r, g, bl, h, s, v);
            hsv2rgb(L[h], L[256 + s], L[512 + v], r, g, bl);
        }
        o[x] = (float)r / 255.0f;
        o[plane + x] = (float)g / 255.0f;
        o[2 * plane + x] = (float)bl / 255.0f;
    }
}

constexpr int MAX_DIM = 1 << 16;
constexpr int MAX_TAPS = 4096;

// Pillow's bicubic_filter (a = -0.5) as augment._bicubic writes it.
__device__ __forceinline__ double bicubic(double x) {
    x = fabs(x);
    if (x < 1.0) return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * -0.5;
    return 0.0;
}

// augment.resample_table(n_in, n_out) into n_out rows of (first, count, k[0..ksize)), one thread per row.
__device__ void resample_table(int n_in, int n_out, int ksize, int32_t* __restrict__ t) {
    if (n_in == n_out) {                          // the pass Pillow skips: ksize is 1 (validated on the host)
        for (int o = threadIdx.x; o < n_out; o += NTHR) {
            int32_t* row = t + (long long)o * 3;
            row[0] = o, row[1] = 1, row[2] = 1 << PREC;
        }
        return;
    }
    const double scale = (double)(float)n_in / n_out;
    const double filterscale = fmax(scale, 1.0);
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    for (int o = threadIdx.x; o < n_out; o += NTHR) {
        const double center = 0.0 + (o + 0.5) * scale;
        const long long xmin = (long long)fmax(trunc(center - support + 0.5), 0.0);
        const long long xmax = min((long long)trunc(center + support + 0.5), (long long)n_in) - xmin;
        double ww = 0.0;                           // the row sum, in tap order
        for (int j = 0; j < ksize; ++j)
            ww = ww + (j < xmax ? bicubic((((double)(j + xmin) - center) + 0.5) * ss) : 0.0);
        int32_t* row = t + (long long)o * (ksize + 2);
        row[0] = (int32_t)xmin, row[1] = (int32_t)xmax;
        for (int j = 0; j < ksize; ++j) {
            double w = j < xmax ? bicubic((((double)(j + xmin) - center) + 0.5) * ss) : 0.0;
            if (ww != 0.0) w = w / ww;
            row[2 + j] = (int32_t)(w < 0 ? trunc(-0.5 + w * (double)(1 << PREC)) : trunc(0.5 + w * (double)(1 << PREC)));
        }
    }
}

// blockIdx.x: 0 the horizontal table, 1 the vertical table, 2 augment.point_luts(dhue, dsat, dexp); blockIdx.y: image.
__global__ __launch_bounds__(NTHR) void augment_tables_kernel(const mcamd_augment_desc* __restrict__ descs,
                                                              const double* __restrict__ hsv, int32_t* __restrict__ coef,
                                                              uint8_t* __restrict__ lut, int H, int W) {
    const int b = blockIdx.y;
    const mcamd_augment_desc d = descs[b];
    if (blockIdx.x == 0) {
        resample_table(d.crop_w, W, d.hk, coef + d.hcoef_off);
    } else if (blockIdx.x == 1) {
        resample_table(d.crop_h, H, d.vk, coef + d.vcoef_off);
    } else if (d.lut_off >= 0) {
        const double dhue = hsv[3 * b], dsat = hsv[3 * b + 1], dexp = hsv[3 * b + 2];
        for (int n = threadIdx.x; n < 256; n += NTHR) {
            const double i = (double)n;
            double h = i + dhue * 255;
            if (h > 255) h = h - 255;             // change_hue wraps at 255, not 256
            if (h < 0) h = h + 255;
            const double v[3] = {h, i * dsat, i * dexp};
            for (int c = 0; c < 3; ++c)            // Python's round: half to even
                lut[d.lut_off + 256 * c + n] = (uint8_t)fmin(fmax(rint(v[c]), 0.0), 255.0);
        }
    }
}

// ksize of augment.resample_table(n_in, n_out)
int table_taps(int n_in, int n_out) {
    if (n_in == n_out) return 1;
    return (int)ceil(2.0 * fmax((double)(float)n_in / n_out, 1.0)) * 2 + 1;
}

}  // namespace

extern "C" int mcamd_augment(const mcamd_augment_batch* a, void* stream) {
    MCAMD_REQUIRE(a && a->desc && a->desc_dev && a->src && a->coef && a->tmp && a->out, "augment: null argument");
    MCAMD_REQUIRE(!mcamd_recording(), "augment: not recordable into a launch plan");
    MCAMD_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->H <= MAX_DIM && a->W <= MAX_DIM && a->B <= 65535 &&
                      ((uintptr_t)a->tmp & 3) == 0,
                  "augment: bad batch shape (B %d, %d x %d)", a->B, a->H, a->W);
    MCAMD_REQUIRE(a->src_bytes >= 0 && a->coef_elems >= 0 && a->lut_bytes >= 0 && a->tmp_bytes >= 0,
                  "augment: negative buffer size");
    int max_rows = 0;
    for (int b = 0; b < a->B; ++b) {
        const mcamd_augment_desc& d = a->desc[b];
        MCAMD_REQUIRE(d.src_w > 0 && d.src_h > 0 && d.src_w <= MAX_DIM && d.src_h <= MAX_DIM,
                      "augment: image %d: bad source size %d x %d", b, d.src_w, d.src_h);
        MCAMD_REQUIRE(d.crop_w >= 1 && d.crop_h >= 1,
                      "augment: image %d: empty crop (%d x %d); the reference makes an image of no pixels there", b,
                      d.crop_w, d.crop_h);
        MCAMD_REQUIRE(d.crop_w <= MAX_DIM && d.crop_h <= MAX_DIM && d.crop_x > -MAX_DIM && d.crop_x < MAX_DIM &&
                          d.crop_y > -MAX_DIM && d.crop_y < MAX_DIM,
                      "augment: image %d: crop (%d, %d) %d x %d out of range", b, d.crop_x, d.crop_y, d.crop_w, d.crop_h);
        MCAMD_REQUIRE(d.src_off >= 0 && d.src_off + (int64_t)d.src_w * d.src_h * 3 <= a->src_bytes,
                      "augment: image %d: source outside src (%lld bytes)", b, (long long)a->src_bytes);
        MCAMD_REQUIRE(d.tmp_off >= 0 && d.tmp_off % 4 == 0 && d.tmp_off + (int64_t)d.crop_h * a->W * 4 <= a->tmp_bytes,
                      "augment: image %d: workspace rows outside tmp (%lld bytes)", b, (long long)a->tmp_bytes);
        MCAMD_REQUIRE(d.hk >= 1 && d.hk <= MAX_TAPS && d.vk >= 1 && d.vk <= MAX_TAPS,
                      "augment: image %d: bad tap counts %d, %d", b, d.hk, d.vk);
        MCAMD_REQUIRE(d.hcoef_off >= 0 && d.hcoef_off + (int64_t)a->W * (d.hk + 2) <= a->coef_elems &&
                          d.vcoef_off >= 0 && d.vcoef_off + (int64_t)a->H * (d.vk + 2) <= a->coef_elems,
                      "augment: image %d: resampling table outside coef (%lld entries)", b, (long long)a->coef_elems);
        // lut_off == -1: no HSV distortion for this image (and no LUTs: lut may then be NULL)
        MCAMD_REQUIRE(d.lut_off == -1 || (d.lut_off >= 0 && a->lut && d.lut_off + 768 <= a->lut_bytes),
                      "augment: image %d: LUTs outside lut (lut_off %d)", b, d.lut_off);
        max_rows = max(max_rows, d.crop_h);
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(augment_hpass_kernel, dim3((a->W + NTHR - 1) / NTHR, (max_rows + HROWS - 1) / HROWS, a->B), dim3(NTHR),
                       0, st, a->desc_dev, a->src, a->coef, (uint32_t*)a->tmp, a->W);
    hipLaunchKernelGGL(augment_vpass_kernel, dim3(a->H, a->B), dim3(NTHR), 0, st, a->desc_dev, a->coef, a->lut,
                       (const uint32_t*)a->tmp, a->out, a->H, a->W);
    MCAMD_LAUNCH_CHECK("augment");
    return MCAMD_OK;
}

extern "C" int mcamd_augment_tables(const mcamd_augment_desc* desc_host, const mcamd_augment_desc* desc_dev,
                                    const double* hsv_dev, int32_t B, int32_t H, int32_t W, int32_t* coef,
                                    int64_t coef_elems, uint8_t* lut, int64_t lut_bytes, void* stream) {
    MCAMD_REQUIRE(desc_host && desc_dev && coef, "augment_tables: null argument");
    MCAMD_REQUIRE(!mcamd_recording(), "augment_tables: not recordable into a launch plan");
    MCAMD_REQUIRE(B > 0 && H > 0 && W > 0 && H <= MAX_DIM && W <= MAX_DIM && B <= 65535,
                  "augment_tables: bad batch shape (B %d, %d x %d)", B, H, W);
    MCAMD_REQUIRE(coef_elems >= 0 && lut_bytes >= 0, "augment_tables: negative buffer size");
    for (int b = 0; b < B; ++b) {
        const mcamd_augment_desc& d = desc_host[b];
        MCAMD_REQUIRE(d.crop_w >= 1 && d.crop_h >= 1, "augment_tables: image %d: empty crop (%d x %d)", b, d.crop_w, d.crop_h);
        MCAMD_REQUIRE(d.crop_w <= MAX_DIM && d.crop_h <= MAX_DIM, "augment_tables: image %d: crop %d x %d out of range", b,
                      d.crop_w, d.crop_h);
        const int hk = table_taps(d.crop_w, W), vk = table_taps(d.crop_h, H);
        MCAMD_REQUIRE(d.hk == hk && d.vk == vk && hk <= MAX_TAPS && vk <= MAX_TAPS,
                      "augment_tables: image %d: tap counts %d, %d, the tables of %d -> %d and %d -> %d have %d, %d", b, d.hk,
                      d.vk, d.crop_w, W, d.crop_h, H, hk, vk);
        MCAMD_REQUIRE(d.hcoef_off >= 0 && d.hcoef_off + (int64_t)W * (hk + 2) <= coef_elems && d.vcoef_off >= 0 &&
                          d.vcoef_off + (int64_t)H * (vk + 2) <= coef_elems,
                      "augment_tables: image %d: resampling table outside coef (%lld entries)", b, (long long)coef_elems);
        MCAMD_REQUIRE(d.lut_off == -1 || (d.lut_off >= 0 && lut && hsv_dev && d.lut_off + 768 <= lut_bytes),
                      "augment_tables: image %d: LUTs outside lut, or no hsv / lut buffer (lut_off %d)", b, d.lut_off);
    }
    hipLaunchKernelGGL(augment_tables_kernel, dim3(3, B), dim3(NTHR), 0, (hipStream_t)stream, desc_dev, hsv_dev, coef, lut,
                       H, W);
    MCAMD_LAUNCH_CHECK("augment_tables");
    return MCAMD_OK;
}
