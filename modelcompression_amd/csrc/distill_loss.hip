// Objectness-scaled distillation of a YOLOv2 head against a frozen teacher (include/mcamd.h, mcamd_distill_desc) as ONE pass
// over the two logit tensors: loss and d(loss)/d(student) together, shaped like region_loss.hip.
//   q = sig(t4)                          the teacher's objectness weighs the box and class terms, and is never differentiated
//   L = 1/B sum_n [ obj/2 (sig(s4) - q)^2 + q ( box/2 ((sig(s0) - sig(t0))^2 + (sig(s1) - sig(t1))^2 + (s2 - t2)^2 + (s3 - t3)^2)
//                                              + cls tau^2 sum_c pt_c (log pt_c - log ps_c) ) ]
//   dL/ds0 = q box (sig(s0) - sig(t0)) sig(s0) sig(-s0) / B      dL/ds2 = q box (s2 - t2) / B
//   dL/ds4 = obj (sig(s4) - q) sig(s4) sig(-s4) / B              dL/ds(5+c) = q cls tau (ps_c - pt_c) / B
// The sigmoid's derivative is sig(s) sig(-s): 1 - sig(s) is 0 in fp32 from s = 17 on.  Both log-softmaxes come from the same
// two device functions below (running maximum and sum, then log p = (z - max) - log(sum), p = exp(log p)), so a teacher
// class that underflows to pt = 0 keeps a finite log pt and adds exactly 0, and bit-equal operands give differences that are
// exactly 0 everywhere.  1 / B is the last factor of every gradient element.
// One workgroup per (image, anchor), threads walking the H * W cells: consecutive lanes read consecutive floats of every
// channel plane.  The class planes are walked twice (sum, then probabilities): the second walk is expected to find the
// workgroup's own 2 * C * H * W floats (27 KB at 13x13, C = 20) in cache, so that HBM sees every logit once -- expected from
// the footprint, not measured with counters; nothing is staged through LDS (no reuse across lanes).
// Deterministic: a fixed tree inside the workgroup, per-(image, anchor) partial sums, added by a second one-block launch
// in a fixed order.  No atomics.
#include "common.h"

namespace {
constexpr int NTHR = 256;

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// running maximum m and sum s of exp(z - m) over the classes seen so far (m = -inf, s = 0 before the first)
__device__ __forceinline__ void lse_update(float& m, float& s, float z) {
    const float d = z - m, e = expf(-fabsf(d));
    s = d > 0.f ? s * e + 1.0f : s + e;
    m = fmaxf(m, z);
}
// log softmax of one class from the finished maximum and log(sum)
__device__ __forceinline__ float log_prob(float z, float m, float log_s) { return (z - m) - log_s; }
}  // namespace

struct DistillArgs {
    const float* s;       // [B][A*(5+C)][H][W] student logits
    const float* t;       // same shape, teacher logits
    float* grad;          // same shape
    float* partial;       // [B*A] per-(image, anchor) loss (already / B)
    int B, A, C, H, W;
    float obj_scale, box_scale, cls_scale, tau;
};

__global__ __launch_bounds__(NTHR) void distill_loss_kernel(DistillArgs a) {
    __shared__ float red[NTHR];
    const int b = blockIdx.x, an = blockIdx.y, tid = threadIdx.x;
    const int HW = a.H * a.W, K = 5 + a.C;
    const float inv_b = 1.0f / (float)a.B, tau = a.tau;
    float lsum = 0.f;
    for (int r = tid; r < HW; r += NTHR) {
        const long long base = ((long long)b * a.A + an) * K * HW + r;
        const float* s = a.s + base;
        const float* t = a.t + base;
        float* g = a.grad + base;
        const float s0 = s[0], s1 = s[HW], s2 = s[2 * (long long)HW], s3 = s[3 * (long long)HW], s4 = s[4 * (long long)HW];
        const float t0 = t[0], t1 = t[HW], t2 = t[2 * (long long)HW], t3 = t[3 * (long long)HW], t4 = t[4 * (long long)HW];
        const float q = sigmoidf_(t4);
        const float xs = sigmoidf_(s0), ys = sigmoidf_(s1), cs = sigmoidf_(s4);
        const float d0 = xs - sigmoidf_(t0), d1 = ys - sigmoidf_(t1), d2 = s2 - t2, d3 = s3 - t3, dc = cs - q;
        const float qb = q * a.box_scale, qc = q * a.cls_scale;
        g[0] = qb * d0 * (xs * sigmoidf_(-s0)) * inv_b;
        g[HW] = qb * d1 * (ys * sigmoidf_(-s1)) * inv_b;
        g[2 * (long long)HW] = qb * d2 * inv_b;
        g[3 * (long long)HW] = qb * d3 * inv_b;
        g[4 * (long long)HW] = a.obj_scale * dc * (cs * sigmoidf_(-s4)) * inv_b;
        const float lo = 0.5f * dc * dc, lb = 0.5f * (d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3);
        // a sigmoid maps an infinite logit to a finite 0 or 1: v - v is 0 for a finite v and NaN otherwise, so the loss
        // is non-finite for those too (every other term carries an Inf or NaN through by itself)
        const float finite = (s0 - s0) + (s1 - s1) + (s4 - s4) + (t0 - t0) + (t1 - t1) + (t4 - t4);

        float ms = -INFINITY, ss = 0.f, mt = -INFINITY, st = 0.f;
        for (int c = 0; c < a.C; ++c) {
            lse_update(ms, ss, s[(5 + c) * (long long)HW] / tau);
            lse_update(mt, st, t[(5 + c) * (long long)HW] / tau);
        }
        const float lss = logf(ss), lst = logf(st);
        float kl = 0.f;
        for (int c = 0; c < a.C; ++c) {
            const float lps = log_prob(s[(5 + c) * (long long)HW] / tau, ms, lss);
            const float lpt = log_prob(t[(5 + c) * (long long)HW] / tau, mt, lst);
            const float ps = expf(lps), pt = expf(lpt);
            kl += pt * (lpt - lps);
            g[(5 + c) * (long long)HW] = qc * tau * (ps - pt) * inv_b;
        }
        lsum += a.obj_scale * lo + q * (a.box_scale * lb + a.cls_scale * (tau * tau * kl)) + finite;
    }
    red[tid] = lsum;
    __syncthreads();
    for (int o = NTHR / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) a.partial[b * a.A + an] = red[0] * inv_b;
}

// partial[0..n) in a fixed order: thread i adds elements i, i + 256, ... in index order, then the same tree as above
__global__ __launch_bounds__(256) void distill_loss_sum_kernel(const float* partial, int n, float* loss) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = red[0];
}

extern "C" size_t mcamd_distill_loss_workspace_bytes(int32_t B, int32_t num_anchors) {
    return (size_t)(B > 0 ? B : 1) * (size_t)(num_anchors > 0 ? num_anchors : 1) * sizeof(float);
}

extern "C" int mcamd_distill_loss(const mcamd_distill_desc* d, float* loss, float* grad, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    MCAMD_REQUIRE(d && d->student && d->teacher && loss && grad && workspace, "distill_loss: null argument");
    MCAMD_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->num_anchors > 0 && d->num_anchors <= 8 && d->num_classes > 0,
                  "distill_loss: bad shape (B %d, %d x %d, %d anchors <= 8, %d classes)", d->B, d->H, d->W, d->num_anchors,
                  d->num_classes);
    MCAMD_REQUIRE((long long)d->H * d->W <= (1 << 30), "distill_loss: bad shape (%d x %d cells: too many)", d->H, d->W);
    MCAMD_REQUIRE(d->temperature > 0.f && d->temperature <= 3.0e38f, "distill_loss: temperature %g must be positive and finite",
                  (double)d->temperature);
    MCAMD_REQUIRE(workspace_bytes >= mcamd_distill_loss_workspace_bytes(d->B, d->num_anchors),
                  "distill_loss: workspace %zu < %zu bytes", workspace_bytes,
                  mcamd_distill_loss_workspace_bytes(d->B, d->num_anchors));
    DistillArgs a;
    a.s = d->student, a.t = d->teacher, a.grad = grad, a.partial = (float*)workspace;
    a.B = d->B, a.A = d->num_anchors, a.C = d->num_classes, a.H = d->H, a.W = d->W;
    a.obj_scale = d->obj_scale, a.box_scale = d->box_scale, a.cls_scale = d->cls_scale, a.tau = d->temperature;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(distill_loss_kernel, dim3(d->B, d->num_anchors), dim3(NTHR), 0, st, a);
    hipLaunchKernelGGL(distill_loss_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, d->B * d->num_anchors, loss);
    MCAMD_LAUNCH_CHECK("distill_loss");
    return MCAMD_OK;
}
