// The semseg cross-entropy and foreground losses (modeling/losses/cross_entropy.py:9-48, modeling/model_builder.py:210-244), their gradient
// with respect to the semseg head's output, and the preparation of the training targets (model_builder.py:128-152, data/common.py:195-210).
// One sample per call.
//
//   prepare_targets (1 launch): one thread per 1/4-scale voxel.  F.interpolate(scale_factor = 0.25, bilinear, align_corners = False) of a
//     0 / 1 mask followed by .byte() is the AND of the source pixels (4y + 1 | 4y + 2, 4x + 1 | 4x + 2): the sample point sits in their
//     middle, each weighs 1/4, and the cast truncates.  Output size floor(H / 4) x floor(W / 4), so the taps are never clamped.  The
//     semantic mask is the largest category id over the instances whose downscaled mask is set, 0 where none is.
//   forward (2 launches): per voxel the max-shifted log-sum-exp over the K class channels, lse - logit[target], and on the foreground
//     channel max(x, 0) - x y + log1p(exp(-|x|)) times non-ignore; fp64 per-workgroup sums of the fp32 terms in a fixed tree order, one
//     final kernel that adds the workgroups' sums in a fixed order too.  The per-voxel lse is kept for the backward pass (4 B / voxel).
//   backward (1 launch): one thread per voxel writes all K (+ 1) gradient elements of the voxel once, in the input's own strides.
// The logits are read where the decoder left them: [C][T][h][w] with element strides from the caller, so the reference's permuted
// [T][C][h][w] view of the same memory needs no copy.  No floating-point atomics: two runs give identical bits.
#include <algorithm>

#include "common.h"

namespace stemseg {
namespace {

constexpr int kLT = 256;                 // threads per workgroup
constexpr int kMaxWg = 1024;             // workgroups of the forward's grid-stride reduction (its partial sums: kMaxWg * 3 doubles)
constexpr int kMaxClasses = STEMSEG_MAX_SEMSEG_CLASSES;

struct Dims {
    int K, fg;                           // class channels; 1 when channel K is the foreground channel
    int T, H, W, nwg;
    long long P;
    long long sc, st, sh, sw;            // element strides of the logits and of the gradient
};

struct Ws {
    float* lse;                          // [P]
    double* part;                        // [nwg][3]: ce sum, fg sum, non-ignored voxels
    double* out;                         // [4]: the forward's result, which the backward's divisors come from
    size_t bytes;
};

Ws layout(const Dims& d, void* base) {
    Ws w;
    size_t off = 0;
    auto take = [&](size_t n) { void* q = base ? (char*)base + off : nullptr; off += (size_t)round_up((int64_t)n, 256); return q; };
    w.lse = (float*)take((size_t)d.P * 4);
    w.part = (double*)take((size_t)d.nwg * 3 * 8);
    w.out = (double*)take(4 * 8);
    w.bytes = off;
    return w;
}

// sum over the workgroup in a fixed tree order; every thread gets the result
__device__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int off = kLT / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    return sh[0];
}

__device__ __forceinline__ long long voxel_offset(const Dims& d, long long v) {
    const long long r = v / d.W;
    const int x = (int)(v - r * d.W), t = (int)(r / d.H), y = (int)(r - (long long)t * d.H);
    return t * d.st + y * d.sh + x * d.sw;
}

// ------------------------------------------------------------------------------------------------ targets
__global__ __launch_bounds__(kLT) void prepare_targets_kernel(int I, int T, int H, int W, int h, int w, const unsigned char* __restrict__ masks,
                                                              const unsigned char* __restrict__ ignore, const int* __restrict__ cat,
                                                              unsigned char* __restrict__ masks_out, unsigned char* __restrict__ ignore_out,
                                                              unsigned char* __restrict__ sem_out, int* __restrict__ flag) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < I; i += kLT)
            if (cat[i] < 0 || cat[i] > 255) *flag = 1;             // (every writer stores the same value)
    const long long p = (long long)T * h * w, v = (long long)blockIdx.x * kLT + threadIdx.x;
    if (v >= p) return;
    const long long r = v / w;
    const int x = (int)(v - r * w), t = (int)(r / h), y = (int)(r - (long long)t * h);
    // rows 4y + 1, 4y + 2 <= 4h - 2 <= H - 2 and columns likewise: inside the source for every H, W
    const long long src = ((long long)t * H + 4 * y + 1) * W + 4 * x + 1, full = (long long)T * H * W;
    auto tap = [&](const unsigned char* m) { return m[src] && m[src + 1] && m[src + W] && m[src + W + 1]; };
    ignore_out[v] = tap(ignore) ? 1 : 0;
    int sem = 0;
    for (int i = 0; i < I; ++i) {
        const bool on = tap(masks + (long long)i * full);
        masks_out[(long long)i * p + v] = on ? 1 : 0;
        const int c = cat[i];
        if (on && c > sem) sem = c;
    }
    sem_out[v] = (unsigned char)(sem > 255 ? 255 : sem);
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(kLT) void semseg_loss_partial_kernel(Dims d, const float* __restrict__ x, const unsigned char* __restrict__ sem,
                                                                  const unsigned char* __restrict__ ignore, float* __restrict__ lse,
                                                                  double* __restrict__ part, int* __restrict__ flag) {
    __shared__ double sh[kLT];
    double ce = 0.0, fgs = 0.0, cnt = 0.0;
    for (long long v = (long long)blockIdx.x * kLT + threadIdx.x; v < d.P; v += (long long)d.nwg * kLT) {
        const float* xv = x + voxel_offset(d, v);
        const int tgt = sem[v];
        if (d.K > 0) {
            float m = xv[0];
            for (int c = 1; c < d.K; ++c) m = fmaxf(m, xv[c * d.sc]);
            float s = 0.f;
            for (int c = 0; c < d.K; ++c) s += expf(xv[c * d.sc] - m);
            const float ls = logf(s);
            lse[v] = m + ls;
            if (tgt < d.K) ce += (double)(ls - (xv[tgt * d.sc] - m));
            else *flag = 1;                                        // (never indexed with: no read outside the K channels)
        }
        const float ni = ignore[v] ? 0.f : 1.f;
        cnt += (double)ni;
        if (d.fg) {
            const float xf = xv[d.K * d.sc], y = tgt > 0 ? 1.f : 0.f;
            const float bce = fmaxf(xf, 0.f) - xf * y + log1pf(expf(-fabsf(xf)));
            fgs += (double)(bce * ni);
        }
    }
    const double s0 = block_sum(ce, sh), s1 = block_sum(fgs, sh), s2 = block_sum(cnt, sh);
    if (threadIdx.x == 0) {
        double* o = part + (long long)blockIdx.x * 3;
        o[0] = s0;
        o[1] = s1;
        o[2] = s2;
    }
}

__global__ __launch_bounds__(kLT) void semseg_loss_final_kernel(Dims d, const double* __restrict__ part, double* __restrict__ out,
                                                                double* __restrict__ keep) {
    __shared__ double sh[kLT];
    double a[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < d.nwg; b += kLT)
        for (int f = 0; f < 3; ++f) a[f] += part[(long long)b * 3 + f];
    const double ce = block_sum(a[0], sh), fgs = block_sum(a[1], sh), cnt = block_sum(a[2], sh);
    if (threadIdx.x == 0) {
        const double r[4] = {ce, (double)d.P, fgs, cnt};
        for (int f = 0; f < 4; ++f) out[f] = keep[f] = r[f];
    }
}

// ------------------------------------------------------------------------------------------------ backward
// w_ce = upstream[0] / batch / voxels, w_fg = upstream[1] / batch / non-ignored voxels.  With every voxel ignored the reference divides
// 0 by 0 in both losses and autograd carries inf * 0 into every element of the sample's gradient: NaN, here too.
__global__ __launch_bounds__(kLT) void semseg_loss_backward_kernel(Dims d, const float* __restrict__ x, const unsigned char* __restrict__ sem,
                                                                   const unsigned char* __restrict__ ignore, const float* __restrict__ lse,
                                                                   const double* __restrict__ fwd, const float* __restrict__ up, double batch,
                                                                   float* __restrict__ grad) {
    const long long v = (long long)blockIdx.x * kLT + threadIdx.x;
    if (v >= d.P) return;
    const double cnt = fwd[3], nan = __longlong_as_double(0x7ff8000000000000ll);
    const float w_ce = (float)(cnt > 0.0 ? (double)up[0] / batch / fwd[1] : nan);
    const float w_fg = (float)(cnt > 0.0 ? (double)up[1] / batch / cnt : nan);
    const long long off = voxel_offset(d, v);
    const float* xv = x + off;
    float* gv = grad + off;
    const int tgt = sem[v];
    const float l = d.K > 0 ? lse[v] : 0.f;
    for (int c = 0; c < d.K; ++c) gv[c * d.sc] = (expf(xv[c * d.sc] - l) - (c == tgt ? 1.f : 0.f)) * w_ce;
    if (d.fg) {
        const float xf = xv[d.K * d.sc], y = tgt > 0 ? 1.f : 0.f, ni = ignore[v] ? 0.f : 1.f;
        gv[d.K * d.sc] = (1.f / (1.f + expf(-xf)) - y) * ni * w_fg;
    }
}

int make_dims(const StemsegSemsegLossDesc* desc, Dims* d, const char* who) {
    SS_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
    SS_CHECK_ARG(desc->struct_bytes == (int32_t)sizeof(StemsegSemsegLossDesc), "%s: descriptor size mismatch (%d vs %d): ABI skew", who,
                 desc->struct_bytes, (int)sizeof(StemsegSemsegLossDesc));
    SS_CHECK_ARG(desc->has_foreground_channel == 0 || desc->has_foreground_channel == 1, "%s: has_foreground_channel %d must be 0 or 1", who,
                 desc->has_foreground_channel);
    SS_CHECK_ARG((desc->n_classes >= 2 && desc->n_classes <= kMaxClasses) || (desc->n_classes == 0 && desc->has_foreground_channel),
                 "%s: n_classes %d outside 2..%d (0: the foreground channel alone)", who, desc->n_classes, kMaxClasses);
    SS_CHECK_ARG(desc->T >= 1 && desc->H >= 1 && desc->W >= 1, "%s: bad dims T %d H %d W %d", who, desc->T, desc->H, desc->W);
    const long long P = (long long)desc->T * desc->H * desc->W;
    SS_CHECK_ARG(P < (1ll << 31), "%s: T * H * W = %lld voxels, at most 2^31 - 1", who, P);
    SS_CHECK_ARG(desc->stride_c >= 1 && desc->stride_t >= 1 && desc->stride_h >= 1 && desc->stride_w >= 1,
                 "%s: bad strides c %lld t %lld h %lld w %lld (elements, positive)", who, (long long)desc->stride_c, (long long)desc->stride_t,
                 (long long)desc->stride_h, (long long)desc->stride_w);
    SS_CHECK_ARG(desc->reserved == 0 && desc->reserved2 == 0, "%s: reserved must be 0", who);
    d->K = desc->n_classes;
    d->fg = desc->has_foreground_channel;
    d->T = desc->T;
    d->H = desc->H;
    d->W = desc->W;
    d->P = P;
    d->nwg = (int)std::min<long long>(ceil_div(P, kLT), kMaxWg);
    d->sc = desc->stride_c;
    d->st = desc->stride_t;
    d->sh = desc->stride_h;
    d->sw = desc->stride_w;
    return STEMSEG_OK;
}

}  // namespace
}  // namespace stemseg

using namespace stemseg;

extern "C" int stemseg_hip_prepare_targets(const StemsegTargetPrepDesc* desc, const uint8_t* masks, const uint8_t* ignore_masks,
                                           const int32_t* category_ids, uint8_t* masks_out, uint8_t* ignore_out, uint8_t* semseg_out,
                                           int32_t* flag, void* stream) {
    SS_CHECK_ARG(desc != nullptr, "prepare_targets: null descriptor");
    SS_CHECK_ARG(desc->struct_bytes == (int32_t)sizeof(StemsegTargetPrepDesc), "prepare_targets: descriptor size mismatch (%d vs %d): ABI skew",
                 desc->struct_bytes, (int)sizeof(StemsegTargetPrepDesc));
    SS_CHECK_ARG(desc->n_instances >= 0 && desc->n_instances <= 1024, "prepare_targets: n_instances %d outside 0..1024", desc->n_instances);
    SS_CHECK_ARG(desc->T >= 1 && desc->H >= 4 && desc->W >= 4, "prepare_targets: bad dims T %d H %d W %d (H, W at least 4)", desc->T, desc->H,
                 desc->W);
    SS_CHECK_ARG((long long)desc->T * desc->H * desc->W < (1ll << 31), "prepare_targets: T * H * W = %lld voxels, at most 2^31 - 1",
                 (long long)desc->T * desc->H * desc->W);
    SS_CHECK_ARG(desc->reserved == 0, "prepare_targets: reserved must be 0");
    SS_CHECK_ARG(ignore_masks && ignore_out && semseg_out && flag, "prepare_targets: null pointer");
    SS_CHECK_ARG(desc->n_instances == 0 || (masks && category_ids && masks_out), "prepare_targets: null pointer (masks, category_ids or masks_out)");
    SS_CHECK_ARG(((uintptr_t)flag & 3) == 0 && ((uintptr_t)category_ids & 3) == 0, "prepare_targets: flag and category_ids must be 4-byte aligned");
    hipStream_t s = as_stream(stream);
    const int h = desc->H / 4, w = desc->W / 4;
    SS_HIP(hipMemsetAsync(flag, 0, 4, s));
    hipLaunchKernelGGL(prepare_targets_kernel, dim3((unsigned)ceil_div((long long)desc->T * h * w, kLT)), dim3(kLT), 0, s, desc->n_instances, desc->T,
                       desc->H, desc->W, h, w, masks, ignore_masks, category_ids, masks_out, ignore_out, semseg_out, flag);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" size_t stemseg_hip_semseg_loss_workspace_bytes(const StemsegSemsegLossDesc* desc) {
    Dims d;
    if (make_dims(desc, &d, "semseg_loss_workspace_bytes") != STEMSEG_OK) return 0;
    return layout(d, nullptr).bytes;
}

extern "C" int stemseg_hip_semseg_loss_forward(const StemsegSemsegLossDesc* desc, const float* logits, const uint8_t* semseg_mask,
                                               const uint8_t* ignore_mask, void* workspace, size_t ws_bytes, double* out, int32_t* flag,
                                               void* stream) {
    Dims d;
    if (int rc = make_dims(desc, &d, "semseg_loss_forward")) return rc;
    SS_CHECK_ARG(logits && semseg_mask && ignore_mask && workspace && out && flag, "semseg_loss_forward: null pointer");
    SS_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "semseg_loss_forward: workspace must be 256-byte aligned");
    SS_CHECK_ARG(((uintptr_t)logits & 3) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)flag & 3) == 0,
                 "semseg_loss_forward: logits and flag must be 4-byte aligned, out 8-byte aligned");
    const Ws w = layout(d, workspace);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "semseg_loss_forward: workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
    hipStream_t s = as_stream(stream);
    SS_HIP(hipMemsetAsync(flag, 0, 4, s));
    hipLaunchKernelGGL(semseg_loss_partial_kernel, dim3(d.nwg), dim3(kLT), 0, s, d, logits, semseg_mask, ignore_mask, w.lse, w.part, flag);
    hipLaunchKernelGGL(semseg_loss_final_kernel, dim3(1), dim3(kLT), 0, s, d, w.part, out, w.out);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_semseg_loss_backward(const StemsegSemsegLossDesc* desc, const float* logits, const uint8_t* semseg_mask,
                                                const uint8_t* ignore_mask, void* workspace, size_t ws_bytes, const float* upstream,
                                                int32_t batch_size, float* grad, void* stream) {
    Dims d;
    if (int rc = make_dims(desc, &d, "semseg_loss_backward")) return rc;
    SS_CHECK_ARG(logits && semseg_mask && ignore_mask && workspace && upstream && grad, "semseg_loss_backward: null pointer");
    SS_CHECK_ARG(batch_size >= 1, "semseg_loss_backward: batch_size %d must be positive", batch_size);
    SS_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "semseg_loss_backward: workspace must be 256-byte aligned");
    SS_CHECK_ARG(((uintptr_t)logits & 3) == 0 && ((uintptr_t)upstream & 3) == 0 && ((uintptr_t)grad & 3) == 0,
                 "semseg_loss_backward: logits, upstream and grad must be 4-byte aligned");
    const Ws w = layout(d, workspace);
    SS_CHECK_ARG(ws_bytes >= w.bytes, "semseg_loss_backward: workspace too small (%zu < %zu bytes)", ws_bytes, w.bytes);
    hipLaunchKernelGGL(semseg_loss_backward_kernel, dim3((unsigned)ceil_div(d.P, kLT)), dim3(kLT), 0, as_stream(stream), d, logits, semseg_mask,
                       ignore_mask, w.lse, w.out, upstream, (double)batch_size, grad);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
