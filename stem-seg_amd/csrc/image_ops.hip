// Image-space kernels either side of the path, both built on torch's bilinear rule.
//
// (1) Pre-processing (inference_image_loader.py:23-43 + data/common.py:12-30 + structures/image_list.py:93-104):
//     uint8 HWC frame -> bilinear resize -> (/255) -> (x - mean) / std -> (channel flip) -> zero pad to a multiple of 32.
// (2) Mask materialisation right after the stitched labels: the resampling chain shared by the
// reference's three writers (output_utils/davis.py:76-110, youtube_vis.py:118-155, kitti_mots.py:89-130), fused.
//   scatter:  per-point track labels -> dense uint8 map of "kept instance index + 1" at mask resolution
//   resample: one-hot -> bilinear x mask_scale -> crop the network's zero padding -> bilinear resize to the image size ->
//             > 0.5 -> condensed uint8 map, evaluated per output pixel from the <= 16 source pixels it depends on
//   (the *_ex entry points: the same kernels on a uint16 map, for more than 255 kept instances -- the argument below holds for any K)
// The bilinear weights of an output pixel sum to 1 and every source pixel carries ONE label, so at most one instance can
// exceed 0.5: the condensed map holds exactly the information of the reference's K binary planes.
#include "common.h"
#include "bilinear.h"

#include <algorithm>

using namespace stemseg;

namespace {

template <typename IdxT>
__global__ void mask_zero_kernel(IdxT* dense, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dense[i] = 0;
}

// IdxT = unsigned char (index values 1..255) or unsigned short (1..65535); the uint8 instantiation is the ABI <= 10 kernel
template <typename IdxT>
__global__ void mask_scatter_kernel(const long long* __restrict__ ys, const long long* __restrict__ xs, const long long* __restrict__ labels, long long n,
                                    const int* __restrict__ lut, int lut_len, IdxT* __restrict__ dense, int H, int W) {
    constexpr int kMaxV = sizeof(IdxT) == 1 ? 256 : 65536;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long y = ys[i], x = xs[i], l = labels[i] + 1;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        const int v = (l >= 0 && l < lut_len) ? lut[l] : 0;
        dense[y * W + x] = (IdxT)(v > 0 && v < kMaxV ? v : 0);
    }
}

template <typename IdxT>
__global__ __launch_bounds__(256) void mask_resample_kernel(const IdxT* __restrict__ dense, int h, int w, float up_scale, int up_h, int up_w,
                                                            int crop_h, int crop_w, float sy, float sx, int out_h, int out_w, IdxT* __restrict__ out) {
    const long long n = (long long)out_h * out_w;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int oy = (int)(i / out_w), ox = (int)(i - (long long)oy * out_w);
        // stage 5: cropped up-sampled planes (crop_h x crop_w) -> image size
        const Tap ty = make_tap(sy, oy, crop_h), tx = make_tap(sx, ox, crop_w);
        const int Y[2] = {ty.i0, ty.i1}, X[2] = {tx.i0, tx.i1};
        // stage 3: mask resolution (h x w) -> up-sampled (up_h x up_w); the four points the stage-5 sample reads
        Tap uy[2], ux[2];
        uy[0] = make_tap(up_scale, Y[0], h); uy[1] = make_tap(up_scale, Y[1], h);
        ux[0] = make_tap(up_scale, X[0], w); ux[1] = make_tap(up_scale, X[1], w);
        IdxT L[2][2][2][2];                              // [Y][X][y-tap][x-tap]
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int y0 = uy[a].i0, y1 = uy[a].i1, x0 = ux[b].i0, x1 = ux[b].i1;
                L[a][b][0][0] = dense[y0 * w + x0]; L[a][b][0][1] = dense[y0 * w + x1];
                L[a][b][1][0] = dense[y1 * w + x0]; L[a][b][1][1] = dense[y1 * w + x1];
            }
        const IdxT* flat = &L[0][0][0][0];
        IdxT result = 0;
        for (int k = 0; k < 16; ++k) {
            const IdxT cand = flat[k];
            if (cand == 0) continue;
            bool seen = false;
            for (int j = 0; j < k; ++j) seen = seen || (flat[j] == cand);
            if (seen) continue;
            float s[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    s[a][b] = lerp2(L[a][b][0][0] == cand ? 1.f : 0.f, L[a][b][0][1] == cand ? 1.f : 0.f,
                                    L[a][b][1][0] == cand ? 1.f : 0.f, L[a][b][1][1] == cand ? 1.f : 0.f, uy[a], ux[b]);
            const float v = lerp2(s[0][0], s[0][1], s[1][0], s[1][1], ty, tx);
            if (v > 0.5f && cand > result) result = cand;          // davis.py:104-107: later instances overwrite earlier ones
        }
        out[i] = result;
    }
}

// (/ 255) -> (x - mean) / std, unfused
__device__ __forceinline__ float normalise(float a, float mean, float stdv, int unit_scale) {
    if (unit_scale) a = __fdiv_rn(a, 255.f);
    return __fdiv_rn(__fsub_rn(a, mean), stdv);
}

// one thread per output pixel of the PADDED frame, all three channels (the 4 source pixels are 12 contiguous bytes pairs)
// kMasked (the image datasets' warped frames, coco_data_loader.py: normalise -> x (1 - invalid) -> resize): the bilinear sum of
// normalise(pixel) * (1 - invalid[pixel]); a pixel whose four taps are all valid takes the unmasked arithmetic, bit for bit
template <bool kMasked>
__global__ __launch_bounds__(256) void preprocess_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ invalid, int T, int H0,
                                                         int W0, int nh, int nw, int PH, int PW,
                                                         float sy, float sx, float m0, float m1, float m2, float s0, float s1, float s2,
                                                         int unit_scale, int flip, float* __restrict__ out) {
    const long long plane = (long long)PH * PW, n = (long long)T * plane;
    const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / plane);
        const long long r = i - (long long)t * plane;
        const int y = (int)(r / PW), x = (int)(r - (long long)y * PW);
        float v[3] = {0.f, 0.f, 0.f};
        if (y < nh && x < nw) {
            const Tap ty = make_tap(sy, y, H0), tx = make_tap(sx, x, W0);
            const unsigned char* f = frames + (long long)t * H0 * W0 * 3;
            const unsigned char* p00 = f + ((long long)ty.i0 * W0 + tx.i0) * 3;
            const unsigned char* p01 = f + ((long long)ty.i0 * W0 + tx.i1) * 3;
            const unsigned char* p10 = f + ((long long)ty.i1 * W0 + tx.i0) * 3;
            const unsigned char* p11 = f + ((long long)ty.i1 * W0 + tx.i1) * 3;
            bool any_invalid = false;
            float k00 = 1.f, k01 = 1.f, k10 = 1.f, k11 = 1.f;
            if (kMasked) {
                const unsigned char* iv = invalid + (long long)t * H0 * W0;
                k00 = iv[(long long)ty.i0 * W0 + tx.i0] ? 0.f : 1.f; k01 = iv[(long long)ty.i0 * W0 + tx.i1] ? 0.f : 1.f;
                k10 = iv[(long long)ty.i1 * W0 + tx.i0] ? 0.f : 1.f; k11 = iv[(long long)ty.i1 * W0 + tx.i1] ? 0.f : 1.f;
                any_invalid = k00 == 0.f || k01 == 0.f || k10 == 0.f || k11 == 0.f;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (kMasked && any_invalid) {
                    const float n00 = normalise((float)p00[c], mean[c], stdv[c], unit_scale), n01 = normalise((float)p01[c], mean[c], stdv[c], unit_scale);
                    const float n10 = normalise((float)p10[c], mean[c], stdv[c], unit_scale), n11 = normalise((float)p11[c], mean[c], stdv[c], unit_scale);
                    v[c] = lerp2(__fmul_rn(n00, k00), __fmul_rn(n01, k01), __fmul_rn(n10, k10), __fmul_rn(n11, k11), ty, tx);
                    continue;
                }
                const float a = lerp2((float)p00[c], (float)p01[c], (float)p10[c], (float)p11[c], ty, tx);
                v[c] = normalise(a, mean[c], stdv[c], unit_scale);
            }
        }
        float* o = out + (long long)t * 3 * plane + r;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(long long)(flip ? 2 - c : c) * plane] = v[c];
    }
}

int grid_for(long long n, int cap) { return (int)std::max<long long>(1, std::min<long long>(ceil_div(n, 256), cap)); }

template <typename IdxT>
int launch_scatter(const int64_t* ys, const int64_t* xs, const int64_t* labels, int64_t n, const int32_t* lut, int32_t lut_len, IdxT* dense,
                   int32_t H, int32_t W, void* stream) {
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(mask_zero_kernel<IdxT>, dim3(grid_for((long long)H * W, 2048)), dim3(256), 0, s, dense, (long long)H * W);
    if (n > 0)
        hipLaunchKernelGGL(mask_scatter_kernel<IdxT>, dim3(grid_for(n, 2048)), dim3(256), 0, s, reinterpret_cast<const long long*>(ys),
                           reinterpret_cast<const long long*>(xs), reinterpret_cast<const long long*>(labels), (long long)n, lut, lut_len, dense, H, W);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

template <typename IdxT>
int launch_resample(const IdxT* dense, int32_t h, int32_t w, float mask_scale, int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w,
                    IdxT* out, void* stream) {
    SS_CHECK_ARG(dense && out && h > 0 && w > 0 && out_h > 0 && out_w > 0 && mask_scale > 0.f, "resample_instance_masks: bad arguments");
    // F.interpolate(scale_factor=s): output size floor(in * s), coordinate scale 1 / s (UpSample.h compute_scales_value)
    const int up_h = (int)floorf((float)h * mask_scale), up_w = (int)floorf((float)w * mask_scale);
    SS_CHECK_ARG(crop_h >= 1 && crop_w >= 1 && crop_h <= up_h && crop_w <= up_w,
                 "resample_instance_masks: network input dims without padding (%d, %d) should be <= padded dims (%d, %d)", crop_w, crop_h, up_w, up_h);
    const float up_scale = (float)(1.0 / (double)mask_scale);
    const float sy = (float)crop_h / (float)out_h, sx = (float)crop_w / (float)out_w;   // size-driven resize: in / out
    hipLaunchKernelGGL(mask_resample_kernel<IdxT>, dim3(grid_for((long long)out_h * out_w, 4096)), dim3(256), 0, as_stream(stream), dense, h, w,
                       up_scale, up_h, up_w, crop_h, crop_w, sy, sx, out_h, out_w, out);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

}  // namespace

extern "C" int stemseg_hip_scatter_instance_index(const int64_t* ys, const int64_t* xs, const int64_t* labels, int64_t n, const int32_t* lut,
                                                  int32_t lut_len, uint8_t* dense, int32_t H, int32_t W, void* stream) {
    SS_CHECK_ARG(dense && H > 0 && W > 0 && n >= 0 && lut_len >= 0, "scatter_instance_index: bad arguments");
    SS_CHECK_ARG(n == 0 || (ys && xs && labels && lut), "scatter_instance_index: null pointer");
    return launch_scatter<unsigned char>(ys, xs, labels, n, lut, lut_len, dense, H, W, stream);
}

extern "C" int stemseg_hip_resample_instance_masks(const uint8_t* dense, int32_t h, int32_t w, float mask_scale, int32_t crop_h, int32_t crop_w,
                                                   int32_t out_h, int32_t out_w, uint8_t* out, void* stream) {
    return launch_resample<unsigned char>(dense, h, w, mask_scale, crop_h, crop_w, out_h, out_w, out, stream);
}

extern "C" int stemseg_hip_scatter_instance_index_ex(const int64_t* ys, const int64_t* xs, const int64_t* labels, int64_t n, const int32_t* lut,
                                                     int32_t lut_len, void* dense, int32_t index_bytes, int32_t H, int32_t W, void* stream) {
    SS_CHECK_ARG(index_bytes == 1 || index_bytes == 2, "scatter_instance_index_ex: index_bytes must be 1 or 2, got %d", index_bytes);
    SS_CHECK_ARG(dense && H > 0 && W > 0 && n >= 0 && lut_len >= 0, "scatter_instance_index_ex: bad arguments");
    SS_CHECK_ARG(n == 0 || (ys && xs && labels && lut), "scatter_instance_index_ex: null pointer");
    if (index_bytes == 1) return launch_scatter<unsigned char>(ys, xs, labels, n, lut, lut_len, static_cast<unsigned char*>(dense), H, W, stream);
    return launch_scatter<unsigned short>(ys, xs, labels, n, lut, lut_len, static_cast<unsigned short*>(dense), H, W, stream);
}

extern "C" int stemseg_hip_resample_instance_masks_ex(const void* dense, int32_t index_bytes, int32_t h, int32_t w, float mask_scale, int32_t crop_h,
                                                      int32_t crop_w, int32_t out_h, int32_t out_w, void* out, void* stream) {
    SS_CHECK_ARG(index_bytes == 1 || index_bytes == 2, "resample_instance_masks_ex: index_bytes must be 1 or 2, got %d", index_bytes);
    if (index_bytes == 1)
        return launch_resample<unsigned char>(static_cast<const unsigned char*>(dense), h, w, mask_scale, crop_h, crop_w, out_h, out_w,
                                              static_cast<unsigned char*>(out), stream);
    return launch_resample<unsigned short>(static_cast<const unsigned short*>(dense), h, w, mask_scale, crop_h, crop_w, out_h, out_w,
                                           static_cast<unsigned short*>(out), stream);
}

extern "C" int stemseg_hip_preprocess_frames(const uint8_t* frames, int32_t T, int32_t H0, int32_t W0, int32_t new_h, int32_t new_w,
                                             int32_t pad_h, int32_t pad_w, const float mean[3], const float std[3], int32_t unit_scale,
                                             int32_t flip_channels, float* out, void* stream) {
    SS_CHECK_ARG(frames && out && mean && std, "preprocess_frames: null pointer");
    SS_CHECK_ARG(T >= 1 && H0 >= 1 && W0 >= 1 && new_h >= 1 && new_w >= 1 && pad_h >= new_h && pad_w >= new_w,
                 "preprocess_frames: bad dims (%d, %d, %d) -> (%d, %d) padded (%d, %d)", T, H0, W0, new_h, new_w, pad_h, pad_w);
    SS_CHECK_ARG(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "preprocess_frames: zero std");
    const float sy = (float)H0 / (float)new_h, sx = (float)W0 / (float)new_w;       // size-driven bilinear: scale = in / out
    hipLaunchKernelGGL(preprocess_kernel<false>, dim3(grid_for((long long)T * pad_h * pad_w, 8192)), dim3(256), 0, as_stream(stream), frames, nullptr, T,
                       H0, W0, new_h, new_w, pad_h, pad_w, sy, sx, mean[0], mean[1], mean[2], std[0], std[1], std[2], unit_scale, flip_channels, out);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_preprocess_frames_masked(const uint8_t* frames, const uint8_t* invalid, int32_t T, int32_t H0, int32_t W0, int32_t new_h,
                                                    int32_t new_w, int32_t pad_h, int32_t pad_w, const float mean[3], const float std[3],
                                                    int32_t unit_scale, int32_t flip_channels, float* out, void* stream) {
    SS_CHECK_ARG(frames && invalid && out && mean && std, "preprocess_frames_masked: null pointer");
    SS_CHECK_ARG(T >= 1 && H0 >= 1 && W0 >= 1 && new_h >= 1 && new_w >= 1 && pad_h >= new_h && pad_w >= new_w,
                 "preprocess_frames_masked: bad dims (%d, %d, %d) -> (%d, %d) padded (%d, %d)", T, H0, W0, new_h, new_w, pad_h, pad_w);
    SS_CHECK_ARG(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "preprocess_frames_masked: zero std");
    const float sy = (float)H0 / (float)new_h, sx = (float)W0 / (float)new_w;
    hipLaunchKernelGGL(preprocess_kernel<true>, dim3(grid_for((long long)T * pad_h * pad_w, 8192)), dim3(256), 0, as_stream(stream), frames, invalid, T,
                       H0, W0, new_h, new_w, pad_h, pad_w, sy, sx, mean[0], mean[1], mean[2], std[0], std[1], std[2], unit_scale, flip_channels, out);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
