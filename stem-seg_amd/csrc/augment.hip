// Geometric augmentation of a frame and its instance planes (the reference's data/image_to_seq_augmenter.py, which uses imgaug, and
// data/instance_duplicator.py, which uses cv2.warpAffine): the transforms stemseg_hip.h defines, one launch each.
//
// (1) warp_clip: one source image -> F warped frames, their instance planes and their invalid maps.  One thread per output pixel of
//     every frame: the source coordinate in unfused fp64 (a dozen operations against ~25 gathered bytes and the HSV round trip of each
//     tap), the image bilinear over the JITTERED taps with a zero border, the planes by the nearest source pixel -- the reference's
//     condense -> nearest warp -> expand without the intermediate map: the highest plane set there wins.
// (2) motion_blur: a k x k correlation (k odd, <= 11) per frame with a reflect-101 border; the 16 x 16 tile, its halo and the frame's
//     matrix are staged in LDS.
// (3) duplicate_instance: the shifted, optionally mirrored copy of a lone instance pasted into every frame.
// No atomics; every store is at the thread's own output index; every source index is checked before the read; every output byte is
// written.  All floating-point arithmetic goes through warp.h's helpers: nothing in this file is contracted into an FMA.
#include "common.h"
#include "warp.h"

#include <algorithm>

using namespace stemseg;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 16;                                    // motion blur: 16 x 16 output pixels per workgroup
constexpr int kMaxR = STEMSEG_BLUR_MAX_K / 2;
constexpr int kTileW = kTile + 2 * kMaxR;
constexpr int kTapStride = STEMSEG_BLUR_MAX_K * STEMSEG_BLUR_MAX_K;

struct BlurSizes { signed char k[STEMSEG_BLUR_MAX_FRAMES]; };          // a kernel argument: the host's checked values, no device copy

int grid_for(long long n, int cap) { return (int)std::max<long long>(1, std::min<long long>(ceil_div(n, kThreads), cap)); }

__global__ __launch_bounds__(kThreads) void warp_clip_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ planes, int N,
                                                             int H, int W, const double* __restrict__ hinv, const int* __restrict__ jitter, int F,
                                                             unsigned char* __restrict__ frames, unsigned char* __restrict__ out_planes,
                                                             unsigned char* __restrict__ invalid) {
    const long long HW = (long long)H * W, n = (long long)F * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int f = (int)(i / HW);
        const long long r = i - (long long)f * HW;
        const int y = (int)(r / W), x = (int)(r - (long long)y * W);
        const double* h = hinv + 9 * (long long)f;
        const int add = jitter[3 * f], hs = jitter[3 * f + 1], flags = jitter[3 * f + 2];
        const double xd = (double)x, yd = (double)y;
        const double d = dadd(dadd(dmul(h[6], xd), dmul(h[7], yd)), h[8]);
        float acc[3] = {0.f, 0.f, 0.f}, wsum = 0.f;
        int winner = -1;
        if (d > 1e-12) {
            const double u = ddiv(dadd(dadd(dmul(h[0], xd), dmul(h[1], yd)), h[2]), d);
            const double v = ddiv(dadd(dadd(dmul(h[3], xd), dmul(h[4], yd)), h[5]), d);
            if (u > -1.0 && u < (double)W && v > -1.0 && v < (double)H) {          // (false for a NaN: no tap can lie inside otherwise)
                const Taps4 t = make_taps4(u, v);
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int xt = t.x0 + b, yt = t.y0 + a;
                        const float w = fmul(t.wy[a], t.wx[b]);
                        if (xt >= 0 && xt < W && yt >= 0 && yt < H && w > 0.f) {
                            const unsigned char* p = src + ((long long)yt * W + xt) * 3;
                            const Bgr c = jitter_pixel(p[0], p[1], p[2], add, hs, flags);
                            acc[0] = fadd(acc[0], fmul(w, (float)c.b));
                            acc[1] = fadd(acc[1], fmul(w, (float)c.g));
                            acc[2] = fadd(acc[2], fmul(w, (float)c.r));
                            wsum = fadd(wsum, w);
                        }
                    }
                const int xn = (int)floor(dadd(u, 0.5)), yn = (int)floor(dadd(v, 0.5));
                if (xn >= 0 && xn < W && yn >= 0 && yn < H) {
                    const long long pix = (long long)yn * W + xn;
                    for (int q = N - 1; q >= 0; --q)
                        if (planes[(long long)q * HW + pix]) { winner = q; break; }
                }
            }
        }
        unsigned char* o = frames + i * 3;
        o[0] = (unsigned char)round_u8(acc[0]); o[1] = (unsigned char)round_u8(acc[1]); o[2] = (unsigned char)round_u8(acc[2]);
        invalid[i] = wsum < 0.5f ? 1 : 0;
        for (int q = 0; q < N; ++q) out_planes[((long long)q * F + f) * HW + r] = q == winner ? 1 : 0;
    }
}

// reflect-101 (gfedcb|abcdefgh|gfedcba) of an index at most n - 1 beyond either end; clamped, so that the positions only
// out-of-frame threads would use stay inside as well
__device__ __forceinline__ int reflect101(int i, int n) {
    i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// grid (ceil(W / 16), ceil(H / 16), F); the frame, so k, is the same for the whole workgroup
__global__ __launch_bounds__(kThreads) void motion_blur_kernel(const unsigned char* __restrict__ frames, int H, int W, BlurSizes ksize,
                                                               const float* __restrict__ taps, unsigned char* __restrict__ out) {
    __shared__ unsigned char tile[kTileW][kTileW * 3];
    __shared__ float wk[kTapStride];
    const int f = blockIdx.z, tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    const int x = blockIdx.x * kTile + tx, y = blockIdx.y * kTile + ty;
    const int k = ksize.k[f];                                               // (0, or odd and <= STEMSEG_BLUR_MAX_K: checked before the launch)
    const unsigned char* fr = frames + (long long)f * H * W * 3;
    unsigned char* o = out + (long long)f * H * W * 3;
    if (k == 0) {
        if (x < W && y < H) {
            const long long p = ((long long)y * W + x) * 3;
            o[p] = fr[p]; o[p + 1] = fr[p + 1]; o[p + 2] = fr[p + 2];
        }
        return;
    }
    const int R = k / 2, tw = kTile + 2 * R;
    for (int j = threadIdx.x; j < k * k; j += kThreads) wk[j] = taps[(long long)f * kTapStride + j];
    for (int j = threadIdx.x; j < tw * tw; j += kThreads) {
        const int jy = j / tw, jx = j - jy * tw;
        const int gy = reflect101(blockIdx.y * kTile + jy - R, H), gx = reflect101(blockIdx.x * kTile + jx - R, W);
        const unsigned char* p = fr + ((long long)gy * W + gx) * 3;
        tile[jy][jx * 3] = p[0]; tile[jy][jx * 3 + 1] = p[1]; tile[jy][jx * 3 + 2] = p[2];
    }
    __syncthreads();
    if (x < W && y < H) {
        float acc[3] = {0.f, 0.f, 0.f};
        for (int dy = 0; dy < k; ++dy)
            for (int dx = 0; dx < k; ++dx) {
                const float w = wk[dy * k + dx];
                const unsigned char* p = &tile[ty + dy][(tx + dx) * 3];
                acc[0] = fadd(acc[0], fmul(w, (float)p[0]));
                acc[1] = fadd(acc[1], fmul(w, (float)p[1]));
                acc[2] = fadd(acc[2], fmul(w, (float)p[2]));
            }
        const long long p = ((long long)y * W + x) * 3;
        o[p] = (unsigned char)round_u8(acc[0]); o[p + 1] = (unsigned char)round_u8(acc[1]); o[p + 2] = (unsigned char)round_u8(acc[2]);
    }
}

__global__ __launch_bounds__(kThreads) void duplicate_instance_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ mask,
                                                                      int T, int H, int W, const int* __restrict__ params,
                                                                      unsigned char* __restrict__ frames_out, unsigned char* __restrict__ masks_out) {
    const long long HW = (long long)H * W, n = (long long)T * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(i / HW);
        const long long r = i - (long long)t * HW;
        const int y = (int)(r / W), x = (int)(r - (long long)y * W);
        const int* p = params + 8 * (long long)t;
        const int has_box = p[0], xmin = p[1], ymin = p[2], xmax = p[3], ymax = p[4], flip = p[5];
        const unsigned char mv = mask[i];
        const unsigned char* px = frames + i * 3;
        unsigned char c0 = px[0], c1 = px[1], c2 = px[2], orig = mv, dup = mv;
        if (has_box) {
            const double u = dsub((double)x, (double)__int_as_float(p[6])), v = dsub((double)y, (double)__int_as_float(p[7]));     // (exact)
            float acc[3] = {0.f, 0.f, 0.f}, macc = 0.f;
            if (u > -1.0 && u < (double)W && v > -1.0 && v < (double)H) {
                const Taps4 tp = make_taps4(u, v);
                const unsigned char* fr = frames + (long long)t * HW * 3;
                const unsigned char* mk = mask + (long long)t * HW;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        int xt = tp.x0 + b;
                        const int yt = tp.y0 + a;
                        const float w = fmul(tp.wy[a], tp.wx[b]);
                        if (!(xt >= 0 && xt < W && yt >= 0 && yt < H && w > 0.f)) continue;
                        if (flip && xt >= xmin && xt < xmax && yt >= ymin && yt < ymax) {
                            xt = xmin + xmax - 1 - xt;
                            if (xt < 0 || xt >= W) continue;                 // (a box that leaves the frame: the tap reads nothing)
                        }
                        const long long pix = (long long)yt * W + xt;
                        const unsigned char* s = fr + pix * 3;
                        acc[0] = fadd(acc[0], fmul(w, (float)s[0]));
                        acc[1] = fadd(acc[1], fmul(w, (float)s[1]));
                        acc[2] = fadd(acc[2], fmul(w, (float)s[2]));
                        if (mk[pix]) macc = fadd(macc, w);
                    }
            }
            dup = macc >= 0.5f ? 1 : 0;                                      // floor(macc + 0.5) of a value in [0, 1]
            if (dup) {
                orig = 0;
                c0 = (unsigned char)round_u8(acc[0]); c1 = (unsigned char)round_u8(acc[1]); c2 = (unsigned char)round_u8(acc[2]);
            }
        }
        unsigned char* o = frames_out + i * 3;
        o[0] = c0; o[1] = c1; o[2] = c2;
        masks_out[i] = orig;
        masks_out[n + i] = dup;
    }
}

}  // namespace

extern "C" int stemseg_hip_warp_clip(const uint8_t* src, const uint8_t* planes, int32_t N, int32_t H, int32_t W, const double* hinv,
                                     const int32_t* jitter, int32_t F, uint8_t* frames, uint8_t* out_planes, uint8_t* invalid, void* stream) {
    SS_CHECK_ARG(N >= 0 && N <= STEMSEG_WARP_MAX_PLANES && H >= 1 && W >= 1 && F >= 1, "warp_clip: bad dims N=%d H=%d W=%d F=%d", N, H, W, F);
    SS_CHECK_ARG((long long)H * W < (1ll << 31), "warp_clip: a frame of %d x %d exceeds 2^31 pixels", H, W);
    SS_CHECK_ARG(src && hinv && jitter && frames && invalid && (N == 0 || (planes && out_planes)), "warp_clip: null pointer");
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(hinv) % 8 == 0 && reinterpret_cast<uintptr_t>(jitter) % 4 == 0,
                 "warp_clip: the homographies must be 8-byte aligned, the jitter table 4-byte aligned");
    hipLaunchKernelGGL(warp_clip_kernel, dim3(grid_for((long long)F * H * W, 8192)), dim3(kThreads), 0, as_stream(stream), src, planes, N, H, W, hinv,
                       jitter, F, frames, out_planes, invalid);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_motion_blur(const uint8_t* frames, int32_t F, int32_t H, int32_t W, const int32_t* ksize_host, const float* taps,
                                       uint8_t* out, void* stream) {
    SS_CHECK_ARG(F >= 1 && F <= STEMSEG_BLUR_MAX_FRAMES && H >= 1 && W >= 1, "motion_blur: bad dims F=%d (at most %d) H=%d W=%d", F,
                 STEMSEG_BLUR_MAX_FRAMES, H, W);
    SS_CHECK_ARG((long long)H * W < (1ll << 31), "motion_blur: a frame of %d x %d exceeds 2^31 pixels", H, W);
    SS_CHECK_ARG(frames && ksize_host && taps && out, "motion_blur: null pointer");
    SS_CHECK_ARG(out != frames, "motion_blur: the output must be another buffer (a pixel reads its neighbours)");
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(taps) % 4 == 0, "motion_blur: misaligned table");
    BlurSizes sizes;
    memset(&sizes, 0, sizeof(sizes));
    for (int f = 0; f < F; ++f) {
        const int k = ksize_host[f];
        SS_CHECK_ARG(k == 0 || (k > 0 && k <= STEMSEG_BLUR_MAX_K && (k & 1)), "motion_blur: frame %d has kernel size %d (0, or odd and at most %d)", f, k,
                     STEMSEG_BLUR_MAX_K);
        SS_CHECK_ARG(H > k / 2 && W > k / 2, "motion_blur: a %d x %d frame cannot be reflected under a %d x %d kernel", H, W, k, k);
        sizes.k[f] = (signed char)k;
    }
    SS_CHECK_ARG(ceil_div(H, kTile) <= 65535, "motion_blur: H=%d is too large", H);
    hipLaunchKernelGGL(motion_blur_kernel, dim3((unsigned)ceil_div(W, kTile), (unsigned)ceil_div(H, kTile), (unsigned)F), dim3(kThreads), 0,
                       as_stream(stream), frames, H, W, sizes, taps, out);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_duplicate_instance(const uint8_t* frames, const uint8_t* mask, int32_t T, int32_t H, int32_t W, const int32_t* params,
                                              uint8_t* frames_out, uint8_t* masks_out, void* stream) {
    SS_CHECK_ARG(T >= 1 && H >= 1 && W >= 1, "duplicate_instance: bad dims T=%d H=%d W=%d", T, H, W);
    SS_CHECK_ARG((long long)H * W < (1ll << 31), "duplicate_instance: a frame of %d x %d exceeds 2^31 pixels", H, W);
    SS_CHECK_ARG(frames && mask && params && frames_out && masks_out, "duplicate_instance: null pointer");
    SS_CHECK_ARG(frames_out != frames && masks_out != mask, "duplicate_instance: the outputs must be other buffers (a pixel reads its neighbours)");
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(params) % 4 == 0, "duplicate_instance: misaligned parameter table");
    hipLaunchKernelGGL(duplicate_instance_kernel, dim3(grid_for((long long)T * H * W, 8192)), dim3(kThreads), 0, as_stream(stream), frames, mask, T, H, W,
                       params, frames_out, masks_out);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
