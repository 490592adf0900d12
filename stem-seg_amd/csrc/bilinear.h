// torch's bilinear rule (align_corners=False) in unfused fp32, shared by the image-space kernels (image_ops.hip) and the training
// data loader (data_loader.hip).
#pragma once
#include "common.h"

namespace stemseg {
namespace {

// torch's align_corners=False source coordinate (UpSample.h: area_pixel_compute_source_index + guard_index_and_lambda)
struct Tap { int i0, i1; float w0, w1; };
__device__ __forceinline__ Tap make_tap(float scale, int dst, int in_size) {
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    src = src < 0.f ? 0.f : src;
    int i0 = (int)src;
    i0 = i0 < in_size - 1 ? i0 : in_size - 1;
    float l1 = __fsub_rn(src, (float)i0);
    l1 = fminf(fmaxf(l1, 0.f), 1.f);
    Tap t;
    t.i0 = i0; t.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    t.w1 = l1; t.w0 = __fsub_rn(1.f, l1);
    return t;
}

// value = (v00*wx0 + v01*wx1)*wy0 + (v10*wx0 + v11*wx1)*wy1   (UpSampleKernel.cpp Interpolate<2>, unfused)
__device__ __forceinline__ float lerp2(float v00, float v01, float v10, float v11, const Tap& ty, const Tap& tx) {
    const float r0 = __fadd_rn(__fmul_rn(v00, tx.w0), __fmul_rn(v01, tx.w1));
    const float r1 = __fadd_rn(__fmul_rn(v10, tx.w0), __fmul_rn(v11, tx.w1));
    return __fadd_rn(__fmul_rn(r0, ty.w0), __fmul_rn(r1, ty.w1));
}

}  // namespace
}  // namespace stemseg
