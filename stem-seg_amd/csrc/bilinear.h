// torch's bilinear rule (align_corners=False) in fp32, shared by the image-space kernels (image_ops.hip) and the training data loader
// (data_loader.hip).
// The roundings are spelled out: a fused multiply-add exactly where `fmaf` is written, one rounding per operator everywhere else (the
// compiler's own contraction is switched off inside each function).  The source index is ONE fma, as in torch's own kernels: the tests
// that hold these kernels to F.interpolate within 1e-4 need it (rounding the product first moves the result by up to 8e-4 on noise).
// HIP's __fmul_rn / __fadd_rn / __fsub_rn do not pin any of this down -- they are plain operators in an inline function of the header
// and are contracted like any other -- so they are not used here.  tests/image_ops_oracle.py restates these functions bit for bit.
#pragma once
#include "common.h"

namespace stemseg {
namespace {

// torch's align_corners=False source coordinate (UpSample.h: area_pixel_compute_source_index + guard_index_and_lambda)
struct Tap { int i0, i1; float w0, w1; };
__device__ __forceinline__ Tap make_tap(float scale, int dst, int in_size) {
#pragma clang fp contract(off)
    float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
    src = src < 0.f ? 0.f : src;
    int i0 = (int)src;
    i0 = i0 < in_size - 1 ? i0 : in_size - 1;
    float l1 = src - (float)i0;
    l1 = fminf(fmaxf(l1, 0.f), 1.f);
    Tap t;
    t.i0 = i0; t.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    t.w1 = l1; t.w0 = 1.f - l1;
    return t;
}

// value = (v00*wx0 + v01*wx1)*wy0 + (v10*wx0 + v11*wx1)*wy1   (UpSampleKernel.cpp Interpolate<2>); in each sum the second product is
// rounded and the first is fused into the addition
__device__ __forceinline__ float lerp2(float v00, float v01, float v10, float v11, const Tap& ty, const Tap& tx) {
#pragma clang fp contract(off)
    const float r0 = fmaf(v00, tx.w0, v01 * tx.w1);
    const float r1 = fmaf(v10, tx.w0, v11 * tx.w1);
    return fmaf(r0, ty.w0, r1 * ty.w1);
}

}  // namespace
}  // namespace stemseg
