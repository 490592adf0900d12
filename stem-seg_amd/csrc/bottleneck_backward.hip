// The streaming kernels of the bottleneck backward (hip.py bottleneck_backward / body_backward; the GEMMs are conv_backward.hip's weight gradients and
// the forward 1x1x1 kernel on transposed weights).  Maps are [C][F][H][W] over F independent frames.
//
//     relu_backward   out = (y <= 0) ? 0 : (g + addend)             torch's threshold_backward: a NaN activation lets the gradient through, +-0.0 blocks it.
//                                                                    y any view (dense, or the interior of the zero-haloed 2-D layout conv2 reads);
//                                                                    the addend is the residual join of an identity block: one pass for both
//     subsample2      [C][F][2h][2w] -> [C][F][h][w], even rows and columns: the input of a stride-2 1x1 convolution, and of its weight gradient
//     scatter2        its adjoint: out = addend + (even, even ? g : 0); at the other positions the addend's own bits (no + 0.0: -0.0 stays -0.0)
//     scale_rows      dw[co][...] *= s[co]: the gradient of a convolution's weight from that of the weight with FrozenBN folded in
//     sum_partials    out = sum over j of parts[j] (+ addend) in fp64, in order, rounded once: the K chunks of a wide 1x1 data gradient (hip.py conv1x1_dgrad:
//                     instead of one fp32 chain over 512 .. 2048 output channels in every block -- one of the two changes that brought the body's
//                     gradients inside the tests' bound)
//
// One thread per 4 consecutive elements of a row where the row length is a multiple of 4 and every pointer and stride keeps 16-byte alignment, one thread
// per element otherwise; grid-stride loops on 64-bit indices.  No floating-point atomics, no allocation, no synchronisation; every argument is checked
// before the launch.
#include "common.h"
#include <algorithm>

namespace stemseg {

constexpr int BB_MAX_BLOCKS = 256 * 16;

static inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
static inline unsigned bb_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, 256), BB_MAX_BLOCKS)); }

// ---- relu_backward.  VEC: 4 elements of a row per thread (g, addend, out as float4); VY: y as float4 too (a dense y; the interior of the haloed layout
// starts one float behind a 16-byte boundary and is read by element)
template <bool VEC, bool VY>
__global__ __launch_bounds__(256) void relu_backward_kernel(BBView y, const float* g, const float* addend, float* out, int F, int H, int W, int64_t items) {
    const int per = VEC ? 4 : 1, WQ = W / per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int xq = (int)(i % WQ);
        int64_t r = i / WQ;
        const int yy = (int)(r % H);
        r /= H;
        const int f = (int)(r % F);
        const int64_t c = r / F;
        const float* yp = y.ptr + c * y.cs + (int64_t)f * y.ts + (int64_t)yy * y.ys + xq * per;
        const int64_t o = i * per;
        if (VEC) {
            float4 yv;
            if (VY) yv = *reinterpret_cast<const float4*>(yp);
            else { yv.x = yp[0]; yv.y = yp[1]; yv.z = yp[2]; yv.w = yp[3]; }
            float4 v = *reinterpret_cast<const float4*>(g + o);
            if (addend) {
                const float4 a = *reinterpret_cast<const float4*>(addend + o);
                v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
            }
            v.x = relu_mask(yv.x, v.x); v.y = relu_mask(yv.y, v.y); v.z = relu_mask(yv.z, v.z); v.w = relu_mask(yv.w, v.w);
            *reinterpret_cast<float4*>(out + o) = v;
        } else {
            float v = g[o];
            if (addend) v += addend[o];
            out[o] = relu_mask(yp[0], v);
        }
    }
}

// ---- subsample2: planes = C F; out [planes][h][w] from in [planes][2h][2w].  VEC: 4 outputs from 8 consecutive inputs of an even row
template <bool VEC>
__global__ __launch_bounds__(256) void bb_subsample2_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, int64_t items) {
    const int per = VEC ? 4 : 1, WQ = w / per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int xq = (int)(i % WQ);
        int64_t r = i / WQ;
        const int y = (int)(r % h);
        const int64_t plane = r / h;
        const float* src = in + (plane * (2 * h) + 2 * y) * (int64_t)(2 * w) + 2 * xq * per;
        if (VEC) {
            const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
            *reinterpret_cast<float4*>(out + i * 4) = make_float4(a.x, a.z, b.x, b.z);
        } else {
            out[i] = src[0];
        }
    }
}

// ---- scatter2: out [planes][2h][2w].  VEC: 4 consecutive outputs of a row, two of them at even columns (2w % 4 == 0: w even, and g's pair is 8-byte aligned)
template <bool VEC>
__global__ __launch_bounds__(256) void bb_scatter2_kernel(const float* __restrict__ g, const float* __restrict__ addend, float* __restrict__ out, int h, int w,
                                                         int64_t items) {
    const int W = 2 * w, H = 2 * h, per = VEC ? 4 : 1, WQ = W / per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int X = (int)(i % WQ) * per;
        int64_t r = i / WQ;
        const int Y = (int)(r % H);
        const int64_t plane = r / H;
        const bool even_row = (Y & 1) == 0;
        const float* gp = g + (plane * h + (Y >> 1)) * (int64_t)w + (X >> 1);
        const int64_t o = i * per;
        if (VEC) {
            float4 v = addend ? *reinterpret_cast<const float4*>(addend + o) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (even_row) {
                const float2 gv = *reinterpret_cast<const float2*>(gp);
                v.x = addend ? v.x + gv.x : gv.x;
                v.z = addend ? v.z + gv.y : gv.y;
            }
            *reinterpret_cast<float4*>(out + o) = v;
        } else {
            float v = addend ? addend[o] : 0.f;
            if (even_row && (X & 1) == 0) v = addend ? v + gp[0] : gp[0];
            out[o] = v;
        }
    }
}

// ---- scale_rows: dw [rows][n] *= s[row]
template <bool VEC>
__global__ __launch_bounds__(256) void bb_scale_rows_kernel(float* __restrict__ dw, const float* __restrict__ s, int64_t n, int64_t items) {
    const int per = VEC ? 4 : 1;
    const int64_t NQ = n / per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const float sc = s[i / NQ];
        if (VEC) {
            float4 v = *reinterpret_cast<float4*>(dw + i * 4);
            v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
            *reinterpret_cast<float4*>(dw + i * 4) = v;
        } else {
            dw[i] *= sc;
        }
    }
}

// ---- sum_partials: parts [n][N]
template <bool VEC>
__global__ __launch_bounds__(256) void bb_sum_partials_kernel(const float* __restrict__ parts, int n, int64_t N, const float* __restrict__ addend,
                                                             float* __restrict__ out, int64_t items) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        if (VEC) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (int j = 0; j < n; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(parts + (int64_t)j * N + i * 4);
                a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
            }
            if (addend) {
                const float4 v = *reinterpret_cast<const float4*>(addend + i * 4);
                a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
            }
            *reinterpret_cast<float4*>(out + i * 4) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
        } else {
            double a = 0.0;
            for (int j = 0; j < n; ++j) a += (double)parts[(int64_t)j * N + i];
            if (addend) a += (double)addend[i];
            out[i] = (float)a;
        }
    }
}

static BBView bb_view(const StemsegVolume& v) { return BBView{v.ptr, v.c_stride, v.t_stride, v.y_stride}; }

}  // namespace stemseg

using namespace stemseg;

extern "C" int stemseg_hip_relu_backward(const StemsegVolume* y, const float* g, const float* addend, float* out, void* stream) {
    SS_CHECK_ARG(y && y->ptr, "relu_backward: y is a null pointer");
    SS_CHECK_ARG(g, "relu_backward: g is a null pointer");
    SS_CHECK_ARG(out, "relu_backward: out is a null pointer");
    const int rc = check_view("relu_backward", "y", *y);
    if (rc) return rc;
    const int64_t total = (int64_t)y->C * y->T * y->H * y->W;
    SS_CHECK_ARG(total < (1ll << 40), "relu_backward: y holds too many elements");
    const bool vec = y->W % 4 == 0 && aligned16(g) && aligned16(out) && (!addend || aligned16(addend));
    const bool vy = vec && aligned16(y->ptr) && y->c_stride % 4 == 0 && y->t_stride % 4 == 0 && y->y_stride % 4 == 0;
    const int64_t items = vec ? total / 4 : total;
    hipStream_t s = as_stream(stream);
    void* ev = profile_begin(56, 4.0 * (addend ? 4.0 : 3.0) * (double)total, s);
    const dim3 grid(bb_grid(items)), block(256);
    if (vy) hipLaunchKernelGGL((relu_backward_kernel<true, true>), grid, block, 0, s, bb_view(*y), g, addend, out, y->T, y->H, y->W, items);
    else if (vec) hipLaunchKernelGGL((relu_backward_kernel<true, false>), grid, block, 0, s, bb_view(*y), g, addend, out, y->T, y->H, y->W, items);
    else hipLaunchKernelGGL((relu_backward_kernel<false, false>), grid, block, 0, s, bb_view(*y), g, addend, out, y->T, y->H, y->W, items);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

// (H, W: the extents of the LARGE map of either call)
static int check_sub2(const char* who, int C, int F, int H, int W) {
    SS_CHECK_ARG(C > 0 && F > 0 && H > 0 && W > 0 && (int64_t)C * F * H * W < (1ll << 40), "%s: bad dims (C=%d, F=%d, H=%d, W=%d)", who, C, F, H, W);
    SS_CHECK_ARG(H % 2 == 0 && W % 2 == 0, "%s: H and W of the large map must be even, got H=%d, W=%d", who, H, W);
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_subsample2(const float* in, int32_t C, int32_t F, int32_t H, int32_t W, float* out, void* stream) {
    SS_CHECK_ARG(in, "subsample2: in is a null pointer");
    SS_CHECK_ARG(out, "subsample2: out is a null pointer");
    const int rc = check_sub2("subsample2", C, F, H, W);
    if (rc) return rc;
    const int h = H / 2, w = W / 2;
    const int64_t total = (int64_t)C * F * h * w;
    const bool vec = w % 4 == 0 && aligned16(in) && aligned16(out);
    const int64_t items = vec ? total / 4 : total;
    hipStream_t s = as_stream(stream);
    void* ev = profile_begin(58, 4.0 * 3.0 * (double)total, s);
    if (vec) hipLaunchKernelGGL(bb_subsample2_kernel<true>, dim3(bb_grid(items)), dim3(256), 0, s, in, out, h, w, items);
    else hipLaunchKernelGGL(bb_subsample2_kernel<false>, dim3(bb_grid(items)), dim3(256), 0, s, in, out, h, w, items);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_scatter2(const float* g, int32_t C, int32_t F, int32_t H, int32_t W, const float* addend, float* out, void* stream) {
    SS_CHECK_ARG(g, "scatter2: g is a null pointer");
    SS_CHECK_ARG(out, "scatter2: out is a null pointer");
    const int rc = check_sub2("scatter2", C, F, H, W);
    if (rc) return rc;
    const int h = H / 2, w = W / 2;
    const int64_t total = (int64_t)C * F * H * W;
    const bool vec = W % 4 == 0 && aligned16(out) && (!addend || aligned16(addend)) && reinterpret_cast<uintptr_t>(g) % 8 == 0;
    const int64_t items = vec ? total / 4 : total;
    hipStream_t s = as_stream(stream);
    void* ev = profile_begin(59, 4.0 * (addend ? 2.25 : 1.25) * (double)total, s);
    if (vec) hipLaunchKernelGGL(bb_scatter2_kernel<true>, dim3(bb_grid(items)), dim3(256), 0, s, g, addend, out, h, w, items);
    else hipLaunchKernelGGL(bb_scatter2_kernel<false>, dim3(bb_grid(items)), dim3(256), 0, s, g, addend, out, h, w, items);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_scale_rows(float* dw, const float* scale, int32_t rows, int64_t row_len, void* stream) {
    SS_CHECK_ARG(dw, "scale_rows: dw is a null pointer");
    SS_CHECK_ARG(scale, "scale_rows: scale is a null pointer");
    SS_CHECK_ARG(rows > 0, "scale_rows: rows must be positive, got %d", rows);
    SS_CHECK_ARG(row_len > 0 && (int64_t)rows * row_len < (1ll << 40), "scale_rows: bad row_len %lld", (long long)row_len);
    const int64_t total = (int64_t)rows * row_len;
    const bool vec = row_len % 4 == 0 && aligned16(dw);
    const int64_t items = vec ? total / 4 : total;
    hipStream_t s = as_stream(stream);
    void* ev = profile_begin(60, 4.0 * 2.0 * (double)total, s);
    if (vec) hipLaunchKernelGGL(bb_scale_rows_kernel<true>, dim3(bb_grid(items)), dim3(256), 0, s, dw, scale, row_len, items);
    else hipLaunchKernelGGL(bb_scale_rows_kernel<false>, dim3(bb_grid(items)), dim3(256), 0, s, dw, scale, row_len, items);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_sum_partials(const float* parts, int32_t n, int64_t N, const float* addend, float* out, void* stream) {
    SS_CHECK_ARG(parts, "sum_partials: parts is a null pointer");
    SS_CHECK_ARG(out, "sum_partials: out is a null pointer");
    SS_CHECK_ARG(n > 0 && n <= 4096, "sum_partials: n must be 1 .. 4096, got %d", n);
    SS_CHECK_ARG(N > 0 && (int64_t)n * N < (1ll << 40), "sum_partials: bad N %lld", (long long)N);
    const bool vec = N % 4 == 0 && aligned16(parts) && aligned16(out) && (!addend || aligned16(addend));
    const int64_t items = vec ? N / 4 : N;
    hipStream_t s = as_stream(stream);
    void* ev = profile_begin(61, 4.0 * (n + (addend ? 2.0 : 1.0)) * (double)N, s);
    if (vec) hipLaunchKernelGGL(bb_sum_partials_kernel<true>, dim3(bb_grid(items)), dim3(256), 0, s, parts, n, N, addend, out, items);
    else hipLaunchKernelGGL(bb_sum_partials_kernel<false>, dim3(bb_grid(items)), dim3(256), 0, s, parts, n, N, addend, out, items);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
