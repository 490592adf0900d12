// 2-D encoder (ResNet-50/101 + FPN) on the same fp32-MFMA implicit-GEMM core as the decoder.
//
// Reference: /root/reference/stemseg/modeling/backbone/resnet.py:105-113 (ResNet.forward), :263-282 (Bottleneck,
// stride in the first 1x1), :292-304 (stem + max-pool), fpn.py:47-69 (FPN.forward), make_layers.py:51-63
// (FrozenBatchNorm2d, folded into weight/bias by the host once), model_builder.py:154-169 (run_backbone).
//
// MI355X-first choices
//   * a clip's T frames are the T axis of one [C][T][H][W] volume, so every 2-D convolution is the decoder's conv
//     kernel with KT = 1 and the FPN outputs land directly in the [C][T][h][w] (optionally zero-haloed) layout the 3-D
//     decoders consume -- no per-frame launches, no torch.stack, no pad copy;
//   * bias (= folded BN shift), ReLU and the residual add live in the conv epilogue: a bottleneck block is 3 (4 with a
//     projection shortcut) launches instead of conv + BN + ReLU + add chains;
//   * 1x1 convs run on the flat [C][V] view (aligned 16-B rows regardless of W); when their consumer is a 3x3 conv the
//     epilogue decodes the voxel index and writes the interior of a zero-haloed 2-D layout [C][T][h+2][pitch];
//   * stride-2 1x1 convs (first block of layers 2-4, conv1 and the shortcut) read one shared 2x-subsampled copy;
//   * layers with few voxels (layer3/4: 12 960 / 3 240 voxels) use the conv kernel's split-K to fill 256 CUs.
#include "common.h"
#include <algorithm>
#include <cstddef>

namespace stemseg {

// zero-haloed 2-D layout: [C][T][H+2][pitch], halo only in H and W
struct Padded2D {
    int64_t pitch, ts, cs, total, interior;
    Padded2D() = default;
    Padded2D(int C, int T, int H, int W) {
        pitch = round_up((int64_t)W + 2, 4);
        ts = (int64_t)(H + 2) * pitch;
        cs = (int64_t)T * ts;
        total = (int64_t)C * cs + 64;
        interior = pitch + 1;
    }
};
static inline StemsegVolume halo2d_view(float* base, int C, int T, int H, int W) {
    Padded2D g(C, T, H, W);
    return make_volume(base, g.cs, g.ts, g.pitch, C, T, H + 2, W + 2, g.total);
}
static inline StemsegVolume interior2d_view(float* base, int C, int T, int H, int W) {
    Padded2D g(C, T, H, W);
    return make_volume(base + g.interior, g.cs, g.ts, g.pitch, C, T, H, W, g.total - g.interior);
}
static inline StemsegVolume flat_view(float* base, int C, int64_t V) { return make_volume(base, V, 0, 0, C, 1, 1, (int)V, (int64_t)C * V); }

// stem tile: 8 x 64 output pixels of one frame, all 64 channels
constexpr int ST_ROWS = 8, ST_COLS = 64, ST_PR = 2 * ST_ROWS + 5, ST_PC = 2 * ST_COLS + 5;

// ---- stem on the matrix cores: the 7x7 stride-2 convolution (3 -> 64, + bias + ReLU) as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32
// products, fp32 accumulation).  M = 64 output channels, N = 8 rows x 64 columns of outputs per workgroup, K = 3 x 7 x 8 taps (the
// eighth column tap is zero padding): an MFMA consumes TWO taps per issue -- lane half 0 an even dx, lane half 1 the odd dx next to
// it -- so the input patch is staged DE-INTERLEAVED by column parity: plane p holds the input columns x = 2 i + p, and tap
// (c, dy, dx = 2 q + p) of output column ox is plane[p][c][2 oy + dy][ox + q]: consecutive lanes read consecutive LDS words and
// every tap is a compile-time immediate on one per-lane base (stride-2 reads of an interleaved patch would be 2-way bank
// conflicts).  Four waves; wave w owns output rows 2w, 2w + 1 (four 32-column blocks) x both 32-channel halves: 8 accumulator
// tiles, 6 LDS reads per 8 MFMAs.  (Through round 3 the stem was a VALU kernel -- the step's only VALU-bound one, and the only kernel
// whose results were not bit-stable under concurrently replaying graphs; this form is also 1.5x faster.)
constexpr int SM_PW = 68, SM_ROWS_IN = 2 * ST_ROWS + 6;          // plane row pitch (words); staged input rows (one spare for nothing: 21 used)
constexpr int SM_PLANE = 3 * SM_ROWS_IN * SM_PW;                  // words per parity plane
constexpr int SM_KSTEPS = 3 * 7 * 4;                              // (c, dy, q): two taps each
typedef float f32x16s __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256, 2) void stem_conv7x7_mfma_kernel(const float* __restrict__ frames, const float* __restrict__ w_tap_major,
                                                                 const float* __restrict__ bias, float* __restrict__ out, int T, int H, int W) {
    __shared__ __attribute__((aligned(16))) float lds[2 * SM_PLANE + SM_KSTEPS * 2 * 64];
    float* const planes = lds;
    float* const wl = lds + 2 * SM_PLANE;
    const int Ho = H / 2, Wo = W / 2;
    const int tiles_x = (Wo + ST_COLS - 1) / ST_COLS, tiles_y = (Ho + ST_ROWS - 1) / ST_ROWS;
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y;
    const int t = b / tiles_y;
    const int oy0 = ty * ST_ROWS, ox0 = tx * ST_COLS;
    const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
    // weights: [step = (c * 7 + dy) * 4 + q][half][64] <- w_tap_major[(c * 7 + dy) * 7 + 2 q + half][64], zero for dx = 7
    for (int i = threadIdx.x; i < SM_KSTEPS * 2 * 64; i += 256) {
        const int co = i & 63, half = (i >> 6) & 1, step = i >> 7;
        const int q = step & 3, cdy = step >> 2, dx = 2 * q + half;
        wl[i] = dx < 7 ? w_tap_major[(cdy * 7 + dx) * 64 + co] : 0.f;
    }
    // input patch, 21 rows x 133 columns per channel, split by column parity (columns beyond 133 and the spare rows: zero)
    for (int i = threadIdx.x; i < 2 * SM_PLANE; i += 256) {
        const int par = i / SM_PLANE, r = i - par * SM_PLANE;
        const int xi = r % SM_PW, yy = (r / SM_PW) % SM_ROWS_IN, c = r / (SM_PW * SM_ROWS_IN);
        const int iy = iy0 + yy, ix = ix0 + 2 * xi + par;
        float v = 0.f;
        if (yy < ST_PR && 2 * xi + par < ST_PC && iy >= 0 && iy < H && ix >= 0 && ix < W) v = frames[(((int64_t)t * 3 + c) * H + iy) * W + ix];
        planes[i] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    f32x16s acc[2][4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    const float* a_ptr = wl + half * 64 + l31;
    const float* b_ptr[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) b_ptr[ni] = planes + half * SM_PLANE + (2 * (2 * wave + (ni >> 1))) * SM_PW + (ni & 1) * 32 + l31;
    auto ld = [&](const int step, float (&a)[2], float (&bv)[4]) __attribute__((always_inline)) {
        const int q = step & 3, cdy = step >> 2, c = cdy / 7, dy = cdy - 7 * c;
        const int boff = (c * SM_ROWS_IN + dy) * SM_PW + q;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) a[mi] = a_ptr[step * 128 + mi * 32];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) bv[ni] = b_ptr[ni][boff];
    };
    auto mm = [&](const float (&a)[2], const float (&bv)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    };
    // software pipeline over the k-steps (operands of step i + 1 requested before the MFMAs of step i issue)
    float a0[2], b0[4], a1[2], b1[4];
    ld(0, a0, b0);
#pragma unroll
    for (int i = 0; i < SM_KSTEPS; i += 2) {
        ld(i + 1, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mm(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (i + 2 < SM_KSTEPS) ld(i + 2, a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        mm(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
    }
    // epilogue: C/D layout col = lane & 31 (output column), row = (r & 3) + 8 * (r >> 2) + 4 * half (channel)
    const int64_t plane = (int64_t)Ho * Wo;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int oy = oy0 + 2 * wave + (ni >> 1), ox = ox0 + (ni & 1) * 32 + l31;
        if (oy < Ho && ox < Wo) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    out[((int64_t)ch * T + t) * plane + (int64_t)oy * Wo + ox] = relu_keep_nan(acc[mi][ni][r] + bias[ch]);
                }
        }
    }
}

// ---- the stem in f16x3 mode: space-to-depth, then a stride-1 4x4 convolution on the split-staged MFMA kernel (conv_igemm.h, Y4Stem).
// out[oy][ox] = sum w[c][ky][kx] in[c][2 oy + ky - 3][2 ox + kx - 3]; with ky + 1 = 2 a + p, kx + 1 = 2 b + q (a, b in 0..3, p, q in 0..1; the
// index 0 is a zero tap) the input index is 2 (oy - 2 + a) + p: a 4x4 convolution over S[(p, q, c)][Y][X] = in[c][2 Y + p][2 X + q] with two
// halo positions before and one after.  12 channels (one 16-channel chunk), K = 16 taps x 16 = 256 per output in three fp16 products:
// 3/8 of the matrix time of the exact fp32-MFMA stem (84 steps of K = 2), which the default mode no longer needs: every other convolution of
// the mode carries 22-bit operands as well.  One thread = one input pixel pair (q = 0, 1) of one (t, c, row).
__global__ __launch_bounds__(256) void stem_s2d_kernel(const float* __restrict__ frames, float* __restrict__ s2d, int T, int H, int W, int64_t ts, int pitch) {
    const int W2 = W / 2, H2 = H / 2;
    const int64_t total = (int64_t)T * 3 * H * W2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int X = (int)(i % W2);
        int64_t r = i / W2;
        const int y = (int)(r % H);
        r /= H;
        const int c = (int)(r % 3), t = (int)(r / 3);
        const float2 v = *reinterpret_cast<const float2*>(frames + (((int64_t)t * 3 + c) * H + y) * W + 2 * X);
        const int p = y & 1, Y = y >> 1;
        (void)H2;
        float* o = s2d + ((int64_t)((p * 2 + 0) * 3 + c) * T + t) * ts + (int64_t)(Y + 2) * pitch + X + 2;
        o[0] = v.x;
        o[(int64_t)3 * T * ts] = v.y;                          // q = 1: three channels further
    }
}

// max-pool 3x3 stride 2 pad 1 over every [c][t] plane (resnet.py:303)
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t planes, int H, int W) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t total = planes * Ho * Wo;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo);
        int64_t r = i / Wo;
        const int y = (int)(r % Ho);
        const int64_t pl = r / Ho;
        const float* p = in + pl * H * W;
        float m = -INFINITY;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = 2 * y + dy;
            if (yy < 0 || yy >= H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = 2 * x + dx;
                if (xx < 0 || xx >= W) continue;
                m = max_keep_nan(m, p[(int64_t)yy * W + xx]);
            }
        }
        out[i] = m;
    }
}

// 16-B forms (W % 8 == 0, aligned planes): one thread = 4 consecutive outputs of one row; 32-bit index arithmetic (n_items =
// output rows over all planes x float4 pieces per row).
__global__ __launch_bounds__(256) void maxpool3x3s2_vec4_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, unsigned n_items) {
    const int Ho = H / 2, Wo = W / 2;
    const unsigned wq = Wo / 4, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n_items) return;
    const unsigned row = idx / wq;                         // plane * Ho + y
    const int j = (int)(idx - row * wq);
    const unsigned pl = row / (unsigned)Ho, y = row - pl * (unsigned)Ho;
    const float* p = in + (size_t)pl * H * W;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = 2 * (int)y + dy;
        if (yy < 0 || yy >= H) continue;
        const float* r = p + (size_t)yy * W + 8 * j;       // inputs 8j-1 .. 8j+7 feed outputs 4j .. 4j+3
        const float4 a = *reinterpret_cast<const float4*>(r), b = *reinterpret_cast<const float4*>(r + 4);
        const float left = j > 0 ? r[-1] : -INFINITY;
        m[0] = max_keep_nan(m[0], max_keep_nan(left, max_keep_nan(a.x, a.y)));
        m[1] = max_keep_nan(m[1], max_keep_nan(a.y, max_keep_nan(a.z, a.w)));
        m[2] = max_keep_nan(m[2], max_keep_nan(a.w, max_keep_nan(b.x, b.y)));
        m[3] = max_keep_nan(m[3], max_keep_nan(b.y, max_keep_nan(b.z, b.w)));
    }
    *reinterpret_cast<float4*>(out + (size_t)row * Wo + 4 * j) = make_float4(m[0], m[1], m[2], m[3]);
}
__global__ __launch_bounds__(256) void subsample2_vec4_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, unsigned n_items) {
    const int Ho = H / 2, Wo = W / 2;
    const unsigned wq = Wo / 4, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n_items) return;
    const unsigned row = idx / wq;
    const int j = (int)(idx - row * wq);
    const unsigned pl = row / (unsigned)Ho, y = row - pl * (unsigned)Ho;
    const float* r = in + (size_t)pl * H * W + (size_t)(2 * y) * W + 8 * j;
    const float4 a = *reinterpret_cast<const float4*>(r), b = *reinterpret_cast<const float4*>(r + 4);
    *reinterpret_cast<float4*>(out + (size_t)row * Wo + 4 * j) = make_float4(a.x, a.z, b.x, b.z);
}

// out[pl][y][x] = in[pl][2y][2x]   (shared input of a stride-2 block's conv1 and projection shortcut)
__global__ __launch_bounds__(256) void subsample2_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t planes, int H, int W) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t total = planes * Ho * Wo;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo);
        int64_t r = i / Wo;
        const int y = (int)(r % Ho);
        const int64_t pl = r / Ho;
        out[i] = in[pl * H * W + (int64_t)(2 * y) * W + 2 * x];
    }
}

// The bilinear blend of the FPN top-down path with its rounding steps spelled out -- fma(1 - wx, c[x0], wx c[x1]) per coarse row, then
// fma(1 - wy, row0, wy row1): what the compiler's contraction made of the plain expression, fixed here so that the three forms below agree by
// construction, not by the optimiser's choice (the two-row form shares the row blends between two outputs: a value with two uses contracts
// differently).
__device__ __forceinline__ float up2_blend(const float c00, const float c01, const float c10, const float c11, const float wx, const float wy) {
    const float h0 = __fmaf_rn(1.f - wx, c00, __fmul_rn(wx, c01));
    const float h1 = __fmaf_rn(1.f - wx, c10, __fmul_rn(wx, c11));
    return __fmaf_rn(1.f - wy, h0, __fmul_rn(wy, h1));
}

// FPN top-down path (fpn.py:64-66): fine += bilinear_x2(coarse), both zero-haloed 2-D layouts, align_corners = False
__global__ __launch_bounds__(256) void upsample2x_add_kernel(float* __restrict__ fine, const float* __restrict__ coarse, int64_t planes, int H, int W,
                                                              int64_t f_ts, int64_t f_pitch, int64_t c_ts, int64_t c_pitch) {
    const int Hc = H / 2, Wc = W / 2;
    const int64_t total = planes * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        int64_t r = i / W;
        const int y = (int)(r % H);
        const int64_t pl = r / H;
        float sy = 0.5f * ((float)y + 0.5f) - 0.5f, sx = 0.5f * ((float)x + 0.5f) - 0.5f;
        sy = sy < 0.f ? 0.f : sy;
        sx = sx < 0.f ? 0.f : sx;
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < Hc - 1 ? 1 : 0), x1 = x0 + (x0 < Wc - 1 ? 1 : 0);
        const float wy = sy - (float)y0, wx = sx - (float)x0;
        const float* c = coarse + pl * c_ts;
        const float v = up2_blend(c[y0 * c_pitch + x0], c[y0 * c_pitch + x1], c[y1 * c_pitch + x0], c[y1 * c_pitch + x1], wx, wy);
        float* fo = fine + pl * f_ts + (int64_t)y * f_pitch + x;
        *fo = __fadd_rn(*fo, v);
    }
}

// 16-B form: one thread = one ALIGNED group of four columns of the zero-haloed fine rows (haloed columns 4k .. 4k + 3 = map columns 4k - 1 .. 4k + 2:
// the interior starts at haloed column 1, so aligned groups straddle it by one), TWO fine rows per thread.  A fine row is read and written as one
// float4 (a halo word in the group is written back unchanged).  Rows 2m - 1 and 2m interpolate between the SAME coarse rows (m - 1, m), and the four
// columns of the group between coarse columns 2k - 1, 2k, 2k + 1 (clamped exactly as the scalar form clamps them): six coarse loads, two 16-byte loads
// and two 16-byte stores for eight outputs.  m = 0 holds row 0 alone (its row - 1 does not exist), m = Hc row H - 1 alone.  Every output goes through
// up2_blend with the (x0, x1, wx) / (y0, y1, wy) the scalar form computes for it -- for even H and W these are exact quarters: x = 2n + 1 -> (n, .25),
// x = 2n + 2 -> (n, .75), x = 0 -> (0, 0), clamped at the far edge -- so the bits are the scalar form's.  Needs even H and W, pitch % 4 == 0, ts % 4 == 0,
// 4 gq <= pitch and a 16-B aligned haloed base (launch_upsample2x_add checks them).  n_items = planes x (H / 2 + 1) x groups per row.
__global__ __launch_bounds__(256) void upsample2x_add_vec4x2_kernel(float* __restrict__ fine_halo, const float* __restrict__ coarse, int H, int W, unsigned gq,
                                                                     unsigned n_items, int64_t f_ts, int f_pitch, int64_t c_ts, int c_pitch) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n_items) return;
    const int Hc = H / 2, Wc = W / 2;
    const unsigned rowp = idx / gq;                          // plane * (Hc + 1) + m
    const int k = (int)(idx - rowp * gq);
    const unsigned pl = rowp / (unsigned)(Hc + 1);
    const int m = (int)(rowp - pl * (unsigned)(Hc + 1));
    const bool row_a = m >= 1, row_b = m < Hc;               // rows 2m - 1, 2m
    const int y0 = m >= 1 ? m - 1 : 0, y1 = y0 + (y0 < Hc - 1 ? 1 : 0);
    const float wy_a = 0.25f, wy_b = m >= 1 ? 0.75f : 0.f;
    const float* c0 = coarse + (int64_t)pl * c_ts + (int64_t)y0 * c_pitch;
    const float* c1 = coarse + (int64_t)pl * c_ts + (int64_t)y1 * c_pitch;
    const int xa = min(max(2 * k - 1, 0), Wc - 1), xb = min(2 * k, Wc - 1), xc = min(2 * k + 1, Wc - 1);
    const float a0 = c0[xa], b0 = c0[xb], d0 = c0[xc], a1 = c1[xa], b1 = c1[xb], d1 = c1[xc];
    float* fbase = fine_halo + (int64_t)pl * f_ts + 4 * k;
    float4 fa = {0.f, 0.f, 0.f, 0.f}, fb = {0.f, 0.f, 0.f, 0.f};
    if (row_a) fa = *reinterpret_cast<const float4*>(fbase + (int64_t)(2 * m) * f_pitch);            // (row y sits at haloed row y + 1)
    if (row_b) fb = *reinterpret_cast<const float4*>(fbase + (int64_t)(2 * m + 1) * f_pitch);
    float* va = reinterpret_cast<float*>(&fa);
    float* vb = reinterpret_cast<float*>(&fb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = 4 * k - 1 + j;
        if (x < 0 || x >= W) continue;
        // corners (c[x0], c[x1]) of the two coarse rows and wx: j = 0, 1 -> columns (2k - 1, 2k), j = 2, 3 -> (2k, 2k + 1); x = 0 -> (0, 1) with wx = 0
        const bool first = j < 2 && x > 0;
        const float p0 = first ? a0 : (x == 0 ? a0 : b0), p1 = first ? b0 : d0;
        const float q0 = first ? a1 : (x == 0 ? a1 : b1), q1 = first ? b1 : d1;
        const float wx = x == 0 ? 0.f : ((x & 1) ? 0.25f : 0.75f);
        if (row_a) va[j] = __fadd_rn(va[j], up2_blend(p0, p1, q0, q1, wx, wy_a));
        if (row_b) vb[j] = __fadd_rn(vb[j], up2_blend(p0, p1, q0, q1, wx, wy_b));
    }
    if (row_a) *reinterpret_cast<float4*>(fbase + (int64_t)(2 * m) * f_pitch) = fa;
    if (row_b) *reinterpret_cast<float4*>(fbase + (int64_t)(2 * m + 1) * f_pitch) = fb;
}

// The same two-row form reading the fine term from a DENSE [planes][H][W] map (the lateral conv's output written by the 16-byte epilogue; its
// by-element epilogue into the zero-haloed layout issued four times the store instructions and ran at 2.2 TB/s) and writing the zero-haloed
// consumer layout: the layout change rides on the pass that touches every element anyway.  A group's four map columns 4k - 1 .. 4k + 2 straddle two
// aligned dense groups: two 16-byte loads per row (the first is the neighbouring thread's second: an L1 hit).  Halo words of a group are written
// as zero.  Same expression per output as the in-place form => the same bits.
__global__ __launch_bounds__(256) void upsample2x_add_dense_vec4x2_kernel(float* __restrict__ fine_halo, const float* __restrict__ fine_dense,
                                                                           const float* __restrict__ coarse, int H, int W, unsigned gq, unsigned n_items,
                                                                           int64_t f_ts, int f_pitch, int64_t c_ts, int c_pitch) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n_items) return;
    const int Hc = H / 2, Wc = W / 2;
    const unsigned rowp = idx / gq;                          // plane * (Hc + 1) + m
    const int k = (int)(idx - rowp * gq);
    const unsigned pl = rowp / (unsigned)(Hc + 1);
    const int m = (int)(rowp - pl * (unsigned)(Hc + 1));
    const bool row_a = m >= 1, row_b = m < Hc;               // rows 2m - 1, 2m
    const int y0 = m >= 1 ? m - 1 : 0, y1 = y0 + (y0 < Hc - 1 ? 1 : 0);
    const float wy_a = 0.25f, wy_b = m >= 1 ? 0.75f : 0.f;
    const float* c0 = coarse + (int64_t)pl * c_ts + (int64_t)y0 * c_pitch;
    const float* c1 = coarse + (int64_t)pl * c_ts + (int64_t)y1 * c_pitch;
    const int xa = min(max(2 * k - 1, 0), Wc - 1), xb = min(2 * k, Wc - 1), xc = min(2 * k + 1, Wc - 1);
    const float a0 = c0[xa], b0 = c0[xb], d0 = c0[xc], a1 = c1[xa], b1 = c1[xb], d1 = c1[xc];
    const float* dbase = fine_dense + (int64_t)pl * H * W;
    float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f};
    // map columns 4k - 1 .. 4k + 2 of rows 2m - 1 / 2m: the last word of dense group k - 1 and the first three of group k (W % 4 == 0)
    const bool g_lo = k >= 1, g_hi = 4 * k < W;
    if (row_a) {
        const float* r = dbase + (int64_t)(2 * m - 1) * W;
        if (g_lo) va[0] = reinterpret_cast<const float4*>(r)[k - 1].w;
        if (g_hi) { const float4 q = reinterpret_cast<const float4*>(r)[k]; va[1] = q.x; va[2] = q.y; va[3] = q.z; }
    }
    if (row_b) {
        const float* r = dbase + (int64_t)(2 * m) * W;
        if (g_lo) vb[0] = reinterpret_cast<const float4*>(r)[k - 1].w;
        if (g_hi) { const float4 q = reinterpret_cast<const float4*>(r)[k]; vb[1] = q.x; vb[2] = q.y; vb[3] = q.z; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = 4 * k - 1 + j;
        if (x < 0 || x >= W) { va[j] = 0.f; vb[j] = 0.f; continue; }      // halo words of the group
        const bool first = j < 2 && x > 0;
        const float p0 = first ? a0 : (x == 0 ? a0 : b0), p1 = first ? b0 : d0;
        const float q0 = first ? a1 : (x == 0 ? a1 : b1), q1 = first ? b1 : d1;
        const float wx = x == 0 ? 0.f : ((x & 1) ? 0.25f : 0.75f);
        if (row_a) va[j] = __fadd_rn(va[j], up2_blend(p0, p1, q0, q1, wx, wy_a));
        if (row_b) vb[j] = __fadd_rn(vb[j], up2_blend(p0, p1, q0, q1, wx, wy_b));
    }
    float* fbase = fine_halo + (int64_t)pl * f_ts + 4 * k;
    if (row_a) *reinterpret_cast<float4*>(fbase + (int64_t)(2 * m) * f_pitch) = make_float4(va[0], va[1], va[2], va[3]);            // (row y sits at haloed row y + 1)
    if (row_b) *reinterpret_cast<float4*>(fbase + (int64_t)(2 * m + 1) * f_pitch) = make_float4(vb[0], vb[1], vb[2], vb[3]);
}

static int grid1d(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 256), 256 * 16)); }

// ---- the streaming passes' launch functions: each pass's choice of kernel lives HERE and nowhere else -- stemseg_hip_encoder_forward and the per-pass
// entry points (stemseg_hip_maxpool3x3s2, _encoder_subsample2, _upsample2x_add, _stem_s2d) both come through them.  form 0 = the function's own choice,
// > 0 forces one kernel (STEMSEG_E_INVALID with a message, and no launch, where its preconditions do not hold); *form_used = what ran.  The pointers
// need not be the encoder's: what the workspace layout guarantees there (16-B aligned slices, pitch % 4, ts % 4) is checked per launch, and a launch
// that misses it takes the scalar form.
static inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// max-pool and stride-2 copy, [planes][H][W] -> [planes][H / 2][W / 2]: the 16-B form holds one thread per four outputs of a row (eight input columns)
// and indexes in 32 bits
static int64_t stride2_vec_items(int64_t planes, int H, int W) { return planes * (H / 2) * (W / 8); }
static int stride2_form(int64_t planes, int H, int W, bool aligned) {
    return (W % 8 == 0 && stride2_vec_items(planes, H, W) < (1ll << 31) && aligned) ? STEMSEG_STREAM_FORM_VEC4 : STEMSEG_STREAM_FORM_SCALAR;
}
static int check_stride2(const char* who, const float* in, int64_t planes, int H, int W, const float* out, int form, int* used) {
    SS_CHECK_ARG(in && out, "%s: null pointer", who);
    SS_CHECK_ARG(planes >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && planes <= (1ll << 40) / ((int64_t)H * W),
                 "%s: planes=%lld H=%d W=%d (H, W even)", who, (long long)planes, H, W);
    SS_CHECK_ARG(form == STEMSEG_STREAM_FORM_AUTO || form == STEMSEG_STREAM_FORM_SCALAR || form == STEMSEG_STREAM_FORM_VEC4, "%s: form=%d", who, form);
    const int own = stride2_form(planes, H, W, aligned16(in) && aligned16(out));
    SS_CHECK_ARG(form != STEMSEG_STREAM_FORM_VEC4 || own == STEMSEG_STREAM_FORM_VEC4,
                 "%s: the 16-byte form needs W %% 8 == 0 (W=%d), 16-byte aligned pointers and fewer than 2^31 items", who, W);
    *used = form ? form : own;
    return STEMSEG_OK;
}

// max-pool 3x3 stride 2 pad 1 of every plane
static int launch_maxpool3x3s2(const float* in, int64_t planes, int H, int W, float* out, int form, int* form_used, hipStream_t s) {
    int used = 0;
    int rc = check_stride2("maxpool3x3s2", in, planes, H, W, out, form, &used);
    if (rc) return rc;
    void* ev = profile_begin(48, 4.0 * (double)planes * ((double)H * W + (double)(H / 2) * (W / 2)), s);
    if (used == STEMSEG_STREAM_FORM_VEC4) {
        const int64_t items = stride2_vec_items(planes, H, W);
        hipLaunchKernelGGL(maxpool3x3s2_vec4_kernel, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, s, in, out, H, W, (unsigned)items);
    } else {
        hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(grid1d(planes * (H / 2) * (W / 2))), dim3(256), 0, s, in, out, planes, H, W);
    }
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    if (form_used) *form_used = used;
    return STEMSEG_OK;
}

// out[pl][y][x] = in[pl][2y][2x]
static int launch_encoder_subsample2(const float* in, int64_t planes, int H, int W, float* out, int form, int* form_used, hipStream_t s) {
    int used = 0;
    int rc = check_stride2("encoder_subsample2", in, planes, H, W, out, form, &used);
    if (rc) return rc;
    void* ev = profile_begin(49, 4.0 * 2.0 * (double)planes * (H / 2) * (W / 2), s);       // (the kept quarter is read, sector granularity aside)
    if (used == STEMSEG_STREAM_FORM_VEC4) {
        const int64_t items = stride2_vec_items(planes, H, W);
        hipLaunchKernelGGL(subsample2_vec4_kernel, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, s, in, out, H, W, (unsigned)items);
    } else {
        hipLaunchKernelGGL(subsample2_kernel, dim3(grid1d(planes * (H / 2) * (W / 2))), dim3(256), 0, s, in, out, planes, H, W);
    }
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    if (form_used) *form_used = used;
    return STEMSEG_OK;
}

// FPN top-down add.  The 16-B forms write whole aligned groups of the HALOED fine rows: gq groups cover haloed columns 1 .. W and must fit the pitch; their
// item count (the in-place form is held to the count of one thread per row and group, H x gq a plane, which bounds its own (H / 2 + 1) x gq) stays in 32 bits.
static unsigned up2_groups(int W) { return (unsigned)((W + 1) / 4 + 1); }
static bool up2_vec_ok(int64_t planes, int H, int W, int64_t f_ts, int64_t f_pitch, bool base_aligned) {
    const unsigned gq = up2_groups(W);
    return f_pitch % 4 == 0 && (int64_t)4 * gq <= f_pitch && planes * H * gq < (1ll << 32) - 256 && base_aligned && f_ts % 4 == 0;
}
static bool up2_dense_ok(int64_t planes, int H, int W, int64_t f_ts, int64_t f_pitch, bool base_aligned, bool dense_aligned) {
    const unsigned gq = up2_groups(W);
    return W % 4 == 0 && f_pitch % 4 == 0 && (int64_t)4 * gq <= f_pitch && planes * (H / 2 + 1) * gq < (1ll << 32) - 256 && base_aligned && f_ts % 4 == 0 &&
           dense_aligned;
}
// H and W even.  dense: the fine term comes from a dense [planes][H][W] map -- only the dense form reads one (0: none applies); else in place
static int up2_form(int64_t planes, int H, int W, int64_t f_ts, int64_t f_pitch, bool base_aligned, bool dense, bool dense_aligned) {
    if (dense) return up2_dense_ok(planes, H, W, f_ts, f_pitch, base_aligned, dense_aligned) ? STEMSEG_UP2_FORM_DENSE : 0;
    return up2_vec_ok(planes, H, W, f_ts, f_pitch, base_aligned) ? STEMSEG_UP2_FORM_VEC4X2 : STEMSEG_UP2_FORM_SCALAR;
}

// fine (+)= bilinear_x2(coarse): fine [C][T][H][W] and coarse [C][T][H / 2][W / 2] the INTERIOR views of zero-haloed 2-D buffers (one halo row above and
// one halo column left of the view belong to the buffer: the 16-B forms address the haloed rows).  fine_dense: null (in place), or the dense map the fine
// term is read from.
static int launch_upsample2x_add(const StemsegVolume& fine, const float* fine_dense, const StemsegVolume& coarse, int form, int* form_used, hipStream_t s) {
    SS_CHECK_ARG(fine.ptr && coarse.ptr, "upsample2x_add: null pointer");
    int rc = check_view("upsample2x_add", "fine", fine);
    if (rc) return rc;
    rc = check_view("upsample2x_add", "coarse", coarse);
    if (rc) return rc;
    const int H = fine.H, W = fine.W;
    SS_CHECK_ARG(H % 2 == 0 && W % 2 == 0 && coarse.C == fine.C && coarse.T == fine.T && coarse.H == H / 2 && coarse.W == W / 2,
                 "upsample2x_add: fine [%d][%d][%d][%d] must be exactly twice coarse [%d][%d][%d][%d] (H, W even)", fine.C, fine.T, H, W, coarse.C, coarse.T,
                 coarse.H, coarse.W);
    SS_CHECK_ARG(fine.c_stride == (int64_t)fine.T * fine.t_stride && coarse.c_stride == (int64_t)coarse.T * coarse.t_stride,
                 "upsample2x_add: the planes of a view must lie one t_stride apart (c_stride == T * t_stride)");
    SS_CHECK_ARG(fine.y_stride >= W + 2 && coarse.y_stride < (1ll << 31) && fine.y_stride < (1ll << 31),
                 "upsample2x_add: fine's row pitch %lld does not hold the haloed row (W + 2 = %d)", (long long)fine.y_stride, W + 2);
    SS_CHECK_ARG(form >= 0 && form <= STEMSEG_UP2_FORM_DENSE, "upsample2x_add: form=%d", form);
    const int64_t planes = (int64_t)fine.C * fine.T, f_ts = fine.t_stride, f_pitch = fine.y_stride;
    float* fine_halo = fine.ptr - (f_pitch + 1);
    const int own = up2_form(planes, H, W, f_ts, f_pitch, aligned16(fine_halo), fine_dense != nullptr, aligned16(fine_dense));
    if (fine_dense) {
        SS_CHECK_ARG(form == 0 || form == STEMSEG_UP2_FORM_DENSE, "upsample2x_add: form %d does not read a dense fine map", form);
        SS_CHECK_ARG(own == STEMSEG_UP2_FORM_DENSE,
                     "upsample2x_add: the dense form needs W %% 4 == 0 (W=%d), pitch %% 4 == 0, t_stride %% 4 == 0, 4 * %u groups <= pitch %lld, 16-byte aligned "
                     "haloed rows and dense map, and fewer than 2^32 items", W, up2_groups(W), (long long)f_pitch);
    } else {
        SS_CHECK_ARG(form != STEMSEG_UP2_FORM_DENSE, "upsample2x_add: the dense form needs a dense fine map");
        SS_CHECK_ARG(form != STEMSEG_UP2_FORM_VEC4X2 || own == STEMSEG_UP2_FORM_VEC4X2,
                     "upsample2x_add: the two-row form needs pitch %% 4 == 0, t_stride %% 4 == 0, 4 * %u groups <= pitch %lld, 16-byte aligned haloed rows and "
                     "fewer than 2^32 items", up2_groups(W), (long long)f_pitch);
    }
    const int used = form ? form : own;
    const unsigned gq = up2_groups(W);
    const int64_t items = planes * (H / 2 + 1) * gq;
    void* ev = profile_begin(50, 4.0 * (double)planes * (2.0 * H * W + (double)(H / 2) * (W / 2)), s);         // fine read + written, coarse read
    if (used == STEMSEG_UP2_FORM_DENSE)
        hipLaunchKernelGGL(upsample2x_add_dense_vec4x2_kernel, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, s, fine_halo, fine_dense,
                           (const float*)coarse.ptr, H, W, gq, (unsigned)items, f_ts, (int)f_pitch, coarse.t_stride, (int)coarse.y_stride);
    else if (used == STEMSEG_UP2_FORM_VEC4X2)
        hipLaunchKernelGGL(upsample2x_add_vec4x2_kernel, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, s, fine_halo, (const float*)coarse.ptr, H, W, gq,
                           (unsigned)items, f_ts, (int)f_pitch, coarse.t_stride, (int)coarse.y_stride);
    else
        hipLaunchKernelGGL(upsample2x_add_kernel, dim3(grid1d(planes * H * W)), dim3(256), 0, s, fine.ptr, (const float*)coarse.ptr, planes, H, W, f_ts, f_pitch,
                           coarse.t_stride, coarse.y_stride);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    if (form_used) *form_used = used;
    return STEMSEG_OK;
}

// frames [T][3][H][W] -> the space-to-depth image [12][T][H / 2 + 3][W / 2 + 3] (see stem_s2d_kernel): the data two rows and columns into each plane; the
// halo is not written
static int launch_stem_s2d(const float* frames, int T, int H, int W, const StemsegVolume& v, hipStream_t s) {
    SS_CHECK_ARG(frames && v.ptr, "stem_s2d: null pointer");
    SS_CHECK_ARG(T >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "stem_s2d: T=%d H=%d W=%d (H, W even)", T, H, W);
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(frames) % 8 == 0, "stem_s2d: frames must be 8-byte aligned");
    int rc = check_view("stem_s2d", "s2d", v);
    if (rc) return rc;
    SS_CHECK_ARG(v.C == 12 && v.T == T && v.H == H / 2 + 3 && v.W == W / 2 + 3 && v.c_stride == (int64_t)T * v.t_stride && v.y_stride < (1ll << 31),
                 "stem_s2d: the image must be [12][%d][%d][%d] with c_stride == T * t_stride, got [%d][%d][%d][%d]", T, H / 2 + 3, W / 2 + 3, v.C, v.T, v.H, v.W);
    hipLaunchKernelGGL(stem_s2d_kernel, dim3(grid1d((int64_t)T * 3 * H * (W / 2))), dim3(256), 0, s, frames, v.ptr, T, H, W, v.t_stride, (int)v.y_stride);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

struct EncoderPlan {
    GuardList guards;          // one guard block behind every slice below (common.h: workspace canaries)
    int T, H, W, nblk[4], total_blocks;
    int h[4], w[4];            // 4x, 8x, 16x, 32x
    int64_t V[4];
    int64_t S0, X1, A, B, Cst[4], M1[4], M2, DS, XS, L[4], FO[4], SK, SKfloats, total;
    int64_t LAT[3];            // dense FPN lateral maps of the stage-end tails (levels 4x, 8x, 16x)
    int64_t S2D, s2d_ts, s2d_pitch;
    int groups, s3, mid[4];    // conv2 groups, stride in the 3x3 (first block of stages 1-3), bottleneck channels per stage
    int64_t M1S[4];            // stride in the 3x3: conv1 output of a stage's first block at the previous stage's resolution (-1: absent)
    int plan_frames;           // 0: launches decide on their real shape
    int64_t plan_SKfloats;     // split-K scratch a planned launch may count on
};
constexpr int64_t ENC_PLAN_SK_FLOATS = 32ll << 20;

static int make_encoder_plan(const StemsegEncoderDesc* d, EncoderPlan& p) {
    SS_CHECK_ARG(d, "encoder: null descriptor");
    // the architecture fields came after ABI 11 shipped: a descriptor of the older size means today's network
    constexpr int32_t old_bytes = (int32_t)offsetof(StemsegEncoderDesc, conv2_groups);
    SS_CHECK_ARG(d->struct_bytes == (int32_t)sizeof(StemsegEncoderDesc) || d->struct_bytes == old_bytes,
                 "encoder: descriptor size mismatch (%d vs %d or %d): ABI skew", d->struct_bytes, (int)sizeof(StemsegEncoderDesc), (int)old_bytes);
    const bool has_arch = d->struct_bytes == (int32_t)sizeof(StemsegEncoderDesc);
    const int groups = has_arch && d->conv2_groups > 0 ? d->conv2_groups : 1;
    const int wpg = has_arch && d->width_per_group > 0 ? d->width_per_group : 64;
    SS_CHECK_ARG(!has_arch || (d->conv2_groups >= 0 && d->width_per_group >= 0 && (d->stride_in_3x3 == 0 || d->stride_in_3x3 == 1)),
                 "encoder: conv2_groups=%d width_per_group=%d stride_in_3x3=%d", d->conv2_groups, d->width_per_group, d->stride_in_3x3);
    if (groups == 1) {
        SS_CHECK_ARG(wpg == 64, "encoder: width_per_group=%d with one group (64 only)", wpg);
    } else {
        SS_CHECK_ARG((wpg == 4 || wpg == 8) && groups <= 1024 && (groups * wpg) % 32 == 0,
                     "encoder: %d groups x %d channels (width_per_group 4 or 8: 4..64 channels per group over the stages; groups x width a multiple of 32)",
                     groups, wpg);
    }
    p.groups = groups;
    p.s3 = has_arch ? d->stride_in_3x3 : 0;
    for (int i = 0; i < 4; ++i) p.mid[i] = (groups * wpg) << i;
    SS_CHECK_ARG(d->n_clips >= 1 && d->clip_frames >= 0 && d->clip_stride >= 0, "encoder: bad clip layout");
    if (d->clip_frames > 0) {
        SS_CHECK_ARG(d->clip_stride > 0 && (d->n_clips - 1) * d->clip_stride + d->clip_frames == d->T,
                     "encoder: %d windows of %d frames every %d frames do not cover T=%d", d->n_clips, d->clip_frames, d->clip_stride, d->T);
    } else {
        SS_CHECK_ARG(d->T % d->n_clips == 0, "encoder: T=%d is not n_clips=%d whole clips", d->T, d->n_clips);
    }
    SS_CHECK_ARG(d->T >= 1 && d->H >= 32 && d->W >= 32 && d->H % 32 == 0 && d->W % 32 == 0, "encoder: T=%d H=%d W=%d (H, W multiples of 32)", d->T, d->H, d->W);
    p.T = d->T; p.H = d->H; p.W = d->W;
    p.total_blocks = 0;
    for (int i = 0; i < 4; ++i) {
        SS_CHECK_ARG(d->blocks[i] >= 1 && d->blocks[i] <= 64, "encoder: blocks[%d]=%d", i, d->blocks[i]);
        p.nblk[i] = d->blocks[i];
        p.total_blocks += d->blocks[i];
        p.h[i] = d->H >> (2 + i); p.w[i] = d->W >> (2 + i);
        p.V[i] = (int64_t)d->T * p.h[i] * p.w[i];
    }
    SS_CHECK_ARG(p.total_blocks <= STEMSEG_MAX_ENCODER_BLOCKS, "encoder: more than %d bottleneck blocks", STEMSEG_MAX_ENCODER_BLOCKS);
    int64_t off = 0;
    p.guards.n = 0;
    auto take = [&](int64_t floats) {            // a slice + its guard block
        int64_t o = off;
        off += round_up(floats, 64);
        p.guards.push(off);
        off += WS_GUARD_FLOATS;
        return o;
    };
    p.S0 = take(64 * 4 * p.V[0]);
    // space-to-depth image of the frames for the f16x3 stem: [12][T][H/2 + 3][pitch], two halo rows / columns before, one after (zero, written once)
    p.s2d_pitch = round_up(d->W / 2 + 3, 4);
    p.s2d_ts = (int64_t)(d->H / 2 + 3) * p.s2d_pitch;
    p.S2D = take(12 * (int64_t)d->T * p.s2d_ts + 64);
    p.X1 = take(64 * p.V[0]);
    p.A = take(256 * p.V[0]);
    p.B = take(256 * p.V[0]);
    for (int i = 0; i < 4; ++i) {
        p.Cst[i] = take((int64_t)(256 << i) * p.V[i]);
        // one zero-haloed buffer PER STAGE: the halo stays zero only while a buffer keeps one geometry
        p.M1[i] = take(Padded2D(p.mid[i], p.T, p.h[i], p.w[i]).total);
    }
    p.M2 = take((int64_t)p.mid[0] * p.V[0]);          // (mid_s x V_s halves per stage: stage 0 holds the most)
    p.DS = take(256 * p.V[0]);
    p.XS = take(256 * p.V[1]);
    for (int i = 0; i < 4; ++i) p.L[i] = take(Padded2D(256, p.T, p.h[i], p.w[i]).total);
    // overlapping windows: the FPN output convs run ONCE over all frames into dense maps, each clip's window is then copied out
    const bool shared_out = d->clip_frames > 0 && d->clip_stride < d->clip_frames && d->n_clips > 1;
    for (int i = 0; i < 4; ++i) p.FO[i] = shared_out ? take(256 * p.V[i]) : -1;
    for (int i = 0; i < 4; ++i) p.M1S[i] = (p.s3 && i > 0) ? take(Padded2D(p.mid[i], p.T, p.h[i - 1], p.w[i - 1]).total) : -1;
    SS_CHECK_ARG(d->plan_frames >= 0 && d->plan_frames <= 4096, "encoder: plan_frames=%d", d->plan_frames);
    p.plan_frames = d->plan_frames;
    p.plan_SKfloats = ENC_PLAN_SK_FLOATS;
    // a pass of more frames than planned keeps the plan's K-partition, so its slabs are T / plan_frames times the planned ones
    p.SKfloats = ENC_PLAN_SK_FLOATS * (d->plan_frames > 0 ? std::max<int64_t>(1, ceil_div(d->T, d->plan_frames)) : 1);
    p.SK = take(p.SKfloats);
    // The lateral maps the stage-end tails (bottleneck_fused.hip) write must outlive the rest of the backbone, which A does not.  S0 -- the stem's output,
    // 256 V[0] floats -- is dead behind the max-pool, and X1 -- the max-pool's, 64 V[0] = 256 V[1] floats -- behind stage 1's first block (conv1 and the
    // shortcut read it, nothing later does; a stage end is never a stage's first block): levels 4x and 8x.  Level 16x gets a slice of its own behind the
    // existing ones.
    p.LAT[0] = p.S0;
    p.LAT[1] = p.X1;
    p.LAT[2] = take(256 * p.V[2]);
    p.total = off;
    SS_CHECK_ARG(!p.guards.full, "encoder: the plan has more than %d workspace slices (GuardList)", WS_MAX_GUARDS);
    return STEMSEG_OK;
}

// The stem and the max-pool of a pass (resnet.py:292-304): frames -> stem_out [64][T][H / 2][W / 2] -> pooled [64][T][H / 4][W / 4].  What
// stemseg_hip_encoder_forward runs first, and what stemseg_hip_encoder_stem_forward runs again for the backward: one code path, so the same bits.
// s2d: the plan's space-to-depth slice (the f16x3 path's staging image; its halo holds the zeros stemseg_hip_encoder_init_workspace wrote).
static int run_stem(const EncoderPlan& p, const StemsegEncoderWeights* wts, int prec, const float* frames, float* s2d, float* stem_out, float* pooled,
                    hipStream_t s) {
    const int T = p.T;
    int rc;
    const int Ho = p.H / 2, Wo = p.W / 2;
    const int blocks = (int)(ceil_div(Wo, ST_COLS) * ceil_div(Ho, ST_ROWS) * T);
    void* ev = profile_begin(47, 4.0 * ((double)3 * T * p.H * p.W + 64.0 * T * Ho * Wo), s);
    if (wts->stem_w_s2d && prec == STEMSEG_PRECISION_F16X3 && p.W % 2 == 0) {
        // space-to-depth + 4x4 convolution on the split-staged kernel (see stem_s2d_kernel)
        const StemsegVolume in = make_volume(s2d, (int64_t)T * p.s2d_ts, p.s2d_ts, p.s2d_pitch, 12, T, Ho + 3, Wo + 3, 12 * (int64_t)T * p.s2d_ts + 64);
        rc = launch_stem_s2d(frames, T, p.H, p.W, in, s);
        if (rc) return rc;
        ConvEpilogue es;                // this precision, and the launch decisions on the planning frame count (epi_for of the pass)
        es.precision = prec;
        if (p.plan_frames > 0) { es.frames = T; es.plan_frames = p.plan_frames; es.plan_scratch_floats = p.plan_SKfloats; }
        es.relu = 1;
        rc = launch_conv3d(in, wts->stem_w_s2d, wts->stem_b, dense_volume(stem_out, 64, T, Ho, Wo), 1, 4, 4, 0, s, nullptr, 0, &es);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(stem_conv7x7_mfma_kernel, dim3((unsigned)blocks), dim3(256), 0, s, frames, wts->stem_w, wts->stem_b, stem_out, T, p.H, p.W);
    }
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return launch_maxpool3x3s2(stem_out, (int64_t)64 * T, Ho, Wo, pooled, 0, nullptr, s);
}

// Stage-end tail (f16x3; bottleneck_fused.hip): the last block of stages 1-3 ends in conv3 + the level's FPN lateral + the stride-2 copy the next stage
// starts from, in one launch.  Bit k: stage k + 1's end takes it, as far as the descriptor decides -- the pass then asks that block's conv2 for operand
// planes, and the tail runs where conv2's plan is un-split (else the block keeps its launches, and their bits).
static int stage_end_mask(const StemsegEncoderDesc* d, const EncoderPlan& p) {
    int mask = 0;
    for (int k = 0; k < 3; ++k) {
        const int h = p.h[k], w = p.w[k], mid = p.mid[k];
        // the stage runs fused tails at all and its end is not switched off (fuse_tail bits 6-8); today's widths, stride in conv1; the end is not also the
        // stage's first block
        bool ok = ((d->fuse_tail >> k) & 1) && !((d->fuse_tail >> (6 + k)) & 1) && d->precision == STEMSEG_PRECISION_F16X3 && p.groups == 1 && !p.s3 &&
                  mid * 4 == (256 << k) && p.nblk[k] >= 2 && fused_stage_end_supported(mid, p.V[k]) && (int64_t)p.T * (h + 2) * (w + 4) <= (1ll << 27);
        // the level's add pass can read a dense lateral map (up2_form, as the FPN loop asks it, for 16-B aligned slices)
        Padded2D gf0(256, p.T, h, w);
        ok = ok && up2_form((int64_t)256 * p.T, h, w, gf0.ts, gf0.pitch, true, true, true) == STEMSEG_UP2_FORM_DENSE;
        // ... and the stand-alone lateral is the un-split 256-channel tile (conv_split_family.h: from half a round of its 256-voxel workgroups on the planning
        // shape), whose sums the tail's slot repeats; a smaller map's launch may split K, and keeps its own bits
        const int64_t v_plan = p.plan_frames > 0 ? p.V[k] / p.T * p.plan_frames : p.V[k];
        ok = ok && ceil_div(v_plan, 256) >= 128;
        if (ok) mask |= 1 << k;
    }
    return mask;
}

}  // namespace stemseg

using namespace stemseg;

// Debugging aid (tests): bit k = the end of stage k + 1 takes the stage-end tail, as far as the descriptor decides (stage_end_mask).
extern "C" int stemseg_hip_encoder_stage_end_mask(const StemsegEncoderDesc* desc, int32_t* mask_out) {
    EncoderPlan p;
    int rc = make_encoder_plan(desc, p);
    if (rc) return rc;
    SS_CHECK_ARG(mask_out, "encoder_stage_end_mask: null pointer");
    *mask_out = stage_end_mask(desc, p);
    return STEMSEG_OK;
}

extern "C" size_t stemseg_hip_encoder_workspace_bytes(const StemsegEncoderDesc* desc) {
    EncoderPlan p;
    if (make_encoder_plan(desc, p) != STEMSEG_OK) return 0;
    return (size_t)p.total * sizeof(float);
}

// Debugging aid (tests, tools): float offsets of the plan's buffers inside the workspace, in the order S0, X1, A, B, Cst[4], M1[4], M2, DS,
// XS, L[4], FO[4], SK, total (25 values; -1 = not present).
extern "C" int stemseg_hip_encoder_plan_offsets(const StemsegEncoderDesc* desc, int64_t* out25) {
    EncoderPlan p;
    int rc = make_encoder_plan(desc, p);
    if (rc) return rc;
    SS_CHECK_ARG(out25, "encoder_plan_offsets: null pointer");
    int n = 0;
    out25[n++] = p.S0; out25[n++] = p.X1; out25[n++] = p.A; out25[n++] = p.B;
    for (int i = 0; i < 4; ++i) out25[n++] = p.Cst[i];
    for (int i = 0; i < 4; ++i) out25[n++] = p.M1[i];
    out25[n++] = p.M2; out25[n++] = p.DS; out25[n++] = p.XS;
    for (int i = 0; i < 4; ++i) out25[n++] = p.L[i];
    for (int i = 0; i < 4; ++i) out25[n++] = p.FO[i];
    out25[n++] = p.SK; out25[n++] = p.total;
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_encoder_init_workspace(const StemsegEncoderDesc* desc, void* workspace, size_t ws_bytes, void* stream) {
    EncoderPlan p;
    int rc = make_encoder_plan(desc, p);
    if (rc) return rc;
    SS_CHECK_ARG(workspace && (reinterpret_cast<uintptr_t>(workspace) % 256 == 0), "encoder: workspace must be 256-byte aligned");
    if (ws_bytes < (size_t)p.total * sizeof(float)) {
        set_error("encoder: workspace too small (%zu < %zu bytes)", ws_bytes, (size_t)p.total * sizeof(float));
        return STEMSEG_E_WORKSPACE;
    }
    // only the zero-haloed buffers need it, but one memset keeps the rule simple
    SS_HIP(hipMemsetAsync(workspace, 0, (size_t)p.total * sizeof(float), as_stream(stream)));
    return launch_canary_fill(reinterpret_cast<float*>(workspace), p.guards, as_stream(stream));
}

extern "C" int stemseg_hip_encoder_check_workspace(const StemsegEncoderDesc* desc, const void* workspace, size_t ws_bytes, int32_t* n_bad_host,
                                                   int64_t* first_bad_host, void* stream) {
    EncoderPlan p;
    int rc = make_encoder_plan(desc, p);
    if (rc) return rc;
    SS_CHECK_ARG(workspace && ws_bytes >= (size_t)p.total * sizeof(float), "encoder_check_workspace: bad workspace");
    return canary_check(reinterpret_cast<const float*>(workspace), p.guards, n_bad_host, first_bad_host, as_stream(stream));
}

extern "C" int stemseg_hip_stem_conv(const float* frames, const float* w_tap_major, const float* bias, float* out, int32_t T, int32_t H, int32_t W,
                                     void* stream) {
    SS_CHECK_ARG(frames && w_tap_major && bias && out, "stem_conv: null pointer");
    SS_CHECK_ARG(T >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "stem_conv: T=%d H=%d W=%d (H, W even)", T, H, W);
    const int Ho = H / 2, Wo = W / 2;
    const int64_t blocks = ceil_div(Wo, ST_COLS) * ceil_div(Ho, ST_ROWS) * T;
    SS_CHECK_ARG(blocks < (1ll << 31), "stem_conv: too many tiles");
    hipLaunchKernelGGL(stem_conv7x7_mfma_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), frames, w_tap_major, bias, out, T, H, W);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

// ---- the streaming passes on their own (tests, per-kernel benches): the launch functions the pass itself calls
extern "C" int stemseg_hip_maxpool3x3s2(const float* in, int64_t planes, int32_t H, int32_t W, float* out, int32_t form, int32_t* form_used, void* stream) {
    return launch_maxpool3x3s2(in, planes, H, W, out, form, form_used, as_stream(stream));
}

extern "C" int stemseg_hip_encoder_subsample2(const float* in, int64_t planes, int32_t H, int32_t W, float* out, int32_t form, int32_t* form_used,
                                              void* stream) {
    return launch_encoder_subsample2(in, planes, H, W, out, form, form_used, as_stream(stream));
}

extern "C" int stemseg_hip_upsample2x_add(const StemsegVolume* fine, const float* fine_dense, const StemsegVolume* coarse, int32_t form, int32_t* form_used,
                                          void* stream) {
    SS_CHECK_ARG(fine && coarse, "upsample2x_add: null view");
    return launch_upsample2x_add(*fine, fine_dense, *coarse, form, form_used, as_stream(stream));
}

extern "C" int stemseg_hip_stem_s2d(const float* frames, int32_t T, int32_t H, int32_t W, const StemsegVolume* s2d, void* stream) {
    SS_CHECK_ARG(s2d, "stem_s2d: null view");
    return launch_stem_s2d(frames, T, H, W, *s2d, as_stream(stream));
}

// Debugging aid (tests): the form each streaming pass of stemseg_hip_encoder_forward takes for this descriptor on a 16-B aligned workspace -- the max-pool,
// the stride-2 copy in front of stages 2, 3, 4 (where it runs: a stage-end tail writes that copy itself), the top-down add of levels 4x, 8x, 16x.
extern "C" int stemseg_hip_encoder_stream_forms(const StemsegEncoderDesc* desc, int32_t* out7) {
    EncoderPlan p;
    int rc = make_encoder_plan(desc, p);
    if (rc) return rc;
    SS_CHECK_ARG(out7, "encoder_stream_forms: null pointer");
    out7[0] = stride2_form((int64_t)64 * p.T, p.H / 2, p.W / 2, true);
    for (int st = 1; st < 4; ++st) out7[st] = stride2_form((int64_t)(256 << (st - 1)) * p.T, 2 * p.h[st], 2 * p.w[st], true);
    for (int k = 0; k < 3; ++k) {
        Padded2D g(256, p.T, p.h[k], p.w[k]);
        int f = up2_form((int64_t)256 * p.T, p.h[k], p.w[k], g.ts, g.pitch, true, true, true);           // the lateral writes a dense map where that form applies
        out7[4 + k] = f ? f : up2_form((int64_t)256 * p.T, p.h[k], p.w[k], g.ts, g.pitch, true, false, true);
    }
    return STEMSEG_OK;
}

// The stem and the max-pool of stemseg_hip_encoder_forward again, into the caller's buffers (run_stem): the backward's recompute -- the pass's own S0 and
// X1 slices are the stage-end tails' lateral maps by then
extern "C" int stemseg_hip_encoder_stem_forward(const StemsegEncoderDesc* desc, const StemsegEncoderWeights* wts, const float* frames, float* stem_out,
                                                float* pooled, void* workspace, size_t ws_bytes, void* stream) {
    EncoderPlan p;
    int rc = make_encoder_plan(desc, p);
    if (rc) return rc;
    SS_CHECK_ARG(wts && frames && stem_out && pooled && workspace, "encoder_stem_forward: null pointer");
    if (ws_bytes < (size_t)p.total * sizeof(float)) {
        set_error("encoder_stem_forward: workspace too small (%zu < %zu bytes)", ws_bytes, (size_t)p.total * sizeof(float));
        return STEMSEG_E_WORKSPACE;
    }
    SS_CHECK_ARG(wts->stem_w && wts->stem_b, "encoder_stem_forward: null stem weights");
    SS_CHECK_ARG(desc->precision == STEMSEG_PRECISION_F32 || desc->precision == STEMSEG_PRECISION_BF16X6 || desc->precision == STEMSEG_PRECISION_F16X3,
                 "encoder_stem_forward: precision must be 0 (f32), 2 (bf16x6) or 3 (f16x3)");
    return run_stem(p, wts, desc->precision, frames, reinterpret_cast<float*>(workspace) + p.S2D, stem_out, pooled, as_stream(stream));
}

extern "C" int stemseg_hip_encoder_forward(const StemsegEncoderDesc* desc, const StemsegEncoderWeights* wts, const float* frames,
                                           const StemsegVolume* out, void* workspace, size_t ws_bytes, void* stream) {
    EncoderPlan p;
    int rc = make_encoder_plan(desc, p);
    if (rc) return rc;
    SS_CHECK_ARG(wts && frames && out && workspace, "encoder_forward: null pointer");
    if (ws_bytes < (size_t)p.total * sizeof(float)) {
        set_error("encoder: workspace too small (%zu < %zu bytes)", ws_bytes, (size_t)p.total * sizeof(float));
        return STEMSEG_E_WORKSPACE;
    }
    SS_CHECK_ARG(wts->stem_w && wts->stem_b, "encoder_forward: null stem weights");
    for (int i = 0; i < 4; ++i) {
        for (int c = 0; c < desc->n_clips; ++c) {
            const StemsegVolume& o = out[4 * c + i];
            const int Tc_ = desc->clip_frames > 0 ? desc->clip_frames : p.T / desc->n_clips;
            SS_CHECK_ARG(o.ptr && o.C == desc->out_channels && o.T == Tc_ && o.H == p.h[i] && o.W == p.w[i],
                         "encoder_forward: output volume %d of clip %d must be [%d][%d][%d][%d]", i, c, desc->out_channels, Tc_, p.h[i], p.w[i]);
        }
        SS_CHECK_ARG(wts->fpn_inner_w[i] && wts->fpn_inner_b[i] && wts->fpn_layer_w[i] && wts->fpn_layer_b[i], "encoder_forward: null FPN weights %d", i);
    }
    SS_CHECK_ARG(desc->out_channels == 256, "encoder: out_channels must be 256");
    SS_CHECK_ARG(desc->precision == STEMSEG_PRECISION_F32 || desc->precision == STEMSEG_PRECISION_BF16X6 || desc->precision == STEMSEG_PRECISION_F16X3,
                 "encoder: precision must be 0 (f32), 2 (bf16x6) or 3 (f16x3)");
    const int prec = desc->precision;
    // every convolution of the pass: this precision, and its launch decisions on the planning frame count (conv_igemm.h, PlanCtx)
    auto epi_for = [&](int frames) {
        ConvEpilogue e;
        e.precision = prec;
        if (p.plan_frames > 0) { e.frames = frames; e.plan_frames = p.plan_frames; e.plan_scratch_floats = p.plan_SKfloats; }
        return e;
    };
    hipStream_t s = as_stream(stream);
    float* ws = reinterpret_cast<float*>(workspace);
    const int T = p.T;

    // stem (resnet.py:292-304)
    rc = run_stem(p, wts, prec, frames, ws + p.S2D, ws + p.S0, ws + p.X1, s);
    if (rc) return rc;
    // residual stages (resnet.py:105-113)
    float* x = ws + p.X1;
    int cin = 64, bi = 0;
    bool conv1_done = false;            // this block's conv1 came out of the previous block's fused tail (bottleneck_fused.hip)
    // Stage-end tail (f16x3; bottleneck_fused.hip): the last block of stages 1-3 ends in conv3 + the level's FPN lateral + the stride-2 copy the next
    // stage starts from, in one launch -- the stage output is written once and not read back by either.  lat_ok: the level's dense-lateral add pass
    // can run from the map that launch leaves (the conditions of lat_dense below); end_done: it did.  fuse_tail bits 6-8 keep the stand-alone launches.
    const int end_mask = stage_end_mask(desc, p);
    bool lat_ok[3], end_done[3] = {false, false, false};
    for (int k = 0; k < 3; ++k)
        lat_ok[k] = ((end_mask >> k) & 1) && reinterpret_cast<uintptr_t>(ws + p.L[k]) % 16 == 0 && reinterpret_cast<uintptr_t>(ws + p.LAT[k]) % 16 == 0;
    for (int st = 0; st < 4; ++st) {
        const int mid = p.mid[st], cout = 256 << st, h = p.h[st], w = p.w[st];
        const int64_t V = p.V[st];
        for (int b = 0; b < p.nblk[st]; ++b, ++bi) {
            const bool first = (b == 0), stride2 = first && st > 0;
            const bool s3 = stride2 && p.s3;                 // stride in the 3x3: conv1 at the previous resolution, conv2 stride 2
            const bool grouped = p.groups > 1 || s3;          // conv2 on the grouped kernel (grouped_conv.hip)
            SS_CHECK_ARG(wts->conv1_w[bi] && wts->conv1_b[bi] && wts->conv2_w[bi] && wts->conv2_b[bi] && wts->conv3_w[bi] && wts->conv3_b[bi],
                         "encoder_forward: null weights for block %d", bi);
            SS_CHECK_ARG(!first || (wts->down_w[bi] && wts->down_b[bi]), "encoder_forward: block %d needs a projection shortcut", bi);
            float* xin = x;
            if (stride2 && end_done[st - 1]) {
                xin = ws + p.XS;                // (the previous stage's end wrote it)
            } else if (stride2) {
                rc = launch_encoder_subsample2(x, (int64_t)cin * T, 2 * h, 2 * w, ws + p.XS, 0, nullptr, s);
                if (rc) return rc;
                xin = ws + p.XS;
            }
            float* y = (b == p.nblk[st] - 1) ? ws + p.Cst[st] : ((b & 1) ? ws + p.B : ws + p.A);
            // conv2's input: the stage's zero-haloed buffer, or (stride in the 3x3) the one at the previous stage's resolution
            const int h1 = s3 ? 2 * h : h, w1 = s3 ? 2 * w : w;
            float* m1 = ws + (s3 ? p.M1S[st] : p.M1[st]);
            if (!conv1_done) {
                ConvEpilogue e1 = epi_for(T);       // conv1 + bn1 + relu -> zero-haloed 2-D layout (input of the 3x3)
                e1.relu = 1; e1.dec_H = h1; e1.dec_W = w1;
                rc = launch_conv3d(flat_view(s3 ? x : xin, cin, (int64_t)T * h1 * w1), wts->conv1_w[bi], wts->conv1_b[bi], interior2d_view(m1, mid, T, h1, w1), 1, 1,
                                   1, 0, s, ws + p.SK, p.SKfloats, &e1);
                if (rc) return rc;
            }
            // Fused tail (f16x3): conv3 of this block and conv1 of the next in one back-to-back kernel.  conv2 then writes its output as the
            // fp16 operand planes that kernel stages by LDS-DMA (same bytes, the M2 buffer) -- unless its plan splits K, in which case it
            // says so and the block runs its three launches (a function of the planning shape: the same choice for every batch).
            // (only at today's widths: one group, mid x 4 == cout; ResNeXt blocks run their three launches)
            const bool want_fuse = ((desc->fuse_tail >> st) & 1) && prec == STEMSEG_PRECISION_F16X3 && b + 1 < p.nblk[st] && !grouped && p.groups == 1 &&
                                   mid * 4 == cout && fused_tail_supported(mid) && V <= (1ll << 27) && (int64_t)T * (h + 2) * (w + 4) <= (1ll << 27);
            // the stage's end (stage_end_mask: what the descriptor decides of it)
            const bool want_end = st < 3 && b + 1 == p.nblk[st] && lat_ok[st];
            int p16_done = 0;
            if (grouped) {                      // conv2 (grouped and / or stride 2) + bn2 + relu -> dense
                rc = launch_grouped_conv(halo2d_view(m1, mid, T, h1, w1), wts->conv2_w[bi], wts->conv2_b[bi], dense_volume(ws + p.M2, mid, T, h, w), p.groups,
                                         s3 ? 2 : 1, 1, prec, s);
            } else {
                ConvEpilogue e2 = epi_for(T);       // conv2 (3x3) + bn2 + relu -> dense
                e2.relu = 1;
                if (want_fuse) { e2.p16_out = reinterpret_cast<unsigned int*>(ws + p.M2); e2.p16_done = &p16_done; }
                // (the stage's end asks without un-splitting a split plan: where this conv2 splits K the block keeps its launches, and their bits)
                if (want_end) { e2.p16_out = reinterpret_cast<unsigned int*>(ws + p.M2); e2.p16_done = &p16_done; e2.p16_keep_plan = 1; }
                rc = launch_conv3d(halo2d_view(m1, mid, T, h, w), wts->conv2_w[bi], wts->conv2_b[bi], dense_volume(ws + p.M2, mid, T, h, w), 1, 3, 3, 0, s,
                                   ws + p.SK, p.SKfloats, &e2);
            }
            if (rc) return rc;
            const float* idt = xin;
            ConvEpilogue ed = epi_for(T);
            // The shortcut inside the fused tail (bottleneck_fused.hip): the tail computes the shortcut's sums itself from xin -- same operands, k
            // order and rounding steps as the launch below -- and the DS map is neither written nor read.  fuse_tail bit 5 keeps the launch.
            // (stage 2's variant is the one-wave-per-SIMD kernel: not where the form bits ask for the 32-column form)
            const bool ds_in_tail = first && want_fuse && p16_done && !(desc->fuse_tail & 32) && st < 2 && !(st == 1 && ((desc->fuse_tail >> 3) & 3) == 1) &&
                                    fused_shortcut_supported(mid, cin, V);
            if (first && !ds_in_tail) {         // projection shortcut: 1x1 (stride folded into xin) + bn
                rc = launch_conv3d(flat_view(xin, cin, V), wts->down_w[bi], wts->down_b[bi], flat_view(ws + p.DS, cout, V), 1, 1, 1, 0, s, ws + p.SK, p.SKfloats,
                                   &ed);
                if (rc) return rc;
                idt = ws + p.DS;
            }
            if (want_fuse && p16_done) {
                SS_CHECK_ARG(wts->conv1_w[bi + 1] && wts->conv1_b[bi + 1], "encoder_forward: null weights for block %d", bi + 1);
                rc = launch_fused_tail(mid, reinterpret_cast<const unsigned int*>(ws + p.M2), wts->conv3_w[bi], wts->conv3_b[bi], ds_in_tail ? nullptr : idt, y,
                                       wts->conv1_w[bi + 1], wts->conv1_b[bi + 1], interior2d_view(ws + p.M1[st], mid, T, h, w), h, w, V, (desc->fuse_tail >> 3) & 3, s,
                                       ds_in_tail ? xin : nullptr, cin, ds_in_tail ? wts->down_w[bi] : nullptr, ds_in_tail ? wts->down_b[bi] : nullptr);
                if (rc) return rc;
                conv1_done = true;
            } else if (want_end && p16_done) {
                rc = launch_fused_stage_end(mid, reinterpret_cast<const unsigned int*>(ws + p.M2), wts->conv3_w[bi], wts->conv3_b[bi], idt, y, wts->fpn_inner_w[st],
                                            wts->fpn_inner_b[st], ws + p.LAT[st], ws + p.XS, T, h, w, s);
                if (rc) return rc;
                end_done[st] = true;
                conv1_done = false;
            } else {
                ConvEpilogue e3 = epi_for(T);       // conv3 + bn3 + identity + relu
                e3.relu = 1; e3.res = idt; e3.res_cs = V; e3.res_ts = 0; e3.res_ys = 0;
                rc = launch_conv3d(flat_view(ws + p.M2, mid, V), wts->conv3_w[bi], wts->conv3_b[bi], flat_view(y, cout, V), 1, 1, 1, 0, s, ws + p.SK, p.SKfloats, &e3);
                if (rc) return rc;
                conv1_done = false;
            }
            x = y;
            cin = cout;
        }
    }
    // FPN (fpn.py:47-69), coarsest level first
    for (int k = 3; k >= 0; --k) {
        const int h = p.h[k], w = p.w[k];
        ConvEpilogue e = epi_for(T), el = epi_for(T);
        e.dec_H = h; e.dec_W = w;
        // Levels with a top-down term: the lateral conv writes a DENSE map (16-byte epilogue: its by-element epilogue into the zero-haloed layout
        // issued four times the store instructions -- 770 us for the 4x level's 1.7 GB) into the idle block buffer A, and the add pass, which
        // touches every element anyway, writes the zero-haloed layout.  Same tile, same sums: the same bits.
        Padded2D gf0(256, T, h, w);
        const bool lat_dense = k < 3 && up2_form((int64_t)256 * T, h, w, gf0.ts, gf0.pitch, aligned16(ws + p.L[k]), true, aligned16(ws + p.A)) == STEMSEG_UP2_FORM_DENSE;
        const bool lat_stored = k < 3 && end_done[k];      // the stage-end tail left the dense lateral map
        const float* lat_map = lat_stored ? ws + p.LAT[k] : ws + p.A;
        if (lat_dense || lat_stored) {
            if (!lat_stored) {
                ConvEpilogue ed = epi_for(T);
                rc = launch_conv3d(flat_view(ws + p.Cst[k], 256 << k, p.V[k]), wts->fpn_inner_w[k], wts->fpn_inner_b[k], flat_view(ws + p.A, 256, p.V[k]), 1, 1, 1, 0, s,
                                   ws + p.SK, p.SKfloats, &ed);
                if (rc) return rc;
            }
            rc = launch_upsample2x_add(interior2d_view(ws + p.L[k], 256, T, h, w), lat_map, interior2d_view(ws + p.L[k + 1], 256, T, p.h[k + 1], p.w[k + 1]), 0,
                                       nullptr, s);
            if (rc) return rc;
        } else {
        rc = launch_conv3d(flat_view(ws + p.Cst[k], 256 << k, p.V[k]), wts->fpn_inner_w[k], wts->fpn_inner_b[k], interior2d_view(ws + p.L[k], 256, T, h, w), 1, 1, 1, 0, s,
                           ws + p.SK, p.SKfloats, &e);
        if (rc) return rc;
        }
        if (k < 3 && !lat_dense && !lat_stored) {
            // (Measured in round 5 and not kept: the add fused into the lateral conv's epilogue -- four gathered coarse loads per output
            // element in the by-element epilogue of a flat launch.  The separate pass goes (-0.22 ms per clip), the 1x1 class pays +0.38 ms
            // and every tile's kernel arguments grow: the step 103.0 vs 104.8 clips/s, interleaved on one box.)
            rc = launch_upsample2x_add(interior2d_view(ws + p.L[k], 256, T, h, w), nullptr, interior2d_view(ws + p.L[k + 1], 256, T, p.h[k + 1], p.w[k + 1]), 0,
                                       nullptr, s);
            if (rc) return rc;
        }
        // the output conv runs once per clip: each clip's map goes to its own (usually zero-haloed) consumer volume
        const int Tc = desc->clip_frames > 0 ? desc->clip_frames : T / desc->n_clips;
        const int Ts = desc->clip_frames > 0 ? desc->clip_stride : Tc;          // first frame of clip c within the pass: c * Ts
        if (p.FO[k] >= 0) {
            // ... unless the clips overlap: then once over all T frames into a dense map, and every clip copies its window
            // (a shared frame's output conv is not repeated; the copy is 0.1 ms per clip against ~2.3 ms of convs)
            rc = launch_conv3d(halo2d_view(ws + p.L[k], 256, T, h, w), wts->fpn_layer_w[k], wts->fpn_layer_b[k], dense_volume(ws + p.FO[k], 256, T, h, w), 1, 3, 3,
                               0, s, ws + p.SK, p.SKfloats, &el);
            if (rc) return rc;
            for (int c = 0; c < desc->n_clips; ++c) {
                rc = launch_copy_strided(ws + p.FO[k] + (int64_t)c * Ts * h * w, (int64_t)T * h * w, (int64_t)h * w, out[4 * c + k], s);
                if (rc) return rc;
            }
            continue;
        }
        // ... in ONE launch when the clips' consumer volumes lie a fixed stride apart (the decoders' clip batch allocates them so): the clip
        // is a grid dimension of the conv (decided, like every launch of the pass, on the planning shape: same bits either way)
        bool uniform = desc->n_clips > 1 && desc->n_clips <= 65535;
        const int64_t obs = uniform ? out[4 + k].ptr - out[k].ptr : 0;
        for (int c = 1; c < desc->n_clips && uniform; ++c) {
            const StemsegVolume &a = out[4 * c + k], &b = out[k];
            uniform = a.ptr == b.ptr + c * obs && a.c_stride == b.c_stride && a.t_stride == b.t_stride && a.y_stride == b.y_stride && a.limit == b.limit;
        }
        if (uniform && obs > 0 && obs % 4 == 0) {
            StemsegVolume in = halo2d_view(ws + p.L[k], 256, T, h, w);
            ConvEpilogue ec = epi_for(Tc);
            ec.nb = desc->n_clips;
            ec.in_bs = (int64_t)Ts * in.t_stride;
            ec.out_bs = obs;
            in.limit -= (int64_t)(desc->n_clips - 1) * ec.in_bs;        // (the last clip's room: every clip reads Tc frames from its own origin)
            in.T = Tc;
            rc = launch_conv3d(in, wts->fpn_layer_w[k], wts->fpn_layer_b[k], out[k], 1, 3, 3, 0, s, ws + p.SK, p.SKfloats, &ec);
            if (rc) return rc;
            continue;
        }
        for (int c = 0; c < desc->n_clips; ++c) {
            StemsegVolume in = halo2d_view(ws + p.L[k], 256, T, h, w);
            in.ptr += (int64_t)c * Ts * in.t_stride;
            in.limit -= (int64_t)c * Ts * in.t_stride;
            in.T = Tc;
            const ConvEpilogue ec = epi_for(Tc);
            rc = launch_conv3d(in, wts->fpn_layer_w[k], wts->fpn_layer_b[k], out[4 * c + k], 1, 3, 3, 0, s, ws + p.SK, p.SKfloats, &ec);
            if (rc) return rc;
        }
    }
    return STEMSEG_OK;
}
