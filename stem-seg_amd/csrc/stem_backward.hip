// Backward of the stem (resnet.py:285-304): the adjoint of the 3x3 stride-2 max-pool, with the stem's ReLU adjoint in the same pass, and the weight
// gradient of the 7x7 stride-2 convolution.  The convolution's input is the frames, so it has no data gradient; the FrozenBN shift is a buffer, so it
// has no bias gradient.
//
// ---- maxpool3x3s2_backward: dx = the adjoint of max_pool2d(x, 3, 2, 1) applied to g, in the GATHER form: one thread per input pixel (or per 2 x 4 of
// them), no atomics.  An input coordinate lies in one window per axis when it is even (window y / 2) and in two when it is odd (windows (y - 1) / 2 and
// (y + 1) / 2, the second where it exists), so a pixel looks at up to 2 x 2 windows.  For each of them the thread recomputes the window's arg-max with
// torch's rule -- scan the rows, then the columns, of the window clipped to the map; the running value starts as the first element in range and a value v
// replaces it when v > best or v is a NaN: the FIRST maximum wins, the LAST NaN wins -- and adds the window's g where the arg-max is the pixel itself, in
// ascending (oy, ox) order, in fp32, starting from +0: what torch's CPU backward does (a zero-filled map, the windows in order), bit for bit.
// mask_relu: x is the stem's output AFTER its ReLU, and relu_backward's rule (common.h relu_mask) decides between that sum and 0.
//
// ---- stem_wgrad: dw[co][c][ky][kx] = sum over (f, oy, ox) of g[co][f][oy][ox] * frames[f][c][2 oy + ky - 3][2 ox + kx - 3] (0 outside the frame).
// Under the rules at the top of conv_backward.hip: a GEMM with M = 64 output channels, N = 147 = 3 x 7 x 7 taps (padded to 160: five 32-column blocks)
// and K = F Ho Wo on v_mfma_f32_32x32x2_f32 (exact products, fp32 accumulation; never a split mode).  K is cut into chunks whose length is a function
// of (F, H, W) only; a workgroup owns one chunk, writes its fp64 partial [64][147] into the caller's workspace -- every slot by every call -- and a
// second launch adds the chunks in a fixed order -- sixteen runs of consecutive chunks, each in chunk order, then the runs in order -- and rounds once.
// No floating-point atomics, no allocation, no synchronisation.
//
// A K step of a workgroup is a TILE of 4 output rows x 32 output columns of one frame.  It stages g [64][4 x 32] and the frames' patch with its halo,
// 3 colour planes of (2 x 4 + 5) rows x (2 x 32 + 5) columns, zero outside the frame, in LDS: the patch is addressed directly at stride 2 (the
// space-to-depth view of the forward would need a second staged image and four tap classes; here one per-lane offset per column block does it).
// Wave w takes row w of the tile and ALL ten accumulator blocks (2 x 5 x 16 VGPRs): per k-step of two output pixels, 2 A reads and 5 B reads feed 10
// MFMAs.  LDS banks: lane j of a half wave reads tap n = 32 nb + j at offset c PLANE + ky PITCH + kx; with PITCH = 7 and PLANE = 49 mod 32 that offset
// is n mod 32: 32 consecutive taps fall on 32 distinct banks, and the stride-2 pixel offset is common to the half wave.  g's row stride is odd.  A lane
// whose pixel lies beyond the map's last column gets b = 0 against the staged a = 0 (never 0 x a frame value), k-steps and rows that lie beyond the map
// entirely are left out.  The taps 147 .. 159 of the last block read tap 146's address and are never stored.  No fp32 chain is longer than a wave's
// share of a chunk (a quarter of its pixels, at most 128 k-steps: SW_MAX_TILES_PER_CHUNK); the four waves' sums are added in wave order in fp64 through LDS.
#include "common.h"
#include <algorithm>

namespace stemseg {

typedef float sw_f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------------ max-pool backward
// arg-max (*ay, *ax) of window (oy, ox) of plane p [H][W] by torch's rule
__device__ __forceinline__ void pool_window_argmax(const float* __restrict__ p, int H, int W, int oy, int ox, int* ay, int* ax) {
    const int y0 = max(2 * oy - 1, 0), y1 = min(2 * oy + 1, H - 1), x0 = max(2 * ox - 1, 0), x1 = min(2 * ox + 1, W - 1);
    int by = y0, bx = x0;
    float best = p[y0 * W + x0];
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            const float v = p[y * W + x];
            if (v > best || v != v) { best = v; by = y; bx = x; }
        }
    *ay = by; *ax = bx;
}

// Scalar form: one pixel per thread, 64-bit grid-stride indices, any even shape.  The windows of rows oy_lo .. oy_hi x columns ox_lo .. ox_hi are the
// windows the pixel lies in, visited in ascending (oy, ox) order
template <bool MASK>
__global__ __launch_bounds__(256) void maxpool3x3s2_backward_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ dx,
                                                                    int H, int W, int64_t items) {
    const int Ho = H / 2, Wo = W / 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int xb = (int)(i % W);
        int64_t r = i / W;
        const int y = (int)(r % H);
        const int64_t pl = r / H;
        const float* xp = x + pl * H * W;
        const float* gp = g + pl * Ho * Wo;
        const int oy_lo = y >> 1, oy_hi = min((y + 1) >> 1, Ho - 1);
        const int ox_lo = xb >> 1, ox_hi = min((xb + 1) >> 1, Wo - 1);
        float sum = 0.f;
        for (int oy = oy_lo; oy <= oy_hi; ++oy)
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                int ay, ax;
                pool_window_argmax(xp, H, W, oy, ox, &ay, &ax);
                const float gv = gp[oy * Wo + ox];
                if (ay == y && ax == xb) sum = __fadd_rn(sum, gv);
            }
        dx[pl * H * W + (int64_t)y * W + xb] = MASK ? relu_mask(xp[y * W + xb], sum) : sum;
    }
}

// 16-byte form (W % 4 == 0, x and dx 16-byte aligned): one thread = the 2 x 4 pixels of rows 2 m, 2 m + 1 and columns xb .. xb + 3.  They lie in the 2 x 3
// windows (m, m + 1) x (xb / 2 .. xb / 2 + 2) and nowhere else; those windows span input rows 2 m - 1 .. 2 m + 3 and columns xb - 1 .. xb + 5, which the
// thread reads once into registers -- per row one scalar, one 16-byte and one 8-byte load -- 35 values for 8 outputs (the scalar form reads up to 36
// for one).  Each window's arg-max comes from the registers by the same scan -- rows, then columns, positions outside the map skipped, the first
// position in range starts it -- as predicated selects, no branch; a window's g goes to the pixel that is its arg-max when that pixel is one of the
// thread's own (another thread's otherwise).  Windows in ascending (oy, ox) order: the same sums, the same bits as the scalar form.
template <bool MASK>
__global__ __launch_bounds__(256) void maxpool3x3s2_backward_vec4_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ dx,
                                                                         int H, int W, int64_t items) {
    const int Ho = H / 2, Wo = W / 2, WQ = W / 4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int xb = (int)(i % WQ) * 4;
        int64_t r = i / WQ;
        const int m = (int)(r % Ho);
        const int64_t pl = r / Ho;
        const float* xp = x + pl * H * W;
        const float* gp = g + pl * Ho * Wo;
        const bool left = xb > 0, right = xb + 4 < W;        // columns xb - 1 and xb + 4, xb + 5 exist
        float v[5][7];
        bool rv[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int iy = 2 * m - 1 + k;
            rv[k] = iy >= 0 && iy < H;
#pragma unroll
            for (int c = 0; c < 7; ++c) v[k][c] = 0.f;
            if (rv[k]) {
                const float* row = xp + (int64_t)iy * W + xb;
                const float4 q = *reinterpret_cast<const float4*>(row);
                v[k][1] = q.x; v[k][2] = q.y; v[k][3] = q.z; v[k][4] = q.w;
                if (left) v[k][0] = row[-1];
                if (right) {
                    const float2 t = *reinterpret_cast<const float2*>(row + 4);
                    v[k][5] = t.x; v[k][6] = t.y;
                }
            }
        }
        float sum[2][4];
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 4; ++px) sum[py][px] = 0.f;
#pragma unroll
        for (int wy = 0; wy < 2; ++wy)
#pragma unroll
            for (int wx = 0; wx < 3; ++wx) {
                if (m + wy >= Ho || (wx == 2 && !right)) continue;             // the window does not exist
                int a = -1;                                  // the arg-max as 7 (row in v) + (column in v); -1: nothing taken yet
                float best = 0.f;
#pragma unroll
                for (int dr = 0; dr < 3; ++dr)
#pragma unroll
                    for (int dc = 0; dc < 3; ++dc) {
                        const int rr = 2 * wy + dr, cc = 2 * wx + dc;
                        const bool valid = rv[rr] && (cc == 0 ? left : cc >= 5 ? right : true);
                        const float val = v[rr][cc];
                        const bool take = valid && (a < 0 || val > best || val != val);
                        best = take ? val : best;
                        a = take ? rr * 7 + cc : a;
                    }
                const float gv = gp[(m + wy) * Wo + (xb >> 1) + wx];
#pragma unroll
                for (int py = 0; py < 2; ++py)
#pragma unroll
                    for (int px = 0; px < 4; ++px)
                        if (a == (py + 1) * 7 + px + 1) sum[py][px] = __fadd_rn(sum[py][px], gv);
            }
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            if (MASK) {
#pragma unroll
                for (int px = 0; px < 4; ++px) sum[py][px] = relu_mask(v[py + 1][px + 1], sum[py][px]);
            }
            *reinterpret_cast<float4*>(dx + pl * H * W + (int64_t)(2 * m + py) * W + xb) = make_float4(sum[py][0], sum[py][1], sum[py][2], sum[py][3]);
        }
    }
}

static int launch_maxpool3x3s2_backward(const float* x, const float* g, int64_t planes, int H, int W, int mask_relu, float* dx, int form, int* form_used,
                                        hipStream_t s) {
    const char* who = "maxpool3x3s2_backward";
    SS_CHECK_ARG(x && g && dx, "%s: null pointer", who);
    SS_CHECK_ARG(planes >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && (int64_t)H * W < (1ll << 31) && planes <= (1ll << 40) / ((int64_t)H * W),
                 "%s: planes=%lld H=%d W=%d (H, W even)", who, (long long)planes, H, W);
    SS_CHECK_ARG(mask_relu == 0 || mask_relu == 1, "%s: mask_relu=%d", who, mask_relu);
    SS_CHECK_ARG(form == STEMSEG_STREAM_FORM_AUTO || form == STEMSEG_STREAM_FORM_SCALAR || form == STEMSEG_STREAM_FORM_VEC4, "%s: form=%d", who, form);
    const bool aligned = reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(dx) % 16 == 0;
    const int own = (W % 4 == 0 && aligned) ? STEMSEG_STREAM_FORM_VEC4 : STEMSEG_STREAM_FORM_SCALAR;
    SS_CHECK_ARG(form != STEMSEG_STREAM_FORM_VEC4 || own == STEMSEG_STREAM_FORM_VEC4, "%s: the 16-byte form needs W %% 4 == 0 (W=%d) and 16-byte aligned x and dx",
                 who, W);
    const int used = form ? form : own;
    const bool vec = used == STEMSEG_STREAM_FORM_VEC4;
    const int64_t items = vec ? planes * (H / 2) * (W / 4) : planes * H * W;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, 256), 256 * 64))), block(256);
    if (vec) {
        if (mask_relu) hipLaunchKernelGGL(maxpool3x3s2_backward_vec4_kernel<true>, grid, block, 0, s, x, g, dx, H, W, items);
        else hipLaunchKernelGGL(maxpool3x3s2_backward_vec4_kernel<false>, grid, block, 0, s, x, g, dx, H, W, items);
    } else {
        if (mask_relu) hipLaunchKernelGGL(maxpool3x3s2_backward_kernel<true>, grid, block, 0, s, x, g, dx, H, W, items);
        else hipLaunchKernelGGL(maxpool3x3s2_backward_kernel<false>, grid, block, 0, s, x, g, dx, H, W, items);
    }
    SS_LAUNCH_CHECK();
    if (form_used) *form_used = used;
    return STEMSEG_OK;
}

// ------------------------------------------------------------------------------------------------ stem weight gradient
constexpr int SW_CO = 64, SW_TAPS = 147, SW_NB = 5;           // 5 x 32 = 160 columns, 147 of them taps
constexpr int SW_TR = 4, SW_TC = 32, SW_TILE = SW_TR * SW_TC; // the tile: 4 output rows (one per wave) x 32 output columns
constexpr int SW_G_STRIDE = SW_TILE + 1;                      // odd: 32 channels at one pixel fall on 32 banks
constexpr int SW_PR = 2 * SW_TR + 5, SW_PC = 2 * SW_TC + 5;   // the patch: 13 rows x 69 columns per colour plane
constexpr int SW_PITCH = 71;                                  // >= 69, = 7 mod 32
constexpr int SW_PLANE = 945;                                 // >= 13 x 71 = 923, = 49 mod 32
constexpr int SW_G_FLOATS = SW_CO * SW_G_STRIDE, SW_P_FLOATS = 3 * SW_PLANE;
constexpr int SW_RED_FLOATS = 2 * SW_NB * 16 * 64;            // the cross-wave sum of one 32-channel half: 5 x 16 x 64 doubles, over the staged tile
constexpr int SW_LDS_FLOATS = SW_G_FLOATS + SW_P_FLOATS > SW_RED_FLOATS ? SW_G_FLOATS + SW_P_FLOATS : SW_RED_FLOATS;
constexpr int SW_MIN_TILES_PER_CHUNK = 4;                     // 512 pixels behind a chunk's 64 x 147 doubles
constexpr int SW_MAX_TILES_PER_CHUNK = 8;                     // a wave's fp32 chain: at most 8 x 16 k-steps = 256 products, whatever the shape
constexpr int SW_TARGET_WORKGROUPS = 1024;
constexpr int64_t SW_N_DW = (int64_t)SW_CO * SW_TAPS;
static_assert(SW_PITCH % 32 == 7 && SW_PITCH >= SW_PC && SW_PLANE % 32 == 49 % 32 && SW_PLANE >= SW_PR * SW_PITCH, "the bank layout of the patch");

struct StemWgradPlan {
    int Ho, Wo, tiles_x, tiles_y, ntiles, tiles_per_chunk, nchunks;
    size_t bytes;
};

struct StemWgradParams {
    const float* frames;                                      // [F][3][H][W]
    const float* g;                                           // [64][F][Ho][Wo]
    double* part;                                             // [chunk][64][147]
    int F, H, W, Ho, Wo, tiles_x, tiles_y, ntiles, tiles_per_chunk;
};

__global__ __launch_bounds__(256, 2) void stem_wgrad_kernel(StemWgradParams p) {
    __shared__ __attribute__((aligned(16))) float lds[SW_LDS_FLOATS];
    float* const gs = lds;                                   // g [64][4 x 32]
    float* const ps = lds + SW_G_FLOATS;                     // the patch [3][13][69] at pitch 71, plane 945
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int chunk = blockIdx.x;
    const int64_t HoWo = (int64_t)p.Ho * p.Wo, HW = (int64_t)p.H * p.W;

    sw_f32x16 acc[2][SW_NB];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nb = 0; nb < SW_NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][nb][r] = 0.f;
    // the lane's tap of each column block: its offset inside the patch
    int boff[SW_NB];
#pragma unroll
    for (int nb = 0; nb < SW_NB; ++nb) {
        const int n = min(nb * 32 + l31, SW_TAPS - 1), c = n / 49, k = n - 49 * c, ky = k / 7, kx = k - 7 * ky;
        boff[nb] = c * SW_PLANE + ky * SW_PITCH + kx;
    }

    const int tile_beg = chunk * p.tiles_per_chunk, tile_end = min(tile_beg + p.tiles_per_chunk, p.ntiles);
    for (int tile = tile_beg; tile < tile_end; ++tile) {
        const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, f = tile / (p.tiles_x * p.tiles_y);
        const int ox0 = tx * SW_TC, oy0 = ty * SW_TR;
        const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
        __syncthreads();                                     // the previous tile's reads are done
#pragma unroll 8
        for (int i = tid; i < SW_CO * SW_TILE; i += 256) {   // g: consecutive threads along x
            const int col = i & (SW_TC - 1), row = (i >> 5) & (SW_TR - 1), co = i >> 7;
            const int oy = oy0 + row, ox = ox0 + col;
            float v = 0.f;
            if (oy < p.Ho && ox < p.Wo) v = p.g[((int64_t)co * p.F + f) * HoWo + (int64_t)oy * p.Wo + ox];
            gs[co * SW_G_STRIDE + row * SW_TC + col] = v;
        }
        const float* fr = p.frames + (int64_t)f * 3 * HW;
        for (int i = tid; i < 3 * SW_PR * SW_PC; i += 256) {
            const int col = i % SW_PC, r = i / SW_PC, row = r % SW_PR, c = r / SW_PR;
            const int iy = iy0 + row, ix = ix0 + col;
            float v = 0.f;
            if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) v = fr[(int64_t)c * HW + (int64_t)iy * p.W + ix];
            ps[c * SW_PLANE + row * SW_PITCH + col] = v;
        }
        __syncthreads();
        if (oy0 + wave < p.Ho) {                             // (wave-uniform) a row beyond the map: g is 0 there
            const int cols_in = min(SW_TC, p.Wo - ox0);
            const int nsteps = (cols_in + 1) / 2;            // k-step s: output columns 2 s and 2 s + 1 of the wave's row
            const float* a_row = gs + l31 * SW_G_STRIDE + wave * SW_TC + half;
            const float* b_row = ps + 2 * wave * SW_PITCH + 2 * half;
            float a[2], b[SW_NB], an[2], bn[SW_NB];
            auto ld = [&](const int s, float (&av)[2], float (&bv)[SW_NB]) __attribute__((always_inline)) {
                const bool in = 2 * s + half < cols_in;
                av[0] = a_row[2 * s];
                av[1] = a_row[32 * SW_G_STRIDE + 2 * s];
#pragma unroll
                for (int nb = 0; nb < SW_NB; ++nb) {
                    const float v = b_row[boff[nb] + 4 * s];
                    bv[nb] = in ? v : 0.f;
                }
            };
            ld(0, a, b);
            for (int s = 0; s < nsteps; ++s) {
                ld(min(s + 1, nsteps - 1), an, bn);          // the next k-step's operands are on their way while this one's MFMAs issue
#pragma unroll
                for (int nb = 0; nb < SW_NB; ++nb) {
                    acc[0][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[nb], acc[0][nb], 0, 0, 0);
                    acc[1][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[nb], acc[1][nb], 0, 0, 0);
                }
                a[0] = an[0]; a[1] = an[1];
#pragma unroll
                for (int nb = 0; nb < SW_NB; ++nb) b[nb] = bn[nb];
            }
        }
    }
    // the four waves' sums in wave order, one 32-channel half at a time.  C/D map of the 32x32 MFMA: column = lane & 31 (the tap), row = (r & 3) + 8 (r >> 2) +
    // 4 (lane >> 5) (the output channel)
    double* red = reinterpret_cast<double*>(lds);
    double* pc = p.part + (int64_t)chunk * SW_N_DW;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        for (int w = 0; w < 4; ++w) {
            __syncthreads();                                 // the last tile's reads (and the previous half's) are done
            if (wave == w) {
#pragma unroll
                for (int nb = 0; nb < SW_NB; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        double* slot = red + (nb * 16 + r) * 64 + lane;
                        const double v = (double)acc[mi][nb][r];
                        if (w == 0) {
                            *slot = v;
                        } else if (w < 3) {
                            *slot += v;
                        } else {
                            const int n = nb * 32 + l31, co = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                            if (n < SW_TAPS) pc[(int64_t)co * SW_TAPS + n] = *slot + v;
                        }
                    }
            }
        }
    }
}

// The slots [co][tap] lie as torch lays the weight [64][3][7][7].  The chunks are cut into SW_RUNS runs of consecutive chunks (a run's length a function
// of the chunk count only): 16 threads per slot add one run each in chunk order, the 16 sums are added in run order, and the result is rounded once.  (A
// thread alone per slot walks hundreds of chunks 75 kB apart: a chain of dependent latencies that made up most of the call.)
constexpr int SW_RUNS = 16, SW_SLOTS_PER_BLOCK = 256 / SW_RUNS;
__global__ __launch_bounds__(256) void stem_wgrad_combine_kernel(const double* __restrict__ part, int nchunks, float* __restrict__ dw) {
    __shared__ double runs[SW_RUNS][SW_SLOTS_PER_BLOCK];
    const int sl = threadIdx.x & (SW_SLOTS_PER_BLOCK - 1), run = threadIdx.x / SW_SLOTS_PER_BLOCK;
    const int64_t i = (int64_t)blockIdx.x * SW_SLOTS_PER_BLOCK + sl;              // (9408 slots = 588 blocks of 16: no ragged block)
    const int per = (nchunks + SW_RUNS - 1) / SW_RUNS, k0 = run * per, k1 = min(k0 + per, nchunks);
    double s = 0.0;
#pragma unroll 4
    for (int k = k0; k < k1; ++k) s += part[(int64_t)k * SW_N_DW + i];
    runs[run][sl] = s;
    __syncthreads();
    if (run == 0) {
        double t = runs[0][sl];
#pragma unroll
        for (int r = 1; r < SW_RUNS; ++r) t += runs[r][sl];
        dw[i] = (float)t;
    }
}
static_assert(SW_N_DW % SW_SLOTS_PER_BLOCK == 0, "the combine's blocks hold whole slots");

// Chunk length: a function of (F, H, W) only.  As many chunks as bring the launch to about SW_TARGET_WORKGROUPS workgroups, none shorter than
// SW_MIN_TILES_PER_CHUNK tiles (the last one aside) and none longer than SW_MAX_TILES_PER_CHUNK: beyond 8192 tiles the launch grows instead of the
// chains.  (The tests hold chains of up to 64 k-steps to their fp64 bound; the 112 of F = 8 on 480 x 864 lay 5e-7 of max|dw| from stock torch's
// result, tools/stem_backward_bench.py.  The 1-tap kernel of conv_backward.hip, whose chunk-long chains sat at its bound, had 256 and more k-steps.)
static int stem_wgrad_plan(int F, int H, int W, StemWgradPlan& pl) {
    SS_CHECK_ARG(F >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "stem_wgrad: F=%d H=%d W=%d (H, W even)", F, H, W);
    SS_CHECK_ARG((int64_t)F * 3 * H * W < (1ll << 31), "stem_wgrad: F=%d H=%d W=%d: more than 2^31 frame elements", F, H, W);
    pl.Ho = H / 2; pl.Wo = W / 2;
    pl.tiles_x = (int)ceil_div(pl.Wo, SW_TC);
    pl.tiles_y = (int)ceil_div(pl.Ho, SW_TR);
    pl.ntiles = F * pl.tiles_x * pl.tiles_y;
    pl.tiles_per_chunk = (int)std::min<int64_t>(SW_MAX_TILES_PER_CHUNK, std::max<int64_t>(SW_MIN_TILES_PER_CHUNK, ceil_div(pl.ntiles, SW_TARGET_WORKGROUPS)));
    pl.nchunks = (int)ceil_div(pl.ntiles, pl.tiles_per_chunk);
    pl.bytes = (size_t)pl.nchunks * (size_t)SW_N_DW * sizeof(double);
    return STEMSEG_OK;
}

}  // namespace stemseg

using namespace stemseg;

extern "C" int stemseg_hip_maxpool3x3s2_backward(const float* x, const float* g, int64_t planes, int32_t H, int32_t W, int32_t mask_relu, float* dx,
                                                 int32_t form, int32_t* form_used, void* stream) {
    return launch_maxpool3x3s2_backward(x, g, planes, H, W, mask_relu, dx, form, form_used, as_stream(stream));
}

extern "C" size_t stemseg_hip_stem_wgrad_workspace_bytes(int32_t F, int32_t H, int32_t W) {
    StemWgradPlan pl;
    return stem_wgrad_plan(F, H, W, pl) == STEMSEG_OK ? pl.bytes : 0;
}

extern "C" int stemseg_hip_stem_wgrad_chunks(int32_t F, int32_t H, int32_t W) {
    StemWgradPlan pl;
    const int rc = stem_wgrad_plan(F, H, W, pl);
    return rc == STEMSEG_OK ? pl.nchunks : rc;
}

extern "C" int stemseg_hip_stem_wgrad(const float* frames, const float* g, int32_t F, int32_t H, int32_t W, float* dw, void* workspace, size_t ws_bytes,
                                      void* stream) {
    SS_CHECK_ARG(frames, "stem_wgrad: frames is a null pointer");
    SS_CHECK_ARG(g, "stem_wgrad: g is a null pointer");
    SS_CHECK_ARG(dw, "stem_wgrad: dw is a null pointer");
    SS_CHECK_ARG(workspace, "stem_wgrad: workspace is a null pointer");
    StemWgradPlan pl;
    const int rc = stem_wgrad_plan(F, H, W, pl);
    if (rc) return rc;
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "stem_wgrad: workspace must be 256-byte aligned");
    if (ws_bytes < pl.bytes) {
        set_error("stem_wgrad: workspace too small (%zu < %zu bytes)", ws_bytes, pl.bytes);
        return STEMSEG_E_WORKSPACE;
    }
    StemWgradParams p;
    p.frames = frames; p.g = g; p.part = reinterpret_cast<double*>(workspace);
    p.F = F; p.H = H; p.W = W; p.Ho = pl.Ho; p.Wo = pl.Wo;
    p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.ntiles = pl.ntiles; p.tiles_per_chunk = pl.tiles_per_chunk;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3((unsigned)pl.nchunks), dim3(256), 0, s, p);
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(stem_wgrad_combine_kernel, dim3((unsigned)(SW_N_DW / SW_SLOTS_PER_BLOCK)), dim3(256), 0, s, (const double*)p.part, pl.nchunks, dw);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
