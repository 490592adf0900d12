// Backward of the decoders' 3x3x3 convolution (padding 1, stride 1): the weight and bias gradients, and the tap gather of the data gradient
// (hip.py conv3d_dgrad: the per-tap products are one 1x1x1 convolution on the forward kernel; conv3d_col2vol_kernel below sums them).
//
//     dW[co][ci][kt][ky][kx] = sum over (t, y, x) of dy[co][t, y, x] * x[ci][t + kt, y + ky, x + kx]      (x in haloed coordinates)
//     db[co] = sum dy[co]
//
// a GEMM with M = Cout, N = 27 Cin, K = T H W, on v_mfma_f32_32x32x2_f32 (exact products, fp32 accumulation: the library's "f32"
// arithmetic; gradients have no bounded magnitude, so the scaled fp16 split of the forward is not an option here).  The rules of
// decoder_backward.hip hold: K is cut into chunks whose length is a function of the shape only, a workgroup accumulates its chunk in fp32
// and writes fp64 partials into the caller's workspace -- every slot by every call -- and a second launch adds the chunks in chunk order and
// rounds once.  No floating-point atomics, no allocation, no synchronisation; two runs give the same bits.
#include "common.h"
#include <algorithm>

namespace stemseg {

typedef float wg_f32x16 __attribute__((ext_vector_type(16)));

// A K step of a workgroup is a TILE of 64 output voxels of one plane t: RY rows x XS columns, XS = 8 .. 64 by the map's width (RY = 64 / XS).
// The workgroup owns 128 output channels (wave w the 32 from 32 w), 32 input channels and one kt; per tile it stages dy [128][64] and the
// x halo tile [32][RY + 2][XS + 2] of plane t + kt in LDS, which serves all nine in-plane taps: 9 x 16 accumulator VGPRs per wave.  x is
// zero-haloed, so no tap needs a bounds test; what a tile holds beyond the map (rows >= H, columns >= W) is staged as zeros, and the
// k-steps that lie there entirely are left out (they add exact zeros).  Both LDS channel strides are odd: the 32 lanes of a half wave
// read 32 channels at one voxel, bank = channel stride x channel mod 32.
constexpr int WG_TILE = 64;
constexpr int WG_CO = 128, WG_CI = 32;
constexpr int WG_DY_STRIDE = WG_TILE + 1;
constexpr int WG_X_FLOATS = WG_CI * 199;                      // XS = 64: 3 rows x 66 columns = 198 -> 199; every other tile shape is smaller
constexpr int WG_MIN_TILES_PER_CHUNK = 8;                     // a chunk's partials are 27 x 128 x 32 doubles per workgroup: at least 512 voxels behind them
constexpr int WG_TARGET_WORKGROUPS = 1024;
constexpr int WG_MAX_CHUNKS = 64;
constexpr size_t WG_MAX_PARTIAL_BYTES = size_t(256) << 20;    // chunks are fewer where Cout x Cin is large

struct WgradPlan {
    int xs_log2, tiles_x, tiles_y, ntiles, tiles_per_chunk, nchunks, x_cs;
    int64_t n_dw;                                             // 27 Cout Cin
    size_t bytes;
};

struct WgradParams {
    const float* x;
    int64_t x_cs, x_ts, x_ys;
    const float* dy;
    double* part;                                             // [chunk][27][Cout][Cin]
    double* part_b;                                           // [chunk][Cout]
    int Cin, Cout, T, H, W;
    int xs_log2, tiles_x, tiles_y, ntiles, tiles_per_chunk, lds_cs;
    int64_t n_dw;
};

__global__ __launch_bounds__(256, 2) void conv3d_wgrad_kernel(WgradParams p) {
    __shared__ float xs[WG_X_FLOATS];
    __shared__ float dys[WG_CO * WG_DY_STRIDE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int chunk = blockIdx.x;
    const int kt = blockIdx.y % 3, ci0 = (blockIdx.y / 3) * WG_CI, co0 = blockIdx.z * WG_CO;
    const int XS = 1 << p.xs_log2, RY = WG_TILE >> p.xs_log2, XSH = XS + 2, RYH = RY + 2, n_halo = RYH * XSH;
    const bool wave_on = co0 + wave * 32 < p.Cout;            // (Cout % 32 == 0: a wave's 32 channels exist together)
    const bool do_b = blockIdx.y == 0;
    const int64_t HW = (int64_t)p.H * p.W;

    wg_f32x16 acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    double accb = 0.0;

    const int tile_beg = chunk * p.tiles_per_chunk, tile_end = min(tile_beg + p.tiles_per_chunk, p.ntiles);
    for (int tile = tile_beg; tile < tile_end; ++tile) {
        const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, t = tile / (p.tiles_x * p.tiles_y);
        const int x0 = tx * XS, y0 = ty * RY;
        __syncthreads();                                     // the previous tile's reads are done
        // dy [128][64]: consecutive threads along x
        for (int i = tid; i < WG_CO * WG_TILE; i += 256) {
            const int j = i & (WG_TILE - 1), col = i >> 6;
            const int y = y0 + (j >> p.xs_log2), x = x0 + (j & (XS - 1)), co = co0 + col;
            float v = 0.f;
            if (co < p.Cout && y < p.H && x < p.W) v = p.dy[((int64_t)co * p.T + t) * HW + (int64_t)y * p.W + x];
            dys[col * WG_DY_STRIDE + j] = v;
        }
        // x halo tile of plane t + kt: a wave stages 8 of the 32 channels
        for (int k = 0; k < 8; ++k) {
            const int cl = wave * 8 + k, ci = ci0 + cl;
            const float* xc = p.x + (int64_t)ci * p.x_cs + (int64_t)(t + kt) * p.x_ts;
            for (int r = lane; r < n_halo; r += 64) {
                const int row = r / XSH, c = r - row * XSH;
                const int hy = y0 + row, hx = x0 + c;
                float v = 0.f;
                if (ci < p.Cin && hy < p.H + 2 && hx < p.W + 2) v = xc[(int64_t)hy * p.x_ys + hx];
                xs[cl * p.lds_cs + r] = v;
            }
        }
        __syncthreads();
        if (do_b) {                                          // bias: thread pair per output channel, 32 voxels each
            const float* row = dys + (tid >> 1) * WG_DY_STRIDE + (tid & 1) * 32;
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 32; ++i) s += row[i];
            accb += (double)s;
        }
        if (wave_on) {
            const int rows_in = min(RY, p.H - y0), cols_in = min(XS, p.W - x0);
            const float* a_row = dys + (wave * 32 + (lane & 31)) * WG_DY_STRIDE + (lane >> 5);
            const float* b_ch = xs + (lane & 31) * p.lds_cs + (lane >> 5);
#pragma unroll 2
            for (int s = 0; s < WG_TILE / 2; ++s) {          // k-step: voxels 2 s and 2 s + 1 of the tile (one row: XS is even)
                const int j = 2 * s, ry = j >> p.xs_log2, xx = j & (XS - 1);
                if (ry >= rows_in || xx >= cols_in) continue;                    // (wave-uniform) both voxels beyond the map: dy is 0 there
                const float a = a_row[j];
                const float* b = b_ch + ry * XSH + xx;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
                        acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[ky * XSH + kx], acc[ky * 3 + kx], 0, 0, 0);
            }
        }
    }
    // the chunk's partials.  C/D map of the 32x32 MFMA: column = lane & 31 (the input channel), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    if (wave_on) {
        const int ci = ci0 + (lane & 31);
        if (ci < p.Cin) {
            double* pc = p.part + (int64_t)chunk * p.n_dw + (int64_t)kt * 9 * p.Cout * p.Cin;
#pragma unroll
            for (int j = 0; j < 9; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    pc[((int64_t)j * p.Cout + co) * p.Cin + ci] = (double)acc[j][r];
                }
        }
    }
    if (do_b) {
        accb += __shfl_xor(accb, 1, 64);
        const int co = co0 + (tid >> 1);
        if ((tid & 1) == 0 && co < p.Cout) p.part_b[(int64_t)chunk * p.Cout + co] = accb;
    }
}

// one thread per slot (tap, co, ci), ci fastest as the partials lie: the chunks in chunk order, rounded once -> dw in torch's layout
// [Cout][Cin][27]; the threads behind them the bias slots
__global__ __launch_bounds__(256) void conv3d_wgrad_combine_kernel(const double* __restrict__ part, const double* __restrict__ part_b, int nchunks,
                                                                   int Cout, int Cin, int64_t n_dw, float* __restrict__ dw, float* __restrict__ db) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_dw) {
        double s = 0.0;
        for (int k = 0; k < nchunks; ++k) s += part[(int64_t)k * n_dw + i];
        const int ci = (int)(i % Cin);
        const int64_t r = i / Cin;
        const int co = (int)(r % Cout), tap = (int)(r / Cout);
        dw[((int64_t)co * Cin + ci) * 27 + tap] = (float)s;
    } else if (i < n_dw + Cout && db) {
        const int co = (int)(i - n_dw);
        double s = 0.0;
        for (int k = 0; k < nchunks; ++k) s += part_b[(int64_t)k * Cout + co];
        db[co] = (float)s;
    }
}

// The data gradient's second half.  dX[ci][u] = sum over taps k of O_k[ci][u - k + 1], O_k = W_k^T dy the per-tap products (one 1x1x1
// convolution with 27 Cin output channels: Cout terms each): one thread per input voxel gathers its (at most) 27 taps in tap order, in
// fp64, and rounds once.  Summing the taps here instead of in the convolution's fp32 accumulator keeps 27 Cout-term sums apart.
__global__ __launch_bounds__(256) void conv3d_col2vol_kernel(const float* __restrict__ cols, int Cin, int T, int H, int W, float* __restrict__ dx) {
    const int64_t HW = (int64_t)H * W, per_c = (int64_t)T * HW, total = per_c * Cin;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i / per_c);
        int64_t r = i - (int64_t)ci * per_c;
        const int t = (int)(r / HW);
        r -= (int64_t)t * HW;
        const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
        double acc = 0.0;
        for (int kt = 0; kt < 3; ++kt) {
            const int vt = t - kt + 1;
            if (vt < 0 || vt >= T) continue;
            for (int ky = 0; ky < 3; ++ky) {
                const int vy = y - ky + 1;
                if (vy < 0 || vy >= H) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    const int vx = x - kx + 1;
                    if (vx < 0 || vx >= W) continue;
                    const int k = (kt * 3 + ky) * 3 + kx;
                    acc += (double)cols[((int64_t)k * Cin + ci) * per_c + (int64_t)vt * HW + (int64_t)vy * W + vx];
                }
            }
        }
        dx[i] = (float)acc;
    }
}

// Tile shape and chunk length: functions of (Cin, Cout, T, H, W) only.  As many chunks as bring the launch to about WG_TARGET_WORKGROUPS
// workgroups, at most WG_MAX_CHUNKS and at most what WG_MAX_PARTIAL_BYTES of partials hold, and no chunk shorter than
// WG_MIN_TILES_PER_CHUNK tiles (the last one aside).
static int wgrad_plan(int Cin, int Cout, int T, int H, int W, WgradPlan& pl) {
    SS_CHECK_ARG(Cin > 0 && Cin % 4 == 0 && Cout > 0 && Cout % 32 == 0, "conv3d_wgrad: Cin %% 4 == 0 and Cout %% 32 == 0 required (Cin=%d, Cout=%d)", Cin,
                 Cout);
    SS_CHECK_ARG(Cin <= 4096 && Cout <= 4096, "conv3d_wgrad: at most 4096 channels (Cin=%d, Cout=%d)", Cin, Cout);
    SS_CHECK_ARG(T > 0 && H > 0 && W > 0 && (int64_t)T * H * W < (1ll << 30), "conv3d_wgrad: bad dims (T=%d, H=%d, W=%d)", T, H, W);
    pl.xs_log2 = W <= 8 ? 3 : W <= 16 ? 4 : W <= 32 ? 5 : 6;
    const int XS = 1 << pl.xs_log2, RY = WG_TILE / XS;
    pl.tiles_x = (int)ceil_div(W, XS);
    pl.tiles_y = (int)ceil_div(H, RY);
    pl.ntiles = T * pl.tiles_x * pl.tiles_y;
    pl.x_cs = ((RY + 2) * (XS + 2)) | 1;
    pl.n_dw = (int64_t)27 * Cout * Cin;
    const int64_t slot_bytes = (pl.n_dw + Cout) * (int64_t)sizeof(double);
    const int64_t base = ceil_div(Cout, WG_CO) * ceil_div(Cin, WG_CI) * 3;
    int64_t want = std::min<int64_t>(ceil_div(WG_TARGET_WORKGROUPS, base), WG_MAX_CHUNKS);
    want = std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)WG_MAX_PARTIAL_BYTES / slot_bytes));
    pl.tiles_per_chunk = (int)std::max<int64_t>(WG_MIN_TILES_PER_CHUNK, ceil_div(pl.ntiles, want));
    pl.nchunks = (int)ceil_div(pl.ntiles, pl.tiles_per_chunk);
    pl.bytes = (size_t)pl.nchunks * (size_t)slot_bytes;
    return STEMSEG_OK;
}

}  // namespace stemseg

using namespace stemseg;

extern "C" size_t stemseg_hip_conv3d_wgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t T, int32_t H, int32_t W) {
    WgradPlan pl;
    return wgrad_plan(Cin, Cout, T, H, W, pl) == STEMSEG_OK ? pl.bytes : 0;
}

extern "C" int stemseg_hip_conv3d_wgrad_chunks(int32_t Cin, int32_t Cout, int32_t T, int32_t H, int32_t W) {
    WgradPlan pl;
    const int rc = wgrad_plan(Cin, Cout, T, H, W, pl);
    return rc == STEMSEG_OK ? pl.nchunks : rc;
}

extern "C" int stemseg_hip_conv3d_wgrad(const StemsegVolume* x_haloed, const float* dy, int32_t Cout, float* dw, float* db, void* workspace,
                                        size_t ws_bytes, void* stream) {
    SS_CHECK_ARG(x_haloed && x_haloed->ptr && dy && dw && workspace, "conv3d_wgrad: null pointer");
    const StemsegVolume& x = *x_haloed;
    SS_CHECK_ARG(x.T >= 3 && x.H >= 3 && x.W >= 3, "conv3d_wgrad: x must be the haloed view (T + 2, H + 2, W + 2), got (%d, %d, %d)", x.T, x.H, x.W);
    const int Cin = x.C, T = x.T - 2, H = x.H - 2, W = x.W - 2;
    WgradPlan pl;
    const int rc = wgrad_plan(Cin, Cout, T, H, W, pl);
    if (rc) return rc;
    SS_CHECK_ARG(x.y_stride >= x.W && x.t_stride >= (int64_t)x.H * x.y_stride && x.c_stride >= (int64_t)x.T * x.t_stride,
                 "conv3d_wgrad: the strides of x do not hold its extents");
    SS_CHECK_ARG(x.limit >= (int64_t)(Cin - 1) * x.c_stride + (int64_t)(x.T - 1) * x.t_stride + (int64_t)(x.H - 1) * x.y_stride + x.W,
                 "conv3d_wgrad: the view of x reaches past its limit");
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "conv3d_wgrad: workspace must be 256-byte aligned");
    if (ws_bytes < pl.bytes) {
        set_error("conv3d_wgrad: workspace too small (%zu < %zu bytes)", ws_bytes, pl.bytes);
        return STEMSEG_E_WORKSPACE;
    }
    WgradParams p;
    p.x = x.ptr; p.x_cs = x.c_stride; p.x_ts = x.t_stride; p.x_ys = x.y_stride;
    p.dy = dy;
    p.part = reinterpret_cast<double*>(workspace);
    p.part_b = p.part + (int64_t)pl.nchunks * pl.n_dw;
    p.Cin = Cin; p.Cout = Cout; p.T = T; p.H = H; p.W = W;
    p.xs_log2 = pl.xs_log2; p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.ntiles = pl.ntiles; p.tiles_per_chunk = pl.tiles_per_chunk;
    p.lds_cs = pl.x_cs; p.n_dw = pl.n_dw;
    hipStream_t s = as_stream(stream);
    void* ev = profile_begin(53, 2.0 * 27.0 * (double)Cout * Cin * T * H * W, s);
    const dim3 grid((unsigned)pl.nchunks, (unsigned)(ceil_div(Cin, WG_CI) * 3), (unsigned)ceil_div(Cout, WG_CO));
    hipLaunchKernelGGL(conv3d_wgrad_kernel, grid, dim3(256), 0, s, p);
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(conv3d_wgrad_combine_kernel, dim3((unsigned)ceil_div(pl.n_dw + Cout, 256)), dim3(256), 0, s, (const double*)p.part,
                       (const double*)p.part_b, pl.nchunks, Cout, Cin, pl.n_dw, dw, db);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_conv3d_col2vol(const float* cols, int32_t Cin, int32_t T, int32_t H, int32_t W, float* dx, void* stream) {
    SS_CHECK_ARG(cols && dx, "conv3d_col2vol: null pointer");
    SS_CHECK_ARG(Cin > 0 && T > 0 && H > 0 && W > 0 && (int64_t)27 * Cin * T * H * W < (1ll << 40), "conv3d_col2vol: bad dims");
    const int64_t total = (int64_t)Cin * T * H * W;
    hipLaunchKernelGGL(conv3d_col2vol_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(total, 256), 256 * 16)), dim3(256), 0, as_stream(stream), cols,
                       Cin, T, H, W, dx);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
