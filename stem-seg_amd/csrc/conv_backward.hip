// Backward of the tap convolutions (padding 1; stride 1, the grouped form also stride 2): the weight and bias gradients, and the tap gather of the data gradient, for
//     27 taps   the decoders' 3x3x3 convolution over a volume [C][T][H][W]                    (x zero-haloed in t, y and x)
//      9 taps   the encoder's 3x3 convolutions over F independent frames [C][F][H][W]          (x zero-haloed in y and x; no tap across frames)
//      1 tap    its 1x1 convolutions over F frames                                             (x any view, dense or strided)
//
//     dW[co][ci][kt][ky][kx] = sum over (t, y, x) of dy[co][t, y, x] * x[ci][t + kt, y + ky, x + kx]      (x in haloed coordinates)
//     db[co] = sum dy[co]
//
// GEMMs with M = Cout, N = taps Cin, K = T H W on v_mfma_f32_32x32x2_f32 (exact products, fp32 accumulation: the library's "f32" arithmetic;
// gradients have no bounded magnitude, so the scaled fp16 split of the forward is not an option).  The rules of decoder_backward.hip hold, for
// every kernel of this file: K is cut into chunks whose length is a function of the shape only, a workgroup accumulates its chunk in fp32 and
// writes fp64 partials into the caller's workspace -- every slot by every call -- and a second launch adds the chunks in chunk order and rounds
// once.  No floating-point atomics, no allocation, no synchronisation; two runs give the same bits.  (One exception to "in chunk order", named here
// because stem_backward.hip takes this contract: its combine walks up to a thousand chunks and more, so it adds them in sixteen runs of consecutive
// chunks, each run in chunk order, and then the runs in run order -- still one fixed order that is a function of the chunk count alone, in fp64.)
//
// The 2-D 9-tap form is the 3-D kernel without its temporal taps (KT = 1 instead of 3): one kernel template, one plan, one combine.  The data
// gradient needs no GEMM of its own (hip.py _tap_dgrad: the per-tap products are one 1x1x1 convolution on the forward kernel); the gather
// below sums them, again one template for 27 and 9 taps, with and without the ReLU mask of the bottleneck backward.
//
// The grouped / strided 3x3 convolution of the ResNeXt bottleneck (grouped_conv.hip; stride 1 or 2) has its weight gradient here too, with that
// kernel's geometry and this file's rules, plan struct and combine (conv2d_grouped_wgrad_kernel below); its data gradient is the forward grouped
// kernel on the per-group transposed, tap-flipped weight (hip.py conv2d_grouped_dgrad).
//
// x is checked with check_view (common.h) in every form: the strides hold the extents as far as they are read -- a channel's last frame and a
// frame's last row may stop at the last element, so the 27-tap entry accepts the same stride combinations as the 2-D one -- and every read
// lies below the view's limit.
#include "common.h"
#include <algorithm>

namespace stemseg {

typedef float wg_f32x16 __attribute__((ext_vector_type(16)));

// ---- 9 in-plane taps (x KT planes).  A K step of a workgroup is a TILE of 64 output voxels of one plane t: RY rows x XS columns, XS = 8 .. 64 by
// the map's width (RY = 64 / XS).  The workgroup owns 128 output channels (wave w the 32 from 32 w), 32 input channels and one kt; per tile it
// stages dy [128][64] and the x halo tile [32][RY + 2][XS + 2] of plane t + kt in LDS, which serves all nine in-plane taps: 9 x 16 accumulator
// VGPRs per wave.  x is zero-haloed, so no tap needs a bounds test; what a tile holds beyond the map (rows >= H, columns >= W) is staged as
// zeros, and the k-steps that lie there entirely are left out (they add exact zeros).  Both LDS channel strides are odd: the 32 lanes of a half
// wave read 32 channels at one voxel, bank = channel stride x channel mod 32.
constexpr int WG_TILE = 64;
constexpr int WG_CO = 128, WG_CI = 32;
constexpr int WG_DY_STRIDE = WG_TILE + 1;
constexpr int WG_X_FLOATS = WG_CI * 199;                      // XS = 64: 3 rows x 66 columns = 198 -> 199; every other tile shape is smaller
constexpr int WG_MIN_TILES_PER_CHUNK = 8;                     // a chunk's partials are 9 x 128 x 32 doubles per workgroup: at least 512 voxels behind them
// ---- 1 tap.  A K step of a workgroup is a tile of 32 consecutive voxels; the workgroup owns 128 x 128 (co, ci), wave (wr, wc) the 64 x 64 at (64 wr, 64 wc)
// as 2 x 2 MFMA blocks: per k-step two A and two B values from LDS feed four MFMAs.  Row stride 33 (odd) for both operands.  With one tap the 64
// accumulators leave room for their fp64 twins: every W1_FLUSH_STEPS k-steps (16 voxels) the fp32 sums move into fp64 registers, so no fp32 chain is longer
// than that -- a chunk-long chain (512 voxels and more) sat at 0.85 ... 1.13 of the tests' bound, torch's blocked GEMM being the yardstick, and a 64-voxel one
// still made up half of the error of the widest lateral's gradient.  The flush points are voxel counts from the tile's start: a function of the shape only.
constexpr int W1_TILE = 32;
constexpr int W1_CO = 128, W1_CI = 128;
constexpr int W1_STRIDE = W1_TILE + 1;
constexpr int W1_MIN_TILES_PER_CHUNK = 16;                    // 512 voxels, as above
constexpr int W1_FLUSH_STEPS = 8;
constexpr int WG_TARGET_WORKGROUPS = 1024;
constexpr int WG_MAX_CHUNKS = 64;
constexpr size_t WG_MAX_PARTIAL_BYTES = size_t(256) << 20;    // chunks are fewer where Cout x Cin is large
constexpr int GATHER_MAX_BLOCKS = 256 * 16;

struct WgradPlan {
    int xs_log2, tiles_x, tiles_y, ntiles, tiles_per_chunk, nchunks, x_cs;
    int min_tiles;
    int64_t base;                                             // workgroups per chunk
    int64_t n_dw;                                             // taps Cout Cin
    size_t bytes;
};

struct WgradParams {
    const float* x;
    int64_t x_cs, x_ts, x_ys;
    const float* dy;
    double* part;                                             // [chunk][taps][Cout][Cin]
    double* part_b;                                           // [chunk][Cout]
    int Cin, Cout, T, H, W;                                   // T: the planes of dy (frames in 2-D)
    int xs_log2, tiles_x, tiles_y, ntiles, tiles_per_chunk, lds_cs;
    int x_dense;                                              // 1 tap: x[ci] is T H W consecutive floats
    int64_t n_dw, V;
};

// KT = 3: the 3x3x3 convolution, blockIdx.y = (input channel tile, kt); KT = 1: the 3x3 convolution over frames, plane t of x is frame t
template <int KT>
__global__ __launch_bounds__(256, 2) void conv_wgrad9_kernel(WgradParams p) {
    __shared__ float xs[WG_X_FLOATS];
    __shared__ float dys[WG_CO * WG_DY_STRIDE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int chunk = blockIdx.x;
    const int kt = blockIdx.y % KT, ci0 = (blockIdx.y / KT) * WG_CI, co0 = blockIdx.z * WG_CO;
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

__global__ __launch_bounds__(256, 2) void conv2d_wgrad1_kernel(WgradParams p) {
    __shared__ float as[W1_CO * W1_STRIDE];                  // dy [128 co][32 voxels]
    __shared__ float bs[W1_CI * W1_STRIDE];                  // x  [128 ci][32 voxels]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int chunk = blockIdx.x;
    const int ci0 = blockIdx.y * W1_CI, co0 = blockIdx.z * W1_CO;
    const int wco = (wave >> 1) * 64, wci = (wave & 1) * 64;   // the wave's 64 x 64 inside the workgroup's 128 x 128
    // (Cout % 32 == 0, and a 32-block of input channels is staged as zeros beyond Cin: a block is at work when its first channel exists)
    const bool a_on[2] = {co0 + wco < p.Cout, co0 + wco + 32 < p.Cout};
    const bool b_on[2] = {ci0 + wci < p.Cin, ci0 + wci + 32 < p.Cin};
    const bool do_b = blockIdx.y == 0;
    const int64_t HW = (int64_t)p.H * p.W;

    wg_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    double acc64[2][2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc64[i][j][r] = 0.0;
    double accb = 0.0;

    const int tile_beg = chunk * p.tiles_per_chunk, tile_end = min(tile_beg + p.tiles_per_chunk, p.ntiles);
    for (int tile = tile_beg; tile < tile_end; ++tile) {
        const int64_t v0 = (int64_t)tile * W1_TILE;
        __syncthreads();                                     // the previous tile's reads are done
        // both operands [128][32]: consecutive threads along the voxels
        for (int i = tid; i < W1_CO * W1_TILE; i += 256) {
            const int j = i & (W1_TILE - 1), row = i >> 5;
            const int64_t v = v0 + j;
            const int co = co0 + row, ci = ci0 + row;
            float a = 0.f, b = 0.f;
            if (v < p.V) {
                if (co < p.Cout) a = p.dy[(int64_t)co * p.V + v];
                if (ci < p.Cin) {
                    if (p.x_dense) {
                        b = p.x[(int64_t)ci * p.x_cs + v];
                    } else {
                        const int f = (int)(v / HW);
                        const int64_t r = v - (int64_t)f * HW;
                        const int y = (int)(r / p.W), xx = (int)(r - (int64_t)y * p.W);
                        b = p.x[(int64_t)ci * p.x_cs + (int64_t)f * p.x_ts + (int64_t)y * p.x_ys + xx];
                    }
                }
            }
            as[row * W1_STRIDE + j] = a;
            bs[row * W1_STRIDE + j] = b;
        }
        __syncthreads();
        if (do_b) {                                          // bias: thread pair per output channel, 16 voxels each
            const float* row = as + (tid >> 1) * W1_STRIDE + (tid & 1) * 16;
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) s += row[i];
            accb += (double)s;
        }
        if (a_on[0] && b_on[0]) {
            const int n_in = (int)min((int64_t)W1_TILE, p.V - v0);
            const float* a_row = as + (wco + (lane & 31)) * W1_STRIDE + (lane >> 5);
            const float* b_row = bs + (wci + (lane & 31)) * W1_STRIDE + (lane >> 5);
            auto flush = [&]() {                             // the fp32 sums of the last k-steps -> fp64
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            acc64[i][j][r] += (double)acc[i][j][r];
                            acc[i][j][r] = 0.f;
                        }
            };
#pragma unroll
            for (int s = 0; s < W1_TILE / 2; ++s) {          // k-step: voxels 2 s and 2 s + 1 of the tile
                const int j = 2 * s;
                if (j >= n_in) break;                        // (wave-uniform) beyond the last voxel: zeros
                const float a0 = a_row[j], a1 = a_row[32 * W1_STRIDE + j];
                const float b0 = b_row[j], b1 = b_row[32 * W1_STRIDE + j];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                if (b_on[1]) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                if (a_on[1]) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                if (a_on[1] && b_on[1]) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
                if (s % W1_FLUSH_STEPS == W1_FLUSH_STEPS - 1) flush();
            }
            if ((n_in + 1) / 2 % W1_FLUSH_STEPS) flush();    // a last tile that ends between two flush points
        }
    }
    // the chunk's partials (C/D map as above): every (co, ci) of the problem lies in exactly one block of one wave of one workgroup
    double* pc = p.part + (int64_t)chunk * p.n_dw;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ci = ci0 + wci + 32 * j + (lane & 31);
            const int cob = co0 + wco + 32 * i;
            if (cob < p.Cout && ci < p.Cin) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = cob + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    pc[(int64_t)co * p.Cin + ci] = acc64[i][j][r];
                }
            }
        }
    if (do_b) {
        accb += __shfl_xor(accb, 1, 64);
        const int co = co0 + (tid >> 1);
        if ((tid & 1) == 0 && co < p.Cout) p.part_b[(int64_t)chunk * p.Cout + co] = accb;
    }
}

// ---- The grouped / strided 3x3 weight gradient (stride S = 1 or 2, padding 1): conv2 of a ResNeXt bottleneck and the stride-in-3x3 conv2.
//     dW[co][cj][ky][kx] = sum over (f, y, x) of dy[co][f, y, x] * x[g(co) Cg + cj][f, S y + ky, S x + kx]        (x in haloed coordinates)
// The geometry of the forward kernel (grouped_conv.hip): a workgroup owns one 16-output-channel block, one 16-channel slice of the block's window of
// Kc = max(16, Cg) input channels, and one K chunk.  A K step is a TILE of 4 output rows x 32 output columns of one frame: dy [16][4 x 32] and the x
// halo tile [16][S 3 + 3][S 31 + 3] are staged in LDS and the one halo tile serves all nine taps (at stride 2 the tap reads step two columns).  Wave w
// takes row w of the tile: 8 k-steps of 4 pixels on v_mfma_f32_16x16x4_f32 (A = dy [16 co][4 px], B = x [4 px][16 ci]), 9 taps x 4 accumulator VGPRs,
// each with an fp64 twin the fp32 sums move into every GW_FLUSH_STEPS k-steps (16 pixels: no fp32 chain is longer, as in the 1-tap kernel above).  The
// four waves' fp64 sums are added in wave order through LDS, and the chunk's partial goes to the workspace as [chunk][tap][co][cj].  For 4 and 8
// channels per group the 16 x 16 block holds 4 or 2 groups: only the diagonal sub-blocks are written out, the other products are discarded (a
// value of another group's input, NaN and inf included, only ever reaches columns that are never stored).
constexpr int GW_TR = 4, GW_TC = 32, GW_CB = 16;
constexpr int GW_DY_STRIDE = GW_TR * GW_TC + 4;               // 132 = 4 mod 32: the 16 channels x 4 pixels of an A read fall on distinct banks mod 64
constexpr int GW_FLUSH_STEPS = 4;
constexpr int GW_MIN_TILES_PER_CHUNK = 4;                     // 512 voxels, as above
typedef float gw_f32x4 __attribute__((ext_vector_type(4)));

template <int S>
struct GwGeom {
    static constexpr int PR = S * (GW_TR - 1) + 3;            // staged input rows
    static constexpr int PC = S * (GW_TC - 1) + 3;            // staged input columns
    static constexpr int PCP = S == 1 ? 38 : 72;              // row pitch: PLANE = 4 S mod 32
    static constexpr int PLANE = PR * PCP;
    static constexpr int X_FLOATS = GW_CB * PLANE;
    static constexpr int RED_FLOATS = 2 * 9 * GW_CB * GW_CB;  // the cross-wave sum: 9 x 16 x 16 doubles, over the x tile
    static constexpr int LDS_FLOATS = X_FLOATS > RED_FLOATS ? X_FLOATS : RED_FLOATS;
};

struct GwParams {
    const float* x;
    int64_t x_cs, x_ts, x_ys;
    const float* dy;
    double* part;                                             // [chunk][9][C][Cg]
    int C, Cg, Kc, nck, F, Hh, Wh, Ho, Wo;                    // Hh, Wh: the haloed extents of x
    int tiles_x, tiles_y, ntiles, tiles_per_chunk;
    int64_t n_dw;
};

template <int S>
__global__ __launch_bounds__(256) void conv2d_grouped_wgrad_kernel(GwParams p) {
    using G = GwGeom<S>;
    __shared__ __attribute__((aligned(16))) float xs[G::LDS_FLOATS];
    __shared__ float dys[GW_CB * GW_DY_STRIDE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c16 = lane & 15;
    const int chunk = blockIdx.x, cc = blockIdx.y, co0 = blockIdx.z * GW_CB;
    const int ci0 = (co0 / p.Kc) * p.Kc + cc * GW_CB;         // first input channel of the slice
    const int64_t HWo = (int64_t)p.Ho * p.Wo;

    gw_f32x4 acc[9];
    double acc64[9][4];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        acc[j] = gw_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) acc64[j][r] = 0.0;
    }
    auto flush = [&]() {
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc64[j][r] += (double)acc[j][r];
                acc[j][r] = 0.f;
            }
    };

    const int tile_beg = chunk * p.tiles_per_chunk, tile_end = min(tile_beg + p.tiles_per_chunk, p.ntiles);
    for (int tile = tile_beg; tile < tile_end; ++tile) {
        const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, f = tile / (p.tiles_x * p.tiles_y);
        const int x0 = tx * GW_TC, y0 = ty * GW_TR;
        __syncthreads();                                     // the previous tile's reads are done
        for (int i = tid; i < GW_CB * GW_TR * GW_TC; i += 256) {
            const int col = i & (GW_TC - 1), row = (i >> 5) & (GW_TR - 1), c = i >> 7;
            const int y = y0 + row, x = x0 + col;
            float v = 0.f;
            if (y < p.Ho && x < p.Wo) v = p.dy[((int64_t)(co0 + c) * p.F + f) * HWo + (int64_t)y * p.Wo + x];
            dys[c * GW_DY_STRIDE + row * GW_TC + col] = v;
        }
        const float* xf = p.x + (int64_t)f * p.x_ts;
        for (int i = tid; i < GW_CB * G::PR * G::PC; i += 256) {
            const int col = i % G::PC, r = i / G::PC, row = r % G::PR, c = r / G::PR;
            const int Y = S * y0 + row, X = S * x0 + col;
            float v = 0.f;
            if (Y < p.Hh && X < p.Wh) v = xf[(int64_t)(ci0 + c) * p.x_cs + (int64_t)Y * p.x_ys + X];
            xs[c * G::PLANE + row * G::PCP + col] = v;
        }
        __syncthreads();
        if (y0 + wave < p.Ho) {                              // (wave-uniform) a row beyond the map: dy is 0 there
            const int cols_in = min(GW_TC, p.Wo - x0);
            const float* a_row = dys + c16 * GW_DY_STRIDE + wave * GW_TC + q;
            const float* b_ch = xs + c16 * G::PLANE + (S * wave) * G::PCP + S * q;
#pragma unroll
            for (int s = 0; s < GW_TC / 4; ++s) {            // k-step: output columns 4 s .. 4 s + 3 of the wave's row
                if (4 * s < cols_in) {                       // (wave-uniform)
                    const float a = a_row[4 * s];
                    const float* b = b_ch + S * 4 * s;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx)
                            acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[ky * G::PCP + kx], acc[ky * 3 + kx], 0, 0, 0);
                }
                if (s % GW_FLUSH_STEPS == GW_FLUSH_STEPS - 1) flush();
            }
        }
    }
    // the four waves' sums in wave order.  C/D map of the 16x16 MFMA: column = lane & 15 (the input channel), row = 4 (lane >> 4) + r
    double* red = reinterpret_cast<double*>(xs);
    for (int w = 0; w < 4; ++w) {
        __syncthreads();                                     // w = 0: the last tile's reads are done
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < 9; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double* slot = red + (j * 4 + r) * 64 + lane;
                    if (w == 0) *slot = acc64[j][r];
                    else if (w < 3) *slot += acc64[j][r];
                    else acc64[j][r] += *slot;
                }
        }
    }
    if (wave == 3) {
        double* pc = p.part + (int64_t)chunk * p.n_dw;
        const int co_l = 4 * q;
        const bool dense = p.Cg >= GW_CB;                    // the slice lies inside the block's own group
        const int cj = dense ? cc * GW_CB + c16 : c16 % p.Cg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!dense && (co_l + r) / p.Cg != c16 / p.Cg) continue;             // another group's product: discarded
#pragma unroll
            for (int j = 0; j < 9; ++j) pc[((int64_t)j * p.C + co0 + co_l + r) * p.Cg + cj] = acc64[j][r];
        }
    }
}

// one thread per slot (tap, co, ci), ci fastest as the partials lie: the chunks in chunk order, rounded once -> dw in torch's layout
// [Cout][Cin][taps]; the threads behind them the bias slots
__global__ __launch_bounds__(256) void conv_wgrad_combine_kernel(const double* __restrict__ part, const double* __restrict__ part_b, int nchunks,
                                                                 int Cout, int Cin, int taps, int64_t n_dw, float* __restrict__ dw,
                                                                 float* __restrict__ db) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_dw) {
        double s = 0.0;
        for (int k = 0; k < nchunks; ++k) s += part[(int64_t)k * n_dw + i];
        const int ci = (int)(i % Cin);
        const int64_t r = i / Cin;
        const int co = (int)(r % Cout), tap = (int)(r / Cout);
        dw[((int64_t)co * Cin + ci) * taps + tap] = (float)s;
    } else if (i < n_dw + Cout && db) {
        const int co = (int)(i - n_dw);
        double s = 0.0;
        for (int k = 0; k < nchunks; ++k) s += part_b[(int64_t)k * Cout + co];
        db[co] = (float)s;
    }
}

// ---- The data gradient's second half.  dX[ci][u] = sum over taps k of O_k[ci][u - k + 1], O_k = W_k^T dy the per-tap products (one 1x1x1
// convolution with 9 KT Cin output channels: Cout terms each; cols = [9 KT][Cin][T][H][W]): the (at most) 9 KT in-range taps of voxel
// (ci, t, y, x) in tap order, in fp64, then the addend's value at the voxel's dense index i (if any).  Summing the taps here instead of in the
// convolution's fp32 accumulator keeps the Cout-term sums apart.  KT = 1: no tap leaves the frame.
template <int KT>
__device__ __forceinline__ double gather_taps(const float* __restrict__ cols, int Cin, int64_t per_c, int64_t HW, int T, int H, int W, int ci, int t, int y,
                                              int x, const float* __restrict__ addend, int64_t i) {
    double acc = 0.0;
    for (int kt = 0; kt < KT; ++kt) {
        const int vt = KT == 1 ? t : t - kt + 1;
        if (KT != 1 && (vt < 0 || vt >= T)) continue;
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
    if (addend) acc += (double)addend[i];
    return acc;
}

// one rounding of the fp64 sum; MASK: m is a view [Cin][T][H][W] of the convolution's input after its ReLU, and relu_backward's rule decides between
// that value and 0.  VEC: 4 voxels of a row per thread, one 16-byte store
template <int KT, bool VEC, bool MASK>
__global__ __launch_bounds__(256) void conv_tap_gather_kernel(const float* __restrict__ cols, int Cin, int T, int H, int W, const float* __restrict__ addend,
                                                              BBView m, float* __restrict__ dx, int64_t items) {
    const int per = VEC ? 4 : 1, WQ = W / per;
    const int64_t HW = (int64_t)H * W, per_c = (int64_t)T * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int x0 = (int)(i % WQ) * per;
        int64_t r = i / WQ;
        const int y = (int)(r % H);
        r /= H;
        const int t = (int)(r % T);
        const int ci = (int)(r / T);
        const float* mp = MASK ? m.ptr + (int64_t)ci * m.cs + (int64_t)t * m.ts + (int64_t)y * m.ys + x0 : nullptr;
        const int64_t o = i * per;
        auto voxel = [&](int e) {
            const float mv = MASK ? mp[e] : 0.f;             // (read ahead of the taps, not behind their branches)
            const float v = (float)gather_taps<KT>(cols, Cin, per_c, HW, T, H, W, ci, t, y, x0 + e, addend, o + e);
            return MASK ? relu_mask(mv, v) : v;
        };
        if (VEC) {
            float4 v;
            v.x = voxel(0); v.y = voxel(1); v.z = voxel(2); v.w = voxel(3);
            *reinterpret_cast<float4*>(dx + o) = v;
        } else {
            dx[o] = voxel(0);
        }
    }
}

// The plain gathers run one voxel per thread: 4 per thread took 1.7 x the time on the 120 x 216 map; the masked one keeps the
// 4-per-thread form where a row is a multiple of 4 and dx keeps 16-byte alignment
template <int KT>
static void launch_tap_gather(const float* cols, int Cin, int T, int H, int W, const float* addend, const StemsegVolume* mask, float* dx, hipStream_t s) {
    const int64_t total = (int64_t)Cin * T * H * W;
    const bool vec = mask && W % 4 == 0 && reinterpret_cast<uintptr_t>(dx) % 16 == 0;
    const int64_t items = vec ? total / 4 : total;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, 256), GATHER_MAX_BLOCKS))), block(256);
    if constexpr (KT == 1) {
        if (mask) {
            const BBView m{mask->ptr, mask->c_stride, mask->t_stride, mask->y_stride};
            if (vec) hipLaunchKernelGGL((conv_tap_gather_kernel<1, true, true>), grid, block, 0, s, cols, Cin, T, H, W, addend, m, dx, items);
            else hipLaunchKernelGGL((conv_tap_gather_kernel<1, false, true>), grid, block, 0, s, cols, Cin, T, H, W, addend, m, dx, items);
            return;
        }
    }
    hipLaunchKernelGGL((conv_tap_gather_kernel<KT, false, false>), grid, block, 0, s, cols, Cin, T, H, W, addend, BBView{nullptr, 0, 0, 0}, dx, items);
}

// Tile shape and chunk length: functions of (Cin, Cout, taps, T, H, W) only; taps = 9 kt_planes (kt_planes 3: the volume, 1: frames) or 1.  As
// many chunks as bring the launch to about WG_TARGET_WORKGROUPS workgroups, at most WG_MAX_CHUNKS and at most what WG_MAX_PARTIAL_BYTES of
// partials hold, and no chunk shorter than the form's minimum of tiles (the last one aside).
static int wgrad_plan(int Cin, int Cout, int taps, int kt_planes, int T, int H, int W, WgradPlan& pl) {
    const char* who = kt_planes == 3 ? "conv3d_wgrad" : "conv2d_wgrad";
    SS_CHECK_ARG(taps == 9 * kt_planes || (taps == 1 && kt_planes == 1), "%s: taps must be 1 or 9, got %d", who, taps);
    SS_CHECK_ARG(Cin > 0 && Cin % 4 == 0 && Cout > 0 && Cout % 32 == 0, "%s: Cin %% 4 == 0 and Cout %% 32 == 0 required (Cin=%d, Cout=%d)", who, Cin, Cout);
    SS_CHECK_ARG(Cin <= 4096 && Cout <= 4096, "%s: at most 4096 channels (Cin=%d, Cout=%d)", who, Cin, Cout);
    SS_CHECK_ARG(T > 0 && H > 0 && W > 0 && (int64_t)T * H * W < (1ll << 30), "%s: bad dims (%c=%d, H=%d, W=%d)", who, kt_planes == 3 ? 'T' : 'F', T, H, W);
    if (taps != 1) {
        pl.xs_log2 = W <= 8 ? 3 : W <= 16 ? 4 : W <= 32 ? 5 : 6;
        const int XS = 1 << pl.xs_log2, RY = WG_TILE / XS;
        pl.tiles_x = (int)ceil_div(W, XS);
        pl.tiles_y = (int)ceil_div(H, RY);
        pl.ntiles = T * pl.tiles_x * pl.tiles_y;
        pl.x_cs = ((RY + 2) * (XS + 2)) | 1;
        pl.base = ceil_div(Cout, WG_CO) * ceil_div(Cin, WG_CI) * kt_planes;
        pl.min_tiles = WG_MIN_TILES_PER_CHUNK;
    } else {
        pl.xs_log2 = 0; pl.tiles_x = pl.tiles_y = 1; pl.x_cs = 0;
        pl.ntiles = (int)ceil_div((int64_t)T * H * W, W1_TILE);
        pl.base = ceil_div(Cout, W1_CO) * ceil_div(Cin, W1_CI);
        pl.min_tiles = W1_MIN_TILES_PER_CHUNK;
    }
    pl.n_dw = (int64_t)taps * Cout * Cin;
    const int64_t slot_bytes = (pl.n_dw + Cout) * (int64_t)sizeof(double);
    int64_t want = std::min<int64_t>(ceil_div(WG_TARGET_WORKGROUPS, pl.base), WG_MAX_CHUNKS);
    want = std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)WG_MAX_PARTIAL_BYTES / slot_bytes));
    pl.tiles_per_chunk = (int)std::max<int64_t>(pl.min_tiles, ceil_div(pl.ntiles, want));
    pl.nchunks = (int)ceil_div(pl.ntiles, pl.tiles_per_chunk);
    pl.bytes = (size_t)pl.nchunks * (size_t)slot_bytes;
    return STEMSEG_OK;
}

// x: the input view, haloed by 2 in y and x for 9 in-plane taps and in t too for kt_planes = 3 (the entry points have checked that the extents
// exceed the halo)
static int wgrad_run(const StemsegVolume& x, const float* dy, int Cout, int taps, int kt_planes, float* dw, float* db, void* workspace, size_t ws_bytes,
                     void* stream) {
    const char* who = kt_planes == 3 ? "conv3d_wgrad" : "conv2d_wgrad";
    const int halo = taps == 1 ? 0 : 2;
    const int Cin = x.C, T = x.T - (kt_planes - 1), H = x.H - halo, W = x.W - halo;
    WgradPlan pl;
    int rc = wgrad_plan(Cin, Cout, taps, kt_planes, T, H, W, pl);
    if (rc) return rc;
    rc = check_view(who, "x", x);
    if (rc) return rc;
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "%s: workspace must be 256-byte aligned", who);
    if (ws_bytes < pl.bytes) {
        set_error("%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, pl.bytes);
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
    p.V = (int64_t)T * H * W;
    p.x_dense = taps == 1 && x.y_stride == W && x.t_stride == (int64_t)H * W;
    hipStream_t s = as_stream(stream);
    void* ev = profile_begin(kt_planes == 3 ? 53 : taps == 9 ? 54 : 55, 2.0 * taps * (double)Cout * Cin * T * H * W, s);
    if (taps == 1) {
        const dim3 grid((unsigned)pl.nchunks, (unsigned)ceil_div(Cin, W1_CI), (unsigned)ceil_div(Cout, W1_CO));
        hipLaunchKernelGGL(conv2d_wgrad1_kernel, grid, dim3(256), 0, s, p);
    } else {
        const dim3 grid((unsigned)pl.nchunks, (unsigned)(ceil_div(Cin, WG_CI) * kt_planes), (unsigned)ceil_div(Cout, WG_CO));
        if (kt_planes == 3) hipLaunchKernelGGL(conv_wgrad9_kernel<3>, grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL(conv_wgrad9_kernel<1>, grid, dim3(256), 0, s, p);
    }
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(conv_wgrad_combine_kernel, dim3((unsigned)ceil_div(pl.n_dw + Cout, 256)), dim3(256), 0, s, (const double*)p.part,
                       (const double*)p.part_b, pl.nchunks, Cout, Cin, taps, pl.n_dw, dw, db);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

// The grouped weight gradient's plan: a function of (C, groups, stride, F, H, W) only; H, W the INPUT map's extents
static int grouped_wgrad_plan(int C, int groups, int stride, int F, int H, int W, GwParams& p, WgradPlan& pl) {
    const char* who = "conv2d_grouped_wgrad";
    SS_CHECK_ARG(C >= 16 && C % 16 == 0 && C <= 4096, "%s: C = %d is no multiple of 16 (at most 4096)", who, C);
    SS_CHECK_ARG(groups >= 1 && C % groups == 0, "%s: %d channels in %d groups", who, C, groups);
    const int Cg = C / groups;
    SS_CHECK_ARG(groups == 1 || Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32 || Cg == 64,
                 "%s: %d channels per group unsupported (4, 8, 16, 32, 64; one group: a multiple of 16)", who, Cg);
    SS_CHECK_ARG(stride == 1 || stride == 2, "%s: stride %d (1 or 2)", who, stride);
    SS_CHECK_ARG(F > 0 && H > 0 && W > 0 && (int64_t)F * H * W < (1ll << 30), "%s: bad dims (F=%d, H=%d, W=%d)", who, F, H, W);
    p.C = C; p.Cg = Cg; p.Kc = std::max(GW_CB, Cg); p.nck = p.Kc / GW_CB; p.F = F; p.Hh = H + 2; p.Wh = W + 2;
    p.Ho = (H - 1) / stride + 1; p.Wo = (W - 1) / stride + 1;
    p.tiles_x = (int)ceil_div(p.Wo, GW_TC); p.tiles_y = (int)ceil_div(p.Ho, GW_TR);
    p.ntiles = F * p.tiles_x * p.tiles_y;
    pl.base = (int64_t)(C / GW_CB) * p.nck;
    pl.n_dw = (int64_t)9 * C * Cg;
    const int64_t slot_bytes = pl.n_dw * (int64_t)sizeof(double);
    int64_t want = std::min<int64_t>(ceil_div(WG_TARGET_WORKGROUPS, pl.base), WG_MAX_CHUNKS);
    want = std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)WG_MAX_PARTIAL_BYTES / slot_bytes));
    pl.tiles_per_chunk = (int)std::max<int64_t>(GW_MIN_TILES_PER_CHUNK, ceil_div(p.ntiles, want));
    pl.nchunks = (int)ceil_div(p.ntiles, pl.tiles_per_chunk);
    pl.bytes = (size_t)pl.nchunks * (size_t)slot_bytes;
    p.tiles_per_chunk = pl.tiles_per_chunk; p.n_dw = pl.n_dw;
    return STEMSEG_OK;
}

}  // namespace stemseg

using namespace stemseg;

extern "C" size_t stemseg_hip_conv3d_wgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t T, int32_t H, int32_t W) {
    WgradPlan pl;
    return wgrad_plan(Cin, Cout, 27, 3, T, H, W, pl) == STEMSEG_OK ? pl.bytes : 0;
}

extern "C" int stemseg_hip_conv3d_wgrad_chunks(int32_t Cin, int32_t Cout, int32_t T, int32_t H, int32_t W) {
    WgradPlan pl;
    const int rc = wgrad_plan(Cin, Cout, 27, 3, T, H, W, pl);
    return rc == STEMSEG_OK ? pl.nchunks : rc;
}

extern "C" int stemseg_hip_conv3d_wgrad(const StemsegVolume* x_haloed, const float* dy, int32_t Cout, float* dw, float* db, void* workspace,
                                        size_t ws_bytes, void* stream) {
    SS_CHECK_ARG(x_haloed && x_haloed->ptr && dy && dw && workspace, "conv3d_wgrad: null pointer");
    const StemsegVolume& x = *x_haloed;
    SS_CHECK_ARG(x.T >= 3 && x.H >= 3 && x.W >= 3, "conv3d_wgrad: x must be the haloed view (T + 2, H + 2, W + 2), got (%d, %d, %d)", x.T, x.H, x.W);
    return wgrad_run(x, dy, Cout, 27, 3, dw, db, workspace, ws_bytes, stream);
}

extern "C" size_t stemseg_hip_conv2d_wgrad_workspace_bytes(int32_t Cin, int32_t Cout, int32_t taps, int32_t F, int32_t H, int32_t W) {
    WgradPlan pl;
    return wgrad_plan(Cin, Cout, taps, 1, F, H, W, pl) == STEMSEG_OK ? pl.bytes : 0;
}

extern "C" int stemseg_hip_conv2d_wgrad_chunks(int32_t Cin, int32_t Cout, int32_t taps, int32_t F, int32_t H, int32_t W) {
    WgradPlan pl;
    const int rc = wgrad_plan(Cin, Cout, taps, 1, F, H, W, pl);
    return rc == STEMSEG_OK ? pl.nchunks : rc;
}

extern "C" int stemseg_hip_conv2d_wgrad(const StemsegVolume* x_view, const float* dy, int32_t Cout, int32_t taps, float* dw, float* db, void* workspace,
                                        size_t ws_bytes, void* stream) {
    SS_CHECK_ARG(x_view && x_view->ptr && dy && dw && workspace, "conv2d_wgrad: null pointer");
    SS_CHECK_ARG(taps == 1 || taps == 9, "conv2d_wgrad: taps must be 1 or 9, got %d", taps);
    const StemsegVolume& x = *x_view;
    const int halo = taps == 9 ? 2 : 0;
    SS_CHECK_ARG(x.T >= 1 && x.H > halo && x.W > halo, "conv2d_wgrad: x must be the y/x-haloed view (F, H + 2, W + 2) for 9 taps, got (%d, %d, %d)", x.T, x.H,
                 x.W);
    return wgrad_run(x, dy, Cout, taps, 1, dw, db, workspace, ws_bytes, stream);
}

extern "C" size_t stemseg_hip_conv2d_grouped_wgrad_workspace_bytes(int32_t C, int32_t groups, int32_t stride, int32_t F, int32_t H, int32_t W) {
    GwParams p;
    WgradPlan pl;
    return grouped_wgrad_plan(C, groups, stride, F, H, W, p, pl) == STEMSEG_OK ? pl.bytes : 0;
}

extern "C" int stemseg_hip_conv2d_grouped_wgrad_chunks(int32_t C, int32_t groups, int32_t stride, int32_t F, int32_t H, int32_t W) {
    GwParams p;
    WgradPlan pl;
    const int rc = grouped_wgrad_plan(C, groups, stride, F, H, W, p, pl);
    return rc == STEMSEG_OK ? pl.nchunks : rc;
}

extern "C" int stemseg_hip_conv2d_grouped_wgrad(const StemsegVolume* x_haloed, const float* dy, int32_t C, int32_t groups, int32_t stride, float* dw,
                                                void* workspace, size_t ws_bytes, void* stream) {
    SS_CHECK_ARG(x_haloed && x_haloed->ptr, "conv2d_grouped_wgrad: x_haloed is a null pointer");
    SS_CHECK_ARG(dy, "conv2d_grouped_wgrad: dy is a null pointer");
    SS_CHECK_ARG(dw, "conv2d_grouped_wgrad: dw is a null pointer");
    SS_CHECK_ARG(workspace, "conv2d_grouped_wgrad: workspace is a null pointer");
    const StemsegVolume& x = *x_haloed;
    SS_CHECK_ARG(x.T >= 1 && x.H >= 3 && x.W >= 3, "conv2d_grouped_wgrad: x must be the y/x-haloed view (F, H + 2, W + 2), got (%d, %d, %d)", x.T, x.H, x.W);
    SS_CHECK_ARG(x.C == C, "conv2d_grouped_wgrad: x has %d channels, C = %d", x.C, C);
    GwParams p;
    WgradPlan pl;
    int rc = grouped_wgrad_plan(C, groups, stride, x.T, x.H - 2, x.W - 2, p, pl);
    if (rc) return rc;
    rc = check_view("conv2d_grouped_wgrad", "x", x);
    if (rc) return rc;
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "conv2d_grouped_wgrad: workspace must be 256-byte aligned");
    if (ws_bytes < pl.bytes) {
        set_error("conv2d_grouped_wgrad: workspace too small (%zu < %zu bytes)", ws_bytes, pl.bytes);
        return STEMSEG_E_WORKSPACE;
    }
    p.x = x.ptr; p.x_cs = x.c_stride; p.x_ts = x.t_stride; p.x_ys = x.y_stride;
    p.dy = dy;
    p.part = reinterpret_cast<double*>(workspace);
    hipStream_t s = as_stream(stream);
    void* ev = profile_begin(62, 2.0 * 9 * (double)C * p.Cg * p.F * p.Ho * p.Wo, s);
    const dim3 grid((unsigned)pl.nchunks, (unsigned)p.nck, (unsigned)(C / GW_CB));
    if (stride == 1) hipLaunchKernelGGL(conv2d_grouped_wgrad_kernel<1>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(conv2d_grouped_wgrad_kernel<2>, grid, dim3(256), 0, s, p);
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(conv_wgrad_combine_kernel, dim3((unsigned)ceil_div(pl.n_dw, 256)), dim3(256), 0, s, (const double*)p.part, (const double*)nullptr,
                       pl.nchunks, C, p.Cg, 9, pl.n_dw, dw, (float*)nullptr);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_conv3d_col2vol(const float* cols, int32_t Cin, int32_t T, int32_t H, int32_t W, float* dx, void* stream) {
    SS_CHECK_ARG(cols && dx, "conv3d_col2vol: null pointer");
    SS_CHECK_ARG(Cin > 0 && T > 0 && H > 0 && W > 0 && (int64_t)27 * Cin * T * H * W < (1ll << 40), "conv3d_col2vol: bad dims");
    launch_tap_gather<3>(cols, Cin, T, H, W, nullptr, nullptr, dx, as_stream(stream));
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_conv2d_col2img(const float* cols, int32_t Cin, int32_t F, int32_t H, int32_t W, const float* addend, float* dx, void* stream) {
    SS_CHECK_ARG(cols && dx, "conv2d_col2img: null pointer");
    SS_CHECK_ARG(Cin > 0 && F > 0 && H > 0 && W > 0 && (int64_t)9 * Cin * F * H * W < (1ll << 40), "conv2d_col2img: bad dims");
    launch_tap_gather<1>(cols, Cin, F, H, W, addend, nullptr, dx, as_stream(stream));
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_conv2d_col2img_relu(const float* cols, int32_t Cin, int32_t F, int32_t H, int32_t W, const float* addend,
                                               const StemsegVolume* mask, float* dx, void* stream) {
    SS_CHECK_ARG(cols, "conv2d_col2img_relu: cols is a null pointer");
    SS_CHECK_ARG(dx, "conv2d_col2img_relu: dx is a null pointer");
    SS_CHECK_ARG(mask && mask->ptr, "conv2d_col2img_relu: mask is a null pointer");
    SS_CHECK_ARG(Cin > 0 && F > 0 && H > 0 && W > 0 && (int64_t)9 * Cin * F * H * W < (1ll << 40), "conv2d_col2img_relu: bad dims (Cin=%d, F=%d, H=%d, W=%d)", Cin,
                 F, H, W);
    const int rc = check_view("conv2d_col2img_relu", "mask", *mask);
    if (rc) return rc;
    SS_CHECK_ARG(mask->C == Cin && mask->T == F && mask->H == H && mask->W == W, "conv2d_col2img_relu: mask is [%d][%d][%d][%d], expected [%d][%d][%d][%d]",
                 mask->C, mask->T, mask->H, mask->W, Cin, F, H, W);
    hipStream_t s = as_stream(stream);
    void* ev = profile_begin(57, 4.0 * (addend ? 12.0 : 11.0) * (double)Cin * F * H * W, s);
    launch_tap_gather<1>(cols, Cin, F, H, W, addend, mask, dx, s);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
